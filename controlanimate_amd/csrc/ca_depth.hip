// Added to ABI v16: the depth annotator (controlanimate_amd/depth.py: DepthAnnotator; the specification is tests/depth_ref.py, pinned to
// transformers' DPTForDepthEstimation / DPTImageProcessor / depth-estimation pipeline and to Pillow by tests/golden/dpt_tiny.npz).  The ViT
// runs on ca_gemm / ca_layernorm / ca_attention and the decoder on ca_conv3x3 / ca_relu / ca_upsample2x_bilinear_ac; these are the stages
// none of them covers:
//
//   resize    k_pil_pass        Pillow's Image.resize for uint8 RGB: one pass per axis (horizontal first) over host-built bounds and 22-bit
//                               fixed-point coefficient tables, the intermediate rounded and clipped to uint8 as Resample.c does
//   patches   k_dpt_patches     uint8 [n, S, S, 3] -> (x / 255 - 0.5) / 0.5 as the rows [n g g, 3 P P] of the patch-embedding GEMM, columns in the
//                               weight's (c, ky, kx) order
//   d2s       k_depth_to_space  the scatter behind a ConvTranspose2d(k = stride) run as ONE GEMM with N = k k Cout: row (img, y, x), column
//                               (ky, kx, co) -> pixel (y k + ky, x k + kx) of a contiguous NHWC plane.  The rows are read at a stride and an
//                               offset per image, so the class-token row of every image is skipped without a copy; k = 1 is that gather alone
//   head      k_dpt_head        head.head.1 .. 5 in ONE launch: the align-corners bilinear x2 of [n, h, w, Cmid], the 3x3 Cmid -> 32 convolution
//                               + bias + ReLU on the MFMA and the 1x1 32 -> 1 + bias + ReLU, fp32 [n, 2h, 2w] out.  The upsampled plane (the
//                               largest tensor of the network) is never written: a block owns 16 x 16 output pixels and stages the 18 x 18
//                               INTERPOLATED pixels under them in LDS 32 channels at a time, with k_up2_ac's arithmetic and rounding, zero
//                               outside the upsampled plane.  The 32 -> 1 sum runs across the lanes that hold the 32 channels
//                               (measured 2.5x slower than the composed head at DPT-large width: not the default, context.dispatch.dpt_head_fused)
//             k_dpt_logit       the last step of the composed head (ca_upsample2x_bilinear_ac + ca_conv3x3(RELU, fp32 out) + this): 32 -> 1
//   tail      k_bicubic_f32     torch's interpolate(mode = "bicubic", align_corners = False) of fp32 planes, with the per-frame max and min
//                               through order-preserving integer atomics (values can be negative: the float bits are not ordered as they are)
//   finish    k_depth_finish    the uint8 map of either normalisation and / or the control tensor (ca_annot.h), from the device-side max / min
//
// No launch depends on device data on the host side: the chain can be captured in a hipGraph.  Max and min do not depend on the order of
// the atomics: two runs give the same bits.
#include "ca_common.h"
#include "ca_annot.h"

namespace {

constexpr int PIL_PRECISION_BITS = 32 - 8 - 2;

// ---- Pillow's resampler: one axis -----------------------------------------------------------------------------------------------------
// in [outer][in_len][inner] -> out [outer][out_len][inner] (horizontal: outer = rows, inner = 3; vertical: outer = images, inner = 3 * width).
// The bounds are clamped to the source, so that a wrong table cannot read outside it.
__global__ __launch_bounds__(256) void k_pil_pass(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int64_t total, int in_len, int out_len, int inner,
                                                  const int32_t* __restrict__ bounds, const int32_t* __restrict__ kk, int ksize) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int j = (int)(idx % inner);
  const int64_t r = idx / inner;
  const int xx = (int)(r % out_len);
  const int64_t o = r / out_len;
  int xmin = bounds[2 * xx], cnt = bounds[2 * xx + 1];
  xmin = xmin < 0 ? 0 : (xmin > in_len ? in_len : xmin);
  cnt = cnt > ksize ? ksize : cnt;
  cnt = cnt > in_len - xmin ? in_len - xmin : cnt;
  const int32_t* k = kk + (int64_t)xx * ksize;
  const uint8_t* p = in + (o * in_len + xmin) * inner + j;
  int32_t ss = 1 << (PIL_PRECISION_BITS - 1);
  for (int x = 0; x < cnt; ++x) ss += (int32_t)p[(int64_t)x * inner] * k[x];
  ss >>= PIL_PRECISION_BITS;
  out[idx] = (uint8_t)(ss < 0 ? 0 : (ss > 255 ? 255 : ss));
}

// ---- patch rows -----------------------------------------------------------------------------------------------------------------------
// A thread writes 8 consecutive kx of one (patch, c, ky): P % 8 == 0.
template <int DT>
__global__ __launch_bounds__(256) void k_dpt_patches(const uint8_t* __restrict__ src, u16* __restrict__ out, int64_t total, int S, int P) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int g = S / P, pk = P >> 3;
  const int kx8 = (int)(idx % pk);
  int64_t t = idx / pk;
  const int ky = (int)(t % P);
  t /= P;
  const int c = (int)(t % 3);
  const int64_t patch = t / 3;
  const int px = (int)(patch % g), py = (int)((patch / g) % g);
  const int64_t img = patch / ((int64_t)g * g);
  const uint8_t* s = src + ((img * S + py * P + ky) * S + px * P + kx8 * 8) * 3 + c;
  float f[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = __fdiv_rn((float)s[e * 3] * 0.00392156862745098f - 0.5f, 0.5f);
  st16(out + patch * (3 * P * P) + (c * P + ky) * P + kx8 * 8, pack8<DT>(f));
}

// ---- depth to space -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_depth_to_space(const u16* __restrict__ x, u16* __restrict__ y, int64_t total, int gh, int gw, int k, int cout, int64_t ldx,
                                                        int rows_per_image, int row0) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cl = cout >> 3;
  const int cg = (int)(idx % cl);
  const int64_t op = idx / cl;
  const int ow = gw * k, oh = gh * k;
  const int ox = (int)(op % ow), oy = (int)((op / ow) % oh);
  const int64_t img = op / ((int64_t)ow * oh);
  const int sy = oy / k, sx = ox / k, ky = oy - sy * k, kx = ox - sx * k;
  const int64_t row = img * rows_per_image + row0 + sy * gw + sx;
  st16(y + op * cout + cg * 8, ld16(x + row * ldx + (ky * k + kx) * cout + cg * 8));
}

// ---- the head ---------------------------------------------------------------------------------------------------------------------------
// src = dst * (in - 1) / (out - 1), as k_up2_ac of ca_mlsd.hip computes it (the composed head runs that kernel: both round alike)
__device__ __forceinline__ void ac_coord(int d, int in, int out, int& i0, int& i1, float& f) {
  const float s = out > 1 ? __fdiv_rn((float)(d * (in - 1)), (float)(out - 1)) : 0.f;
  i0 = (int)s;
  i0 = i0 > in - 1 ? in - 1 : i0;
  i1 = i0 + 1 < in ? i0 + 1 : in - 1;
  f = s - (float)i0;
}

// A block owns 16 x 16 pixels of the 2h x 2w plane; its four waves are 2 (halves of the rows) x 2 (halves of the 32 channels).  MFMA 16x16x32:
// A = 16 output channels x 32 input channels of one tap, read from memory; B = the 16 pixels of one tile row, from the LDS halo (a pixel
// every 40 elements: the 16 lanes of a fragment row fall on different bank groups).  A lane ends up with 4 consecutive channels of one pixel.
constexpr int HD_T = 16, HD_HALO = HD_T + 2, HD_KC = 32, HD_PITCH = HD_KC + 8, HD_ROWS = HD_T / 2;

template <int DT>
__global__ __launch_bounds__(256) void k_dpt_head(const u16* __restrict__ x, const u16* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ w3,
                                                  const float* __restrict__ b3, float* __restrict__ out, int h, int w, int cmid, int tiles_x, int tiles_y) {
  __shared__ __attribute__((aligned(16))) u16 tile[HD_HALO * HD_HALO * HD_PITCH];
  __shared__ float red[2][HD_T * HD_T];
  int b = blockIdx.x;
  const int bx = b % tiles_x;
  b /= tiles_x;
  const int by = b % tiles_y;
  const int img = b / tiles_y;
  const int oh = 2 * h, ow = 2 * w;
  const int y0 = by * HD_T, x0 = bx * HD_T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, r16 = lane & 15;
  const int wm = wave & 1, wn = wave >> 1;
  const u16* xi = x + (int64_t)img * h * w * cmid;
  const u16* wrow = w2 + (int64_t)(wn * 16 + r16) * 9 * cmid + q * 8;
  f32x4 acc[HD_ROWS];
#pragma unroll
  for (int j = 0; j < HD_ROWS; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  bool rowlive[HD_ROWS];
#pragma unroll
  for (int j = 0; j < HD_ROWS; ++j) rowlive[j] = y0 + wm * HD_ROWS + j < oh;  // wave-uniform

  for (int c0 = 0; c0 < cmid; c0 += HD_KC) {
    if (c0) __syncthreads();
    for (int i = threadIdx.x; i < HD_HALO * HD_HALO * (HD_KC / 8); i += 256) {
      const int pix = i / (HD_KC / 8), part = i - pix * (HD_KC / 8);
      const int r = pix / HD_HALO, c = pix - r * HD_HALO;
      const int gy = y0 - 1 + r, gx = x0 - 1 + c;
      u32x4 v = (u32x4){0u, 0u, 0u, 0u};  // the zero padding belongs to the upsampled plane
      if (gy >= 0 && gy < oh && gx >= 0 && gx < ow) {
        int ya, yb, xa, xb;
        float fy, fx;
        ac_coord(gy, h, oh, ya, yb, fy);
        ac_coord(gx, w, ow, xa, xb, fx);
        const u16* s = xi + c0 + part * 8;
        float a[8], bb[8], cc[8], d[8], o[8];
        unpack8<DT>(ld16(s + ((int64_t)ya * w + xa) * cmid), a);
        unpack8<DT>(ld16(s + ((int64_t)ya * w + xb) * cmid), bb);
        unpack8<DT>(ld16(s + ((int64_t)yb * w + xa) * cmid), cc);
        unpack8<DT>(ld16(s + ((int64_t)yb * w + xb) * cmid), d);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float top = a[e] * (1.0f - fx) + bb[e] * fx;
          const float bot = cc[e] * (1.0f - fx) + d[e] * fx;
          o[e] = top * (1.0f - fy) + bot * fy;
        }
        v = pack8<DT>(o);
      }
      st16(tile + pix * HD_PITCH + part * 8, v);
    }
    __syncthreads();
#pragma unroll 3
    for (int tap = 0; tap < 9; ++tap) {
      const int ty = tap / 3, tx = tap - ty * 3;
      const u32x4 a = ld16(wrow + (int64_t)tap * cmid + c0);
      u32x4 bf[HD_ROWS];
#pragma unroll
      for (int j = 0; j < HD_ROWS; ++j) bf[j] = ld16(tile + ((wm * HD_ROWS + j + ty) * HD_HALO + r16 + tx) * HD_PITCH + q * 8);
#pragma unroll
      for (int j = 0; j < HD_ROWS; ++j) {
        if (!rowlive[j]) continue;
        acc[j] = Elem<DT>::mfma(a, bf[j], acc[j]);
      }
    }
  }
  // 32 -> 1: a lane's four channels, then the four lane groups of the wave, then the two channel halves through LDS -- a fixed order
  float bq[4], wq[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    bq[i] = b2[wn * 16 + q * 4 + i];
    wq[i] = w3[wn * 16 + q * 4 + i];
  }
#pragma unroll
  for (int j = 0; j < HD_ROWS; ++j) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) s += wq[i] * fmaxf(acc[j][i] + bq[i], 0.f);
    s = rowgroup_sum(s);
    if (q == 0) red[wn][(wm * HD_ROWS + j) * HD_T + r16] = s;
  }
  __syncthreads();
  const int py = threadIdx.x >> 4, px = threadIdx.x & 15;
  const int gy = y0 + py, gx = x0 + px;
  if (gy < oh && gx < ow) out[((int64_t)img * oh + gy) * ow + gx] = fmaxf((red[0][threadIdx.x] + red[1][threadIdx.x]) + b3[0], 0.f);
}

// the composed head's last step: t fp32 [pixels][32] (already through the ReLU) -> max(sum_c w3[c] t[c] + b3, 0)
__global__ __launch_bounds__(256) void k_dpt_logit(const float* __restrict__ t, const float* __restrict__ w3, const float* __restrict__ b3, float* __restrict__ out,
                                                   int64_t pixels) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= pixels) return;
  const f32x4* v = (const f32x4*)(t + p * 32);
  float s = 0.f;
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const f32x4 a = v[g];
#pragma unroll
    for (int i = 0; i < 4; ++i) s += w3[g * 4 + i] * a[i];
  }
  out[p] = fmaxf(s + b3[0], 0.f);
}

// ---- the tail ---------------------------------------------------------------------------------------------------------------------------
// unsigned keys in the order of the floats: negative values have all bits flipped, the others the sign bit set
__device__ __forceinline__ unsigned order_key(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

__global__ void k_minmax_init(unsigned* __restrict__ keys, int images) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < images) {
    keys[2 * i] = 0u;           // the maximum: below every float
    keys[2 * i + 1] = ~0u;      // the minimum: above every float
  }
}

// torch's upsample_bicubic2d: A = -0.75, source = scale * (dst + 0.5) - 0.5, indices clamped to the plane
__device__ __forceinline__ void cubic_taps(int d, float scale, float* wt, int& i0) {
  const float A = -0.75f;
  const float s = fmaf(scale, (float)d + 0.5f, -0.5f);  // one rounding, as torch's contracted kernels: a coordinate one ulp off moves an upsampled value by 3e-6
  const float fl = floorf(s);
  const float t = s - fl;
  i0 = (int)fl;
  const float t1 = t + 1.0f, t2 = 1.0f - t, t3 = t2 + 1.0f;
  wt[0] = ((A * t1 - 5.0f * A) * t1 + 8.0f * A) * t1 - 4.0f * A;
  wt[1] = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
  wt[2] = ((A + 2.0f) * t2 - (A + 3.0f)) * t2 * t2 + 1.0f;
  wt[3] = ((A * t3 - 5.0f * A) * t3 + 8.0f * A) * t3 - 4.0f * A;
}

__global__ __launch_bounds__(256) void k_bicubic_f32(const float* __restrict__ src, float* __restrict__ dst, unsigned* __restrict__ keys, int sh, int sw, int dh,
                                                     int dw, float scale_y, float scale_x) {
  __shared__ float smax[4], smin[4];
  const int img = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = p < (int64_t)dh * dw;
  float v = 0.f;
  if (live) {
    const int oy = (int)(p / dw), ox = (int)(p - (int64_t)oy * dw);
    float wy[4], wx[4];
    int y0, x0;
    cubic_taps(oy, scale_y, wy, y0);
    cubic_taps(ox, scale_x, wx, x0);
    const float* s = src + (int64_t)img * sh * sw;
    int xi[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int x = x0 - 1 + i;
      xi[i] = x < 0 ? 0 : (x > sw - 1 ? sw - 1 : x);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int y = y0 - 1 + j;
      y = y < 0 ? 0 : (y > sh - 1 ? sh - 1 : y);
      const float* r = s + (int64_t)y * sw;
      const float row = ((r[xi[0]] * wx[0] + r[xi[1]] * wx[1]) + r[xi[2]] * wx[2]) + r[xi[3]] * wx[3];
      v += row * wy[j];
    }
    dst[(int64_t)img * dh * dw + p] = v;
  }
  float mx = live ? v : -INFINITY, mn = live ? v : INFINITY;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    mx = fmaxf(mx, __shfl_xor(mx, o));
    mn = fminf(mn, __shfl_xor(mn, o));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) smax[wave] = mx, smin[wave] = mn;
  __syncthreads();
  if (threadIdx.x == 0) {
    mx = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    mn = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
    atomicMax(keys + 2 * img, order_key(mx));
    atomicMin(keys + 2 * img + 1, order_key(mn));
  }
}

__global__ void k_minmax_values(const unsigned* __restrict__ keys, float* __restrict__ out, int images) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 2 * images) out[i] = key_value(keys[i]);
}

// mode 0 ("max"): d * 255 / max;  mode 1 ("minmax"): (d - min) / (max - min) * 255; fp32 operation for operation as numpy's, truncated toward
// zero into 0 .. 255: a value <= -1 saturates to 0 (numpy's cast there is platform-defined), a NaN counts as 0.  max <= 0 or max <= min: 0.
template <typename T>
__global__ __launch_bounds__(256) void k_depth_finish(const float* __restrict__ d, const unsigned* __restrict__ keys, uint8_t* __restrict__ map, T* __restrict__ ctrl,
                                                      int images, int64_t hw, int mode, int rep) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= images * hw) return;
  const int img = (int)(g / hw);
  const int64_t p = g - img * hw;
  const float mx = key_value(keys[2 * img]), mn = key_value(keys[2 * img + 1]);
  float v = 0.f;
  if (mode == 0) {
    if (mx > 0.f) v = __fdiv_rn(__fmul_rn(d[g], 255.0f), mx);
  } else {
    if (mx > mn) v = __fmul_rn(__fdiv_rn(__fsub_rn(d[g], mn), __fsub_rn(mx, mn)), 255.0f);
  }
  v = !(v > 0.f) ? 0.f : (v > 255.f ? 255.f : v);
  const int level = (int)v;
  if (map) map[g] = (uint8_t)level;
  if (ctrl) emit_control1(ctrl, images, img, hw, p, rep, level);
}

}  // namespace

extern "C" int ca_resize_pil_u8(const uint8_t* src, uint8_t* tmp, uint8_t* dst, int32_t images, int32_t sh, int32_t sw, int32_t dh, int32_t dw,
                                const int32_t* xbounds, const int32_t* xcoef, int32_t xksize, const int32_t* ybounds, const int32_t* ycoef, int32_t yksize,
                                void* stream) {
  CA_REQUIRE(src && tmp && dst && xbounds && xcoef && ybounds && ycoef, "ca_resize_pil_u8: src, tmp, dst and the four tables are required");
  CA_REQUIRE(sizes_ok(images, sh, sw, 3) && sizes_ok(images, dh, dw, 3) && sizes_ok(images, sh, dw, 3),
             "ca_resize_pil_u8: images=%d source %d x %d destination %d x %d (each >= 1, images * h * w * 3 < 2^31)", images, sh, sw, dh, dw);
  CA_REQUIRE(xksize >= 1 && xksize <= 4096 && yksize >= 1 && yksize <= 4096, "ca_resize_pil_u8: xksize=%d yksize=%d (1 .. 4096)", xksize, yksize);
  CA_REQUIRE((((uintptr_t)xbounds | (uintptr_t)xcoef | (uintptr_t)ybounds | (uintptr_t)ycoef) & 3) == 0, "ca_resize_pil_u8: the tables must be 4-byte aligned");
  CA_REQUIRE(tmp != src && tmp != dst && dst != src, "ca_resize_pil_u8: src, tmp and dst must be three buffers");
  hipStream_t st = (hipStream_t)stream;
  const int64_t t1 = (int64_t)images * sh * dw * 3, t2 = (int64_t)images * dh * dw * 3;
  hipLaunchKernelGGL(k_pil_pass, dim3((unsigned)((t1 + 255) / 256)), dim3(256), 0, st, src, tmp, t1, (int)sw, (int)dw, 3, xbounds, xcoef, (int)xksize);
  hipLaunchKernelGGL(k_pil_pass, dim3((unsigned)((t2 + 255) / 256)), dim3(256), 0, st, (const uint8_t*)tmp, dst, t2, (int)sh, (int)dh, 3 * dw, ybounds, ycoef,
                     (int)yksize);
  CA_CHECK_LAUNCH("ca_resize_pil_u8");
  return CA_OK;
}

extern "C" int ca_dpt_patches(const uint8_t* src, void* out, int32_t images, int32_t size, int32_t patch, int32_t dtype, void* stream) {
  CA_REQUIRE(src && out, "ca_dpt_patches: src and out are required");
  CA_REQUIRE(patch >= 8 && patch % 8 == 0 && size >= patch && size % patch == 0, "ca_dpt_patches: size=%d patch=%d (patch a multiple of 8, size a multiple of patch)",
             size, patch);
  CA_REQUIRE(sizes_ok(images, size, size, 6), "ca_dpt_patches: images=%d size=%d (images >= 1, images * size * size * 6 < 2^31)", images, size);
  CA_REQUIRE(dtype_ok(dtype), "ca_dpt_patches: dtype %d", dtype);
  CA_REQUIRE(((uintptr_t)out & 15) == 0, "ca_dpt_patches: out must be 16-byte aligned");
  const int64_t total = (int64_t)images * size * size * 3 / 8;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_dpt_patches<DT>, grid, block, 0, (hipStream_t)stream, src, (u16*)out, total, (int)size, (int)patch));
  CA_CHECK_LAUNCH("ca_dpt_patches");
  return CA_OK;
}

extern "C" int ca_depth_to_space(const void* x, void* y, int32_t images, int32_t gh, int32_t gw, int32_t k, int32_t cout, int64_t ldx, int32_t rows_per_image,
                                 int32_t row0, int32_t dtype, void* stream) {
  CA_REQUIRE(x && y, "ca_depth_to_space: x and y are required");
  CA_REQUIRE(k == 1 || k == 2 || k == 4, "ca_depth_to_space: k=%d (1, 2 or 4)", k);
  CA_REQUIRE(sizes_ok(images, gh, gw, k * k), "ca_depth_to_space: images=%d gh=%d gw=%d k=%d (each >= 1, images * gh k * gw k < 2^31)", images, gh, gw, k);
  CA_REQUIRE(cout >= 8 && cout % 8 == 0 && cout <= 4096, "ca_depth_to_space: cout=%d must be a multiple of 8 in 8 .. 4096", cout);
  CA_REQUIRE(ldx % 8 == 0 && ldx >= (int64_t)k * k * cout, "ca_depth_to_space: ldx=%lld (a multiple of 8, at least k * k * cout = %d)", (long long)ldx, k * k * cout);
  CA_REQUIRE(row0 >= 0 && rows_per_image >= row0 + (int64_t)gh * gw, "ca_depth_to_space: rows_per_image=%d row0=%d (row0 >= 0, row0 + gh * gw <= rows_per_image)",
             rows_per_image, row0);
  CA_REQUIRE((int64_t)images * rows_per_image * ldx * 2 <= kMaxBytes && (int64_t)images * gh * gw * k * k * cout * 2 <= kMaxBytes,
             "ca_depth_to_space: images=%d gh=%d gw=%d k=%d cout=%d: an operand would pass 2^31 bytes", images, gh, gw, k, cout);
  CA_REQUIRE(dtype_ok(dtype), "ca_depth_to_space: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0 && x != y, "ca_depth_to_space: x and y must be 16-byte aligned and distinct");
  const int64_t total = (int64_t)images * gh * gw * k * k * (cout / 8);
  hipLaunchKernelGGL(k_depth_to_space, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const u16*)x, (u16*)y, total, (int)gh, (int)gw, (int)k,
                     (int)cout, ldx, (int)rows_per_image, (int)row0);
  CA_CHECK_LAUNCH("ca_depth_to_space");
  return CA_OK;
}

extern "C" int ca_dpt_head_supported(int32_t cmid) { return cmid == 32 || cmid == 64 || cmid == 128; }

extern "C" int ca_dpt_head(const void* x, const void* w2, const float* b2, const float* w3, const float* b3, float* out, int32_t images, int32_t h, int32_t w,
                           int32_t cmid, int32_t dtype, void* stream) {
  CA_REQUIRE(x && w2 && b2 && w3 && b3 && out, "ca_dpt_head: x, w2, b2, w3, b3 and out are required");
  CA_REQUIRE(sizes_ok(images, h, w, 4), "ca_dpt_head: images=%d h=%d w=%d (each >= 1, images * 2 h * 2 w < 2^31)", images, h, w);
  CA_REQUIRE(ca_dpt_head_supported(cmid), "ca_dpt_head: cmid=%d (32, 64 or 128; the composed head serves the rest)", cmid);
  CA_REQUIRE((int64_t)images * h * w * cmid * 2 <= kMaxBytes, "ca_dpt_head: images=%d h=%d w=%d cmid=%d: x would pass 2^31 bytes", images, h, w, cmid);
  CA_REQUIRE(dtype_ok(dtype), "ca_dpt_head: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)w2) & 15) == 0 && (((uintptr_t)b2 | (uintptr_t)w3 | (uintptr_t)b3 | (uintptr_t)out) & 3) == 0,
             "ca_dpt_head: x and w2 must be 16-byte aligned, b2, w3, b3 and out 4-byte aligned");
  const int tx = ceil_div_i(2 * w, HD_T), ty = ceil_div_i(2 * h, HD_T);
  const int64_t blocks = (int64_t)images * tx * ty;
  CA_REQUIRE(blocks < ((int64_t)1 << 31), "ca_dpt_head: grid too large");
  const dim3 grid((unsigned)blocks), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_dpt_head<DT>, grid, block, 0, (hipStream_t)stream, (const u16*)x, (const u16*)w2, b2, w3, b3, out, (int)h, (int)w, (int)cmid, tx, ty));
  CA_CHECK_LAUNCH("ca_dpt_head");
  return CA_OK;
}

extern "C" int ca_dpt_logit(const float* t, const float* w3, const float* b3, float* out, int64_t pixels, void* stream) {
  CA_REQUIRE(t && w3 && b3 && out, "ca_dpt_logit: t, w3, b3 and out are required");
  CA_REQUIRE(pixels >= 1 && pixels <= kMaxPixels, "ca_dpt_logit: pixels=%lld (1 .. 2^31 - 1)", (long long)pixels);
  CA_REQUIRE(((uintptr_t)t & 15) == 0 && (((uintptr_t)w3 | (uintptr_t)b3 | (uintptr_t)out) & 3) == 0, "ca_dpt_logit: t must be 16-byte aligned, w3, b3 and out 4-byte aligned");
  hipLaunchKernelGGL(k_dpt_logit, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, (hipStream_t)stream, t, w3, b3, out, pixels);
  CA_CHECK_LAUNCH("ca_dpt_logit");
  return CA_OK;
}

extern "C" int ca_resize_bicubic_f32(const float* src, float* dst, void* minmax_keys, float* minmax, int32_t images, int32_t sh, int32_t sw, int32_t dh, int32_t dw,
                                     void* stream) {
  CA_REQUIRE(src && dst && minmax_keys, "ca_resize_bicubic_f32: src, dst and minmax_keys are required");
  CA_REQUIRE(sizes_ok(images, sh, sw) && sizes_ok(images, dh, dw) && images <= 65535,
             "ca_resize_bicubic_f32: images=%d source %d x %d destination %d x %d (each >= 1, images <= 65535, images * h * w < 2^31)", images, sh, sw, dh, dw);
  CA_REQUIRE((((uintptr_t)src | (uintptr_t)dst | (uintptr_t)minmax_keys | (uintptr_t)minmax) & 3) == 0 && src != dst,
             "ca_resize_bicubic_f32: the buffers must be 4-byte aligned, src and dst distinct");
  hipStream_t st = (hipStream_t)stream;
  unsigned* keys = (unsigned*)minmax_keys;
  hipLaunchKernelGGL(k_minmax_init, dim3((unsigned)((images + 255) / 256)), dim3(256), 0, st, keys, (int)images);
  const dim3 grid((unsigned)(((int64_t)dh * dw + 255) / 256), (unsigned)images);
  hipLaunchKernelGGL(k_bicubic_f32, grid, dim3(256), 0, st, src, dst, keys, (int)sh, (int)sw, (int)dh, (int)dw, (float)sh / (float)dh, (float)sw / (float)dw);
  if (minmax) hipLaunchKernelGGL(k_minmax_values, dim3((unsigned)((2 * images + 255) / 256)), dim3(256), 0, st, (const unsigned*)keys, minmax, (int)images);
  CA_CHECK_LAUNCH("ca_resize_bicubic_f32");
  return CA_OK;
}

extern "C" int ca_depth_finish(const float* depth, const void* minmax_keys, int32_t images, int32_t h, int32_t w, int32_t mode, uint8_t* map, void* control,
                               int32_t rep, int32_t control_dtype, void* stream) {
  CA_REQUIRE(depth && minmax_keys, "ca_depth_finish: depth and minmax_keys are required");
  CA_REQUIRE(sizes_ok(images, h, w, 6), "ca_depth_finish: images=%d h=%d w=%d (each >= 1, images * h * w * 6 < 2^31)", images, h, w);
  CA_REQUIRE(mode == 0 || mode == 1, "ca_depth_finish: mode=%d (0 max, 1 minmax)", mode);
  if (const int rc = control_out_checks("ca_depth_finish", false, h, w, "map", map || control, rep, control_dtype)) return rc;
  CA_REQUIRE((((uintptr_t)depth | (uintptr_t)minmax_keys) & 3) == 0 && ctrl_aligned(control, control_dtype, 1),
             "ca_depth_finish: depth and minmax_keys must be 4-byte aligned, control aligned to its element");
  const int64_t hw = (int64_t)h * w, total = (int64_t)images * hw;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  CA_DISPATCH_CTRL(control_dtype,
                   hipLaunchKernelGGL(k_depth_finish<T>, grid, block, 0, st, depth, (const unsigned*)minmax_keys, map, (T*)control, (int)images, hw, (int)mode, (int)rep));
  CA_CHECK_LAUNCH("ca_depth_finish");
  return CA_OK;
}
