// Added to ABI v16: the stages of the lineart annotator that ca_conv3x3 / ca_gemm do not cover (controlanimate_amd/lineart.py:
// LineartAnnotator; the specification is tests/lineart_ref.py, restated from the published "informative drawings" Generator and
// controlnet_aux's LineartDetector).  The two stride-2 and the six 256 -> 256 convolutions run on ca_conv3x3; around them:
//
//   conv_in   k_lineart_conv_in   uint8 RGB [n,H,W,3] -> the 7x7, 3 -> 64 convolution's output [n,H,W,64] (before its InstanceNorm):
//                                 reflection padding 3 and the / 255 folded in; MFMA 16x16x32 with K = 147 padded to 160, the B
//                                 operand gathered from an LDS tile of the byte frame (no im2col tensor in memory)
//   instnorm  k_in_stats          per (image, channel) shifted sums over H x W as fp32 partials per chunk of pixels,
//             k_in_apply          combined in a fixed order by every block that applies them: (x - mean) * rstd, optional ReLU,
//                                 optional residual add, optionally written reflection-padded by 1; the input (and the residual) may
//                                 be stored with a one-pixel ring that is ignored -- what lets ca_conv3x3 (zero padding 1) serve the
//                                 reflection-padded convolutions of the residual blocks: its result on the padded tensor is right
//                                 in the interior
//   convt     k_convt_gather      ConvTranspose2d(k 3, s 2, p 1, op 1) as ONE ca_gemm with N = 9 * Cout (every tap of every input
//                                 pixel) and this gather, which sums the 1 / 2 / 2 / 4 taps of an output pixel by its phase: no
//                                 zero-stuffed tensor
//   conv_out  k_lineart_conv_out  64 -> 1, 7x7, reflection padding 3 -> fp32 logits [n,H,W]: an LDS tile of the input per 16x16
//                                 outputs, fp32 weights through the scalar cache, fp32 accumulation
//   finish    k_lineart_finish    255 - trunc(clip(sigmoid(logit) * 255)) -> the uint8 map and / or the control tensor
//                                 [rep * n,3,H,W] with map / 255 (the contract in ca_annot.h)
//
// No launch depends on device data on the host side: the chain can be captured in a hipGraph.  No atomics: two runs give the same bits.
#include "ca_common.h"
#include "ca_annot.h"

namespace {

// index i of an axis of n >= 2 samples padded by reflection (no repeated edge); an index that reflection does not bring inside --
// a tile's overhang past the image, never read by a live output -- is clamped
__device__ __forceinline__ int reflect_clamp(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * n - 2 - i;
  return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// ---- input convolution --------------------------------------------------------------------------------------------------------------
// A block owns a 16 x 64 tile of output pixels and keeps the 22 x 70 pixels of the byte frame under it in LDS.  k = ky * 21 + kx * 3 + c:
// for one ky the 21 values of a pixel are 21 consecutive bytes of a tile row.  The weights [64][160] are the A operand (4 row tiles x
// 5 k-steps, held in registers for the whole block), 16 pixels of one tile row the B operand: a lane ends up with 4 consecutive output
// channels of one pixel per row tile -- one 8-byte store each.
constexpr int CI_TH = 16, CI_TW = 64, CI_K = 147, CI_KP = 160;
constexpr int CI_PITCH = (CI_TW + 6) * 3 + 2;  // bytes per tile row

template <int DT>
__global__ __launch_bounds__(256) void k_lineart_conv_in(const uint8_t* __restrict__ src, const u16* __restrict__ wp, u16* __restrict__ dst, int h, int w,
                                                         int tiles_x, int tiles_y) {
  __shared__ uint8_t tile[(CI_TH + 6) * CI_PITCH];
  const int bx = blockIdx.x % tiles_x;
  const int by = (blockIdx.x / tiles_x) % tiles_y;
  const int img = blockIdx.x / (tiles_x * tiles_y);
  const int y0 = by * CI_TH, x0 = bx * CI_TW;
  const uint8_t* s = src + (int64_t)img * h * w * 3;
  for (int i = threadIdx.x; i < (CI_TH + 6) * (CI_TW + 6); i += 256) {
    const int r = i / (CI_TW + 6), c = i - r * (CI_TW + 6);
    const uint8_t* p = s + ((int64_t)reflect_clamp(y0 - 3 + r, h) * w + reflect_clamp(x0 - 3 + c, w)) * 3;
    uint8_t* t = tile + r * CI_PITCH + c * 3;
    t[0] = p[0], t[1] = p[1], t[2] = p[2];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, r16 = lane & 15;
  u32x4 wf[4][5];
  int off[5][8];
#pragma unroll
  for (int ks = 0; ks < 5; ++ks) {
#pragma unroll
    for (int t = 0; t < 4; ++t) wf[t][ks] = ld16(wp + (t * 16 + r16) * CI_KP + ks * 32 + q * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = ks * 32 + q * 8 + e;
      off[ks][e] = k < CI_K ? (k / 21) * CI_PITCH + (k % 21) : 0;  // (the padded columns of the weight are zero: any byte of the tile will do)
    }
  }
  __syncthreads();
  for (int it = 0; it < 16; ++it) {
    const int row = wave * 4 + (it >> 2), px = (it & 3) * 16 + r16;
    if (y0 + row >= h || x0 + (it & 3) * 16 >= w) continue;  // wave-uniform
    const uint8_t* base = tile + row * CI_PITCH + px * 3;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 5; ++ks) {
      u32x4 b;
#pragma unroll
      for (int e = 0; e < 4; ++e) b[e] = pack2<DT>((float)base[off[ks][2 * e]], (float)base[off[ks][2 * e + 1]]);  // 0 .. 255: exact in fp16 and bf16
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = Elem<DT>::mfma(wf[t][ks], b, acc[t]);
    }
    const int gy = y0 + row, gx = x0 + px;
    if (gx < w) {
      u16* d = dst + (((int64_t)img * h + gy) * w + gx) * 64 + q * 4;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        u32x2 v;
        v[0] = pack2<DT>(__fdiv_rn(acc[t][0], 255.0f), __fdiv_rn(acc[t][1], 255.0f));
        v[1] = pack2<DT>(__fdiv_rn(acc[t][2], 255.0f), __fdiv_rn(acc[t][3], 255.0f));
        *(u32x2*)(d + t * 16) = v;
      }
    }
  }
}

// ---- InstanceNorm ---------------------------------------------------------------------------------------------------------------------
// Chunks of pixels per image: a block of either kernel moves about 512 KiB.
__host__ __device__ inline int in_chunk_pixels(int c) { return 262144 / c; }
inline int in_chunks(int64_t hw, int c) { return (int)((hw + in_chunk_pixels(c) - 1) / in_chunk_pixels(c)); }

// pixel p (row-major in h x w) of image img -> element offset of its channel 0 in a tensor stored with `ring` extra pixels all round
__device__ __forceinline__ int64_t pix_off(int img, int p, int h, int w, int c, int ring) {
  const int y = p / w, x = p - y * w;
  return (((int64_t)img * (h + 2 * ring) + y + ring) * (w + 2 * ring) + x + ring) * c;
}

// partials [images][chunks][2][c]: sum and sum of squares of x - shift over the chunk's pixels, shift = the image's first pixel of
// that channel (the subtraction keeps var = E[d^2] - E[d]^2 free of cancellation when |mean| >> std).  A thread owns 8 channels of
// every (256 / (c / 8))-th pixel; the threads of a channel are added through LDS in thread order.
template <int DT>
__global__ __launch_bounds__(256) void k_in_stats(const u16* __restrict__ x, float* __restrict__ partials, int h, int w, int c, int ring, int chunks) {
  __shared__ float red[4096];  // [256 / cl][2][c]
  const int img = blockIdx.x / chunks, chunk = blockIdx.x - img * chunks;
  const int cl = c >> 3, j = threadIdx.x % cl, pl = threadIdx.x / cl, npl = 256 / cl;
  const int hw = h * w, per = in_chunk_pixels(c);
  const int p0 = chunk * per, p1 = p0 + per < hw ? p0 + per : hw;
  float k8[8], s[8], ss[8];
  unpack8<DT>(ld16(x + pix_off(img, 0, h, w, c, ring) + j * 8), k8);
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = 0.f, ss[e] = 0.f;
  for (int p = p0 + pl; p < p1; p += npl) {
    float f[8];
    unpack8<DT>(ld16(x + pix_off(img, p, h, w, c, ring) + j * 8), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float d = f[e] - k8[e];
      s[e] += d;
      ss[e] = fmaf(d, d, ss[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    red[(pl * 2 + 0) * c + j * 8 + e] = s[e];
    red[(pl * 2 + 1) * c + j * 8 + e] = ss[e];
  }
  __syncthreads();
  float* out = partials + ((int64_t)img * chunks + chunk) * 2 * c;
  for (int i = threadIdx.x; i < 2 * c; i += 256) {
    float a = 0.f;
    for (int k = 0; k < npl; ++k) a += red[k * 2 * c + i];
    out[i] = a;
  }
}

template <int DT>
__global__ __launch_bounds__(256) void k_in_apply(const u16* __restrict__ x, const float* __restrict__ partials, const u16* __restrict__ res, u16* __restrict__ y,
                                                  int h, int w, int c, int in_ring, int res_ring, int out_pad, int relu, int chunks, float eps) {
  __shared__ float mean_s[256], rstd_s[256];
  const int img = blockIdx.x / chunks, chunk = blockIdx.x - img * chunks;
  const int hw = h * w;
  for (int ch = threadIdx.x; ch < c; ch += 256) {
    const float* p = partials + (int64_t)img * chunks * 2 * c + ch;
    float s = 0.f, ss = 0.f;
    for (int k = 0; k < chunks; ++k) {  // fixed order
      s += p[(int64_t)k * 2 * c];
      ss += p[(int64_t)k * 2 * c + c];
    }
    const float inv = 1.0f / (float)hw;
    const float m = s * inv;
    float var = fmaf(-m, m, ss * inv);  // biased
    var = var > 0.f ? var : 0.f;
    mean_s[ch] = Elem<DT>::to_f(x[pix_off(img, 0, h, w, c, in_ring) + ch]) + m;
    rstd_s[ch] = 1.0f / sqrtf(var + eps);
  }
  __syncthreads();
  const int cl = c >> 3, j = threadIdx.x % cl, pl = threadIdx.x / cl, npl = 256 / cl;
  const int per = in_chunk_pixels(c);
  const int p0 = chunk * per, p1 = p0 + per < hw ? p0 + per : hw;
  float mu[8], rs[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) mu[e] = mean_s[j * 8 + e], rs[e] = rstd_s[j * 8 + e];
  for (int p = p0 + pl; p < p1; p += npl) {
    float f[8];
    unpack8<DT>(ld16(x + pix_off(img, p, h, w, c, in_ring) + j * 8), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      f[e] = (f[e] - mu[e]) * rs[e];
      if (relu) f[e] = fmaxf(f[e], 0.f);
    }
    if (res) {
      float r[8];
      unpack8<DT>(ld16(res + pix_off(img, p, h, w, c, res_ring) + j * 8), r);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] += r[e];
    }
    const u32x4 v = pack8<DT>(f);
    if (!out_pad) {
      st16(y + pix_off(img, p, h, w, c, 0) + j * 8, v);
    } else {
      // padded row 0 mirrors interior row 1, padded row h + 1 interior row h - 2 (the same for columns): the pixel's owner writes its mirrors
      const int yy = p / w, xx = p - yy * w;
      int rows[3], cols[3], nr = 0, nc = 0;
      rows[nr++] = yy + 1;
      if (yy == 1) rows[nr++] = 0;
      if (yy == h - 2) rows[nr++] = h + 1;
      cols[nc++] = xx + 1;
      if (xx == 1) cols[nc++] = 0;
      if (xx == w - 2) cols[nc++] = w + 1;
      for (int a = 0; a < nr; ++a)
        for (int b = 0; b < nc; ++b) st16(y + (((int64_t)img * (h + 2) + rows[a]) * (w + 2) + cols[b]) * c + j * 8, v);
    }
  }
}

// ---- transposed convolution: the gather behind the 9-tap GEMM ---------------------------------------------------------------------------
// taps [images, h, w, 3, 3, cout]: taps[p][ky][kx] = W[ky][kx] . x[p].  Output pixel (2 i + py, 2 j + px) sums, over dy <= py and
// dx <= px with (i + dy, j + dx) inside the image, taps[i + dy, j + dx][ky][kx] with ky = 1 for py = 0, else 2 - 2 dy (kx likewise):
//   (0,0): W11 x[i,j]      (0,1): W12 x[i,j] + W10 x[i,j+1]      (1,0): W21 x[i,j] + W01 x[i+1,j]
//   (1,1): W22 x[i,j] + W20 x[i,j+1] + W02 x[i+1,j] + W00 x[i+1,j+1]        -- added in this order, in fp32
template <int DT>
__global__ __launch_bounds__(256) void k_convt_gather(const u16* __restrict__ taps, u16* __restrict__ y, int64_t total, int h, int w, int cout) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cl = cout >> 3;
  const int cj = (int)(idx % cl);
  const int64_t op = idx / cl;
  const int ox = (int)(op % (2 * w));
  const int oy = (int)((op / (2 * w)) % (2 * h));
  const int64_t img = op / ((int64_t)4 * h * w);
  const int i = oy >> 1, py = oy & 1, j = ox >> 1, px = ox & 1;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int dy = 0; dy <= py; ++dy)
    for (int dx = 0; dx <= px; ++dx) {
      if (i + dy >= h || j + dx >= w) continue;  // the zero row and column past the edge
      const int ky = py ? 2 - 2 * dy : 1, kx = px ? 2 - 2 * dx : 1;
      float f[8];
      unpack8<DT>(ld16(taps + (((img * h + i + dy) * w + j + dx) * 9 + ky * 3 + kx) * cout + cj * 8), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += f[e];
    }
  st16(y + op * cout + cj * 8, pack8<DT>(acc));
}

// ---- output convolution ---------------------------------------------------------------------------------------------------------------
// A block owns 16 x 16 output pixels, a thread one of them.  The 22 x 22 input pixels under the tile go through LDS in two halves of
// 32 channels (a pixel every 80 bytes: the 16 lanes of a quarter wave read 16 different bank groups).  The weight index is the same in
// every lane: the compiler reads it through the scalar cache.
constexpr int CO_T = 16, CO_IN = CO_T + 6, CO_PIX = 40;  // u16 per pixel in LDS: 32 channels + 8 of padding

template <int DT>
__global__ __launch_bounds__(256) void k_lineart_conv_out(const u16* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ bias,
                                                          float* __restrict__ logits, int h, int w, int tiles_x, int tiles_y) {
  __shared__ __attribute__((aligned(16))) u16 tile[CO_IN * CO_IN * CO_PIX];
  const int bx = blockIdx.x % tiles_x;
  const int by = (blockIdx.x / tiles_x) % tiles_y;
  const int img = blockIdx.x / (tiles_x * tiles_y);
  const int y0 = by * CO_T, x0 = bx * CO_T;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  const u16* xi = x + (int64_t)img * h * w * 64;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int half = 0; half < 2; ++half) {
    if (half) __syncthreads();
    for (int i = threadIdx.x; i < CO_IN * CO_IN * 4; i += 256) {
      const int pix = i >> 2, part = i & 3;
      const int r = pix / CO_IN, c = pix - r * CO_IN;
      const int64_t g = (int64_t)reflect_clamp(y0 - 3 + r, h) * w + reflect_clamp(x0 - 3 + c, w);
      st16(tile + pix * CO_PIX + part * 8, ld16(xi + g * 64 + half * 32 + part * 8));
    }
    __syncthreads();
    for (int ky = 0; ky < 7; ++ky)
      for (int kx = 0; kx < 7; ++kx) {
        const u16* t = tile + ((ty + ky) * CO_IN + tx + kx) * CO_PIX;
        const float* wk = wt + (ky * 7 + kx) * 64 + half * 32;
#pragma unroll
        for (int part = 0; part < 4; ++part) {
          float f[8];
          unpack8<DT>(ld16(t + part * 8), f);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e & 3] = fmaf(f[e], wk[part * 8 + e], acc[e & 3]);
        }
      }
  }
  const int gy = y0 + ty, gx = x0 + tx;
  if (gy < h && gx < w) logits[((int64_t)img * h + gy) * w + gx] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + bias[0];
}

// ---- sigmoid, quantise, invert ----------------------------------------------------------------------------------------------------------
// 4 consecutive pixels per thread (h * w % 4 == 0): one 4-byte store to the map, 16 / 8-byte stores to the control tensor
template <typename T>
__global__ __launch_bounds__(256) void k_lineart_finish(const float* __restrict__ logits, uint8_t* __restrict__ map, T* __restrict__ ctrl, int images, int64_t hw,
                                                        int rep) {
  const int64_t g0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (g0 >= images * hw) return;
  const int img = (int)(g0 / hw);
  const int64_t p = g0 - img * hw;
  const f32x4 v = *(const f32x4*)(logits + g0);
  int level[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double e = (1.0 / (1.0 + exp(-(double)v[i]))) * 255.0;
    e = !(e > 0.0) ? 0.0 : (e > 255.0 ? 255.0 : e);  // (a NaN logit counts as 0)
    level[i] = 255 - (int)e;                         // truncation, as astype(uint8) of a value in [0, 255]
  }
  if (map) *(uint32_t*)(map + g0) = pack_levels4(level);
  if (ctrl) emit_control4(ctrl, images, img, hw, p, rep, level);
}

inline bool in_c_ok(int32_t c) { return c == 64 || c == 128 || c == 256; }

}  // namespace

extern "C" int ca_lineart_conv_in(const uint8_t* src, const void* w_packed, void* dst, int32_t images, int32_t h, int32_t w, int32_t dtype, void* stream) {
  CA_REQUIRE(src && w_packed && dst, "ca_lineart_conv_in: src, w_packed and dst are required");
  CA_REQUIRE(sizes_ok(images, h, w) && h >= 4 && w >= 4, "ca_lineart_conv_in: images=%d h=%d w=%d (images >= 1, h and w >= 4, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE(dtype_ok(dtype), "ca_lineart_conv_in: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)w_packed | (uintptr_t)dst) & 15) == 0, "ca_lineart_conv_in: w_packed and dst must be 16-byte aligned");
  const int tx = ceil_div_i(w, CI_TW), ty = ceil_div_i(h, CI_TH);
  const int64_t blocks = (int64_t)images * tx * ty;
  CA_REQUIRE(blocks < ((int64_t)1 << 31), "ca_lineart_conv_in: grid too large");
  const dim3 grid((unsigned)blocks), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_lineart_conv_in<DT>, grid, block, 0, (hipStream_t)stream, src, (const u16*)w_packed, (u16*)dst, (int)h, (int)w, tx, ty));
  CA_CHECK_LAUNCH("ca_lineart_conv_in");
  return CA_OK;
}

extern "C" int64_t ca_instnorm_partials_floats(int32_t images, int32_t h, int32_t w, int32_t c) {
  if (!sizes_ok(images, h, w) || !in_c_ok(c)) return 0;
  return (int64_t)images * in_chunks((int64_t)h * w, c) * 2 * c;
}

static int instnorm_common(const char* who, const void* x, const void* partials, int32_t images, int32_t h, int32_t w, int32_t c, int32_t in_ring, int32_t dtype) {
  CA_REQUIRE(x && partials, "%s: x and partials are required", who);
  CA_REQUIRE(in_ring == 0 || in_ring == 1, "%s: in_ring=%d (0 or 1)", who, in_ring);
  CA_REQUIRE(sizes_ok(images, h + 2, w + 2), "%s: images=%d h=%d w=%d (each >= 1, images * (h + 2) * (w + 2) < 2^31)", who, images, h, w);
  CA_REQUIRE(in_c_ok(c), "%s: c=%d (64, 128 or 256)", who, c);
  CA_REQUIRE(dtype_ok(dtype), "%s: dtype %d", who, dtype);
  CA_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)partials & 3) == 0, "%s: x must be 16-byte aligned, partials 4-byte aligned", who);
  CA_REQUIRE((int64_t)images * in_chunks((int64_t)h * w, c) < ((int64_t)1 << 31), "%s: grid too large", who);
  return CA_OK;
}

extern "C" int ca_instnorm_stats(const void* x, float* partials, int32_t images, int32_t h, int32_t w, int32_t c, int32_t in_ring, int32_t dtype, void* stream) {
  const int rc = instnorm_common("ca_instnorm_stats", x, partials, images, h, w, c, in_ring, dtype);
  if (rc != CA_OK) return rc;
  const int chunks = in_chunks((int64_t)h * w, c);
  const dim3 grid((unsigned)((int64_t)images * chunks)), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_in_stats<DT>, grid, block, 0, (hipStream_t)stream, (const u16*)x, partials, (int)h, (int)w, (int)c, (int)in_ring, chunks));
  CA_CHECK_LAUNCH("ca_instnorm_stats");
  return CA_OK;
}

extern "C" int ca_instnorm_apply(const void* x, const float* partials, const void* residual, void* y, int32_t images, int32_t h, int32_t w, int32_t c,
                                 int32_t in_ring, int32_t res_ring, int32_t out_pad, int32_t relu, float eps, int32_t dtype, void* stream) {
  const int rc = instnorm_common("ca_instnorm_apply", x, partials, images, h, w, c, in_ring, dtype);
  if (rc != CA_OK) return rc;
  CA_REQUIRE(y && ((uintptr_t)y & 15) == 0 && ((uintptr_t)residual & 15) == 0, "ca_instnorm_apply: y is required; y and residual must be 16-byte aligned");
  CA_REQUIRE((res_ring == 0 || res_ring == 1) && (out_pad == 0 || out_pad == 1) && (relu == 0 || relu == 1),
             "ca_instnorm_apply: res_ring=%d out_pad=%d relu=%d (each 0 or 1)", res_ring, out_pad, relu);
  CA_REQUIRE(!out_pad || (h >= 2 && w >= 2), "ca_instnorm_apply: out_pad needs h >= 2 and w >= 2 (reflection by one pixel), got %d x %d", h, w);
  CA_REQUIRE(eps > 0.f, "ca_instnorm_apply: eps=%g must be positive", (double)eps);
  const int chunks = in_chunks((int64_t)h * w, c);
  const dim3 grid((unsigned)((int64_t)images * chunks)), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_in_apply<DT>, grid, block, 0, (hipStream_t)stream, (const u16*)x, partials, (const u16*)residual, (u16*)y, (int)h, (int)w, (int)c,
                       (int)in_ring, (int)res_ring, (int)out_pad, (int)relu, chunks, eps));
  CA_CHECK_LAUNCH("ca_instnorm_apply");
  return CA_OK;
}

extern "C" int ca_convt3x3s2_gather(const void* taps, void* y, int32_t images, int32_t h, int32_t w, int32_t cout, int32_t dtype, void* stream) {
  CA_REQUIRE(taps && y, "ca_convt3x3s2_gather: taps and y are required");
  CA_REQUIRE(sizes_ok(images, h, w, 4), "ca_convt3x3s2_gather: images=%d h=%d w=%d (each >= 1, images * 2 h * 2 w < 2^31)", images, h, w);
  CA_REQUIRE(cout >= 8 && cout % 8 == 0 && cout <= 1024, "ca_convt3x3s2_gather: cout=%d must be a multiple of 8 in 8 .. 1024", cout);
  CA_REQUIRE(dtype_ok(dtype), "ca_convt3x3s2_gather: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)taps | (uintptr_t)y) & 15) == 0, "ca_convt3x3s2_gather: taps and y must be 16-byte aligned");
  const int64_t total = (int64_t)images * 4 * h * w * (cout / 8);
  CA_REQUIRE((total + 255) / 256 < ((int64_t)1 << 31), "ca_convt3x3s2_gather: grid too large");
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_convt_gather<DT>, grid, block, 0, (hipStream_t)stream, (const u16*)taps, (u16*)y, total, (int)h, (int)w, (int)cout));
  CA_CHECK_LAUNCH("ca_convt3x3s2_gather");
  return CA_OK;
}

extern "C" int ca_lineart_conv_out(const void* x, const float* wt, const float* bias, float* logits, int32_t images, int32_t h, int32_t w, int32_t dtype,
                                   void* stream) {
  CA_REQUIRE(x && wt && bias && logits, "ca_lineart_conv_out: x, wt, bias and logits are required");
  CA_REQUIRE(sizes_ok(images, h, w) && h >= 4 && w >= 4, "ca_lineart_conv_out: images=%d h=%d w=%d (images >= 1, h and w >= 4, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE(dtype_ok(dtype), "ca_lineart_conv_out: dtype %d", dtype);
  CA_REQUIRE(((uintptr_t)x & 15) == 0 && (((uintptr_t)wt | (uintptr_t)bias | (uintptr_t)logits) & 3) == 0,
             "ca_lineart_conv_out: x must be 16-byte aligned, wt, bias and logits 4-byte aligned");
  const int tx = ceil_div_i(w, CO_T), ty = ceil_div_i(h, CO_T);
  const int64_t blocks = (int64_t)images * tx * ty;
  CA_REQUIRE(blocks < ((int64_t)1 << 31), "ca_lineart_conv_out: grid too large");
  const dim3 grid((unsigned)blocks), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_lineart_conv_out<DT>, grid, block, 0, (hipStream_t)stream, (const u16*)x, wt, bias, logits, (int)h, (int)w, tx, ty));
  CA_CHECK_LAUNCH("ca_lineart_conv_out");
  return CA_OK;
}

extern "C" int ca_lineart_finish(const float* logits, int32_t images, int32_t h, int32_t w, uint8_t* map, void* control, int32_t rep, int32_t control_dtype,
                                 void* stream) {
  CA_REQUIRE(logits, "ca_lineart_finish: logits are required");
  CA_REQUIRE(sizes_ok(images, h, w), "ca_lineart_finish: images=%d h=%d w=%d (each >= 1, images * h * w < 2^31)", images, h, w);
  if (const int rc = control_out_checks("ca_lineart_finish", true, h, w, "map", map || control, rep, control_dtype)) return rc;
  CA_REQUIRE(((uintptr_t)logits & 15) == 0 && ((uintptr_t)map & 3) == 0 && ctrl_aligned(control, control_dtype, 4),
             "ca_lineart_finish: logits must be 16-byte aligned, map 4-byte aligned, control aligned to four of its elements");
  const int64_t hw = (int64_t)h * w, total = (int64_t)images * hw;
  const dim3 grid((unsigned)((total / 4 + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  CA_DISPATCH_CTRL(control_dtype, hipLaunchKernelGGL(k_lineart_finish<T>, grid, block, 0, st, logits, map, (T*)control, (int)images, hw, (int)rep));
  CA_CHECK_LAUNCH("ca_lineart_finish");
  return CA_OK;
}
