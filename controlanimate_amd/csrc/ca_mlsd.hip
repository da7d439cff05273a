// Added to ABI v16: the stages of the M-LSD straight-line annotator that ca_conv3x3 / ca_gemm / ca_add_bcast do not cover
// (controlanimate_amd/mlsd.py: MlsdAnnotator; the specification is tests/mlsd_ref.py, restated from the published MobileV2_MLSD_Large,
// its decode and OpenCV's line iterator).  The stem, the two 3x3 convolutions of a block B and the second convolution of block C run on
// ca_conv3x3, every 1x1 convolution on ca_gemm; around them:
//
//   prep      MlsdFill        uint8 RGB [n,H,W,3] -> [n,H,W,8]: x / 127.5 - 1 in channels 0..2, the constant 1 / 127.5 - 1 in channel 3
//                             (the detector's channel of ones), zeros in 4..7 (the stem's weight is zero-padded to 8 input channels)
//   dw        k_dwconv3x3     depthwise 3x3, stride 1 (padding 1) or 2 (one row / column of zeros after, none before), fp32 bias,
//                             optional ReLU6.  A thread owns 8 channels (16 bytes) of one output column and walks down a strip of
//                             output rows; the nine taps of its channels stay in registers.  Rows are reused by REGISTER ROTATION of
//                             the output rows in flight (an input row adds its three horizontal sums to the up to three output rows
//                             it belongs to, then is dropped), so a thread reads each input row of its strip once; the two horizontal
//                             neighbours are the loads of the adjacent lanes and hit the L1 line those lanes fetch.  An LDS row ring
//                             would add a store, a barrier and a load per row for the same global traffic.
//   up        k_up2_ac        bilinear x2 with align_corners into a column range of a wider tensor (one half of a concatenation)
//   dil       k_conv3x3_dil   3x3, 64 -> 64, dilation 5, padding 5, bias, optional ReLU on the 16x16x32 MFMA: a block owns 16 x 16
//                             output pixels and keeps the 26 x 26 halo in LDS, 32 channels at a time (two passes; 53 KB), the B operand
//                             read straight out of it per tap; the weights are the A operand, read per tap from L2 (72 KB in all)
//   decode    k_mlsd_decode   one block per frame: sigmoid, 3x3 plateau-keeping maximum test and the score threshold feed a candidate
//                             list; the exact top 200 by (score descending, index ascending) through an 8-pass radix select on the
//                             64-bit key (score bits, ~index); distance test, float64 endpoints; segments in rank order
//   draw      k_mlsd_draw     one lane per segment: OpenCV's clipLine and 8-connected line iterator, byte stores of 255
//             k_mlsd_emit     the map -> the control tensor [rep * n,3,H,W] (ca_annot.h)
//
// No launch depends on device data on the host side: the chain can be captured in a hipGraph.  The only atomics are integer LDS
// counters whose arrival order never reaches the output (the candidates are ranked afterwards): two runs give the same bits.
#include "ca_common.h"
#include "ca_annot.h"

namespace {

constexpr int kTopK = CA_MLSD_TOPK;

// ---- prep ------------------------------------------------------------------------------------------------------------------------
struct MlsdFill {
  __device__ __forceinline__ void operator()(const uint8_t* s, float f[8]) const {
#pragma unroll
    for (int c = 0; c < 3; ++c) f[c] = __fdiv_rn((float)s[c], 127.5f) - 1.0f;
    f[3] = __fdiv_rn(1.0f, 127.5f) - 1.0f;
    f[4] = f[5] = f[6] = f[7] = 0.f;
  }
};

// ---- depthwise 3x3 ---------------------------------------------------------------------------------------------------------------
constexpr int DW_ROWS = 8;  // output rows per strip

template <int DT>
__device__ __forceinline__ void dw_load3(const u16* __restrict__ xi, int iy, int ix0, int h, int w, int c, int cg, float v[3][8]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int ix = ix0 + k;
    if (iy >= 0 && iy < h && ix >= 0 && ix < w) {
      unpack8<DT>(ld16(xi + ((int64_t)iy * w + ix) * c + cg * 8), v[k]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[k][e] = 0.f;
    }
  }
}

// the horizontal sum of kernel row ky over the three loaded columns
__device__ __forceinline__ void dw_hsum(const float wk[9][8], int ky, const float v[3][8], float out[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) out[e] = fmaf(wk[ky * 3 + 2][e], v[2][e], fmaf(wk[ky * 3 + 1][e], v[1][e], wk[ky * 3][e] * v[0][e]));
}

template <int DT>
__device__ __forceinline__ void dw_store(u16* __restrict__ yo, int oy, int ox, int wo, int c, int cg, float a[8], int relu6) {
  if (relu6) {
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = fminf(fmaxf(a[e], 0.f), 6.f);
  }
  st16(yo + ((int64_t)oy * wo + ox) * c + cg * 8, pack8<DT>(a));
}

template <int DT, int STRIDE>
__global__ __launch_bounds__(256) void k_dwconv3x3(const u16* __restrict__ x, const u16* __restrict__ wt, const float* __restrict__ bias, u16* __restrict__ y,
                                                   int64_t total, int h, int w, int ho, int wo, int c, int strips, int relu6) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cl = c >> 3;
  const int cg = (int)(idx % cl);
  int64_t r = idx / cl;
  const int ox = (int)(r % wo);
  r /= wo;
  const int strip = (int)(r % strips);
  const int64_t img = r / strips;
  const u16* xi = x + img * h * w * c;
  u16* yo = y + img * ho * wo * c;
  float wk[9][8], b8[8];
#pragma unroll
  for (int t = 0; t < 9; ++t) unpack8<DT>(ld16(wt + (int64_t)t * c + cg * 8), wk[t]);
#pragma unroll
  for (int e = 0; e < 8; ++e) b8[e] = bias[cg * 8 + e];
  const int oy0 = strip * DW_ROWS, oy1 = oy0 + DW_ROWS < ho ? oy0 + DW_ROWS : ho;
  float v[3][8], hs[8];
  if (STRIDE == 1) {
    // a0: output row iy - 1 (waits for kernel row 2), a1: output row iy (waits for kernel rows 1 and 2)
    float a0[8], a1[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) a0[e] = a1[e] = b8[e];
    for (int iy = oy0 - 1; iy <= oy1; ++iy) {
      dw_load3<DT>(xi, iy, ox - 1, h, w, c, cg, v);
      dw_hsum(wk, 2, v, hs);
#pragma unroll
      for (int e = 0; e < 8; ++e) a0[e] += hs[e];
      if (iy - 1 >= oy0) dw_store<DT>(yo, iy - 1, ox, wo, c, cg, a0, relu6);
      dw_hsum(wk, 1, v, hs);
#pragma unroll
      for (int e = 0; e < 8; ++e) a0[e] = a1[e] + hs[e];
      dw_hsum(wk, 0, v, hs);
#pragma unroll
      for (int e = 0; e < 8; ++e) a1[e] = b8[e] + hs[e];
    }
  } else {
    // output row oy reads input rows 2 oy, 2 oy + 1, 2 oy + 2; the last is the first of the next output row
    float a[8];
    dw_load3<DT>(xi, 2 * oy0, 2 * ox, h, w, c, cg, v);
    dw_hsum(wk, 0, v, hs);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = b8[e] + hs[e];
    for (int oy = oy0; oy < oy1; ++oy) {
      dw_load3<DT>(xi, 2 * oy + 1, 2 * ox, h, w, c, cg, v);
      dw_hsum(wk, 1, v, hs);
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] += hs[e];
      dw_load3<DT>(xi, 2 * oy + 2, 2 * ox, h, w, c, cg, v);
      dw_hsum(wk, 2, v, hs);
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] += hs[e];
      dw_store<DT>(yo, oy, ox, wo, c, cg, a, relu6);
      dw_hsum(wk, 0, v, hs);
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] = b8[e] + hs[e];
    }
  }
}

// ---- bilinear x2, align_corners --------------------------------------------------------------------------------------------------
// src = dst * (in - 1) / (out - 1): the integer product is exact and the division correctly rounded, so the last sample is exactly in - 1
__device__ __forceinline__ void ac_coord(int d, int in, int out, int& i0, int& i1, float& f) {
  const float s = out > 1 ? __fdiv_rn((float)(d * (in - 1)), (float)(out - 1)) : 0.f;
  i0 = (int)s;
  i0 = i0 > in - 1 ? in - 1 : i0;
  i1 = i0 + 1 < in ? i0 + 1 : in - 1;
  f = s - (float)i0;
}

template <int DT>
__global__ __launch_bounds__(256) void k_up2_ac(const u16* __restrict__ x, u16* __restrict__ y, int64_t total, int h, int w, int c, int64_t ld, int col0) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cl = c >> 3;
  const int cg = (int)(idx % cl);
  const int64_t op = idx / cl;
  const int ox = (int)(op % (2 * w));
  const int oy = (int)((op / (2 * w)) % (2 * h));
  const int64_t img = op / ((int64_t)4 * h * w);
  int y0, y1, x0, x1;
  float fy, fx;
  ac_coord(oy, h, 2 * h, y0, y1, fy);
  ac_coord(ox, w, 2 * w, x0, x1, fx);
  const u16* xi = x + img * h * w * c + cg * 8;
  float a[8], b[8], cc[8], d[8], o[8];
  unpack8<DT>(ld16(xi + ((int64_t)y0 * w + x0) * c), a);
  unpack8<DT>(ld16(xi + ((int64_t)y0 * w + x1) * c), b);
  unpack8<DT>(ld16(xi + ((int64_t)y1 * w + x0) * c), cc);
  unpack8<DT>(ld16(xi + ((int64_t)y1 * w + x1) * c), d);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float top = a[e] * (1.0f - fx) + b[e] * fx;
    const float bot = cc[e] * (1.0f - fx) + d[e] * fx;
    o[e] = top * (1.0f - fy) + bot * fy;
  }
  st16(y + op * ld + col0 + cg * 8, pack8<DT>(o));
}

// ---- dilated 3x3 convolution, 64 -> 64 ---------------------------------------------------------------------------------------------
constexpr int DL_T = 16, DL_D = 5, DL_IN = DL_T + 2 * DL_D, DL_PIX = 40;  // u16 per pixel in LDS: 32 channels + 8 of padding

template <int DT>
__global__ __launch_bounds__(256) void k_conv3x3_dil(const u16* __restrict__ x, const u16* __restrict__ wt, const float* __restrict__ bias, u16* __restrict__ y,
                                                     int h, int w, int tiles_x, int tiles_y, int relu) {
  __shared__ __attribute__((aligned(16))) u16 tile[DL_IN * DL_IN * DL_PIX];
  const int bx = blockIdx.x % tiles_x;
  const int by = (blockIdx.x / tiles_x) % tiles_y;
  const int img = blockIdx.x / (tiles_x * tiles_y);
  const int y0 = by * DL_T, x0 = bx * DL_T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, r16 = lane & 15;
  const u16* xi = x + (int64_t)img * h * w * 64;
  f32x4 acc[4][4];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[rr][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int half = 0; half < 2; ++half) {
    if (half) __syncthreads();
    for (int i = threadIdx.x; i < DL_IN * DL_IN * 4; i += 256) {
      const int pix = i >> 2, part = i & 3;
      const int r = pix / DL_IN, cc = pix - r * DL_IN;
      const int gy = y0 - DL_D + r, gx = x0 - DL_D + cc;
      u32x4 v = (u32x4){0u, 0u, 0u, 0u};
      if (gy >= 0 && gy < h && gx >= 0 && gx < w) v = ld16(xi + ((int64_t)gy * w + gx) * 64 + half * 32 + part * 8);
      st16(tile + pix * DL_PIX + part * 8, v);
    }
    __syncthreads();
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - ky * 3;
      u32x4 wf[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) wf[t] = ld16(wt + ((int64_t)(t * 16 + r16) * 9 + tap) * 64 + half * 32 + q * 8);
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int row = wave * 4 + rr;
        const u32x4 b = ld16(tile + ((row + DL_D * ky) * DL_IN + r16 + DL_D * kx) * DL_PIX + q * 8);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[rr][t] = Elem<DT>::mfma(wf[t], b, acc[rr][t]);
      }
    }
  }
  // a lane holds output channels t * 16 + q * 4 .. + 3 of pixel (wave * 4 + rr, r16)
  const int gx = x0 + r16;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int gy = y0 + wave * 4 + rr;
    if (gy < h && gx < w) {
      u16* d = y + (((int64_t)img * h + gy) * w + gx) * 64 + q * 4;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o[e] = acc[rr][t][e] + bias[t * 16 + q * 4 + e];
          if (relu) o[e] = fmaxf(o[e], 0.f);
        }
        u32x2 v;
        v[0] = pack2<DT>(o[0], o[1]);
        v[1] = pack2<DT>(o[2], o[3]);
        *(u32x2*)(d + t * 16) = v;
      }
    }
  }
}

// ---- decode ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float heat_of(float logit) { return __fdiv_rn(1.0f, 1.0f + expf(-logit)); }

// endpoint 2 * (pixel + displacement) in float64, truncated toward zero; out-of-range and NaN values are pinned (a line that far out is
// clipped away or reduced to the image's edge all the same)
__device__ __forceinline__ int endpoint(int pix, float disp) {
  const double v = 2.0 * ((double)pix + (double)disp);
  if (!(v == v)) return 0;
  if (v >= 1073741824.0) return 1073741824;
  if (v <= -1073741824.0) return -1073741824;
  return (int)v;
}

constexpr int DEC_T = 1024;  // threads of the one block per frame

__global__ __launch_bounds__(DEC_T) void k_mlsd_decode(const float* __restrict__ tp, unsigned long long* __restrict__ cand_all, int32_t* __restrict__ segments,
                                                     int32_t* __restrict__ count, int h, int w, float thr_v, float thr_d) {
  __shared__ unsigned long long sel[kTopK], sorted[kTopK];
  __shared__ int hist[256];
  __shared__ int flag[kTopK];
  __shared__ int n_cand, n_sel, s_k;
  __shared__ unsigned long long s_prefix;
  const int img = blockIdx.x, tid = threadIdx.x;
  const int hw = h * w;
  const float* t = tp + (int64_t)img * hw * 8;
  unsigned long long* cand = cand_all + (int64_t)img * hw;
  if (tid == 0) n_cand = 0, n_sel = 0;
  __syncthreads();
  // candidates: heat > thr_v and no 3x3 neighbour with a larger heat (plateaus keep every pixel; outside the map counts as -inf)
  for (int p = tid; p < hw; p += DEC_T) {
    const float lg = t[(int64_t)p * 8];
    const float ht = heat_of(lg);
    if (!(ht > thr_v)) continue;
    const int py = p / w, px = p - py * w;
    bool keep = true;
    for (int dy = -1; dy <= 1 && keep; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int yy = py + dy, xx = px + dx;
        if ((dy == 0 && dx == 0) || yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
        const float ln = t[((int64_t)yy * w + xx) * 8];
        if (ln > lg && heat_of(ln) > ht) {  // (a neighbour with a smaller logit cannot have a larger heat)
          keep = false;
          break;
        }
      }
    if (keep) {
      const int slot = atomicAdd(&n_cand, 1);  // slot < hw: at most one per pixel
      cand[slot] = ((unsigned long long)__float_as_uint(ht) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)p);
    }
  }
  __syncthreads();
  const int nc = n_cand;
  const int k = nc < kTopK ? nc : kTopK;
  // the k-th largest key (keys are distinct): 8 passes of 8 bits, most significant first
  unsigned long long thr_key = 0ull;
  if (nc > kTopK) {
    if (tid == 0) s_prefix = 0ull, s_k = kTopK;
    for (int pass = 0; pass < 8; ++pass) {
      const int shift = 56 - 8 * pass;
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      const unsigned long long prefix = s_prefix;
      for (int i = tid; i < nc; i += DEC_T) {
        const unsigned long long key = cand[i];
        if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(int)((key >> shift) & 255ull)], 1);
      }
      __syncthreads();
      if (tid == 0) {
        int need = s_k, b = 255;
        for (; b > 0; --b) {
          if (hist[b] >= need) break;
          need -= hist[b];
        }
        s_k = need;
        s_prefix = (prefix << 8) | (unsigned long long)b;
      }
      __syncthreads();
    }
    thr_key = s_prefix;
  }
  for (int i = tid; i < nc; i += DEC_T) {
    const unsigned long long key = cand[i];
    if (key >= thr_key) {
      const int slot = atomicAdd(&n_sel, 1);
      if (slot < kTopK) sel[slot] = key;
    }
  }
  __syncthreads();
  // rank order: score descending, index ascending
  if (tid < k) {
    const unsigned long long mine = sel[tid];
    int rank = 0;
    for (int j = 0; j < k; ++j) rank += sel[j] > mine ? 1 : 0;
    sorted[rank] = mine;
  }
  __syncthreads();
  int seg[4] = {0, 0, 0, 0};
  int live = 0;
  if (tid < k) {
    const int p = (int)(0xFFFFFFFFu - (unsigned)(sorted[tid] & 0xFFFFFFFFull));
    const int py = p / w, px = p - py * w;
    const float* d = t + (int64_t)p * 8;
    const float dxs = d[1], dys = d[2], dxe = d[3], dye = d[4];
    const float ex = dxs - dxe, ey = dys - dye;
    const float dist = sqrtf(ex * ex + ey * ey);
    live = dist > thr_d ? 1 : 0;
    seg[0] = endpoint(px, dxs), seg[1] = endpoint(py, dys), seg[2] = endpoint(px, dxe), seg[3] = endpoint(py, dye);
  }
  if (tid < kTopK) flag[tid] = live;
  __syncthreads();
  int32_t* so = segments + (int64_t)img * kTopK * 4;
  if (tid < kTopK) {
    int pos = 0, total = 0;
    for (int j = 0; j < kTopK; ++j) {
      pos += (j < tid) ? flag[j] : 0;
      total += flag[j];
    }
    if (live) {
#pragma unroll
      for (int e = 0; e < 4; ++e) so[pos * 4 + e] = seg[e];
    }
    if (tid >= total) {  // the unused tail is zero: the buffer is a function of the input alone
#pragma unroll
      for (int e = 0; e < 4; ++e) so[tid * 4 + e] = 0;
    }
    if (tid == 0) count[img] = total;
  }
}

// ---- draw ------------------------------------------------------------------------------------------------------------------------
// cv2.line(map, pt1, pt2, 255, 1): clipLine, then LineIterator(connectivity 8, left to right)
__global__ __launch_bounds__(256) void k_mlsd_draw(const int32_t* __restrict__ segments, const int32_t* __restrict__ count, uint8_t* __restrict__ map, int images,
                                                   int h, int w) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= images * kTopK) return;
  const int img = idx / kTopK, s = idx - img * kTopK;
  int n = count[img];
  n = n < 0 ? 0 : (n > kTopK ? kTopK : n);
  if (s >= n) return;
  const int32_t* sg = segments + (int64_t)idx * 4;
  uint8_t* m = map + (int64_t)img * h * w;
  cv_line8(h, w, sg[0], sg[1], sg[2], sg[3], [m, w](long long px, long long py) { m[py * w + px] = 255; });
}

template <typename T>
__global__ __launch_bounds__(256) void k_mlsd_emit(const uint8_t* __restrict__ map, T* __restrict__ ctrl, int images, int64_t hw, int rep) {
  const int64_t g0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (g0 >= images * hw) return;
  const int img = (int)(g0 / hw);
  const int64_t p = g0 - img * hw;
  const uint32_t four = *(const uint32_t*)(map + g0);
  int level[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) level[i] = (int)((four >> (8 * i)) & 255u);
  emit_control4(ctrl, images, img, hw, p, rep, level);
}

}  // namespace

extern "C" int ca_mlsd_prep(const uint8_t* src, void* dst, int32_t images, int32_t h, int32_t w, int32_t dtype, void* stream) {
  return launch_rgb8_prep("ca_mlsd_prep", "src and dst", src && dst, src, dst, images, h, w, dtype, true, "dst must be 16-byte aligned", stream, MlsdFill{});
}

extern "C" int ca_dwconv3x3(const void* x, const void* wt, const float* bias, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t stride,
                            int32_t relu6, int32_t dtype, void* stream) {
  CA_REQUIRE(x && wt && bias && y, "ca_dwconv3x3: x, wt, bias and y are required");
  CA_REQUIRE(sizes_ok(images, h, w), "ca_dwconv3x3: images=%d h=%d w=%d (each >= 1, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE(c >= 16 && c <= 576 && c % 8 == 0, "ca_dwconv3x3: c=%d must be a multiple of 8 in 16 .. 576", c);
  CA_REQUIRE(stride == 1 || stride == 2, "ca_dwconv3x3: stride=%d (1 or 2)", stride);
  CA_REQUIRE(stride == 1 || (h % 2 == 0 && w % 2 == 0), "ca_dwconv3x3: stride 2 needs even h and w, got %d x %d", h, w);
  CA_REQUIRE(relu6 == 0 || relu6 == 1, "ca_dwconv3x3: relu6=%d (0 or 1)", relu6);
  CA_REQUIRE(dtype_ok(dtype), "ca_dwconv3x3: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)wt | (uintptr_t)y) & 15) == 0 && ((uintptr_t)bias & 3) == 0,
             "ca_dwconv3x3: x, wt and y must be 16-byte aligned, bias 4-byte aligned");
  CA_REQUIRE((int64_t)images * h * w * c <= kMaxPixels * 8, "ca_dwconv3x3: tensor too large");
  const int ho = h / stride, wo = w / stride;
  const int strips = ceil_div_i(ho, DW_ROWS);
  const int64_t total = (int64_t)images * strips * wo * (c / 8);
  CA_REQUIRE((total + 255) / 256 < ((int64_t)1 << 31), "ca_dwconv3x3: grid too large");
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define CA_DW_LAUNCH(DT, S)                                                                                                                                   \
  hipLaunchKernelGGL((k_dwconv3x3<DT, S>), grid, block, 0, st, (const u16*)x, (const u16*)wt, bias, (u16*)y, total, (int)h, (int)w, ho, wo, (int)c, strips, \
                     (int)relu6)
  CA_DISPATCH_DT(dtype, if (stride == 1) CA_DW_LAUNCH(DT, 1);
    else CA_DW_LAUNCH(DT, 2));
#undef CA_DW_LAUNCH
  CA_CHECK_LAUNCH("ca_dwconv3x3");
  return CA_OK;
}

extern "C" int ca_upsample2x_bilinear_ac(const void* x, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int64_t ld, int32_t col0, int32_t dtype,
                                         void* stream) {
  CA_REQUIRE(x && y, "ca_upsample2x_bilinear_ac: x and y are required");
  CA_REQUIRE(sizes_ok(images, h, w, 4), "ca_upsample2x_bilinear_ac: images=%d h=%d w=%d (each >= 1, images * 2 h * 2 w < 2^31)", images, h, w);
  CA_REQUIRE(c >= 8 && c % 8 == 0 && c <= 1024, "ca_upsample2x_bilinear_ac: c=%d must be a multiple of 8 in 8 .. 1024", c);
  CA_REQUIRE(ld % 8 == 0 && col0 >= 0 && col0 % 8 == 0 && (int64_t)col0 + c <= ld, "ca_upsample2x_bilinear_ac: ld=%lld col0=%d c=%d (multiples of 8, col0 + c <= ld)",
             (long long)ld, col0, c);
  CA_REQUIRE(dtype_ok(dtype), "ca_upsample2x_bilinear_ac: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "ca_upsample2x_bilinear_ac: x and y must be 16-byte aligned");
  const int64_t total = (int64_t)images * 4 * h * w * (c / 8);
  CA_REQUIRE((total + 255) / 256 < ((int64_t)1 << 31), "ca_upsample2x_bilinear_ac: grid too large");
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_up2_ac<DT>, grid, block, 0, (hipStream_t)stream, (const u16*)x, (u16*)y, total, (int)h, (int)w, (int)c, ld, (int)col0));
  CA_CHECK_LAUNCH("ca_upsample2x_bilinear_ac");
  return CA_OK;
}

extern "C" int ca_conv3x3_dil(const void* x, const void* wt, const float* bias, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t dilation,
                              int32_t relu, int32_t dtype, void* stream) {
  CA_REQUIRE(x && wt && bias && y, "ca_conv3x3_dil: x, wt, bias and y are required");
  CA_REQUIRE(sizes_ok(images, h, w), "ca_conv3x3_dil: images=%d h=%d w=%d (each >= 1, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE(c == 64 && dilation == DL_D, "ca_conv3x3_dil: c=%d dilation=%d (cin = cout = 64 and dilation = padding = 5 are what the kernel is built for)", c,
             dilation);
  CA_REQUIRE(relu == 0 || relu == 1, "ca_conv3x3_dil: relu=%d (0 or 1)", relu);
  CA_REQUIRE(dtype_ok(dtype), "ca_conv3x3_dil: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)wt | (uintptr_t)y) & 15) == 0 && ((uintptr_t)bias & 3) == 0,
             "ca_conv3x3_dil: x, wt and y must be 16-byte aligned, bias 4-byte aligned");
  CA_REQUIRE(x != y, "ca_conv3x3_dil: y must not be x");
  const int tx = ceil_div_i(w, DL_T), ty = ceil_div_i(h, DL_T);
  const int64_t blocks = (int64_t)images * tx * ty;
  CA_REQUIRE(blocks < ((int64_t)1 << 31), "ca_conv3x3_dil: grid too large");
  const dim3 grid((unsigned)blocks), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_conv3x3_dil<DT>, grid, block, 0, (hipStream_t)stream, (const u16*)x, (const u16*)wt, bias, (u16*)y, (int)h, (int)w, tx, ty, (int)relu));
  CA_CHECK_LAUNCH("ca_conv3x3_dil");
  return CA_OK;
}

extern "C" int64_t ca_mlsd_decode_workspace_bytes(int32_t images, int32_t h, int32_t w) {
  if (!sizes_ok(images, h, w)) return 0;
  return (int64_t)images * h * w * 8;
}

extern "C" int ca_mlsd_decode(const float* tp, int32_t images, int32_t h, int32_t w, float thr_v, float thr_d, void* workspace, int64_t workspace_bytes,
                              int32_t* segments, int32_t* count, void* stream) {
  CA_REQUIRE(tp && workspace && segments && count, "ca_mlsd_decode: tp, workspace, segments and count are required");
  CA_REQUIRE(sizes_ok(images, h, w), "ca_mlsd_decode: images=%d h=%d w=%d (each >= 1, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE(thr_v >= 0.f && thr_v < 1.f && thr_d >= 0.f && thr_d < 3.0e38f, "ca_mlsd_decode: thr_v=%g (0 <= thr_v < 1) thr_d=%g (finite, >= 0)", (double)thr_v,
             (double)thr_d);
  CA_REQUIRE(workspace_bytes >= ca_mlsd_decode_workspace_bytes(images, h, w), "ca_mlsd_decode: the workspace holds %lld bytes, %lld are needed",
             (long long)workspace_bytes, (long long)ca_mlsd_decode_workspace_bytes(images, h, w));
  CA_REQUIRE(((uintptr_t)tp & 15) == 0 && ((uintptr_t)workspace & 7) == 0 && (((uintptr_t)segments | (uintptr_t)count) & 3) == 0,
             "ca_mlsd_decode: tp must be 16-byte aligned, the workspace 8-byte aligned, segments and count 4-byte aligned");
  hipLaunchKernelGGL(k_mlsd_decode, dim3((unsigned)images), dim3(DEC_T), 0, (hipStream_t)stream, tp, (unsigned long long*)workspace, segments, count, (int)h, (int)w,
                     thr_v, thr_d);
  CA_CHECK_LAUNCH("ca_mlsd_decode");
  return CA_OK;
}

extern "C" int ca_mlsd_draw(const int32_t* segments, const int32_t* count, int32_t images, int32_t h, int32_t w, uint8_t* map, void* control, int32_t rep,
                            int32_t control_dtype, void* stream) {
  CA_REQUIRE(segments && count && map, "ca_mlsd_draw: segments, count and map are required");
  CA_REQUIRE(sizes_ok(images, h, w), "ca_mlsd_draw: images=%d h=%d w=%d (each >= 1, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE((int64_t)images * kTopK < kMaxPixels, "ca_mlsd_draw: too many images");
  if (const int rc = control_out_checks("ca_mlsd_draw", true, h, w, nullptr, true, rep, control_dtype)) return rc;  // (the map is required above)
  CA_REQUIRE((((uintptr_t)segments | (uintptr_t)count | (uintptr_t)map) & 3) == 0 && ctrl_aligned(control, control_dtype, 4),
             "ca_mlsd_draw: segments, count and map must be 4-byte aligned, control aligned to four of its elements");
  hipStream_t st = (hipStream_t)stream;
  const int64_t hw = (int64_t)h * w, total = (int64_t)images * hw;
  if (hipMemsetAsync(map, 0, (size_t)total, st) != hipSuccess) {
    (void)hipGetLastError();
    CA_FAIL(CA_ERR_LAUNCH, "ca_mlsd_draw: clearing the map failed");
  }
  hipLaunchKernelGGL(k_mlsd_draw, dim3((unsigned)((images * kTopK + 255) / 256)), dim3(256), 0, st, segments, count, map, (int)images, (int)h, (int)w);
  CA_CHECK_LAUNCH("ca_mlsd_draw");
  if (control) {
    const dim3 grid((unsigned)((total / 4 + 255) / 256)), block(256);
    CA_DISPATCH_CTRL(control_dtype, hipLaunchKernelGGL(k_mlsd_emit<T>, grid, block, 0, st, (const uint8_t*)map, (T*)control, (int)images, hw, (int)rep));
    CA_CHECK_LAUNCH("ca_mlsd_draw");
  }
  return CA_OK;
}
