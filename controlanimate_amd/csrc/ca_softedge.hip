// Added to ABI v16: the stages of the softedge (PiDiNet) annotator that ca_conv3x3 / ca_gemm do not cover (controlanimate_amd/softedge.py:
// SoftedgeAnnotator; the specification is tests/softedge_ref.py, restated from the published PiDiNet(60, carv4, dil = 24, sa = True) and
// PidiNetDetector).  The 3 -> 64 init_block runs on ca_conv3x3 (the pixel-difference operator folded into a plain 3x3 weight on the
// host), every 1x1 convolution on ca_gemm; around them:
//
//   prep      SeFill           uint8 RGB [n,H,W,3] -> [n,H,W,8]: x / 255 in channels 0..2, zeros in 3..7
//   dw        k_dwconv_k       depthwise 3x3 / 5x5 (the folded cd / ad / cv and rd operators), stride 1, no bias, optional ReLU.  As
//                              k_dwconv3x3 a thread owns 8 (5x5: 4) channels of one output column and walks down a strip of output rows; the KS
//                              output rows in flight rotate through registers, so an input row of the strip is read once.  The sum of one
//                              output is fixed: kernel rows ascending, inside a row w0 * v0, then fma over the columns ascending
//   pool      k_maxpool2x2     2x2 / stride-2 maximum
//   block     k_pdc_block      y = x + W2 . relu(dw_k(x)) at C = 64 in ONE pass: a block owns 16 x 16 pixels and keeps their halo tile
//                              ((16 + 2p)^2 pixels, 144 bytes each: 128 of channels + 16 of padding, so that the sixteen pixels a
//                              quarter-wave reads fall into sixteen different 16-byte bank groups) and the depthwise taps in LDS
//                              (60.8 KB at 5x5: two blocks per CU).  A lane owns one column of four rows: it forms the depthwise sum
//                              of 8 channels in fp32 -- the SAME operation order as k_dwconv_k --, applies the ReLU, rounds once and
//                              holds exactly the B fragment (pixel = lane & 15, k = 8 (lane >> 4) ..) of the 16x16x32 MFMA whose A
//                              operand is W2 (64 x 64, in registers for the whole block).  A's rows are permuted (row 4 q + e of
//                              MFMA t is output channel 16 q + 4 t + e) so that a lane ends with 16 consecutive output channels of
//                              its pixel: the product is rounded to the activation type (where ca_gemm's residual epilogue, and an fp16
//                              torch pipeline, round it), x comes back from the LDS tile, is added in fp32, and the sum leaves as two
//                              16-byte stores
//   relu      k_se_relu        max(x, 0): the ReLU in FRONT of a CDCM's 1x1 convolution (not an epilogue of anything)
//   cdcm      k_cdcm_dil4      the four dilated 3x3 convolutions (5, 7, 9, 11) of a CDCM summed in one MFMA accumulation, K = 4 * 9 * 32;
//                              the B operand is read straight from global memory (a quarter-wave's sixteen pixels are 1 KB
//                              contiguous; a 38 x 38 halo tile would not fit two blocks into LDS), zero outside the image; taps that
//                              miss the whole map for a block are skipped
//   csam      k_csam_a / _b    t = b1 + W1 relu(f) (4 channels) and r = wr . f per pixel, then side = br + sigmoid(conv3x3(t)) * r
//   fuse      k_se_fuse        the four side maps sampled bilinearly (align_corners = False), the 1x1 classifier, the fp32 sigmoid, the
//                              optional safe step, x 255, truncation -> uint8 map and / or the control tensor (ca_annot.h)
//
// Compiled with -ffp-contract=off: the depthwise sums of k_dwconv_k and k_pdc_block then are the same operations, and the bilinear
// sample and the classifier round as written.  No atomics; no launch depends on device data on the host side.
#include "ca_common.h"
#include "ca_annot.h"

namespace {

// ---- prep ------------------------------------------------------------------------------------------------------------------------
struct SeFill {
  __device__ __forceinline__ void operator()(const uint8_t* s, float f[8]) const {
#pragma unroll
    for (int c = 0; c < 3; ++c) f[c] = __fdiv_rn((float)s[c], 255.0f);
    f[3] = f[4] = f[5] = f[6] = f[7] = 0.f;
  }
};

// ---- ReLU ------------------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void k_se_relu(const u16* __restrict__ x, u16* __restrict__ y, int64_t groups) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= groups) return;
  float f[8];
  unpack8<DT>(ld16(x + i * 8), f);
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = fmaxf(f[e], 0.f);
  st16(y + i * 8, pack8<DT>(f));  // (exact: every value is an input or zero)
}

// ---- the depthwise sum, shared by k_dwconv_k and k_pdc_block ------------------------------------------------------------------------
// kernel row: hs = w0 * v0, then hs = fma(w_kx, v_kx, hs) for kx = 1 .. KS - 1
template <int N = 8>
__device__ __forceinline__ void dk_tap(int kx, const float* wf, const float* v, float* hs) {
#pragma unroll
  for (int e = 0; e < N; ++e) hs[e] = kx == 0 ? wf[e] * v[e] : fmaf(wf[e], v[e], hs[e]);
}

// CH (8 or 4) consecutive channels <-> CH / 2 registers
template <int DT, int CH>
struct Chan {
  unsigned r[CH / 2];
  __device__ __forceinline__ void load(const u16* p) {
    if (CH == 8) {
      const u32x4 v = ld16(p);
#pragma unroll
      for (int i = 0; i < CH / 2; ++i) r[i] = v[i];
    } else {
      const u32x2 v = *reinterpret_cast<const u32x2*>(p);
#pragma unroll
      for (int i = 0; i < CH / 2; ++i) r[i] = v[i];
    }
  }
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < CH / 2; ++i) r[i] = 0u;
  }
  __device__ __forceinline__ void unpack(float* f) const {
#pragma unroll
    for (int i = 0; i < CH / 2; ++i) {
      f[2 * i] = Elem<DT>::to_f((u16)(r[i] & 0xffffu));
      f[2 * i + 1] = Elem<DT>::to_f((u16)(r[i] >> 16));
    }
  }
  static __device__ __forceinline__ void store(u16* p, const float* f) {
    if (CH == 8) {
      st16(p, pack8<DT>(f));
    } else {
      u32x2 v;
      v[0] = pack2<DT>(f[0], f[1]);
      v[1] = pack2<DT>(f[2], f[3]);
      *reinterpret_cast<u32x2*>(p) = v;
    }
  }
};

// ---- depthwise KS x KS -------------------------------------------------------------------------------------------------------------
// 3x3: 8 channels per thread, strips of 8 output rows.  5x5: 4 channels per thread (25 packed taps, five rows of sums and five columns
// of input for 8 channels need all 256 registers: one wave per SIMD, 0.7 TB/s; with 4 it is 8-byte accesses at four times the
// occupancy), strips of 16 output rows (20 input rows read per 16 written instead of 12 per 8).
template <int KS>
struct DkShape {
  static constexpr int CH = KS == 5 ? 4 : 8;
  static constexpr int ROWS = KS == 5 ? 16 : 8;
};

template <int DT, int KS>
__global__ __launch_bounds__(256) void k_dwconv_k(const u16* __restrict__ x, const u16* __restrict__ wt, u16* __restrict__ y, int64_t total, int h, int w, int c,
                                                  int strips, int relu) {
  constexpr int P = KS / 2, CH = DkShape<KS>::CH, ROWS = DkShape<KS>::ROWS;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cl = c / CH;
  const int cg = (int)(idx % cl);
  int64_t r = idx / cl;
  const int ox = (int)(r % w);
  r /= w;
  const int strip = (int)(r % strips);
  const int64_t img = r / strips;
  const u16* xi = x + img * h * w * c + cg * CH;
  u16* yo = y + img * h * w * c + cg * CH;
  Chan<DT, CH> wk[KS * KS];  // the taps stay packed
#pragma unroll
  for (int t = 0; t < KS * KS; ++t) wk[t].load(wt + (int64_t)t * c + cg * CH);
  const int oy0 = strip * ROWS, oy1 = oy0 + ROWS < h ? oy0 + ROWS : h;
  // a[j]: output row iy - P + j, which input row iy reaches through kernel row KS - 1 - j
  float a[KS][CH];
#pragma unroll
  for (int j = 0; j < KS; ++j)
#pragma unroll
    for (int e = 0; e < CH; ++e) a[j][e] = 0.f;
  for (int iy = oy0 - P; iy <= oy1 - 1 + P; ++iy) {
    float v[KS][CH];
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      const int ix = ox - P + k;
      Chan<DT, CH> in;
      if (iy >= 0 && iy < h && ix >= 0 && ix < w) in.load(xi + ((int64_t)iy * w + ix) * c);
      else in.zero();
      in.unpack(v[k]);
    }
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      const int ky = KS - 1 - j;
      float hs[CH], wf[CH];
#pragma unroll
      for (int kx = 0; kx < KS; ++kx) {
        wk[ky * KS + kx].unpack(wf);
        dk_tap<CH>(kx, wf, v[kx], hs);
      }
#pragma unroll
      for (int e = 0; e < CH; ++e) a[j][e] += hs[e];
    }
    const int oy = iy - P;
    if (oy >= oy0 && oy < oy1) {
      float o[CH];
#pragma unroll
      for (int e = 0; e < CH; ++e) o[e] = relu ? fmaxf(a[0][e], 0.f) : a[0][e];
      Chan<DT, CH>::store(yo + ((int64_t)oy * w + ox) * c, o);
    }
#pragma unroll
    for (int j = 0; j + 1 < KS; ++j)
#pragma unroll
      for (int e = 0; e < CH; ++e) a[j][e] = a[j + 1][e];
#pragma unroll
    for (int e = 0; e < CH; ++e) a[KS - 1][e] = 0.f;
  }
}

// ---- max pool ----------------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void k_maxpool2x2(const u16* __restrict__ x, u16* __restrict__ y, int64_t total, int ho, int wo, int c) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cl = c >> 3;
  const int cg = (int)(idx % cl);
  const int64_t op = idx / cl;
  const int ox = (int)(op % wo);
  const int oy = (int)((op / wo) % ho);
  const int64_t img = op / ((int64_t)ho * wo);
  const int w = 2 * wo;
  const u16* p = x + ((img * (2 * ho) + 2 * oy) * w + 2 * ox) * c + cg * 8;
  float m[8], f[8];
  unpack8<DT>(ld16(p), m);
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    unpack8<DT>(ld16(p + ((int64_t)(k >> 1) * w + (k & 1)) * c), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], f[e]);
  }
  st16(y + op * c + cg * 8, pack8<DT>(m));  // (the maximum is one of the inputs: the conversion back is exact)
}

// ---- the fused block at C = 64 ---------------------------------------------------------------------------------------------------
constexpr int PB_T = 16, PB_C = 64, PB_PIX = 72;  // tile side; channels; u16 per pixel in LDS (64 channels + 8 of padding)

template <int DT, int KS>
__global__ __launch_bounds__(256) void k_pdc_block(const u16* __restrict__ x, const u16* __restrict__ wdw, const u16* __restrict__ w2, u16* __restrict__ y, int h, int w,
                                                   int tiles_x, int tiles_y) {
  constexpr int P = KS / 2, IN = PB_T + 2 * P;
  __shared__ __attribute__((aligned(16))) u16 tile[IN * IN * PB_PIX];
  __shared__ __attribute__((aligned(16))) u16 wsm[KS * KS * PB_C];
  const int bx = blockIdx.x % tiles_x;
  const int by = (blockIdx.x / tiles_x) % tiles_y;
  const int img = blockIdx.x / (tiles_x * tiles_y);
  const int y0 = by * PB_T, x0 = bx * PB_T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, r16 = lane & 15;
  const u16* xi = x + (int64_t)img * h * w * PB_C;
  for (int i = threadIdx.x; i < IN * IN * 8; i += 256) {
    const int pix = i >> 3, part = i & 7;
    const int r = pix / IN, cc = pix - r * IN;
    const int gy = y0 - P + r, gx = x0 - P + cc;
    u32x4 v = (u32x4){0u, 0u, 0u, 0u};
    if (gy >= 0 && gy < h && gx >= 0 && gx < w) v = ld16(xi + ((int64_t)gy * w + gx) * PB_C + part * 8);
    st16(tile + pix * PB_PIX + part * 8, v);
  }
  for (int i = threadIdx.x; i < KS * KS * 8; i += 256) st16(wsm + i * 8, ld16(wdw + i * 8));
  // A operand: row r16 of MFMA t is output channel 16 (r16 >> 2) + 4 t + (r16 & 3); k = 32 half + 8 q ..
  u32x4 wf[4][2];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int half = 0; half < 2; ++half) wf[t][half] = ld16(w2 + (int64_t)((r16 >> 2) * 16 + t * 4 + (r16 & 3)) * PB_C + half * 32 + q * 8);
  f32x4 acc[4][4];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[rr][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  __syncthreads();
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    float d[4][8];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
#pragma unroll
      for (int e = 0; e < 8; ++e) d[rr][e] = 0.f;
#pragma unroll
    for (int ky = 0; ky < KS; ++ky) {
      float wk[KS][8];
#pragma unroll
      for (int kx = 0; kx < KS; ++kx) unpack8<DT>(ld16(wsm + (ky * KS + kx) * PB_C + half * 32 + q * 8), wk[kx]);
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const u16* row = tile + ((wave * 4 + rr + ky) * IN + r16) * PB_PIX + half * 32 + q * 8;  // output row r reads tile rows r .. r + KS - 1
        float hs[8], v[8];
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
          unpack8<DT>(ld16(row + kx * PB_PIX), v);
          dk_tap<8>(kx, wk[kx], v, hs);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) d[rr][e] += hs[e];
      }
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
#pragma unroll
      for (int e = 0; e < 8; ++e) d[rr][e] = fmaxf(d[rr][e], 0.f);
      const u32x4 b = pack8<DT>(d[rr]);  // rounded once, where the two-launch form stores it
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[rr][t] = Elem<DT>::mfma(wf[t][half], b, acc[rr][t]);
    }
  }
  // a lane holds output channels 16 q + 4 t + e of pixel (wave * 4 + rr, r16)
  const int gx = x0 + r16;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int gy = y0 + wave * 4 + rr;
    if (gy < h && gx < w) {
      const u16* res = tile + ((wave * 4 + rr + P) * IN + r16 + P) * PB_PIX + q * 16;
      u16* dst = y + (((int64_t)img * h + gy) * w + gx) * PB_C + q * 16;
#pragma unroll
      for (int hv = 0; hv < 2; ++hv) {
        float xr[8], o[8];
        unpack8<DT>(ld16(res + hv * 8), xr);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = Elem<DT>::to_f(Elem<DT>::from_f(acc[rr][hv * 2 + (e >> 2)][e & 3])) + xr[e];  // rounded, then the skip: ca_gemm's residual epilogue
        st16(dst + hv * 8, pack8<DT>(o));
      }
    }
  }
}

// ---- CDCM: four dilated 3x3 convolutions, summed ---------------------------------------------------------------------------------
constexpr int CD_T = 16, CD_C = 32;

template <int DT>
__global__ __launch_bounds__(256) void k_cdcm_dil4(const u16* __restrict__ x, const u16* __restrict__ wt, u16* __restrict__ y, int h, int w, int tiles_x, int tiles_y) {
  const int bx = blockIdx.x % tiles_x;
  const int by = (blockIdx.x / tiles_x) % tiles_y;
  const int img = blockIdx.x / (tiles_x * tiles_y);
  const int y0 = by * CD_T, x0 = bx * CD_T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, r16 = lane & 15;
  const u16* xi = x + (int64_t)img * h * w * CD_C + q * 8;
  f32x4 acc[4][2];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr)
#pragma unroll
    for (int t = 0; t < 2; ++t) acc[rr][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int di = 0; di < 4; ++di) {
    const int dil = 5 + 2 * di;
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - ky * 3;
      const int oy = dil * (ky - 1), ox = dil * (kx - 1);
      if (y0 + oy + CD_T <= 0 || y0 + oy >= h || x0 + ox + CD_T <= 0 || x0 + ox >= w) continue;  // (block-uniform) the tap misses the map
      u32x4 wf[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) wf[t] = ld16(wt + ((int64_t)((di * CD_C + t * 16 + r16) * 9 + tap)) * CD_C + q * 8);
      const int gx = x0 + r16 + ox;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int gy = y0 + wave * 4 + rr + oy;
        u32x4 b = (u32x4){0u, 0u, 0u, 0u};
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) b = ld16(xi + ((int64_t)gy * w + gx) * CD_C);
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[rr][t] = Elem<DT>::mfma(wf[t], b, acc[rr][t]);
      }
    }
  }
  // a lane holds output channels t * 16 + q * 4 .. + 3 of pixel (wave * 4 + rr, r16)
  const int gx = x0 + r16;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int gy = y0 + wave * 4 + rr;
    if (gy < h && gx < w) {
      u16* d = y + (((int64_t)img * h + gy) * w + gx) * CD_C + q * 4;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        u32x2 v;
        v[0] = pack2<DT>(acc[rr][t][0], acc[rr][t][1]);
        v[1] = pack2<DT>(acc[rr][t][2], acc[rr][t][3]);
        *(u32x2*)(d + t * 16) = v;
      }
    }
  }
}

// ---- CSAM + conv_reduce ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sigmoid_f(float z) { return __fdiv_rn(1.0f, 1.0f + expf(-z)); }

template <int DT>
__global__ __launch_bounds__(256) void k_csam_a(const u16* __restrict__ f, const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ wr,
                                                float* __restrict__ t, float* __restrict__ r, int64_t pixels) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= pixels) return;
  float t4[4] = {b1[0], b1[1], b1[2], b1[3]};
  float rs = 0.f;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    float v[8];
    unpack8<DT>(ld16(f + p * CD_C + g * 8), v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = g * 8 + e;
      rs = fmaf(wr[c], v[e], rs);
      const float pos = fmaxf(v[e], 0.f);
#pragma unroll
      for (int j = 0; j < 4; ++j) t4[j] = fmaf(w1[j * CD_C + c], pos, t4[j]);
    }
  }
  *(f32x4*)(t + p * 4) = (f32x4){t4[0], t4[1], t4[2], t4[3]};
  r[p] = rs;
}

__global__ __launch_bounds__(256) void k_csam_b(const float* __restrict__ t, const float* __restrict__ r, const float* __restrict__ w2, const float* __restrict__ br,
                                                float* __restrict__ side, int64_t pixels, int h, int w) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= pixels) return;
  const int px = (int)(p % w);
  const int py = (int)((p / w) % h);
  float s = 0.f;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int yy = py + ky - 1, xx = px + kx - 1;
      if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
      const f32x4 v = *(const f32x4*)(t + (p + (int64_t)(ky - 1) * w + (kx - 1)) * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) s = fmaf(w2[(ky * 3 + kx) * 4 + j], v[j], s);
    }
  side[p] = br[0] + sigmoid_f(s) * r[p];
}

// ---- resize, classifier, sigmoid, quantise -----------------------------------------------------------------------------------------
// F.interpolate(mode = "bilinear", align_corners = False) from in = out >> k at destination index d of one axis:
// src = max((d + 0.5) * in / out - 0.5, 0), i0 = trunc(src), i1 = min(i0 + 1, in - 1), l1 = src - i0, l0 = 1 - l1
__device__ __forceinline__ void se_coord(int d, int k, int in, int& i0, int& i1, float& l0, float& l1) {
  float s = ((float)d + 0.5f) * (1.0f / (float)(1 << k)) - 0.5f;  // exact: a dyadic scale
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  i0 = i0 > in - 1 ? in - 1 : i0;
  i1 = i0 + 1 < in ? i0 + 1 : in - 1;
  l1 = s - (float)i0;
  l0 = 1.0f - l1;
}

struct SeSides {
  const float* s[4];
};

// 4 consecutive pixels of one row per thread (w % 8 == 0)
template <typename T>
__global__ __launch_bounds__(256) void k_se_fuse(SeSides sd, const float* __restrict__ cls, float* __restrict__ logit, uint8_t* __restrict__ edges, T* __restrict__ ctrl,
                                                 int images, int h, int w, int rep, int safe) {
  const int64_t hw = (int64_t)h * w;
  const int64_t g0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (g0 >= images * hw) return;
  const int img = (int)(g0 / hw);
  const int64_t p = g0 - img * hw;
  const int y = (int)(p / w), x0 = (int)(p - (int64_t)y * w);
  float z[4];
  {
    const f32x4 v = *(const f32x4*)(sd.s[0] + g0);  // level 0 has the output's size: the sample is the value
    const float cb = cls[4], c0 = cls[0];
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = __fadd_rn(cb, __fmul_rn(c0, v[i]));
  }
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    const int hs = h >> k, ws = w >> k;
    const float* base = sd.s[k] + (int64_t)img * hs * ws;
    const float ck = cls[k];
    int ya, yb;
    float ly0, ly1;
    se_coord(y, k, hs, ya, yb, ly0, ly1);
    const float* ra = base + (int64_t)ya * ws;
    const float* rb = base + (int64_t)yb * ws;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int xa, xb;
      float lx0, lx1;
      se_coord(x0 + i, k, ws, xa, xb, lx0, lx1);
      const float top = __fadd_rn(__fmul_rn(lx0, ra[xa]), __fmul_rn(lx1, ra[xb]));  // columns first,
      const float bot = __fadd_rn(__fmul_rn(lx0, rb[xa]), __fmul_rn(lx1, rb[xb]));
      const float v = __fadd_rn(__fmul_rn(ly0, top), __fmul_rn(ly1, bot));            // then rows
      z[i] = __fadd_rn(z[i], __fmul_rn(ck, v));
    }
  }
  if (logit) *(f32x4*)(logit + g0) = (f32x4){z[0], z[1], z[2], z[3]};
  if (!edges && !ctrl) return;
  int level[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float e = sigmoid_f(z[i]);
    if (safe) e = __fdiv_rn(truncf(__fmul_rn(e, 3.0f)), 2.0f);
    e = __fmul_rn(e, 255.0f);
    e = e < 0.f ? 0.f : (e > 255.f ? 255.f : e);
    level[i] = (int)e;  // truncation, as astype(uint8) of a value in [0, 255]
  }
  if (edges) *(uint32_t*)(edges + g0) = pack_levels4(level);
  if (ctrl) emit_control4(ctrl, images, img, hw, p, rep, level);
}

inline bool ranges_overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

}  // namespace

extern "C" int ca_softedge_prep(const uint8_t* src, void* dst, int32_t images, int32_t h, int32_t w, int32_t dtype, void* stream) {
  return launch_rgb8_prep("ca_softedge_prep", "src and dst", src && dst, src, dst, images, h, w, dtype, true, "dst must be 16-byte aligned", stream, SeFill{});
}

extern "C" int ca_relu(const void* x, void* y, int64_t numel, int32_t dtype, void* stream) {
  CA_REQUIRE(x && y, "ca_relu: x and y are required");
  CA_REQUIRE(numel >= 8 && numel % 8 == 0 && numel <= kMaxPixels * 256, "ca_relu: numel=%lld must be a multiple of 8 in 8 .. 2^39", (long long)numel);
  CA_REQUIRE(dtype_ok(dtype), "ca_relu: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "ca_relu: x and y must be 16-byte aligned");
  const int64_t groups = numel / 8;
  const dim3 grid((unsigned)((groups + 255) / 256)), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_se_relu<DT>, grid, block, 0, (hipStream_t)stream, (const u16*)x, (u16*)y, groups));
  CA_CHECK_LAUNCH("ca_relu");
  return CA_OK;
}

extern "C" int ca_dwconv_k(const void* x, const void* wt, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t ksize, int32_t relu, int32_t dtype,
                           void* stream) {
  CA_REQUIRE(x && wt && y, "ca_dwconv_k: x, wt and y are required");
  CA_REQUIRE(sizes_ok(images, h, w), "ca_dwconv_k: images=%d h=%d w=%d (each >= 1, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE(c >= 8 && c <= 256 && c % 8 == 0, "ca_dwconv_k: c=%d must be a multiple of 8 in 8 .. 256", c);
  CA_REQUIRE(ksize == 3 || ksize == 5, "ca_dwconv_k: ksize=%d (3 or 5)", ksize);
  CA_REQUIRE(relu == 0 || relu == 1, "ca_dwconv_k: relu=%d (0 or 1)", relu);
  CA_REQUIRE(dtype_ok(dtype), "ca_dwconv_k: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)wt | (uintptr_t)y) & 15) == 0, "ca_dwconv_k: x, wt and y must be 16-byte aligned");
  CA_REQUIRE((int64_t)images * h * w * c <= kMaxPixels * 8, "ca_dwconv_k: tensor too large");
  const int64_t bytes = (int64_t)images * h * w * c * 2;
  CA_REQUIRE(!ranges_overlap(x, bytes, y, bytes), "ca_dwconv_k: y must not overlap x");
  const int strips = ceil_div_i(h, ksize == 3 ? DkShape<3>::ROWS : DkShape<5>::ROWS);
  const int64_t total = (int64_t)images * strips * w * (c / (ksize == 3 ? DkShape<3>::CH : DkShape<5>::CH));
  CA_REQUIRE((total + 255) / 256 < ((int64_t)1 << 31), "ca_dwconv_k: grid too large");
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define CA_DK_LAUNCH(DT, KS) \
  hipLaunchKernelGGL((k_dwconv_k<DT, KS>), grid, block, 0, st, (const u16*)x, (const u16*)wt, (u16*)y, total, (int)h, (int)w, (int)c, strips, (int)relu)
  CA_DISPATCH_DT(dtype, if (ksize == 3) CA_DK_LAUNCH(DT, 3);
    else CA_DK_LAUNCH(DT, 5));
#undef CA_DK_LAUNCH
  CA_CHECK_LAUNCH("ca_dwconv_k");
  return CA_OK;
}

extern "C" int ca_maxpool2x2(const void* x, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t dtype, void* stream) {
  CA_REQUIRE(x && y, "ca_maxpool2x2: x and y are required");
  CA_REQUIRE(sizes_ok(images, h, w), "ca_maxpool2x2: images=%d h=%d w=%d (each >= 1, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE(h % 2 == 0 && w % 2 == 0, "ca_maxpool2x2: h=%d w=%d must be even", h, w);
  CA_REQUIRE(c >= 8 && c <= 1024 && c % 8 == 0, "ca_maxpool2x2: c=%d must be a multiple of 8 in 8 .. 1024", c);
  CA_REQUIRE(dtype_ok(dtype), "ca_maxpool2x2: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "ca_maxpool2x2: x and y must be 16-byte aligned");
  CA_REQUIRE((int64_t)images * h * w * c <= kMaxPixels * 8, "ca_maxpool2x2: tensor too large");
  const int64_t total = (int64_t)images * (h / 2) * (w / 2) * (c / 8);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_maxpool2x2<DT>, grid, block, 0, (hipStream_t)stream, (const u16*)x, (u16*)y, total, h / 2, w / 2, (int)c));
  CA_CHECK_LAUNCH("ca_maxpool2x2");
  return CA_OK;
}

extern "C" int ca_pdc_block_supported(int32_t c, int32_t ksize) { return c == PB_C && (ksize == 3 || ksize == 5) ? 1 : 0; }

extern "C" int ca_pdc_block(const void* x, const void* wt_dw, const void* w2, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t ksize, int32_t dtype,
                            void* stream) {
  CA_REQUIRE(x && wt_dw && w2 && y, "ca_pdc_block: x, wt_dw, w2 and y are required");
  CA_REQUIRE(sizes_ok(images, h, w), "ca_pdc_block: images=%d h=%d w=%d (each >= 1, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE(c == PB_C, "ca_pdc_block: c=%d (64 is what the kernel is built for; other widths run as ca_dwconv_k + ca_gemm)", c);
  CA_REQUIRE(ksize == 3 || ksize == 5, "ca_pdc_block: ksize=%d (3 or 5)", ksize);
  CA_REQUIRE(dtype_ok(dtype), "ca_pdc_block: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)wt_dw | (uintptr_t)w2 | (uintptr_t)y) & 15) == 0, "ca_pdc_block: x, wt_dw, w2 and y must be 16-byte aligned");
  const int64_t bytes = (int64_t)images * h * w * c * 2;
  CA_REQUIRE(!ranges_overlap(x, bytes, y, bytes), "ca_pdc_block: y must not overlap x");
  const int tx = ceil_div_i(w, PB_T), ty = ceil_div_i(h, PB_T);
  const int64_t blocks = (int64_t)images * tx * ty;
  CA_REQUIRE(blocks < ((int64_t)1 << 31), "ca_pdc_block: grid too large");
  const dim3 grid((unsigned)blocks), block(256);
  hipStream_t st = (hipStream_t)stream;
#define CA_PB_LAUNCH(DT, KS) hipLaunchKernelGGL((k_pdc_block<DT, KS>), grid, block, 0, st, (const u16*)x, (const u16*)wt_dw, (const u16*)w2, (u16*)y, (int)h, (int)w, tx, ty)
  CA_DISPATCH_DT(dtype, if (ksize == 3) CA_PB_LAUNCH(DT, 3);
    else CA_PB_LAUNCH(DT, 5));
#undef CA_PB_LAUNCH
  CA_CHECK_LAUNCH("ca_pdc_block");
  return CA_OK;
}

extern "C" int ca_cdcm_dil4(const void* x, const void* wt, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t dtype, void* stream) {
  CA_REQUIRE(x && wt && y, "ca_cdcm_dil4: x, wt and y are required");
  CA_REQUIRE(sizes_ok(images, h, w), "ca_cdcm_dil4: images=%d h=%d w=%d (each >= 1, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE(c == CD_C, "ca_cdcm_dil4: c=%d (cin = cout = 32 is what the kernel is built for)", c);
  CA_REQUIRE(dtype_ok(dtype), "ca_cdcm_dil4: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)wt | (uintptr_t)y) & 15) == 0, "ca_cdcm_dil4: x, wt and y must be 16-byte aligned");
  const int64_t bytes = (int64_t)images * h * w * c * 2;
  CA_REQUIRE(!ranges_overlap(x, bytes, y, bytes), "ca_cdcm_dil4: y must not overlap x");
  const int tx = ceil_div_i(w, CD_T), ty = ceil_div_i(h, CD_T);
  const int64_t blocks = (int64_t)images * tx * ty;
  CA_REQUIRE(blocks < ((int64_t)1 << 31), "ca_cdcm_dil4: grid too large");
  const dim3 grid((unsigned)blocks), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_cdcm_dil4<DT>, grid, block, 0, (hipStream_t)stream, (const u16*)x, (const u16*)wt, (u16*)y, (int)h, (int)w, tx, ty));
  CA_CHECK_LAUNCH("ca_cdcm_dil4");
  return CA_OK;
}

extern "C" int ca_csam_reduce(const void* f, const float* w1, const float* b1, const float* w2, const float* wr, const float* br, float* t, float* r, float* side,
                              int32_t images, int32_t h, int32_t w, int32_t c, int32_t dtype, void* stream) {
  CA_REQUIRE(f && w1 && b1 && w2 && wr && br && t && r && side, "ca_csam_reduce: f, w1, b1, w2, wr, br, t, r and side are required");
  CA_REQUIRE(sizes_ok(images, h, w), "ca_csam_reduce: images=%d h=%d w=%d (each >= 1, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE(c == CD_C, "ca_csam_reduce: c=%d (32 is what the kernel is built for)", c);
  CA_REQUIRE(dtype_ok(dtype), "ca_csam_reduce: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)f | (uintptr_t)t) & 15) == 0 && (((uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)w2 | (uintptr_t)wr | (uintptr_t)br | (uintptr_t)r | (uintptr_t)side) & 3) == 0,
             "ca_csam_reduce: f and t must be 16-byte aligned, the fp32 operands 4-byte aligned");
  const int64_t pixels = (int64_t)images * h * w;
  CA_REQUIRE(!ranges_overlap(t, pixels * 16, side, pixels * 4) && !ranges_overlap(r, pixels * 4, side, pixels * 4) && !ranges_overlap(t, pixels * 16, r, pixels * 4),
             "ca_csam_reduce: t, r and side must not overlap");
  const dim3 grid((unsigned)((pixels + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_csam_a<DT>, grid, block, 0, st, (const u16*)f, w1, b1, wr, t, r, pixels));
  CA_CHECK_LAUNCH("ca_csam_reduce");
  hipLaunchKernelGGL(k_csam_b, grid, block, 0, st, (const float*)t, (const float*)r, w2, br, side, pixels, (int)h, (int)w);
  CA_CHECK_LAUNCH("ca_csam_reduce");
  return CA_OK;
}

extern "C" int ca_softedge_fuse(const float* side0, const float* side1, const float* side2, const float* side3, const float* classifier, int32_t images, int32_t h,
                                int32_t w, int32_t safe, float* logit, uint8_t* edges, void* control, int32_t rep, int32_t control_dtype, void* stream) {
  CA_REQUIRE(side0 && side1 && side2 && side3 && classifier, "ca_softedge_fuse: the four side maps and the classifier are required");
  CA_REQUIRE(sizes_ok(images, h, w), "ca_softedge_fuse: images=%d h=%d w=%d (each >= 1, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE(h % 8 == 0 && w % 8 == 0, "ca_softedge_fuse: h=%d w=%d must be multiples of 8 (four levels, the k-th of (h >> k, w >> k))", h, w);
  CA_REQUIRE(logit || edges || control, "ca_softedge_fuse: logit, edges or control is required");
  CA_REQUIRE(safe == 0 || safe == 1, "ca_softedge_fuse: safe=%d (0 or 1)", safe);
  if (const int rc = control_out_checks("ca_softedge_fuse", false, h, w, nullptr, true, rep, control_dtype)) return rc;  // (logit is a third output: above)
  CA_REQUIRE((((uintptr_t)side0 | (uintptr_t)logit) & 15) == 0 && (((uintptr_t)side1 | (uintptr_t)side2 | (uintptr_t)side3 | (uintptr_t)classifier) & 3) == 0,
             "ca_softedge_fuse: side0 and logit must be 16-byte aligned, the other side maps and the classifier 4-byte aligned");
  CA_REQUIRE(((uintptr_t)edges & 3) == 0 && ctrl_aligned(control, control_dtype, 4),
             "ca_softedge_fuse: edges must be 4-byte aligned, control aligned to four of its elements");
  SeSides sd;
  sd.s[0] = side0, sd.s[1] = side1, sd.s[2] = side2, sd.s[3] = side3;
  const int64_t total = (int64_t)images * h * w;
  const dim3 grid((unsigned)((total / 4 + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  CA_DISPATCH_CTRL(control_dtype,
                   hipLaunchKernelGGL(k_se_fuse<T>, grid, block, 0, st, sd, classifier, logit, edges, (T*)control, (int)images, (int)h, (int)w, (int)rep, (int)safe));
  CA_CHECK_LAUNCH("ca_softedge_fuse");
  return CA_OK;
}
