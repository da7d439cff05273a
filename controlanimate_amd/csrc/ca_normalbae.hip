// The NormalBae annotator's stages beside ca_gemm / ca_conv3x3 / ca_upsample2x_bilinear_ac (controlanimate_amd/normalbae.py): the
// EfficientNet encoder's 1x1 convolutions run on ca_gemm (CA_ACT_SILU; the projections with the block's residual), the decoder's 3x3
// convolutions on ca_conv3x3 (CA_ACT_LEAKY001, the skip as the second source) and the per-pixel MLPs of the refinement stages on ca_gemm
// (CA_ACT_RELU, the interpolated prediction as the second source); this file holds what none of them can run:
//
//   stem       k_nbae_stem        uint8 RGB [n,H,W,3] -> swish(Conv3x3 s2 SAME((src / 255 - mean) / std) + bias) at cout channels; the zero
//                                 padding (0 before, 1 after) lies in the NORMALISED image; fp32 weights [27][cout] (BatchNorm folded), VALU
//   depthwise  k_dwconv_same      depthwise 3x3 / 5x5, stride 1 / 2, TensorFlow-SAME padding, fp32 bias, swish.  A thread owns 8 channels of
//                                 one output column over a strip of 8 output rows and keeps the rows that are still open in registers: an
//                                 input row is loaded once per strip (+ ksize - 1 rows of overlap).  It also leaves the per-block sums of the
//                                 values it STORED (the rounded ones), which k_dw_sum_finish adds in a fixed order into sums [n][c]: the
//                                 squeeze-and-excite pool costs no pass over the expanded tensor
//   gate       k_se_gate          sigmoid(W_e swish(W_r mean + b_r) + b_e), fp32, the whole batch in one launch (the reduce widths are no
//                                 multiples of 8: VALU)
//   scale      k_scale_channels   y = round(x * gate[image][channel]), in place allowed
//   cat_pred   k_nbae_cat_pred    the 4-channel fp32 prediction, x2 bilinear with align_corners, rounded into 8 columns (4 of them zero) of
//                                 the MLP's second source
//   normalize  k_nbae_normalize   norm_normalize: xyz / (|xyz| + 1e-10), kappa = elu(k) + 1 + min_kappa, fp32
//   refine     k_nbae_refine      one refinement stage in one launch: interpolation into LDS, four layers on the MFMA, norm_normalize
//   finish     k_nbae_finish      trunc(clip(clip((xyz + 1) * 0.5, 0, 1) * 255, 0, 255)) -> the uint8 map [n,H,W,3] and / or the control tensor
//                                 (ca_annot.h; one level per channel)
//
// Compiled with -ffp-contract=off: the finish and the normalisation round operation by operation, as numpy and torch do; the sums of the
// convolutions use fmaf explicitly.  No launch reads device data on the host, there are no floating-point atomics: two runs give the
// same bits, and the chain can be captured in a hipGraph.
#include "ca_common.h"
#include "ca_annot.h"

namespace {

// TensorFlow "SAME": out = ceil(in / stride), total = max((out - 1) * stride + k - in, 0), total / 2 of it in front
struct SamePad {
  int out, before;
};
inline SamePad same_pad(int in, int k, int s) {
  const int out = (in + s - 1) / s;
  int total = (out - 1) * s + k - in;
  total = total < 0 ? 0 : total;
  return {out, total / 2};
}

// ---- stem ------------------------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void k_nbae_stem(const uint8_t* __restrict__ src, const float* __restrict__ wt, const float* __restrict__ bias,
                                                   u16* __restrict__ y, int64_t total, int H, int W, int cout) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cl = cout >> 3, ho = H >> 1, wo = W >> 1;
  const int cg = (int)(idx % cl);
  const int64_t op = idx / cl;
  const int ox = (int)(op % wo);
  const int oy = (int)((op / wo) % ho);
  const int64_t img = op / ((int64_t)ho * wo);
  const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = bias[cg * 8 + e];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = 2 * oy + ky;
    if (iy >= H) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = 2 * ox + kx;
      if (ix >= W) continue;
      const uint8_t* p = src + ((img * H + iy) * W + ix) * 3;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float xn = __fdiv_rn(__fdiv_rn((float)p[ch], 255.0f) - mean[ch], sd[ch]);
        const float* wk = wt + (int64_t)((ky * 3 + kx) * 3 + ch) * cout + cg * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(wk[e], xn, acc[e]);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = silu_f(acc[e]);
  st16(y + op * cout + cg * 8, pack8<DT>(acc));
}

// ---- depthwise, SAME padding, swish, pooled sums --------------------------------------------------------------------------------------
constexpr int DS_ROWS = 8;  // output rows per strip

// how a block of 256 threads is cut: cgb groups of 8 channels x pxb output columns
inline void dw_block_shape(int c, int& cgb, int& pxb) {
  const int cl = c >> 3;
  cgb = cl < 32 ? cl : 32;
  pxb = 256 / cgb;
}

// Padded row r = S * oy + ky.  The step m handles the padded rows S * m .. S * m + S - 1; output row oy is open during the steps oy .. oy + NA - 1,
// NA = KS (stride 1) or (KS + 1) / 2 (stride 2).  acc[j] belongs to output row m - (NA - 1) + j and takes the kernel rows S * (NA - 1 - j) + sub.
template <int DT, int KS, int S>
__global__ __launch_bounds__(256) void k_dwconv_same(const u16* __restrict__ x, const u16* __restrict__ wt, const float* __restrict__ bias, u16* __restrict__ y,
                                                     float* __restrict__ partials, int h, int w, int ho, int wo, int c, int pt, int pl, int strips, int xchunks,
                                                     int cchunks, int cgb, int pxb) {
  __shared__ float red[256 * 8];
  constexpr int NA = S == 1 ? KS : (KS + 1) / 2;
  int b = blockIdx.x;
  const int cchunk = b % cchunks;
  b /= cchunks;
  const int xchunk = b % xchunks;
  b /= xchunks;
  const int strip = b % strips;
  const int img = b / strips;
  const int t = threadIdx.x;
  const int cgl = t % cgb, pxl = t / cgb;
  const int cl = c >> 3;
  const int cg = cchunk * cgb + cgl;
  const int ox = xchunk * pxb + pxl;
  const bool live = pxl < pxb && cg < cl && ox < wo;
  float lsum[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) lsum[e] = 0.f;
  if (live) {
    const u16* xi = x + (int64_t)img * h * w * c + cg * 8;
    u16* yo = y + (int64_t)img * ho * wo * c + cg * 8;
    u32x4 wk[KS * KS];
#pragma unroll
    for (int k = 0; k < KS * KS; ++k) wk[k] = ld16(wt + (int64_t)k * c + cg * 8);
    float b8[8], acc[NA][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) b8[e] = bias[cg * 8 + e];
#pragma unroll
    for (int j = 0; j < NA; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[j][e] = b8[e];
    const int oy0 = strip * DS_ROWS, oy1 = oy0 + DS_ROWS < ho ? oy0 + DS_ROWS : ho;
    const int ix0 = ox * S - pl;
    for (int m = oy0; m < oy1 + NA - 1; ++m) {
#pragma unroll
      for (int sub = 0; sub < S; ++sub) {
        const int iy = m * S + sub - pt;
        const bool rowok = iy >= 0 && iy < h;
        float v[KS][8];
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
          const int ix = ix0 + kx;
          if (rowok && ix >= 0 && ix < w) {
            unpack8<DT>(ld16(xi + ((int64_t)iy * w + ix) * c), v[kx]);
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[kx][e] = 0.f;
          }
        }
#pragma unroll
        for (int j = 0; j < NA; ++j) {
          const int ky = S * (NA - 1 - j) + sub;
          if (ky < KS) {
#pragma unroll
            for (int kx = 0; kx < KS; ++kx) {
              float wf[8];
              unpack8<DT>(wk[ky * KS + kx], wf);
#pragma unroll
              for (int e = 0; e < 8; ++e) acc[j][e] = fmaf(wf[e], v[kx][e], acc[j][e]);
            }
          }
        }
      }
      const int oy = m - (NA - 1);
      if (oy >= oy0) {  // (oy < oy1 by the loop's bound)
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = silu_f(acc[0][e]);
        const u32x4 pk = pack8<DT>(o);
        st16(yo + ((int64_t)oy * wo + ox) * c, pk);
        unpack8<DT>(pk, o);  // the stored values are what the pool sums
#pragma unroll
        for (int e = 0; e < 8; ++e) lsum[e] += o[e];
      }
#pragma unroll
      for (int j = 0; j + 1 < NA; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[j][e] = acc[j + 1][e];
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[NA - 1][e] = b8[e];
    }
  }
  if (pxl < pxb) {
#pragma unroll
    for (int e = 0; e < 8; ++e) red[(pxl * cgb + cgl) * 8 + e] = lsum[e];
  }
  __syncthreads();
  if (t < cgb * 8) {
    const int ch = cchunk * cgb * 8 + t;
    if (ch < c) {
      float s = 0.f;
      for (int p = 0; p < pxb; ++p) s += red[p * cgb * 8 + t];
      const int64_t chunks = (int64_t)strips * xchunks;
      partials[((int64_t)img * chunks + (int64_t)strip * xchunks + xchunk) * c + ch] = s;
    }
  }
}

// sums[img][ch] = the chunk sums in four runs of consecutive chunks, each in order, then ((s0 + s1) + s2) + s3
__global__ __launch_bounds__(256) void k_dw_sum_finish(const float* __restrict__ partials, float* __restrict__ sums, int chunks, int c, int cblocks) {
  __shared__ float seg[4][64];
  const int img = blockIdx.x / cblocks, cb = blockIdx.x % cblocks;
  const int l = threadIdx.x & 63, sg = threadIdx.x >> 6;
  const int ch = cb * 64 + l;
  const int per = (chunks + 3) / 4;
  const int lo = sg * per, hi = lo + per < chunks ? lo + per : chunks;
  float s = 0.f;
  if (ch < c)
    for (int k = lo; k < hi; ++k) s += partials[((int64_t)img * chunks + k) * c + ch];
  seg[sg][l] = s;
  __syncthreads();
  if (sg == 0 && ch < c) sums[(int64_t)img * c + ch] = ((seg[0][l] + seg[1][l]) + seg[2][l]) + seg[3][l];
}

// Every block of an image (ceil(c / 256) of them) computes the whole reduce layer for itself: r dot products of length c, at most
// 76 x 3072 multiply-adds for B5, instead of a second launch and a round trip of r floats through memory -- deliberate.
// ---- squeeze-and-excite gate ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_se_gate(const float* __restrict__ sums, const float* __restrict__ wr, const float* __restrict__ br,
                                                 const float* __restrict__ wet, const float* __restrict__ be, float* __restrict__ gate, int c, int r,
                                                 float inv_pixels) {
  __shared__ float sq[256];
  const int img = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* sm = sums + (int64_t)img * c;
  for (int j = wave; j < r; j += 4) {
    float s = 0.f;
    for (int i = lane; i < c; i += 64) s = fmaf(wr[(int64_t)j * c + i], sm[i] * inv_pixels, s);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) {
      const float v = s + br[j];
      sq[j] = v / (1.0f + expf(-v));
    }
  }
  __syncthreads();
  const int ch = blockIdx.x * 256 + threadIdx.x;
  if (ch < c) {
    float a = be[ch];
    for (int j = 0; j < r; ++j) a = fmaf(wet[(int64_t)j * c + ch], sq[j], a);
    gate[(int64_t)img * c + ch] = 1.0f / (1.0f + expf(-a));
  }
}

template <int DT>
__global__ __launch_bounds__(256) void k_scale_channels(const u16* x, const float* __restrict__ gate, u16* y, int64_t total, int64_t pixels, int c) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cl = c >> 3;
  const int cg = (int)(idx % cl);
  const int64_t img = (idx / cl) / pixels;
  const float* g = gate + img * c + cg * 8;
  float v[8];
  unpack8<DT>(ld16(x + idx * 8), v);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = v[e] * g[e];
  st16(y + idx * 8, pack8<DT>(v));
}

// ---- the refinement stages' pieces ----------------------------------------------------------------------------------------------------------
// src = dst * (in - 1) / (out - 1), as k_up2_ac of ca_mlsd.hip computes it
__device__ __forceinline__ void ac_coord(int d, int in, int out, int& i0, int& i1, float& f) {
  const float s = out > 1 ? __fdiv_rn((float)(d * (in - 1)), (float)(out - 1)) : 0.f;
  i0 = (int)s;
  i0 = i0 > in - 1 ? in - 1 : i0;
  i1 = i0 + 1 < in ? i0 + 1 : in - 1;
  f = s - (float)i0;
}

template <int DT>
__global__ __launch_bounds__(256) void k_nbae_cat_pred(const float* __restrict__ pred, u16* __restrict__ y, int64_t total, int h, int w, int64_t ld, int col0) {
  const int64_t op = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (op >= total) return;
  const int ox = (int)(op % (2 * w));
  const int oy = (int)((op / (2 * w)) % (2 * h));
  const int64_t img = op / ((int64_t)4 * h * w);
  int y0, y1, x0, x1;
  float fy, fx;
  ac_coord(oy, h, 2 * h, y0, y1, fy);
  ac_coord(ox, w, 2 * w, x0, x1, fx);
  const float* pi = pred + img * h * w * 4;
  const f32x4 a = *(const f32x4*)(pi + ((int64_t)y0 * w + x0) * 4), b = *(const f32x4*)(pi + ((int64_t)y0 * w + x1) * 4);
  const f32x4 cc = *(const f32x4*)(pi + ((int64_t)y1 * w + x0) * 4), d = *(const f32x4*)(pi + ((int64_t)y1 * w + x1) * 4);
  float o[8];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float top = a[e] * (1.0f - fx) + b[e] * fx;
    const float bot = cc[e] * (1.0f - fx) + d[e] * fx;
    o[e] = top * (1.0f - fy) + bot * fy;
    o[e + 4] = 0.f;
  }
  st16(y + op * ld + col0, pack8<DT>(o));
}

__global__ __launch_bounds__(256) void k_nbae_normalize(const float* __restrict__ raw, int64_t ld, float* __restrict__ pred, int64_t rows, float min_kappa) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  const f32x4 v = *(const f32x4*)(raw + row * ld);
  const float nrm = __fsqrt_rn((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + 1e-10f;
  f32x4 o;
  o[0] = __fdiv_rn(v[0], nrm), o[1] = __fdiv_rn(v[1], nrm), o[2] = __fdiv_rn(v[2], nrm);
  o[3] = ((v[3] > 0.f ? v[3] : expm1f(v[3])) + 1.0f) + min_kappa;
  *(f32x4*)(pred + row * 4) = o;
}

// ---- one refinement stage in one launch ------------------------------------------------------------------------------------------------
// A block owns RF_PIX consecutive output pixels.  It interpolates their C feature channels (k_up2_ac's arithmetic and rounding: the row is
// what the composed form's ca_upsample2x_bilinear_ac stores) and the fp32 prediction (k_nbae_cat_pred's) ONCE into LDS rows of KP = C + 8
// padded to a multiple of 32 columns, then runs the four layers on the MFMA: wave = (pixel group of 16) x (half of the 128 hidden
// channels); the hidden activations go from one LDS buffer to the other and never leave the chip.  The weights come as MFMA fragments in
// the order the host made (normalbae.pack_mlp_frag): fragment (ks, t) is 64 lanes x 16 bytes, one coalesced 1 KB read from L2 per wave.
constexpr int RF_PIX = 32, RF_HID = 128, RF_HP = RF_HID + 8;

template <int DT, int KSTEPS>
__device__ __forceinline__ void rf_layer(const u16* xin, int pitch, const u16* __restrict__ wfrag, const float* __restrict__ bias, u16* hout, int pg, int ch, int lane) {
  const int q = lane >> 4, r16 = lane & 15;
  f32x4 acc[4];
#pragma unroll
  for (int tt = 0; tt < 4; ++tt) acc[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const u16* row = xin + (pg * 16 + r16) * pitch + q * 8;
#pragma unroll 2
  for (int ks = 0; ks < KSTEPS; ++ks) {
    const u32x4 b = ld16(row + ks * 32);
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const u32x4 a = ld16(wfrag + ((int64_t)(ks * 8 + ch * 4 + tt) * 64 + lane) * 8);
      acc[tt] = Elem<DT>::mfma(a, b, acc[tt]);
    }
  }
#pragma unroll
  for (int tt = 0; tt < 4; ++tt) {
    const int c0 = (ch * 4 + tt) * 16 + q * 4;
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = fmaxf(acc[tt][i] + bias[c0 + i], 0.f);
    u32x2 o;
    o[0] = pack2<DT>(v[0], v[1]), o[1] = pack2<DT>(v[2], v[3]);
    *(u32x2*)(hout + (pg * 16 + r16) * RF_HP + c0) = o;
  }
}

template <int DT, int C>
__global__ __launch_bounds__(256) void k_nbae_refine(const u16* __restrict__ feat, const float* __restrict__ pred, const u16* __restrict__ w0, const u16* __restrict__ w1,
                                                     const u16* __restrict__ w2, const u16* __restrict__ w3, const float* __restrict__ b0, const float* __restrict__ b1,
                                                     const float* __restrict__ b2, const float* __restrict__ b3, float* __restrict__ out, int64_t total, int h, int w,
                                                     float min_kappa) {
  constexpr int KP = (C + 8 + 31) / 32 * 32, XP = KP + 8, ITEMS = KP / 8;
  __shared__ __attribute__((aligned(16))) u16 xs[RF_PIX * XP];
  __shared__ __attribute__((aligned(16))) u16 ha[RF_PIX * RF_HP];
  __shared__ __attribute__((aligned(16))) u16 hb[RF_PIX * RF_HP];
  const int64_t p0 = (int64_t)blockIdx.x * RF_PIX;
  for (int i = threadIdx.x; i < RF_PIX * ITEMS; i += 256) {
    const int pl = i / ITEMS, it = i - pl * ITEMS;
    const int64_t op = p0 + pl;
    u32x4 v = (u32x4){0u, 0u, 0u, 0u};
    if (op < total && it <= C / 8) {
      const int ox = (int)(op % (2 * w));
      const int oy = (int)((op / (2 * w)) % (2 * h));
      const int64_t img = op / ((int64_t)4 * h * w);
      int y0, y1, x0, x1;
      float fy, fx;
      ac_coord(oy, h, 2 * h, y0, y1, fy);
      ac_coord(ox, w, 2 * w, x0, x1, fx);
      float o[8];
      if (it < C / 8) {
        const u16* xi = feat + img * h * w * C + it * 8;
        float a[8], b[8], cc[8], d[8];
        unpack8<DT>(ld16(xi + ((int64_t)y0 * w + x0) * C), a);
        unpack8<DT>(ld16(xi + ((int64_t)y0 * w + x1) * C), b);
        unpack8<DT>(ld16(xi + ((int64_t)y1 * w + x0) * C), cc);
        unpack8<DT>(ld16(xi + ((int64_t)y1 * w + x1) * C), d);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float top = a[e] * (1.0f - fx) + b[e] * fx;
          const float bot = cc[e] * (1.0f - fx) + d[e] * fx;
          o[e] = top * (1.0f - fy) + bot * fy;
        }
      } else {
        const float* pi = pred + img * h * w * 4;
        const f32x4 a = *(const f32x4*)(pi + ((int64_t)y0 * w + x0) * 4), b = *(const f32x4*)(pi + ((int64_t)y0 * w + x1) * 4);
        const f32x4 cc = *(const f32x4*)(pi + ((int64_t)y1 * w + x0) * 4), d = *(const f32x4*)(pi + ((int64_t)y1 * w + x1) * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float top = a[e] * (1.0f - fx) + b[e] * fx;
          const float bot = cc[e] * (1.0f - fx) + d[e] * fx;
          o[e] = top * (1.0f - fy) + bot * fy;
          o[e + 4] = 0.f;
        }
      }
      v = pack8<DT>(o);
    }
    st16(xs + pl * XP + it * 8, v);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pg = wave & 1, ch = wave >> 1;
  rf_layer<DT, KP / 32>(xs, XP, w0, b0, ha, pg, ch, lane);
  __syncthreads();
  rf_layer<DT, RF_HID / 32>(ha, RF_HP, w1, b1, hb, pg, ch, lane);
  __syncthreads();
  rf_layer<DT, RF_HID / 32>(hb, RF_HP, w2, b2, ha, pg, ch, lane);
  __syncthreads();
  if (ch == 0) {  // the last layer: 4 outputs in one 16-row tile (rows 4 .. 15 of the fragment are zero)
    const int q = lane >> 4, r16 = lane & 15;
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < RF_HID / 32; ++ks) {
      const u32x4 b = ld16(ha + (pg * 16 + r16) * RF_HP + ks * 32 + q * 8);
      const u32x4 a = ld16(w3 + ((int64_t)ks * 64 + lane) * 8);
      acc = Elem<DT>::mfma(a, b, acc);
    }
    const int64_t op = p0 + pg * 16 + r16;
    if (q == 0 && op < total) {
      const float x = acc[0] + b3[0], y = acc[1] + b3[1], z = acc[2] + b3[2], k = acc[3] + b3[3];
      const float nrm = __fsqrt_rn((x * x + y * y) + z * z) + 1e-10f;
      f32x4 o;
      o[0] = __fdiv_rn(x, nrm), o[1] = __fdiv_rn(y, nrm), o[2] = __fdiv_rn(z, nrm);
      o[3] = ((k > 0.f ? k : expm1f(k)) + 1.0f) + min_kappa;
      *(f32x4*)(out + op * 4) = o;
    }
  }
}

// ---- finish ------------------------------------------------------------------------------------------------------------------------------
// 4 consecutive pixels per thread (h * w % 4 == 0): 12 bytes of the map, 16 / 8-byte stores to the control tensor
template <typename T>
__global__ __launch_bounds__(256) void k_nbae_finish(const float* __restrict__ pred, uint8_t* __restrict__ map, T* __restrict__ ctrl, int images, int64_t hw, int rep) {
  const int64_t g0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (g0 >= images * hw) return;
  const int img = (int)(g0 / hw);
  const int64_t p = g0 - img * hw;
  int level[4][3];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x4 v = *(const f32x4*)(pred + (g0 + i) * 4);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float t = (v[ch] + 1.0f) * 0.5f;
      t = !(t > 0.0f) ? 0.0f : (t > 1.0f ? 1.0f : t);  // (a NaN counts as 0)
      float u = t * 255.0f;
      u = u < 0.0f ? 0.0f : (u > 255.0f ? 255.0f : u);
      level[i][ch] = (int)u;                           // truncation, as astype(uint8) of a value in [0, 255]
    }
  }
  if (map) {
    uint32_t wds[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 12; ++k) wds[k >> 2] |= (uint32_t)level[k / 3][k % 3] << (8 * (k & 3));
    uint32_t* m = (uint32_t*)(map + g0 * 3);
    m[0] = wds[0], m[1] = wds[1], m[2] = wds[2];
  }
  if (ctrl) {
    Vec4<T> o[3];  // one level per channel
#pragma unroll
    for (int k = 0; k < 12; ++k) ctrl_from_level(level[k & 3][k >> 2], o[k >> 2].v[k & 3]);
    emit_vec4(ctrl, images, img, hw, p, rep, o);
  }
}

struct DwGeom {
  SamePad py, px;
  int strips, xchunks, cchunks, cgb, pxb;
  int64_t chunks;
};
inline DwGeom dw_geom(int h, int w, int c, int ksize, int stride) {
  DwGeom g;
  g.py = same_pad(h, ksize, stride), g.px = same_pad(w, ksize, stride);
  dw_block_shape(c, g.cgb, g.pxb);
  g.strips = ceil_div_i(g.py.out, DS_ROWS);
  g.xchunks = ceil_div_i(g.px.out, g.pxb);
  g.cchunks = ceil_div_i(c >> 3, g.cgb);
  g.chunks = (int64_t)g.strips * g.xchunks;
  return g;
}
inline bool dw_args_ok(int32_t images, int32_t h, int32_t w, int32_t c, int32_t stride) {
  return sizes_ok(images, h, w) && c >= 8 && c <= 3072 && c % 8 == 0 && (stride == 1 || stride == 2) && (int64_t)images * h * w * c * 2 <= kMaxBytes;
}

template <int DT, int KS, int S>
void launch_dw(dim3 grid, hipStream_t st, const void* x, const void* wt, const float* bias, void* y, float* partials, int h, int w, int c, const DwGeom& g) {
  hipLaunchKernelGGL((k_dwconv_same<DT, KS, S>), grid, dim3(256), 0, st, (const u16*)x, (const u16*)wt, bias, (u16*)y, partials, h, w, g.py.out, g.px.out, c,
                     g.py.before, g.px.before, g.strips, g.xchunks, g.cchunks, g.cgb, g.pxb);
}
template <int DT>
void launch_dw_dt(int ksize, int stride, dim3 grid, hipStream_t st, const void* x, const void* wt, const float* bias, void* y, float* partials, int h, int w, int c,
                  const DwGeom& g) {
  if (ksize == 3 && stride == 1) launch_dw<DT, 3, 1>(grid, st, x, wt, bias, y, partials, h, w, c, g);
  else if (ksize == 3) launch_dw<DT, 3, 2>(grid, st, x, wt, bias, y, partials, h, w, c, g);
  else if (stride == 1) launch_dw<DT, 5, 1>(grid, st, x, wt, bias, y, partials, h, w, c, g);
  else launch_dw<DT, 5, 2>(grid, st, x, wt, bias, y, partials, h, w, c, g);
}

}  // namespace

extern "C" int ca_nbae_stem(const uint8_t* src, const float* wt, const float* bias, void* y, int32_t images, int32_t h, int32_t w, int32_t cout, int32_t dtype,
                            void* stream) {
  CA_REQUIRE(src && wt && bias && y, "ca_nbae_stem: src, wt, bias and y are required");
  CA_REQUIRE(sizes_ok(images, h, w) && h % 2 == 0 && w % 2 == 0, "ca_nbae_stem: images=%d h=%d w=%d (images >= 1, h and w even and >= 2, images * h * w < 2^31)",
             images, h, w);
  CA_REQUIRE(cout >= 8 && cout <= 64 && cout % 8 == 0, "ca_nbae_stem: cout=%d must be a multiple of 8 in 8 .. 64", cout);
  CA_REQUIRE(dtype_ok(dtype), "ca_nbae_stem: dtype %d", dtype);
  CA_REQUIRE(((uintptr_t)y & 15) == 0 && (((uintptr_t)wt | (uintptr_t)bias) & 3) == 0, "ca_nbae_stem: y must be 16-byte aligned, wt and bias 4-byte aligned");
  CA_REQUIRE((int64_t)images * (h / 2) * (w / 2) * cout * 2 <= kMaxBytes, "ca_nbae_stem: images=%d h=%d w=%d: y would pass 2^31 bytes", images, h, w);
  const int64_t total = (int64_t)images * (h / 2) * (w / 2) * (cout / 8);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_nbae_stem<DT>, grid, block, 0, (hipStream_t)stream, src, wt, bias, (u16*)y, total, (int)h, (int)w, (int)cout));
  CA_CHECK_LAUNCH("ca_nbae_stem");
  return CA_OK;
}

extern "C" int64_t ca_dwconv_same_partials_floats(int32_t images, int32_t h, int32_t w, int32_t c, int32_t stride) {
  if (!dw_args_ok(images, h, w, c, stride)) return 0;
  return (int64_t)images * dw_geom(h, w, c, 3, stride).chunks * c;  // (the output plane, and with it the chunks, is the same for ksize 3 and 5)
}

extern "C" int ca_dwconv_same(const void* x, const void* wt, const float* bias, void* y, float* sums, float* partials, int32_t images, int32_t h, int32_t w,
                              int32_t c, int32_t ksize, int32_t stride, int32_t dtype, void* stream) {
  CA_REQUIRE(x && wt && bias && y && sums && partials, "ca_dwconv_same: x, wt, bias, y, sums and partials are required");
  CA_REQUIRE(dw_args_ok(images, h, w, c, stride),
             "ca_dwconv_same: images=%d h=%d w=%d c=%d stride=%d (sizes >= 1, c a multiple of 8 in 8 .. 3072, stride 1 or 2, x below 2^31 bytes)", images, h, w, c, stride);
  CA_REQUIRE(ksize == 3 || ksize == 5, "ca_dwconv_same: ksize=%d (3 or 5)", ksize);
  CA_REQUIRE(dtype_ok(dtype), "ca_dwconv_same: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)wt | (uintptr_t)y) & 15) == 0 && (((uintptr_t)bias | (uintptr_t)sums | (uintptr_t)partials) & 3) == 0,
             "ca_dwconv_same: x, wt and y must be 16-byte aligned, bias, sums and partials 4-byte aligned");
  const DwGeom g = dw_geom(h, w, c, ksize, stride);
  const int64_t xbytes = (int64_t)images * h * w * c * 2, ybytes = (int64_t)images * g.py.out * g.px.out * c * 2;
  CA_REQUIRE((const char*)y + ybytes <= (const char*)x || (const char*)x + xbytes <= (const char*)y, "ca_dwconv_same: y must not overlap x");
  const int64_t blocks = (int64_t)images * g.chunks * g.cchunks;
  CA_REQUIRE(blocks < ((int64_t)1 << 31) && g.chunks < ((int64_t)1 << 30), "ca_dwconv_same: grid too large");
  const dim3 grid((unsigned)blocks);
  hipStream_t st = (hipStream_t)stream;
  CA_DISPATCH_DT(dtype, launch_dw_dt<DT>(ksize, stride, grid, st, x, wt, bias, y, partials, h, w, c, g));
  CA_CHECK_LAUNCH("ca_dwconv_same");
  const int cblocks = ceil_div_i(c, 64);
  hipLaunchKernelGGL(k_dw_sum_finish, dim3((unsigned)(images * cblocks)), dim3(256), 0, st, (const float*)partials, sums, (int)g.chunks, (int)c, cblocks);
  CA_CHECK_LAUNCH("ca_dwconv_same (sums)");
  return CA_OK;
}

extern "C" int ca_se_gate(const float* sums, const float* w_reduce, const float* b_reduce, const float* w_expand_t, const float* b_expand, float* gate,
                          int32_t images, int32_t c, int32_t r, float inv_pixels, void* stream) {
  CA_REQUIRE(sums && w_reduce && b_reduce && w_expand_t && b_expand && gate, "ca_se_gate: sums, w_reduce, b_reduce, w_expand_t, b_expand and gate are required");
  CA_REQUIRE(images >= 1 && images <= 65535 && c >= 1 && c <= 3072 && r >= 1 && r <= 256, "ca_se_gate: images=%d c=%d r=%d (1 .. 65535, 1 .. 3072, 1 .. 256)", images, c, r);
  CA_REQUIRE(inv_pixels > 0.f, "ca_se_gate: inv_pixels=%g must be positive", (double)inv_pixels);
  CA_REQUIRE((((uintptr_t)sums | (uintptr_t)w_reduce | (uintptr_t)b_reduce | (uintptr_t)w_expand_t | (uintptr_t)b_expand | (uintptr_t)gate) & 3) == 0,
             "ca_se_gate: operands must be 4-byte aligned");
  hipLaunchKernelGGL(k_se_gate, dim3((unsigned)ceil_div_i(c, 256), (unsigned)images), dim3(256), 0, (hipStream_t)stream, sums, w_reduce, b_reduce, w_expand_t, b_expand,
                     gate, (int)c, (int)r, inv_pixels);
  CA_CHECK_LAUNCH("ca_se_gate");
  return CA_OK;
}

extern "C" int ca_scale_channels(const void* x, const float* gate, void* y, int32_t images, int64_t pixels, int32_t c, int32_t dtype, void* stream) {
  CA_REQUIRE(x && gate && y, "ca_scale_channels: x, gate and y are required");
  CA_REQUIRE(images >= 1 && pixels >= 1 && c >= 8 && c <= 3072 && c % 8 == 0 && (int64_t)images * pixels <= kMaxPixels && (int64_t)images * pixels * c * 2 <= kMaxBytes,
             "ca_scale_channels: images=%d pixels=%lld c=%d (c a multiple of 8 in 8 .. 3072, x below 2^31 bytes)", images, (long long)pixels, c);
  CA_REQUIRE(dtype_ok(dtype), "ca_scale_channels: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0 && ((uintptr_t)gate & 3) == 0, "ca_scale_channels: x and y must be 16-byte aligned, gate 4-byte aligned");
  const int64_t bytes = (int64_t)images * pixels * c * 2;
  CA_REQUIRE(x == y || (const char*)y + bytes <= (const char*)x || (const char*)x + bytes <= (const char*)y, "ca_scale_channels: y is x or does not overlap it");
  const int64_t total = (int64_t)images * pixels * (c / 8);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_scale_channels<DT>, grid, block, 0, (hipStream_t)stream, (const u16*)x, gate, (u16*)y, total, pixels, (int)c));
  CA_CHECK_LAUNCH("ca_scale_channels");
  return CA_OK;
}

extern "C" int ca_nbae_cat_pred(const float* pred, void* y, int32_t images, int32_t h, int32_t w, int64_t ld, int32_t col0, int32_t dtype, void* stream) {
  CA_REQUIRE(pred && y, "ca_nbae_cat_pred: pred and y are required");
  CA_REQUIRE(sizes_ok(images, h, w, 4), "ca_nbae_cat_pred: images=%d h=%d w=%d (each >= 1, images * 2 h * 2 w < 2^31)", images, h, w);
  CA_REQUIRE(ld >= 8 && ld % 8 == 0 && col0 >= 0 && col0 % 8 == 0 && (int64_t)col0 + 8 <= ld, "ca_nbae_cat_pred: ld=%lld col0=%d (multiples of 8, col0 + 8 <= ld)",
             (long long)ld, col0);
  CA_REQUIRE((int64_t)images * h * w * 4 * ld * 2 <= kMaxBytes, "ca_nbae_cat_pred: y would pass 2^31 bytes");
  CA_REQUIRE(dtype_ok(dtype), "ca_nbae_cat_pred: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)pred | (uintptr_t)y) & 15) == 0, "ca_nbae_cat_pred: pred and y must be 16-byte aligned");
  const int64_t total = (int64_t)images * h * w * 4;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_nbae_cat_pred<DT>, grid, block, 0, (hipStream_t)stream, pred, (u16*)y, total, (int)h, (int)w, ld, (int)col0));
  CA_CHECK_LAUNCH("ca_nbae_cat_pred");
  return CA_OK;
}

extern "C" int ca_nbae_normalize(const float* raw, int64_t ld, float* pred, int64_t rows, float min_kappa, void* stream) {
  CA_REQUIRE(raw && pred, "ca_nbae_normalize: raw and pred are required");
  CA_REQUIRE(rows >= 1 && rows <= kMaxPixels && ld >= 4 && ld % 4 == 0 && ld <= 4096, "ca_nbae_normalize: rows=%lld ld=%lld (rows in 1 .. 2^31 - 1, ld a multiple of 4)",
             (long long)rows, (long long)ld);
  CA_REQUIRE((((uintptr_t)raw | (uintptr_t)pred) & 15) == 0, "ca_nbae_normalize: raw and pred must be 16-byte aligned");
  hipLaunchKernelGGL(k_nbae_normalize, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, raw, ld, pred, rows, min_kappa);
  CA_CHECK_LAUNCH("ca_nbae_normalize");
  return CA_OK;
}

extern "C" int ca_nbae_refine(const void* feat, const float* pred, const void* w0, const void* w1, const void* w2, const void* w3, const float* b0, const float* b1,
                              const float* b2, const float* b3, float* out, int32_t images, int32_t h, int32_t w, int32_t c, float min_kappa, int32_t dtype,
                              void* stream) {
  CA_REQUIRE(feat && pred && w0 && w1 && w2 && w3 && b0 && b1 && b2 && b3 && out, "ca_nbae_refine: feat, pred, four weight fragments, four biases and out are required");
  CA_REQUIRE(sizes_ok(images, h, w, 4), "ca_nbae_refine: images=%d h=%d w=%d (each >= 1, images * 2 h * 2 w < 2^31)", images, h, w);
  CA_REQUIRE(c == 128 || c == 256 || c == 512, "ca_nbae_refine: c=%d (128, 256 or 512; other widths run in the composed form)", c);
  CA_REQUIRE((int64_t)images * h * w * c * 2 <= kMaxBytes, "ca_nbae_refine: feat would pass 2^31 bytes");
  CA_REQUIRE(dtype_ok(dtype), "ca_nbae_refine: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)feat | (uintptr_t)pred | (uintptr_t)w0 | (uintptr_t)w1 | (uintptr_t)w2 | (uintptr_t)w3 | (uintptr_t)out) & 15) == 0 &&
                 (((uintptr_t)b0 | (uintptr_t)b1 | (uintptr_t)b2 | (uintptr_t)b3) & 3) == 0,
             "ca_nbae_refine: feat, pred, the fragments and out must be 16-byte aligned, the biases 4-byte aligned");
  const int64_t total = (int64_t)images * h * w * 4;
  const dim3 grid((unsigned)((total + RF_PIX - 1) / RF_PIX)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define CA_RF_LAUNCH(DT, C)                                                                                                                                  \
  hipLaunchKernelGGL((k_nbae_refine<DT, C>), grid, block, 0, st, (const u16*)feat, pred, (const u16*)w0, (const u16*)w1, (const u16*)w2, (const u16*)w3, b0, b1, b2, b3, \
                     out, total, (int)h, (int)w, min_kappa)
  CA_DISPATCH_DT(dtype, if (c == 128) CA_RF_LAUNCH(DT, 128);
    else if (c == 256) CA_RF_LAUNCH(DT, 256);
    else CA_RF_LAUNCH(DT, 512));
#undef CA_RF_LAUNCH
  CA_CHECK_LAUNCH("ca_nbae_refine");
  return CA_OK;
}

extern "C" int ca_nbae_finish(const float* pred, int32_t images, int32_t h, int32_t w, uint8_t* map, void* control, int32_t rep, int32_t control_dtype, void* stream) {
  CA_REQUIRE(pred, "ca_nbae_finish: the prediction is required");
  CA_REQUIRE(sizes_ok(images, h, w, 3), "ca_nbae_finish: images=%d h=%d w=%d (each >= 1, 3 * images * h * w < 2^31)", images, h, w);
  if (const int rc = control_out_checks("ca_nbae_finish", true, h, w, "map", map || control, rep, control_dtype)) return rc;
  CA_REQUIRE(((uintptr_t)pred & 15) == 0 && ((uintptr_t)map & 3) == 0 && ctrl_aligned(control, control_dtype, 4),
             "ca_nbae_finish: pred must be 16-byte aligned, map 4-byte aligned, control aligned to four of its elements");
  const int64_t hw = (int64_t)h * w, quads = (int64_t)images * hw / 4;
  const dim3 grid((unsigned)((quads + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  CA_DISPATCH_CTRL(control_dtype, hipLaunchKernelGGL(k_nbae_finish<T>, grid, block, 0, st, pred, map, (T*)control, (int)images, hw, (int)rep));
  CA_CHECK_LAUNCH("ca_nbae_finish");
  return CA_OK;
}
