// Added to ABI v16: the GFPGAN face restorer for aligned faces (controlanimate_amd/gfpgan.py: FaceRestorer; the specification is
// tests/gfpgan_ref.py, restated from the published GFPGANv1Clean / StyleGAN2GeneratorCSFT).  The U-Net's and the SFT branches' 3x3
// convolutions run on ca_conv3x3 (CA_ACT_LEAKY02), the 1x1 skips and final_linear on ca_gemm; none of the other entry points runs a
// modulated convolution, whose weight differs per sample.  These do:
//
//   prep      k_gfp_prep        uint8 faces -> LeakyReLU(conv_body_first((src / 255 - 0.5) / 0.5)), 3 -> cout on the VALU, the channel
//                               reversal a flag
//   resample  k_gfp_up2,        the bilinear x2 (align_corners = False: weights 0.25 / 0.75, clamped edges) and x1/2 (the 2x2 mean) of an
//             k_gfp_down2       NHWC tensor, in torch's operation order (this file is compiled without contraction)
//   styles    k_gfp_styles      every modulated layer's s / m and demod' = m * demod for every image in ONE launch: a block per (layer,
//                               image), fp32 sums in index order
//   modconv   k_gfp_modconv     one StyleConv per launch: demod[n, o] * conv(W, s[n, i] * x) keeps ONE weight for the batch.  An implicit
//                               GEMM on 16x16x32 MFMAs: a block owns 8 x 16 output pixels x 128 (64) output channels and keeps the
//                               10 x 18 input pixels under them in LDS 64 channels at a time, scaled by s while they are staged; with
//                               upsample the tile is the bilinear x2 of a 6 x 10 low-resolution halo that is staged first.  Epilogue:
//                               demod * sqrt(2), noise, bias, LeakyReLU, SFT on the second half of the channels
//   composed  k_gfp_modulate,   the same StyleConv as three launches around ca_conv3x3, whose tiles are faster on the planes below 512 x 512
//             k_gfp_style_      (measured per level; kernels.modconv3x3 picks): the staging (s * x, with the bilinear x2) and the epilogue as
//             epilogue          passes of their own, the same arithmetic; the convolution's output carries one rounding more
//   to_rgb    k_gfp_to_rgb      the 1x1 modulated convolution to 3 channels + bias + the bilinear x2 of the previous fp32 image (VALU)
//   finish    k_gfp_finish      clamp, (x + 1) / 2 * 255, half-to-even rounding, channel reversal -> uint8
//
// No launch depends on device data on the host side: the chain can be captured in a hipGraph.  No atomics: two runs give the same bits.
#include "ca_common.h"
#include "ca_annot.h"

namespace {

__device__ __forceinline__ float leaky02(float v) { return v > 0.f ? v : 0.2f * v; }

// torch's bilinear taps at scale 2, align_corners = False, for output index u of an axis of `size` source elements: source index
// u / 2 - 0.25, clamped at 0 -- (ia, ib) with weights (wa, wb)
__device__ __forceinline__ void up_taps(int u, int size, int& ia, int& ib, float& wa, float& wb) {
  const int k = u >> 1;
  if (u == 0) {
    ia = 0, ib = size > 1 ? 1 : 0, wa = 1.f, wb = 0.f;
  } else if (u & 1) {
    ia = k, ib = k + 1 < size ? k + 1 : size - 1, wa = 0.75f, wb = 0.25f;
  } else {
    ia = k - 1, ib = k, wa = 0.25f, wb = 0.75f;
  }
}
__device__ __forceinline__ float bilin(float a, float b, float c, float d, float wa, float wb, float ha, float hb) {
  return ha * (wa * a + wb * b) + hb * (wa * c + wb * d);
}

// ---- prep --------------------------------------------------------------------------------------------------------------------------
// a thread owns 8 output channels of one pixel
template <int DT>
__global__ __launch_bounds__(256) void k_gfp_prep(const uint8_t* __restrict__ src, const float* __restrict__ wt, const float* __restrict__ bias, u16* __restrict__ y,
                                                  int64_t pixels, int cout, int reverse) {
  const int cl = cout >> 3;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= pixels * cl) return;
  const int64_t pix = idx / cl;
  const int j = (int)(idx - pix * cl);
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = (__fdiv_rn((float)src[pix * 3 + (reverse ? 2 - c : c)], 255.0f) - 0.5f) / 0.5f;
  float f[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int o = j * 8 + e;
    float a = bias[o];
    a = fmaf(wt[o * 3 + 0], v[0], a);
    a = fmaf(wt[o * 3 + 1], v[1], a);
    a = fmaf(wt[o * 3 + 2], v[2], a);
    f[e] = leaky02(a);
  }
  st16(y + pix * cout + j * 8, pack8<DT>(f));
}

// ---- resample ----------------------------------------------------------------------------------------------------------------------
// a thread owns 8 channels of one output pixel
template <int DT>
__global__ __launch_bounds__(256) void k_gfp_up2(const u16* __restrict__ x, u16* __restrict__ y, int64_t total, int h, int w, int c) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cl = c >> 3;
  const int j = (int)(idx % cl);
  const int64_t op = idx / cl;
  const int ox = (int)(op % (2 * w)), oy = (int)((op / (2 * w)) % (2 * h));
  const int64_t img = op / ((int64_t)4 * w * h);
  int ya, yb, xa, xb;
  float ha, hb, wa, wb;
  up_taps(oy, h, ya, yb, ha, hb);
  up_taps(ox, w, xa, xb, wa, wb);
  const u16* xi = x + img * h * w * c + j * 8;
  float a[8], b[8], cc[8], d[8], f[8];
  unpack8<DT>(ld16(xi + ((int64_t)ya * w + xa) * c), a);
  unpack8<DT>(ld16(xi + ((int64_t)ya * w + xb) * c), b);
  unpack8<DT>(ld16(xi + ((int64_t)yb * w + xa) * c), cc);
  unpack8<DT>(ld16(xi + ((int64_t)yb * w + xb) * c), d);
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = bilin(a[e], b[e], cc[e], d[e], wa, wb, ha, hb);
  st16(y + idx * 8, pack8<DT>(f));
}

template <int DT>
__global__ __launch_bounds__(256) void k_gfp_down2(const u16* __restrict__ x, u16* __restrict__ y, int64_t total, int h, int w, int c) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cl = c >> 3, ho = h >> 1, wo = w >> 1;
  const int j = (int)(idx % cl);
  const int64_t op = idx / cl;
  const int ox = (int)(op % wo), oy = (int)((op / wo) % ho);
  const int64_t img = op / ((int64_t)wo * ho);
  const u16* xi = x + ((img * h + 2 * oy) * w + 2 * ox) * c + j * 8;
  float a[8], b[8], cc[8], d[8], f[8];
  unpack8<DT>(ld16(xi), a);
  unpack8<DT>(ld16(xi + c), b);
  unpack8<DT>(ld16(xi + (int64_t)w * c), cc);
  unpack8<DT>(ld16(xi + (int64_t)w * c + c), d);
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = bilin(a[e], b[e], cc[e], d[e], 0.5f, 0.5f, 0.5f, 0.5f);
  st16(y + idx * 8, pack8<DT>(f));
}

// ---- styles ------------------------------------------------------------------------------------------------------------------------
constexpr int GS_MAX_LAYERS = 32, GS_FEAT = 512;
struct StyleDesc {
  int32_t d[GS_MAX_LAYERS * 6];
};

// a block per (layer, image); thread t owns channels t and t + 256
__global__ __launch_bounds__(256) void k_gfp_styles(const float* __restrict__ latents, const float* __restrict__ params, StyleDesc desc, float* __restrict__ out,
                                                    int64_t out_stride, int layers, int num_latent) {
  __shared__ float lat[GS_FEAT];
  __shared__ float sv[512];
  __shared__ float red[256];
  const int layer = blockIdx.x % layers, img = blockIdx.x / layers;
  const int32_t* d = desc.d + layer * 6;
  const int li = d[0], cin = d[1], cout = d[2];
  const float* wm = params + d[3];
  const float* wsq = params + d[4];
  float* o = out + (int64_t)img * out_stride + d[5];
  const float* l = latents + ((int64_t)img * num_latent + li) * GS_FEAT;
  for (int k = threadIdx.x; k < GS_FEAT; k += 256) lat[k] = l[k];
  __syncthreads();
  float amax = 0.f;
  for (int i = threadIdx.x; i < cin; i += 256) {
    float a = 0.f;
    for (int k = 0; k < GS_FEAT; ++k) a = fmaf(lat[k], wm[(int64_t)k * cin + i], a);
    a += wm[(int64_t)GS_FEAT * cin + i];
    sv[i] = a;
    amax = fmaxf(amax, fabsf(a));
  }
  if (cout == 0) {  // ToRGB: s as it is
    for (int i = threadIdx.x; i < cin; i += 256) o[i] = sv[i];
    return;
  }
  red[threadIdx.x] = amax;
  __syncthreads();
  for (int step = 128; step > 0; step >>= 1) {  // (a maximum: the order does not matter)
    if (threadIdx.x < step) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + step]);
    __syncthreads();
  }
  const float m = fmaxf(red[0], 1e-20f);
  for (int i = threadIdx.x; i < cin; i += 256) {
    const float v = sv[i] / m;
    sv[i] = v;
    o[i] = v;
  }
  __syncthreads();
  const float e = (1e-8f / m) / m;
  for (int oc = threadIdx.x; oc < cout; oc += 256) {
    float a = 0.f;
    for (int i = 0; i < cin; ++i) a = fmaf(sv[i] * sv[i], wsq[(int64_t)i * cout + oc], a);
    o[cin + oc] = 1.0f / sqrtf(a + e);
  }
}

// ---- the modulated 3x3 convolution ---------------------------------------------------------------------------------------------------
// The tile kernel of ca_lineart_anime.hip (k_conv_tile) at 3 x 3 taps and stride 1: four waves = 2 (halves of the 8 rows) x 2 (halves of
// the CT = 32 RT output channels); MFMA 16x16x32 with A = 16 output channels x 32 input channels of one tap, read from memory, and B =
// the 16 positions of one tile row, read from LDS (a pixel every KC + 8 elements); a lane ends up with 4 consecutive output channels of
// one position.
constexpr int MC_TW = 16, MC_CTL = 4, MC_TH = 2 * MC_CTL, MC_KC = 64, MC_PITCH = MC_KC + 8, MC_PARTS = MC_KC / 8;
constexpr int MC_HR = MC_TH + 2, MC_HC = MC_TW + 2;          // the halo of the output tile
constexpr int MC_LR = MC_TH / 2 + 2, MC_LC = MC_TW / 2 + 2;  // upsample: the low-resolution pixels under that halo

struct ModconvP {
  const u16 *x, *wt, *sft_scale, *sft_shift;
  const float *s, *demod, *noise, *bias;
  u16* y;
  int64_t s_stride, demod_stride;
  int h, w, cin, cout, gh, gw, tiles_x, tiles_y, x_shared;
  float noise_weight;
};

template <int DT, int RT, bool UP>
__global__ __launch_bounds__(256) void k_gfp_modconv(ModconvP p) {
  constexpr int CT = 32 * RT;
  __shared__ __attribute__((aligned(16))) u16 tile[MC_HR * MC_HC * MC_PITCH];
  __shared__ __attribute__((aligned(16))) u16 low[UP ? MC_LR * MC_LC * MC_PITCH : 8];
  __shared__ float s_s[512];
  const int cts = p.cout / CT;
  int b = blockIdx.x;
  const int ct = b % cts;
  b /= cts;
  const int bx = b % p.tiles_x;
  b /= p.tiles_x;
  const int by = b % p.tiles_y;
  const int img = b / p.tiles_y;
  const int h = p.h, w = p.w, cin = p.cin, cout = p.cout, gh = p.gh, gw = p.gw;
  const int y0 = by * MC_TH, x0 = bx * MC_TW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, r16 = lane & 15;
  const int wm = wave & 1, wn = wave >> 1;
  const u16* xi = p.x + (p.x_shared ? (int64_t)0 : (int64_t)img * h * w * cin);
  for (int i = threadIdx.x; i < cin; i += 256) s_s[i] = p.s[(int64_t)img * p.s_stride + i];
  const u16* wrow[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) wrow[t] = p.wt + ((int64_t)ct * CT + wn * (CT / 2) + t * 16 + r16) * 9 * cin + q * 8;
  f32x4 acc[RT][MC_CTL];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int j = 0; j < MC_CTL; ++j) acc[t][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  bool rowlive[MC_CTL];
#pragma unroll
  for (int j = 0; j < MC_CTL; ++j) rowlive[j] = y0 + wm * MC_CTL + j < gh;  // wave-uniform
  __syncthreads();  // s_s

  for (int c0 = 0; c0 < cin; c0 += MC_KC) {
    if (c0) __syncthreads();
    if (UP) {
      // the low-resolution pixels under the halo, indices clamped to the plane (what the bilinear taps read at the edges)
      const int ly0 = (y0 >> 1) - 1, lx0 = (x0 >> 1) - 1;
      for (int i = threadIdx.x; i < MC_LR * MC_LC * MC_PARTS; i += 256) {
        const int pix = i / MC_PARTS, part = i - pix * MC_PARTS;
        const int r = pix / MC_LC, c = pix - r * MC_LC;
        int ly = ly0 + r, lx = lx0 + c;
        ly = ly < 0 ? 0 : (ly > h - 1 ? h - 1 : ly);
        lx = lx < 0 ? 0 : (lx > w - 1 ? w - 1 : lx);
        st16(low + pix * MC_PITCH + part * 8, ld16(xi + ((int64_t)ly * w + lx) * cin + c0 + part * 8));
      }
      __syncthreads();
      for (int i = threadIdx.x; i < MC_HR * MC_HC * MC_PARTS; i += 256) {
        const int pix = i / MC_PARTS, part = i - pix * MC_PARTS;
        const int r = pix / MC_HC, c = pix - r * MC_HC;
        const int gy = y0 - 1 + r, gx = x0 - 1 + c;
        u32x4 v = (u32x4){0u, 0u, 0u, 0u};
        if (gy >= 0 && gy < gh && gx >= 0 && gx < gw) {
          int ya, yb, xa, xb;
          float ha, hb, wa, wb;
          up_taps(gy, h, ya, yb, ha, hb);
          up_taps(gx, w, xa, xb, wa, wb);
          ya -= ly0, yb -= ly0, xa -= lx0, xb -= lx0;  // within 0 .. MC_LR - 1 / MC_LC - 1 for every pixel of the halo inside the plane
          float a[8], bb[8], cc[8], d[8], f[8];
          unpack8<DT>(ld16(low + (ya * MC_LC + xa) * MC_PITCH + part * 8), a);
          unpack8<DT>(ld16(low + (ya * MC_LC + xb) * MC_PITCH + part * 8), bb);
          unpack8<DT>(ld16(low + (yb * MC_LC + xa) * MC_PITCH + part * 8), cc);
          unpack8<DT>(ld16(low + (yb * MC_LC + xb) * MC_PITCH + part * 8), d);
#pragma unroll
          for (int e = 0; e < 8; ++e) f[e] = bilin(a[e], bb[e], cc[e], d[e], wa, wb, ha, hb) * s_s[c0 + part * 8 + e];
          v = pack8<DT>(f);
        }
        st16(tile + pix * MC_PITCH + part * 8, v);
      }
    } else {
      for (int i = threadIdx.x; i < MC_HR * MC_HC * MC_PARTS; i += 256) {
        const int pix = i / MC_PARTS, part = i - pix * MC_PARTS;
        const int r = pix / MC_HC, c = pix - r * MC_HC;
        const int gy = y0 - 1 + r, gx = x0 - 1 + c;
        u32x4 v = (u32x4){0u, 0u, 0u, 0u};
        if (gy >= 0 && gy < gh && gx >= 0 && gx < gw) {
          float f[8];
          unpack8<DT>(ld16(xi + ((int64_t)gy * w + gx) * cin + c0 + part * 8), f);
#pragma unroll
          for (int e = 0; e < 8; ++e) f[e] *= s_s[c0 + part * 8 + e];
          v = pack8<DT>(f);
        }
        st16(tile + pix * MC_PITCH + part * 8, v);
      }
    }
    __syncthreads();
#pragma unroll 3
    for (int tap = 0; tap < 9; ++tap) {
      const int ty = tap / 3, tx = tap - ty * 3;
#pragma unroll
      for (int ks = 0; ks < MC_KC / 32; ++ks) {
        u32x4 a[RT], bf[MC_CTL];
#pragma unroll
        for (int t = 0; t < RT; ++t) a[t] = ld16(wrow[t] + (int64_t)tap * cin + c0 + ks * 32);
#pragma unroll
        for (int j = 0; j < MC_CTL; ++j) bf[j] = ld16(tile + ((wm * MC_CTL + j + ty) * MC_HC + r16 + tx) * MC_PITCH + ks * 32 + q * 8);
#pragma unroll
        for (int j = 0; j < MC_CTL; ++j) {
          if (!rowlive[j]) continue;
#pragma unroll
          for (int t = 0; t < RT; ++t) acc[t][j] = Elem<DT>::mfma(a[t], bf[j], acc[t][j]);
        }
      }
    }
  }
  const int gx = x0 + r16;
  const int half = cout >> 1;
  const float sqrt2 = 1.41421356237309515f;
  float dm[RT][4], bs[RT][4];  // a lane's output channels are the same in every row: read their demod and bias once
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int o = ct * CT + wn * (CT / 2) + t * 16 + q * 4 + i;
      dm[t][i] = p.demod[(int64_t)img * p.demod_stride + o], bs[t][i] = p.bias[o];
    }
#pragma unroll
  for (int j = 0; j < MC_CTL; ++j) {
    const int gy = y0 + wm * MC_CTL + j;
    if (gy >= gh || gx >= gw) continue;
    const int64_t pix = ((int64_t)img * gh + gy) * gw + gx;
    const float nz = p.noise_weight * p.noise[pix];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int o = ct * CT + wn * (CT / 2) + t * 16 + q * 4;
      float f[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) f[i] = leaky02(((acc[t][j][i] * dm[t][i]) * sqrt2 + nz) + bs[t][i]);
      if (p.sft_scale && o >= half) {  // (16 consecutive channels lie in one half)
        const u32x2 sc = *(const u32x2*)(p.sft_scale + pix * half + (o - half));
        const u32x2 sh = *(const u32x2*)(p.sft_shift + pix * half + (o - half));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float a = Elem<DT>::to_f((u16)((sc[i >> 1] >> ((i & 1) * 16)) & 0xffffu));
          const float c = Elem<DT>::to_f((u16)((sh[i >> 1] >> ((i & 1) * 16)) & 0xffffu));
          f[i] = f[i] * a + c;
        }
      }
      u32x2 v;
      v[0] = pack2<DT>(f[0], f[1]);
      v[1] = pack2<DT>(f[2], f[3]);
      *(u32x2*)(p.y + pix * cout + o) = v;
    }
  }
}

// ---- the composed form of a StyleConv: modulate -> ca_conv3x3 -> style epilogue ---------------------------------------------------------
// y[n, Y, X, c] = round(s[n, c] * X(x)), X = x or its bilinear x2: the tile kernel's staging as a pass of its own (the same arithmetic, one
// rounding).  A thread owns 8 channels of one output pixel.
template <int DT, bool UP>
__global__ __launch_bounds__(256) void k_gfp_modulate(const u16* __restrict__ x, const float* __restrict__ s, int64_t s_stride, u16* __restrict__ y, int64_t total,
                                                      int h, int w, int c, int x_shared) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cl = c >> 3, gh = UP ? 2 * h : h, gw = UP ? 2 * w : w;
  const int j = (int)(idx % cl);
  const int64_t op = idx / cl;
  const int ox = (int)(op % gw), oy = (int)((op / gw) % gh);
  const int64_t img = op / ((int64_t)gw * gh);
  const u16* xi = x + (x_shared ? (int64_t)0 : img * h * w * c) + j * 8;
  float f[8];
  if (UP) {
    int ya, yb, xa, xb;
    float ha, hb, wa, wb;
    up_taps(oy, h, ya, yb, ha, hb);
    up_taps(ox, w, xa, xb, wa, wb);
    float a[8], b[8], cc[8], d[8];
    unpack8<DT>(ld16(xi + ((int64_t)ya * w + xa) * c), a);
    unpack8<DT>(ld16(xi + ((int64_t)ya * w + xb) * c), b);
    unpack8<DT>(ld16(xi + ((int64_t)yb * w + xa) * c), cc);
    unpack8<DT>(ld16(xi + ((int64_t)yb * w + xb) * c), d);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = bilin(a[e], b[e], cc[e], d[e], wa, wb, ha, hb);
  } else {
    unpack8<DT>(ld16(xi + ((int64_t)oy * w + ox) * c), f);
  }
  const float* si = s + img * s_stride + j * 8;
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] *= si[e];
  st16(y + idx * 8, pack8<DT>(f));
}

// the tile kernel's epilogue as a pass of its own, on the convolution's rounded output t (y may be t: a thread reads what it writes)
template <int DT>
__global__ __launch_bounds__(256) void k_gfp_style_epilogue(const u16* t, const float* __restrict__ demod, int64_t demod_stride,
                                                            const float* __restrict__ noise, float noise_weight, const float* __restrict__ bias,
                                                            const u16* __restrict__ sft_scale, const u16* __restrict__ sft_shift, u16* y, int64_t total,
                                                            int64_t hw, int c) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cl = c >> 3, half = c >> 1;
  const int j = (int)(idx % cl), o = j * 8;
  const int64_t pix = idx / cl, img = pix / hw;
  const float sqrt2 = 1.41421356237309515f;
  const float nz = noise_weight * noise[pix];
  float f[8];
  unpack8<DT>(ld16(t + idx * 8), f);
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = leaky02(((f[e] * demod[img * demod_stride + o + e]) * sqrt2 + nz) + bias[o + e]);
  if (sft_scale && o >= half) {
    float a[8], b[8];
    unpack8<DT>(ld16(sft_scale + pix * half + (o - half)), a);
    unpack8<DT>(ld16(sft_shift + pix * half + (o - half)), b);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = f[e] * a[e] + b[e];
  }
  st16(y + idx * 8, pack8<DT>(f));
}

// ---- ToRGB -------------------------------------------------------------------------------------------------------------------------
// a block owns 256 consecutive pixels of one image, a thread one pixel; ws = wt * s of that image in LDS
template <int DT>
__global__ __launch_bounds__(256) void k_gfp_to_rgb(const u16* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ s, int64_t s_stride,
                                                    const float* __restrict__ bias, const float* __restrict__ prev, float* __restrict__ out, int h, int w, int cin,
                                                    int blocks_per_image) {
  __shared__ float ws[3 * 512];
  const int img = blockIdx.x / blocks_per_image;
  const int p = (blockIdx.x - img * blocks_per_image) * 256 + threadIdx.x;
  for (int i = threadIdx.x; i < 3 * cin; i += 256) ws[i] = wt[i] * s[(int64_t)img * s_stride + (i % cin)];
  __syncthreads();
  if (p >= h * w) return;
  const u16* xp = x + ((int64_t)img * h * w + p) * cin;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (int c0 = 0; c0 < cin; c0 += 8) {
    float f[8];
    unpack8<DT>(ld16(xp + c0), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      a0 = fmaf(f[e], ws[c0 + e], a0);
      a1 = fmaf(f[e], ws[cin + c0 + e], a1);
      a2 = fmaf(f[e], ws[2 * cin + c0 + e], a2);
    }
  }
  float r[3] = {a0 + bias[0], a1 + bias[1], a2 + bias[2]};
  if (prev) {
    const int gy = p / w, gx = p - gy * w;
    const int lh = h >> 1, lw = w >> 1;
    int ya, yb, xa, xb;
    float ha, hb, wa, wb;
    up_taps(gy, lh, ya, yb, ha, hb);
    up_taps(gx, lw, xa, xb, wa, wb);
    const float* pi = prev + (int64_t)img * lh * lw * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      r[c] += bilin(pi[((int64_t)ya * lw + xa) * 3 + c], pi[((int64_t)ya * lw + xb) * 3 + c], pi[((int64_t)yb * lw + xa) * 3 + c], pi[((int64_t)yb * lw + xb) * 3 + c],
                    wa, wb, ha, hb);
  }
  float* o = out + ((int64_t)img * h * w + p) * 3;
  o[0] = r[0], o[1] = r[1], o[2] = r[2];
}

// ---- finish ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gfp_finish(const float* __restrict__ pre, uint8_t* __restrict__ out, int64_t pixels, int reverse) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= pixels) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v = pre[p * 3 + c];
    v = !(v > -1.0f) ? -1.0f : (v > 1.0f ? 1.0f : v);  // (a NaN counts as -1)
    v = ((v + 1.0f) / 2.0f) * 255.0f;
    out[p * 3 + (reverse ? 2 - c : c)] = (uint8_t)rintf(v);  // half to even
  }
}

inline bool mc_c_ok(int32_t c) { return c == 64 || c == 128 || c == 256 || c == 512; }

template <int DT>
void launch_modconv(const ModconvP& p, bool up, int rt, dim3 grid, hipStream_t st) {
  if (up) {
    if (rt == 4) hipLaunchKernelGGL((k_gfp_modconv<DT, 4, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((k_gfp_modconv<DT, 2, true>), grid, dim3(256), 0, st, p);
  } else {
    if (rt == 4) hipLaunchKernelGGL((k_gfp_modconv<DT, 4, false>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((k_gfp_modconv<DT, 2, false>), grid, dim3(256), 0, st, p);
  }
}

}  // namespace

extern "C" int ca_gfp_prep(const uint8_t* src, const float* wt, const float* bias, void* y, int32_t images, int32_t h, int32_t w, int32_t cout,
                           int32_t reverse_channels, int32_t dtype, void* stream) {
  CA_REQUIRE(src && wt && bias && y, "ca_gfp_prep: src, wt, bias and y are required");
  CA_REQUIRE(sizes_ok(images, h, w), "ca_gfp_prep: images=%d h=%d w=%d (each >= 1, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE(cout >= 8 && cout % 8 == 0 && cout <= 256, "ca_gfp_prep: cout=%d must be a multiple of 8 in 8 .. 256", cout);
  CA_REQUIRE((int64_t)images * h * w * cout * 2 <= kMaxBytes, "ca_gfp_prep: images=%d h=%d w=%d cout=%d: y would pass 2^31 bytes", images, h, w, cout);
  CA_REQUIRE(reverse_channels == 0 || reverse_channels == 1, "ca_gfp_prep: reverse_channels=%d (0 or 1)", reverse_channels);
  CA_REQUIRE(dtype_ok(dtype), "ca_gfp_prep: dtype %d", dtype);
  CA_REQUIRE(((uintptr_t)y & 15) == 0 && (((uintptr_t)wt | (uintptr_t)bias) & 3) == 0, "ca_gfp_prep: y must be 16-byte aligned, wt and bias 4-byte aligned");
  const int64_t pixels = (int64_t)images * h * w, total = pixels * (cout / 8);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_gfp_prep<DT>, grid, block, 0, (hipStream_t)stream, src, wt, bias, (u16*)y, pixels, (int)cout, (int)reverse_channels));
  CA_CHECK_LAUNCH("ca_gfp_prep");
  return CA_OK;
}

extern "C" int ca_resample2x(const void* x, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t up, int32_t dtype, void* stream) {
  CA_REQUIRE(x && y && x != y, "ca_resample2x: x and y are required and differ");
  CA_REQUIRE(up == 0 || up == 1, "ca_resample2x: up=%d (0 or 1)", up);
  CA_REQUIRE(sizes_ok(images, h, w, up ? 4 : 1), "ca_resample2x: images=%d h=%d w=%d (each >= 1, the larger plane below 2^31 pixels)", images, h, w);
  CA_REQUIRE(up || (h % 2 == 0 && w % 2 == 0), "ca_resample2x: h=%d w=%d must be even for the resize by 1/2", h, w);
  CA_REQUIRE(c >= 8 && c % 8 == 0 && c <= 4096, "ca_resample2x: c=%d must be a multiple of 8 in 8 .. 4096", c);
  CA_REQUIRE((int64_t)images * h * w * (up ? 4 : 1) * c * 2 <= kMaxBytes, "ca_resample2x: images=%d h=%d w=%d c=%d: an operand would pass 2^31 bytes", images, h, w, c);
  CA_REQUIRE(dtype_ok(dtype), "ca_resample2x: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "ca_resample2x: x and y must be 16-byte aligned");
  const int64_t total = up ? (int64_t)images * 4 * h * w * (c / 8) : (int64_t)images * (h / 2) * (w / 2) * (c / 8);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (up) {
    CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_gfp_up2<DT>, grid, block, 0, st, (const u16*)x, (u16*)y, total, (int)h, (int)w, (int)c));
  } else {
    CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_gfp_down2<DT>, grid, block, 0, st, (const u16*)x, (u16*)y, total, (int)h, (int)w, (int)c));
  }
  CA_CHECK_LAUNCH("ca_resample2x");
  return CA_OK;
}

extern "C" int ca_gfp_styles(const float* latents, const float* params, int64_t params_floats, const int32_t* desc, int32_t layers, float* out, int64_t out_stride,
                             int32_t images, int32_t num_latent, void* stream) {
  CA_REQUIRE(latents && params && desc && out, "ca_gfp_styles: latents, params, desc and out are required");
  CA_REQUIRE(layers >= 1 && layers <= GS_MAX_LAYERS, "ca_gfp_styles: layers=%d (1 .. %d)", layers, GS_MAX_LAYERS);
  CA_REQUIRE(images >= 1 && images <= 65536 && num_latent >= 1 && num_latent <= 64, "ca_gfp_styles: images=%d num_latent=%d (1 .. 65536, 1 .. 64)", images, num_latent);
  CA_REQUIRE(params_floats > 0 && out_stride > 0 && out_stride < ((int64_t)1 << 24), "ca_gfp_styles: params_floats=%lld out_stride=%lld", (long long)params_floats,
             (long long)out_stride);
  CA_REQUIRE((((uintptr_t)latents | (uintptr_t)params | (uintptr_t)out) & 3) == 0, "ca_gfp_styles: latents, params and out must be 4-byte aligned");
  StyleDesc d;
  for (int l = 0; l < layers; ++l) {
    const int32_t* e = desc + l * 6;
    const int64_t li = e[0], cin = e[1], cout = e[2], w_off = e[3], wsq_off = e[4], out_off = e[5];
    CA_REQUIRE(li >= 0 && li < num_latent, "ca_gfp_styles: layer %d: latent index %lld outside 0 .. %d", l, (long long)li, num_latent - 1);
    CA_REQUIRE(mc_c_ok((int32_t)cin) && (cout == 0 || mc_c_ok((int32_t)cout)), "ca_gfp_styles: layer %d: cin=%lld cout=%lld (64, 128, 256 or 512; cout 0 for a ToRGB)", l,
               (long long)cin, (long long)cout);
    CA_REQUIRE(w_off >= 0 && w_off + (GS_FEAT + 1) * cin <= params_floats, "ca_gfp_styles: layer %d: w_off=%lld leaves params (%lld floats)", l, (long long)w_off,
               (long long)params_floats);
    CA_REQUIRE(cout == 0 || (wsq_off >= 0 && wsq_off + cin * cout <= params_floats), "ca_gfp_styles: layer %d: wsq_off=%lld leaves params (%lld floats)", l,
               (long long)wsq_off, (long long)params_floats);
    CA_REQUIRE(out_off >= 0 && out_off + cin + cout <= out_stride, "ca_gfp_styles: layer %d: out_off=%lld leaves out_stride=%lld", l, (long long)out_off,
               (long long)out_stride);
    for (int k = 0; k < 6; ++k) d.d[l * 6 + k] = e[k];
  }
  for (int k = layers * 6; k < GS_MAX_LAYERS * 6; ++k) d.d[k] = 0;
  const dim3 grid((unsigned)(images * layers)), block(256);
  hipLaunchKernelGGL(k_gfp_styles, grid, block, 0, (hipStream_t)stream, latents, params, d, out, out_stride, (int)layers, (int)num_latent);
  CA_CHECK_LAUNCH("ca_gfp_styles");
  return CA_OK;
}

extern "C" int ca_modconv3x3(const ca_modconv_args* a, void* stream) {
  CA_REQUIRE(a != nullptr, "ca_modconv3x3: null args");
  CA_REQUIRE(a->x && a->wt && a->s && a->demod && a->noise && a->bias && a->y, "ca_modconv3x3: x, wt, s, demod, noise, bias and y are required");
  CA_REQUIRE((a->sft_scale == nullptr) == (a->sft_shift == nullptr), "ca_modconv3x3: sft_scale and sft_shift come together");
  CA_REQUIRE(a->upsample == 0 || a->upsample == 1, "ca_modconv3x3: upsample=%d (0 or 1)", a->upsample);
  CA_REQUIRE(a->x_shared == 0 || a->x_shared == 1, "ca_modconv3x3: x_shared=%d (0 or 1)", a->x_shared);
  const int64_t up = a->upsample ? 2 : 1;
  CA_REQUIRE(sizes_ok(a->images, a->h, a->w, up * up), "ca_modconv3x3: images=%d h=%d w=%d (each >= 1, the output plane below 2^31 pixels)", a->images, a->h, a->w);
  CA_REQUIRE(mc_c_ok(a->cin) && mc_c_ok(a->cout), "ca_modconv3x3: cin=%d cout=%d (64, 128, 256 or 512)", a->cin, a->cout);
  CA_REQUIRE((int64_t)a->images * a->h * a->w * a->cin * 2 <= kMaxBytes && (int64_t)a->images * a->h * a->w * up * up * a->cout * 2 <= kMaxBytes,
             "ca_modconv3x3: images=%d h=%d w=%d cin=%d cout=%d: an operand would pass 2^31 bytes", a->images, a->h, a->w, a->cin, a->cout);
  CA_REQUIRE(a->s_stride >= 0 && a->s_stride < ((int64_t)1 << 24) && a->demod_stride >= 0 && a->demod_stride < ((int64_t)1 << 24),
             "ca_modconv3x3: s_stride=%lld demod_stride=%lld", (long long)a->s_stride, (long long)a->demod_stride);
  CA_REQUIRE(a->noise_weight == a->noise_weight, "ca_modconv3x3: noise_weight is NaN");
  CA_REQUIRE(dtype_ok(a->dtype), "ca_modconv3x3: dtype %d", a->dtype);
  CA_REQUIRE((((uintptr_t)a->x | (uintptr_t)a->wt | (uintptr_t)a->y | (uintptr_t)a->sft_scale | (uintptr_t)a->sft_shift) & 15) == 0 &&
                 (((uintptr_t)a->s | (uintptr_t)a->demod | (uintptr_t)a->noise | (uintptr_t)a->bias) & 3) == 0 && a->x != a->y,
             "ca_modconv3x3: x, wt, y and sft_* must be 16-byte aligned, s, demod, noise and bias 4-byte aligned, and y must not be x");
  ModconvP p;
  p.x = (const u16*)a->x, p.wt = (const u16*)a->wt, p.sft_scale = (const u16*)a->sft_scale, p.sft_shift = (const u16*)a->sft_shift;
  p.s = a->s, p.demod = a->demod, p.noise = a->noise, p.bias = a->bias, p.y = (u16*)a->y, p.s_stride = a->s_stride, p.demod_stride = a->demod_stride;
  p.h = a->h, p.w = a->w, p.cin = a->cin, p.cout = a->cout, p.gh = (int)(a->h * up), p.gw = (int)(a->w * up);
  p.tiles_x = ceil_div_i(p.gw, MC_TW), p.tiles_y = ceil_div_i(p.gh, MC_TH), p.x_shared = a->x_shared, p.noise_weight = a->noise_weight;
  const int rt = a->cout == 64 ? 2 : 4;
  const int64_t blocks = (int64_t)a->images * p.tiles_x * p.tiles_y * (a->cout / (32 * rt));
  CA_REQUIRE(blocks < ((int64_t)1 << 31), "ca_modconv3x3: grid too large");
  const dim3 grid((unsigned)blocks);
  if (a->dtype == CA_BF16) launch_modconv<CA_BF16>(p, a->upsample != 0, rt, grid, (hipStream_t)stream);
  else launch_modconv<CA_F16>(p, a->upsample != 0, rt, grid, (hipStream_t)stream);
  CA_CHECK_LAUNCH("ca_modconv3x3");
  return CA_OK;
}

extern "C" int ca_gfp_modulate(const void* x, const float* s, int64_t s_stride, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t upsample,
                               int32_t x_shared, int32_t dtype, void* stream) {
  CA_REQUIRE(x && s && y && x != y, "ca_gfp_modulate: x, s and y are required, and y must not be x");
  CA_REQUIRE((upsample == 0 || upsample == 1) && (x_shared == 0 || x_shared == 1), "ca_gfp_modulate: upsample=%d x_shared=%d (0 or 1)", upsample, x_shared);
  const int64_t up = upsample ? 4 : 1;
  CA_REQUIRE(sizes_ok(images, h, w, up), "ca_gfp_modulate: images=%d h=%d w=%d (each >= 1, the output plane below 2^31 pixels)", images, h, w);
  CA_REQUIRE(mc_c_ok(c), "ca_gfp_modulate: c=%d (64, 128, 256 or 512)", c);
  CA_REQUIRE((int64_t)images * h * w * up * c * 2 <= kMaxBytes, "ca_gfp_modulate: images=%d h=%d w=%d c=%d: an operand would pass 2^31 bytes", images, h, w, c);
  CA_REQUIRE(s_stride >= 0 && s_stride < ((int64_t)1 << 24), "ca_gfp_modulate: s_stride=%lld", (long long)s_stride);
  CA_REQUIRE(dtype_ok(dtype), "ca_gfp_modulate: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0 && ((uintptr_t)s & 3) == 0, "ca_gfp_modulate: x and y must be 16-byte aligned, s 4-byte aligned");
  const int64_t total = (int64_t)images * h * w * up * (c / 8);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  const u16* xs = (const u16*)x;
  CA_DISPATCH_DT(dtype, if (upsample) hipLaunchKernelGGL((k_gfp_modulate<DT, true>), grid, block, 0, st, xs, s, s_stride, (u16*)y, total, (int)h, (int)w, (int)c, (int)x_shared);
    else hipLaunchKernelGGL((k_gfp_modulate<DT, false>), grid, block, 0, st, xs, s, s_stride, (u16*)y, total, (int)h, (int)w, (int)c, (int)x_shared));
  CA_CHECK_LAUNCH("ca_gfp_modulate");
  return CA_OK;
}

extern "C" int ca_gfp_style_epilogue(const void* t, const float* demod, int64_t demod_stride, const float* noise, float noise_weight, const float* bias,
                                     const void* sft_scale, const void* sft_shift, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t dtype,
                                     void* stream) {
  CA_REQUIRE(t && demod && noise && bias && y, "ca_gfp_style_epilogue: t, demod, noise, bias and y are required");
  CA_REQUIRE((sft_scale == nullptr) == (sft_shift == nullptr), "ca_gfp_style_epilogue: sft_scale and sft_shift come together");
  CA_REQUIRE(sizes_ok(images, h, w), "ca_gfp_style_epilogue: images=%d h=%d w=%d (each >= 1, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE(mc_c_ok(c), "ca_gfp_style_epilogue: c=%d (64, 128, 256 or 512)", c);
  CA_REQUIRE((int64_t)images * h * w * c * 2 <= kMaxBytes, "ca_gfp_style_epilogue: images=%d h=%d w=%d c=%d: an operand would pass 2^31 bytes", images, h, w, c);
  CA_REQUIRE(demod_stride >= 0 && demod_stride < ((int64_t)1 << 24), "ca_gfp_style_epilogue: demod_stride=%lld", (long long)demod_stride);
  CA_REQUIRE(noise_weight == noise_weight, "ca_gfp_style_epilogue: noise_weight is NaN");
  CA_REQUIRE(dtype_ok(dtype), "ca_gfp_style_epilogue: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)t | (uintptr_t)y | (uintptr_t)sft_scale | (uintptr_t)sft_shift) & 15) == 0 && (((uintptr_t)demod | (uintptr_t)noise | (uintptr_t)bias) & 3) == 0,
             "ca_gfp_style_epilogue: t, y and sft_* must be 16-byte aligned, demod, noise and bias 4-byte aligned");
  const int64_t hw = (int64_t)h * w, total = (int64_t)images * hw * (c / 8);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_gfp_style_epilogue<DT>, grid, block, 0, st, (const u16*)t, demod, demod_stride, noise, noise_weight, bias, (const u16*)sft_scale,
                       (const u16*)sft_shift, (u16*)y, total, hw, (int)c));
  CA_CHECK_LAUNCH("ca_gfp_style_epilogue");
  return CA_OK;
}

extern "C" int ca_gfp_to_rgb(const void* x, const float* wt, const float* s, int64_t s_stride, const float* bias, const float* prev, float* out, int32_t images,
                             int32_t h, int32_t w, int32_t cin, int32_t dtype, void* stream) {
  CA_REQUIRE(x && wt && s && bias && out, "ca_gfp_to_rgb: x, wt, s, bias and out are required");
  CA_REQUIRE(sizes_ok(images, h, w, 3), "ca_gfp_to_rgb: images=%d h=%d w=%d (each >= 1, images * h * w * 3 < 2^31)", images, h, w);
  CA_REQUIRE(!prev || (h % 2 == 0 && w % 2 == 0), "ca_gfp_to_rgb: h=%d w=%d must be even with a previous image", h, w);
  CA_REQUIRE(mc_c_ok(cin), "ca_gfp_to_rgb: cin=%d (64, 128, 256 or 512)", cin);
  CA_REQUIRE((int64_t)images * h * w * cin * 2 <= kMaxBytes, "ca_gfp_to_rgb: images=%d h=%d w=%d cin=%d: x would pass 2^31 bytes", images, h, w, cin);
  CA_REQUIRE(s_stride >= 0 && s_stride < ((int64_t)1 << 24), "ca_gfp_to_rgb: s_stride=%lld", (long long)s_stride);
  CA_REQUIRE(dtype_ok(dtype), "ca_gfp_to_rgb: dtype %d", dtype);
  CA_REQUIRE(((uintptr_t)x & 15) == 0 && (((uintptr_t)wt | (uintptr_t)s | (uintptr_t)bias | (uintptr_t)prev | (uintptr_t)out) & 3) == 0 && prev != out,
             "ca_gfp_to_rgb: x must be 16-byte aligned, the fp32 operands 4-byte aligned, and out must not be prev");
  const int bpi = ceil_div_i((int64_t)h * w, 256);
  const int64_t blocks = (int64_t)images * bpi;
  CA_REQUIRE(blocks < ((int64_t)1 << 31), "ca_gfp_to_rgb: grid too large");
  const dim3 grid((unsigned)blocks), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_gfp_to_rgb<DT>, grid, block, 0, (hipStream_t)stream, (const u16*)x, wt, s, s_stride, bias, prev, out, (int)h, (int)w, (int)cin, bpi));
  CA_CHECK_LAUNCH("ca_gfp_to_rgb");
  return CA_OK;
}

extern "C" int ca_gfp_finish(const float* pre, uint8_t* out, int64_t pixels, int32_t reverse_channels, void* stream) {
  CA_REQUIRE(pre && out, "ca_gfp_finish: pre and out are required");
  CA_REQUIRE(pixels >= 1 && pixels * 3 <= kMaxPixels, "ca_gfp_finish: pixels=%lld (1 .. (2^31 - 1) / 3)", (long long)pixels);
  CA_REQUIRE(reverse_channels == 0 || reverse_channels == 1, "ca_gfp_finish: reverse_channels=%d (0 or 1)", reverse_channels);
  CA_REQUIRE(((uintptr_t)pre & 3) == 0, "ca_gfp_finish: pre must be 4-byte aligned");
  const dim3 grid((unsigned)((pixels + 255) / 256)), block(256);
  hipLaunchKernelGGL(k_gfp_finish, grid, block, 0, (hipStream_t)stream, pre, out, pixels, (int)reverse_channels);
  CA_CHECK_LAUNCH("ca_gfp_finish");
  return CA_OK;
}
