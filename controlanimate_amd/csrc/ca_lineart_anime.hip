// Added to ABI v16: the lineart_anime annotator (controlanimate_amd/lineart_anime.py: LineartAnimeAnnotator; the specification is
// tests/lineart_anime_ref.py, restated from the published pix2pix UnetGenerator(3, 1, 8, 64, InstanceNorm2d) and controlnet_aux's
// LineartAnimeDetector).  None of the other entry points runs a 4x4 stride-2 convolution, its transpose, or an InstanceNorm at 512
// channels; these do:
//
//   conv_in   k_lanime_conv_in  uint8 RGB [n,H,W,3] -> d0 = Conv4x4s2p1(src / 127.5 - 1) + bias at 64 channels, written twice:
//                               L0 = LeakyReLU(d0) and ReLU(d0) into the first half of C0.  MFMA 16x16x32 with K = 48 padded to 64,
//                               the B operand gathered from an LDS tile of the byte frame.  The zero padding is in the NORMALISED
//                               image: bytes outside the frame count 0 in sum(w * byte), and a second MFMA against the taps' validity
//                               mask gives the sum of the valid taps' weights that is subtracted
//   conv      k_conv_tile<4,2>  Conv2d(k 4, s 2, p 1) as an implicit GEMM: a block owns 8 x 16 output pixels x 128 output channels,
//                               keeps the 18 x 34 input pixels under them in LDS 32 channels at a time (zero outside the image) and
//                               reads its B fragments from there at the 16 taps; the weights [cout][4][4][cin] are the A operand, read
//                               from memory (L2) as fragments.  No im2col tensor.  Optional bias + ReLU (the innermost level)
//             k_im2col4x4s2     the levels with fewer than 4096 output rows are bound by their 8 MB of weights and under-fill the chip
//                               on the tile kernel: kernels.conv4x4s2 runs them as this small gather + ca_gemm (split-K)
//   convt     k_conv_tile<2,1>  ConvTranspose2d(k 4, s 2, p 1) as four 2x2 phase convolutions in ONE launch (the phase is part of the
//                               block index): the same kernel with a 9 x 17 halo (17 x 17 where the plane has 16 rows: a block then owns
//                               16 x 16 source pixels), 64 channels at a time, writing every second pixel
//   instnorm  k_ina_stats,      InstanceNorm2d(affine = False) at 64 .. 512 channels with up to two outputs, each with its own
//             k_ina_apply       activation, channel offset and channel stride: one pass fills L_i and a half of the concatenation
//                               buffer C_i.  Planes of one chunk of pixels (up to 16384 / c pixels: the innermost levels) run as ONE
//                               launch, a block per image; larger ones as statistics + apply over chunks sized to fill the chip
//   conv_out  k_lanime_conv_out 128 -> 1 transposed convolution + bias on the VALU: a thread owns one source pixel and its four output
//                               phases, fp32 weights through the scalar cache, fp32 accumulation in a fixed order
//   finish    k_lanime_finish   255 - trunc(clip(tanh(t) * 127.5 + 127.5)) -> the uint8 map and / or the control tensor (ca_annot.h)
//
// No launch depends on device data on the host side: the chain can be captured in a hipGraph.  No atomics: two runs give the same bits.
#include "ca_common.h"
#include "ca_annot.h"

namespace {

enum { ACT_NONE_ = 0, ACT_RELU_ = 1, ACT_LEAKY_ = 2 };
__device__ __forceinline__ float act3(float v, int act) { return act == ACT_RELU_ ? fmaxf(v, 0.f) : (act == ACT_LEAKY_ ? (v > 0.f ? v : 0.2f * v) : v); }

// ---- input convolution --------------------------------------------------------------------------------------------------------------
// A block owns 16 x 64 output pixels and keeps the 34 x 130 pixels of the byte frame under them in LDS (0 outside the frame).
// k = ky * 12 + kx * 3 + c: for one ky the 12 values of an output pixel are 12 consecutive bytes of a tile row.
constexpr int AI_TH = 16, AI_TW = 64, AI_K = 48, AI_KP = 64;
constexpr int AI_HR = 2 * AI_TH + 2, AI_HC = 2 * AI_TW + 2;
constexpr int AI_PITCH = AI_HC * 3 + 2;

template <int DT>
__global__ __launch_bounds__(256) void k_lanime_conv_in(const uint8_t* __restrict__ src, const u16* __restrict__ wp, const float* __restrict__ bias,
                                                        u16* __restrict__ l0, u16* __restrict__ c0, int H, int W, int tiles_x, int tiles_y) {
  __shared__ uint8_t tile[AI_HR * AI_PITCH];
  const int bx = blockIdx.x % tiles_x;
  const int by = (blockIdx.x / tiles_x) % tiles_y;
  const int img = blockIdx.x / (tiles_x * tiles_y);
  const int h = H >> 1, w = W >> 1;
  const int y0 = by * AI_TH, x0 = bx * AI_TW;
  const uint8_t* s = src + (int64_t)img * H * W * 3;
  for (int i = threadIdx.x; i < AI_HR * AI_HC; i += 256) {
    const int r = i / AI_HC, c = i - r * AI_HC;
    const int gy = 2 * y0 - 1 + r, gx = 2 * x0 - 1 + c;
    uint8_t* t = tile + r * AI_PITCH + c * 3;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const uint8_t* p = s + ((int64_t)gy * W + gx) * 3;
      t[0] = p[0], t[1] = p[1], t[2] = p[2];
    } else {
      t[0] = 0, t[1] = 0, t[2] = 0;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, r16 = lane & 15;
  u32x4 wf[4][2];
  int off[2][8], tky[2][8], tkx[2][8];
  float b4[4][4];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
    for (int t = 0; t < 4; ++t) wf[t][ks] = ld16(wp + (t * 16 + r16) * AI_KP + ks * 32 + q * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = ks * 32 + q * 8 + e;
      const bool live = k < AI_K;  // (the padded columns of the weight are zero: any byte will do, and their mask is 0)
      off[ks][e] = live ? (k / 12) * AI_PITCH + (k % 12) : 0;
      tky[ks][e] = live ? k / 12 : 1 << 20;
      tkx[ks][e] = live ? (k % 12) / 3 : 1 << 20;
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) b4[t][i] = bias[t * 16 + q * 4 + i];
  __syncthreads();
  const u16 one = Elem<DT>::from_f(1.0f);
  for (int it = 0; it < 16; ++it) {
    const int row = wave * 4 + (it >> 2), px = (it & 3) * 16 + r16;
    if (y0 + row >= h || x0 + (it & 3) * 16 >= w) continue;  // wave-uniform
    const uint8_t* base = tile + 2 * row * AI_PITCH + 2 * px * 3;
    const int gy0 = 2 * (y0 + row) - 1, gx0 = 2 * (x0 + px) - 1;
    f32x4 acc[4], wsum[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f}, wsum[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      u32x4 b, m;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        b[e] = pack2<DT>((float)base[off[ks][2 * e]], (float)base[off[ks][2 * e + 1]]);  // 0 .. 255: exact in fp16 and bf16
        const bool v0 = (unsigned)(gy0 + tky[ks][2 * e]) < (unsigned)H && (unsigned)(gx0 + tkx[ks][2 * e]) < (unsigned)W;
        const bool v1 = (unsigned)(gy0 + tky[ks][2 * e + 1]) < (unsigned)H && (unsigned)(gx0 + tkx[ks][2 * e + 1]) < (unsigned)W;
        m[e] = (v0 ? (unsigned)one : 0u) | ((v1 ? (unsigned)one : 0u) << 16);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        acc[t] = Elem<DT>::mfma(wf[t][ks], b, acc[t]);
        wsum[t] = Elem<DT>::mfma(wf[t][ks], m, wsum[t]);
      }
    }
    const int gy = y0 + row, gx = x0 + px;
    if (gx < w) {
      const int64_t pix = ((int64_t)img * h + gy) * w + gx;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        float d[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = (__fdiv_rn(acc[t][i], 127.5f) - wsum[t][i]) + b4[t][i];
        u32x2 a, r;
        a[0] = pack2<DT>(act3(d[0], ACT_LEAKY_), act3(d[1], ACT_LEAKY_));
        a[1] = pack2<DT>(act3(d[2], ACT_LEAKY_), act3(d[3], ACT_LEAKY_));
        r[0] = pack2<DT>(fmaxf(d[0], 0.f), fmaxf(d[1], 0.f));
        r[1] = pack2<DT>(fmaxf(d[2], 0.f), fmaxf(d[3], 0.f));
        *(u32x2*)(l0 + pix * 64 + t * 16 + q * 4) = a;
        *(u32x2*)(c0 + pix * 128 + t * 16 + q * 4) = r;
      }
    }
  }
}

// ---- the 4x4 stride-2 convolution and its transpose: one implicit-GEMM tile kernel ---------------------------------------------------------
// T x T taps at stride S over a grid of gh x gw "positions": the stride-2 convolution has T = 4, S = 2 and its positions are the output
// pixels; a phase (py, px) of the transposed convolution has T = 2, S = 1, its positions are the source pixels (y, x) and it writes output
// pixel (2 y + py, 2 x + px).  Position (y, x) at tap (ty, tx) reads input pixel (S y + oy + ty, S x + ox + tx), zero outside the image
// (oy = ox = -1 for the convolution, py - 1 / px - 1 for a phase).
//
// A block owns 2 CTL x 16 positions (CTL = 4 or 8) and CT = 16 * 2 * RT output channels; its four waves are 2 (halves of the rows) x 2 (halves
// of CT), so a wave reuses a weight fragment for CTL rows and a row fragment for RT weight fragments.  The
// halo of the positions lies in LDS KC input channels at a time, a pixel every KC + 8 elements (the 16 lanes of a fragment row fall on
// different bank groups).  MFMA 16x16x32: A = 16 output channels x 32 input channels of one tap, read from memory; B = the 16 positions
// of one tile row; a lane ends up with 4 consecutive output channels of one position -- one 8-byte store.
constexpr int CV_TW = 16;

template <int DT, int T, int S, int KC, int RT, int CTL>
__global__ __launch_bounds__(256) void k_conv_tile(const u16* __restrict__ x, const u16* __restrict__ wt, const float* __restrict__ bias, u16* __restrict__ y,
                                                   int h, int w, int cin, int cout, int gh, int gw, int tiles_x, int tiles_y, int relu) {
  constexpr int TH = 2 * CTL, HR = (TH - 1) * S + T, HC = (CV_TW - 1) * S + T, PITCH = KC + 8, CT = 32 * RT, PARTS = KC / 8;
  __shared__ __attribute__((aligned(16))) u16 tile[HR * HC * PITCH];
  const int phases = T == 2 ? 4 : 1;
  const int cts = cout / CT;
  int b = blockIdx.x;
  const int ct = b % cts;
  b /= cts;
  const int ph = b % phases;
  b /= phases;
  const int bx = b % tiles_x;
  b /= tiles_x;
  const int by = b % tiles_y;
  const int img = b / tiles_y;
  const int py = T == 2 ? ph >> 1 : 0, px = T == 2 ? ph & 1 : 0;
  const int oy = T == 2 ? py - 1 : -1, ox = T == 2 ? px - 1 : -1;
  const int y0 = by * TH, x0 = bx * CV_TW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, r16 = lane & 15;
  const int wm = wave & 1, wn = wave >> 1;
  const u16* xi = x + (int64_t)img * h * w * cin;
  const u16* wrow[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) wrow[t] = wt + ((int64_t)ph * cout + ct * CT + wn * (CT / 2) + t * 16 + r16) * (T * T) * cin + q * 8;
  f32x4 acc[RT][CTL];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int j = 0; j < CTL; ++j) acc[t][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  bool rowlive[CTL];
#pragma unroll
  for (int j = 0; j < CTL; ++j) rowlive[j] = y0 + wm * CTL + j < gh;  // wave-uniform

  for (int c0 = 0; c0 < cin; c0 += KC) {
    if (c0) __syncthreads();
    for (int i = threadIdx.x; i < HR * HC * PARTS; i += 256) {
      const int pix = i / PARTS, part = i - pix * PARTS;
      const int r = pix / HC, c = pix - r * HC;
      const int gy = S * y0 + oy + r, gx = S * x0 + ox + c;
      u32x4 v = (u32x4){0u, 0u, 0u, 0u};
      if (gy >= 0 && gy < h && gx >= 0 && gx < w) v = ld16(xi + ((int64_t)gy * w + gx) * cin + c0 + part * 8);
      st16(tile + pix * PITCH + part * 8, v);
    }
    __syncthreads();
#pragma unroll 2
    for (int tap = 0; tap < T * T; ++tap) {
      const int ty = tap / T, tx = tap - ty * T;
#pragma unroll
      for (int ks = 0; ks < KC / 32; ++ks) {
        u32x4 a[RT], bf[CTL];
#pragma unroll
        for (int t = 0; t < RT; ++t) a[t] = ld16(wrow[t] + (int64_t)tap * cin + c0 + ks * 32);
#pragma unroll
        for (int j = 0; j < CTL; ++j) bf[j] = ld16(tile + (((wm * CTL + j) * S + ty) * HC + r16 * S + tx) * PITCH + ks * 32 + q * 8);
#pragma unroll
        for (int j = 0; j < CTL; ++j) {
          if (!rowlive[j]) continue;
#pragma unroll
          for (int t = 0; t < RT; ++t) acc[t][j] = Elem<DT>::mfma(a[t], bf[j], acc[t][j]);
        }
      }
    }
  }
  const int OS = T == 2 ? 2 : 1;
  const int oh = gh * OS, ow = gw * OS;
  const int gx = x0 + r16;
#pragma unroll
  for (int j = 0; j < CTL; ++j) {
    const int gy = y0 + wm * CTL + j;
    if (gy >= gh || gx >= gw) continue;
    u16* d = y + (((int64_t)img * oh + gy * OS + py) * ow + gx * OS + px) * cout + ct * CT + wn * (CT / 2) + q * 4;
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      float f[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f[i] = acc[t][j][i];
        if (bias) f[i] += bias[ct * CT + wn * (CT / 2) + t * 16 + q * 4 + i];
        if (relu) f[i] = fmaxf(f[i], 0.f);
      }
      u32x2 v;
      v[0] = pack2<DT>(f[0], f[1]);
      v[1] = pack2<DT>(f[2], f[3]);
      *(u32x2*)(d + t * 16) = v;
    }
  }
}

// ---- the gather in front of ca_gemm for the levels that are bound by their weights ------------------------------------------------------
// cols [images * h/2 * w/2][16 * cin]: column (ky * 4 + kx) * cin + ci of row (img, oy, ox) = x[img, 2 oy - 1 + ky, 2 ox - 1 + kx, ci], zero
// outside the image -- the row order of the weight [cout][4][4][cin].  A thread moves 8 channels of one tap.
__global__ __launch_bounds__(256) void k_im2col4x4s2(const u16* __restrict__ x, u16* __restrict__ cols, int64_t total, int h, int w, int cin) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cl = cin >> 3;
  const int cj = (int)(idx % cl);
  const int tap = (int)((idx / cl) & 15);
  const int64_t op = idx / (cl * 16);
  const int wo = w >> 1, ho = h >> 1;
  const int ox = (int)(op % wo), oy = (int)((op / wo) % ho);
  const int64_t img = op / ((int64_t)wo * ho);
  const int gy = 2 * oy - 1 + (tap >> 2), gx = 2 * ox - 1 + (tap & 3);
  u32x4 v = (u32x4){0u, 0u, 0u, 0u};
  if (gy >= 0 && gy < h && gx >= 0 && gx < w) v = ld16(x + ((img * h + gy) * w + gx) * cin + cj * 8);
  st16(cols + idx * 8, v);
}

// ---- InstanceNorm with up to two activated outputs ------------------------------------------------------------------------------------
// Chunks of pixels per image: a block of either kernel moves at most 512 KiB (4096 pixels at 64 channels, 512 at 512), and less --
// down to 32 KiB -- while the launch has fewer than 256 blocks: the planes from 1/16 of the frame downward are small, and a block per
// image would leave the chip idle.  A function of the arguments alone, so the order of every sum is fixed.
inline int ina_chunk_pixels(int images, int64_t hw, int c) {
  int per = 262144 / c;
  const int per_min = 16384 / c;
  while (per > per_min && (int64_t)images * ((hw + per - 1) / per) < 256) per >>= 1;
  return per;
}
inline int ina_chunks(int images, int64_t hw, int c) {
  const int per = ina_chunk_pixels(images, hw, c);
  return (int)((hw + per - 1) / per);
}

// sum and sum of squares of x - shift over pixels p0 .. p1 - 1 of image `xi` into out[2 * c] (shift = the image's first pixel of that
// channel: var = E[d^2] - E[d]^2 stays free of cancellation when |mean| >> std).  A thread owns 8 channels of every (256 / (c / 8))-th
// pixel; the threads of a channel are added through LDS in thread order.  red: [256 / (c / 8)][2][c] = 4096 floats.
template <int DT>
__device__ __forceinline__ void ina_block_sums(const u16* __restrict__ xi, int p0, int p1, int c, float* red, float* out) {
  const int cl = c >> 3, j = threadIdx.x % cl, pl = threadIdx.x / cl, npl = 256 / cl;
  float k8[8], s[8], ss[8];
  unpack8<DT>(ld16(xi + j * 8), k8);
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = 0.f, ss[e] = 0.f;
  for (int p = p0 + pl; p < p1; p += npl) {
    float f[8];
    unpack8<DT>(ld16(xi + (int64_t)p * c + j * 8), f);
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
  for (int i = threadIdx.x; i < 2 * c; i += 256) {
    float a = 0.f;
    for (int k = 0; k < npl; ++k) a += red[k * 2 * c + i];
    out[i] = a;
  }
}

template <int DT>
__global__ __launch_bounds__(256) void k_ina_stats(const u16* __restrict__ x, float* __restrict__ partials, int hw, int c, int chunks, int per) {
  __shared__ float red[4096];
  const int img = blockIdx.x / chunks, chunk = blockIdx.x - img * chunks;
  const int p0 = chunk * per, p1 = p0 + per < hw ? p0 + per : hw;
  ina_block_sums<DT>(x + (int64_t)img * hw * c, p0, p1, c, red, partials + ((int64_t)img * chunks + chunk) * 2 * c);
}

struct InaOut {
  u16* y[2];
  int act[2], off[2], stride[2];
};

// FUSED: chunks == 1 and the block computes the sums itself (partials unused)
template <int DT, bool FUSED>
__global__ __launch_bounds__(256) void k_ina_apply(const u16* __restrict__ x, const float* __restrict__ partials, InaOut o, int hw, int c, int chunks, int per, float eps) {
  __shared__ float red[FUSED ? 4096 : 1];
  __shared__ float sums[FUSED ? 1024 : 1];
  __shared__ float mean_s[512], rstd_s[512];
  const int img = blockIdx.x / chunks, chunk = blockIdx.x - img * chunks;
  const u16* xi = x + (int64_t)img * hw * c;
  if (FUSED) {
    ina_block_sums<DT>(xi, 0, hw, c, red, sums);
    __syncthreads();
  }
  for (int ch = threadIdx.x; ch < c; ch += 256) {
    float s = 0.f, ss = 0.f;
    if (FUSED) {
      s = sums[ch], ss = sums[c + ch];
    } else {
      const float* p = partials + (int64_t)img * chunks * 2 * c + ch;
      for (int k = 0; k < chunks; ++k) {  // fixed order
        s += p[(int64_t)k * 2 * c];
        ss += p[(int64_t)k * 2 * c + c];
      }
    }
    const float inv = 1.0f / (float)hw;
    const float m = s * inv;
    float var = fmaf(-m, m, ss * inv);  // biased
    var = var > 0.f ? var : 0.f;
    mean_s[ch] = Elem<DT>::to_f(xi[ch]) + m;
    rstd_s[ch] = 1.0f / sqrtf(var + eps);
  }
  __syncthreads();
  const int cl = c >> 3, j = threadIdx.x % cl, pl = threadIdx.x / cl, npl = 256 / cl;
  const int p0 = chunk * per, p1 = p0 + per < hw ? p0 + per : hw;
  float mu[8], rs[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) mu[e] = mean_s[j * 8 + e], rs[e] = rstd_s[j * 8 + e];
  for (int p = p0 + pl; p < p1; p += npl) {
    float f[8];
    unpack8<DT>(ld16(xi + (int64_t)p * c + j * 8), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = (f[e] - mu[e]) * rs[e];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (!o.y[k]) continue;
      float g[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] = act3(f[e], o.act[k]);
      st16(o.y[k] + ((int64_t)img * hw + p) * o.stride[k] + o.off[k] + j * 8, pack8<DT>(g));
    }
  }
}

// ---- output convolution: ConvTranspose2d(128, 1, 4, 2, 1) + bias ------------------------------------------------------------------------
// A block owns 16 x 16 source pixels, a thread one of them and its four output pixels (2 y + py, 2 x + px).  The 18 x 18 source pixels
// around the tile go through LDS in four quarters of 32 channels (a pixel every 80 bytes).  Output phase (py, px) adds, over dy, dx in
// {0, 1}, x[y + py - 1 + dy, x + px - 1 + dx] . W[3 - py - 2 dy][3 - px - 2 dx]: of the 3 x 3 neighbours (sy, sx) of a source pixel,
// phase (py, px) takes those with sy - py and sx - px in {0, 1}.  The weight index is the same in every lane (scalar cache).
constexpr int AO_T = 16, AO_IN = AO_T + 2, AO_PIX = 40;

template <int DT>
__global__ __launch_bounds__(256) void k_lanime_conv_out(const u16* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ bias,
                                                         float* __restrict__ out, int h, int w, int tiles_x, int tiles_y) {
  __shared__ __attribute__((aligned(16))) u16 tile[AO_IN * AO_IN * AO_PIX];
  const int bx = blockIdx.x % tiles_x;
  const int by = (blockIdx.x / tiles_x) % tiles_y;
  const int img = blockIdx.x / (tiles_x * tiles_y);
  const int y0 = by * AO_T, x0 = bx * AO_T;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  const u16* xi = x + (int64_t)img * h * w * 128;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};  // per phase py * 2 + px
  for (int quarter = 0; quarter < 4; ++quarter) {
    if (quarter) __syncthreads();
    for (int i = threadIdx.x; i < AO_IN * AO_IN * 4; i += 256) {
      const int pix = i >> 2, part = i & 3;
      const int r = pix / AO_IN, c = pix - r * AO_IN;
      const int gy = y0 - 1 + r, gx = x0 - 1 + c;
      u32x4 v = (u32x4){0u, 0u, 0u, 0u};
      if (gy >= 0 && gy < h && gx >= 0 && gx < w) v = ld16(xi + ((int64_t)gy * w + gx) * 128 + quarter * 32 + part * 8);
      st16(tile + pix * AO_PIX + part * 8, v);
    }
    __syncthreads();
#pragma unroll
    for (int sy = 0; sy < 3; ++sy)
#pragma unroll
      for (int sx = 0; sx < 3; ++sx) {
        const u16* t = tile + ((ty + sy) * AO_IN + tx + sx) * AO_PIX;
        float f[32];
#pragma unroll
        for (int part = 0; part < 4; ++part) unpack8<DT>(ld16(t + part * 8), f + part * 8);
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
          for (int px = 0; px < 2; ++px) {
            const int dy = sy - py, dx = sx - px;
            if (dy < 0 || dy > 1 || dx < 0 || dx > 1) continue;
            const float* wk = wt + ((3 - py - 2 * dy) * 4 + (3 - px - 2 * dx)) * 128 + quarter * 32;
            float a = acc[py * 2 + px];
#pragma unroll
            for (int e = 0; e < 32; ++e) a = fmaf(f[e], wk[e], a);
            acc[py * 2 + px] = a;
          }
      }
  }
  const int gy = y0 + ty, gx = x0 + tx;
  if (gy < h && gx < w) {
    const float b = bias[0];
    float* o = out + ((int64_t)img * 2 * h + 2 * gy) * (2 * w) + 2 * gx;
    *(f32x2*)o = (f32x2){acc[0] + b, acc[1] + b};
    *(f32x2*)(o + 2 * w) = (f32x2){acc[2] + b, acc[3] + b};
  }
}

// ---- tanh, quantise, invert -------------------------------------------------------------------------------------------------------------
// 4 consecutive pixels per thread (h * w % 4 == 0): one 4-byte store to the map, 16 / 8-byte stores to the control tensor
template <typename T>
__global__ __launch_bounds__(256) void k_lanime_finish(const float* __restrict__ pre, uint8_t* __restrict__ map, T* __restrict__ ctrl, int images, int64_t hw,
                                                       int rep) {
  const int64_t g0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (g0 >= images * hw) return;
  const int img = (int)(g0 / hw);
  const int64_t p = g0 - img * hw;
  const f32x4 v = *(const f32x4*)(pre + g0);
  int level[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double e = tanh((double)v[i]) * 127.5 + 127.5;
    e = !(e > 0.0) ? 0.0 : (e > 255.0 ? 255.0 : e);  // (a NaN counts as 0)
    level[i] = 255 - (int)e;                         // truncation, as astype(uint8) of a value in [0, 255]
  }
  if (map) *(uint32_t*)(map + g0) = pack_levels4(level);
  if (ctrl) emit_control4(ctrl, images, img, hw, p, rep, level);
}

inline bool ina_c_ok(int32_t c) { return c == 64 || c == 128 || c == 256 || c == 512; }
inline bool act_ok(int32_t a) { return a == ACT_NONE_ || a == ACT_RELU_ || a == ACT_LEAKY_; }

template <int DT, int T, int S, int KC, int CTL>
void launch_tile(int rt, dim3 grid, hipStream_t st, const u16* x, const u16* wt, const float* bias, u16* y, int h, int w, int cin, int cout, int gh, int gw, int tx,
                 int ty, int relu) {
  if (rt == 4) hipLaunchKernelGGL((k_conv_tile<DT, T, S, KC, 4, CTL>), grid, dim3(256), 0, st, x, wt, bias, y, h, w, cin, cout, gh, gw, tx, ty, relu);
  else hipLaunchKernelGGL((k_conv_tile<DT, T, S, KC, 2, CTL>), grid, dim3(256), 0, st, x, wt, bias, y, h, w, cin, cout, gh, gw, tx, ty, relu);
}

}  // namespace

extern "C" int ca_lanime_conv_in(const uint8_t* src, const void* w_packed, const float* bias, void* l0, void* c0, int32_t images, int32_t h, int32_t w,
                                 int32_t dtype, void* stream) {
  CA_REQUIRE(src && w_packed && bias && l0 && c0, "ca_lanime_conv_in: src, w_packed, bias, l0 and c0 are required");
  CA_REQUIRE(sizes_ok(images, h, w) && h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0,
             "ca_lanime_conv_in: images=%d h=%d w=%d (images >= 1, h and w even and >= 2, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE((int64_t)images * (h / 2) * (w / 2) * 256 <= kMaxBytes, "ca_lanime_conv_in: images=%d h=%d w=%d: c0 would pass 2^31 bytes", images, h, w);
  CA_REQUIRE(dtype_ok(dtype), "ca_lanime_conv_in: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)w_packed | (uintptr_t)l0 | (uintptr_t)c0) & 15) == 0 && ((uintptr_t)bias & 3) == 0,
             "ca_lanime_conv_in: w_packed, l0 and c0 must be 16-byte aligned, bias 4-byte aligned");
  const int tx = ceil_div_i(w / 2, AI_TW), ty = ceil_div_i(h / 2, AI_TH);
  const int64_t blocks = (int64_t)images * tx * ty;
  CA_REQUIRE(blocks < ((int64_t)1 << 31), "ca_lanime_conv_in: grid too large");
  const dim3 grid((unsigned)blocks), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_lanime_conv_in<DT>, grid, block, 0, (hipStream_t)stream, src, (const u16*)w_packed, bias, (u16*)l0, (u16*)c0, (int)h, (int)w, tx, ty));
  CA_CHECK_LAUNCH("ca_lanime_conv_in");
  return CA_OK;
}

extern "C" int ca_conv4x4s2(const void* x, const void* wt, const float* bias, void* y, int32_t images, int32_t h, int32_t w, int32_t cin, int32_t cout,
                            int32_t relu, int32_t dtype, void* stream) {
  CA_REQUIRE(x && wt && y, "ca_conv4x4s2: x, w and y are required");
  CA_REQUIRE(sizes_ok(images, h, w) && h % 2 == 0 && w % 2 == 0, "ca_conv4x4s2: images=%d h=%d w=%d (images >= 1, h and w even and >= 2, images * h * w < 2^31)",
             images, h, w);
  CA_REQUIRE(cin == 64 || cin == 128 || cin == 256 || cin == 512, "ca_conv4x4s2: cin=%d (64, 128, 256 or 512)", cin);
  CA_REQUIRE(cout == 128 || cout == 256 || cout == 512, "ca_conv4x4s2: cout=%d (128, 256 or 512)", cout);
  CA_REQUIRE((int64_t)images * h * w * cin * 2 <= kMaxBytes && (int64_t)images * (h / 2) * (w / 2) * cout * 2 <= kMaxBytes,
             "ca_conv4x4s2: images=%d h=%d w=%d cin=%d cout=%d: an operand would pass 2^31 bytes", images, h, w, cin, cout);
  CA_REQUIRE(relu == 0 || relu == 1, "ca_conv4x4s2: relu=%d (0 or 1)", relu);
  CA_REQUIRE(dtype_ok(dtype), "ca_conv4x4s2: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)wt | (uintptr_t)y) & 15) == 0 && ((uintptr_t)bias & 3) == 0,
             "ca_conv4x4s2: x, w and y must be 16-byte aligned, bias 4-byte aligned");
  const int gh = h / 2, gw = w / 2;
  const int tx = ceil_div_i(gw, CV_TW), ty = ceil_div_i(gh, 8);
  const int64_t blocks = (int64_t)images * tx * ty * (cout / 128);
  CA_REQUIRE(blocks < ((int64_t)1 << 31), "ca_conv4x4s2: grid too large");
  const dim3 grid((unsigned)blocks);
  CA_DISPATCH_DT(dtype, launch_tile<DT, 4, 2, 32, 4>(4, grid, (hipStream_t)stream, (const u16*)x, (const u16*)wt, bias, (u16*)y, h, w, cin, cout, gh, gw, tx, ty, relu));
  CA_CHECK_LAUNCH("ca_conv4x4s2");
  return CA_OK;
}

extern "C" int ca_im2col4x4s2(const void* x, void* cols, int32_t images, int32_t h, int32_t w, int32_t cin, int32_t dtype, void* stream) {
  CA_REQUIRE(x && cols, "ca_im2col4x4s2: x and cols are required");
  CA_REQUIRE(sizes_ok(images, h, w) && h % 2 == 0 && w % 2 == 0, "ca_im2col4x4s2: images=%d h=%d w=%d (images >= 1, h and w even and >= 2, images * h * w < 2^31)",
             images, h, w);
  CA_REQUIRE(cin >= 8 && cin % 8 == 0 && cin <= 1024, "ca_im2col4x4s2: cin=%d must be a multiple of 8 in 8 .. 1024", cin);
  CA_REQUIRE((int64_t)images * (h / 2) * (w / 2) * 16 * cin * 2 <= kMaxBytes, "ca_im2col4x4s2: images=%d h=%d w=%d cin=%d: cols would pass 2^31 bytes", images, h, w, cin);
  CA_REQUIRE(dtype_ok(dtype), "ca_im2col4x4s2: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)cols) & 15) == 0, "ca_im2col4x4s2: x and cols must be 16-byte aligned");
  const int64_t total = (int64_t)images * (h / 2) * (w / 2) * 16 * (cin / 8);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipLaunchKernelGGL(k_im2col4x4s2, grid, block, 0, (hipStream_t)stream, (const u16*)x, (u16*)cols, total, (int)h, (int)w, (int)cin);
  CA_CHECK_LAUNCH("ca_im2col4x4s2");
  return CA_OK;
}

extern "C" int ca_convt4x4s2(const void* x, const void* w_phase, void* y, int32_t images, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t dtype,
                             void* stream) {
  CA_REQUIRE(x && w_phase && y, "ca_convt4x4s2: x, w_phase and y are required");
  CA_REQUIRE(sizes_ok(images, h, w, 4), "ca_convt4x4s2: images=%d h=%d w=%d (each >= 1, images * 2 h * 2 w < 2^31)", images, h, w);
  CA_REQUIRE(cin == 256 || cin == 512 || cin == 1024, "ca_convt4x4s2: cin=%d (256, 512 or 1024)", cin);
  CA_REQUIRE(cout == 64 || cout == 128 || cout == 256 || cout == 512, "ca_convt4x4s2: cout=%d (64, 128, 256 or 512)", cout);
  CA_REQUIRE((int64_t)images * h * w * cin * 2 <= kMaxBytes && (int64_t)images * h * w * 4 * cout * 2 <= kMaxBytes,
             "ca_convt4x4s2: images=%d h=%d w=%d cin=%d cout=%d: an operand would pass 2^31 bytes", images, h, w, cin, cout);
  CA_REQUIRE(dtype_ok(dtype), "ca_convt4x4s2: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)w_phase | (uintptr_t)y) & 15) == 0, "ca_convt4x4s2: x, w_phase and y must be 16-byte aligned");
  const int rt = cout == 64 ? 2 : 4;
  const int ctl = h >= 16 ? 8 : 4;  // 16 x 16 source pixels per block where the plane has them: a weight fragment then serves 8 rows
  const int tx = ceil_div_i(w, CV_TW), ty = ceil_div_i(h, 2 * ctl);
  const int64_t blocks = (int64_t)images * tx * ty * 4 * (cout / (32 * rt));
  CA_REQUIRE(blocks < ((int64_t)1 << 31), "ca_convt4x4s2: grid too large");
  const dim3 grid((unsigned)blocks);
  hipStream_t st = (hipStream_t)stream;
  const u16 *xs = (const u16*)x, *ws = (const u16*)w_phase;
  CA_DISPATCH_DT(dtype, if (ctl == 8) launch_tile<DT, 2, 1, 64, 8>(rt, grid, st, xs, ws, nullptr, (u16*)y, h, w, cin, cout, h, w, tx, ty, 0);
    else launch_tile<DT, 2, 1, 64, 4>(rt, grid, st, xs, ws, nullptr, (u16*)y, h, w, cin, cout, h, w, tx, ty, 0));
  CA_CHECK_LAUNCH("ca_convt4x4s2");
  return CA_OK;
}

extern "C" int64_t ca_instnorm_act_partials_floats(int32_t images, int32_t h, int32_t w, int32_t c) {
  if (!sizes_ok(images, h, w) || !ina_c_ok(c)) return 0;
  return (int64_t)images * ina_chunks(images, (int64_t)h * w, c) * 2 * c;
}

extern "C" int ca_instnorm_act(const void* x, float* partials, void* y0, int32_t act0, int32_t off0, int32_t stride0, void* y1, int32_t act1, int32_t off1,
                               int32_t stride1, int32_t images, int32_t h, int32_t w, int32_t c, float eps, int32_t dtype, void* stream) {
  CA_REQUIRE(x && partials && y0, "ca_instnorm_act: x, partials and y0 are required");
  CA_REQUIRE(sizes_ok(images, h, w), "ca_instnorm_act: images=%d h=%d w=%d (each >= 1, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE(ina_c_ok(c), "ca_instnorm_act: c=%d (64, 128, 256 or 512)", c);
  CA_REQUIRE(dtype_ok(dtype), "ca_instnorm_act: dtype %d", dtype);
  CA_REQUIRE(eps > 0.f, "ca_instnorm_act: eps=%g must be positive", (double)eps);
  CA_REQUIRE(act_ok(act0) && (!y1 || act_ok(act1)), "ca_instnorm_act: act0=%d act1=%d (0 none, 1 ReLU, 2 LeakyReLU 0.2)", act0, act1);
  CA_REQUIRE(off0 >= 0 && off0 % 8 == 0 && stride0 % 8 == 0 && stride0 >= off0 + c && stride0 <= 4096,
             "ca_instnorm_act: off0=%d stride0=%d (multiples of 8, 0 <= off0, off0 + c <= stride0 <= 4096)", off0, stride0);
  CA_REQUIRE(!y1 || (off1 >= 0 && off1 % 8 == 0 && stride1 % 8 == 0 && stride1 >= off1 + c && stride1 <= 4096),
             "ca_instnorm_act: off1=%d stride1=%d (multiples of 8, 0 <= off1, off1 + c <= stride1 <= 4096)", off1, stride1);
  CA_REQUIRE((int64_t)images * h * w * (y1 && stride1 > stride0 ? stride1 : stride0) * 2 <= kMaxBytes, "ca_instnorm_act: images=%d h=%d w=%d: an output would pass 2^31 bytes",
             images, h, w);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)y0 | (uintptr_t)y1) & 15) == 0 && ((uintptr_t)partials & 3) == 0,
             "ca_instnorm_act: x, y0 and y1 must be 16-byte aligned, partials 4-byte aligned");
  const int hw = h * w;
  const int per = ina_chunk_pixels(images, hw, c), chunks = ina_chunks(images, hw, c);
  CA_REQUIRE((int64_t)images * chunks < ((int64_t)1 << 31), "ca_instnorm_act: grid too large");
  InaOut o;
  o.y[0] = (u16*)y0, o.act[0] = act0, o.off[0] = off0, o.stride[0] = stride0;
  o.y[1] = (u16*)y1, o.act[1] = y1 ? act1 : 0, o.off[1] = y1 ? off1 : 0, o.stride[1] = y1 ? stride1 : 0;
  const dim3 grid((unsigned)((int64_t)images * chunks)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (chunks == 1) {  // one launch: a block per image computes its sums and applies them
    CA_DISPATCH_DT(dtype, hipLaunchKernelGGL((k_ina_apply<DT, true>), grid, block, 0, st, (const u16*)x, (const float*)partials, o, hw, (int)c, 1, per, eps));
  } else {
    CA_DISPATCH_DT(dtype, {
      hipLaunchKernelGGL(k_ina_stats<DT>, grid, block, 0, st, (const u16*)x, partials, hw, (int)c, chunks, per);
      hipLaunchKernelGGL((k_ina_apply<DT, false>), grid, block, 0, st, (const u16*)x, (const float*)partials, o, hw, (int)c, chunks, per, eps);
    });
  }
  CA_CHECK_LAUNCH("ca_instnorm_act");
  return CA_OK;
}

extern "C" int ca_lanime_conv_out(const void* x, const float* wt, const float* bias, float* out, int32_t images, int32_t h, int32_t w, int32_t dtype,
                                  void* stream) {
  CA_REQUIRE(x && wt && bias && out, "ca_lanime_conv_out: x, wt, bias and out are required");
  CA_REQUIRE(sizes_ok(images, h, w, 4), "ca_lanime_conv_out: images=%d h=%d w=%d (each >= 1, images * 2 h * 2 w < 2^31)", images, h, w);
  CA_REQUIRE((int64_t)images * h * w * 256 <= kMaxBytes, "ca_lanime_conv_out: images=%d h=%d w=%d: x would pass 2^31 bytes", images, h, w);
  CA_REQUIRE(dtype_ok(dtype), "ca_lanime_conv_out: dtype %d", dtype);
  CA_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 7) == 0 && (((uintptr_t)wt | (uintptr_t)bias) & 3) == 0,
             "ca_lanime_conv_out: x must be 16-byte aligned, out 8-byte aligned, wt and bias 4-byte aligned");
  const int tx = ceil_div_i(w, AO_T), ty = ceil_div_i(h, AO_T);
  const int64_t blocks = (int64_t)images * tx * ty;
  CA_REQUIRE(blocks < ((int64_t)1 << 31), "ca_lanime_conv_out: grid too large");
  const dim3 grid((unsigned)blocks), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_lanime_conv_out<DT>, grid, block, 0, (hipStream_t)stream, (const u16*)x, wt, bias, out, (int)h, (int)w, tx, ty));
  CA_CHECK_LAUNCH("ca_lanime_conv_out");
  return CA_OK;
}

extern "C" int ca_lanime_finish(const float* pre, int32_t images, int32_t h, int32_t w, uint8_t* map, void* control, int32_t rep, int32_t control_dtype,
                                void* stream) {
  CA_REQUIRE(pre, "ca_lanime_finish: the pre-tanh values are required");
  CA_REQUIRE(sizes_ok(images, h, w), "ca_lanime_finish: images=%d h=%d w=%d (each >= 1, images * h * w < 2^31)", images, h, w);
  if (const int rc = control_out_checks("ca_lanime_finish", true, h, w, "map", map || control, rep, control_dtype)) return rc;
  CA_REQUIRE(((uintptr_t)pre & 15) == 0 && ((uintptr_t)map & 3) == 0 && ctrl_aligned(control, control_dtype, 4),
             "ca_lanime_finish: pre must be 16-byte aligned, map 4-byte aligned, control aligned to four of its elements");
  const int64_t hw = (int64_t)h * w, total = (int64_t)images * hw;
  const dim3 grid((unsigned)((total / 4 + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  CA_DISPATCH_CTRL(control_dtype, hipLaunchKernelGGL(k_lanime_finish<T>, grid, block, 0, st, pre, map, (T*)control, (int)images, hw, (int)rep));
  CA_CHECK_LAUNCH("ca_lanime_finish");
  return CA_OK;
}
