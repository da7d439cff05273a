// ABI v14: the Real-ESRGAN RRDBNet (anime-6B) upscaler -- the narrow 3x3 convolution of its 90 dense-block layers and its
// upsampling tail, the uint8 <-> NHWC conversions around the net and the LANCZOS4 resize of `outscale != 4`.
// LeakyReLU lives in this file's own epilogue (ca_common.h's act_f is shared with every other kernel and stays as it is).
#include "ca_common.h"

namespace {

// k_conv3x3n<DT, NT, MT>: one wave computes MT x 16 consecutive output pixels x NT x 16 output channels (all of cout), four
// independent waves per block.  The GEMM is D[cout][pixel] = W[cout][k] . X[k][pixel] with k = (tap, channel): the weight is
// the MFMA's A operand and the pixels its B operand, so that a lane's accumulator holds FOUR CONSECUTIVE CHANNELS of ONE pixel
// (16x16x32 C/D layout: column = lane & 15, rows 4 (lane >> 4) .. +3) and the epilogue stores 8 bytes per lane per tile.
// Operand fragments come straight from global memory (16 bytes per lane: 8 channels of one pixel / one weight row), the
// weight through L2 / L1 shared by the block's waves, which walk the same K sequence.
template <int DT, int NT, int MT>
__global__ __launch_bounds__(256) void k_conv3x3n(const u16* __restrict__ x, const u16* __restrict__ w, void* y,
                                                  const float* __restrict__ bias, const u16* r1, const u16* r2,
                                                  int64_t ldx, int64_t ldy, int64_t ld_r1, int64_t ld_r2,
                                                  int hin, int win, int cin, int cinp, int cout, int npix,
                                                  int cofs, int up, int lrelu, float s0, float s1, float s2, int out_u8) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, kq = (lane >> 4) * 8;
  const int hout = hin << up, wout = win << up;
  const int tile0 = (blockIdx.x * 4 + wave) * (MT * 16);
  if (tile0 >= npix) return;
  int oy[MT], ox[MT], img[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    int p = tile0 + m * 16 + col;
    if (p >= npix) p = -1;
    if (p >= 0) {
      const int hw = hout * wout;
      img[m] = p / hw;
      const int r = p - img[m] * hw;
      oy[m] = r / wout;
      ox[m] = r - oy[m] * wout;
    } else {
      img[m] = 0, oy[m] = -4, ox[m] = -4;  // every tap out of range: zeros, no store
    }
  }
  f32x4 acc[NT][MT];
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[n][m] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const u16* wrow[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) wrow[n] = w + (int64_t)(n * 16 + col) * 9 * cinp + kq;

  for (int tap = 0; tap < 9; ++tap) {
    const int ky = tap / 3, kx = tap - ky * 3;
    int64_t off[MT];  // element offset of this lane's pixel for the tap, -1 = zero padding
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int iy = oy[m] + ky - 1, ix = ox[m] + kx - 1;
      const bool ok = iy >= 0 && iy < hout && ix >= 0 && ix < wout;
      const int sy = iy >> up, sx = ix >> up;
      off[m] = ok ? (int64_t)((img[m] * hin + sy) * win + sx) * ldx + kq : -1;
    }
    for (int c0 = 0; c0 < cin; c0 += 32) {
      u32x4 a[NT], b[MT];
#pragma unroll
      for (int n = 0; n < NT; ++n) a[n] = ld16(wrow[n] + tap * cinp + c0);
      const bool cok = c0 + kq < cin;
#pragma unroll
      for (int m = 0; m < MT; ++m) b[m] = (cok && off[m] >= 0) ? ld16(x + off[m] + c0) : (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
      for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[n][m] = Elem<DT>::mfma(a[n], b[m], acc[n][m]);
    }
  }

  // ---- epilogue: lane holds channels n * 16 + 4 (lane >> 4) + 0..3 of pixel tile0 + m * 16 + col
  const int cq = (lane >> 4) * 4;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int p = tile0 + m * 16 + col;
    if (p >= npix) continue;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int c = n * 16 + cq;
      if (c >= cout) continue;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float t = acc[n][m][r] + (bias ? bias[min(c + r, cout - 1)] : 0.f);
        if (lrelu) t = t > 0.f ? t : 0.2f * t;
        v[r] = s0 * t;
      }
      if (out_u8) {  // cout == 3: clamp to [0, 1], x 255, round half to even, channels reversed
        uint8_t* o = reinterpret_cast<uint8_t*>(y) + (int64_t)p * 3;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const float q = __builtin_rintf(__builtin_amdgcn_fmed3f(v[r], 0.f, 1.f) * 255.f);
          o[2 - r] = (uint8_t)(int)q;
        }
        continue;
      }
      if (r1) {
        const u32x2 q = *reinterpret_cast<const u32x2*>(r1 + (int64_t)p * ld_r1 + c);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += s1 * Elem<DT>::to_f((u16)(q[r >> 1] >> ((r & 1) * 16)));
      }
      if (r2) {
        const u32x2 q = *reinterpret_cast<const u32x2*>(r2 + (int64_t)p * ld_r2 + c);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += s2 * Elem<DT>::to_f((u16)(q[r >> 1] >> ((r & 1) * 16)));
      }
      u32x2 o;
      o[0] = pack2<DT>(v[0], v[1]);
      o[1] = pack2<DT>(v[2], v[3]);
      *reinterpret_cast<u32x2*>(reinterpret_cast<u16*>(y) + (int64_t)p * ldy + cofs + c) = o;
    }
  }
}

template <int DT>
__global__ __launch_bounds__(256) void k_rgb8_to_nhwc(const uint8_t* __restrict__ src, u16* __restrict__ dst, int64_t npix) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const uint8_t* s = src + i * 3;
  float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 3; ++c) f[c] = (float)s[2 - c] / 255.0f;
  st16(dst + i * 8, pack8<DT>(f));
}

__global__ __launch_bounds__(256) void k_resize_lanczos4_u8(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int sh, int sw,
                                                            int dh, int dw, int64_t npix, const int* __restrict__ xofs,
                                                            const short* __restrict__ alpha, const int* __restrict__ yofs,
                                                            const short* __restrict__ beta) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const int dx = (int)(i % dw);
  const int64_t t = i / dw;
  const int dy = (int)(t % dh);
  const int64_t im = t / dh;
  const uint8_t* base = src + im * sh * sw * 3;
  int cx[8];
  int ax[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    cx[j] = min(max(xofs[dx] + j, 0), sw - 1) * 3;
    ax[j] = alpha[dx * 8 + j];
  }
  int acc[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int sy = min(max(yofs[dy] + k, 0), sh - 1);
    const uint8_t* row = base + (int64_t)sy * sw * 3;
    const int b = beta[dy * 8 + k];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int hsum = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) hsum += (int)row[cx[j] + c] * ax[j];
      acc[c] += hsum * b;
    }
  }
  uint8_t* o = dst + i * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = (uint8_t)min(max((acc[c] + (1 << 21)) >> 22, 0), 255);
}

enum NarrowPlan { NP_N64 = 0, NP_N32, NP_N16 };

int narrow_validate(const ca_conv3x3_narrow_args* a, NarrowPlan* plan) {
  CA_REQUIRE(a, "ca_conv3x3_narrow: args is NULL");
  CA_REQUIRE(a->x && a->w && a->y, "ca_conv3x3_narrow: x, w and y are required");
  CA_REQUIRE(a->dtype == CA_F16 || a->dtype == CA_BF16, "ca_conv3x3_narrow: dtype %d (CA_BF16 or CA_F16)", a->dtype);
  CA_REQUIRE(a->images > 0 && a->hin > 0 && a->win > 0, "ca_conv3x3_narrow: images=%d hin=%d win=%d", a->images, a->hin, a->win);
  CA_REQUIRE(a->upsample == 0 || a->upsample == 1, "ca_conv3x3_narrow: upsample=%d (0 or 1)", a->upsample);
  CA_REQUIRE(a->leaky_relu == 0 || a->leaky_relu == 1, "ca_conv3x3_narrow: leaky_relu=%d (0 or 1)", a->leaky_relu);
  CA_REQUIRE(a->cin > 0 && a->cin % 8 == 0, "ca_conv3x3_narrow: cin=%d must be a positive multiple of 8", a->cin);
  CA_REQUIRE(a->ldx >= a->cin && a->ldx % 8 == 0, "ca_conv3x3_narrow: ldx=%lld must be >= cin=%d and a multiple of 8", (long long)a->ldx, a->cin);
  CA_REQUIRE(((uintptr_t)a->x & 15) == 0 && ((uintptr_t)a->w & 15) == 0, "ca_conv3x3_narrow: x and w must be 16-byte aligned");
  const int64_t npix = (int64_t)a->images * (a->hin << a->upsample) * (a->win << a->upsample);
  const int64_t nin = (int64_t)a->images * a->hin * a->win;
  CA_REQUIRE(npix < ((int64_t)1 << 31) && nin < ((int64_t)1 << 31), "ca_conv3x3_narrow: %lld output pixels (must be < 2^31)", (long long)npix);
  if (a->out_u8) {
    CA_REQUIRE(a->out_u8 == 1, "ca_conv3x3_narrow: out_u8=%d (0 or 1)", a->out_u8);
    CA_REQUIRE(a->cout == 3, "ca_conv3x3_narrow: out_u8 needs cout == 3 (got %d)", a->cout);
    CA_REQUIRE(!a->r1 && !a->r2 && a->channel_offset == 0, "ca_conv3x3_narrow: out_u8 takes no residuals and no channel_offset");
    *plan = NP_N16;
    return CA_OK;
  }
  CA_REQUIRE(a->cout == 16 || a->cout == 32 || a->cout == 64, "ca_conv3x3_narrow: cout=%d (16, 32 or 64; 3 only with out_u8)", a->cout);
  CA_REQUIRE(a->channel_offset >= 0 && a->channel_offset % 4 == 0, "ca_conv3x3_narrow: channel_offset=%d must be a non-negative multiple of 4",
             a->channel_offset);
  CA_REQUIRE(a->ldy % 4 == 0 && a->channel_offset + a->cout <= a->ldy, "ca_conv3x3_narrow: channel_offset=%d + cout=%d must be <= ldy=%lld (ldy %% 4 == 0)",
             a->channel_offset, a->cout, (long long)a->ldy);
  CA_REQUIRE(((uintptr_t)a->y & 7) == 0, "ca_conv3x3_narrow: y must be 8-byte aligned");
  CA_REQUIRE(!a->r1 || (a->ld_r1 >= a->cout && a->ld_r1 % 4 == 0 && ((uintptr_t)a->r1 & 7) == 0),
             "ca_conv3x3_narrow: r1 needs ld_r1 >= cout, ld_r1 %% 4 == 0 and 8-byte alignment (ld_r1=%lld)", (long long)a->ld_r1);
  CA_REQUIRE(!a->r2 || (a->ld_r2 >= a->cout && a->ld_r2 % 4 == 0 && ((uintptr_t)a->r2 & 7) == 0),
             "ca_conv3x3_narrow: r2 needs ld_r2 >= cout, ld_r2 %% 4 == 0 and 8-byte alignment (ld_r2=%lld)", (long long)a->ld_r2);
  *plan = a->cout == 64 ? NP_N64 : a->cout == 32 ? NP_N32 : NP_N16;
  return CA_OK;
}

template <int DT, int NT, int MT>
void launch_narrow(const ca_conv3x3_narrow_args* a, hipStream_t st) {
  const int hout = a->hin << a->upsample, wout = a->win << a->upsample;
  const int npix = a->images * hout * wout;
  const int per_block = 4 * MT * 16;
  const int cinp = (a->cin + 31) / 32 * 32;
  hipLaunchKernelGGL((k_conv3x3n<DT, NT, MT>), dim3(ceil_div_i(npix, per_block)), dim3(256), 0, st,
                     (const u16*)a->x, (const u16*)a->w, a->y, a->bias, (const u16*)a->r1, (const u16*)a->r2, (int64_t)a->ldx,
                     (int64_t)a->ldy, (int64_t)a->ld_r1, (int64_t)a->ld_r2, a->hin, a->win, a->cin, cinp, a->cout, npix,
                     a->channel_offset, a->upsample, a->leaky_relu, a->s0, a->s1, a->s2, a->out_u8);
}

template <int DT>
void launch_narrow_dt(const ca_conv3x3_narrow_args* a, NarrowPlan plan, hipStream_t st) {
  if (plan == NP_N64) launch_narrow<DT, 4, 4>(a, st);
  else if (plan == NP_N32) launch_narrow<DT, 2, 8>(a, st);
  else launch_narrow<DT, 1, 8>(a, st);
}

}  // namespace

extern "C" int ca_conv3x3_narrow(const ca_conv3x3_narrow_args* a, void* stream) {
  NarrowPlan plan;
  const int rc = narrow_validate(a, &plan);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (a->dtype == CA_F16) launch_narrow_dt<CA_F16>(a, plan, st);
  else launch_narrow_dt<CA_BF16>(a, plan, st);
  CA_CHECK_LAUNCH("ca_conv3x3_narrow");
  return CA_OK;
}

extern "C" int ca_conv3x3_narrow_plan_name(const ca_conv3x3_narrow_args* a, char* buf, int32_t len) {
  CA_REQUIRE(buf && len > 0, "ca_conv3x3_narrow_plan_name: buffer");
  NarrowPlan plan;
  const int rc = narrow_validate(a, &plan);
  if (rc) return rc;
  snprintf(buf, (size_t)len, "%s", plan == NP_N64 ? "convn_n64m64" : plan == NP_N32 ? "convn_n32m128" : "convn_n16m128");
  return CA_OK;
}

extern "C" int ca_rgb8_to_nhwc(const uint8_t* src, void* dst, int32_t images, int32_t h, int32_t w, int32_t dtype, void* stream) {
  CA_REQUIRE(src && dst, "ca_rgb8_to_nhwc: src and dst are required");
  CA_REQUIRE(images > 0 && h > 0 && w > 0, "ca_rgb8_to_nhwc: images=%d h=%d w=%d", images, h, w);
  CA_REQUIRE(dtype == CA_F16 || dtype == CA_BF16, "ca_rgb8_to_nhwc: dtype %d (CA_BF16 or CA_F16)", dtype);
  CA_REQUIRE(((uintptr_t)dst & 15) == 0, "ca_rgb8_to_nhwc: dst must be 16-byte aligned");
  const int64_t npix = (int64_t)images * h * w;
  const int blocks = ceil_div_i(npix, 256);
  if (dtype == CA_F16)
    hipLaunchKernelGGL(k_rgb8_to_nhwc<CA_F16>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, (u16*)dst, npix);
  else
    hipLaunchKernelGGL(k_rgb8_to_nhwc<CA_BF16>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, (u16*)dst, npix);
  CA_CHECK_LAUNCH("ca_rgb8_to_nhwc");
  return CA_OK;
}

extern "C" int ca_resize_lanczos4_u8(const uint8_t* src, uint8_t* dst, int32_t images, int32_t sh, int32_t sw, int32_t dh, int32_t dw,
                                     const int32_t* xofs, const int16_t* alpha, const int32_t* yofs, const int16_t* beta, void* stream) {
  CA_REQUIRE(src && dst && xofs && alpha && yofs && beta, "ca_resize_lanczos4_u8: src, dst and the four tables are required");
  CA_REQUIRE(images > 0 && sh > 0 && sw > 0 && dh > 0 && dw > 0, "ca_resize_lanczos4_u8: images=%d %dx%d -> %dx%d", images, sh, sw, dh, dw);
  const int64_t npix = (int64_t)images * dh * dw;
  CA_REQUIRE((int64_t)images * sh * sw * 3 < ((int64_t)1 << 40), "ca_resize_lanczos4_u8: source too large");
  hipLaunchKernelGGL(k_resize_lanczos4_u8, dim3(ceil_div_i(npix, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, sh, sw, dh, dw, npix,
                     (const int*)xofs, (const short*)alpha, (const int*)yofs, (const short*)beta);
  CA_CHECK_LAUNCH("ca_resize_lanczos4_u8");
  return CA_OK;
}
