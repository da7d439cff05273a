// Added to ABI v16: the memory-bound stages of the HED edge annotator (controlanimate_amd/hed.py: HedAnnotator; the specification is
// tests/hed_ref.py, restated from the published ControlNetHED_Apache2 / HEDdetector).  The thirteen 3x3 convolutions of the VGG
// stack run on ca_conv3x3 with CA_ACT_RELU; around them:
//
//   prep       HedFill          uint8 RGB [n,H,W,3] -> NHWC [n,H,W,8] fp16 / bf16: channel c < 3 = (float)src[c] - norm[c], 3..7 = 0
//                               (the first convolution's weight is zero-padded to cin = 8): one 16-byte store per pixel
//   pool_side  k_hed_pool_side  ONE pass over a block's output [n,h,w,C]: the 1x1 projection to the side map (fp32 [n,h,w], fp32
//                               accumulation) and, unless the block is the last, the 2x2 / stride-2 max pool [n,h/2,w/2,C]
//   fuse       k_hed_fuse       per output pixel: the five side maps sampled as cv2.resize(INTER_LINEAR) samples float32, their fp32
//                               mean, the float64 sigmoid, x 255, truncation -> uint8 [n,H,W] and / or the control tensor
//                               [rep * n,3,H,W] with level / 255 (ca_annot.h)
//
// Compiled with -ffp-contract=off: the bilinear sample is a * w0 + b * w1 with three roundings, as numpy computes it.
// No launch depends on device data on the host side: the chain can be captured in a hipGraph.
#include "ca_common.h"
#include "ca_annot.h"

namespace {

// ---- prep ------------------------------------------------------------------------------------------------------------------------
struct HedFill {
  const float* norm;
  __device__ __forceinline__ void operator()(const uint8_t* s, float f[8]) const {
#pragma unroll
    for (int c = 0; c < 3; ++c) f[c] = (float)s[c] - norm[c];
    f[3] = f[4] = f[5] = f[6] = f[7] = 0.f;
  }
};

// ---- projection + max pool ---------------------------------------------------------------------------------------------------------
// A group of G lanes (G = the power of two >= C / 8, 8 .. 64) owns one 2x2 quad of pixels; lane j of the group holds channels
// 8 j .. 8 j + 7 of its four pixels (four 16-byte loads, consecutive lanes consecutive addresses).  The max of the four goes out as
// one 16-byte store; the four partial dot products are summed over the group by xor shuffles (offsets < G stay inside the aligned
// group) and lane 0 writes them as two 8-byte stores.  Lanes with 8 j >= C load nothing and add zeros.
template <int DT>
__global__ __launch_bounds__(256) void k_hed_pool_side(const u16* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ bias,
                                                       float* __restrict__ side, u16* __restrict__ pooled, int64_t quads, int h2, int w2, int c, int glog) {
  const int g = 1 << glog;
  const int64_t q = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> glog;
  const int j = threadIdx.x & (g - 1);
  const bool live = q < quads && j * 8 < c;
  float d[4] = {0.f, 0.f, 0.f, 0.f};
  int64_t img = 0;
  int y2 = 0, x2 = 0;
  if (q < quads) {
    img = q / ((int64_t)h2 * w2);
    const int r = (int)(q - img * ((int64_t)h2 * w2));
    y2 = r / w2;
    x2 = r - y2 * w2;
  }
  const int w = 2 * w2;
  if (live) {
    float wv[8];
    *(f32x4*)wv = *(const f32x4*)(wp + j * 8);
    *(f32x4*)(wv + 4) = *(const f32x4*)(wp + j * 8 + 4);
    const int64_t p00 = (img * (2 * h2) + 2 * y2) * w + 2 * x2;  // pixel index of the quad's top-left corner
    float m[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t p = p00 + (k >> 1) * w + (k & 1);
      float f[8];
      unpack8<DT>(ld16(x + p * c + j * 8), f);
      float acc = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        acc = fmaf(f[e], wv[e], acc);
        m[e] = k == 0 ? f[e] : fmaxf(m[e], f[e]);
      }
      d[k] = acc;
    }
    if (pooled) st16(pooled + ((img * h2 + y2) * w2 + x2) * c + j * 8, pack8<DT>(m));  // (the max is one of the inputs: the conversion back is exact)
  }
  for (int o = 1; o < g; o <<= 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] += __shfl_xor(d[k], o, 64);
  }
  if (live && j == 0) {
    const float b = bias[0];
    float* s = side + (img * (2 * h2) + 2 * y2) * w + 2 * x2;  // even column, even row length: 8-byte aligned with the base
    *(float2*)s = make_float2(b + d[0], b + d[1]);
    *(float2*)(s + w) = make_float2(b + d[2], b + d[3]);
  }
}

// ---- resize, mean, sigmoid, quantise -------------------------------------------------------------------------------------------------
// cv2.resize(INTER_LINEAR) of a float32 map from (h >> k, w >> k) to (h, w) at destination index d of one axis:
// f = (d + 0.5) * src / dst - 0.5, s = floor(f), f -= s; s < 0 -> s = 0, f = 0; s >= src - 1 -> s = src - 1, f = 0.
__device__ __forceinline__ void lin_coord(int d, int k, int srcn, int& s0, int& s1, float& w0, float& w1) {
  float f = ((float)d + 0.5f) * (1.0f / (float)(1 << k)) - 0.5f;  // exact: a dyadic scale
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) {
    s = 0;
    f = 0.f;
  }
  if (s >= srcn - 1) {
    s = srcn - 1;
    f = 0.f;
  }
  s0 = s;
  s1 = s + 1 < srcn ? s + 1 : srcn - 1;
  w0 = 1.0f - f;
  w1 = f;
}

struct Sides {
  const float* s[5];
};

// 4 consecutive pixels of one row per thread (w % 16 == 0): one 4-byte store to edges, 16 / 8-byte stores to the control tensor
template <typename T>
__global__ __launch_bounds__(256) void k_hed_fuse(Sides sd, uint8_t* __restrict__ edges, T* __restrict__ ctrl, int images, int h, int w, int rep) {
  const int64_t hw = (int64_t)h * w;
  const int64_t g0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (g0 >= images * hw) return;
  const int img = (int)(g0 / hw);
  const int64_t p = g0 - img * hw;
  const int y = (int)(p / w), x0 = (int)(p - (int64_t)y * w);
  float acc[4];
  {
    const f32x4 v = *(const f32x4*)(sd.s[0] + g0);  // level 0 has the output's size: the sample is the value (weights 1 and 0)
    acc[0] = v[0], acc[1] = v[1], acc[2] = v[2], acc[3] = v[3];
  }
#pragma unroll
  for (int k = 1; k < 5; ++k) {
    const int hs = h >> k, ws = w >> k;
    const float* base = sd.s[k] + (int64_t)img * hs * ws;
    int ya, yb;
    float wy0, wy1;
    lin_coord(y, k, hs, ya, yb, wy0, wy1);
    const float* ra = base + (int64_t)ya * ws;
    const float* rb = base + (int64_t)yb * ws;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int xa, xb;
      float wx0, wx1;
      lin_coord(x0 + i, k, ws, xa, xb, wx0, wx1);
      const float top = __fadd_rn(__fmul_rn(ra[xa], wx0), __fmul_rn(ra[xb], wx1));  // columns first,
      const float bot = __fadd_rn(__fmul_rn(rb[xa], wx0), __fmul_rn(rb[xb], wx1));
      const float v = __fadd_rn(__fmul_rn(top, wy0), __fmul_rn(bot, wy1));            // then rows
      acc[i] = __fadd_rn(acc[i], v);
    }
  }
  int level[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double m = (double)__fdiv_rn(acc[i], 5.0f);
    double e = (1.0 / (1.0 + exp(-m))) * 255.0;
    e = e < 0.0 ? 0.0 : (e > 255.0 ? 255.0 : e);
    level[i] = (int)e;  // truncation, as astype(uint8) of a value in [0, 255]
  }
  if (edges) *(uint32_t*)(edges + g0) = pack_levels4(level);
  if (ctrl) emit_control4(ctrl, images, img, hw, p, rep, level);
}

}  // namespace

extern "C" int ca_hed_prep(const uint8_t* src, const float* norm, void* dst, int32_t images, int32_t h, int32_t w, int32_t dtype, void* stream) {
  return launch_rgb8_prep("ca_hed_prep", "src, norm and dst", src && norm && dst, src, dst, images, h, w, dtype, ((uintptr_t)norm & 3) == 0,
                          "dst must be 16-byte aligned, norm 4-byte aligned", stream, HedFill{norm});
}

extern "C" int ca_hed_pool_side(const void* x, const float* proj_w, const float* proj_bias, float* side, void* pooled, int32_t images, int32_t h,
                                int32_t w, int32_t c, int32_t dtype, void* stream) {
  CA_REQUIRE(x && proj_w && proj_bias && side, "ca_hed_pool_side: x, proj_w, proj_bias and side are required (pooled may be NULL)");
  CA_REQUIRE(sizes_ok(images, h, w), "ca_hed_pool_side: images=%d h=%d w=%d (each >= 1, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE(h % 2 == 0 && w % 2 == 0, "ca_hed_pool_side: h=%d w=%d must be even", h, w);
  CA_REQUIRE(c >= 64 && c <= 512 && c % 8 == 0, "ca_hed_pool_side: c=%d must be a multiple of 8 in 64 .. 512", c);
  CA_REQUIRE(dtype_ok(dtype), "ca_hed_pool_side: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)pooled | (uintptr_t)proj_w) & 15) == 0 && ((uintptr_t)side & 7) == 0 && ((uintptr_t)proj_bias & 3) == 0,
             "ca_hed_pool_side: x, pooled and proj_w must be 16-byte aligned, side 8-byte aligned, proj_bias 4-byte aligned");
  int glog = 3;
  while ((8 << glog) < c) ++glog;  // lanes per quad: the power of two >= c / 8
  const int64_t quads = (int64_t)images * (h / 2) * (w / 2);
  const int64_t threads = quads << glog;
  CA_REQUIRE((threads + 255) / 256 < ((int64_t)1 << 31), "ca_hed_pool_side: grid too large");
  const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_hed_pool_side<DT>, grid, block, 0, (hipStream_t)stream, (const u16*)x, proj_w, proj_bias, side, (u16*)pooled, quads, h / 2, w / 2, (int)c, glog));
  CA_CHECK_LAUNCH("ca_hed_pool_side");
  return CA_OK;
}

extern "C" int ca_hed_fuse(const float* side0, const float* side1, const float* side2, const float* side3, const float* side4, int32_t images,
                           int32_t h, int32_t w, uint8_t* edges, void* control, int32_t rep, int32_t control_dtype, void* stream) {
  CA_REQUIRE(side0 && side1 && side2 && side3 && side4, "ca_hed_fuse: the five side maps are required");
  CA_REQUIRE(sizes_ok(images, h, w), "ca_hed_fuse: images=%d h=%d w=%d (each >= 1, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE(h % 16 == 0 && w % 16 == 0, "ca_hed_fuse: h=%d w=%d must be multiples of 16 (five levels, the k-th of (h >> k, w >> k))", h, w);
  if (const int rc = control_out_checks("ca_hed_fuse", false, h, w, "edges", edges || control, rep, control_dtype)) return rc;
  CA_REQUIRE(((uintptr_t)side0 & 15) == 0 && (((uintptr_t)side1 | (uintptr_t)side2 | (uintptr_t)side3 | (uintptr_t)side4) & 3) == 0,
             "ca_hed_fuse: side0 must be 16-byte aligned, the other side maps 4-byte aligned");
  CA_REQUIRE(((uintptr_t)edges & 3) == 0 && ctrl_aligned(control, control_dtype, 4),
             "ca_hed_fuse: edges must be 4-byte aligned, control aligned to four of its elements");
  Sides sd;
  sd.s[0] = side0, sd.s[1] = side1, sd.s[2] = side2, sd.s[3] = side3, sd.s[4] = side4;
  const int64_t total = (int64_t)images * h * w;
  const dim3 grid((unsigned)((total / 4 + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  CA_DISPATCH_CTRL(control_dtype, hipLaunchKernelGGL(k_hed_fuse<T>, grid, block, 0, st, sd, edges, (T*)control, (int)images, (int)h, (int)w, (int)rep));
  CA_CHECK_LAUNCH("ca_hed_fuse");
  return CA_OK;
}
