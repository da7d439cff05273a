// What the annotators' translation units share (ca_canny, ca_hed, ca_lineart, ca_lineart_anime, ca_mlsd, ca_softedge, ca_depth,
// ca_normalbae, ca_openpose, ...): the size and dtype guards, the uint8 RGB prep kernel, and the CONTROL TENSOR CONTRACT, stated here once:
//
//   control is [rep * images, 3, H, W], fp32 or fp16 (rep = 2 writes both classifier-free-guidance halves); pixel p of image img
//   goes to ((r * images + img) * 3 + c) * hw + p for every r < rep and c < 3.  The three channels hold the same level unless the
//   kernel says otherwise (k_nbae_finish, k_pose_resolve: one level per channel).  The value is level / 255 with level the uint8 map's value:
//   rounded once by __fdiv_rn in fp32, and for an fp16 tensor once more to fp16.  So control == map.float() / 255 cast to the
//   control dtype, bit for bit.
//
// Header only, templates and inline functions: a kernel is instantiated in the translation unit that launches it.  Some of those are
// compiled with contraction allowed and some with -ffp-contract=off, so nothing here may depend on it: __fdiv_rn and its kin,
// conversions, integer work and stores only, no a * b + c in plain operators.  Include after ca_common.h.
#pragma once
#include "ca_common.h"

// ---- guards ------------------------------------------------------------------------------------------------------------------------
constexpr int64_t kMaxPixels = ((int64_t)1 << 31) - 1;  // pixel counts and linear indices fit int32
constexpr int64_t kMaxBytes = 0x7FFFFF00;               // an operand addressed with 32-bit byte offsets

inline bool sizes_ok(int32_t images, int32_t h, int32_t w, int64_t scale = 1) {
  return images >= 1 && h >= 1 && w >= 1 && (int64_t)images * h * w * scale <= kMaxPixels;
}
inline bool dtype_ok(int32_t dtype) { return dtype == CA_BF16 || dtype == CA_F16; }

// control is aligned for stores of `elems` of its elements (NULL passes: the entry says separately whether it is required)
inline bool ctrl_aligned(const void* control, int32_t control_dtype, int elems) {
  return ((uintptr_t)control & ((control_dtype == CA_F32 ? 4 : 2) * elems - 1)) == 0;
}

// The checks every entry with a control output makes, in their order: h * w % 4 (quads: the entry's kernel stores four pixels per
// thread and has no other rule that implies it), a map or the control tensor present (outputs names the maps in the message; NULL:
// the entry has a rule of its own), rep, control_dtype.  Alignment stays with the entry, which names its own operands.
static inline int control_out_checks(const char* who, bool quads, int32_t h, int32_t w, const char* outputs, bool present, int32_t rep, int32_t control_dtype) {
  CA_REQUIRE(!quads || ((int64_t)h * w) % 4 == 0, "%s: h * w = %d x %d must be a multiple of 4", who, h, w);
  CA_REQUIRE(!outputs || present, "%s: %s or control is required", who, outputs);
  CA_REQUIRE(rep == 1 || rep == 2, "%s: rep=%d (1 or 2)", who, rep);
  CA_REQUIRE(control_dtype == CA_F16 || control_dtype == CA_F32, "%s: control_dtype=%d (CA_F16 or CA_F32)", who, control_dtype);
  return CA_OK;
}

// Runs stmt with T = float or u16 (the bits of an fp16), after control_out_checks
#define CA_DISPATCH_CTRL(control_dtype, ...) \
  do {                                       \
    if ((control_dtype) == CA_F32) {         \
      typedef float T;                       \
      __VA_ARGS__;                           \
    } else {                                 \
      typedef u16 T;                         \
      __VA_ARGS__;                           \
    }                                        \
  } while (0)

// ---- the control tensor ------------------------------------------------------------------------------------------------------------
template <typename T>
struct alignas(4 * sizeof(T)) Vec4 {
  T v[4];
};

__device__ __forceinline__ void ctrl_from_level(int level, float& out) { out = __fdiv_rn((float)level, 255.0f); }
__device__ __forceinline__ void ctrl_from_level(int level, u16& out) { out = Elem<CA_F16>::from_f(__fdiv_rn((float)level, 255.0f)); }

// four consecutive pixels' levels -> the 32-bit word of the uint8 map
__device__ __forceinline__ uint32_t pack_levels4(const int level[4]) {
  return (uint32_t)level[0] | ((uint32_t)level[1] << 8) | ((uint32_t)level[2] << 16) | ((uint32_t)level[3] << 24);
}

// Four consecutive pixels (p % 4 == 0, hw % 4 == 0, ctrl aligned to four elements): v[c] goes to channel c of every rep, one vector
// store each.
template <typename T>
__device__ __forceinline__ void emit_vec4(T* __restrict__ ctrl, int images, int img, int64_t hw, int64_t p, int rep, const Vec4<T> v[3]) {
  for (int r = 0; r < rep; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) *(Vec4<T>*)(ctrl + (((int64_t)r * images + img) * 3 + c) * hw + p) = v[c];
}
// the same four levels in the three channels
template <typename T>
__device__ __forceinline__ void emit_control4(T* __restrict__ ctrl, int images, int img, int64_t hw, int64_t p, int rep, const int level[4]) {
  Vec4<T> v;
#pragma unroll
  for (int i = 0; i < 4; ++i) ctrl_from_level(level[i], v.v[i]);
  const Vec4<T> v3[3] = {v, v, v};
  emit_vec4(ctrl, images, img, hw, p, rep, v3);
}
// one pixel, any alignment: level[c] goes to channel c of every rep
template <typename T>
__device__ __forceinline__ void emit_control1(T* __restrict__ ctrl, int images, int img, int64_t hw, int64_t p, int rep, const int level[3]) {
  T v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) ctrl_from_level(level[c], v[c]);
  for (int r = 0; r < rep; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) ctrl[(((int64_t)r * images + img) * 3 + c) * hw + p] = v[c];
}
// the same level in the three channels
template <typename T>
__device__ __forceinline__ void emit_control1(T* __restrict__ ctrl, int images, int img, int64_t hw, int64_t p, int rep, int level) {
  const int l3[3] = {level, level, level};
  emit_control1(ctrl, images, img, hw, p, rep, l3);
}

// ---- uint8 RGB [n,H,W,3] -> NHWC [n,H,W,8] fp16 / bf16 -------------------------------------------------------------------------------
// F fills the eight channels of a pixel from its three bytes (the first convolution's weight is zero-padded to cin = 8); one 16-byte
// store per pixel.
template <int DT, typename F>
__global__ __launch_bounds__(256) void k_rgb8_prep(const uint8_t* __restrict__ src, u16* __restrict__ dst, int64_t pixels, F fill) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= pixels) return;
  float f[8];
  fill(src + p * 3, f);
  st16(dst + p * 8, pack8<DT>(f));
}

// A prep entry: its checks in their order (operands names the required pointers, align_msg the alignment rule; dst must be 16-byte
// aligned, more_ok is what else the entry asks) and the launch.
template <typename F>
static inline int launch_rgb8_prep(const char* who, const char* operands, bool present, const uint8_t* src, void* dst, int32_t images, int32_t h, int32_t w,
                                   int32_t dtype, bool more_ok, const char* align_msg, void* stream, F fill) {
  CA_REQUIRE(present, "%s: %s are required", who, operands);
  CA_REQUIRE(sizes_ok(images, h, w), "%s: images=%d h=%d w=%d (each >= 1, images * h * w < 2^31)", who, images, h, w);
  CA_REQUIRE(dtype_ok(dtype), "%s: dtype %d", who, dtype);
  CA_REQUIRE(((uintptr_t)dst & 15) == 0 && more_ok, "%s: %s", who, align_msg);
  const int64_t pixels = (int64_t)images * h * w;
  const dim3 grid((unsigned)((pixels + 255) / 256)), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL((k_rgb8_prep<DT, F>), grid, block, 0, (hipStream_t)stream, src, (u16*)dst, pixels, fill));
  CA_CHECK_LAUNCH(who);
  return CA_OK;
}
