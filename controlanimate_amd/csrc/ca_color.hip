// ABI v15: the 'hm-mkl-hm' colour transfer of the window loop (controlanimate_amd/vid2vid.py: match_colors) as device stages:
// byte histograms, float64 centred moments, the linear map into float64 channel planes, a segmented LSD radix sort of float64
// keys, the rank -> quantile -> reference-value map and the final stretch to uint8.  The 256-entry tables and the 3x3 matrix
// between the stages are computed on the host (controlanimate_amd/color_match.py).
//
// This file is compiled with -ffp-contract=off (controlanimate_amd/_build.py: EXTRA): a * b + c rounds twice, as numpy's does.
// There are no floating-point atomics: every float64 reduction has a fixed order, two runs give the same bits.
#include "ca_common.h"

namespace {

constexpr int kSortTile = 4096;   // keys per block and pass: 4 waves x 16 rounds x 64 lanes
constexpr int kMomBlocks = 64;    // partial sums per image (ca_color_moments_f64)
constexpr int kMmBlocks = 64;     // min / max partials per (image, channel) plane (ca_color_rank_map_f64)
constexpr int64_t kMaxSortPixels = (int64_t)1 << 30;

struct WsLayout {
  int64_t counts, base, mom, mm, total;  // byte offsets; the second key buffer is at 0
  int nblk;
};

inline WsLayout ws_layout(int64_t images, int64_t pixels) {
  WsLayout l;
  const int64_t segs = 3 * images;
  l.nblk = (int)((pixels + kSortTile - 1) / kSortTile);
  l.counts = segs * pixels * 8;
  l.base = l.counts + segs * l.nblk * 256 * 4;
  l.mom = l.base + segs * 256 * 4;
  l.mm = l.mom + images * kMomBlocks * 6 * 8;
  l.total = l.mm + segs * kMmBlocks * 2 * 8;
  return l;
}

inline bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

// ---- histograms ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_hist_u8x3(const uint8_t* __restrict__ src, unsigned* __restrict__ hist, int64_t pixels,
                                                   int64_t per_block) {
  __shared__ unsigned sh[4][768];  // one sub-histogram per wave
  const int tid = threadIdx.x, wave = tid >> 6, img = blockIdx.y;
  for (int b = tid; b < 4 * 768; b += 256) (&sh[0][0])[b] = 0;
  __syncthreads();
  const uint8_t* p = src + (int64_t)img * pixels * 3;
  const int64_t begin = (int64_t)blockIdx.x * per_block;
  const int64_t end = begin + per_block < pixels ? begin + per_block : pixels;
  for (int64_t i = begin + tid; i < end; i += 256) {
    atomicAdd(&sh[wave][p[i * 3]], 1u);
    atomicAdd(&sh[wave][256 + p[i * 3 + 1]], 1u);
    atomicAdd(&sh[wave][512 + p[i * 3 + 2]], 1u);
  }
  __syncthreads();
  for (int b = tid; b < 768; b += 256) {
    const unsigned s = sh[0][b] + sh[1][b] + sh[2][b] + sh[3][b];
    if (s) atomicAdd(&hist[(int64_t)img * 768 + b], s);
  }
}

// ---- centred second moments ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_moments(const uint8_t* __restrict__ src, const double* __restrict__ lut,
                                                 const double* __restrict__ mean, double* __restrict__ part, int64_t pixels) {
  __shared__ double sl[768];
  __shared__ double red[6][256];
  const int tid = threadIdx.x, img = blockIdx.y;
  for (int b = tid; b < 768; b += 256) sl[b] = lut[(int64_t)img * 768 + b];
  __syncthreads();
  const double m0 = mean[img * 3], m1 = mean[img * 3 + 1], m2 = mean[img * 3 + 2];
  const uint8_t* p = src + (int64_t)img * pixels * 3;
  double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < pixels; i += (int64_t)kMomBlocks * 256) {
    const double d0 = sl[p[i * 3]] - m0, d1 = sl[256 + p[i * 3 + 1]] - m1, d2 = sl[512 + p[i * 3 + 2]] - m2;
    a00 += d0 * d0;
    a01 += d0 * d1;
    a02 += d0 * d2;
    a11 += d1 * d1;
    a12 += d1 * d2;
    a22 += d2 * d2;
  }
  red[0][tid] = a00;
  red[1][tid] = a01;
  red[2][tid] = a02;
  red[3][tid] = a11;
  red[4][tid] = a12;
  red[5][tid] = a22;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {  // fixed tree
    if (tid < s) {
#pragma unroll
      for (int j = 0; j < 6; ++j) red[j][tid] += red[j][tid + s];
    }
    __syncthreads();
  }
  if (tid < 6) part[((int64_t)img * kMomBlocks + blockIdx.x) * 6 + tid] = red[tid][0];
}

__global__ __launch_bounds__(64) void k_moments_final(const double* __restrict__ part, double* __restrict__ out) {
  const int img = blockIdx.x, j = threadIdx.x;
  if (j >= 6) return;
  double s = 0;
  for (int b = 0; b < kMomBlocks; ++b) s += part[((int64_t)img * kMomBlocks + b) * 6 + j];  // fixed order
  out[img * 6 + j] = s;
}

// ---- y = (LUT1[a] - mx) @ T + my, into channel planes ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_transform(const uint8_t* __restrict__ src, const double* __restrict__ lut,
                                                   const double* __restrict__ mean, const double* __restrict__ t,
                                                   const double* __restrict__ my, double* __restrict__ y, int64_t pixels) {
  __shared__ double sl[768];
  const int tid = threadIdx.x, img = blockIdx.y;
  for (int b = tid; b < 768; b += 256) sl[b] = lut[(int64_t)img * 768 + b];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  if (i >= pixels) return;
  const uint8_t* p = src + ((int64_t)img * pixels + i) * 3;
  const double d0 = sl[p[0]] - mean[img * 3], d1 = sl[256 + p[1]] - mean[img * 3 + 1], d2 = sl[512 + p[2]] - mean[img * 3 + 2];
  const double* tm = t + img * 9;
#pragma unroll
  for (int j = 0; j < 3; ++j)
    y[((int64_t)img * 3 + j) * pixels + i] = ((d0 * tm[j] + d1 * tm[3 + j]) + d2 * tm[6 + j]) + my[j];
}

// ---- segmented LSD radix sort of float64 keys, 8 passes of 8 bits ------------------------------------------------------------
// order-preserving image of a finite double: negative values have all bits flipped, the others only the sign bit
__device__ __forceinline__ uint64_t key_enc(uint64_t u) { return u ^ ((u >> 63) ? ~0ull : 0x8000000000000000ull); }
__device__ __forceinline__ uint64_t key_dec(uint64_t k) { return k ^ ((k >> 63) ? 0x8000000000000000ull : ~0ull); }

// counts[seg][block][digit] = number of keys of the block's tile with that digit
template <bool ENC>
__global__ __launch_bounds__(256) void k_radix_hist(const uint64_t* __restrict__ src, unsigned* __restrict__ counts, int64_t n,
                                                    int nblk, int shift) {
  __shared__ unsigned h[256];
  const int tid = threadIdx.x, seg = blockIdx.y;
  h[tid] = 0;
  __syncthreads();
  const uint64_t* s = src + (int64_t)seg * n;
  const int64_t tile0 = (int64_t)blockIdx.x * kSortTile;
#pragma unroll 4
  for (int r = 0; r < kSortTile / 256; ++r) {
    const int64_t i = tile0 + r * 256 + tid;
    if (i < n) {
      uint64_t k = s[i];
      if (ENC) k = key_enc(k);
      atomicAdd(&h[(unsigned)(k >> shift) & 255u], 1u);
    }
  }
  __syncthreads();
  counts[((int64_t)seg * nblk + blockIdx.x) * 256 + tid] = h[tid];
}

// per segment: counts[block][digit] -> exclusive prefix over the blocks; base[digit] = exclusive prefix of the digit totals
__global__ __launch_bounds__(256) void k_radix_scan(unsigned* __restrict__ counts, unsigned* __restrict__ base, int nblk) {
  __shared__ unsigned tot[256];
  const int d = threadIdx.x, seg = blockIdx.x;
  unsigned* c = counts + (int64_t)seg * nblk * 256 + d;
  unsigned run = 0;
  for (int b0 = 0; b0 < nblk; b0 += 8) {
    unsigned v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = b0 + j < nblk ? c[(int64_t)(b0 + j) * 256] : 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (b0 + j < nblk) c[(int64_t)(b0 + j) * 256] = run;
      run += v[j];
    }
  }
  tot[d] = run;
  __syncthreads();
  if (d == 0) {
    unsigned acc = 0;
    for (int j = 0; j < 256; ++j) {
      const unsigned t = tot[j];
      tot[j] = acc;
      acc += t;
    }
  }
  __syncthreads();
  base[seg * 256 + d] = tot[d];
}

// stable scatter: a wave owns 1024 consecutive keys of the tile and walks them in 16 rounds of 64; the rank of a key among the
// keys of equal digit in its round comes from 8 ballots, the running offset per (wave, digit) lives in LDS
template <bool ENC, bool DEC>
__global__ __launch_bounds__(256) void k_radix_scatter(const uint64_t* __restrict__ src, uint64_t* __restrict__ dst,
                                                       const unsigned* __restrict__ counts, const unsigned* __restrict__ base,
                                                       int64_t n, int nblk, int shift) {
  __shared__ unsigned woff[4][256];
  constexpr int kRounds = kSortTile / 256;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, seg = blockIdx.y;
  const uint64_t* s = src + (int64_t)seg * n;
  uint64_t* o = dst + (int64_t)seg * n;
  const int64_t w0 = (int64_t)blockIdx.x * kSortTile + (int64_t)wave * (kRounds * 64);
  for (int b = lane; b < 256; b += 64) woff[wave][b] = 0;
  __syncthreads();
  uint64_t k[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int64_t i = w0 + r * 64 + lane;
    k[r] = 0;
    if (i < n) {
      k[r] = s[i];
      if (ENC) k[r] = key_enc(k[r]);
      atomicAdd(&woff[wave][(unsigned)(k[r] >> shift) & 255u], 1u);
    }
  }
  __syncthreads();
  {
    unsigned off = base[seg * 256 + tid] + counts[((int64_t)seg * nblk + blockIdx.x) * 256 + tid];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const unsigned c = woff[w][tid];
      woff[w][tid] = off;
      off += c;
    }
  }
  __syncthreads();
  volatile unsigned* wo = woff[wave];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int64_t i = w0 + r * 64 + lane;
    const bool valid = i < n;
    const unsigned digit = (unsigned)(k[r] >> shift) & 255u;
    unsigned long long mask = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool set = (digit >> bit) & 1u;
      const unsigned long long b = __ballot(set);
      mask &= set ? b : ~b;
    }
    const unsigned rank = __popcll(mask & ((1ull << lane) - 1ull));
    const unsigned cnt = __popcll(mask);
    unsigned off = 0;
    if (valid) off = wo[digit];
    __builtin_amdgcn_wave_barrier();
    if (valid && rank == 0) wo[digit] = off + cnt;
    __builtin_amdgcn_wave_barrier();
    const int64_t pos = (int64_t)off + rank;
    if (valid && pos < n) o[pos] = DEC ? key_dec(k[r]) : k[r];
  }
}

// ---- rank -> quantile -> reference value ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rank_map(const double* y, const double* __restrict__ sorted, double* o,
                                                  const double* __restrict__ kq, const double* __restrict__ kv,
                                                  const int* __restrict__ kn, double* __restrict__ mm, int64_t n) {
  __shared__ double xp[256], fp[256], sl[256];
  __shared__ double rlo[256], rhi[256];
  const int tid = threadIdx.x, plane = blockIdx.y, c = plane % 3;
  int K = kn[c];
  K = K < 1 ? 1 : (K > 256 ? 256 : K);
  if (tid < K) {
    xp[tid] = kq[c * 256 + tid];
    fp[tid] = kv[c * 256 + tid];
  }
  __syncthreads();
  if (tid < K - 1) sl[tid] = (fp[tid + 1] - fp[tid]) / (xp[tid + 1] - xp[tid]);
  __syncthreads();
  const double* s = sorted + (int64_t)plane * n;
  const double dn = (double)n;
  double lo = __builtin_inf(), hi = -__builtin_inf();
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)kMmBlocks * 256) {
    const double v = y[(int64_t)plane * n + i];
    int64_t l = 0, h = n;  // upper bound: the number of keys <= v
    while (l < h) {
      const int64_t m = (l + h) >> 1;
      if (s[m] <= v) l = m + 1; else h = m;
    }
    const double q = (double)l / dn;
    double res;
    if (K == 1 || q < xp[0]) {
      res = fp[0];
    } else if (q >= xp[K - 1]) {
      res = fp[K - 1];
    } else {
      int a = 0, b = K - 1;  // xp[a] <= q < xp[b]
      while (b - a > 1) {
        const int m = (a + b) >> 1;
        if (xp[m] <= q) a = m; else b = m;
      }
      res = xp[a] == q ? fp[a] : sl[a] * (q - xp[a]) + fp[a];
    }
    o[(int64_t)plane * n + i] = res;
    lo = res < lo ? res : lo;
    hi = res > hi ? res : hi;
  }
  rlo[tid] = lo;
  rhi[tid] = hi;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) {
      rlo[tid] = rlo[tid + st] < rlo[tid] ? rlo[tid + st] : rlo[tid];
      rhi[tid] = rhi[tid + st] > rhi[tid] ? rhi[tid + st] : rhi[tid];
    }
    __syncthreads();
  }
  if (tid == 0) {
    mm[((int64_t)plane * kMmBlocks + blockIdx.x) * 2] = rlo[0];
    mm[((int64_t)plane * kMmBlocks + blockIdx.x) * 2 + 1] = rhi[0];
  }
}

// ---- stretch, round, interleave ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_finish_u8(const double* __restrict__ o, uint8_t* __restrict__ dst,
                                                   const double* __restrict__ mm, int64_t n, int normalize) {
  __shared__ double rlo[256], rhi[256];
  const int tid = threadIdx.x, img = blockIdx.y;
  double lo = 0, hi = 0;
  if (normalize) {
    double l = __builtin_inf(), h = -__builtin_inf();
    if (tid < 3 * kMmBlocks) {
      l = mm[((int64_t)img * 3 * kMmBlocks + tid) * 2];
      h = mm[((int64_t)img * 3 * kMmBlocks + tid) * 2 + 1];
    }
    rlo[tid] = l;
    rhi[tid] = h;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if (tid < st) {
        rlo[tid] = rlo[tid + st] < rlo[tid] ? rlo[tid + st] : rlo[tid];
        rhi[tid] = rhi[tid + st] > rhi[tid] ? rhi[tid + st] : rhi[tid];
      }
      __syncthreads();
    }
    lo = rlo[0];
    hi = rhi[0];
  }
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  if (i >= n) return;
  const bool stretch = normalize && hi != lo;
  const double span = hi - lo;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double v = o[((int64_t)img * 3 + c) * n + i];
    if (stretch) v = (v - lo) / span;
    double r = __builtin_rint(v * 255.0);
    r = r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r);
    dst[((int64_t)img * n + i) * 3 + c] = (uint8_t)(int)r;
  }
}

static_assert(3 * kMmBlocks <= 256, "k_finish_u8 reduces the min / max partials of an image with one thread each");

}  // namespace

extern "C" int64_t ca_color_match_workspace_bytes(int32_t images, int64_t pixels) {
  if (images <= 0 || pixels <= 0 || pixels > kMaxSortPixels || images > 65535 / 3) return 0;
  return ws_layout(images, pixels).total;
}

#define CA_COLOR_SIZES(name)                                                                                              \
  CA_REQUIRE(images > 0 && images <= 65535 / 3 && pixels > 0 && pixels <= kMaxSortPixels, name ": images=%d pixels=%lld", images, \
             (long long)pixels)

extern "C" int ca_hist_u8x3(const uint8_t* src, uint32_t* hist, int32_t images, int64_t pixels, void* stream) {
  CA_REQUIRE(src && hist, "ca_hist_u8x3: src and hist are required");
  CA_COLOR_SIZES("ca_hist_u8x3");
  CA_REQUIRE(((uintptr_t)hist & 3) == 0, "ca_hist_u8x3: hist must be 4-byte aligned");
  hipError_t e = hipMemsetAsync(hist, 0, (size_t)images * 768 * 4, (hipStream_t)stream);
  if (e != hipSuccess) CA_FAIL(CA_ERR_LAUNCH, "ca_hist_u8x3: %s", hipGetErrorString(e));
  int64_t blocks = (pixels + 2047) / 2048;
  if (blocks > 256) blocks = 256;
  const int64_t per_block = (pixels + blocks - 1) / blocks;
  hipLaunchKernelGGL(k_hist_u8x3, dim3((unsigned)blocks, images), dim3(256), 0, (hipStream_t)stream, src, (unsigned*)hist, pixels, per_block);
  CA_CHECK_LAUNCH("ca_hist_u8x3");
  return CA_OK;
}

extern "C" int ca_color_moments_f64(const uint8_t* src, const double* lut, const double* mean, double* moments, int32_t images,
                                    int64_t pixels, void* workspace, int64_t workspace_bytes, void* stream) {
  CA_REQUIRE(src && lut && mean && moments, "ca_color_moments_f64: src, lut, mean and moments are required");
  CA_COLOR_SIZES("ca_color_moments_f64");
  CA_REQUIRE(aligned8(lut) && aligned8(mean) && aligned8(moments) && aligned8(workspace), "ca_color_moments_f64: float64 buffers must be 8-byte aligned");
  const WsLayout l = ws_layout(images, pixels);
  CA_REQUIRE(workspace && workspace_bytes >= l.total, "ca_color_moments_f64: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
             (long long)l.total);
  double* part = (double*)((char*)workspace + l.mom);
  hipLaunchKernelGGL(k_moments, dim3(kMomBlocks, images), dim3(256), 0, (hipStream_t)stream, src, lut, mean, part, pixels);
  hipLaunchKernelGGL(k_moments_final, dim3(images), dim3(64), 0, (hipStream_t)stream, (const double*)part, moments);
  CA_CHECK_LAUNCH("ca_color_moments_f64");
  return CA_OK;
}

extern "C" int ca_color_transform_f64(const uint8_t* src, const double* lut, const double* mean, const double* t, const double* my,
                                      double* y, int32_t images, int64_t pixels, void* stream) {
  CA_REQUIRE(src && lut && mean && t && my && y, "ca_color_transform_f64: src, lut, mean, t, my and y are required");
  CA_COLOR_SIZES("ca_color_transform_f64");
  CA_REQUIRE(aligned8(lut) && aligned8(mean) && aligned8(t) && aligned8(my) && aligned8(y), "ca_color_transform_f64: float64 buffers must be 8-byte aligned");
  hipLaunchKernelGGL(k_transform, dim3((unsigned)((pixels + 255) / 256), images), dim3(256), 0, (hipStream_t)stream, src, lut, mean, t, my, y, pixels);
  CA_CHECK_LAUNCH("ca_color_transform_f64");
  return CA_OK;
}

extern "C" int ca_sort_f64_segments(const double* keys, double* sorted, int32_t segments, int64_t n, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  CA_REQUIRE(keys && sorted, "ca_sort_f64_segments: keys and sorted are required");
  CA_REQUIRE(segments > 0 && segments <= 65535 && n > 0 && n <= kMaxSortPixels, "ca_sort_f64_segments: segments=%d n=%lld", segments, (long long)n);
  CA_REQUIRE(aligned8(keys) && aligned8(sorted) && aligned8(workspace), "ca_sort_f64_segments: float64 buffers must be 8-byte aligned");
  const WsLayout l = ws_layout((segments + 2) / 3, n);
  CA_REQUIRE(workspace && workspace_bytes >= l.total, "ca_sort_f64_segments: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
             (long long)l.total);
  uint64_t* tmp = (uint64_t*)workspace;
  uint64_t* out = (uint64_t*)sorted;
  unsigned* counts = (unsigned*)((char*)workspace + l.counts);
  unsigned* base = (unsigned*)((char*)workspace + l.base);
  const dim3 grid(l.nblk, segments), block(256);
  hipStream_t st = (hipStream_t)stream;
  for (int pass = 0; pass < 8; ++pass) {  // keys -> tmp -> sorted -> tmp -> ... -> sorted
    const uint64_t* src = pass == 0 ? (const uint64_t*)keys : ((pass & 1) ? tmp : out);
    uint64_t* dst = (pass & 1) ? out : tmp;
    const int shift = 8 * pass;
    if (pass == 0)
      hipLaunchKernelGGL(k_radix_hist<true>, grid, block, 0, st, src, counts, n, l.nblk, shift);
    else
      hipLaunchKernelGGL(k_radix_hist<false>, grid, block, 0, st, src, counts, n, l.nblk, shift);
    hipLaunchKernelGGL(k_radix_scan, dim3(segments), block, 0, st, counts, base, l.nblk);
    if (pass == 0)
      hipLaunchKernelGGL((k_radix_scatter<true, false>), grid, block, 0, st, src, dst, (const unsigned*)counts, (const unsigned*)base, n, l.nblk, shift);
    else if (pass == 7)
      hipLaunchKernelGGL((k_radix_scatter<false, true>), grid, block, 0, st, src, dst, (const unsigned*)counts, (const unsigned*)base, n, l.nblk, shift);
    else
      hipLaunchKernelGGL((k_radix_scatter<false, false>), grid, block, 0, st, src, dst, (const unsigned*)counts, (const unsigned*)base, n, l.nblk, shift);
  }
  CA_CHECK_LAUNCH("ca_sort_f64_segments");
  return CA_OK;
}

extern "C" int ca_color_rank_map_f64(const double* y, const double* sorted, double* o, const double* knots_q, const double* knots_val,
                                     const int32_t* knots_n, int32_t images, int64_t pixels, void* workspace, int64_t workspace_bytes,
                                     void* stream) {
  CA_REQUIRE(y && sorted && o && knots_q && knots_val && knots_n, "ca_color_rank_map_f64: y, sorted, o and the three knot arrays are required");
  CA_COLOR_SIZES("ca_color_rank_map_f64");
  CA_REQUIRE(sorted != o, "ca_color_rank_map_f64: o may alias y, not sorted");
  CA_REQUIRE(aligned8(y) && aligned8(sorted) && aligned8(o) && aligned8(knots_q) && aligned8(knots_val) && aligned8(workspace),
             "ca_color_rank_map_f64: float64 buffers must be 8-byte aligned");
  const WsLayout l = ws_layout(images, pixels);
  CA_REQUIRE(workspace && workspace_bytes >= l.total, "ca_color_rank_map_f64: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
             (long long)l.total);
  hipLaunchKernelGGL(k_rank_map, dim3(kMmBlocks, 3 * images), dim3(256), 0, (hipStream_t)stream, y, sorted, o, knots_q, knots_val, (const int*)knots_n,
                     (double*)((char*)workspace + l.mm), pixels);
  CA_CHECK_LAUNCH("ca_color_rank_map_f64");
  return CA_OK;
}

extern "C" int ca_color_finish_u8(const double* o, uint8_t* dst, int32_t images, int64_t pixels, int32_t normalize, const void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  CA_REQUIRE(o && dst, "ca_color_finish_u8: o and dst are required");
  CA_COLOR_SIZES("ca_color_finish_u8");
  CA_REQUIRE(normalize == 0 || normalize == 1, "ca_color_finish_u8: normalize=%d (0 or 1)", normalize);
  CA_REQUIRE(aligned8(o) && aligned8(workspace), "ca_color_finish_u8: float64 buffers must be 8-byte aligned");
  const WsLayout l = ws_layout(images, pixels);
  CA_REQUIRE(!normalize || (workspace && workspace_bytes >= l.total), "ca_color_finish_u8: workspace of %lld bytes, %lld needed",
             (long long)workspace_bytes, (long long)l.total);
  const double* mm = normalize ? (const double*)((const char*)workspace + l.mm) : nullptr;
  hipLaunchKernelGGL(k_finish_u8, dim3((unsigned)((pixels + 255) / 256), images), dim3(256), 0, (hipStream_t)stream, o, dst, mm, pixels, (int)normalize);
  CA_CHECK_LAUNCH("ca_color_finish_u8");
  return CA_OK;
}
