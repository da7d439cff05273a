// Added to ABI v16: the OpenPose body annotator (controlanimate_amd/openpose.py: OpenposeAnnotator; the specification is
// tests/pose_ref.py, restated from the published controlnet_aux open_pose/{__init__,body,util}.py and OpenCV's resize, ellipse2Poly,
// fillConvexPoly and circle).  Beside ca_conv3x3 / ca_maxpool2x2 / ca_gemm the chain needs:
//
//   prep      k_pose_prep       uint8 RGB [n,H,W,3] -> the network's input [n,hp,wp,8]: INTER_AREA resize to hs x ws as a separable weighted sum
//                               (per-axis tables from the host, fp32, fixed order, rounded to a byte half-to-even), BGR order, the
//                               constant-128 padding to multiples of 8 (= 0 after x / 256 - 0.5), channels 3 .. 7 zero
//   conv7     k_conv7           the 7x7 convolutions of the refinement stages as an implicit GEMM: a block owns 8 x 16 output pixels x 64
//                               output channels of one of up to two independent problems (the two branches), keeps the 14 x 22 input pixels
//                               under them in LDS 32 channels at a time (zero outside the image) and reads its B fragments from there at the
//                               49 taps; the weights [cout][7][7][cin] are the A operand, read from memory (L2) as fragments.  No im2col
//                               tensor, no split of the reduction: an output's sum runs over (channel chunk, tap, k) whatever the batch
//             k_im2col7         the gather in front of ca_gemm: the alternative form (context.dispatch.pose_conv7_direct = False)
//   copy      k_copy_cols       a [rows, c] tensor into columns of a wider one (the features into the 192-wide concatenation)
//   maps      k_pose_cols/rows  the x8 LANCZOS4 resize, the crop, the LANCZOS4 resize to the frame and (for the smoothed maps) the sigma-3
//                               Gaussian as ONE matrix per axis, composed on the host in float64: a columns pass and a rows pass in fp32
//   peaks     k_pose_peaks      per (frame, part): the peak test on the smoothed map, ordered (row-major) compaction, capped
//   connect   k_pose_connect    per (frame, limb): float64 candidate scores as body.py writes them, then the stable greedy matching as
//                               at most 64 block-wide arg-max rounds (the first of the sorted list whose ends are both free = the best
//                               free pair, ties to the earlier candidate)
//   assemble  k_pose_assemble   per frame, one wave: the subset table (a lane per row), the deletion rule, the keypoint tables
//   draw      k_pose_raster     per (frame, person, primitive): ellipse2Poly + fillConvexPoly / circle, atomicMax of the draw index
//             k_pose_resolve    the index plane -> colours: the uint8 map and / or the control tensor
//             k_face_raster     ca_pose_draw_faces only: per (frame, person) the 71 radius-3 discs of the face points (ca_openpose_face.hip finds
//                               them) into the same index plane, after that person's body primitives and before the next person's
//
// Every loop of the decode is bounded by a compile-time constant.  No launch depends on device data on the host side: the chain can be
// captured in a hipGraph.  atomicMax / atomicOr only where the result does not depend on the order.
#include "ca_common.h"
#include "ca_annot.h"

namespace {

constexpr int kParts = 18, kLimbs = 19, kDrawLimbs = 17, kPrims = kDrawLimbs + kParts;
constexpr int kFaceParts = CA_FACE_PARTS, kPrimsFace = kPrims + kFaceParts;  // ca_pose_draw_faces: a person's 71 discs follow the body's primitives
constexpr int kMaxPeaks = CA_POSE_MAX_PEAKS, kMaxPeople = CA_POSE_MAX_PEOPLE;
constexpr int kPafCh = 38, kMapCh = 2 * kParts + kPafCh;  // raw heat, smoothed heat, PAF
constexpr int kMidNum = 10;
constexpr int kAreaTaps = CA_POSE_AREA_TAPS;
constexpr int kMaxSide = 2048;
static_assert(kMaxPeople == 64, "k_pose_assemble keeps one subset row per lane of a wave");

__constant__ int c_limb_a[kLimbs] = {1, 1, 2, 3, 5, 6, 1, 8, 9, 1, 11, 12, 1, 0, 14, 0, 15, 2, 5};
__constant__ int c_limb_b[kLimbs] = {2, 5, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 0, 14, 16, 15, 17, 16, 17};
__constant__ int c_paf_x[kLimbs] = {12, 20, 14, 16, 22, 24, 0, 2, 4, 6, 8, 10, 28, 30, 34, 32, 36, 18, 26};
__constant__ unsigned char c_color[kParts][3] = {{255, 0, 0},   {255, 85, 0},  {255, 170, 0}, {255, 255, 0}, {170, 255, 0}, {85, 255, 0},
                                                 {0, 255, 0},   {0, 255, 85},  {0, 255, 170}, {0, 255, 255}, {0, 170, 255}, {0, 85, 255},
                                                 {0, 0, 255},   {85, 0, 255},  {170, 0, 255}, {255, 0, 255}, {255, 0, 170}, {255, 0, 85}};
__constant__ int c_circle_half[5] = {4, 3, 3, 2, 0};  // cv2.circle(radius 4, filled): half width of the row |dy|
__constant__ int c_disc_half[4] = {3, 2, 2, 0};       // ... of radius 3 (draw_facepose)

// ---- prep ---------------------------------------------------------------------------------------------------------------------------
// A thread owns one pixel of the padded input.  ofs / cnt / wgt per destination index of an axis: source index of the first tap, number
// of taps (<= kAreaTaps), fp32 weights.  The horizontal sums come first (left to right), then their vertical sum (top to bottom).
template <int DT>
__global__ __launch_bounds__(256) void k_pose_prep(const uint8_t* __restrict__ src, u16* __restrict__ dst, const int32_t* __restrict__ xofs,
                                                   const int32_t* __restrict__ xcnt, const float* __restrict__ xw, const int32_t* __restrict__ yofs,
                                                   const int32_t* __restrict__ ycnt, const float* __restrict__ yw, int64_t total, int H, int W, int hs, int ws,
                                                   int hp, int wp) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int dx = (int)(idx % wp), dy = (int)((idx / wp) % hp);
  const int64_t img = idx / ((int64_t)wp * hp);
  float v[3] = {0.f, 0.f, 0.f};
  if (dx < ws && dy < hs) {
    const int x0 = xofs[dx], nx = xcnt[dx], y0 = yofs[dy], ny = ycnt[dy];
    float acc[3] = {0.f, 0.f, 0.f};
    for (int j = 0; j < kAreaTaps; ++j) {
      if (j >= ny) break;
      const int sy = y0 + j;
      if (sy < 0 || sy >= H) continue;  // (the host's tables never leave the frame)
      const uint8_t* row = src + ((img * H + sy) * W) * 3;
      float hsum[3] = {0.f, 0.f, 0.f};
      for (int k = 0; k < kAreaTaps; ++k) {
        if (k >= nx) break;
        const int sx = x0 + k;
        if (sx < 0 || sx >= W) continue;
        const float a = xw[dx * kAreaTaps + k];
#pragma unroll
        for (int c = 0; c < 3; ++c) hsum[c] = hsum[c] + a * (float)row[sx * 3 + c];
      }
      const float b = yw[dy * kAreaTaps + j];
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] = acc[c] + b * hsum[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float r = rintf(acc[2 - c]);  // BGR; half to even, as saturate_cast<uchar>(float)
      r = r < 0.f ? 0.f : (r > 255.f ? 255.f : r);
      v[c] = r / 256.0f - 0.5f;
    }
  }
  float f[8] = {v[0], v[1], v[2], 0.f, 0.f, 0.f, 0.f, 0.f};
  st16(dst + idx * 8, pack8<DT>(f));
}

// ---- the 7x7 convolution ------------------------------------------------------------------------------------------------------------
// Stride 1, padding 3.  A block owns 8 x 16 output pixels and 64 output channels of problem blockIdx.z; its four waves are 2 (halves of the
// rows) x 2 (halves of the channels), so a wave reuses a weight fragment for 4 rows and a row fragment for 2 weight fragments.  The halo
// lies in LDS 32 input channels at a time, a pixel every 40 elements (the 16 lanes of a fragment row fall on different bank groups).
// MFMA 16x16x32: A = 16 output channels x 32 input channels of one tap, B = the 16 pixels of one tile row; a lane ends up with 4
// consecutive output channels of one pixel -- one 8-byte store.
constexpr int C7_T = 7, C7_TH = 8, C7_TW = 16, C7_KC = 32, C7_PITCH = C7_KC + 8, C7_CT = 64, C7_CTL = 4, C7_RT = 2;
constexpr int C7_HR = C7_TH + C7_T - 1, C7_HC = C7_TW + C7_T - 1;

struct C7Problems {
  const u16* x[2];
  const u16* w[2];
  const float* bias[2];
  u16* y[2];
};

template <int DT>
__global__ __launch_bounds__(256) void k_conv7(C7Problems p, int h, int w, int cin, int cout, int64_t ldx, int64_t ldy, int tiles_x, int tiles_y, int relu) {
  __shared__ __attribute__((aligned(16))) u16 tile[C7_HR * C7_HC * C7_PITCH];
  const int g = blockIdx.z;
  const u16* __restrict__ x = p.x[g];
  const u16* __restrict__ wt = p.w[g];
  const float* __restrict__ bias = p.bias[g];
  u16* __restrict__ y = p.y[g];
  const int cts = cout / C7_CT;
  int b = blockIdx.x;
  const int ct = b % cts;
  b /= cts;
  const int bx = b % tiles_x;
  b /= tiles_x;
  const int by = b % tiles_y;
  const int img = b / tiles_y;
  const int y0 = by * C7_TH, x0 = bx * C7_TW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, r16 = lane & 15;
  const int wm = wave & 1, wn = wave >> 1;
  const u16* xi = x + (int64_t)img * h * w * ldx;
  const u16* wrow[C7_RT];
#pragma unroll
  for (int t = 0; t < C7_RT; ++t) wrow[t] = wt + ((int64_t)ct * C7_CT + wn * (C7_CT / 2) + t * 16 + r16) * (C7_T * C7_T) * cin + q * 8;
  f32x4 acc[C7_RT][C7_CTL];
#pragma unroll
  for (int t = 0; t < C7_RT; ++t)
#pragma unroll
    for (int j = 0; j < C7_CTL; ++j) acc[t][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  bool rowlive[C7_CTL];
#pragma unroll
  for (int j = 0; j < C7_CTL; ++j) rowlive[j] = y0 + wm * C7_CTL + j < h;  // wave-uniform

  for (int c0 = 0; c0 < cin; c0 += C7_KC) {
    if (c0) __syncthreads();
    for (int i = threadIdx.x; i < C7_HR * C7_HC * (C7_KC / 8); i += 256) {
      const int pix = i / (C7_KC / 8), part = i - pix * (C7_KC / 8);
      const int r = pix / C7_HC, c = pix - r * C7_HC;
      const int gy = y0 - 3 + r, gx = x0 - 3 + c;
      u32x4 v = (u32x4){0u, 0u, 0u, 0u};
      if (gy >= 0 && gy < h && gx >= 0 && gx < w) v = ld16(xi + ((int64_t)gy * w + gx) * ldx + c0 + part * 8);
      st16(tile + pix * C7_PITCH + part * 8, v);
    }
    __syncthreads();
#pragma unroll 7
    for (int tap = 0; tap < C7_T * C7_T; ++tap) {
      const int ty = tap / C7_T, tx = tap - ty * C7_T;
      u32x4 a[C7_RT], bf[C7_CTL];
#pragma unroll
      for (int t = 0; t < C7_RT; ++t) a[t] = ld16(wrow[t] + (int64_t)tap * cin + c0);
#pragma unroll
      for (int j = 0; j < C7_CTL; ++j) bf[j] = ld16(tile + ((wm * C7_CTL + j + ty) * C7_HC + r16 + tx) * C7_PITCH + q * 8);
#pragma unroll
      for (int j = 0; j < C7_CTL; ++j) {
        if (!rowlive[j]) continue;
#pragma unroll
        for (int t = 0; t < C7_RT; ++t) acc[t][j] = Elem<DT>::mfma(a[t], bf[j], acc[t][j]);
      }
    }
  }
  const int gx = x0 + r16;
#pragma unroll
  for (int j = 0; j < C7_CTL; ++j) {
    const int gy = y0 + wm * C7_CTL + j;
    if (gy >= h || gx >= w) continue;
    const int ch0 = ct * C7_CT + wn * (C7_CT / 2) + q * 4;
    u16* d = y + (((int64_t)img * h + gy) * w + gx) * ldy + ch0;
#pragma unroll
    for (int t = 0; t < C7_RT; ++t) {
      float f[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f[i] = acc[t][j][i];
        if (bias) f[i] += bias[ch0 + t * 16 + i];
        if (relu) f[i] = fmaxf(f[i], 0.f);
      }
      u32x2 v;
      v[0] = pack2<DT>(f[0], f[1]);
      v[1] = pack2<DT>(f[2], f[3]);
      *(u32x2*)(d + t * 16) = v;
    }
  }
}

// cols [images * h * w][49 * cin]: column (ky * 7 + kx) * cin + ci of row (img, oy, ox) = x[img, oy - 3 + ky, ox - 3 + kx, ci], zero outside
// the image -- the row order of the weight [cout][7][7][cin].  A thread moves 8 channels of one tap.
__global__ __launch_bounds__(256) void k_im2col7(const u16* __restrict__ x, u16* __restrict__ cols, int64_t total, int h, int w, int cin, int64_t ldx) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cl = cin >> 3;
  const int cj = (int)(idx % cl);
  const int tap = (int)((idx / cl) % 49);
  const int64_t op = idx / ((int64_t)cl * 49);
  const int ox = (int)(op % w), oy = (int)((op / w) % h);
  const int64_t img = op / ((int64_t)w * h);
  const int gy = oy - 3 + tap / 7, gx = ox - 3 + tap % 7;
  u32x4 v = (u32x4){0u, 0u, 0u, 0u};
  if (gy >= 0 && gy < h && gx >= 0 && gx < w) v = ld16(x + ((img * h + gy) * w + gx) * ldx + cj * 8);
  st16(cols + idx * 8, v);
}

__global__ __launch_bounds__(256) void k_copy_cols(const u16* __restrict__ src, u16* __restrict__ dst, int64_t total, int c, int64_t ld, int col0) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cl = c >> 3;
  const int64_t row = idx / cl;
  const int cj = (int)(idx - row * cl);
  st16(dst + row * ld + col0 + cj * 8, ld16(src + idx * 8));
}

// ---- maps ---------------------------------------------------------------------------------------------------------------------------
// low [n, hl, wl, 64] fp32: PAF in columns 0 .. 37, heat in 40 .. 58.  Output channel ch of the 74: 0 .. 17 raw heat (matrix A), 18 .. 35
// smoothed heat (matrix G A), 36 .. 73 PAF (matrix A).  mx [2][W][wl], my [2][H][hl]: A, then G A.  Sums run over the source index upward.
__device__ __forceinline__ void map_channel(int ch, int& col, int& which) {
  if (ch < kParts) col = 40 + ch, which = 0;
  else if (ch < 2 * kParts) col = 40 + ch - kParts, which = 1;
  else col = ch - 2 * kParts, which = 0;
}

__global__ __launch_bounds__(256) void k_pose_cols(const float* __restrict__ low, const float* __restrict__ mx, float* __restrict__ tmp, int64_t total, int hl, int wl,
                                                   int W) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (img, ch, y, X)
  if (idx >= total) return;
  const int X = (int)(idx % W), yy = (int)((idx / W) % hl);
  const int ch = (int)((idx / ((int64_t)W * hl)) % kMapCh);
  const int64_t img = idx / ((int64_t)W * hl * kMapCh);
  int col, which;
  map_channel(ch, col, which);
  const float* m = mx + ((int64_t)which * W + X) * wl;
  const float* s = low + ((img * hl + yy) * wl) * 64 + col;
  float a = 0.f;
  for (int j = 0; j < wl; ++j) a = fmaf(m[j], s[(int64_t)j * 64], a);
  tmp[idx] = a;
}

// A block owns 256 columns of 4 output rows of one (image, channel) plane: no index division, the matrix rows are the same in every lane
// (scalar loads), and a loaded sample serves four outputs.  Each output's sum still runs over the source row upward.
constexpr int kRowsPerThread = 4;
__global__ __launch_bounds__(256) void k_pose_rows(const float* __restrict__ tmp, const float* __restrict__ my, float* __restrict__ raw, float* __restrict__ smooth,
                                                   float* __restrict__ paf, int hl, int H, int W) {
  const int X = blockIdx.x * 256 + threadIdx.x;
  if (X >= W) return;
  const int Y0 = blockIdx.y * kRowsPerThread;
  const int ch = blockIdx.z % kMapCh;
  const int64_t img = blockIdx.z / kMapCh;
  const int which = ch >= kParts && ch < 2 * kParts;
  const float* s = tmp + ((img * kMapCh + ch) * hl) * W + X;
  const float* m[kRowsPerThread];
  float a[kRowsPerThread];
#pragma unroll
  for (int r = 0; r < kRowsPerThread; ++r) {
    const int Y = Y0 + r < H ? Y0 + r : H - 1;
    m[r] = my + ((int64_t)which * H + Y) * hl;
    a[r] = 0.f;
  }
  for (int i = 0; i < hl; ++i) {
    const float v = s[(int64_t)i * W];
#pragma unroll
    for (int r = 0; r < kRowsPerThread; ++r) a[r] = fmaf(m[r][i], v, a[r]);
  }
  const int64_t hw = (int64_t)H * W;
  float* dst = ch < kParts ? raw + (img * kParts + ch) * hw : (ch < 2 * kParts ? smooth + (img * kParts + ch - kParts) * hw : paf + (img * kPafCh + ch - 2 * kParts) * hw);
#pragma unroll
  for (int r = 0; r < kRowsPerThread; ++r)
    if (Y0 + r < H) dst[(int64_t)(Y0 + r) * W + X] = a[r];
}

// ---- peaks --------------------------------------------------------------------------------------------------------------------------
// A block per (part, frame) sweeps the plane in row-major chunks of 256 pixels; the pixels of a chunk that pass are numbered by a prefix
// sum, so the list is in np.nonzero order.  The sweep goes on past the cap only to know whether it was exceeded.
__global__ __launch_bounds__(256) void k_pose_peaks(const float* __restrict__ raw, const float* __restrict__ smooth, int32_t* __restrict__ peaks,
                                                    float* __restrict__ scores, int32_t* __restrict__ counts, int32_t* __restrict__ overflow, int H, int W) {
  __shared__ int wave_sum[4];
  __shared__ int base_s;
  const int part = blockIdx.x, img = blockIdx.y;
  const int64_t hw = (int64_t)H * W;
  const float* sm = smooth + ((int64_t)img * kParts + part) * hw;
  const float* rw = raw + ((int64_t)img * kParts + part) * hw;
  int32_t* pk = peaks + ((int64_t)img * kParts + part) * kMaxPeaks * 2;
  float* sc = scores + ((int64_t)img * kParts + part) * kMaxPeaks;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) base_s = 0;
  __syncthreads();
  const int chunks = (int)((hw + 255) / 256);
  for (int c = 0; c < chunks; ++c) {
    const int64_t p = (int64_t)c * 256 + threadIdx.x;
    bool hit = false;
    int px = 0, py = 0;
    if (p < hw) {
      py = (int)(p / W), px = (int)(p - (int64_t)py * W);
      const float v = sm[p];
      const float up = py > 0 ? sm[p - W] : 0.f, down = py + 1 < H ? sm[p + W] : 0.f;
      const float left = px > 0 ? sm[p - 1] : 0.f, right = px + 1 < W ? sm[p + 1] : 0.f;
      hit = v >= up && v >= down && v >= left && v >= right && (double)v > 0.1;
    }
    const unsigned long long mask = __ballot(hit);
    if (lane == 0) wave_sum[wave] = __popcll(mask);
    __syncthreads();
    int pos = base_s;
    for (int k = 0; k < 4; ++k)
      if (k < wave) pos += wave_sum[k];
    pos += __popcll(mask & ((1ull << lane) - 1ull));
    if (hit && pos < kMaxPeaks) {
      pk[pos * 2] = px, pk[pos * 2 + 1] = py;
      sc[pos] = rw[p];
    }
    __syncthreads();
    if (threadIdx.x == 0) base_s += wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int n = base_s;
    counts[img * kParts + part] = n < kMaxPeaks ? n : kMaxPeaks;
    if (n > kMaxPeaks) atomicOr(overflow + img, CA_POSE_OVERFLOW_PEAKS);
  }
}

// ---- connections --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pose_connect(const float* __restrict__ paf, const int32_t* __restrict__ peaks, const int32_t* __restrict__ counts,
                                                      int32_t* __restrict__ conn_ij, double* __restrict__ conn_score, int32_t* __restrict__ conn_n, int H, int W) {
  __shared__ double score[kMaxPeaks * kMaxPeaks];
  __shared__ double red_s[256];
  __shared__ int red_i[256];
  __shared__ int ax[kMaxPeaks], ay[kMaxPeaks], bx[kMaxPeaks], by[kMaxPeaks];
  __shared__ unsigned char used_a[kMaxPeaks], used_b[kMaxPeaks];
  const int limb = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
  const int pa = c_limb_a[limb], pb = c_limb_b[limb];
  int na = counts[img * kParts + pa], nb = counts[img * kParts + pb];
  na = na < 0 ? 0 : (na > kMaxPeaks ? kMaxPeaks : na);
  nb = nb < 0 ? 0 : (nb > kMaxPeaks ? kMaxPeaks : nb);
  const int64_t hw = (int64_t)H * W;
  const float* fx = paf + ((int64_t)img * kPafCh + c_paf_x[limb]) * hw;
  const float* fy = fx + hw;
  if (tid < kMaxPeaks) {
    const int32_t* a = peaks + (((int64_t)img * kParts + pa) * kMaxPeaks + tid) * 2;
    const int32_t* b = peaks + (((int64_t)img * kParts + pb) * kMaxPeaks + tid) * 2;
    ax[tid] = tid < na ? a[0] : 0, ay[tid] = tid < na ? a[1] : 0;
    bx[tid] = tid < nb ? b[0] : 0, by[tid] = tid < nb ? b[1] : 0;
    used_a[tid] = 0, used_b[tid] = 0;
  }
  __syncthreads();
  const int total = na * nb;
  for (int it = 0; it < kMaxPeaks * kMaxPeaks / 256; ++it) {
    const int c = it * 256 + tid;
    if (c >= total) break;
    const int i = c / nb, j = c - i * nb;
    const int vxi = bx[j] - ax[i], vyi = by[j] - ay[i];
    double norm = sqrt((double)(vxi * vxi + vyi * vyi));
    norm = norm > 0.001 ? norm : 0.001;
    const double ux = (double)vxi / norm, uy = (double)vyi / norm;
    const double stepx = (double)vxi / 9.0, stepy = (double)vyi / 9.0;  // np.linspace(a, b, 10): i * step + a, the last one b
    double sum = 0.0;
    int above = 0;
    for (int s = 0; s < kMidNum; ++s) {
      const double sx = s == kMidNum - 1 ? (double)bx[j] : (double)s * stepx + (double)ax[i];
      const double sy = s == kMidNum - 1 ? (double)by[j] : (double)s * stepy + (double)ay[i];
      int xi = (int)rint(sx), yi = (int)rint(sy);
      xi = xi < 0 ? 0 : (xi >= W ? W - 1 : xi);  // (between two pixels of the frame: never out of it)
      yi = yi < 0 ? 0 : (yi >= H ? H - 1 : yi);
      const double m = (double)fx[(int64_t)yi * W + xi] * ux + (double)fy[(int64_t)yi * W + xi] * uy;
      sum = sum + m;
      above += m > 0.05;
    }
    const double prior = 0.5 * (double)H / norm - 1.0;
    const double sc = sum / 10.0 + (prior < 0.0 ? prior : 0.0);
    score[c] = (above > 8 && sc > 0.0) ? sc : -1.0;  // more than 0.8 * 10 samples
  }
  __syncthreads();
  const int want = na < nb ? na : nb;
  int made = 0;
  int32_t* out_ij = conn_ij + ((int64_t)img * kLimbs + limb) * kMaxPeaks * 2;
  double* out_s = conn_score + ((int64_t)img * kLimbs + limb) * kMaxPeaks;
  for (int round = 0; round < kMaxPeaks; ++round) {
    if (made >= want) break;  // block-uniform
    double best = -1.0;
    int best_c = 0x7fffffff;
    for (int it = 0; it < kMaxPeaks * kMaxPeaks / 256; ++it) {
      const int c = it * 256 + tid;
      if (c >= total) break;
      const double s = score[c];
      if (!(s > 0.0)) continue;
      const int i = c / nb, j = c - i * nb;
      if (used_a[i] || used_b[j]) continue;
      if (s > best) best = s, best_c = c;  // (c ascends: the earlier candidate keeps a tie)
    }
    red_s[tid] = best, red_i[tid] = best_c;
    __syncthreads();
    for (int half = 128; half >= 1; half >>= 1) {
      if (tid < half) {
        const double s2 = red_s[tid + half];
        const int c2 = red_i[tid + half];
        if (s2 > red_s[tid] || (s2 == red_s[tid] && c2 < red_i[tid])) red_s[tid] = s2, red_i[tid] = c2;
      }
      __syncthreads();
    }
    const double win = red_s[0];
    const int win_c = red_i[0];
    __syncthreads();
    if (!(win > 0.0)) break;  // block-uniform: no free pair is left
    if (tid == 0) {
      const int i = win_c / nb, j = win_c - i * nb;
      used_a[i] = 1, used_b[j] = 1;
      out_ij[made * 2] = i, out_ij[made * 2 + 1] = j;
      out_s[made] = win;
    }
    ++made;
    __syncthreads();
  }
  if (tid == 0) conn_n[img * kLimbs + limb] = made;
}

// ---- assembly -----------------------------------------------------------------------------------------------------------------------
// One wave per frame; lane r owns row r of the subset table.  A part's peak i is the id part * 64 + i (the specification numbers the peaks
// across parts; only equality of ids of one part is ever asked).
__global__ __launch_bounds__(64) void k_pose_assemble(const int32_t* __restrict__ peaks, const float* __restrict__ scores, const int32_t* __restrict__ conn_ij,
                                                      const double* __restrict__ conn_score, const int32_t* __restrict__ conn_n, int32_t* __restrict__ keypoints,
                                                      int32_t* __restrict__ coords, int32_t* __restrict__ people, int32_t* __restrict__ overflow, int H, int W) {
  __shared__ int ids[kMaxPeople][kParts];
  __shared__ double total[kMaxPeople];
  __shared__ int parts_n[kMaxPeople];
  const int img = blockIdx.x, lane = threadIdx.x;
  const float* sc = scores + (int64_t)img * kParts * kMaxPeaks;
  int rows = 0;  // wave-uniform
  bool over = false;
  for (int k = 0; k < kLimbs; ++k) {
    const int a = c_limb_a[k], b = c_limb_b[k];
    int nc = conn_n[img * kLimbs + k];
    nc = nc < 0 ? 0 : (nc > kMaxPeaks ? kMaxPeaks : nc);
    const int32_t* cij = conn_ij + ((int64_t)img * kLimbs + k) * kMaxPeaks * 2;
    const double* cs = conn_score + ((int64_t)img * kLimbs + k) * kMaxPeaks;
    for (int c = 0; c < kMaxPeaks; ++c) {
      if (c >= nc) break;
      const int ia = cij[c * 2] & (kMaxPeaks - 1), ib = cij[c * 2 + 1] & (kMaxPeaks - 1);
      const int ida = a * kMaxPeaks + ia, idb = b * kMaxPeaks + ib;
      const double s = cs[c];
      const bool match = lane < rows && (ids[lane][a] == ida || ids[lane][b] == idb);
      const unsigned long long mask = __ballot(match);
      const int found = __popcll(mask);
      if (found == 1) {
        const int j = __ffsll((long long)mask) - 1;
        if (lane == 0 && ids[j][b] != idb) {
          ids[j][b] = idb;
          parts_n[j] += 1;
          total[j] = total[j] + ((double)sc[idb] + s);
        }
      } else if (found == 2) {
        const int j1 = __ffsll((long long)mask) - 1;
        const int j2 = __ffsll((long long)(mask & (mask - 1ull))) - 1;
        const bool both = lane < kParts && ids[j1][lane] >= 0 && ids[j2][lane] >= 0;
        if (__ballot(both) == 0ull) {  // disjoint: merge j2 into j1, delete j2
          if (lane < kParts && ids[j1][lane] < 0) ids[j1][lane] = ids[j2][lane];
          if (lane == 0) {
            total[j1] = (total[j1] + total[j2]) + s;
            parts_n[j1] += parts_n[j2];
          }
          __syncthreads();
          int row[kParts];
          double t = 0.0;
          int pn = 0;
          const bool moves = lane > j2 && lane < rows;
          if (moves) {
#pragma unroll
            for (int q = 0; q < kParts; ++q) row[q] = ids[lane][q];
            t = total[lane], pn = parts_n[lane];
          }
          __syncthreads();
          if (moves) {
#pragma unroll
            for (int q = 0; q < kParts; ++q) ids[lane - 1][q] = row[q];
            total[lane - 1] = t, parts_n[lane - 1] = pn;
          }
          rows -= 1;
        } else if (lane == 0) {
          ids[j1][b] = idb;
          parts_n[j1] += 1;
          total[j1] = total[j1] + ((double)sc[idb] + s);
        }
      } else if (found == 0 && k < 17) {
        if (rows < kMaxPeople) {
          if (lane < kParts) ids[rows][lane] = lane == a ? ida : (lane == b ? idb : -1);
          if (lane == 0) {
            parts_n[rows] = 2;
            total[rows] = ((0.0 + (double)sc[ida]) + (double)sc[idb]) + s;
          }
          rows += 1;
        } else {
          over = true;
        }
      }  // (three or more rows share an end: the published code fails there; the connection is skipped.  A matching uses a peak once,
         //  so only limbs 17 and 18 can leave an id in two rows, and no later limb asks for those parts: not reachable from ca_pose_connect)
      __syncthreads();
    }
  }
  const bool keep = lane < rows && !(parts_n[lane] < 4 || total[lane] / (double)parts_n[lane] < 0.4);
  const unsigned long long kmask = __ballot(keep);
  const int kept = __popcll(kmask);
  const int slot = __popcll(kmask & ((1ull << lane) - 1ull));
  int32_t* kp = keypoints + (int64_t)img * kMaxPeople * kParts * 2;
  int32_t* co = coords + (int64_t)img * kMaxPeople * kParts * 2;
  const int32_t* pk = peaks + (int64_t)img * kParts * kMaxPeaks * 2;
  if (keep) {
    for (int q = 0; q < kParts; ++q) {
      const int id = ids[lane][q];
      int x = -1, y = -1, kx = -1, ky = -1;
      if (id >= 0) {
        x = pk[id * 2], y = pk[id * 2 + 1];
        kx = (int)(((double)x / (double)W) * (double)W);  // format_body_result's x / float(W), draw_bodypose's int(x * W)
        ky = (int)(((double)y / (double)H) * (double)H);
      }
      kp[(slot * kParts + q) * 2] = kx, kp[(slot * kParts + q) * 2 + 1] = ky;
      co[(slot * kParts + q) * 2] = x, co[(slot * kParts + q) * 2 + 1] = y;
    }
  }
  if (lane >= kept)
    for (int q = 0; q < kParts * 2; ++q) kp[lane * kParts * 2 + q] = -1, co[lane * kParts * 2 + q] = -1;
  if (lane == 0) {
    people[img] = kept;
    if (over) atomicOr(overflow + img, CA_POSE_OVERFLOW_PEOPLE);
  }
}

// ---- draw ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void put(unsigned* plane, int H, int W, long long x, long long y, unsigned v) {
  if (x >= 0 && x < W && y >= 0 && y < H) atomicMax(plane + y * W + x, v);
}

constexpr int kPolyMax = 361;

__global__ __launch_bounds__(256) void k_pose_raster(const int32_t* __restrict__ coords, const int32_t* __restrict__ people, const float* __restrict__ sin_table,
                                                     unsigned* __restrict__ index, int H, int W, int prims) {
  __shared__ int ptx[kPolyMax], pty[kPolyMax];
  __shared__ int vx[kPolyMax], vy[kPolyMax];
  __shared__ int npts_s, row0_s, rows_s;
  __shared__ int ext1[kMaxSide], ext2[kMaxSide];
  const int prim = blockIdx.x, person = blockIdx.y, img = blockIdx.z, tid = threadIdx.x;
  int np = people[img];
  np = np < 0 ? 0 : (np > kMaxPeople ? kMaxPeople : np);
  if (person >= np) return;
  const int32_t* co = coords + ((int64_t)img * kMaxPeople + person) * kParts * 2;
  unsigned* plane = index + (int64_t)img * H * W;
  const unsigned value = (unsigned)(person * prims + prim) + 1u;  // prims: the primitives of a person (kPrims, or kPrimsFace with faces)
  if (prim >= kDrawLimbs) {  // cv2.circle(canvas, (x, y), 4, color, -1)
    const int q = prim - kDrawLimbs;
    if (co[q * 2] < 0) return;
    const int cx = (int)(((double)co[q * 2] / (double)W) * (double)W), cy = (int)(((double)co[q * 2 + 1] / (double)H) * (double)H);
    if (tid < 81) {
      const int dy = tid / 9 - 4, dx = tid % 9 - 4;
      const int half = c_circle_half[dy < 0 ? -dy : dy];
      if (dx >= -half && dx <= half) put(plane, H, W, cx + dx, cy + dy, value);
    }
    return;
  }
  const int a = c_limb_a[prim], b = c_limb_b[prim];
  if (co[a * 2] < 0 || co[b * 2] < 0) return;
  // draw_bodypose: Y = x * W, X = y * H of the normalised keypoints
  const double Y0 = ((double)co[a * 2] / (double)W) * (double)W, Y1 = ((double)co[b * 2] / (double)W) * (double)W;
  const double X0 = ((double)co[a * 2 + 1] / (double)H) * (double)H, X1 = ((double)co[b * 2 + 1] / (double)H) * (double)H;
  const double mX = (X0 + X1) / 2.0, mY = (Y0 + Y1) / 2.0;
  const double length = sqrt((X0 - X1) * (X0 - X1) + (Y0 - Y1) * (Y0 - Y1));
  const double angle = atan2(X0 - X1, Y0 - Y1) * (180.0 / 3.141592653589793);
  const int cx = (int)mY, cy = (int)mX, aw = (int)(length / 2.0), ah = 4;
  int ang = (int)angle;
  if (ang < 0) ang += 360;
  ang = ang < 0 ? 0 : (ang > 360 ? 360 : ang);
  const float alpha = sin_table[450 - ang], beta = sin_table[ang];
  for (int i = tid; i < kPolyMax; i += 256) {  // ellipse2Poly(center, axes, angle, 0, 360, 1)
    const double ex = (double)aw * (double)sin_table[450 - i], ey = (double)ah * (double)sin_table[i];
    const double fx = ((double)cx + ex * (double)alpha) - ey * (double)beta;
    const double fy = ((double)cy + ex * (double)beta) + ey * (double)alpha;
    ptx[i] = (int)rint(fx), pty[i] = (int)rint(fy);
  }
  __syncthreads();
  if (tid == 0) {  // consecutive equal points are dropped
    int n = 0;
    for (int i = 0; i < kPolyMax; ++i)
      if (n == 0 || ptx[i] != vx[n - 1] || pty[i] != vy[n - 1]) vx[n] = ptx[i], vy[n] = pty[i], ++n;
    if (n == 1) vx[0] = vx[1] = cx, vy[0] = vy[1] = cy, n = 2;
    npts_s = n;
  }
  __syncthreads();
  const int n = npts_s;
  // fillConvexPoly: the outline ...
  for (int i = tid; i < kPolyMax; i += 256) {
    if (i >= n) break;
    const int i0 = i == 0 ? n - 1 : i - 1;
    cv_line8(H, W, vx[i0], vy[i0], vx[i], vy[i], [plane, W, value](long long px, long long py) { atomicMax(plane + py * W + px, value); });
  }
  // ... then the rows between the two edge chains that start at the topmost vertex, x in 16.16 fixed point
  if (tid == 0) {
    int xmin = vx[0], xmax = vx[0], ymin = vy[0], ymax = vy[0], imin = 0;
    for (int i = 0; i < kPolyMax; ++i) {
      if (i >= n) break;
      if (vy[i] < ymin) ymin = vy[i], imin = i;
      ymax = vy[i] > ymax ? vy[i] : ymax;
      xmax = vx[i] > xmax ? vx[i] : xmax;
      xmin = vx[i] < xmin ? vx[i] : xmin;
    }
    int first = 0, count = 0;
    if (!(n < 3 || xmax < 0 || ymax < 0 || xmin >= W || ymin >= H)) {
      ymax = ymax < H - 1 ? ymax : H - 1;
      int e_idx[2] = {imin, imin}, e_di[2] = {1, n - 1}, e_ye[2] = {ymin, ymin};
      long long e_x[2] = {-65536, -65536}, e_dx[2] = {0, 0};
      int edges = n, y = ymin;
      first = ymin < 0 ? 0 : ymin;
      for (int step = 0; step < 3 * kMaxSide; ++step) {
        for (int e = 0; e < 2; ++e) {
          if (y >= e_ye[e]) {
            int idx0 = e_idx[e];
            const int di = e_di[e];
            int idx = idx0 + di;
            if (idx >= n) idx -= n;
            for (int guard = 0; guard <= kPolyMax; ++guard) {
              const int had = edges;
              edges -= 1;
              if (!(had > 0)) break;
              const int ty = vy[idx];
              if (ty > y) {
                const long long xs = (long long)vx[idx0] << 16, xe = (long long)vx[idx] << 16;
                e_ye[e] = ty;
                e_dx[e] = ((xe - xs) * 2 + (ty - y)) / (2 * (ty - y));
                e_x[e] = xs;
                e_idx[e] = idx;
                break;
              }
              idx0 = idx;
              idx += di;
              if (idx >= n) idx -= n;
            }
          }
        }
        if (edges < 0) break;
        if (y >= 0) {
          const int left = e_x[0] > e_x[1] ? 1 : 0, right = 1 - left;
          int xx1 = (int)((e_x[left] + 32768) >> 16), xx2 = (int)((e_x[right] + 32768) >> 16);
          if (xx2 >= 0 && xx1 < W) {
            xx1 = xx1 < 0 ? 0 : xx1;
            xx2 = xx2 >= W ? W - 1 : xx2;
          } else {
            xx1 = 1, xx2 = 0;  // nothing
          }
          if (y - first < kMaxSide) ext1[y - first] = xx1, ext2[y - first] = xx2, count = y - first + 1;
        }
        e_x[0] += e_dx[0], e_x[1] += e_dx[1];
        if (++y > ymax) break;
      }
    }
    row0_s = first, rows_s = count;
  }
  __syncthreads();
  const int row0 = row0_s, rows = rows_s;
  for (int r = tid; r < kMaxSide; r += 256) {
    if (r >= rows) break;
    const int x1 = ext1[r], x2 = ext2[r];
    for (int x = 0; x < kMaxSide; ++x) {
      if (x1 + x > x2) break;
      put(plane, H, W, x1 + x, row0 + r, value);
    }
  }
}

// draw_facepose: a filled radius-3 disc at (xmap[px], ymap[py]) of every face point whose two coordinates come out positive.  A block per
// (person, frame); a thread per pixel of the 7 x 7 square around a point.
__global__ __launch_bounds__(256) void k_face_raster(const int32_t* __restrict__ points, const int32_t* __restrict__ people, const int32_t* __restrict__ xmap,
                                                     const int32_t* __restrict__ ymap, unsigned* __restrict__ index, int H, int W, int prims, int base) {
  const int person = blockIdx.x, img = blockIdx.y;
  int np = people[img];
  np = np < 0 ? 0 : (np > kMaxPeople ? kMaxPeople : np);
  if (person >= np) return;
  const int32_t* pt = points + ((int64_t)img * kMaxPeople + person) * kFaceParts * 2;
  unsigned* plane = index + (int64_t)img * H * W;
  for (int i = threadIdx.x; i < kFaceParts * 49; i += 256) {
    const int q = i / 49, t = i - q * 49, dy = t / 7 - 3, dx = t % 7 - 3;
    const int px = pt[q * 2], py = pt[q * 2 + 1];
    if (px < 0 || py < 0 || px >= W || py >= H) continue;
    const int cx = xmap[px], cy = ymap[py];
    if (!(cx > 0 && cy > 0)) continue;  // x > eps and y > eps of integers
    const int half = c_disc_half[dy < 0 ? -dy : dy];
    if (dx >= -half && dx <= half) put(plane, H, W, cx + dx, cy + dy, (unsigned)(person * prims + base + q) + 1u);
  }
}

// draw_handpose: per hand 20 edges cv2.line(thickness = 2) and then 21 filled circles of radius 4.  A thick line is OpenCV's ThickLine:
// the endpoints at 16 fractional bits, dp = (cvRound(dy r), cvRound(dx r)) with r = 65536 / sqrt(dx^2 + dy^2), the four corners p0 +- dp,
// p1 -+ dp through FillConvexPoly at shift 16 (the outline with Line2, then the rows between the two edge chains), and a filled circle of
// radius 1 at each end; a zero-length edge draws only the circles.  An edge is short and thin, so one thread walks it.
__device__ bool cv_clip_line(long long wd, long long ht, long long& x1, long long& y1, long long& x2, long long& y2) {
  const long long right = wd - 1, bottom = ht - 1;
  if (wd <= 0 || ht <= 0) return false;
  int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
  int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
  if ((c1 & c2) == 0 && (c1 | c2) != 0) {
    long long a;
    if (c1 & 12) {
      a = c1 < 8 ? 0 : bottom;
      x1 += (long long)((double)(a - y1) * (double)(x2 - x1) / (double)(y2 - y1));
      y1 = a;
      c1 = (x1 < 0) + (x1 > right) * 2;
    }
    if (c2 & 12) {
      a = c2 < 8 ? 0 : bottom;
      x2 += (long long)((double)(a - y2) * (double)(x2 - x1) / (double)(y2 - y1));
      y2 = a;
      c2 = (x2 < 0) + (x2 > right) * 2;
    }
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
      if (c1) {
        a = c1 == 1 ? 0 : right;
        y1 += (long long)((double)(a - x1) * (double)(y2 - y1) / (double)(x2 - x1));
        x1 = a;
        c1 = 0;
      }
      if (c2) {
        a = c2 == 1 ? 0 : right;
        y2 += (long long)((double)(a - x2) * (double)(y2 - y1) / (double)(x2 - x1));
        x2 = a;
        c2 = 0;
      }
    }
  }
  return (c1 | c2) == 0;
}

// OpenCV's Line2: a line between two points at 16 fractional bits, one pixel per step of the longer axis.
__device__ void cv_line2(unsigned* plane, int H, int W, unsigned v, long long x1, long long y1, long long x2, long long y2) {
  if (!cv_clip_line((long long)W << 16, (long long)H << 16, x1, y1, x2, y2)) return;
  long long dx = x2 - x1, dy = y2 - y1;
  const long long ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
  long long x_step, y_step;
  int ecount;
  if (ax > ay) {
    if (dx < 0) {
      long long t = x1;
      x1 = x2, x2 = t, t = y1, y1 = y2, y2 = t, dy = -dy;
    }
    x_step = 65536, y_step = (dy * 65536) / (ax | 1);
    ecount = (int)((x2 - x1) >> 16);
  } else {
    if (dy < 0) {
      long long t = x1;
      x1 = x2, x2 = t, t = y1, y1 = y2, y2 = t, dx = -dx;
    }
    x_step = (dx * 65536) / (ay | 1), y_step = 65536;
    ecount = (int)((y2 - y1) >> 16);
  }
  x1 += 32768, y1 += 32768;
  put(plane, H, W, (x2 + 32768) >> 16, (y2 + 32768) >> 16, v);
  if (ax > ay) {
    x1 >>= 16;
    for (int k = 0; k <= kMaxSide; ++k) {
      if (k > ecount) break;
      put(plane, H, W, x1, y1 >> 16, v);
      x1 += 1, y1 += y_step;
    }
  } else {
    y1 >>= 16;
    for (int k = 0; k <= kMaxSide; ++k) {
      if (k > ecount) break;
      put(plane, H, W, x1 >> 16, y1, v);
      x1 += x_step, y1 += 1;
    }
  }
  (void)x_step;
}

// FillConvexPoly(pts, 4, line_type 8, shift 16): the routine k_pose_raster runs at shift 0 for the limbs, for four corners at 16 fractional bits.
__device__ void cv_fill_quad16(unsigned* plane, int H, int W, unsigned v, const long long* vx, const long long* vy) {
  constexpr int n = 4;
  constexpr long long delta = 32768;
  long long xmin = vx[0], xmax = vx[0], ymin = vy[0], ymax = vy[0];
  int imin = 0;
  for (int i = 0; i < n; ++i) {
    if (vy[i] < ymin) ymin = vy[i], imin = i;
    ymax = vy[i] > ymax ? vy[i] : ymax;
    xmax = vx[i] > xmax ? vx[i] : xmax;
    xmin = vx[i] < xmin ? vx[i] : xmin;
    const int i0 = i == 0 ? n - 1 : i - 1;
    cv_line2(plane, H, W, v, vx[i0], vy[i0], vx[i], vy[i]);
  }
  xmin = (xmin + delta) >> 16, xmax = (xmax + delta) >> 16, ymin = (ymin + delta) >> 16, ymax = (ymax + delta) >> 16;
  if ((int)xmax < 0 || (int)ymax < 0 || (int)xmin >= W || (int)ymin >= H) return;
  ymax = ymax < H - 1 ? ymax : H - 1;
  int e_idx[2] = {imin, imin}, e_di[2] = {1, n - 1}, e_ye[2] = {(int)ymin, (int)ymin};
  long long e_x[2] = {-65536, -65536}, e_dx[2] = {0, 0};
  int edges = n, y = (int)ymin;
  for (int step = 0; step < 3 * kMaxSide; ++step) {
    for (int e = 0; e < 2; ++e) {
      if (y >= e_ye[e]) {
        int idx0 = e_idx[e];
        const int di = e_di[e];
        int idx = idx0 + di;
        if (idx >= n) idx -= n;
        for (int guard = 0; guard <= n; ++guard) {
          const int had = edges;
          edges -= 1;
          if (!(had > 0)) break;
          const int ty = (int)((vy[idx] + delta) >> 16);
          if (ty > y) {
            const long long xs = vx[idx0], xe = vx[idx];
            e_ye[e] = ty;
            e_dx[e] = ((xe - xs) * 2 + (ty - y)) / (2 * (ty - y));
            e_x[e] = xs;
            e_idx[e] = idx;
            break;
          }
          idx0 = idx;
          idx += di;
          if (idx >= n) idx -= n;
        }
      }
    }
    if (edges < 0) break;
    if (y >= 0) {
      const int left = e_x[0] > e_x[1] ? 1 : 0, right = 1 - left;
      int xx1 = (int)((e_x[left] + 32768) >> 16), xx2 = (int)((e_x[right] + 32768) >> 16);
      if (xx2 >= 0 && xx1 < W) {
        xx1 = xx1 < 0 ? 0 : xx1;
        xx2 = xx2 >= W ? W - 1 : xx2;
        for (int x = 0; x < kMaxSide; ++x) {
          if (xx1 + x > xx2) break;
          put(plane, H, W, xx1 + x, y, v);
        }
      }
    }
    e_x[0] += e_dx[0], e_x[1] += e_dx[1];
    if (++y > (int)ymax) break;
  }
}

__constant__ unsigned char c_hand_color[20][3] = {{255, 0, 0},   {255, 77, 0},  {255, 153, 0}, {255, 229, 0}, {204, 255, 0}, {128, 255, 0}, {51, 255, 0},
                                                  {0, 255, 25},  {0, 255, 102}, {0, 255, 179}, {0, 255, 255}, {0, 178, 255}, {0, 102, 255}, {0, 25, 255},
                                                  {51, 0, 255},  {128, 0, 255}, {204, 0, 255}, {255, 0, 230}, {255, 0, 153}, {255, 0, 77}};  // openpose_hand.hand_colors()
__constant__ int c_hand_edge[20][2] = {{0, 1},  {1, 2},   {2, 3},   {3, 4},   {0, 5},   {5, 6},   {6, 7},   {7, 8},   {0, 9},   {9, 10},
                                       {10, 11}, {11, 12}, {0, 13}, {13, 14}, {14, 15}, {15, 16}, {0, 17}, {17, 18}, {18, 19}, {19, 20}};
constexpr int kHandParts = CA_HAND_PARTS, kHandEdges = 20, kHandPrims = kHandEdges + kHandParts;  // 41 per hand
constexpr int kPrimsAll = kPrims + 2 * kHandPrims + kFaceParts;                                     // body, left hand, right hand, face

// A block per (primitive of a hand, hand of a person, frame): hand_points int32 [images, 64, 2, 21, 2].
__global__ __launch_bounds__(64) void k_hand_raster(const int32_t* __restrict__ points, const int32_t* __restrict__ people, const int32_t* __restrict__ xmap,
                                                    const int32_t* __restrict__ ymap, unsigned* __restrict__ index, int H, int W) {
  const int prim = blockIdx.x, person = blockIdx.y >> 1, hand = blockIdx.y & 1, img = blockIdx.z, tid = threadIdx.x;
  int np = people[img];
  np = np < 0 ? 0 : (np > kMaxPeople ? kMaxPeople : np);
  if (person >= np) return;
  const int32_t* pt = points + (((int64_t)img * kMaxPeople + person) * 2 + hand) * kHandParts * 2;
  unsigned* plane = index + (int64_t)img * H * W;
  const unsigned value = (unsigned)(person * kPrimsAll + kPrims + hand * kHandPrims + prim) + 1u;
  if (prim >= kHandEdges) {  // cv2.circle(canvas, (x, y), 4, (0, 0, 255), -1)
    const int q = prim - kHandEdges;
    const int px = pt[q * 2], py = pt[q * 2 + 1];
    if (px < 0 || py < 0 || px >= W || py >= H) return;
    const int cx = xmap[px], cy = ymap[py];
    if (!(cx > 0 && cy > 0)) return;
    for (int i = tid; i < 81; i += 64) {
      const int dy = i / 9 - 4, dx = i % 9 - 4;
      const int half = c_circle_half[dy < 0 ? -dy : dy];
      if (dx >= -half && dx <= half) put(plane, H, W, cx + dx, cy + dy, value);
    }
    return;
  }
  if (tid != 0) return;
  const int a = c_hand_edge[prim][0], b = c_hand_edge[prim][1];
  const int ax = pt[a * 2], ay = pt[a * 2 + 1], bx = pt[b * 2], by = pt[b * 2 + 1];
  if (ax < 0 || ay < 0 || bx < 0 || by < 0 || ax >= W || bx >= W || ay >= H || by >= H) return;
  const int x1 = xmap[ax], y1 = ymap[ay], x2 = xmap[bx], y2 = ymap[by];
  if (!(x1 > 0 && y1 > 0 && x2 > 0 && y2 > 0)) return;
  const long long p0x = (long long)x1 << 16, p0y = (long long)y1 << 16, p1x = (long long)x2 << 16, p1y = (long long)y2 << 16;
  const double dx = (double)(p0x - p1x) * (1.0 / 65536.0), dy = (double)(p1y - p0y) * (1.0 / 65536.0);
  double r = dx * dx + dy * dy;
  if (fabs(r) > 2.220446049250313e-16) {
    r = 65536.0 / sqrt(r);
    const long long dpx = (long long)rint(dy * r), dpy = (long long)rint(dx * r);
    const long long vx[4] = {p0x + dpx, p0x - dpx, p1x - dpx, p1x + dpx}, vy[4] = {p0y + dpy, p0y - dpy, p1y - dpy, p1y + dpy};
    cv_fill_quad16(plane, H, W, value, vx, vy);
  }
  const int ex[2] = {x1, x2}, ey[2] = {y1, y2};
  for (int e = 0; e < 2; ++e) {  // Circle(center, 1, filled): the centre's row three wide, one pixel above and below
    put(plane, H, W, ex[e] - 1, ey[e], value), put(plane, H, W, ex[e], ey[e], value), put(plane, H, W, ex[e] + 1, ey[e], value);
    put(plane, H, W, ex[e], ey[e] - 1, value), put(plane, H, W, ex[e], ey[e] + 1, value);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_pose_resolve(const unsigned* __restrict__ index, uint8_t* __restrict__ map, T* __restrict__ ctrl, int images, int64_t hw,
                                                      int rep, int prims, int hands) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= images * hw) return;
  const int img = (int)(g / hw);
  const int64_t p = g - img * hw;
  const unsigned v = index[g];
  int rgb[3] = {0, 0, 0};
  if (v) {
    const int prim = (int)((v - 1u) % (unsigned)prims);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      rgb[c] = prim < kDrawLimbs ? (int)((double)c_color[prim][c] * 0.6) : (prim < kPrims ? (int)c_color[prim - kDrawLimbs][c] : 255);  // a face disc is white
    if (hands && prim >= kPrims && prim < kPrims + 2 * kHandPrims) {  // a hand's edge in its hsv colour, its circles (0, 0, 255)
      const int j = (prim - kPrims) % kHandPrims;
#pragma unroll
      for (int c = 0; c < 3; ++c) rgb[c] = j < kHandEdges ? (int)c_hand_color[j][c] : (c == 2 ? 255 : 0);
    }
  }
  if (map) {
#pragma unroll
    for (int c = 0; c < 3; ++c) map[g * 3 + c] = (uint8_t)rgb[c];
  }
  if (ctrl) emit_control1(ctrl, images, img, hw, p, rep, rgb);  // (ca_annot.h: one level per channel)
}

}  // namespace

extern "C" int ca_pose_prep(const uint8_t* frames, void* out, const int32_t* xofs, const int32_t* xcnt, const float* xw, const int32_t* yofs, const int32_t* ycnt,
                            const float* yw, int32_t images, int32_t h, int32_t w, int32_t hs, int32_t ws, int32_t hp, int32_t wp, int32_t dtype, void* stream) {
  CA_REQUIRE(frames && out && xofs && xcnt && xw && yofs && ycnt && yw, "ca_pose_prep: frames, out and the six tables are required");
  CA_REQUIRE(sizes_ok(images, h, w) && sizes_ok(images, hp, wp), "ca_pose_prep: images=%d h=%d w=%d hp=%d wp=%d (each >= 1, images * h * w < 2^31)", images, h, w, hp, wp);
  CA_REQUIRE(hs >= 1 && ws >= 1 && hs <= hp && ws <= wp && hp % 8 == 0 && wp % 8 == 0 && hp - hs < 8 && wp - ws < 8,
             "ca_pose_prep: hs=%d ws=%d hp=%d wp=%d (the resized size, padded below and to the right to the next multiples of 8)", hs, ws, hp, wp);
  CA_REQUIRE((int64_t)images * hp * wp * 16 <= kMaxBytes, "ca_pose_prep: images=%d hp=%d wp=%d: out would pass 2^31 bytes", images, hp, wp);
  CA_REQUIRE(dtype_ok(dtype), "ca_pose_prep: dtype %d", dtype);
  CA_REQUIRE(((uintptr_t)out & 15) == 0 && (((uintptr_t)xofs | (uintptr_t)xcnt | (uintptr_t)xw | (uintptr_t)yofs | (uintptr_t)ycnt | (uintptr_t)yw) & 3) == 0,
             "ca_pose_prep: out must be 16-byte aligned, the tables 4-byte aligned");
  const int64_t total = (int64_t)images * hp * wp;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_pose_prep<DT>, grid, block, 0, (hipStream_t)stream, frames, (u16*)out, xofs, xcnt, xw, yofs, ycnt, yw, total, (int)h, (int)w, (int)hs, (int)ws,
                       (int)hp, (int)wp));
  CA_CHECK_LAUNCH("ca_pose_prep");
  return CA_OK;
}

extern "C" int ca_conv7x7(const ca_conv7x7_args* a, void* stream) {
  CA_REQUIRE(a, "ca_conv7x7: args is NULL");
  CA_REQUIRE(a->groups == 1 || a->groups == 2, "ca_conv7x7: groups=%d (1 or 2)", a->groups);
  for (int g = 0; g < a->groups; ++g) {
    CA_REQUIRE(a->x[g] && a->w[g] && a->y[g], "ca_conv7x7: x, w and y of problem %d are required", g);
    CA_REQUIRE((((uintptr_t)a->x[g] | (uintptr_t)a->w[g]) & 15) == 0 && ((uintptr_t)a->y[g] & 7) == 0 && ((uintptr_t)a->bias[g] & 3) == 0,
               "ca_conv7x7: x and w must be 16-byte aligned, y 8-byte aligned, bias 4-byte aligned (problem %d)", g);
  }
  CA_REQUIRE(sizes_ok(a->images, a->h, a->w_px), "ca_conv7x7: images=%d h=%d w=%d (each >= 1, images * h * w < 2^31)", a->images, a->h, a->w_px);
  CA_REQUIRE(a->cin >= 32 && a->cin % 32 == 0 && a->cin <= 1024, "ca_conv7x7: cin=%d must be a multiple of 32 in 32 .. 1024", a->cin);
  CA_REQUIRE(a->cout >= 64 && a->cout % 64 == 0 && a->cout <= 1024, "ca_conv7x7: cout=%d must be a multiple of 64 in 64 .. 1024", a->cout);
  CA_REQUIRE(a->ldx >= a->cin && a->ldx % 8 == 0 && a->ldy >= a->cout && a->ldy % 4 == 0, "ca_conv7x7: ldx=%lld ldy=%lld (ldx >= cin, a multiple of 8; ldy >= cout, a multiple of 4)",
             (long long)a->ldx, (long long)a->ldy);
  CA_REQUIRE((int64_t)a->images * a->h * a->w_px * a->ldx * 2 <= kMaxBytes && (int64_t)a->images * a->h * a->w_px * a->ldy * 2 <= kMaxBytes,
             "ca_conv7x7: images=%d h=%d w=%d: an operand would pass 2^31 bytes", a->images, a->h, a->w_px);
  CA_REQUIRE(a->relu == 0 || a->relu == 1, "ca_conv7x7: relu=%d (0 or 1)", a->relu);
  CA_REQUIRE(dtype_ok(a->dtype), "ca_conv7x7: dtype %d", a->dtype);
  const int tx = ceil_div_i(a->w_px, C7_TW), ty = ceil_div_i(a->h, C7_TH);
  const int64_t blocks = (int64_t)a->images * tx * ty * (a->cout / C7_CT);
  CA_REQUIRE(blocks < ((int64_t)1 << 31), "ca_conv7x7: grid too large");
  C7Problems p;
  for (int g = 0; g < 2; ++g) {
    const int s = g < a->groups ? g : 0;
    p.x[g] = (const u16*)a->x[s], p.w[g] = (const u16*)a->w[s], p.bias[g] = a->bias[s], p.y[g] = (u16*)a->y[s];
  }
  const dim3 grid((unsigned)blocks, 1, (unsigned)a->groups), block(256);
  if (a->dtype == CA_BF16)
    hipLaunchKernelGGL(k_conv7<CA_BF16>, grid, block, 0, (hipStream_t)stream, p, (int)a->h, (int)a->w_px, (int)a->cin, (int)a->cout, a->ldx, a->ldy, tx, ty, (int)a->relu);
  else
    hipLaunchKernelGGL(k_conv7<CA_F16>, grid, block, 0, (hipStream_t)stream, p, (int)a->h, (int)a->w_px, (int)a->cin, (int)a->cout, a->ldx, a->ldy, tx, ty, (int)a->relu);
  CA_CHECK_LAUNCH("ca_conv7x7");
  return CA_OK;
}

extern "C" int ca_im2col7x7(const void* x, void* cols, int32_t images, int32_t h, int32_t w, int32_t cin, int64_t ldx, int32_t dtype, void* stream) {
  CA_REQUIRE(x && cols, "ca_im2col7x7: x and cols are required");
  CA_REQUIRE(sizes_ok(images, h, w), "ca_im2col7x7: images=%d h=%d w=%d (each >= 1, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE(cin >= 8 && cin % 8 == 0 && cin <= 1024, "ca_im2col7x7: cin=%d must be a multiple of 8 in 8 .. 1024", cin);
  CA_REQUIRE(ldx >= cin && ldx % 8 == 0, "ca_im2col7x7: ldx=%lld (>= cin, a multiple of 8)", (long long)ldx);
  CA_REQUIRE((int64_t)images * h * w * 49 * cin * 2 <= kMaxBytes && (int64_t)images * h * w * ldx * 2 <= kMaxBytes,
             "ca_im2col7x7: images=%d h=%d w=%d cin=%d: an operand would pass 2^31 bytes", images, h, w, cin);
  CA_REQUIRE(dtype_ok(dtype), "ca_im2col7x7: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)cols) & 15) == 0, "ca_im2col7x7: x and cols must be 16-byte aligned");
  const int64_t total = (int64_t)images * h * w * 49 * (cin / 8);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipLaunchKernelGGL(k_im2col7, grid, block, 0, (hipStream_t)stream, (const u16*)x, (u16*)cols, total, (int)h, (int)w, (int)cin, ldx);
  CA_CHECK_LAUNCH("ca_im2col7x7");
  return CA_OK;
}

extern "C" int ca_copy_cols(const void* src, void* dst, int64_t rows, int32_t c, int64_t ld, int32_t col0, int32_t dtype, void* stream) {
  CA_REQUIRE(src && dst, "ca_copy_cols: src and dst are required");
  CA_REQUIRE(rows >= 1 && c >= 8 && c % 8 == 0 && col0 >= 0 && col0 % 8 == 0 && ld % 8 == 0 && ld >= (int64_t)col0 + c,
             "ca_copy_cols: rows=%lld c=%d ld=%lld col0=%d (multiples of 8, col0 + c <= ld)", (long long)rows, c, (long long)ld, col0);
  CA_REQUIRE(rows * ld * 2 <= kMaxBytes, "ca_copy_cols: rows=%lld ld=%lld: dst would pass 2^31 bytes", (long long)rows, (long long)ld);
  CA_REQUIRE(dtype_ok(dtype), "ca_copy_cols: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 15) == 0, "ca_copy_cols: src and dst must be 16-byte aligned");
  const int64_t total = rows * (c / 8);
  hipLaunchKernelGGL(k_copy_cols, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const u16*)src, (u16*)dst, total, (int)c, ld, (int)col0);
  CA_CHECK_LAUNCH("ca_copy_cols");
  return CA_OK;
}

extern "C" int64_t ca_pose_maps_workspace_bytes(int32_t images, int32_t hl, int32_t w) {
  if (images < 1 || hl < 1 || w < 1) return 0;
  return (int64_t)images * kMapCh * hl * w * 4;
}

extern "C" int ca_pose_maps(const float* low, const float* mx, const float* my, void* workspace, int64_t workspace_bytes, float* raw, float* smooth, float* paf,
                            int32_t images, int32_t hl, int32_t wl, int32_t h, int32_t w, void* stream) {
  CA_REQUIRE(low && mx && my && workspace && raw && smooth && paf, "ca_pose_maps: low, mx, my, workspace, raw, smooth and paf are required");
  CA_REQUIRE(sizes_ok(images, h, w) && hl >= 1 && wl >= 1 && hl <= h && wl <= w, "ca_pose_maps: images=%d hl=%d wl=%d h=%d w=%d (1 <= hl <= h, 1 <= wl <= w, images * h * w < 2^31)",
             images, hl, wl, h, w);
  CA_REQUIRE(workspace_bytes >= ca_pose_maps_workspace_bytes(images, hl, w), "ca_pose_maps: the workspace holds %lld bytes, %lld are needed", (long long)workspace_bytes,
             (long long)ca_pose_maps_workspace_bytes(images, hl, w));
  CA_REQUIRE((((uintptr_t)low | (uintptr_t)mx | (uintptr_t)my | (uintptr_t)workspace | (uintptr_t)raw | (uintptr_t)smooth | (uintptr_t)paf) & 3) == 0,
             "ca_pose_maps: every pointer must be 4-byte aligned");
  const int64_t t1 = (int64_t)images * kMapCh * hl * w, t2 = (int64_t)images * kMapCh * h * w;
  CA_REQUIRE((int64_t)images * kMapCh <= 65535 && (h + kRowsPerThread - 1) / kRowsPerThread <= 65535, "ca_pose_maps: images=%d h=%d: grid too large (images <= 885)", images, h);
  (void)t2;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_pose_cols, dim3((unsigned)((t1 + 255) / 256)), dim3(256), 0, st, low, mx, (float*)workspace, t1, (int)hl, (int)wl, (int)w);
  hipLaunchKernelGGL(k_pose_rows, dim3((unsigned)((w + 255) / 256), (unsigned)((h + kRowsPerThread - 1) / kRowsPerThread), (unsigned)(images * kMapCh)), dim3(256), 0, st,
                     (const float*)workspace, my, raw, smooth, paf, (int)hl, (int)h, (int)w);
  CA_CHECK_LAUNCH("ca_pose_maps");
  return CA_OK;
}

extern "C" int ca_pose_peaks(const float* raw, const float* smooth, int32_t* peaks, float* scores, int32_t* counts, int32_t* overflow, int32_t images, int32_t h,
                             int32_t w, void* stream) {
  CA_REQUIRE(raw && smooth && peaks && scores && counts && overflow, "ca_pose_peaks: raw, smooth, peaks, scores, counts and overflow are required");
  CA_REQUIRE(sizes_ok(images, h, w) && images <= 65535, "ca_pose_peaks: images=%d h=%d w=%d (each >= 1, images <= 65535, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE((((uintptr_t)raw | (uintptr_t)smooth | (uintptr_t)peaks | (uintptr_t)scores | (uintptr_t)counts | (uintptr_t)overflow) & 3) == 0,
             "ca_pose_peaks: every pointer must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(overflow, 0, (size_t)images * 4, st);
  if (e != hipSuccess) CA_FAIL(CA_ERR_LAUNCH, "ca_pose_peaks: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(k_pose_peaks, dim3(kParts, (unsigned)images), dim3(256), 0, st, raw, smooth, peaks, scores, counts, overflow, (int)h, (int)w);
  CA_CHECK_LAUNCH("ca_pose_peaks");
  return CA_OK;
}

extern "C" int ca_pose_connect(const float* paf, const int32_t* peaks, const int32_t* counts, int32_t* conn_ij, double* conn_score, int32_t* conn_n, int32_t images,
                               int32_t h, int32_t w, void* stream) {
  CA_REQUIRE(paf && peaks && counts && conn_ij && conn_score && conn_n, "ca_pose_connect: paf, peaks, counts, conn_ij, conn_score and conn_n are required");
  CA_REQUIRE(sizes_ok(images, h, w) && images <= 65535, "ca_pose_connect: images=%d h=%d w=%d (each >= 1, images <= 65535, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE((((uintptr_t)paf | (uintptr_t)peaks | (uintptr_t)counts | (uintptr_t)conn_ij | (uintptr_t)conn_n) & 3) == 0 && ((uintptr_t)conn_score & 7) == 0,
             "ca_pose_connect: conn_score must be 8-byte aligned, the other pointers 4-byte aligned");
  hipLaunchKernelGGL(k_pose_connect, dim3(kLimbs, (unsigned)images), dim3(256), 0, (hipStream_t)stream, paf, peaks, counts, conn_ij, conn_score, conn_n, (int)h, (int)w);
  CA_CHECK_LAUNCH("ca_pose_connect");
  return CA_OK;
}

extern "C" int ca_pose_assemble(const int32_t* peaks, const float* scores, const int32_t* conn_ij, const double* conn_score, const int32_t* conn_n, int32_t* keypoints,
                                int32_t* coords, int32_t* people, int32_t* overflow, int32_t images, int32_t h, int32_t w, void* stream) {
  CA_REQUIRE(peaks && scores && conn_ij && conn_score && conn_n && keypoints && coords && people && overflow,
             "ca_pose_assemble: peaks, scores, conn_ij, conn_score, conn_n, keypoints, coords, people and overflow are required");
  CA_REQUIRE(sizes_ok(images, h, w), "ca_pose_assemble: images=%d h=%d w=%d (each >= 1, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE((((uintptr_t)peaks | (uintptr_t)scores | (uintptr_t)conn_ij | (uintptr_t)conn_n | (uintptr_t)keypoints | (uintptr_t)coords | (uintptr_t)people |
               (uintptr_t)overflow) & 3) == 0 && ((uintptr_t)conn_score & 7) == 0,
             "ca_pose_assemble: conn_score must be 8-byte aligned, the other pointers 4-byte aligned");
  hipLaunchKernelGGL(k_pose_assemble, dim3((unsigned)images), dim3(64), 0, (hipStream_t)stream, peaks, scores, conn_ij, conn_score, conn_n, keypoints, coords, people,
                     overflow, (int)h, (int)w);
  CA_CHECK_LAUNCH("ca_pose_assemble");
  return CA_OK;
}

extern "C" int ca_pose_draw(const int32_t* coords, const int32_t* people, const float* sin_table, uint32_t* index, uint8_t* map, void* control, int32_t images,
                            int32_t h, int32_t w, int32_t rep, int32_t control_dtype, void* stream) {
  CA_REQUIRE(coords && people && sin_table && index, "ca_pose_draw: coords, people, sin_table and index are required");
  CA_REQUIRE(map || control, "ca_pose_draw: map or control is required");
  CA_REQUIRE(sizes_ok(images, h, w) && images <= 65535 && h <= kMaxSide && w <= kMaxSide,
             "ca_pose_draw: images=%d h=%d w=%d (each >= 1, images <= 65535, h and w <= %d, images * h * w < 2^31)", images, h, w, kMaxSide);
  if (const int rc = control_out_checks("ca_pose_draw", false, h, w, nullptr, true, rep, control_dtype)) return rc;
  CA_REQUIRE((((uintptr_t)coords | (uintptr_t)people | (uintptr_t)sin_table | (uintptr_t)index) & 3) == 0 &&
                 ctrl_aligned(control, control_dtype, 1),
             "ca_pose_draw: coords, people, sin_table and index must be 4-byte aligned, control aligned to its element");
  hipStream_t st = (hipStream_t)stream;
  const int64_t hw = (int64_t)h * w, total = (int64_t)images * hw;
  hipError_t e = hipMemsetAsync(index, 0, (size_t)total * 4, st);
  if (e != hipSuccess) CA_FAIL(CA_ERR_LAUNCH, "ca_pose_draw: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(k_pose_raster, dim3(kPrims, kMaxPeople, (unsigned)images), dim3(256), 0, st, coords, people, sin_table, (unsigned*)index, (int)h, (int)w, kPrims);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  CA_DISPATCH_CTRL(control_dtype, hipLaunchKernelGGL(k_pose_resolve<T>, grid, block, 0, st, (const unsigned*)index, map, (T*)control, (int)images, hw, (int)rep, kPrims, 0));
  CA_CHECK_LAUNCH("ca_pose_draw");
  return CA_OK;
}

extern "C" int ca_pose_draw_faces(const int32_t* coords, const int32_t* people, const float* sin_table, const int32_t* points, const int32_t* xmap, const int32_t* ymap,
                                  uint32_t* index, uint8_t* map, void* control, int32_t images, int32_t h, int32_t w, int32_t rep, int32_t control_dtype,
                                  void* stream) {
  CA_REQUIRE(coords && people && sin_table && index, "ca_pose_draw_faces: coords, people, sin_table and index are required");
  CA_REQUIRE(!points || (xmap && ymap), "ca_pose_draw_faces: points need xmap and ymap");
  CA_REQUIRE(map || control, "ca_pose_draw_faces: map or control is required");
  CA_REQUIRE(sizes_ok(images, h, w) && images <= 65535 && h <= kMaxSide && w <= kMaxSide,
             "ca_pose_draw_faces: images=%d h=%d w=%d (each >= 1, images <= 65535, h and w <= %d, images * h * w < 2^31)", images, h, w, kMaxSide);
  if (const int rc = control_out_checks("ca_pose_draw_faces", false, h, w, nullptr, true, rep, control_dtype)) return rc;
  CA_REQUIRE((((uintptr_t)coords | (uintptr_t)people | (uintptr_t)sin_table | (uintptr_t)index | (uintptr_t)points | (uintptr_t)xmap | (uintptr_t)ymap) & 3) == 0 &&
                 ctrl_aligned(control, control_dtype, 1),
             "ca_pose_draw_faces: coords, people, sin_table, points, xmap, ymap and index must be 4-byte aligned, control aligned to its element");
  hipStream_t st = (hipStream_t)stream;
  const int64_t hw = (int64_t)h * w, total = (int64_t)images * hw;
  hipError_t e = hipMemsetAsync(index, 0, (size_t)total * 4, st);
  if (e != hipSuccess) CA_FAIL(CA_ERR_LAUNCH, "ca_pose_draw_faces: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(k_pose_raster, dim3(kPrims, kMaxPeople, (unsigned)images), dim3(256), 0, st, coords, people, sin_table, (unsigned*)index, (int)h, (int)w, kPrimsFace);
  if (points) hipLaunchKernelGGL(k_face_raster, dim3(kMaxPeople, (unsigned)images), dim3(256), 0, st, points, people, xmap, ymap, (unsigned*)index, (int)h, (int)w, kPrimsFace, kPrims);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  CA_DISPATCH_CTRL(control_dtype, hipLaunchKernelGGL(k_pose_resolve<T>, grid, block, 0, st, (const unsigned*)index, map, (T*)control, (int)images, hw, (int)rep, kPrimsFace, 0));
  CA_CHECK_LAUNCH("ca_pose_draw_faces");
  return CA_OK;
}

extern "C" int ca_pose_draw_hands(const int32_t* coords, const int32_t* people, const float* sin_table, const int32_t* hand_points, const int32_t* face_points,
                                  const int32_t* xmap, const int32_t* ymap, uint32_t* index, uint8_t* map, void* control, int32_t images, int32_t h, int32_t w,
                                  int32_t rep, int32_t control_dtype, void* stream) {
  CA_REQUIRE(coords && people && sin_table && index && hand_points && xmap && ymap, "ca_pose_draw_hands: coords, people, sin_table, hand_points, xmap, ymap and index are required");
  CA_REQUIRE(map || control, "ca_pose_draw_hands: map or control is required");
  CA_REQUIRE(sizes_ok(images, h, w) && images <= 65535 && h <= kMaxSide && w <= kMaxSide,
             "ca_pose_draw_hands: images=%d h=%d w=%d (each >= 1, images <= 65535, h and w <= %d, images * h * w < 2^31)", images, h, w, kMaxSide);
  if (const int rc = control_out_checks("ca_pose_draw_hands", false, h, w, nullptr, true, rep, control_dtype)) return rc;
  CA_REQUIRE((((uintptr_t)coords | (uintptr_t)people | (uintptr_t)sin_table | (uintptr_t)index | (uintptr_t)hand_points | (uintptr_t)face_points | (uintptr_t)xmap |
               (uintptr_t)ymap) & 3) == 0 && ctrl_aligned(control, control_dtype, 1),
             "ca_pose_draw_hands: coords, people, sin_table, the points, xmap, ymap and index must be 4-byte aligned, control aligned to its element");
  hipStream_t st = (hipStream_t)stream;
  const int64_t hw = (int64_t)h * w, total = (int64_t)images * hw;
  hipError_t e = hipMemsetAsync(index, 0, (size_t)total * 4, st);
  if (e != hipSuccess) CA_FAIL(CA_ERR_LAUNCH, "ca_pose_draw_hands: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(k_pose_raster, dim3(kPrims, kMaxPeople, (unsigned)images), dim3(256), 0, st, coords, people, sin_table, (unsigned*)index, (int)h, (int)w, kPrimsAll);
  hipLaunchKernelGGL(k_hand_raster, dim3(kHandPrims, 2 * kMaxPeople, (unsigned)images), dim3(64), 0, st, hand_points, people, xmap, ymap, (unsigned*)index, (int)h, (int)w);
  if (face_points)
    hipLaunchKernelGGL(k_face_raster, dim3(kMaxPeople, (unsigned)images), dim3(256), 0, st, face_points, people, xmap, ymap, (unsigned*)index, (int)h, (int)w, kPrimsAll,
                       kPrims + 2 * kHandPrims);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  CA_DISPATCH_CTRL(control_dtype, hipLaunchKernelGGL(k_pose_resolve<T>, grid, block, 0, st, (const unsigned*)index, map, (T*)control, (int)images, hw, (int)rep, kPrimsAll, 1));
  CA_CHECK_LAUNCH("ca_pose_draw_hands");
  return CA_OK;
}
