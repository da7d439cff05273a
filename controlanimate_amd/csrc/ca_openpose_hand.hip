// Added to ABI v16: the hand stage of the OpenPose annotator around its network (controlanimate_amd/openpose_hand.py; the specification is
// tests/hand_ref.py, restated from the published controlnet_aux open_pose/{__init__,hand,util}.py, scipy's gaussian_filter and
// skimage.measure.label).  The hand network has FaceNet's layers with 22 output maps and runs on ca_conv3x3 / ca_maxpool2x2 / ca_gemm /
// ca_conv7x7 / ca_copy_cols; this file holds what the stage needs around it:
//
//   boxes   k_hand_boxes   per frame, one wave, a lane per person: util.handDetect in double, operation by operation (the keypoints are
//                          integers), left before right; the slots of the first max_hands boxes in that order (two ballots and prefix
//                          counts), the overflow bits
//   crop    k_hand_blur    cv2.GaussianBlur(crop, (0, 0), 0.8) as the specification restates it (float taps, double sums, one rounding) into a
//                          per-slot buffer; k_hand_resize: cv2.resize of that to one of the four sides through host-made tables, a thread
//                          per output pixel, in the face stage's arithmetic (INTER_LANCZOS4 in 11-bit fixed point, INTER_AREA as fp32
//                          sums, horizontal before vertical), plus OpenCV's exact-2x path (a + b + c + d + 2) >> 2
//   maps    k_hand_maps  per (slot, part, plane): sum over the four scales s of M_s H_s M_s^T / 4 for the 128 x 128 average (M_s = A_s, the
//                          composed x8 LANCZOS4 and INTER_AREA resizes of one axis) and for its sigma-3 Gaussian (M_s = G A_s).  A scale's
//                          map and its column pass stay in LDS; no x8 plane is ever written
//   peaks   k_hand_peaks   per (slot, part): binary = smooth > 0.05, its 8-connected components by union-find in LDS with the raster-minimum
//                          index as root (so the roots ascend in skimage's label order), the mass of every component as a double sum in
//                          a fixed order, the heaviest component (the first on a tie), the first row-major maximum of raw inside it
//
// No launch depends on device data on the host side: the stage can be captured in a hipGraph.
#include "ca_common.h"

#include <climits>

namespace {

constexpr int kParts = 18, kMaxPeople = CA_POSE_MAX_PEOPLE;
constexpr int kHandParts = CA_HAND_PARTS, kHeatCols = CA_HAND_HEAT_COLS, kSide = CA_HAND_MAP, kPix = kSide * kSide, kSlot = CA_HAND_SLOT_INTS;
constexpr int kScales = CA_HAND_SCALES, kMaxSide = 2048, kMaxHands = 2 * kMaxPeople;
constexpr int kMinBox = CA_HAND_MIN_BOX, kBlurTaps = 7, kLzTaps = 8, kAreaTaps = CA_HAND_AREA_TAPS;
constexpr int kBase = 184;                                   // the four network inputs are 1, 2, 3, 4 times 184 pixels, their maps 23 times that
constexpr int kMapMax = 92, kMapRows = 23 + 46 + 69 + 92;     // the rows of the four transposed axis matrices behind each other
static_assert(kMaxPeople == 64, "k_hand_boxes keeps one person per lane of a wave");
static_assert(kSide == 128 && kPix == 16384, "k_hand_peaks: a row is two waves' worth of pixels, a run slot is a pixel pair");

// ---- boxes --------------------------------------------------------------------------------------------------------------------------
// util.handDetect's arithmetic in double and in its order (this file is compiled with -ffp-contract=off).  p1 shoulder, p2 elbow, p3 wrist.
__device__ __forceinline__ bool hand_box(const int32_t* kp, int p1, int p2, int p3, int H, int W, int& bx, int& by, int& bw) {
  const int x1 = kp[p1 * 2], y1 = kp[p1 * 2 + 1], x2 = kp[p2 * 2], y2 = kp[p2 * 2 + 1], x3 = kp[p3 * 2], y3 = kp[p3 * 2 + 1];
  if (x1 < 0 || y1 < 0 || x2 < 0 || y2 < 0 || x3 < 0 || y3 < 0) return false;   // a missing part is -1
  double x = (double)x3 + 0.33 * (double)(x3 - x2);
  double y = (double)y3 + 0.33 * (double)(y3 - y2);
  const double dwe = sqrt((double)((x3 - x2) * (x3 - x2) + (y3 - y2) * (y3 - y2)));
  const double des = sqrt((double)((x2 - x1) * (x2 - x1) + (y2 - y1) * (y2 - y1)));
  const double scaled = 0.9 * des;
  double width = 1.5 * (dwe > scaled ? dwe : scaled);
  x -= width / 2.0;
  y -= width / 2.0;
  if (x < 0.0) x = 0.0;
  if (y < 0.0) y = 0.0;
  double w1 = width, w2 = width;
  if (x + width > (double)W) w1 = (double)W - x;
  if (y + width > (double)H) w2 = (double)H - y;
  width = w1 < w2 ? w1 : w2;
  if (!(width >= 20.0)) return false;
  bx = (int)x, by = (int)y, bw = (int)width;
  return true;
}

// The resize of a w x w crop to the four sides is restated unless INTER_AREA meets an exact integer ratio other than 2 at some scale:
// w a multiple of 184 from 552 on (w = 368 meets only the 2x ratio, at side 184).
__device__ __forceinline__ bool hand_resize_restated(int w) { return !(w % kBase == 0 && w / kBase >= 3); }

__global__ __launch_bounds__(64) void k_hand_boxes(const int32_t* __restrict__ keypoints, const int32_t* __restrict__ people, const int32_t* __restrict__ overflow_in,
                                                   int32_t* __restrict__ boxes, int32_t* __restrict__ slots, int32_t* __restrict__ overflow, int H, int W, int max_hands) {
  const int img = blockIdx.x, lane = threadIdx.x;
  int np = people[img];
  np = np < 0 ? 0 : (np > kMaxPeople ? kMaxPeople : np);
  const int32_t* kp = keypoints + ((int64_t)img * kMaxPeople + lane) * kParts * 2;
  int bx[2] = {0, 0}, by[2] = {0, 0}, bw[2] = {0, 0};
  bool has[2] = {false, false};
  if (lane < np) {
    has[0] = hand_box(kp, 5, 6, 7, H, W, bx[0], by[0], bw[0]);   // left
    has[1] = hand_box(kp, 2, 3, 4, H, W, bx[1], by[1], bw[1]);   // right
  }
  const unsigned long long ml = __ballot(has[0]), mr = __ballot(has[1]), below = (1ull << lane) - 1ull;
  const int count = __popcll(ml) + __popcll(mr);
  const int before = __popcll(ml & below) + __popcll(mr & below);
  int32_t* so = slots + (int64_t)img * max_hands * kSlot;
  bool flagged = false;
#pragma unroll
  for (int hd = 0; hd < 2; ++hd) {
    const int rank = before + (hd == 1 && has[0] ? 1 : 0);
    const int slot = has[hd] && rank < max_hands ? rank : -1;
    int32_t* bo = boxes + (((int64_t)img * kMaxPeople + lane) * 2 + hd) * 4;
    bo[0] = bx[hd], bo[1] = by[hd], bo[2] = bw[hd], bo[3] = slot;
    if (slot >= 0) {
      const bool ok = hand_resize_restated(bw[hd]);
      flagged = flagged || !ok;
      int32_t* s = so + slot * kSlot;
      s[0] = lane, s[1] = bx[hd], s[2] = by[hd], s[3] = bw[hd], s[4] = hd, s[5] = ok ? CA_HAND_MODE_RESIZE : CA_HAND_MODE_NONE, s[6] = 0, s[7] = 0;
    }
  }
  for (int e = lane; e < kMaxHands; e += 64) {
    if (e >= max_hands) break;
    if (e < count) continue;
    int32_t* s = so + e * kSlot;
    s[0] = -1, s[1] = 0, s[2] = 0, s[3] = 0, s[4] = 0, s[5] = CA_HAND_MODE_NONE, s[6] = 0, s[7] = 0;
  }
  const unsigned long long fmask = __ballot(flagged);
  if (lane == 0)
    overflow[img] = (overflow_in ? overflow_in[img] : 0) | (count > max_hands ? CA_POSE_OVERFLOW_HANDS : 0) | (fmask ? CA_POSE_OVERFLOW_HAND_RESIZE : 0);
}

// ---- crop ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// A slot whose crop can be read: ca_hand_boxes writes no other (an empty or skipped slot gets a constant input).
__device__ __forceinline__ bool slot_ok(const int32_t* sl, int H, int W, int wmax) {
  const int bx = sl[1], by = sl[2], bw = sl[3];
  return sl[0] >= 0 && sl[5] == CA_HAND_MODE_RESIZE && bw >= kMinBox && bw <= wmax && bx >= 0 && by >= 0 && bx + bw <= W && by + bw <= H;
}

// cv2.GaussianBlur(crop, (0, 0), 0.8) as the specification restates it: the seven float taps, the row sums and then their column sum in
// double (each from the first tap on), BORDER_REFLECT_101 inside the crop, one rounding (half to even) at the end.  A thread per pixel
// of the wmax x wmax square of a slot; blurred [slots, wmax, wmax, 3] keeps the frame's channel order.
__global__ __launch_bounds__(256) void k_hand_blur(const uint8_t* __restrict__ frames, const int32_t* __restrict__ slots, const double* __restrict__ taps,
                                                   uint8_t* __restrict__ blurred, int H, int W, int max_hands, int first, int wmax) {
  const int s = first + blockIdx.y;
  const int32_t* sl = slots + (int64_t)s * kSlot;
  if (!slot_ok(sl, H, W, wmax)) return;   // block-uniform
  const int bx = sl[1], by = sl[2], bw = sl[3];
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int py = idx / wmax, px = idx - py * wmax;
  if (py >= bw || px >= bw) return;
  const int img = s / max_hands;
  const uint8_t* src = frames + (((int64_t)img * H + by) * W + bx) * 3;
  int xs[kBlurTaps], ys[kBlurTaps];
#pragma unroll
  for (int k = 0; k < kBlurTaps; ++k) {
    int x = px + k - kBlurTaps / 2, y = py + k - kBlurTaps / 2;
    x = x < 0 ? -x : x, y = y < 0 ? -y : y;
    xs[k] = x >= bw ? 2 * (bw - 1) - x : x;
    ys[k] = y >= bw ? 2 * (bw - 1) - y : y;
  }
  double t[kBlurTaps];
#pragma unroll
  for (int k = 0; k < kBlurTaps; ++k) t[k] = taps[k];
  uint8_t* dst = blurred + (((int64_t)s * wmax + py) * wmax + px) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double a = 0.0;
#pragma unroll
    for (int ky = 0; ky < kBlurTaps; ++ky) {
      const uint8_t* row = src + (int64_t)ys[ky] * W * 3 + c;
      double r = t[0] * (double)row[xs[0] * 3];
#pragma unroll
      for (int kx = 1; kx < kBlurTaps; ++kx) r = r + t[kx] * (double)row[xs[kx] * 3];
      a = ky == 0 ? t[0] * r : a + t[ky] * r;
    }
    a = rint(a);
    dst[c] = (uint8_t)(a < 0.0 ? 0.0 : (a > 255.0 ? 255.0 : a));
  }
}

// cv2.resize of the blurred w x w crop to side x side, a thread per output pixel: INTER_LANCZOS4 (w <= side) in OpenCV's 11-bit fixed
// point, the exact 2x INTER_AREA (a + b + c + d + 2) >> 2, or INTER_AREA as fp32 weighted sums -- each the horizontal sums first, then
// their vertical sum, in the specification's order (the face stage's arithmetic).  The tables of this side, made on the host: lz_* for
// w = kMinBox .. min(side, side_max) (row w - kMinBox), ar_* for w = side + 1 .. side_max (row w - side - 1), `side` entries per row.
template <int DT>
__global__ __launch_bounds__(256) void k_hand_resize(const uint8_t* __restrict__ blurred, const int32_t* __restrict__ slots, u16* __restrict__ out,
                                                     const int32_t* __restrict__ lz_ofs, const short* __restrict__ lz_coef, const int32_t* __restrict__ ar_ofs,
                                                     const int32_t* __restrict__ ar_cnt, const float* __restrict__ ar_w, int H, int W, int first, int side, int side_max,
                                                     int wmax) {
  const int crop = blockIdx.y, s = first + crop;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= side * side) return;
  const int dy = idx / side, dx = idx - dy * side;
  u16* dst = out + ((int64_t)crop * side * side + idx) * 8;
  const int32_t* sl = slots + (int64_t)s * kSlot;
  const int bw = sl[3];
  if (!slot_ok(sl, H, W, wmax)) {   // (wmax == side_max: the tables reach every box that passes)
    st16(dst, (u32x4){0u, 0u, 0u, 0u});
    return;
  }
  const uint8_t* src = blurred + (int64_t)s * wmax * wmax * 3;
  const int64_t pitch = (int64_t)wmax * 3;
  int px[3];
  if (bw <= side) {
    const int32_t* xo = lz_ofs + (int64_t)(bw - kMinBox) * side;
    const short* xa = lz_coef + (int64_t)(bw - kMinBox) * side * kLzTaps;
    const int x0 = xo[dx], y0 = xo[dy];
    int acc[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < kLzTaps; ++k) {
      const uint8_t* row = src + (int64_t)clampi(y0 + k, 0, bw - 1) * pitch;
      int a0 = 0, a1 = 0, a2 = 0;
#pragma unroll
      for (int j = 0; j < kLzTaps; ++j) {
        const int sx = clampi(x0 + j, 0, bw - 1) * 3;
        const int a = xa[dx * kLzTaps + j];
        a0 += (int)row[sx] * a, a1 += (int)row[sx + 1] * a, a2 += (int)row[sx + 2] * a;
      }
      const int b = xa[dy * kLzTaps + k];
      acc[0] += a0 * b, acc[1] += a1 * b, acc[2] += a2 * b;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = clampi((acc[c] + (1 << 21)) >> 22, 0, 255);
  } else if (bw == 2 * side) {
    const uint8_t* r0 = src + (int64_t)(2 * dy) * pitch + 2 * dx * 3;
    const uint8_t* r1 = r0 + pitch;
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = ((int)r0[c] + (int)r0[3 + c] + (int)r1[c] + (int)r1[3 + c] + 2) >> 2;
  } else {
    const int64_t t = (int64_t)(bw - side - 1) * side;
    const int32_t* xo = ar_ofs + t;
    const int32_t* xc = ar_cnt + t;
    const float* xw = ar_w + t * kAreaTaps;
    const int x0 = xo[dx], nx = xc[dx], y0 = xo[dy], ny = xc[dy];
    float acc[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < kAreaTaps; ++k) {
      if (k >= ny) break;
      const int sy = y0 + k;
      if (sy < 0 || sy >= bw) continue;   // (the host's tables never leave the crop)
      const uint8_t* row = src + (int64_t)sy * pitch;
      float h0 = 0.f, h1 = 0.f, h2 = 0.f;
      for (int j = 0; j < kAreaTaps; ++j) {
        if (j >= nx) break;
        const int sx = x0 + j;
        if (sx < 0 || sx >= bw) continue;
        const float a = xw[dx * kAreaTaps + j];
        h0 = h0 + a * (float)row[sx * 3], h1 = h1 + a * (float)row[sx * 3 + 1], h2 = h2 + a * (float)row[sx * 3 + 2];
      }
      const float b = xw[dy * kAreaTaps + k];
      acc[0] = acc[0] + b * h0, acc[1] = acc[1] + b * h1, acc[2] = acc[2] + b * h2;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = rintf(acc[c]);   // half to even, as saturate_cast<uchar>(float)
      px[c] = (int)(v < 0.f ? 0.f : (v > 255.f ? 255.f : v));
    }
  }
  float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 3; ++c) f[c] = (float)px[2 - c] / 256.0f - 0.5f;   // BGR
  st16(dst, pack8<DT>(f));
}

// ---- maps ---------------------------------------------------------------------------------------------------------------------------
// heat of scale s: fp32 [slots, m, m, 24] with m = 23 (s + 1).  mats [2][230][128]: plane 0 the transposed A_s ([m][128]) of the four scales
// behind each other, plane 1 the transposed G A_s.  A block owns one (part, plane, slot): thread (x, half) keeps the 64 outputs of column
// x and rows 64 half .. 64 half + 63 in registers.  Per scale: the map to LDS, t[i][x] = sum_j H[i][j] M[x][j] to LDS (j upward), then
// out[y][x] += sum_i M[y][i] t[i][x] (i upward; M[y][i] is the same in every lane of a wave: scalar loads of contiguous rows).
__global__ __launch_bounds__(256) void k_hand_maps(const float* __restrict__ h0, const float* __restrict__ h1, const float* __restrict__ h2, const float* __restrict__ h3,
                                                   const float* __restrict__ mats, float* __restrict__ raw, float* __restrict__ smooth) {
  __shared__ float hs[kMapMax * kMapMax];
  __shared__ float ts[kMapMax * kSide];
  const int part = blockIdx.x, plane = blockIdx.y, slot = blockIdx.z, tid = threadIdx.x;
  const int x = tid & (kSide - 1), half = __builtin_amdgcn_readfirstlane(tid >> 7);   // (a wave lies within one half)
  float acc[64];
#pragma unroll
  for (int r = 0; r < 64; ++r) acc[r] = 0.f;
  int row0 = 0;
  for (int s = 0; s < kScales; ++s) {
    const int m = 23 * (s + 1);
    const float* heat = (s == 0 ? h0 : (s == 1 ? h1 : (s == 2 ? h2 : h3))) + (int64_t)slot * m * m * kHeatCols + part;
    const float* mt = mats + ((int64_t)plane * kMapRows + row0) * kSide;   // [m][128]
    __syncthreads();   // the previous scale's ts has been read
    for (int i = tid; i < m * m; i += 256) hs[i] = heat[(int64_t)i * kHeatCols];
    __syncthreads();
    for (int i = half; i < kMapMax; i += 2) {
      if (i >= m) break;
      float a = 0.f;
      for (int j = 0; j < kMapMax; ++j) {
        if (j >= m) break;
        a = fmaf(hs[i * m + j], mt[j * kSide + x], a);
      }
      ts[i * kSide + x] = a;
    }
    __syncthreads();
    const float* my = mt + half * 64;
    for (int i = 0; i < kMapMax; ++i) {
      if (i >= m) break;
      const float v = ts[i * kSide + x];
#pragma unroll
      for (int r = 0; r < 64; ++r) acc[r] = fmaf(my[i * kSide + r], v, acc[r]);
    }
    row0 += m;
  }
  float* dst = (plane ? smooth : raw) + ((int64_t)slot * kHandParts + part) * kPix + (int64_t)half * 64 * kSide + x;
#pragma unroll
  for (int r = 0; r < 64; ++r) dst[r * kSide] = acc[r] * 0.25f;
}

// ---- peaks --------------------------------------------------------------------------------------------------------------------------
// lab[p]: -1 outside the binary plane, else the parent of pixel p in the union-find forest.  A parent is never larger than its child and
// always lies in the child's component, so a walk to the root strictly descends (at most kPix - 1 steps) and the root of a finished
// component is its smallest index: its first pixel in raster order.
__device__ __forceinline__ int uf_find(volatile int* lab, int a) {
  for (int k = 0; k < kPix; ++k) {
    const int q = lab[a];
    if (q == a) break;
    a = q;
  }
  return a;
}

// Hooks the larger root under the smaller with atomicMin.  When another thread got there first (old != a), old is smaller than a and
// has to be joined with b as well (the min may have replaced it): the larger of the pair strictly descends on every retry, so 2 kPix
// retries are never reached.
__device__ __forceinline__ void uf_unite(int* lab, int a, int b) {
  for (int k = 0; k < 2 * kPix; ++k) {
    a = uf_find(lab, a), b = uf_find(lab, b);
    if (a == b) break;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = atomicMin(lab + a, b);
    if (old == a) break;
    a = old;
  }
}

__device__ __forceinline__ int run_slot(int p) { return (p >> 7) * 64 + ((p & 127) >> 1); }   // two run starts of a row are never neighbours

__global__ __launch_bounds__(1024) void k_hand_peaks(const float* __restrict__ raw, const float* __restrict__ smooth, const int32_t* __restrict__ slots,
                                                     int32_t* __restrict__ points, int32_t* __restrict__ peaks, double* __restrict__ mass, int H, int W, int max_hands) {
  __shared__ int lab[kPix];            // 64 KiB
  __shared__ double rsum[kPix / 2];    // 64 KiB: the sum of a run at the slot of its first pixel; the root's slot ends as the component's mass
  __shared__ double red_d[16];
  __shared__ float red_f[16];
  __shared__ int red_i[16];
  __shared__ int win_s;
  const int part = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* rp = raw + ((int64_t)s * kHandParts + part) * kPix;
  const float* sp = smooth + ((int64_t)s * kHandParts + part) * kPix;
  // binary = smooth > 0.05
  int any = 0;
  for (int p = tid; p < kPix; p += 1024) {
    const bool in = (double)sp[p] > 0.05;
    lab[p] = in ? p : -1;
    any |= in;
  }
  any = __syncthreads_or(any);
  int win = -1;
  double win_mass = 0.0;
  if (any) {   // block-uniform
    // every pixel starts under the first pixel of its horizontal run
    int start[kPix / 1024];
#pragma unroll
    for (int k = 0; k < kPix / 1024; ++k) {
      const int p = tid + k * 1024;
      int q = p;
      if (lab[p] >= 0)
        for (int t = 0; t < kSide - 1; ++t) {
          if ((q & (kSide - 1)) == 0 || lab[q - 1] < 0) break;
          --q;
        }
      start[k] = q;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPix / 1024; ++k) {
      const int p = tid + k * 1024;
      if (lab[p] >= 0) lab[p] = start[k];
    }
    __syncthreads();
    // the row above: its pixel straight above joins both diagonal ones already (they are in its run); else the two diagonals
    for (int p = tid; p < kPix; p += 1024) {
      if (p < kSide || lab[p] < 0) continue;
      const int up = p - kSide, xx = p & (kSide - 1);
      if (lab[up] >= 0) {
        uf_unite(lab, p, up);
      } else {
        if (xx > 0 && lab[up - 1] >= 0) uf_unite(lab, p, up - 1);
        if (xx < kSide - 1 && lab[up + 1] >= 0) uf_unite(lab, p, up + 1);
      }
    }
    __syncthreads();
    // flatten: every pixel under its root (a store replaces a parent by an ancestor, so concurrent walks stay right)
    for (int p = tid; p < kPix; p += 1024)
      if (lab[p] >= 0) lab[p] = uf_find(lab, p);
    __syncthreads();
    // the sum of every run, left to right, in double
    for (int p = tid; p < kPix; p += 1024) {
      const int xx = p & (kSide - 1);
      if (lab[p] < 0 || (xx > 0 && lab[p - 1] >= 0)) continue;
      double a = 0.0;
      for (int t = 0; t < kSide; ++t) {
        if (xx + t >= kSide || lab[p + t] < 0) break;
        a = a + (double)rp[p + t];
      }
      rsum[run_slot(p)] = a;
    }
    __syncthreads();
    // the masses: wave 0 takes the rows downward, lane j the run that starts in pixel pair j.  Per row the first run of a component adds
    // the row's runs of that component from left to right and then adds that to the root's slot: one fixed order, no floating-point atomics.
    if (wave == 0) {
      volatile double* vsum = rsum;
      for (int y = 0; y < kSide; ++y) {
        const int p0 = y * kSide + 2 * lane;
        const int l0 = lab[p0], l1 = lab[p0 + 1], lprev = lane ? lab[p0 - 1] : -1;
        int key = -1, pos = 0;
        if (l0 >= 0 && lprev < 0) key = l0, pos = p0;
        else if (l1 >= 0 && l0 < 0) key = l1, pos = p0 + 1;
        unsigned long long todo = __ballot(key >= 0);
        if (!todo) continue;   // wave-uniform
        const double val = key >= 0 ? vsum[run_slot(pos)] : 0.0;
        double a = 0.0;
        bool first = true;
        for (int t = 0; t < 64; ++t) {
          if (!todo) break;
          const int j = __ffsll((long long)todo) - 1;
          todo &= todo - 1ull;
          const int kj = __shfl(key, j);
          const double vj = __shfl(val, j);
          if (kj == key) {
            if (j < lane) first = false;
            a = a + vj;
          }
        }
        if (key >= 0 && first) {
          const int rs = run_slot(key);
          vsum[rs] = key == pos ? a : vsum[rs] + a;   // the root's own run is the first one of the component
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
    }
    __syncthreads();
    // the heaviest component, the first label among equals
    double bm = -INFINITY;
    int bp = INT_MAX;
    for (int p = tid; p < kPix; p += 1024) {
      if (lab[p] != p) continue;
      const double m = rsum[run_slot(p)];
      if (m > bm) bm = m, bp = p;
    }
    for (int d = 32; d >= 1; d >>= 1) {
      const double m2 = __shfl_down(bm, d);
      const int p2 = __shfl_down(bp, d);
      if (m2 > bm || (m2 == bm && p2 < bp)) bm = m2, bp = p2;
    }
    if (lane == 0) red_d[wave] = bm, red_i[wave] = bp;
    __syncthreads();
    if (tid == 0) {
      for (int k = 1; k < 16; ++k)
        if (red_d[k] > bm || (red_d[k] == bm && red_i[k] < bp)) bm = red_d[k], bp = red_i[k];
      win_s = bp == INT_MAX ? -1 : bp;
      red_d[0] = bp == INT_MAX ? 0.0 : bm;
    }
    __syncthreads();
    win = win_s;
    win_mass = red_d[0];
    __syncthreads();
  }
  // util.npmax of raw zeroed outside the winner: the first row-major maximum (an empty binary plane leaves all zeros: pixel 0)
  int bi = 0;
  if (win >= 0) {
    float bv = -INFINITY;
    bi = INT_MAX;
    for (int p = tid; p < kPix; p += 1024) {
      const float v = lab[p] == win ? rp[p] : 0.f;
      if (v > bv) bv = v, bi = p;
    }
    for (int d = 32; d >= 1; d >>= 1) {
      const float v2 = __shfl_down(bv, d);
      const int i2 = __shfl_down(bi, d);
      if (v2 > bv || (v2 == bv && i2 < bi)) bv = v2, bi = i2;
    }
    if (lane == 0) red_f[wave] = bv, red_i[wave] = bi;
    __syncthreads();
    if (tid == 0)
      for (int k = 1; k < 16; ++k)
        if (red_f[k] > bv || (red_f[k] == bv && red_i[k] < bi)) bv = red_f[k], bi = red_i[k];
    if (bi == INT_MAX) bi = 0;   // (only NaN inside the winner)
  }
  if (tid != 0) return;
  const int px = bi & (kSide - 1), py = bi >> 7;
  int32_t* pk = peaks + ((int64_t)s * kHandParts + part) * 2;
  pk[0] = px, pk[1] = py;
  mass[(int64_t)s * kHandParts + part] = win_mass;
  const int32_t* sl = slots + (int64_t)s * kSlot;
  const int person = sl[0], bx = sl[1], by = sl[2], bw = sl[3], hand = sl[4], mode = sl[5];
  if (person < 0 || person >= kMaxPeople || mode != CA_HAND_MODE_RESIZE || (hand != 0 && hand != 1) || bw < 1 || bx < 0 || by < 0 || bx + bw > W || by + bw > H) return;
  // x = int(float(x) * float(w) / 128.0); detect_hands: -1 if x < 1e-6 else x + box_x
  const int lx = (int)((double)px * (double)bw / 128.0), ly = (int)((double)py * (double)bw / 128.0);
  const int img = s / max_hands;
  int32_t* pt = points + (((((int64_t)img * kMaxPeople + person) * 2 + hand) * kHandParts) + part) * 2;
  pt[0] = lx > 0 ? lx + bx : -1;
  pt[1] = ly > 0 ? ly + by : -1;
}

inline bool frame_ok(int32_t images, int32_t h, int32_t w) { return images >= 1 && images <= 65535 && h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide; }
inline bool hands_ok(int32_t images, int32_t max_hands) { return max_hands >= 1 && max_hands <= kMaxHands && (int64_t)images * max_hands <= 65535; }

}  // namespace

extern "C" int ca_hand_boxes(const int32_t* keypoints, const int32_t* people, const int32_t* overflow_in, int32_t* boxes, int32_t* slots, int32_t* overflow,
                             int32_t images, int32_t h, int32_t w, int32_t max_hands, void* stream) {
  CA_REQUIRE(keypoints && people && boxes && slots && overflow, "ca_hand_boxes: keypoints, people, boxes, slots and overflow are required");
  CA_REQUIRE(frame_ok(images, h, w), "ca_hand_boxes: images=%d h=%d w=%d (images in 1 .. 65535, h and w in 1 .. %d)", images, h, w, kMaxSide);
  CA_REQUIRE(hands_ok(images, max_hands), "ca_hand_boxes: max_hands=%d (1 .. %d, images * max_hands <= 65535)", max_hands, kMaxHands);
  CA_REQUIRE((((uintptr_t)keypoints | (uintptr_t)people | (uintptr_t)overflow_in | (uintptr_t)boxes | (uintptr_t)slots | (uintptr_t)overflow) & 3) == 0,
             "ca_hand_boxes: every pointer must be 4-byte aligned");
  hipLaunchKernelGGL(k_hand_boxes, dim3((unsigned)images), dim3(64), 0, (hipStream_t)stream, keypoints, people, overflow_in, boxes, slots, overflow, (int)h, (int)w,
                     (int)max_hands);
  CA_CHECK_LAUNCH("ca_hand_boxes");
  return CA_OK;
}

extern "C" int ca_hand_crop(const uint8_t* frames, const int32_t* slots, const double* taps, uint8_t* blurred, void* out, const int32_t* lz_ofs, const int16_t* lz_coef,
                            const int32_t* ar_ofs, const int32_t* ar_cnt, const float* ar_w, int32_t images, int32_t h, int32_t w, int32_t max_hands, int32_t first,
                            int32_t crops, int32_t side, int32_t side_max, int32_t blur, int32_t dtype, void* stream) {
  CA_REQUIRE(frames && slots && taps && blurred && out && lz_ofs && lz_coef, "ca_hand_crop: frames, slots, taps, blurred, out and the LANCZOS4 tables are required");
  CA_REQUIRE(frame_ok(images, h, w), "ca_hand_crop: images=%d h=%d w=%d (images in 1 .. 65535, h and w in 1 .. %d)", images, h, w, kMaxSide);
  CA_REQUIRE(hands_ok(images, max_hands), "ca_hand_crop: max_hands=%d (1 .. %d, images * max_hands <= 65535)", max_hands, kMaxHands);
  CA_REQUIRE(first >= 0 && crops >= 1 && (int64_t)first + crops <= (int64_t)images * max_hands, "ca_hand_crop: first=%d crops=%d of %d slots", first, crops,
             images * max_hands);
  CA_REQUIRE(side == kBase || side == 2 * kBase || side == 3 * kBase || side == 4 * kBase, "ca_hand_crop: side=%d (184, 368, 552 or 736)", side);
  CA_REQUIRE(side_max == (h < w ? h : w) && side_max >= kMinBox, "ca_hand_crop: side_max=%d (the frame's smaller side, the widest box: min(h=%d, w=%d) >= %d)", side_max, h,
             w, kMinBox);
  CA_REQUIRE(side_max <= side || (ar_ofs && ar_cnt && ar_w), "ca_hand_crop: side_max=%d > side=%d needs the INTER_AREA tables", side_max, side);
  CA_REQUIRE((int64_t)crops * side * side * 16 <= (int64_t)0x7FFFFF00, "ca_hand_crop: crops=%d side=%d: out would pass 2^31 bytes", crops, side);
  CA_REQUIRE(blur == 0 || blur == 1, "ca_hand_crop: blur=%d (0 or 1)", blur);
  CA_REQUIRE(dtype == CA_BF16 || dtype == CA_F16, "ca_hand_crop: dtype %d", dtype);
  CA_REQUIRE(((uintptr_t)out & 15) == 0 && ((uintptr_t)taps & 7) == 0 && (((uintptr_t)slots | (uintptr_t)lz_ofs | (uintptr_t)ar_ofs | (uintptr_t)ar_cnt | (uintptr_t)ar_w) & 3) == 0 &&
                 ((uintptr_t)lz_coef & 1) == 0,
             "ca_hand_crop: out must be 16-byte aligned, taps 8-byte, slots and the 32-bit tables 4-byte, lz_coef 2-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int wmax = side_max;
  if (blur)
    hipLaunchKernelGGL(k_hand_blur, dim3((unsigned)(((int64_t)wmax * wmax + 255) / 256), (unsigned)crops), dim3(256), 0, st, frames, slots, taps, blurred, (int)h, (int)w,
                       (int)max_hands, (int)first, wmax);
  const dim3 grid((unsigned)((side * side + 255) / 256), (unsigned)crops), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_hand_resize<DT>, grid, block, 0, st, (const uint8_t*)blurred, slots, (u16*)out, lz_ofs, (const short*)lz_coef, ar_ofs, ar_cnt, ar_w, (int)h,
                       (int)w, (int)first, (int)side, (int)side_max, wmax));
  CA_CHECK_LAUNCH("ca_hand_crop");
  return CA_OK;
}

extern "C" int ca_hand_maps(const float* heat184, const float* heat368, const float* heat552, const float* heat736, const float* mats, float* raw, float* smooth,
                            int32_t slots, void* stream) {
  CA_REQUIRE(heat184 && heat368 && heat552 && heat736 && mats && raw && smooth, "ca_hand_maps: the four heat tensors, mats, raw and smooth are required");
  CA_REQUIRE(slots >= 1 && slots <= 65535, "ca_hand_maps: slots=%d (1 .. 65535)", slots);
  CA_REQUIRE((((uintptr_t)heat184 | (uintptr_t)heat368 | (uintptr_t)heat552 | (uintptr_t)heat736 | (uintptr_t)mats | (uintptr_t)raw | (uintptr_t)smooth) & 3) == 0,
             "ca_hand_maps: every pointer must be 4-byte aligned");
  hipLaunchKernelGGL(k_hand_maps, dim3(kHandParts, 2, (unsigned)slots), dim3(256), 0, (hipStream_t)stream, heat184, heat368, heat552, heat736, mats, raw, smooth);
  CA_CHECK_LAUNCH("ca_hand_maps");
  return CA_OK;
}

extern "C" int ca_hand_peaks(const float* raw, const float* smooth, const int32_t* slots, int32_t* points, int32_t* peaks, double* mass, int32_t images,
                             int32_t max_hands, int32_t h, int32_t w, void* stream) {
  CA_REQUIRE(raw && smooth && slots && points && peaks && mass, "ca_hand_peaks: raw, smooth, slots, points, peaks and mass are required");
  CA_REQUIRE(frame_ok(images, h, w), "ca_hand_peaks: images=%d h=%d w=%d (images in 1 .. 65535, h and w in 1 .. %d)", images, h, w, kMaxSide);
  CA_REQUIRE(hands_ok(images, max_hands), "ca_hand_peaks: max_hands=%d (1 .. %d, images * max_hands <= 65535)", max_hands, kMaxHands);
  CA_REQUIRE((((uintptr_t)raw | (uintptr_t)smooth | (uintptr_t)slots | (uintptr_t)points | (uintptr_t)peaks) & 3) == 0 && ((uintptr_t)mass & 7) == 0,
             "ca_hand_peaks: mass must be 8-byte aligned, the other pointers 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(points, 0xFF, (size_t)images * kMaxPeople * 2 * kHandParts * 2 * 4, st);   // every point -1
  if (e != hipSuccess) CA_FAIL(CA_ERR_LAUNCH, "ca_hand_peaks: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(k_hand_peaks, dim3(kHandParts, (unsigned)(images * max_hands)), dim3(1024), 0, st, raw, smooth, slots, points, peaks, mass, (int)h, (int)w,
                     (int)max_hands);
  CA_CHECK_LAUNCH("ca_hand_peaks");
  return CA_OK;
}
