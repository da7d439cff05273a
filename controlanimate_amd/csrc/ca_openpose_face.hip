// Added to ABI v16: the face stage of the OpenPose annotator (controlanimate_amd/openpose_face.py: FaceStage; the specification is
// tests/face_ref.py, restated from the published controlnet_aux open_pose/{__init__,face,util}.py and OpenCV's resize).  The face network
// itself runs on ca_conv3x3 / ca_maxpool2x2 / ca_gemm / ca_conv7x7 / ca_copy_cols; around it the stage needs:
//
//   boxes   k_face_boxes   per frame, one wave, a lane per person: util.faceDetect in integer arithmetic on half pixels (the factors are 3.0
//                          and 1.5), the slots of the first max_faces people with a box (a ballot and a prefix count: person order), the
//                          resize mode of each slot, the overflow bits
//   crop    k_face_crop    per (two output rows, crop): cv2.resize of the crop to 384 x 384 through host-made tables indexed by the crop's
//                          side -- INTER_LANCZOS4 in OpenCV's 11-bit fixed point, INTER_AREA as fp32 weighted sums.  The horizontal pass of
//                          the source rows under the two output rows goes to LDS, the vertical pass reads it: the operation order of
//                          the specification.  No sine or cosine on the device.
//   peaks   k_face_peaks   per (part, crop): the align-corners bilinear value of every crop pixel from the 48 x 48 map in LDS, the largest one
//                          above 0.05 at its first row-major position; the upsampled plane is never written
//
// No launch depends on device data on the host side: the stage can be captured in a hipGraph.  The drawing is ca_pose_draw_faces
// (ca_openpose.hip).
#include "ca_common.h"
#include "ca_annot.h"

#include <climits>

namespace {

constexpr int kParts = 18, kMaxPeople = CA_POSE_MAX_PEOPLE;
constexpr int kSize = CA_FACE_SIZE, kHeat = CA_FACE_HEAT, kFaceParts = CA_FACE_PARTS, kHeatCols = 72;
constexpr int kMinSide = CA_FACE_MIN_SIDE, kMaxSide = 2048, kSlot = CA_FACE_SLOT_INTS, kTaps = 8;
constexpr int kRowsOut = 2;   // output rows of a block of k_face_crop
constexpr int kRowsIn = 13;   // source rows under them: INTER_AREA at most 2 * 2048 / 384 + 2, INTER_LANCZOS4 (hc + wc <= 768) at most 2 * 2 + 8
static_assert(kMaxPeople == 64, "k_face_boxes keeps one person per lane of a wave");
static_assert(kRowsIn * kSize * 3 * 4 <= 65536, "the horizontal sums of a block must fit in LDS");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int absi(int v) { return v < 0 ? -v : v; }

// ---- boxes --------------------------------------------------------------------------------------------------------------------------
// Every length is kept doubled: width = max(3.0 d, 1.5 d') is the integer w2 / 2, x = nose.x - width is x2 / 2.  int(x), int(y) and
// int(width) of the non-negative results are the shifts.
__global__ __launch_bounds__(64) void k_face_boxes(const int32_t* __restrict__ keypoints, const int32_t* __restrict__ people, const int32_t* __restrict__ overflow_in,
                                                   int32_t* __restrict__ boxes, int32_t* __restrict__ slots, int32_t* __restrict__ overflow, int H, int W, int max_faces) {
  const int img = blockIdx.x, lane = threadIdx.x;
  int np = people[img];
  np = np < 0 ? 0 : (np > kMaxPeople ? kMaxPeople : np);
  const int32_t* kp = keypoints + ((int64_t)img * kMaxPeople + lane) * kParts * 2;
  int bx = 0, by = 0, bw = 0;
  bool has = false;
  if (lane < np) {
    const int nx = kp[0], ny = kp[1];
    if (nx >= 0 && ny >= 0 && nx < W && ny < H) {
      int w2 = 0;
      bool any = false;
      for (int q = 14; q < 18; ++q) {
        const int px = kp[q * 2], py = kp[q * 2 + 1];
        if (px < 0 || py < 0 || px >= W || py >= H) continue;
        const int dx = absi(nx - px), dy = absi(ny - py);
        const int d = (q < 16 ? 6 : 3) * (dx > dy ? dx : dy);
        w2 = d > w2 ? d : w2;
        any = true;
      }
      if (any) {
        int x2 = 2 * nx - w2, y2 = 2 * ny - w2;
        x2 = x2 < 0 ? 0 : x2;
        y2 = y2 < 0 ? 0 : y2;
        int wa = 2 * w2, wb = 2 * w2;
        if (x2 + w2 > 2 * W) wa = 2 * W - x2;   // (the published test uses width, not 2 * width)
        if (y2 + w2 > 2 * H) wb = 2 * H - y2;
        const int ww = wa < wb ? wa : wb;
        if (ww >= 40) has = true, bx = x2 >> 1, by = y2 >> 1, bw = ww >> 1;
      }
    }
  }
  const unsigned long long mask = __ballot(has);
  const int count = __popcll(mask);
  const int rank = __popcll(mask & ((1ull << lane) - 1ull));
  const int slot = has && rank < max_faces ? rank : -1;
  int mode = CA_FACE_MODE_NONE, hc = 0, wc = 0;
  bool flagged = false;
  if (has) {
    hc = bw < H - by ? bw : H - by;
    wc = bw < W - bx ? bw : W - bx;
    if (hc + wc > 2 * kSize) {   // k = 768 / (hc + wc) < 1: INTER_AREA
      if (hc < kSize || wc < kSize) flagged = true;   // an axis grows: OpenCV takes another path
      else if (hc % kSize == 0 && wc % kSize == 0) flagged = true;   // both scales integers (one of them >= 2 here): the fast path
      else mode = CA_FACE_MODE_AREA;
    } else {
      mode = CA_FACE_MODE_LANCZOS4;
    }
  }
  int32_t* bo = boxes + ((int64_t)img * kMaxPeople + lane) * 4;
  bo[0] = bx, bo[1] = by, bo[2] = bw, bo[3] = slot;
  int32_t* so = slots + (int64_t)img * max_faces * kSlot;
  if (slot >= 0) {
    int32_t* s = so + slot * kSlot;
    s[0] = lane, s[1] = bx, s[2] = by, s[3] = bw, s[4] = hc, s[5] = wc, s[6] = mode, s[7] = 0;
  }
  if (lane < max_faces && lane >= count) {
    int32_t* s = so + lane * kSlot;
    s[0] = -1, s[1] = 0, s[2] = 0, s[3] = 0, s[4] = 0, s[5] = 0, s[6] = CA_FACE_MODE_NONE, s[7] = 0;
  }
  const unsigned long long fmask = __ballot(flagged && slot >= 0);
  if (lane == 0)
    overflow[img] = (overflow_in ? overflow_in[img] : 0) | (count > max_faces ? CA_POSE_OVERFLOW_FACES : 0) | (fmask ? CA_POSE_OVERFLOW_FACE_RESIZE : 0);
}

// ---- crop ---------------------------------------------------------------------------------------------------------------------------
// hbuf [rows][384][3]: the horizontal sums of the source rows lo .. lo + rows - 1 of the crop, int32 (INTER_LANCZOS4) or fp32
// (INTER_AREA).  The tables of side s start at (s - CA_FACE_MIN_SIDE) * 384 (LANCZOS4) and (s - 384) * 384 (AREA) entries.
template <int DT>
__global__ __launch_bounds__(256) void k_face_crop(const uint8_t* __restrict__ frames, const int32_t* __restrict__ slots, u16* __restrict__ out,
                                                   const int32_t* __restrict__ lz_ofs, const short* __restrict__ lz_coef, const int32_t* __restrict__ ar_ofs,
                                                   const int32_t* __restrict__ ar_cnt, const float* __restrict__ ar_w, int H, int W, int max_faces, int first,
                                                   int side_max) {
  __shared__ int32_t hbuf[kRowsIn * kSize * 3];
  const int crop = blockIdx.y, dy0 = blockIdx.x * kRowsOut, tid = threadIdx.x;
  const int s = first + crop;
  const int32_t* sl = slots + (int64_t)s * kSlot;
  const int img = s / max_faces;
  const int bx = sl[1], by = sl[2], hc = sl[4], wc = sl[5];
  int mode = sl[6];
  // (ca_face_boxes never writes a slot that fails these; a slot that does is treated as empty: no read leaves the frame or the tables)
  if (sl[0] < 0 || (mode != CA_FACE_MODE_LANCZOS4 && mode != CA_FACE_MODE_AREA) || hc < kMinSide || wc < kMinSide || hc > side_max || wc > side_max || bx < 0 ||
      by < 0 || bx + wc > W || by + hc > H || (mode == CA_FACE_MODE_AREA && (hc < kSize || wc < kSize)) ||
      (mode == CA_FACE_MODE_LANCZOS4 && hc + wc > 2 * kSize))   // (the host checks the kRowsIn span of the LANCZOS4 tables for these sides only)
    mode = CA_FACE_MODE_NONE;
  u16* dst = out + ((int64_t)crop * kSize + dy0) * kSize * 8;
  if (mode == CA_FACE_MODE_NONE) {   // block-uniform
    for (int i = tid; i < kRowsOut * kSize; i += 256) st16(dst + (int64_t)i * 8, (u32x4){0u, 0u, 0u, 0u});
    return;
  }
  const uint8_t* src = frames + (((int64_t)img * H + by) * W + bx) * 3;
  const int64_t pitch = (int64_t)W * 3;
  if (mode == CA_FACE_MODE_LANCZOS4) {
    const int32_t* xo = lz_ofs + (int64_t)(wc - kMinSide) * kSize;
    const short* xa = lz_coef + (int64_t)(wc - kMinSide) * kSize * kTaps;
    const int32_t* yo = lz_ofs + (int64_t)(hc - kMinSide) * kSize;
    const short* yb = lz_coef + (int64_t)(hc - kMinSide) * kSize * kTaps;
    const int lo = clampi(yo[dy0], 0, hc - 1), hi = clampi(yo[dy0 + kRowsOut - 1] + kTaps - 1, 0, hc - 1);
    int rows = hi - lo + 1;
    rows = rows < 1 ? 1 : (rows > kRowsIn ? kRowsIn : rows);   // (openpose_face.resize_tables refuses tables that span more: only LDS safety here)
    for (int i = tid; i < rows * kSize; i += 256) {
      const int r = i / kSize, dx = i - r * kSize;
      const uint8_t* row = src + (int64_t)(lo + r) * pitch;
      const int x0 = xo[dx];
      int a0 = 0, a1 = 0, a2 = 0;
#pragma unroll
      for (int j = 0; j < kTaps; ++j) {
        const int sx = clampi(x0 + j, 0, wc - 1) * 3;
        const int a = xa[dx * kTaps + j];
        a0 += (int)row[sx] * a, a1 += (int)row[sx + 1] * a, a2 += (int)row[sx + 2] * a;
      }
      hbuf[i * 3] = a0, hbuf[i * 3 + 1] = a1, hbuf[i * 3 + 2] = a2;
    }
    __syncthreads();
    for (int i = tid; i < kRowsOut * kSize; i += 256) {
      const int r = i / kSize, dx = i - r * kSize, dy = dy0 + r;
      const int y0 = yo[dy];
      int acc[3] = {0, 0, 0};
#pragma unroll
      for (int k = 0; k < kTaps; ++k) {
        const int sy = clampi(clampi(y0 + k, 0, hc - 1) - lo, 0, rows - 1);
        const int b = yb[dy * kTaps + k];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += hbuf[(sy * kSize + dx) * 3 + c] * b;
      }
      float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 3; ++c) f[c] = (float)clampi((acc[2 - c] + (1 << 21)) >> 22, 0, 255) / 256.0f - 0.5f;   // BGR
      st16(dst + (int64_t)i * 8, pack8<DT>(f));
    }
    return;
  }
  const int32_t* xo = ar_ofs + (int64_t)(wc - kSize) * kSize;
  const int32_t* xc = ar_cnt + (int64_t)(wc - kSize) * kSize;
  const float* xw = ar_w + (int64_t)(wc - kSize) * kSize * kTaps;
  const int32_t* yo = ar_ofs + (int64_t)(hc - kSize) * kSize;
  const int32_t* yc = ar_cnt + (int64_t)(hc - kSize) * kSize;
  const float* yw = ar_w + (int64_t)(hc - kSize) * kSize * kTaps;
  float* hb = (float*)hbuf;
  const int lo = clampi(yo[dy0], 0, hc - 1), hi = clampi(yo[dy0 + kRowsOut - 1] + yc[dy0 + kRowsOut - 1] - 1, 0, hc - 1);
  int rows = hi - lo + 1;
  rows = rows < 1 ? 1 : (rows > kRowsIn ? kRowsIn : rows);   // (openpose_face.resize_tables refuses tables that span more: only LDS safety here)
  for (int i = tid; i < rows * kSize; i += 256) {
    const int r = i / kSize, dx = i - r * kSize;
    const uint8_t* row = src + (int64_t)(lo + r) * pitch;
    const int x0 = xo[dx], nx = xc[dx];
    float h0 = 0.f, h1 = 0.f, h2 = 0.f;
    for (int j = 0; j < kTaps; ++j) {
      if (j >= nx) break;
      const int sx = x0 + j;
      if (sx < 0 || sx >= wc) continue;   // (the host's tables never leave the crop)
      const float a = xw[dx * kTaps + j];
      h0 = h0 + a * (float)row[sx * 3], h1 = h1 + a * (float)row[sx * 3 + 1], h2 = h2 + a * (float)row[sx * 3 + 2];
    }
    hb[i * 3] = h0, hb[i * 3 + 1] = h1, hb[i * 3 + 2] = h2;
  }
  __syncthreads();
  for (int i = tid; i < kRowsOut * kSize; i += 256) {
    const int r = i / kSize, dx = i - r * kSize, dy = dy0 + r;
    const int y0 = yo[dy], ny = yc[dy];
    float acc[3] = {0.f, 0.f, 0.f};
    for (int j = 0; j < kTaps; ++j) {
      if (j >= ny) break;
      const int sy = y0 + j - lo;
      if (sy < 0 || sy >= rows) continue;
      const float b = yw[dy * kTaps + j];
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] = acc[c] + b * hb[(sy * kSize + dx) * 3 + c];
    }
    float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = rintf(acc[2 - c]);   // BGR; half to even, as saturate_cast<uchar>(float)
      v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
      f[c] = v / 256.0f - 0.5f;
    }
    st16(dst + (int64_t)i * 8, pack8<DT>(f));
  }
}

// ---- peaks --------------------------------------------------------------------------------------------------------------------------
// torch's upsample_bilinear2d with align_corners: source = dst * (47 / (side - 1)) in fp32, the weights 1 - l and l, the value
// my * (mx * a + lx * b) + ly * (mx * c + lx * d).  A thread's pixels ascend, so a strict comparison keeps its first maximum; the block's
// reduction prefers the lower index among equal values.
__global__ __launch_bounds__(256) void k_face_peaks(const float* __restrict__ heat, const int32_t* __restrict__ slots, int32_t* __restrict__ points, int H, int W,
                                                    int max_faces) {
  __shared__ float plane[kHeat * kHeat];
  __shared__ float red_v[256];
  __shared__ int red_i[256];
  const int part = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
  const int32_t* sl = slots + (int64_t)s * kSlot;
  const int person = sl[0], bx = sl[1], by = sl[2], hc = sl[4], wc = sl[5], mode = sl[6];
  // an empty slot, a skipped crop shape (CA_FACE_MODE_NONE), or a slot whose crop leaves the frame (ca_face_boxes writes none)
  if (person < 0 || person >= kMaxPeople || (mode != CA_FACE_MODE_LANCZOS4 && mode != CA_FACE_MODE_AREA) || hc < 1 || wc < 1 || bx < 0 || by < 0 || bx + wc > W ||
      by + hc > H)
    return;   // block-uniform: the person's row keeps its -1
  const int img = s / max_faces;
  const float* hp = heat + (int64_t)s * kHeat * kHeat * kHeatCols + part;
  for (int i = tid; i < kHeat * kHeat; i += 256) plane[i] = hp[(int64_t)i * kHeatCols];
  __syncthreads();
  const float sy = hc > 1 ? (float)(kHeat - 1) / (float)(hc - 1) : 0.f, sx = wc > 1 ? (float)(kHeat - 1) / (float)(wc - 1) : 0.f;
  const int total = hc * wc;
  float best = -INFINITY;
  int best_i = INT_MAX;
  for (int p = tid; p < total; p += 256) {
    const int y = p / wc, x = p - y * wc;
    const float fy = sy * (float)y, fx = sx * (float)x;
    int y0 = (int)fy, x0 = (int)fx;
    y0 = y0 > kHeat - 1 ? kHeat - 1 : y0;
    x0 = x0 > kHeat - 1 ? kHeat - 1 : x0;
    const int y1 = y0 + (y0 < kHeat - 1), x1 = x0 + (x0 < kHeat - 1);
    const float ly = fy - (float)y0, lx = fx - (float)x0, my = 1.f - ly, mx = 1.f - lx;
    const float v = my * (mx * plane[y0 * kHeat + x0] + lx * plane[y0 * kHeat + x1]) + ly * (mx * plane[y1 * kHeat + x0] + lx * plane[y1 * kHeat + x1]);
    if (v > 0.05f && v > best) best = v, best_i = p;
  }
  red_v[tid] = best, red_i[tid] = best_i;
  __syncthreads();
  for (int half = 128; half >= 1; half >>= 1) {
    if (tid < half) {
      const float v2 = red_v[tid + half];
      const int i2 = red_i[tid + half];
      if (v2 > red_v[tid] || (v2 == red_v[tid] && i2 < red_i[tid])) red_v[tid] = v2, red_i[tid] = i2;
    }
    __syncthreads();
  }
  if (tid == 0) {
    int px = -1, py = -1;
    const int win = red_i[0];
    if (win != INT_MAX) {
      const int y = win / wc, x = win - y * wc;
      px = x > 0 ? x + bx : -1;   // compute_peaks_from_heatmaps' coordinate < 1e-6 -> -1
      py = y > 0 ? y + by : -1;
    }
    int32_t* pt = points + ((((int64_t)img * kMaxPeople + person) * kFaceParts) + part) * 2;
    pt[0] = px, pt[1] = py;
  }
}

inline bool frame_ok(int32_t images, int32_t h, int32_t w) { return images >= 1 && images <= 65535 && h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide; }
inline bool faces_ok(int32_t images, int32_t max_faces) { return max_faces >= 1 && max_faces <= kMaxPeople && (int64_t)images * max_faces <= 65535; }

}  // namespace

extern "C" int ca_face_boxes(const int32_t* keypoints, const int32_t* people, const int32_t* overflow_in, int32_t* boxes, int32_t* slots, int32_t* overflow,
                             int32_t images, int32_t h, int32_t w, int32_t max_faces, void* stream) {
  CA_REQUIRE(keypoints && people && boxes && slots && overflow, "ca_face_boxes: keypoints, people, boxes, slots and overflow are required");
  CA_REQUIRE(frame_ok(images, h, w), "ca_face_boxes: images=%d h=%d w=%d (images in 1 .. 65535, h and w in 1 .. %d)", images, h, w, kMaxSide);
  CA_REQUIRE(faces_ok(images, max_faces), "ca_face_boxes: max_faces=%d (1 .. %d, images * max_faces <= 65535)", max_faces, kMaxPeople);
  CA_REQUIRE((((uintptr_t)keypoints | (uintptr_t)people | (uintptr_t)overflow_in | (uintptr_t)boxes | (uintptr_t)slots | (uintptr_t)overflow) & 3) == 0,
             "ca_face_boxes: every pointer must be 4-byte aligned");
  hipLaunchKernelGGL(k_face_boxes, dim3((unsigned)images), dim3(64), 0, (hipStream_t)stream, keypoints, people, overflow_in, boxes, slots, overflow, (int)h, (int)w,
                     (int)max_faces);
  CA_CHECK_LAUNCH("ca_face_boxes");
  return CA_OK;
}

extern "C" int ca_face_crop(const uint8_t* frames, const int32_t* slots, void* out, const int32_t* lz_ofs, const int16_t* lz_coef, const int32_t* ar_ofs,
                            const int32_t* ar_cnt, const float* ar_w, int32_t images, int32_t h, int32_t w, int32_t max_faces, int32_t first, int32_t crops,
                            int32_t side_max, int32_t dtype, void* stream) {
  CA_REQUIRE(frames && slots && out && lz_ofs && lz_coef && ar_ofs && ar_cnt && ar_w, "ca_face_crop: frames, slots, out and the five tables are required");
  CA_REQUIRE(frame_ok(images, h, w), "ca_face_crop: images=%d h=%d w=%d (images in 1 .. 65535, h and w in 1 .. %d)", images, h, w, kMaxSide);
  CA_REQUIRE(faces_ok(images, max_faces), "ca_face_crop: max_faces=%d (1 .. %d, images * max_faces <= 65535)", max_faces, kMaxPeople);
  CA_REQUIRE(first >= 0 && crops >= 1 && (int64_t)first + crops <= (int64_t)images * max_faces, "ca_face_crop: first=%d crops=%d of %d slots", first, crops,
             images * max_faces);
  CA_REQUIRE(side_max >= kSize && side_max <= kMaxSide && h <= side_max && w <= side_max,
             "ca_face_crop: side_max=%d (the tables reach from %d to side_max: %d .. %d, and no less than h=%d and w=%d)", side_max, kMinSide, kSize, kMaxSide, h, w);
  CA_REQUIRE((int64_t)crops * kSize * kSize * 16 <= (int64_t)0x7FFFFF00, "ca_face_crop: crops=%d: out would pass 2^31 bytes", crops);
  CA_REQUIRE(dtype_ok(dtype), "ca_face_crop: dtype %d", dtype);
  CA_REQUIRE(((uintptr_t)out & 15) == 0 && (((uintptr_t)slots | (uintptr_t)lz_ofs | (uintptr_t)ar_ofs | (uintptr_t)ar_cnt | (uintptr_t)ar_w) & 3) == 0 &&
                 ((uintptr_t)lz_coef & 1) == 0,
             "ca_face_crop: out must be 16-byte aligned, slots and the 32-bit tables 4-byte aligned, lz_coef 2-byte aligned");
  const dim3 grid(kSize / kRowsOut, (unsigned)crops), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_face_crop<DT>, grid, block, 0, (hipStream_t)stream, frames, slots, (u16*)out, lz_ofs, (const short*)lz_coef, ar_ofs, ar_cnt, ar_w, (int)h,
                       (int)w, (int)max_faces, (int)first, (int)side_max));
  CA_CHECK_LAUNCH("ca_face_crop");
  return CA_OK;
}

extern "C" int ca_face_peaks(const float* heat, const int32_t* slots, int32_t* points, int32_t images, int32_t max_faces, int32_t h, int32_t w, void* stream) {
  CA_REQUIRE(heat && slots && points, "ca_face_peaks: heat, slots and points are required");
  CA_REQUIRE(frame_ok(images, h, w), "ca_face_peaks: images=%d h=%d w=%d (images in 1 .. 65535, h and w in 1 .. %d)", images, h, w, kMaxSide);
  CA_REQUIRE(faces_ok(images, max_faces), "ca_face_peaks: max_faces=%d (1 .. %d, images * max_faces <= 65535)", max_faces, kMaxPeople);
  CA_REQUIRE((((uintptr_t)heat | (uintptr_t)slots | (uintptr_t)points) & 3) == 0, "ca_face_peaks: every pointer must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(points, 0xFF, (size_t)images * kMaxPeople * kFaceParts * 2 * 4, st);   // every point -1
  if (e != hipSuccess) CA_FAIL(CA_ERR_LAUNCH, "ca_face_peaks: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(k_face_peaks, dim3(kFaceParts, (unsigned)(images * max_faces)), dim3(256), 0, st, heat, slots, points, (int)h, (int)w, (int)max_faces);
  CA_CHECK_LAUNCH("ca_face_peaks");
  return CA_OK;
}
