// Added to ABI v16: the paste-back behind the GFPGAN face restorer (controlanimate_amd/face_paste.py: FacePaster; the specification is
// tests/facepaste_ref.py, restated from memory of facexlib's ParseNet and FaceRestoreHelper.paste_faces_to_input_image and of OpenCV's
// GaussianBlur / warpAffine).  None of the other entry points pads by reflection, blurs a float64 mask or blends through an inverse warp:
//
//   prep      k_parse_prep       uint8 faces [n,S,S,3] -> NHWC [n,S,S,32]: ((byte / 255) - 0.5) / 0.5 in fp32, rounded once; the channels
//                                reversed by flag; channels 3 .. 31 zero (the first convolution's weight is zero-padded to cin = 32)
//   conv      k_conv_reflect     Conv2d(k 3, s 1 | 2) behind ReflectionPad2d(1), optionally behind a nearest x2, as an implicit GEMM: a block
//                                owns TH x 16 output pixels x CT output channels and keeps the halo under them in LDS 32 input channels at
//                                a time.  The REFLECTION IS AN INDEX MAP AT TILE LOAD: tile pixel (r, c) is loaded from the reflected
//                                coordinate, so no padded tensor and no im2col exist.  With the x2 source the map runs on the upsampled
//                                plane and ends in a shift (coordinate >> 1): reflection there is replication of the source border, and
//                                the x2 plane is never written.  The weights [cout][3][3][cin] are the A operand, read from memory (L2)
//                                as fragments; MFMA 16x16x32; fp32 bias, optional residual, optional LeakyReLU(0.2), 16-bit or fp32 output.
//                                Any operand may be a RINGED tensor [n, H+2, W+2, C] whose interior is addressed (the ring route below)
//   mask      k_conv_reflect<EPI_MASK>  the last layer in one launch: the 64 -> 19 convolution (N padded to 32), the logits in registers,
//                                the first-maximum argmax across the four lanes that share a pixel, the colour map -> uint8 0 / 255
//   labels    k_parse_labels     the composed form's tail: fp32 logits [pixels, 32] -> the label and / or the 0 / 255 mask
//   ring      k_ring_fill        the one-pixel ring of [n, H+2, W+2, C] from its interior, by reflection or replication: a stride-1 layer
//                                can then run on the zero-padded ca_conv3x3 over the ringed tensor (its interior is right)
//   blur      k_blur_pass        cv2.GaussianBlur(mask, (101, 101), 11) twice on float64: four 1-D passes (row, column, row, column)
//                                through an LDS tile of 32 lines x (64 + 100) positions, BORDER_REFLECT_101 as an index map, the taps from
//                                a host-made table, the sum k0 x0 + sum_i k_i (x_-i + x_+i) for i = 1 .. 50 in that order with __dmul_rn /
//                                __dadd_rn (no contraction); the last pass zeroes the outer 10 rows / columns and divides by 255
//   paste     k_face_paste       one launch per window: an output pixel walks its frame's faces in order, samples the restored face in
//                                OpenCV's fixed point and the float64 mask bilinearly at the same coordinates, blends in a double register
//                                and truncates once.  The float64 frame never exists
//
// No launch depends on device data on the host side: the chain can be captured in a hipGraph.  No atomics: two runs give the same bits.
#include "ca_common.h"
#include "ca_annot.h"

namespace {

constexpr int PN_CPAD = 32;     // the prep's channel count
constexpr int PN_CLASSES = 19;
constexpr int RING_IN = 1, RING_OUT = 2, RING_RES = 4;

// pixel (y, x) of image img in a dense [n, h, w] or ringed [n, h + 2, w + 2] plane
__device__ __forceinline__ int64_t pix_index(int ring, int img, int h, int w, int y, int x) {
  return ring ? ((int64_t)img * (h + 2) + y + 1) * (w + 2) + x + 1 : ((int64_t)img * h + y) * w + x;
}

// ---- prep ------------------------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void k_parse_prep(const uint8_t* __restrict__ src, u16* __restrict__ dst, int64_t pixels, int s, int reverse, int ring) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= pixels) return;
  const int x = (int)(p % s), y = (int)((p / s) % s), img = (int)(p / ((int64_t)s * s));
  float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 3; ++c) f[c] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)src[p * 3 + (reverse ? 2 - c : c)], 255.0f), 0.5f), 0.5f);
  u16* d = dst + pix_index(ring, img, s, s, y, x) * PN_CPAD;
  st16(d, pack8<DT>(f));
  const u32x4 z = (u32x4){0u, 0u, 0u, 0u};
  st16(d + 8, z), st16(d + 16, z), st16(d + 24, z);
}

// ---- the reflected 3x3 convolution ------------------------------------------------------------------------------------------------------
// Output pixel (y, x) at tap (ty, tx) reads logical input pixel (S y - 1 + ty, S x - 1 + tx) of the lh x lw plane (the source, or its nearest
// x2), reflected at the plane's edge: -1 -> 1, lh -> lh - 2.  A block's four waves are WM (rows) x WN (halves of CT); a wave owns CTL rows of 16
// positions and 16 RT output channels, so it reuses a weight fragment for CTL rows and a row fragment for RT weight fragments.  The halo lies in
// LDS 32 input channels at a time, a pixel every 40 elements (80 bytes: the 16 lanes of a fragment row start on different 16-byte slots of the
// 256-byte bank row at stride 1; at stride 2 the lane pitch is 160 bytes and lanes l and l + 8 of a row share a slot -- a two-way conflict that
// is not measured yet).  MFMA 16x16x32: A = 16 output channels x 32 input channels of one tap; B = the 16 positions of one tile row; a lane ends
// up with 4 consecutive output channels of one position.
constexpr int CR_TW = 16, CR_KC = 32, CR_PITCH = CR_KC + 8;
enum { EPI_STORE = 0, EPI_MASK = 1 };

struct ReflArgs {
  const u16* x;
  const u16* wt;
  const float* bias;
  const u16* res;
  void* y;
  int h, w, cin, cout, gh, gw, tiles_x, tiles_y, leaky, out_f32, rings, classes;
};

template <int DT, int S, int UP, int WN, int RT, int CTL, int EPI>
__global__ __launch_bounds__(256) void k_conv_reflect(const ReflArgs a) {
  constexpr int WM = 4 / WN, TH = WM * CTL, HR = (TH - 1) * S + 3, HC = (CR_TW - 1) * S + 3, CT = 16 * RT * WN, PARTS = CR_KC / 8;
  __shared__ __attribute__((aligned(16))) u16 tile[HR * HC * CR_PITCH];
  const int cts = a.cout / CT;
  int b = blockIdx.x;
  const int ct = b % cts;
  b /= cts;
  const int bx = b % a.tiles_x;
  b /= a.tiles_x;
  const int by = b % a.tiles_y;
  const int img = b / a.tiles_y;
  const int y0 = by * TH, x0 = bx * CR_TW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, r16 = lane & 15;
  const int wm = wave % WM, wn = wave / WM;
  const int h = a.h, w = a.w, cin = a.cin, cout = a.cout, gh = a.gh, gw = a.gw;
  const int lh = UP ? 2 * h : h, lw = UP ? 2 * w : w;
  const int ch0 = ct * CT + wn * (16 * RT);
  const u16* wrow[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) wrow[t] = a.wt + (int64_t)(ch0 + t * 16 + r16) * 9 * cin + q * 8;
  f32x4 acc[RT][CTL];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int j = 0; j < CTL; ++j) acc[t][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  bool rowlive[CTL];
#pragma unroll
  for (int j = 0; j < CTL; ++j) rowlive[j] = y0 + wm * CTL + j < gh;  // wave-uniform

  for (int c0 = 0; c0 < cin; c0 += CR_KC) {
    if (c0) __syncthreads();
    for (int i = threadIdx.x; i < HR * HC * PARTS; i += 256) {
      const int pix = i / PARTS, part = i - pix * PARTS;
      const int r = pix / HC, c = pix - r * HC;
      int ly = S * y0 - 1 + r, lx = S * x0 - 1 + c;
      ly = ly < 0 ? -ly : ly, lx = lx < 0 ? -lx : lx;
      ly = ly >= lh ? 2 * lh - 2 - ly : ly, lx = lx >= lw ? 2 * lw - 2 - lx : lx;
      ly = min(max(ly, 0), lh - 1), lx = min(max(lx, 0), lw - 1);  // (a tile that hangs over the plane: those pixels feed no stored output)
      const int gy = UP ? ly >> 1 : ly, gx = UP ? lx >> 1 : lx;
      st16(tile + pix * CR_PITCH + part * 8, ld16(a.x + pix_index(a.rings & RING_IN, img, h, w, gy, gx) * cin + c0 + part * 8));
    }
    __syncthreads();
#pragma unroll 3
    for (int tap = 0; tap < 9; ++tap) {
      const int ty = tap / 3, tx = tap - ty * 3;
      u32x4 af[RT], bf[CTL];
#pragma unroll
      for (int t = 0; t < RT; ++t) af[t] = ld16(wrow[t] + tap * cin + c0);
#pragma unroll
      for (int j = 0; j < CTL; ++j) bf[j] = ld16(tile + (((wm * CTL + j) * S + ty) * HC + r16 * S + tx) * CR_PITCH + q * 8);
#pragma unroll
      for (int j = 0; j < CTL; ++j) {
        if (!rowlive[j]) continue;
#pragma unroll
        for (int t = 0; t < RT; ++t) acc[t][j] = Elem<DT>::mfma(af[t], bf[j], acc[t][j]);
      }
    }
  }
  const int gx = x0 + r16;
#pragma unroll
  for (int j = 0; j < CTL; ++j) {
    const int gy = y0 + wm * CTL + j;
    if (!rowlive[j]) continue;
    const bool inside = gx < gw;
    if (EPI == EPI_STORE) {
      if (!inside) continue;
      const int64_t opix = pix_index(a.rings & RING_OUT, img, gh, gw, gy, gx);
      const int64_t rpix = pix_index(a.rings & RING_RES, img, gh, gw, gy, gx);
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        const int ch = ch0 + t * 16 + q * 4;
        float f[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = acc[t][j][i] + a.bias[ch + i];
        if (a.res) {
          const u32x2 rv = *(const u32x2*)(a.res + rpix * cout + ch);
          f[0] += Elem<DT>::to_f((u16)(rv[0] & 0xffffu)), f[1] += Elem<DT>::to_f((u16)(rv[0] >> 16));
          f[2] += Elem<DT>::to_f((u16)(rv[1] & 0xffffu)), f[3] += Elem<DT>::to_f((u16)(rv[1] >> 16));
        }
        if (a.leaky) {
#pragma unroll
          for (int i = 0; i < 4; ++i) f[i] = f[i] > 0.f ? f[i] : 0.2f * f[i];
        }
        if (a.out_f32) {
          *(f32x4*)((float*)a.y + opix * cout + ch) = (f32x4){f[0], f[1], f[2], f[3]};
        } else {
          u32x2 v;
          v[0] = pack2<DT>(f[0], f[1]);
          v[1] = pack2<DT>(f[2], f[3]);
          *(u32x2*)((u16*)a.y + opix * cout + ch) = v;
        }
      }
    } else {
      // the pixel's 32 logits lie in the four lanes r16, r16 + 16, + 32, + 48 (channels t * 16 + q * 4 + i): the first maximum over the classes
      float best = -INFINITY;
      int bch = 0x7fffffff;
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int ch = t * 16 + q * 4 + i;
          const float v = acc[t][j][i] + a.bias[ch];
          if (ch < a.classes && (v > best || (v == best && ch < bch))) best = v, bch = ch;
        }
#pragma unroll
      for (int m = 16; m <= 32; m <<= 1) {
        const float ov = __shfl_xor(best, m, 64);
        const int oc = __shfl_xor(bch, m, 64);
        if (ov > best || (ov == best && oc < bch)) best = ov, bch = oc;
      }
      if (inside && q == 0) ((uint8_t*)a.y)[((int64_t)img * gh + gy) * gw + gx] = (bch == 0 || bch == 14 || bch >= 16) ? 0 : 255;
    }
  }
}

template <int DT, int S, int UP, int CTLW1, int CTLW2>
void launch_reflect(const ReflArgs& a, int images, hipStream_t st) {
  // cout 32: one wave column of 32 channels; 64: two of 32; 128 and 256: two of 64 (CT = 128)
  const int ct = a.cout == 32 ? 32 : (a.cout == 64 ? 64 : 128);
  const int th = a.cout == 32 ? 4 * CTLW1 : 2 * CTLW2;
  ReflArgs b = a;
  b.tiles_x = ceil_div_i(a.gw, CR_TW), b.tiles_y = ceil_div_i(a.gh, th);
  const dim3 grid((unsigned)((int64_t)images * b.tiles_x * b.tiles_y * (a.cout / ct))), block(256);
  if (a.cout == 32) hipLaunchKernelGGL((k_conv_reflect<DT, S, UP, 1, 2, CTLW1, EPI_STORE>), grid, block, 0, st, b);
  else if (a.cout == 64) hipLaunchKernelGGL((k_conv_reflect<DT, S, UP, 2, 2, CTLW2, EPI_STORE>), grid, block, 0, st, b);
  else hipLaunchKernelGGL((k_conv_reflect<DT, S, UP, 2, 4, CTLW2, EPI_STORE>), grid, block, 0, st, b);
}

inline int refl_th(int cout, int stride) { return cout == 32 ? (stride == 2 ? 8 : 16) : 8; }

inline bool refl_c_ok(int c) { return c == 32 || c == 64 || c == 128 || c == 256; }

// bytes of a [n, h, w, c] operand of `elem` bytes per element, ringed or not
inline int64_t plane_bytes(int64_t n, int h, int w, int c, int ring, int elem) { return n * (h + (ring ? 2 : 0)) * (w + (ring ? 2 : 0)) * c * elem; }

// ---- labels -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_parse_labels(const float* __restrict__ logits, uint8_t* __restrict__ labels, uint8_t* __restrict__ mask, int64_t pixels,
                                                      int cols, int classes) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= pixels) return;
  const float* l = logits + p * cols;
  float best = l[0];
  int bch = 0;
  for (int c = 1; c < classes; ++c) {
    const float v = l[c];
    if (v > best) best = v, bch = c;
  }
  if (labels) labels[p] = (uint8_t)bch;
  if (mask) mask[p] = (bch == 0 || bch == 14 || bch >= 16) ? 0 : 255;
}

// ---- ring -------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ring_src(int t, int len, int reflect) { return t == 0 ? (reflect ? 2 : 1) : (t == len + 1 ? (reflect ? len - 1 : len) : t); }

__global__ __launch_bounds__(256) void k_ring_fill(u16* __restrict__ x, int64_t total, int h, int w, int c, int reflect) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cl = c >> 3;
  const int part = (int)(idx % cl);
  const int per = 2 * (w + 2) + 2 * h;
  const int k = (int)((idx / cl) % per);
  const int64_t img = idx / ((int64_t)cl * per);
  int ty, tx;
  if (k < w + 2) ty = 0, tx = k;
  else if (k < 2 * (w + 2)) ty = h + 1, tx = k - (w + 2);
  else if (k < 2 * (w + 2) + h) ty = k - 2 * (w + 2) + 1, tx = 0;
  else ty = k - 2 * (w + 2) - h + 1, tx = w + 1;
  const int sy = ring_src(ty, h, reflect), sx = ring_src(tx, w, reflect);
  u16* base = x + img * (h + 2) * (w + 2) * c + part * 8;
  st16(base + ((int64_t)ty * (w + 2) + tx) * c, ld16(base + ((int64_t)sy * (w + 2) + sx) * c));
}

// ---- blur -------------------------------------------------------------------------------------------------------------------------------
constexpr int BL_S = CA_FACE_ALIGN_SIZE, BL_R = 50, BL_LINES = 32, BL_SEG = 64, BL_ROWS = BL_SEG + 2 * BL_R, BL_LP = BL_LINES + 1, BL_EDGE = 10;

// One 1-D pass over [n, 512, 512]: COL = false sums along x (a line is a row), true along y (a line is a column).  A block owns 32 lines x 64
// positions; thread t owns line t % 32 and 8 positions, so the lanes of a wave read consecutive doubles of the tile.
template <typename SrcT, bool COL, bool LAST>
__global__ __launch_bounds__(256) void k_blur_pass(const SrcT* __restrict__ src, const double* __restrict__ taps, double* __restrict__ dst) {
  __shared__ double tile[BL_ROWS * BL_LP];
  __shared__ double kt[BL_R + 1];
  const int line0 = blockIdx.x * BL_LINES, p0 = blockIdx.y * BL_SEG;
  const int64_t plane = (int64_t)blockIdx.z * BL_S * BL_S;
  if (threadIdx.x <= BL_R) kt[threadIdx.x] = taps[threadIdx.x];
  for (int i = threadIdx.x; i < BL_ROWS * BL_LINES; i += 256) {
    int line, p;
    if (COL) p = i / BL_LINES, line = i - p * BL_LINES;   // consecutive threads: consecutive columns of one row
    else line = i / BL_ROWS, p = i - line * BL_ROWS;      // consecutive threads: consecutive pixels of one row
    int g = p0 - BL_R + p;
    g = g < 0 ? -g : g;
    g = g >= BL_S ? 2 * BL_S - 2 - g : g;                 // BORDER_REFLECT_101
    const int64_t at = COL ? (int64_t)g * BL_S + line0 + line : (int64_t)(line0 + line) * BL_S + g;
    tile[p * BL_LP + line] = (double)src[plane + at];
  }
  __syncthreads();
  const int line = threadIdx.x & (BL_LINES - 1), grp = threadIdx.x / BL_LINES;
#pragma unroll 1
  for (int o = 0; o < BL_SEG / 8; ++o) {
    const int p = grp * (BL_SEG / 8) + o;
    const double* t = tile + (p + BL_R) * BL_LP + line;
    double acc = __dmul_rn(kt[0], t[0]);
    for (int i = 1; i <= BL_R; ++i) acc = __dadd_rn(acc, __dmul_rn(kt[i], __dadd_rn(t[-i * BL_LP], t[i * BL_LP])));
    const int gp = p0 + p, gl = line0 + line;
    if (LAST) {
      const bool edge = gp < BL_EDGE || gp >= BL_S - BL_EDGE || gl < BL_EDGE || gl >= BL_S - BL_EDGE;
      acc = __ddiv_rn(edge ? 0.0 : acc, 255.0);
    }
    dst[plane + (COL ? (int64_t)gp * BL_S + gl : (int64_t)gl * BL_S + gp)] = acc;
  }
}

// ---- paste ------------------------------------------------------------------------------------------------------------------------------
constexpr int FP_S = CA_FACE_ALIGN_SIZE;

__device__ __forceinline__ void invert_affine(const double m[6], double out[6]) {  // cv2.invertAffineTransform, operation by operation (ca_retinaface.hip)
  double d = m[0] * m[4] - m[1] * m[3];
  d = d != 0.0 ? 1.0 / d : 0.0;
  const double a11 = m[4] * d, a22 = m[0] * d, a12 = m[1] * -d, a21 = m[3] * -d;
  out[0] = a11, out[1] = a12, out[2] = -a11 * m[2] - a12 * m[5];
  out[3] = a21, out[4] = a22, out[5] = -a21 * m[2] - a22 * m[5];
}

__device__ __forceinline__ int sat_int(double v) {  // saturate_cast<int>(double): round half to even, clamped
  return (int)fmin(fmax(rint(v), -2147483648.0), 2147483647.0);
}

__global__ __launch_bounds__(256) void k_face_paste(const uint8_t* __restrict__ bg, const uint8_t* __restrict__ restored, const double* __restrict__ masks,
                                                    const double* __restrict__ inverse, const int* __restrict__ count, uint8_t* __restrict__ out, int64_t total,
                                                    int h, int w, int max_faces, double offset) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int x = (int)(idx % w), y = (int)((idx / w) % h), img = (int)(idx / ((int64_t)w * h));
  double px[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) px[c] = (double)bg[idx * 3 + c];
  const int faces = min(max(count[img], 0), max_faces);
  for (int r = 0; r < faces; ++r) {
    const int slot = img * max_faces + r;
    double m[6], inv[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) m[i] = inverse[(int64_t)slot * 6 + i];
    m[2] = m[2] + offset, m[5] = m[5] + offset;
    invert_affine(m, inv);
    // the source coordinate in the 512 x 512 face, as cv2.warpAffine computes it (the sums wrap as 32-bit integers)
    const unsigned X0 = (unsigned)sat_int((inv[1] * (double)y + inv[2]) * 1024.0) + 16u, Y0 = (unsigned)sat_int((inv[4] * (double)y + inv[5]) * 1024.0) + 16u;
    const double xd = (double)x;
    const int X = (int)(X0 + (unsigned)sat_int(inv[0] * xd * 1024.0)) >> 5, Y = (int)(Y0 + (unsigned)sat_int(inv[3] * xd * 1024.0)) >> 5;
    const int sx = min(max(X >> 5, -32768), 32767), sy = min(max(Y >> 5, -32768), 32767), fx = X & 31, fy = Y & 31;
    if (sx < -1 || sx >= FP_S || sy < -1 || sy >= FP_S) continue;  // every tap outside: the face and its mask sample 0, the pixel stays
    const int wt[4] = {(32 - fy) * (32 - fx), (32 - fy) * fx, fy * (32 - fx), fy * fx};
    const uint8_t* face = restored + (int64_t)slot * FP_S * FP_S * 3;
    const double* mk = masks + (int64_t)slot * FP_S * FP_S;
    int acc[3] = {0, 0, 0};
    double ms = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int yy = sy + (t >> 1), xx = sx + (t & 1);
      const bool inside = yy >= 0 && yy < FP_S && xx >= 0 && xx < FP_S;
      const int at = inside ? yy * FP_S + xx : 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += (inside ? (int)face[at * 3 + c] : 0) * (wt[t] * 32);
      // the float table's weight (32 - fy)(32 - fx) / 1024 is exact; four products summed in double, in the taps' order
      const double prod = __dmul_rn(inside ? mk[at] : 0.0, (double)((float)wt[t] * (1.0f / 1024.0f)));
      ms = t == 0 ? prod : __dadd_rn(ms, prod);
    }
    const double keep = __dsub_rn(1.0, ms);
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = __dadd_rn(__dmul_rn(ms, (double)((acc[c] + (1 << 14)) >> 15)), __dmul_rn(keep, px[c]));
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) out[idx * 3 + c] = (uint8_t)(int)px[c];  // astype(uint8) of a value in [0, 255]: truncation
}

}  // namespace

extern "C" int ca_parse_prep(const uint8_t* faces, void* out, int32_t images, int32_t size, int32_t reverse, int32_t ring, int32_t dtype, void* stream) {
  CA_REQUIRE(faces && out, "ca_parse_prep: faces and out are required");
  CA_REQUIRE(sizes_ok(images, size, size) && plane_bytes(images, size, size, PN_CPAD, 1, 2) <= kMaxBytes,
             "ca_parse_prep: images=%d size=%d (each >= 1, the [images, size + 2, size + 2, 32] output below 2^31 bytes)", images, size);
  CA_REQUIRE((reverse == 0 || reverse == 1) && (ring == 0 || ring == 1), "ca_parse_prep: reverse=%d ring=%d (0 or 1)", reverse, ring);
  CA_REQUIRE(dtype_ok(dtype), "ca_parse_prep: dtype %d", dtype);
  CA_REQUIRE(((uintptr_t)out & 15) == 0, "ca_parse_prep: out must be 16-byte aligned");
  const int64_t pixels = (int64_t)images * size * size;
  const dim3 grid((unsigned)((pixels + 255) / 256)), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_parse_prep<DT>, grid, block, 0, (hipStream_t)stream, faces, (u16*)out, pixels, (int)size, (int)reverse, (int)ring));
  CA_CHECK_LAUNCH("ca_parse_prep");
  return CA_OK;
}

// the checks ca_conv3x3_reflect and ca_parse_mask share, in their order
static int reflect_checks(const char* who, const void* x, const void* wt, const float* bias, const void* y, int32_t images, int32_t h, int32_t w, int32_t cin,
                          int32_t cout, int32_t stride, int32_t up2, int32_t rings, int32_t dtype) {
  CA_REQUIRE(x && wt && bias && y, "%s: x, wt, bias and y are required", who);
  CA_REQUIRE(stride == 1 || stride == 2, "%s: stride=%d (1 or 2)", who, stride);
  CA_REQUIRE(up2 == 0 || (up2 == 1 && stride == 1), "%s: up2=%d stride=%d (up2 is 0 or 1, and 1 only at stride 1)", who, up2, stride);
  CA_REQUIRE(sizes_ok(images, h, w, up2 ? 4 : 1) && (up2 || (h >= 2 && w >= 2)),
             "%s: images=%d h=%d w=%d (images >= 1, h and w >= 2 for the reflection -- >= 1 behind up2 --, the output's pixels < 2^31)", who, images, h, w);
  CA_REQUIRE(refl_c_ok(cin) && refl_c_ok(cout), "%s: cin=%d cout=%d (each 32, 64, 128 or 256)", who, cin, cout);
  CA_REQUIRE(rings >= 0 && rings <= 7, "%s: rings=%d (a sum of 1: x ringed, 2: y ringed, 4: residual ringed)", who, rings);
  CA_REQUIRE(dtype_ok(dtype), "%s: dtype %d", who, dtype);
  return CA_OK;
}

extern "C" int ca_conv3x3_reflect(const void* x, const void* wt, const float* bias, const void* residual, void* y, int32_t images, int32_t h, int32_t w, int32_t cin,
                                  int32_t cout, int32_t stride, int32_t up2, int32_t leaky, int32_t out_f32, int32_t rings, int32_t dtype, void* stream) {
  const int rc = reflect_checks("ca_conv3x3_reflect", x, wt, bias, y, images, h, w, cin, cout, stride, up2, rings, dtype);
  if (rc != CA_OK) return rc;
  CA_REQUIRE((leaky == 0 || leaky == 1) && (out_f32 == 0 || out_f32 == 1), "ca_conv3x3_reflect: leaky=%d out_f32=%d (0 or 1)", leaky, out_f32);
  CA_REQUIRE(residual || !(rings & RING_RES), "ca_conv3x3_reflect: rings=%d names a residual that is not given", rings);
  const int lh = up2 ? 2 * h : h, lw = up2 ? 2 * w : w;
  const int gh = (lh - 1) / stride + 1, gw = (lw - 1) / stride + 1;
  CA_REQUIRE(plane_bytes(images, h, w, cin, rings & RING_IN, 2) <= kMaxBytes && plane_bytes(images, gh, gw, cout, rings & RING_OUT, out_f32 ? 4 : 2) <= kMaxBytes &&
                 plane_bytes(images, gh, gw, cout, rings & RING_RES, 2) <= kMaxBytes,
             "ca_conv3x3_reflect: images=%d h=%d w=%d cin=%d cout=%d: an operand would pass 2^31 bytes", images, h, w, cin, cout);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)wt | (uintptr_t)y | (uintptr_t)residual) & 15) == 0 && ((uintptr_t)bias & 3) == 0,
             "ca_conv3x3_reflect: x, wt, residual and y must be 16-byte aligned, bias 4-byte aligned");
  CA_REQUIRE(x != y && residual != y, "ca_conv3x3_reflect: y must not be x or the residual");
  const int64_t blocks = (int64_t)images * ceil_div_i(gw, CR_TW) * ceil_div_i(gh, refl_th(cout, stride)) * (cout / (cout >= 128 ? 128 : cout));
  CA_REQUIRE(blocks < ((int64_t)1 << 31), "ca_conv3x3_reflect: grid too large");
  ReflArgs a = {(const u16*)x, (const u16*)wt, bias, (const u16*)residual, y, h, w, cin, cout, gh, gw, 0, 0, leaky, out_f32, rings, 0};
  const hipStream_t st = (hipStream_t)stream;
  CA_DISPATCH_DT(dtype, if (stride == 2) launch_reflect<DT, 2, 0, 2, 4>(a, images, st); else if (up2) launch_reflect<DT, 1, 1, 4, 4>(a, images, st);
                 else launch_reflect<DT, 1, 0, 4, 4>(a, images, st));
  CA_CHECK_LAUNCH("ca_conv3x3_reflect");
  return CA_OK;
}

extern "C" int ca_parse_mask(const void* x, const void* wt, const float* bias, uint8_t* mask, int32_t images, int32_t h, int32_t w, int32_t cin, int32_t classes,
                             int32_t ring, int32_t dtype, void* stream) {
  const int rc = reflect_checks("ca_parse_mask", x, wt, bias, mask, images, h, w, cin, 32, 1, 0, ring, dtype);
  if (rc != CA_OK) return rc;
  CA_REQUIRE(classes == PN_CLASSES, "ca_parse_mask: classes=%d (the colour map has %d; wt and bias are padded to 32 rows)", classes, PN_CLASSES);
  CA_REQUIRE(ring == 0 || ring == 1, "ca_parse_mask: ring=%d (0 or 1)", ring);
  CA_REQUIRE(plane_bytes(images, h, w, cin, ring, 2) <= kMaxBytes, "ca_parse_mask: images=%d h=%d w=%d cin=%d: x would pass 2^31 bytes", images, h, w, cin);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)wt) & 15) == 0 && ((uintptr_t)bias & 3) == 0, "ca_parse_mask: x and wt must be 16-byte aligned, bias 4-byte aligned");
  ReflArgs a = {(const u16*)x, (const u16*)wt, bias, nullptr, mask, h, w, cin, 32, h, w, ceil_div_i(w, CR_TW), ceil_div_i(h, 16), 0, 0, ring ? RING_IN : 0, classes};
  const int64_t blocks = (int64_t)images * a.tiles_x * a.tiles_y;
  CA_REQUIRE(blocks < ((int64_t)1 << 31), "ca_parse_mask: grid too large");
  const dim3 grid((unsigned)blocks), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL((k_conv_reflect<DT, 1, 0, 1, 2, 4, EPI_MASK>), grid, block, 0, (hipStream_t)stream, a));
  CA_CHECK_LAUNCH("ca_parse_mask");
  return CA_OK;
}

extern "C" int ca_parse_labels(const float* logits, uint8_t* labels, uint8_t* mask, int64_t pixels, int32_t cols, int32_t classes, void* stream) {
  CA_REQUIRE(logits && (labels || mask), "ca_parse_labels: logits and one of labels, mask are required");
  CA_REQUIRE(pixels >= 1 && pixels <= kMaxPixels, "ca_parse_labels: pixels=%lld (1 .. 2^31 - 1)", (long long)pixels);
  CA_REQUIRE(classes == PN_CLASSES && cols >= classes && cols <= 256, "ca_parse_labels: classes=%d cols=%d (%d classes in rows of classes .. 256 floats)", classes, cols,
             PN_CLASSES);
  CA_REQUIRE(((uintptr_t)logits & 3) == 0, "ca_parse_labels: logits must be 4-byte aligned");
  const dim3 grid((unsigned)((pixels + 255) / 256)), block(256);
  hipLaunchKernelGGL(k_parse_labels, grid, block, 0, (hipStream_t)stream, logits, labels, mask, pixels, (int)cols, (int)classes);
  CA_CHECK_LAUNCH("ca_parse_labels");
  return CA_OK;
}

extern "C" int ca_ring_fill(void* x, int32_t images, int32_t h, int32_t w, int32_t c, int32_t mode, int32_t dtype, void* stream) {
  CA_REQUIRE(x, "ca_ring_fill: x is required");
  CA_REQUIRE(mode == CA_RING_REFLECT || mode == CA_RING_REPLICATE, "ca_ring_fill: mode=%d (CA_RING_REFLECT or CA_RING_REPLICATE)", mode);
  CA_REQUIRE(sizes_ok(images, h, w) && (mode == CA_RING_REPLICATE || (h >= 2 && w >= 2)), "ca_ring_fill: images=%d h=%d w=%d (each >= 1, h and w >= 2 to reflect)", images,
             h, w);
  CA_REQUIRE(c >= 8 && c % 8 == 0 && plane_bytes(images, h, w, c, 1, 2) <= kMaxBytes, "ca_ring_fill: c=%d (a multiple of 8; [images, h + 2, w + 2, c] below 2^31 bytes)", c);
  CA_REQUIRE(dtype_ok(dtype), "ca_ring_fill: dtype %d", dtype);
  CA_REQUIRE(((uintptr_t)x & 15) == 0, "ca_ring_fill: x must be 16-byte aligned");
  const int64_t total = (int64_t)images * (2 * (w + 2) + 2 * h) * (c / 8);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipLaunchKernelGGL(k_ring_fill, grid, block, 0, (hipStream_t)stream, (u16*)x, total, (int)h, (int)w, (int)c, mode == CA_RING_REFLECT ? 1 : 0);
  CA_CHECK_LAUNCH("ca_ring_fill");
  return CA_OK;
}

extern "C" int ca_mask_blur(const uint8_t* mask, const double* taps, double* workspace, double* out, int32_t images, int32_t size, int32_t ntaps, void* stream) {
  CA_REQUIRE(mask && taps && workspace && out, "ca_mask_blur: mask, taps, workspace and out are required");
  CA_REQUIRE(size == BL_S, "ca_mask_blur: size=%d (the masks are %d x %d)", size, BL_S, BL_S);
  CA_REQUIRE(ntaps == BL_R + 1, "ca_mask_blur: ntaps=%d (the centre tap and the %d behind it of the 101-tap kernel)", ntaps, BL_R);
  CA_REQUIRE(images >= 1 && images <= 65535, "ca_mask_blur: images=%d (1 .. 65535)", images);
  CA_REQUIRE((((uintptr_t)taps | (uintptr_t)workspace | (uintptr_t)out) & 7) == 0, "ca_mask_blur: taps, workspace and out must be 8-byte aligned");
  CA_REQUIRE(workspace != out, "ca_mask_blur: workspace must not be out");
  const dim3 grid(BL_S / BL_LINES, BL_S / BL_SEG, (unsigned)images), block(256);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((k_blur_pass<uint8_t, false, false>), grid, block, 0, st, mask, taps, workspace);
  hipLaunchKernelGGL((k_blur_pass<double, true, false>), grid, block, 0, st, (const double*)workspace, taps, out);
  hipLaunchKernelGGL((k_blur_pass<double, false, false>), grid, block, 0, st, (const double*)out, taps, workspace);
  hipLaunchKernelGGL((k_blur_pass<double, true, true>), grid, block, 0, st, (const double*)workspace, taps, out);
  CA_CHECK_LAUNCH("ca_mask_blur");
  return CA_OK;
}

extern "C" int ca_face_paste(const uint8_t* background, const uint8_t* restored, const double* masks, const double* inverse_affine, const int32_t* count, uint8_t* out,
                             int32_t images, int32_t h, int32_t w, int32_t max_faces, double upscale, void* stream) {
  CA_REQUIRE(background && restored && masks && inverse_affine && count && out, "ca_face_paste: background, restored, masks, inverse_affine, count and out are required");
  CA_REQUIRE(sizes_ok(images, h, w, 3) && h < 32768 && w < 32768 && images <= 65535,
             "ca_face_paste: images=%d h=%d w=%d (each >= 1, h and w < 32768, images <= 65535, images * h * w * 3 < 2^31)", images, h, w);
  CA_REQUIRE(max_faces >= 1 && max_faces <= CA_RFACE_MAX_FACES && (int64_t)images * max_faces * FP_S * FP_S <= kMaxPixels, "ca_face_paste: max_faces=%d (1 .. %d, images * max_faces * 512 * 512 < 2^31)",
             max_faces, CA_RFACE_MAX_FACES);
  CA_REQUIRE(upscale > 0.0, "ca_face_paste: upscale=%g (> 0)", upscale);
  CA_REQUIRE((((uintptr_t)masks | (uintptr_t)inverse_affine) & 7) == 0 && ((uintptr_t)count & 3) == 0, "ca_face_paste: masks and inverse_affine must be 8-byte aligned, count 4-byte aligned");
  const int64_t total = (int64_t)images * h * w;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipLaunchKernelGGL(k_face_paste, grid, block, 0, (hipStream_t)stream, background, restored, masks, inverse_affine, count, out, total, (int)h, (int)w, (int)max_faces,
                     upscale > 1.0 ? 0.5 * upscale : 0.0);
  CA_CHECK_LAUNCH("ca_face_paste");
  return CA_OK;
}
