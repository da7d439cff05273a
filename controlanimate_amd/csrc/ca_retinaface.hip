// Face detection and alignment in front of the GFPGAN face restorer (controlanimate_amd/face_align.py; the specification is
// tests/retinaface_ref.py).  RetinaFace-ResNet50's 1x1 convolutions run on ca_gemm (a bottleneck's identity as the residual: the epilogue
// adds it before the ReLU), its 3x3 convolutions on ca_conv3x3 (CA_ACT_RELU), the SSH concatenation through ca_copy_cols; this file holds
// the rest:
//
//   stem       k_rface_stem       uint8 frames -> relu(conv 7x7 s2 p3 of (byte - mean) + bias), the zero padding in the mean-subtracted image;
//                                 MFMA 16x16x32 with K = 147 padded to 160, the B operand gathered from an LDS tile of the byte frame (no
//                                 im2col tensor in memory)
//   pool       k_maxpool3x3s2     3x3 / stride 2 / padding 1, only the taps inside the image
//   subsample  k_subsample2       x[:, ::2, ::2, :], in front of the stride-2 1x1 shortcut on ca_gemm
//   add_up2    k_add_up2          a + nearest x2 (b), the FPN's top-down sum
//   decode     k_rface_decode     one block per frame: scores, the CA_RFACE_MAX_CAND best candidates (a binary search on the 64-bit key
//                                 (score bits, ~prior index) when there are more, then a bitonic sort in LDS), the float64 decode, the greedy
//                                 NMS (sequential over kept boxes, parallel over the rest), the eye-distance filter, the choice of one face
//   align      k_face_align       the closed-form least-squares similarity of the five landmarks onto the template, and its scaled inverse
//   warp       k_face_warp        cv2.warpAffine in OpenCV's fixed point, four pixels per thread
//
// Compiled with -ffp-contract=off: the float64 arithmetic of the decode, the fit and the warp's coordinates rounds operation by operation, as
// numpy's.  The only atomics are integer counters in LDS whose final values do not depend on the order; what they order (the slots of the
// candidate list) is sorted by a unique key afterwards.  No launch reads device data on the host: the chain can be captured in a hipGraph.
#include "ca_common.h"
#include "ca_annot.h"

namespace {

// ---- stem ----------------------------------------------------------------------------------------------------------------------------
// The stride-2, zero-padded sibling of k_lineart_conv_in (ca_lineart.hip).  A block owns a 16 x 64 tile of output pixels and keeps the
// 37 x 133 pixels of the byte frame under it in LDS, in the network's channel order; a pixel outside the image holds the mean
// (104, 117, 123 are bytes), so that byte - mean, the B operand, is exactly 0 there: the zero padding lies in the mean-subtracted image.
// k = ky * 21 + kx * 3 + c: for one ky the 21 values of an output pixel are 21 consecutive bytes of tile row 2 * row + ky from column
// 2 * px.  The weights [tiles * 16][160] are the A operand (up to 4 row tiles x 5 k-steps, in registers for the whole block), 16 pixels
// of one tile row the B operand: a lane ends up with 4 consecutive output channels of one pixel per row tile -- one 8-byte store each.
// byte - mean is an integer in -123 .. 151: exact in fp16 and bf16.
constexpr int ST_TH = 16, ST_TW = 64, ST_K = 147, ST_KP = 160, ST_MAX_C = 64;
constexpr int ST_ROWS = 2 * ST_TH + 5, ST_COLS = 2 * ST_TW + 5;
constexpr int ST_PITCH = ST_COLS * 3 + 3;  // bytes per tile row

template <int DT>
__global__ __launch_bounds__(256) void k_rface_stem(const uint8_t* __restrict__ src, const u16* __restrict__ wp, const float* __restrict__ bias,
                                                    u16* __restrict__ y, int H, int W, int cout, int bgr, int tiles_x, int tiles_y) {
  __shared__ uint8_t tile[ST_ROWS * ST_PITCH];
  const int bx = blockIdx.x % tiles_x;
  const int by = (blockIdx.x / tiles_x) % tiles_y;
  const int img = blockIdx.x / (tiles_x * tiles_y);
  const int ho = H >> 1, wo = W >> 1;
  const int y0 = by * ST_TH, x0 = bx * ST_TW;
  const uint8_t* s = src + (int64_t)img * H * W * 3;
  for (int i = threadIdx.x; i < ST_ROWS * ST_COLS; i += 256) {
    const int r = i / ST_COLS, c = i - r * ST_COLS;
    const int iy = 2 * y0 - 3 + r, ix = 2 * x0 - 3 + c;
    uint8_t* t = tile + r * ST_PITCH + c * 3;
    if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
      const uint8_t* p = s + ((int64_t)iy * W + ix) * 3;
      t[0] = p[bgr ? 2 : 0], t[1] = p[1], t[2] = p[bgr ? 0 : 2];
    } else {
      t[0] = 104, t[1] = 117, t[2] = 123;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, r16 = lane & 15;
  const int tiles = (cout + 15) >> 4;
  const float mean[3] = {104.0f, 117.0f, 123.0f};
  u32x4 wf[4][5];
  int off[5][8];
  float mk[5][8];
#pragma unroll
  for (int ks = 0; ks < 5; ++ks) {
#pragma unroll
    for (int t = 0; t < 4; ++t) wf[t][ks] = t < tiles ? ld16(wp + (t * 16 + r16) * ST_KP + ks * 32 + q * 8) : (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = ks * 32 + q * 8 + e;
      off[ks][e] = k < ST_K ? (k / 21) * ST_PITCH + (k % 21) : 0;  // (the padded columns of the weight are zero: any byte of the tile will do)
      mk[ks][e] = mean[k < ST_K ? k % 3 : 0];
    }
  }
  __syncthreads();
  for (int it = 0; it < 16; ++it) {
    const int row = wave * 4 + (it >> 2), px = (it & 3) * 16 + r16;
    if (y0 + row >= ho || x0 + (it & 3) * 16 >= wo) continue;  // wave-uniform
    const uint8_t* base = tile + 2 * row * ST_PITCH + 2 * px * 3;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 5; ++ks) {
      u32x4 b;
#pragma unroll
      for (int e = 0; e < 4; ++e) b[e] = pack2<DT>((float)base[off[ks][2 * e]] - mk[ks][2 * e], (float)base[off[ks][2 * e + 1]] - mk[ks][2 * e + 1]);
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (t < tiles) acc[t] = Elem<DT>::mfma(wf[t][ks], b, acc[t]);
    }
    const int gy = y0 + row, gx = x0 + px;
    if (gx < wo) {
      u16* d = y + (((int64_t)img * ho + gy) * wo + gx) * cout + q * 4;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (t * 16 + q * 4 >= cout) continue;
        const float* bb = bias + t * 16 + q * 4;
        u32x2 v;
        v[0] = pack2<DT>(fmaxf(acc[t][0] + bb[0], 0.0f), fmaxf(acc[t][1] + bb[1], 0.0f));
        v[1] = pack2<DT>(fmaxf(acc[t][2] + bb[2], 0.0f), fmaxf(acc[t][3] + bb[3], 0.0f));
        *(u32x2*)(d + t * 16) = v;
      }
    }
  }
}

// ---- pool, subsample, add ----------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void k_maxpool3x3s2(const u16* __restrict__ x, u16* __restrict__ y, int64_t total, int h, int w, int ho, int wo, int c) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cl = c >> 3;
  const int cg = (int)(idx % cl);
  const int64_t op = idx / cl;
  const int ox = (int)(op % wo);
  const int oy = (int)((op / wo) % ho);
  const int64_t img = op / ((int64_t)ho * wo);
  float m[8], f[8];
  unpack8<DT>(ld16(x + ((img * h + 2 * oy) * (int64_t)w + 2 * ox) * c + cg * 8), m);  // the centre tap is always inside
#pragma unroll
  for (int ky = -1; ky <= 1; ++ky) {
    const int iy = 2 * oy + ky;
    if (iy < 0 || iy >= h) continue;
#pragma unroll
    for (int kx = -1; kx <= 1; ++kx) {
      const int ix = 2 * ox + kx;
      if (ix < 0 || ix >= w) continue;
      unpack8<DT>(ld16(x + ((img * h + iy) * (int64_t)w + ix) * c + cg * 8), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], f[e]);
    }
  }
  st16(y + op * c + cg * 8, pack8<DT>(m));  // (the maximum is one of the inputs: the conversion back is exact)
}

__global__ __launch_bounds__(256) void k_subsample2(const u16* __restrict__ x, u16* __restrict__ y, int64_t total, int h, int w, int ho, int wo, int c) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cl = c >> 3;
  const int cg = (int)(idx % cl);
  const int64_t op = idx / cl;
  const int ox = (int)(op % wo);
  const int oy = (int)((op / wo) % ho);
  const int64_t img = op / ((int64_t)ho * wo);
  st16(y + op * c + cg * 8, ld16(x + ((img * h + 2 * oy) * (int64_t)w + 2 * ox) * c + cg * 8));
}

template <int DT>
__global__ __launch_bounds__(256) void k_add_up2(const u16* __restrict__ a, const u16* __restrict__ b, u16* __restrict__ y, int64_t total, int h, int w, int c) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cl = c >> 3;
  const int cg = (int)(idx % cl);
  const int64_t op = idx / cl;
  const int ox = (int)(op % w);
  const int oy = (int)((op / w) % h);
  const int64_t img = op / ((int64_t)h * w);
  float fa[8], fb[8];
  unpack8<DT>(ld16(a + op * c + cg * 8), fa);
  unpack8<DT>(ld16(b + ((img * (h >> 1) + (oy >> 1)) * (int64_t)(w >> 1) + (ox >> 1)) * c + cg * 8), fb);
#pragma unroll
  for (int e = 0; e < 8; ++e) fa[e] = fa[e] + fb[e];
  st16(y + op * c + cg * 8, pack8<DT>(fa));
}

// ---- decode ------------------------------------------------------------------------------------------------------------------------
constexpr int RF_T = CA_RFACE_MAX_CAND;  // threads of a block = candidates
constexpr int RF_COLS = CA_RFACE_HEAD_COLS;

struct RfGeom {
  const float* head[3];
  int fh[3], fw[3];
  int H, W, P;
};

struct RfPrior {
  const float* row;  // the head row of the prior's cell (this frame)
  int a;             // which of the cell's two priors
  double cx, cy, sw, sh;
};

inline int rf_cells(int size, int step) { return (size + step - 1) / step; }

__device__ __forceinline__ RfPrior rf_prior(const RfGeom& g, int img, int idx) {
  int lvl = 0, r = idx;
  const int n0 = 2 * g.fh[0] * g.fw[0], n1 = 2 * g.fh[1] * g.fw[1];
  if (r >= n0) {
    r -= n0, lvl = 1;
    if (r >= n1) r -= n1, lvl = 2;
  }
  const int cell = r >> 1, fw = g.fw[lvl];
  const int i = cell / fw, j = cell % fw;
  RfPrior p;
  p.a = r & 1;
  p.row = g.head[lvl] + ((int64_t)img * g.fh[lvl] * fw + cell) * RF_COLS;
  const double step = (double)(8 << lvl), size = (double)(16 << (2 * lvl + p.a));
  p.cx = ((double)j + 0.5) * step / (double)g.W;
  p.cy = ((double)i + 0.5) * step / (double)g.H;
  p.sw = size / (double)g.W;
  p.sh = size / (double)g.H;
  return p;
}

__device__ __forceinline__ void rf_box(const RfGeom& g, const RfPrior& p, float out[4]) {
  const float* b = p.row + 4 + 4 * p.a;
  const double cx = p.cx + ((double)b[0] * 0.1) * p.sw, cy = p.cy + ((double)b[1] * 0.1) * p.sh;
  const double bw = p.sw * exp((double)b[2] * 0.2), bh = p.sh * exp((double)b[3] * 0.2);
  const double x1 = cx - bw / 2, y1 = cy - bh / 2;
  const double x2 = bw + x1, y2 = bh + y1;
  out[0] = (float)(x1 * (double)g.W), out[1] = (float)(y1 * (double)g.H), out[2] = (float)(x2 * (double)g.W), out[3] = (float)(y2 * (double)g.H);
}

// landmark coordinate t (0 .. 9: x0, y0, x1, ...)
__device__ __forceinline__ float rf_landmark(const RfGeom& g, const RfPrior& p, int t) {
  const double l = (double)p.row[12 + 10 * p.a + t];
  return (t & 1) ? (float)((p.cy + (l * 0.1) * p.sh) * (double)g.H) : (float)((p.cx + (l * 0.1) * p.sw) * (double)g.W);
}

__device__ __forceinline__ double rf_overlap(const float* a, const float* b) {  // a: the kept box
  const double ax1 = a[0], ay1 = a[1], ax2 = a[2], ay2 = a[3], bx1 = b[0], by1 = b[1], bx2 = b[2], by2 = b[3];
  const double ww = fmax(0.0, fmin(ax2, bx2) - fmax(ax1, bx1) + 1.0), hh = fmax(0.0, fmin(ay2, by2) - fmax(ay1, by1) + 1.0);
  const double inter = ww * hh;
  return inter / ((ax2 - ax1 + 1.0) * (ay2 - ay1 + 1.0) + (bx2 - bx1 + 1.0) * (by2 - by1 + 1.0) - inter);
}

__global__ __launch_bounds__(RF_T) void k_rface_decode(RfGeom g, float conf, double nms, double eye_dist, int flags, int max_faces,
                                                       unsigned long long* __restrict__ ws, float* __restrict__ dets, int* __restrict__ count,
                                                       int* __restrict__ overflow) {
  __shared__ unsigned long long s_key[RF_T];
  __shared__ float s_box[RF_T][4];
  __shared__ int s_list[RF_T];
  __shared__ unsigned char s_sup[RF_T], s_face[RF_T];
  __shared__ int s_cnt, s_n;
  const int img = blockIdx.x, tid = threadIdx.x;
  unsigned long long* keys = ws + (int64_t)img * g.P;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  // the candidates' keys: (score bits, ~prior index); a larger key comes first
  for (int idx = tid; idx < g.P; idx += RF_T) {
    const RfPrior p = rf_prior(g, img, idx);
    const float s = (float)(1.0 / (1.0 + exp((double)p.row[2 * p.a] - (double)p.row[2 * p.a + 1])));
    if (s > conf) keys[atomicAdd(&s_cnt, 1)] = ((unsigned long long)__float_as_uint(s) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)idx);
  }
  __syncthreads();
  const int cand = s_cnt;
  int ov = 0, m = cand;
  if (cand > RF_T) {
    ov |= CA_RFACE_OVERFLOW_CAND;
    m = RF_T;
    // the RF_T-th largest key: the largest T with count(key >= T) >= RF_T (keys are unique, so exactly RF_T keys are >= it)
    unsigned long long lo = 0, hi = ~0ull;
    while (lo < hi) {
      const unsigned long long d = hi - lo, mid = lo + (d >> 1) + (d & 1);
      if (tid == 0) s_n = 0;
      __syncthreads();
      int local = 0;
      for (int k = tid; k < cand; k += RF_T) local += keys[k] >= mid;
      if (local) atomicAdd(&s_n, local);
      __syncthreads();
      if (s_n >= RF_T) lo = mid;
      else hi = mid - 1;
      __syncthreads();
    }
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int k = tid; k < cand; k += RF_T) {
      const unsigned long long key = keys[k];
      if (key >= lo) {
        const int slot = atomicAdd(&s_n, 1);
        if (slot < RF_T) s_key[slot] = key;
      }
    }
  } else {
    s_key[tid] = tid < cand ? keys[tid] : 0ull;
  }
  __syncthreads();
  // bitonic sort, descending
  for (int k = 2; k <= RF_T; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int other = tid ^ j;
      if (other > tid) {
        const unsigned long long a = s_key[tid], b = s_key[other];
        if ((tid & k) == 0 ? a < b : a > b) s_key[tid] = b, s_key[other] = a;
      }
      __syncthreads();
    }
  const int my_idx = (int)(0xFFFFFFFFu - (unsigned)(s_key[tid] & 0xFFFFFFFFull));
  if (tid < m) {
    rf_box(g, rf_prior(g, img, my_idx), s_box[tid]);
    s_sup[tid] = 0;
  } else {
    s_sup[tid] = 1;
  }
  __syncthreads();
  // greedy NMS: candidate i is kept when nothing kept before it has suppressed it
  for (int i = 0; i < m; ++i) {
    if (s_sup[i]) continue;  // (uniform: written before the last barrier)
    if (tid > i && tid < m && !s_sup[tid] && rf_overlap(s_box[i], s_box[tid]) > nms) s_sup[tid] = 1;
    __syncthreads();
  }
  bool face = false;
  if (tid < m && !s_sup[tid]) {
    const RfPrior p = rf_prior(g, img, my_idx);
    const double dx = (double)rf_landmark(g, p, 0) - (double)rf_landmark(g, p, 2), dy = (double)rf_landmark(g, p, 1) - (double)rf_landmark(g, p, 3);
    face = !(sqrt(dx * dx + dy * dy) < eye_dist);
  }
  s_face[tid] = face;
  __syncthreads();
  if (tid == 0) {
    int f = 0;
    for (int i = 0; i < m; ++i)
      if (s_face[i]) s_list[f++] = i;
    if (f > 0 && (flags & (CA_RFACE_LARGEST | CA_RFACE_CENTER))) {
      const bool largest = flags & CA_RFACE_LARGEST;
      int best = s_list[0];
      double best_v = 0.0;
      for (int r = 0; r < f; ++r) {
        const float* b = s_box[s_list[r]];
        const double x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
        double v;
        if (largest) {
          v = (x2 - x1) * (y2 - y1);
        } else {
          const double cx = (x1 + x2) / 2 - (double)g.W / 2, cy = (y1 + y2) / 2 - (double)g.H / 2;
          v = sqrt(cx * cx + cy * cy);
        }
        if (r == 0 || (largest ? v > best_v : v < best_v)) best = s_list[r], best_v = v;
      }
      s_list[0] = best;
      f = 1;
    }
    if (f > max_faces) {
      ov |= CA_RFACE_OVERFLOW_FACES;
      f = max_faces;
    }
    s_n = f;
    count[img] = f;
    overflow[img] = ov;
  }
  __syncthreads();
  if (tid < max_faces * CA_RFACE_DET_COLS) {
    const int r = tid / CA_RFACE_DET_COLS, c = tid % CA_RFACE_DET_COLS;
    float v = 0.0f;
    if (r < s_n) {
      const int k = s_list[r];
      if (c < 4) {
        v = s_box[k][c];
      } else if (c == 4) {
        v = __uint_as_float((unsigned)(s_key[k] >> 32));
      } else {
        const int idx = (int)(0xFFFFFFFFu - (unsigned)(s_key[k] & 0xFFFFFFFFull));
        v = rf_landmark(g, rf_prior(g, img, idx), c - 5);
      }
    }
    dets[((int64_t)img * max_faces + r) * CA_RFACE_DET_COLS + c] = v;
  }
}

// ---- fit -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void invert_affine(const double m[6], double out[6]) {  // cv2.invertAffineTransform, operation by operation
  double d = m[0] * m[4] - m[1] * m[3];
  d = d != 0.0 ? 1.0 / d : 0.0;
  const double a11 = m[4] * d, a22 = m[0] * d, a12 = m[1] * -d, a21 = m[3] * -d;
  out[0] = a11, out[1] = a12, out[2] = -a11 * m[2] - a12 * m[5];
  out[3] = a21, out[4] = a22, out[5] = -a21 * m[2] - a22 * m[5];
}

__global__ __launch_bounds__(64) void k_face_align(const float* __restrict__ dets, const int* __restrict__ count, int slots, int max_faces, double upscale,
                                                   double* __restrict__ affine, double* __restrict__ inverse) {
  const int slot = blockIdx.x * 64 + threadIdx.x;
  if (slot >= slots) return;
  const double tpl[5][2] = {{192.98138, 239.94708}, {318.90277, 240.1936}, {256.63416, 314.01935}, {201.26117, 371.41043}, {313.08905, 371.15118}};
  double m[6] = {0, 0, 0, 0, 0, 0}, inv[6] = {0, 0, 0, 0, 0, 0};
  if (slot % max_faces < count[slot / max_faces]) {
    const float* l = dets + (int64_t)slot * CA_RFACE_DET_COLS + 5;
    double mx = 0.0, my = 0.0, mu = 0.0, mv = 0.0;
    for (int i = 0; i < 5; ++i) mx = mx + (double)l[2 * i], my = my + (double)l[2 * i + 1], mu = mu + tpl[i][0], mv = mv + tpl[i][1];
    mx = mx / 5.0, my = my / 5.0, mu = mu / 5.0, mv = mv / 5.0;
    double sa = 0.0, sb = 0.0, ss = 0.0;
    for (int i = 0; i < 5; ++i) {
      const double x = (double)l[2 * i] - mx, y = (double)l[2 * i + 1] - my, u = tpl[i][0] - mu, v = tpl[i][1] - mv;
      sa = sa + (x * u + y * v);
      sb = sb + (x * v - y * u);
      ss = ss + (x * x + y * y);
    }
    const double a = sa / ss, b = sb / ss;
    m[0] = a, m[1] = -b, m[2] = mu - (a * mx - b * my);
    m[3] = b, m[4] = a, m[5] = mv - (b * mx + a * my);
    invert_affine(m, inv);
    for (int i = 0; i < 6; ++i) inv[i] = inv[i] * upscale;
  }
  for (int i = 0; i < 6; ++i) affine[(int64_t)slot * 6 + i] = m[i], inverse[(int64_t)slot * 6 + i] = inv[i];
}

// ---- warp ----------------------------------------------------------------------------------------------------------------------------
constexpr int FW_SIZE = CA_FACE_ALIGN_SIZE;

__device__ __forceinline__ int sat_int(double v) {  // saturate_cast<int>(double): round half to even, clamped
  return (int)fmin(fmax(rint(v), -2147483648.0), 2147483647.0);
}

__global__ __launch_bounds__(256) void k_face_warp(const uint8_t* __restrict__ frames, const double* __restrict__ affine, const int* __restrict__ count,
                                                   uint8_t* __restrict__ faces, int64_t total, int h, int w, int max_faces, int bgr) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  constexpr int QUADS = FW_SIZE / 4;
  const int x0 = 4 * (int)(idx % QUADS);
  const int y = (int)((idx / QUADS) % FW_SIZE);
  const int slot = (int)(idx / ((int64_t)QUADS * FW_SIZE));
  const int img = slot / max_faces;
  const int border[3] = {bgr ? 132 : 135, 133, bgr ? 135 : 132};
  uint8_t px[12];
  if (slot % max_faces >= count[img]) {
#pragma unroll
    for (int i = 0; i < 12; ++i) px[i] = (uint8_t)border[i % 3];
  } else {
    double m[6], inv[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) m[i] = affine[(int64_t)slot * 6 + i];
    invert_affine(m, inv);
    // (the sums wrap as 32-bit integers)
    const unsigned X0 = (unsigned)sat_int((inv[1] * (double)y + inv[2]) * 1024.0) + 16u, Y0 = (unsigned)sat_int((inv[4] * (double)y + inv[5]) * 1024.0) + 16u;
    const uint8_t* frame = frames + (int64_t)img * h * w * 3;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double xd = (double)(x0 + q);
      const int X = (int)(X0 + (unsigned)sat_int(inv[0] * xd * 1024.0)) >> 5, Y = (int)(Y0 + (unsigned)sat_int(inv[3] * xd * 1024.0)) >> 5;
      const int sx = min(max(X >> 5, -32768), 32767), sy = min(max(Y >> 5, -32768), 32767), fx = X & 31, fy = Y & 31;
      const int wt[4] = {(32 - fy) * (32 - fx) * 32, (32 - fy) * fx * 32, fy * (32 - fx) * 32, fy * fx * 32};
      int acc[3] = {0, 0, 0};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int yy = sy + (t >> 1), xx = sx + (t & 1);
        const bool inside = yy >= 0 && yy < h && xx >= 0 && xx < w;
        const uint8_t* p = frame + ((int64_t)(inside ? yy : 0) * w + (inside ? xx : 0)) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += (inside ? (int)p[c] : border[c]) * wt[t];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) px[q * 3 + c] = (uint8_t)((acc[c] + (1 << 14)) >> 15);
    }
  }
  uint32_t* out = (uint32_t*)(faces + (((int64_t)slot * FW_SIZE + y) * FW_SIZE + x0) * 3);
#pragma unroll
  for (int i = 0; i < 3; ++i)
    out[i] = (uint32_t)px[4 * i] | ((uint32_t)px[4 * i + 1] << 8) | ((uint32_t)px[4 * i + 2] << 16) | ((uint32_t)px[4 * i + 3] << 24);
}

inline bool plane_ok(int32_t images, int32_t h, int32_t w, int32_t c) {
  return sizes_ok(images, h, w) && c >= 8 && c % 8 == 0 && (int64_t)images * h * w * c * 2 <= kMaxBytes;
}

}  // namespace

extern "C" int ca_rface_stem(const uint8_t* src, const void* w_packed, const float* bias, void* y, int32_t images, int32_t h, int32_t w, int32_t cout, int32_t bgr,
                             int32_t dtype, void* stream) {
  CA_REQUIRE(src && w_packed && bias && y, "ca_rface_stem: src, w_packed, bias and y are required");
  CA_REQUIRE(sizes_ok(images, h, w) && h % 2 == 0 && w % 2 == 0, "ca_rface_stem: images=%d h=%d w=%d (images >= 1, h and w even, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE(cout >= 8 && cout <= ST_MAX_C && cout % 8 == 0, "ca_rface_stem: cout=%d must be a multiple of 8 in 8 .. 64", cout);
  CA_REQUIRE(bgr == 0 || bgr == 1, "ca_rface_stem: bgr=%d (0 or 1)", bgr);
  CA_REQUIRE(dtype_ok(dtype), "ca_rface_stem: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)w_packed | (uintptr_t)y) & 15) == 0 && ((uintptr_t)bias & 3) == 0, "ca_rface_stem: w_packed and y must be 16-byte aligned, bias 4-byte aligned");
  CA_REQUIRE((int64_t)images * (h / 2) * (w / 2) * cout * 2 <= kMaxBytes, "ca_rface_stem: images=%d h=%d w=%d: y would pass 2^31 bytes", images, h, w);
  const int tx = (w / 2 + ST_TW - 1) / ST_TW, ty = (h / 2 + ST_TH - 1) / ST_TH;
  const int64_t blocks = (int64_t)images * tx * ty;
  CA_REQUIRE(blocks < ((int64_t)1 << 31), "ca_rface_stem: grid too large");
  const dim3 grid((unsigned)blocks), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_rface_stem<DT>, grid, block, 0, (hipStream_t)stream, src, (const u16*)w_packed, bias, (u16*)y, (int)h, (int)w, (int)cout, (int)bgr,
                                           tx, ty));
  CA_CHECK_LAUNCH("ca_rface_stem");
  return CA_OK;
}

extern "C" int ca_maxpool3x3s2(const void* x, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t dtype, void* stream) {
  CA_REQUIRE(x && y, "ca_maxpool3x3s2: x and y are required");
  CA_REQUIRE(plane_ok(images, h, w, c), "ca_maxpool3x3s2: images=%d h=%d w=%d c=%d (each >= 1, c a multiple of 8, the tensor below 2^31 bytes)", images, h, w, c);
  CA_REQUIRE(dtype_ok(dtype), "ca_maxpool3x3s2: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "ca_maxpool3x3s2: x and y must be 16-byte aligned");
  const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
  const int64_t total = (int64_t)images * ho * wo * (c / 8);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_maxpool3x3s2<DT>, grid, block, 0, (hipStream_t)stream, (const u16*)x, (u16*)y, total, (int)h, (int)w, ho, wo, (int)c));
  CA_CHECK_LAUNCH("ca_maxpool3x3s2");
  return CA_OK;
}

extern "C" int ca_subsample2(const void* x, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t dtype, void* stream) {
  CA_REQUIRE(x && y, "ca_subsample2: x and y are required");
  CA_REQUIRE(plane_ok(images, h, w, c), "ca_subsample2: images=%d h=%d w=%d c=%d (each >= 1, c a multiple of 8, the tensor below 2^31 bytes)", images, h, w, c);
  CA_REQUIRE(dtype_ok(dtype), "ca_subsample2: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "ca_subsample2: x and y must be 16-byte aligned");
  const int ho = (h + 1) / 2, wo = (w + 1) / 2;
  const int64_t total = (int64_t)images * ho * wo * (c / 8);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipLaunchKernelGGL(k_subsample2, grid, block, 0, (hipStream_t)stream, (const u16*)x, (u16*)y, total, (int)h, (int)w, ho, wo, (int)c);
  CA_CHECK_LAUNCH("ca_subsample2");
  return CA_OK;
}

extern "C" int ca_add_up2(const void* a, const void* b, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t dtype, void* stream) {
  CA_REQUIRE(a && b && y, "ca_add_up2: a, b and y are required");
  CA_REQUIRE(plane_ok(images, h, w, c) && h % 2 == 0 && w % 2 == 0,
             "ca_add_up2: images=%d h=%d w=%d c=%d (each >= 1, h and w even, c a multiple of 8, the tensor below 2^31 bytes)", images, h, w, c);
  CA_REQUIRE(dtype_ok(dtype), "ca_add_up2: dtype %d", dtype);
  CA_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)y) & 15) == 0, "ca_add_up2: a, b and y must be 16-byte aligned");
  const int64_t total = (int64_t)images * h * w * (c / 8);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL(k_add_up2<DT>, grid, block, 0, (hipStream_t)stream, (const u16*)a, (const u16*)b, (u16*)y, total, (int)h, (int)w, (int)c));
  CA_CHECK_LAUNCH("ca_add_up2");
  return CA_OK;
}

static int64_t rface_priors(int32_t h, int32_t w) {
  int64_t p = 0;
  for (int k = 0; k < 3; ++k) p += 2 * (int64_t)rf_cells(h, 8 << k) * rf_cells(w, 8 << k);
  return p;
}

extern "C" int64_t ca_rface_decode_workspace_bytes(int32_t images, int32_t h, int32_t w) {
  if (!sizes_ok(images, h, w)) return 0;
  return (int64_t)images * rface_priors(h, w) * 8;
}

extern "C" int ca_rface_decode(const float* heads0, const float* heads1, const float* heads2, int32_t images, int32_t h, int32_t w, float conf, float nms,
                               float eye_dist, int32_t flags, int32_t max_faces, void* workspace, int64_t workspace_bytes, float* dets, int32_t* count,
                               int32_t* overflow, void* stream) {
  CA_REQUIRE(heads0 && heads1 && heads2 && workspace && dets && count && overflow, "ca_rface_decode: heads0 .. 2, workspace, dets, count and overflow are required");
  CA_REQUIRE(sizes_ok(images, h, w) && images <= 65535, "ca_rface_decode: images=%d h=%d w=%d (each >= 1, images <= 65535, images * h * w < 2^31)", images, h, w);
  CA_REQUIRE(conf >= 0.0f && conf < 1.0f, "ca_rface_decode: conf=%g (0 <= conf < 1)", (double)conf);
  CA_REQUIRE(nms >= 0.0f && nms <= 1.0f && eye_dist >= 0.0f, "ca_rface_decode: nms=%g (0 .. 1) eye_dist=%g (>= 0)", (double)nms, (double)eye_dist);
  CA_REQUIRE(flags >= 0 && flags <= (CA_RFACE_CENTER | CA_RFACE_LARGEST), "ca_rface_decode: flags=%d (CA_RFACE_CENTER | CA_RFACE_LARGEST)", flags);
  CA_REQUIRE(max_faces >= 1 && max_faces <= CA_RFACE_MAX_FACES, "ca_rface_decode: max_faces=%d (1 .. %d)", max_faces, CA_RFACE_MAX_FACES);
  CA_REQUIRE(workspace_bytes >= ca_rface_decode_workspace_bytes(images, h, w), "ca_rface_decode: workspace_bytes=%lld, %lld are needed", (long long)workspace_bytes,
             (long long)ca_rface_decode_workspace_bytes(images, h, w));
  CA_REQUIRE(((uintptr_t)workspace & 7) == 0 && (((uintptr_t)heads0 | (uintptr_t)heads1 | (uintptr_t)heads2 | (uintptr_t)dets | (uintptr_t)count | (uintptr_t)overflow) & 3) == 0,
             "ca_rface_decode: workspace must be 8-byte aligned, the other operands 4-byte aligned");
  RfGeom g;
  g.head[0] = heads0, g.head[1] = heads1, g.head[2] = heads2;
  for (int k = 0; k < 3; ++k) g.fh[k] = rf_cells(h, 8 << k), g.fw[k] = rf_cells(w, 8 << k);
  g.H = h, g.W = w, g.P = (int)rface_priors(h, w);
  hipLaunchKernelGGL(k_rface_decode, dim3((unsigned)images), dim3(RF_T), 0, (hipStream_t)stream, g, conf, (double)nms, (double)eye_dist, (int)flags, (int)max_faces,
                     (unsigned long long*)workspace, dets, count, overflow);
  CA_CHECK_LAUNCH("ca_rface_decode");
  return CA_OK;
}

extern "C" int ca_face_align(const float* dets, const int32_t* count, int32_t images, int32_t max_faces, double upscale, double* affine, double* inverse,
                             void* stream) {
  CA_REQUIRE(dets && count && affine && inverse, "ca_face_align: dets, count, affine and inverse are required");
  CA_REQUIRE(images >= 1 && images <= 65535 && max_faces >= 1 && max_faces <= CA_RFACE_MAX_FACES, "ca_face_align: images=%d (1 .. 65535) max_faces=%d (1 .. %d)", images,
             max_faces, CA_RFACE_MAX_FACES);
  CA_REQUIRE(upscale > 0.0, "ca_face_align: upscale=%g (> 0)", upscale);
  CA_REQUIRE((((uintptr_t)affine | (uintptr_t)inverse) & 7) == 0 && (((uintptr_t)dets | (uintptr_t)count) & 3) == 0,
             "ca_face_align: affine and inverse must be 8-byte aligned, dets and count 4-byte aligned");
  const int slots = images * max_faces;
  hipLaunchKernelGGL(k_face_align, dim3((unsigned)((slots + 63) / 64)), dim3(64), 0, (hipStream_t)stream, dets, count, slots, (int)max_faces, upscale, affine, inverse);
  CA_CHECK_LAUNCH("ca_face_align");
  return CA_OK;
}

extern "C" int ca_face_warp(const uint8_t* frames, const double* affine, const int32_t* count, uint8_t* faces, int32_t images, int32_t h, int32_t w, int32_t max_faces,
                            int32_t bgr, void* stream) {
  CA_REQUIRE(frames && affine && count && faces, "ca_face_warp: frames, affine, count and faces are required");
  CA_REQUIRE(sizes_ok(images, h, w, 3) && h < 32768 && w < 32768 && images <= 65535,
             "ca_face_warp: images=%d h=%d w=%d (each >= 1, h and w < 32768, images <= 65535, images * h * w * 3 < 2^31)", images, h, w);
  CA_REQUIRE(max_faces >= 1 && max_faces <= CA_RFACE_MAX_FACES, "ca_face_warp: max_faces=%d (1 .. %d)", max_faces, CA_RFACE_MAX_FACES);
  CA_REQUIRE(bgr == 0 || bgr == 1, "ca_face_warp: bgr=%d (0 or 1)", bgr);
  CA_REQUIRE(((uintptr_t)affine & 7) == 0 && (((uintptr_t)count | (uintptr_t)faces) & 3) == 0, "ca_face_warp: affine must be 8-byte aligned, count and faces 4-byte aligned");
  const int64_t total = (int64_t)images * max_faces * FW_SIZE * (FW_SIZE / 4);
  CA_REQUIRE(total <= kMaxPixels, "ca_face_warp: images=%d max_faces=%d: too many slots", images, max_faces);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipLaunchKernelGGL(k_face_warp, grid, block, 0, (hipStream_t)stream, frames, affine, count, faces, total, (int)h, (int)w, (int)max_faces, (int)bgr);
  CA_CHECK_LAUNCH("ca_face_warp");
  return CA_OK;
}
