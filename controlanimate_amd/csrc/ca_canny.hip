// ABI v16: the canny annotator of the ControlNet path (controlanimate_amd/annotators.py: canny_edges, the numpy restatement of
// cv2.Canny(img, low, high) with aperture 3 and the L1 norm) for a whole window of frames, as five launches:
//
//   classify  k_classify<C>  Sobel 3x3 (replicated borders), channel choice, non-maximum suppression, thresholds -> one class
//                            byte per pixel (0 none, 1 weak candidate, 2 strong)
//   link      k_label_tile   union-find over the candidates of one 64 x 16 tile in LDS; label = global linear index of the root
//             k_merge_tiles  unions of the 8-neighbour pairs that straddle a tile border, atomicMin on the int32 labels in HBM
//             k_flatten      label = root for every candidate; one byte per root: the component holds a strong pixel
//   emit      k_emit         edge = candidate whose root is marked -> uint8 0 / 255 and / or the control tensor 0.0 / 1.0 (ca_annot.h)
//
// Everything is int32, so the result equals the host function's byte for byte.  The hysteresis result is the unique fixed point
// "every candidate 8-connected to a strong pixel through candidates": the order in which the unions happen does not show.
// No launch depends on device data on the host side: the chain can be captured in a hipGraph.
#include "ca_common.h"
#include "ca_annot.h"

namespace {

constexpr int kTW = 64;                  // tile width: one wave per tile row
constexpr int kTH = 16;                  // tile height: 4 waves x 4 rows
constexpr int kRawRows = kTH + 4;        // 2-pixel halo: a neighbour's magnitude needs its own Sobel window
constexpr int kRawDwords = 52;           // (kTW + 4) * 3 bytes + up to 3 bytes of misalignment = 207 <= 208
constexpr int kMergeThreads = kTW + 2 * kTH;  // k_merge_tiles: a tile's top row, left column and right column
constexpr int kMagW = kTW + 2, kMagH = kTH + 2;

static_assert((kTW + 4) * 3 + 3 <= kRawDwords * 4, "a raw row of the RGB tile with its halo fits its LDS row");

struct WsLayout {
  int64_t label, cls, flag, total;  // byte offsets
};

inline WsLayout ws_layout(int64_t pixels) {  // pixels = images * h * w
  WsLayout l;
  l.label = 0;
  l.cls = pixels * 4;
  l.flag = l.cls + pixels;
  l.total = (l.flag + pixels + 255) / 256 * 256;
  return l;
}

struct Geom {
  int h, w, tiles_x, tiles_y;
};

// blockIdx.x -> (frame, tile origin)
__device__ __forceinline__ void tile_of_block(const Geom& g, int& frame, int& y0, int& x0) {
  const int per_frame = g.tiles_x * g.tiles_y;
  frame = blockIdx.x / per_frame;
  const int t = blockIdx.x - frame * per_frame;
  const int tyi = t / g.tiles_x;
  y0 = tyi * kTH;
  x0 = (t - tyi * g.tiles_x) * kTW;
}

// ---- gradient, non-maximum suppression, thresholds -----------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void k_classify(const uint8_t* __restrict__ src, uint8_t* __restrict__ cls, Geom g, int low, int high) {
  __shared__ uint32_t raw[kRawRows][kRawDwords];  // image rows y0 - 2 .. y0 + kTH + 1 (clamped), bytes of columns xs .. xe - 1
  __shared__ int raw_a[kRawRows];                 // where column xs starts in its raw row: the row's address modulo 4
  __shared__ short sdx[kMagH][kMagW], sdy[kMagH][kMagW], smag[kMagH][kMagW];  // rows y0 - 1 .., columns x0 - 1 ..
  const int tid = threadIdx.x;
  int frame, y0, x0;
  tile_of_block(g, frame, y0, x0);
  const int xs = x0 - 2 < 0 ? 0 : x0 - 2;
  const int xe = x0 + kTW + 2 > g.w ? g.w : x0 + kTW + 2;
  const int len = (xe - xs) * C;

  // Aligned 4-byte loads.  A row starts at any address modulo 4, so the first dword of a row can begin up to 3 bytes before the
  // row (before the tensor, for row 0 of frame 0) and the last can end up to 3 bytes after it (after the tensor, for the last
  // row).  Those bytes are read and never used.  The read cannot fault: a dword is loaded only when it holds at least one byte
  // of the row (i * 4 < a + len), and an aligned dword lies in one page, the page of that byte.  Whoever changes kRawDwords or
  // widens these loads keeps both conditions: alignment to the load's own size, and one image byte in every load.
  for (int idx = tid; idx < kRawRows * kRawDwords; idx += 256) {
    const int r = idx / kRawDwords, i = idx - r * kRawDwords;
    int yy = y0 - 2 + r;
    yy = yy < 0 ? 0 : (yy >= g.h ? g.h - 1 : yy);
    const uint8_t* p = src + (((int64_t)frame * g.h + yy) * g.w + xs) * C;
    const int a = (int)((uintptr_t)p & 3);
    if (i * 4 < a + len) raw[r][i] = *(const uint32_t*)(p - a + i * 4);
    if (i == 0) raw_a[r] = a;
  }
  __syncthreads();

  const uint8_t* rawb = (const uint8_t*)&raw[0][0];
  for (int idx = tid; idx < kMagH * kMagW; idx += 256) {
    const int my = idx / kMagW, mx = idx - my * kMagW;
    const int y = y0 - 1 + my, x = x0 - 1 + mx;
    int bdx = 0, bdy = 0, bm = 0;
    if (y >= 0 && y < g.h && x >= 0 && x < g.w) {  // outside the image the magnitude is 0 (constant pad)
      const int xl = (x > 0 ? x - 1 : 0) - xs, xc = x - xs, xr = (x < g.w - 1 ? x + 1 : x) - xs;
      bm = -1;
#pragma unroll
      for (int k = 0; k < C; ++k) {
        int v[3][3];
#pragma unroll
        for (int dr = 0; dr < 3; ++dr) {
          const int r = my + dr;  // raw row of image row y - 1 + dr (the rows were clamped when they were loaded)
          const uint8_t* row = rawb + r * (kRawDwords * 4) + raw_a[r] + k;
          v[dr][0] = row[xl * C];
          v[dr][1] = row[xc * C];
          v[dr][2] = row[xr * C];
        }
        const int gx = (v[0][2] + 2 * v[1][2] + v[2][2]) - (v[0][0] + 2 * v[1][0] + v[2][0]);
        const int gy = (v[2][0] + 2 * v[2][1] + v[2][2]) - (v[0][0] + 2 * v[0][1] + v[0][2]);
        const int m = abs(gx) + abs(gy);
        if (m > bm) {  // strict: the first channel wins ties
          bm = m;
          bdx = gx;
          bdy = gy;
        }
      }
    }
    sdx[my][mx] = (short)bdx;
    sdy[my][mx] = (short)bdy;
    smag[my][mx] = (short)bm;
  }
  __syncthreads();

  const int tx = tid & 63, x = x0 + tx;
#pragma unroll
  for (int j = 0; j < kTH / 4; ++j) {
    const int ty = (tid >> 6) + 4 * j, y = y0 + ty;
    if (x >= g.w || y >= g.h) continue;
    const int my = ty + 1, mx = tx + 1;
    const int dx = sdx[my][mx], dy = sdy[my][mx], c0 = smag[my][mx];
    const int ax = abs(dx), ay = abs(dy) << 15;
    const int tg22x = ax * 13573;
    const int tg67x = tg22x + (ax << 16);
    bool keep;
    if (ay < tg22x) {
      keep = c0 > smag[my][mx - 1] && c0 >= smag[my][mx + 1];
    } else if (ay > tg67x) {
      keep = c0 > smag[my - 1][mx] && c0 >= smag[my + 1][mx];
    } else {
      const int s = (dx ^ dy) < 0 ? -1 : 1;
      keep = c0 > smag[my - 1][mx - s] && c0 > smag[my + 1][mx + s];
    }
    const bool cand = keep && c0 > low;
    cls[((int64_t)frame * g.h + y) * g.w + x] = cand ? (c0 > high ? 2 : 1) : 0;
  }
}

// ---- union-find ----------------------------------------------------------------------------------------------------------------
// label[i] <= i always; a root has label[i] == i.  Unions only lower labels (atomicMin), so the forest stays a forest whatever
// the interleaving, and a stale read is still an ancestor.
__device__ __forceinline__ int ld_shared(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <bool GLOBAL>
__device__ __forceinline__ int uf_find(const int* lab, int i) {
  for (;;) {
    const int p = GLOBAL ? ld_agent(lab + i) : ld_shared(lab + i);
    if (p >= i || p < 0) return i;  // p == i: a root.  (Anything else cannot happen; the walk stays inside [0, i) regardless.)
    i = p;
  }
}

template <bool GLOBAL>
__device__ __forceinline__ void uf_union(int* lab, int a, int b) {
  for (;;) {
    a = uf_find<GLOBAL>(lab, a);
    b = uf_find<GLOBAL>(lab, b);
    if (a == b) return;
    if (a > b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(lab + b, a);  // b was a root iff old == b
    if (old == b || old < 0) return;
    b = old;
  }
}

// The links a candidate p makes: W, N, and NW / NE when N is no candidate (with N a candidate, NW - N and N - NE are W links of
// their own).  A link inside a tile belongs to k_label_tile (W: as row runs), one across a tile border to k_merge_tiles.
__global__ __launch_bounds__(256) void k_label_tile(const uint8_t* __restrict__ cls, int* __restrict__ label, uint8_t* __restrict__ flag, Geom g) {
  __shared__ int lab[kTH * kTW];
  const int tid = threadIdx.x, tx = tid & 63;
  int frame, y0, x0;
  tile_of_block(g, frame, y0, x0);
  const int x = x0 + tx;
  bool cand[kTH / 4];
#pragma unroll
  for (int j = 0; j < kTH / 4; ++j) {
    const int ty = (tid >> 6) + 4 * j, y = y0 + ty;
    const bool in = x < g.w && y < g.h;
    const int64_t gi = ((int64_t)frame * g.h + y) * g.w + x;
    cand[j] = in && cls[gi] != 0;
    if (in) flag[gi] = 0;
    // the first label is the start of the pixel's run of candidates in its tile row
    const unsigned long long run = __ballot(cand[j]);
    const unsigned long long gaps = ~run & ((1ull << tx) - 1ull);
    const int start = gaps ? 64 - __builtin_clzll(gaps) : 0;
    lab[ty * kTW + tx] = cand[j] ? ty * kTW + start : -1;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kTH / 4; ++j) {
    const int ty = (tid >> 6) + 4 * j, li = ty * kTW + tx;
    if (!cand[j] || ty == 0) continue;
    if (ld_shared(lab + li - kTW) >= 0) {
      uf_union<false>(lab, li, li - kTW);
    } else {
      if (tx > 0 && ld_shared(lab + li - kTW - 1) >= 0) uf_union<false>(lab, li, li - kTW - 1);
      if (tx < kTW - 1 && ld_shared(lab + li - kTW + 1) >= 0) uf_union<false>(lab, li, li - kTW + 1);
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kTH / 4; ++j) {
    const int ty = (tid >> 6) + 4 * j, y = y0 + ty;
    if (x >= g.w || y >= g.h) continue;
    int out = -1;
    if (cand[j]) {
      const int r = uf_find<false>(lab, ty * kTW + tx);
      out = (frame * g.h + y0 + (r >> 6)) * g.w + x0 + (r & 63);
    }
    label[((int64_t)frame * g.h + y) * g.w + x] = out;
  }
}

static_assert(kTW == 64, "k_label_tile: one wave per tile row, r >> 6 / r & 63");

// threads 0..63: the tile's top row; 64..79: its left column; 80..95: its right column (their top pixels belong to the top row)
__global__ __launch_bounds__(kMergeThreads) void k_merge_tiles(const uint8_t* __restrict__ cls, int* __restrict__ label, Geom g) {
  const int tid = threadIdx.x;
  int frame, y0, x0;
  tile_of_block(g, frame, y0, x0);
  int tx, ty;
  if (tid < kTW) {
    tx = tid;
    ty = 0;
  } else if (tid < kTW + kTH) {
    tx = 0;
    ty = tid - kTW;
  } else {
    tx = kTW - 1;
    ty = tid - kTW - kTH;
  }
  if (tid >= kTW && ty == 0) return;
  const int x = x0 + tx, y = y0 + ty;
  if (x >= g.w || y >= g.h) return;
  const int64_t gi = ((int64_t)frame * g.h + y) * g.w + x;
  const int p = (int)gi;  // a label: images * h * w < 2^31
  if (cls[gi] == 0) return;
  const bool has_n = y > 0, has_w = x > 0, has_e = x < g.w - 1;
  const bool n_cand = has_n && cls[gi - g.w] != 0;
  if (tx == 0 && has_w && cls[gi - 1] != 0) uf_union<true>(label, p, p - 1);
  if (n_cand) {
    if (ty == 0) uf_union<true>(label, p, p - g.w);
  } else if (has_n) {
    if ((tx == 0 || ty == 0) && has_w && cls[gi - g.w - 1] != 0) uf_union<true>(label, p, p - g.w - 1);
    if ((tx == kTW - 1 || ty == 0) && has_e && cls[gi - g.w + 1] != 0) uf_union<true>(label, p, p - g.w + 1);
  }
}

__global__ __launch_bounds__(256) void k_flatten(const uint8_t* __restrict__ cls, int* __restrict__ label, uint8_t* __restrict__ flag, int total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = cls[i];
  if (c == 0) return;
  const int r = uf_find<true>(label, (int)i);  // no unions in this launch: the roots are final
  label[i] = r;  // a plain store under other threads' walks: old or new, they read an ancestor of i and reach the same root
  if (c == 2) flag[r] = 1;
}

// ---- emit ------------------------------------------------------------------------------------------------------------------------
// 4 consecutive pixels per thread.  vec: h * w is a multiple of 4 and the outputs are aligned for 4-element stores.
template <typename T>
__global__ __launch_bounds__(256) void k_emit(const int* __restrict__ label, const uint8_t* __restrict__ flag, uint8_t* __restrict__ edges,
                                              T* __restrict__ ctrl, int total, int hw, int images, int rep, T one, int vec) {
  const int64_t g0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (g0 >= total) return;
  const int cnt = total - g0 < 4 ? (int)(total - g0) : 4;
  bool e[4] = {false, false, false, false};
  if (cnt == 4) {
    const int4 l = *(const int4*)(label + g0);  // the labels start the workspace, which is 16-byte aligned
    e[0] = l.x >= 0 && flag[l.x];
    e[1] = l.y >= 0 && flag[l.y];
    e[2] = l.z >= 0 && flag[l.z];
    e[3] = l.w >= 0 && flag[l.w];
  } else {
    for (int k = 0; k < cnt; ++k) {
      const int l = label[g0 + k];
      e[k] = l >= 0 && flag[l];
    }
  }
  if (edges) {
    if (vec && cnt == 4) {
      *(uint32_t*)(edges + g0) = (e[0] ? 0xffu : 0u) | (e[1] ? 0xff00u : 0u) | (e[2] ? 0xff0000u : 0u) | (e[3] ? 0xff000000u : 0u);
    } else {
      for (int k = 0; k < cnt; ++k) edges[g0 + k] = e[k] ? 255 : 0;
    }
  }
  if (ctrl) {
    const T zero = T(0);
    if (vec && cnt == 4) {
      const int frame = (int)(g0 / hw);
      const int64_t p = g0 - (int64_t)frame * hw;
      Vec4<T> v;  // (levels 0 / 255 of the contract: `one` is 255 / 255 in T)
#pragma unroll
      for (int k = 0; k < 4; ++k) v.v[k] = e[k] ? one : zero;
      const Vec4<T> v3[3] = {v, v, v};
      emit_vec4(ctrl, images, frame, hw, p, rep, v3);
    } else {
      for (int k = 0; k < cnt; ++k) {
        const int frame = (int)((g0 + k) / hw);
        emit_control1(ctrl, images, frame, hw, g0 + k - (int64_t)frame * hw, rep, e[k] ? 255 : 0);
      }
    }
  }
}

inline Geom geom(int32_t h, int32_t w) { return Geom{h, w, (w + kTW - 1) / kTW, (h + kTH - 1) / kTH}; }

}  // namespace

#define CA_CANNY_SIZES(name)                                                                                                  \
  CA_REQUIRE(sizes_ok(images, h, w), name ": images=%d h=%d w=%d (each >= 1, images * h * w < 2^31)", images, h, w)
#define CA_CANNY_WORKSPACE(name)                                                                                              \
  const WsLayout l = ws_layout((int64_t)images * h * w);                                                                      \
  CA_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= l.total,                                     \
             name ": a 16-byte aligned workspace of %lld bytes is needed, %lld given", (long long)l.total, (long long)workspace_bytes)

extern "C" int32_t ca_canny_tile_w(void) { return kTW; }
extern "C" int32_t ca_canny_tile_h(void) { return kTH; }

extern "C" int64_t ca_canny_workspace_bytes(int32_t images, int32_t h, int32_t w) {
  if (!sizes_ok(images, h, w)) return 0;
  return ws_layout((int64_t)images * h * w).total;
}

extern "C" int ca_canny_classify(const uint8_t* src, int32_t images, int32_t h, int32_t w, int32_t channels, int32_t low, int32_t high,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
  CA_REQUIRE(src, "ca_canny_classify: src is required");
  CA_CANNY_SIZES("ca_canny_classify");
  CA_REQUIRE(channels == 1 || channels == 3, "ca_canny_classify: channels=%d (1 or 3)", channels);
  CA_REQUIRE(low <= high, "ca_canny_classify: low=%d > high=%d", low, high);
  CA_CANNY_WORKSPACE("ca_canny_classify");
  const Geom g = geom(h, w);
  const dim3 grid((unsigned)((int64_t)images * g.tiles_x * g.tiles_y)), block(256);
  uint8_t* cls = (uint8_t*)workspace + l.cls;
  if (channels == 1)
    hipLaunchKernelGGL(k_classify<1>, grid, block, 0, (hipStream_t)stream, src, cls, g, (int)low, (int)high);
  else
    hipLaunchKernelGGL(k_classify<3>, grid, block, 0, (hipStream_t)stream, src, cls, g, (int)low, (int)high);
  CA_CHECK_LAUNCH("ca_canny_classify");
  return CA_OK;
}

namespace {

// One launch of the hysteresis (arguments already checked).
void launch_link_stage(int stage, int32_t images, int32_t h, int32_t w, void* workspace, const WsLayout& l, hipStream_t st) {
  const Geom g = geom(h, w);
  const int total = (int)((int64_t)images * h * w);
  const dim3 tiles((unsigned)((int64_t)images * g.tiles_x * g.tiles_y));
  int* label = (int*)((char*)workspace + l.label);
  const uint8_t* cls = (const uint8_t*)workspace + l.cls;
  uint8_t* flag = (uint8_t*)workspace + l.flag;
  if (stage == CA_CANNY_LINK_LABEL)
    hipLaunchKernelGGL(k_label_tile, tiles, dim3(256), 0, st, cls, label, flag, g);
  else if (stage == CA_CANNY_LINK_MERGE)
    hipLaunchKernelGGL(k_merge_tiles, tiles, dim3(kMergeThreads), 0, st, cls, label, g);
  else
    hipLaunchKernelGGL(k_flatten, dim3((unsigned)(((int64_t)total + 255) / 256)), dim3(256), 0, st, cls, label, flag, total);
}

}  // namespace

extern "C" int ca_canny_link(int32_t images, int32_t h, int32_t w, void* workspace, int64_t workspace_bytes, void* stream) {
  CA_CANNY_SIZES("ca_canny_link");
  CA_CANNY_WORKSPACE("ca_canny_link");
  for (int stage = CA_CANNY_LINK_LABEL; stage <= CA_CANNY_LINK_FLATTEN; ++stage)
    launch_link_stage(stage, images, h, w, workspace, l, (hipStream_t)stream);
  CA_CHECK_LAUNCH("ca_canny_link");
  return CA_OK;
}

extern "C" int ca_canny_link_stage(int32_t images, int32_t h, int32_t w, void* workspace, int64_t workspace_bytes, int32_t stage,
                                   void* stream) {
  CA_CANNY_SIZES("ca_canny_link_stage");
  CA_REQUIRE(stage >= CA_CANNY_LINK_LABEL && stage <= CA_CANNY_LINK_FLATTEN, "ca_canny_link_stage: stage=%d (0 label, 1 merge, 2 flatten)", stage);
  CA_CANNY_WORKSPACE("ca_canny_link_stage");
  launch_link_stage(stage, images, h, w, workspace, l, (hipStream_t)stream);
  CA_CHECK_LAUNCH("ca_canny_link_stage");
  return CA_OK;
}

extern "C" int ca_canny_emit(int32_t images, int32_t h, int32_t w, const void* workspace, int64_t workspace_bytes, uint8_t* edges,
                             void* control, int32_t rep, int32_t control_dtype, void* stream) {
  CA_CANNY_SIZES("ca_canny_emit");
  if (const int rc = control_out_checks("ca_canny_emit", false, h, w, "edges", edges || control, rep, control_dtype)) return rc;
  CA_CANNY_WORKSPACE("ca_canny_emit");
  const int total = (int)((int64_t)images * h * w);
  const int hw = (int)((int64_t)h * w);
  CA_REQUIRE(ctrl_aligned(control, control_dtype, 1), "ca_canny_emit: control is not aligned to its element size");
  const int vec = hw % 4 == 0 && ((uintptr_t)edges & 3) == 0 && ctrl_aligned(control, control_dtype, 4);  // (a NULL output is aligned)
  const int* label = (const int*)((const char*)workspace + l.label);
  const uint8_t* flag = (const uint8_t*)workspace + l.flag;
  const dim3 grid((unsigned)(((int64_t)total + 1023) / 1024)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (control_dtype == CA_F32)
    hipLaunchKernelGGL(k_emit<float>, grid, block, 0, st, label, flag, edges, (float*)control, total, hw, (int)images, (int)rep, 1.0f, vec);
  else
    hipLaunchKernelGGL(k_emit<u16>, grid, block, 0, st, label, flag, edges, (u16*)control, total, hw, (int)images, (int)rep, (u16)0x3c00, vec);
  CA_CHECK_LAUNCH("ca_canny_emit");
  return CA_OK;
}
