// MFMA GEMM / implicit-GEMM 3x3 convolution core for gfx950.
//
//   C[M,N] = epilogue(A[M,K] * W[N,K]^T),  A dense (linear / 1x1 conv) or gathered on the fly
//   from an NHWC activation (3x3 conv, pad 1, stride 1/2, optional nearest-x2 upsample and
//   two-source channel concat).  Both operands are K-contiguous, so MFMA fragments are plain
//   16-byte reads.
//
// Tiling: 256 threads = 4 waves, block tile BM x BN x 64, double-buffered LDS, one barrier per K
// tile.  Two staging variants share the MFMA loop and the epilogue:
//   k_gemm_dma  global->LDS by LDS-DMA (`buffer_load_dwordx4 ... lds`): no VGPR round trip, no
//               ds_write pass; out-of-range lanes (conv halo, M/N tails) are given an offset beyond
//               the buffer descriptor's size and the hardware writes zeros (probed on MI355X,
//               tools/probe_glds.hip).  The DMA writes lane-linear, so the bank swizzle is applied
//               to the per-lane SOURCE chunk and again on the fragment read (same involution).
//               Needs channel counts that are multiples of 64 (every UNet/ControlNet layer but conv_in).
//   k_gemm      register-staged copies issued one tile ahead; handles any multiple-of-8 shape.
// LDS rows are 128 B (64 elements);
// the 16-byte chunk index is XOR-swizzled with (row>>1)&7 so that every ds_read_b128 lane group
// of a fragment read hits 16 distinct 16-B slots (MI355X_MICROARCH.md, LDS table).
// MFMA is issued with swapped operands (mfma(Wfrag, Afrag)) so each lane ends up holding 4
// consecutive output columns of one output row -> 8-byte epilogue stores.

#include "ca_gemm_plan.h"  // the launch planner (host only): which kernel, how many K ranges, how much workspace

namespace {
using namespace ca_gemm_detail;
#include "ca_conv_wino.h"

template <int DT, int BM, int BN, int WAVES_M, int WAVES_N, int MODE>
__global__ __launch_bounds__(256) void k_gemm(GemmKParams p) {
  constexpr int TM = BM / WAVES_M / 16;
  constexpr int TN = BN / WAVES_N / 16;
  constexpr int AI = BM / 32;  // A rows per loader thread
  constexpr int BI = BN / 32;
  static_assert(2 * (BM + BN) * BK >= BM * (BN + 8), "epilogue staging must fit");
  __shared__ __attribute__((aligned(16))) u16 smem[2 * (BM + BN) * BK];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = wid / WAVES_N, wn = wid % WAVES_N;
  const int g = lane >> 4, l15 = lane & 15;

  const int tiles_n = (p.n + BN - 1) / BN;
  const unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
  int tile_m, tile_n;
  tile_coords(bid, (p.m + BM - 1) / BM, tiles_n, tile_m, tile_n);
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  // ---- loader setup -------------------------------------------------------------------
  const int lr = tid >> 3;  // 0..31
  const int lc = tid & 7;   // 16-byte chunk within the 64-wide K tile
  const int kc = p.c1 + p.c2;
  const int64_t wld = (int64_t)p.taps * kc;

  // per-row state of the A loader
  int a_img[AI], a_ho[AI], a_wo[AI];
  bool a_ok[AI];
  int64_t a_rowoff[AI];
#pragma unroll
  for (int i = 0; i < AI; ++i) {
    int m = m0 + lr + 32 * i;
    a_ok[i] = m < p.m;
    if (MODE == 1) {
      int mm = a_ok[i] ? m : 0;
      int hw = p.hout * p.wout;
      a_img[i] = mm / hw;
      int rem = mm - a_img[i] * hw;
      a_ho[i] = rem / p.wout;
      a_wo[i] = rem - a_ho[i] * p.wout;
      a_rowoff[i] = 0;
    } else {
      a_img[i] = a_ho[i] = a_wo[i] = 0;
      a_rowoff[i] = (int64_t)m;
    }
  }
  bool b_ok[BI];
  int64_t b_rowoff[BI];
#pragma unroll
  for (int i = 0; i < BI; ++i) {
    int n = n0 + lr + 32 * i;
    b_ok[i] = n < p.n;
    b_rowoff[i] = (int64_t)n * wld;
  }

  u32x4 ra[AI], rb[BI];
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

  auto load_tile = [&](int t) {
    int tap, cc;
    k_tile_split(p, t, p.kc_tiles, tap, cc);
    int ci = cc * BK + lc * 8;
    bool cok = ci < kc;
    // weights
#pragma unroll
    for (int i = 0; i < BI; ++i) {
      rb[i] = (cok && b_ok[i]) ? ld16(p.w + b_rowoff[i] + (int64_t)tap * kc + ci) : zero4;
    }
    // activations
    const bool src2 = ci >= p.c1;
    const u16* base = src2 ? p.a2 : p.a;
    const int cs = src2 ? p.c2 : p.c1;
    const int cio = src2 ? ci - p.c1 : ci;
    if (MODE == 1) {
      int kh = tap / 3, kw = tap - kh * 3;
#pragma unroll
      for (int i = 0; i < AI; ++i) {
        int hi = a_ho[i] * p.stride + kh - p.pad_lo;
        int wi = a_wo[i] * p.stride + kw - p.pad_lo;
        bool ok = cok && a_ok[i] && hi >= 0 && wi >= 0 && hi < (p.hin << p.ups) && wi < (p.win << p.ups);
        int hs = hi >> p.ups, ws = wi >> p.ups;
        int64_t pix = ((int64_t)a_img[i] * p.hin + hs) * p.win + ws;
        ra[i] = ok ? ld16(base + pix * cs + cio) : zero4;
      }
    } else {
      const int64_t ld = src2 ? p.lda2 : p.lda;
#pragma unroll
      for (int i = 0; i < AI; ++i) {
        ra[i] = (cok && a_ok[i]) ? ld16(base + a_rowoff[i] * ld + cio) : zero4;
      }
    }
  };
  auto store_tile = [&](int buf) {
    u16* sa = smem + buf * (BM + BN) * BK;
    u16* sb = sa + BM * BK;
#pragma unroll
    for (int i = 0; i < AI; ++i) st16(sa + lds_off(lr + 32 * i, lc), ra[i]);
#pragma unroll
    for (int i = 0; i < BI; ++i) st16(sb + lds_off(lr + 32 * i, lc), rb[i]);
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nt = p.taps * p.kc_tiles;
  load_tile(0);
  store_tile(0);
  __syncthreads();

  for (int t = 0; t < nt; ++t) {
    const int buf = t & 1;
    if (t + 1 < nt) load_tile(t + 1);
    const u16* sa = smem + buf * (BM + BN) * BK;
    const u16* sb = sa + BM * BK;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      u32x4 fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[i] = ld16(sa + lds_off(wm * TM * 16 + i * 16 + l15, s * 4 + g));
#pragma unroll
      for (int j = 0; j < TN; ++j) fb[j] = ld16(sb + lds_off(wn * TN * 16 + j * 16 + l15, s * 4 + g));
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = Elem<DT>::mfma(fb[j], fa[i], acc[i][j]);
    }
    if (t + 1 < nt) store_tile(buf ^ 1);
    __syncthreads();
  }

  gemm_epilogue<DT, BM, BN, TM, TN>(p, acc, smem, m0, n0, wm, wn, l15, g, tid);
}

// ---- LDS-DMA variant ------------------------------------------------------------------------

// NBUF = 1: one LDS stage, two `__syncthreads()` per tile (hipcc precedes them with vmcnt(0)); 4 blocks (128 x 160 tiles: 3)
//           per CU cover each other's transfer latency.
// NBUF = 3: tiles are issued NBUF - 1 ahead into a ring; a wave waits with a COUNTED
//           `s_waitcnt vmcnt(per-tile DMA count x younger tiles)` (tile t landed, the younger ones may still be in
//           flight), then a raw s_barrier: DMA transfers stay in flight across barriers
//           (cdna_hip_programming.md "Pipelining across barriers").  All LDS is one array; 2 blocks per CU.
// Instantiated (launch_gemm): 128x160 / 1, 128x128 / 1, 128x64 / 1 and 128x64 / 3; the double buffer, deeper rings, 256-row
// tiles and a 32-wide K stage were measured and lost.
template <int DT, int BM, int BN, int WAVES_M, int WAVES_N, int MODE, int NBUF>
__global__ __launch_bounds__(256, NBUF == 1 ? (BN > 128 ? 3 : 4) : 2)
void k_gemm_dma(GemmKParams p) {
  static_assert(WAVES_M * WAVES_N == 4 && (NBUF == 1 || NBUF == 3), "instantiations: see above");
  constexpr int KT = BK;             // K elements per LDS stage: one 128-byte row per tile row
  constexpr int CPR = KT / 8;        // 16-byte chunks per LDS row
  constexpr int RPI = 64 / CPR;      // tile rows one wave-wide DMA instruction covers
  constexpr int NW = WAVES_M * WAVES_N, NT = NW * 64;
  constexpr int TM = BM / WAVES_M / 16;
  constexpr int TN = BN / WAVES_N / 16;
  constexpr int AG = BM / RPI / NW;  // DMA instructions per wave per stage (A)
  constexpr int BG = BN / RPI / NW;  // (W)
  // the LDS-staged epilogue needs BM x (BN + 8) elements: more than ONE 128x128x64 stage
  constexpr int SMEM_ELEMS = NBUF * (BM + BN) * KT > BM * (BN + 8) ? NBUF * (BM + BN) * KT : BM * (BN + 8);
  // XOR swizzle of the chunk index: conflict-free ds_read_b128 for the hardware's 16-lane groups
  auto swz = [](int row) { return (row >> 1) & 7; };
  auto lds_at = [&](int row, int chunk) { return row * KT + ((chunk ^ swz(row)) << 3); };
  __shared__ __attribute__((aligned(16))) u16 smem[SMEM_ELEMS];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = wid / WAVES_N, wn = wid % WAVES_N;
  const int g = lane >> 4, l15 = lane & 15;

  const int tiles_n = (p.n + BN - 1) / BN;
  const int tiles_m = (p.m + BM - 1) / BM;
  unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
  int split = 0;
  if (p.splits > 1) {  // consecutive ids = the tiles of ONE K range (they share the weight slices)
    split = bid / (unsigned)(tiles_m * tiles_n);
    bid -= split * (unsigned)(tiles_m * tiles_n);
  }
  int tile_m, tile_n;
  tile_coords(bid, tiles_m, tiles_n, tile_m, tile_n);
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc((void*)p.a, 0, p.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_a2 = __builtin_amdgcn_make_buffer_rsrc((void*)(p.a2 ? p.a2 : p.a), 0, p.a2 ? p.a2_bytes : p.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, p.w_bytes, 0x00020000);

  const int r8 = lane / CPR, cp = lane % CPR;  // row inside a DMA row group, LDS chunk position
  const int kc = p.c1 + p.c2;
  const int kct = kc / KT;  // K tiles per tap (the DMA path requires kc % 64 == 0)
  const unsigned wld = (unsigned)(p.taps * kc);

  // per staged row: swizzled source chunk, and either a byte offset (dense / weights) or pixel coords (conv)
  int a_chunk[AG], a_img[AG], a_ho[AG], a_wo[AG];
  unsigned a_off1[AG], a_off2[AG];
  bool a_ok[AG];
#pragma unroll
  for (int i = 0; i < AG; ++i) {
    const int row = (wid * AG + i) * RPI + r8;
    a_chunk[i] = cp ^ swz(row);
    const int m = m0 + row;
    a_ok[i] = m < p.m;
    const int mm = a_ok[i] ? m : p.m - 1;
    if (MODE == 1) {
      const int hw = p.hout * p.wout;
      a_img[i] = mm / hw;
      const int rem = mm - a_img[i] * hw;
      a_ho[i] = rem / p.wout;
      a_wo[i] = rem - a_ho[i] * p.wout;
      a_off1[i] = a_off2[i] = 0;
    } else {
      a_img[i] = a_ho[i] = a_wo[i] = 0;
      a_off1[i] = (unsigned)((int64_t)mm * p.lda * 2);
      a_off2[i] = (unsigned)((int64_t)mm * p.lda2 * 2);
    }
  }
  int b_chunk[BG];
  unsigned b_off[BG];
#pragma unroll
  for (int j = 0; j < BG; ++j) {
    const int row = (wid * BG + j) * RPI + r8;
    b_chunk[j] = cp ^ swz(row);
    int n = n0 + row;
    if (n >= p.n) n = p.n - 1;  // clamped rows feed accumulators that are never stored
    b_off[j] = (unsigned)n * wld * 2u;
  }

  auto stage = [&](int t, int buf) {
    u16* sa = smem + buf * (BM + BN) * KT;
    u16* sb = sa + BM * KT;
    int tap, cc;
    k_tile_split(p, t, kct, tap, cc);
    const int c0 = cc * KT;            // first channel of this K tile (tile-uniform)
    const bool src2 = c0 >= p.c1;      // c1 % 64 == 0 => a tile never straddles the two sources
    const int cs = src2 ? p.c2 : p.c1;
    const int cbase = src2 ? c0 - p.c1 : c0;
#pragma unroll
    for (int j = 0; j < BG; ++j) {
      const unsigned off = b_off[j] + (unsigned)(tap * kc + c0 + b_chunk[j] * 8) * 2u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (__attribute__((address_space(3))) void*)(sb + (wid * BG + j) * RPI * KT), 16, off, 0, 0, 0);
    }
    if (MODE == 1) {
      const int kh = tap / 3, kw = tap - kh * 3;
#pragma unroll
      for (int i = 0; i < AG; ++i) {
        const int hi = a_ho[i] * p.stride + kh - p.pad_lo;
        const int wi = a_wo[i] * p.stride + kw - p.pad_lo;
        const bool ok = a_ok[i] && hi >= 0 && wi >= 0 && hi < (p.hin << p.ups) && wi < (p.win << p.ups);
        const int pix = (a_img[i] * p.hin + (hi >> p.ups)) * p.win + (wi >> p.ups);
        const unsigned off = ok ? ((unsigned)pix * (unsigned)cs + (unsigned)(cbase + a_chunk[i] * 8)) * 2u : DMA_OOB;
        void* dst = sa + (wid * AG + i) * RPI * KT;
        if (src2) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_a2, (__attribute__((address_space(3))) void*)dst, 16, off, 0, 0, 0);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_a, (__attribute__((address_space(3))) void*)dst, 16, off, 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int i = 0; i < AG; ++i) {
        const unsigned off = (src2 ? a_off2[i] : a_off1[i]) + (unsigned)(cbase + a_chunk[i] * 8) * 2u;
        void* dst = sa + (wid * AG + i) * RPI * KT;
        if (src2) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_a2, (__attribute__((address_space(3))) void*)dst, 16, off, 0, 0, 0);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_a, (__attribute__((address_space(3))) void*)dst, 16, off, 0, 0, 0);
      }
    }
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nt_all = p.taps * kct;
  const int t_first = p.splits > 1 ? (int)((int64_t)nt_all * split / p.splits) : 0;
  const int nt = (p.splits > 1 ? (int)((int64_t)nt_all * (split + 1) / p.splits) : nt_all) - t_first;
  auto compute = [&](int buf) {
    const u16* sa = smem + buf * (BM + BN) * KT;
    const u16* sb = sa + BM * KT;
    // (tid and lane stay captured, in this position: the removed timing ablations named them here, and without the two closure
    //  fields hipcc orders the inlined body differently -- other registers and schedule in every k_gemm_dma.  Dropping this line
    //  is a code-generation change to be measured, not a clean-up.)
    (void)tid, (void)lane;
#pragma unroll
    for (int s = 0; s < KT / 32; ++s) {
      u32x4 fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[i] = ld16(sa + lds_at(wm * TM * 16 + i * 16 + l15, s * 4 + g));
#pragma unroll
      for (int j = 0; j < TN; ++j) fb[j] = ld16(sb + lds_at(wn * TN * 16 + j * 16 + l15, s * 4 + g));
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = Elem<DT>::mfma(fb[j], fa[i], acc[i][j]);
    }
  };
  if (NBUF == 1) {
    // single LDS buffer (32 KB for 128x128): two barriers per tile, but 3 blocks per CU -- the
    // other resident blocks' MFMA phases cover this block's transfer latency
    for (int t = 0; t < nt; ++t) {
      stage(t_first + t, 0);
      __syncthreads();  // hipcc drains the LDS-DMA queue (vmcnt(0)) ahead of the barrier
      compute(0);
      __syncthreads();
    }
  } else {
    // NBUF >= 3 (round 4): a ring with NBUF - 1 tiles in flight, for the launches whose K loop is a chain of DMA round trips with
    // almost nothing to compute per tile (M = 2048: the 8x8-latent level -- 8 MFMAs per wave and K tile against ~1.2 us per
    // round trip).  With two stages ONE tile would be in flight while the previous one is computed; here tile t is awaited with a
    // COUNTED vmcnt (the pieces of the min(NBUF - 2, tiles left) younger tiles stay outstanding), one raw barrier per tile
    // publishes it, and tile t + NBUF - 1 goes into the slot whose reads the same barrier has just retired.
    constexpr int PER = AG + BG;  // DMA instructions per wave and stage
    static_assert((NBUF - 2) * PER < 64, "vmcnt");
#pragma unroll
    for (int s = 0; s < NBUF - 1; ++s)
      if (s < nt) stage(t_first + s, s);
    int slot = 0, slot_in = NBUF - 1;
    for (int t = 0; t < nt; ++t) {
      const int younger = nt - 1 - t < NBUF - 2 ? nt - 1 - t : NBUF - 2;
      if (younger <= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER) : "memory");
      else if (younger == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PER) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NBUF - 2) * PER < 64 ? (NBUF - 2) * PER : 0) : "memory");
      __builtin_amdgcn_s_barrier();
      if (t + NBUF - 1 < nt) stage(t_first + t + NBUF - 1, slot_in);
      compute(slot);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (this tile's fragment reads have returned before the next barrier lets its slot go)
      slot = slot + 1 == NBUF ? 0 : slot + 1;
      slot_in = slot_in + 1 == NBUF ? 0 : slot_in + 1;
    }
    __syncthreads();  // the staged epilogue re-uses the ring's LDS
  }
  if (p.splits > 1) {  // raw fp32 slab; lane holds C[m = .. + l15][n = .. + 4g + (0..3)]
    float* slab = p.partial + (int64_t)split * p.m * p.n;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = m0 + wm * TM * 16 + i * 16 + l15;
      if (m >= p.m) continue;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * TN * 16 + j * 16 + g * 4;
        if (n < p.n) *reinterpret_cast<f32x4*>(slab + (int64_t)m * p.n + n) = acc[i][j];
      }
    }
    return;
  }
  gemm_epilogue<DT, BM, BN, TM, TN, NT>(p, acc, smem, m0, n0, wm, wn, l15, g, tid);
}

// Adds the split-K slabs in split order and applies the same epilogue as gemm_epilogue (including its
// rounding of (acc + bias + rowbias) * alpha to the activation type before the residual add).
template <int DT>
__global__ __launch_bounds__(256) void k_splitk_reduce(GemmKParams p) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c8n = p.n >> 3;
  const int64_t m = id / c8n;
  if (m >= p.m) return;
  const int n = (int)(id - m * c8n) * 8;
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = 0.f;
  for (int sp = 0; sp < p.splits; ++sp) {
    const float* src = p.partial + ((int64_t)sp * p.m + m) * p.n + n;
    const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] += a[k];
      v[4 + k] += b[k];
    }
  }
  if (p.ln_stats) {  // folded LayerNorm: rstd * (x W'^T - mean * colsum(W'))
    const float2 st = *reinterpret_cast<const float2*>(p.ln_stats + m * 2);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = st.y * (v[k] - st.x * p.ln_colsum[n + k]);
  }
  if (p.bias) {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] += p.bias[n + k];
  }
  if (p.rowbias) {
    const float* rbp = p.rowbias + (m / p.rows_per_group) * p.ld_rowbias + n;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] += rbp[k];
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] *= p.alpha;
  unpack8<DT>(pack8<DT>(v), v);
  if (p.res) {
    float r[8];
    unpack8<DT>(ld16(p.res + m * p.ld_res + n), r);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] += r[k];
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] *= p.post;
  if (p.act != CA_ACT_NONE) {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = act_f(v[k], p.act);
  }
  const int64_t off = m * p.ldc + n;
  if (p.out_f32) {
    float* cp = reinterpret_cast<float*>(p.c) + off;
    *reinterpret_cast<f32x4*>(cp) = (f32x4){v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(cp + 4) = (f32x4){v[4], v[5], v[6], v[7]};
  } else {
    st16(reinterpret_cast<u16*>(p.c) + off, pack8<DT>(v));
  }
}

// the plan (plan_gemm, ca_gemm_plan.h) -> the template instantiation it names
template <int DT, int MODE>
int launch_gemm(const GemmKParams& p, const GemmPlan& g, hipStream_t st) {
  const dim3 grid(ceil_div_i(p.m, g.bm) * ceil_div_i(p.n, g.bn));  // (the one-block-per-tile kernels below)
  switch (g.kind) {
    case PK_WRES: return ca_launch_gemm_pp(p, DT, MODE, PK_WRES, 0u, st);
    case PK_AR: return ca_launch_gemm_ar(p, DT, st);
    case PK_PP2:
    case PK_PS:
    case PK_PQ: return ca_launch_gemm_pp(p, DT, MODE, g.kind, g.tiles, st);
    case PK_PP2_SPLITK: {
      GemmKParams q = p;
      q.splits = g.splits;
      const int rc = ca_launch_gemm_pp(q, DT, MODE, PK_PP2, g.tiles * (unsigned)g.splits, st);
      hipLaunchKernelGGL((k_splitk_reduce<DT>), dim3(ceil_div_i((int64_t)q.m * (q.n / 8), 256)), dim3(256), 0, st, q);
      return rc;
    }
    case PK_DMA_SPLITK:
      hipLaunchKernelGGL((k_gemm_dma<DT, 128, 128, 2, 2, MODE, 1>), dim3(g.tiles * (unsigned)p.splits), dim3(256), 0, st, p);
      hipLaunchKernelGGL((k_splitk_reduce<DT>), dim3(ceil_div_i((int64_t)p.m * (p.n / 8), 256)), dim3(256), 0, st, p);
      return CA_OK;
    case PK_DMA:  // the instantiations plan_gemm can ask for
      if (g.bn == 160 && g.nbuf == 1) hipLaunchKernelGGL((k_gemm_dma<DT, 128, 160, 2, 2, MODE, 1>), grid, dim3(256), 0, st, p);
      else if (g.bn == 128 && g.nbuf == 1) hipLaunchKernelGGL((k_gemm_dma<DT, 128, 128, 2, 2, MODE, 1>), grid, dim3(256), 0, st, p);
      else if (g.bn == 64 && g.nbuf == 1) hipLaunchKernelGGL((k_gemm_dma<DT, 128, 64, 4, 1, MODE, 1>), grid, dim3(256), 0, st, p);
      else if (g.bn == 64 && g.nbuf == 3) hipLaunchKernelGGL((k_gemm_dma<DT, 128, 64, 4, 1, MODE, 3>), grid, dim3(256), 0, st, p);
      else break;
      return CA_OK;
    case PK_REG:
      if (g.bn == 128) hipLaunchKernelGGL((k_gemm<DT, 128, 128, 2, 2, MODE>), grid, dim3(256), 0, st, p);
      else if (g.bn == 64) hipLaunchKernelGGL((k_gemm<DT, 128, 64, 4, 1, MODE>), grid, dim3(256), 0, st, p);
      else break;
      return CA_OK;
  }
  CA_FAIL(CA_ERR_LAUNCH, "ca_gemm: no kernel for plan kind %d, tile %dx%d, %d stages", (int)g.kind, g.bm, g.bn, g.nbuf);
}

}  // namespace

extern "C" int ca_gemm(const ca_gemm_args* a, void* stream) {
  DenseLaunch d;
  int rc = gemm_prepare(a, d);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  rc = a->dtype == CA_BF16 ? launch_gemm<CA_BF16, 0>(d.p, d.plan, st) : launch_gemm<CA_F16, 0>(d.p, d.plan, st);
  if (rc) return rc;
  CA_CHECK_LAUNCH("ca_gemm");
  return CA_OK;
}

// ---- questions about a dense launch, each over the same resolved view as ca_gemm itself (gemm_resolve, ca_gemm_plan.h)
extern "C" int64_t ca_gemm_workspace_bytes(const ca_gemm_args* a) {
  DenseLaunch d;
  return gemm_resolve(a, d) == CA_OK ? d.workspace : 0;
}

extern "C" int ca_gemm_row_sums_parts(const ca_gemm_args* a) {
  DenseLaunch d;
  DenseAsk ask{};
  ask.without_row_sums = true;  // (the question is about the launch, whatever the pointer)
  return gemm_resolve(a, d, ask) == CA_OK ? row_sums_parts_of(d.p) : 0;
}

extern "C" int ca_gemm_ln_inline_supported(const ca_gemm_args* a) {
  DenseLaunch d;
  return a && a->ln_colsum && gemm_resolve(a, d) == CA_OK && wres_eligible(d.p) ? 1 : 0;
}

// 1 if this launch, which hands over partial sums (ln_parts > 0), would run on a kernel that takes finished (mean, rstd) only
// and is the faster one for the shape (the 256 x 320 streaming kernel): the caller then finishes the sums (ca_ln_finish_sums)
// and passes ln_parts = 0.
extern "C" int ca_gemm_wants_finished_stats(const ca_gemm_args* a) {
  if (!a || !a->ln_colsum || !a->ln_stats || a->ln_parts <= 0 || a->row_sums_out) return 0;
  DenseLaunch d;
  DenseAsk ask{};
  ask.stats_finished = true;
  return gemm_resolve(a, d, ask) == CA_OK && d.plan.kind == PK_PQ ? 1 : 0;
}

extern "C" int64_t ca_conv3x3_workspace_bytes(const ca_conv_args* a) { return conv_workspace_bytes(a); }

static int launch_conv_wino(const ca_conv_args* a, const GemmKParams& cp, hipStream_t st) {
  const int kc = a->cin1 + a->cin2;
  const ConvGeom g = conv_geom(a);
  const int64_t tiles = wino_tiles(a, g);
  WinoParams w{};
  w.x = (const u16*)a->x;
  w.x2 = (const u16*)a->x2;
  w.v = (u16*)a->workspace;
  u16* mm = (u16*)a->workspace + (a->x_is_wino_v ? 0 : 16 * tiles * kc);
  w.mm = mm;
  w.y = (u16*)a->y;
  w.bias = a->bias;
  w.rowbias = a->rowbias;
  w.res = (const u16*)a->residual;
  w.ld_res = a->ld_res;
  w.ld_rowbias = a->ld_rowbias;
  w.images = a->images, w.h = g.hl, w.w = g.wl, w.c1 = a->cin1, w.c2 = a->cin2, w.cout = a->cout;
  w.ups = a->upsample;
  w.rows_per_group = cp.rows_per_group;
  w.alpha = a->alpha, w.post = a->post_scale, w.act = a->act;
  const int64_t in_threads = tiles * (kc / 8), out_threads = tiles * (a->cout / 8);
  if (a->x_is_wino_v) w.v = (u16*)a->x;  // V was written by the GroupNorm in front (ca_groupnorm_args.wino_v)
  else if (a->dtype == CA_BF16) hipLaunchKernelGGL((k_wino_in<CA_BF16>), dim3((unsigned)((in_threads + 255) / 256)), dim3(256), 0, st, w);
  else hipLaunchKernelGGL((k_wino_in<CA_F16>), dim3((unsigned)((in_threads + 255) / 256)), dim3(256), 0, st, w);
  // the sixteen transformed GEMMs as ONE launch of the 256 x 320 kernel: A = V [16 T, kc], weights U_f for the rows of group f
  GemmKParams q{};
  q.a = w.v;
  q.w = (const u16*)a->w_wino;
  q.c = mm;
  q.lda = kc;
  q.ldc = a->cout;
  q.a_bytes = desc_bytes(16 * tiles * kc);
  q.w_bytes = desc_bytes((int64_t)16 * a->cout * kc);
  q.m = (int)(16 * tiles);
  q.n = a->cout;
  q.c1 = kc;
  q.taps = 1;
  q.kc_tiles = kc / BK;
  q.rows_per_group = 1;
  q.alpha = 1.f, q.post = 1.f;
  q.splits = 1;
  q.w_group_rows = (int)tiles;
  q.w_group_stride = (unsigned)((int64_t)a->cout * kc * 2);
  const unsigned gemm_tiles = (unsigned)((q.m / 256) * (q.n / 320));
  int rc = ca_launch_gemm_pp(q, a->dtype, 0, PK_PQ, gemm_tiles, st);
  if (rc) return rc;
  if (a->dtype == CA_BF16) hipLaunchKernelGGL((k_wino_out<CA_BF16>), dim3((unsigned)((out_threads + 255) / 256)), dim3(256), 0, st, w);
  else hipLaunchKernelGGL((k_wino_out<CA_F16>), dim3((unsigned)((out_threads + 255) / 256)), dim3(256), 0, st, w);
  return CA_OK;
}

extern "C" int ca_pack_w_wino(const void* w, int32_t cout, int32_t cin, int32_t dtype, void* dst, void* stream) {
  CA_REQUIRE(w && dst, "ca_pack_w_wino: null operand");
  CA_REQUIRE(cout > 0 && cin > 0 && (dtype == CA_BF16 || dtype == CA_F16), "ca_pack_w_wino: cout=%d cin=%d dtype=%d", cout, cin, dtype);
  const int64_t n = (int64_t)cout * cin;
  CA_DISPATCH_DT(dtype, hipLaunchKernelGGL((k_pack_w_wino<DT>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const u16*)w, (u16*)dst, cout, cin));
  CA_CHECK_LAUNCH("ca_pack_w_wino");
  return CA_OK;
}

extern "C" int ca_conv3x3(const ca_conv_args* a, void* stream) {
  GemmKParams p{};
  int rc = conv_prepare(a, p);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (wino_taken(a)) {
    rc = launch_conv_wino(a, p, st);
    if (rc) return rc;
    CA_CHECK_LAUNCH("ca_conv3x3(winograd)");
    return CA_OK;
  }
  CA_REQUIRE(!a->x_is_wino_v, "ca_conv3x3: x_is_wino_v, but the Winograd route does not take these arguments (images=%d %dx%d cin=%d+%d cout=%d dtype=%d w_wino=%p "
             "workspace=%p of %lld bytes, needs %lld)", a->images, a->hin, a->win, a->cin1, a->cin2, a->cout, a->dtype, a->w_wino, a->workspace,
             (long long)a->workspace_bytes, (long long)wino_workspace_bytes(a));
  rc = a->dtype == CA_BF16 ? launch_gemm<CA_BF16, 1>(p, plan_gemm(p, 1), st) : launch_gemm<CA_F16, 1>(p, plan_gemm(p, 1), st);
  if (rc) return rc;
  CA_CHECK_LAUNCH("ca_conv3x3");
  return CA_OK;
}

extern "C" int ca_conv_up2_phase_supported(const ca_conv_args* a) {
  GemmKParams p{};
  return up2_capable(a, p) && up2_pays(p) ? 1 : 0;
}

extern "C" int ca_conv_up2_phase(const ca_conv_args* a, void* stream) {
  GemmKParams p{};
  CA_REQUIRE(up2_capable(a, p), "ca_conv_up2_phase: arguments the phase form does not take (one fp16 / bf16 source with cin %% 64 == 0, cout %% 320 == 0, upsample = 1, "
             "stride 1, symmetric padding, no row bias / activation / post scale / fp32 output, 16-byte aligned operands, < 2^23 source pixels)");
  int rc = ca_launch_gemm_pp(p, a->dtype, 2, PK_PQ, up2_tiles_total(p), (hipStream_t)stream);
  if (rc) return rc;
  CA_CHECK_LAUNCH("ca_conv_up2_phase");
  return CA_OK;
}

extern "C" int ca_conv_up2_phase_plan_name(const ca_conv_args* a, char* buf, int32_t len) {
  CA_REQUIRE(buf && len > 0, "ca_conv_up2_phase_plan_name: buffer");
  GemmKParams p{};
  CA_REQUIRE(up2_capable(a, p), "ca_conv_up2_phase_plan_name: arguments the phase form does not take");
  snprintf(buf, (size_t)len, "up2_pq256x320");
  return CA_OK;
}

// ---- which kernel would these arguments run?  (no launch, no device access: the pointers only have to be non-NULL where
// the launch requires them)
extern "C" int ca_gemm_plan_name(const ca_gemm_args* a, char* buf, int32_t len) {
  CA_REQUIRE(buf && len > 0, "ca_gemm_plan_name: buffer");
  DenseLaunch d;
  int rc = gemm_prepare(a, d);
  if (rc) return rc;
  plan_label(d.plan, buf, len);
  return CA_OK;
}

extern "C" int ca_conv3x3_plan_name(const ca_conv_args* a, char* buf, int32_t len) {
  CA_REQUIRE(buf && len > 0, "ca_conv3x3_plan_name: buffer");
  GemmKParams p{};
  int rc = conv_prepare(a, p);
  if (rc) return rc;
  if (wino_taken(a)) {
    snprintf(buf, (size_t)len, "wino_pq256x320");
    return CA_OK;
  }
  plan_label(plan_gemm(p, 1), buf, len);
  return CA_OK;
}
