// The launch planner of the GEMM / implicit-GEMM convolution entry points (ca_gemm.hip): WHICH kernel a set of arguments runs, in how
// many K ranges and with how much workspace.  Host arithmetic on sizes, flags and pointer presence only -- no kernel, no launch, no
// device: the entry points are thin wrappers over it, and every question about a launch has ONE answer here (the LDS-DMA predicate,
// the split-K rule and decision, the convolution geometry, the resolved dense launch).
#pragma once
#include "ca_gemm_core.h"

namespace ca_gemm_detail {

// descriptor size in bytes, or 0 when the buffer is too large for 32-bit offsets (-> register variant)
inline unsigned desc_bytes(int64_t elems) {
  const int64_t b = elems * 2;
  return (b > 0 && b < (int64_t)0xFFFFFF00ll) ? (unsigned)b : 0u;
}

// Can this launch stage its operands by LDS-DMA (k_gemm_dma and every tiled kernel)?  THE predicate: whoever asks calls it.  Its two
// halves: whole 64-channel K tiles that never straddle the two sources (shape), and operands a 32-bit buffer descriptor can address
// (size: desc_bytes gave each a size) -- the weight-resident and phase-convolution kernels have tile rules of their own and ask for
// the size half alone.
inline bool dma_shape_ok(const GemmKParams& p) { return (p.c1 + p.c2) % BK == 0 && (p.c2 == 0 || p.c1 % BK == 0); }
inline bool dma_sizes_ok(const GemmKParams& p) { return p.a_bytes != 0 && p.w_bytes != 0 && (p.c2 == 0 || p.a2_bytes != 0); }
inline bool dma_capable(const GemmKParams& p) { return dma_shape_ok(p) && dma_sizes_ok(p); }

// Weight-resident streaming kernel (ca_gemm_wres.h) for the K = 320 GEMMs of the 64x64-latent level: does this dense
// launch take it?  M >= 16384 (measured: a tie at 32768 rows, ahead above).  (Also the condition under which ca_gemm can
// compute folded-LayerNorm statistics itself: ca_gemm_ln_inline_supported.)  The kernel reads ln_stats as (mean, rstd)
// per row: a launch that hands over partial sums (ln_parts) is not eligible.
inline bool wres_eligible(const GemmKParams& p) {
  static const int wres_env = CA_KNOB("CA_GEMM_WRES", -1);  // (experiment builds: 0 = never, 1 = whenever the shape qualifies)
  const int kc = p.c1 + p.c2;
  return wres_env != 0 && kc == 320 && p.taps == 1 && (p.c2 == 0 || p.c1 % 32 == 0) && p.n % 160 == 0 && p.n / 160 <= 32 && !p.out_f32 &&
         p.splits <= 1 && !p.ln_parts && dma_sizes_ok(p) &&
         (!p.rowbias || p.rows_per_group % 32 == 0) &&
         act_out_fit31(p) &&  // (w_bytes needs no bound here: K = 320 and N <= 32 x 160 make the weights 3.3 MB at most)
         (wres_env == 1 || p.m >= 16384);
}

// Activation-resident kernel (ca_gemm_ar.h, round 4): the same K = 320 launches when the caller also hands over W in fragment
// order (ca_gemm_args.w_frag).  A subset of what the weight-resident kernel takes: one A source, N a multiple of 64 (64-column
// panels dealt to four waves), alpha = post = 1, no activation, residual only without LayerNorm / GEGLU, row-bias groups of whole
// 128-row tiles; in-kernel LayerNorm statistics need the caller's scratch (p.partial: 8 M bytes) -- `scratch`: is it there?  (The
// workspace query asks "if it were".)
// CA_GEMM_AR (experiment builds): 0 = never, 1 = every launch it can take (also N = 320), default: N >= 960.
inline bool ar_eligible(const GemmKParams& p, bool scratch) {
  static const int ar_env = CA_KNOB("CA_GEMM_AR", -1);
  if (ar_env == 0 || !p.wf || !wres_eligible(p)) return false;
  return p.c2 == 0 && p.n % 64 == 0 && p.alpha == 1.f && p.post == 1.f && p.act == CA_ACT_NONE && !p.row_sums && ((uintptr_t)p.wf & 15) == 0 &&
         ((uintptr_t)p.c & 15) == 0 && p.ldc % 8 == 0 && (!p.res || (((uintptr_t)p.res & 15) == 0 && p.ld_res % 8 == 0 && !p.geglu && !p.ln_colsum)) &&
         (!p.rowbias || (p.rows_per_group % 128 == 0 && !p.geglu)) && (!p.ln_inline || scratch) &&
         (ar_env == 1 || p.n >= 960);
}

// ---- the launch plan: WHICH kernel instantiation a set of arguments runs, as a pure function of the arguments (the
// product build has no environment knobs: CA_KNOB compiles to its default; experiment builds, -DCA_EXPERIMENTS, read
// them for same-box A/B runs).  ca_gemm_plan_name / ca_conv3x3_plan_name report it without a launch;
// tests/test_dispatch_plan.py pins every shape of the benchmark workload to its label.  (PlanKind: ca_gemm_core.h)
struct GemmPlan {
  PlanKind kind;
  int bm, bn, nbuf;   // block tile; LDS stages of k_gemm_dma (0: not that kernel)
  int splits;       // K ranges (PK_*_SPLITK), else 1
  unsigned tiles;   // output tiles (x splits = blocks) of the ping-pong kernels
};

// Persistent streaming kernel (ca_gemm_ps.h): can this launch run on it?
inline bool ps_capable(const GemmKParams& p) {
  const int nt = p.taps * p.kc_tiles;
  const bool fits32 = act_out_fit31(p) && p.w_bytes < FIT31;  // (the weights of a convolution or a wide projection can be large: bounded too)
  const bool aligned = ((uintptr_t)p.c & 15) == 0 && (!p.res || ((uintptr_t)p.res & 15) == 0) && p.ldc % 8 == 0 && (!p.res || p.ld_res % 8 == 0);
  return dma_capable(p) && p.n % 320 == 0 && nt >= 2 && p.splits <= 1 && !p.out_f32 && !p.ln_inline && (p.ln_parts <= 2 || p.ln_parts == 4) && fits32 && aligned &&
         (!p.rowbias || p.rows_per_group % 64 == 0) && !(p.geglu && (p.res || p.row_sums)) && p.post == 1.f && p.act == CA_ACT_NONE;
}

// 256 x 320 streaming kernel (ca_gemm_pq.h): bias, row bias, alpha and residual only
inline bool pq_capable(const GemmKParams& p, int mode) {
  // (packed row state of the convolution gather: tap-0 pixel index in 24 signed bits, middle tap always inside the image)
  const bool conv_ok = mode != 1 || (p.pad_lo == 1 && p.ups == 0 && p.hin >= 2 && p.win >= 2 && (int64_t)(p.m / (p.hout * p.wout) + 1) * p.hin * p.win < (1 << 23) &&
                                     (p.hout - 1) * p.stride < p.hin && (p.wout - 1) * p.stride < p.win);
  const bool epi1 = p.geglu || p.ln_colsum || p.ln_stats;  // the LayerNorm / GEGLU epilogue variant: dense, no residual
  return ps_capable(p) && (!p.row_sums || (mode == 0 && !epi1)) && (mode == 1 || p.c2 == 0) && (!p.rowbias || p.rows_per_group % 128 == 0) && conv_ok &&
         (!epi1 || (mode == 0 && !p.res && !p.rowbias && p.ln_parts == 0 && (!p.ln_colsum || p.ln_stats)));
}

// Split-K: does this launch split, into how many K ranges, needing how many bytes of fp32 slabs?  (ranges = 1: no.)  Only grids that
// leave the chip under-filled (8x8 / 16x16 latent levels) and have a long K loop are split; the tile shape used with a split is
// 128x128 (N % 128 == 0).
// Dense GEMMs of the 8x8-latent level (M = 2048: 160 tiles of 128x128 for 256 CUs, each walking its 20..80 K tiles
// alone at one DMA round trip per tile): the same slab schedule as the small convolutions.
// ONE rule; dense and convolution differ in the grid they still split (max_blocks 128x128 tiles), in fp32 outputs (dense: never) and
// in the knob of experiment builds (env: CA_SPLITK_DENSE / CA_SPLITK; 0 = never, S > 0 = S ranges wherever the rule splits).
struct SplitKRule { int env, max_blocks; bool f32_out; };
struct SplitK { int ranges; int64_t bytes; };
inline SplitK splitk_decide(const GemmKParams& p, int mode) {
  static const SplitKRule conv{CA_KNOB("CA_SPLITK", -1), 383, true}, dense{CA_KNOB("CA_SPLITK_DENSE", -1), 192, false};
  const SplitKRule& r = mode == 0 ? dense : conv;
  const SplitK none{1, 0};
  // (k_splitk_reduce and the weight-resident kernel read ln_stats as (mean, rstd): partial sums never take those plans)
  if (!dma_capable(p) || p.ln_inline || p.row_sums || p.ln_parts) return none;
  if (r.env == 0 || p.geglu || (p.out_f32 && !r.f32_out) || p.n % 128 != 0) return none;
  const int nt = p.taps * p.kc_tiles;
  const int64_t blocks = (int64_t)ceil_div_i(p.m, 128) * (p.n / 128);
  // (measured: 2048x1280x5120, 80 K tiles: 55 vs 61 us; 2048x1280x1280, 20 K tiles: 34 vs 19 us -- the fp32 slabs and the
  //  second launch cost more than a short K loop saves, hence the same threshold as the convolutions)
  if (blocks > r.max_blocks || nt < 48) return none;
  int s = r.env > 0 ? r.env : (int)((960 + blocks - 1) / blocks);  // measured best on 160 tiles: 6 (89 vs 181 us unsplit)
  if (s > 8) s = 8;
  while (s > 1 && nt / s < 12) --s;
  return s > 1 ? SplitK{s, (int64_t)s * p.m * p.n * 4} : none;
}
// the launch splits when the caller handed over enough workspace for the slabs
inline void splitk_apply(const SplitK& k, void* workspace, int64_t workspace_bytes, GemmKParams& p) {
  if (k.ranges > 1 && workspace && workspace_bytes >= k.bytes) {
    p.splits = k.ranges;
    p.partial = reinterpret_cast<float*>(workspace);
  }
}

inline GemmPlan plan_gemm(const GemmKParams& p, int mode) {
  const bool dma = dma_capable(p);
  const int nt = p.taps * p.kc_tiles;
  if (dma && p.splits > 1) {
    // dense only: 128x320 ping-pong tiles -- the pipelined K loop needs fewer blocks to cover the DMA latency, so fewer
    // (larger) K ranges and slabs: 2048x1280x5120 in 4 ranges x 64 tiles 45 vs 52 us.  (The 8x8-latent convolution
    // 2048x1280x11520 measured 88 vs 82 us this way and stays on the 128x128 schedule.)
    static const int pp_split_env = CA_KNOB("CA_SPLITK_PP", 1);
    if (pp_split_env && mode == 0 && p.n % 320 == 0) {
      const int tiles320 = ceil_div_i(p.m, 128) * (p.n / 320);
      int s_eff = 256 / tiles320;
      if (s_eff > p.splits) s_eff = p.splits;
      if (s_eff >= 2 && tiles320 * s_eff >= 128 && nt / s_eff >= 12) {
        return GemmPlan{PK_PP2_SPLITK, 128, 320, 0, s_eff, (unsigned)tiles320};
      }
    }
    return GemmPlan{PK_DMA_SPLITK, 128, 128, 1, p.splits, (unsigned)(ceil_div_i(p.m, 128) * (p.n / 128))};
  }
  // Ping-pong kernels (8 waves, one block per CU, two wave groups alternating between an MFMA segment and a
  // fragment-read / DMA-issue segment, counted vmcnt).  Measured: the 128x320 tile divides every
  // channel count of the SD1.5 UNet exactly and wins where the 128x128 grid under-fills the chip (<= 2 rounds of tiles:
  // the 16x16- and 32x32-latent levels, +10..19%); with many rounds the exposed epilogue of a one-block-per-CU kernel
  // (35..45% of a K = 1280 GEMM) loses against 4 co-resident blocks of k_gemm_dma.
  static const int pp_env = CA_KNOB("CA_GEMM_PP", -1);  // (experiment builds: 0 = never, 2 = whenever N % 320 == 0)
  // Persistent streaming kernel (ca_gemm_ps.h): same main loop as the 128 x 320 ping-pong kernel, but no launch / prologue
  // bubble per tile and an epilogue whose stores nothing waits for.  Measured against the kernel each shape had before
  // (tools/ps_check.py --time, same box): 131072x320x1280 149 vs 180 us, 32768x640x640 50 vs 58, 8192x1280x1280 41.6 vs 43.3,
  // 8192x10240x1280 GEGLU 261 vs 270, 2048x10240x1280 GEGLU 67.6 vs 71.0, 32768x5120x640 GEGLU 321 vs 327; behind on long K
  // loops (its flag pieces cost ~5% of the main loop: 32768x640x2560 134 vs 122, 8192x1280x5120 114 vs 109), on wide plain
  // outputs where four co-resident 128x128 blocks already hide their epilogues (32768x1920x640 116 vs 107) and on every
  // convolution (-10..-25%).  Hence: dense, 2..20 K tiles, at least one tile per CU, GEGLU or at most four column tiles.
  // CA_GEMM_PS (experiment builds): 0 = never, 1 = every launch it can take, 2 = the same except the weight-resident kernel's.
  // 256 x 320 streaming kernel (ca_gemm_pq.h): 128 x 80 wave tiles take a quarter of the 128 x 320 kernels' LDS-port and
  // global -> LDS traffic per FLOP; it needs one tile per CU and a long K loop, and has no LayerNorm / GEGLU / row-sum epilogue.
  // Measured against the kernel each shape had before (tools/ps_check.py --time, one process, us): dense 32768x640x2560 106 vs
  // 124, 131072x320x1280 136 vs 157, 32768x640x640 42 vs 52, 32768x1920x640 (folded LayerNorm) 90 vs 102, GEGLU projections
  // 32768x5120x640 260 vs 331, 8192x10240x1280 210 vs 291 (1.02 PFLOP/s), 2048x10240x1280 58 vs 77; convolutions at 32x32
  // latents 640->640 228 vs 290, 1280->640 433 vs 556; behind where the 256-row tiles leave CUs idle (M = 8192 x N = 1280: 128
  // tiles, 154 vs 109; 8192x3840x1280: 384 tiles = 1.5 rounds, 107 vs 95) and on the 64x64-latent convolutions (320->320 296 vs
  // 265).  Step, one box, knobs build: off 66.04 / 65.82, convolutions only 65.84 / 65.62, + GEGLU 64.95 / 64.79, + plain dense
  // 64.37 / 64.34, + folded-LayerNorm projections 63.75 / 63.94.
  // CA_GEMM_PQ (experiment builds): 0 = never, 1 = every launch it can take
  static const int pq_env = CA_KNOB("CA_GEMM_PQ", -1);
  if (pq_env != 0 && pq_capable(p, mode)) {
    const int64_t tiles = (int64_t)ceil_div_i(p.m, 256) * (p.n / 320);
    // (whole rounds of 256 tiles, or many: 8192x3840x1280 = 384 tiles measured 107 vs 95 us on the 128x128 kernel)
    // (convolutions, clean build: 64x64 latents 640->320 468 vs 508, 640->640 908 vs 986, 32x32 1280->1280 820 vs 929; 320->320 at 64x64 -- N = 320, 45 K tiles -- 256 vs 251: not)
    const bool dflt = mode == 1 ? (tiles >= 256 && (p.n >= 640 || nt >= 64)) : (tiles >= 256 && (tiles % 256 == 0 || tiles >= 1024) && nt >= 8 && !wres_eligible(p));
    // (experiment builds, CA_GEMM_PQ: 2 = convolutions + GEGLU projections, 3 = convolutions only, 4 = 2 + plain dense, 5 = everything the rule allows)
    const bool epi1 = p.geglu || p.ln_colsum || p.ln_stats;
    const bool dflt2 = dflt && (mode == 1 || p.geglu), dflt3 = dflt && mode == 1, dflt4 = dflt && (mode == 1 || p.geglu || !epi1);
    if ((pq_env < 0 && dflt) || pq_env == 1 || (pq_env == 2 && dflt2) || (pq_env == 3 && dflt3) || (pq_env == 4 && dflt4) || (pq_env == 5 && dflt)) {
      return GemmPlan{PK_PQ, 256, 320, 0, 1, (unsigned)tiles};
    }
  }
  static const int ps_env = CA_KNOB("CA_GEMM_PS", -1);
  if (ps_env != 0 && ps_capable(p)) {
    const int64_t tiles = (int64_t)ceil_div_i(p.m, 128) * (p.n / 320);
    const bool dflt = mode == 0 && !wres_eligible(p) && nt <= 20 && tiles >= 256 && (p.geglu || p.n <= 1280);
    if ((ps_env < 0 && dflt) || ps_env == 1 || (ps_env == 2 && !(mode == 0 && wres_eligible(p)))) {
      return GemmPlan{PK_PS, 128, 320, 0, 1, (unsigned)tiles};
    }
  }
  if (mode == 0 && dma && ar_eligible(p, p.partial != nullptr)) return GemmPlan{PK_AR, 128, 64, 0, 1, 0u};
  if (mode == 0 && dma && wres_eligible(p)) return GemmPlan{PK_WRES, 256, 160, 0, 1, 0u};
  if (dma && pp_env != 0 && nt >= 2 && p.n % 320 == 0 && p.splits <= 1) {  // 128 x 320 tiles
    const int64_t tiles = (int64_t)ceil_div_i(p.m, 128) * (p.n / 320);
    // (thresholds re-checked inside the step, same box, interleaved: dense 768 / 1024 tiles +0.25 ms, conv 512 +0.7, conv 128 +0.2)
    if (p.row_sums || pp_env == 2 || (pp_env < 0 && tiles >= 128 && nt >= 10 && (tiles <= 256 || (tiles <= 512 && mode == 0)))) {
      return GemmPlan{PK_PP2, 128, 320, 0, 1, (unsigned)tiles};
    }
  }
  // 128x128 tiles unless N is not a multiple of 128 or the grid would leave CUs idle
  // (8x8 / 16x16 latent levels: M = 2048 / 8192 rows -> < 2 blocks per CU with the big tile).
  const bool wide = p.n % 128 == 0 && (int64_t)ceil_div_i(p.m, 128) * ceil_div_i(p.n, 128) >= 512;
  const int64_t blocks = (int64_t)ceil_div_i(p.m, 128) * ceil_div_i(p.n, wide ? 128 : 64);
  // LDS stages: ONE buffer (32 KB, two barriers per tile) lets 4 blocks share a CU, whose MFMA phases
  // cover each other's transfer latency: measured +10..25% over double buffering (2 blocks per CU)
  // and far better than 3-4 stage rings (1 block per CU).  Small grids (< 2 blocks per CU) have no
  // co-resident blocks to overlap with: three stages (round 4; before that the double buffer) -- their K loops are chains of
  // DMA round trips with 8 MFMAs per wave and tile in between; two tiles in flight instead of one: -0.3 ms per step, 62.0 vs
  // 62.3 interleaved three times.  The 128 x 64 tile's ring is 74 KB: two blocks still share a CU.  Four stages (98 KB, one
  // block per CU) lose.  (wide implies blocks >= 512: the 128 x 128 tile only ever runs single-buffered.)
  const int nbuf = blocks >= 512 ? 1 : 3;
  // N = 320 / 960 (every projection and conv of the 64x64-latent level): 128x160 tiles divide N
  // exactly and read the A panel 2 / 6 times instead of 5 / 15 times
  if (dma && !wide && p.n % 160 == 0 && (int64_t)ceil_div_i(p.m, 128) * (p.n / 160) >= 512) return GemmPlan{PK_DMA, 128, 160, 1, 1, 0u};
  return GemmPlan{dma ? PK_DMA : PK_REG, 128, wide ? 128 : 64, dma ? nbuf : 2, 1, 0u};
}

// can the epilogue of this (dense) launch leave per-row sums of its output (ca_gemm_args.row_sums_out)?  Only the 128 x 320
// tile kernels do; the answer is about the launch the arguments get WITHOUT the pointer.
inline int row_sums_parts_of(GemmKParams p) {  // partial sums per row the launch can leave (0: none)
  p.row_sums = nullptr;
  if (p.geglu || p.out_f32) return 0;
  const PlanKind k = plan_gemm(p, 0).kind;
  if (k == PK_PP2 || k == PK_PS) return p.n / 320;          // one (sum, sum of squares) per 320-column tile
  if (k == PK_PQ && !p.ln_colsum && !p.ln_stats) return 4 * (p.n / 320);  // the 256 x 320 kernel: one per 80-column wave quarter
  return 0;
}
inline bool row_sums_capable(const GemmKParams& p) { return row_sums_parts_of(p) > 0; }

inline void plan_label(const GemmPlan& g, char* buf, int len) {
  switch (g.kind) {
    case PK_WRES: snprintf(buf, len, "wres160"); break;
    case PK_AR: snprintf(buf, len, "ar128x64"); break;
    case PK_PP2: snprintf(buf, len, "pp128x320"); break;
    case PK_PS: snprintf(buf, len, "ps128x320"); break;
    case PK_PQ: snprintf(buf, len, "pq256x320"); break;
    case PK_PP2_SPLITK: snprintf(buf, len, "pp128x320_splitk%d", g.splits); break;
    case PK_DMA: snprintf(buf, len, "%dx%d%s", g.bm, g.bn, g.nbuf == 3 ? "_r3" : ""); break;
    case PK_DMA_SPLITK: snprintf(buf, len, "128x128_splitk%d", g.splits); break;
    case PK_REG: snprintf(buf, len, "reg_%dx%d", g.bm, g.bn); break;
  }
}

inline int check_epilogue(const char* who, int n, int geglu, int64_t ldc, int64_t ld_res, const void* res) {
  // N = 4 (conv_out) takes the direct 4-column epilogue; everything wider goes through the LDS-staged
  // epilogue, which moves 8-column (16-byte) chunks: N, ldc and ld_res must then be multiples of 8
  // (N = 12, 20, ... would store 8 values at column N-4: past the row end)
  CA_REQUIRE(n == 4 || (n >= 8 && n % 8 == 0), "%s: N=%d must be 4 or a multiple of 8", who, n);
  CA_REQUIRE(!geglu || n % 8 == 0, "%s: geglu needs N %% 8 == 0", who);
  if (n >= 8) {
    CA_REQUIRE(ldc % (geglu ? 4 : 8) == 0, "%s: ldc=%lld must be a multiple of %d", who, (long long)ldc, geglu ? 4 : 8);
    CA_REQUIRE(!res || ld_res % 8 == 0, "%s: ld_res=%lld must be a multiple of 8", who, (long long)ld_res);
  } else {
    CA_REQUIRE(ldc % 4 == 0, "%s: ldc=%lld misaligned", who, (long long)ldc);
    CA_REQUIRE(!res || ld_res % 4 == 0, "%s: ld_res=%lld misaligned", who, (long long)ld_res);
  }
  return CA_OK;
}

// "What if ...?"  A query entry point may ask about a launch OTHER than the one the arguments describe; it says so here, and the
// arguments are read accordingly -- nobody patches a copy of ca_gemm_args.
struct DenseAsk {
  bool without_row_sums;  // the launch the arguments get WITHOUT row_sums_out (ca_gemm_row_sums_parts: whatever the pointer)
  bool stats_finished;    // ... once the partial LayerNorm sums are finished: ln_parts = 0 (ca_gemm_wants_finished_stats)
};

inline int gemm_fill(const ca_gemm_args* a, GemmKParams& p, const DenseAsk& ask) {
  CA_REQUIRE(a != nullptr, "ca_gemm: null args");
  CA_REQUIRE(a->a && a->w && a->c, "ca_gemm: null operand");
  CA_REQUIRE(a->m > 0 && a->k1 > 0 && a->k2 >= 0, "ca_gemm: bad sizes m=%d k1=%d k2=%d", a->m, a->k1, a->k2);
  CA_REQUIRE(a->k1 % 8 == 0 && a->k2 % 8 == 0, "ca_gemm: k1=%d k2=%d must be multiples of 8", a->k1, a->k2);
  CA_REQUIRE(a->lda % 8 == 0 && (a->k2 == 0 || (a->a2 && a->lda2 % 8 == 0)), "ca_gemm: lda/lda2 misaligned or a2 missing");
  CA_REQUIRE(a->dtype == CA_BF16 || a->dtype == CA_F16, "ca_gemm: dtype %d", a->dtype);
  CA_REQUIRE(!a->rowbias || a->rows_per_group > 0, "ca_gemm: rows_per_group");
  CA_REQUIRE(!a->rowbias || a->ld_rowbias % 4 == 0, "ca_gemm: ld_rowbias misaligned");
  int rc = check_epilogue("ca_gemm", a->n, a->geglu, a->ldc, a->ld_res, a->residual);
  if (rc) return rc;
  p.a = (const u16*)a->a, p.a2 = (const u16*)a->a2, p.w = (const u16*)a->w, p.c = a->c;
  p.bias = a->bias, p.rowbias = a->rowbias, p.ln_stats = a->ln_stats, p.ln_colsum = a->ln_colsum;
  p.row_sums = ask.without_row_sums ? nullptr : a->row_sums_out;
  p.ln_parts = ask.stats_finished ? 0 : a->ln_parts;
  CA_REQUIRE(p.ln_parts >= 0 && p.ln_parts <= 16, "ca_gemm: ln_parts=%d", p.ln_parts);
  CA_REQUIRE(p.ln_parts == 0 || (a->ln_stats && a->ln_colsum && a->ln_eps > 0.f), "ca_gemm: ln_parts needs ln_stats (the partial sums), ln_colsum and ln_eps > 0");
  p.ln_inline = (a->ln_colsum && !a->ln_stats) ? 1 : 0;
  p.ln_eps = a->ln_eps;
  p.wf = (const u16*)a->w_frag;
  CA_REQUIRE(!a->ln_stats || a->ln_colsum, "ca_gemm: ln_stats without ln_colsum");
  CA_REQUIRE(!p.ln_inline || a->ln_eps > 0.f, "ca_gemm: ln_colsum without ln_stats asks for in-kernel statistics and needs ln_eps > 0");
  CA_REQUIRE(!a->ln_colsum || (a->n >= 8 && a->k2 == 0), "ca_gemm: the folded LayerNorm needs N >= 8 and a single A source");
  p.res = (const u16*)a->residual;
  p.lda = a->lda, p.lda2 = a->lda2, p.ldc = a->ldc, p.ld_res = a->ld_res, p.ld_rowbias = a->ld_rowbias;
  p.a_bytes = desc_bytes((int64_t)(a->m - 1) * a->lda + a->k1);
  p.a2_bytes = a->k2 ? desc_bytes((int64_t)(a->m - 1) * a->lda2 + a->k2) : 0u;
  p.w_bytes = desc_bytes((int64_t)a->n * (a->k1 + a->k2));
  p.m = a->m, p.n = a->n, p.c1 = a->k1, p.c2 = a->k2;
  p.taps = 1;
  p.kc_tiles = ceil_div_i(a->k1 + a->k2, BK);
  p.rows_per_group = a->rows_per_group > 0 ? a->rows_per_group : 1;
  p.alpha = a->alpha, p.post = a->post_scale, p.act = a->act, p.geglu = a->geglu, p.out_f32 = a->out_f32;
  p.splits = 1;
  return CA_OK;
}

// The resolved view of a dense launch: gemm_fill + the split-K decision + the statistics scratch = everything the plan depends on,
// the plan, and the workspace the launch can use.  ca_gemm and its query entry points are a few lines over it.
struct DenseLaunch {
  GemmKParams p;
  GemmPlan plan;
  int64_t workspace;  // bytes wanted, whatever was handed over: split-K slabs, or (mean, rstd) per row for k_gemm_ar; 0: none
};
inline int gemm_resolve(const ca_gemm_args* a, DenseLaunch& d, const DenseAsk& ask = DenseAsk{}) {
  d = DenseLaunch{};
  GemmKParams& p = d.p;
  int rc = gemm_fill(a, p, ask);
  if (rc) return rc;
  const SplitK k = splitk_decide(p, 0);
  splitk_apply(k, a->workspace, a->workspace_bytes, p);
  d.workspace = k.bytes;
  if (p.ln_inline && p.wf) {  // in-kernel LayerNorm statistics of the activation-resident kernel: (mean, rstd) scratch of k_gemm_ar
    if (ar_eligible(p, true)) d.workspace = (int64_t)p.m * 8;  // "a scratch is there": would the launch take that kernel?
    if (a->workspace && a->workspace_bytes >= (int64_t)p.m * 8) p.partial = reinterpret_cast<float*>(a->workspace);
  }
  d.plan = plan_gemm(p, 0);
  return CA_OK;
}

// gemm_resolve + what the launch itself insists on
inline int gemm_prepare(const ca_gemm_args* a, DenseLaunch& d) {
  int rc = gemm_resolve(a, d);
  if (rc) return rc;
  CA_REQUIRE(!d.p.row_sums || row_sums_capable(d.p), "ca_gemm: row_sums_out is not available for this launch: ask ca_gemm_row_sums_parts() first");
  CA_REQUIRE(!d.p.ln_inline || wres_eligible(d.p), "ca_gemm: in-kernel LayerNorm statistics (ln_stats NULL) are not available for this launch: "
             "ask ca_gemm_ln_inline_supported() first and pass ln_stats otherwise");
  return CA_OK;
}

// Geometry of a 3x3 convolution: logical input (after the nearest-x2 upsample), total padding per axis, output size and rows.
// (stride and upsample checked by the caller.)
struct ConvGeom { int hl, wl, hout, wout; int64_t m; };
inline ConvGeom conv_geom(const ca_conv_args* a) {
  ConvGeom g;
  g.hl = a->hin << a->upsample, g.wl = a->win << a->upsample;
  const int pad = a->pad_asym ? 1 : 2;  // total padding per axis: 1+1, or 0 before / 1 after
  g.hout = (g.hl + pad - 3) / a->stride + 1;
  g.wout = (g.wl + pad - 3) / a->stride + 1;
  g.m = (int64_t)a->images * g.hout * g.wout;
  return g;
}
inline int64_t wino_tiles(const ca_conv_args* a, const ConvGeom& g) { return (int64_t)a->images * (g.hl / 2) * (g.wl / 2); }  // 2x2 output tiles

// The Winograd route of ca_conv3x3 (ca_conv_wino.h): 0 = not taken, else the workspace it needs (V [16][T][cin] + M [16][T][cout]).
inline int64_t wino_workspace_bytes(const ca_conv_args* a) {
  if (!a || !a->w_wino || (a->dtype != CA_F16 && a->dtype != CA_BF16) || a->stride != 1 || a->pad_asym || a->out_f32) return 0;
  if (a->upsample != 0 && a->upsample != 1) return 0;
  if (a->x_is_wino_v && (a->cin2 != 0 || a->upsample)) return 0;
  const ConvGeom g = conv_geom(a);  // logical input = output size
  if (a->images <= 0 || g.hl < 2 || g.wl < 2 || (g.hl & 1) || (g.wl & 1)) return 0;
  const int kc = a->cin1 + a->cin2;
  static const int min_cin = CA_KNOB("CA_WINO_MIN_CIN", 1280);  // (experiments: where the route stops paying)
  if (kc < 640 || kc % BK != 0 || a->cin1 % 8 != 0 || a->cin2 % 8 != 0 || a->cout % 320 != 0) return 0;
  const int64_t tiles = wino_tiles(a, g);
  // input channels: >= 1280 everywhere in the window; 640 .. 1279 only at <= 4096 tiles, where the direct form is short of tiles
  // (32 x 16x16 640->1280: 100 vs 160 us; at 8192 tiles 640->640 254 vs 233-252, 960->640 318 vs 331: no / marginal gain)
  if (kc < min_cin && !(min_cin == 1280 && tiles <= 4096)) return 0;
  // whole 256-row tiles per transformed GEMM.  Measured (tools/wino_check.py, us, Winograd vs direct): 32 x 16x16 1280->1280 170 vs 276,
  // 2560->1280 285 vs 529, 32 x 8x8 1280->1280 66 vs 87, 32 x 32x32 1920->640 510 vs 584, 1280->1280 634 vs 800; with 640 input channels
  // the sixteen K = 640 GEMMs are epilogue-bound and the 4 x larger V / M tensors cost more than the saved MFMAs (no gain): >= 1280 only
  static const int max_tiles = CA_KNOB("CA_WINO_MAX_TILES", 16384);
  if (tiles % 256 != 0 || tiles > max_tiles) return 0;
  if (16 * tiles * (int64_t)(kc > a->cout ? kc : a->cout) * 2 >= 0x7FFFFF00ll) return 0;  // 32-bit byte offsets in the GEMM
  return 16 * tiles * (int64_t)((a->x_is_wino_v ? 0 : kc) + a->cout) * 2;  // V (unless the caller hands it over as x) + M
}

inline bool wino_taken(const ca_conv_args* a) {
  const int64_t wb = wino_workspace_bytes(a);
  return wb > 0 && a->workspace && a->workspace_bytes >= wb && (((uintptr_t)a->workspace | (uintptr_t)a->w_wino) & 15) == 0;
}

// the sizes the plan of a direct convolution depends on: all of GemmKParams but the pointers and the epilogue
inline void conv_fill_sizes(const ca_conv_args* a, const ConvGeom& g, GemmKParams& p) {
  p.a_bytes = desc_bytes((int64_t)a->images * a->hin * a->win * a->cin1);
  p.a2_bytes = a->cin2 ? desc_bytes((int64_t)a->images * a->hin * a->win * a->cin2) : 0u;
  p.w_bytes = desc_bytes((int64_t)a->cout * 9 * (a->cin1 + a->cin2));
  p.m = (int)g.m, p.n = a->cout, p.c1 = a->cin1, p.c2 = a->cin2;
  p.taps = 9;
  static const int tap_inner_env = CA_KNOB("CA_CONV_TAP_INNER", 1);
  p.tap_inner = tap_inner_env;  // (0: taps outermost, the round-1 order -- A/B experiments)
  p.kc_tiles = ceil_div_i(a->cin1 + a->cin2, BK);
  p.hin = a->hin, p.win = a->win, p.hout = g.hout, p.wout = g.wout;
  p.stride = a->stride, p.ups = a->upsample, p.pad_lo = a->pad_asym ? 0 : 1;
  p.geglu = 0, p.out_f32 = a->out_f32;
  p.splits = 1;
}

inline int conv_prepare(const ca_conv_args* a, GemmKParams& p) {
  CA_REQUIRE(a != nullptr, "ca_conv3x3: null args");
  CA_REQUIRE(a->x && a->w && a->y, "ca_conv3x3: null operand");
  CA_REQUIRE(a->images > 0 && a->hin > 0 && a->win > 0, "ca_conv3x3: bad geometry");
  CA_REQUIRE(a->cin1 > 0 && a->cin1 % 8 == 0 && a->cin2 >= 0 && a->cin2 % 8 == 0,
             "ca_conv3x3: cin1=%d cin2=%d must be multiples of 8", a->cin1, a->cin2);
  CA_REQUIRE(a->cin2 == 0 || a->x2, "ca_conv3x3: x2 missing");
  CA_REQUIRE(a->stride == 1 || a->stride == 2, "ca_conv3x3: stride %d", a->stride);
  CA_REQUIRE(a->upsample == 0 || a->upsample == 1, "ca_conv3x3: upsample %d", a->upsample);
  CA_REQUIRE(a->dtype == CA_BF16 || a->dtype == CA_F16, "ca_conv3x3: dtype %d", a->dtype);
  CA_REQUIRE(!a->rowbias || a->rows_per_group > 0, "ca_conv3x3: rows_per_group");
  int rc = check_epilogue("ca_conv3x3", a->cout, 0, a->cout, a->ld_res, a->residual);
  if (rc) return rc;
  CA_REQUIRE(a->pad_asym == 0 || a->pad_asym == 1, "ca_conv3x3: pad_asym %d", a->pad_asym);
  const ConvGeom g = conv_geom(a);
  CA_REQUIRE(g.m < (1ll << 31), "ca_conv3x3: too many output pixels");
  conv_fill_sizes(a, g, p);
  p.a = (const u16*)a->x, p.a2 = (const u16*)a->x2, p.w = (const u16*)a->w, p.c = a->y;
  p.bias = a->bias, p.rowbias = a->rowbias, p.res = (const u16*)a->residual;
  p.ldc = a->cout, p.ld_res = a->ld_res, p.ld_rowbias = a->ld_rowbias;
  p.rows_per_group = a->rows_per_group > 0 ? a->rows_per_group : 1;
  p.alpha = a->alpha, p.post = a->post_scale, p.act = a->act;
  splitk_apply(splitk_decide(p, 1), a->workspace, a->workspace_bytes, p);
  return CA_OK;
}

// what ca_conv3x3 can use: the Winograd route's V and M tensors where that route takes the arguments, else the split-K slabs.  (Asked
// before the operands exist: sizes only, no pointer is looked at.)
inline int64_t conv_workspace_bytes(const ca_conv_args* a) {
  if (!a || a->images <= 0 || a->hin <= 0 || a->win <= 0 || (a->stride != 1 && a->stride != 2)) return 0;
  const int64_t wb = wino_workspace_bytes(a);
  if (wb > 0) return wb;
  const ConvGeom g = conv_geom(a);
  if (g.m >= (1ll << 31)) return 0;
  GemmKParams p{};
  conv_fill_sizes(a, g, p);
  return splitk_decide(p, 1).bytes;
}

// ---- nearest-x2 upsampling 3x3 convolution as four 2x2 phase convolutions in one launch (k_gemm_pq MODE 2, ca_gemm_pq.h).
// An output pixel of parity (py, px) reads a 2x2 neighbourhood of the SOURCE image; the nine taps that land on the same source
// pixel are summed at pack time (a->w = w_phase [4][cout][2][2][cin]): 4/9 of the multiply-adds of ca_conv3x3(upsample = 1).
// up2_capable: what the kernel implements; up2_pays: where the form is taken by default (ca_conv_up2_phase_supported = both).
inline bool up2_capable(const ca_conv_args* a, GemmKParams& p) {
  if (!a || !a->x || !a->w || !a->y || a->x2 || a->cin2 != 0 || a->images <= 0 || a->hin <= 0 || a->win <= 0) return false;
  if (a->upsample != 1 || a->stride != 1 || a->pad_asym || a->out_f32 || a->x_is_wino_v || a->rowbias) return false;
  if ((a->dtype != CA_F16 && a->dtype != CA_BF16) || a->act != CA_ACT_NONE || a->post_scale != 1.f) return false;
  if (a->cin1 <= 0 || a->cin1 % BK != 0 || a->cout <= 0 || a->cout % 320 != 0) return false;
  if ((((uintptr_t)a->x | (uintptr_t)a->w | (uintptr_t)a->y | (uintptr_t)a->residual) & 15) != 0) return false;
  if (a->residual && (a->ld_res < a->cout || a->ld_res % 8 != 0)) return false;
  const int64_t rows = (int64_t)a->images * a->hin * a->win;  // per phase: the source pixels
  if (rows + a->win + 2 >= (1 << 23)) return false;           // packed row state of the gather: 24 signed bits of pixel index
  p = GemmKParams{};
  p.a = (const u16*)a->x;
  p.w = (const u16*)a->w;
  p.c = a->y;
  p.bias = a->bias;
  p.res = (const u16*)a->residual;
  p.ldc = a->cout;
  p.ld_res = a->ld_res;
  p.a_bytes = desc_bytes(rows * a->cin1);
  p.w_bytes = desc_bytes((int64_t)4 * a->cout * 4 * a->cin1);
  p.n = a->cout;
  p.c1 = a->cin1;
  p.taps = 4;
  p.tap_inner = 1;
  p.kc_tiles = a->cin1 / BK;
  p.hin = a->hin, p.win = a->win, p.hout = 2 * a->hin, p.wout = 2 * a->win;
  p.stride = 1, p.ups = 1, p.pad_lo = 1;
  p.rows_per_group = 1;
  p.alpha = a->alpha, p.post = 1.f;
  p.splits = 1;
  p.up2_rows = (int)rows;
  p.up2_tiles = ceil_div_i((int)rows, 256);
  p.m = 4 * p.up2_tiles * 256;
  p.up2_mag_w = a->win == 1 ? 0xFFFFFFFFu : (unsigned)((1ull << 32) / (unsigned)a->win);
  p.up2_mag_h = a->hin == 1 ? 0xFFFFFFFFu : (unsigned)((1ull << 32) / (unsigned)a->hin);
  p.w_group_stride = (unsigned)((int64_t)a->cout * 4 * a->cin1 * 2);
  return dma_sizes_ok(p) && act_out_fit31(p) && p.w_bytes < FIT31;
}
inline unsigned up2_tiles_total(const GemmKParams& p) { return (unsigned)(4 * p.up2_tiles * (p.n / 320)); }
// Whole rounds of 256 tiles, or many (the rule of the 256 x 320 kernel's dense launches): 32 x 32x32 640->640 is 1024 tiles,
// 32 x 16x16 1280->1280 is 512; 32 x 8x8 1280->1280 is 128 tiles -- half the chip -- and stays on the Winograd form.
inline bool up2_pays(const GemmKParams& p) {
  const unsigned tiles = up2_tiles_total(p);
  return tiles >= 256 && (tiles % 256 == 0 || tiles >= 1024);
}

}  // namespace ca_gemm_detail
