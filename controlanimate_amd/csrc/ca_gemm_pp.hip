// Ping-pong and streaming GEMM kernels (128 x 320, 256 x 320, weight-resident): separate translation unit (compile time).
#include "ca_gemm_core.h"
#include <type_traits>

namespace {
using namespace ca_gemm_detail;
#include "ca_gemm_pp2.h"
#include "ca_gemm_wres.h"
#include "ca_gemm_ps.h"
#include "ca_gemm_pq.h"

int cu_count() {
  static int n = 0;
  if (!n) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n = prop.multiProcessorCount;
    if (n <= 0) n = 256;
  }
  return n;
}

// Timing experiment (--experiments --stamps builds, CA_PP_DBG=9): `launch(q)` runs the kernel with q.partial pointing at a
// stamp buffer; block 0's shader-clock stamps (the `stamp` lambdas of ca_gemm_ps.h / ca_gemm_pq.h) of the first such launch
// are printed to stderr as tag:delta_cycles, with a separator after tag `sep` and a new line after tag `eol`.
template <class Launch>
int launch_stamped(const GemmKParams& p, hipStream_t st, const char* label, unsigned sep, unsigned eol, Launch launch) {
  static unsigned long long* dbuf = nullptr;
  if (!dbuf && hipMalloc(&dbuf, 4096 * 8) != hipSuccess) return CA_ERR_LAUNCH;
  (void)hipMemsetAsync(dbuf, 0, 4096 * 8, st);
  GemmKParams q = p;
  q.partial = reinterpret_cast<float*>(dbuf);
  launch(q);
  (void)hipStreamSynchronize(st);
  static int printed = 0;
  if (printed++ < 1) {
    static unsigned long long host[4096];
    (void)hipMemcpy(host, dbuf, sizeof(host), hipMemcpyDeviceToHost);
    for (int g = 0; g < 2; ++g) {
      fprintf(stderr, "[%s stamps group %d, %dx%dx%d] tag:delta_cycles ...\n", label, g, p.m, p.n, (p.c1 + p.c2) * p.taps);
      unsigned long long prev = host[g * 2048];
      for (int i = 0; i < 1000 && host[g * 2048 + 2 * i]; ++i) {
        fprintf(stderr, "%llu:%llu ", host[g * 2048 + 2 * i + 1], host[g * 2048 + 2 * i] - prev);
        prev = host[g * 2048 + 2 * i];
        if (host[g * 2048 + 2 * i + 1] == sep) fprintf(stderr, "| ");
        if (host[g * 2048 + 2 * i + 1] == eol) fprintf(stderr, "\n");
      }
      fprintf(stderr, "\n");
    }
  }
  return CA_OK;
}

template <int DT, int MODE>
int launch_pp(const GemmKParams& p, PlanKind kind, unsigned tiles, hipStream_t st) {
  // descriptor sizes of the output and the residual: the extents the capability predicates bounded (ca_gemm_core.h)
  const unsigned c_bytes = (unsigned)c_extent_bytes(p), res_bytes = (unsigned)res_extent_bytes(p);
  const unsigned grid = tiles < (unsigned)cu_count() ? tiles : (unsigned)cu_count();  // the persistent kernels: one block per CU
  switch (kind) {
    case PK_PQ: {  // persistent streaming kernel, 256 x 320 tiles (ca_gemm_pq.h)
      auto launch = [&](const GemmKParams& q) {
        // (the LayerNorm / GEGLU variant takes no residual -- pq_capable -- so res_bytes is 0 there; the others never see GEGLU)
        if (MODE == 0 && (q.geglu || q.ln_colsum || q.ln_stats)) hipLaunchKernelGGL((k_gemm_pq<DT, 0, 1>), dim3(grid), dim3(512), 0, st, q, (int)tiles, c_bytes, 0u);
        else if (MODE == 0 && q.row_sums) hipLaunchKernelGGL((k_gemm_pq<DT, 0, 2>), dim3(grid), dim3(512), 0, st, q, (int)tiles, c_bytes, res_bytes);
        else hipLaunchKernelGGL((k_gemm_pq<DT, MODE>), dim3(grid), dim3(512), 0, st, q, (int)tiles, c_bytes, res_bytes);
      };
#ifdef CA_STAMPS
      if (p.dbg == 9) return launch_stamped(p, st, "pq", 8, 10, launch);
#endif
      launch(p);
      return CA_OK;
    }
    case PK_PS: {  // persistent streaming kernel, 128 x 320 tiles (ca_gemm_ps.h)
      auto launch = [&](const GemmKParams& q) { hipLaunchKernelGGL((k_gemm_ps<DT, MODE>), dim3(grid), dim3(512), 0, st, q, (int)tiles, c_bytes, res_bytes); };
#ifdef CA_STAMPS
      if (p.dbg == 9) return launch_stamped(p, st, "ps", 8, 10, launch);
#endif
      launch(p);
      return CA_OK;
    }
    case PK_WRES: {  // weight-resident streaming kernel (K = 320, dense only)
      if (MODE != 0) return CA_ERR_LAUNCH;
      const int panels = p.n / 160;
      const int chunks = (p.m + 255) / 256;
      int per = (cu_count() / 8) / panels;  // slab lanes per XCD
      if (per * 8 > chunks) per = chunks / 8;
      if (per < 1) per = 1;
      const unsigned rb_bytes = p.rowbias ? (unsigned)(((int64_t)((p.m - 1) / p.rows_per_group) * p.ld_rowbias + p.n) * 4) : 16u;
      hipLaunchKernelGGL((k_gemm_wres<DT>), dim3(8 * per * panels), dim3(512), 0, st, p, panels, 8 * per, chunks, rb_bytes, c_bytes, res_bytes);
      return CA_OK;
    }
    case PK_PP2:  // 128 x 320 ping-pong tiles, one block per tile (and per K range with split-K)
      hipLaunchKernelGGL((k_gemm_pp2<DT, MODE>), dim3(tiles), dim3(512), 0, st, p);
      return CA_OK;
    default: return CA_ERR_LAUNCH;
  }
}

// mode 2, the four-phase upsampling convolution (ca_conv_up2_phase): the 256 x 320 kernel only
template <int DT>
int launch_up2(const GemmKParams& p, PlanKind kind, unsigned tiles, hipStream_t st) {
  if (kind != PK_PQ) return CA_ERR_LAUNCH;
  const unsigned grid = tiles < (unsigned)cu_count() ? tiles : (unsigned)cu_count();
  hipLaunchKernelGGL((k_gemm_pq<DT, 2>), dim3(grid), dim3(512), 0, st, p, (int)tiles, (unsigned)c_extent_bytes(p), (unsigned)res_extent_bytes(p));
  return CA_OK;
}
}  // namespace

int ca_launch_gemm_pp(const ca_gemm_detail::GemmKParams& p0, int dtype, int mode, ca_gemm_detail::PlanKind kind, unsigned tiles, hipStream_t st) {
  static const int dbg = CA_KNOB("CA_PP_DBG", 0);  // (timing experiments: 1 = no epilogue, 2 = no main loop)
  ca_gemm_detail::GemmKParams p = p0;
  p.dbg = dbg;
  if (mode == 2) CA_DISPATCH_DT(dtype, return launch_up2<DT>(p, kind, tiles, st));
  CA_DISPATCH_DT(dtype, return mode ? launch_pp<DT, 1>(p, kind, tiles, st) : launch_pp<DT, 0>(p, kind, tiles, st));
}
