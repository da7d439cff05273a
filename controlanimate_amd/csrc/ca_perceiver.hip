// ca_perceiver_attn: the attention of the IP-Adapter Plus Resampler (controlanimate_amd/resampler.py).  At most 16 latent queries
// per (batch, head) attend to the image features AND to the latents themselves under ONE softmax; the two key/value sources live in
// different buffers (the image side in a column slice of the all-layers K|V GEMM, the latent side in the layer's q|k|v GEMM), which
// ca_attention cannot express: its `accumulate` adds two separately normalised attentions.
//
// One block of NW waves per (batch, head), head_dim = 64.  S^T = K Q^T as 16x16x16 MFMAs per 16-key tile of the joined key list
// (n_x rows of X, then n_l rows of L): a lane (g = lane >> 4, i = lane & 15) holds the logits of keys 4 g .. 4 g + 3 for query i,
// which is already the B fragment of O^T = V^T P^T.  The Q fragments (rows >= nq zero) are loaded once; wave w takes tiles
// w, w + NW, ... and keeps an online-softmax (m, l, O^T) of its own; the partials meet in LDS and are merged in wave order by every
// thread in the same way: no atomics, the result is bit-reproducible.  A wave without a tile leaves (-inf, 0, 0), which the merge
// weighs with exactly 0.  The launch is latency-bound (24 blocks of ~150 MFMAs at the product shape): nothing here is tuned.
#include "ca_common.h"
#include <math.h>

namespace {

constexpr int kPercWaves = 4;
constexpr int kPercD = 64;

struct PercParams {
  const u16* q; const u16* x; const u16* l; u16* o;
  int64_t q_row, q_batch, x_row, x_batch, x_v_off, l_row, l_batch, l_v_off, o_row, o_batch;
  int heads, nq, n_x, n_l;
  float scale_log2;
};

template <int DT>
__global__ __launch_bounds__(kPercWaves * 64) void k_perceiver_attn(PercParams p) {
  constexpr int NW = kPercWaves, D = kPercD;
  __shared__ float s_m[NW][16], s_l[NW][16];
  __shared__ float s_o[NW][16][D + 4];  // (+4: the four g rows of a wave's store land in different banks)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, i15 = lane & 15;
  const int b = (int)blockIdx.x / p.heads, h = (int)blockIdx.x - b * p.heads;
  const int nkeys = p.n_x + p.n_l;
  const int ntiles = (nkeys + 15) >> 4;

  const u16* xb = p.x + (int64_t)b * p.x_batch + (int64_t)h * D;
  const u16* lb = p.l + (int64_t)b * p.l_batch + (int64_t)h * D;
  // row `key` of the joined list: (pointer to its 64 K elements of this head, offset of its V elements)
  auto key_row = [&](int key, int64_t& voff) __attribute__((always_inline)) -> const u16* {
    if (key < p.n_x) {
      voff = p.x_v_off;
      return xb + (int64_t)key * p.x_row;
    }
    voff = p.l_v_off;
    return lb + (int64_t)(key - p.n_x) * p.l_row;
  };

  // Q fragments: query i15, 16-deep chunk c holds d = 32 (c >> 1) + 8 g + 4 (c & 1) .. + 3 -- K is read in the same order, and a
  // contraction does not care in which order it meets its terms.  (One 16-byte load feeds two chunks.)
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  u32x2 qf[4];
  {
    const u16* qp = p.q + (int64_t)b * p.q_batch + (int64_t)h * D + (int64_t)i15 * p.q_row;
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2) {
      const u32x4 v = i15 < p.nq ? ld16(qp + c2 * 32 + g * 8) : zero4;
      qf[2 * c2] = (u32x2){v[0], v[1]};
      qf[2 * c2 + 1] = (u32x2){v[2], v[3]};
    }
  }

  float m = -INFINITY, l = 0.f;  // (l: this lane's share, keys 4 g + r of every tile; summed over g at the end)
  f32x4 o[4];                    // O^T: d_v = 16 j + 4 g + r of query i15
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int t = wave; t < ntiles; t += NW) {  // (wave-uniform)
    // K fragment: key t * 16 + i15
    u32x2 kf[4];
    {
      const int key = t * 16 + i15;
      int64_t voff;
      const u16* kp = key_row(key < nkeys ? key : 0, voff);
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2) {
        const u32x4 v = key < nkeys ? ld16(kp + c2 * 32 + g * 8) : zero4;
        kf[2 * c2] = (u32x2){v[0], v[1]};
        kf[2 * c2 + 1] = (u32x2){v[2], v[3]};
      }
    }
    // V^T fragments: row d_v = 16 j + i15, k slot e = key t * 16 + 4 g + e (16 lanes read 32 contiguous bytes of one row)
    u32x2 vf[4];
    {
      unsigned short ve[4][4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int key = t * 16 + 4 * g + e;
        int64_t voff;
        const u16* kp = key_row(key < nkeys ? key : 0, voff);
#pragma unroll
        for (int j = 0; j < 4; ++j) ve[j][e] = key < nkeys ? kp[voff + 16 * j + i15] : (u16)0;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        vf[j] = (u32x2){(unsigned)ve[j][0] | ((unsigned)ve[j][1] << 16), (unsigned)ve[j][2] | ((unsigned)ve[j][3] << 16)};
    }

    f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c) s = Elem<DT>::mfma16(kf[c], qf[c], s);
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = t * 16 + 4 * g + r < nkeys ? s[r] * p.scale_log2 : -INFINITY;  // one fp32 scale on the logits
    // every tile t < ntiles holds at least one key, so m_new is finite (for finite inputs) and exp2(m - m_new) is 0 on the first tile
    const float m_new = vmax2(m, rowgroup_max(vmax2(vmax2(s[0], s[1]), vmax2(s[2], s[3]))));
    const float alpha = __builtin_amdgcn_exp2f(m - m_new);
    m = m_new;
    float pr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) pr[r] = __builtin_amdgcn_exp2f(s[r] - m_new);
    l = l * alpha + ((pr[0] + pr[1]) + (pr[2] + pr[3]));
    const u32x2 pf = {pack2<DT>(pr[0], pr[1]), pack2<DT>(pr[2], pr[3])};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) o[j][r] *= alpha;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = Elem<DT>::mfma16(vf[j], pf, o[j]);
  }

  l = rowgroup_sum(l);
  if (g == 0) {
    s_m[wave][i15] = m;
    s_l[wave][i15] = l;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) s_o[wave][i15][16 * j + 4 * g + r] = o[j][r];
  __syncthreads();

  // merge: thread -> (query qi, four d_v); wave 0 always has tile 0, so mx is finite
  const int qi = tid >> 4, d0 = (tid & 15) * 4;
  float mx = s_m[0][qi];
#pragma unroll
  for (int w = 1; w < NW; ++w) mx = vmax2(mx, s_m[w][qi]);
  float lsum = 0.f, acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const float mw = s_m[w][qi];
    const float f = mw == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mw - mx);  // (a wave without a tile: weight 0, never inf - inf)
    lsum += s_l[w][qi] * f;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] += s_o[w][qi][d0 + r] * f;
  }
  if (qi < p.nq) {
    const float inv = 1.0f / lsum;
    u16* op = p.o + (int64_t)b * p.o_batch + (int64_t)qi * p.o_row + (int64_t)h * D + d0;
    *reinterpret_cast<u32x2*>(op) = (u32x2){pack2<DT>(acc[0] * inv, acc[1] * inv), pack2<DT>(acc[2] * inv, acc[3] * inv)};
  }
}

}  // namespace

extern "C" int ca_perceiver_attn(const ca_perceiver_attn_args* a, void* stream) {
  CA_REQUIRE(a != nullptr, "ca_perceiver_attn: null args");
  CA_REQUIRE(a->q && a->x && a->l && a->o, "ca_perceiver_attn: null operand");
  CA_REQUIRE(a->dtype == CA_BF16 || a->dtype == CA_F16, "ca_perceiver_attn: dtype %d", a->dtype);
  CA_REQUIRE(a->head_dim == kPercD, "ca_perceiver_attn: head_dim=%d, only 64 is implemented", a->head_dim);
  CA_REQUIRE(a->nq >= 1 && a->nq <= 16, "ca_perceiver_attn: nq=%d must be 1..16", a->nq);
  CA_REQUIRE(a->n_x >= 1 && a->n_l >= 1, "ca_perceiver_attn: n_x=%d n_l=%d must both be >= 1", a->n_x, a->n_l);
  CA_REQUIRE((int64_t)a->n_x + a->n_l < (1ll << 30), "ca_perceiver_attn: too many keys");
  CA_REQUIRE(a->batches >= 1 && a->heads >= 1 && (int64_t)a->batches * a->heads < (1ll << 31), "ca_perceiver_attn: bad batches=%d heads=%d",
             a->batches, a->heads);
  CA_REQUIRE(((uintptr_t)a->q | (uintptr_t)a->x | (uintptr_t)a->l | (uintptr_t)a->o) % 16 == 0, "ca_perceiver_attn: pointers must be 16-byte aligned");
  CA_REQUIRE(a->q_row % 8 == 0 && a->x_row % 8 == 0 && a->l_row % 8 == 0 && a->o_row % 8 == 0 && a->q_batch % 8 == 0 && a->x_batch % 8 == 0 &&
                 a->l_batch % 8 == 0 && a->o_batch % 8 == 0,
             "ca_perceiver_attn: row and batch strides must be multiples of 8 elements");
  CA_REQUIRE(a->q_row >= 0 && a->x_row >= 0 && a->l_row >= 0 && a->o_row >= (int64_t)a->heads * kPercD && a->q_batch >= 0 && a->x_batch >= 0 &&
                 a->l_batch >= 0 && a->o_batch >= 0,
             "ca_perceiver_attn: negative stride, or output rows that overlap");
  PercParams p;
  p.q = (const u16*)a->q; p.x = (const u16*)a->x; p.l = (const u16*)a->l; p.o = (u16*)a->o;
  p.q_row = a->q_row; p.q_batch = a->q_batch;
  p.x_row = a->x_row; p.x_batch = a->x_batch; p.x_v_off = a->x_v_off;
  p.l_row = a->l_row; p.l_batch = a->l_batch; p.l_v_off = a->l_v_off;
  p.o_row = a->o_row; p.o_batch = a->o_batch;
  p.heads = a->heads; p.nq = a->nq; p.n_x = a->n_x; p.n_l = a->n_l;
  p.scale_log2 = a->scale * 1.4426950408889634f;
  const dim3 grid((unsigned)(a->batches * a->heads)), block(kPercWaves * 64);
  if (a->dtype == CA_BF16) hipLaunchKernelGGL((k_perceiver_attn<CA_BF16>), grid, block, 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL((k_perceiver_attn<CA_F16>), grid, block, 0, (hipStream_t)stream, p);
  CA_CHECK_LAUNCH("ca_perceiver_attn");
  return CA_OK;
}
