/*
 * controlanimate_hip.h -- C ABI of the MI355X (gfx950) denoising-loop kernels.
 *
 * The reference (intellerce/controlanimate) has NO native/FFI boundary: its hot path is
 * Python calling torch/cuDNN/cuBLAS/xformers ops.  This header is therefore the boundary
 * a maintainer would bind UNDER the reference's Python modules (see INTEGRATION.md for the
 * ctypes stub).  Each entry point names the reference call site(s) it replaces.
 *
 * Conventions:
 *   - plain C, extern "C"; plain pointers and sizes; no torch / C++ types.
 *   - all pointers are DEVICE pointers on the current HIP device; the caller owns every
 *     buffer (kernels never allocate or free; scratch is passed in).
 *   - every call is asynchronous on the `stream` argument (a hipStream_t passed as void*).
 *   - returns CA_OK (0) or a negative CA_ERR_* code; never throws, never exits.
 *     ca_last_error() returns a thread-local message for the last failing call.
 *   - activations are channels-last: [images, H, W, C] (images = b*f in (b f) order),
 *     element type `dtype` = CA_BF16 or CA_F16; accumulation is always fp32.
 *   - "rows" means pixels/tokens: rows = images*H*W.
 */
#ifndef CONTROLANIMATE_HIP_H
#define CONTROLANIMATE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CA_ABI_VERSION 16

/* element types */
#define CA_BF16 0
#define CA_F16 1
#define CA_F32 2 /* control tensor of ca_canny_emit / ca_hed_fuse only (ABI v16) */

/* error codes */
#define CA_OK 0
#define CA_ERR_INVALID_ARG (-1)
#define CA_ERR_UNSUPPORTED (-2)
#define CA_ERR_LAUNCH (-3)

/* epilogue activations */
#define CA_ACT_NONE 0
#define CA_ACT_SILU 1
#define CA_ACT_QUICK_GELU 2 /* x * sigmoid(1.702 x): CLIP ViT-L text/vision MLPs */
#define CA_ACT_GELU 3       /* erf GELU: CLIP ViT-H vision MLP (IP-Adapter image encoder) */
#define CA_ACT_RELU 4       /* max(x, 0): the VGG stack of the HED annotator (added to ABI v16) */
#define CA_ACT_RELU6 5      /* min(max(x, 0), 6): the MobileNetV2 backbone of the M-LSD annotator (added to ABI v16) */
#define CA_ACT_LEAKY02 6    /* x > 0 ? x : 0.2 x: the U-Net and the SFT branches of the GFPGAN face restorer (added to ABI v16) */
#define CA_ACT_LEAKY001 7   /* x > 0 ? x : 0.01 x: nn.LeakyReLU() of the NormalBae decoder (added to ABI v16) */

int ca_abi_version(void);
const char* ca_last_error(void);

/* ------------------------------------------------------------------------------------
 * ca_gemm: C[M,N] = epilogue( A[M,K] * W[N,K]^T )        (MFMA 16x16x32, fp32 accumulate)
 *
 * Replaces: every nn.Linear / 1x1 conv on the path --
 *   diffusers Attention.to_q/to_k/to_v/to_out (animatediff/models/attention.py:206-285 via
 *   modules/attention_processor.py:233-262), GEGLU.proj + ff.net[2]
 *   (animatediff/models/attention.py:303-357), Transformer3DModel.proj_in/proj_out
 *   (animatediff/models/attention.py:90,118), motion-module proj_in/proj_out
 *   (animatediff/models/motion_module.py:112,134), ResnetBlock3D.time_emb_proj and
 *   conv_shortcut (animatediff/models/resnet.py:163,186), TimestepEmbedding
 *   (animatediff/models/unet.py:526-534), ControlNet zero-convs.
 *
 * A may be the channel-concatenation of two sources (a2 != NULL): columns [0,k1) come from
 * `a` and [k1,k1+k2) from `a2` (replaces torch.cat at animatediff/models/unet_blocks.py:636,742
 * for the shortcut conv).  K = k1 + k2.
 *
 * epilogue, per element (m,n), v = acc:
 *   v += bias[n]                      (bias fp32 or NULL)
 *   v += rowbias[(m / rows_per_group) * ld_rowbias + n]   (fp32 or NULL; time-embedding add,
 *                                      animatediff/models/resnet.py:199-200)
 *   v *= alpha
 *   v += residual[m*ld_res + n]       (dtype or NULL; residual adds attention.py:273,285,288;
 *                                      motion_module.py:218-222; resnet.py:216)
 *   v *= post_scale                   (1/output_scale_factor, resnet.py:216)
 *   v = act(v)
 *   if geglu: weight rows are interleaved (h0,g0,h1,g1,...); out[m, n/2] = h * gelu_erf(g)
 *             (diffusers GEGLU); C then has N/2 columns.
 *   out_f32: store fp32 instead of dtype.
 * Requirements: K1, K2, N multiples of 8 (N multiple of 4 allowed when N < 8), lda/ldc/ld_res
 * multiples of 8 (dtype) so that 16-byte accesses are aligned.
 * ------------------------------------------------------------------------------------ */
typedef struct ca_gemm_args {
  const void* a;        /* [M, k1] rows at stride lda            */
  const void* a2;       /* [M, k2] rows at stride lda2, or NULL  */
  const void* w;        /* [N, K] row-major (PyTorch Linear.weight layout), dtype */
  void* c;              /* [M, N or N/2]                          */
  const float* bias;    /* [N] fp32 or NULL                       */
  const float* rowbias; /* [ceil(M/rows_per_group), ld_rowbias] fp32 or NULL */
  const void* residual; /* [M, N] dtype or NULL                   */
  int64_t lda, lda2, ldc, ld_res, ld_rowbias;
  int32_t m, n, k1, k2;
  int32_t rows_per_group;
  float alpha, post_scale;
  int32_t act;          /* CA_ACT_*      */
  int32_t geglu;        /* 0/1           */
  int32_t out_f32;      /* 0/1           */
  int32_t dtype;        /* CA_BF16/CA_F16 */
  /* LayerNorm folded into the GEMM (nn.LayerNorm + the Linear it feeds: animatediff/models/attention.py:
   * 214-237,263-288 norm1/2/3, motion_module.py:203-224 norms / ff_norm):  with W' = W diag(gamma) packed as
   * `w` and bias' = W beta + b as `bias`,
   *     LN(x) W^T + b = rstd * (x W'^T - mean * colsum(W')) + bias'
   * `ln_stats` [M][2] = (mean, rstd) per A row (ca_layernorm with `stats` set), `ln_colsum` [N] = the row sums
   * of W' as packed (both fp32, both or neither).  Applied to the accumulator before bias/rowbias.  A is then the
   * un-normalised tensor: the normalised copy is never written or re-read. */
  const float* ln_stats;
  const float* ln_colsum;
  /* ABI v6: `ln_colsum` set and `ln_stats` NULL = the kernel computes (mean, rstd = 1/sqrt(var + ln_eps)) of the A rows
   * itself while it streams them -- the separate statistics pass over A (ca_layernorm `stats`) disappears.  Available
   * only where ca_gemm_ln_inline_supported(args) returns 1 (the weight-resident K = 320 kernel of the 64x64-latent
   * level); elsewhere ca_gemm returns CA_ERR_ARG and the caller passes ln_stats. */
  float ln_eps;
  /* ABI v6: optional split-K scratch (device memory, caller-owned, may be shared by every call on one stream) of at
   * least ca_gemm_workspace_bytes(args) bytes, or NULL / too small: the GEMM then runs unsplit -- same results up to
   * fp32 summation order, only slower on grids that under-fill the chip (M = 2048: the 8x8-latent level). */
  void* workspace;
  int64_t workspace_bytes;
  /* ABI v6: LayerNorm statistics handed from the producing GEMM to the consuming one, without a pass over the tensor.
   *   producer: `row_sums_out` [M][P][2] fp32, P = ca_gemm_row_sums_parts(args) = N / 320 > 0: the epilogue also writes
   *             (sum, sum of squares) of every STORED output row per 320-column tile (the 128x320-tile kernel only;
   *             0 from the query = not available for this launch, do not set the pointer);
   *   consumer: `ln_parts` = P and `ln_stats` = that array instead of (mean, rstd): the epilogue adds the P partial
   *             sums in order and finishes mean / rstd = 1 / sqrt(var + ln_eps) itself (K of the consumer = the row width). */
  float* row_sums_out;
  int32_t ln_parts;
  /* ABI v9: `w` once more in MFMA-fragment order (written by ca_pack_w_frag(w, n, k, geglu, ...) with the SAME geglu flag as
   * this call), or NULL.  With it the K = 320 projections of the 64x64-latent level (M >= 16384, N % 320 == 0, N >= 960, one A source,
   * alpha = post_scale = 1, no activation: q|k|v, the GEGLU projection -- animatediff/models/attention.py:214-237,303-357,
   * motion_module.py:203-224) run on the activation-resident kernel, whose waves read W fragments straight from L2; `w` is
   * still what every other plan reads.  With ln_colsum set and ln_stats NULL that kernel leaves its (mean, rstd) in
   * `workspace` (ca_gemm_workspace_bytes = 8 M); without the workspace the launch keeps the weight-resident kernel. */
  const void* w_frag;
} ca_gemm_args;
int ca_gemm(const ca_gemm_args* args, void* stream);
/* ABI v9: dst[n * k] = the fragment-ordered copy of w[n, k] (k = 320, n % 64 == 0, 16-bit elements, 16-byte aligned) that
 * ca_gemm_args.w_frag takes; geglu = the flag of the ca_gemm calls that will use it (the weight-row interleave behind the
 * 16-byte stores differs).  Weights are packed once per model, so this runs at load time. */
int ca_pack_w_frag(const void* w, int32_t n, int32_t k, int32_t geglu, void* dst, void* stream);
/* ------------------------------------------------------------------------------------
 * ca_ff_fused (ABI v9): the whole feed-forward of a transformer block in one launch,
 *     y = GEGLU(LN(x) W1^T + b1) W2^T + b2 + residual
 * Replaces: BasicTransformerBlock / TemporalTransformerBlock feed-forward (animatediff/models/attention.py:288,303-357:
 *   `ff(norm3(hidden)) + hidden`; motion_module.py:203-224) at the 64x64-latent level -- LayerNorm fold, GEGLU projection and
 *   output projection as ca_gemm computes them (same rounding of the projection output and of h to the activation type), but
 *   the [M, 1280] intermediate stays in LDS.  Available for c = 320, inner = 1280, M >= 16384 (ca_ff_fused_supported; no
 *   launch, no device access); everything else runs as two ca_gemm calls.
 *   w1_frag: the LayerNorm-folded GEGLU weight [2560, 320] (rows value / gate interleaved) in the order of ca_pack_w_frag(geglu = 1);
 *   bias1 / colsum1 [2560] fp32 as ca_gemm's bias / ln_colsum; ln_stats [M][2] (mean, rstd) or NULL = computed in the kernel
 *   (ln_eps > 0); w2_frag: the output weight [320, 1280] in the order of ca_pack_w2_frag; bias2 [320] fp32 or NULL;
 *   residual [M, 320] or NULL. */
typedef struct ca_ff_args {
  const void* x;        /* [M, c] rows at stride lda */
  const void* w1_frag;
  const float* bias1;
  const float* colsum1;
  const float* ln_stats;
  const void* w2_frag;
  const float* bias2;
  const void* residual; /* [M, c] rows at stride ld_res, or NULL */
  void* y;              /* [M, c] rows at stride ldc */
  int64_t lda, ldc, ld_res;
  int32_t m, c, inner;
  float ln_eps;
  int32_t dtype;
  /* ABI v12: the transformer's output projection behind its last feed-forward, in the same launch
   * (animatediff/models/attention.py:163-175 `proj_out(hidden) + residual`; motion_module.py:158-163):  `y` then receives
   *   y_out = (feed-forward output) Wout^T + bias_out + residual_out.
   * w_out_frag: CA_ATTN_WOUT_FRAG_ELEMS elements written by ca_pack_w_out(proj_out.weight [c, c]); NULL = no output stage (as ABI v9).
   * Needs m % 128 == 0.  bias_out [c] fp32 or NULL; residual_out rows at stride ld_res_out (the transformer's input) or NULL. */
  const void* w_out_frag;
  const float* bias_out;
  const void* residual_out;
  int64_t ld_res_out;
} ca_ff_args;
int ca_ff_fused(const ca_ff_args* args, void* stream);
int ca_ff_fused_supported(const ca_ff_args* args);
/* dst[320 * 1280] = w[320, 1280] in the fragment order ca_ff_args.w2_frag takes (16-bit elements, 16-byte aligned). */
int ca_pack_w2_frag(const void* w, int32_t n, int32_t k, void* dst, void* stream);
/* ABI v10: the motion module's temporal self-attention of the 64x64-latent level up to (not including) its output projection,
 *   o = softmax(q k^T * scale) v per (pixel, head) over the frames,  q | k | v = (LayerNorm(x) + pe[frame]) Wqkv^T,
 * in one launch (animatediff/models/motion_module.py:251-331: norm, pos_encoder, to_q / to_k / to_v, attention with the frames
 * as the sequence).  Rows of x and o are in (batch, frame, token) order.  Takes c = 320, 8 heads, 16 frames (ABI v12: also 8 and 32
 * frames when the output stage is used), tokens a multiple of 128 / frames, >= 16384 rows (ca_tattn_fused_supported: no launch, no device access); everything else runs as ca_gemm + ca_attention.
 *   w_frag: CA_TATTN_W_FRAG_ELEMS 16-bit elements in the order of ca_pack_w_tattn (the UNFOLDED Wq | Wk | Wv);
 *   gamma [c] fp32: the LayerNorm weight; bias_pe [frames][ld_bias_pe] fp32: LayerNorm bias + positional encoding of the frame. */
#define CA_TATTN_W_FRAG_ELEMS 368640
typedef struct ca_tattn_args {
  const void* x;        /* [batch * frames * tokens, c] rows at stride lda */
  const void* w_frag;
  const float* gamma;
  const float* bias_pe;
  void* o;              /* [batch * frames * tokens, c] rows at stride ldo */
  int64_t lda, ldo, ld_bias_pe;
  int32_t batch, frames, tokens, heads, c;
  float ln_eps, scale;  /* scale = head_dim ** -0.5 */
  int32_t dtype;
  /* ABI v12: the attention's output projection, bias and residual in the SAME launch (motion_module.py:212-224,
   * `attention_block(norm(x)) + x`; modules/attention_processor.py:258-270 to_out[0]):  `o` then receives
   *   y = o Wout^T + bias_out + residual        instead of the attention output.
   * w_out_frag: CA_ATTN_WOUT_FRAG_ELEMS elements written by ca_pack_w_out(Wout [c, c]); NULL = no output stage (as ABI v10).
   * bias_out [c] fp32 or NULL; residual rows at stride ld_res (same row order as x / o) or NULL. */
  const void* w_out_frag;
  const float* bias_out;
  const void* residual;
  int64_t ld_res;
} ca_tattn_args;
int ca_tattn_fused(const ca_tattn_args* args, void* stream);
int ca_tattn_fused_supported(const ca_tattn_args* args);
/* ABI v12: dst[CA_ATTN_WOUT_FRAG_ELEMS] = w[320, 320] (an attention's to_out[0].weight) in the fragment order the output stage of
 * ca_tattn_fused / ca_xattn_fused streams (ca_tattn_args.w_out_frag); 16-bit elements, 16-byte aligned. */
#define CA_ATTN_WOUT_FRAG_ELEMS 102400
int ca_pack_w_out(const void* w, int32_t n, int32_t k, void* dst, void* stream);
/* dst[CA_TATTN_W_FRAG_ELEMS] = w[960, 320] (rows Wq, Wk, Wv) in the fragment order ca_tattn_args.w_frag takes (head dim 40
 * padded to 48 with zero rows; 16-bit elements, 16-byte aligned). */
int ca_pack_w_tattn(const void* w, int32_t n, int32_t k, void* dst, void* stream);
/* ABI v11: the text cross-attention of the 64x64-latent level up to (not including) its output projection,
 *   o = softmax(q K^T * scale) V per (row, head),  q = LayerNorm(x) Wq^T + bias,  K / V = the projected text tokens of the row's batch element,
 * in one launch (animatediff/models/attention.py:253-262: norm2, attn2.to_q, attention over encoder_hidden_states).  Row r belongs to
 * image r / tokens; image z uses text batch (z / frames_per_kv) % kv_mod.  Takes c = 320, 8 heads of 40, 65..80 keys, tokens % 128 == 0,
 * m >= 16384 and a multiple of tokens (ca_xattn_fused_supported: no launch, no device access); everything else runs as ca_gemm + ca_attention.
 *   wq_frag: CA_XATTN_W_FRAG_ELEMS 16-bit elements written by ca_xattn_pack_w from the LayerNorm-FOLDED Wq (Wq diag(gamma));
 *   bias [c] fp32 (Wq beta + b) or NULL;  kv_frag: kv_batches * 8 * CA_XATTN_KV_FRAG_ELEMS elements written by ca_xattn_pack_kv
 *   (K pre-multiplied by scale * log2 e, once per window and layer). */
#define CA_XATTN_W_FRAG_ELEMS 122880
#define CA_XATTN_KV_FRAG_ELEMS 7680
typedef struct ca_xattn_args {
  const void* x;        /* [m, c] rows at stride lda */
  const void* wq_frag;
  const float* bias;
  const void* kv_frag;
  void* o;              /* [m, c] rows at stride ldo */
  int64_t lda, ldo;
  int32_t m, tokens, frames_per_kv, kv_mod, kv_batches, nk, heads, c;
  float ln_eps;
  int32_t dtype;
  /* ABI v12: output projection + bias + residual in the same launch, as ca_tattn_args (animatediff/models/attention.py:253-262
   * `attn2(norm2(hidden)) + hidden`).  w_out_frag NULL = no output stage (as ABI v11). */
  const void* w_out_frag;
  const float* bias_out;
  const void* residual;
  int64_t ld_res;
  /* ABI v13: the IP-Adapter's image-prompt tokens in the same launch (modules/attention_processor.py:433-477, IPAttnProcessor2_0:
   * `hidden = attention(q, K, V) + scale * attention(q, K_ip, V_ip)` before to_out).  kv_frag_ip: a second ca_xattn_pack_kv buffer
   * (same kv_batches; packed from the to_k_ip | to_v_ip projection of the last nk_ip context rows, nk_ip 1..16); needs w_out_frag.
   * NULL / 0 = no image-prompt tokens (as ABI v12). */
  const void* kv_frag_ip;
  int32_t nk_ip;
  float ip_scale;
} ca_xattn_args;
int ca_xattn_fused(const ca_xattn_args* args, void* stream);
int ca_xattn_fused_supported(const ca_xattn_args* args);
/* dst[CA_XATTN_W_FRAG_ELEMS] = w[320, 320] in the per-head fragment order ca_xattn_args.wq_frag takes (head dim 40 padded to 48 with zero rows). */
int ca_xattn_pack_w(const void* w, int32_t n, int32_t k, void* dst, void* stream);
/* dst[kv_batches * 8 * CA_XATTN_KV_FRAG_ELEMS] = the K (columns 0..319, * scale * log2 e) and V (columns 320..639) rows
 * row_offset .. row_offset + nk of every batch of kv [kv_batches * rows_per_batch, ld] as MFMA fragments in lane order; nk 65..80 (the text keys) or, ABI v13,
 * 1..16 (the image-prompt set: ca_xattn_args.kv_frag_ip). */
int ca_xattn_pack_kv(const void* kv, int64_t ld, int32_t kv_batches, int32_t rows_per_batch, int32_t row_offset, int32_t nk, float scale, int32_t dtype,
                     void* dst, void* stream);
/* bytes of split-K scratch this launch can use (0: it would not split) */
int64_t ca_gemm_workspace_bytes(const ca_gemm_args* args);
/* partial sums per row this launch can leave in row_sums_out (0: it cannot).  N / 320 on the 128 x 320-tile kernels; ABI v8:
 * 4 * N / 320 on the 256 x 320 kernel (one per 80-column wave quarter) -- a consumer's ln_parts takes at most 4, so more are
 * finished with ca_ln_finish_sums first. */
int ca_gemm_row_sums_parts(const ca_gemm_args* args);
/* 1 if ca_gemm can take these args with ln_stats == NULL (fields other than the pointers' values are what matters;
 * no launch, no device access). */
int ca_gemm_ln_inline_supported(const ca_gemm_args* args);
/* ABI v8: 1 if a consumer launch with partial sums (ln_parts > 0) should rather get finished statistics: the kernel the plan
 * prefers for the shape (256 x 320 tiles) reads (mean, rstd) only.  The caller then runs ca_ln_finish_sums and passes
 * ln_stats = its output, ln_parts = 0.  No launch, no device access. */
int ca_gemm_wants_finished_stats(const ca_gemm_args* args);
/* ABI v8: (mean, rstd = 1 / sqrt(var + eps)) [rows][2] from `sums` [rows][parts][2] = (sum, sum of squares) per row and
 * 320-column tile as left by a producing GEMM (row_sums_out); k = the row width.  Same arithmetic and order as the consuming
 * epilogues that finish the sums themselves (reference: nn.LayerNorm statistics, animatediff/models/attention.py:214-237). */
int ca_ln_finish_sums(const float* sums, int parts, int64_t rows, int k, float eps, float* mean_rstd, void* stream);
/* ABI v7: the label of the kernel instantiation ca_gemm would launch for these arguments ("wres160", "pp128x320",
 * "ps128x320", "128x128", "128x160", "128x64_db", "128x128_splitk6", "reg_128x64", ...), written NUL-terminated into
 * buf[len].  No launch, no device access: the choice is a pure function of the sizes, strides, flags and which pointers
 * are set (the product library has no tuning environment variables).  Returns CA_OK or the error ca_gemm would return. */
int ca_gemm_plan_name(const ca_gemm_args* args, char* buf, int32_t len);

/* ------------------------------------------------------------------------------------
 * ca_conv3x3: NHWC 3x3 convolution, padding 1, stride 1 or 2, as an implicit GEMM
 *   (M = images*Hout*Wout, N = Cout, K = 9*Cin) on the same MFMA core as ca_gemm.
 *
 * Replaces: InflatedConv3d (animatediff/models/resnet.py:12-20) at conv_in/conv_out
 *   (unet.py:140,319), ResnetBlock3D.conv1/conv2 (resnet.py:153,173), Downsample3D
 *   (resnet.py:96, stride 2), Upsample3D (resnet.py:47,67: `upsample`=1 folds the nearest x2
 *   F.interpolate into the input gather), ControlNet convs and hint embedding.
 * Input may be the channel concat of two NHWC sources (x2 != NULL).
 * Weight layout: [Cout][kh][kw][Cin] (packed once at load from PyTorch's [Cout][Cin][kh][kw]).
 * Epilogue fields as in ca_gemm (rowbias = time embedding per batch element b:
 *   rows_per_group = f*Hout*Wout; residual = shortcut input).
 * Hin/Win are the dimensions of the STORED input; with upsample=1 the logical input is
 * 2*Hin x 2*Win.  Cin1, Cin2, Cout multiples of 8 (Cout multiple of 4 when < 8).
 * ------------------------------------------------------------------------------------ */
typedef struct ca_conv_args {
  const void* x;        /* [images, Hin, Win, cin1] */
  const void* x2;       /* [images, Hin, Win, cin2] or NULL */
  const void* w;        /* [cout, 3, 3, cin1+cin2] */
  void* y;              /* [images, Hout, Wout, cout] */
  const float* bias;
  const float* rowbias;
  const void* residual; /* [images*Hout*Wout, ld_res] */
  int64_t ld_res, ld_rowbias;
  int32_t images, hin, win, cin1, cin2, cout;
  int32_t stride;       /* 1 or 2 */
  int32_t upsample;     /* 0 or 1 (nearest x2 before the conv) */
  int32_t rows_per_group;
  float alpha, post_scale;
  int32_t act;
  int32_t out_f32;
  int32_t dtype;
  /* Scratch for the split-K schedule of small-M convolutions (8x8 / 16x16 latent levels, where
   * M/128 x Cout/128 tiles cannot fill 256 CUs).  Caller-owned device memory of at least
   * ca_conv3x3_workspace_bytes(args) bytes, or NULL / too small: the convolution then runs
   * unsplit.  Results are deterministic either way (slabs are added in a fixed order). */
  void* workspace;
  int64_t workspace_bytes;
  /* 0: zero padding 1 on every side (Conv2d padding=1).  1: no padding before, one row/column after
   * (diffusers Downsample2D(padding=0): F.pad(x, (0,1,0,1)) + Conv2d(stride=2), the VAE encoder's
   * downsamplers): Hout = (H + 1 - 3) / stride + 1. */
  int32_t pad_asym;
  /* ABI v12: the weight once more in Winograd form, U [16][cout][cin1 + cin2] = G g G^T per (cout, cin) (written by ca_pack_w_wino
   * from `w`), or NULL.  With it -- and a workspace of ca_conv3x3_workspace_bytes(args) bytes -- the deep convolutions of the small-latent
   * levels (stride 1, padding 1, with or without `upsample`, even output H and W, cin >= 1280 (>= 640 at up to 4096 tiles), cout % 320 == 0,
   * images * Hout * Wout / 4 a multiple of 256 and at most 16384 tiles) run as F(2x2, 3x3): an input transform, ONE launch of the 256 x 320 GEMM kernel over the sixteen transformed GEMMs,
   * an output transform that applies the epilogue.  2.25 x fewer multiply-adds; results differ from the direct form by fp16 rounding
   * of the transformed operands (tests/test_kernels_gpu.py::test_conv3x3_winograd).  NULL / no workspace / another shape: the direct form. */
  const void* w_wino;
  /* ABI v12: 1 = `x` IS the transformed input V [16][tiles][cin1] already (written by ca_groupnorm's wino_v; cin2 = 0): the Winograd
   * route starts at its GEMM.  The call fails unless the route is taken (w_wino, workspace, shape); the workspace then holds M only
   * (ca_conv3x3_workspace_bytes says how much). */
  int32_t x_is_wino_v;
} ca_conv_args;
/* ABI v12: dst[16 * cout * cin] = G g G^T of w [cout][3][3][cin] (the layout of ca_conv_args.w) in the element type `dtype`. */
int ca_pack_w_wino(const void* w, int32_t cout, int32_t cin, int32_t dtype, void* dst, void* stream);
int64_t ca_conv3x3_workspace_bytes(const ca_conv_args* args);
int ca_conv3x3(const ca_conv_args* args, void* stream);
/* ABI v7: as ca_gemm_plan_name, for ca_conv3x3 */
int ca_conv3x3_plan_name(const ca_conv_args* args, char* buf, int32_t len);
/* Added to ABI v16 (three new functions; no struct or existing function changes, so the version number stays): the upsampling convolution (upsample = 1, stride 1, padding 1) as four 2x2 "phase" convolutions in ONE launch of the
 * 256 x 320 kernel.  An output pixel (2y + py, 2x + px) reads only the 2x2 source pixels (y + py - 1 + dy, x + px - 1 + dx), so the nine
 * taps that land on the same source pixel are summed ahead of time: args->w is w_phase [4][cout][2][2][cin], phase = 2 py + px, with
 *   rows  py = 0: {w[0], w[1] + w[2]}   py = 1: {w[0] + w[1], w[2]}     (columns alike; summed in fp32, rounded once)
 * and an out-of-image source row / column is exactly the zero padding of the upsampled image.  4/9 of the multiply-adds of
 * ca_conv3x3(upsample = 1); same output dtype, bias, residual and alpha; deterministic.  Takes one source (x2 NULL) with cin % 64 == 0,
 * cout % 320 == 0, no row bias / activation / post_scale / fp32 output, 16-byte aligned operands; w_wino and workspace are ignored.
 * ca_conv_up2_phase_supported: 1 where the kernel takes the arguments AND the form pays (whole rounds of 256 output tiles over the four
 * phases, or >= 1024 tiles); ca_conv_up2_phase itself runs every shape the kernel implements and fails on the others. */
int ca_conv_up2_phase_supported(const ca_conv_args* args);
int ca_conv_up2_phase(const ca_conv_args* args, void* stream);
int ca_conv_up2_phase_plan_name(const ca_conv_args* args, char* buf, int32_t len);

/* ------------------------------------------------------------------------------------
 * GroupNorm (+ optional SiLU), NHWC, two launches: statistics then apply.
 *
 * Replaces: InflatedGroupNorm / nn.GroupNorm + SiLU (animatediff/models/resnet.py:23-31,
 *   148-151,169-170,191-192,202,208; unet.py:316-317,614-615), GroupNorm eps=1e-6 without
 *   activation (animatediff/models/attention.py:86,130; motion_module.py:111,144).
 * `frames_per_stat` = 1 gives per-frame statistics (InflatedGroupNorm / v2); = f gives the
 * cross-frame statistics of plain nn.GroupNorm on the 5-D tensor (v1 motion module configs,
 * SURVEY App. C-5).  Input may be a channel concat of two sources.
 *
 * ca_groupnorm_stats writes partial (sum, sumsq) per (stat group, row chunk, norm group)
 * into `partials` (fp32, ca_groupnorm_partials_floats() elements); ca_groupnorm_apply
 * reduces the partials deterministically (fixed order, fp64 combine) and normalises.
 * ------------------------------------------------------------------------------------ */
typedef struct ca_groupnorm_args {
  const void* x;        /* [images, hw, c1] */
  const void* x2;       /* [images, hw, c2] or NULL */
  void* y;              /* [images, hw, c1+c2] */
  const float* gamma;   /* [c1+c2] */
  const float* beta;    /* [c1+c2] */
  float* partials;      /* scratch, see ca_groupnorm_partials_floats */
  int32_t images, hw, c1, c2;
  int32_t groups;       /* 32 */
  int32_t frames_per_stat;
  float eps;
  int32_t act;          /* CA_ACT_NONE / CA_ACT_SILU */
  int32_t dtype;
  /* ABI v12 (ca_groupnorm only): with wino_v the launch writes, INSTEAD of y, the Winograd F(2x2, 3x3) input transform of the
   * normalised (+ activated) tensor -- V [16][images * (wino_h / 2) * (wino_w / 2)][c1 + c2], what ca_conv3x3's Winograd route computes
   * from y as its first stage -- so that the convolution behind it (ca_conv_args.x_is_wino_v) starts at its GEMM and y never exists
   * (ResnetBlock3D: norm -> nonlinearity -> conv, animatediff/models/resnet.py:188-212).  hw = wino_h * wino_w.  Only where
   * ca_groupnorm_wino_supported(args) says 1; y and partials are unused then. */
  void* wino_v;
  int32_t wino_h, wino_w;
} ca_groupnorm_args;
int ca_groupnorm_wino_supported(const ca_groupnorm_args* args);
int64_t ca_groupnorm_partials_floats(int32_t images, int32_t hw, int32_t frames_per_stat, int32_t groups);
int ca_groupnorm_stats(const ca_groupnorm_args* args, void* stream);
int ca_groupnorm_apply(const ca_groupnorm_args* args, void* stream);
/* ABI v6: both passes in one call; small statistics groups (8x8 / 16x16 latents) run as ONE launch that keeps the
 * group in registers between the passes.  `partials` as above (unused by the fused kernel, still required). */
int ca_groupnorm(const ca_groupnorm_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * ca_layernorm: y[r,:] = LN(x[r,:]) * gamma + beta (+ pos[(r / rows_per_frame) % frames, :])
 *
 * Replaces: nn.LayerNorm in BasicTransformerBlock (animatediff/models/attention.py:214,231,237)
 *   and TemporalTransformerBlock (motion_module.py:203,209); the optional `pos` table fuses
 *   PositionalEncoding.forward (motion_module.py:243-245: x + pe[:, :f]) -- rows are in
 *   (b f n) order so the frame of row r is (r / rows_per_frame) % frames.
 * eps = 1e-5 (torch default). C multiple of 8, C <= 2048.
 * ------------------------------------------------------------------------------------ */
typedef struct ca_layernorm_args {
  const void* x; void* y;
  const float* gamma; const float* beta;
  const float* pos;     /* [frames, c] fp32 or NULL */
  int64_t rows;
  int32_t c;
  int32_t rows_per_frame, frames;
  float eps;
  int32_t dtype;
  float* stats;         /* non-NULL: write (mean, rstd) per row to stats[2*row ..] and nothing else
                           (y, gamma, beta, pos unused): input of ca_gemm_args.ln_stats */
} ca_layernorm_args;
int ca_layernorm(const ca_layernorm_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * ca_attention: O = softmax(Q K^T * scale) V per (batch z, head), flash-style online softmax,
 *   MFMA for QK^T and PV.  One kernel serves:
 *   - spatial self-attention  (AttnProcessor2_0, modules/attention_processor.py:200-272;
 *     called from animatediff/models/attention.py:271)
 *   - cross-attention with per-b text K/V shared by the f frames of b (kv_div = f; replaces the
 *     `repeat 'b n c -> (b f) n c'` at animatediff/models/attention.py:125) incl. the
 *     ControlNet variant that drops the last 4 tokens (CNAttnProcessor2_0, :608-609: pass nk-4)
 *   - IP-Adapter's second attention over the 4 image tokens, accumulated into O
 *     (IPAttnProcessor2_0, modules/attention_processor.py:461-477): accumulate=1, out_scale=scale
 *   - temporal self-attention over frames (VersatileAttention, animatediff/models/
 *     motion_module.py:272-329): the `(b f) d c -> (b d) f c` transposes are replaced by
 *     strided addressing (row_stride = tokens*ld, inner = tokens).
 *
 * Addressing (element offsets): for batch z (0 <= z < batches):
 *   zo = z / inner_count, zi = z % inner_count
 *   Q row i  at q + zo*q_outer + zi*q_inner + i*q_row + head*head_dim   (same scheme for O)
 *   z' = (z / kv_div) % kv_mod; K row j at k + (z'/kv_inner_count)*k_outer + (z'%kv_inner_count)*k_inner
 *                                   + j*k_row + head*head_dim   (same for V with v pointer)
 * kv_mod reproduces the reference's ControlNet prompt tiling torch.cat([embeds]*frame_count)
 * (modules/controlresiduals_pipeline.py:292: image z reads embeds[z % b]); pass kv_mod = batches when unused.
 * head_dim multiple of 8, <= 160.
 * ------------------------------------------------------------------------------------ */
typedef struct ca_attn_args {
  const void* q; const void* k; const void* v; void* o;
  int64_t q_outer, q_inner, q_row;
  int64_t o_outer, o_inner, o_row;
  int64_t k_outer, k_inner, k_row;   /* shared by K and V */
  int32_t inner_count, kv_inner_count, kv_div, kv_mod;
  int32_t batches, heads, head_dim;
  int32_t nq, nk;
  float scale;          /* softmax scale (head_dim^-0.5) */
  float out_scale;      /* multiplies the attention output */
  int32_t accumulate;   /* 1: O += out_scale * attn */
  int32_t dtype;
  int32_t causal;       /* 1: key j visible to query i only if j <= i (nq == nk).  CLIP text encoder
                           (transformers CLIPTextModel's causal mask; called through Compel at
                           modules/controlanimate_pipeline.py:133-135) */
  /* ABI v7: optional key mask, one byte per (batch z, key j) at key_mask[z * key_mask_stride + j]; 0 = the key is
   * invisible to every query of that batch element (its score is -inf before the softmax), combined with `causal`.
   * transformers' CLIPTextModel `attention_mask` ([B, L] -> additive [B,1,1,L]): what Compel 2.0.2's default
   * DownweightMode.MASK passes for a down-weighted fragment such as `(muscle body)0.2`
   * (modules/controlanimate_pipeline.py:133-135, configs/prompts/SampleConfig.yaml:16).  NULL = no mask.  A query whose
   * keys are ALL masked gets zeros (with `accumulate`: its output row is left as it was). */
  const uint8_t* key_mask;
  int64_t key_mask_stride;
} ca_attn_args;
int ca_attention(const ca_attn_args* args, void* stream);
/* ABI v12: the label of the kernel ca_attention runs for these arguments ("attn_dma40" the LDS-DMA kernel at head_dim 40,
 * "attn_dma80", "attn_dma_fold" / "attn_dma_sr" / "attn_dma", "attn_short" the register-resident text cross-attention,
 * "attn_tiny16" / "attn_tiny32" the one-wave temporal forms, "attn_generic").  No launch, no device access: the parity tests
 * assert with it that the headline shapes ran on the kernels DESIGN.md names (tests/test_fullsize_gpu.py, test_dispatch_plan.py). */
int ca_attention_plan_name(const ca_attn_args* args, char* buf, int32_t len);

/* ------------------------------------------------------------------------------------
 * Small elementwise kernels of the loop.
 * ------------------------------------------------------------------------------------ */

/* out[i] = a[i] + b[i % b_period]  (dtype).  ControlNet residual adds incl. the broadcast of
 * b=1 residuals over the CFG batch (animatediff/models/unet.py:567-576,584-585). n multiple of 8. */
int ca_add_bcast(const void* a, const void* b, void* out, int64_t n, int64_t b_period,
                 int32_t dtype, void* stream);
/* ABI v8: dst = `times` copies of the `bytes` of src behind each other (one read of src): torch.cat([x] * times) along the
 * leading dimension -- the reference's torch.cat([latents] * 2) (animatediff/pipelines/controlanimation_pipeline.py:797) makes
 * the two CFG halves identical, the shared prefix is computed once and repeated here.  16-byte vector copies when bytes % 16 == 0
 * and both pointers are 16-byte aligned, a byte-granular kernel otherwise (any size, any alignment). */
int ca_repeat(const void* src, void* dst, int64_t bytes, int32_t times, void* stream);

/* y[r, :] = softmax(scale * x[r, :]) for an fp32 score matrix, written in `dtype`.
 * Replaces the softmax inside F.scaled_dot_product_attention for the VAE's mid-block attention
 * (third-party diffusers==0.23.0 AutoencoderKL: Attention(heads=1, dim_head=512) called at
 * animatediff/pipelines/controlanimation_pipeline.py:508 (decode) and :577,589 (encode)), whose
 * head_dim is beyond ca_attention's fused kernel: scores and P.V run through ca_gemm. cols % 4 == 0. */
int ca_softmax_rows(const float* x, void* y, int64_t rows, int32_t cols, int64_t ldx, int64_t ldy,
                    float scale, int32_t dtype, void* stream);

/* y = silu(x) on fp32 vectors (ResnetBlock3D: time_emb_proj(silu(temb)), resnet.py:196). */
int ca_silu_f32(const float* x, float* y, int64_t n, void* stream);

/* Timesteps(320, flip_sin_to_cos=True, freq_shift=0) (unet.py:526):
 * out[b, :] = [cos(t*f_i), sin(t*f_i)], f_i = exp(-ln(10000)*i/half); out dtype for the
 * following linear_1 GEMM. `t` per batch element in a device fp32 array or (t_dev NULL) the
 * scalar t_host. */
int ca_timestep_embedding(const float* t_dev, float t_host, void* out, int32_t batch,
                          int32_t dim, int32_t dtype, void* stream);

/* latents [b0, c, f, h, w] fp32 -> UNet input NHWC [rep*b0*f, h, w, cpad] dtype, multiplied by
 * in_scale (scheduler.scale_model_input) and duplicated `rep` times for CFG
 * (controlanimation_pipeline.py:797-800).  Channels c..cpad-1 are zero. */
int ca_latents_to_nhwc(const float* latents, void* out, int32_t b0, int32_t c, int32_t f,
                       int32_t h, int32_t w, int32_t cpad, int32_t rep, float in_scale,
                       int32_t dtype, void* stream);

/* UNet output NHWC [b*f, h, w, c] (dtype or fp32) -> [b, c, f, h, w] fp32 (API boundary). */
int ca_nhwc_to_ncfhw_f32(const void* x, float* out, int32_t b, int32_t c, int32_t f, int32_t h,
                         int32_t w, int32_t ldx, int32_t x_is_f32, int32_t dtype, void* stream);

/* generic layout converters at the module API boundary:
 * [b, c, f, h, w] (fp32 | fp16 | bf16, arbitrary strides given in elements) <-> NHWC dtype. */
int ca_ncfhw_to_nhwc(const void* x, int32_t x_kind /*0 f32,1 f16,2 bf16*/, const int64_t strides[5],
                     void* out, int32_t b, int32_t c, int32_t f, int32_t h, int32_t w, int32_t cpad,
                     int32_t dtype, void* stream);

/* Fused classifier-free-guidance combine + scheduler update
 * (controlanimation_pipeline.py:844-849 and the step functions :1520-1609 / diffusers
 * DDIM/LCM/Euler restated in oracle/schedulers.py).  eps comes NHWC fp32 [rep*f, h, w, ld_eps]
 * from conv_out; latents/noise/prev/denoised are [1, c, f, h, w] fp32.
 *   eps  = rep==2 ? e_u + g*(e_c - e_u) : e
 *   x0   = (x - coef[0]*eps) * coef[1];  if clip > 0: x0 = clamp(x0, -clip, clip)
 *   den  = coef[2]*x0 + coef[3]*x
 *   prev = coef[4]*den + coef[5]*eps + coef[6]*noise
 * `noise` / `denoised` may be NULL. */
int ca_cfg_scheduler_step(const float* eps, int32_t ld_eps, int32_t rep, float guidance,
                          const float* latents, const float* noise, float* prev, float* denoised,
                          int32_t c, int32_t f, int32_t h, int32_t w, const float coef[7],
                          float clip, void* stream);

/* out[i] = sum_k coef[k] * x[k][i], fp32, 1 <= n_terms <= 8 (out may alias any x[k]).
 * The update rule of the MULTISTEP / history-carrying samplers the reference's facade offers
 * (modules/controlanimate_pipeline.py:52-61: DPMSolverMultistep, LMSDiscrete, PNDM): each of their steps is a fixed
 * linear combination of the current sample, the current and earlier model outputs and (ancestral) noise, with
 * host-computed coefficients (controlanimate_amd/schedulers.py).  The CFG combine that precedes it is
 * ca_cfg_scheduler_step with coef = {0,1,0,0, 0,1,0} (prev := combined eps). */
int ca_lincomb(float* out, const float* const* x, const float* coef, int32_t n_terms, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------
 * ABI v14: the Real-ESRGAN upscaler (RRDBNet anime-6B, num_feat 64, num_grow_ch 32, scale 4) that the reference runs on
 * every emitted frame (modules/upscaler.py:25-47, scripts/vid2vid.py:236-242, through RealESRGANer.enhance).
 *
 * ca_conv3x3_narrow: NHWC 3x3 convolution, padding 1, stride 1, for the narrow output widths of RRDBNet (cout 16 / 32 / 64,
 *   and conv_last's 3 with out_u8).  Implicit GEMM on the 16x16x32 MFMA; every block computes ALL cout columns of its pixels,
 *   so the input strip is read once per block; the weight is streamed over K (tap, 32-channel chunk) from L2.
 *   - input `x` [images, hin, win, ldx]: the first `cin` channels are read (cin % 8 == 0, ldx >= cin, ldx % 8 == 0), so a
 *     layer reads the leading channels of a dense block's concat buffer [x | x1 | x2 | x3 | x4] without a torch.cat;
 *   - upsample = 1: nearest x2 (F.interpolate(scale_factor=2, mode='nearest')) folded into the gather: hout = 2 hin;
 *   - output written at y + pixel * ldy + channel_offset + c (channel_offset % 4 == 0, channel_offset + cout <= ldy, ldy % 4 == 0):
 *     x1 .. x4 land in their slices of the concat buffer; other channels of y are never touched;
 *   - epilogue: v = conv + bias[c]; v = leaky_relu ? (v > 0 ? v : 0.2 v) : v; y = s0 v + s1 r1[pixel, c] + s2 r2[pixel, c]
 *     (r1 / r2 may be NULL; ld_r1 / ld_r2 % 4 == 0).  r1 / r2 may alias y at the same pixel and channel (read before written by
 *     the same lane);
 *   - out_u8 = 1 (cout == 3, the last conv): y is uint8 [images, hout, wout, 3]: clamp(v, 0, 1) * 255 rounded half to even,
 *     channels reversed (RealESRGANer's output_img[[2, 1, 0]]); ldy / channel_offset / r1 / r2 unused.
 *   The weight `w` is [round_up(cout, 16)][3][3][round_up(cin, 32)] in `dtype`, zero padded (the padding is read).
 *   Addresses are flat 64-bit (no buffer resource descriptors): a 2048 x 3072 x 64 activation per frame is addressable; the
 *   pixel count images * hout * wout must stay below 2^31.
 * ------------------------------------------------------------------------------------ */
typedef struct ca_conv3x3_narrow_args {
  const void* x;
  const void* w;
  void* y;
  const float* bias;    /* [cout] fp32 or NULL */
  const void* r1;
  const void* r2;
  int64_t ldx, ldy, ld_r1, ld_r2;
  int32_t images, hin, win, cin, cout;
  int32_t channel_offset;
  int32_t upsample;     /* 0 or 1 */
  int32_t leaky_relu;   /* 0 or 1: LeakyReLU(negative_slope = 0.2) */
  float s0, s1, s2;
  int32_t out_u8;       /* 0 or 1 */
  int32_t dtype;
} ca_conv3x3_narrow_args;
int ca_conv3x3_narrow(const ca_conv3x3_narrow_args* args, void* stream);
/* as ca_conv3x3_plan_name, for ca_conv3x3_narrow ("convn_n64m64", "convn_n32m128", "convn_n16m128"); no launch */
int ca_conv3x3_narrow_plan_name(const ca_conv3x3_narrow_args* args, char* buf, int32_t len);

/* uint8 RGB frames [images, h, w, 3] -> RRDBNet input NHWC [images, h, w, 8] in `dtype`: channel c = src[2 - c] / 255 (fp32
 * division, then rounded to `dtype`) for c < 3, zero for c = 3..7.  RealESRGANer.enhance treats the RGB array the reference hands
 * it (np.asarray(pil_image)) as BGR and converts BGR -> RGB: the net sees the channels reversed. */
int ca_rgb8_to_nhwc(const uint8_t* src, void* dst, int32_t images, int32_t h, int32_t w, int32_t dtype, void* stream);

/* uint8 [images, sh, sw, 3] -> [images, dh, dw, 3] with OpenCV's INTER_LANCZOS4 integer path (cv2.resize on 8-bit data, called
 * by RealESRGANer.enhance when outscale != 4): for every destination column dx, xofs[dx] = floor(fx) - 3 and alpha[dx][0..7]
 * the 11-bit fixed-point Lanczos-4 weights of source columns xofs[dx] + k (clamped to the image: edge replication); rows the
 * same with yofs / beta.  dst = saturate((sum_k beta[k] * (sum_j alpha[j] * src[row k][col j]) + 2^21) >> 22), all in int32.
 * The tables are computed on the host (controlanimate_amd/upscaler.py: lanczos4_tables). */
int ca_resize_lanczos4_u8(const uint8_t* src, uint8_t* dst, int32_t images, int32_t sh, int32_t sw, int32_t dh, int32_t dw,
                          const int32_t* xofs, const int16_t* alpha, const int32_t* yofs, const int16_t* beta, void* stream);

/* ------------------------------------------------------------------------------------
 * ABI v15: the colour match of the window loop.  Every window after the first is matched to the previous window's output
 * with color_matcher's compound method 'hm-mkl-hm' (scripts/vid2vid.py:216-218 through modules/utils.py:116-130; the host
 * restatement is controlanimate_amd/vid2vid.py: match_colors / _hist_match / _mkl / _minmax).  For uint8 frames the compound is
 * a chain of device stages with 256-entry float64 tables and one 3x3 matrix between them; the tables and the matrix are
 * computed on the host from the histograms and the moments (controlanimate_amd/color_match.py).  Frames are uint8
 * [images, pixels, 3] (pixels = H * W, interleaved RGB); float64 images are channel planes [images][3][pixels].
 * All float64 arithmetic is unfused (a * b + c rounds twice, as numpy's); no reduction uses floating-point atomics, so two
 * runs on the same input give the same bits.  1 <= images <= 21845, 1 <= pixels <= 2^30; float64 buffers 8-byte aligned.
 * ------------------------------------------------------------------------------------ */

/* Bytes of the scratch buffer the entry points below share for `images` frames of `pixels` pixels: the second key buffer of
 * the sort (3 * images * pixels float64), its per-pass block counters, the partial sums of the moments and the min / max
 * partials that the rank map leaves for the finish.  0 for sizes out of range.  No stage reads scratch that it or an earlier stage of
 * the same call chain did not write. */
int64_t ca_color_match_workspace_bytes(int32_t images, int64_t pixels);

/* hist[image][channel][value] = number of pixels of that image whose channel has that value (uint32 [images][3][256]; zeroed
 * by the call).  Replaces the np.unique(..., return_counts=True) sorts of _hist_match on integer-valued images and the
 * a.min() / a.max() of _minmax in type_norm (vid2vid.py:79-80, :109): per-wave LDS sub-histograms, one integer atomic add per
 * non-empty bin and block. */
int ca_hist_u8x3(const uint8_t* src, uint32_t* hist, int32_t images, int64_t pixels, void* stream);

/* moments[image] = { s00, s01, s02, s11, s12, s22 }, s_ij = sum over the pixels of (lut[image][i][a_i] - mean[image][i]) *
 * (lut[image][j][a_j] - mean[image][j]): np.cov's numerator in _mkl (vid2vid.py:93) for the image whose channel c is
 * lut[image][c][.] applied to the bytes.  lut float64 [images][3][256], mean float64 [images][3], moments float64 [images][6].
 * 64 block partials per image into the workspace, summed in a fixed order by a second launch. */
int ca_color_moments_f64(const uint8_t* src, const double* lut, const double* mean, double* moments, int32_t images,
                         int64_t pixels, void* workspace, int64_t workspace_bytes, void* stream);

/* y[image][j][p] = ((d0 t[image][0][j] + d1 t[image][1][j]) + d2 t[image][2][j]) + my[j], d_i = lut[image][i][a_i] - mean[image][i]:
 * the first histogram match (as the table lut) and `(x - mx) @ t + my` of _mkl (vid2vid.py:83, :103) in one pass.
 * t float64 [images][3][3] row major, my float64 [3] (one reference for all images), y float64 planes [images][3][pixels]. */
int ca_color_transform_f64(const uint8_t* src, const double* lut, const double* mean, const double* t, const double* my,
                           double* y, int32_t images, int64_t pixels, void* stream);

/* sorted[s][0..n) = keys[s][0..n) in ascending order for each of `segments` runs of n float64 keys; finite values come out in
 * np.sort's order (-0.0 before +0.0).  Replaces the np.unique sort of the second _hist_match (vid2vid.py:79), whose input has about as
 * many distinct values as pixels.  LSD radix sort on the order-preserving 64-bit integer image of the double, eight 8-bit
 * passes, each a block histogram, a scan and a stable scatter ranked with 64-lane ballots.  `sorted` may be `keys` (in place);
 * `keys` is otherwise left untouched.  Needs the workspace of ca_color_match_workspace_bytes((segments + 2) / 3, n).
 * 1 <= segments <= 65535. */
int ca_sort_f64_segments(const double* keys, double* sorted, int32_t segments, int64_t n, void* workspace,
                         int64_t workspace_bytes, void* stream);

/* o[image][c][p] = interp(rank / pixels; knots_q[c], knots_val[c]) with rank = the number of values of sorted[image][c] that are <=
 * y[image][c][p] (ties share the upper rank, as np.unique + cumsum give) and numpy's np.interp: the first value below the first
 * knot, the last at or above the last knot, a knot's value on an exact hit, else val[j] + slope_j * (q - q[j]) -- the second
 * _hist_match (vid2vid.py:81-83).  knots_q / knots_val float64 [3][256], knots_n int32 [3] (1 .. 256 knots per channel, q
 * strictly increasing).  `o` may alias `y`, not `sorted`.  Leaves 64 min / max partials of o per plane in the workspace for
 * ca_color_finish_u8. */
int ca_color_rank_map_f64(const double* y, const double* sorted, double* o, const double* knots_q, const double* knots_val,
                          const int32_t* knots_n, int32_t images, int64_t pixels, void* workspace, int64_t workspace_bytes,
                          void* stream);

/* dst[image][p][c] = (uint8) clamp(rint(v * 255), 0, 255), v = normalize ? (o - lo) / (hi - lo) : o, with lo / hi the minimum and
 * maximum of o over the whole image (all channels) as ca_color_rank_map_f64 left them in the same workspace; v = o when hi == lo
 * (_minmax, np.round and np.clip of match_colors, vid2vid.py:139-141).  With normalize = 0 the workspace is not read and may be NULL. */
int ca_color_finish_u8(const double* o, uint8_t* dst, int32_t images, int64_t pixels, int32_t normalize, const void* workspace,
                       int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * ABI v16: the canny annotator of the ControlNet path for a whole window of frames.  The reference annotates every frame on the
 * host with cv2.Canny(img, 100, 200) (modules/controlresiduals_pipeline.py:48-55: 8-bit RGB, aperture 3, L1 gradient norm); the
 * host restatement, which is the specification of these entry points down to its tie rules, is
 * controlanimate_amd/annotators.py: canny_edges.  All arithmetic is int32, so the device result equals the host's byte for byte.
 * Frames are uint8 [images, h, w, channels], channels = 1 or 3; images * h * w < 2^31 (labels are int32 pixel indices).
 * The three stages share one caller-owned workspace and run in the order classify, link, emit on one stream; a fixed set of
 * launches (1 + 3 + 1) with no device-to-host read, so the chain can be captured in a hipGraph.  Nothing in the workspace is
 * assumed: every byte a stage reads was written by an earlier stage of the same chain.  Frames never link to each other.
 * ------------------------------------------------------------------------------------ */

/* Bytes of the workspace for `images` frames of h x w pixels: an int32 label, a class byte and a root flag byte per pixel,
 * rounded up to 256.  0 for sizes out of range.  The workspace must be 16-byte aligned. */
int64_t ca_canny_workspace_bytes(int32_t images, int32_t h, int32_t w);

/* The tile of the kernels (64 x 16 pixels): the sizes at which tests/test_canny_gpu.py places its tile-border cases. */
int32_t ca_canny_tile_w(void);
int32_t ca_canny_tile_h(void);

/* Class byte per pixel into the workspace: 0 none, 1 weak candidate (mag > low), 2 strong (mag > high), for pixels that survive
 * the non-maximum suppression.  One launch: a 64 x 16 tile with a 2-pixel halo goes into LDS through aligned 4-byte loads; Sobel
 * 3x3 with replicated image borders; per pixel the channel with the largest |dx| + |dy| (the first wins ties); the sector test
 * ay < tg22x / ay > tg67x / (dx ^ dy) < 0 with tg22 = 13573 / 2^15 and the host's > / >= pattern, magnitudes outside the image
 * counting as 0.  low / high are the floors of cv2's thresholds; low <= high. */
int ca_canny_classify(const uint8_t* src, int32_t images, int32_t h, int32_t w, int32_t channels, int32_t low, int32_t high,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* Hysteresis as connected-component labelling of the candidates (8-neighbourhood), three launches: union-find per tile in LDS
 * with label = the global pixel index of the tile-local root; unions of the neighbour pairs that straddle a tile border (the
 * diagonal pairs at tile corners included) by atomicMin on the labels; label = root for every candidate, and one flag byte per
 * root that says whether its component holds a strong pixel.  Needs the class bytes of ca_canny_classify in the workspace. */
int ca_canny_link(int32_t images, int32_t h, int32_t w, void* workspace, int64_t workspace_bytes, void* stream);

/* One of the three launches of ca_canny_link, for timing each on its own (tools/bench_canny.py): the stages in the order
 * label, merge, flatten on one stream are ca_canny_link. */
#define CA_CANNY_LINK_LABEL 0
#define CA_CANNY_LINK_MERGE 1
#define CA_CANNY_LINK_FLATTEN 2
int ca_canny_link_stage(int32_t images, int32_t h, int32_t w, void* workspace, int64_t workspace_bytes, int32_t stage, void* stream);

/* edge = candidate whose root is flagged.  Writes either or both of: `edges`, uint8 [images, h, w] with 0 / 255; `control`,
 * [rep * images, 3, h, w] of control_dtype (CA_F16 or CA_F32) with 0.0 / 1.0, the three channels equal and, with
 * rep = 2, the frames written twice (torch.cat([ctrl] * 2) of classifier-free guidance, controlresiduals_pipeline.py:268-269).
 * Needs the workspace as ca_canny_link left it.  rep is 1 or 2. */
int ca_canny_emit(int32_t images, int32_t h, int32_t w, const void* workspace, int64_t workspace_bytes, uint8_t* edges,
                  void* control, int32_t rep, int32_t control_dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * ca_perceiver_attn (added to ABI v16: no struct or existing function changes, the number stays): the attention of the
 * IP-Adapter Plus Resampler (PerceiverAttention, modules/resampler.py:49-78).  For batch b and head h:
 *   Q    = rows 0 .. nq-1 of q + b*q_batch, columns h*64 .. h*64+63
 *   keys = the n_x rows of x + b*x_batch followed by the n_l rows of l + b*l_batch, the same columns; the values are the
 *          same rows x_v_off / l_v_off elements further on
 *   o + b*o_batch, rows 0 .. nq-1, the same columns = softmax_fp32(scale * Q K^T) V  -- ONE softmax over both sources
 * (ca_attention's `accumulate` adds two separately normalised attentions, a different function).  Every tensor has its own row
 * and batch stride in elements.  head_dim == 64, 1 <= nq <= 16, n_x >= 1, n_l >= 1, pointers 16-byte aligned, strides multiples
 * of 8 elements; anything else is CA_ERR_INVALID_ARG before any launch.  One block per (batch, head); the partial softmaxes of
 * its waves are merged in a fixed order, without atomics: two runs give the same bits.
 * ------------------------------------------------------------------------------------ */
typedef struct ca_perceiver_attn_args {
  const void* q; const void* x; const void* l; void* o;
  int64_t q_row, q_batch;
  int64_t x_row, x_batch, x_v_off;
  int64_t l_row, l_batch, l_v_off;
  int64_t o_row, o_batch;
  int32_t batches, heads, head_dim;
  int32_t nq, n_x, n_l;
  float scale;          /* softmax scale (head_dim^-0.5), applied in fp32 to the logits */
  int32_t dtype;
} ca_perceiver_attn_args;
int ca_perceiver_attn(const ca_perceiver_attn_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * The HED edge annotator (added to ABI v16: no struct or existing function changes, the number stays).  The reference's sample
 * config annotates every frame with controlnet_aux's HEDdetector (modules/controlresiduals_pipeline.py:58, 116-117): a VGG-style
 * stack of thirteen 3x3 convolutions with ReLU in five blocks, a 1x1 projection to a one-channel side map per block, a 2x2 max
 * pool between blocks; the side maps are resized to the frame with cv2.resize(INTER_LINEAR), averaged, and squashed by a sigmoid.
 * The convolutions are ca_conv3x3 with act = CA_ACT_RELU; the three entry points below are the stages around them
 * (controlanimate_amd/hed.py: HedAnnotator; the specification is tests/hed_ref.py).  Every launch is a function of its arguments
 * alone, with no device-to-host read: the chain can be captured in a hipGraph.  Anything outside the stated ranges is
 * CA_ERR_INVALID_ARG before any launch.  images * h * w < 2^31 everywhere.
 * ------------------------------------------------------------------------------------ */

/* dst [images, h, w, 8] of dtype (CA_F16 / CA_BF16, 16-byte aligned): channel c < 3 = (float)src[.., c] - norm[c] in fp32, rounded
 * once to dtype; channels 3 .. 7 = 0 (the first convolution's weight is zero-padded to cin = 8).  src uint8 RGB [images, h, w, 3],
 * norm fp32 [3] on the device. */
int ca_hed_prep(const uint8_t* src, const float* norm, void* dst, int32_t images, int32_t h, int32_t w, int32_t dtype, void* stream);

/* One pass over a block's output x [images, h, w, c] (dtype CA_F16 / CA_BF16; c a multiple of 8 in 64 .. 512; h and w even):
 * side [images, h, w] fp32 = proj_bias[0] + sum_c x[p, c] * proj_w[c], accumulated in fp32 (proj_w fp32 [c], proj_bias fp32 [1],
 * both on the device), and, when pooled is not NULL, pooled [images, h / 2, w / 2, c] = the 2x2 / stride-2 maximum.  x, pooled and
 * proj_w 16-byte aligned, side 8-byte aligned.  The sum's order is fixed: two runs give the same bits. */
int ca_hed_pool_side(const void* x, const float* proj_w, const float* proj_bias, float* side, void* pooled, int32_t images, int32_t h,
                     int32_t w, int32_t c, int32_t dtype, void* stream);

/* The five side maps (side_k fp32 [images, h >> k, w >> k]; h and w multiples of 16) -> per output pixel: each map sampled as
 * cv2.resize(INTER_LINEAR) to (h, w) samples float32 (f = (d + 0.5) * src / dst - 0.5, s = floor(f), f -= s; s < 0: s = 0, f = 0;
 * s >= src - 1: s = src - 1, f = 0; weights 1 - f and f in fp32, columns combined first, then rows, every product and sum rounded),
 * the fp32 mean (sum k = 0 .. 4, divided by 5), 1 / (1 + exp(-mean)) in float64, x 255, truncated to uint8.  Writes either or both
 * of: edges, uint8 [images, h, w] (4-byte aligned); control, [rep * images, 3, h, w] of control_dtype (CA_F16 or CA_F32, aligned
 * to four elements) with level / 255, the three channels equal and, with rep = 2, the frames written twice (as ca_canny_emit). */
int ca_hed_fuse(const float* side0, const float* side1, const float* side2, const float* side3, const float* side4, int32_t images,
                int32_t h, int32_t w, uint8_t* edges, void* control, int32_t rep, int32_t control_dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * The lineart annotator (added to ABI v16: no struct or existing function changes, the number stays).  The reference's
 * SampleConfigIPAdapter.yaml annotates frames for control_v11p_sd15_lineart with controlnet_aux's LineartDetector
 * (modules/controlresiduals_pipeline.py:60, 125-129): the "informative drawings" Generator -- a 7x7 convolution behind reflection
 * padding, two stride-2 convolutions, three residual blocks of reflection-padded 3x3 convolutions, two transposed convolutions, a
 * 7x7 convolution to one channel and a sigmoid, with a non-affine InstanceNorm after every convolution but the last.  The stride-2
 * and residual-block convolutions are the 3x3 convolution entry point above; the entry points below are the rest
 * (controlanimate_amd/lineart.py: LineartAnnotator; the specification is tests/lineart_ref.py).  Tensors are NHWC, CA_F16 or CA_BF16.
 * Every launch is a function of its arguments alone, with no device-to-host read and no atomics: the chain can be captured in a
 * hipGraph and two runs give the same bits.  Anything outside the stated ranges is CA_ERR_INVALID_ARG before any launch.
 * ------------------------------------------------------------------------------------ */

/* dst [images, h, w, 64] = Conv2d(3, 64, 7)(ReflectionPad2d(3)(src / 255)) without its bias (a bias in front of a non-affine
 * InstanceNorm cancels).  src uint8 RGB [images, h, w, 3]; w_packed [64][160] of dtype: column ky * 21 + kx * 3 + c holds
 * weight[o][c][ky][kx], columns 147 .. 159 zero.  The sum over the bytes runs in fp32 (MFMA), is divided by 255 and rounded once.
 * h, w >= 4; images * h * w < 2^31; w_packed and dst 16-byte aligned. */
int ca_lineart_conv_in(const uint8_t* src, const void* w_packed, void* dst, int32_t images, int32_t h, int32_t w, int32_t dtype, void* stream);

/* InstanceNorm2d(affine = False) over h x w per (image, channel), biased variance.  x is [images, h, w, c], or, with in_ring = 1,
 * [images, h + 2, w + 2, c] whose outermost pixels are ignored; c is 64, 128 or 256; images * (h + 2) * (w + 2) < 2^31.  The
 * statistics pass writes fp32 partial sums (of x minus the image's first pixel, per chunk of pixels) into `partials`, which holds
 * the number of floats the first function returns (0 for arguments out of range); the apply pass adds them in a fixed order and
 * writes y = relu?((x - mean) / sqrt(var + eps)) + residual?, rounded once.  residual (may be NULL) has x's shape, stored with a
 * ring when res_ring = 1.  With out_pad = 1 y is [images, h + 2, w + 2, c], the result padded by reflection of one pixel
 * (h, w >= 2; the ring is bit-equal to the mirrored interior); else [images, h, w, c].  x, residual and y 16-byte aligned; y must
 * not overlap x or residual. */
int64_t ca_instnorm_partials_floats(int32_t images, int32_t h, int32_t w, int32_t c);
int ca_instnorm_stats(const void* x, float* partials, int32_t images, int32_t h, int32_t w, int32_t c, int32_t in_ring, int32_t dtype, void* stream);
int ca_instnorm_apply(const void* x, const float* partials, const void* residual, void* y, int32_t images, int32_t h, int32_t w, int32_t c,
                      int32_t in_ring, int32_t res_ring, int32_t out_pad, int32_t relu, float eps, int32_t dtype, void* stream);

/* The second half of ConvTranspose2d(cin, cout, 3, stride = 2, padding = 1, output_padding = 1) without bias.  The first half is one
 * GEMM: taps [images * h * w, 9 * cout] = x [images * h * w, cin] times the weight packed as [ky][kx][cout][cin].  This gathers
 * y [images, 2 h, 2 w, cout]: with T(i, j, ky, kx) the cout values of tap (ky, kx) of input pixel (i, j), zero outside the image,
 *   y[2i, 2j] = T(i,j,1,1)                          y[2i, 2j+1] = T(i,j,1,2) + T(i,j+1,1,0)
 *   y[2i+1, 2j] = T(i,j,2,1) + T(i+1,j,0,1)         y[2i+1, 2j+1] = T(i,j,2,2) + T(i,j+1,2,0) + T(i+1,j,0,2) + T(i+1,j+1,0,0)
 * added in fp32 in this order and rounded once.  cout a multiple of 8 up to 1024; images * 2 h * 2 w < 2^31; both 16-byte aligned. */
int ca_convt3x3s2_gather(const void* taps, void* y, int32_t images, int32_t h, int32_t w, int32_t cout, int32_t dtype, void* stream);

/* logits [images, h, w] fp32 = Conv2d(64, 1, 7)(ReflectionPad2d(3)(x)), x [images, h, w, 64] of dtype; wt fp32 [7][7][64]
 * (weight[0][c][ky][kx] at [ky][kx][c]) and bias fp32 [1] on the device; fp32 accumulation in a fixed order.  h, w >= 4;
 * images * h * w < 2^31; x 16-byte aligned. */
int ca_lineart_conv_out(const void* x, const float* wt, const float* bias, float* logits, int32_t images, int32_t h, int32_t w, int32_t dtype,
                        void* stream);

/* Per pixel: level = 255 - trunc(clip(sigmoid(logit) * 255, 0, 255)), the sigmoid in float64.  Writes either or both of: map, uint8
 * [images, h, w] (4-byte aligned); control, [rep * images, 3, h, w] of control_dtype (CA_F16 or CA_F32, aligned to four elements)
 * with level / 255, the three channels equal and, with rep = 2, the frames written twice (the contract of the HED fuse above).
 * h * w a multiple of 4; logits 16-byte aligned. */
int ca_lineart_finish(const float* logits, int32_t images, int32_t h, int32_t w, uint8_t* map, void* control, int32_t rep, int32_t control_dtype,
                      void* stream);

/* ------------------------------------------------------------------------------------
 * The M-LSD straight-line annotator (added to ABI v16: no struct or existing function changes, the number stays).  Every sample
 * config of the reference with ControlNets lists control_v11p_sd15_mlsd, whose frames come from controlnet_aux's MLSDdetector
 * (modules/controlresiduals_pipeline.py:56, 101-105): MobileV2_MLSD_Large (a MobileNetV2 backbone and an FPN-style decoder), a
 * top-200 decode of its centre map and cv2.line.  The stem and the plain 3x3 convolutions are ca_conv3x3 (act = CA_ACT_RELU6 /
 * CA_ACT_RELU), every 1x1 convolution ca_gemm, the ReLU-then-add of the decoder ca_add_bcast; the entry points below are the rest
 * (controlanimate_amd/mlsd.py: MlsdAnnotator; the specification is tests/mlsd_ref.py).  Tensors are NHWC, CA_F16 or CA_BF16.  Every
 * launch is a function of its arguments alone with no device-to-host read: the chain can be captured in a hipGraph, and two runs
 * give the same bits.  Anything outside the stated ranges is CA_ERR_INVALID_ARG before any launch.
 * ------------------------------------------------------------------------------------ */
#define CA_MLSD_TOPK 200

/* dst [images, h, w, 8] of dtype (16-byte aligned): channel c < 3 = src[.., c] / 127.5 - 1 in fp32, rounded once; channel 3 =
 * 1 / 127.5 - 1 (the detector's fourth input channel of ones); channels 4 .. 7 = 0.  src uint8 RGB [images, h, w, 3]. */
int ca_mlsd_prep(const uint8_t* src, void* dst, int32_t images, int32_t h, int32_t w, int32_t dtype, void* stream);

/* Depthwise 3x3 convolution: y[n, oy, ox, ch] = act(bias[ch] + sum_{ky,kx} wt[ky * 3 + kx][ch] * x[n, oy * stride + ky - p, ox * stride + kx - p, ch]),
 * zero outside the image.  stride 1: p = 1, output h x w.  stride 2: p = 0 with one row and column of zeros after the image
 * (F.pad(x, (0, 1, 0, 1)) + Conv2d(padding = 0)), h and w even, output h / 2 x w / 2.  wt [9][c] of dtype, bias fp32 [c];
 * relu6 = 1 clamps to [0, 6].  c a multiple of 8 in 16 .. 576; fp32 accumulation, rounded once; x, wt, y 16-byte aligned. */
int ca_dwconv3x3(const void* x, const void* wt, const float* bias, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t stride,
                 int32_t relu6, int32_t dtype, void* stream);

/* Bilinear x2 upsampling with align_corners = True (F.interpolate): x [images, h, w, c] -> columns col0 .. col0 + c - 1 of
 * y [images, 2 h, 2 w, ld]; the other columns of y are never touched (one half of a channel concatenation).  Per axis
 * src = dst * (in - 1) / (out - 1) in fp32 (the integer product divided once), i0 = trunc(src), f = src - i0; the columns are combined
 * first (a * (1 - f) + b * f), then the rows, in fp32, rounded once.  c, ld and col0 multiples of 8; both 16-byte aligned. */
int ca_upsample2x_bilinear_ac(const void* x, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int64_t ld, int32_t col0, int32_t dtype,
                              void* stream);

/* y [images, h, w, 64] = act(bias + Conv2d(64, 64, 3, dilation = 5, padding = 5)(x)), x [images, h, w, 64]; wt [64][3][3][64]
 * (the layout of ca_conv_args.w) of dtype, bias fp32 [64]; relu = 1: max(., 0).  c must be 64 and dilation 5 (what the kernel is built
 * for).  MFMA with fp32 accumulation, rounded once.  x, wt, y 16-byte aligned; y must not be x. */
int ca_conv3x3_dil(const void* x, const void* wt, const float* bias, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t dilation,
                   int32_t relu, int32_t dtype, void* stream);

/* tp fp32 [images, h, w, 8]: channel 0 the centre logit, channels 1 .. 4 the displacements (dx_s, dy_s, dx_e, dy_e), 5 .. 7 unused.
 * heat = 1 / (1 + exp(-logit)) in fp32; a pixel is a candidate when heat > thr_v and no 3x3 neighbour inside the map has a larger heat
 * (plateaus keep every pixel).  The CA_MLSD_TOPK candidates first by (heat descending, flat index ascending) are the points; a point
 * with sqrt((dx_s - dx_e)^2 + (dy_s - dy_e)^2) > thr_d (fp32) is a line -- a dropped point is not replaced.  segments int32
 * [images, CA_MLSD_TOPK, 4] = (xs, ys, xe, ye) = trunc(2 * (x + dx_s)), ... in float64, pinned to +-2^30, in rank order, the unused tail
 * zero; count int32 [images].  workspace: ca_mlsd_decode_workspace_bytes bytes (the candidate list, h * w keys per image: a saturated
 * plateau cannot overflow it; 0 for sizes out of range), 8-byte aligned.  0 <= thr_v < 1, thr_d >= 0. */
int64_t ca_mlsd_decode_workspace_bytes(int32_t images, int32_t h, int32_t w);
int ca_mlsd_decode(const float* tp, int32_t images, int32_t h, int32_t w, float thr_v, float thr_d, void* workspace, int64_t workspace_bytes,
                   int32_t* segments, int32_t* count, void* stream);

/* map uint8 [images, h, w] = zeros, then cv2.line(map, (xs, ys), (xe, ye), 255, 1) for the first min(count, CA_MLSD_TOPK) segments of
 * every image: OpenCV's clipLine to the image and its 8-connected left-to-right line iterator.  With control != NULL also
 * control [rep * images, 3, h, w] of control_dtype (CA_F16 or CA_F32, aligned to four elements) = map / 255, the three channels equal
 * and, with rep = 2, the frames written twice (the contract of ca_canny_emit).  h * w a multiple of 4; map 4-byte aligned. */
int ca_mlsd_draw(const int32_t* segments, const int32_t* count, int32_t images, int32_t h, int32_t w, uint8_t* map, void* control, int32_t rep,
                 int32_t control_dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * The softedge annotator (added to ABI v16: no struct or existing function changes, the number stays).  The reference's
 * SampleConfigIPAdapter.yaml lists control_v11p_sd15_softedge, whose frames come from controlnet_aux's PidiNetDetector
 * (modules/controlresiduals_pipeline.py:62, 134-138): PiDiNet(60, carv4, dil = 24, sa = True) -- fifteen blocks of a depthwise
 * pixel-difference convolution, ReLU, a 1x1 convolution and a skip at four resolutions, and per resolution a CDCM (ReLU, 1x1, four
 * dilated 3x3 convolutions summed), a CSAM (a one-channel spatial attention) and a 1x1 reduction to a side map; the four side maps
 * are resized to the frame, mixed by a 1x1 classifier and passed through a sigmoid.  The pixel-difference operators are linear and
 * are folded into plain 3x3 / 5x5 kernels on the host; channels are zero-padded to 64 / 128 / 256 / 32.  The init_block is
 * ca_conv3x3, every 1x1 convolution ca_gemm; the entry points below are the rest (controlanimate_amd/softedge.py: SoftedgeAnnotator;
 * the specification is tests/softedge_ref.py).  Tensors are NHWC, CA_F16 or CA_BF16.  Every launch is a function of its arguments
 * alone, with no device-to-host read and no atomics: the chain can be captured in a hipGraph and two runs give the same bits.
 * Anything outside the stated ranges is CA_ERR_INVALID_ARG before any launch.  images * h * w < 2^31 everywhere.
 * ------------------------------------------------------------------------------------ */

/* dst [images, h, w, 8] of dtype (16-byte aligned): channel c < 3 = src[.., c] / 255 in fp32, rounded once; channels 3 .. 7 = 0
 * (the init_block's weight is zero-padded to 8 input channels).  src uint8 RGB [images, h, w, 3]. */
int ca_softedge_prep(const uint8_t* src, void* dst, int32_t images, int32_t h, int32_t w, int32_t dtype, void* stream);

/* y = max(x, 0) over numel elements of dtype (numel a multiple of 8; both 16-byte aligned; y may be x): the ReLU in front of a
 * CDCM's 1x1 convolution, which is no epilogue of the block that produced x (the next block reads x itself). */
int ca_relu(const void* x, void* y, int64_t numel, int32_t dtype, void* stream);

/* Depthwise ksize x ksize convolution, stride 1, padding ksize / 2, no bias:
 * y[n, oy, ox, ch] = act(sum_{ky,kx} wt[ky * ksize + kx][ch] * x[n, oy + ky - p, ox + kx - p, ch]), zero outside the image.
 * ksize is 3 or 5; wt [ksize * ksize][c] of dtype; relu = 1: max(., 0); c a multiple of 8 up to 256.  The fp32 sum has a fixed
 * order -- kernel rows ascending, inside a row w0 * v0 and then fma over the columns ascending, each row's sum added to the total --
 * and is rounded once.  x, wt, y 16-byte aligned; y must not overlap x.  (ca_dwconv3x3 is the form with a bias, ReLU6 and stride 2.) */
int ca_dwconv_k(const void* x, const void* wt, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t ksize, int32_t relu, int32_t dtype,
                void* stream);

/* y [images, h / 2, w / 2, c] = the 2x2 / stride-2 maximum of x [images, h, w, c]; h and w even, c a multiple of 8 up to 1024;
 * both 16-byte aligned. */
int ca_maxpool2x2(const void* x, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t dtype, void* stream);

/* A stride-1 block of the network in one launch: y = x + W2 . relu(dw(x)), x and y [images, h, w, c]; dw is the depthwise
 * convolution of ca_dwconv_k with the same wt_dw [ksize * ksize][c] (ksize 3 or 5) and the same order of operations, its result
 * rounded once to dtype (where the two-launch form, ca_dwconv_k and then ca_gemm with residual = x, stores it); w2 [c][c] of dtype
 * ([cout][cin]) multiplies it on the MFMA with fp32 accumulation; the product is rounded to dtype, x added in fp32 and the sum rounded
 * (the two roundings of ca_gemm's residual epilogue, which are those of an fp16 pipeline: conv2's output, then + x).  c must be 64
 * (ca_pdc_block_supported(c, ksize) != 0: no launch, no device access; other widths run as the two launches).  x is read once
 * plus a halo of ksize / 2 pixels around every 16 x 16 tile, y written once.  All four 16-byte aligned; y must not overlap x. */
int ca_pdc_block_supported(int32_t c, int32_t ksize);
int ca_pdc_block(const void* x, const void* wt_dw, const void* w2, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t ksize, int32_t dtype,
                 void* stream);

/* y [images, h, w, 32] = sum over d in (5, 7, 9, 11) of Conv2d(32, 32, 3, dilation = d, padding = d, bias = False)(x), zero outside
 * the image, as one MFMA accumulation over K = 4 * 9 * 32 in fp32, rounded once.  wt [4][32][3][3][32] of dtype: [dilation index]
 * [cout][ky][kx][cin].  c must be 32.  Maps smaller than a dilation are legal (the taps that miss the map add nothing).  x, wt, y
 * 16-byte aligned; y must not overlap x. */
int ca_cdcm_dil4(const void* x, const void* wt, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t dtype, void* stream);

/* The CSAM and the 1x1 reduction behind it, from f [images, h, w, 32] of dtype (c must be 32), in two launches:
 *   t[p, j] = b1[j] + sum_c w1[j][c] * max(f[p, c], 0)   (j < 4)   and   r[p] = sum_c wr[c] * f[p, c],   fp32, c ascending, fma;
 *   side[p] = br[0] + sigmoid(sum_{ky,kx,j} w2[ky][kx][j] * t[p + (ky - 1, kx - 1), j]) * r[p],  zero outside the image, fp32.
 * The attention is one scalar per pixel, so wr . (f * a) = a * (wr . f): the 32-channel product is never written.  w1 fp32 [4][32],
 * b1 fp32 [4], w2 fp32 [3][3][4], wr fp32 [32], br fp32 [1] on the device; t fp32 [images, h, w, 4] (16-byte aligned) and r fp32
 * [images, h, w] are scratch, side fp32 [images, h, w]; t, r and side must not overlap.  f 16-byte aligned. */
int ca_csam_reduce(const void* f, const float* w1, const float* b1, const float* w2, const float* wr, const float* br, float* t, float* r, float* side,
                   int32_t images, int32_t h, int32_t w, int32_t c, int32_t dtype, void* stream);

/* The four side maps (side_k fp32 [images, h >> k, w >> k]; h and w multiples of 8) -> per output pixel: each map sampled as
 * F.interpolate(mode = "bilinear", align_corners = False) to (h, w) samples it (per axis src = max((d + 0.5) * in / out - 0.5, 0),
 * i0 = trunc(src), i1 = min(i0 + 1, in - 1), l1 = src - i0, l0 = 1 - l1 in fp32; columns first, l0 * a + l1 * b, then rows, every
 * product and sum rounded; level 0 is the value itself), z = classifier[4] + sum_k classifier[k] * e_k added for k = 0 .. 3 in
 * fp32, edge = 1 / (1 + expf(-z)) in fp32, with safe = 1 edge = trunc(edge * 3) / 2, then trunc(clip(edge * 255, 0, 255)).
 * classifier fp32 [5] on the device (the four weights, then the bias).  Writes any of: logit fp32 [images, h, w] = z (16-byte
 * aligned); edges, uint8 [images, h, w] (4-byte aligned); control, [rep * images, 3, h, w] of control_dtype (CA_F16 or CA_F32,
 * aligned to four elements) with level / 255, the three channels equal and, with rep = 2, the frames written twice (the contract of
 * ca_hed_fuse). */
int ca_softedge_fuse(const float* side0, const float* side1, const float* side2, const float* side3, const float* classifier, int32_t images, int32_t h,
                     int32_t w, int32_t safe, float* logit, uint8_t* edges, void* control, int32_t rep, int32_t control_dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * The lineart_anime annotator (added to ABI v16: no struct or existing function changes, the number stays).  Every sample config of
 * the reference lists control_v11p_sd15s2_lineart_anime, whose frames come from controlnet_aux's LineartAnimeDetector
 * (modules/controlresiduals_pipeline.py:59, 119-123): the pix2pix UnetGenerator(3, 1, num_downs = 8, ngf = 64) with a non-affine
 * InstanceNorm -- eight 4x4 stride-2 convolutions down to 1/256 of the frame, eight 4x4 stride-2 transposed convolutions back up
 * over skip concatenations, and a tanh.  None of the entry points above runs these layers; the ones below do
 * (controlanimate_amd/lineart_anime.py: LineartAnimeAnnotator; the specification is tests/lineart_anime_ref.py).  Tensors are NHWC,
 * CA_F16 or CA_BF16, with fp32 accumulation.  Every activation is stored in the form its consumers read: L_i = LeakyReLU(0.2)(d_i)
 * for the next convolution down, and a concatenation buffer C_i [images, h_i, w_i, 2 c_i] = (ReLU(d_i), ReLU(IN(up_{i+1}))) for the
 * transposed convolution up, so no MFMA operand path applies an activation.  Every launch is a function of its arguments alone,
 * with no device-to-host read and no atomics: the chain can be captured in a hipGraph and two runs give the same bits.  Anything
 * outside the stated ranges is CA_ERR_INVALID_ARG before any launch.  No operand may reach 2^31 bytes.
 * ------------------------------------------------------------------------------------ */

/* d0 = Conv2d(3, 64, 4, stride 2, padding 1)(src / 127.5 - 1) + bias, the zero padding applied to the NORMALISED image: over the taps
 * inside the frame, (sum w * byte) / 127.5 - sum w, both sums in fp32 (MFMA).  src uint8 RGB [images, h, w, 3], h and w even;
 * w_packed [64][64] of dtype: column ky * 12 + kx * 3 + c holds weight[o][c][ky][kx], columns 48 .. 63 zero; bias fp32 [64].
 * Writes l0 [images, h / 2, w / 2, 64] = LeakyReLU(0.2)(d0) and channels 0 .. 63 of c0 [images, h / 2, w / 2, 128] = ReLU(d0);
 * channels 64 .. 127 of c0 are not touched.  w_packed, l0 and c0 16-byte aligned. */
int ca_lanime_conv_in(const uint8_t* src, const void* w_packed, const float* bias, void* l0, void* c0, int32_t images, int32_t h, int32_t w,
                      int32_t dtype, void* stream);

/* y [images, h / 2, w / 2, cout] = Conv2d(cin, cout, 4, stride 2, padding 1)(x), x [images, h, w, cin] with h and w even, zero
 * outside the image; wt [cout][4][4][cin] of dtype.  cin is 64, 128, 256 or 512; cout 128, 256 or 512.  bias (fp32 [cout], may be
 * NULL) is added and, with relu = 1, max(., 0) applied before the one rounding.  An implicit GEMM on the MFMA whose B operand is
 * read from an LDS tile of the input (8 x 16 output pixels x 128 output channels per block): no im2col tensor is written.
 * x, wt, y 16-byte aligned; y must not overlap x. */
int ca_conv4x4s2(const void* x, const void* wt, const float* bias, void* y, int32_t images, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t relu,
                 int32_t dtype, void* stream);

/* The gather in front of ca_gemm for the levels of that convolution with few output rows (they are bound by their 8 MB of weights,
 * and ca_gemm splits K): cols [images * h / 2 * w / 2][16 * cin], column (ky * 4 + kx) * cin + ci of row (image, oy, ox) =
 * x[image, 2 oy - 1 + ky, 2 ox - 1 + kx, ci], zero outside the image -- the row order of wt above, so that
 * y = ca_gemm(cols, wt as [cout][16 * cin]).  cin a multiple of 8 up to 1024, h and w even.  Both 16-byte aligned. */
int ca_im2col4x4s2(const void* x, void* cols, int32_t images, int32_t h, int32_t w, int32_t cin, int32_t dtype, void* stream);

/* y [images, 2 h, 2 w, cout] = ConvTranspose2d(cin, cout, 4, stride 2, padding 1)(x) without bias, x [images, h, w, cin], as four
 * 2x2 "phase" convolutions in ONE launch: output pixel (2 y + py, 2 x + px) = sum over dy, dx in {0, 1} of
 * w_phase[py * 2 + px][.][dy][dx][.] . x[y + py - 1 + dy, x + px - 1 + dx], zero outside the image, where
 * w_phase [4][cout][2][2][cin] of dtype holds weight[ci][co][3 - py - 2 dy][3 - px - 2 dx] (lineart_anime.pack_convt4x4_phases; the
 * layout of ca_conv_up2_phase's weight).  cin is 256, 512 or 1024; cout 64, 128, 256 or 512.  No zero-stuffed tensor and no tap
 * tensor is written.  x, w_phase, y 16-byte aligned; y must not overlap x. */
int ca_convt4x4s2(const void* x, const void* w_phase, void* y, int32_t images, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t dtype, void* stream);

/* InstanceNorm2d(affine = False) over h x w (from 1 x 1 upward) per (image, channel) of x [images, h, w, c], biased variance, c = 64,
 * 128, 256 or 512, written to up to two outputs (y1 may be NULL): y_k[(image, pixel) * stride_k + off_k + channel] =
 * act_k((x - mean) / sqrt(var + eps)), act 0 = none, 1 = ReLU, 2 = LeakyReLU(0.2); off_k and stride_k are multiples of 8 with
 * off_k + c <= stride_k <= 4096, and the other channels of a destination are not touched -- one pass fills L_i and a half of C_i.
 * fp32 statistics in a fixed order (of x minus the image's first pixel, per chunk of pixels, through `partials`, which holds the
 * number of floats the first function returns, 0 for arguments out of range).  A chunk is 262144 / c pixels, halved down to
 * 16384 / c while the launch has fewer than 256 blocks -- a function of the arguments alone.  A plane of one chunk runs as ONE
 * launch, larger ones as two.  x, y0, y1 16-byte aligned; the outputs must not overlap x. */
int64_t ca_instnorm_act_partials_floats(int32_t images, int32_t h, int32_t w, int32_t c);
int ca_instnorm_act(const void* x, float* partials, void* y0, int32_t act0, int32_t off0, int32_t stride0, void* y1, int32_t act1, int32_t off1, int32_t stride1,
                    int32_t images, int32_t h, int32_t w, int32_t c, float eps, int32_t dtype, void* stream);

/* out fp32 [images, 2 h, 2 w] = ConvTranspose2d(128, 1, 4, stride 2, padding 1)(x) + bias, x [images, h, w, 128] of dtype (the
 * concatenation buffer C_0); wt fp32 [4][4][128] (weight[c][0][ky][kx] at [ky][kx][c]) and bias fp32 [1] on the device; fp32
 * accumulation in a fixed order on the VALU (512 terms per output).  x 16-byte aligned, out 8-byte aligned. */
int ca_lanime_conv_out(const void* x, const float* wt, const float* bias, float* out, int32_t images, int32_t h, int32_t w, int32_t dtype, void* stream);

/* Per pixel: level = 255 - trunc(clip(tanh(t) * 127.5 + 127.5, 0, 255)), the tanh in float64.  Writes either or both of: map, uint8
 * [images, h, w] (4-byte aligned); control, [rep * images, 3, h, w] of control_dtype (CA_F16 or CA_F32, aligned to four elements)
 * with level / 255, the three channels equal and, with rep = 2, the frames written twice (the contract of ca_lineart_finish).
 * h * w a multiple of 4; pre 16-byte aligned. */
int ca_lanime_finish(const float* pre, int32_t images, int32_t h, int32_t w, uint8_t* map, void* control, int32_t rep, int32_t control_dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * The GFPGAN face restorer for aligned faces (added to ABI v16: no struct or existing function changes, the number stays).  Three
 * of the reference's sample configs set use_face_enhancer, and every emitted frame then passes through
 * GFPGANer(arch='clean', channel_multiplier=2).enhance (modules/upscaler.py:53-70): GFPGANv1Clean, a U-Net whose features modulate
 * (SFT) a StyleGAN2 decoder.  The U-Net's and the SFT branches' 3x3 convolutions are ca_conv3x3 (act = CA_ACT_LEAKY02), its 1x1
 * skips and final_linear ca_gemm; the entry points below are the rest (controlanimate_amd/gfpgan.py: FaceRestorer; the
 * specification is tests/gfpgan_ref.py).  Tensors are NHWC, CA_F16 or CA_BF16, with fp32 accumulation.
 *
 * The modulated convolution keeps ONE weight for the whole batch:
 *     modconv(x, style)[n, o] = demod[n, o] * conv(W, s[n, i] * x),   demod[n, o] = rsqrt(sum_i s[n, i]^2 Wsq[o, i] + 1e-8),
 * Wsq[o, i] = sum over the taps of W[o, i]^2, packed once.  s is divided by its per-image largest magnitude m, and
 * demod' = rsqrt(sum (s / m)^2 Wsq + 1e-8 / m^2) = m * demod: the product is unchanged and (s / m) * x stays inside fp16's range.
 *
 * Every launch is a function of its arguments alone, with no device-to-host read and no atomics: the chain can be captured in a
 * hipGraph and two runs give the same bits.  Anything outside the stated ranges is CA_ERR_INVALID_ARG before any launch.  No operand
 * may reach 2^31 bytes.  The bilinear resamplings are torch's align_corners = False ones at scale 2 (weights 0.25 / 0.75, the index
 * clamped at the edges, h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d) in fp32 without contraction) and 1/2 (the 2x2 mean).
 * ------------------------------------------------------------------------------------ */

/* y [images, h, w, cout] = LeakyReLU(0.2)(conv_body_first(v)), v[c] = (src[c'] / 255 - 0.5) / 0.5 with c' = 2 - c when
 * reverse_channels (GFPGANer.enhance takes BGR and swaps; the reference hands it RGB), else c.  src uint8 [images, h, w, 3];
 * wt fp32 [cout][3], bias fp32 [cout]; cout a multiple of 8 up to 256.  On the VALU.  y 16-byte aligned. */
int ca_gfp_prep(const uint8_t* src, const float* wt, const float* bias, void* y, int32_t images, int32_t h, int32_t w, int32_t cout,
                int32_t reverse_channels, int32_t dtype, void* stream);

/* The bilinear resize of x [images, h, w, c] by 2 (up = 1: y [images, 2 h, 2 w, c]) or by 1/2 (up = 0, h and w even:
 * y [images, h / 2, w / 2, c]), c a multiple of 8 up to 4096; fp32 arithmetic, one rounding.  x, y 16-byte aligned. */
int ca_resample2x(const void* x, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t up, int32_t dtype, void* stream);

/* One launch for every modulated layer of the decoder.  Layer l is described by six host integers desc[6 l ..]:
 * (latent index, cin, cout, w_off, wsq_off, out_off).  With lat = latents[image][latent index] (fp32 [images][num_latent][512]):
 *     s[i] = sum_k lat[k] * params[w_off + k * cin + i] + params[w_off + 512 * cin + i]     (the modulation Linear, transposed, then its bias)
 * cout > 0 (a StyleConv):  m = max |s| (at least 1e-20);  out[image * out_stride + out_off + i] = s[i] / m;
 *     out[.. + cin + o] = 1 / sqrt(sum_i (s[i] / m)^2 * params[wsq_off + i * cout + o] + 1e-8 / m^2)
 * cout = 0 (a ToRGB, which does not demodulate): out[.. + i] = s[i].
 * cin and cout are 64, 128, 256 or 512, at most 32 layers; all sums fp32 in index order.  The offsets are checked against
 * params_floats and out_stride. */
int ca_gfp_styles(const float* latents, const float* params, int64_t params_floats, const int32_t* desc, int32_t layers, float* out, int64_t out_stride,
                  int32_t images, int32_t num_latent, void* stream);

/* One StyleConv in one launch:
 *     v = acc * demod[image][o] * sqrt(2) + noise_weight * noise[image][y][x] + bias[o],   acc = conv3x3(wt, s[image][i] * X)
 *     v = LeakyReLU(0.2)(v);   o >= cout / 2 and sft_scale:  v = v * sft_scale[image][y][x][o - cout / 2] + sft_shift[..]
 * X = x, or with upsample = 1 the bilinear x2 of x, computed from the low-resolution halo in LDS (the 2h x 2w input never exists in
 * memory); zero outside the plane.  An implicit GEMM on 16x16x32 MFMAs from an LDS halo tile (8 x 16 output pixels x 128 or 64
 * output channels per block), the input-channel scale applied while the tile is staged (one rounding of s * X).  x [images, h, w, cin],
 * or ONE image shared by all (x_shared = 1: the decoder's constant); wt [cout][3][3][cin] of dtype; s fp32, image n at s + n * s_stride,
 * demod fp32, image n at demod + n * demod_stride (ca_gfp_styles' output); noise fp32 [images, H, W] with H x W the output plane; bias fp32 [cout];
 * sft_scale / sft_shift [images, H, W, cout / 2] of dtype, both or neither; y [images, H, W, cout].  cin and cout are 64, 128, 256 or
 * 512; planes from 1 x 1 (smaller than a tile: handled by bounds).  x, wt, y, sft_* 16-byte aligned; y must not overlap x. */
typedef struct ca_modconv_args {
  const void* x;
  const void* wt;
  const float* s;
  const float* demod;
  const float* noise;
  const float* bias;
  const void* sft_scale;
  const void* sft_shift;
  void* y;
  int64_t s_stride, demod_stride;
  int32_t images, h, w, cin, cout;
  int32_t upsample, x_shared;
  float noise_weight;
  int32_t dtype;
} ca_modconv_args;
int ca_modconv3x3(const ca_modconv_args* args, void* stream);

/* The same StyleConv composed of three launches, for the planes where ca_conv3x3's tiles beat the one-launch kernel
 * (kernels.modconv3x3 picks by the output plane):
 *     y1 = ca_gfp_modulate:        round(s[image][i] * X), X = x [images, h, w, c] (ONE image with x_shared = 1) or, with upsample = 1, its
 *                                  bilinear x2: [images, H, W, c] -- the staging of ca_modconv3x3 as a pass of its own
 *     t  = ca_conv3x3(y1, wt):     no bias, no activation, and NO workspace, so that K is never split: an output's sum then has the same
 *                                  order whatever the batch, and a batch split across passes gives the same bits
 *     y  = ca_gfp_style_epilogue:  LeakyReLU(0.2)(t * demod[image][o] * sqrt(2) + noise_weight * noise[image][y][x] + bias[o]), then SFT on the
 *                                  channels >= c / 2 as in ca_modconv3x3; y may be t.  t carries one rounding more than the accumulator.
 * c is 64, 128, 256 or 512; x, y, t, sft_* 16-byte aligned; ca_gfp_modulate's y must not be x. */
int ca_gfp_modulate(const void* x, const float* s, int64_t s_stride, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t upsample,
                    int32_t x_shared, int32_t dtype, void* stream);
int ca_gfp_style_epilogue(const void* t, const float* demod, int64_t demod_stride, const float* noise, float noise_weight, const float* bias,
                          const void* sft_scale, const void* sft_shift, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t dtype, void* stream);

/* ToRGB: out fp32 [images, h, w, 3] = sum_i wt[c][i] * s[image][i] * x[image, y, x, i] + bias[c] + the bilinear x2 of prev
 * (fp32 [images, h / 2, w / 2, 3], may be NULL; h and w even then).  x [images, h, w, cin] of dtype, cin 64 .. 512; wt fp32 [3][cin];
 * s fp32, image n at s + n * s_stride (not demodulated, not scaled).  On the VALU: the per-image wt * s lies in LDS, the sum runs in
 * fp32 in channel order.  x 16-byte aligned. */
int ca_gfp_to_rgb(const void* x, const float* wt, const float* s, int64_t s_stride, const float* bias, const float* prev, float* out, int32_t images,
                  int32_t h, int32_t w, int32_t cin, int32_t dtype, void* stream);

/* tensor2img(rgb2bgr, min_max = (-1, 1)): out uint8 [images * pixels][3], channel 2 - c when reverse_channels, =
 * rint(((clamp(pre, -1, 1) + 1) / 2) * 255) in fp32, half to even (a NaN counts as -1).  pre fp32 [images * pixels][3]. */
int ca_gfp_finish(const float* pre, uint8_t* out, int64_t pixels, int32_t reverse_channels, void* stream);

/* ---- added to ABI v16: the depth annotator's stages beside ca_gemm / ca_attention / ca_conv3x3 (controlanimate_amd/depth.py) ---- */

/* Pillow's Image.resize of uint8 RGB frames src [images, sh, sw, 3] -> dst [images, dh, dw, 3], as Resample.c runs it for 8-bit pixels: a
 * horizontal pass into tmp [images, sh, dw, 3], then a vertical one.  Output index i of a pass reads the bounds[2 i + 1] source samples from
 * bounds[2 i] on through the int32 coefficients coef[i * ksize ..] (22 fractional bits), adds 2^21, shifts by 22 and clips to 0 .. 255.  The
 * tables are device memory, built by the host (depth.pil_coeffs); the bounds are clamped to the source.  Two launches. */
int ca_resize_pil_u8(const uint8_t* src, uint8_t* tmp, uint8_t* dst, int32_t images, int32_t sh, int32_t sw, int32_t dh, int32_t dw, const int32_t* xbounds,
                     const int32_t* xcoef, int32_t xksize, const int32_t* ybounds, const int32_t* ycoef, int32_t yksize, void* stream);

/* uint8 RGB src [images, size, size, 3] -> out [images * (size / patch)^2][3 * patch * patch] of dtype: (src / 255 - 0.5) / 0.5, column
 * (c * patch + ky) * patch + kx -- the flattening of a Conv2d(3, C, patch, stride patch) weight.  patch a multiple of 8. */
int ca_dpt_patches(const uint8_t* src, void* out, int32_t images, int32_t size, int32_t patch, int32_t dtype, void* stream);

/* The scatter behind ConvTranspose2d(kernel = stride = k) run as a GEMM with N = k * k * cout: y [images, gh * k, gw * k, cout] pixel
 * (sy * k + ky, sx * k + kx) = columns (ky * k + kx) * cout .. of row image * rows_per_image + row0 + sy * gw + sx of x (row stride ldx
 * elements).  k is 1 (a gather of rows into a contiguous plane), 2 or 4; cout a multiple of 8; both 16-byte aligned. */
int ca_depth_to_space(const void* x, void* y, int32_t images, int32_t gh, int32_t gw, int32_t k, int32_t cout, int64_t ldx, int32_t rows_per_image,
                      int32_t row0, int32_t dtype, void* stream);

/* The tail of the DPT depth head in one launch: out fp32 [images, 2h, 2w] =
 *     max(sum_c w3[c] * max(conv3x3(w2, U)[c] + b2[c], 0) + b3, 0),   U = the align-corners bilinear x2 of x [images, h, w, cmid] of dtype,
 * rounded to dtype as ca_upsample2x_bilinear_ac rounds it and zero outside the 2h x 2w plane.  U is never written.  w2 [32][3][3][cmid] of
 * dtype, b2 fp32 [32], w3 fp32 [32], b3 fp32 [1].  cmid is 32, 64 or 128 (ca_dpt_head_supported: no launch); x and w2 16-byte aligned. */
int ca_dpt_head_supported(int32_t cmid);
int ca_dpt_head(const void* x, const void* w2, const float* b2, const float* w3, const float* b3, float* out, int32_t images, int32_t h, int32_t w,
                int32_t cmid, int32_t dtype, void* stream);
/* The last step of the same head composed of ca_upsample2x_bilinear_ac + ca_conv3x3(CA_ACT_RELU, out_f32): out[p] =
 * max(sum_c w3[c] * t[p][c] + b3, 0) over t fp32 [pixels][32]. */
int ca_dpt_logit(const float* t, const float* w3, const float* b3, float* out, int64_t pixels, void* stream);

/* torch's interpolate(mode = "bicubic", align_corners = False) of fp32 planes src [images, sh, sw] -> dst [images, dh, dw] (A = -0.75,
 * clamped indices, no antialias), and the per-image maximum and minimum of dst: minmax_keys receives 2 * images uint32 (max, min) in an
 * order-preserving encoding (what ca_depth_finish reads), minmax (may be NULL) the same as fp32.  Two or three launches. */
int ca_resize_bicubic_f32(const float* src, float* dst, void* minmax_keys, float* minmax, int32_t images, int32_t sh, int32_t sw, int32_t dh, int32_t dw,
                          void* stream);

/* depth fp32 [images, h, w] and ca_resize_bicubic_f32's minmax_keys -> the uint8 map [images, h, w] (may be NULL) and / or the control
 * tensor [rep * images, 3, h, w] of control_dtype (CA_F32 / CA_F16; map / 255, three equal channels, the frames written rep = 1 or 2 times).
 * mode 0: d * 255 / max;  mode 1: (d - min) / (max - min) * 255; fp32, operation for operation, truncated toward zero.  A value <= -1
 * saturates to 0, a NaN counts as 0; max <= 0 (mode 0) or max <= min (mode 1) gives an all-zero map. */
int ca_depth_finish(const float* depth, const void* minmax_keys, int32_t images, int32_t h, int32_t w, int32_t mode, uint8_t* map, void* control, int32_t rep,
                    int32_t control_dtype, void* stream);

/* ---- added to ABI v16 (no struct or existing function changes, the number stays): the OpenPose body annotator's stages beside
 * ca_conv3x3 / ca_maxpool2x2 / ca_gemm (controlanimate_amd/openpose.py; csrc/ca_openpose.hip) ---- */
#define CA_POSE_MAX_PEAKS 64        /* peaks kept per part and frame: the first ones in row-major order */
#define CA_POSE_MAX_PEOPLE 64       /* rows of the subset table */
#define CA_POSE_AREA_TAPS 8         /* taps per axis of ca_pose_prep's tables */
#define CA_POSE_OVERFLOW_PEAKS 1    /* bits of overflow[frame] */
#define CA_POSE_OVERFLOW_PEOPLE 2

/* uint8 RGB frames [images, h, w, 3] -> out [images, hp, wp, 8] of dtype: the INTER_AREA resize to hs x ws as a separable weighted sum
 * (per destination index of an axis: first source index ofs, number of taps cnt <= CA_POSE_AREA_TAPS, fp32 weights w [.., CA_POSE_AREA_TAPS];
 * horizontal sums first, left to right, then their vertical sum, top to bottom, fp32, no fused multiply-add; rounded to a byte half to
 * even), channels in BGR order, byte / 256 - 0.5; the pixels right of ws and below hs (the constant-128 padding) and channels 3 .. 7
 * are zero. */
int ca_pose_prep(const uint8_t* frames, void* out, const int32_t* xofs, const int32_t* xcnt, const float* xw, const int32_t* yofs, const int32_t* ycnt,
                 const float* yw, int32_t images, int32_t h, int32_t w, int32_t hs, int32_t ws, int32_t hp, int32_t wp, int32_t dtype, void* stream);

/* Conv2d(cin, cout, 7, stride 1, padding 3) of NHWC x [images, h, w_px, cin] (a pixel every ldx elements) into y (a pixel every ldy
 * elements) for `groups` = 1 or 2 independent problems of one shape in ONE launch; w [cout, 7, 7, cin] of dtype, fp32 bias (may be NULL),
 * optional ReLU; fp32 accumulation over (32-channel chunk, tap, channel), rounded once.  An implicit GEMM on MFMA 16x16x32 from an LDS
 * halo tile; no im2col tensor, no split of the reduction: an image's result does not depend on the batch.  cin % 32 == 0, cout % 64 == 0. */
typedef struct {
  const void* x[2];
  const void* w[2];
  const float* bias[2];
  void* y[2];
  int64_t ldx, ldy;
  int32_t groups, images, h, w_px, cin, cout, relu, dtype;
} ca_conv7x7_args;
int ca_conv7x7(const ca_conv7x7_args* args, void* stream);

/* The gather in front of ca_gemm for the same convolution: cols [images * h * w, 49 * cin], column (ky * 7 + kx) * cin + ci of row
 * (img, oy, ox) = x[img, oy - 3 + ky, ox - 3 + kx, ci], zero outside the image. */
int ca_im2col7x7(const void* x, void* cols, int32_t images, int32_t h, int32_t w, int32_t cin, int64_t ldx, int32_t dtype, void* stream);

/* src [rows, c] -> columns col0 .. col0 + c - 1 of dst [rows, ld] (16-bit elements; c, col0 and ld multiples of 8). */
int ca_copy_cols(const void* src, void* dst, int64_t rows, int32_t c, int64_t ld, int32_t col0, int32_t dtype, void* stream);

/* low fp32 [images, hl, wl, 64] (PAF in columns 0 .. 37, heat in 40 .. 58) -> planar fp32 raw [images, 18, h, w], smooth [images, 18, h, w]
 * and paf [images, 38, h, w].  mx [2, w, wl] and my [2, h, hl]: per axis the matrix A of (x8 LANCZOS4, crop, LANCZOS4 to the frame) and the
 * matrix G A with the sigma-3 Gaussian (reflect) on top, composed on the host in float64; raw and paf take A, smooth G A.  A columns pass
 * into the workspace and a rows pass (a thread owns one column of four output rows), fp32, the source index ascending.  images <= 885. */
int64_t ca_pose_maps_workspace_bytes(int32_t images, int32_t hl, int32_t w);
int ca_pose_maps(const float* low, const float* mx, const float* my, void* workspace, int64_t workspace_bytes, float* raw, float* smooth, float* paf,
                 int32_t images, int32_t hl, int32_t wl, int32_t h, int32_t w, void* stream);

/* Per (frame, part): smooth >= its four neighbours (zero outside the frame) and (double) smooth > 0.1; the first CA_POSE_MAX_PEAKS in
 * row-major order -> peaks int32 [images, 18, 64, 2] (x, y), scores fp32 [images, 18, 64] read from raw, counts int32 [images, 18];
 * overflow int32 [images] is zeroed and gets CA_POSE_OVERFLOW_PEAKS where a part had more. */
int ca_pose_peaks(const float* raw, const float* smooth, int32_t* peaks, float* scores, int32_t* counts, int32_t* overflow, int32_t images, int32_t h, int32_t w,
                  void* stream);

/* Per (frame, limb): the float64 score of every candidate pair (10 samples at int(round(linspace)), mean(paf . unit) + min(0.5 h / norm
 * - 1, 0), kept when more than 8 samples exceed 0.05 and the score is positive), the stable descending order and the greedy matching ->
 * conn_ij int32 [images, 19, 64, 2] (index into the two parts' peaks), conn_score float64 [images, 19, 64], conn_n int32 [images, 19]. */
int ca_pose_connect(const float* paf, const int32_t* peaks, const int32_t* counts, int32_t* conn_ij, double* conn_score, int32_t* conn_n, int32_t images, int32_t h,
                    int32_t w, void* stream);

/* Per frame: the subset table (found == 1 / found == 2 merge or extend / new row for the first 17 limbs), rows with fewer than 4 parts or
 * score / parts < 0.4 deleted -> keypoints int32 [images, 64, 18, 2] = int(x / float(w) * w), int(y / float(h) * h) (-1 where a part is
 * missing or the row is unused), coords (the same table with the peaks' own pixels, what ca_pose_draw reads), people int32 [images];
 * overflow gets CA_POSE_OVERFLOW_PEOPLE where a 65th row was needed. */
int ca_pose_assemble(const int32_t* peaks, const float* scores, const int32_t* conn_ij, const double* conn_score, const int32_t* conn_n, int32_t* keypoints,
                     int32_t* coords, int32_t* people, int32_t* overflow, int32_t images, int32_t h, int32_t w, void* stream);

/* draw_bodypose of every person in order: per person 17 limbs (ellipse2Poly + fillConvexPoly, colour int(c * 0.6)) and then 18 filled
 * radius-4 circles; primitive person * 35 + k writes its index with atomicMax into index uint32 [images, h, w] (zeroed here), a second
 * pass writes the colours: map uint8 [images, h, w, 3] (may be NULL) and / or control [rep * images, 3, h, w] of control_dtype (CA_F32 /
 * CA_F16) = map / 255.  sin_table: fp32 [451], OpenCV's table of sin(degrees). */
int ca_pose_draw(const int32_t* coords, const int32_t* people, const float* sin_table, uint32_t* index, uint8_t* map, void* control, int32_t images, int32_t h,
                 int32_t w, int32_t rep, int32_t control_dtype, void* stream);

/* ---- added to ABI v16 likewise: the face stage of the OpenPose annotator, around the face network that ca_conv3x3 / ca_maxpool2x2 /
 * ca_gemm / ca_conv7x7 / ca_copy_cols run (controlanimate_amd/openpose_face.py; csrc/ca_openpose_face.hip, ca_pose_draw_faces in
 * csrc/ca_openpose.hip; the specification is tests/face_ref.py) ---- */
#define CA_FACE_SIZE 384              /* every crop is resized to 384 x 384 */
#define CA_FACE_HEAT 48               /* the network's output is 48 x 48 */
#define CA_FACE_PARTS 71              /* heat maps that are read for peaks (the network writes 72 columns, the last one zero) */
#define CA_FACE_MIN_SIDE 11           /* the smallest side of a crop the box rule can produce */
#define CA_FACE_SLOT_INTS 8           /* a slot: person (-1: empty), x, y, w, hc, wc, mode, 0 */
#define CA_FACE_MODE_NONE 0           /* empty slot, or a crop shape whose resize is not restated: constant input, no points */
#define CA_FACE_MODE_LANCZOS4 1
#define CA_FACE_MODE_AREA 2
#define CA_POSE_OVERFLOW_FACES 4        /* more people with a face box than max_faces: the first max_faces in person order are taken */
#define CA_POSE_OVERFLOW_FACE_RESIZE 8  /* a face was skipped: INTER_AREA while an axis grows, or both scales integers with one >= 2 */

/* util.faceDetect per person, from keypoints int32 [images, 64, 18, 2] (pixels, -1: missing) and people int32 [images]: the box from
 * the nose (0), eyes (14, 15: 3.0 x) and ears (16, 17: 1.5 x), in exact integer arithmetic on half pixels -> boxes int32 [images, 64, 4]
 * = (x, y, w, slot) (w = 0 and slot = -1 where there is no box; slot = -1 too where the box got no slot), slots int32 [images, max_faces,
 * CA_FACE_SLOT_INTS] in person order, overflow[img] = (overflow_in ? overflow_in[img] : 0) | the two face bits.  The crop of a box is
 * rows y .. y + hc - 1, columns x .. x + wc - 1 with hc = min(w, h - y), wc = min(w, w_px - x); the mode is CA_FACE_MODE_AREA when hc +
 * wc > 768, else CA_FACE_MODE_LANCZOS4 (smart_resize's k < 1), CA_FACE_MODE_NONE for the shapes of CA_POSE_OVERFLOW_FACE_RESIZE. */
int ca_face_boxes(const int32_t* keypoints, const int32_t* people, const int32_t* overflow_in, int32_t* boxes, int32_t* slots, int32_t* overflow, int32_t images,
                  int32_t h, int32_t w, int32_t max_faces, void* stream);

/* The crops of slots first .. first + crops - 1 (of images * max_faces) of uint8 RGB frames [images, h, w, 3] -> out [crops, 384, 384, 8] of
 * dtype: cv2.resize of the BGR crop to 384 x 384, byte / 256 - 0.5, channels 3 .. 7 zero; zeros for a slot of CA_FACE_MODE_NONE.  Tables
 * per crop side s of an axis (made on the host): INTER_LANCZOS4 for s = CA_FACE_MIN_SIDE .. side_max, lz_ofs int32 [.., 384] and lz_coef
 * int16 [.., 384, 8] (11-bit fixed point; indices clamped to the crop; (sum + 2^21) >> 22); INTER_AREA for s = 384 .. side_max, ar_ofs /
 * ar_cnt int32 [.., 384] and ar_w fp32 [.., 384, 8] (horizontal sums first, then their vertical sum, fp32, no fused multiply-add,
 * rounded half to even).  A block owns two output rows: the horizontal pass of the source rows under them into LDS, then the vertical
 * pass; the host checks that no table a slot can use spans more than the 13 source rows a block keeps (a LANCZOS4 slot with hc + wc > 768
 * is treated as empty).  max(h, w) <= side_max <= 2048. */
int ca_face_crop(const uint8_t* frames, const int32_t* slots, void* out, const int32_t* lz_ofs, const int16_t* lz_coef, const int32_t* ar_ofs, const int32_t* ar_cnt,
                 const float* ar_w, int32_t images, int32_t h, int32_t w, int32_t max_faces, int32_t first, int32_t crops, int32_t side_max, int32_t dtype,
                 void* stream);

/* heat fp32 [images * max_faces, 48, 48, 72] and the slots -> points int32 [images, 64, 71, 2] (frame pixels, -1: none; every row
 * without a slot is -1), the point written to the row of the slot's person.  Per (crop, part) one block evaluates F.interpolate(bilinear,
 * align_corners = True) to (hc, wc) at every crop pixel in fp32 (the plane is never written) and keeps the largest value above 0.05 at
 * its first row-major position; a local coordinate 0 makes that axis -1, otherwise the box origin is added.  A slot of CA_FACE_MODE_NONE, or one
 * whose crop would leave the h x w frame, gives no points. */
int ca_face_peaks(const float* heat, const int32_t* slots, int32_t* points, int32_t images, int32_t max_faces, int32_t h, int32_t w, void* stream);

/* ca_pose_draw with faces: per person the 35 body primitives, then 71 filled radius-3 white discs (draw_facepose) at (xmap[px], ymap[py])
 * of points int32 [images, 64, 71, 2] where both are > 0; primitive person * 106 + k.  xmap int32 [w], ymap int32 [h]:
 * int(float32(float32(p) / side) * side), made on the host.  points == NULL draws the bodies only: ca_pose_draw's bytes. */
int ca_pose_draw_faces(const int32_t* coords, const int32_t* people, const float* sin_table, const int32_t* points, const int32_t* xmap, const int32_t* ymap,
                       uint32_t* index, uint8_t* map, void* control, int32_t images, int32_t h, int32_t w, int32_t rep, int32_t control_dtype, void* stream);

/* ---- added to ABI v16 likewise: the hand stage of the OpenPose annotator around the hand network (FaceNet's layers with 22 output maps;
 * controlanimate_amd/openpose_hand.py; csrc/ca_openpose_hand.hip; the specification is tests/hand_ref.py) ---- */
#define CA_HAND_PARTS 21              /* heat maps that are decoded (the network writes 22, padded to CA_HAND_HEAT_COLS columns) */
#define CA_HAND_HEAT_COLS 24
#define CA_HAND_MAP 128               /* the four-scale average is 128 x 128 */
#define CA_HAND_SCALES 4              /* network inputs of 184, 368, 552 and 736 pixels, maps of 23, 46, 69 and 92 */
#define CA_HAND_SLOT_INTS 8           /* a slot: person (-1: empty), x, y, w, hand (0 left, 1 right), mode, 0, 0 */
#define CA_HAND_MODE_NONE 0           /* empty slot, or a crop side whose resize is not restated: no points */
#define CA_HAND_MODE_RESIZE 1
#define CA_POSE_OVERFLOW_HANDS 16        /* more hand boxes than max_hands: the first max_hands are taken, people in order, left before right */
#define CA_POSE_OVERFLOW_HAND_RESIZE 32  /* a hand was skipped: INTER_AREA at an exact integer ratio other than 2 (w = 184 k, k >= 3) */

/* util.handDetect per person, from keypoints int32 [images, 64, 18, 2] (pixels, -1: missing) and people int32 [images], in double and in
 * the published operation order: left from parts (5, 6, 7), right from (2, 3, 4) = shoulder, elbow, wrist; x = wrist + 0.33 (wrist -
 * elbow), width = 1.5 max(|wrist - elbow|, 0.9 |elbow - shoulder|), the corner moved by width / 2 and clamped at 0, the width cut at the
 * frame, kept from 20 on.  boxes int32 [images, 64, 2, 4] = (x, y, w, slot) (w = 0 and slot = -1 where there is no box; slot = -1 too where
 * the box got no slot), slots int32 [images, max_hands, CA_HAND_SLOT_INTS] in person order, left before right, overflow[img] =
 * (overflow_in ? overflow_in[img] : 0) | the two hand bits.  The crop of a box is always the full w x w square. */
int ca_hand_boxes(const int32_t* keypoints, const int32_t* people, const int32_t* overflow_in, int32_t* boxes, int32_t* slots, int32_t* overflow, int32_t images,
                  int32_t h, int32_t w, int32_t max_hands, void* stream);

/* The input of the hand network at one side (184, 368, 552 or 736) for slots first .. first + crops - 1 of uint8 RGB frames [images, h,
 * w, 3] -> out [crops, side, side, 8] of dtype (BGR, byte / 256 - 0.5, channels 3 .. 7 zero; zeros for an empty or skipped slot).  blur = 1
 * first writes cv2.GaussianBlur(crop, (0, 0), 0.8) of those slots into blurred uint8 [images * max_hands, side_max, side_max, 3] (taps:
 * the 7 double taps; rows then columns in double, BORDER_REFLECT_101 inside the crop, one rounding); blur = 0 reads what an earlier call
 * wrote there.  The resize of the blurred w x w crop is cv2.resize's: INTER_LANCZOS4 for w <= side (lz_ofs int32 [min(side, side_max) - 19,
 * side], lz_coef int16 [.., side, 8], row w - 20: OpenCV's 11-bit fixed point), (a + b + c + d + 2) >> 2 for w = 2 side, else INTER_AREA
 * (ar_ofs, ar_cnt int32 [side_max - side, side], ar_w fp32 [.., side, CA_HAND_AREA_TAPS], row w - side - 1: fp32 weighted sums, rounded
 * half to even).  side_max = min(h, w): no box is wider. */
#define CA_HAND_MIN_BOX 20
#define CA_HAND_AREA_TAPS 16
int ca_hand_crop(const uint8_t* frames, const int32_t* slots, const double* taps, uint8_t* blurred, void* out, const int32_t* lz_ofs, const int16_t* lz_coef,
                 const int32_t* ar_ofs, const int32_t* ar_cnt, const float* ar_w, int32_t images, int32_t h, int32_t w, int32_t max_hands, int32_t first, int32_t crops,
                 int32_t side, int32_t side_max, int32_t blur, int32_t dtype, void* stream);

/* The network's maps of the four scales, fp32 [slots, m, m, CA_HAND_HEAT_COLS] with m = 23, 46, 69, 92, -> raw and smooth fp32 [slots, 21,
 * 128, 128]: raw = sum over the scales of A_s H_s A_s^T / 4 (A_s: the x8 INTER_LANCZOS4 resize and the INTER_AREA resize to 128 of one
 * axis composed), smooth its gaussian_filter(sigma = 3) through G A_s.  mats fp32 [2][230][128]: the transposed A_s ([m][128]) of the
 * four scales behind each other, then the transposed G A_s.  No x8 plane is written. */
int ca_hand_maps(const float* heat184, const float* heat368, const float* heat552, const float* heat736, const float* mats, float* raw, float* smooth,
                 int32_t slots, void* stream);

/* Per (slot, part) of raw / smooth fp32 [images * max_hands, 21, 128, 128]: binary = smooth > 0.05; its 8-connected components
 * (skimage.measure.label(connectivity = 2): numbered by their first pixel in raster order); the one with the largest sum of raw (a
 * double sum in a fixed order: bit-identical from run to run; the first label on a tie); the first row-major maximum of raw zeroed
 * outside it (pixel 0 for an empty binary plane).  peaks int32 [slots, 21, 2] = that (x, y) on the 128 grid, mass double [slots, 21] the
 * winner's sum (0 for none); points int32 [images, 64, 2, 21, 2] (frame pixels; every entry without a slot is -1): int(x * w / 128.0) of the
 * slot's box, -1 where that is 0, else plus the box origin.  A slot of CA_HAND_MODE_NONE gives no points. */
int ca_hand_peaks(const float* raw, const float* smooth, const int32_t* slots, int32_t* points, int32_t* peaks, double* mass, int32_t images, int32_t max_hands,
                  int32_t h, int32_t w, void* stream);

/* ca_pose_draw_faces with hands: per person the 35 body primitives, then per hand (left, right) 20 edges cv2.line(thickness = 2) in their
 * hsv colours and 21 filled radius-4 circles in (0, 0, 255) (draw_handpose; hand_points int32 [images, 64, 2, 21, 2] through xmap / ymap,
 * an edge where all four coordinates come out positive, a circle where both do), then the 71 face discs (face_points NULL: none);
 * primitive person * 188 + k.  A thick line is OpenCV's ThickLine: the corners p0 +- dp, p1 -+ dp at 16 fractional bits through
 * FillConvexPoly, and a filled radius-1 circle at each end. */
int ca_pose_draw_hands(const int32_t* coords, const int32_t* people, const float* sin_table, const int32_t* hand_points, const int32_t* face_points,
                       const int32_t* xmap, const int32_t* ymap, uint32_t* index, uint8_t* map, void* control, int32_t images, int32_t h, int32_t w, int32_t rep,
                       int32_t control_dtype, void* stream);

/* ---- added to ABI v16 likewise: the NormalBae annotator's stages beside ca_gemm / ca_conv3x3 / ca_upsample2x_bilinear_ac
 * (controlanimate_amd/normalbae.py; csrc/ca_normalbae.hip).  Tensors are NHWC of dtype CA_F16 / CA_BF16 with fp32 accumulation; no entry
 * point reads device data on the host or uses floating-point atomics: two runs give the same bits.  Anything out of range is
 * CA_ERR_INVALID_ARG before any launch. ---- */

/* The EfficientNet stem: uint8 RGB src [images, h, w, 3] (h, w even) -> y [images, h/2, w/2, cout] = swish(conv3x3 stride 2 of
 * (src / 255 - mean) / std + bias), ImageNet mean / std, TensorFlow-SAME padding (0 before, 1 after) whose zeros lie in the NORMALISED
 * image.  wt fp32 [27][cout], row (ky * 3 + kx) * 3 + channel, BatchNorm folded; bias fp32 [cout]; cout a multiple of 8 up to 64. */
int ca_nbae_stem(const uint8_t* src, const float* wt, const float* bias, void* y, int32_t images, int32_t h, int32_t w, int32_t cout, int32_t dtype, void* stream);

/* Depthwise ksize x ksize (3 or 5) convolution, stride 1 or 2, TensorFlow-SAME padding (out = ceil(in / stride), total =
 * max((out - 1) * stride + ksize - in, 0), total / 2 in front), + fp32 bias [c], swish: x [images, h, w, c] -> y [images, ho, wo, c];
 * wt [ksize * ksize][c] of dtype (tap ky * ksize + kx of every channel); c a multiple of 8 up to 3072; planes down to 1 x 1.  It also
 * writes sums fp32 [images][c]: the sum over the plane of the values it STORED (the rounded ones) in a fixed order, through partials
 * (ca_dwconv_same_partials_floats(images, h, w, c, stride) floats of scratch; 0 for arguments out of range).  y must not overlap x. */
int64_t ca_dwconv_same_partials_floats(int32_t images, int32_t h, int32_t w, int32_t c, int32_t stride);
int ca_dwconv_same(const void* x, const void* wt, const float* bias, void* y, float* sums, float* partials, int32_t images, int32_t h, int32_t w, int32_t c,
                   int32_t ksize, int32_t stride, int32_t dtype, void* stream);

/* The squeeze-and-excite gate of the whole batch in one launch, fp32 throughout: gate[n][c] = sigmoid(W_e swish(W_r (sums[n] *
 * inv_pixels) + b_r) + b_e).  w_reduce [r][c], b_reduce [r], w_expand_t [r][c] (the expand weight [c][r] transposed), b_expand [c];
 * c up to 3072, r up to 256 (any value: no multiple of 8 is asked for). */
int ca_se_gate(const float* sums, const float* w_reduce, const float* b_reduce, const float* w_expand_t, const float* b_expand, float* gate, int32_t images,
               int32_t c, int32_t r, float inv_pixels, void* stream);

/* y[n][p][c] = round(x[n][p][c] * gate[n][c]) for x [images, pixels, c] of dtype, gate fp32 [images][c]; y == x is allowed. */
int ca_scale_channels(const void* x, const float* gate, void* y, int32_t images, int64_t pixels, int32_t c, int32_t dtype, void* stream);

/* The pieces of a refinement stage run as GEMMs: ca_nbae_cat_pred interpolates the fp32 prediction pred [images, h, w, 4] x2 (bilinear,
 * align_corners, fp32) and rounds it into columns col0 .. col0 + 3 of y [images, 2h, 2w, ld] of dtype, zeros into col0 + 4 .. col0 + 7
 * (the MLP's input width C + 4 padded to C + 8); ca_nbae_normalize is norm_normalize on the first four of ld fp32 columns of raw [rows]:
 * pred [rows][4] = (xyz / (sqrt(x^2 + y^2 + z^2) + 1e-10), elu(k) + 1 + min_kappa). */
int ca_nbae_cat_pred(const float* pred, void* y, int32_t images, int32_t h, int32_t w, int64_t ld, int32_t col0, int32_t dtype, void* stream);
int ca_nbae_normalize(const float* raw, int64_t ld, float* pred, int64_t rows, float min_kappa, void* stream);

/* One refinement stage in ONE launch: feat [images, h, w, c] of dtype (c = 128, 256 or 512) and the fp32 prediction pred [images, h, w, 4],
 * both x2 (bilinear, align_corners; the feature row rounded as ca_upsample2x_bilinear_ac rounds it, the prediction as ca_nbae_cat_pred),
 * through the MLP (c + 4) -> 128 -> 128 -> 128 -> 4 (ReLU, hidden activations rounded to dtype, kept in LDS) on the MFMA, norm_normalize ->
 * out fp32 [images, 2h, 2w, 4].  w0 .. w3: the weights as MFMA fragments of dtype, fragment (ks, t) = 64 lanes x 8 elements at
 * ((ks * T + t) * 64 + lane) * 8 holding W[t * 16 + lane % 16][ks * 32 + lane / 16 * 8 + e], T = 8 (w3: T = 1, rows 4 .. 15 zero), K
 * padded with zeros to a multiple of 32 (w0: c + 4 -> the next multiple of 32 at or above c + 8); b0 .. b2 fp32 [128], b3 fp32 [4]. */
int ca_nbae_refine(const void* feat, const float* pred, const void* w0, const void* w1, const void* w2, const void* w3, const float* b0, const float* b1,
                   const float* b2, const float* b3, float* out, int32_t images, int32_t h, int32_t w, int32_t c, float min_kappa, int32_t dtype, void* stream);

/* pred fp32 [images, h, w, 4] (xyz in the first three) -> map uint8 [images, h, w, 3] = trunc(clip(clip((xyz + 1) * 0.5, 0, 1) * 255, 0,
 * 255)), every operation in fp32 and rounded by itself (byte-exact against numpy), and / or control [rep * images, 3, h, w] = map / 255
 * (CA_F32 or CA_F16; rep = 2 writes the frames twice).  h * w a multiple of 4. */
int ca_nbae_finish(const float* pred, int32_t images, int32_t h, int32_t w, uint8_t* map, void* control, int32_t rep, int32_t control_dtype, void* stream);

/* ---- added to ABI v16 likewise: face detection and alignment in front of the GFPGAN face restorer -- RetinaFace-ResNet50, its decode and
 * NMS, get_face_landmarks_5's filters, the 5-point similarity and the warp to 512 x 512 (controlanimate_amd/face_align.py;
 * csrc/ca_retinaface.hip; the specification is tests/retinaface_ref.py).  The bottlenecks' 1x1 convolutions, the FPN's and the heads' run
 * on ca_gemm (the block's identity as its residual: the epilogue adds it before the activation), every 3x3 convolution on ca_conv3x3
 * (CA_ACT_RELU), the SSH concatenation through ca_copy_cols.  No entry reads device data on the host, none uses floating-point atomics:
 * two runs give the same bits and the chain can be captured in a hipGraph. ---- */
#define CA_RFACE_MAX_CAND 1024        /* candidates above the threshold that enter the NMS, per frame */
#define CA_RFACE_HEAD_COLS 32         /* a level's head row: 4 class | 8 box | 20 landmark columns (two priors per cell) */
#define CA_RFACE_DET_COLS 15          /* x1, y1, x2, y2, score, five landmarks (x, y) */
#define CA_RFACE_MAX_FACES 64
#define CA_RFACE_OVERFLOW_CAND 1      /* more than CA_RFACE_MAX_CAND candidates: the best by (score, lower prior index) were taken */
#define CA_RFACE_OVERFLOW_FACES 2     /* more faces than max_faces: the first max_faces in NMS order were taken */
#define CA_RFACE_CENTER 1             /* flags: only_center_face */
#define CA_RFACE_LARGEST 2            /* flags: only_keep_largest (wins over CA_RFACE_CENTER) */
#define CA_FACE_ALIGN_SIZE 512

/* uint8 frames src [images, h, w, 3] -> y [images, h / 2, w / 2, cout] of dtype = relu(conv 7x7 stride 2 padding 3 of (byte - mean) + bias):
 * mean (104, 117, 123) by the network's channel, which is the array's channel c (bgr = 0) or 2 - c (bgr = 1); the zero padding lies in the
 * mean-subtracted image.  w_packed of dtype [ceil(cout / 16) * 16][160]: column ky * 21 + kx * 3 + network channel, columns 147 .. 159 and
 * the rows from cout on zero (BatchNorm folded); bias fp32 [cout].  h and w even, cout a multiple of 8 in 8 .. 64; on the MFMA, fp32 sums. */
int ca_rface_stem(const uint8_t* src, const void* w_packed, const float* bias, void* y, int32_t images, int32_t h, int32_t w, int32_t cout, int32_t bgr, int32_t dtype,
                  void* stream);

/* The 3x3 / stride-2 / padding-1 maximum of x [images, h, w, c] -> y [images, (h - 1) / 2 + 1, (w - 1) / 2 + 1, c]; only the taps inside the
 * image take part.  c a multiple of 8. */
int ca_maxpool3x3s2(const void* x, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t dtype, void* stream);

/* y [images, (h + 1) / 2, (w + 1) / 2, c] = x[:, ::2, ::2, :]: the gather in front of a stride-2 1x1 convolution on ca_gemm. */
int ca_subsample2(const void* x, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t dtype, void* stream);

/* y [images, h, w, c] = a [images, h, w, c] + b [images, h / 2, w / 2, c] at (y / 2, x / 2) (F.interpolate(mode='nearest') to twice the size),
 * the sum in fp32, rounded once; h and w even; y may be a. */
int ca_add_up2(const void* a, const void* b, void* y, int32_t images, int32_t h, int32_t w, int32_t c, int32_t dtype, void* stream);

int64_t ca_rface_decode_workspace_bytes(int32_t images, int32_t h, int32_t w);

/* One launch per window, one block per frame.  heads0 .. 2: fp32 [images, ceil(h / 8 | 16 | 32), ceil(w / ..), 32] (CA_RFACE_HEAD_COLS: per
 * prior a of a cell, class logits at 2a, box at 4 + 4a, landmarks at 12 + 10a).  Prior k of a frame: levels in order, cells row-major, two
 * priors per cell, (cx, cy, s / w, s / h) computed from the indices in float64.  score = 1 / (1 + exp(c0 - c1)) in float64, rounded to fp32,
 * kept when > conf; the CA_RFACE_MAX_CAND best by (score descending, prior index ascending); boxes and landmarks decoded in float64
 * (variances 0.1, 0.2) and rounded once to fp32; the greedy NMS in float64 with areas (x2 - x1 + 1)(y2 - y1 + 1), a box stays while its
 * overlap with every kept box is <= nms; faces whose landmarks 0 and 1 are closer than eye_dist are dropped; flags choose one face.
 * -> dets fp32 [images, max_faces, 15] (zero rows behind the count), count int32 [images], overflow int32 [images] (CA_RFACE_OVERFLOW_*).
 * workspace: at least ca_rface_decode_workspace_bytes(images, h, w) bytes, 8-byte aligned. */
int ca_rface_decode(const float* heads0, const float* heads1, const float* heads2, int32_t images, int32_t h, int32_t w, float conf, float nms, float eye_dist,
                    int32_t flags, int32_t max_faces, void* workspace, int64_t workspace_bytes, float* dets, int32_t* count, int32_t* overflow, void* stream);

/* dets, count -> affine float64 [images, max_faces, 2, 3]: the least-squares similarity (scale, rotation, translation) of the five landmarks
 * onto the 512 x 512 template, closed form in float64; inverse float64 likewise: invertAffineTransform(affine) * upscale.  Slots behind the
 * count are zero.  One thread per slot. */
int ca_face_align(const float* dets, const int32_t* count, int32_t images, int32_t max_faces, double upscale, double* affine, double* inverse, void* stream);

/* cv2.warpAffine(frame, affine, (512, 512)) of every slot -> faces uint8 [images * max_faces, 512, 512, 3]: INTER_LINEAR in OpenCV's fixed
 * point (coordinates at 10 fractional bits rounded to 5, 15-bit weights, (sum + 2^14) >> 15), BORDER_CONSTANT (135, 133, 132) by channel
 * position (bgr = 1: (132, 133, 135)); a slot behind the count is filled with the border value.  h and w below 32768. */
int ca_face_warp(const uint8_t* frames, const double* affine, const int32_t* count, uint8_t* faces, int32_t images, int32_t h, int32_t w, int32_t max_faces,
                 int32_t bgr, void* stream);

/* ---- added to ABI v16 likewise: the paste-back behind the face restorer -- facexlib's ParseNet, the parsing mask's two Gaussian blurs, the
 * inverse warp and the blend of FaceRestoreHelper.paste_faces_to_input_image (controlanimate_amd/face_paste.py; csrc/ca_facepaste.hip; the
 * specification is tests/facepaste_ref.py).  ParseNet pads by REFLECTION: its convolutions run on ca_conv3x3_reflect, or -- the stride-1
 * ones, by a host-side switch -- on the zero-padded ca_conv3x3 over a ringed tensor that ca_ring_fill completes.  `rings` / `ring` say which
 * operands are ringed tensors [n, H + 2, W + 2, C] of which the interior is addressed.  No entry reads device data on the host, none uses
 * atomics: two runs give the same bits and the chain can be captured in a hipGraph. ---- */
#define CA_PARSE_CLASSES 19           /* ParseNet's parsing maps; MASK_COLORMAP is 0 for classes 0, 14, 16, 17, 18 and 255 for the rest */
#define CA_PARSE_CPAD 32              /* channels of ca_parse_prep's output, and rows of the last layer's padded weight */
#define CA_BLUR_TAPS 51               /* the centre tap and the 50 behind it of the symmetric 101-tap kernel */
#define CA_RING_IN 1                  /* rings: x is ringed */
#define CA_RING_OUT 2                 /*        y is ringed (its interior is written, its ring is left alone) */
#define CA_RING_RES 4                 /*        the residual is ringed */
#define CA_RING_REFLECT 0             /* ca_ring_fill's mode: ring row 0 = interior row 1 (ReflectionPad2d(1)) */
#define CA_RING_REPLICATE 1           /*                      ring row 0 = interior row 0 */

/* uint8 faces [images, size, size, 3] -> out [images, size, size, 32] of dtype (ringed when ring = 1): channel c = ((byte / 255) - 0.5) / 0.5
 * of channel c (reverse = 0) or 2 - c (reverse = 1), each operation in fp32, rounded once to dtype; channels 3 .. 31 are zero. */
int ca_parse_prep(const uint8_t* faces, void* out, int32_t images, int32_t size, int32_t reverse, int32_t ring, int32_t dtype, void* stream);

/* y [images, gh, gw, cout] = act(Conv2d(k 3, stride, padding 0)(ReflectionPad2d(1)(u)) + bias + residual), u = x [images, h, w, cin] or, with
 * up2 = 1, its nearest x2 (the x2 plane is never written: reflection on it is replication of x's border).  gh = (lh - 1) / stride + 1 with
 * lh = h or 2 h.  wt of dtype [cout][3][3][cin]; bias fp32 [cout]; residual of dtype [images, gh, gw, cout] or NULL; act = LeakyReLU(0.2) when
 * leaky; y of dtype, or fp32 when out_f32.  cin and cout each 32, 64, 128 or 256; stride 1 or 2, up2 only at stride 1.  An implicit GEMM on
 * the MFMA from an LDS halo tile whose load applies the reflection as an index map; fp32 sums. */
int ca_conv3x3_reflect(const void* x, const void* wt, const float* bias, const void* residual, void* y, int32_t images, int32_t h, int32_t w, int32_t cin,
                       int32_t cout, int32_t stride, int32_t up2, int32_t leaky, int32_t out_f32, int32_t rings, int32_t dtype, void* stream);

/* ParseNet's last layer in one launch: the reflected stride-1 convolution of x [images, h, w, cin] (ringed when ring = 1) with wt of dtype
 * [32][3][3][cin] (rows classes .. 31 zero) and bias fp32 [32], the first maximum over the `classes` logits (the lowest index wins a tie) and
 * the colour map -> mask uint8 [images, h, w] of 0 / 255.  The logits never reach memory.  classes = CA_PARSE_CLASSES. */
int ca_parse_mask(const void* x, const void* wt, const float* bias, uint8_t* mask, int32_t images, int32_t h, int32_t w, int32_t cin, int32_t classes,
                  int32_t ring, int32_t dtype, void* stream);

/* The composed form's tail: logits fp32 [pixels, cols] -> labels uint8 [pixels] (the first maximum over columns 0 .. classes - 1) and / or
 * mask uint8 [pixels] (the colour map of the label). */
int ca_parse_labels(const float* logits, uint8_t* labels, uint8_t* mask, int64_t pixels, int32_t cols, int32_t classes, void* stream);

/* Writes the one-pixel ring of x [images, h + 2, w + 2, c] of dtype from its interior (corners included), by CA_RING_REFLECT or
 * CA_RING_REPLICATE.  c a multiple of 8. */
int ca_ring_fill(void* x, int32_t images, int32_t h, int32_t w, int32_t c, int32_t mode, int32_t dtype, void* stream);

/* mask uint8 [images, 512, 512] -> out float64 [images, 512, 512]: cv2.GaussianBlur(., (101, 101), 11) twice (each a row pass, then a column
 * pass, BORDER_REFLECT_101), the outer 10 rows and columns zeroed, divided by 255.  taps float64 [ntaps = CA_BLUR_TAPS]: the normalised
 * kernel's centre tap k0 and k1 .. k50.  A pass computes k0 x0 + sum over i = 1 .. 50, in that order, of k_i (x_-i + x_+i), every product and
 * sum rounded by itself.  workspace float64 [images, 512, 512], not out.  size must be 512. */
int ca_mask_blur(const uint8_t* mask, const double* taps, double* workspace, double* out, int32_t images, int32_t size, int32_t ntaps, void* stream);

/* out uint8 [images, h, w, 3]: every pixel starts from background [images, h, w, 3] and walks the faces r < count[image] in order:
 * v = cv2.warpAffine(restored[image * max_faces + r], M, (w, h)) in OpenCV's fixed point with border 0, m = the bilinear sample of
 * masks[image * max_faces + r] (float64 [., 512, 512]) at the same coordinates (5 fractional bits, four products summed in double, border 0),
 * pixel = m v + (1 - m) pixel in float64; one truncation to uint8 at the end.  M = inverse_affine float64 [images, max_faces, 2, 3] with
 * 0.5 upscale added to its translation column when upscale > 1 (inside the kernel; the matrices are only read).  out may be background. */
int ca_face_paste(const uint8_t* background, const uint8_t* restored, const double* masks, const double* inverse_affine, const int32_t* count, uint8_t* out,
                  int32_t images, int32_t h, int32_t w, int32_t max_faces, double upscale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CONTROLANIMATE_HIP_H */
