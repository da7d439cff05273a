"""Thin torch-tensor front end of the C ABI (device pointers + current HIP stream).

torch is used only for device memory and streams; every arithmetic op below is a call into
`libcontrolanimate_hip.so`.  All activations are channels-last ("NHWC"): `[images, H, W, C]`.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _capi
from .context import dispatch
from ._operands import _D2, _D3, _D4, _D5, _need, _req_cuda, _t  # every operand rule raises CAHipError (python -O keeps them)
from ._capi import (AttnArgs, ConvArgs, ConvNarrowArgs, FfArgs, PerceiverAttnArgs, TattnArgs, XattnArgs, GemmArgs, GroupNormArgs, LayerNormArgs, CA_ACT_NONE,
                    CA_ACT_SILU, CA_BF16, CA_F16, check, lib)

ACT_NONE, ACT_SILU = CA_ACT_NONE, CA_ACT_SILU
ACT_QUICK_GELU, ACT_GELU = _capi.CA_ACT_QUICK_GELU, _capi.CA_ACT_GELU  # CLIP MLPs
ACT_RELU = _capi.CA_ACT_RELU     # the VGG stack of the HED annotator (hed.py)
ACT_RELU6 = _capi.CA_ACT_RELU6   # the MobileNetV2 backbone of the M-LSD annotator (mlsd.py)


def dt_code(dtype: torch.dtype) -> int:
    if dtype == torch.bfloat16:
        return CA_BF16
    if dtype == torch.float16:
        return CA_F16
    raise TypeError(f"activations must be bf16 or fp16, got {dtype}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _out(who: str, name: str, out: Optional[torch.Tensor], shape, dtype, device) -> torch.Tensor:
    """The output operand: allocated when None, else held to exactly that shape and dtype, contiguous."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    _t(who, name, out, dtype, shape)
    return out


_plan_sink = None  # a list: receives the kernel label (ca_gemm_plan_name / ca_conv3x3_plan_name) of every launch -- bench.py, tests


def _record_plan(query, args) -> None:
    if _plan_sink is not None:
        buf = C.create_string_buffer(64)
        _plan_sink.append(buf.value.decode() if query(C.byref(args), buf, 64) == 0 else "?")


def gemm(a: torch.Tensor, w: torch.Tensor, *, a2: Optional[torch.Tensor] = None,
         bias: Optional[torch.Tensor] = None, rowbias: Optional[torch.Tensor] = None,
         rows_per_group: int = 0, residual: Optional[torch.Tensor] = None, alpha: float = 1.0,
         post_scale: float = 1.0, act: int = ACT_NONE, geglu: bool = False, out_f32: bool = False,
         out: Optional[torch.Tensor] = None, ln=None, row_sums: bool = False) -> torch.Tensor:
    """out[M, N] = epilogue(cat(a, a2)[M, K] @ w[N, K]^T); see ca_gemm in the header.
    ln = (row_stats(a), colsum(w) fp32 [N]): LayerNorm of `a` folded in (w, bias packed accordingly)."""
    who = "ca_gemm"
    _req_cuda(who, "a w a2 bias rowbias residual out", a, w, a2, bias, rowbias, residual, out)
    _need(a.dim() == 2 and a.stride(1) == 1, who, "a must be [M, K1] with unit column stride", a)
    _t(who, "w", w, None, _D2)
    m, k1 = a.shape
    k2 = 0
    if a2 is not None:
        _need(a2.dim() == 2 and a2.stride(1) == 1 and a2.shape[0] == m and a2.dtype == a.dtype, who, "a2 must be [M, K2] of a's dtype with unit column stride", a2)
        k2 = a2.shape[1]
    n = w.shape[0]
    _t(who, "w", w, a.dtype, (None, k1 + k2), contiguous=False)
    ncols = n // 2 if geglu else n
    if out is None:
        out = torch.empty((m, ncols), device=a.device, dtype=torch.float32 if out_f32 else a.dtype)
    _need(out.shape == (m, ncols) and out.stride(1) == 1, who, "out must be [M, N] (GEGLU: [M, N / 2]) with unit column stride", out)
    if residual is not None:
        _need(residual.shape == (m, n) and residual.stride(1) == 1 and residual.dtype == a.dtype, who, "residual must be [M, N] of a's dtype with unit column stride", residual)
    if bias is not None:
        _t(who, "bias", bias, torch.float32, numel=n, contiguous=False)
    if rowbias is not None:
        _need(rowbias.dtype == torch.float32 and rowbias.dim() == 2 and rowbias.shape[1] == n and rows_per_group > 0, who,
              "rowbias must be float32 [groups, N] with rows_per_group > 0", rowbias)
    args = GemmArgs(a=_p(a), a2=_p(a2), w=_p(w), c=_p(out), bias=_p(bias), rowbias=_p(rowbias),
                    residual=_p(residual), lda=a.stride(0), lda2=a2.stride(0) if a2 is not None else 0,
                    ldc=out.stride(0), ld_res=residual.stride(0) if residual is not None else 0,
                    ld_rowbias=rowbias.stride(0) if rowbias is not None else 0,
                    m=m, n=n, k1=k1, k2=k2, rows_per_group=rows_per_group, alpha=alpha,
                    post_scale=post_scale, act=act, geglu=int(geglu), out_f32=int(out_f32),
                    dtype=dt_code(a.dtype))
    frag = getattr(w, "_frag", None)  # (tensor, geglu flag it was packed for): attach_w_frag
    if frag is not None and frag[1] == bool(geglu) and dispatch.gemm_ar:
        args.w_frag = _p(frag[0])
    if ln is not None:
        st, cs = ln
        _t(who, "ln colsum", cs, torch.float32, numel=n, contiguous=False)
        args.ln_colsum = _p(cs)
        if isinstance(st, RowStats):  # statistics on demand: inside the GEMM where the library can, else the partial
            # sums the producing GEMM left (row_sums=True), else the separate pass
            _need(st.x.data_ptr() == a.data_ptr() and st.x.shape == a.shape, who, "ln: RowStats belongs to another tensor than a")
            args.ln_eps = st.eps
            if lib().ca_gemm_ln_inline_supported(C.byref(args)):
                pass
            elif st.sums is not None:
                rs, parts = st.sums
                _t(who, "ln row sums", rs, torch.float32, (m, parts, 2))
                args.ln_stats, args.ln_parts = _p(rs), min(parts, 4)
                # (more than 4 partial sums per row -- a producer on the 256 x 320 kernel leaves one per 80-column wave quarter --
                #  are always finished first: the consuming epilogues add at most 4)
                if parts > 4 or lib().ca_gemm_wants_finished_stats(C.byref(args)):
                    # the kernel the plan prefers for this shape (256 x 320 tiles) reads finished (mean, rstd): a 3 us pass
                    # over [m, parts, 2] instead of the consumer's epilogue adding the parts (ABI v8)
                    fin = getattr(st, "_finished", None)
                    if fin is None:
                        fin = torch.empty((m, 2), device=a.device, dtype=torch.float32)
                        check(lib().ca_ln_finish_sums(_p(rs), parts, m, k1 + k2, st.eps, _p(fin), _stream()), "ca_ln_finish_sums")
                        st._finished = fin
                    args.ln_stats, args.ln_parts = _p(fin), 0
            else:
                st = st.tensor()
        if not isinstance(st, RowStats):
            _t(who, "ln stats", st, torch.float32, (m, 2))
            args.ln_stats = _p(st)
    if hasattr(out, "_row_sums"):  # a caller-supplied `out` reused from an earlier call: its sums describe the old contents
        del out._row_sums
    if row_sums and dispatch.ln_row_sums and not geglu and not out_f32:
        parts = int(lib().ca_gemm_row_sums_parts(C.byref(args)))
        if parts > 0:  # the epilogue leaves (sum, sum of squares) per row and 320-column tile: the next LayerNorm's statistics
            rs = torch.empty((m, parts, 2), device=a.device, dtype=torch.float32)
            args.row_sums_out = _p(rs)
            out._row_sums = (rs, parts)
    wbytes = 0 if args.row_sums_out else int(lib().ca_gemm_workspace_bytes(C.byref(args)))
    if wbytes > 0:  # split-K slabs for the 8x8-latent level (allocator-cached, stream-ordered)
        ws = torch.empty((wbytes,), device=a.device, dtype=torch.uint8)
        args.workspace, args.workspace_bytes = _p(ws), wbytes
    _record_plan(lib().ca_gemm_plan_name, args)
    check(lib().ca_gemm(C.byref(args), _stream()), "ca_gemm")
    return out


def attach_w_frag(w: torch.Tensor, geglu: bool = False) -> torch.Tensor:
    """Gives a packed [N, 320] weight its fragment-ordered twin (ca_pack_w_frag, ABI v9): `gemm` hands both over and the K = 320
    projections of the 64x64-latent level run on the activation-resident kernel.  No-op for shapes that kernel cannot take.
    Called once per weight at prepare() time; the twin lives beside the arena (N x 640 bytes)."""
    _req_cuda("ca_pack_w_frag", "w", w)
    if w.dim() != 2 or w.shape[1] != 320 or w.shape[0] % 320 != 0 or not w.is_contiguous() or w.dtype not in (torch.float16, torch.bfloat16):
        return w
    dst = torch.empty_like(w)
    check(lib().ca_pack_w_frag(w.data_ptr(), w.shape[0], w.shape[1], int(bool(geglu)), dst.data_ptr(), _stream()), "ca_pack_w_frag")
    w._frag = (dst, bool(geglu))
    return w


def ff_fused(x: torch.Tensor, w1_frag: torch.Tensor, bias1: torch.Tensor, colsum1: torch.Tensor, w2_frag: torch.Tensor,
             bias2: Optional[torch.Tensor], ln_eps: float, residual: Optional[torch.Tensor] = None,
             ln_stats: Optional[torch.Tensor] = None, *, w_out_frag: Optional[torch.Tensor] = None, bias_out: Optional[torch.Tensor] = None,
             residual_out: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """y = GEGLU(LN(x) W1^T + b1) W2^T + b2 + residual in one launch (ca_ff_fused, ABI v9: the 64x64-latent level's feed-forward,
    C = 320) -- or None where the library does not take the arguments (the caller then runs the two GEMMs).
    With w_out_frag (layers.frag_order_wout of the transformer's proj_out.weight; ABI v12) the launch also applies that projection
    and returns y Wout^T + bias_out + residual_out."""
    if not dispatch.ff_fused:
        return None
    _req_cuda("ca_ff_fused", "x w1_frag bias1 colsum1 w2_frag bias2 residual ln_stats w_out_frag bias_out residual_out", x, w1_frag, bias1, colsum1, w2_frag, bias2, residual,
              ln_stats, w_out_frag, bias_out, residual_out)
    if x.dim() != 2 or x.stride(1) != 1 or (residual is not None and (residual.shape != x.shape or residual.stride(1) != 1 or residual.dtype != x.dtype)):
        return None
    if w_out_frag is None and (bias_out is not None or residual_out is not None):
        return None
    if residual_out is not None and (residual_out.shape != x.shape or residual_out.stride(1) != 1 or residual_out.dtype != x.dtype):
        return None
    m, c = x.shape
    inner = w2_frag.shape[1]
    y = torch.empty((m, c), device=x.device, dtype=x.dtype)
    args = FfArgs(x=_p(x), w1_frag=_p(w1_frag), bias1=_p(bias1), colsum1=_p(colsum1), ln_stats=_p(ln_stats), w2_frag=_p(w2_frag),
                  bias2=_p(bias2), residual=_p(residual), y=_p(y), lda=x.stride(0), ldc=y.stride(0),
                  ld_res=residual.stride(0) if residual is not None else 0, m=m, c=c, inner=inner, ln_eps=float(ln_eps), dtype=dt_code(x.dtype),
                  w_out_frag=_p(w_out_frag), bias_out=_p(bias_out), residual_out=_p(residual_out),
                  ld_res_out=residual_out.stride(0) if residual_out is not None else 0)
    if not lib().ca_ff_fused_supported(C.byref(args)):
        return None
    if _plan_sink is not None:
        _plan_sink.append("ff_out128" if w_out_frag is not None else "ff_fused128")
    check(lib().ca_ff_fused(C.byref(args), _stream()), "ca_ff_fused")
    return y


def tattn_fused(x: torch.Tensor, w_frag: torch.Tensor, gamma: torch.Tensor, bias_pe: torch.Tensor, b: int, frames: int, tokens: int,
                heads: int, ln_eps: float, scale: float, *, w_out_frag: Optional[torch.Tensor] = None, bias_out: Optional[torch.Tensor] = None,
                residual: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """o = softmax(q k^T scale) v over the frame axis with q|k|v = (LayerNorm(x) + pe[frame]) Wqkv^T in one launch (ca_tattn_fused,
    ABI v10: the motion modules of the 64x64-latent level) -- or None where the library does not take the arguments (the caller
    then runs the folded q|k|v GEMM and attention_temporal).  x rows in (b f n) order; bias_pe [>= frames, C] fp32.
    With w_out_frag (layers.frag_order_wout of to_out[0].weight; ABI v12) the launch also applies the output projection and returns
    y = o Wout^T + bias_out + residual."""
    if not dispatch.tattn_fused:
        return None
    _req_cuda("ca_tattn_fused", "x w_frag gamma bias_pe w_out_frag bias_out residual", x, w_frag, gamma, bias_pe, w_out_frag, bias_out, residual)
    if x.dim() != 2 or x.stride(1) != 1 or x.shape[0] != b * frames * tokens or bias_pe.shape[0] < frames or bias_pe.stride(1) != 1:
        return None
    if w_out_frag is None and (bias_out is not None or residual is not None):
        return None
    if residual is not None and (residual.shape != x.shape or residual.stride(1) != 1 or residual.dtype != x.dtype):
        return None
    c = x.shape[1]
    o = torch.empty((x.shape[0], c), device=x.device, dtype=x.dtype)
    args = TattnArgs(x=_p(x), w_frag=_p(w_frag), gamma=_p(gamma), bias_pe=_p(bias_pe), o=_p(o), lda=x.stride(0), ldo=o.stride(0),
                     ld_bias_pe=bias_pe.stride(0), batch=b, frames=frames, tokens=tokens, heads=heads, c=c, ln_eps=float(ln_eps),
                     scale=float(scale), dtype=dt_code(x.dtype), w_out_frag=_p(w_out_frag), bias_out=_p(bias_out), residual=_p(residual),
                     ld_res=residual.stride(0) if residual is not None else 0)
    if not lib().ca_tattn_fused_supported(C.byref(args)):
        return None
    if _plan_sink is not None:
        _plan_sink.append("tattn_out128" if w_out_frag is not None else "tattn_fused128")
    check(lib().ca_tattn_fused(C.byref(args), _stream()), "ca_tattn_fused")
    return o


def xattn_pack_kv(kv: torch.Tensor, kv_batches: int, rows_per_batch: int, nk: int, scale: float, row_offset: int = 0,
                  out: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """The K | V rows of `kv` [kv_batches * rows_per_batch, 2 * 320] as the MFMA fragments ca_xattn_fused reads (ca_xattn_pack_kv,
    ABI v11; once per window and layer) -- or None for shapes the fused kernel does not take: 65..80 text keys, or (ABI v13) the 1..16
    image-prompt tokens of the IP-Adapter's second attention (row_offset = the first of them)."""
    if (not dispatch.xattn_fused or kv.dim() != 2 or kv.shape[1] != 640 or kv.stride(1) != 1 or not (64 < nk <= 80 or 1 <= nk <= 16)
            or kv.dtype not in (torch.float16, torch.bfloat16)):
        return None
    _req_cuda("ca_xattn_pack_kv", "kv", kv)
    dst = _out("ca_xattn_pack_kv", "out", out, (kv_batches, 8, _capi.XATTN_KV_FRAG_ELEMS), kv.dtype, kv.device)
    check(lib().ca_xattn_pack_kv(kv.data_ptr(), kv.stride(0), kv_batches, rows_per_batch, row_offset, nk, float(scale), dt_code(kv.dtype),
                                 dst.data_ptr(), _stream()), "ca_xattn_pack_kv")
    return dst


def xattn_fused(x: torch.Tensor, wq_frag: torch.Tensor, bias: Optional[torch.Tensor], kv_frag: torch.Tensor, images: int, tokens: int,
                frames_per_kv: int, kv_mod: int, nk: int, ln_eps: float, *, w_out_frag: Optional[torch.Tensor] = None,
                bias_out: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, kv_frag_ip: Optional[torch.Tensor] = None,
                nk_ip: int = 0, ip_scale: float = 1.0) -> Optional[torch.Tensor]:
    """o = softmax(q K^T scale) V with q = LayerNorm(x) Wq^T + bias in one launch (ca_xattn_fused, ABI v11: the text cross-attention of
    the 64x64-latent level) -- or None where the library does not take the arguments (the caller then runs the folded q GEMM and
    attention_cross).  kv_frag from xattn_pack_kv; image z uses its text batch (z // frames_per_kv) % kv_mod, kv_mod = 0 meaning `images`
    exactly as attention_cross does (the library refuses a launch that would index past the packed text batches).
    With w_out_frag (layers.frag_order_wout of to_out[0].weight; ABI v12) the launch also applies the output projection and returns
    y = o Wout^T + bias_out + residual.  With kv_frag_ip (xattn_pack_kv of the IP-Adapter's to_k_ip | to_v_ip projection of the nk_ip
    image-prompt tokens; ABI v13, needs w_out_frag) o = o_text + ip_scale * softmax(q K_ip^T scale) V_ip before that projection."""
    if not dispatch.xattn_fused or kv_frag is None:
        return None
    _req_cuda("ca_xattn_fused", "x wq_frag bias kv_frag w_out_frag bias_out residual kv_frag_ip", x, wq_frag, bias, kv_frag, w_out_frag, bias_out, residual, kv_frag_ip)
    if kv_frag_ip is not None and (w_out_frag is None or kv_frag_ip.shape != kv_frag.shape or kv_frag_ip.dtype != x.dtype or not kv_frag_ip.is_contiguous()):
        return None
    if x.dim() != 2 or x.stride(1) != 1 or x.shape[0] != images * tokens:
        return None
    if w_out_frag is None and (bias_out is not None or residual is not None):
        return None
    if residual is not None and (residual.shape != x.shape or residual.stride(1) != 1 or residual.dtype != x.dtype):
        return None
    _need(kv_frag.dtype == x.dtype and wq_frag.dtype == x.dtype, "ca_xattn_fused", "x, the packed Wq and the packed K/V must share one dtype (x, wq_frag, kv_frag)")
    c = x.shape[1]
    o = torch.empty((x.shape[0], c), device=x.device, dtype=x.dtype)
    args = XattnArgs(x=_p(x), wq_frag=_p(wq_frag), bias=_p(bias), kv_frag=_p(kv_frag), o=_p(o), lda=x.stride(0), ldo=o.stride(0), m=x.shape[0],
                     tokens=tokens, frames_per_kv=frames_per_kv, kv_mod=kv_mod if kv_mod > 0 else images, kv_batches=kv_frag.shape[0],
                     nk=nk, heads=8, c=c, ln_eps=float(ln_eps), dtype=dt_code(x.dtype), w_out_frag=_p(w_out_frag), bias_out=_p(bias_out),
                     residual=_p(residual), ld_res=residual.stride(0) if residual is not None else 0, kv_frag_ip=_p(kv_frag_ip),
                     nk_ip=nk_ip if kv_frag_ip is not None else 0, ip_scale=float(ip_scale) if kv_frag_ip is not None else 0.0)
    if not lib().ca_xattn_fused_supported(C.byref(args)):
        return None
    if _plan_sink is not None:
        _plan_sink.append(("xattn_ip_out128" if kv_frag_ip is not None else "xattn_out128") if w_out_frag is not None else "xattn_fused128")
    check(lib().ca_xattn_fused(C.byref(args), _stream()), "ca_xattn_fused")
    return o


def row_sums_of(t: torch.Tensor):
    """The partial row sums the GEMM that produced `t` left for the next LayerNorm, or None."""
    return getattr(t, "_row_sums", None)


def carry_row_sums(dst: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
    """`dst` is a view of `src` (same rows): keep the producer's row sums attached."""
    s = getattr(src, "_row_sums", None)
    if s is not None:
        dst._row_sums = s
    return dst


class RowStats:
    """LayerNorm statistics of the rows of `x`, not computed yet: `gemm(x, w, ln=(RowStats(x, eps), colsum))` lets the GEMM
    compute them itself while it streams x (ca_gemm_args.ln_eps, ABI v6: the K = 320 weight-resident kernel) and falls
    back to the separate pass (`row_stats`) where the library cannot."""

    def __init__(self, x: torch.Tensor, eps: float = 1e-5, sums=None):
        # sums = (partial sums [rows, parts, 2], parts) left by the GEMM that produced x (gemm(..., row_sums=True))
        self.x, self.eps, self._t, self.sums = x, float(eps), None, sums

    def tensor(self) -> torch.Tensor:
        if self._t is None:
            self._t = row_stats(self.x, self.eps)
        return self._t


def conv3x3(x: torch.Tensor, w: torch.Tensor, *, x2: Optional[torch.Tensor] = None,
            bias: Optional[torch.Tensor] = None, rowbias: Optional[torch.Tensor] = None,
            rows_per_group: int = 0, residual: Optional[torch.Tensor] = None, stride: int = 1,
            upsample: bool = False, alpha: float = 1.0, post_scale: float = 1.0, act: int = ACT_NONE,
            out_f32: bool = False, pad_asym: bool = False, w_wino: Optional[torch.Tensor] = None,
            out: Optional[torch.Tensor] = None, split_k: bool = True) -> torch.Tensor:
    """x: [images, H, W, Cin1] (+x2 [.., Cin2]); w: [Cout, 3, 3, Cin1+Cin2]; returns NHWC (written into `out` when given: a
    contiguous tensor of the output's shape and dtype that overlaps no operand).
    pad_asym: pad (0 before, 1 after) instead of 1/1 -- diffusers Downsample2D(padding=0).
    w_wino: the weight once more in Winograd form [16, Cout, Cin] (layers.HipConv3x3._winograd_weight / ca_pack_w_wino): the library
    then runs the shapes it names as F(2x2, 3x3) (ca_conv_args.w_wino, ABI v12)."""
    who = "ca_conv3x3"
    _req_cuda(who, "x w x2 bias rowbias residual w_wino out", x, w, x2, bias, rowbias, residual, w_wino, out)
    images, hin, win, cin1 = _t(who, "x", x, None, _D4)
    _t(who, "w", w, None, _D4)
    cin2 = 0
    if x2 is not None:
        _need(x2.is_contiguous() and x2.shape[:3] == x.shape[:3] and x2.dtype == x.dtype, who, "x2 must be contiguous [images, H, W, Cin2] of x's dtype", x2)
        cin2 = x2.shape[3]
    cout = w.shape[0]
    _t(who, "w", w, x.dtype, (None, 3, 3, cin1 + cin2), contiguous=False)
    hl, wl = (hin * 2, win * 2) if upsample else (hin, win)
    pad = 1 if pad_asym else 2
    hout, wout = (hl + pad - 3) // stride + 1, (wl + pad - 3) // stride + 1
    if out is not None:
        _t(who, "out", out, torch.float32 if out_f32 else x.dtype, (images, hout, wout, cout))
    ld_res = 0
    if residual is not None:
        if not (residual.dtype == x.dtype and residual.is_contiguous() and residual.numel() == images * hout * wout * cout):
            _need(False, who, f"residual {tuple(residual.shape)} {residual.dtype} contiguous={residual.is_contiguous()} vs output {(images, hout, wout, cout)} {x.dtype}")
        ld_res = cout
    if rowbias is not None:
        _need(rowbias.dtype == torch.float32 and rowbias.dim() == 2 and rowbias.shape[1] == cout and rows_per_group > 0, who,
              "rowbias must be float32 [groups, Cout] with rows_per_group > 0", rowbias)
    if bias is not None:
        _t(who, "bias", bias, torch.float32, numel=cout, contiguous=False)
    y = torch.empty((images, hout, wout, cout), device=x.device, dtype=torch.float32 if out_f32 else x.dtype) if out is None else out
    args = ConvArgs(x=_p(x), x2=_p(x2), w=_p(w), y=_p(y), bias=_p(bias), rowbias=_p(rowbias),
                    residual=_p(residual), ld_res=ld_res,
                    ld_rowbias=rowbias.stride(0) if rowbias is not None else 0, images=images, hin=hin,
                    win=win, cin1=cin1, cin2=cin2, cout=cout, stride=stride, upsample=int(upsample),
                    rows_per_group=rows_per_group, alpha=alpha, post_scale=post_scale, act=act,
                    out_f32=int(out_f32), dtype=dt_code(x.dtype), pad_asym=int(pad_asym))
    if w_wino is not None and dispatch.conv_winograd:
        _t(who, "w_wino", w_wino, x.dtype, (16, cout, cin1 + cin2))
        args.w_wino = _p(w_wino)
    # split_k=False hands over no workspace, and the library then never splits K (whether it would depends on the number of images): the
    # order of an output's sum is the same whatever the batch (modconv3x3's composed form)
    wbytes = int(lib().ca_conv3x3_workspace_bytes(C.byref(args))) if split_k else 0
    if wbytes > 0:  # split-K slabs for the small-M levels (allocator-cached, stream-ordered)
        ws = torch.empty((wbytes,), device=x.device, dtype=torch.uint8)
        args.workspace, args.workspace_bytes = _p(ws), wbytes
    _record_plan(lib().ca_conv3x3_plan_name, args)
    check(lib().ca_conv3x3(C.byref(args), _stream()), "ca_conv3x3")
    return y


def _up2_args(x, w_phase, bias, residual, alpha, y=None) -> ConvArgs:
    """ca_conv_args of the phase form; without an output yet (the `_supported` query: pointers are only checked for alignment) y = x."""
    images, hin, win, cin = x.shape
    cout = w_phase.shape[1]
    return ConvArgs(x=_p(x), w=_p(w_phase), y=_p(y) if y is not None else _p(x), bias=_p(bias), residual=_p(residual),
                    ld_res=cout if residual is not None else 0, images=images, hin=hin, win=win, cin1=cin, cin2=0, cout=cout, stride=1,
                    upsample=1, rows_per_group=0, alpha=alpha, post_scale=1.0, act=ACT_NONE, out_f32=0, dtype=dt_code(x.dtype), pad_asym=0)


def conv_up2_phase_supported(x: torch.Tensor, w_phase: torch.Tensor, *, bias: Optional[torch.Tensor] = None,
                             residual: Optional[torch.Tensor] = None, alpha: float = 1.0) -> bool:
    """Does the library take this nearest-x2 upsampling convolution as four phase convolutions by default (ca_conv_up2_phase_supported:
    the kernel implements the arguments and the form pays at the size)?  No launch, no device access."""
    if x.dim() != 4 or w_phase.dim() != 5 or not x.is_contiguous() or x.dtype not in (torch.float16, torch.bfloat16):
        return False
    return bool(lib().ca_conv_up2_phase_supported(C.byref(_up2_args(x, w_phase, bias, residual, alpha))))


def conv_up2_phase(x: torch.Tensor, w_phase: torch.Tensor, *, bias: Optional[torch.Tensor] = None,
                   residual: Optional[torch.Tensor] = None, alpha: float = 1.0) -> torch.Tensor:
    """conv3x3(nearest_x2(x)) as four 2x2 phase convolutions in one launch (ca_conv_up2_phase): x [images, H, W, Cin],
    w_phase [4, Cout, 2, 2, Cin] (layers.phase_weights of the 3x3 weight); returns [images, 2H, 2W, Cout].  Runs every shape the
    kernel implements (Cin % 64 == 0, Cout % 320 == 0); whether the form PAYS at a size is conv_up2_phase_supported's answer."""
    _req_cuda("ca_conv_up2_phase", "x w_phase bias residual", x, w_phase, bias, residual)
    images, hin, win, cin = _t("ca_conv_up2_phase", "x", x, None, _D4)
    cout = _t("ca_conv_up2_phase", "w_phase", w_phase, x.dtype, _D5)[1]
    _t("ca_conv_up2_phase", "w_phase", w_phase, None, (4, cout, 2, 2, cin))
    if residual is not None:
        _t("ca_conv_up2_phase", "residual", residual, x.dtype, numel=images * 2 * hin * 2 * win * cout)
    if bias is not None:
        _t("ca_conv_up2_phase", "bias", bias, torch.float32, numel=cout, contiguous=False)
    y = torch.empty((images, 2 * hin, 2 * win, cout), device=x.device, dtype=x.dtype)
    args = _up2_args(x, w_phase, bias, residual, alpha, y)
    _record_plan(lib().ca_conv_up2_phase_plan_name, args)
    check(lib().ca_conv_up2_phase(C.byref(args), _stream()), "ca_conv_up2_phase")
    return y


_gn_wino_declined: dict = {}  # shapes group_norm_conv3x3_wino has declined (the library's answer depends on nothing else)


def group_norm_conv3x3_wino(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, w: torch.Tensor, w_wino: torch.Tensor, *,
                            x2: Optional[torch.Tensor] = None, groups: int = 32, eps: float = 1e-5, act: int = ACT_NONE,
                            bias: Optional[torch.Tensor] = None, rowbias: Optional[torch.Tensor] = None, rows_per_group: int = 0,
                            residual: Optional[torch.Tensor] = None, post_scale: float = 1.0) -> Optional[torch.Tensor]:
    """conv3x3(GroupNorm(+act)(cat(x, x2))) where the convolution takes the Winograd route AND the one-launch GroupNorm applies: the
    GroupNorm writes the transformed input V itself (ca_groupnorm_args.wino_v, ABI v12) and the convolution starts at its GEMM
    (ca_conv_args.x_is_wino_v) -- the normalised tensor is never written.  Per-image statistics only.  None where either side
    declines: the caller runs group_norm, then conv3x3."""
    if not (dispatch.conv_winograd and dispatch.gn_winograd):
        return None
    _req_cuda("ca_groupnorm", "x gamma beta w w_wino x2 bias rowbias residual", x, gamma, beta, w, w_wino, x2, bias, rowbias, residual)
    if x.dim() != 4 or not x.is_contiguous() or x.dtype != torch.float16 or (x2 is not None and (not x2.is_contiguous() or x2.shape[:3] != x.shape[:3])):
        return None
    images, h, w_, c1 = x.shape
    c2 = 0 if x2 is None else x2.shape[3]
    c, cout = c1 + c2, w.shape[0]
    tiles = images * (h // 2) * (w_ // 2)
    # the cheap declines first (the probes only need non-null pointers: x stands in for V and y until both sides have accepted;
    # the decision is remembered per shape, so a resnet whose level the route declines costs two dictionary look-ups per eager step)
    key = (images, h, w_, c1, c2, cout, groups, act, rowbias is not None, residual is not None, rows_per_group)
    if _gn_wino_declined.get(key):
        return None
    cargs = ConvArgs(x=_p(x), x2=None, w=_p(w), y=_p(x), bias=_p(bias), rowbias=_p(rowbias), residual=_p(residual),
                     ld_res=cout if residual is not None else 0, ld_rowbias=rowbias.stride(0) if rowbias is not None else 0, images=images, hin=h,
                     win=w_, cin1=c, cin2=0, cout=cout, stride=1, upsample=0, rows_per_group=rows_per_group, alpha=1.0, post_scale=post_scale,
                     act=ACT_NONE, out_f32=0, dtype=dt_code(x.dtype), pad_asym=0, w_wino=_p(w_wino), x_is_wino_v=1)
    # would the convolution take the Winograd route (given enough workspace)?  ca_conv3x3_workspace_bytes alone cannot tell: it also
    # answers > 0 for the split-K plan of a shape the route declines
    cargs.workspace, cargs.workspace_bytes = _p(x), 1 << 60
    buf = C.create_string_buffer(64)
    if lib().ca_conv3x3_plan_name(C.byref(cargs), buf, 64) != 0 or not buf.value.decode().startswith("wino"):
        _gn_wino_declined[key] = True
        return None
    wbytes = int(lib().ca_conv3x3_workspace_bytes(C.byref(cargs)))
    gargs = GroupNormArgs(x=_p(x), x2=_p(x2), y=None, gamma=_p(gamma), beta=_p(beta), partials=None, images=images, hw=h * w_, c1=c1, c2=c2,
                          groups=groups, frames_per_stat=1, eps=eps, act=act, dtype=dt_code(x.dtype), wino_v=_p(x), wino_h=h, wino_w=w_)
    if wbytes <= 0 or not lib().ca_groupnorm_wino_supported(C.byref(gargs)):
        _gn_wino_declined[key] = True
        return None
    if residual is not None:
        _t("ca_conv3x3", "residual", residual, x.dtype, numel=images * h * w_ * cout)
    y = torch.empty((images, h, w_, cout), device=x.device, dtype=x.dtype)
    v = torch.empty((16, tiles, c), device=x.device, dtype=x.dtype)
    ws = torch.empty((wbytes,), device=x.device, dtype=torch.uint8)
    cargs.x, cargs.y, gargs.wino_v = _p(v), _p(y), _p(v)
    cargs.workspace, cargs.workspace_bytes = _p(ws), wbytes
    if _plan_sink is not None:
        buf = C.create_string_buffer(64)
        _plan_sink.append("gn_" + (buf.value.decode() if lib().ca_conv3x3_plan_name(C.byref(cargs), buf, 64) == 0 else "?"))
    check(lib().ca_groupnorm(C.byref(gargs), _stream()), "ca_groupnorm(wino)")
    check(lib().ca_conv3x3(C.byref(cargs), _stream()), "ca_conv3x3(wino, V given)")
    return y


def group_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, *, x2: Optional[torch.Tensor] = None,
               groups: int = 32, frames_per_stat: int = 1, eps: float = 1e-5, act: int = ACT_NONE) -> torch.Tensor:
    """GroupNorm (+SiLU) over NHWC x (optionally channel-concatenated with x2)."""
    _req_cuda("ca_groupnorm", "x gamma beta x2", x, gamma, beta, x2)
    images, h, w_, c1 = _t("ca_groupnorm", "x", x, None, _D4)
    c2 = 0
    if x2 is not None:
        _need(x2.is_contiguous() and x2.shape[:3] == x.shape[:3] and x2.dtype == x.dtype, "ca_groupnorm", "x2 must be contiguous [images, H, W, C2] of x's dtype", x2)
        c2 = x2.shape[3]
    c = c1 + c2
    _t("ca_groupnorm", "gamma", gamma, torch.float32, numel=c, contiguous=False)
    _t("ca_groupnorm", "beta", beta, torch.float32, numel=c, contiguous=False)
    y = torch.empty((images, h, w_, c), device=x.device, dtype=x.dtype)
    nfl = lib().ca_groupnorm_partials_floats(images, h * w_, frames_per_stat, groups)
    partials = torch.empty((max(int(nfl), 1),), device=x.device, dtype=torch.float32)
    args = GroupNormArgs(x=_p(x), x2=_p(x2), y=_p(y), gamma=_p(gamma), beta=_p(beta), partials=_p(partials),
                         images=images, hw=h * w_, c1=c1, c2=c2, groups=groups,
                         frames_per_stat=frames_per_stat, eps=eps, act=act, dtype=dt_code(x.dtype))
    check(lib().ca_groupnorm(C.byref(args), _stream()), "ca_groupnorm")
    return y


def layer_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, *, pos: Optional[torch.Tensor] = None,
               rows_per_frame: int = 1, frames: int = 1, eps: float = 1e-5) -> torch.Tensor:
    _req_cuda("ca_layernorm", "x gamma beta pos", x, gamma, beta, pos)
    rows, c = _t("ca_layernorm", "x", x, None, _D2)
    _need(gamma.dtype == torch.float32 and beta.dtype == torch.float32, "ca_layernorm", "gamma and beta must be float32")
    if pos is not None:
        _t("ca_layernorm", "pos", pos, torch.float32, (frames, c))
    y = torch.empty_like(x)
    args = LayerNormArgs(x=_p(x), y=_p(y), gamma=_p(gamma), beta=_p(beta), pos=_p(pos), rows=rows, c=c,
                         rows_per_frame=rows_per_frame, frames=frames, eps=eps, dtype=dt_code(x.dtype))
    check(lib().ca_layernorm(C.byref(args), _stream()), "ca_layernorm")
    return y


def row_stats(x: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """(mean, rstd) of every row of x [rows, C] as fp32 [rows, 2]: the statistics of a LayerNorm that is
    folded into the following GEMM (gemm(..., ln=(stats, colsum)))."""
    _req_cuda("ca_layernorm", "x", x)
    rows, c = _t("ca_layernorm", "x", x, None, _D2)
    st = torch.empty((rows, 2), device=x.device, dtype=torch.float32)
    args = LayerNormArgs(x=_p(x), y=None, gamma=None, beta=None, pos=None, rows=rows, c=c, rows_per_frame=1, frames=1,
                         eps=eps, dtype=dt_code(x.dtype), stats=_p(st))
    check(lib().ca_layernorm(C.byref(args), _stream()), "ca_layernorm(stats)")
    return st


def attention_raw(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, o: torch.Tensor, *, q_off: int, k_off: int,
                  v_off: int, o_off: int, q_strides, o_strides, k_strides, inner_count: int, kv_inner_count: int,
                  kv_div: int, batches: int, heads: int, head_dim: int, nq: int, nk: int, scale: float,
                  out_scale: float = 1.0, accumulate: bool = False, kv_mod: int = 0, causal: bool = False,
                  key_mask: Optional[torch.Tensor] = None) -> None:
    """Direct mapping of ca_attention. *_off are element offsets into the given storage tensors;
    *_strides = (outer, inner, row) in elements.  key_mask: uint8 [batches, nk], 0 = key invisible (ca_attn_args.key_mask)."""
    _req_cuda("ca_attention", "q k v o key_mask", q, k, v, o, key_mask)
    if key_mask is not None:
        _need(key_mask.dtype == torch.uint8 and key_mask.dim() == 2 and key_mask.shape == (batches, nk) and key_mask.stride(1) == 1, "ca_attention",
              "key_mask must be uint8 [batches, nk] with unit column stride", key_mask)
    es = q.element_size()
    args = AttnArgs(q=q.data_ptr() + q_off * es, k=k.data_ptr() + k_off * es, v=v.data_ptr() + v_off * es,
                    o=o.data_ptr() + o_off * es,
                    q_outer=q_strides[0], q_inner=q_strides[1], q_row=q_strides[2],
                    o_outer=o_strides[0], o_inner=o_strides[1], o_row=o_strides[2],
                    k_outer=k_strides[0], k_inner=k_strides[1], k_row=k_strides[2],
                    inner_count=inner_count, kv_inner_count=kv_inner_count, kv_div=kv_div,
                    kv_mod=kv_mod if kv_mod > 0 else batches, batches=batches, heads=heads, head_dim=head_dim, nq=nq, nk=nk, scale=scale, out_scale=out_scale,
                    accumulate=int(accumulate), dtype=dt_code(q.dtype), causal=int(causal),
                    key_mask=_p(key_mask), key_mask_stride=key_mask.stride(0) if key_mask is not None else 0)
    _record_plan(lib().ca_attention_plan_name, args)
    check(lib().ca_attention(C.byref(args), _stream()), "ca_attention")


def attention_spatial(qkv: torch.Tensor, images: int, tokens: int, heads: int, causal: bool = False,
                      key_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Self-attention per image. qkv: [images*tokens, 3C] (q | k | v); returns [images*tokens, C].
    key_mask: uint8 [images, tokens], 0 = that token is invisible as a key (transformers' attention_mask)."""
    _req_cuda("ca_attention", "qkv", qkv)
    c = qkv.shape[1] // 3
    d = c // heads
    o = torch.empty((images * tokens, c), device=qkv.device, dtype=qkv.dtype)
    ld = qkv.stride(0)
    attention_raw(qkv, qkv, qkv, o, q_off=0, k_off=c, v_off=2 * c, o_off=0,
                  q_strides=(tokens * ld, 0, ld), o_strides=(tokens * c, 0, c), k_strides=(tokens * ld, 0, ld),
                  inner_count=1, kv_inner_count=1, kv_div=1, batches=images, heads=heads, head_dim=d,
                  nq=tokens, nk=tokens, scale=d ** -0.5, causal=causal, key_mask=key_mask)
    return o


def attention_cross(q: torch.Tensor, kv: torch.Tensor, images: int, tokens: int, heads: int, kv_tokens: int,
                    kv_rows_per_batch: int, frames_per_kv: int, *, out: Optional[torch.Tensor] = None,
                    out_scale: float = 1.0, accumulate: bool = False, kv_row_offset: int = 0,
                    kv_mod: int = 0, key_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Cross-attention. q: [images*tokens, C]; kv: [kv_batches*kv_rows_per_batch, 2C] (k | v).
    Image z uses kv batch (z // frames_per_kv) % kv_mod, rows [kv_row_offset, kv_row_offset + kv_tokens).
    key_mask: uint8 [images, kv_tokens], 0 = that key is invisible to the image's queries."""
    _req_cuda("ca_attention", "q kv out", q, kv, out)
    c = q.shape[1]
    d = c // heads
    if out is None:
        out = torch.empty_like(q)
    ldk = kv.stride(0)
    attention_raw(q, kv, kv, out, q_off=0, k_off=kv_row_offset * ldk, v_off=kv_row_offset * ldk + c, o_off=0,
                  q_strides=(tokens * q.stride(0), 0, q.stride(0)), o_strides=(tokens * out.stride(0), 0, out.stride(0)),
                  k_strides=(kv_rows_per_batch * ldk, 0, ldk), inner_count=1, kv_inner_count=1,
                  kv_div=frames_per_kv, batches=images, heads=heads, head_dim=d, nq=tokens, nk=kv_tokens,
                  scale=d ** -0.5, out_scale=out_scale, accumulate=accumulate, kv_mod=kv_mod, key_mask=key_mask)
    return out


def attention_temporal(qkv: torch.Tensor, b: int, frames: int, tokens: int, heads: int) -> torch.Tensor:
    """Attention over the frame axis. qkv rows are in (b f n) order: [b*frames*tokens, 3C]."""
    _req_cuda("ca_attention", "qkv", qkv)
    c = qkv.shape[1] // 3
    d = c // heads
    o = torch.empty((b * frames * tokens, c), device=qkv.device, dtype=qkv.dtype)
    ld = qkv.stride(0)
    attention_raw(qkv, qkv, qkv, o, q_off=0, k_off=c, v_off=2 * c, o_off=0,
                  q_strides=(frames * tokens * ld, ld, tokens * ld), o_strides=(frames * tokens * c, c, tokens * c),
                  k_strides=(frames * tokens * ld, ld, tokens * ld), inner_count=tokens, kv_inner_count=tokens,
                  kv_div=1, batches=b * tokens, heads=heads, head_dim=d, nq=frames, nk=frames, scale=d ** -0.5)
    return o


def perceiver_attn(q: torch.Tensor, x_k: torch.Tensor, x_v: torch.Tensor, l_k: torch.Tensor, l_v: torch.Tensor, heads: int, *,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """o = softmax(head_dim^-0.5 q [k_x ; k_l]^T) [v_x ; v_l] per (batch, head) under ONE softmax (ca_perceiver_attn: the Resampler of
    IP-Adapter Plus).  q [B, nq, heads * 64]; x_k / x_v [B, n_x, heads * 64] views of one buffer with the same strides (a column slice of
    the all-layers K|V GEMM), l_k / l_v [B, n_l, heads * 64] likewise (the layer's q|k|v GEMM); the last dimension contiguous.  Returns
    [B, nq, heads * 64] (`out`: any view with a contiguous last dimension)."""
    who = "ca_perceiver_attn"
    _req_cuda(who, "q x_k x_v l_k l_v out", q, x_k, x_v, l_k, l_v, out)
    b, nq, inner = q.shape
    for name, t in (("q", q), ("x_k", x_k), ("x_v", x_v), ("l_k", l_k), ("l_v", l_v)):
        _need(t.dim() == 3 and t.shape[0] == b and t.shape[2] == inner and t.stride(2) == 1 and t.dtype == q.dtype, who,
              name + " must be [B, n, heads * 64] of q's dtype with a contiguous last dimension", t)
    _need(x_k.shape == x_v.shape and x_k.stride() == x_v.stride() and l_k.shape == l_v.shape and l_k.stride() == l_v.stride(), who,
          "x_k / x_v (and l_k / l_v) must be views of one buffer with the same shape and strides")
    _need(inner % heads == 0, who, "heads must divide the last dimension of q")
    if out is None:
        out = torch.empty((b, nq, inner), device=q.device, dtype=q.dtype)
    _need(out.shape == (b, nq, inner) and out.stride(2) == 1 and out.dtype == q.dtype, who, "out must be [B, nq, heads * 64] of q's dtype with a contiguous last dimension", out)
    d = inner // heads
    es = q.element_size()
    args = PerceiverAttnArgs(q=_p(q), x=_p(x_k), l=_p(l_k), o=_p(out), q_row=q.stride(1), q_batch=q.stride(0),
                             x_row=x_k.stride(1), x_batch=x_k.stride(0), x_v_off=(x_v.data_ptr() - x_k.data_ptr()) // es,
                             l_row=l_k.stride(1), l_batch=l_k.stride(0), l_v_off=(l_v.data_ptr() - l_k.data_ptr()) // es,
                             o_row=out.stride(1), o_batch=out.stride(0), batches=b, heads=heads, head_dim=d, nq=nq, n_x=x_k.shape[1],
                             n_l=l_k.shape[1], scale=float(d ** -0.5), dtype=dt_code(q.dtype))
    if _plan_sink is not None:
        _plan_sink.append("perceiver_attn")
    check(lib().ca_perceiver_attn(C.byref(args), _stream()), "ca_perceiver_attn")
    return out


def add_bcast(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a + b where b is tiled along the leading dimension (b.numel() divides a.numel())."""
    _req_cuda("ca_add_bcast", "a b", a, b)
    _need(a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype and a.numel() % b.numel() == 0, "ca_add_bcast",
          "a and b must be contiguous, of one dtype, and b.numel() must divide a.numel()", b)
    if out is None:
        out = torch.empty_like(a)
    check(lib().ca_add_bcast(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), b.numel(), dt_code(a.dtype),
                             _stream()), "ca_add_bcast")
    return out


def repeat_batch(x: torch.Tensor, times: int = 2) -> torch.Tensor:
    """torch.cat([x] * times) along dim 0 with one read of x (ca_repeat, ABI v8; context.dispatch.repeat_kernel = False: torch.cat, for A/B runs)."""
    if not dispatch.repeat_kernel:
        return torch.cat([x] * times)
    _req_cuda("ca_repeat", "x", x)
    if not x.is_contiguous():
        x = x.contiguous()  # (a strided view: one gather first; sizes / alignments the 16-byte kernel cannot take go byte-wise in the library)
    if x.numel() == 0:
        return x.new_empty((times * x.shape[0],) + tuple(x.shape[1:]))
    out = torch.empty((times * x.shape[0],) + tuple(x.shape[1:]), device=x.device, dtype=x.dtype)
    check(lib().ca_repeat(x.data_ptr(), out.data_ptr(), x.numel() * x.element_size(), times, _stream()), "ca_repeat")
    return out


def softmax_rows(x: torch.Tensor, dtype: torch.dtype, scale: float = 1.0) -> torch.Tensor:
    """Row softmax of an fp32 [rows, cols] score matrix (last dim contiguous), output in `dtype`."""
    _req_cuda("ca_softmax_rows", "x", x)
    _need(x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1, "ca_softmax_rows", "x must be float32 [rows, cols] with unit column stride", x)
    y = torch.empty(x.shape, device=x.device, dtype=dtype)
    check(lib().ca_softmax_rows(x.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1], x.stride(0), y.stride(0), float(scale),
                                dt_code(dtype), _stream()), "ca_softmax_rows")
    return y


def silu_f32(x: torch.Tensor) -> torch.Tensor:
    _req_cuda("ca_silu_f32", "x", x)
    _t("ca_silu_f32", "x", x, torch.float32)
    y = torch.empty_like(x)
    check(lib().ca_silu_f32(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "ca_silu_f32")
    return y


def timestep_embedding(t, batch: int, dim: int, dtype: torch.dtype, device) -> torch.Tensor:
    """t: python number (same for the whole batch) or fp32 device tensor [batch]."""
    out = torch.empty((batch, dim), device=device, dtype=dtype)
    if isinstance(t, torch.Tensor):
        _req_cuda("ca_timestep_embedding", "t", t)
        _t("ca_timestep_embedding", "t", t, torch.float32, numel=batch, contiguous=False)
        check(lib().ca_timestep_embedding(t.data_ptr(), 0.0, out.data_ptr(), batch, dim, dt_code(dtype), _stream()),
              "ca_timestep_embedding")
    else:
        check(lib().ca_timestep_embedding(None, float(t), out.data_ptr(), batch, dim, dt_code(dtype), _stream()),
              "ca_timestep_embedding")
    return out


def latents_to_nhwc(latents: torch.Tensor, cpad: int, rep: int, in_scale: float, dtype: torch.dtype,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _req_cuda("ca_latents_to_nhwc", "latents", latents)
    b0, c, f, h, w = _t("ca_latents_to_nhwc", "latents", latents, torch.float32, _D5)
    out = _out("ca_latents_to_nhwc", "out", out, (rep * b0 * f, h, w, cpad), dtype, latents.device)
    check(lib().ca_latents_to_nhwc(latents.data_ptr(), out.data_ptr(), b0, c, f, h, w, cpad, rep, in_scale,
                                   dt_code(dtype), _stream()), "ca_latents_to_nhwc")
    return out


def nhwc_to_ncfhw_f32(x: torch.Tensor, b: int, c: int, f: int) -> torch.Tensor:
    """x: [b*f, h, w, ldx] (act dtype or fp32) -> [b, c, f, h, w] fp32."""
    _req_cuda("ca_nhwc_to_ncfhw_f32", "x", x)
    _, h, w, ldx = _t("ca_nhwc_to_ncfhw_f32", "x", x, None, _D4)
    out = torch.empty((b, c, f, h, w), device=x.device, dtype=torch.float32)
    is_f32 = x.dtype == torch.float32
    check(lib().ca_nhwc_to_ncfhw_f32(x.data_ptr(), out.data_ptr(), b, c, f, h, w, ldx, int(is_f32),
                                     CA_BF16 if is_f32 else dt_code(x.dtype), _stream()), "ca_nhwc_to_ncfhw_f32")
    return out


_KIND = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def ncfhw_to_nhwc(x: torch.Tensor, cpad: int, dtype: torch.dtype) -> torch.Tensor:
    """x: [b, c, f, h, w] any strides, fp32/fp16/bf16 -> [b*f, h, w, cpad] `dtype` (zero padded)."""
    _req_cuda("ca_ncfhw_to_nhwc", "x", x)
    b, c, f, h, w = _t("ca_ncfhw_to_nhwc", "x", x, _KIND, _D5, contiguous=False)
    out = torch.empty((b * f, h, w, cpad), device=x.device, dtype=dtype)
    st = (C.c_int64 * 5)(*x.stride())
    check(lib().ca_ncfhw_to_nhwc(x.data_ptr(), _KIND[x.dtype], st, out.data_ptr(), b, c, f, h, w, cpad,
                                 dt_code(dtype), _stream()), "ca_ncfhw_to_nhwc")
    return out


def cfg_scheduler_step(eps: torch.Tensor, rep: int, guidance: float, latents: torch.Tensor,
                       noise: Optional[torch.Tensor], coef, clip: float = 0.0, want_denoised: bool = False):
    """eps: NHWC fp32 [rep*f, h, w, ld]; latents/noise: [1, c, f, h, w] fp32. Returns (prev, denoised|None)."""
    _req_cuda("ca_cfg_scheduler_step", "eps latents noise", eps, latents, noise)
    _t("ca_cfg_scheduler_step", "eps", eps, torch.float32)
    _t("ca_cfg_scheduler_step", "latents", latents, torch.float32)
    _, c, f, h, w = latents.shape
    _need(latents.shape[0] == 1 and eps.shape[0] == rep * f, "ca_cfg_scheduler_step", "latents must be [1, c, f, h, w] and eps [rep * f, h, w, ld]", eps)
    if noise is not None:
        _t("ca_cfg_scheduler_step", "noise", noise, torch.float32, tuple(latents.shape))
    prev = torch.empty_like(latents)
    den = torch.empty_like(latents) if want_denoised else None
    cf = (C.c_float * 7)(*[float(v) for v in coef])
    check(lib().ca_cfg_scheduler_step(eps.data_ptr(), eps.shape[3], rep, float(guidance), latents.data_ptr(),
                                      _p(noise), prev.data_ptr(), _p(den), c, f, h, w, cf, float(clip), _stream()),
          "ca_cfg_scheduler_step")
    return prev, den


def lincomb(terms, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = sum_k coef_k * x_k for fp32 tensors of one shape; terms: [(tensor, coef), ...] (1..8). ca_lincomb."""
    xs = [t for t, _ in terms]
    _req_cuda("ca_lincomb", "terms", *xs)
    _need(1 <= len(terms) <= 8 and all(t.dtype == torch.float32 and t.is_contiguous() and t.shape == xs[0].shape for t in xs), "ca_lincomb",
          "terms must be 1..8 contiguous float32 tensors of one shape")
    if out is None:
        out = torch.empty_like(xs[0])
    ptrs = (C.c_void_p * len(xs))(*[t.data_ptr() for t in xs])
    cf = (C.c_float * len(xs))(*[float(c) for _, c in terms])
    check(lib().ca_lincomb(out.data_ptr(), ptrs, cf, len(xs), xs[0].numel(), _stream()), "ca_lincomb")
    return out


def cfg_combined_eps(eps: torch.Tensor, rep: int, guidance: float, latents: torch.Tensor) -> torch.Tensor:
    """The classifier-free-guidance combine alone: eps NHWC fp32 [rep*f,h,w,ld] -> [1,c,f,h,w] fp32
    (ca_cfg_scheduler_step with prev := eps; the multistep samplers keep it as history)."""
    e, _ = cfg_scheduler_step(eps, rep, guidance, latents, None, [0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0], 0.0)
    return e


# ---- ABI v14: the RRDBNet upscaler (controlanimate_amd/upscaler.py) ----------------------------------------------------------

def conv3x3_narrow(x: torch.Tensor, w: torch.Tensor, y: torch.Tensor, *, cin: int, cout: int, bias: Optional[torch.Tensor] = None,
                   channel_offset: int = 0, upsample: bool = False, leaky_relu: bool = False, s0: float = 1.0,
                   r1: Optional[torch.Tensor] = None, s1: float = 0.0, r2: Optional[torch.Tensor] = None, s2: float = 0.0,
                   out_u8: bool = False) -> torch.Tensor:
    """ca_conv3x3_narrow into the caller's `y`: x [images, H, W, ldx] (its first `cin` channels are read), w packed
    [round_up(cout, 16), 3, 3, round_up(cin, 32)], y [images, Hout, Wout, ldy] (channels channel_offset .. + cout written) or, with
    out_u8, uint8 [images, Hout, Wout, 3].  r1 / r2 [images, Hout, Wout, ld] (their first cout channels are read)."""
    who = "ca_conv3x3_narrow"
    _req_cuda(who, "x w y bias r1 r2", x, w, y, bias, r1, r2)
    for name, t in (("x", x), ("w", w), ("y", y), ("r1", r1), ("r2", r2)):
        _need(t is None or t.is_contiguous(), who, name + " must be contiguous", t)
    images, hin, win, ldx = x.shape
    hout, wout = (2 * hin, 2 * win) if upsample else (hin, win)
    if out_u8:
        _t(who, "y", y, torch.uint8, (images, hout, wout, 3), contiguous=False)
    else:
        _need(y.dtype == x.dtype and tuple(y.shape[:3]) == (images, hout, wout), who, "y must be [images, Hout, Wout, ldy] of x's dtype", y)
    for name, r in (("r1", r1), ("r2", r2)):
        _need(r is None or (r.dtype == x.dtype and tuple(r.shape[:3]) == (images, hout, wout)), who, name + " must be [images, Hout, Wout, ld] of x's dtype", r)
    _t(who, "w", w, x.dtype, ((cout + 15) // 16 * 16, 3, 3, (cin + 31) // 32 * 32), contiguous=False)
    if bias is not None:
        _t(who, "bias", bias, torch.float32, numel=cout, contiguous=False)
    args = ConvNarrowArgs(x=_p(x), w=_p(w), y=_p(y), bias=_p(bias), r1=_p(r1), r2=_p(r2), ldx=ldx, ldy=0 if out_u8 else y.shape[3],
                          ld_r1=r1.shape[3] if r1 is not None else 0, ld_r2=r2.shape[3] if r2 is not None else 0,
                          images=images, hin=hin, win=win, cin=cin, cout=cout, channel_offset=channel_offset, upsample=int(upsample),
                          leaky_relu=int(leaky_relu), s0=s0, s1=s1, s2=s2, out_u8=int(out_u8), dtype=dt_code(x.dtype))
    _record_plan(lib().ca_conv3x3_narrow_plan_name, args)
    check(lib().ca_conv3x3_narrow(C.byref(args), _stream()), "ca_conv3x3_narrow")
    return y


def rgb8_to_nhwc(frames: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """uint8 [n, H, W, 3] -> [n, H, W, 8] `dtype`, channels reversed, /255, zero padded (ca_rgb8_to_nhwc)."""
    _req_cuda("ca_rgb8_to_nhwc", "frames", frames)
    n, h, w = _req_rgb8("ca_rgb8_to_nhwc", "frames", frames)
    out = torch.empty((n, h, w, 8), device=frames.device, dtype=dtype)
    check(lib().ca_rgb8_to_nhwc(_p(frames), _p(out), n, h, w, dt_code(dtype), _stream()), "ca_rgb8_to_nhwc")
    return out


def resize_lanczos4_u8(frames: torch.Tensor, dh: int, dw: int, xofs: torch.Tensor, alpha: torch.Tensor, yofs: torch.Tensor,
                       beta: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [n, sh, sw, 3] -> [n, dh, dw, 3] with the INTER_LANCZOS4 tables of upscaler.lanczos4_tables (ca_resize_lanczos4_u8); written
    into `out` when given."""
    _req_cuda("ca_resize_lanczos4_u8", "frames xofs alpha yofs beta out", frames, xofs, alpha, yofs, beta, out)
    n, sh, sw = _req_rgb8("ca_resize_lanczos4_u8", "frames", frames)
    for name, t, dt, count in (("xofs", xofs, torch.int32, dw), ("alpha", alpha, torch.int16, 8 * dw), ("yofs", yofs, torch.int32, dh), ("beta", beta, torch.int16, 8 * dh)):
        _t("ca_resize_lanczos4_u8", name, t, dt, numel=count, contiguous=False)
    out = _out("ca_resize_lanczos4_u8", "out", out, (n, dh, dw, 3), torch.uint8, frames.device)
    check(lib().ca_resize_lanczos4_u8(_p(frames), _p(out), n, sh, sw, dh, dw, _p(xofs), _p(alpha), _p(yofs), _p(beta), _stream()),
          "ca_resize_lanczos4_u8")
    return out


# ---- ABI v15: the colour match (controlanimate_amd/color_match.py) --------------------------------------------------------------

def color_match_workspace_bytes(images: int, pixels: int) -> int:
    """ca_color_match_workspace_bytes; the sort of `segments` runs needs images = (segments + 2) // 3."""
    need = lib().ca_color_match_workspace_bytes(images, pixels)
    if need <= 0:
        raise _capi.CAHipError(f"ca_color_match_workspace_bytes: images={images} pixels={pixels} out of range")
    return need


def _req_u8_frames(who: str, frames: torch.Tensor):
    _req_cuda(who, "frames", frames)
    return tuple(_t(who, "frames", frames, torch.uint8, (None, None, 3), what="uint8 [images, pixels, 3]")[:2])


def _req_rgb8(who: str, name: str, frames: torch.Tensor):
    """(images, H, W) of contiguous uint8 RGB frames."""
    return tuple(_t(who, name, frames, torch.uint8, (None, None, None, 3), what="uint8 [images, H, W, 3]")[:3])


_CONTROL_DT = {torch.float16: CA_F16, torch.float32: _capi.CA_F32}


def _control_args(who: str, n: int, h: int, w: int, edges: Optional[torch.Tensor], control: Optional[torch.Tensor], rep: int, map_shape=None,
                  map_name: str = "edges") -> int:
    """The outputs of a finish entry (csrc/ca_annot.h): the uint8 map [n, H, W] (or map_shape) and the control tensor [rep * n, 3, H, W];
    returns control_dtype for the C call."""
    if edges is not None:
        _t(who, map_name, edges, torch.uint8, map_shape or (n, h, w))
    if control is None:
        return _capi.CA_F32
    if control.dtype not in _CONTROL_DT:
        raise TypeError(f"the control tensor must be float32 or float16, got {control.dtype}")
    _t(who, "control", control, None, (rep * n, 3, h, w))
    return _CONTROL_DT[control.dtype]


def _req_f64(who: str, names: str, *ts):
    _req_cuda(who, names, *ts)
    for name, t in zip(names.split(), ts):
        _t(who, name, t, torch.float64)


def hist_u8x3(frames: torch.Tensor, hist: torch.Tensor) -> torch.Tensor:
    """uint8 [images, pixels, 3] -> counts [images, 3, 256] into the caller's int32 `hist` (ca_hist_u8x3)."""
    images, pixels = _req_u8_frames("ca_hist_u8x3", frames)
    _req_cuda("ca_hist_u8x3", "hist", hist)
    _t("ca_hist_u8x3", "hist", hist, torch.int32, (images, 3, 256))
    check(lib().ca_hist_u8x3(_p(frames), _p(hist), images, pixels, _stream()), "ca_hist_u8x3")
    return hist


def color_moments_f64(frames: torch.Tensor, lut: torch.Tensor, mean: torch.Tensor, moments: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    """The six centred second moments per image of lut[image][c][byte] (ca_color_moments_f64) into `moments` [images, 6]."""
    images, pixels = _req_u8_frames("ca_color_moments_f64", frames)
    _req_f64("ca_color_moments_f64", "lut mean moments", lut, mean, moments)
    _req_cuda("ca_color_moments_f64", "ws", ws)
    for name, t, shape in (("lut", lut, (images, 3, 256)), ("mean", mean, (images, 3)), ("moments", moments, (images, 6))):
        _t("ca_color_moments_f64", name, t, None, shape)
    check(lib().ca_color_moments_f64(_p(frames), _p(lut), _p(mean), _p(moments), images, pixels, _p(ws), _ws_bytes(ws), _stream()),
          "ca_color_moments_f64")
    return moments


def color_transform_f64(frames: torch.Tensor, lut: torch.Tensor, mean: torch.Tensor, t: torch.Tensor, my: torch.Tensor,
                        y: torch.Tensor) -> torch.Tensor:
    """y[image, j, p] = (lut[image, :, byte] - mean[image]) @ t[image] + my into float64 planes [images, 3, pixels] (ca_color_transform_f64)."""
    images, pixels = _req_u8_frames("ca_color_transform_f64", frames)
    _req_f64("ca_color_transform_f64", "lut mean t my y", lut, mean, t, my, y)
    for name, v, shape in (("lut", lut, (images, 3, 256)), ("mean", mean, (images, 3)), ("t", t, (images, 3, 3)), ("y", y, (images, 3, pixels))):
        _t("ca_color_transform_f64", name, v, None, shape)
    _t("ca_color_transform_f64", "my", my, None, numel=3)
    check(lib().ca_color_transform_f64(_p(frames), _p(lut), _p(mean), _p(t), _p(my), _p(y), images, pixels, _stream()), "ca_color_transform_f64")
    return y


def sort_f64_segments(keys: torch.Tensor, out: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    """Sorts every run keys[..., :] (float64, last dimension) ascending into `out` (may be `keys`) (ca_sort_f64_segments)."""
    _req_f64("ca_sort_f64_segments", "keys out", keys, out)
    _req_cuda("ca_sort_f64_segments", "ws", ws)
    _need(keys.shape == out.shape and keys.dim() >= 1, "ca_sort_f64_segments", "out must have the shape of keys (at least 1-D)", out)
    n = keys.shape[-1]
    segments = keys.numel() // n
    check(lib().ca_sort_f64_segments(_p(keys), _p(out), segments, n, _p(ws), _ws_bytes(ws), _stream()), "ca_sort_f64_segments")
    return out


def color_rank_map_f64(y: torch.Tensor, srt: torch.Tensor, o: torch.Tensor, knots_q: torch.Tensor, knots_val: torch.Tensor,
                       knots_n: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    """o = interp(rank of y in its sorted plane / pixels; knots) (ca_color_rank_map_f64); `o` may be `y`.  Leaves the min / max
    partials of o in `ws` for color_finish_u8."""
    _req_f64("ca_color_rank_map_f64", "y srt o knots_q knots_val", y, srt, o, knots_q, knots_val)
    _req_cuda("ca_color_rank_map_f64", "knots_n ws", knots_n, ws)
    images, _, pixels = y.shape
    _need(y.shape[1] == 3 and srt.shape == y.shape and o.shape == y.shape, "ca_color_rank_map_f64", "y, srt and o must be [images, 3, pixels]", y)
    _t("ca_color_rank_map_f64", "knots_q", knots_q, None, (3, 256))
    _t("ca_color_rank_map_f64", "knots_val", knots_val, None, (3, 256))
    _t("ca_color_rank_map_f64", "knots_n", knots_n, torch.int32, numel=3, contiguous=False)
    check(lib().ca_color_rank_map_f64(_p(y), _p(srt), _p(o), _p(knots_q), _p(knots_val), _p(knots_n), images, pixels, _p(ws), _ws_bytes(ws), _stream()),
          "ca_color_rank_map_f64")
    return o


def color_finish_u8(o: torch.Tensor, out: torch.Tensor, normalize: bool, ws: torch.Tensor) -> torch.Tensor:
    """float64 planes [images, 3, pixels] -> uint8 [images, pixels, 3]: min-max stretch (normalize), x255, round half to even, clamp
    (ca_color_finish_u8; `ws` as color_rank_map_f64 left it)."""
    _req_f64("ca_color_finish_u8", "o", o)
    _req_cuda("ca_color_finish_u8", "out ws", out, ws)
    images, _, pixels = o.shape
    _t("ca_color_finish_u8", "out", out, torch.uint8, (images, pixels, 3))
    check(lib().ca_color_finish_u8(_p(o), _p(out), images, pixels, int(bool(normalize)), _p(ws), _ws_bytes(ws), _stream()),
          "ca_color_finish_u8")
    return out


# ---- ABI v16: the canny annotator (controlanimate_amd/annotators.py: CannyAnnotator) ---------------------------------------------

CANNY_TILE_H, CANNY_TILE_W = 16, 64  # kTH / kTW of csrc/ca_canny.hip (ca_canny_tile_h / ca_canny_tile_w; tests/test_canny_cpu.py compares)
CANNY_LINK_STAGES = ("label", "merge", "flatten")  # CA_CANNY_LINK_LABEL / _MERGE / _FLATTEN


def canny_workspace_bytes(images: int, h: int, w: int) -> int:
    """ca_canny_workspace_bytes: the scratch of classify / link / emit for `images` frames of h x w pixels."""
    need = lib().ca_canny_workspace_bytes(images, h, w)
    if need <= 0:
        raise _capi.CAHipError(f"ca_canny_workspace_bytes: images={images} h={h} w={w} out of range (images * h * w < 2^31)")
    return need


def _ws_bytes(ws: torch.Tensor) -> int:
    return ws.numel() * ws.element_size()


def canny_classify(frames: torch.Tensor, low: int, high: int, ws: torch.Tensor) -> None:
    """uint8 [images, H, W, C] (C = 1 or 3) -> class byte per pixel in `ws` (ca_canny_classify)."""
    _req_cuda("ca_canny_classify", "frames ws", frames, ws)
    n, h, w, c = _t("ca_canny_classify", "frames", frames, torch.uint8, _D4, what="uint8 [images, H, W, C]")
    check(lib().ca_canny_classify(_p(frames), n, h, w, c, int(low), int(high), _p(ws), _ws_bytes(ws), _stream()), "ca_canny_classify")


def canny_link(images: int, h: int, w: int, ws: torch.Tensor) -> None:
    """Hysteresis over the class bytes in `ws`: component labels and the strong flag per root (ca_canny_link, three launches)."""
    _req_cuda("ca_canny_link", "ws", ws)
    check(lib().ca_canny_link(images, h, w, _p(ws), _ws_bytes(ws), _stream()), "ca_canny_link")


def canny_link_stage(images: int, h: int, w: int, ws: torch.Tensor, stage: str) -> None:
    """One launch of canny_link, `stage` in CANNY_LINK_STAGES: the three in that order are canny_link (ca_canny_link_stage; for
    timing each launch on its own)."""
    _req_cuda("ca_canny_link_stage", "ws", ws)
    check(lib().ca_canny_link_stage(images, h, w, _p(ws), _ws_bytes(ws), CANNY_LINK_STAGES.index(stage), _stream()), "ca_canny_link_stage")


def canny_emit(images: int, h: int, w: int, ws: torch.Tensor, edges: Optional[torch.Tensor] = None, control: Optional[torch.Tensor] = None,
               rep: int = 1) -> None:
    """Writes the edge map (uint8 [images, H, W], 0 / 255) and / or the control tensor ([rep * images, 3, H, W], 0.0 / 1.0) from
    `ws` as canny_link left it (ca_canny_emit)."""
    _req_cuda("ca_canny_emit", "ws edges control", ws, edges, control)
    dt = _control_args("ca_canny_emit", images, h, w, edges, control, rep)
    check(lib().ca_canny_emit(images, h, w, _p(ws), _ws_bytes(ws), _p(edges), _p(control), int(rep), dt, _stream()), "ca_canny_emit")


# ---- added to ABI v16: the stages of the HED annotator around its convolutions (controlanimate_amd/hed.py: HedAnnotator) -----------

def hed_prep(frames: torch.Tensor, norm: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """uint8 RGB [images, H, W, 3] -> NHWC `out` [images, H, W, 8] fp16 / bf16: (float)frames - norm in channels 0..2, zeros in 3..7
    (ca_hed_prep).  norm: float32 [3] on the device."""
    _req_cuda("ca_hed_prep", "frames norm out", frames, norm, out)
    n, h, w = _req_rgb8("ca_hed_prep", "frames", frames)
    _t("ca_hed_prep", "norm", norm, torch.float32, numel=3)
    _t("ca_hed_prep", "out", out, None, (n, h, w, 8))
    check(lib().ca_hed_prep(_p(frames), _p(norm), _p(out), n, h, w, dt_code(out.dtype), _stream()), "ca_hed_prep")
    return out


def hed_pool_side(x: torch.Tensor, proj_w: torch.Tensor, proj_bias: torch.Tensor, side: torch.Tensor, pooled: Optional[torch.Tensor] = None) -> None:
    """One pass over a block's output x [images, h, w, C]: side [images, h, w] float32 = proj_bias + x . proj_w (fp32 accumulation)
    and, when `pooled` [images, h / 2, w / 2, C] is given, the 2x2 / stride-2 max pool (ca_hed_pool_side)."""
    _req_cuda("ca_hed_pool_side", "x proj_w proj_bias side pooled", x, proj_w, proj_bias, side, pooled)
    n, h, w, c = _t("ca_hed_pool_side", "x", x, None, _D4)
    _t("ca_hed_pool_side", "proj_w", proj_w, torch.float32, numel=c)
    _t("ca_hed_pool_side", "proj_bias", proj_bias, torch.float32, numel=1, contiguous=False)
    _t("ca_hed_pool_side", "side", side, torch.float32, (n, h, w))
    if pooled is not None:
        _t("ca_hed_pool_side", "pooled", pooled, x.dtype, (n, h // 2, w // 2, c))
    check(lib().ca_hed_pool_side(_p(x), _p(proj_w), _p(proj_bias), _p(side), _p(pooled), n, h, w, c, dt_code(x.dtype), _stream()), "ca_hed_pool_side")


_SIDE_MAP = tuple(f"sides: side map {k}" for k in range(5))


def hed_fuse(sides, edges: Optional[torch.Tensor] = None, control: Optional[torch.Tensor] = None, rep: int = 1) -> None:
    """The five float32 side maps [images, H >> k, W >> k] -> the uint8 edge map [images, H, W] and / or the control tensor
    [rep * images, 3, H, W] (float32 / float16, level / 255): bilinear resize, mean, sigmoid and quantisation in one launch (ca_hed_fuse)."""
    _need(len(sides) == 5, "ca_hed_fuse", "sides must be the five side maps")
    _req_cuda("ca_hed_fuse", "edges control sides", edges, control, *sides)
    n, h, w = sides[0].shape
    for k, s in enumerate(sides):
        _t("ca_hed_fuse", _SIDE_MAP[k], s, torch.float32, (n, h >> k, w >> k))
    dt = _control_args("ca_hed_fuse", n, h, w, edges, control, rep)
    check(lib().ca_hed_fuse(*[_p(s) for s in sides], n, h, w, _p(edges), _p(control), int(rep), dt, _stream()), "ca_hed_fuse")


# ---- added to ABI v16: the lineart annotator's stages beside conv3x3 / gemm (controlanimate_amd/lineart.py: LineartAnnotator) -----------

def lineart_conv_in(frames: torch.Tensor, w_packed: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """uint8 RGB [images, H, W, 3] -> `out` [images, H, W, 64] fp16 / bf16: the 7x7 convolution behind reflection padding 3 of
    frames / 255, without bias (ca_lineart_conv_in).  w_packed: [64, 160] of out's dtype (lineart.pack_conv_in)."""
    _req_cuda("ca_lineart_conv_in", "frames w_packed out", frames, w_packed, out)
    n, h, w = _req_rgb8("ca_lineart_conv_in", "frames", frames)
    _t("ca_lineart_conv_in", "w_packed", w_packed, out.dtype, (64, 160))
    _t("ca_lineart_conv_in", "out", out, None, (n, h, w, 64))
    check(lib().ca_lineart_conv_in(_p(frames), _p(w_packed), _p(out), n, h, w, dt_code(out.dtype), _stream()), "ca_lineart_conv_in")
    return out


def instance_norm(x: torch.Tensor, *, relu: bool = False, residual: Optional[torch.Tensor] = None, in_ring: bool = False, res_ring: bool = False,
                  out_pad: bool = False, eps: float = 1e-5, out: Optional[torch.Tensor] = None, partials: Optional[torch.Tensor] = None) -> torch.Tensor:
    """InstanceNorm2d(affine=False) of NHWC x per (image, channel), then optional ReLU, then optional residual add (ca_instnorm_stats +
    ca_instnorm_apply).  in_ring / res_ring: that operand is stored as [images, H + 2, W + 2, C] and its outermost pixels are ignored.
    out_pad: the result is written as [images, H + 2, W + 2, C], padded by reflection of one pixel.  C is 64, 128 or 256."""
    who = "ca_instnorm"
    _req_cuda(who, "x residual out partials", x, residual, out, partials)
    n, hs, ws, c = _t(who, "x", x, None, _D4)
    h, w = (hs - 2, ws - 2) if in_ring else (hs, ws)
    if residual is not None:
        _t(who, "residual", residual, x.dtype, (n, h + 2, w + 2, c) if res_ring else (n, h, w, c))
    out = _out(who, "out", out, (n, h + 2, w + 2, c) if out_pad else (n, h, w, c), x.dtype, x.device)
    _need(out.data_ptr() != x.data_ptr(), who, "out must not be x")
    floats = int(lib().ca_instnorm_partials_floats(n, h, w, c))
    if floats <= 0:
        raise _capi.CAHipError(f"ca_instnorm: images={n} h={h} w={w} c={c} is out of range (c is 64, 128 or 256)")
    if partials is None:
        partials = torch.empty(floats, dtype=torch.float32, device=x.device)
    _t(who, "partials", partials, torch.float32)
    _need(partials.numel() >= floats, who, "partials holds fewer floats than ca_instnorm_partials_floats asks for", partials)
    dt = dt_code(x.dtype)
    check(lib().ca_instnorm_stats(_p(x), _p(partials), n, h, w, c, int(in_ring), dt, _stream()), "ca_instnorm_stats")
    check(lib().ca_instnorm_apply(_p(x), _p(partials), _p(residual), _p(out), n, h, w, c, int(in_ring), int(res_ring), int(out_pad), int(relu),
                                  float(eps), dt, _stream()), "ca_instnorm_apply")
    return out


def conv_transpose3x3s2(x: torch.Tensor, w_taps: torch.Tensor, *, taps: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ConvTranspose2d(Cin, Cout, 3, stride=2, padding=1, output_padding=1) without bias: x [images, H, W, Cin] -> [images, 2H, 2W, Cout].
    One gemm with N = 9 * Cout (w_taps [3, 3, Cout, Cin]: lineart.pack_convt_phases) into `taps`, then ca_convt3x3s2_gather."""
    _req_cuda("ca_convt3x3s2_gather", "x w_taps taps out", x, w_taps, taps, out)
    n, h, w, cin = _t("ca_convt3x3s2_gather", "x", x, None, _D4)
    cout = _t("ca_convt3x3s2_gather", "w_taps", w_taps, x.dtype, _D4)[2]
    _t("ca_convt3x3s2_gather", "w_taps", w_taps, None, (3, 3, cout, cin))
    if taps is not None:
        _t("ca_convt3x3s2_gather", "taps", taps, x.dtype, (n * h * w, 9 * cout))
    out = _out("ca_convt3x3s2_gather", "out", out, (n, 2 * h, 2 * w, cout), x.dtype, x.device)
    if taps is None:
        taps = torch.empty((n * h * w, 9 * cout), dtype=x.dtype, device=x.device)
    gemm(x.view(n * h * w, cin), w_taps.view(9 * cout, cin), out=taps)
    check(lib().ca_convt3x3s2_gather(_p(taps), _p(out), n, h, w, cout, dt_code(x.dtype), _stream()), "ca_convt3x3s2_gather")
    return out


def lineart_conv_out(x: torch.Tensor, wt: torch.Tensor, bias: torch.Tensor, logits: torch.Tensor) -> torch.Tensor:
    """x [images, H, W, 64] -> `logits` float32 [images, H, W]: the 7x7 convolution to one channel behind reflection padding 3
    (ca_lineart_conv_out).  wt: float32 [7, 7, 64]; bias: float32 [1]."""
    _req_cuda("ca_lineart_conv_out", "x wt bias logits", x, wt, bias, logits)
    n, h, w, _ = _t("ca_lineart_conv_out", "x", x, None, (None, None, None, 64))
    _t("ca_lineart_conv_out", "wt", wt, torch.float32, (7, 7, 64))
    _t("ca_lineart_conv_out", "bias", bias, torch.float32, numel=1, contiguous=False)
    _t("ca_lineart_conv_out", "logits", logits, torch.float32, (n, h, w))
    check(lib().ca_lineart_conv_out(_p(x), _p(wt), _p(bias), _p(logits), n, h, w, dt_code(x.dtype), _stream()), "ca_lineart_conv_out")
    return logits


def lineart_finish(logits: torch.Tensor, edges: Optional[torch.Tensor] = None, control: Optional[torch.Tensor] = None, rep: int = 1) -> None:
    """float32 logits [images, H, W] -> the uint8 map 255 - trunc(sigmoid * 255) [images, H, W] and / or the control tensor
    [rep * images, 3, H, W] (float32 / float16, map / 255) in one launch (ca_lineart_finish)."""
    _req_cuda("ca_lineart_finish", "logits edges control", logits, edges, control)
    n, h, w = _t("ca_lineart_finish", "logits", logits, torch.float32, _D3)
    dt = _control_args("ca_lineart_finish", n, h, w, edges, control, rep)
    check(lib().ca_lineart_finish(_p(logits), n, h, w, _p(edges), _p(control), int(rep), dt, _stream()), "ca_lineart_finish")


# ---- added to ABI v16: the lineart_anime annotator's U-Net layers (controlanimate_amd/lineart_anime.py: LineartAnimeAnnotator) -------------
IN_ACT_NONE, IN_ACT_RELU, IN_ACT_LEAKY = 0, 1, 2  # the activations of instance_norm_act's outputs


def lanime_conv_in(frames: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, l0: torch.Tensor, c0: torch.Tensor) -> None:
    """uint8 RGB [images, H, W, 3] -> d0 = Conv2d(3, 64, 4, 2, 1)(frames / 127.5 - 1) + bias, written as l0 [images, H/2, W/2, 64] =
    LeakyReLU(0.2)(d0) and c0[..., :64] = ReLU(d0), c0 [images, H/2, W/2, 128] (ca_lanime_conv_in).  w_packed: [64, 64] of l0's dtype
    (lineart_anime.pack_conv_in); bias: float32 [64]."""
    _req_cuda("ca_lanime_conv_in", "frames w_packed bias l0 c0", frames, w_packed, bias, l0, c0)
    n, h, w = _req_rgb8("ca_lanime_conv_in", "frames", frames)
    _t("ca_lanime_conv_in", "w_packed", w_packed, l0.dtype, (64, 64))
    _t("ca_lanime_conv_in", "bias", bias, torch.float32, numel=64)
    _t("ca_lanime_conv_in", "l0", l0, None, (n, h // 2, w // 2, 64))
    _t("ca_lanime_conv_in", "c0", c0, l0.dtype, (n, h // 2, w // 2, 128))
    check(lib().ca_lanime_conv_in(_p(frames), _p(w_packed), _p(bias), _p(l0), _p(c0), n, h, w, dt_code(l0.dtype), _stream()), "ca_lanime_conv_in")


# Below this many output rows conv4x4s2 runs as a gather + gemm: the level is bound by its weights.  A design choice, not the measured
# crossover: it keeps the levels that hold the work (1 .. 4 of a 16-frame window of 512 x 768) free of an im2col tensor, although the
# gather form measured faster up to 24576 rows (profiles/lineart_anime_bench.json: stages.conv.forms).
CONV4X4S2_GEMM_ROWS = 4096


def conv4x4s2(x: torch.Tensor, w: torch.Tensor, *, bias: Optional[torch.Tensor] = None, relu: bool = False, out: Optional[torch.Tensor] = None,
              form: Optional[str] = None, cols: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Conv2d(Cin, Cout, 4, stride=2, padding=1): x [images, H, W, Cin] -> [images, H/2, W/2, Cout]; w [Cout, 4, 4, Cin]; optional
    float32 bias and ReLU in the epilogue.  form "tile": ca_conv4x4s2, the implicit GEMM from an LDS halo tile, without an im2col tensor;
    form "gemm": ca_im2col4x4s2 into `cols` [rows, 16 Cin] + gemm (split-K), for the levels whose few output rows leave the tile kernel's grid
    small while 8 MB of weights stream; None: "gemm" below CONV4X4S2_GEMM_ROWS output rows."""
    who = "ca_conv4x4s2"
    _req_cuda(who, "x w bias out cols", x, w, bias, out, cols)
    n, h, wd, cin = _t(who, "x", x, None, _D4)
    cout = _t(who, "w", w, x.dtype, (None, 4, 4, cin))[0]
    _need(form in (None, "tile", "gemm"), who, 'form must be None, "tile" or "gemm"')
    if bias is not None:
        _t(who, "bias", bias, torch.float32, numel=cout)
    out = _out(who, "out", out, (n, h // 2, wd // 2, cout), x.dtype, x.device)
    rows = n * (h // 2) * (wd // 2)
    if form is None:
        form = "gemm" if rows < CONV4X4S2_GEMM_ROWS else "tile"
    if form == "tile":
        check(lib().ca_conv4x4s2(_p(x), _p(w), _p(bias), _p(out), n, h, wd, cin, cout, int(relu), dt_code(x.dtype), _stream()), "ca_conv4x4s2")
        return out
    if cols is None:
        cols = torch.empty((rows, 16 * cin), dtype=x.dtype, device=x.device)
    else:
        _t(who, "cols", cols, x.dtype)
        _need(cols.numel() >= rows * 16 * cin, who, "cols holds fewer than rows * 16 * Cin elements", cols)
        cols = cols.view(-1)[: rows * 16 * cin].view(rows, 16 * cin)
    check(lib().ca_im2col4x4s2(_p(x), _p(cols), n, h, wd, cin, dt_code(x.dtype), _stream()), "ca_im2col4x4s2")
    gemm(cols, w.view(cout, 16 * cin), bias=bias, act=ACT_RELU if relu else ACT_NONE, out=out.view(rows, cout))
    return out


def conv_transpose4x4s2(x: torch.Tensor, w_phase: torch.Tensor, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ConvTranspose2d(Cin, Cout, 4, stride=2, padding=1) without bias: x [images, H, W, Cin] -> [images, 2H, 2W, Cout] as four 2x2
    phase convolutions in one launch (ca_convt4x4s2).  w_phase [4, Cout, 2, 2, Cin]: lineart_anime.pack_convt4x4_phases."""
    _req_cuda("ca_convt4x4s2", "x w_phase out", x, w_phase, out)
    n, h, w, cin = _t("ca_convt4x4s2", "x", x, None, _D4)
    cout = _t("ca_convt4x4s2", "w_phase", w_phase, x.dtype, (4, None, 2, 2, cin))[1]
    out = _out("ca_convt4x4s2", "out", out, (n, 2 * h, 2 * w, cout), x.dtype, x.device)
    check(lib().ca_convt4x4s2(_p(x), _p(w_phase), _p(out), n, h, w, cin, cout, dt_code(x.dtype), _stream()), "ca_convt4x4s2")
    return out


def instance_norm_act(x: torch.Tensor, outs, *, eps: float = 1e-5, partials: Optional[torch.Tensor] = None) -> None:
    """InstanceNorm2d(affine=False) of NHWC x [images, H, W, C] (C 64 .. 512) into one or two destinations (ca_instnorm_act).
    outs: [(tensor [images, H, W, stride], act, channel offset)]; act is IN_ACT_NONE / IN_ACT_RELU / IN_ACT_LEAKY (0.2).  Only channels
    offset .. offset + C of a destination are written."""
    who = "ca_instnorm_act"
    _req_cuda(who, "x partials outs", x, partials, *[o[0] for o in outs])
    n, h, w, c = _t(who, "x", x, None, _D4)
    _need(1 <= len(outs) <= 2, who, "outs must hold one or two destinations")
    args = []
    for t, act, off in outs:
        _t(who, "outs", t, x.dtype, (n, h, w, None))
        _need(t.data_ptr() != x.data_ptr(), who, "outs: a destination must not be x")
        args += [_p(t), int(act), int(off), int(t.shape[3])]
    if len(outs) == 1:
        args += [None, 0, 0, 0]
    floats = int(lib().ca_instnorm_act_partials_floats(n, h, w, c))
    if floats <= 0:
        raise _capi.CAHipError(f"ca_instnorm_act: images={n} h={h} w={w} c={c} is out of range (c is 64, 128, 256 or 512)")
    if partials is None:
        partials = torch.empty(floats, dtype=torch.float32, device=x.device)
    _t(who, "partials", partials, torch.float32)
    _need(partials.numel() >= floats, who, "partials holds fewer floats than ca_instnorm_act_partials_floats asks for", partials)
    check(lib().ca_instnorm_act(_p(x), _p(partials), *args, n, h, w, c, float(eps), dt_code(x.dtype), _stream()), "ca_instnorm_act")


def lanime_conv_out(x: torch.Tensor, wt: torch.Tensor, bias: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """x [images, H, W, 128] -> `out` float32 [images, 2H, 2W]: ConvTranspose2d(128, 1, 4, 2, 1) + bias (ca_lanime_conv_out).
    wt: float32 [4, 4, 128]; bias: float32 [1]."""
    _req_cuda("ca_lanime_conv_out", "x wt bias out", x, wt, bias, out)
    n, h, w, _ = _t("ca_lanime_conv_out", "x", x, None, (None, None, None, 128))
    _t("ca_lanime_conv_out", "wt", wt, torch.float32, (4, 4, 128))
    _t("ca_lanime_conv_out", "bias", bias, torch.float32, numel=1, contiguous=False)
    _t("ca_lanime_conv_out", "out", out, torch.float32, (n, 2 * h, 2 * w))
    check(lib().ca_lanime_conv_out(_p(x), _p(wt), _p(bias), _p(out), n, h, w, dt_code(x.dtype), _stream()), "ca_lanime_conv_out")
    return out


def lanime_finish(pre: torch.Tensor, edges: Optional[torch.Tensor] = None, control: Optional[torch.Tensor] = None, rep: int = 1) -> None:
    """float32 pre-tanh values [images, H, W] -> the uint8 map 255 - trunc(clip(tanh * 127.5 + 127.5)) [images, H, W] and / or the
    control tensor [rep * images, 3, H, W] (float32 / float16, map / 255) in one launch (ca_lanime_finish)."""
    _req_cuda("ca_lanime_finish", "pre edges control", pre, edges, control)
    n, h, w = _t("ca_lanime_finish", "pre", pre, torch.float32, _D3)
    dt = _control_args("ca_lanime_finish", n, h, w, edges, control, rep)
    check(lib().ca_lanime_finish(_p(pre), n, h, w, _p(edges), _p(control), int(rep), dt, _stream()), "ca_lanime_finish")


# ---- added to ABI v16: the M-LSD annotator's stages beside conv3x3 / gemm / add_bcast (controlanimate_amd/mlsd.py: MlsdAnnotator) -----------
MLSD_TOPK = _capi.CA_MLSD_TOPK


def mlsd_prep(frames: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """uint8 RGB [images, H, W, 3] -> NHWC `out` [images, H, W, 8] fp16 / bf16: frames / 127.5 - 1 in channels 0..2, 1 / 127.5 - 1 in
    channel 3 (the detector's channel of ones), zeros in 4..7 (ca_mlsd_prep)."""
    _req_cuda("ca_mlsd_prep", "frames out", frames, out)
    n, h, w = _req_rgb8("ca_mlsd_prep", "frames", frames)
    _t("ca_mlsd_prep", "out", out, None, (n, h, w, 8))
    check(lib().ca_mlsd_prep(_p(frames), _p(out), n, h, w, dt_code(out.dtype), _stream()), "ca_mlsd_prep")
    return out


def dwconv3x3(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, *, stride: int = 1, relu6: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Depthwise 3x3 convolution of NHWC x [images, H, W, C] (ca_dwconv3x3).  w: [9, C] of x's dtype (tap ky * 3 + kx of every channel:
    mlsd.pack_depthwise), bias float32 [C].  stride 1: padding 1; stride 2: F.pad(x, (0, 1, 0, 1)) and padding 0, even H and W."""
    _req_cuda("ca_dwconv3x3", "x w bias out", x, w, bias, out)
    n, h, ww, c = _t("ca_dwconv3x3", "x", x, None, _D4)
    _t("ca_dwconv3x3", "w", w, x.dtype, (9, c))
    _t("ca_dwconv3x3", "bias", bias, torch.float32, numel=c)
    if stride in (1, 2):  # (another stride goes through: the library's message names the ones it takes)
        out = _out("ca_dwconv3x3", "out", out, (n, h // stride, ww // stride, c), x.dtype, x.device)
        _need(out.data_ptr() != x.data_ptr(), "ca_dwconv3x3", "out must not be x")
    check(lib().ca_dwconv3x3(_p(x), _p(w), _p(bias), _p(out), n, h, ww, c, int(stride), int(relu6), dt_code(x.dtype), _stream()), "ca_dwconv3x3")
    return out


def upsample2x_bilinear_ac(x: torch.Tensor, out: torch.Tensor, col0: int = 0) -> torch.Tensor:
    """F.interpolate(scale_factor=2, mode="bilinear", align_corners=True) of NHWC x [images, h, w, C] into channels col0 .. col0 + C - 1 of
    `out` [images, 2h, 2w, ld]; the other channels of `out` are left as they are (ca_upsample2x_bilinear_ac)."""
    _req_cuda("ca_upsample2x_bilinear_ac", "x out", x, out)
    n, h, w, c = _t("ca_upsample2x_bilinear_ac", "x", x, None, _D4)
    _t("ca_upsample2x_bilinear_ac", "out", out, x.dtype, (n, 2 * h, 2 * w, None))
    check(lib().ca_upsample2x_bilinear_ac(_p(x), _p(out), n, h, w, c, out.shape[3], int(col0), dt_code(x.dtype), _stream()), "ca_upsample2x_bilinear_ac")
    return out


def conv3x3_dil(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, *, dilation: int = 5, relu: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Conv2d(64, 64, 3, dilation=5, padding=5) + bias (+ ReLU) of NHWC x [images, H, W, 64] on the MFMA (ca_conv3x3_dil).
    w: [64, 3, 3, 64] of x's dtype (the layout conv3x3 takes), bias float32 [64]."""
    _req_cuda("ca_conv3x3_dil", "x w bias out", x, w, bias, out)
    n, h, ww, c = _t("ca_conv3x3_dil", "x", x, None, _D4)
    _t("ca_conv3x3_dil", "w", w, x.dtype, (c, 3, 3, c))
    _t("ca_conv3x3_dil", "bias", bias, torch.float32, numel=c)
    out = _out("ca_conv3x3_dil", "out", out, (n, h, ww, c), x.dtype, x.device)
    check(lib().ca_conv3x3_dil(_p(x), _p(w), _p(bias), _p(out), n, h, ww, c, int(dilation), int(relu), dt_code(x.dtype), _stream()), "ca_conv3x3_dil")
    return out


def mlsd_decode_workspace_bytes(images: int, h: int, w: int) -> int:
    n = int(lib().ca_mlsd_decode_workspace_bytes(images, h, w))
    if n <= 0:
        raise _capi.CAHipError(f"ca_mlsd_decode_workspace_bytes: images={images} h={h} w={w} is out of range")
    return n


def mlsd_decode(tp: torch.Tensor, thr_v: float = 0.1, thr_d: float = 0.1, *, segments: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None,
                ws: Optional[torch.Tensor] = None):
    """tp float32 [images, h, w, 8] (channel 0 the centre logit, 1..4 the displacements) -> (segments int32 [images, 200, 4] at full
    resolution in rank order, count int32 [images]): sigmoid, plateau-keeping 3x3 maximum test, exact top 200, distance test, float64
    endpoints in one launch, no host read (ca_mlsd_decode)."""
    _req_cuda("ca_mlsd_decode", "tp segments count ws", tp, segments, count, ws)
    n, h, w, _ = _t("ca_mlsd_decode", "tp", tp, torch.float32, (None, None, None, 8))
    if count is not None:
        _t("ca_mlsd_decode", "count", count, torch.int32, (n,))
    segments = _out("ca_mlsd_decode", "segments", segments, (n, MLSD_TOPK, 4), torch.int32, tp.device)
    if count is None:
        count = torch.empty((n,), dtype=torch.int32, device=tp.device)
    if ws is None:
        ws = torch.empty(mlsd_decode_workspace_bytes(n, h, w), dtype=torch.uint8, device=tp.device)
    check(lib().ca_mlsd_decode(_p(tp), n, h, w, float(thr_v), float(thr_d), _p(ws), _ws_bytes(ws), _p(segments), _p(count), _stream()), "ca_mlsd_decode")
    return segments, count


def mlsd_draw(segments: torch.Tensor, count: torch.Tensor, h: int, w: int, edges: Optional[torch.Tensor] = None, control: Optional[torch.Tensor] = None,
              rep: int = 1) -> torch.Tensor:
    """cv2.line(map, (xs, ys), (xe, ye), 255, 1) of the first count[i] segments of every image on a zeroed uint8 map [images, h, w]
    (`edges`, allocated when None, returned) and, when given, the control tensor [rep * images, 3, h, w] (float32 / float16) = map / 255
    (ca_mlsd_draw)."""
    _req_cuda("ca_mlsd_draw", "segments count edges control", segments, count, edges, control)
    n = segments.shape[0]
    _t("ca_mlsd_draw", "segments", segments, torch.int32, (n, MLSD_TOPK, 4))
    _t("ca_mlsd_draw", "count", count, torch.int32, (n,))
    if edges is None:
        edges = torch.empty((n, h, w), dtype=torch.uint8, device=segments.device)
    dt = _control_args("ca_mlsd_draw", n, h, w, edges, control, rep)
    check(lib().ca_mlsd_draw(_p(segments), _p(count), n, h, w, _p(edges), _p(control), int(rep), dt, _stream()), "ca_mlsd_draw")
    return edges


# ---- added to ABI v16: the softedge (PiDiNet) annotator's stages beside conv3x3 / gemm (controlanimate_amd/softedge.py: SoftedgeAnnotator) -----------

def softedge_prep(frames: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """uint8 RGB [images, H, W, 3] -> NHWC `out` [images, H, W, 8] fp16 / bf16: frames / 255 in channels 0..2, zeros in 3..7
    (ca_softedge_prep)."""
    _req_cuda("ca_softedge_prep", "frames out", frames, out)
    n, h, w = _req_rgb8("ca_softedge_prep", "frames", frames)
    _t("ca_softedge_prep", "out", out, None, (n, h, w, 8))
    check(lib().ca_softedge_prep(_p(frames), _p(out), n, h, w, dt_code(out.dtype), _stream()), "ca_softedge_prep")
    return out


def relu(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """max(x, 0) of a contiguous fp16 / bf16 tensor whose element count is a multiple of 8 (ca_relu); `out` may be x."""
    _req_cuda("ca_relu", "x out", x, out)
    _t("ca_relu", "x", x)
    if out is None:
        out = torch.empty_like(x)
    _t("ca_relu", "out", out, x.dtype, numel=x.numel())
    check(lib().ca_relu(_p(x), _p(out), x.numel(), dt_code(x.dtype), _stream()), "ca_relu")
    return out


def _ksize_of(who: str, name: str, w: torch.Tensor, c: int) -> int:
    if not (w.dim() == 2 and w.shape[1] == c and w.shape[0] in (9, 25) and w.is_contiguous()):
        _need(False, who, f"{name} must be the depthwise taps [9 or 25, {c}], got {tuple(w.shape)}", w)
    return 3 if w.shape[0] == 9 else 5


def dwconv_k(x: torch.Tensor, w: torch.Tensor, *, relu: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Depthwise 3x3 (padding 1) or 5x5 (padding 2) convolution of NHWC x [images, H, W, C], stride 1, no bias, optional ReLU
    (ca_dwconv_k).  w: [9, C] or [25, C] of x's dtype (tap ky * ksize + kx of every channel: softedge.pack_depthwise)."""
    _req_cuda("ca_dwconv_k", "x w out", x, w, out)
    n, h, ww, c = _t("ca_dwconv_k", "x", x, None, _D4)
    _t("ca_dwconv_k", "w", w, x.dtype, contiguous=False)
    ks = _ksize_of("ca_dwconv_k", "w", w, c)
    out = _out("ca_dwconv_k", "out", out, (n, h, ww, c), x.dtype, x.device)
    check(lib().ca_dwconv_k(_p(x), _p(w), _p(out), n, h, ww, c, ks, int(relu), dt_code(x.dtype), _stream()), "ca_dwconv_k")
    return out


def maxpool2x2(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """MaxPool2d(2, 2) of NHWC x [images, H, W, C], H and W even (ca_maxpool2x2)."""
    _req_cuda("ca_maxpool2x2", "x out", x, out)
    n, h, w, c = _t("ca_maxpool2x2", "x", x, None, _D4)
    if out is None:
        out = torch.empty((n, h // 2, w // 2, c), dtype=x.dtype, device=x.device)
    _t("ca_maxpool2x2", "out", out, x.dtype, None if h % 2 or w % 2 else (n, h // 2, w // 2, c))  # (odd sizes go through: the library's message says "even")
    check(lib().ca_maxpool2x2(_p(x), _p(out), n, h, w, c, dt_code(x.dtype), _stream()), "ca_maxpool2x2")
    return out


def pdc_block_supported(c: int, ksize: int) -> bool:
    """Does ca_pdc_block take this width and kernel size (no launch, no device access)?"""
    return bool(lib().ca_pdc_block_supported(int(c), int(ksize)))


def pdc_block(x: torch.Tensor, w_dw: torch.Tensor, w2: torch.Tensor, *, out: Optional[torch.Tensor] = None, fused: Optional[bool] = None,
              tmp: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x + W2 . relu(dw(x)) of NHWC x [images, H, W, C]: one stride-1 block of PiDiNet.  w_dw: [9 or 25, C]; w2: [C, C] ([cout, cin]).
    fused (default: context.dispatch.pdc_block_fused where the library takes the width): ONE launch (ca_pdc_block); otherwise
    dwconv_k(relu) into `tmp` and gemm(residual = x)."""
    _req_cuda("ca_pdc_block", "x w_dw w2 out tmp", x, w_dw, w2, out, tmp)
    n, h, w, c = _t("ca_pdc_block", "x", x, None, _D4)
    _t("ca_pdc_block", "w_dw", w_dw, x.dtype, contiguous=False)
    ks = _ksize_of("ca_pdc_block", "w_dw", w_dw, c)
    _t("ca_pdc_block", "w2", w2, x.dtype, (c, c))
    out = _out("ca_pdc_block", "out", out, (n, h, w, c), x.dtype, x.device)
    if fused is None:
        fused = dispatch.pdc_block_fused and pdc_block_supported(c, ks)
    if fused:
        check(lib().ca_pdc_block(_p(x), _p(w_dw), _p(w2), _p(out), n, h, w, c, ks, dt_code(x.dtype), _stream()), "ca_pdc_block")
        return out
    d = dwconv_k(x, w_dw, relu=True, out=tmp)
    m = n * h * w
    gemm(d.view(m, c), w2, residual=x.view(m, c), out=out.view(m, c))
    return out


def cdcm_dil4(x: torch.Tensor, w: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The four dilated 3x3 convolutions (5, 7, 9, 11) of a CDCM, summed: NHWC x [images, H, W, 32] -> [images, H, W, 32] in one launch
    (ca_cdcm_dil4).  w: [4, 32, 3, 3, 32] of x's dtype ([dilation index, cout, ky, kx, cin])."""
    _req_cuda("ca_cdcm_dil4", "x w out", x, w, out)
    n, h, ww, c = _t("ca_cdcm_dil4", "x", x, None, _D4)
    _t("ca_cdcm_dil4", "w", w, x.dtype, (4, c, 3, 3, c))
    out = _out("ca_cdcm_dil4", "out", out, (n, h, ww, c), x.dtype, x.device)
    check(lib().ca_cdcm_dil4(_p(x), _p(w), _p(out), n, h, ww, c, dt_code(x.dtype), _stream()), "ca_cdcm_dil4")
    return out


def csam_reduce(f: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, wr: torch.Tensor, br: torch.Tensor, *,
                side: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """f [images, H, W, 32] -> side float32 [images, H, W] = br + sigmoid(conv3x3(b1 + W1 relu(f))) * (wr . f) (ca_csam_reduce).
    Float32 operands: w1 [4, 32], b1 [4], w2 [3, 3, 4], wr [32], br [1]; scratch: float32, 5 * images * H * W elements."""
    _req_cuda("ca_csam_reduce", "f w1 b1 w2 wr br side scratch", f, w1, b1, w2, wr, br, side, scratch)
    n, h, w, c = _t("ca_csam_reduce", "f", f, None, _D4)
    for name, t, shape in (("w1", w1, (4, c)), ("b1", b1, (4,)), ("w2", w2, (3, 3, 4)), ("wr", wr, (c,)), ("br", br, (1,))):
        _t("ca_csam_reduce", name, t, torch.float32, shape)
    px = n * h * w
    if scratch is not None:
        _t("ca_csam_reduce", "scratch", scratch, torch.float32)
        _need(scratch.numel() >= 5 * px, "ca_csam_reduce", "scratch holds fewer than 5 * images * H * W floats", scratch)
    side = _out("ca_csam_reduce", "side", side, (n, h, w), torch.float32, f.device)
    if scratch is None:
        scratch = torch.empty(5 * px, dtype=torch.float32, device=f.device)
    check(lib().ca_csam_reduce(_p(f), _p(w1), _p(b1), _p(w2), _p(wr), _p(br), _p(scratch), scratch.data_ptr() + 16 * px, _p(side), n, h, w, c,
                               dt_code(f.dtype), _stream()), "ca_csam_reduce")
    return side


def softedge_fuse(sides, classifier: torch.Tensor, *, safe: bool = False, logit: Optional[torch.Tensor] = None, edges: Optional[torch.Tensor] = None,
                  control: Optional[torch.Tensor] = None, rep: int = 1) -> None:
    """The four float32 side maps [images, H >> k, W >> k] and the classifier (float32 [5]: four weights, the bias) -> any of the float32
    fused logit [images, H, W], the uint8 map [images, H, W] and the control tensor [rep * images, 3, H, W] (float32 / float16, level / 255):
    bilinear resize (align_corners = False), classifier, sigmoid, the optional safe step and quantisation in one launch (ca_softedge_fuse)."""
    _need(len(sides) == 4, "ca_softedge_fuse", "sides must be the four side maps")
    _req_cuda("ca_softedge_fuse", "classifier logit edges control sides", classifier, logit, edges, control, *sides)
    n, h, w = sides[0].shape
    for k, s in enumerate(sides):
        _t("ca_softedge_fuse", _SIDE_MAP[k], s, torch.float32, (n, h >> k, w >> k))
    _t("ca_softedge_fuse", "classifier", classifier, torch.float32, numel=5)
    if logit is not None:
        _t("ca_softedge_fuse", "logit", logit, torch.float32, (n, h, w))
    dt = _control_args("ca_softedge_fuse", n, h, w, edges, control, rep)
    check(lib().ca_softedge_fuse(*[_p(s) for s in sides], _p(classifier), n, h, w, int(safe), _p(logit), _p(edges), _p(control), int(rep), dt, _stream()),
          "ca_softedge_fuse")


# ---- added to ABI v16: the GFPGAN face restorer's stages beside conv3x3 / gemm (controlanimate_amd/gfpgan.py: FaceRestorer) ------------------
ACT_LEAKY02 = _capi.CA_ACT_LEAKY02  # LeakyReLU(0.2) in the epilogue of conv3x3 / gemm
GFP_STYLE_FEAT = 512


def gfp_prep(faces: torch.Tensor, wt: torch.Tensor, bias: torch.Tensor, out: torch.Tensor, reverse_channels: bool = True) -> torch.Tensor:
    """uint8 [images, H, W, 3] -> `out` [images, H, W, Cout] = LeakyReLU(0.2)(conv1x1((faces / 255 - 0.5) / 0.5)), the channels read in
    reverse order with reverse_channels (ca_gfp_prep).  wt: float32 [Cout, 3]; bias: float32 [Cout]."""
    _req_cuda("ca_gfp_prep", "faces wt bias out", faces, wt, bias, out)
    n, h, w = _req_rgb8("ca_gfp_prep", "faces", faces)
    cout = out.shape[3]
    _t("ca_gfp_prep", "out", out, None, (n, h, w, cout))
    _t("ca_gfp_prep", "wt", wt, torch.float32, (cout, 3))
    _t("ca_gfp_prep", "bias", bias, torch.float32, numel=cout)
    check(lib().ca_gfp_prep(_p(faces), _p(wt), _p(bias), _p(out), n, h, w, cout, int(bool(reverse_channels)), dt_code(out.dtype), _stream()), "ca_gfp_prep")
    return out


def resample2x(x: torch.Tensor, up: bool, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The bilinear resize (align_corners = False) of NHWC x by 2 (up) or by 1/2 (H and W even: the 2x2 mean), fp32 arithmetic in torch's
    order and one rounding (ca_resample2x)."""
    _req_cuda("ca_resample2x", "x out", x, out)
    n, h, w, c = _t("ca_resample2x", "x", x, None, _D4)
    out = _out("ca_resample2x", "out", out, (n, 2 * h, 2 * w, c) if up else (n, h // 2, w // 2, c), x.dtype, x.device)
    check(lib().ca_resample2x(_p(x), _p(out), n, h, w, c, int(bool(up)), dt_code(x.dtype), _stream()), "ca_resample2x")
    return out


def gfp_styles(latents: torch.Tensor, params: torch.Tensor, desc, out: torch.Tensor) -> torch.Tensor:
    """Every modulated layer's per-image scales in one launch (ca_gfp_styles).  latents: float32 [images, num_latent, 512]; params: flat
    float32 (per layer the transposed modulation weight [512, cin] + bias [cin]; per StyleConv Wsq^T [cin, cout]); desc: six integers per
    layer (latent index, cin, cout -- 0 for a ToRGB --, w_off, wsq_off, out_off); out: float32 [images, out_stride], per layer
    s / max|s| [cin] then demod' [cout] at out_off (a ToRGB: s [cin])."""
    _req_cuda("ca_gfp_styles", "latents params out", latents, params, out)
    n, num_latent, _ = _t("ca_gfp_styles", "latents", latents, torch.float32, (None, None, GFP_STYLE_FEAT))
    _t("ca_gfp_styles", "params", params, torch.float32, (None,))
    _t("ca_gfp_styles", "out", out, torch.float32, (n, None))
    desc = [int(v) for v in desc]
    _need(len(desc) % 6 == 0 and desc, "ca_gfp_styles", "desc must hold six integers per layer, for at least one layer")
    arr = (C.c_int32 * len(desc))(*desc)
    check(lib().ca_gfp_styles(_p(latents), _p(params), params.numel(), arr, len(desc) // 6, _p(out), out.shape[1], n, num_latent, _stream()), "ca_gfp_styles")
    return out


# From this many output pixels per image upward a StyleConv runs on the one-launch kernel, below it as three launches around ca_conv3x3
# (measured per level, 16 faces: profiles/gfpgan_bench.json: style_convs).
MODCONV_FUSED_MIN_PIXELS = 512 * 512


def modconv3x3(x: torch.Tensor, wt: torch.Tensor, s: torch.Tensor, demod: torch.Tensor, noise: torch.Tensor, bias: torch.Tensor, noise_weight: float, *,
               upsample: bool = False, sft=None, images: Optional[int] = None, out: Optional[torch.Tensor] = None, form: Optional[str] = None,
               scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One StyleConv: LeakyReLU(0.2)(conv3x3(wt, s[n] * X) * demod[n] * sqrt(2) + noise_weight * noise + bias), X = x or its bilinear x2, then
    with sft = (scale, shift) [images, H, W, Cout / 2] the second half of the channels * scale + shift.
    x [images, h, w, Cin], or [1, h, w, Cin] shared by `images` images; wt [Cout, 3, 3, Cin]; s float32 [images, Cin] and demod float32
    [images, Cout], rows at any stride (views of gfp_styles' output); noise float32 [images, H, W]; bias float32 [Cout].
    form "fused": ca_modconv3x3, one launch, X never written; form "composed": ca_gfp_modulate into `scratch` ([images, H, W, Cin], allocated
    when None) + conv3x3 without split-K + ca_gfp_style_epilogue in place (one rounding more, of the convolution's output); None: "fused"
    from MODCONV_FUSED_MIN_PIXELS output pixels per image.  Either form gives an image the same bits whatever the batch it is part of."""
    who = "ca_modconv3x3"
    _need(form in (None, "fused", "composed"), who, 'form must be None, "fused" or "composed"')
    sc, sh = sft if sft is not None else (None, None)
    _req_cuda(who, "x wt s demod noise bias sft sft out", x, wt, s, demod, noise, bias, sc, sh, out)
    nx, h, w, cin = _t(who, "x", x, None, _D4)
    n = nx if images is None else int(images)
    cout = _t(who, "wt", wt, x.dtype, _D4)[0]
    _need(nx == n or nx == 1, who, "x holds one image per output image, or one shared by all", x)
    _t(who, "wt", wt, None, (cout, 3, 3, cin))
    hh, ww = (2 * h, 2 * w) if upsample else (h, w)
    _t(who, "s", s, torch.float32, (n, cin), contiguous=False)
    _t(who, "demod", demod, torch.float32, (n, cout), contiguous=False)
    _need(s.stride(1) == 1 and demod.stride(1) == 1, who, "s and demod must have unit column stride", s)
    _t(who, "noise", noise, torch.float32, (n, hh, ww))
    _t(who, "bias", bias, torch.float32, numel=cout)
    if sc is not None:
        _t(who, "sft scale", sc, x.dtype, (n, hh, ww, cout // 2))
        _t(who, "sft shift", sh, x.dtype, (n, hh, ww, cout // 2))
    out = _out(who, "out", out, (n, hh, ww, cout), x.dtype, x.device)
    s_stride, demod_stride = (s.stride(0), demod.stride(0)) if n > 1 else (0, 0)
    if form is None:
        form = "fused" if hh * ww >= MODCONV_FUSED_MIN_PIXELS else "composed"
    if form == "composed":
        if scratch is None:
            scratch = torch.empty((n, hh, ww, cin), dtype=x.dtype, device=x.device)
        _t(who, "scratch", scratch, x.dtype, (n, hh, ww, cin))
        check(lib().ca_gfp_modulate(_p(x), _p(s), s_stride, _p(scratch), n, h, w, cin, int(bool(upsample)), int(nx == 1 and n > 1), dt_code(x.dtype), _stream()),
              "ca_gfp_modulate")
        conv3x3(scratch, wt, out=out, split_k=False)
        check(lib().ca_gfp_style_epilogue(_p(out), _p(demod), demod_stride, _p(noise), float(noise_weight), _p(bias), _p(sc), _p(sh), _p(out), n, hh, ww, cout,
                                          dt_code(x.dtype), _stream()), "ca_gfp_style_epilogue")
        return out
    args = _capi.ModconvArgs(x=_p(x), wt=_p(wt), s=_p(s), demod=_p(demod), noise=_p(noise), bias=_p(bias), sft_scale=_p(sc), sft_shift=_p(sh), y=_p(out),
                             s_stride=s_stride, demod_stride=demod_stride, images=n, h=h, w=w, cin=cin, cout=cout, upsample=int(bool(upsample)),
                             x_shared=int(nx == 1 and n > 1), noise_weight=float(noise_weight), dtype=dt_code(x.dtype))
    check(lib().ca_modconv3x3(C.byref(args), _stream()), "ca_modconv3x3")
    return out


def gfp_to_rgb(x: torch.Tensor, wt: torch.Tensor, s: torch.Tensor, bias: torch.Tensor, out: torch.Tensor, prev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ToRGB (ca_gfp_to_rgb): `out` float32 [images, H, W, 3] = conv1x1(wt * s[n], x) + bias + the bilinear x2 of prev (float32
    [images, H / 2, W / 2, 3]).  x [images, H, W, Cin]; wt float32 [3, Cin]; s float32 [images, Cin] (rows at any stride); bias float32 [3]."""
    who = "ca_gfp_to_rgb"
    _req_cuda(who, "x wt s bias out prev", x, wt, s, bias, out, prev)
    n, h, w, cin = _t(who, "x", x, None, _D4)
    _t(who, "wt", wt, torch.float32, (3, cin))
    _t(who, "bias", bias, torch.float32, numel=3, contiguous=False)
    _t(who, "s", s, torch.float32, (n, cin), contiguous=False)
    _need(s.stride(1) == 1, who, "s must have unit column stride", s)
    _t(who, "out", out, torch.float32, (n, h, w, 3))
    if prev is not None:
        _t(who, "prev", prev, torch.float32, (n, h // 2, w // 2, 3))
        _need(h % 2 == 0 and w % 2 == 0, who, "with prev, H and W of x must be even", x)
    check(lib().ca_gfp_to_rgb(_p(x), _p(wt), _p(s), s.stride(0) if n > 1 else 0, _p(bias), _p(prev), _p(out), n, h, w, cin, dt_code(x.dtype), _stream()),
          "ca_gfp_to_rgb")
    return out


def gfp_finish(pre: torch.Tensor, out: torch.Tensor, reverse_channels: bool = True) -> torch.Tensor:
    """float32 [..., 3] -> uint8 of the same shape: rint((clamp(pre, -1, 1) + 1) / 2 * 255), half to even, the channel order reversed with
    reverse_channels (ca_gfp_finish)."""
    _req_cuda("ca_gfp_finish", "pre out", pre, out)
    _need(pre.dtype == torch.float32 and pre.shape[-1] == 3 and pre.is_contiguous() and pre.numel() > 0, "ca_gfp_finish", "pre must be contiguous float32 [..., 3]", pre)
    _t("ca_gfp_finish", "out", out, torch.uint8, tuple(pre.shape))
    check(lib().ca_gfp_finish(_p(pre), _p(out), pre.numel() // 3, int(bool(reverse_channels)), _stream()), "ca_gfp_finish")
    return out


# ---- added to ABI v16: the depth annotator's stages beside gemm / attention_spatial / conv3x3 (controlanimate_amd/depth.py: DepthAnnotator) -----------
def _req_i32(who: str, names: str, *ts):
    for name, t in zip(names.split(), ts):
        _t(who, name, t, torch.int32, what="int32 tables, contiguous")


def resize_pil_u8(frames: torch.Tensor, dh: int, dw: int, xbounds: torch.Tensor, xcoef: torch.Tensor, ybounds: torch.Tensor, ycoef: torch.Tensor,
                  tmp: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Pillow's Image.resize of uint8 RGB frames [images, H, W, 3] -> [images, dh, dw, 3] (ca_resize_pil_u8): bounds int32 [out, 2] and
    coefficients int32 [out, ksize] per axis, as depth.pil_coeffs builds them; tmp uint8 [images, H, dw, 3]."""
    _req_cuda("ca_resize_pil_u8", "frames xbounds xcoef ybounds ycoef tmp out", frames, xbounds, xcoef, ybounds, ycoef, tmp, out)
    n, sh, sw = _req_rgb8("ca_resize_pil_u8", "frames", frames)
    for name, t, shape in (("xbounds", xbounds, (dw, 2)), ("xcoef", xcoef, (dw, None)), ("ybounds", ybounds, (dh, 2)), ("ycoef", ycoef, (dh, None))):
        _t("ca_resize_pil_u8", name, t, torch.int32, shape, what="int32 tables [out, 2] / [out, ksize]")
    if tmp is not None:
        _t("ca_resize_pil_u8", "tmp", tmp, torch.uint8)
        _need(tmp.numel() >= n * sh * dw * 3, "ca_resize_pil_u8", "tmp holds fewer than images * H * dw * 3 bytes", tmp)
    out = _out("ca_resize_pil_u8", "out", out, (n, dh, dw, 3), torch.uint8, frames.device)
    if tmp is None:
        tmp = torch.empty((n, sh, dw, 3), dtype=torch.uint8, device=frames.device)
    check(lib().ca_resize_pil_u8(_p(frames), _p(tmp), _p(out), n, sh, sw, dh, dw, _p(xbounds), _p(xcoef), xcoef.shape[1], _p(ybounds), _p(ycoef), ycoef.shape[1],
                                 _stream()), "ca_resize_pil_u8")
    return out


def dpt_patches(frames: torch.Tensor, patch: int, dtype: torch.dtype, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 RGB [images, S, S, 3] -> (x / 255 - 0.5) / 0.5 as patch rows [images * (S / patch)^2, 3 * patch * patch] in the (c, ky, kx)
    order of the patch-embedding weight (ca_dpt_patches)."""
    _req_cuda("ca_dpt_patches", "frames out", frames, out)
    n, s, s2 = _req_rgb8("ca_dpt_patches", "frames", frames)
    _need(s == s2 and patch > 0 and s % patch == 0, "ca_dpt_patches", "frames must be square with a side that is a multiple of patch", frames)
    rows = n * (s // patch) ** 2
    out = _out("ca_dpt_patches", "out", out, (rows, 3 * patch * patch), dtype, frames.device)
    check(lib().ca_dpt_patches(_p(frames), _p(out), n, s, patch, dt_code(dtype), _stream()), "ca_dpt_patches")
    return out


def depth_to_space(x: torch.Tensor, images: int, gh: int, gw: int, k: int, cout: int, *, rows_per_image: Optional[int] = None, row0: int = 0,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The scatter behind ConvTranspose2d(kernel = stride = k) as a GEMM with N = k * k * cout (ca_depth_to_space): x [rows, >= k * k * cout]
    (columns (ky, kx, co)), row images * rows_per_image + row0 + y * gw + x -> NHWC [images, gh * k, gw * k, cout]."""
    _req_cuda("ca_depth_to_space", "x out", x, out)
    rpi = gh * gw if rows_per_image is None else rows_per_image
    _need(x.dim() == 2 and x.stride(1) == 1 and x.shape[0] >= images * rpi and x.shape[1] >= k * k * cout, "ca_depth_to_space",
          "x must be [>= images * rows_per_image, >= k * k * cout] with unit column stride", x)
    out = _out("ca_depth_to_space", "out", out, (images, gh * k, gw * k, cout), x.dtype, x.device)
    check(lib().ca_depth_to_space(_p(x), _p(out), images, gh, gw, k, cout, x.stride(0), rpi, row0, dt_code(x.dtype), _stream()), "ca_depth_to_space")
    return out


def dpt_head_supported(cmid: int) -> bool:
    """Does ca_dpt_head take this width (no launch, no device access)?"""
    return bool(lib().ca_dpt_head_supported(int(cmid)))


def dpt_head(x: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, w3: torch.Tensor, b3: torch.Tensor, *, out: Optional[torch.Tensor] = None,
             fused: Optional[bool] = None, up: Optional[torch.Tensor] = None, mid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """head.head.1 .. 5 of DPTDepthEstimationHead on x [images, h, w, Cmid]: align-corners bilinear x2, Conv3x3(Cmid -> 32) + bias + ReLU,
    Conv1x1(32 -> 1) + bias + ReLU -> float32 [images, 2h, 2w].  w2: [32, 3, 3, Cmid] of x's dtype; b2, w3 float32 [32]; b3 float32 [1].
    fused (default: context.dispatch.dpt_head_fused, which is off, where the library takes the width): ONE launch that never writes the
    upsampled plane (ca_dpt_head); otherwise upsample2x_bilinear_ac into `up`, conv3x3(act=RELU, out_f32) into `mid` and ca_dpt_logit -- the
    faster form as measured (profiles/depth_bench.json), and the default."""
    _req_cuda("ca_dpt_head", "x w2 b2 w3 b3 out up mid", x, w2, b2, w3, b3, out, up, mid)
    n, h, w, c = _t("ca_dpt_head", "x", x, None, _D4)
    _t("ca_dpt_head", "w2", w2, x.dtype, (32, 3, 3, c))
    for name, t, k in (("b2", b2, 32), ("w3", w3, 32), ("b3", b3, 1)):
        _t("ca_dpt_head", name, t, torch.float32, numel=k)
    out = _out("ca_dpt_head", "out", out, (n, 2 * h, 2 * w), torch.float32, x.device)
    if fused is None:
        fused = dispatch.dpt_head_fused and dpt_head_supported(c)
    if fused:
        check(lib().ca_dpt_head(_p(x), _p(w2), _p(b2), _p(w3), _p(b3), _p(out), n, h, w, c, dt_code(x.dtype), _stream()), "ca_dpt_head")
        return out
    if up is None:
        up = torch.empty((n, 2 * h, 2 * w, c), dtype=x.dtype, device=x.device)
    upsample2x_bilinear_ac(x, up)
    mid = conv3x3(up, w2, bias=b2, act=ACT_RELU, out_f32=True, out=mid)
    check(lib().ca_dpt_logit(_p(mid), _p(w3), _p(b3), _p(out), n * 4 * h * w, _stream()), "ca_dpt_logit")
    return out


def resize_bicubic_f32(x: torch.Tensor, dh: int, dw: int, *, out: Optional[torch.Tensor] = None, keys: Optional[torch.Tensor] = None,
                       minmax: Optional[torch.Tensor] = None):
    """F.interpolate(mode="bicubic", align_corners=False) of float32 [images, h, w] -> (out [images, dh, dw], keys): keys int32 [images, 2] is
    the per-image (max, min) of `out` in the order-preserving encoding depth_finish reads; minmax float32 [images, 2] receives them as
    floats when given (ca_resize_bicubic_f32)."""
    _req_cuda("ca_resize_bicubic_f32", "x out keys minmax", x, out, keys, minmax)
    n, h, w = _t("ca_resize_bicubic_f32", "x", x, torch.float32, _D3)
    for name, t, dt in (("keys", keys, torch.int32), ("minmax", minmax, torch.float32)):
        if t is not None:
            _t("ca_resize_bicubic_f32", name, t, dt)
            _need(t.numel() >= 2 * n, "ca_resize_bicubic_f32", name + " holds fewer than 2 * images elements", t)
    out = _out("ca_resize_bicubic_f32", "out", out, (n, dh, dw), torch.float32, x.device)
    if keys is None:
        keys = torch.empty((n, 2), dtype=torch.int32, device=x.device)
    check(lib().ca_resize_bicubic_f32(_p(x), _p(out), _p(keys), _p(minmax), n, h, w, dh, dw, _stream()), "ca_resize_bicubic_f32")
    return out, keys


DEPTH_NORMALIZE = {"max": 0, "minmax": 1}


def depth_finish(depth: torch.Tensor, keys: torch.Tensor, normalize: str = "max", *, map: Optional[torch.Tensor] = None, control: Optional[torch.Tensor] = None,
                 rep: int = 1) -> None:
    """float32 depth [images, H, W] and resize_bicubic_f32's keys -> the uint8 map [images, H, W] and / or the control tensor
    [rep * images, 3, H, W] (float32 / float16, map / 255) in one launch (ca_depth_finish).  "max": trunc(d * 255 / max); "minmax":
    trunc((d - min) / (max - min) * 255); values <= -1 saturate to 0."""
    _req_cuda("ca_depth_finish", "depth keys map control", depth, keys, map, control)
    n, h, w = _t("ca_depth_finish", "depth", depth, torch.float32, _D3)
    _t("ca_depth_finish", "keys", keys, torch.int32)
    _need(keys.numel() >= 2 * n, "ca_depth_finish", "keys holds fewer than 2 * images elements", keys)
    if normalize not in DEPTH_NORMALIZE:
        raise ValueError(f"normalize={normalize!r} ('max' or 'minmax')")
    dt = _control_args("ca_depth_finish", n, h, w, map, control, rep, map_name="map")
    check(lib().ca_depth_finish(_p(depth), _p(keys), n, h, w, DEPTH_NORMALIZE[normalize], _p(map), _p(control), int(rep), dt, _stream()), "ca_depth_finish")


# ---- added to ABI v16: the OpenPose body annotator's stages beside conv3x3 / maxpool2x2 / gemm (controlanimate_amd/openpose.py: OpenposeAnnotator) ----

POSE_MAX_PEAKS, POSE_MAX_PEOPLE, POSE_AREA_TAPS = _capi.CA_POSE_MAX_PEAKS, _capi.CA_POSE_MAX_PEOPLE, _capi.CA_POSE_AREA_TAPS
POSE_OVERFLOW_PEAKS, POSE_OVERFLOW_PEOPLE = _capi.CA_POSE_OVERFLOW_PEAKS, _capi.CA_POSE_OVERFLOW_PEOPLE
POSE_PARTS, POSE_LIMBS, POSE_PAF = 18, 19, 38


def pose_prep(frames: torch.Tensor, tables, hs: int, ws: int, out: torch.Tensor) -> torch.Tensor:
    """uint8 RGB [images, H, W, 3] -> `out` [images, hp, wp, 8] fp16 / bf16: the INTER_AREA resize to hs x ws through the per-axis tables
    (xofs, xcnt, xw, yofs, ycnt, yw: openpose.area_tables), BGR, x / 256 - 0.5, zeros in the padding and in channels 3 .. 7 (ca_pose_prep)."""
    _req_cuda("ca_pose_prep", "frames out tables", frames, out, *tables)
    n, h, w = _req_rgb8("ca_pose_prep", "frames", frames)
    hp, wp = out.shape[1], out.shape[2]
    _t("ca_pose_prep", "out", out, None, (n, hp, wp, 8))
    xofs, xcnt, xw, yofs, ycnt, yw = tables
    for name, t, count in (("xofs", xofs, ws), ("xcnt", xcnt, ws), ("yofs", yofs, hs), ("ycnt", ycnt, hs)):
        _t("ca_pose_prep", name, t, torch.int32, numel=count, what="int32 tables, contiguous, one entry per output pixel of the axis")
    _t("ca_pose_prep", "xw", xw, torch.float32, (ws, POSE_AREA_TAPS))
    _t("ca_pose_prep", "yw", yw, torch.float32, (hs, POSE_AREA_TAPS))
    check(lib().ca_pose_prep(_p(frames), _p(out), _p(xofs), _p(xcnt), _p(xw), _p(yofs), _p(ycnt), _p(yw), n, h, w, hs, ws, hp, wp, dt_code(out.dtype), _stream()),
          "ca_pose_prep")
    return out


def _pixels_view(who: str, name: str, t: torch.Tensor):
    """(images, h, w, channels, pixel stride) of an NHWC tensor whose pixels are evenly spaced (a column range of a wider tensor)."""
    _need(t.dim() == 4 and t.stride(3) == 1, who, name + " must be NHWC with unit channel stride", t)
    n, h, w, c = t.shape
    ld = t.stride(2)
    _need(t.stride(1) == w * ld and (n == 1 or t.stride(0) == h * w * ld), who, name + ": pixels must be evenly spaced", t)
    return n, h, w, c, ld


def conv7x7(xs, ws_, *, biases=None, relu: bool = False, outs=None, direct: Optional[bool] = None, cols: Optional[torch.Tensor] = None):
    """Conv2d(Cin, Cout, 7, padding=3) of one or two independent problems of one shape: xs [images, H, W, Cin] NHWC tensors (each may be
    a column range of a wider tensor), ws_ [Cout, 7, 7, Cin], fp32 biases, optional ReLU -> outs (allocated when None; each may be a
    column range of a wider tensor).  direct (default: context.dispatch.pose_conv7_direct): ca_conv7x7, one launch for all problems, the
    implicit GEMM from an LDS halo tile; otherwise ca_im2col7x7 into `cols` + gemm (split-K) per problem."""
    xs, ws_ = list(xs), list(ws_)
    g = len(xs)
    who = "ca_conv7x7"
    _need(g in (1, 2) and len(ws_) == g, who, "xs and ws_ must hold the same one or two problems")
    biases = [None] * g if biases is None else list(biases)
    _req_cuda(who, "cols tensors", cols, *xs, *ws_, *biases)
    n, h, w, cin, ldx = _pixels_view(who, "xs", xs[0])
    cout = ws_[0].shape[0]
    for x, wt, b in zip(xs, ws_, biases):
        _need(_pixels_view(who, "xs", x) == (n, h, w, cin, ldx) and x.dtype == xs[0].dtype, who, "xs must share one shape, pixel stride and dtype", x)
        _t(who, "ws_", wt, x.dtype, (cout, 7, 7, cin))
        if b is not None:
            _t(who, "biases", b, torch.float32, numel=cout)
    if outs is None:
        outs = [torch.empty((n, h, w, cout), dtype=xs[0].dtype, device=xs[0].device) for _ in range(g)]
    outs = list(outs)
    ldy = _pixels_view(who, "outs", outs[0])[4]
    for o in outs:
        _need(_pixels_view(who, "outs", o) == (n, h, w, cout, ldy) and o.dtype == xs[0].dtype, who, "outs must be [images, H, W, Cout] of one pixel stride, of xs' dtype", o)
    if direct is None:
        direct = bool(dispatch.pose_conv7_direct)
    if direct:
        a = _capi.Conv7x7Args(ldx=ldx, ldy=ldy, groups=g, images=n, h=h, w_px=w, cin=cin, cout=cout, relu=int(relu), dtype=dt_code(xs[0].dtype))
        for i in range(g):
            a.x[i], a.w[i], a.bias[i], a.y[i] = _p(xs[i]), _p(ws_[i]), _p(biases[i]), _p(outs[i])
        check(lib().ca_conv7x7(C.byref(a), _stream()), "ca_conv7x7")
        return outs
    rows = n * h * w
    if cols is None:
        cols = torch.empty((rows, 49 * cin), dtype=xs[0].dtype, device=xs[0].device)
    else:
        _t(who, "cols", cols, xs[0].dtype)
        _need(cols.numel() >= rows * 49 * cin, who, "cols holds fewer than rows * 49 * Cin elements", cols)
        cols = cols.view(-1)[: rows * 49 * cin].view(rows, 49 * cin)
    for x, wt, b, o in zip(xs, ws_, biases, outs):
        check(lib().ca_im2col7x7(_p(x), _p(cols), n, h, w, cin, ldx, dt_code(x.dtype), _stream()), "ca_im2col7x7")
        gemm(cols, wt.view(cout, 49 * cin), bias=b, act=ACT_RELU if relu else ACT_NONE, out=torch.as_strided(o, (rows, cout), (ldy, 1)))
    return outs


def copy_cols(src: torch.Tensor, dst: torch.Tensor, col0: int) -> torch.Tensor:
    """src [rows, c] into columns col0 .. col0 + c - 1 of the contiguous dst [rows, ld] (ca_copy_cols)."""
    _req_cuda("ca_copy_cols", "src dst", src, dst)
    _t("ca_copy_cols", "src", src, None, _D2)
    _t("ca_copy_cols", "dst", dst, src.dtype, (src.shape[0], None))
    check(lib().ca_copy_cols(_p(src), _p(dst), src.shape[0], src.shape[1], dst.shape[1], col0, dt_code(src.dtype), _stream()), "ca_copy_cols")
    return dst


def pose_maps_workspace_bytes(images: int, hl: int, w: int) -> int:
    n = int(lib().ca_pose_maps_workspace_bytes(images, hl, w))
    if n <= 0:
        raise _capi.CAHipError(f"ca_pose_maps_workspace_bytes: images={images} hl={hl} w={w} is out of range")
    return n


def pose_maps(low: torch.Tensor, mx: torch.Tensor, my: torch.Tensor, raw: torch.Tensor, smooth: torch.Tensor, paf: torch.Tensor,
              ws: Optional[torch.Tensor] = None) -> None:
    """low fp32 [images, hl, wl, 64] (PAF in columns 0 .. 37, heat in 40 .. 58), mx fp32 [2, W, wl], my fp32 [2, H, hl] (the composite
    resampling matrix of an axis, then the same with the Gaussian on top) -> raw [images, 18, H, W], smooth [images, 18, H, W] and paf
    [images, 38, H, W], fp32 (ca_pose_maps)."""
    _req_cuda("ca_pose_maps", "low mx my raw smooth paf ws", low, mx, my, raw, smooth, paf, ws)
    n, hl, wl, c = low.shape
    h, w = my.shape[1], mx.shape[1]
    _t("ca_pose_maps", "low", low, torch.float32, (n, hl, wl, 64))
    _t("ca_pose_maps", "mx", mx, torch.float32, (2, w, wl))
    _t("ca_pose_maps", "my", my, torch.float32, (2, h, hl))
    _pose_planes("ca_pose_maps", raw, smooth, paf, n, h, w)
    if ws is None:
        ws = torch.empty(pose_maps_workspace_bytes(n, hl, w), dtype=torch.uint8, device=low.device)
    check(lib().ca_pose_maps(_p(low), _p(mx), _p(my), _p(ws), _ws_bytes(ws), _p(raw), _p(smooth), _p(paf), n, hl, wl, h, w, _stream()), "ca_pose_maps")


def _pose_planes(who: str, raw: torch.Tensor, smooth: torch.Tensor, paf: torch.Tensor, n: int, h: int, w: int) -> None:
    for name, t, ch in (("raw", raw, POSE_PARTS), ("smooth", smooth, POSE_PARTS), ("paf", paf, POSE_PAF)):
        _t(who, name, t, torch.float32, (n, ch, h, w))


def pose_decode_buffers(n: int, device) -> dict:
    """The tensors the three decode launches pass on, for n frames."""
    i32 = dict(dtype=torch.int32, device=device)
    return {"peaks": torch.empty((n, POSE_PARTS, POSE_MAX_PEAKS, 2), **i32), "scores": torch.empty((n, POSE_PARTS, POSE_MAX_PEAKS), dtype=torch.float32, device=device),
            "counts": torch.empty((n, POSE_PARTS), **i32), "overflow": torch.empty((n,), **i32),
            "conn_ij": torch.empty((n, POSE_LIMBS, POSE_MAX_PEAKS, 2), **i32), "conn_score": torch.empty((n, POSE_LIMBS, POSE_MAX_PEAKS), dtype=torch.float64, device=device),
            "conn_n": torch.empty((n, POSE_LIMBS), **i32), "keypoints": torch.empty((n, POSE_MAX_PEOPLE, POSE_PARTS, 2), **i32),
            "coords": torch.empty((n, POSE_MAX_PEOPLE, POSE_PARTS, 2), **i32), "people": torch.empty((n,), **i32)}


def pose_decode(raw: torch.Tensor, smooth: torch.Tensor, paf: torch.Tensor, buf: Optional[dict] = None, stage=None) -> dict:
    """raw / smooth [images, 18, H, W] and paf [images, 38, H, W], fp32 -> the buffers of pose_decode_buffers filled: peaks (ca_pose_peaks),
    connections (ca_pose_connect), keypoints / coords / people / overflow (ca_pose_assemble).  Three launches, no host read.
    stage(name) -> a (start, end) pair of events whose start is recorded, or None: called before each launch (the annotator's timings)."""
    _req_cuda("ca_pose_peaks", "raw smooth paf", raw, smooth, paf)
    n, _, h, w = raw.shape
    _pose_planes("ca_pose_peaks", raw, smooth, paf, n, h, w)
    b = pose_decode_buffers(n, raw.device) if buf is None else buf
    stage = stage or (lambda name: None)
    ev = stage("peaks")
    check(lib().ca_pose_peaks(_p(raw), _p(smooth), _p(b["peaks"]), _p(b["scores"]), _p(b["counts"]), _p(b["overflow"]), n, h, w, _stream()), "ca_pose_peaks")
    if ev:
        ev[1].record()
    ev = stage("connect")
    check(lib().ca_pose_connect(_p(paf), _p(b["peaks"]), _p(b["counts"]), _p(b["conn_ij"]), _p(b["conn_score"]), _p(b["conn_n"]), n, h, w, _stream()), "ca_pose_connect")
    if ev:
        ev[1].record()
    ev = stage("assemble")
    pose_assemble(b, h, w)
    if ev:
        ev[1].record()
    return b


def pose_assemble(b: dict, h: int, w: int) -> dict:
    """The peaks and connections of the buffers `b` (pose_decode_buffers) -> their keypoints, coords and people; overflow gets
    POSE_OVERFLOW_PEOPLE where a 65th subset row was needed (ca_pose_assemble; overflow must hold ca_pose_peaks' bits or zeros)."""
    n = b["people"].shape[0]
    check(lib().ca_pose_assemble(_p(b["peaks"]), _p(b["scores"]), _p(b["conn_ij"]), _p(b["conn_score"]), _p(b["conn_n"]), _p(b["keypoints"]), _p(b["coords"]),
                                 _p(b["people"]), _p(b["overflow"]), n, h, w, _stream()), "ca_pose_assemble")
    return b


def _draw_inputs(who: str, coords: torch.Tensor, people: torch.Tensor, sin_table: torch.Tensor) -> int:
    """What every pose_draw* reads: coords int32 [images, 64, 18, 2], people int32 [images], the float32 sine table; returns images."""
    n = coords.shape[0]
    _t(who, "coords", coords, torch.int32, (n, POSE_MAX_PEOPLE, POSE_PARTS, 2))
    _t(who, "people", people, torch.int32, (n,))
    _t(who, "sin_table", sin_table, torch.float32, numel=451)
    return n


def pose_draw(coords: torch.Tensor, people: torch.Tensor, sin_table: torch.Tensor, h: int, w: int, *, index: Optional[torch.Tensor] = None,
              skeleton: Optional[torch.Tensor] = None, control: Optional[torch.Tensor] = None, rep: int = 1) -> Optional[torch.Tensor]:
    """draw_bodypose of the people of every frame (coords int32 [images, 64, 18, 2] and people int32 [images] of pose_decode): the uint8
    map `skeleton` [images, h, w, 3] and / or the control tensor [rep * images, 3, h, w] (float32 / float16) = map / 255 (ca_pose_draw).
    index: the uint32 [images, h, w] plane the primitives' draw indices are resolved from."""
    _req_cuda("ca_pose_draw", "coords people sin_table index skeleton control", coords, people, sin_table, index, skeleton, control)
    n = _draw_inputs("ca_pose_draw", coords, people, sin_table)
    index = _out("ca_pose_draw", "index", index, (n, h, w), torch.int32, coords.device)
    if skeleton is None and control is None:
        skeleton = torch.empty((n, h, w, 3), dtype=torch.uint8, device=coords.device)
    dt = _control_args("ca_pose_draw", n, h, w, skeleton, control, rep, map_shape=(n, h, w, 3), map_name="skeleton")
    check(lib().ca_pose_draw(_p(coords), _p(people), _p(sin_table), _p(index), _p(skeleton), _p(control), n, h, w, int(rep), dt, _stream()), "ca_pose_draw")
    return skeleton


# ---- added to ABI v16: the face stage of the OpenPose annotator around its network (controlanimate_amd/openpose_face.py: FaceStage) ----

POSE_OVERFLOW_FACES, POSE_OVERFLOW_FACE_RESIZE = _capi.CA_POSE_OVERFLOW_FACES, _capi.CA_POSE_OVERFLOW_FACE_RESIZE
FACE_SIZE, FACE_HEAT, FACE_PARTS, FACE_MIN_SIDE, FACE_SLOT_INTS = _capi.CA_FACE_SIZE, _capi.CA_FACE_HEAT, _capi.CA_FACE_PARTS, _capi.CA_FACE_MIN_SIDE, _capi.CA_FACE_SLOT_INTS
FACE_MODE_NONE, FACE_MODE_LANCZOS4, FACE_MODE_AREA = _capi.CA_FACE_MODE_NONE, _capi.CA_FACE_MODE_LANCZOS4, _capi.CA_FACE_MODE_AREA


def face_buffers(n: int, max_faces: int, device) -> dict:
    """The tensors the face stage's launches pass on, for n frames."""
    i32 = dict(dtype=torch.int32, device=device)
    return {"boxes": torch.empty((n, POSE_MAX_PEOPLE, 4), **i32), "slots": torch.empty((n, max_faces, FACE_SLOT_INTS), **i32), "overflow": torch.empty((n,), **i32),
            "points": torch.empty((n, POSE_MAX_PEOPLE, FACE_PARTS, 2), **i32)}


def _boxes_operands(who: str, keypoints: torch.Tensor, people: torch.Tensor, overflow_in: Optional[torch.Tensor], buf: dict, box_shape: tuple, slot_ints: int) -> int:
    """The operands face_boxes and hand_boxes share; returns the slots per frame of buf["slots"]."""
    _req_cuda(who, "keypoints people overflow_in boxes slots overflow", keypoints, people, overflow_in, buf["boxes"], buf["slots"], buf["overflow"])
    n = keypoints.shape[0]
    _t(who, "keypoints", keypoints, torch.int32, (n, POSE_MAX_PEOPLE, POSE_PARTS, 2))
    _t(who, "people", people, torch.int32, (n,))
    if overflow_in is not None:
        _t(who, "overflow_in", overflow_in, torch.int32, (n,))
    slots = buf["slots"].shape[1]
    for name, shape in (("boxes", (n,) + box_shape), ("slots", (n, slots, slot_ints)), ("overflow", (n,))):
        _t(who, name, buf[name], torch.int32, shape, what="int32 tables as face_buffers / hand_buffers make them")
    return slots


def face_boxes(keypoints: torch.Tensor, people: torch.Tensor, h: int, w: int, buf: dict, overflow_in: Optional[torch.Tensor] = None) -> dict:
    """util.faceDetect per person of keypoints int32 [images, 64, 18, 2] / people int32 [images] -> buf["boxes"] (x, y, w, slot),
    buf["slots"] [images, max_faces, 8] (person, x, y, w, hc, wc, mode, 0) and buf["overflow"] = overflow_in | the face bits (ca_face_boxes)."""
    max_faces = _boxes_operands("ca_face_boxes", keypoints, people, overflow_in, buf, (POSE_MAX_PEOPLE, 4), FACE_SLOT_INTS)
    n = keypoints.shape[0]
    check(lib().ca_face_boxes(_p(keypoints), _p(people), _p(overflow_in), _p(buf["boxes"]), _p(buf["slots"]), _p(buf["overflow"]), n, h, w, max_faces, _stream()),
          "ca_face_boxes")
    return buf


def face_crop(frames: torch.Tensor, slots: torch.Tensor, tables: dict, out: torch.Tensor, first: int = 0) -> torch.Tensor:
    """uint8 RGB [images, H, W, 3] and slots [images, max_faces, 8] -> `out` [crops, 384, 384, 8] fp16 / bf16: the crops of slots first ..
    first + crops - 1 resized as cv2.resize does (INTER_LANCZOS4 / INTER_AREA by the slot's mode), BGR, x / 256 - 0.5 (ca_face_crop).
    tables: openpose_face.resize_tables(side_max) on the device (lz_ofs, lz_coef, ar_ofs, ar_cnt, ar_w, side_max)."""
    who = "ca_face_crop"
    _req_cuda(who, "frames slots out lz_ofs lz_coef ar_ofs ar_cnt ar_w", frames, slots, out, tables["lz_ofs"], tables["lz_coef"], tables["ar_ofs"], tables["ar_cnt"], tables["ar_w"])
    n, h, w = _req_rgb8(who, "frames", frames)
    max_faces = slots.shape[1]
    _t(who, "slots", slots, torch.int32, (n, max_faces, FACE_SLOT_INTS))
    crops = out.shape[0]
    _t(who, "out", out, None, (crops, FACE_SIZE, FACE_SIZE, 8))
    side_max = int(tables["side_max"])
    nl, na = side_max - FACE_MIN_SIDE + 1, side_max - FACE_SIZE + 1
    for name, dt, shape in (("lz_ofs", torch.int32, (nl, FACE_SIZE)), ("lz_coef", torch.int16, (nl, FACE_SIZE, 8)), ("ar_ofs", torch.int32, (na, FACE_SIZE)),
                            ("ar_cnt", torch.int32, (na, FACE_SIZE)), ("ar_w", torch.float32, (na, FACE_SIZE, 8))):
        _t(who, name, tables[name], dt, shape)
    check(lib().ca_face_crop(_p(frames), _p(slots), _p(out), _p(tables["lz_ofs"]), _p(tables["lz_coef"]), _p(tables["ar_ofs"]), _p(tables["ar_cnt"]), _p(tables["ar_w"]),
                             n, h, w, max_faces, int(first), crops, side_max, dt_code(out.dtype), _stream()), "ca_face_crop")
    return out


def face_peaks(heat: torch.Tensor, slots: torch.Tensor, points: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """heat fp32 [images * max_faces, 48, 48, 72] and slots [images, max_faces, 8] -> points int32 [images, 64, 71, 2]: per crop and part the
    first position of the largest align-corners bilinear value above 0.05 over the crop's pixels, in frame pixels (ca_face_peaks)."""
    _req_cuda("ca_face_peaks", "heat slots points", heat, slots, points)
    n, max_faces = slots.shape[0], slots.shape[1]
    _t("ca_face_peaks", "slots", slots, torch.int32, (n, max_faces, FACE_SLOT_INTS))
    _t("ca_face_peaks", "heat", heat, torch.float32, (n * max_faces, FACE_HEAT, FACE_HEAT, FACE_PARTS + 1))
    _t("ca_face_peaks", "points", points, torch.int32, (n, POSE_MAX_PEOPLE, FACE_PARTS, 2))
    check(lib().ca_face_peaks(_p(heat), _p(slots), _p(points), n, max_faces, h, w, _stream()), "ca_face_peaks")
    return points


def pose_draw_faces(coords: torch.Tensor, people: torch.Tensor, sin_table: torch.Tensor, points: Optional[torch.Tensor], xmap: Optional[torch.Tensor],
                    ymap: Optional[torch.Tensor], h: int, w: int, *, index: Optional[torch.Tensor] = None, skeleton: Optional[torch.Tensor] = None,
                    control: Optional[torch.Tensor] = None, rep: int = 1) -> Optional[torch.Tensor]:
    """pose_draw with the 71 radius-3 white discs of every person's face points int32 [images, 64, 71, 2] after that person's body and
    before the next person's (ca_pose_draw_faces).  xmap int32 [w], ymap int32 [h]: openpose_face.pixel_map.  points None: the bodies only."""
    who = "ca_pose_draw_faces"
    _req_cuda(who, "coords people sin_table points xmap ymap index skeleton control", coords, people, sin_table, points, xmap, ymap, index, skeleton, control)
    n = _draw_inputs(who, coords, people, sin_table)
    if points is not None:
        _t(who, "points", points, torch.int32, (n, POSE_MAX_PEOPLE, FACE_PARTS, 2))
        _t(who, "xmap", xmap, torch.int32, (w,), contiguous=False)
        _t(who, "ymap", ymap, torch.int32, (h,), contiguous=False)
    index = _out(who, "index", index, (n, h, w), torch.int32, coords.device)
    if skeleton is None and control is None:
        skeleton = torch.empty((n, h, w, 3), dtype=torch.uint8, device=coords.device)
    dt = _control_args(who, n, h, w, skeleton, control, rep, map_shape=(n, h, w, 3), map_name="skeleton")
    check(lib().ca_pose_draw_faces(_p(coords), _p(people), _p(sin_table), _p(points), _p(xmap), _p(ymap), _p(index), _p(skeleton), _p(control), n, h, w, int(rep), dt,
                                   _stream()), "ca_pose_draw_faces")
    return skeleton


# ---- added to ABI v16: the hand stage of the OpenPose annotator around its network (controlanimate_amd/openpose_hand.py) ------------------

POSE_OVERFLOW_HANDS, POSE_OVERFLOW_HAND_RESIZE = _capi.CA_POSE_OVERFLOW_HANDS, _capi.CA_POSE_OVERFLOW_HAND_RESIZE
HAND_PARTS, HAND_HEAT_COLS, HAND_MAP, HAND_SCALES, HAND_SLOT_INTS = _capi.CA_HAND_PARTS, _capi.CA_HAND_HEAT_COLS, _capi.CA_HAND_MAP, _capi.CA_HAND_SCALES, _capi.CA_HAND_SLOT_INTS
HAND_MODE_NONE, HAND_MODE_RESIZE = _capi.CA_HAND_MODE_NONE, _capi.CA_HAND_MODE_RESIZE
HAND_MAP_SIDES = (23, 46, 69, 92)
_HAND_HEATS = tuple(f"heats: heat of side {m}" for m in HAND_MAP_SIDES)


def hand_buffers(n: int, max_hands: int, device) -> dict:
    """The tensors the hand stage's launches pass on, for n frames."""
    i32 = dict(dtype=torch.int32, device=device)
    slots = n * max_hands
    return {"boxes": torch.empty((n, POSE_MAX_PEOPLE, 2, 4), **i32), "slots": torch.empty((n, max_hands, HAND_SLOT_INTS), **i32), "overflow": torch.empty((n,), **i32),
            "points": torch.empty((n, POSE_MAX_PEOPLE, 2, HAND_PARTS, 2), **i32), "peaks": torch.empty((slots, HAND_PARTS, 2), **i32),
            "mass": torch.empty((slots, HAND_PARTS), dtype=torch.float64, device=device),
            "raw": torch.empty((slots, HAND_PARTS, HAND_MAP, HAND_MAP), dtype=torch.float32, device=device),
            "smooth": torch.empty((slots, HAND_PARTS, HAND_MAP, HAND_MAP), dtype=torch.float32, device=device)}


def hand_boxes(keypoints: torch.Tensor, people: torch.Tensor, h: int, w: int, buf: dict, overflow_in: Optional[torch.Tensor] = None) -> dict:
    """util.handDetect per person of keypoints int32 [images, 64, 18, 2] / people int32 [images] -> buf["boxes"] [images, 64, 2, 4] (x, y, w,
    slot; left then right), buf["slots"] [images, max_hands, 8] (person, x, y, w, hand, mode, 0, 0) and buf["overflow"] = overflow_in | the
    hand bits (ca_hand_boxes)."""
    max_hands = _boxes_operands("ca_hand_boxes", keypoints, people, overflow_in, buf, (POSE_MAX_PEOPLE, 2, 4), HAND_SLOT_INTS)
    n = keypoints.shape[0]
    check(lib().ca_hand_boxes(_p(keypoints), _p(people), _p(overflow_in), _p(buf["boxes"]), _p(buf["slots"]), _p(buf["overflow"]), n, h, w, max_hands, _stream()),
          "ca_hand_boxes")
    return buf


def hand_crop(frames: torch.Tensor, slots: torch.Tensor, tables: dict, blurred: torch.Tensor, out: torch.Tensor, first: int = 0, blur: bool = True) -> torch.Tensor:
    """uint8 RGB [images, H, W, 3] and slots [images, max_hands, 8] -> `out` [crops, side, side, 8] fp16 / bf16: the Gaussian-blurred crops of
    slots first .. first + crops - 1 resized to side x side as cv2.resize does, BGR, x / 256 - 0.5 (ca_hand_crop).  blurred uint8 [images *
    max_hands, min(H, W), min(H, W), 3] is written when `blur`, else read.  tables: openpose_hand.resize_tables(side, min(H, W)) on the
    device (taps, lz_ofs, lz_coef, ar_ofs, ar_cnt, ar_w; the AREA ones None when no box can be wider than side)."""
    who = "ca_hand_crop"
    _req_cuda(who, "frames slots blurred out tables", frames, slots, blurred, out, *[t for t in tables.values() if isinstance(t, torch.Tensor)])
    n, h, w = _req_rgb8(who, "frames", frames)
    max_hands, side_max = slots.shape[1], min(h, w)
    _t(who, "slots", slots, torch.int32, (n, max_hands, HAND_SLOT_INTS))
    crops, side = out.shape[0], out.shape[1]
    _t(who, "out", out, None, (crops, side, side, 8))
    _t(who, "blurred", blurred, torch.uint8, (n * max_hands, side_max, side_max, 3))
    nl, na = min(side, side_max) - _capi.CA_HAND_MIN_BOX + 1, max(side_max - side, 0)
    _t(who, "taps", tables["taps"], torch.float64, (7,), contiguous=False)
    _t(who, "lz_ofs", tables["lz_ofs"], torch.int32, (nl, side))
    _t(who, "lz_coef", tables["lz_coef"], torch.int16, (nl, side, 8))
    if na:
        _t(who, "ar_ofs", tables["ar_ofs"], torch.int32, (na, side))
        _t(who, "ar_cnt", tables["ar_cnt"], torch.int32, (na, side))
        _t(who, "ar_w", tables["ar_w"], torch.float32, (na, side, _capi.CA_HAND_AREA_TAPS))
    check(lib().ca_hand_crop(_p(frames), _p(slots), _p(tables["taps"]), _p(blurred), _p(out), _p(tables["lz_ofs"]), _p(tables["lz_coef"]), _p(tables.get("ar_ofs")),
                             _p(tables.get("ar_cnt")), _p(tables.get("ar_w")), n, h, w, max_hands, int(first), crops, side, side_max, int(bool(blur)), dt_code(out.dtype),
                             _stream()), "ca_hand_crop")
    return out


def hand_maps(heats, mats: torch.Tensor, raw: torch.Tensor, smooth: torch.Tensor) -> None:
    """heats: the network's fp32 maps of the four scales, [slots, m, m, 24] with m = 23, 46, 69, 92; mats fp32 [2, 230, 128]
    (openpose_hand.map_matrices) -> raw, smooth fp32 [slots, 21, 128, 128]: the four-scale average and its sigma-3 Gaussian (ca_hand_maps)."""
    _req_cuda("ca_hand_maps", "mats raw smooth heats", mats, raw, smooth, *heats)
    slots = raw.shape[0]
    _need(len(heats) == HAND_SCALES, "ca_hand_maps", "heats must be the maps of the four scales")
    for name, m, t in zip(_HAND_HEATS, HAND_MAP_SIDES, heats):
        _t("ca_hand_maps", name, t, torch.float32, (slots, m, m, HAND_HEAT_COLS))
    _t("ca_hand_maps", "mats", mats, torch.float32, (2, sum(HAND_MAP_SIDES), HAND_MAP))
    _t("ca_hand_maps", "raw", raw, torch.float32, (slots, HAND_PARTS, HAND_MAP, HAND_MAP))
    _t("ca_hand_maps", "smooth", smooth, torch.float32, (slots, HAND_PARTS, HAND_MAP, HAND_MAP))
    check(lib().ca_hand_maps(*[_p(t) for t in heats], _p(mats), _p(raw), _p(smooth), slots, _stream()), "ca_hand_maps")


def hand_peaks(raw: torch.Tensor, smooth: torch.Tensor, buf: dict, h: int, w: int) -> dict:
    """raw, smooth fp32 [images * max_hands, 21, 128, 128] and buf["slots"] -> buf["peaks"] (x, y on the 128 grid), buf["mass"] (the winning
    component's double sum) and buf["points"] int32 [images, 64, 2, 21, 2] in frame pixels (ca_hand_peaks)."""
    _req_cuda("ca_hand_peaks", "raw smooth slots points peaks mass", raw, smooth, buf["slots"], buf["points"], buf["peaks"], buf["mass"])
    n, max_hands = buf["slots"].shape[0], buf["slots"].shape[1]
    slots = n * max_hands
    _t("ca_hand_peaks", "raw", raw, torch.float32, (slots, HAND_PARTS, HAND_MAP, HAND_MAP))
    _t("ca_hand_peaks", "smooth", smooth, torch.float32, (slots, HAND_PARTS, HAND_MAP, HAND_MAP))
    for name, shape in (("slots", (n, max_hands, HAND_SLOT_INTS)), ("points", (n, POSE_MAX_PEOPLE, 2, HAND_PARTS, 2)), ("peaks", (slots, HAND_PARTS, 2))):
        _t("ca_hand_peaks", name, buf[name], torch.int32, shape, what="int32 tables as hand_buffers makes them")
    _t("ca_hand_peaks", "mass", buf["mass"], torch.float64, (slots, HAND_PARTS))
    check(lib().ca_hand_peaks(_p(raw), _p(smooth), _p(buf["slots"]), _p(buf["points"]), _p(buf["peaks"]), _p(buf["mass"]), n, max_hands, h, w, _stream()), "ca_hand_peaks")
    return buf


def pose_draw_hands(coords: torch.Tensor, people: torch.Tensor, sin_table: torch.Tensor, hand_points: torch.Tensor, face_points: Optional[torch.Tensor],
                    xmap: torch.Tensor, ymap: torch.Tensor, h: int, w: int, *, index: Optional[torch.Tensor] = None, skeleton: Optional[torch.Tensor] = None,
                    control: Optional[torch.Tensor] = None, rep: int = 1) -> Optional[torch.Tensor]:
    """pose_draw_faces with hands: per person the body, the left hand, the right hand (20 thickness-2 edges and 21 radius-4 circles each, from
    hand_points int32 [images, 64, 2, 21, 2]), then the face discs (face_points int32 [images, 64, 71, 2] or None) (ca_pose_draw_hands)."""
    who = "ca_pose_draw_hands"
    _req_cuda(who, "coords people sin_table hand_points face_points xmap ymap index skeleton control", coords, people, sin_table, hand_points, face_points, xmap, ymap, index,
              skeleton, control)
    n = _draw_inputs(who, coords, people, sin_table)
    _t(who, "hand_points", hand_points, torch.int32, (n, POSE_MAX_PEOPLE, 2, HAND_PARTS, 2))
    if face_points is not None:
        _t(who, "face_points", face_points, torch.int32, (n, POSE_MAX_PEOPLE, FACE_PARTS, 2))
    _t(who, "xmap", xmap, torch.int32, (w,), contiguous=False)
    _t(who, "ymap", ymap, torch.int32, (h,), contiguous=False)
    index = _out(who, "index", index, (n, h, w), torch.int32, coords.device)
    if skeleton is None and control is None:
        skeleton = torch.empty((n, h, w, 3), dtype=torch.uint8, device=coords.device)
    dt = _control_args(who, n, h, w, skeleton, control, rep, map_shape=(n, h, w, 3), map_name="skeleton")
    check(lib().ca_pose_draw_hands(_p(coords), _p(people), _p(sin_table), _p(hand_points), _p(face_points), _p(xmap), _p(ymap), _p(index), _p(skeleton), _p(control),
                                   n, h, w, int(rep), dt, _stream()), "ca_pose_draw_hands")
    return skeleton


# ---- added to ABI v16: the NormalBae annotator's stages beside gemm / conv3x3 / upsample2x_bilinear_ac (controlanimate_amd/normalbae.py: NormalBaeAnnotator) ----
ACT_LEAKY001 = _capi.CA_ACT_LEAKY001  # nn.LeakyReLU() (slope 0.01) in the epilogue of conv3x3 / gemm


def same_out(size: int, stride: int) -> int:
    """The output size of a TensorFlow-SAME convolution: ceil(size / stride)."""
    return -(-size // stride)


def nbae_stem(frames: torch.Tensor, wt: torch.Tensor, bias: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """uint8 RGB [images, H, W, 3] -> `out` [images, H/2, W/2, cout]: swish(Conv3x3 stride 2, SAME padding, of the ImageNet-normalised frame +
    bias) (ca_nbae_stem).  wt: float32 [27, cout] (row (ky * 3 + kx) * 3 + channel, BatchNorm folded); bias: float32 [cout]."""
    _req_cuda("ca_nbae_stem", "frames wt bias out", frames, wt, bias, out)
    n, h, w = _req_rgb8("ca_nbae_stem", "frames", frames)
    cout = out.shape[3]
    _t("ca_nbae_stem", "wt", wt, torch.float32, (27, cout))
    _t("ca_nbae_stem", "bias", bias, torch.float32, numel=cout, contiguous=False)
    _need(h % 2 == 0 and w % 2 == 0, "ca_nbae_stem", "H and W of frames must be even", frames)
    _t("ca_nbae_stem", "out", out, None, (n, h // 2, w // 2, cout))
    check(lib().ca_nbae_stem(_p(frames), _p(wt), _p(bias), _p(out), n, h, w, cout, dt_code(out.dtype), _stream()), "ca_nbae_stem")
    return out


def dwconv_same_partials_floats(images: int, h: int, w: int, c: int, stride: int) -> int:
    n = int(lib().ca_dwconv_same_partials_floats(images, h, w, c, stride))
    if n <= 0:
        raise _capi.CAHipError(f"ca_dwconv_same_partials_floats: images={images} h={h} w={w} c={c} stride={stride} out of range")
    return n


def dwconv_same(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, *, stride: int = 1, out: Optional[torch.Tensor] = None, sums: Optional[torch.Tensor] = None,
                partials: Optional[torch.Tensor] = None):
    """Depthwise k x k (3 or 5) convolution with TensorFlow-SAME padding + bias + swish of NHWC x [images, H, W, C] (ca_dwconv_same).
    w: [k * k, C] of x's dtype (tap ky * k + kx of every channel), bias float32 [C].  -> (out [images, ceil(H / stride), ceil(W / stride), C],
    sums float32 [images, C]: the sum over the plane of the stored values).  partials: float32 scratch of dwconv_same_partials_floats."""
    who = "ca_dwconv_same"
    _req_cuda(who, "x w bias out sums partials", x, w, bias, out, sums, partials)
    n, h, ww, c = _t(who, "x", x, None, _D4)
    _need(stride in (1, 2), who, "stride must be 1 or 2")
    _need(w.dim() == 2 and w.shape[0] in (9, 25), who, "w: [9 or 25, C] of x's dtype", w)
    _t(who, "w", w, x.dtype, (None, c), what="w: [9 or 25, C] of x's dtype")
    _t(who, "bias", bias, torch.float32, numel=c)
    ksize = 3 if w.shape[0] == 9 else 5
    if sums is not None:
        _t(who, "sums", sums, torch.float32, (n, c))
    out = _out(who, "out", out, (n, same_out(h, stride), same_out(ww, stride), c), x.dtype, x.device)
    if sums is None:
        sums = torch.empty((n, c), dtype=torch.float32, device=x.device)
    need = dwconv_same_partials_floats(n, h, ww, c, stride)
    if partials is None:
        partials = torch.empty(need, dtype=torch.float32, device=x.device)
    _t(who, "partials", partials, torch.float32)
    _need(partials.numel() >= need, who, "partials holds fewer floats than dwconv_same_partials_floats asks for", partials)
    check(lib().ca_dwconv_same(_p(x), _p(w), _p(bias), _p(out), _p(sums), _p(partials), n, h, ww, c, ksize, int(stride), dt_code(x.dtype), _stream()), "ca_dwconv_same")
    return out, sums


def se_gate(sums: torch.Tensor, w_reduce: torch.Tensor, b_reduce: torch.Tensor, w_expand_t: torch.Tensor, b_expand: torch.Tensor, pixels: int,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gate float32 [images, C] = sigmoid(W_e swish(W_r (sums / pixels) + b_r) + b_e), all float32 (ca_se_gate).  w_reduce [r, C], b_reduce [r],
    w_expand_t [r, C] (the expand weight transposed), b_expand [C]."""
    who = "ca_se_gate"
    _req_cuda(who, "sums w_reduce b_reduce w_expand_t b_expand out", sums, w_reduce, b_reduce, w_expand_t, b_expand, out)
    n, c = sums.shape
    r = w_reduce.shape[0]
    for name, t, shape in (("sums", sums, (n, c)), ("w_reduce", w_reduce, (r, c)), ("b_reduce", b_reduce, (r,)), ("w_expand_t", w_expand_t, (r, c)), ("b_expand", b_expand, (c,))):
        _t(who, name, t, torch.float32, shape)
    out = _out(who, "out", out, (n, c), torch.float32, sums.device)
    check(lib().ca_se_gate(_p(sums), _p(w_reduce), _p(b_reduce), _p(w_expand_t), _p(b_expand), _p(out), n, c, r, 1.0 / float(pixels), _stream()), "ca_se_gate")
    return out


def scale_channels(x: torch.Tensor, gate: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """round(x * gate[image, channel]) for NHWC x and gate float32 [images, C]; out=x scales in place (ca_scale_channels)."""
    _req_cuda("ca_scale_channels", "x gate out", x, gate, out)
    n, h, w, c = _t("ca_scale_channels", "x", x, None, _D4)
    _t("ca_scale_channels", "gate", gate, torch.float32, (n, c))
    out = _out("ca_scale_channels", "out", out, (n, h, w, c), x.dtype, x.device)
    check(lib().ca_scale_channels(_p(x), _p(gate), _p(out), n, h * w, c, dt_code(x.dtype), _stream()), "ca_scale_channels")
    return out


def nbae_cat_pred(pred: torch.Tensor, out: torch.Tensor, col0: int = 0) -> torch.Tensor:
    """The float32 prediction [images, h, w, 4], x2 bilinear with align_corners in float32, rounded into columns col0 .. col0 + 3 of `out`
    [images, 2h, 2w, ld] and zeros into col0 + 4 .. col0 + 7 (ca_nbae_cat_pred)."""
    _req_cuda("ca_nbae_cat_pred", "pred out", pred, out)
    n, h, w, _ = _t("ca_nbae_cat_pred", "pred", pred, torch.float32, (None, None, None, 4))
    _t("ca_nbae_cat_pred", "out", out, None, (n, 2 * h, 2 * w, None))
    check(lib().ca_nbae_cat_pred(_p(pred), _p(out), n, h, w, out.shape[3], int(col0), dt_code(out.dtype), _stream()), "ca_nbae_cat_pred")
    return out


NBAE_MIN_KAPPA = 0.01


def nbae_normalize(raw: torch.Tensor, out: torch.Tensor, min_kappa: float = NBAE_MIN_KAPPA) -> torch.Tensor:
    """norm_normalize of the first four of raw's float32 columns [rows, ld] -> `out` float32 [rows, 4]: xyz / (|xyz| + 1e-10),
    elu(kappa) + 1 + min_kappa (ca_nbae_normalize)."""
    _req_cuda("ca_nbae_normalize", "raw out", raw, out)
    _t("ca_nbae_normalize", "raw", raw, torch.float32, _D2)
    _need(raw.shape[1] % 4 == 0, "ca_nbae_normalize", "raw must have a multiple of 4 columns", raw)
    _t("ca_nbae_normalize", "out", out, torch.float32, numel=raw.shape[0] * 4)
    check(lib().ca_nbae_normalize(_p(raw), raw.shape[1], _p(out), raw.shape[0], float(min_kappa), _stream()), "ca_nbae_normalize")
    return out


NBAE_REFINE_C = (128, 256, 512)   # the feature widths ca_nbae_refine is built for (hidden width 128)


def nbae_refine(feat: torch.Tensor, pred: torch.Tensor, frags, biases, out: torch.Tensor, min_kappa: float = NBAE_MIN_KAPPA) -> torch.Tensor:
    """One refinement stage in one launch (ca_nbae_refine): feat [images, h, w, C], C in NBAE_REFINE_C, and the float32 prediction
    [images, h, w, 4] -> `out` float32 [images, 2h, 2w, 4].  frags: the four weight fragments of normalbae.pack_mlp_frag; biases: float32
    [128] x 3 and [4]."""
    who = "ca_nbae_refine"
    _req_cuda(who, "feat pred out tensors", feat, pred, out, *frags, *biases)
    n, h, w, c = _t(who, "feat", feat, None, _D4)
    _need(c in NBAE_REFINE_C, who, "feat must have 128, 256 or 512 channels", feat)
    kp = (c + 8 + 31) // 32 * 32
    _t(who, "pred", pred, torch.float32, (n, h, w, 4))
    _t(who, "out", out, torch.float32, (n, 2 * h, 2 * w, 4))
    for f, elems in zip(frags, (128 * kp, 128 * 128, 128 * 128, 16 * 128)):
        _t(who, "frags", f, feat.dtype, numel=elems)
    for b, elems in zip(biases, (128, 128, 128, 4)):
        _t(who, "biases", b, torch.float32, numel=elems)
    if _plan_sink is not None:
        _plan_sink.append(f"nbae_refine_c{c}")
    check(lib().ca_nbae_refine(_p(feat), _p(pred), *[_p(f) for f in frags], *[_p(b) for b in biases], _p(out), n, h, w, c, float(min_kappa), dt_code(feat.dtype),
                               _stream()), "ca_nbae_refine")
    return out


def nbae_finish(pred: torch.Tensor, map: Optional[torch.Tensor] = None, control: Optional[torch.Tensor] = None, rep: int = 1) -> None:
    """float32 prediction [images, H, W, 4] -> the uint8 map [images, H, W, 3] = trunc(clip(clip((xyz + 1) * 0.5, 0, 1) * 255, 0, 255)) and / or
    the control tensor [rep * images, 3, H, W] (float32 / float16, map / 255) in one launch (ca_nbae_finish)."""
    _req_cuda("ca_nbae_finish", "pred map control", pred, map, control)
    n, h, w, _ = _t("ca_nbae_finish", "pred", pred, torch.float32, (None, None, None, 4))
    dt = _control_args("ca_nbae_finish", n, h, w, map, control, rep, map_shape=(n, h, w, 3), map_name="map")
    check(lib().ca_nbae_finish(_p(pred), n, h, w, _p(map), _p(control), int(rep), dt, _stream()), "ca_nbae_finish")


# ---- face detection and alignment (controlanimate_amd/face_align.py; csrc/ca_retinaface.hip) -------------------------------------------------
RFACE_MAX_CAND, RFACE_HEAD_COLS, RFACE_DET_COLS, FACE_ALIGN_SIZE = _capi.CA_RFACE_MAX_CAND, _capi.CA_RFACE_HEAD_COLS, _capi.CA_RFACE_DET_COLS, _capi.CA_FACE_ALIGN_SIZE


_RFACE_HEADS = tuple(f"heads: the level of step {step}" for step in (8, 16, 32))


def rface_stem(frames: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, out: torch.Tensor, bgr: bool = False) -> torch.Tensor:
    """uint8 [images, H, W, 3] -> `out` [images, H/2, W/2, cout]: relu(conv 7x7 stride 2 padding 3 of (byte - (104, 117, 123)) + bias), the zero
    padding in the mean-subtracted image (ca_rface_stem).  w_packed: face_align.pack_stem's, out's dtype [ceil(cout / 16) * 16, 160]."""
    _req_cuda("ca_rface_stem", "frames w_packed bias out", frames, w_packed, bias, out)
    n, h, w = _req_rgb8("ca_rface_stem", "frames", frames)
    cout = out.shape[3]
    _t("ca_rface_stem", "w_packed", w_packed, out.dtype, (-(-cout // 16) * 16, 160))
    _t("ca_rface_stem", "bias", bias, torch.float32, numel=cout, contiguous=False)
    _need(h % 2 == 0 and w % 2 == 0, "ca_rface_stem", "H and W of frames must be even", frames)
    _t("ca_rface_stem", "out", out, None, (n, h // 2, w // 2, cout))
    check(lib().ca_rface_stem(_p(frames), _p(w_packed), _p(bias), _p(out), n, h, w, cout, int(bool(bgr)), dt_code(out.dtype), _stream()), "ca_rface_stem")
    return out


def _nhwc_out(who: str, name: str, x: torch.Tensor, out: Optional[torch.Tensor], ho: int, wo: int) -> torch.Tensor:
    _t(who, name, x, None, _D4)
    return _out(who, "out", out, (x.shape[0], ho, wo, x.shape[3]), x.dtype, x.device)


def maxpool3x3s2(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.max_pool2d(x, 3, 2, 1) of NHWC x (ca_maxpool3x3s2): the padding never wins."""
    _req_cuda("ca_maxpool3x3s2", "x out", x, out)
    n, h, w, c = x.shape
    out = _nhwc_out("ca_maxpool3x3s2", "x", x, out, (h - 1) // 2 + 1, (w - 1) // 2 + 1)
    check(lib().ca_maxpool3x3s2(_p(x), _p(out), n, h, w, c, dt_code(x.dtype), _stream()), "ca_maxpool3x3s2")
    return out


def subsample2(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x[:, ::2, ::2, :] of NHWC x (ca_subsample2)."""
    _req_cuda("ca_subsample2", "x out", x, out)
    n, h, w, c = x.shape
    out = _nhwc_out("ca_subsample2", "x", x, out, (h + 1) // 2, (w + 1) // 2)
    check(lib().ca_subsample2(_p(x), _p(out), n, h, w, c, dt_code(x.dtype), _stream()), "ca_subsample2")
    return out


def add_up2(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a [n, h, w, c] + nearest x2 of b [n, h/2, w/2, c], rounded once (ca_add_up2); out may be a."""
    _req_cuda("ca_add_up2", "a b out", a, b, out)
    n, h, w, c = a.shape
    _t("ca_add_up2", "b", b, a.dtype, (n, h // 2, w // 2, c))
    _need(h % 2 == 0 and w % 2 == 0, "ca_add_up2", "H and W of a must be even", a)
    out = _nhwc_out("ca_add_up2", "a", a, out, h, w)
    check(lib().ca_add_up2(_p(a), _p(b), _p(out), n, h, w, c, dt_code(a.dtype), _stream()), "ca_add_up2")
    return out


def rface_decode_workspace_bytes(images: int, h: int, w: int) -> int:
    n = int(lib().ca_rface_decode_workspace_bytes(images, h, w))
    if n <= 0:
        raise _capi.CAHipError(f"ca_rface_decode_workspace_bytes: images={images} h={h} w={w} is out of range")
    return n


def rface_decode(heads, h: int, w: int, conf: float, nms: float, eye_dist: float, flags: int, ws: torch.Tensor, dets: torch.Tensor, count: torch.Tensor,
                 overflow: torch.Tensor) -> None:
    """The three levels' fp32 head tensors [images, ceil(h / step), ceil(w / step), 32] -> dets fp32 [images, max_faces, 15], count and overflow
    int32 [images] in one launch (ca_rface_decode)."""
    who = "ca_rface_decode"
    _req_cuda(who, "ws dets count overflow heads", ws, dets, count, overflow, *heads)
    n, max_faces = dets.shape[0], dets.shape[1]
    _need(len(heads) == 3, who, "heads must be the three levels' head tensors")
    for name, t, step in zip(_RFACE_HEADS, heads, (8, 16, 32)):
        _t(who, name, t, torch.float32, (n, -(-h // step), -(-w // step), RFACE_HEAD_COLS))
    _need(dets.dtype == torch.float32 and dets.is_contiguous() and dets.shape[2] == RFACE_DET_COLS, who, "dets must be contiguous float32 [images, max_faces, 15]", dets)
    _t(who, "count", count, torch.int32, numel=n, what="int32 tables, contiguous, one entry per image")
    _t(who, "overflow", overflow, torch.int32, numel=n, what="int32 tables, contiguous, one entry per image")
    check(lib().ca_rface_decode(_p(heads[0]), _p(heads[1]), _p(heads[2]), n, h, w, float(conf), float(nms), float(eye_dist), int(flags), max_faces, _p(ws),
                                _ws_bytes(ws), _p(dets), _p(count), _p(overflow), _stream()), "ca_rface_decode")


def face_align(dets: torch.Tensor, count: torch.Tensor, upscale: float, affine: torch.Tensor, inverse: torch.Tensor) -> None:
    """dets, count -> the float64 similarity [images, max_faces, 2, 3] onto the 512 x 512 template and its inverse times upscale (ca_face_align)."""
    who = "ca_face_align"
    _req_cuda(who, "dets count", dets, count)
    _req_f64(who, "affine inverse", affine, inverse)
    n, max_faces = dets.shape[0], dets.shape[1]
    _need(dets.dtype == torch.float32 and dets.is_contiguous() and dets.shape[2] == RFACE_DET_COLS, who, "dets must be contiguous float32 [images, max_faces, 15]", dets)
    _t(who, "count", count, torch.int32, numel=n, contiguous=False)
    _t(who, "affine", affine, None, (n, max_faces, 2, 3))
    _t(who, "inverse", inverse, None, (n, max_faces, 2, 3))
    check(lib().ca_face_align(_p(dets), _p(count), n, max_faces, float(upscale), _p(affine), _p(inverse), _stream()), "ca_face_align")


def face_warp(frames: torch.Tensor, affine: torch.Tensor, count: torch.Tensor, faces: torch.Tensor, bgr: bool = False) -> torch.Tensor:
    """cv2.warpAffine(frame, affine, (512, 512)) of every slot in OpenCV's fixed point -> faces uint8 [images * max_faces, 512, 512, 3]; a slot
    behind the count is filled with the border value (ca_face_warp)."""
    _req_cuda("ca_face_warp", "frames count faces", frames, count, faces)
    _req_f64("ca_face_warp", "affine", affine)
    n, h, w = _req_rgb8("ca_face_warp", "frames", frames)
    max_faces = affine.shape[1]
    _t("ca_face_warp", "affine", affine, None, (n, max_faces, 2, 3))
    _t("ca_face_warp", "count", count, torch.int32, numel=n, contiguous=False)
    _t("ca_face_warp", "faces", faces, torch.uint8, (n * max_faces, FACE_ALIGN_SIZE, FACE_ALIGN_SIZE, 3))
    check(lib().ca_face_warp(_p(frames), _p(affine), _p(count), _p(faces), n, h, w, max_faces, int(bool(bgr)), _stream()), "ca_face_warp")
    return faces


# ---- the paste-back behind the face restorer (controlanimate_amd/face_paste.py; csrc/ca_facepaste.hip) ---------------------------------------
PARSE_CLASSES, PARSE_CPAD, BLUR_TAPS = _capi.CA_PARSE_CLASSES, _capi.CA_PARSE_CPAD, _capi.CA_BLUR_TAPS
RING_IN, RING_OUT, RING_RES = _capi.CA_RING_IN, _capi.CA_RING_OUT, _capi.CA_RING_RES


def _ringed(shape, ring: bool) -> tuple:
    n, h, w, c = shape
    return (n, h + 2, w + 2, c) if ring else (n, h, w, c)


def parse_prep(faces: torch.Tensor, out: torch.Tensor, reverse: bool = True, ring: bool = False) -> torch.Tensor:
    """uint8 faces [n, S, S, 3] -> `out` [n, S, S, 32] (ringed: [n, S + 2, S + 2, 32], the interior written): ((byte / 255) - 0.5) / 0.5, the
    channels reversed by flag, channels 3 .. 31 zero (ca_parse_prep)."""
    _req_cuda("ca_parse_prep", "faces out", faces, out)
    n, s, s2 = _req_rgb8("ca_parse_prep", "faces", faces)
    _need(s == s2, "ca_parse_prep", "faces must be square", faces)
    _t("ca_parse_prep", "out", out, None, _ringed((n, s, s, PARSE_CPAD), ring))
    check(lib().ca_parse_prep(_p(faces), _p(out), n, s, int(bool(reverse)), int(bool(ring)), dt_code(out.dtype), _stream()), "ca_parse_prep")
    return out


def conv3x3_reflect(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, *, stride: int = 1, up2: bool = False, leaky: bool = False,
                    residual: Optional[torch.Tensor] = None, out_f32: bool = False, out: Optional[torch.Tensor] = None, in_ring: bool = False,
                    out_ring: bool = False, res_ring: bool = False) -> torch.Tensor:
    """act(Conv2d(k 3, stride)(ReflectionPad2d(1)(u)) + bias + residual) of NHWC x [n, H, W, Cin], u = x or (up2) its nearest x2; w
    [Cout, 3, 3, Cin]; act = LeakyReLU(0.2) when leaky (ca_conv3x3_reflect).  in_ring / out_ring / res_ring: that operand is a ringed
    tensor [n, H + 2, W + 2, C] whose interior is read / written."""
    _req_cuda("ca_conv3x3_reflect", "x w bias residual out", x, w, bias, residual, out)
    n, h, wd, cin = _t("ca_conv3x3_reflect", "x", x, None, _D4)
    if in_ring:
        h, wd = h - 2, wd - 2
    cout = _t("ca_conv3x3_reflect", "w", w, x.dtype, (None, 3, 3, cin))[0]
    _t("ca_conv3x3_reflect", "bias", bias, torch.float32, numel=cout, contiguous=False)
    lh, lw = (2 * h, 2 * wd) if up2 else (h, wd)
    gh, gw = (lh - 1) // stride + 1, (lw - 1) // stride + 1
    if residual is not None:
        _t("ca_conv3x3_reflect", "residual", residual, x.dtype, _ringed((n, gh, gw, cout), res_ring))
    out = _out("ca_conv3x3_reflect", "out", out, _ringed((n, gh, gw, cout), out_ring), torch.float32 if out_f32 else x.dtype, x.device)
    rings = (RING_IN if in_ring else 0) | (RING_OUT if out_ring else 0) | (RING_RES if res_ring and residual is not None else 0)
    check(lib().ca_conv3x3_reflect(_p(x), _p(w), _p(bias), _p(residual), _p(out), n, h, wd, cin, cout, int(stride), int(bool(up2)), int(bool(leaky)),
                                   int(bool(out_f32)), rings, dt_code(x.dtype), _stream()), "ca_conv3x3_reflect")
    return out


def ring_fill(x: torch.Tensor, mode: str = "reflect") -> torch.Tensor:
    """Writes the one-pixel ring of x [n, H + 2, W + 2, C] from its interior, in place: 'reflect' (ReflectionPad2d(1)) or 'replicate'
    (ca_ring_fill)."""
    _req_cuda("ca_ring_fill", "x", x)
    n, h, w, c = _t("ca_ring_fill", "x", x, None, _D4)
    _need(mode in ("reflect", "replicate"), "ca_ring_fill", "mode must be 'reflect' or 'replicate'")
    check(lib().ca_ring_fill(_p(x), n, h - 2, w - 2, c, _capi.CA_RING_REFLECT if mode == "reflect" else _capi.CA_RING_REPLICATE, dt_code(x.dtype), _stream()),
          "ca_ring_fill")
    return x


def parse_mask(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, mask: torch.Tensor, in_ring: bool = False) -> torch.Tensor:
    """ParseNet's last layer in one launch: the reflected convolution of x [n, H, W, Cin] with w [32, 3, 3, Cin] (19 rows used), the
    first-maximum argmax and the colour map -> mask uint8 [n, H, W] of 0 / 255 (ca_parse_mask)."""
    _req_cuda("ca_parse_mask", "x w bias mask", x, w, bias, mask)
    n, h, wd, cin = _t("ca_parse_mask", "x", x, None, _D4)
    if in_ring:
        h, wd = h - 2, wd - 2
    _t("ca_parse_mask", "w", w, x.dtype, (PARSE_CPAD, 3, 3, cin))
    _t("ca_parse_mask", "bias", bias, torch.float32, numel=PARSE_CPAD, contiguous=False)
    _t("ca_parse_mask", "mask", mask, torch.uint8, (n, h, wd))
    check(lib().ca_parse_mask(_p(x), _p(w), _p(bias), _p(mask), n, h, wd, cin, PARSE_CLASSES, int(bool(in_ring)), dt_code(x.dtype), _stream()), "ca_parse_mask")
    return mask


def parse_labels(logits: torch.Tensor, labels: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None) -> None:
    """fp32 logits [.., cols] -> labels uint8 [..] (the first maximum over the 19 classes) and / or the 0 / 255 mask uint8 [..] (ca_parse_labels)."""
    _req_cuda("ca_parse_labels", "logits labels mask", logits, labels, mask)
    _t("ca_parse_labels", "logits", logits, torch.float32)
    pixels = logits.numel() // logits.shape[-1]
    for name, t in (("labels", labels), ("mask", mask)):
        if t is not None:
            _t("ca_parse_labels", name, t, torch.uint8, numel=pixels)
    check(lib().ca_parse_labels(_p(logits), _p(labels), _p(mask), pixels, logits.shape[-1], PARSE_CLASSES, _stream()), "ca_parse_labels")


def mask_blur(mask: torch.Tensor, taps: torch.Tensor, ws: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """uint8 mask [n, 512, 512] -> `out` float64 [n, 512, 512]: two Gaussian blurs (101 taps, sigma 11, reflect-101) in float64, the outer 10
    rows and columns zeroed, / 255 (ca_mask_blur).  taps: float64 [51], the centre tap and the 50 behind it; ws: float64 like out."""
    _req_cuda("ca_mask_blur", "mask", mask)
    _req_f64("ca_mask_blur", "taps ws out", taps, ws, out)
    n, s, _ = mask.shape
    _t("ca_mask_blur", "mask", mask, torch.uint8, (n, s, s))
    _t("ca_mask_blur", "out", out, None, (n, s, s))
    _t("ca_mask_blur", "ws", ws, None, (n, s, s))
    check(lib().ca_mask_blur(_p(mask), _p(taps), _p(ws), _p(out), n, s, taps.numel(), _stream()), "ca_mask_blur")
    return out


def face_paste(background: torch.Tensor, restored: torch.Tensor, masks: torch.Tensor, inverse_affine: torch.Tensor, count: torch.Tensor, out: torch.Tensor,
               upscale: float = 1.0) -> torch.Tensor:
    """The blend of every frame's faces r < count into its background, one launch per window (ca_face_paste): background and out uint8
    [n, H, W, 3], restored uint8 [n * max_faces, 512, 512, 3], masks float64 [n * max_faces, 512, 512], inverse_affine float64
    [n, max_faces, 2, 3] (read only: the 0.5 upscale offset is applied inside), count int32 [n]."""
    who = "ca_face_paste"
    _req_cuda(who, "background restored count out", background, restored, count, out)
    _req_f64(who, "masks inverse_affine", masks, inverse_affine)
    n, h, w = _req_rgb8(who, "background", background)
    max_faces = inverse_affine.shape[1]
    _t(who, "inverse_affine", inverse_affine, None, (n, max_faces, 2, 3))
    _t(who, "count", count, torch.int32, numel=n)
    _t(who, "restored", restored, torch.uint8, (n * max_faces, FACE_ALIGN_SIZE, FACE_ALIGN_SIZE, 3))
    _t(who, "masks", masks, None, (n * max_faces, FACE_ALIGN_SIZE, FACE_ALIGN_SIZE))
    _t(who, "out", out, torch.uint8, (n, h, w, 3))
    check(lib().ca_face_paste(_p(background), _p(restored), _p(masks), _p(inverse_affine), _p(count), _p(out), n, h, w, max_faces, float(upscale), _stream()),
          "ca_face_paste")
    return out
