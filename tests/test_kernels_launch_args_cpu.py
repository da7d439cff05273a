"""CPU: what kernels.py hands to the library, pinned call by call.

Every public wrapper of controlanimate_amd/kernels.py runs here without a GPU against a recording stand-in for the library, and
the record is compared with tests/golden/kernels_launch_args.json.  That file was recorded with this same module at commit
5cf3f56 ("One network pass for the packed-tree models"), the last one whose wrappers validated their operands with `assert`; a
refactor of the front end must hand the library exactly what that commit handed it.

How it runs without a GPU
  * operands are CPU tensors viewed as a torch.Tensor subclass whose `is_cuda` is True, so the device check of kernels.py stays
    live (a plain CPU tensor is still rejected);
  * kernels.lib is replaced by a recorder: an entry that launches work is recorded and answers 0; an entry that only answers a
    question on the host (HOST_QUERIES) goes to the real library, with its arguments and answer recorded too;
  * kernels._stream answers 0, and what a wrapper allocates itself (kernels.torch.empty) comes back as the same subclass.

What a line of the record holds: pointers as `name+byte offset` into the tensors the case made ("alloc" for memory the wrapper
allocated, null for NULL), structs field by field, integers and floats as they are; after the call the shape and dtype of what
the wrapper returned and which input it `is`.  A negative case holds `rejected: <exception type>` or, where the wrapper lets the
operand through on purpose so that the library's own message reaches the caller, the recorded call.

Re-recording (a wrapper was added or deliberately changed): `CA_RECORD_LAUNCH_ARGS=1 python -m pytest
tests/test_kernels_launch_args_cpu.py`, review the diff of the json, commit it.  A refactor records at its parent commit only.
"""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from controlanimate_amd import _capi, kernels as K  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "kernels_launch_args.json")
RECORD_ENV = "CA_RECORD_LAUNCH_ARGS"
HOST_QUERIES = re.compile(r"(_supported|_workspace_bytes|_partials_floats|_row_sums_parts|_plan_name)$|^ca_gemm_wants_finished_stats$|^ca_canny_tile_[hw]$")
# symbols kernels.py calls that cannot run under the stand-in, each with its reason (the issue allows five at the most)
EXCUSED = {}

F16, BF16, F32, F64, I16, I32, I64, U8 = (torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.int16, torch.int32, torch.int64,
                                          torch.uint8)


class Dev(torch.Tensor):
    """A CPU tensor that says it is on the device."""
    is_cuda = property(lambda self: True)


class _Torch:
    """kernels' view of torch: what a wrapper allocates is a device stand-in as well."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def empty(*a, **k):
        return torch.empty(*a, **k).as_subclass(Dev)


class Tensors:
    """The operands of one case, by name: t("x", 1, 4, 8, 16) is an fp16 stand-in; dt= another dtype, nc= non-contiguous (same
    shape), cpu= a plain CPU tensor."""

    def __init__(self):
        self.named = []

    def adopt(self, name, tensor):
        self.named.append((name, tensor))
        return tensor

    def __call__(self, name, *shape, dt=F16, nc=False, cpu=False):
        if nc:
            x = torch.empty(shape[:-1] + (2 * shape[-1],), dtype=dt)[..., ::2]
        else:
            x = torch.empty(shape, dtype=dt)
        return self.adopt(name, x if cpu else x.as_subclass(Dev))

    def f(self, name, *shape, **kw):
        return self(name, *shape, dt=F32, **kw)

    def i(self, name, *shape, **kw):
        return self(name, *shape, dt=I32, **kw)

    def u(self, name, *shape, **kw):
        return self(name, *shape, dt=U8, **kw)

    def d(self, name, *shape, **kw):
        return self(name, *shape, dt=F64, **kw)

    def bufs(self, d):
        return {k: self.adopt(k, v) for k, v in d.items()}

    def ptr(self, p):
        if not p:
            return None
        for name, x in self.named:
            st = x.untyped_storage()
            if st.data_ptr() <= p < st.data_ptr() + max(st.nbytes(), 1):
                return f"{name}+{p - st.data_ptr()}"
        return "alloc"

    def which(self, r):
        for name, x in self.named:
            if r is x:
                return name
        return None


class Recorder:
    def __init__(self, real, tensors):
        self.real, self.t, self.calls = real, tensors, []

    def _value(self, ctype, v):
        t = self.t
        if ctype is C.c_void_p:
            return t.ptr(v.value if isinstance(v, C.c_void_p) else v)
        if ctype is C.c_char_p:
            return "buf"
        if isinstance(ctype, type) and issubclass(ctype, C._Pointer):
            if v is None:
                return None
            target = ctype._type_
            if issubclass(target, C.Structure):
                return self._struct(v._obj)
            return [t.ptr(e) if target is C.c_void_p else e for e in v]
        return v

    def _struct(self, s):
        out = {}
        for name, ctype in s._fields_:
            v = getattr(s, name)
            if ctype is C.c_void_p:
                v = self.t.ptr(v)
            elif issubclass(ctype, C.Array):
                v = [self.t.ptr(e) if ctype._type_ is C.c_void_p else e for e in v]
            out[name] = v
        return out

    def __getattr__(self, sym):
        restype, argtypes = _capi.SYMBOLS[sym]

        def call(*args):
            if len(args) != len(argtypes):
                raise TypeError(f"{sym}: {len(args)} arguments for {len(argtypes)} parameters")
            rec = {"sym": sym, "args": [self._value(ct, v) for ct, v in zip(argtypes, args)]}
            rc = 0
            if HOST_QUERIES.search(sym):
                rc = getattr(self.real, sym)(*args)
                rec["answer"] = rc
                bufs = [a.value.decode() for a in args if isinstance(a, C.Array) and a._type_ is C.c_char]
                if bufs:
                    rec["text"] = bufs
            self.calls.append(rec)
            return rc
        return call


def _describe(r, t):
    if isinstance(r, torch.Tensor):
        return {"shape": list(r.shape), "dtype": str(r.dtype).replace("torch.", ""), "is": t.which(r)}
    if isinstance(r, (tuple, list)):
        return [_describe(e, t) for e in r]
    if isinstance(r, dict):
        return {k: _describe(v, t) for k, v in r.items()}
    return r


_real = None


def real_lib():
    global _real
    if _real is None:
        from controlanimate_amd import _build
        _build.build(verbose=False)
        _real = _capi.lib()
    return _real


def run_case(case):
    """One case under the stand-in -> (lines of the record, the exception or None)."""
    t = Tensors()
    rec = Recorder(real_lib(), t)
    saved = K.lib, K._stream, K.__dict__.get("torch"), K._plan_sink
    K.lib, K._stream, K.torch, K._plan_sink = (lambda: rec), (lambda: 0), _Torch(), ([] if case.sink else None)
    K._gn_wino_declined.clear()
    err = ret = None
    try:
        ret = _describe(case.fn(t), t)
        sink = K._plan_sink
    except Exception as e:  # noqa: BLE001 -- the type is what the record holds
        err = e
    finally:
        K.lib, K._stream, K.torch, K._plan_sink = saved
    lines = [dict(case=case.id, **c) for c in rec.calls]
    if err is not None:
        lines.append({"case": case.id, "rejected": type(err).__name__})
    else:
        lines.append({"case": case.id, "ret": ret, **({"plans": sink} if case.sink else {})})
    return lines, err


class Case:
    def __init__(self, id, fn, entry=None, operand=None, sink=False):
        self.id, self.fn, self.entry, self.operand, self.sink = id, fn, entry, operand, sink


CASES = []


def P(id, fn, sink=False):
    """A call the wrapper accepts."""
    CASES.append(Case(id, fn, sink=sink))


def N(id, entry, operand, fn):
    """A call with one wrong operand: the wrapper rejects it naming `entry` and `operand`, or lets it through to the library."""
    CASES.append(Case("not/" + id, fn, entry, operand))


def _views(t, name, b, n, inner):
    """k | v as column halves of one buffer (perceiver_attn's operands)."""
    buf = t(name, b, n, 2 * inner)
    return buf[..., :inner], buf[..., inner:]


def _sides(t, n, count, h=16, w=16, bad=None):
    return [t.f(f"side{k}", n, (h >> k) + (k == bad), w >> k) for k in range(count)]


COEF = [0.5, 0.25, 0.0, 1.0, 0.0, 1.0, 0.0]

# ---- the diffusion path ---------------------------------------------------------------------------------------------------------------
P("gemm", lambda t: K.gemm(t("a", 16, 16), t("w", 16, 16)), sink=True)
P("gemm/full", lambda t: K.gemm(t("a", 16, 16), t("w", 32, 24), a2=t("a2", 16, 8), bias=t.f("bias", 32), rowbias=t.f("rowbias", 2, 32), rows_per_group=8,
                                 residual=t("residual", 16, 32), alpha=0.5, post_scale=2.0, act=K.ACT_SILU, out=t("out", 16, 32)))
P("gemm/geglu_f32", lambda t: K.gemm(t("a", 16, 16, dt=BF16), t("w", 32, 16, dt=BF16), geglu=True, out_f32=True))
P("gemm/strided", lambda t: K.gemm(t("a", 16, 32)[:, :16], t("w", 16, 16), out=t("out", 16, 32)[:, 16:]))
P("gemm/ln_tensor", lambda t: K.gemm(t("a", 16, 16), t("w", 16, 16), ln=(t.f("st", 16, 2), t.f("cs", 16))))


def _gemm_rowstats(t, m, n, sums=None):
    a = t("a", m, 320)
    s = None if sums is None else (t.f("rs", m, sums, 2), sums)
    return K.gemm(a, t("w", n, 320), ln=(K.RowStats(a, 1e-5, sums=s), t.f("cs", n)))


P("gemm/ln_inline", lambda t: _gemm_rowstats(t, 131072, 960))
P("gemm/ln_pass", lambda t: _gemm_rowstats(t, 16, 16))
P("gemm/ln_sums8", lambda t: _gemm_rowstats(t, 16, 16, sums=8))
P("gemm/ln_sums4", lambda t: _gemm_rowstats(t, 16, 16, sums=4))
P("gemm/row_sums", lambda t: K.row_sums_of(K.gemm(t("a", 8192, 1280), t("w", 1280, 1280), row_sums=True)))
P("gemm/workspace", lambda t: K.gemm(t("a", 2048, 5120), t("w", 1280, 5120)))
P("gemm/w_frag", lambda t: K.gemm(t("a", 16, 320), K.attach_w_frag(t("w", 320, 320))))
P("attach_w_frag/geglu", lambda t: K.attach_w_frag(t("w", 640, 320), geglu=True))
P("attach_w_frag/noop", lambda t: K.attach_w_frag(t("w", 16, 16)))
N("gemm", "ca_gemm", "w", lambda t: K.gemm(t("a", 16, 16), t("w", 16, 24)))
N("gemm/dtype", "ca_gemm", "a", lambda t: K.gemm(t.f("a", 16, 16), t.f("w", 16, 16)))  # dt_code's TypeError
N("attach_w_frag", "ca_pack_w_frag", "w", lambda t: K.attach_w_frag(t("w", 320, 320, cpu=True)))


def _ff(t, full=False, **bad):
    x = t("x", 16384, 320)
    kw = dict(residual=t("residual", 16384, 320), ln_stats=t.f("ln_stats", 16384, 2), w_out_frag=t("w_out_frag", 8), bias_out=t.f("bias_out", 320),
              residual_out=t("residual_out", 16384, 320)) if full else {}
    return K.ff_fused(x, t("w1_frag", 8), t.f("bias1", 8, **bad), t.f("colsum1", 8), t("w2_frag", 1, 1280), t.f("bias2", 8) if full else None, 1e-5, **kw)


P("ff_fused", _ff, sink=True)
P("ff_fused/full", lambda t: _ff(t, True), sink=True)
P("ff_fused/declined", lambda t: K.ff_fused(t("x", 16, 320), t("w1_frag", 8), t.f("bias1", 8), t.f("colsum1", 8), t("w2_frag", 1, 1280), None, 1e-5))
N("ff_fused", "ca_ff_fused", "bias1", lambda t: _ff(t, cpu=True))


def _tattn(t, full=False, **bad):
    kw = dict(w_out_frag=t("w_out_frag", 8), bias_out=t.f("bias_out", 320), residual=t("residual", 16384, 320)) if full else {}
    return K.tattn_fused(t("x", 16384, 320), t("w_frag", 8), t.f("gamma", 320), t.f("bias_pe", 16, 320, **bad), 1, 16, 1024, 8, 1e-5, 0.158, **kw)


P("tattn_fused", _tattn, sink=True)
P("tattn_fused/full", lambda t: _tattn(t, True), sink=True)
N("tattn_fused", "ca_tattn_fused", "bias_pe", lambda t: _tattn(t, cpu=True))

P("xattn_pack_kv", lambda t: K.xattn_pack_kv(t("kv", 77, 640), 1, 77, 77, 0.158))
P("xattn_pack_kv/out", lambda t: K.xattn_pack_kv(t("kv", 2 * 93, 640), 2, 93, 16, 0.158, row_offset=77, out=t("out", 2, 8, _capi.XATTN_KV_FRAG_ELEMS)))
P("xattn_pack_kv/declined", lambda t: K.xattn_pack_kv(t("kv", 40, 640), 1, 40, 40, 0.158))
N("xattn_pack_kv", "ca_xattn_pack_kv", "out", lambda t: K.xattn_pack_kv(t("kv", 77, 640), 1, 77, 77, 0.158, out=t("out", 1, 8, 7679)))


def _xattn(t, full=False, kv_dt=F16):
    kv = t("kv_frag", 1, 8, _capi.XATTN_KV_FRAG_ELEMS, dt=kv_dt)
    kw = dict(w_out_frag=t("w_out_frag", 8), bias_out=t.f("bias_out", 320), residual=t("residual", 16384, 320),
              kv_frag_ip=t("kv_frag_ip", 1, 8, _capi.XATTN_KV_FRAG_ELEMS), nk_ip=4, ip_scale=0.5) if full else {}
    return K.xattn_fused(t("x", 16384, 320), t("wq_frag", 8), t.f("bias", 320) if full else None, kv, 16, 1024, 16, 0, 77, 1e-5, **kw)


P("xattn_fused", _xattn, sink=True)
P("xattn_fused/full", lambda t: _xattn(t, True), sink=True)
N("xattn_fused", "ca_xattn_fused", "kv_frag", lambda t: _xattn(t, kv_dt=BF16))

P("conv3x3", lambda t: K.conv3x3(t("x", 1, 4, 4, 8), t("w", 8, 3, 3, 8)), sink=True)
P("conv3x3/full", lambda t: K.conv3x3(t("x", 1, 4, 4, 8), t("w", 16, 3, 3, 16), x2=t("x2", 1, 4, 4, 8), bias=t.f("bias", 16), rowbias=t.f("rowbias", 1, 16),
                                       rows_per_group=16, residual=t("residual", 1, 4, 4, 16), alpha=0.5, post_scale=2.0, act=K.ACT_SILU, out=t("out", 1, 4, 4, 16)))
P("conv3x3/down", lambda t: K.conv3x3(t("x", 1, 4, 4, 8), t("w", 8, 3, 3, 8), stride=2, pad_asym=True, out_f32=True, split_k=False))
P("conv3x3/up", lambda t: K.conv3x3(t("x", 1, 4, 4, 8, dt=BF16), t("w", 8, 3, 3, 8, dt=BF16), upsample=True))
P("conv3x3/wino", lambda t: K.conv3x3(t("x", 4, 32, 32, 640), t("w", 320, 3, 3, 640), w_wino=t("w_wino", 16, 320, 640)), sink=True)
P("conv3x3/split_k", lambda t: K.conv3x3(t("x", 32, 8, 8, 1280), t("w", 1280, 3, 3, 1280)))
N("conv3x3", "ca_conv3x3", "w", lambda t: K.conv3x3(t("x", 1, 4, 4, 8), t.f("w", 8, 3, 3, 8)))
N("conv3x3/out", "ca_conv3x3", "out", lambda t: K.conv3x3(t("x", 1, 4, 4, 8), t("w", 8, 3, 3, 8), out=t("out", 1, 4, 4, 8, cpu=True)))

P("conv_up2_phase_supported", lambda t: K.conv_up2_phase_supported(t("x", 1, 4, 4, 64), t("w_phase", 4, 320, 2, 2, 64)))
P("conv_up2_phase_supported/full", lambda t: K.conv_up2_phase_supported(t("x", 32, 32, 32, 1280), t("w_phase", 4, 640, 2, 2, 1280), bias=t.f("bias", 640),
                                                                        residual=t("residual", 32, 64, 64, 640), alpha=0.5))
P("conv_up2_phase_supported/no", lambda t: K.conv_up2_phase_supported(t.f("x", 1, 4, 4, 64), t("w_phase", 4, 320, 2, 2, 64)))
P("conv_up2_phase", lambda t: K.conv_up2_phase(t("x", 1, 4, 4, 64), t("w_phase", 4, 320, 2, 2, 64)), sink=True)
P("conv_up2_phase/full", lambda t: K.conv_up2_phase(t("x", 1, 4, 4, 64), t("w_phase", 4, 320, 2, 2, 64), bias=t.f("bias", 320),
                                                    residual=t("residual", 1, 8, 8, 320), alpha=0.5))
N("conv_up2_phase", "ca_conv_up2_phase", "w_phase", lambda t: K.conv_up2_phase(t("x", 1, 4, 4, 64), t("w_phase", 4, 320, 2, 2, 64, nc=True)))


def _gn_wino(t, full=False, **bad):
    kw = dict(bias=t.f("bias", 320), rowbias=t.f("rowbias", 4, 320), rows_per_group=256, residual=t("residual", 4, 16, 16, 320), act=K.ACT_SILU) if full else {}
    x2 = {"x2": t("x2", 4, 16, 16, 640)} if full else {}
    return K.group_norm_conv3x3_wino(t("x", 4, 16, 16, 640 if full else 1280), t.f("gamma", 1280, **bad), t.f("beta", 1280), t("w", 320, 3, 3, 1280),
                                     t("w_wino", 16, 320, 1280), **x2, **kw)


P("group_norm_conv3x3_wino", _gn_wino, sink=True)
P("group_norm_conv3x3_wino/full", lambda t: _gn_wino(t, True))
P("group_norm_conv3x3_wino/declined", lambda t: K.group_norm_conv3x3_wino(t("x", 1, 4, 4, 32), t.f("gamma", 32), t.f("beta", 32), t("w", 32, 3, 3, 32),
                                                                        t("w_wino", 16, 32, 32)))
N("group_norm_conv3x3_wino", "ca_groupnorm", "gamma", lambda t: _gn_wino(t, cpu=True))

P("group_norm", lambda t: K.group_norm(t("x", 2, 4, 4, 32), t.f("gamma", 32), t.f("beta", 32)))
P("group_norm/full", lambda t: K.group_norm(t("x", 2, 4, 4, 32), t.f("gamma", 64), t.f("beta", 64), x2=t("x2", 2, 4, 4, 32), groups=8, frames_per_stat=2, eps=1e-6,
                                             act=K.ACT_SILU))
N("group_norm", "ca_groupnorm", "beta", lambda t: K.group_norm(t("x", 2, 4, 4, 32), t.f("gamma", 32), t("beta", 32)))
P("layer_norm", lambda t: K.layer_norm(t("x", 4, 32), t.f("gamma", 32), t.f("beta", 32)))
P("layer_norm/pos", lambda t: K.layer_norm(t("x", 4, 32), t.f("gamma", 32), t.f("beta", 32), pos=t.f("pos", 2, 32), rows_per_frame=2, frames=2, eps=1e-6))
N("layer_norm", "ca_layernorm", "pos", lambda t: K.layer_norm(t("x", 4, 32), t.f("gamma", 32), t.f("beta", 32), pos=t.f("pos", 3, 32), rows_per_frame=2, frames=2))
P("row_stats", lambda t: K.row_stats(t("x", 4, 32), 1e-6))
N("row_stats", "ca_layernorm", "x", lambda t: K.row_stats(t("x", 4, 32, nc=True)))


def _attn_raw(t, mask_dt=U8):
    q = t("qkv", 8, 96)
    return K.attention_raw(q, q, q, t("o", 8, 32), q_off=0, k_off=32, v_off=64, o_off=0, q_strides=(4 * 96, 0, 96), o_strides=(4 * 32, 0, 32),
                           k_strides=(4 * 96, 0, 96), inner_count=1, kv_inner_count=1, kv_div=1, batches=2, heads=2, head_dim=16, nq=4, nk=4, scale=0.25,
                           out_scale=0.5, accumulate=True, kv_mod=1, key_mask=t("key_mask", 2, 4, dt=mask_dt))


P("attention_raw", _attn_raw, sink=True)
N("attention_raw", "ca_attention", "key_mask", lambda t: _attn_raw(t, mask_dt=I32))
P("attention_spatial", lambda t: K.attention_spatial(t("qkv", 8, 96), 2, 4, 2))
P("attention_spatial/mask", lambda t: K.attention_spatial(t("qkv", 8, 96), 2, 4, 2, causal=True, key_mask=t.u("key_mask", 2, 4)))
N("attention_spatial", "ca_attention", "qkv", lambda t: K.attention_spatial(t("qkv", 8, 96, cpu=True), 2, 4, 2))
P("attention_cross", lambda t: K.attention_cross(t("q", 8, 32), t("kv", 6, 64), 2, 4, 2, 3, 3, 1))
P("attention_cross/full", lambda t: K.attention_cross(t("q", 8, 32), t("kv", 10, 64), 2, 4, 2, 3, 5, 1, out=t("out", 8, 32), out_scale=0.5, accumulate=True,
                                                       kv_row_offset=2, kv_mod=1, key_mask=t.u("key_mask", 2, 3)))
N("attention_cross", "ca_attention", "kv", lambda t: K.attention_cross(t("q", 8, 32), t("kv", 6, 64, cpu=True), 2, 4, 2, 3, 3, 1))
P("attention_temporal", lambda t: K.attention_temporal(t("qkv", 16, 96), 1, 4, 4, 2))
N("attention_temporal", "ca_attention", "qkv", lambda t: K.attention_temporal(t("qkv", 16, 96, cpu=True), 1, 4, 4, 2))


def _perceiver(t, out=None):
    return K.perceiver_attn(t("q", 1, 4, 128), *_views(t, "x", 1, 6, 128), *_views(t, "l", 1, 4, 128), 2, out=out)


P("perceiver_attn", _perceiver, sink=True)
P("perceiver_attn/out", lambda t: _perceiver(t, t("out", 1, 4, 256)[..., 128:]))
N("perceiver_attn", "ca_perceiver_attn", "out", lambda t: _perceiver(t, t("out", 1, 4, 64)))

P("add_bcast", lambda t: K.add_bcast(t("a", 4, 8), t("b", 8)))
P("add_bcast/out", lambda t: K.add_bcast(t("a", 4, 8), t("b", 8), out=t("out", 4, 8)))
N("add_bcast", "ca_add_bcast", "b", lambda t: K.add_bcast(t("a", 4, 8), t("b", 8, dt=BF16)))
P("repeat_batch", lambda t: K.repeat_batch(t("x", 2, 8)))
P("repeat_batch/strided", lambda t: K.repeat_batch(t("x", 2, 8, nc=True), times=3))
P("repeat_batch/empty", lambda t: K.repeat_batch(t("x", 0, 8)))
N("repeat_batch", "ca_repeat", "x", lambda t: K.repeat_batch(t("x", 2, 8, cpu=True)))
P("softmax_rows", lambda t: K.softmax_rows(t.f("x", 4, 16)[:, :8], F16, 0.5))
N("softmax_rows", "ca_softmax_rows", "x", lambda t: K.softmax_rows(t("x", 4, 8), F16))
P("silu_f32", lambda t: K.silu_f32(t.f("x", 4, 8)))
N("silu_f32", "ca_silu_f32", "x", lambda t: K.silu_f32(t.f("x", 4, 8, nc=True)))
P("timestep_embedding", lambda t: K.timestep_embedding(7, 2, 32, F16, "cpu"))
P("timestep_embedding/tensor", lambda t: K.timestep_embedding(t.f("t", 2), 2, 32, BF16, "cpu"))
N("timestep_embedding", "ca_timestep_embedding", "t", lambda t: K.timestep_embedding(t.f("t", 3), 2, 32, F16, "cpu"))
P("latents_to_nhwc", lambda t: K.latents_to_nhwc(t.f("latents", 1, 4, 2, 4, 4), 8, 1, 0.5, F16))
P("latents_to_nhwc/out", lambda t: K.latents_to_nhwc(t.f("latents", 1, 4, 2, 4, 4), 8, 2, 1.0, BF16, out=t("out", 4, 4, 4, 8, dt=BF16)))
N("latents_to_nhwc", "ca_latents_to_nhwc", "out", lambda t: K.latents_to_nhwc(t.f("latents", 1, 4, 2, 4, 4), 8, 2, 1.0, F16, out=t("out", 2, 4, 4, 8)))
P("nhwc_to_ncfhw_f32", lambda t: K.nhwc_to_ncfhw_f32(t("x", 2, 4, 4, 8), 1, 4, 2))
P("nhwc_to_ncfhw_f32/f32", lambda t: K.nhwc_to_ncfhw_f32(t.f("x", 2, 4, 4, 8), 1, 4, 2))
N("nhwc_to_ncfhw_f32", "ca_nhwc_to_ncfhw_f32", "x", lambda t: K.nhwc_to_ncfhw_f32(t("x", 2, 16, 8), 1, 4, 2))
P("ncfhw_to_nhwc", lambda t: K.ncfhw_to_nhwc(t.f("x", 1, 4, 2, 4, 4), 8, F16))
P("ncfhw_to_nhwc/strided", lambda t: K.ncfhw_to_nhwc(t("x", 1, 4, 2, 4, 4, nc=True), 8, BF16))
N("ncfhw_to_nhwc", "ca_ncfhw_to_nhwc", "x", lambda t: K.ncfhw_to_nhwc(t.i("x", 1, 4, 2, 4, 4), 8, F16))
P("cfg_scheduler_step", lambda t: K.cfg_scheduler_step(t.f("eps", 4, 4, 4, 8), 2, 7.5, t.f("latents", 1, 4, 2, 4, 4), None, COEF))
P("cfg_scheduler_step/full", lambda t: K.cfg_scheduler_step(t.f("eps", 2, 4, 4, 8), 1, 7.5, t.f("latents", 1, 4, 2, 4, 4), t.f("noise", 1, 4, 2, 4, 4), COEF, clip=1.0,
                                                             want_denoised=True))
N("cfg_scheduler_step", "ca_cfg_scheduler_step", "noise", lambda t: K.cfg_scheduler_step(t.f("eps", 4, 4, 4, 8), 2, 7.5, t.f("latents", 1, 4, 2, 4, 4),
                                                                                         t.f("noise", 1, 4, 2, 4, 2), COEF))
P("lincomb", lambda t: K.lincomb([(t.f("x0", 4, 8), 0.5), (t.f("x1", 4, 8), 2.0)]))
P("lincomb/out", lambda t: K.lincomb([(t.f("x0", 4, 8), 1.0)], out=t.f("out", 4, 8)))
N("lincomb", "ca_lincomb", "terms", lambda t: K.lincomb([(t.f("x0", 4, 8), 0.5), (t("x1", 4, 8), 2.0)]))
P("cfg_combined_eps", lambda t: K.cfg_combined_eps(t.f("eps", 4, 4, 4, 8), 2, 7.5, t.f("latents", 1, 4, 2, 4, 4)))
N("cfg_combined_eps", "ca_cfg_scheduler_step", "latents", lambda t: K.cfg_combined_eps(t.f("eps", 4, 4, 4, 8), 2, 7.5, t.f("latents", 1, 4, 2, 4, 4, cpu=True)))

# ---- the upscaler and the colour match ------------------------------------------------------------------------------------------------
P("conv3x3_narrow", lambda t: K.conv3x3_narrow(t("x", 1, 4, 4, 32), t("w", 16, 3, 3, 32), t("y", 1, 4, 4, 16), cin=32, cout=16), sink=True)
P("conv3x3_narrow/full", lambda t: K.conv3x3_narrow(t("x", 1, 4, 4, 32), t("w", 16, 3, 3, 32), t("y", 1, 8, 8, 32), cin=24, cout=12, bias=t.f("bias", 12),
                                                    channel_offset=16, upsample=True, leaky_relu=True, s0=0.2, r1=t("r1", 1, 8, 8, 16), s1=0.5,
                                                    r2=t("r2", 1, 8, 8, 32), s2=1.0))
P("conv3x3_narrow/u8", lambda t: K.conv3x3_narrow(t("x", 1, 4, 4, 32), t("w", 16, 3, 3, 32), t.u("y", 1, 4, 4, 3), cin=32, cout=3, out_u8=True))
N("conv3x3_narrow", "ca_conv3x3_narrow", "y", lambda t: K.conv3x3_narrow(t("x", 1, 4, 4, 32), t("w", 16, 3, 3, 32), t("y", 1, 3, 4, 16), cin=32, cout=16))
P("rgb8_to_nhwc", lambda t: K.rgb8_to_nhwc(t.u("frames", 1, 4, 4, 3), F16))
N("rgb8_to_nhwc", "ca_rgb8_to_nhwc", "frames", lambda t: K.rgb8_to_nhwc(t("frames", 1, 4, 4, 3), F16))


def _lanczos(t, **out):
    return K.resize_lanczos4_u8(t.u("frames", 1, 4, 4, 3), 8, 8, t.i("xofs", 8), t("alpha", 64, dt=I16), t.i("yofs", 8), t("beta", 64, dt=I16), **out)


P("resize_lanczos4_u8", _lanczos)
P("resize_lanczos4_u8/out", lambda t: _lanczos(t, out=t.u("out", 1, 8, 8, 3)))
N("resize_lanczos4_u8", "ca_resize_lanczos4_u8", "out", lambda t: _lanczos(t, out=t.u("out", 1, 8, 8, 3, cpu=True)))
P("color_match_workspace_bytes", lambda t: K.color_match_workspace_bytes(1, 16))
N("color_match_workspace_bytes", "ca_color_match_workspace_bytes", "images", lambda t: K.color_match_workspace_bytes(0, 0))
P("hist_u8x3", lambda t: K.hist_u8x3(t.u("frames", 1, 16, 3), t.i("hist", 1, 3, 256)))
N("hist_u8x3", "ca_hist_u8x3", "hist", lambda t: K.hist_u8x3(t.u("frames", 1, 16, 3), t.i("hist", 1, 3, 128)))
P("color_moments_f64", lambda t: K.color_moments_f64(t.u("frames", 1, 16, 3), t.d("lut", 1, 3, 256), t.d("mean", 1, 3), t.d("moments", 1, 6), t.f("ws", 16)))
N("color_moments_f64", "ca_color_moments_f64", "lut", lambda t: K.color_moments_f64(t.u("frames", 1, 16, 3), t.f("lut", 1, 3, 256), t.d("mean", 1, 3),
                                                                                    t.d("moments", 1, 6), t.f("ws", 16)))
P("color_transform_f64", lambda t: K.color_transform_f64(t.u("frames", 1, 16, 3), t.d("lut", 1, 3, 256), t.d("mean", 1, 3), t.d("t", 1, 3, 3), t.d("my", 3),
                                                         t.d("y", 1, 3, 16)))
N("color_transform_f64", "ca_color_transform_f64", "y", lambda t: K.color_transform_f64(t.u("frames", 1, 16, 3), t.d("lut", 1, 3, 256), t.d("mean", 1, 3), t.d("t", 1, 3, 3),
                                                                                        t.d("my", 3), t.d("y", 1, 3, 16, nc=True)))
P("sort_f64_segments", lambda t: K.sort_f64_segments(t.d("keys", 2, 16), t.d("out", 2, 16), t.u("ws", 64)))
P("sort_f64_segments/in_place", lambda t: (lambda k: K.sort_f64_segments(k, k, t.u("ws", 64)))(t.d("keys", 2, 16)))
N("sort_f64_segments", "ca_sort_f64_segments", "ws", lambda t: K.sort_f64_segments(t.d("keys", 2, 16), t.d("out", 2, 16), t.u("ws", 64, cpu=True)))


def _rank_map(t, n_dt=I32):
    y = t.d("y", 1, 3, 16)
    return K.color_rank_map_f64(y, t.d("srt", 1, 3, 16), y, t.d("knots_q", 3, 256), t.d("knots_val", 3, 256), t("knots_n", 3, dt=n_dt), t.f("ws", 16))


P("color_rank_map_f64", _rank_map)
N("color_rank_map_f64", "ca_color_rank_map_f64", "knots_n", lambda t: _rank_map(t, I64))
P("color_finish_u8", lambda t: K.color_finish_u8(t.d("o", 1, 3, 16), t.u("out", 1, 16, 3), True, t.f("ws", 16)))
N("color_finish_u8", "ca_color_finish_u8", "out", lambda t: K.color_finish_u8(t.d("o", 1, 3, 16), t.u("out", 1, 15, 3), True, t.f("ws", 16)))

# ---- canny, HED, lineart, lineart_anime ----------------------------------------------------------------------------------------------
P("canny_workspace_bytes", lambda t: K.canny_workspace_bytes(1, 16, 64))
N("canny_workspace_bytes", "ca_canny_workspace_bytes", "images", lambda t: K.canny_workspace_bytes(0, 0, 0))
P("canny_classify", lambda t: K.canny_classify(t.u("frames", 1, 16, 64, 3), 100, 200, t.u("ws", 4096)))
N("canny_classify", "ca_canny_classify", "frames", lambda t: K.canny_classify(t("frames", 1, 16, 64, 3), 100, 200, t.u("ws", 4096)))
P("canny_link", lambda t: K.canny_link(1, 16, 64, t.u("ws", 4096)))
N("canny_link", "ca_canny_link", "ws", lambda t: K.canny_link(1, 16, 64, t.u("ws", 4096, cpu=True)))
P("canny_link_stage", lambda t: [K.canny_link_stage(1, 16, 64, t.u("ws" + s, 4096), s) for s in K.CANNY_LINK_STAGES])
N("canny_link_stage", "ca_canny_link_stage", "ws", lambda t: K.canny_link_stage(1, 16, 64, t.u("ws", 4096, cpu=True), "merge"))
P("canny_emit/edges", lambda t: K.canny_emit(1, 16, 64, t.u("ws", 4096), edges=t.u("edges", 1, 16, 64)))
P("canny_emit/control32", lambda t: K.canny_emit(1, 16, 64, t.u("ws", 4096), control=t.f("control", 2, 3, 16, 64), rep=2))
P("canny_emit/both16", lambda t: K.canny_emit(1, 16, 64, t.u("ws", 4096), edges=t.u("edges", 1, 16, 64), control=t("control", 1, 3, 16, 64)))
N("canny_emit", "ca_canny_emit", "control", lambda t: K.canny_emit(1, 16, 64, t.u("ws", 4096), control=t.d("control", 1, 3, 16, 64)))  # the TypeError
N("canny_emit/shape", "ca_canny_emit", "control", lambda t: K.canny_emit(1, 16, 64, t.u("ws", 4096), control=t.f("control", 1, 3, 16, 64), rep=2))
P("hed_prep", lambda t: K.hed_prep(t.u("frames", 1, 4, 8, 3), t.f("norm", 3), t("out", 1, 4, 8, 8)))
N("hed_prep", "ca_hed_prep", "norm", lambda t: K.hed_prep(t.u("frames", 1, 4, 8, 3), t.f("norm", 3, cpu=True), t("out", 1, 4, 8, 8)))
P("hed_pool_side", lambda t: K.hed_pool_side(t("x", 1, 4, 8, 16), t.f("proj_w", 16), t.f("proj_bias", 1), t.f("side", 1, 4, 8)))
P("hed_pool_side/pooled", lambda t: K.hed_pool_side(t("x", 1, 4, 8, 16), t.f("proj_w", 16), t.f("proj_bias", 1), t.f("side", 1, 4, 8), t("pooled", 1, 2, 4, 16)))
N("hed_pool_side", "ca_hed_pool_side", "side", lambda t: K.hed_pool_side(t("x", 1, 4, 8, 16), t.f("proj_w", 16), t.f("proj_bias", 1), t.f("side", 1, 4, 8, nc=True)))
P("hed_fuse/edges", lambda t: K.hed_fuse(_sides(t, 1, 5), edges=t.u("edges", 1, 16, 16)))
P("hed_fuse/control", lambda t: K.hed_fuse(_sides(t, 1, 5), control=t("control", 2, 3, 16, 16), rep=2))
N("hed_fuse", "ca_hed_fuse", "sides", lambda t: K.hed_fuse(_sides(t, 1, 5, bad=2), edges=t.u("edges", 1, 16, 16)))
P("lineart_conv_in", lambda t: K.lineart_conv_in(t.u("frames", 1, 4, 4, 3), t("w_packed", 64, 160), t("out", 1, 4, 4, 64)))
N("lineart_conv_in", "ca_lineart_conv_in", "w_packed", lambda t: K.lineart_conv_in(t.u("frames", 1, 4, 4, 3), t("w_packed", 64, 160, dt=BF16), t("out", 1, 4, 4, 64)))
P("instance_norm", lambda t: K.instance_norm(t("x", 1, 4, 4, 64)))
P("instance_norm/full", lambda t: K.instance_norm(t("x", 1, 6, 6, 64), relu=True, residual=t("residual", 1, 6, 6, 64), in_ring=True, res_ring=True, out_pad=True,
                                                   eps=1e-6, out=t("out", 1, 6, 6, 64), partials=t.f("partials", 1 << 16)))
N("instance_norm", "ca_instnorm", "out", lambda t: K.instance_norm(t("x", 1, 4, 4, 64), out=t("out", 1, 4, 3, 64)))
P("conv_transpose3x3s2", lambda t: K.conv_transpose3x3s2(t("x", 1, 2, 2, 16), t("w_taps", 3, 3, 16, 16)))
P("conv_transpose3x3s2/given", lambda t: K.conv_transpose3x3s2(t("x", 1, 2, 2, 16), t("w_taps", 3, 3, 16, 16), taps=t("taps", 4, 144), out=t("out", 1, 4, 4, 16)))
N("conv_transpose3x3s2", "ca_convt3x3s2_gather", "w_taps", lambda t: K.conv_transpose3x3s2(t("x", 1, 2, 2, 16), t("w_taps", 3, 3, 16, 8)))
P("lineart_conv_out", lambda t: K.lineart_conv_out(t("x", 1, 4, 4, 64), t.f("wt", 7, 7, 64), t.f("bias", 1), t.f("logits", 1, 4, 4)))
N("lineart_conv_out", "ca_lineart_conv_out", "x", lambda t: K.lineart_conv_out(t("x", 1, 4, 4, 32), t.f("wt", 7, 7, 64), t.f("bias", 1), t.f("logits", 1, 4, 4)))
P("lineart_finish/edges", lambda t: K.lineart_finish(t.f("logits", 1, 4, 4), edges=t.u("edges", 1, 4, 4)))
P("lineart_finish/control", lambda t: K.lineart_finish(t.f("logits", 1, 4, 4), control=t("control", 2, 3, 4, 4), rep=2))
N("lineart_finish", "ca_lineart_finish", "edges", lambda t: K.lineart_finish(t.f("logits", 1, 4, 4), edges=t.u("edges", 1, 4, 3)))
P("lanime_conv_in", lambda t: K.lanime_conv_in(t.u("frames", 1, 4, 4, 3), t("w_packed", 64, 64), t.f("bias", 64), t("l0", 1, 2, 2, 64), t("c0", 1, 2, 2, 128)))
N("lanime_conv_in", "ca_lanime_conv_in", "c0", lambda t: K.lanime_conv_in(t.u("frames", 1, 4, 4, 3), t("w_packed", 64, 64), t.f("bias", 64), t("l0", 1, 2, 2, 64),
                                                                          t("c0", 1, 2, 2, 128, dt=BF16)))
P("conv4x4s2", lambda t: K.conv4x4s2(t("x", 1, 4, 4, 16), t("w", 32, 4, 4, 16)))
P("conv4x4s2/tile", lambda t: K.conv4x4s2(t("x", 1, 4, 4, 16), t("w", 32, 4, 4, 16), bias=t.f("bias", 32), relu=True, out=t("out", 1, 2, 2, 32), form="tile"))
P("conv4x4s2/gemm", lambda t: K.conv4x4s2(t("x", 1, 4, 4, 16), t("w", 32, 4, 4, 16), bias=t.f("bias", 32), relu=True, form="gemm", cols=t("cols", 2048)))
N("conv4x4s2", "ca_conv4x4s2", "bias", lambda t: K.conv4x4s2(t("x", 1, 4, 4, 16), t("w", 32, 4, 4, 16), bias=t.f("bias", 32, nc=True)))
P("conv_transpose4x4s2", lambda t: K.conv_transpose4x4s2(t("x", 1, 2, 2, 16), t("w_phase", 4, 32, 2, 2, 16)))
P("conv_transpose4x4s2/out", lambda t: K.conv_transpose4x4s2(t("x", 1, 2, 2, 16), t("w_phase", 4, 32, 2, 2, 16), out=t("out", 1, 4, 4, 32)))
N("conv_transpose4x4s2", "ca_convt4x4s2", "out", lambda t: K.conv_transpose4x4s2(t("x", 1, 2, 2, 16), t("w_phase", 4, 32, 2, 2, 16), out=t("out", 1, 4, 4, 32, dt=BF16)))
P("instance_norm_act", lambda t: K.instance_norm_act(t("x", 1, 4, 4, 64), [(t("o0", 1, 4, 4, 128), K.IN_ACT_RELU, 64)]))
P("instance_norm_act/two", lambda t: K.instance_norm_act(t("x", 1, 4, 4, 64), [(t("o0", 1, 4, 4, 64), K.IN_ACT_LEAKY, 0), (t("o1", 1, 4, 4, 128), K.IN_ACT_NONE, 64)],
                                                          eps=1e-6, partials=t.f("partials", 1 << 16)))
N("instance_norm_act", "ca_instnorm_act", "outs", lambda t: K.instance_norm_act(t("x", 1, 4, 4, 64), [(t("o0", 1, 4, 2, 128), K.IN_ACT_RELU, 64)]))
P("lanime_conv_out", lambda t: K.lanime_conv_out(t("x", 1, 2, 2, 128), t.f("wt", 4, 4, 128), t.f("bias", 1), t.f("out", 1, 4, 4)))
N("lanime_conv_out", "ca_lanime_conv_out", "wt", lambda t: K.lanime_conv_out(t("x", 1, 2, 2, 128), t.f("wt", 4, 4, 128, cpu=True), t.f("bias", 1), t.f("out", 1, 4, 4)))
P("lanime_finish", lambda t: K.lanime_finish(t.f("pre", 1, 4, 4), edges=t.u("edges", 1, 4, 4), control=t.f("control", 1, 3, 4, 4)))
N("lanime_finish", "ca_lanime_finish", "pre", lambda t: K.lanime_finish(t("pre", 1, 4, 4), edges=t.u("edges", 1, 4, 4)))

# ---- M-LSD and softedge ----------------------------------------------------------------------------------------------------------------
P("mlsd_prep", lambda t: K.mlsd_prep(t.u("frames", 1, 4, 4, 3), t("out", 1, 4, 4, 8)))
N("mlsd_prep", "ca_mlsd_prep", "out", lambda t: K.mlsd_prep(t.u("frames", 1, 4, 4, 3), t("out", 1, 4, 3, 8)))


def _dw3(t, w=(9, 16), **kw):
    return K.dwconv3x3(t("x", 1, 4, 8, 16), t("w", *w), t.f("bias", 16), **kw)


P("dwconv3x3", _dw3)
P("dwconv3x3/s2", lambda t: _dw3(t, stride=2, relu6=True, out=t("out", 1, 2, 4, 16)))
N("dwconv3x3/stride", "ca_dwconv3x3", "stride", lambda t: _dw3(t, stride=3))  # let through: the library names the strides it takes
N("dwconv3x3", "ca_dwconv3x3", "w", lambda t: _dw3(t, w=(8, 16)))
N("dwconv3x3/out", "ca_dwconv3x3", "out", lambda t: _dw3(t, out=t("out", 1, 3, 8, 16)))
P("upsample2x_bilinear_ac", lambda t: K.upsample2x_bilinear_ac(t("x", 1, 2, 2, 8), t("out", 1, 4, 4, 16), col0=8))
N("upsample2x_bilinear_ac", "ca_upsample2x_bilinear_ac", "out", lambda t: K.upsample2x_bilinear_ac(t("x", 1, 2, 2, 8), t("out", 1, 4, 4, 16, dt=BF16)))
P("conv3x3_dil", lambda t: K.conv3x3_dil(t("x", 1, 4, 4, 64), t("w", 64, 3, 3, 64), t.f("bias", 64)))
P("conv3x3_dil/out", lambda t: K.conv3x3_dil(t("x", 1, 4, 4, 64), t("w", 64, 3, 3, 64), t.f("bias", 64), dilation=3, relu=True, out=t("out", 1, 4, 4, 64)))
N("conv3x3_dil", "ca_conv3x3_dil", "w", lambda t: K.conv3x3_dil(t("x", 1, 4, 4, 64), t("w", 64, 3, 3, 32), t.f("bias", 64)))
P("mlsd_decode_workspace_bytes", lambda t: K.mlsd_decode_workspace_bytes(1, 8, 8))
N("mlsd_decode_workspace_bytes", "ca_mlsd_decode_workspace_bytes", "images", lambda t: K.mlsd_decode_workspace_bytes(0, 0, 0))
P("mlsd_decode", lambda t: K.mlsd_decode(t.f("tp", 1, 8, 8, 8)))
P("mlsd_decode/given", lambda t: K.mlsd_decode(t.f("tp", 1, 8, 8, 8), 0.2, 0.3, segments=t.i("segments", 1, 200, 4), count=t.i("count", 1), ws=t.u("ws", 1 << 16)))
N("mlsd_decode", "ca_mlsd_decode", "count", lambda t: K.mlsd_decode(t.f("tp", 1, 8, 8, 8), segments=t.i("segments", 1, 200, 4), count=t.i("count", 2)))
P("mlsd_draw", lambda t: K.mlsd_draw(t.i("segments", 1, 200, 4), t.i("count", 1), 8, 8))
P("mlsd_draw/given", lambda t: K.mlsd_draw(t.i("segments", 1, 200, 4), t.i("count", 1), 8, 8, edges=t.u("edges", 1, 8, 8), control=t("control", 2, 3, 8, 8), rep=2))
N("mlsd_draw", "ca_mlsd_draw", "segments", lambda t: K.mlsd_draw(t.f("segments", 1, 200, 4), t.i("count", 1), 8, 8))
P("softedge_prep", lambda t: K.softedge_prep(t.u("frames", 1, 4, 4, 3), t("out", 1, 4, 4, 8)))
N("softedge_prep", "ca_softedge_prep", "frames", lambda t: K.softedge_prep(t.u("frames", 1, 4, 4, 4), t("out", 1, 4, 4, 8)))
P("relu", lambda t: K.relu(t("x", 4, 8)))
P("relu/in_place", lambda t: (lambda x: K.relu(x, x))(t("x", 4, 8)))
N("relu", "ca_relu", "x", lambda t: K.relu(t("x", 4, 8, nc=True)))
P("dwconv_k", lambda t: K.dwconv_k(t("x", 1, 4, 4, 16), t("w", 9, 16)))
P("dwconv_k/5", lambda t: K.dwconv_k(t("x", 1, 4, 4, 16), t("w", 25, 16), relu=True, out=t("out", 1, 4, 4, 16)))
N("dwconv_k", "ca_dwconv_k", "w", lambda t: K.dwconv_k(t("x", 1, 4, 4, 16), t("w", 10, 16)))
P("maxpool2x2", lambda t: K.maxpool2x2(t("x", 1, 4, 4, 8)))
P("maxpool2x2/out", lambda t: K.maxpool2x2(t("x", 1, 4, 4, 8), t("out", 1, 2, 2, 8)))
N("maxpool2x2/odd", "ca_maxpool2x2", "x", lambda t: K.maxpool2x2(t("x", 1, 3, 4, 8)))  # let through: the library's message says "even"
N("maxpool2x2", "ca_maxpool2x2", "out", lambda t: K.maxpool2x2(t("x", 1, 4, 4, 8), t("out", 1, 2, 2, 8, dt=BF16)))
P("pdc_block_supported", lambda t: [K.pdc_block_supported(64, 3), K.pdc_block_supported(32, 3)])
P("pdc_block", lambda t: K.pdc_block(t("x", 1, 4, 4, 64), t("w_dw", 9, 64), t("w2", 64, 64)))
P("pdc_block/fused", lambda t: K.pdc_block(t("x", 1, 4, 4, 64), t("w_dw", 25, 64), t("w2", 64, 64), out=t("out", 1, 4, 4, 64), fused=True))
P("pdc_block/composed", lambda t: K.pdc_block(t("x", 1, 4, 4, 32), t("w_dw", 9, 32), t("w2", 32, 32), fused=False, tmp=t("tmp", 1, 4, 4, 32)))
N("pdc_block", "ca_pdc_block", "w2", lambda t: K.pdc_block(t("x", 1, 4, 4, 64), t("w_dw", 9, 64), t("w2", 64, 32)))
P("cdcm_dil4", lambda t: K.cdcm_dil4(t("x", 1, 4, 4, 32), t("w", 4, 32, 3, 3, 32)))
P("cdcm_dil4/out", lambda t: K.cdcm_dil4(t("x", 1, 4, 4, 32), t("w", 4, 32, 3, 3, 32), t("out", 1, 4, 4, 32)))
N("cdcm_dil4", "ca_cdcm_dil4", "w", lambda t: K.cdcm_dil4(t("x", 1, 4, 4, 32), t("w", 4, 32, 3, 3, 32, nc=True)))


def _csam(t, **kw):
    return K.csam_reduce(t("f", 1, 4, 4, 32), t.f("w1", 4, 32), t.f("b1", 4), t.f("w2", 3, 3, 4), t.f("wr", 32), t.f("br", 1), **kw)


P("csam_reduce", _csam)
P("csam_reduce/given", lambda t: _csam(t, side=t.f("side", 1, 4, 4), scratch=t.f("scratch", 80)))
N("csam_reduce", "ca_csam_reduce", "scratch", lambda t: _csam(t, scratch=t.f("scratch", 79)))
P("softedge_fuse/edges", lambda t: K.softedge_fuse(_sides(t, 1, 4), t.f("classifier", 5), edges=t.u("edges", 1, 16, 16)))
P("softedge_fuse/full", lambda t: K.softedge_fuse(_sides(t, 1, 4), t.f("classifier", 5), safe=True, logit=t.f("logit", 1, 16, 16), edges=t.u("edges", 1, 16, 16),
                                                   control=t.f("control", 2, 3, 16, 16), rep=2))
N("softedge_fuse", "ca_softedge_fuse", "classifier", lambda t: K.softedge_fuse(_sides(t, 1, 4), t.f("classifier", 5, cpu=True), edges=t.u("edges", 1, 16, 16)))

# ---- GFPGAN and depth ------------------------------------------------------------------------------------------------------------------
P("gfp_prep", lambda t: K.gfp_prep(t.u("faces", 1, 4, 4, 3), t.f("wt", 16, 3), t.f("bias", 16), t("out", 1, 4, 4, 16), reverse_channels=False))
N("gfp_prep", "ca_gfp_prep", "wt", lambda t: K.gfp_prep(t.u("faces", 1, 4, 4, 3), t.f("wt", 16, 4), t.f("bias", 16), t("out", 1, 4, 4, 16)))
P("resample2x/up", lambda t: K.resample2x(t("x", 1, 4, 4, 8), True))
P("resample2x/down", lambda t: K.resample2x(t("x", 1, 4, 4, 8), False, out=t("out", 1, 2, 2, 8)))
N("resample2x", "ca_resample2x", "out", lambda t: K.resample2x(t("x", 1, 4, 4, 8), True, out=t("out", 1, 8, 7, 8)))
P("gfp_styles", lambda t: K.gfp_styles(t.f("latents", 1, 2, 512), t.f("params", 100), [0, 8, 8, 0, 0, 0, 1, 8, 0, 0, 0, 16], t.f("out", 1, 32)))
N("gfp_styles", "ca_gfp_styles", "latents", lambda t: K.gfp_styles(t.f("latents", 1, 2, 256), t.f("params", 100), [0, 8, 8, 0, 0, 0], t.f("out", 1, 32)))


def _modconv(t, n=1, nx=1, up=False, noise_w=4, **kw):
    hw = 8 if up else 4
    return K.modconv3x3(t("x", nx, 4, 4, 16), t("wt", 32, 3, 3, 16), t.f("s", n, 24)[:, :16], t.f("demod", n, 32), t.f("noise", n, hw, noise_w if not up else 8),
                        t.f("bias", 32), 0.5, upsample=up, **kw)


P("modconv3x3", _modconv)
P("modconv3x3/fused", lambda t: _modconv(t, n=2, up=True, images=2, form="fused", sft=(t("scale", 2, 8, 8, 16), t("shift", 2, 8, 8, 16)), out=t("out", 2, 8, 8, 32)))
P("modconv3x3/composed", lambda t: _modconv(t, n=2, nx=2, form="composed", sft=(t("scale", 2, 4, 4, 16), t("shift", 2, 4, 4, 16)), scratch=t("scratch", 2, 4, 4, 16)))
N("modconv3x3", "ca_modconv3x3", "noise", lambda t: _modconv(t, noise_w=3))


def _to_rgb(t, prev_dt=None):
    prev = {} if prev_dt is None else {"prev": t("prev", 1, 2, 2, 3, dt=prev_dt)}
    return K.gfp_to_rgb(t("x", 1, 4, 4, 16), t.f("wt", 3, 16), t.f("s", 1, 16), t.f("bias", 3), t.f("out", 1, 4, 4, 3), **prev)


P("gfp_to_rgb", _to_rgb)
P("gfp_to_rgb/prev", lambda t: _to_rgb(t, F32))
N("gfp_to_rgb", "ca_gfp_to_rgb", "prev", lambda t: _to_rgb(t, F16))
P("gfp_finish", lambda t: K.gfp_finish(t.f("pre", 1, 4, 4, 3), t.u("out", 1, 4, 4, 3)))
N("gfp_finish", "ca_gfp_finish", "out", lambda t: K.gfp_finish(t.f("pre", 1, 4, 4, 3), t.u("out", 1, 4, 4, 3, nc=True)))


def _pil(t, b_dt=I32, **kw):
    return K.resize_pil_u8(t.u("frames", 1, 4, 4, 3), 2, 2, t("xbounds", 2, 2, dt=b_dt), t.i("xcoef", 2, 3), t.i("ybounds", 2, 2), t.i("ycoef", 2, 4), **kw)


P("resize_pil_u8", _pil)
P("resize_pil_u8/given", lambda t: _pil(t, tmp=t.u("tmp", 1, 4, 2, 3), out=t.u("out", 1, 2, 2, 3)))
N("resize_pil_u8", "ca_resize_pil_u8", "xbounds", lambda t: _pil(t, b_dt=I64))
P("dpt_patches", lambda t: K.dpt_patches(t.u("frames", 1, 4, 4, 3), 2, F16))
P("dpt_patches/out", lambda t: K.dpt_patches(t.u("frames", 1, 4, 4, 3), 2, BF16, out=t("out", 4, 12, dt=BF16)))
N("dpt_patches", "ca_dpt_patches", "frames", lambda t: K.dpt_patches(t.u("frames", 1, 4, 6, 3), 2, F16))
P("depth_to_space", lambda t: K.depth_to_space(t("x", 4, 32), 1, 2, 2, 2, 8))
P("depth_to_space/rows", lambda t: K.depth_to_space(t("x", 5, 40)[:, :32], 1, 2, 2, 2, 8, rows_per_image=5, row0=1, out=t("out", 1, 4, 4, 8)))
N("depth_to_space", "ca_depth_to_space", "x", lambda t: K.depth_to_space(t("x", 4, 16), 1, 2, 2, 2, 8))
P("dpt_head_supported", lambda t: [K.dpt_head_supported(32), K.dpt_head_supported(48)])


def _dpt_head(t, b3=1, **kw):
    return K.dpt_head(t("x", 1, 2, 2, 32), t("w2", 32, 3, 3, 32), t.f("b2", 32), t.f("w3", 32), t.f("b3", b3), **kw)


P("dpt_head", _dpt_head)
P("dpt_head/fused", lambda t: _dpt_head(t, fused=True, out=t.f("out", 1, 4, 4)))
P("dpt_head/composed", lambda t: _dpt_head(t, fused=False, up=t("up", 1, 4, 4, 32), mid=t.f("mid", 1, 4, 4, 32)))
N("dpt_head", "ca_dpt_head", "b3", lambda t: _dpt_head(t, b3=2))
P("resize_bicubic_f32", lambda t: K.resize_bicubic_f32(t.f("x", 1, 4, 4), 8, 8))
P("resize_bicubic_f32/given", lambda t: K.resize_bicubic_f32(t.f("x", 1, 4, 4), 8, 8, out=t.f("out", 1, 8, 8), keys=t.i("keys", 1, 2), minmax=t.f("minmax", 1, 2)))
N("resize_bicubic_f32", "ca_resize_bicubic_f32", "keys", lambda t: K.resize_bicubic_f32(t.f("x", 1, 4, 4), 8, 8, keys=t.i("keys", 1)))
P("depth_finish/map", lambda t: K.depth_finish(t.f("depth", 1, 4, 4), t.i("keys", 1, 2), map=t.u("map", 1, 4, 4)))
P("depth_finish/control", lambda t: K.depth_finish(t.f("depth", 1, 4, 4), t.i("keys", 1, 2), "minmax", control=t("control", 2, 3, 4, 4), rep=2))
N("depth_finish", "ca_depth_finish", "keys", lambda t: K.depth_finish(t.f("depth", 1, 4, 4), t.f("keys", 1, 2), map=t.u("map", 1, 4, 4)))

# ---- OpenPose: body, face, hand ----------------------------------------------------------------------------------------------------------


def _area_tables(t, xw_cols=K.POSE_AREA_TAPS):
    return (t.i("xofs", 4), t.i("xcnt", 4), t.f("xw", 4, xw_cols), t.i("yofs", 4), t.i("ycnt", 4), t.f("yw", 4, K.POSE_AREA_TAPS))


P("pose_prep", lambda t: K.pose_prep(t.u("frames", 1, 8, 8, 3), _area_tables(t), 4, 4, t("out", 1, 8, 8, 8)))
N("pose_prep", "ca_pose_prep", "xw", lambda t: K.pose_prep(t.u("frames", 1, 8, 8, 3), _area_tables(t, 4), 4, 4, t("out", 1, 8, 8, 8)))
P("conv7x7", lambda t: K.conv7x7([t("x", 1, 4, 4, 16)], [t("w", 32, 7, 7, 16)]))


def _conv7_two(t, **kw):
    x, y = t("x", 1, 4, 4, 32), t("y", 1, 4, 4, 64)
    return K.conv7x7([x[..., :16], x[..., 16:]], [t("w0", 32, 7, 7, 16), t("w1", 32, 7, 7, 16)], biases=[t.f("b0", 32), None], relu=True,
                     outs=[y[..., :32], y[..., 32:]], **kw)


P("conv7x7/direct", lambda t: _conv7_two(t, direct=True))
P("conv7x7/gemm", lambda t: _conv7_two(t, direct=False, cols=t("cols", 16 * 49 * 16 + 8)))
P("conv7x7/gemm_alloc", lambda t: K.conv7x7([t("x", 1, 4, 4, 16)], [t("w", 32, 7, 7, 16)], direct=False))
N("conv7x7", "ca_conv7x7", "ws_", lambda t: K.conv7x7([t("x", 1, 4, 4, 16)], [t("w", 32, 7, 5, 16)]))
P("copy_cols", lambda t: K.copy_cols(t("src", 4, 8), t("dst", 4, 16), 8))
N("copy_cols", "ca_copy_cols", "dst", lambda t: K.copy_cols(t("src", 4, 8), t("dst", 3, 16), 8))
P("pose_maps_workspace_bytes", lambda t: K.pose_maps_workspace_bytes(1, 4, 8))
N("pose_maps_workspace_bytes", "ca_pose_maps_workspace_bytes", "images", lambda t: K.pose_maps_workspace_bytes(0, 0, 0))


def _pose_maps(t, paf_c=38, **kw):
    return K.pose_maps(t.f("low", 1, 4, 4, 64), t.f("mx", 2, 8, 4), t.f("my", 2, 8, 4), t.f("raw", 1, 18, 8, 8), t.f("smooth", 1, 18, 8, 8),
                       t.f("paf", 1, paf_c, 8, 8), **kw)


P("pose_maps", _pose_maps)
P("pose_maps/ws", lambda t: _pose_maps(t, ws=t.u("ws", 1 << 16)))
N("pose_maps", "ca_pose_maps", "paf", lambda t: _pose_maps(t, paf_c=37))


def _pose_decode(t, smooth_dt=F32, **kw):
    return K.pose_decode(t.f("raw", 1, 18, 8, 8), t("smooth", 1, 18, 8, 8, dt=smooth_dt), t.f("paf", 1, 38, 8, 8), **kw)


P("pose_decode", _pose_decode)
P("pose_decode/buf", lambda t: _pose_decode(t, buf=t.bufs(K.pose_decode_buffers(1, "cpu")), stage=lambda name: None))
N("pose_decode", "ca_pose_peaks", "smooth", lambda t: _pose_decode(t, smooth_dt=F16))
P("pose_assemble", lambda t: K.pose_assemble(t.bufs(K.pose_decode_buffers(2, "cpu")), 8, 8))


def _draw_common(t, sin=451):
    return t.i("coords", 1, 64, 18, 2), t.i("people", 1), t.f("sin_table", sin)


def _draw_outs(t):
    return dict(index=t.i("index", 1, 8, 8), skeleton=t.u("skeleton", 1, 8, 8, 3), control=t("control", 2, 3, 8, 8), rep=2)


P("pose_draw", lambda t: K.pose_draw(*_draw_common(t), 8, 8))
P("pose_draw/given", lambda t: K.pose_draw(*_draw_common(t), 8, 8, **_draw_outs(t)))
P("pose_draw/control", lambda t: K.pose_draw(*_draw_common(t), 8, 8, control=t.f("control", 1, 3, 8, 8)))
N("pose_draw", "ca_pose_draw", "sin_table", lambda t: K.pose_draw(*_draw_common(t, 450), 8, 8))
P("face_boxes", lambda t: K.face_boxes(t.i("keypoints", 1, 64, 18, 2), t.i("people", 1), 8, 8, t.bufs(K.face_buffers(1, 2, "cpu"))))
P("face_boxes/overflow", lambda t: K.face_boxes(t.i("keypoints", 1, 64, 18, 2), t.i("people", 1), 8, 8, t.bufs(K.face_buffers(1, 2, "cpu")), t.i("overflow_in", 1)))


def _face_bufs_bad(t):
    b = t.bufs(K.face_buffers(1, 2, "cpu"))
    b["slots"] = t.f("slots_f32", 1, 2, 8)
    return b


N("face_boxes", "ca_face_boxes", "slots", lambda t: K.face_boxes(t.i("keypoints", 1, 64, 18, 2), t.i("people", 1), 8, 8, _face_bufs_bad(t)))


def _face_tables(t, coef_dt=I16):
    return {"lz_ofs": t.i("lz_ofs", 374, 384), "lz_coef": t("lz_coef", 374, 384, 8, dt=coef_dt), "ar_ofs": t.i("ar_ofs", 1, 384), "ar_cnt": t.i("ar_cnt", 1, 384),
            "ar_w": t.f("ar_w", 1, 384, 8), "side_max": 384}


P("face_crop", lambda t: K.face_crop(t.u("frames", 1, 8, 8, 3), t.i("slots", 1, 2, 8), _face_tables(t), t("out", 1, 384, 384, 8), first=1))
N("face_crop", "ca_face_crop", "lz_coef", lambda t: K.face_crop(t.u("frames", 1, 8, 8, 3), t.i("slots", 1, 2, 8), _face_tables(t, I32), t("out", 1, 384, 384, 8)))
P("face_peaks", lambda t: K.face_peaks(t.f("heat", 2, 48, 48, 72), t.i("slots", 1, 2, 8), t.i("points", 1, 64, 71, 2), 8, 8))
N("face_peaks", "ca_face_peaks", "heat", lambda t: K.face_peaks(t.f("heat", 1, 48, 48, 72), t.i("slots", 1, 2, 8), t.i("points", 1, 64, 71, 2), 8, 8))
P("pose_draw_faces/bodies", lambda t: K.pose_draw_faces(*_draw_common(t), None, None, None, 8, 8))
P("pose_draw_faces", lambda t: K.pose_draw_faces(*_draw_common(t), t.i("points", 1, 64, 71, 2), t.i("xmap", 8), t.i("ymap", 8), 8, 8, **_draw_outs(t)))
N("pose_draw_faces", "ca_pose_draw_faces", "xmap", lambda t: K.pose_draw_faces(*_draw_common(t), t.i("points", 1, 64, 71, 2), t.i("xmap", 7), t.i("ymap", 8), 8, 8))
P("hand_boxes", lambda t: K.hand_boxes(t.i("keypoints", 1, 64, 18, 2), t.i("people", 1), 8, 8, t.bufs(K.hand_buffers(1, 2, "cpu"))))
P("hand_boxes/overflow", lambda t: K.hand_boxes(t.i("keypoints", 1, 64, 18, 2), t.i("people", 1), 8, 8, t.bufs(K.hand_buffers(1, 2, "cpu")), t.i("overflow_in", 1)))
N("hand_boxes", "ca_hand_boxes", "people", lambda t: K.hand_boxes(t.i("keypoints", 2, 64, 18, 2), t.i("people", 2, nc=True), 8, 8, t.bufs(K.hand_buffers(2, 2, "cpu"))))


def _hand_crop(t, side, blurred=32, **kw):
    nl, na = min(side, 32) - 20 + 1, max(32 - side, 0)
    tables = {"taps": t.d("taps", 7), "lz_ofs": t.i("lz_ofs", nl, side), "lz_coef": t("lz_coef", nl, side, 8, dt=I16)}
    if na:
        tables.update(ar_ofs=t.i("ar_ofs", na, side), ar_cnt=t.i("ar_cnt", na, side), ar_w=t.f("ar_w", na, side, 16))
    return K.hand_crop(t.u("frames", 1, 32, 32, 3), t.i("slots", 1, 2, 8), tables, t.u("blurred", 2, blurred, 32, 3), t("out", 2, side, side, 8), **kw)


P("hand_crop", lambda t: _hand_crop(t, 24))
P("hand_crop/no_area", lambda t: _hand_crop(t, 32, first=1, blur=False))
N("hand_crop", "ca_hand_crop", "blurred", lambda t: _hand_crop(t, 24, blurred=31))


def _hand_maps(t, bad=None):
    heats = [t.f(f"heat{m}", 1, m, m + (m == bad), 24) for m in K.HAND_MAP_SIDES]
    return K.hand_maps(heats, t.f("mats", 2, 230, 128), t.f("raw", 1, 21, 128, 128), t.f("smooth", 1, 21, 128, 128))


P("hand_maps", _hand_maps)
N("hand_maps", "ca_hand_maps", "heats", lambda t: _hand_maps(t, bad=46))


def _hand_peaks(t, mass_dt=F64):
    b = t.bufs(K.hand_buffers(1, 2, "cpu"))
    b["mass"] = t("mass_", 2, 21, dt=mass_dt)
    return K.hand_peaks(t.f("raw", 2, 21, 128, 128), t.f("smooth", 2, 21, 128, 128), b, 8, 8)


P("hand_peaks", _hand_peaks)
N("hand_peaks", "ca_hand_peaks", "mass", lambda t: _hand_peaks(t, F32))


def _draw_hands(t, hands=64, face=True, **kw):
    return K.pose_draw_hands(*_draw_common(t), t.i("hand_points", 1, hands, 2, 21, 2), t.i("face_points", 1, 64, 71, 2) if face else None, t.i("xmap", 8), t.i("ymap", 8),
                             8, 8, **kw)


P("pose_draw_hands", lambda t: _draw_hands(t, face=False))
P("pose_draw_hands/given", lambda t: _draw_hands(t, **_draw_outs(t)))
N("pose_draw_hands", "ca_pose_draw_hands", "hand_points", lambda t: _draw_hands(t, hands=63))

# ---- NormalBae, face detection, paste-back ------------------------------------------------------------------------------------------------
P("nbae_stem", lambda t: K.nbae_stem(t.u("frames", 1, 4, 4, 3), t.f("wt", 27, 16), t.f("bias", 16), t("out", 1, 2, 2, 16)))
N("nbae_stem", "ca_nbae_stem", "wt", lambda t: K.nbae_stem(t.u("frames", 1, 4, 4, 3), t.f("wt", 9, 16), t.f("bias", 16), t("out", 1, 2, 2, 16)))
P("dwconv_same_partials_floats", lambda t: K.dwconv_same_partials_floats(1, 4, 4, 16, 1))
N("dwconv_same_partials_floats", "ca_dwconv_same_partials_floats", "images", lambda t: K.dwconv_same_partials_floats(0, 0, 0, 0, 1))
P("dwconv_same", lambda t: K.dwconv_same(t("x", 1, 4, 4, 16), t("w", 9, 16), t.f("bias", 16)))
P("dwconv_same/given", lambda t: K.dwconv_same(t("x", 1, 5, 5, 16), t("w", 25, 16), t.f("bias", 16), stride=2, out=t("out", 1, 3, 3, 16), sums=t.f("sums", 1, 16),
                                                partials=t.f("partials", 1 << 16)))
N("dwconv_same", "ca_dwconv_same", "w", lambda t: K.dwconv_same(t("x", 1, 4, 4, 16), t("w", 9, 8), t.f("bias", 16)))


def _se_gate(t, c_out=16, **kw):
    return K.se_gate(t.f("sums", 1, 16), t.f("w_reduce", 4, 16), t.f("b_reduce", 4), t.f("w_expand_t", 4, 16), t.f("b_expand", c_out), 16, **kw)


P("se_gate", _se_gate)
P("se_gate/out", lambda t: _se_gate(t, out=t.f("out", 1, 16)))
N("se_gate", "ca_se_gate", "b_expand", lambda t: _se_gate(t, c_out=8))
P("scale_channels", lambda t: K.scale_channels(t("x", 1, 4, 4, 16), t.f("gate", 1, 16)))
P("scale_channels/in_place", lambda t: (lambda x: K.scale_channels(x, t.f("gate", 1, 16), x))(t("x", 1, 4, 4, 16)))
N("scale_channels", "ca_scale_channels", "gate", lambda t: K.scale_channels(t("x", 1, 4, 4, 16), t("gate", 1, 16)))
P("nbae_cat_pred", lambda t: K.nbae_cat_pred(t.f("pred", 1, 2, 2, 4), t("out", 1, 4, 4, 16), col0=8))
N("nbae_cat_pred", "ca_nbae_cat_pred", "out", lambda t: K.nbae_cat_pred(t.f("pred", 1, 2, 2, 4), t("out", 4, 4, 16)))
P("nbae_normalize", lambda t: K.nbae_normalize(t.f("raw", 4, 8), t.f("out", 4, 4), 0.02))
N("nbae_normalize", "ca_nbae_normalize", "out", lambda t: K.nbae_normalize(t.f("raw", 4, 8), t.f("out", 3, 4)))


def _refine(t, f1=128 * 128):
    frags = [t(f"frag{i}", n) for i, n in enumerate((128 * 160, f1, 128 * 128, 16 * 128))]
    return K.nbae_refine(t("feat", 1, 2, 2, 128), t.f("pred", 1, 2, 2, 4), frags, [t.f(f"b{i}", n) for i, n in enumerate((128, 128, 128, 4))], t.f("out", 1, 4, 4, 4))


P("nbae_refine", _refine, sink=True)
N("nbae_refine", "ca_nbae_refine", "frags", lambda t: _refine(t, f1=128 * 64))
P("nbae_finish/map", lambda t: K.nbae_finish(t.f("pred", 1, 4, 4, 4), map=t.u("map", 1, 4, 4, 3)))
P("nbae_finish/control", lambda t: K.nbae_finish(t.f("pred", 1, 4, 4, 4), control=t.f("control", 2, 3, 4, 4), rep=2))
N("nbae_finish", "ca_nbae_finish", "map", lambda t: K.nbae_finish(t.f("pred", 1, 4, 4, 4), map=t.u("map", 1, 4, 4)))
P("rface_stem", lambda t: K.rface_stem(t.u("frames", 1, 4, 4, 3), t("w_packed", 16, 160), t.f("bias", 16), t("out", 1, 2, 2, 16), bgr=True))
N("rface_stem", "ca_rface_stem", "bias", lambda t: K.rface_stem(t.u("frames", 1, 4, 4, 3), t("w_packed", 16, 160), t("bias", 16), t("out", 1, 2, 2, 16)))
P("maxpool3x3s2", lambda t: K.maxpool3x3s2(t("x", 1, 5, 5, 8)))
P("maxpool3x3s2/out", lambda t: K.maxpool3x3s2(t("x", 1, 5, 5, 8), t("out", 1, 3, 3, 8)))
N("maxpool3x3s2", "ca_maxpool3x3s2", "out", lambda t: K.maxpool3x3s2(t("x", 1, 5, 5, 8), t("out", 1, 2, 3, 8)))
P("subsample2", lambda t: K.subsample2(t("x", 1, 5, 5, 8)))
P("subsample2/out", lambda t: K.subsample2(t("x", 1, 5, 5, 8), t("out", 1, 3, 3, 8)))
N("subsample2", "ca_subsample2", "x", lambda t: K.subsample2(t("x", 1, 5, 5, 8, nc=True)))
P("add_up2", lambda t: K.add_up2(t("a", 1, 4, 4, 8), t("b", 1, 2, 2, 8)))
P("add_up2/in_place", lambda t: (lambda a: K.add_up2(a, t("b", 1, 2, 2, 8), a))(t("a", 1, 4, 4, 8)))
N("add_up2", "ca_add_up2", "b", lambda t: K.add_up2(t("a", 1, 4, 4, 8), t("b", 1, 2, 2, 4)))
P("rface_decode_workspace_bytes", lambda t: K.rface_decode_workspace_bytes(1, 32, 32))
N("rface_decode_workspace_bytes", "ca_rface_decode_workspace_bytes", "images", lambda t: K.rface_decode_workspace_bytes(0, 0, 0))


def _rface_decode(t, h1=2):
    heads = [t.f("head8", 1, 4, 4, 32), t.f("head16", 1, h1, 2, 32), t.f("head32", 1, 1, 1, 32)]
    return K.rface_decode(heads, 32, 32, 0.5, 0.4, 5.0, 3, t.u("ws", 1 << 16), t.f("dets", 1, 4, 15), t.i("count", 1), t.i("overflow", 1))


P("rface_decode", _rface_decode)
N("rface_decode", "ca_rface_decode", "heads", lambda t: _rface_decode(t, h1=3))
P("face_align", lambda t: K.face_align(t.f("dets", 1, 4, 15), t.i("count", 1), 2.0, t.d("affine", 1, 4, 2, 3), t.d("inverse", 1, 4, 2, 3)))
N("face_align", "ca_face_align", "inverse", lambda t: K.face_align(t.f("dets", 1, 4, 15), t.i("count", 1), 2.0, t.d("affine", 1, 4, 2, 3), t.f("inverse", 1, 4, 2, 3)))
P("face_warp", lambda t: K.face_warp(t.u("frames", 1, 8, 8, 3), t.d("affine", 1, 2, 2, 3), t.i("count", 1), t.u("faces", 2, 512, 512, 3), bgr=True))
N("face_warp", "ca_face_warp", "faces", lambda t: K.face_warp(t.u("frames", 1, 8, 8, 3), t.d("affine", 1, 2, 2, 3), t.i("count", 1), t.u("faces", 1, 512, 512, 3)))
P("parse_prep", lambda t: K.parse_prep(t.u("faces", 1, 4, 4, 3), t("out", 1, 4, 4, 32)))
P("parse_prep/ring", lambda t: K.parse_prep(t.u("faces", 1, 4, 4, 3), t("out", 1, 6, 6, 32), reverse=False, ring=True))
N("parse_prep", "ca_parse_prep", "out", lambda t: K.parse_prep(t.u("faces", 1, 4, 4, 3), t("out", 1, 4, 4, 32), ring=True))
P("conv3x3_reflect", lambda t: K.conv3x3_reflect(t("x", 1, 4, 4, 8), t("w", 16, 3, 3, 8), t.f("bias", 16)))
P("conv3x3_reflect/rings", lambda t: K.conv3x3_reflect(t("x", 1, 6, 6, 8), t("w", 16, 3, 3, 8), t.f("bias", 16), up2=True, leaky=True, residual=t("residual", 1, 10, 10, 16),
                                                        out=t("out", 1, 10, 10, 16), in_ring=True, out_ring=True, res_ring=True))
P("conv3x3_reflect/s2_f32", lambda t: K.conv3x3_reflect(t("x", 1, 4, 4, 8), t("w", 16, 3, 3, 8), t.f("bias", 16), stride=2, out_f32=True))
N("conv3x3_reflect", "ca_conv3x3_reflect", "residual", lambda t: K.conv3x3_reflect(t("x", 1, 4, 4, 8), t("w", 16, 3, 3, 8), t.f("bias", 16), residual=t("residual", 1, 4, 4, 8)))
P("ring_fill", lambda t: K.ring_fill(t("x", 1, 6, 6, 8)))
P("ring_fill/replicate", lambda t: K.ring_fill(t("x", 1, 6, 6, 8), "replicate"))
N("ring_fill", "ca_ring_fill", "x", lambda t: K.ring_fill(t("x", 1, 6, 6, 8, nc=True)))
P("parse_mask", lambda t: K.parse_mask(t("x", 1, 4, 4, 8), t("w", 32, 3, 3, 8), t.f("bias", 32), t.u("mask", 1, 4, 4)))
P("parse_mask/ring", lambda t: K.parse_mask(t("x", 1, 6, 6, 8), t("w", 32, 3, 3, 8), t.f("bias", 32), t.u("mask", 1, 4, 4), in_ring=True))
N("parse_mask", "ca_parse_mask", "mask", lambda t: K.parse_mask(t("x", 1, 4, 4, 8), t("w", 32, 3, 3, 8), t.f("bias", 32), t.i("mask", 1, 4, 4)))
P("parse_labels/labels", lambda t: K.parse_labels(t.f("logits", 1, 4, 4, 32), labels=t.u("labels", 1, 4, 4)))
P("parse_labels/mask", lambda t: K.parse_labels(t.f("logits", 1, 4, 4, 32), mask=t.u("mask", 1, 4, 4)))
N("parse_labels", "ca_parse_labels", "labels", lambda t: K.parse_labels(t.f("logits", 1, 4, 4, 32), labels=t.u("labels", 1, 4, 3)))
P("mask_blur", lambda t: K.mask_blur(t.u("mask", 1, 8, 8), t.d("taps", 51), t.d("ws", 1, 8, 8), t.d("out", 1, 8, 8)))
N("mask_blur", "ca_mask_blur", "ws", lambda t: K.mask_blur(t.u("mask", 1, 8, 8), t.d("taps", 51), t.d("ws", 1, 8, 4), t.d("out", 1, 8, 8)))


def _paste(t, **out_bad):
    return K.face_paste(t.u("background", 1, 8, 8, 3), t.u("restored", 2, 512, 512, 3), t.d("masks", 2, 512, 512), t.d("inverse_affine", 1, 2, 2, 3), t.i("count", 1),
                        t.u("out", 1, 8, 8, 3, **out_bad), upscale=2.0)


P("face_paste", _paste)
N("face_paste", "ca_face_paste", "out", lambda t: _paste(t, cpu=True))

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), "two cases share an id"
MINUS_O = ("not/dwconv3x3/out", "not/conv3x3_dil", "not/hed_prep")


def record():
    lines = []
    for case in CASES:
        lines += run_case(case)[0]
    return [json.dumps(l, separators=(",", ":")) for l in lines]


@pytest.fixture(scope="module")
def recorded():
    lines = record()
    if os.environ.get(RECORD_ENV):
        with open(GOLDEN, "w") as f:
            f.write("\n".join(lines) + "\n")
    return lines


def _as_branch(line):
    """The one difference a later commit may show: what an `assert` rejected is now rejected with CAHipError."""
    return line.replace('"rejected":"AssertionError"', '"rejected":"CAHipError"')


def test_launch_arguments_match_the_record(recorded):
    golden = [_as_branch(l) for l in open(GOLDEN).read().splitlines()]
    got = [_as_branch(l) for l in recorded]
    for i, (a, b) in enumerate(zip(got, golden)):
        assert a == b, f"line {i + 1} of the record differs:\n now    {a}\n record {b}"
    assert len(got) == len(golden), f"{len(got)} lines now, {len(golden)} in the record"


def test_every_symbol_kernels_calls_is_recorded(recorded):
    src = open(os.path.join(ROOT, "controlanimate_amd", "kernels.py")).read()
    called = set(re.findall(r"\blib\(\)\.(ca_\w+)", src))
    assert len(called) > 140 and called <= set(_capi.SYMBOLS)
    seen = {json.loads(l).get("sym") for l in recorded}
    assert len(EXCUSED) <= 5
    missing = sorted(called - seen - set(EXCUSED))
    assert not missing, f"no case reaches {missing}: add one (and re-record) with the wrapper"


def test_every_wrapper_has_a_negative_case():
    src = open(os.path.join(ROOT, "controlanimate_amd", "kernels.py")).read()
    wrappers = set()
    for name, body in re.findall(r"^def ([a-z]\w*)\((.*?)(?=^(?:def|class) |\Z)", src, flags=re.S | re.M):
        if re.search(r"\blib\(\)\.ca_|attention_raw\(|cfg_scheduler_step\(", body):
            wrappers.add(name)
    without = {"pose_assemble", "conv_up2_phase_supported", "pdc_block_supported", "dpt_head_supported"}  # no operand a wrapper could reject: integers, or answers False
    negative = {c.id.split("/")[1] for c in CASES if c.entry}
    assert not sorted(wrappers - negative - without), sorted(wrappers - negative - without)


@pytest.mark.parametrize("case", [c for c in CASES if c.entry], ids=lambda c: c.id)
def test_a_wrong_operand_is_rejected_by_name(case):
    lines, err = run_case(case)
    golden = [json.loads(l) for l in open(GOLDEN).read().splitlines()]
    was = [l for l in golden if l["case"] == case.id]
    if "rejected" not in was[-1]:
        assert err is None, f"{case.id} reached the library at the recorded commit and must still: {err!r}"
        return
    assert err is not None, f"{case.id}: accepted"
    launched = [l["sym"] for l in lines[:-1] if not HOST_QUERIES.search(l["sym"])]  # (a *_workspace_bytes wrapper rejects BY asking the library)
    assert not launched and len(lines) == len(was), f"{case.id}: the library was called before the operand was rejected: {lines[:-1]}"
    if was[-1]["rejected"] == "TypeError":  # dt_code / _control_args: type and text are kept as they were
        assert type(err) is TypeError
    else:
        assert type(err) is _capi.CAHipError, repr(err)
        assert case.entry in str(err), f"{case.id}: {err} does not name {case.entry}"
        assert re.search(rf"(?<![A-Za-z0-9_]){re.escape(case.operand)}(?![A-Za-z0-9_])", str(err)), f"{case.id}: {err} does not name {case.operand}"


def test_operands_are_checked_under_python_O():
    """`python -O` strips assert statements; the operand checks must not go with them."""
    out = subprocess.check_output([sys.executable, "-O", os.path.abspath(__file__), *MINUS_O], text=True, cwd=ROOT)
    got = [json.loads(l) for l in out.strip().splitlines()]
    assert [l["case"] for l in got] == list(MINUS_O), got
    for l in got:
        assert l["optimize"] == 1 and l["reached_library"] == [] and l["rejected"] == "CAHipError", l


if __name__ == "__main__":
    for cid in sys.argv[1:]:
        lines, err = run_case(BY_ID[cid])
        print(json.dumps({"case": cid, "optimize": sys.flags.optimize, "reached_library": [l["sym"] for l in lines if "sym" in l],
                          "rejected": type(err).__name__ if err is not None else None}))
