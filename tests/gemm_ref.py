"""Plain restatement of ca_gemm's contract, integer-valued operands on which a correct kernel has no rounding freedom, and the case
tables the dense-GEMM plan tests share (tests/test_gemm_plans_gpu.py runs them on the kernels, tests/test_gemm_ref_cpu.py checks this
file against torch, pins every case to its plan label and shows that the comparison catches the index errors it is there for).

    y = geglu?(act(post * (round(alpha * (ln?(cat(a, a2)) w^T + bias + rowbias[row // rows_per_group])) + residual)))

a [M, K1], a2 [M, K2], w [N, K1 + K2], residual and y [M, N] (y [M, N / 2] with GEGLU: column pairs (value, gate) -> value * gelu(gate)),
bias [N] and rowbias [groups, N] fp32, and round() is the rounding to the activation type the LDS-staged epilogues apply before the
residual joins (the order of tools/ps_check.gemm_reference; `round_to=None` leaves it out).  The folded LayerNorm is
rstd * (a w^T - mean * colsum) with (mean, rstd) per row and colsum = w.sum(1) handed over as operands.  A launch asked for row sums
leaves (sum, sum of squares) of every STORED row per part -- n / 320 parts of 320 columns, or 4 n / 320 of 80: what the launch reports.

Why integers: with a in {-1, 0, 1}, w in {-1, 0, 1}, bias and row bias in [-3, 3] every partial sum of every accumulation order, K
split and tile shape is an integer far below 2^24, so fp32 accumulation is exact; with mean an integer, rstd in {1/2, 1, 2} and alpha,
post in {1, 2} the fold and the scales are exact too.  The kernel's result must then be `exact.to(dtype)` number for number: one
wrong row, one row-bias group off by one, one dropped K tile in a ragged tile fails the comparison, where a rel-L2 over 65536 mostly
right rows would move by 4e-3.  The conditions are asserted on the OPERANDS by exact_result(), never on the kernel: the value before
the residual and the final value must be numbers of the dtype (fp16: every integer and half-integer below 1024; bf16: every integer up
to 256 and every half-integer below 128), so no rounding happens anywhere; row sums of squares stay below 2^24.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

LN_EPS = 1e-5


class Case(NamedTuple):
    label: str            # the plan label the launch must report (ca_gemm_plan_name, a workspace offered where the query wants one)
    m: int
    n: int
    k1: int
    k2: int = 0
    bias: bool = False
    rowbias: int = 0      # rows per row-bias group (0: none)
    residual: bool = False
    alpha: float = 1.0
    post: float = 1.0
    out_f32: bool = False
    frag: bool = False    # hand over W in fragment order as well (ca_gemm_args.w_frag)
    row_sums: bool = False
    ln: Optional[str] = None   # "stats": finished (mean, rstd); "parts": the producer's partial sums; "inline": in-kernel statistics
    parts: int = 0        # ln == "parts": partial sums per row
    geglu: bool = False
    act: int = 0          # 1 SiLU, 2 quick-GELU, 3 GELU (erf)
    strided: bool = False  # a, out and residual are column slices of wider buffers

    @property
    def id(self) -> str:
        s = f"{self.label}-{self.m}x{self.n}x{self.k1}" + (f"+{self.k2}" if self.k2 else "")
        for on, tag in ((self.bias, "bias"), (self.rowbias, f"rb{self.rowbias}"), (self.residual, "res"), (self.alpha != 1, f"alpha{self.alpha:g}"),
                        (self.post != 1, f"post{self.post:g}"), (self.out_f32, "f32"), (self.row_sums, "sums"), (self.ln, f"ln_{self.ln}{self.parts or ''}"),
                        (self.geglu, "geglu"), (self.act, f"act{self.act}"), (self.strided, "strided")):
            if on:
                s += "-" + tag
        return s

    @property
    def ncols(self) -> int:
        return self.n // 2 if self.geglu else self.n

    def layout(self) -> dict:
        """Leading dimensions and column offsets (elements) of a, out and residual inside their buffers.  Strided cases: offsets that are
        multiples of 8 elements, so every pointer stays 16-byte aligned and the plan is the contiguous launch's."""
        if not self.strided:
            return dict(lda=self.k1, a_off=0, ldc=self.ncols, c_off=0, ld_res=self.n, res_off=0)
        return dict(lda=self.k1 + 16, a_off=8, ldc=self.ncols + 24, c_off=16, ld_res=self.n + 8, res_off=8)


def _c(label, m, n, k, k2=0, **epilogue) -> Case:
    """(m, n, K, of which k2 in the second source): the notation of tests/test_dispatch_plan.py's table."""
    return Case(label, m, n, k - k2, k2, **epilogue)


# Every M is ragged (a last tile of 8 .. 120 rows); every row-bias group size puts boundaries inside tiles at more than one position
# and leaves the last group partial.  One or more cases per plan plan_gemm can return, with the epilogues that kernel implements.
EXACT_CASES = [
    _c("wres160", 16392, 320, 320, bias=True, rowbias=96, residual=True, alpha=2.0),
    _c("wres160", 16392, 320, 320, rowbias=32, residual=True, strided=True),
    _c("wres160", 16392, 160, 320, 64, bias=True),
    _c("wres160", 16392, 480, 320, ln="stats", bias=True),
    _c("ar128x64", 16456, 960, 320, frag=True, bias=True, rowbias=128),
    _c("ar128x64", 16392, 1280, 320, frag=True, residual=True, strided=True),
    _c("ar128x64", 16456, 960, 320, frag=True, ln="stats"),
    _c("pq256x320", 65496, 320, 512, bias=True, rowbias=128, residual=True, alpha=2.0),
    _c("pq256x320", 65496, 320, 512, rowbias=384),
    _c("pq256x320", 32728, 640, 512, residual=True, row_sums=True, strided=True),
    _c("pq256x320", 65496, 320, 512, ln="stats"),
    _c("ps128x320", 32728, 320, 128, rowbias=64, residual=True),
    _c("ps128x320", 32728, 320, 128, rowbias=192, alpha=2.0),
    _c("ps128x320", 32728, 320, 128, 64, row_sums=True),
    _c("ps128x320", 32728, 640, 512, 256, bias=True, strided=True),
    _c("ps128x320", 32728, 320, 128, ln="stats"),
    _c("ps128x320", 8152, 1280, 1280, residual=True, row_sums=True),
    _c("pp128x320", 16344, 320, 640, bias=True, rowbias=64, residual=True, post=2.0),
    _c("pp128x320", 16344, 320, 640, 128, row_sums=True),
    _c("pp128x320", 16344, 320, 640, ln="stats"),
    _c("pp128x320_splitk4", 2008, 1280, 3072, bias=True, rowbias=64, residual=True),
    _c("128x128_splitk4", 1000, 640, 3072, bias=True, rowbias=64, residual=True, alpha=2.0),
    _c("128x128_splitk4", 1000, 256, 3072, 1024),
    _c("128x128", 65496, 128, 64, bias=True, rowbias=64, residual=True),
    _c("128x128", 32728, 256, 128, 64, strided=True),
    _c("128x128", 32728, 256, 128, ln="stats"),
    _c("128x160", 32728, 320, 64, residual=True),
    _c("128x160", 65496, 160, 64, rowbias=72),
    _c("128x160", 65496, 160, 64, ln="stats"),
    _c("128x64", 65496, 64, 64, residual=True),
    _c("128x64", 65496, 8, 64, bias=True),
    _c("128x64", 65496, 24, 128, 64, rowbias=40),
    _c("128x64_r3", 300, 1000, 64, bias=True, rowbias=7, residual=True),      # a 40-column tail in the last 64-column tile
    _c("128x64_r3", 1, 64, 64),
    _c("128x64_r3", 300, 4, 64, residual=True, out_f32=True),                 # the direct 4-column epilogue
    _c("128x64_r3", 300, 24, 128, 64, strided=True),
    _c("128x64_r3", 2, 1280, 320, bias=True, out_f32=True),
    _c("128x64_r3", 300, 320, 128, ln="stats"),
    _c("reg_128x64", 300, 64, 40, bias=True, rowbias=7, residual=True),
    _c("reg_128x64", 300, 24, 64, 32),
    _c("reg_128x64", 300, 4, 32, out_f32=True),
    _c("reg_128x64", 16392, 320, 320, 8),                                     # K = 320 but not the weight-resident kernel's: c1 % 32 != 0
    _c("reg_128x128", 65496, 128, 40, bias=True),
    _c("reg_128x128", 65496, 256, 64, 32, residual=True),
]

# The epilogues with real rounding: each label carries what its kernel implements.
ROUNDING_CASES = [
    # GEGLU
    _c("wres160", 16392, 640, 320, geglu=True, bias=True),
    _c("ar128x64", 16456, 1280, 320, frag=True, geglu=True, bias=True),
    _c("pq256x320", 32728, 640, 512, geglu=True, bias=True),
    _c("pq256x320", 32728, 640, 640, geglu=True, bias=True, ln="stats"),
    _c("ps128x320", 32728, 640, 128, geglu=True, bias=True),
    _c("pp128x320", 16344, 320, 640, geglu=True, bias=True),
    _c("128x128", 32728, 256, 128, geglu=True, bias=True),
    _c("128x160", 32728, 320, 64, geglu=True, bias=True),
    _c("128x64_r3", 300, 256, 64, geglu=True, bias=True),
    _c("reg_128x64", 300, 64, 40, geglu=True, bias=True),
    # in-kernel LayerNorm statistics
    _c("wres160", 16392, 480, 320, ln="inline", bias=True),
    _c("wres160", 16392, 640, 320, ln="inline", bias=True, geglu=True),
    _c("ar128x64", 16456, 960, 320, frag=True, ln="inline", bias=True),
    _c("ar128x64", 16456, 1280, 320, frag=True, ln="inline", bias=True, geglu=True),
    # the producer's partial sums, finished by the consumer's epilogue
    _c("ps128x320", 32728, 640, 640, ln="parts", parts=2, bias=True),
    _c("ps128x320", 32728, 640, 640, ln="parts", parts=2, bias=True, geglu=True),
    _c("ps128x320", 8152, 1280, 1280, ln="parts", parts=4, bias=True),
    _c("pp128x320", 16344, 320, 640, ln="parts", parts=2, bias=True),
    _c("pp128x320", 8152, 640, 1280, ln="parts", parts=4, bias=True, geglu=True),
    _c("128x128", 32728, 256, 640, ln="parts", parts=2, bias=True),
    _c("128x64_r3", 300, 320, 640, ln="parts", parts=2, bias=True),
    # SiLU and the two CLIP activations
    *[_c(label, m, n, k, bias=True, act=act) for (label, m, n, k) in (("128x64_r3", 300, 256, 64), ("128x128", 32728, 256, 128), ("pp128x320", 16344, 320, 640))
      for act in (1, 2, 3)],
]

SMALLEST = next(c for c in EXACT_CASES if (c.m, c.n, c.k1, c.k2) == (300, 24, 64, 64))   # two sources, two K tiles, a 44-row last tile


def kind(label: str) -> str:
    """The plan kind of a label: the split-K count dropped."""
    return label.split("_splitk")[0] + ("_splitkS" if "_splitk" in label else "")


KINDS = {kind(c.label) for c in EXACT_CASES}


# ------------------------------------------------------------------------------------ the restatement
def row_bias_rows(rowbias: torch.Tensor, rows: int, rows_per_group: int, shift: int = 0) -> torch.Tensor:
    """[rows, N]: row r takes rowbias[(r + shift) // rows_per_group] (shift = 0 is the contract)."""
    idx = (torch.arange(rows, device=rowbias.device) + shift).div(rows_per_group, rounding_mode="floor").clamp_(0, rowbias.shape[0] - 1)
    return rowbias[idx]


def activation(y: torch.Tensor, act: int) -> torch.Tensor:
    return {0: lambda t: t, 1: F.silu, 2: lambda t: t * torch.sigmoid(1.702 * t), 3: F.gelu}[act](y)


def row_sums(stored: torch.Tensor, parts: int, acc=torch.float64) -> torch.Tensor:
    """[M, parts, 2]: (sum, sum of squares) of every stored row per part of N / parts columns."""
    t = stored.to(acc).reshape(stored.shape[0], parts, -1)
    return torch.stack([t.sum(2), (t * t).sum(2)], 2)


def gemm_ref(a, w, *, a2=None, bias=None, rowbias=None, rows_per_group=0, residual=None, alpha=1.0, post_scale=1.0, act=0, geglu=False,
             ln=None, layer_norm_eps=None, round_to=None, acc=torch.float64, parts=0, stored_as=None, rb_shift=0):
    """ca_gemm on tensors of any float dtype and device, computed in `acc`; returns y [M, N or N / 2] in `acc`, and with parts > 0
    (y, row sums [M, parts, 2] of y as stored in `stored_as`).  ln = (stats [M, 2] = (mean, rstd), colsum [N]): the folded form.
    layer_norm_eps: the plain form instead -- F.layer_norm of cat(a, a2) (no affine: the caller folded it into w and bias), then linear."""
    x = a.to(acc) if a2 is None else torch.cat([a.to(acc), a2.to(acc)], 1)
    wt = w.to(acc).t()
    if layer_norm_eps is not None:
        assert ln is None
        y = F.layer_norm(x, (x.shape[1],), eps=layer_norm_eps) @ wt
    else:
        y = x @ wt
        if ln is not None:
            st, cs = ln
            y = st[:, 1:2].to(acc) * (y - st[:, 0:1].to(acc) * cs.to(acc)[None, :])
    if bias is not None:
        y = y + bias.to(acc)
    if rowbias is not None:
        y = y + row_bias_rows(rowbias.to(acc), y.shape[0], rows_per_group, rb_shift)
    y = y * alpha
    if round_to is not None:
        y = y.to(round_to).to(acc)
    if residual is not None:
        y = y + residual.to(acc)
    y = activation(y * post_scale, act)
    if geglu:
        y = y[:, 0::2] * F.gelu(y[:, 1::2])
    if parts:
        return y, row_sums(y if stored_as is None else y.to(stored_as), parts, acc)
    return y


def ln_statistics(a: torch.Tensor, eps: float = LN_EPS, acc=torch.float64) -> torch.Tensor:
    """(mean, rstd) per row, [M, 2] in `acc`."""
    x = a.to(acc)
    return torch.stack([x.mean(1), (x.var(1, unbiased=False) + eps).rsqrt()], 1)


def ln_partial_sums(a: torch.Tensor, parts: int) -> torch.Tensor:
    """[M, parts, 2] fp32: (sum, sum of squares) per part of K / parts columns, computed in fp64 -- what a producing GEMM leaves."""
    return row_sums(a, parts).float().contiguous()


# ------------------------------------------------------------------------------------ integer operands
def integer_operands(case: Case, seed: int = 0) -> dict:
    """fp32 CPU tensors with integer values: a (and a2) in {-1, 0, 1} with P(non-zero) = 1/4, w in {-1, 0, 1} uniformly, bias and row
    bias in [-3, 3], residual in [-8, 8]; for ln = "stats" mean an integer in [-2, 2], rstd in {1/2, 1, 2} and colsum = w.sum(1).
    Every value is exact in fp16 and in bf16."""
    assert case.ln in (None, "stats") and not case.geglu and not case.act and case.alpha in (1.0, 2.0) and case.post in (1.0, 2.0)
    g = torch.Generator().manual_seed(2000 + seed)
    k = case.k1 + case.k2

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).float()

    def sparse(*shape):   # r in 0 .. 7: 0 -> -1, 1 -> +1, the other six -> 0
        r = torch.randint(0, 8, shape, generator=g)
        return (r == 1).float() - (r == 0).float()

    d = dict(a=sparse(case.m, case.k1), a2=sparse(case.m, case.k2) if case.k2 else None, w=ints(-1, 1, case.n, k), bias=None, rowbias=None,
             residual=None, ln=None, rows_per_group=case.rowbias, alpha=case.alpha, post_scale=case.post)
    if case.bias:
        d["bias"] = ints(-3, 3, case.n)
    if case.rowbias:
        d["rowbias"] = ints(-3, 3, -(-case.m // case.rowbias), case.n)
    if case.residual:
        d["residual"] = ints(-8, 8, case.m, case.n)
    if case.ln == "stats":
        st = torch.stack([ints(-2, 2, case.m), 2.0 ** ints(-1, 1, case.m)], 1).contiguous()
        d["ln"] = (st, d["w"].sum(1))
    return d


def _whole(t, what, case, step=1.0):
    assert t is None or bool((t / step == (t / step).round()).all()), f"{case.id}: {what} is not a multiple of {step}"


def _numbers_of(t: torch.Tensor, dtype, what, case):
    top = float(t.abs().max())
    assert bool((t.to(dtype).to(t.dtype) == t).all()), \
        f"{case.id}: {what} reaches {top}: not every value is a {dtype} number (fp16: multiples of 1/2 below 1024; bf16: integers up to 256, halves below 128)"


def exact_before_residual(ops: dict, case: Case, acc=torch.float64) -> torch.Tensor:
    """alpha * (ln?(cat(a, a2)) w^T + bias + rowbias) of integer_operands(case) (tensors on any device), after asserting that the
    operands are the integers the argument in the module docstring needs.  fp16 and bf16 comparisons of one case share it."""
    for name in ("a", "a2", "w", "bias", "rowbias", "residual"):
        _whole(ops[name], name, case)
    assert float(ops["a"].abs().max()) <= 1 and float(ops["w"].abs().max()) <= 1 and (ops["a2"] is None or float(ops["a2"].abs().max()) <= 1)
    assert ops["alpha"] in (1.0, 2.0) and ops["post_scale"] in (1.0, 2.0)
    half = False
    if ops["ln"] is not None:
        st, cs = ops["ln"]
        _whole(st[:, 0], "mean", case)
        _whole(st[:, 1], "rstd", case, 0.5)
        assert bool(((st[:, 1] == 0.5) | (st[:, 1] == 1) | (st[:, 1] == 2)).all()) and float(st[:, 0].abs().max()) <= 2
        assert torch.equal(cs, ops["w"].sum(1)), f"{case.id}: colsum is not w.sum(1)"
        half = bool((st[:, 1] == 0.5).any())
    assert case.k1 + case.k2 + 14 < 2 ** 24                     # every partial sum, in any order, is an integer fp32 holds
    pre = gemm_ref(ops["a"], ops["w"], a2=ops["a2"], bias=ops["bias"], rowbias=ops["rowbias"], rows_per_group=ops["rows_per_group"],
                   alpha=ops["alpha"], ln=ops["ln"], acc=acc)
    _whole(pre, "the value before the residual", case, 0.5 if half else 1.0)
    return pre


def exact_result(ops: dict, case: Case, dtype: torch.dtype, *, pre: Optional[torch.Tensor] = None, parts: int = 0):
    """What a correct kernel returns for integer_operands(case) in `dtype` -- (y, row sums [M, parts, 2] in fp32 or None) -- after
    asserting on the OPERANDS that it has no rounding freedom (module docstring).  A case that breaks a bound fails here."""
    assert dtype in (torch.float16, torch.bfloat16)
    if pre is None:
        pre = exact_before_residual(ops, case)
    direct = case.n < 8                      # (the 4-column epilogue keeps fp32 up to the store)
    if not (direct and case.out_f32):
        _numbers_of(pre, dtype, "the value before the residual", case)
    final = (pre + ops["residual"].to(pre.dtype) if ops["residual"] is not None else pre) * ops["post_scale"]
    if not case.out_f32:
        _numbers_of(final, dtype, "the result", case)
    y = final.to(torch.float32 if case.out_f32 else dtype)
    if not parts:
        return y, None
    sums = row_sums(y, parts, pre.dtype)
    top = float(sums[..., 1].max())
    assert top < 2 ** 24, f"{case.id}: a row's sum of squares reaches {top}: fp32 no longer adds it exactly"
    return y, sums.float()


def assert_same(out: torch.Tensor, ref: torch.Tensor, what: str) -> None:
    """out == ref number for number ([M, N], same dtype); on a mismatch: how many elements and rows differ and the first (row, column)."""
    assert out.shape == ref.shape and out.dtype == ref.dtype, f"{what}: {tuple(out.shape)} {out.dtype} vs {tuple(ref.shape)} {ref.dtype}"
    bad = (out != ref) | torch.isnan(out)
    n = int(bad.sum())
    if n:
        first = int(bad.flatten().to(torch.uint8).argmax())
        r, c = divmod(first, out.shape[1])
        raise AssertionError(f"{what}: {n} of {out.numel()} elements in {int(bad.any(1).sum())} rows differ; first at (row {r}, column {c}): "
                             f"got {float(out[r, c])}, want {float(ref[r, c])}")


# ------------------------------------------------------------------------------------ the launch a case describes
FAKE = 0x10000  # never dereferenced: the plan only looks at sizes, flags, which pointers are set and their alignment


def gemm_args(capi, case: Case, dtype_code: int, ptr=None, *, alpha=None, post=None, act=None, out_f32=None):
    """ca_gemm_args of `case`.  ptr: name -> device address (a, a2, w, c, bias, rowbias, residual, ln_stats, ln_colsum, row_sums_out,
    w_frag -- each the address of the VIEW's first element); None: fake addresses with the case's alignment, for the plan query."""
    lay = case.layout()
    if ptr is None:
        ptr = dict(a=FAKE + 2 * lay["a_off"], c=FAKE + 2 * lay["c_off"], residual=FAKE + 2 * lay["res_off"])
    at = lambda name: ptr.get(name, FAKE)
    a = capi.GemmArgs(a=at("a"), w=at("w"), c=at("c"), m=case.m, n=case.n, k1=case.k1, k2=case.k2, lda=lay["lda"], lda2=case.k2, ldc=lay["ldc"],
                      alpha=case.alpha if alpha is None else alpha, post_scale=case.post if post is None else post,
                      act=case.act if act is None else act, out_f32=int(case.out_f32 if out_f32 is None else out_f32),
                      dtype=dtype_code, geglu=int(case.geglu), rows_per_group=case.rowbias)
    if case.k2:
        a.a2 = at("a2")
    if case.bias:
        a.bias = at("bias")
    if case.rowbias:
        a.rowbias, a.ld_rowbias = at("rowbias"), case.n
    if case.residual:
        a.residual, a.ld_res = at("residual"), lay["ld_res"]
    if case.ln:
        a.ln_colsum, a.ln_eps = at("ln_colsum"), LN_EPS
        if case.ln != "inline":
            a.ln_stats = at("ln_stats")
        if case.ln == "parts":
            a.ln_parts = case.parts
    if case.frag:
        a.w_frag = at("w_frag")
    if case.row_sums:
        a.row_sums_out = at("row_sums_out")
    return a


def workspace_wanted(capi, args) -> int:
    """The bytes kernels.gemm would offer this launch: what ca_gemm_workspace_bytes asks for, nothing beside row sums."""
    import ctypes
    return 0 if args.row_sums_out else int(capi.lib().ca_gemm_workspace_bytes(ctypes.byref(args)))


def plan_name(capi, args) -> str:
    import ctypes
    buf = ctypes.create_string_buffer(64)
    rc = capi.lib().ca_gemm_plan_name(ctypes.byref(args), buf, 64)
    assert rc == 0, capi.lib().ca_last_error()
    return buf.value.decode()


def row_sums_parts(capi, args) -> int:
    import ctypes
    return int(capi.lib().ca_gemm_row_sums_parts(ctypes.byref(args)))
