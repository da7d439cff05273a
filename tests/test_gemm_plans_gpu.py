"""GPU: ca_gemm against a plain restatement (tests/gemm_ref.py) on EVERY kernel plan_gemm() can return -- wres160, ar128x64, pq256x320,
ps128x320, pp128x320 (+ split-K), 128x128 (+ split-K), 128x160, 128x64, 128x64_r3, reg_128x64, reg_128x128 -- at the places those
kernels are likeliest to be wrong and a rel-L2 over tens of thousands of mostly right rows cannot see: a ragged last M tile, a
row-bias group boundary inside a tile, the seam between the two A sources, the column tail of an N % 64 != 0 tile, a split-K slab.

Two tests (the tables are tests/gemm_ref.py's, shared with the CPU tests, which pin every case to its label without a GPU):
  exact     integer-valued operands (gemm_ref.integer_operands): every accumulation order gives the same integers, so the result must
            equal gemm_ref's number for number, twice, the row sums too, and nothing outside the output view may be touched.
            tests/test_gemm_ref_cpu.py shows the comparison rejecting a row-bias group off by one, a K tile dropped in the last 8 rows,
            swapped sources, stale ragged rows, a transposed 16 x 16 sub-tile and a residual read with the wrong leading dimension.
  rounding  the epilogues with real rounding (GEGLU, LayerNorm statistics in the kernel or from the producer's partial sums, the
            activations) on Gaussian operands: per 128-row block, at most 1.5x as far from the fp64 truth as fp32 torch in the
            documented order rounded to the dtype.
Every launch is built from the case (gemm_ref.gemm_args: the arguments kernels.gemm would build, partial LayerNorm sums handed over
as they are), reports its plan label, and the label is asserted."""
import ctypes as C
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gemm_ref as R  # noqa: E402
from test_kernels_gpu import DEV  # noqa: E402
from test_rect_latents_gpu import BF16, F16, NAME, both, planned  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -77.0       # exact in fp16, bf16 and fp32
GUARD_ROWS = 256


def _k():
    from controlanimate_amd import kernels
    return kernels


def column_slice(t: torch.Tensor, off: int, ld: int) -> torch.Tensor:
    """`t` [M, W] as columns off .. off + W of a fresh [M, ld] buffer (the rest zero); the contiguous tensor itself when ld == W."""
    if ld == t.shape[1]:
        return t.contiguous()
    buf = torch.zeros(t.shape[0], ld, device=t.device, dtype=t.dtype)
    buf[:, off:off + t.shape[1]] = t
    return buf[:, off:off + t.shape[1]]


class Launch:
    """The device operands of one case in one dtype, laid out as the case says; run() launches into a fresh sentinel-filled buffer."""

    def __init__(self, case, dtype, ops):
        k = _k()
        self.case, self.dtype, lay = case, dtype, case.layout()
        cast = lambda t: None if t is None else t.to(dtype)
        self.keep = keep = dict(a=column_slice(cast(ops["a"]), lay["a_off"], lay["lda"]), a2=None if ops["a2"] is None else cast(ops["a2"]).contiguous(),
                                w=cast(ops["w"]).contiguous(), bias=ops["bias"], rowbias=ops["rowbias"],
                                residual=None if ops["residual"] is None else column_slice(cast(ops["residual"]), lay["res_off"], lay["ld_res"]))
        assert keep["a"].stride(0) == lay["lda"] and (keep["residual"] is None or keep["residual"].stride(0) == lay["ld_res"])
        if case.frag:
            k.attach_w_frag(keep["w"], case.geglu)
            keep["w_frag"] = keep["w"]._frag[0]
        if case.ln:
            keep["ln_colsum"] = ops["ln"][1].float().contiguous()
            if case.ln != "inline":
                keep["ln_stats"] = ops["ln"][0].float().contiguous()
                assert keep["ln_stats"].shape == ((case.m, 2) if case.ln == "stats" else (case.m, case.parts, 2))
        for name in ("bias", "rowbias"):
            assert keep[name] is None or (keep[name].dtype == torch.float32 and keep[name].is_contiguous())
        self.parts = 0
        if case.row_sums:
            probe = R.gemm_args(k._capi, case, k.dt_code(dtype), {n: t.data_ptr() for n, t in keep.items() if t is not None})
            self.parts = R.row_sums_parts(k._capi, probe)
            assert self.parts in (case.n // 320, 4 * case.n // 320), f"{case.id}: the launch leaves no row sums"

    def run(self):
        """-> (output view [M, N or N / 2], its whole buffer, row sums or None)"""
        k, case, lay = _k(), self.case, self.case.layout()
        buf = torch.full((case.m + GUARD_ROWS, lay["ldc"]), SENTINEL, device=DEV, dtype=torch.float32 if case.out_f32 else self.dtype)
        out = buf[:case.m, lay["c_off"]:lay["c_off"] + case.ncols]
        ptr = {n: t.data_ptr() for n, t in self.keep.items() if t is not None}
        ptr["c"] = out.data_ptr()
        sums = None
        if self.parts:
            sums = torch.full((case.m, self.parts, 2), float("nan"), device=DEV)
            ptr["row_sums_out"] = sums.data_ptr()
        args = R.gemm_args(k._capi, case, k.dt_code(self.dtype), ptr)
        wbytes = R.workspace_wanted(k._capi, args)
        if wbytes > 0:
            ws = torch.empty((wbytes,), device=DEV, dtype=torch.uint8)
            args.workspace, args.workspace_bytes = ws.data_ptr(), wbytes
        k._record_plan(k.lib().ca_gemm_plan_name, args)
        k.check(k.lib().ca_gemm(C.byref(args), k._stream()), "ca_gemm")
        return out, buf, sums


def assert_untouched_outside(out, buf, case, what):
    """Every element of the buffer outside the output view still holds the sentinel: the guard rows below a ragged last tile and, for a
    strided case, the columns on both sides."""
    lay = case.layout()
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:case.m, lay["c_off"]:lay["c_off"] + case.ncols] = False
    hit = mask & (buf != SENTINEL)
    n = int(hit.sum())
    if n:
        r, c = divmod(int(hit.flatten().to(torch.uint8).argmax()), buf.shape[1])
        raise AssertionError(f"{what}: {n} elements outside the {case.m} x {case.ncols} output view were written; first at buffer (row {r}, column {c})")


# ------------------------------------------------------------------------------------ exact: integer operands
@functools.lru_cache(maxsize=2)
def integer_case(case):
    """Integer operands on the device (fp32) and alpha * (ln?(a w^T) + bias + row bias) of them in fp64.  Never modified afterwards."""
    ops = {}
    for n, t in R.integer_operands(case).items():
        ops[n] = tuple(x.to(DEV) for x in t) if isinstance(t, tuple) else (t.to(DEV) if torch.is_tensor(t) else t)
    return ops, R.exact_before_residual(ops, case)


@both(R.EXACT_CASES)
def test_every_plan_is_exact_on_integer_operands(case, dtype):
    ops, pre = integer_case(case)
    what = f"{case.id} {NAME[dtype]}"
    launch = Launch(case, dtype, ops)
    want, want_sums = R.exact_result(ops, case, dtype, pre=pre, parts=launch.parts)
    with planned(case.label, case.label):
        (y, buf, sums), (again, buf2, sums2) = launch.run(), launch.run()
    R.assert_same(y, want, what)
    assert_untouched_outside(y, buf, case, what)
    assert torch.equal(y, again) and torch.equal(buf, buf2), "two launches on the same inputs differ"
    if case.row_sums:
        R.assert_same(sums.reshape(case.m, -1), want_sums.reshape(case.m, -1), f"{what} row sums ({launch.parts} parts)")
        assert torch.equal(sums, sums2)


# ------------------------------------------------------------------------------------ rounding: Gaussian operands
def gaussian_operands(case, dtype):
    """As tools/ps_check.gemm_cases: N(0, 1) activations (1.3 N(0, 1) + 0.4 under a LayerNorm), weights scaled by K^-1/2, both rounded to
    the dtype; fp32 bias.  LayerNorm statistics of the ROUNDED a in fp64, handed to kernel and yardstick alike as fp32 (mean, rstd) --
    or, ln = "parts", as the partial sums a producing GEMM would have left."""
    g = torch.Generator(device=DEV).manual_seed(17 * case.m + case.n + case.k1)
    kk = case.k1 + case.k2
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    a = (rn(case.m, case.k1) * 1.3 + 0.4 if case.ln else rn(case.m, case.k1)).to(dtype)
    w = (rn(case.n, kk) * kk ** -0.5).to(dtype)
    d = dict(a=a, a2=rn(case.m, case.k2).to(dtype) if case.k2 else None, w=w, bias=rn(case.n) if case.bias else None, rowbias=None, residual=None, ln=None)
    stats = None
    if case.ln:
        stats = R.ln_statistics(a).float()
        d["ln"] = (R.ln_partial_sums(a, case.parts) if case.ln == "parts" else stats, w.float().sum(1))
    return d, stats


def block_distances(y, truth):
    """(worst rel-L2 of a 128-row block -- the ragged remainder a block of its own --, max-abs distance) of y from the fp64 truth."""
    d = y.double() - truth
    m = d.shape[0]
    pad = -m % 128
    num = torch.nn.functional.pad((d * d).sum(1), (0, pad)).reshape(-1, 128).sum(1)
    den = torch.nn.functional.pad((truth * truth).sum(1), (0, pad)).reshape(-1, 128).sum(1)
    return float((num / den).sqrt().max()), float(d.abs().max())


@both(R.ROUNDING_CASES)
def test_rounding_epilogues_are_as_close_as_fp32_torch_in_every_row_block(case, dtype):
    """Truth: gemm_ref in fp64 without the intermediate rounding, LayerNorm as F.layer_norm then linear.  Yardstick: gemm_ref in fp32
    in the documented order (folded LayerNorm, the value before the residual rounded to the dtype), rounded to the dtype.  The margin of
    1.5 is test_rect_latents_gpu.assert_as_close_as_fp32_torch's: it covers one differing rounding."""
    d, stats = gaussian_operands(case, dtype)
    kw = dict(a2=d["a2"], bias=d["bias"], act=case.act, geglu=case.geglu)
    truth = R.gemm_ref(d["a"], d["w"], layer_norm_eps=R.LN_EPS if case.ln else None, **kw)
    yard = R.gemm_ref(d["a"], d["w"], ln=(stats, d["ln"][1]) if case.ln else None, round_to=dtype, acc=torch.float32, **kw).to(dtype)
    launch = Launch(case, dtype, d)
    with planned(case.label, case.label):
        (y, buf, _), (again, _, _) = launch.run(), launch.run()
    assert y.shape == truth.shape and y.dtype == dtype and torch.isfinite(y.float()).all()
    rk, mk = block_distances(y, truth)
    ry, my = block_distances(yard, truth)
    msg = f"{case.id} {NAME[dtype]}: kernel worst-block rel-L2 {rk:.3e} max-abs {mk:.3e}; fp32 torch worst-block rel-L2 {ry:.3e} max-abs {my:.3e}"
    print(msg)
    assert_untouched_outside(y, buf, case, case.id)
    assert rk <= 1.5 * ry and mk <= 1.5 * my, msg
    assert torch.equal(y, again), "two launches on the same inputs differ"
