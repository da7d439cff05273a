"""CPU: the dense-GEMM restatement the plan parity tests trust (tests/gemm_ref.py, used by tests/test_gemm_plans_gpu.py): it equals
torch in fp64 for every epilogue, every case of both tables is on the kernel it names (ca_gemm_plan_name, no launch), the exact
table covers every plan plan_label can produce, its integer operands satisfy the exactness conditions in both dtypes, and its
comparison REJECTS the index errors the tests are there to catch -- shown here on wrong references, so that a green GPU run means the
kernels do not make them."""
import functools
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as R  # noqa: E402

F16, BF16 = torch.float16, torch.bfloat16
PLAN_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "controlanimate_amd", "csrc", "ca_gemm_plan.h")


@pytest.fixture(scope="module")
def capi():
    from controlanimate_amd import _build, _capi
    _build.build(verbose=False)
    return _capi


# ---- the restatement against torch, fp64
# m, n, k1, k2, bias, rows per row-bias group, residual, alpha, post, act, geglu, ln, round_to
RANDOM_CASES = [(37, 24, 16, 0, False, 0, False, 1.0, 1.0, 0, False, False, None), (37, 24, 16, 8, True, 5, True, 0.75, 0.5, 1, False, False, F16),
                (20, 16, 24, 0, True, 0, False, 1.0, 1.0, 2, False, False, None), (20, 16, 24, 0, True, 0, True, 1.0, 1.0, 3, False, False, BF16),
                (33, 32, 40, 0, True, 0, False, 1.0, 1.0, 0, True, False, F16), (33, 32, 40, 0, True, 7, False, 1.0, 1.0, 0, False, True, None),
                (33, 32, 40, 0, True, 0, False, 1.25, 1.0, 0, True, True, None)]


@pytest.mark.parametrize("case", RANDOM_CASES, ids=lambda c: "-".join(str(v).replace("torch.", "") for v in c))
def test_restatement_equals_torch_in_fp64(case):
    m, n, k1, k2, has_bias, rpg, has_res, alpha, post, act, geglu, ln, round_to = case
    g = torch.Generator().manual_seed(m * 100 + n)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    a, a2, w = rn(m, k1) * 1.3 + 0.4, (rn(m, k2) if k2 else None), rn(n, k1 + k2)
    bias, rb, res = (rn(n) if has_bias else None), (rn(-(-m // rpg), n) if rpg else None), (rn(m, n) if has_res else None)
    st = R.ln_statistics(a) if ln else None
    got = R.gemm_ref(a, w, a2=a2, bias=bias, rowbias=rb, rows_per_group=rpg, residual=res, alpha=alpha, post_scale=post, act=act, geglu=geglu,
                     ln=(st, w.sum(1)) if ln else None, round_to=round_to)
    x = a if a2 is None else torch.cat([a, a2], 1)
    y = F.linear(F.layer_norm(x, (k1,), eps=R.LN_EPS) if ln else x, w, bias)
    if rpg:
        y = y + rb.repeat_interleave(rpg, 0)[:m]
    y = y * alpha
    if round_to is not None:
        y = y.to(round_to).double()
    if has_res:
        y = y + res
    y = y * post
    y = {0: y, 1: F.silu(y), 2: y * torch.sigmoid(1.702 * y), 3: F.gelu(y)}[act]
    if geglu:
        y = y[:, 0::2] * F.gelu(y[:, 1::2])
    # (the folded LayerNorm differs from the plain one by the cancellation in a w^T - mean colsum: 1e-13 at these sizes)
    assert got.shape == y.shape == (m, n // 2 if geglu else n) and (got - y).abs().max().item() < 1e-11
    if ln:   # the plain form (the truth of the rounding tests) is the same function
        plain = R.gemm_ref(a, w, bias=bias, alpha=alpha, layer_norm_eps=R.LN_EPS)
        assert (plain - F.linear(F.layer_norm(x, (k1,), eps=R.LN_EPS), w, bias) * alpha).abs().max().item() < 1e-12


def test_row_sums_and_partial_layernorm_sums():
    g = torch.Generator().manual_seed(3)
    a, w = torch.randn(19, 640, generator=g, dtype=torch.float64), torch.randn(640, 640, generator=g, dtype=torch.float64) / 25
    y, sums = R.gemm_ref(a, w, parts=8, stored_as=F16)
    stored = y.half().double().reshape(19, 8, 80)
    assert sums.shape == (19, 8, 2) and torch.equal(sums[..., 0], stored.sum(2)) and torch.equal(sums[..., 1], (stored * stored).sum(2))
    ps = R.ln_partial_sums(a.half(), 2)
    assert ps.dtype == torch.float32 and ps.shape == (19, 2, 2)
    mean = ps[..., 0].double().sum(1) / 640
    rstd = (ps[..., 1].double().sum(1) / 640 - mean * mean + R.LN_EPS).rsqrt()
    st = R.ln_statistics(a.half())
    assert torch.allclose(mean, st[:, 0], atol=1e-6) and torch.allclose(rstd, st[:, 1], rtol=1e-5)


# ---- every case is on the kernel it names
def label_of(capi, case, dtype_code, **over):
    """The label ca_gemm_plan_name gives the case's launch: fake pointers, the workspace the query asks for offered."""
    a = R.gemm_args(capi, case, dtype_code, **over)
    if R.workspace_wanted(capi, a) > 0:
        a.workspace, a.workspace_bytes = R.FAKE, 1 << 40
    return R.plan_name(capi, a)


@pytest.mark.parametrize("case", R.EXACT_CASES + R.ROUNDING_CASES, ids=lambda c: c.id)
def test_case_is_on_the_kernel_it_names(capi, case):
    for dt in (capi.CA_F16, capi.CA_BF16):
        assert label_of(capi, case, dt) == case.label, (case.id, dt)
    assert case.m % 128 != 0 and (not case.rowbias or case.m % case.rowbias != 0), "a ragged M and a partial last row-bias group"
    if case.row_sums:
        parts = R.row_sums_parts(capi, R.gemm_args(capi, case, capi.CA_F16))
        assert parts in (case.n // 320, 4 * case.n // 320)
    if case.strided:
        lay = case.layout()
        assert all(lay[o] % 8 == 0 and lay[o] > 0 for o in ("a_off", "c_off", "res_off")) and lay["ldc"] >= lay["c_off"] + case.ncols + 8
        assert label_of(capi, case._replace(strided=False), capi.CA_F16) == case.label    # the offsets do not change the plan


def test_the_argument_builder_passes_every_epilogue_field_on(capi):
    """alpha, post, act and out_f32 reach the query: each moves a launch off a kernel that does not implement it."""
    ar = next(c for c in R.EXACT_CASES if c.label == "ar128x64")
    assert label_of(capi, ar, capi.CA_F16, alpha=0.5) == "wres160" and label_of(capi, ar, capi.CA_F16, post=0.5) == "wres160"
    assert label_of(capi, ar, capi.CA_F16, act=1) == "wres160" and label_of(capi, ar, capi.CA_F16, out_f32=True) != "ar128x64"
    ps = next(c for c in R.EXACT_CASES if c.label == "ps128x320")
    assert label_of(capi, ps, capi.CA_F16, act=1) != "ps128x320" and label_of(capi, ps, capi.CA_F16, alpha=0.5) == "ps128x320"
    split = next(c for c in R.EXACT_CASES if c.label == "pp128x320_splitk4")
    assert R.plan_name(capi, R.gemm_args(capi, split, capi.CA_F16)) == "128x64_r3"   # without the workspace: unsplit


def test_exact_cases_cover_every_plan_the_planner_can_label():
    """One or more exact cases per kind of plan_label (csrc/ca_gemm_plan.h), split-K counts ignored.  The kinds are read from the
    source: a fourteenth plan added there later must come with a case here."""
    thirteen = {"wres160", "ar128x64", "pq256x320", "ps128x320", "pp128x320", "pp128x320_splitkS", "128x128", "128x160", "128x64", "128x64_r3",
                "128x128_splitkS", "reg_128x64", "reg_128x128"}
    assert R.KINDS == thirteen, (sorted(R.KINDS - thirteen), sorted(thirteen - R.KINDS))
    src = open(PLAN_H).read()
    body = src[src.index("inline void plan_label("):]
    body = body[:body.index("\n}\n")]
    formats = re.findall(r'case (PK_\w+): snprintf\(buf, len, "([^"]*)"', body)
    assert len(formats) == 9 and len({k for k, _ in formats}) == 9, formats   # every PlanKind has one format
    kinds_src = set(re.findall(r"\b(PK_[A-Z0-9_]+)\b", src))
    assert kinds_src == {k for k, _ in formats}, sorted(kinds_src ^ {k for k, _ in formats})
    can = set()
    for k, f in formats:
        if k == "PK_DMA":
            can |= {"128x160", "128x128", "128x64", "128x64_r3"}      # (128x128 implies >= 512 blocks: never the three-stage ring)
        elif k == "PK_REG":
            can |= {"reg_128x64", "reg_128x128"}
        else:
            can.add(f.replace("%d", "S"))
    assert can == R.KINDS, (sorted(can - R.KINDS), sorted(R.KINDS - can))
    import test_dispatch_plan   # ... and the dense labels that file lists are the same kinds ("wino_pq256x320" is a convolution's)
    assert {R.kind(l) for l in test_dispatch_plan.PLAN_LABELS} - {"wino_pq256x320"} == R.KINDS


# ---- the operand assertions hold where the GPU tests rely on them
@functools.lru_cache(maxsize=None)
def _ops(case):
    return R.integer_operands(case)


def test_integer_operands_are_what_the_argument_assumes():
    case = R.EXACT_CASES[0]._replace(ln="stats")
    ops = _ops(case)
    for name, lo, hi in (("a", -1, 1), ("w", -1, 1), ("bias", -3, 3), ("rowbias", -3, 3), ("residual", -8, 8)):
        t = ops[name]
        assert t.dtype == torch.float32 and (t == t.round()).all() and t.min() == lo and t.max() == hi, name
        assert torch.equal(t.half().float(), t) and torch.equal(t.bfloat16().float(), t)
    nz = (ops["a"] != 0).float().mean().item()
    assert 0.24 < nz < 0.26 and abs(ops["a"].mean().item()) < 0.01, nz
    assert tuple(ops["rowbias"].shape) == (171, 320) and ops["rows_per_group"] == 96 and ops["alpha"] == 2.0
    st, cs = ops["ln"]
    assert set(st[:, 0].tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0} and set(st[:, 1].tolist()) == {0.5, 1.0, 2.0} and torch.equal(cs, ops["w"].sum(1))
    two = _ops(R.SMALLEST)
    assert two["a2"].shape == (300, 64) and set(two["a2"].unique().tolist()) == {-1.0, 0.0, 1.0}


@pytest.mark.parametrize("case", R.EXACT_CASES, ids=lambda c: c.id)
def test_exactness_conditions_hold_at_every_case_of_the_gpu_tests(case):
    """exact_result() asserts them in both dtypes; fp32 accumulation (what the kernels do) gives the numbers fp64 gives; the stored result
    read back is the unrounded one."""
    ops = _ops(case)
    pre = R.exact_before_residual(ops, case, acc=torch.float32)
    parts = (4 if case.label == "pq256x320" else 1) * case.n // 320 if case.row_sums else 0
    final = (pre + ops["residual"] if ops["residual"] is not None else pre) * ops["post_scale"]
    for dt in (F16, BF16):
        y, sums = R.exact_result(ops, case, dt, pre=pre, parts=parts)
        assert y.dtype == (torch.float32 if case.out_f32 else dt) and torch.equal(y.float(), final)
        if parts:
            t = final.reshape(case.m, parts, -1)
            assert sums.dtype == torch.float32 and torch.equal(sums[..., 0], t.sum(2)) and torch.equal(sums[..., 1], (t * t).sum(2))
    if case.m * case.n * (case.k1 + case.k2) < 2e9:    # (the small ones once more in fp64)
        assert torch.equal(R.exact_before_residual(ops, case, acc=torch.float64).float(), pre)


def test_a_case_that_breaks_a_bound_fails_its_own_assertion():
    case = R.SMALLEST._replace(residual=True, strided=False)
    ops = _ops(case)
    R.exact_result(ops, case, BF16)
    res = ops["residual"].clone()
    res[0, 0] = 257 - R.exact_before_residual(ops, case)[0, 0].float()
    with pytest.raises(AssertionError, match="the result reaches"):        # 257 is no bf16 number
        R.exact_result(dict(ops, residual=res), case, BF16)
    with pytest.raises(AssertionError, match="before the residual reaches"):
        R.exact_result(dict(ops, bias=torch.full((case.n,), 2051.0)), case, F16)
    with pytest.raises(AssertionError, match="a is not a multiple"):
        R.exact_result(dict(ops, a=ops["a"] * 0.3), case, F16)
    with pytest.raises(AssertionError, match="colsum"):
        lnc = case._replace(ln="stats")
        o = _ops(lnc)
        R.exact_result(dict(o, ln=(o["ln"][0], o["ln"][1] + 1)), lnc, F16)
    with pytest.raises(AssertionError, match="sum of squares"):            # 24 x 900^2 > 2^24
        R.exact_result(dict(ops, residual=None), case, F16, parts=1, pre=torch.full((case.m, case.n), 900.0, dtype=torch.float64))


# ---- the comparison rejects the errors it is there for: the smallest case, with a row bias per 7 rows and a residual
WRONG = R.SMALLEST._replace(bias=True, rowbias=7, residual=True, strided=False)


def _right():
    ops = _ops(WRONG)
    return ops, R.exact_result(ops, WRONG, F16)[0]


def _ref(ops, **over):
    kw = dict(a2=ops["a2"], bias=ops["bias"], rowbias=ops["rowbias"], rows_per_group=ops["rows_per_group"], residual=ops["residual"])
    kw.update(over)
    a, w = kw.pop("a", ops["a"]), kw.pop("w", ops["w"])
    return R.gemm_ref(a, w, **kw)


def _rejected(wrong, right, what):
    with pytest.raises(AssertionError) as e:
        R.assert_same(wrong, right, what)
    msg = str(e.value)
    n = int((wrong != right).sum())
    assert n > 0 and f"{what}: {n} of {right.numel()} elements in {int((wrong != right).any(1).sum())} rows differ; first at (row " in msg, msg
    return msg


def test_checker_accepts_the_right_result_and_reports_the_first_difference():
    ops, right = _right()
    assert torch.equal(_ref(ops).half(), right)
    R.assert_same(right.clone(), right, "same")
    wrong = right.clone()
    wrong[130, 17] += 1
    wrong[299, 0] += 1
    msg = _rejected(wrong, right, "poked")
    assert "2 of 7200 elements in 2 rows differ; first at (row 130, column 17)" in msg
    nan = right.clone()
    nan[0, 0] = float("nan")
    with pytest.raises(AssertionError, match="1 of 7200"):
        R.assert_same(nan, right, "nan")
    with pytest.raises(AssertionError, match="float32"):
        R.assert_same(right.float(), right, "dtype")


def test_checker_rejects_a_row_bias_group_index_off_by_one():
    ops, right = _right()
    msg = _rejected(_ref(ops, rb_shift=1).half(), right, "row bias off by one")
    assert "first at (row 6, " in msg, msg                       # the last row of group 0 takes group 1's bias
    assert int((_ref(ops, rb_shift=1).half() != right).any(1).sum()) <= 300 // 7


def test_checker_rejects_a_k_tile_dropped_in_the_last_rows_only():
    """A ragged tile whose last 8 rows miss the last 64-column K tile: 8 rows of 300."""
    ops, right = _right()
    y = _ref(ops)
    y[-8:] = _ref(ops, a2=ops["a2"] * 0)[-8:]
    msg = _rejected(y.half(), right, "dropped K tile")
    assert "first at (row 292, " in msg and int((y.half() != right).any(1).sum()) <= 8, msg


def test_checker_rejects_the_two_sources_swapped():
    ops, right = _right()
    _rejected(_ref(ops, a=ops["a2"], a2=ops["a"]).half(), right, "a and a2 swapped")


def test_checker_rejects_stale_ragged_rows():
    """The last tile's 44 rows never stored: whatever the buffer held (here the sentinel of the GPU test)."""
    ops, right = _right()
    y = right.clone()
    y[256:] = -77.0
    msg = _rejected(y, right, "stale rows")
    assert "first at (row 256, column 0)" in msg


def test_checker_rejects_a_transposed_16x16_sub_tile():
    ops, right = _right()
    y = right.clone()
    y[128:144, 0:16] = right[128:144, 0:16].t()
    msg = _rejected(y, right, "transposed sub-tile")
    assert int((y != right).any(1).sum()) <= 16


def test_checker_rejects_a_residual_read_with_the_wrong_leading_dimension():
    ops, right = _right()
    m, n = ops["residual"].shape
    flat = ops["residual"].flatten()
    idx = (torch.arange(m)[:, None] * (n + 8) + torch.arange(n)[None, :]) % flat.numel()
    msg = _rejected(_ref(ops, residual=flat[idx]).half(), right, "residual leading dimension")
    assert "first at (row 1, " in msg, msg                       # row 0 is still right
