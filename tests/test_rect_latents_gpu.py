"""GPU: convolution and GroupNorm parity at the rectangular latents of the 512x768 and 768x768 workloads (64x96 .. 8x12, 96x96 .. 12x12)
on the kernels those sizes actually reach.  Every big convolution kernel turns a flat row index into (image, y, x) with its own copy of
the arithmetic -- k_gemm_pq MODE 1, ca_gemm_pp2.h / ca_gemm_ps.h, k_gemm_dma MODE 1, k_wino_in / k_wino_out, the slab walk of
k_gn_small_wino -- and on a square image H and W swapped anywhere in it is invisible.

Two tests per case (the table is tests/conv_ref.py's, shared with the CPU tests):
  exact     integer-valued operands (conv_ref.integer_operands): every accumulation order gives the same integers, so the result must
            equal conv_ref's number for number, twice.  One dropped or misplaced tap fails it; tests/test_conv_ref_cpu.py shows the
            comparison rejecting an H / W swap, a wrapping border and a row-bias group off by one.
  rounding  Gaussian operands as in test_kernels_gpu.py::test_conv3x3 against fp32 torch, with that file's tolerances.
Every case records the plan label of its launch and asserts it, so a later dispatch change cannot quietly move it onto another kernel.

GroupNorm: group_norm_conv3x3_wino at 8x12 and 12x12 latents, and every GroupNorm path on inputs whose group mean is 0, 4 and 16 times
the group's standard deviation (all paths compute the variance as E[x^2] - mean^2 from fp32 sums: the cancellation is exercised here)."""
import contextlib
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import conv_ref as R  # noqa: E402
from test_kernels_gpu import DEV, close  # noqa: E402

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
NAME = {F16: "fp16", BF16: "bf16"}


def _k():
    from controlanimate_amd import kernels
    return kernels


@contextlib.contextmanager
def planned(*labels):
    """The launches inside run on exactly these kernels."""
    K = _k()
    K._plan_sink = seen = []
    try:
        yield
        torch.cuda.synchronize()
    finally:
        K._plan_sink = None
    assert seen == list(labels), f"planned {labels}, ran {seen}"


def rel_l2(y, ref):
    return ((y.float() - ref).norm() / ref.norm()).item()


def both(cases, dtypes=(F16, BF16)):
    """(case, dtype) pairs, the dtypes of one case next to each other (they share its operands and reference)."""
    return pytest.mark.parametrize("case,dtype", [(c, dt) for c in cases for dt in dtypes], ids=[f"{c.id}-{NAME[dt]}" for c in cases for dt in dtypes])


# ------------------------------------------------------------------------------------ exact: integer operands
@functools.lru_cache(maxsize=2)
def integer_case(case):
    """Integer operands on the device (fp32) and conv + bias + row bias of them in fp64.  Never modified afterwards."""
    ops = {n: (t.to(DEV) if torch.is_tensor(t) else t) for n, t in R.integer_operands(case).items()}
    return ops, R.exact_before_residual(ops, case)


def launch_conv(case, ops, dtype, *, residual=True, winograd=None):
    cast = lambda t: None if t is None else t.to(dtype)
    winograd = case.wino if winograd is None else winograd
    return _k().conv3x3(cast(ops["x"]), cast(ops["w"]), x2=cast(ops["x2"]), bias=ops["bias"], rowbias=ops["rowbias"], rows_per_group=ops["rows_per_group"],
                        residual=cast(ops["residual"]) if residual else None, stride=case.stride, upsample=case.upsample, pad_asym=case.pad_asym,
                        w_wino=cast(R.winograd_weight(ops["w"])) if winograd else None)


@both(R.DIRECT_CASES)
def test_direct_plans_are_exact_on_integer_operands(case, dtype):
    ops, pre = integer_case(case)
    want = R.exact_result(ops, case, dtype, pre=pre)
    res = dtype == F16          # (bf16 would round the value before the residual once more: conv_ref's docstring)
    with planned(case.label, case.label):
        y, again = launch_conv(case, ops, dtype, residual=res), launch_conv(case, ops, dtype, residual=res)
    R.assert_same(y, want, f"{case.id} {NAME[dtype]}")
    assert torch.equal(y, again), "two launches on the same inputs differ"


@pytest.mark.parametrize("case", R.WINO_CASES, ids=lambda c: c.id)
def test_winograd_route_is_exact_on_integer_operands(case):
    """fp16: V, U and the sixteen products are fp16 numbers (exact_result asserts max |M| < 512 on the operands), so F(2x2, 3x3) has no
    rounding freedom either."""
    ops, pre = integer_case(case)
    want = R.exact_result(ops, case, F16, winograd=True, pre=pre)
    with planned(case.label, case.label):
        y, again = launch_conv(case, ops, F16), launch_conv(case, ops, F16)
    R.assert_same(y, want, f"{case.id} fp16")
    assert torch.equal(y, again), "two launches on the same inputs differ"


@both(R.UP2_CASES)
def test_phase_form_is_exact_on_integer_operands(case, dtype):
    """ca_conv_up2_phase: the combined weights are sums of at most four taps -- small integers, exact in both dtypes."""
    from controlanimate_amd.layers import phase_weights
    k = _k()
    ops, pre = integer_case(case)
    want = R.exact_result(ops, case, dtype, pre=pre)
    wp = phase_weights(ops["w"].permute(0, 3, 1, 2).contiguous())
    assert float(wp.abs().max()) <= 4 and torch.equal(wp, wp.round())
    x, wp = ops["x"].to(dtype), wp.to(dtype)
    assert k.conv_up2_phase_supported(x, wp) == (case is R.UP2_CASES[0])
    with planned(case.label, case.label):
        y, again = k.conv_up2_phase(x, wp), k.conv_up2_phase(x, wp)
    R.assert_same(y, want, f"{case.id} {NAME[dtype]}")
    assert torch.equal(y, again), "two launches on the same inputs differ"


# ------------------------------------------------------------------------------------ rounding: Gaussian operands
def gaussian_operands(case, dtype):
    """As test_kernels_gpu.py::test_conv3x3: N(0, 1) activations, weights scaled by (9 cin)^-1/2, all rounded to the dtype."""
    g = torch.Generator().manual_seed(100 * case.h + case.w + case.c1)
    cin = case.c1 + case.c2
    ho, wo = case.out_hw()
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(DEV)
    d = dict(x=rn(case.images, case.h, case.w, case.c1).to(dtype), x2=rn(case.images, case.h, case.w, case.c2).to(dtype) if case.c2 else None,
             w=rn(case.cout, 3, 3, cin, scale=(9 * cin) ** -0.5).to(dtype), bias=None, rowbias=None, residual=None, rows_per_group=0)
    if case.epilogue:
        d.update(bias=rn(case.cout), rowbias=rn(-(-case.images // case.epilogue), case.cout), residual=rn(case.images, ho, wo, case.cout).to(dtype),
                 rows_per_group=case.rows_per_group())
    return d


def conv2d_reference(d, case, dtype):
    """fp32 F.conv2d on the device; the epilogue in the order of tools/ps_check.conv_reference."""
    xin = (d["x"] if d["x2"] is None else torch.cat([d["x"], d["x2"]], 3)).float().permute(0, 3, 1, 2).contiguous()   # (NCHW in memory)
    if case.upsample:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    xin = F.pad(xin, (0, 1, 0, 1)) if case.pad_asym else F.pad(xin, (1, 1, 1, 1))
    y = F.conv2d(xin, d["w"].float().permute(0, 3, 1, 2).contiguous(), stride=case.stride).permute(0, 2, 3, 1)
    return R.epilogue(y, bias=d["bias"], rowbias=d["rowbias"], rows_per_group=d["rows_per_group"], residual=d["residual"], round_to=dtype)


@both(R.DIRECT_CASES)
def test_direct_plans_against_fp32_torch(case, dtype):
    d = gaussian_operands(case, dtype)
    with planned(case.label):
        y = launch_conv(case, d, dtype)
    ref = conv2d_reference(d, case, dtype)
    assert tuple(y.shape) == (case.images, *case.out_hw(), case.cout) and y.dtype == dtype
    if case.label == "pq256x320":   # the bound of test_gemm_and_conv_256x320_streaming_kernel
        rel = rel_l2(y, ref)
        print(f"{case.id} {NAME[dtype]}: rel-L2 {rel:.3e}")
        assert torch.isfinite(y.float()).all() and rel < (2.5e-3 if dtype == F16 else 1.5e-2), rel
    else:
        close(y, ref.cpu(), dtype, case.id)


@both(R.WINO_CASES)
def test_winograd_route_against_fp32_torch(case, dtype):
    """The bounds of test_kernels_gpu.py::test_conv3x3_winograd: rel-L2 < 3e-3 in fp16; < 1.2e-2 and < 5x the direct form's in bf16."""
    import wino_check as W
    k = _k()
    d = W.make(case.images, case.h, case.c1, case.c2, case.cout, dt=dtype, epilogue=bool(case.epilogue), w=case.w)
    assert d["rows_per_group"] == case.rows_per_group()
    kw = dict(x2=d["x2"], bias=d["bias"], rowbias=d["rowbias"], rows_per_group=d["rows_per_group"], residual=d["residual"], post_scale=d["post"],
              upsample=case.upsample)
    with planned(case.label):
        y = k.conv3x3(d["x"], d["w"], w_wino=d["u"], **kw)
    k._plan_sink = labels = []
    try:
        direct = k.conv3x3(d["x"], d["w"], **kw)
    finally:
        k._plan_sink = None
    assert len(labels) == 1 and not labels[0].startswith("wino"), labels
    if case.upsample:
        up = F.interpolate(d["x"].float().permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest")
        ref = F.conv2d(up, d["w"].float().permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
    else:
        ref = W.reference(d)
    assert tuple(y.shape) == tuple(ref.shape)
    rel, rel_d = rel_l2(y, ref), rel_l2(direct, ref)
    print(f"{case.id} {NAME[dtype]}: rel-L2 {rel:.3e} (direct form {rel_d:.3e})")
    assert torch.isfinite(y.float()).all()
    if dtype == F16:
        assert rel < 3e-3, (rel, rel_d)
    else:
        assert rel < 1.2e-2 and rel < 5 * rel_d, (rel, rel_d)


@both(R.UP2_CASES)
def test_phase_form_against_fp32_torch_and_the_existing_path(case, dtype):
    """The yardstick and bounds of test_conv_up2_phase_gpu.py: fp32 torch on x and the ORIGINAL 3x3 weights, both rounded to the dtype; the
    phase form at most 1.5x as far from it as conv3x3(upsample=True), max-abs and rel-L2."""
    from controlanimate_amd.layers import phase_weights
    k = _k()
    g = torch.Generator().manual_seed(1000 * case.h + 10 * case.w + case.c1 // 64)
    x = torch.randn(case.images, case.h, case.w, case.c1, generator=g).to(dtype).to(DEV)
    w16 = (torch.randn(case.cout, case.c1, 3, 3, generator=g) * (9 * case.c1) ** -0.5).to(dtype)
    wk = w16.permute(0, 2, 3, 1).contiguous().to(DEV)
    wp = phase_weights(w16.float()).to(dtype).to(DEV)                     # fp32 sums of the rounded taps, rounded once
    bias = (torch.randn(case.cout, generator=g) * 0.5).to(DEV)
    up = F.interpolate(x.float().permute(0, 3, 1, 2).contiguous(), scale_factor=2.0, mode="nearest")
    ref = F.conv2d(up, w16.float().to(DEV), bias=bias, padding=1).permute(0, 2, 3, 1)
    k._plan_sink = labels = []
    try:
        old = k.conv3x3(x, wk, bias=bias, upsample=True)
        new, again = k.conv_up2_phase(x, wp, bias=bias), k.conv_up2_phase(x, wp, bias=bias)
        torch.cuda.synchronize()
    finally:
        k._plan_sink = None
    assert tuple(new.shape) == (case.images, 2 * case.h, 2 * case.w, case.cout) and new.dtype == dtype
    assert labels[1:] == [case.label] * 2 and not labels[0].startswith("up2"), labels
    assert torch.isfinite(new.float()).all()
    ma_old, rl_old = float((old.float() - ref).abs().max()), rel_l2(old, ref)
    ma_new, rl_new = float((new.float() - ref).abs().max()), rel_l2(new, ref)
    msg = f"{case.id} {NAME[dtype]}: max-abs new {ma_new:.3e} vs existing {ma_old:.3e}, rel-L2 new {rl_new:.3e} vs existing {rl_old:.3e}"
    print(msg)
    assert rl_old < (2e-3 if dtype == F16 else 1.2e-2), msg   # (the existing path is where it always was)
    assert ma_new <= 1.5 * ma_old and rl_new <= 1.5 * rl_old, msg
    assert torch.equal(new, again), "two launches on the same inputs differ"


# ------------------------------------------------------------------------------------ GroupNorm into the Winograd input transform
def _gamma_beta(c):
    g = torch.Generator(device="cpu").manual_seed(5)
    return (1.0 + 0.2 * torch.randn(c, generator=g)).to(DEV), (0.1 * torch.randn(c, generator=g)).to(DEV)


@pytest.mark.parametrize("shape", [(32, 8, 12, 1280, 0, 1280), (32, 8, 12, 1280, 1280, 1280), (64, 12, 12, 1280, 0, 1280)], ids=lambda s: "x".join(map(str, s)))
def test_groupnorm_writes_the_winograd_input_transform_of_rectangular_images(shape):
    """As test_kernels_gpu.py::test_groupnorm_writes_the_winograd_input_transform, with wino_h != wino_w: bit-identical to GroupNorm, then
    the Winograd convolution, and within 3e-3 of fp32 torch."""
    import wino_check as W
    k = _k()
    images, h, w_, c1, c2, cout = shape
    d = W.make(images, h, c1, c2, cout, epilogue=True, w=w_)
    gamma, beta = _gamma_beta(c1 + c2)
    with planned("gn_wino_pq256x320"):
        y = k.group_norm_conv3x3_wino(d["x"], gamma, beta, d["w"], d["u"], x2=d["x2"], act=k.ACT_SILU, eps=1e-6, bias=d["bias"], rowbias=d["rowbias"],
                                      rows_per_group=d["rows_per_group"], residual=d["residual"], post_scale=d["post"])
        assert y is not None
    hn = k.group_norm(d["x"], gamma, beta, x2=d["x2"], eps=1e-6, act=k.ACT_SILU)
    with planned("wino_pq256x320"):
        two = k.conv3x3(hn, d["w"], bias=d["bias"], rowbias=d["rowbias"], rows_per_group=d["rows_per_group"], residual=d["residual"],
                        post_scale=d["post"], w_wino=d["u"])
    assert torch.equal(y, two), f"{int((y != two).sum())} of {y.numel()} elements differ"
    xin = d["x"].float() if d["x2"] is None else torch.cat([d["x"].float(), d["x2"].float()], dim=-1)
    ref_h = F.silu(F.group_norm(xin.permute(0, 3, 1, 2), 32, gamma, beta, 1e-6)).permute(0, 2, 3, 1)
    ref = W.reference(dict(d, x=ref_h.to(torch.float16), x2=None))
    assert rel_l2(y, ref) < 3e-3


@pytest.mark.parametrize("shape", [(8, 16, 24, 1280, 0, 1280), (32, 8, 12, 1280, 640, 1280)], ids=lambda s: "x".join(map(str, s)))
def test_groupnorm_into_winograd_declines_what_it_cannot_take(shape):
    """384 pixels are more than the 256 the slab holds; 60 channels per group (C = 1920) are not whole 16-byte chunks."""
    import wino_check as W
    k = _k()
    images, h, w_, c1, c2, cout = shape
    d = W.make(images, h, c1, c2, cout, epilogue=False, w=w_)
    gamma, beta = torch.ones(c1 + c2, device=DEV), torch.zeros(c1 + c2, device=DEV)
    assert k.group_norm_conv3x3_wino(d["x"], gamma, beta, d["w"], d["u"], x2=d["x2"], act=k.ACT_SILU) is None


# ------------------------------------------------------------------------------------ GroupNorm under an offset
# one shape per path (images, h, w, c): k_gn_small, k_gn_unit<5>, k_gn_unit<20>, statistics + apply
OFFSET_SHAPES = [(2, 8, 12, 1280), (2, 16, 24, 640), (2, 32, 48, 640), (2, 64, 96, 320)]
RATIOS = [0, 4, 16]
# (std, so that the dtype still resolves the spread at mean = 16 std: 8 in fp16 has a spacing of 2^-7, 32 in bf16 one of 2^-2)
STD = {F16: 0.5, BF16: 2.0}


def offset_input(shape, dtype, ratio, seed=31):
    """N(ratio * std, std) in fp32, rounded to the dtype; asserts that the rounded input's own group std is within 10 % of `std`."""
    images, h, w_, c = shape
    std = STD[dtype]
    g = torch.Generator().manual_seed(seed + ratio)
    x = (torch.randn(images, h, w_, c, generator=g) * std + ratio * std).to(dtype)
    grp = x.double().reshape(images, h * w_, 32, c // 32).permute(0, 2, 1, 3).reshape(images, 32, -1)
    sd, mean = grp.std(-1, unbiased=False), grp.mean(-1)
    assert ((sd - std).abs() < 0.1 * std).all() and ((mean - ratio * std).abs() < 0.1 * std).all()
    return x


def distances(y, truth):
    d = y.double() - truth
    return (d.norm() / truth.norm()).item(), d.abs().max().item()


def assert_as_close_as_fp32_torch(y_kernel, y_yard, truth, what):
    """rel-L2 and max-abs distance from the fp64 truth at most 1.5x those of fp32 torch rounded to the dtype (the margin of the suite's
    other two-path comparisons: it covers one differing rounding)."""
    rk, mk = distances(y_kernel, truth)
    ry, my = distances(y_yard, truth)
    msg = f"{what}: kernel rel-L2 {rk:.3e} max-abs {mk:.3e}; fp32 torch rel-L2 {ry:.3e} max-abs {my:.3e}"
    print(msg)
    assert torch.isfinite(y_kernel.float()).all(), what
    assert rk <= 1.5 * ry and mk <= 1.5 * my, msg


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape", OFFSET_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_groupnorm_with_group_mean_far_from_zero(shape, dtype, ratio):
    """mean = 0, 4, 16 group standard deviations: E[x^2] - mean^2 loses (1 + ratio^2) of the sums' precision.  Truth: F.group_norm in fp64
    on the rounded input; yardstick: F.group_norm in fp32 on the same input, rounded to the dtype."""
    k = _k()
    c = shape[3]
    x = offset_input(shape, dtype, ratio)
    gamma, beta = _gamma_beta(c)
    xd = x.to(DEV)
    truth = F.group_norm(xd.double().permute(0, 3, 1, 2), 32, gamma.double(), beta.double(), 1e-5).permute(0, 2, 3, 1)
    yard = F.group_norm(xd.float().permute(0, 3, 1, 2), 32, gamma, beta, 1e-5).permute(0, 2, 3, 1).to(dtype)
    y = k.group_norm(xd, gamma, beta, eps=1e-5)
    torch.cuda.synchronize()
    assert_as_close_as_fp32_torch(y, yard, truth, f"groupnorm {shape} {NAME[dtype]} mean = {ratio} std")
    assert torch.equal(y, k.group_norm(xd, gamma, beta, eps=1e-5))


@pytest.mark.parametrize("ratio", RATIOS)
def test_groupnorm_into_winograd_with_group_mean_far_from_zero(ratio):
    """The wino_v path (k_gn_small_wino) at (32, 8, 12, 1280 -> 1280): its output is the convolution's, so kernel and yardstick go through
    the SAME Winograd convolution -- the fused launch against conv3x3(w_wino) of fp32 torch's GroupNorm + SiLU rounded to fp16 -- and are
    measured against fp64 GroupNorm + SiLU + convolution; what differs between them is the GroupNorm alone.  The fused form stays
    bit-identical to group_norm followed by conv3x3(w_wino), so the statistics are k_gn_small's."""
    import wino_check as W
    k = _k()
    images, h, w_, c, cout = 32, 8, 12, 1280, 1280
    d = W.make(images, h, c, 0, cout, epilogue=False, w=w_)
    x = offset_input((images, h, w_, c), F16, ratio).to(DEV)
    gamma, beta = _gamma_beta(c)
    with planned("gn_wino_pq256x320"):
        y = k.group_norm_conv3x3_wino(x, gamma, beta, d["w"], d["u"], act=k.ACT_SILU, eps=1e-5)
        assert y is not None
    two = k.conv3x3(k.group_norm(x, gamma, beta, eps=1e-5, act=k.ACT_SILU), d["w"], w_wino=d["u"])
    assert torch.equal(y, two), f"{int((y != two).sum())} of {y.numel()} elements differ"
    yard_h = F.silu(F.group_norm(x.float().permute(0, 3, 1, 2), 32, gamma, beta, 1e-5)).permute(0, 2, 3, 1).contiguous().to(F16)
    with planned("wino_pq256x320"):
        yard = k.conv3x3(yard_h, d["w"], w_wino=d["u"])
    truth_h = F.silu(F.group_norm(x.double().permute(0, 3, 1, 2), 32, gamma.double(), beta.double(), 1e-5)).permute(0, 2, 3, 1)
    truth = R.conv_ref(truth_h, d["w"])
    assert_as_close_as_fp32_torch(y, yard, truth, f"groupnorm -> winograd mean = {ratio} std")
