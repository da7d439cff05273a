"""CPU: the convolution restatement the rectangular-latent parity tests trust (tests/conv_ref.py, used by
tests/test_rect_latents_gpu.py): it equals torch's conv2d in fp64, its integer operands satisfy the exactness conditions at every
shape those tests use, and its comparison REJECTS the three index errors the tests are there to catch -- shown here on wrong
references, so that a green GPU run means the kernels do not make them."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as R  # noqa: E402

ALL_CASES = R.DIRECT_CASES + R.WINO_CASES + R.UP2_CASES


def _torch_conv(x, w, *, x2=None, stride=1, upsample=False, pad_asym=False):
    """F.conv2d on NHWC operands, in their dtype."""
    xin = (x if x2 is None else torch.cat([x, x2], 3)).permute(0, 3, 1, 2)
    if upsample:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    xin = F.pad(xin, (0, 1, 0, 1)) if pad_asym else F.pad(xin, (1, 1, 1, 1))
    return F.conv2d(xin, w.permute(0, 3, 1, 2), stride=stride).permute(0, 2, 3, 1)


# images, h, w, c1, c2, cout, stride, upsample, pad_asym, epilogue (images per row-bias group)
RANDOM_CASES = [(3, 6, 10, 8, 0, 16, 1, False, False, 0), (3, 10, 6, 8, 8, 16, 1, False, False, 1), (2, 9, 7, 8, 0, 8, 2, False, False, 0),
                (4, 6, 10, 16, 0, 8, 2, False, True, 2), (2, 5, 7, 8, 8, 8, 1, True, False, 1), (3, 7, 4, 8, 0, 8, 2, True, False, 0)]


@pytest.mark.parametrize("case", RANDOM_CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_restatement_equals_conv2d_in_fp64(case):
    images, h, w_, c1, c2, cout, stride, ups, asym, epi = case
    g = torch.Generator().manual_seed(h * 100 + w_)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, x2, w = rn(images, h, w_, c1), (rn(images, h, w_, c2) if c2 else None), rn(cout, 3, 3, c1 + c2)
    want = _torch_conv(x, w, x2=x2, stride=stride, upsample=ups, pad_asym=asym)
    got = R.conv_ref(x, w, x2=x2, stride=stride, upsample=ups, pad_asym=asym)
    assert got.shape == want.shape and (got - want).abs().max().item() < 1e-12
    assert tuple(got.shape[1:3]) == R.Case("", images, h, w_, c1, c2, cout, stride, ups, asym).out_hw()
    if epi:
        ho, wo = got.shape[1:3]
        bias, rb, res = rn(cout), rn(-(-images // epi), cout), rn(images, ho, wo, cout)
        got = R.conv_ref(x, w, x2=x2, stride=stride, upsample=ups, pad_asym=asym, bias=bias, rowbias=rb, rows_per_group=epi * ho * wo,
                         residual=res, alpha=0.75, post_scale=0.5, act=1, round_to=torch.float16)
        y = (want + bias + rb.repeat_interleave(epi, 0)[:images, None, None, :]) * 0.75
        y = F.silu((y.half().double() + res) * 0.5)
        assert (got - y).abs().max().item() < 1e-12


@functools.lru_cache(maxsize=None)
def _ops(case):
    return R.integer_operands(case)


def test_integer_operands_are_what_the_argument_assumes():
    ops = _ops(R.DIRECT_CASES[1])
    for name, lo, hi in (("x", -1, 1), ("x2", -1, 1), ("w", -1, 1), ("bias", -3, 3), ("rowbias", -3, 3), ("residual", -8, 8)):
        t = ops[name]
        assert t.dtype == torch.float32 and (t == t.round()).all() and t.min() == lo and t.max() == hi, name
        assert torch.equal(t.half().float(), t) and torch.equal(t.bfloat16().float(), t)
    nz = (ops["x"] != 0).float().mean().item()
    assert 0.24 < nz < 0.26, nz
    assert tuple(ops["rowbias"].shape) == (11, 640) and ops["rows_per_group"] == 2 * 32 * 48


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.id)
def test_exactness_conditions_hold_at_every_shape_of_the_gpu_tests(case):
    """exact_result() asserts them; fp32 accumulation (what the kernels do) gives the integers fp64 gives; the fp16 result is exact and
    the bf16 one exact up to 256 and one rounding away above."""
    ops = _ops(case)
    pre = R.exact_before_residual(ops, case, acc=torch.float32)
    wino = case.label.startswith("wino")
    y16 = R.exact_result(ops, case, torch.float16, winograd=wino, pre=pre)
    ybf = R.exact_result(ops, case, torch.bfloat16, pre=pre)
    final = pre + ops["residual"] if ops["residual"] is not None else pre
    assert torch.equal(y16.float(), final)
    small = pre.abs() <= 256
    assert torch.equal(ybf.float()[small], pre[small])
    assert ((ybf.float() - pre).abs() <= pre.abs() * 2.0 ** -8).all()
    if case.images * case.h * case.w * (case.c1 + case.c2) * case.cout < 2e9:   # (the small ones once more in fp64, and against conv2d)
        assert torch.equal(R.exact_before_residual(ops, case, acc=torch.float64).float(), pre)
        plain = _torch_conv(ops["x"], ops["w"], x2=ops["x2"], stride=case.stride, upsample=case.upsample, pad_asym=case.pad_asym)
        assert torch.equal(R.conv_ref(ops["x"], ops["w"], x2=ops["x2"], stride=case.stride, upsample=case.upsample, pad_asym=case.pad_asym,
                                      acc=torch.float32), plain)


def test_winograd_products_reassemble_the_convolution():
    """A^T M A of the helper's M is the convolution: the bound on |M| is a bound on what the route really stores."""
    case = R.Case("", 3, 6, 10, 64, 64, 32, wino=True)
    ops = _ops(case)
    m = R.winograd_products(ops["x"], ops["w"], x2=ops["x2"], acc=torch.float64)
    at = torch.tensor([[1.0, 1.0, 1.0, 0.0], [0.0, 1.0, -1.0, -1.0]], dtype=torch.float64)
    y = torch.einsum("ix,xytc,jy->tijc", at, m.reshape(4, 4, -1, case.cout), at)                 # [tiles, 2, 2, cout]
    y = y.reshape(case.images, case.h // 2, case.w // 2, 2, 2, case.cout).permute(0, 1, 3, 2, 4, 5).reshape(case.images, case.h, case.w, case.cout)
    assert torch.equal(y, R.conv_ref(ops["x"], ops["w"], x2=ops["x2"]))
    u = R.winograd_weight(ops["w"])
    assert torch.equal(u * 4, (u * 4).round()) and torch.equal(u.half().float(), u)
    with pytest.raises(AssertionError, match="max \\|M\\|"):   # the condition is checked, not assumed: 256x the operands break it
        big = dict(ops, x=ops["x"] * 256, residual=None)
        R.exact_result(big, case, torch.float16, winograd=True, pre=torch.zeros(1))


# ---- the comparison rejects the index errors it is there for (smallest rectangular shape of the GPU tests, with a row bias per image)
WRONG = R.SMALLEST._replace(epilogue=1)


def _right():
    ops = _ops(WRONG)
    return ops, R.exact_result(ops, WRONG, torch.float16)


def _rejected(wrong, right, what):
    with pytest.raises(AssertionError) as e:
        R.assert_same(wrong, right, what)
    msg = str(e.value)
    n = int((wrong != right).sum())
    assert n > 0 and f"{what}: {n} of {right.numel()} elements differ; first at (image " in msg, msg
    return msg


def test_checker_accepts_the_right_result_and_reports_the_first_difference():
    ops, right = _right()
    R.assert_same(right.clone(), right, "same")
    wrong = right.clone()
    wrong[1, 4, 7, 5] += 1
    wrong[2, 0, 0, 0] += 1
    msg = _rejected(wrong, right, "poked")
    assert "2 of 5760 elements differ; first at (image 1, y 4, x 7, channel 5)" in msg
    nan = right.clone()
    nan[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError, match="1 of 5760"):
        R.assert_same(nan, right, "nan")


def test_checker_rejects_rows_decomposed_with_h_and_w_swapped():
    """A kernel that splits the flat row index by (W, H) instead of (H, W) convolves the same memory as a W x H image."""
    ops, right = _right()
    c = WRONG
    swapped = c._replace(h=c.w, w=c.h)
    turned = dict(ops, x=ops["x"].reshape(c.images, c.w, c.h, c.c1), residual=ops["residual"].reshape(c.images, c.w, c.h, c.cout))
    wrong = R.exact_result(turned, swapped, torch.float16).reshape(right.shape)
    _rejected(wrong, right, "h/w swapped")


def test_checker_rejects_a_right_border_that_wraps_into_the_next_row():
    """A gather without the x < W test reads the first pixel of the next row (flat address + 1) where the zero padding belongs."""
    ops, right = _right()
    c = WRONG
    xp = R.padded_input(ops["x"].double())
    xp[:, 1:c.h, c.w + 1] = ops["x"].double()[:, 1:, 0]        # padded row y + 1 (image row y), column W  <-  image row y + 1, column 0
    y = R.epilogue(R.conv_taps(xp, ops["w"].double()), bias=ops["bias"], rowbias=ops["rowbias"], rows_per_group=ops["rows_per_group"],
                   residual=ops["residual"])
    _rejected(y.half(), right, "wrapped border")


def test_checker_rejects_a_row_bias_group_index_off_by_one_row():
    ops, right = _right()
    y = R.epilogue(R.conv_taps(R.padded_input(ops["x"].double()), ops["w"].double()), bias=ops["bias"], rowbias=ops["rowbias"],
                   rows_per_group=ops["rows_per_group"], residual=ops["residual"], rb_shift=1)
    msg = _rejected(y.half(), right, "row bias off by one")
    assert "first at (image 0, y 5, x 9," in msg, msg            # the last pixel of image 0 takes image 1's bias
    assert int((y.half() != right).any(-1).sum()) == 2          # ... and the last pixel of image 1; image 2's is clamped
