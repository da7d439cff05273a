"""GPU: ca_conv_up2_phase -- conv3x3(nearest_x2(x)) as four 2x2 phase convolutions in one launch of the 256 x 320 kernel.

Yardstick: fp32 torch (F.interpolate + F.conv2d) on the operands the existing path consumes -- x and the ORIGINAL 3x3 weights, both
rounded to fp16 / bf16.  The existing path, ca_conv3x3(upsample=1), is held to the same yardstick in the same test, and the phase
form may be at most 1.5x as far from it (max-abs and rel-L2): its weights are the fp32 sums of those rounded taps rounded once more,
which is the one rounding the margin covers.

Shapes: the smallest at which the kernel can still go wrong -- a phase of 64 rows (every tile partial), a non-square image whose
180-row phases cross image boundaries inside a tile, four whole tiles per phase with two column tiles, and an 80-tile K loop with
cin != cout.  Operands, yardstick and both results are computed once per (shape, dtype, bias) and shared.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (images, source H, source W, cin, cout)
SHAPES = [(1, 8, 8, 320, 320), (3, 6, 10, 320, 320), (4, 16, 16, 640, 640), (2, 8, 8, 1280, 640)]
DTYPES = [torch.float16, torch.bfloat16]


def _k():
    from controlanimate_amd import kernels
    return kernels


@functools.lru_cache(maxsize=None)
def case(shape, dtype, with_bias, scale=1.0):
    """Operands, the fp32 yardstick, the existing path's result and the phase form's (twice).  Never modified afterwards."""
    from controlanimate_amd.layers import phase_weights
    k = _k()
    images, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(1000 * h + 10 * w + cin // 64 + (7 if with_bias else 0))
    x = (torch.randn(images, h, w, cin, generator=g) * scale).to(dtype).to(DEV)
    w32 = torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5
    w16 = w32.to(dtype)                                                   # the original 3x3 weights as the existing path stores them
    wk = w16.permute(0, 2, 3, 1).contiguous().to(DEV)                     # [Cout, kh, kw, Cin]
    wp = phase_weights(w16.float()).to(dtype).to(DEV)                     # fp32 sums of those taps, rounded once
    bias = (torch.randn(cout, generator=g) * 0.5 * scale).to(DEV) if with_bias else None
    up = F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest")
    ref = F.conv2d(up, w16.float().to(DEV), bias=bias, padding=1).permute(0, 2, 3, 1).contiguous()
    k._plan_sink = labels = []
    try:
        old = k.conv3x3(x, wk, bias=bias, upsample=True)
        new = k.conv_up2_phase(x, wp, bias=bias)
        again = k.conv_up2_phase(x, wp, bias=bias)
    finally:
        k._plan_sink = None
    torch.cuda.synchronize()
    return dict(x=x, wk=wk, wp=wp, bias=bias, ref=ref, old=old, new=new, again=again, labels=labels)


def errors(y, ref):
    d = y.float() - ref
    return float(d.abs().max()), float(d.norm() / ref.norm())


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_phase_form_against_fp32_and_the_existing_path(shape, dtype, with_bias):
    c = case(shape, dtype, with_bias)
    images, h, w, cin, cout = shape
    assert tuple(c["new"].shape) == (images, 2 * h, 2 * w, cout) and c["new"].dtype == dtype
    assert c["labels"][1:] == ["up2_pq256x320"] * 2 and not c["labels"][0].startswith("up2"), c["labels"]
    assert torch.isfinite(c["new"].float()).all()
    ma_old, rl_old = errors(c["old"], c["ref"])
    ma_new, rl_new = errors(c["new"], c["ref"])
    msg = f"{shape} {dtype} bias={with_bias}: max-abs new {ma_new:.3e} vs existing {ma_old:.3e}, rel-L2 new {rl_new:.3e} vs existing {rl_old:.3e}"
    print(msg)
    assert rl_old < (2e-3 if dtype == torch.float16 else 1.2e-2), msg   # (the existing path is where it always was)
    assert ma_new <= 1.5 * ma_old and rl_new <= 1.5 * rl_old, msg
    assert torch.equal(c["new"], c["again"]), "two launches on the same inputs differ"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_large_magnitude_inputs_do_not_overflow(dtype):
    """Inputs x 64 (|x| up to ~300): a combined weight is a sum of up to four taps and the accumulators are fp32, so nothing can
    overflow that the existing path does not overflow; same bound as at unit scale."""
    c = case(SHAPES[2], dtype, True, 64.0)
    assert float(c["x"].float().abs().max()) > 200.0 and float(c["ref"].std()) > 30.0
    assert torch.isfinite(c["new"].float()).all() and torch.isfinite(c["old"].float()).all()
    ma_old, rl_old = errors(c["old"], c["ref"])
    ma_new, rl_new = errors(c["new"], c["ref"])
    msg = f"x64 {dtype}: max-abs new {ma_new:.3e} vs existing {ma_old:.3e}, rel-L2 new {rl_new:.3e} vs existing {rl_old:.3e}"
    print(msg)
    assert ma_new <= 1.5 * ma_old and rl_new <= 1.5 * rl_old, msg
    assert torch.equal(c["new"], c["again"])


def test_residual_and_alpha_follow_conv3x3():
    """(acc + bias) * alpha rounded, + residual, rounded: the order of ca_conv3x3's epilogue."""
    k = _k()
    c = case(SHAPES[1], torch.float16, True)
    g = torch.Generator().manual_seed(5)
    res = torch.randn(c["ref"].shape, generator=g).half().to(DEV)
    old = k.conv3x3(c["x"], c["wk"], bias=c["bias"], upsample=True, residual=res, alpha=0.5)
    new = k.conv_up2_phase(c["x"], c["wp"], bias=c["bias"], residual=res, alpha=0.5)
    ref = (c["ref"] * 0.5).half().float() + res.float()
    ma_old, rl_old = errors(old, ref)
    ma_new, rl_new = errors(new, ref)
    msg = f"residual + alpha: max-abs new {ma_new:.3e} vs existing {ma_old:.3e}, rel-L2 new {rl_new:.3e} vs existing {rl_old:.3e}"
    print(msg)
    assert rl_new < 2e-3 and rl_new <= 1.5 * rl_old + 1e-4, msg   # (fp16 output precision; the margin of the suite's other two-path tests)


def _upsampler(channels, dtype, seed):
    from controlanimate_amd.layers import WeightArena
    from controlanimate_amd.resnet import Upsample3D
    torch.manual_seed(seed)
    up = Upsample3D(channels)
    up.conv.bias.data.normal_(std=0.5)
    arena = WeightArena()
    up.pack(arena, dtype)
    arena.finalize(DEV)
    return up


def test_declined_shape_through_the_module_is_todays_conv3x3():
    """ca_conv_up2_phase_supported == 0 (4 tiles: the form does not pay): InflatedConv3d.run calls ca_conv3x3(upsample=1) exactly as before."""
    k = _k()
    up = _upsampler(320, torch.float16, 3)
    assert up.conv.wp is not None
    x = torch.randn(1, 8, 8, 320, generator=torch.Generator().manual_seed(4)).half().to(DEV)
    assert not k.conv_up2_phase_supported(x, up.conv.wp.t, bias=up.conv.b.t)
    k._plan_sink = labels = []
    try:
        y = up(x)
        want = k.conv3x3(x, up.conv.w.t, bias=up.conv.b.t, upsample=True)
    finally:
        k._plan_sink = None
    assert labels[0] == labels[1] and not labels[0].startswith("up2"), labels
    assert torch.equal(y, want)


def test_taken_shape_through_the_module_and_the_dispatch_switch():
    """16 images 16x16 -> 32x32 at 1280 channels: 256 tiles, one whole round -- taken by default; dispatch.conv_up2_phase = False gives the
    existing path (at this shape the Winograd form)."""
    from controlanimate_amd.context import dispatch
    k = _k()
    up = _upsampler(1280, torch.float16, 6)
    x = torch.randn(16, 16, 16, 1280, generator=torch.Generator().manual_seed(8)).half().to(DEV)
    assert k.conv_up2_phase_supported(x, up.conv.wp.t, bias=up.conv.b.t)
    k._plan_sink = labels = []
    try:
        y = up(x)
        y2 = up(x)
        dispatch.conv_up2_phase = False
        try:
            old = up(x)
        finally:
            dispatch.conv_up2_phase = True
    finally:
        k._plan_sink = None
    assert labels[:2] == ["up2_pq256x320"] * 2 and not labels[2].startswith("up2"), labels
    assert torch.equal(y, y2)
    ref = F.conv2d(F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest"), up.conv.weight.detach().float().to(DEV),
                   bias=up.conv.bias.detach().float().to(DEV), padding=1).permute(0, 2, 3, 1)
    rl_new, rl_old = errors(y, ref)[1], errors(old, ref)[1]
    # (against the fp32 master weights both forms carry one weight rounding; the existing one is the Winograd form here, whose
    #  transformed operands round more often)
    assert rl_new < 2e-3 and rl_new <= 1.5 * rl_old, (rl_new, rl_old)
