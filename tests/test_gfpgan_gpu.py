"""GPU: the GFPGAN face restorer (controlanimate_amd/gfpgan.py, csrc/ca_gfpgan.hip) against its specification (tests/gfpgan_ref.py):
the modulated convolution, the prep, resample, styles, ToRGB and finish kernels on their own, and the whole chain end to end.

Tolerances.  ca_modconv3x3 and ca_gfp_prep meet the project's convolution bar (tests/test_kernels_gpu.py): relative L2 < 2.5 * eps, eps =
2^-10 for fp16 and 2^-8 for bf16, largest error < 4 x that of the largest reference value, against fp32 torch on the same rounded
operands.  ca_resample2x is bit-equal to an fp32 torch interpolate rounded to the type.  ca_gfp_styles' s is within the bound of a
513-term fp32 sum, 513 * 2^-24 * sum |terms|, of float64, its demod' within (cin + 3) / 2 * 2^-24 + 2^-23 relative of the float64 value
from the s it wrote; ca_gfp_to_rgb within (cin + 8) * 2^-24 * sum |terms|.  The uint8 output equals the numpy container wherever the
float64 value in front of the rounding is farther than 1e-3 from a half-integer, and is within one level elsewhere.

End to end the comparison is FaceRestorer.pre_clamp against the fp32 specification with the same rounded weights and the same
explicit noises, and the bar comes from the emulation (gfpgan_ref.emulate: every stored activation rounded to the type, fp32
accumulation), run on these fixtures (gfpgan_ref.make_net seed 5, make_faces seed 7, make_noises seed 8) on the CPU.  It gave, as
relative L2 against the fp32 specification:

    out_size  64, n = 2:   fp16 2.23e-4   bf16 1.80e-3      ->  bars 9e-4 / 8e-3   (4 x the figure, rounded up to one digit)
    out_size 512, n = 1:   fp16 5.71e-4   bf16 4.71e-3      ->  bars 3e-3 / 2e-2

The margin covers the accumulation order, the factored modulation (one more rounding, of s * x, per StyleConv) and, on the planes
where kernels.modconv3x3 runs as three launches, the rounding of the convolution's output in front of the epilogue, none of which the
emulation reproduces.  Both forms of a StyleConv are held to the same convolution bar, and both give an image the same bits in any batch.  The reference images have standard deviation 0.63 (64) and 0.46 (512) with 12 % / 7 % of the values
clamped.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gfpgan_ref as R  # noqa: E402
import rrdb_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
CONV_BAR = {torch.float16: 2.5 * 2.0 ** -10, torch.bfloat16: 2.5 * 2.0 ** -8}  # tests/test_kernels_gpu.py: close()
E2E_BAR = {64: {torch.float16: 9e-4, torch.bfloat16: 8e-3}, 512: {torch.float16: 3e-3, torch.bfloat16: 2e-2}}
NET_SEED, FACE_SEED, NOISE_SEED = 5, 7, 8
U = 2.0 ** -24


def _k():
    from controlanimate_amd import kernels
    return kernels


def rnd(*shape, dtype=torch.float16, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def _conv_bar(what, out, ref, dtype):
    rel = CONV_BAR[dtype]
    rel_l2 = ((out - ref).norm() / ref.norm()).item()
    max_rel = ((out - ref).abs().max() / ref.abs().max()).item()
    print(f"{what} {dtype}: rel_l2={rel_l2:.3e} max_err/max_ref={max_rel:.3e} (tol {rel:.1e})")
    assert torch.isfinite(out).all() and rel_l2 < rel and max_rel < 4 * rel


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


# ---- the modulated convolution -------------------------------------------------------------------------------------------------------
def _modconv_operands(n, h, w, cin, cout, up, dtype, xscale=1.0):
    hh, ww = (2 * h, 2 * w) if up else (h, w)
    g = torch.Generator().manual_seed(31)
    op = {"x": rnd(n, h, w, cin, dtype=dtype, scale=xscale, seed=32), "wt": rnd(cout, cin, 3, 3, dtype=dtype, scale=(1.0 / (9 * cin)) ** 0.5, seed=33),
          "s": torch.rand(n, cin, generator=g) * 2 - 1, "demod": torch.rand(n, cout, generator=g) + 0.5, "noise": torch.randn(n, hh, ww, generator=g),
          "bias": torch.linspace(-0.3, 0.3, cout), "nw": 0.37,
          "scale": (1 + 0.3 * torch.randn(n, hh, ww, cout // 2, generator=g)).to(dtype), "shift": (0.3 * torch.randn(n, hh, ww, cout // 2, generator=g)).to(dtype)}
    return op


def _modconv_ref(op, up, sft, double=False):
    f = (lambda t: t.double()) if double else (lambda t: t.float())
    x = _nchw(f(op["x"]))
    if up:
        x = R.resize2(x, True)
    acc = F.conv2d(x * f(op["s"])[:, :, None, None], f(op["wt"]), padding=1)
    v = acc * f(op["demod"])[:, :, None, None] * (2.0 ** 0.5) + op["nw"] * f(op["noise"])[:, None] + f(op["bias"])[None, :, None, None]
    v = _nhwc(F.leaky_relu(v, 0.2))
    if sft:
        half = v.shape[3] // 2
        v = torch.cat([v[..., :half], v[..., half:] * f(op["scale"]) + f(op["shift"])], dim=3)
    return v


def _modconv_run(op, up, sft, form=None):
    k = _k()
    d = {key: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for key, v in op.items()}
    n, cout = d["s"].shape[0], d["wt"].shape[0]
    hh, ww = d["noise"].shape[1:]
    out = torch.full((n, hh, ww, cout), float("nan"), dtype=op["x"].dtype, device=DEV)
    k.modconv3x3(d["x"], d["wt"].permute(0, 2, 3, 1).contiguous(), d["s"], d["demod"], d["noise"], d["bias"], d["nw"], upsample=up,
                 sft=(d["scale"], d["shift"]) if sft else None, out=out, form=form)
    torch.cuda.synchronize()
    return out.cpu()


MODCONV_CASES = [(2, 4, 4, 512, 512),      # a plane below one tile
                 (1, 6, 10, 128, 64),      # a partial tile in both axes; the 64-channel tile
                 (2, 16, 16, 256, 128),
                 (3, 5, 7, 64, 128)]       # three images: the indexing of s, demod and noise per image


FORMS = ["fused", "composed"]   # ca_modconv3x3; ca_gfp_modulate + ca_conv3x3 + ca_gfp_style_epilogue.  Both are held to the same bar


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("sft", [False, True])
@pytest.mark.parametrize("up", [False, True])
@pytest.mark.parametrize("n,h,w,cin,cout", MODCONV_CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_modconv3x3(n, h, w, cin, cout, up, sft, dtype, form):
    op = _modconv_operands(n, h, w, cin, cout, up, dtype)
    out = _modconv_run(op, up, sft, form)
    _conv_bar(f"modconv3x3 {form} {(n, h, w, cin, cout)} up={up} sft={sft}", out.float(), _modconv_ref(op, up, sft), dtype)
    if sft:      # the first half of the channels does not see the SFT operands: bit-equal to the run without them
        plain = _modconv_run(op, up, False, form)
        assert torch.equal(out[..., :cout // 2], plain[..., :cout // 2]) and not torch.equal(out[..., cout // 2:], plain[..., cout // 2:])


@pytest.mark.parametrize("form", FORMS)
def test_modconv3x3_shared_input_is_the_repeated_one(form):
    """x_shared: the decoder's constant [1, 4, 4, 512] read by every image."""
    k = _k()
    op = _modconv_operands(3, 4, 4, 512, 512, False, torch.float16)
    want = _modconv_run({**op, "x": op["x"][:1].repeat(3, 1, 1, 1)}, False, False, form)
    d = {key: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for key, v in op.items()}
    got = k.modconv3x3(d["x"][:1].contiguous(), d["wt"].permute(0, 2, 3, 1).contiguous(), d["s"], d["demod"], d["noise"], d["bias"], d["nw"], images=3, form=form)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want)


def test_modconv3x3_picks_its_form_by_the_output_plane():
    k = _k()
    assert k.MODCONV_FUSED_MIN_PIXELS == 512 * 512
    op = _modconv_operands(1, 4, 4, 64, 64, False, torch.float16)
    assert torch.equal(_modconv_run(op, False, False), _modconv_run(op, False, False, "composed"))     # a small plane: the composed form


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("h,up,cin,cout", [(4, False, 512, 512), (16, True, 512, 512), (64, False, 512, 512), (32, True, 256, 128), (64, False, 128, 128),
                                            (64, True, 128, 64)])
def test_modconv3x3_gives_an_image_the_same_bits_in_any_batch(h, up, cin, cout, form):
    """Four images at once against each alone, at each channel pair of the decoder: among them the planes where ca_conv3x3 would split K for
    one image and not for four (64 x 64 at 512 channels) or split it differently; the composed form runs it without a workspace, the one-launch
    kernel tiles each image alone."""
    op = _modconv_operands(4, h, h, cin, cout, up, torch.float16)
    whole = _modconv_run(op, up, True, form)
    for i in (0, 3):
        one = {key: (v[i:i + 1].contiguous() if isinstance(v, torch.Tensor) and v.shape[0] == 4 and key not in ("wt", "bias") else v) for key, v in op.items()}
        assert torch.equal(_modconv_run(one, up, True, form), whole[i:i + 1])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("up", [False, True])
def test_modconv3x3_large_styles_stay_finite_in_fp16(up, form):
    """|s| and |x| near 300 in fp16: s * x would leave fp16's range; with s / max|s| and demod' = max|s| * demod from ca_gfp_styles the
    result stays finite and inside the bar.  The reference is demod * conv(W, s * x) in float64."""
    k = _k()
    n, h, w, cin, cout, dtype = 2, 6, 10, 128, 64, torch.float16
    op = _modconv_operands(n, h, w, cin, cout, up, dtype, xscale=300.0)
    g = torch.Generator().manual_seed(34)
    s = (200 + 100 * torch.rand(n, cin, generator=g)) * (torch.randint(0, 2, (n, cin), generator=g) * 2 - 1)   # 200 .. 300, either sign
    assert (s.abs().max() * op["x"].float().abs().max()).item() > 65504
    # a modulation whose weight is zero and whose bias is s: one layer per image's s would need per-image latents; the bias is shared, so
    # the two images' s differ through a weight on latent coordinate 0
    wmod = torch.zeros(512, cin)
    wmod[0] = s[1] - s[0]
    lat = torch.zeros(n, 1, 512)
    lat[1, 0, 0] = 1.0
    wsq = op["wt"].float().pow(2).sum([2, 3]).t().contiguous()                # [cin, cout]
    params = torch.cat([wmod.reshape(-1), s[0], wsq.reshape(-1)]).to(DEV)
    styles = k.gfp_styles(lat.to(DEV), params, [0, cin, cout, 0, 513 * cin, 0], torch.empty(n, cin + cout, device=DEV))
    op2 = {**op, "s": styles[:, :cin], "demod": styles[:, cin:]}
    d = {key: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for key, v in op2.items()}
    out = k.modconv3x3(d["x"], d["wt"].permute(0, 2, 3, 1).contiguous(), d["s"], d["demod"], d["noise"], d["bias"], d["nw"], upsample=up, form=form)
    torch.cuda.synchronize()
    sd = s.double()
    demod = torch.rsqrt((sd * sd) @ wsq.double() + 1e-8)
    ref = _modconv_ref({**op, "s": sd, "demod": demod}, up, False, double=True)
    assert ref.abs().max() < 65504 and ref.abs().max() > 300
    _conv_bar(f"modconv3x3 {form} |s|, |x| ~ 300 up={up}", out.cpu().double(), ref, dtype)


# ---- the stage kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [True, False])
@pytest.mark.parametrize("content", ["random", 0, 255])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gfp_prep(content, reverse, dtype):
    k = _k()
    shape, cout = (2, 6, 10, 3), 32
    g = torch.Generator().manual_seed(21)
    faces = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8) if content == "random" else torch.full(shape, content, dtype=torch.uint8)
    wt, bias = torch.randn(cout, 3, generator=g) * 0.6, torch.linspace(-0.3, 0.3, cout)
    x = R.container_in(faces, reverse_channels=reverse)                                    # the numpy container: [n, 3, h, w]
    ref = F.leaky_relu(_nhwc(F.conv2d(x, wt.view(cout, 3, 1, 1), bias)), 0.2)
    out = torch.full((*shape[:3], cout), float("nan"), dtype=dtype, device=DEV)
    k.gfp_prep(faces.to(DEV), wt.to(DEV), bias.to(DEV), out, reverse_channels=reverse)
    torch.cuda.synchronize()
    _conv_bar(f"gfp_prep {content} reverse={reverse}", out.float().cpu(), ref, dtype)
    if content == "random":
        assert not torch.allclose(ref, F.leaky_relu(_nhwc(F.conv2d(R.container_in(faces, reverse_channels=not reverse), wt.view(cout, 3, 1, 1), bias)), 0.2))


@pytest.mark.parametrize("shape,up", [((2, 6, 10, 64), True), ((1, 5, 7, 8), True), ((3, 1, 1, 16), True), ((2, 6, 10, 64), False), ((1, 4, 2, 8), False)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_resample2x_is_bit_equal_to_torch(shape, up, dtype):
    k = _k()
    x = rnd(*shape, dtype=dtype, scale=3.0, seed=41)
    out = k.resample2x(x.to(DEV), up)
    torch.cuda.synchronize()
    want = R.resample_ref(x, up, dtype)
    assert tuple(out.shape) == tuple(want.shape) and torch.equal(out.cpu(), want)


def test_gfp_styles_against_float64():
    k = _k()
    g = torch.Generator().manual_seed(51)
    n, nlat = 3, 6
    lat = torch.randn(n, nlat, 512, generator=g)
    layers = [(2, 512, 512), (5, 256, 128), (0, 64, 0), (3, 128, 0)]         # (latent, cin, cout); cout 0: a ToRGB
    chunks, desc, p_off, o_off = [], [], 0, 0
    for li, cin, cout in layers:
        wm, b = torch.randn(512, cin, generator=g) * 0.05, 1 + 0.1 * torch.randn(cin, generator=g)
        wsq = torch.rand(cin, cout, generator=g) / cin
        chunks += [wm.reshape(-1), b, wsq.reshape(-1)]
        desc += [li, cin, cout, p_off, p_off + 513 * cin, o_off]
        p_off += 513 * cin + cin * cout
        o_off += cin + cout
    params = torch.cat(chunks)
    out = k.gfp_styles(lat.to(DEV), params.to(DEV), desc, torch.full((n, o_off), float("nan"), device=DEV))
    torch.cuda.synchronize()
    out = out.cpu().double()
    for i, (li, cin, cout) in enumerate(layers):
        _, _, _, w_off, wsq_off, off = desc[6 * i:6 * i + 6]
        wm, b = params[w_off:w_off + 512 * cin].view(512, cin).double(), params[w_off + 512 * cin:w_off + 513 * cin].double()
        l64 = lat[:, li].double()
        s = l64 @ wm + b
        bound = 513 * U * (l64.abs() @ wm.abs() + b.abs())                    # a 513-term fp32 sum
        got = out[:, off:off + cin]
        if cout == 0:
            assert ((got - s).abs() <= bound).all()
            continue
        m = s.abs().amax(dim=1, keepdim=True)
        assert ((got - s / m).abs() <= 1.01 * (bound + bound.amax(dim=1, keepdim=True)) / m + 2 * U).all()
        assert (got.abs().amax(dim=1) == 1.0).all()                           # the largest magnitude divided by itself
        wsq = params[wsq_off:wsq_off + cin * cout].view(cin, cout).double()
        want = torch.rsqrt((got * got) @ wsq + 1e-8 / (m * m))
        rel = ((out[:, off + cin:off + cin + cout] - want).abs() / want).max().item()
        print(f"gfp_styles layer {i} (cin {cin}, cout {cout}): demod' relative error {rel:.2e}")
        assert rel <= (cin + 3) / 2 * U + 2 * U


@pytest.mark.parametrize("with_prev", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gfp_to_rgb(with_prev, dtype):
    k = _k()
    n, h, w, cin = 3, 6, 10, 128
    g = torch.Generator().manual_seed(61)
    x = rnd(n, h, w, cin, dtype=dtype, seed=62)
    wt, s, bias = torch.randn(3, cin, generator=g) * 0.1, 1 + 0.3 * torch.randn(n, cin, generator=g), torch.tensor([0.1, -0.2, 0.3])
    prev = torch.randn(n, h // 2, w // 2, 3, generator=g) if with_prev else None
    out = k.gfp_to_rgb(x.to(DEV), wt.to(DEV), s.to(DEV), bias.to(DEV), torch.full((n, h, w, 3), float("nan"), device=DEV), prev=None if prev is None else prev.to(DEV))
    torch.cuda.synchronize()
    ws = (wt.float()[None] * s.float()[:, None]).double()                      # the kernel's fp32 product, [n, 3, cin]
    ref = torch.einsum("nhwi,nci->nhwc", x.double(), ws) + bias.double()
    mag = torch.einsum("nhwi,nci->nhwc", x.double().abs(), ws.abs()) + bias.double().abs()
    if with_prev:
        up = _nhwc(R.resize2(_nchw(prev.double()), True))
        ref, mag = ref + up, mag + _nhwc(R.resize2(_nchw(prev.double().abs()), True))
    assert ((out.cpu().double() - ref).abs() <= (cin + 8) * U * mag).all()


@pytest.mark.parametrize("reverse", [True, False])
def test_gfp_finish_equals_the_numpy_container(reverse):
    k = _k()
    x = R.make_finish_fixture(NET_SEED + 6)                                   # [n, 3, S, S]; its share of near-ties is checked in test_gfpgan_cpu.py
    pre = _nhwc(x).contiguous()
    out = k.gfp_finish(pre.to(DEV), torch.zeros(pre.shape, dtype=torch.uint8, device=DEV), reverse_channels=reverse)
    torch.cuda.synchronize()
    _check_u8(out.cpu().numpy(), x, reverse)


def _check_u8(got, image_nchw, reverse):
    want = R.container_out(image_nchw, reverse_channels=reverse)
    band = R.in_band(R.pre_round64(image_nchw, reverse_channels=reverse))
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"uint8 tail: {band.mean():.4%} of the values within {R.BAND} of a half-integer, {int((diff > 0).sum())} differ")
    assert (diff[~band] == 0).all() and diff.max() <= 1


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, size, n, dtype):
        from controlanimate_amd.gfpgan import FaceRestorer
        net = R.make_net(size, NET_SEED)
        self.sd = R.round_weights(net.state_dict(), dtype)
        net.load_state_dict(self.sd)
        self.faces, self.noises = R.make_faces(size, n, FACE_SEED), R.make_noises(size, n, NOISE_SEED)
        with torch.no_grad():
            self.ref = net(R.container_in(self.faces), self.noises)           # [n, 3, S, S], computed once
        self.restorer = FaceRestorer(self.sd, device=DEV, dtype=dtype, out_size=size)
        self.size, self.n, self.dtype = size, n, dtype


_cases = {}


def case(size, n, dtype):
    if (size, dtype) not in _cases:
        _cases[(size, dtype)] = Case(size, n, dtype)
    return _cases[(size, dtype)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_end_to_end_64(dtype):
    c = case(64, 2, dtype)
    pre = _nchw(c.restorer.pre_clamp(c.faces, c.noises).cpu())
    rel = ((pre - c.ref).norm() / c.ref.norm()).item()
    print(f"end to end 64 {dtype}: rel_l2={rel:.3e} (bar {E2E_BAR[64][dtype]:.0e}); reference std {c.ref.std().item():.3f}, "
          f"{(c.ref.abs() > 1).float().mean().item():.1%} clamped")
    assert c.ref.std() > 0.3 and (c.ref.abs() < 1).float().mean() > 0.5      # the fixture uses the range and is not all clamped
    assert torch.isfinite(pre).all() and rel < E2E_BAR[64][dtype]
    assert pre.std() > 0.3 and (pre.abs() < 1).float().mean() > 0.5          # and so does the device's own image
    u8 = c.restorer.restore_aligned(c.faces, c.noises)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (2, 64, 64, 3) and u8.is_cuda
    _check_u8(u8.cpu().numpy(), pre, True)                                    # the container's tail applied to the chain's own pre_clamp


def test_end_to_end_512():
    c = case(512, 1, torch.float16)
    pre = _nchw(c.restorer.pre_clamp(c.faces, c.noises).cpu())
    rel = ((pre - c.ref).norm() / c.ref.norm()).item()
    print(f"end to end 512 fp16: rel_l2={rel:.3e} (bar {E2E_BAR[512][torch.float16]:.0e}); reference std {c.ref.std().item():.3f}")
    assert c.ref.std() > 0.3 and (c.ref.abs() < 1).float().mean() > 0.5
    assert torch.isfinite(pre).all() and rel < E2E_BAR[512][torch.float16]
    assert pre.std() > 0.3 and (pre.abs() < 1).float().mean() > 0.5


def test_determinism_noise_and_splitting():
    c = case(64, 2, torch.float16)
    r = c.restorer
    faces, noises = R.make_faces(64, 4, FACE_SEED + 1), R.make_noises(64, 4, NOISE_SEED + 1)   # four faces: one pass, or 3 + 1
    a, b = r.restore_aligned(faces, noises), r.restore_aligned(faces, noises)
    assert tuple(a.shape) == (4, 64, 64, 3) and torch.equal(a, b)             # the same noises: the same bits
    other = R.make_noises(64, 4, NOISE_SEED + 2)
    assert not torch.equal(a, r.restore_aligned(faces, other))                # noise reaches the output
    g = torch.Generator(device=DEV).manual_seed(3)
    d1 = r.restore_aligned(faces, generator=g).clone()
    g.manual_seed(3)
    d2 = r.restore_aligned(faces, generator=g)
    assert torch.equal(d1, d2) and not torch.equal(d1, a)                     # randomize_noise=True from a seeded generator
    from controlanimate_amd.gfpgan import FaceRestorer
    split = FaceRestorer(c.sd, device=DEV, dtype=torch.float16, out_size=64, max_faces_per_launch=3)
    before = split.passes
    assert torch.equal(split.restore_aligned(faces, noises), a) and split.passes == before + 2
    out = torch.zeros_like(a)
    assert r.restore_aligned([f for f in faces.numpy()], noises, out=out) is out and torch.equal(out, a)   # a list of arrays; `out`


def test_chain_replays_in_a_captured_graph():
    c = case(64, 2, torch.float16)
    r = c.restorer
    faces = c.faces.to(DEV)
    noises = [t.to(DEV) for t in c.noises]
    eager = r.restore_aligned(faces, noises).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = r.restore_aligned(faces, noises)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_upscaler_hook_runs_the_net_once_per_frame():
    """Upscaler(scale, face_enhancer=restorer.as_face_enhancer(helper))(frame): the helper's pasted image comes back, the background
    upsampled by the Upscaler itself, and the net ran once for the frame's two faces."""
    from PIL import Image
    from controlanimate_amd.upscaler import Upscaler
    c = case(64, 2, torch.float16)
    r = c.restorer
    frame = np.zeros((80, 96, 3), np.uint8)
    frame[2:66, 3:67], frame[10:74, 30:94] = c.faces[0].numpy(), c.faces[1].numpy()

    class Helper(R.FakeHelper):
        def paste_faces_to_input_image(self, upsample_img=None):
            self.pasted = super().paste_faces_to_input_image(upsample_img)
            return self.pasted
    helper = Helper(64, [(2, 3), (10, 30)])
    up = Upscaler(2, state_dict=rrdb_ref.rrdb_state_dict(seed=1), device=DEV, face_enhancer=r.as_face_enhancer(helper))
    before = r.passes
    out = np.asarray(up(Image.fromarray(frame)))
    assert r.passes == before + 1 and len(helper.restored_faces) == 2
    assert out.shape == (160, 192, 3) and np.array_equal(out, helper.pasted)
    assert helper.calls[-1] == ("paste_faces_to_input_image", True)           # the Upscaler was the background upsampler
    bg, _ = up.enhance(frame, outscale=2)
    assert np.array_equal(out[150:], bg[150:])                                # below the faces: the upsampled background
    assert np.array_equal(out[20:84, 60:124], helper.restored_faces[1])       # the second face's window, pasted last
