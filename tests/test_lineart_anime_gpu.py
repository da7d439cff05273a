"""GPU: the lineart_anime annotator (controlanimate_amd/lineart_anime.py, csrc/ca_lineart_anime.hip) against its specification
(tests/lineart_anime_ref.py): the input convolution, the 4x4 stride-2 convolution, its transpose, the InstanceNorm with two activated
outputs, the output convolution and the finish kernel on their own, in fp16 and bf16, and the whole chain end to end.

Tolerances (those of tests/test_lineart_gpu.py): the convolutions meet relative L2 < 2.5 * eps, eps = 2^-10 for fp16 and 2^-8 for bf16,
largest error < 4 x that of the largest reference value, against fp32 torch on the same rounded operands; the InstanceNorm output is
within relative L2 2^-10 (fp16) / 2^-7 (bf16) of a float64 reference on the same rounded input, and the half of a concatenation buffer
it does not write stays bit-unchanged; a pre-tanh value of the output convolution is within the fp32 accumulation bound
K * 2^-24 * sum |x * w| (K = 512 terms) of a float64 sum; the uint8 map equals the numpy specification wherever the float64
tanh * 127.5 + 127.5 is further than 1e-3 from an integer (elsewhere within one level), control == map / 255 exactly; the end-to-end
pre-tanh values meet the project's bars (relative L2 <= 1e-2 for fp16, <= 8e-2 for bf16).

The emulation behind those end-to-end bars is lineart_anime_ref.emulate_pre_tanh: the chain on the CPU with every weight and every
stored activation rounded to the narrow type, fp32 accumulation and fp32 InstanceNorm statistics.  On the fixtures used here (He-scaled
seeded weights, seeds 5 and 6, two 256 x 256 frames and one 256 x 512 frame) it gave, against the fp32 network with the same rounded
weights: fp16 0.85e-3 .. 1.13e-3, bf16 6.7e-3 .. 8.5e-3; the reference pre-tanh values had standard deviation 0.83 .. 0.84, the fp32
map spanned 1 .. 255, and the fp16 uint8 map differed from fp32's by at most one level (bf16's by up to five).
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lineart_anime_ref as ref_mod  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAME = "lllyasviel/control_v11p_sd15s2_lineart_anime"
DTYPES = [torch.float16, torch.bfloat16]
CONV_BAR = {torch.float16: 2.5 * 2.0 ** -10, torch.bfloat16: 2.5 * 2.0 ** -8}  # tests/test_kernels_gpu.py: close()
SENTINEL = 7.0


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


# ---- input convolution -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", ["random", 255, 0])
@pytest.mark.parametrize("shape", [(2, 12, 20, 3), (1, 10, 70, 3)])   # (10 x 70: a partial tile row and a second pixel group along x)
@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_in(shape, content, dtype):
    from controlanimate_amd.lineart_anime import pack_conv_in
    k = _k()
    n, h, w, _ = shape
    g = torch.Generator().manual_seed(21)
    frames = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8) if content == "random" else torch.full(shape, content, dtype=torch.uint8)
    wt = rnd(64, 3, 4, 4, dtype=dtype, scale=(2.0 / 48) ** 0.5, seed=22)
    wt[:, :, 0, 0] += 0.25          # the taps that fall outside at the top-left corner carry weight: byte 0 taken as -1 there would show
    wt = wt.to(dtype)
    bias = torch.linspace(-0.3, 0.3, 64)
    d0 = _nhwc(F.conv2d(_nchw(frames).float() / 127.5 - 1.0, wt.float(), bias, stride=2, padding=1))     # zero padding of the NORMALISED image
    l0 = torch.full((n, h // 2, w // 2, 64), float("nan"), dtype=dtype, device=DEV)
    c0 = torch.full((n, h // 2, w // 2, 128), SENTINEL, dtype=dtype, device=DEV)
    k.lanime_conv_in(frames.to(DEV), pack_conv_in(wt.float()).to(dtype).to(DEV), bias.to(DEV), l0, c0)
    torch.cuda.synchronize()
    l0, c0 = l0.float().cpu(), c0.float().cpu()
    what = f"conv_in {shape} {content}"
    _conv_bar(what + " L0", l0, F.leaky_relu(d0, 0.2), dtype)
    _conv_bar(what + " C0[:64]", c0[..., :64], F.relu(d0), dtype)
    border = torch.ones(h // 2, w // 2, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    _conv_bar(what + " L0 border", l0[:, border], F.leaky_relu(d0, 0.2)[:, border], dtype)
    assert (c0[..., 64:] == SENTINEL).all()                                           # the second half of C_0 is not touched


# ---- the 4x4 stride-2 convolution ----------------------------------------------------------------------------------------------------
CONV_SHAPES = [(2, 8, 12, 64, 128, False),
               (1, 34, 18, 128, 256, False),     # partial tiles in both directions, three tile rows
               (2, 6, 4, 256, 512, False),
               (2, 2, 2, 512, 512, True)]        # a 1 x 1 output: 12 of 16 taps are padding; the bias + ReLU epilogue


@pytest.mark.parametrize("form", ["tile", "gemm"])   # the implicit GEMM from an LDS halo tile; the gather + ca_gemm of the levels with few output rows
@pytest.mark.parametrize("n,h,w,cin,cout,epilogue", CONV_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_conv4x4s2(n, h, w, cin, cout, epilogue, dtype, form):
    from controlanimate_amd.lineart_anime import pack_conv4x4
    k = _k()
    x = rnd(n, h, w, cin, dtype=dtype, seed=41)
    wt = rnd(cout, cin, 4, 4, dtype=dtype, scale=(2.0 / (cin * 16)) ** 0.5, seed=42)
    bias = torch.linspace(-0.5, 0.5, cout) if epilogue else None
    ref = F.conv2d(_nchw(x.float()), wt.float(), bias, stride=2, padding=1)
    if epilogue:
        ref = F.relu(ref)
    out = torch.full((n, h // 2, w // 2, cout), float("nan"), dtype=dtype, device=DEV)
    k.conv4x4s2(x.to(DEV), pack_conv4x4(wt).to(DEV), bias=None if bias is None else bias.to(DEV), relu=epilogue, out=out, form=form)
    torch.cuda.synchronize()
    _conv_bar(f"conv4x4s2 {form} {(n, h, w, cin, cout)}", out.float().cpu(), _nhwc(ref), dtype)


def test_conv4x4s2_picks_its_form_by_the_output_rows():
    """Below kernels.CONV4X4S2_GEMM_ROWS output rows the default is the gather + ca_gemm, from there on the tile kernel: 4095 and 4096 rows
    (65 x 63 and 64 x 64 output pixels at 64 -> 128 channels) give what the named form gives, bit for bit."""
    from controlanimate_amd.lineart_anime import pack_conv4x4
    k = _k()
    assert k.CONV4X4S2_GEMM_ROWS == 4096
    wt = pack_conv4x4(rnd(128, 64, 4, 4, scale=(2.0 / 1024) ** 0.5, seed=46)).to(DEV)
    for (h, w), form in (((130, 126), "gemm"), ((128, 128), "tile")):
        x = rnd(1, h, w, 64, seed=45).to(DEV)
        plans = []
        k._plan_sink = plans
        try:
            auto = k.conv4x4s2(x, wt)
        finally:
            k._plan_sink = None
        assert (len(plans) == 1) == (form == "gemm")                                          # a ca_gemm launch was recorded, or none
        assert torch.equal(auto, k.conv4x4s2(x, wt, form=form))
        other = k.conv4x4s2(x, wt, form="tile" if form == "gemm" else "gemm")                  # and the two forms agree to the convolutions' bar
        _conv_bar(f"conv4x4s2 forms at {h // 2} x {w // 2}", auto.float().cpu(), other.float().cpu(), torch.float16)


# ---- the transposed convolution ------------------------------------------------------------------------------------------------------
# (planes of 16 rows or more run 16 x 16 source pixels per block, smaller ones 8 x 16; 64 output channels a narrower tile of them)
@pytest.mark.parametrize("n,h,w,cin,cout", [(2, 1, 1, 512, 512), (1, 4, 6, 1024, 512), (2, 5, 9, 256, 64), (1, 18, 34, 512, 128), (1, 16, 20, 256, 64)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_convt4x4s2(n, h, w, cin, cout, dtype):
    from controlanimate_amd.lineart_anime import pack_convt4x4_phases
    k = _k()
    x = rnd(n, h, w, cin, dtype=dtype, seed=43).abs()   # behind a ReLU
    wt = rnd(cin, cout, 4, 4, dtype=dtype, scale=(2.0 / (cin * 4)) ** 0.5, seed=44)
    ref = F.conv_transpose2d(_nchw(x.float()), wt.float(), stride=2, padding=1)
    out = torch.full((n, 2 * h, 2 * w, cout), float("nan"), dtype=dtype, device=DEV)
    k.conv_transpose4x4s2(x.to(DEV), pack_convt4x4_phases(wt).to(DEV), out=out)
    torch.cuda.synchronize()
    _conv_bar(f"convt4x4s2 {(n, h, w, cin, cout)}", out.float().cpu(), _nhwc(ref), dtype)


# ---- InstanceNorm with activated outputs ---------------------------------------------------------------------------------------------
ACTS = {0: lambda t: t, 1: lambda t: t.clamp_min(0), 2: lambda t: torch.where(t > 0, t, 0.2 * t)}
# (destinations): each (width in units of c, channel offset in units of c, activation)
IN_CONFIGS = {"down: L leaky + C[:c] relu": [(1, 0, 2), (2, 0, 1)],
              "up: C[c:] relu": [(2, 1, 1)],
              "plain": [(1, 0, 0)],
              "C[c:] none + C'[:c] leaky": [(2, 1, 0), (2, 0, 2)]}


@pytest.mark.parametrize("config", list(IN_CONFIGS), ids=lambda s: s.replace(" ", "_"))
@pytest.mark.parametrize("shape", [(2, 2, 2, 512), (1, 4, 6, 512), (1, 16, 24, 256), (1, 70, 66, 64)])   # (2 x 2 and 4 x 6: one chunk, the one-launch form; 16 x 24 at 256 channels: 6 chunks, 70 x 66 at 64: 19 -- statistics + apply)
@pytest.mark.parametrize("dtype", DTYPES)
def test_instance_norm_act(shape, config, dtype):
    k = _k()
    n, h, w, c = shape
    g = torch.Generator().manual_seed(31)
    std = 0.5 + torch.rand(c, generator=g)
    mean = torch.where(torch.arange(c) % 2 == 1, 8.0 * std, torch.randn(c, generator=g) * 0.3)   # odd channels: mean = 8 x std
    x = torch.randn(n, h, w, c, generator=g) * std + mean
    x[..., 3] = 1.5                                                                              # a constant channel
    x = x.to(dtype)
    xd = x.double()
    mu, var = xd.mean(dim=(1, 2), keepdim=True), xd.var(dim=(1, 2), unbiased=False, keepdim=True)
    norm = (xd - mu) / torch.sqrt(var + 1e-5)
    dests = [torch.full((n, h, w, wd * c), SENTINEL, dtype=dtype, device=DEV) for wd, _, _ in IN_CONFIGS[config]]
    k.instance_norm_act(x.to(DEV), [(t, act, off * c) for t, (_, off, act) in zip(dests, IN_CONFIGS[config])])
    torch.cuda.synchronize()
    tol = 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7
    for t, (wd, off, act) in zip(dests, IN_CONFIGS[config]):
        t = t.cpu()
        got, want = t[..., off * c:(off + 1) * c], ACTS[act](norm)
        assert torch.isfinite(got).all() and (got[..., 3] == 0).all()                             # the constant channel
        rel = ((got.double() - want).norm() / want.norm()).item()
        print(f"instance_norm_act {shape} {dtype} {config} act {act}: relative L2 {rel:.3e} (tol {tol:.2e})")
        assert rel <= tol
        if wd == 2:
            other = t[..., (1 - off) * c:(2 - off) * c]
            assert torch.equal(other, torch.full_like(other, SENTINEL))                           # the other half: bit-unchanged


# ---- output convolution ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_out(dtype):
    k = _k()
    n, h, w = 2, 6, 10
    x = rnd(n, h, w, 128, dtype=dtype, seed=51).abs()   # behind a ReLU
    wt = rnd(128, 1, 4, 4, dtype=torch.float32, scale=512 ** -0.5, seed=52)
    bias = torch.tensor([0.37])
    xd = _nchw(x.double())
    exact = F.conv_transpose2d(xd, wt.double(), stride=2, padding=1)[:, 0] + bias.double()
    bound = 512 * 2.0 ** -24 * F.conv_transpose2d(xd.abs(), wt.double().abs(), stride=2, padding=1)[:, 0]
    out = torch.full((n, 2 * h, 2 * w), float("nan"), device=DEV)
    k.lanime_conv_out(x.to(DEV), wt[:, 0].permute(1, 2, 0).contiguous().to(DEV), bias.to(DEV), out)
    torch.cuda.synchronize()
    err = (out.cpu().double() - exact).abs()
    print(f"conv_out {dtype}: worst err / bound = {(err / bound).max().item():.3f}")
    assert torch.isfinite(out).all() and (err <= bound).all()


# ---- finish ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def finish_case():
    return ref_mod.finish_case()


@pytest.mark.parametrize("rep", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_finish_equals_the_numpy_specification(finish_case, rep, dtype):
    k = _k()
    n, h, w, pre, want, decided = finish_case
    assert 1.0 - decided.mean() <= 0.01 and want.min() < 40 and want.max() > 215
    dev = torch.from_numpy(pre).to(DEV)
    edges = torch.full((n, h, w), 3, dtype=torch.uint8, device=DEV)
    ctrl = torch.full((rep * n, 3, h, w), 7.0, dtype=dtype, device=DEV)
    k.lanime_finish(dev, edges=edges, control=ctrl, rep=rep)
    torch.cuda.synchronize()
    got = edges.cpu().numpy()
    diff = (got != want) & decided
    assert not diff.any(), f"{diff.sum()} pixels differ from the specification, first at {np.argwhere(diff)[0]}"
    assert (np.abs(got.astype(int) - want.astype(int)) <= 1).all()  # and the undecided ones by one level at most
    assert got[0, 0, 0] == 255 and got[0, 0, 1] == 0
    level = edges.cpu().float() / 255.0                          # control == map / 255 exactly in fp32 (rounded once more for fp16)
    c = ctrl.cpu()
    for r in range(rep):
        for ch in range(3):
            assert torch.equal(c[r * n:(r + 1) * n, ch], level.to(dtype))
    if rep == 2:
        assert torch.equal(c[:n], c[n:])
    only_e = torch.empty_like(edges)                             # either output alone: the same bytes
    k.lanime_finish(dev, edges=only_e)
    only_c = torch.empty_like(ctrl)
    k.lanime_finish(dev, control=only_c, rep=rep)
    assert torch.equal(only_e, edges) and torch.equal(only_c, ctrl)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def _rounded(sd, dtype):
    return {k: (v.to(dtype).float() if k.endswith(".weight") else v) for k, v in sd.items()}


@pytest.fixture(scope="module")
def raw_sd():
    return ref_mod.lineart_anime_state_dict(seed=5)


@pytest.fixture(scope="module")
def e2e(raw_sd):
    """Two 256 x 256 frames (the innermost plane is 1 x 1) and one 256 x 512 frame, seeded weights rounded to fp16 (what the device
    holds), the fp32 reference's pre-tanh values -- computed once -- and the annotator."""
    from controlanimate_amd.annotators import LineartAnimeAnnotator
    sd = _rounded(raw_sd, torch.float16)
    frames, wide = ref_mod.frames_fixture(256, 256, 2), ref_mod.frames_fixture(256, 512, 1)
    return {"sd": sd, "frames": frames, "wide": wide, "pre": ref_mod.pre_tanh_ref(sd, frames), "pre_wide": ref_mod.pre_tanh_ref(sd, wide),
            "ann": LineartAnimeAnnotator(sd, DEV)}


def test_e2e_reference_uses_the_tanh_range(e2e):
    for key in ("pre", "pre_wide"):
        std = float(e2e[key].std())
        print(f"standard deviation of the reference pre-tanh values ({key}): {std:.3f}")
        assert 0.3 <= std <= 2.0
        want, _ = ref_mod.finish_ref(e2e[key].numpy())
        assert want.min() < 40 and want.max() > 215


@pytest.mark.parametrize("which", ["frames", "wide"])
def test_e2e_pre_tanh(e2e, which):
    frames, ref = e2e[which], e2e["pre" if which == "frames" else "pre_wide"]
    got = e2e["ann"].pre_tanh(list(frames))
    torch.cuda.synchronize()
    assert tuple(got.shape) == tuple(ref.shape) and got.dtype == torch.float32 and got.is_cuda
    got = got.cpu()
    rel = ((got - ref).norm() / ref.norm()).item()
    m_got, m_ref = ref_mod.finish_ref(got.numpy())[0], ref_mod.finish_ref(ref.numpy())[0]
    print(f"fp16 pre-tanh {tuple(ref.shape)}: relative L2 {rel:.3e}; largest map difference {np.abs(m_got.astype(int) - m_ref.astype(int)).max()} levels")
    assert torch.isfinite(got).all() and rel <= 1e-2


def test_e2e_bfloat16_runs_the_same_chain(e2e, raw_sd):
    from controlanimate_amd.annotators import LineartAnimeAnnotator
    sd = _rounded(raw_sd, torch.bfloat16)
    ann = LineartAnimeAnnotator(sd, DEV, dtype=torch.bfloat16)
    for frames in (e2e["frames"], e2e["wide"]):
        ref = ref_mod.pre_tanh_ref(sd, frames)
        assert 0.3 <= float(ref.std()) <= 2.0
        got = ann.pre_tanh(list(frames)).cpu()
        rel = ((got - ref).norm() / ref.norm()).item()
        print(f"bf16 pre-tanh {tuple(ref.shape)}: relative L2 {rel:.3e}")
        assert torch.isfinite(got).all() and rel <= 8e-2  # 8 x the fp16 bar: bf16 carries 3 bits less


def test_e2e_map_is_the_finish_of_the_chains_own_pre_tanh(e2e):
    k, ann, frames = _k(), e2e["ann"], e2e["frames"]
    pre = ann.pre_tanh(torch.from_numpy(frames).to(DEV))
    alone = torch.empty((2, 256, 256), dtype=torch.uint8, device=DEV)
    k.lanime_finish(pre, edges=alone)
    got = ann.edges(list(frames))
    assert got.dtype == torch.uint8 and got.is_cuda and torch.equal(got, alone)
    assert got.min() < 40 and got.max() > 215
    assert torch.equal(ann.pre_tanh(list(frames)), pre)                                 # two runs: the same bits
    # frame chunks: one frame per pass through the network gives the same bytes
    from controlanimate_amd.annotators import LineartAnimeAnnotator
    one = LineartAnimeAnnotator(e2e["sd"], DEV)
    one.max_activation_bytes = 256 * 256 * 64
    assert one.chunk_frames(256, 256) == 1 and torch.equal(one.edges(list(frames)), got)


def test_e2e_short_last_chunk_gathers_where_the_full_chunk_tiles(e2e):
    """Seven 256 x 256 frames in chunks of four: level 2 (64 x 64 -> 32 x 32 pixels) has 4096 rows in the full chunk, the tile kernel's, and
    3072 in the tail of three, the gather's -- whose im2col tensor (3072 x 2048) is larger than any the full chunk needs.  InstanceNorm
    is per image, so every frame meets the reference of its own content."""
    from controlanimate_amd.annotators import LineartAnimeAnnotator
    from controlanimate_amd.lineart_anime import cols_elems
    frames, ref = e2e["frames"][[0, 1, 0, 1, 0, 1, 0]], e2e["pre"][[0, 1, 0, 1, 0, 1, 0]]
    ann = LineartAnimeAnnotator(e2e["sd"], DEV)
    ann.max_activation_bytes = 4 * 256 * 256 * 64
    assert ann.chunk_frames(256, 256) == 4
    assert cols_elems(4, 256, 256) == 3072 * 2048 > 4 * 256 * 16 * 256          # the tail's level 2 > the full chunk's largest (level 3)
    k, plans = _k(), []
    k._plan_sink = plans
    try:
        got = ann.pre_tanh(list(frames)).cpu()
    finally:
        k._plan_sink = None
    assert len(plans) == 5 + 6                                                    # ca_gemm launches: levels 3 .. 7 of the full chunk, 2 .. 7 of the tail
    rel = ((got - ref).norm() / ref.norm()).item()
    print(f"fp16 pre-tanh, 7 frames as 4 + 3: relative L2 {rel:.3e}")
    assert torch.isfinite(got).all() and rel <= 1e-2
    for i in range(7):
        assert ((got[i] - ref[i]).norm() / ref[i].norm()).item() <= 1e-2, i


def test_e2e_call_and_annotate_batch_contracts(e2e):
    from PIL import Image
    ann, frames = e2e["ann"], e2e["frames"]
    edges = ann.edges(list(frames)).cpu()
    pil = ann(Image.fromarray(e2e["wide"][0]))
    assert isinstance(pil, Image.Image) and pil.mode == "RGB" and pil.size == (512, 256)
    a = np.asarray(pil)
    assert np.array_equal(a[..., 0], a[..., 1]) and np.array_equal(a[..., 0], a[..., 2]) and np.array_equal(a[..., 0], ann.edges(e2e["wide"])[0].cpu().numpy())
    arr = ann(frames[1])
    assert isinstance(arr, np.ndarray) and arr.shape == (256, 256, 3) and np.array_equal(arr[..., 2], edges[1].numpy())
    base = (edges.float() / 255.0)[:, None].expand(-1, 3, -1, -1)
    for dtype in (torch.float32, torch.float16):
        for rep in (1, 2):
            got = ann.annotate_batch([Image.fromarray(f) for f in frames], rep=rep, dtype=dtype)
            assert got.dtype == dtype and got.is_cuda and torch.equal(got.cpu(), torch.cat([base] * rep).to(dtype))
        t = torch.full((4, 3, 256, 256), 7.0, dtype=dtype, device=DEV)
        ptr = t.data_ptr()
        ret = ann.annotate_batch(list(frames), out=t, rep=2)
        assert ret is t and t.data_ptr() == ptr and torch.equal(t.cpu(), torch.cat([base] * 2).to(dtype))
    out = torch.empty((2, 256, 256), dtype=torch.uint8, device=DEV)
    assert ann.edges(torch.from_numpy(frames), out=out) is out and torch.equal(out.cpu(), edges)
    grey = ann.edges([Image.fromarray(frames[0][..., 0])]).cpu()                       # mode L: the three channels are the grey one
    assert torch.equal(grey, ann.edges([np.repeat(frames[0][..., :1], 3, axis=2)]).cpu())


def test_e2e_timed_stages_are_the_same_chain(e2e):
    from controlanimate_amd.lineart_anime import STAGES
    ann, frames = e2e["ann"], e2e["frames"]
    plain = ann.edges(list(frames)).clone()
    ann.timings = {}
    try:
        timed = ann.edges(list(frames))
        torch.cuda.synchronize()
        assert {k: len(v) for k, v in ann.timings.items()} == STAGES == {"conv_in": 1, "conv": 7, "instnorm": 13, "convt": 7, "conv_out": 1, "finish": 1}
        assert all(a.elapsed_time(b) >= 0 for evs in ann.timings.values() for a, b in evs)
    finally:
        ann.timings = None
    assert torch.equal(timed, plain)


def test_e2e_chain_replays_in_a_captured_graph(e2e):
    """No launch of the chain waits for the host: captured once (a linear chain, no parallel branches), it replays for new frames copied
    into the captured buffer."""
    ann, frames = e2e["ann"], e2e["frames"]
    eager = [ann.annotate_batch(torch.from_numpy(f).to(DEV), rep=2).clone() for f in (frames, frames[::-1].copy())]
    buf = torch.from_numpy(frames).to(DEV)
    out = torch.empty((4, 3, 256, 256), dtype=torch.float32, device=DEV)
    ann.annotate_batch(buf, out=out, rep=2)   # warm-up: the workspace and the weights are on the device before the capture
    out.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ann.annotate_batch(buf, out=out, rep=2)
    for i in (0, 1, 0):
        buf.copy_(torch.from_numpy(frames if i == 0 else frames[::-1].copy()).to(DEV))
        graph.replay()
        assert torch.equal(out, eager[i]), i
    assert 0.05 < out.mean() < 0.95


@pytest.mark.parametrize("cfg", [True, False])
def test_prep_control_images_goes_through_annotate_batch_once_per_list(e2e, cfg):
    from PIL import Image
    from controlanimate_amd.configs import controlnet_config
    from controlanimate_amd.controlnet import ControlNetModel
    from controlanimate_amd.controlresiduals_pipeline import MultiControlNetResidualsPipeline
    ann, frames = e2e["ann"], [Image.fromarray(f) for f in e2e["frames"]]
    calls = []

    class Counting:
        def __call__(self, image):
            raise AssertionError("the per-frame path must not be taken")

        def annotate_batch(self, fr, out=None, rep=1, dtype=None):
            calls.append({"n": len(fr), "out": out, "rep": rep, "dtype": dtype})
            return ann.annotate_batch(fr, out=out, rep=rep, dtype=dtype)

    net = ControlNetModel.from_config(controlnet_config(block_out_channels=(32, 64, 64, 64)))
    def plain_lineart(image):
        raise AssertionError("the key `lineart` serves no lineart_anime net")

    pipe = MultiControlNetResidualsPipeline([NAME], [1.0], use_lcm=False, controlnets=[net], device="cuda",
                                            annotators={"lineart": plain_lineart, "lineart_anime": Counting()})
    pipe.prep_control_images(frames, do_classifier_free_guidance=cfg)
    rep = 2 if cfg else 1
    assert len(calls) == 1 and calls[0]["n"] == 2 and calls[0]["rep"] == rep and calls[0]["out"] is None and calls[0]["dtype"] == torch.float32
    got = pipe.prep_images[0]
    want = torch.cat([(ann.edges(frames).cpu().float() / 255.0)[:, None].expand(-1, 3, -1, -1)] * rep)  # (divided on the host: IEEE division)
    assert got.shape == (2 * rep, 3, 256, 256) and got.dtype == torch.float32 and got.is_cuda and got._cfg_doubled is cfg
    assert torch.equal(got.cpu(), want) and 0.05 < got.mean() < 0.95
    ptr = got.data_ptr()
    pipe.prep_control_images(frames[::-1], do_classifier_free_guidance=cfg)  # the next window goes into the tensor the ControlNets hold
    assert len(calls) == 2 and calls[1]["out"] is got and pipe.prep_images[0] is got and got.data_ptr() == ptr
    assert torch.equal(got[:2].cpu(), want[:2].flip(0))
    # the annotator itself plugs in under the same key
    direct = MultiControlNetResidualsPipeline([NAME], [1.0], use_lcm=False, controlnets=[net], device="cuda", annotators={"lineart_anime": ann})
    direct.prep_control_images(frames[::-1], do_classifier_free_guidance=cfg)
    assert torch.equal(direct.prep_images[0], got)
