"""GPU: the lineart annotator (controlanimate_amd/lineart.py, csrc/ca_lineart.hip) against its specification (tests/lineart_ref.py):
the input convolution, the InstanceNorm with its options, the transposed convolution, the output convolution and the finish kernel on
their own, and the whole chain end to end.

Tolerances: the convolutions use the bar of tests/test_kernels_gpu.py's convolution test (relative L2 < 2.5 * eps, eps = 2^-10 for fp16 and
2^-8 for bf16, largest error < 4 x that of the largest reference value); the InstanceNorm output is within relative L2 2^-10
(fp16: twice the output's half-ulp) / 2^-7 (bf16) of a float64 reference on the same rounded input, its padded ring bit-equal to the
mirrored interior; an output logit is within the fp32 accumulation bound K * 2^-24 * sum |x * w| (K = 3136 terms) of a float64 dot;
the uint8 map equals the numpy specification wherever the float64 sigmoid * 255 is further than 1e-3 from an integer (elsewhere
within one level), control == map / 255 exactly; the end-to-end logits meet the project's fp16 bar (relative L2 <= 1e-2; bf16 8e-2).
A CPU emulation of the chain that stores every activation in fp16 gave 1.7e-3 .. 2.1e-3 at reference logits of standard deviation
2.4 .. 2.7.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lineart_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAME = "lllyasviel/control_v11p_sd15_lineart"
CONV_BAR = {torch.float16: 2.5 * 2.0 ** -10, torch.bfloat16: 2.5 * 2.0 ** -8}  # tests/test_kernels_gpu.py: close()


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


# ---- input convolution -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 12, 20, 3), (1, 9, 70, 3)])   # (9 x 70: a partial tile row and a second tile along x)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_conv_in(shape, dtype):
    from controlanimate_amd.lineart import pack_conv_in
    k = _k()
    n, h, w, _ = shape
    g = torch.Generator().manual_seed(21)
    frames = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    wt = rnd(64, 3, 7, 7, dtype=dtype, scale=(2.0 / 147) ** 0.5, seed=22)
    x = F.pad(frames.permute(0, 3, 1, 2).float() / 255.0, (3, 3, 3, 3), mode="reflect")
    ref = F.conv2d(x, wt.float()).permute(0, 2, 3, 1)
    out = torch.full((n, h, w, 64), float("nan"), dtype=dtype, device=DEV)
    k.lineart_conv_in(frames.to(DEV), pack_conv_in(wt.float()).to(dtype).to(DEV), out)
    torch.cuda.synchronize()
    _conv_bar(f"conv_in {shape}", out.float().cpu(), ref, dtype)


# ---- InstanceNorm ------------------------------------------------------------------------------------------------------------------
IN_OPTIONS = [dict(), dict(relu=True), dict(relu=True, in_ring=True, out_pad=True), dict(residual=True, res_ring=True, in_ring=True, out_pad=True),
              dict(residual=True, in_ring=True), dict(relu=True, residual=True, out_pad=True)]


@pytest.mark.parametrize("opts", IN_OPTIONS, ids=lambda o: "+".join(sorted(o)) or "plain")
@pytest.mark.parametrize("shape", [(2, 6, 10, 64), (1, 5, 7, 256), (1, 40, 72, 128)])   # (40 x 72 at 128 channels: two chunks of partial sums)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_instance_norm(shape, opts, dtype):
    k = _k()
    n, h, w, c = shape
    g = torch.Generator().manual_seed(31)
    std = 0.5 + torch.rand(c, generator=g)
    mean = torch.where(torch.arange(c) % 2 == 1, 8.0 * std, torch.randn(c, generator=g) * 0.3)   # odd channels: mean = 8 x std
    x = (torch.randn(n, h, w, c, generator=g) * std + mean)
    x[..., 3] = 1.5                                                                              # a constant channel
    x = x.to(dtype)
    res = rnd(n, h, w, c, dtype=dtype, seed=32) if opts.get("residual") else None

    def ringed(t):   # stored with a one-pixel ring that must be ignored
        out = torch.full((n, h + 2, w + 2, c), float("nan"), dtype=dtype)
        out[:, 1:-1, 1:-1] = t
        return out

    xd = x.double()
    mu, var = xd.mean(dim=(1, 2), keepdim=True), xd.var(dim=(1, 2), unbiased=False, keepdim=True)
    ref = (xd - mu) / torch.sqrt(var + 1e-5)
    if opts.get("relu"):
        ref = ref.clamp_min(0)
    if res is not None:
        ref = ref + res.double()
    got = k.instance_norm((ringed(x) if opts.get("in_ring") else x).to(DEV), relu=bool(opts.get("relu")),
                          residual=None if res is None else (ringed(res) if opts.get("res_ring") else res).to(DEV),
                          in_ring=bool(opts.get("in_ring")), res_ring=bool(opts.get("res_ring")), out_pad=bool(opts.get("out_pad")))
    torch.cuda.synchronize()
    got = got.cpu()
    if opts.get("out_pad"):
        assert tuple(got.shape) == (n, h + 2, w + 2, c)
        bits = got.view(torch.int16)
        assert torch.equal(bits[:, 0], bits[:, 2]) and torch.equal(bits[:, h + 1], bits[:, h - 1])        # reflection: no repeated edge
        assert torch.equal(bits[:, :, 0], bits[:, :, 2]) and torch.equal(bits[:, :, w + 1], bits[:, :, w - 1])
        got = got[:, 1:-1, 1:-1]
    assert tuple(got.shape) == shape and torch.isfinite(got).all()
    if res is None:
        assert (got[..., 3] == 0).all()                                                                   # the constant channel
    rel = ((got.double() - ref).norm() / ref.norm()).item()
    tol = 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7
    print(f"instance_norm {shape} {dtype} {opts}: relative L2 {rel:.3e} (tol {tol:.2e})")
    assert rel <= tol


# ---- transposed convolution --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w,cin,cout", [(2, 5, 7, 128, 64), (1, 6, 10, 256, 128), (1, 33, 18, 128, 64)])   # (odd sizes: the zero row / column past the edge)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_conv_transpose(n, h, w, cin, cout, dtype):
    from controlanimate_amd.lineart import pack_convt_phases
    k = _k()
    x = rnd(n, h, w, cin, dtype=dtype, seed=41)
    wt = rnd(cin, cout, 3, 3, dtype=dtype, scale=(2.0 / (cin * 9 / 4)) ** 0.5, seed=42)
    ref = F.conv_transpose2d(x.float().permute(0, 3, 1, 2), wt.float(), stride=2, padding=1, output_padding=1).permute(0, 2, 3, 1)
    out = k.conv_transpose3x3s2(x.to(DEV), pack_convt_phases(wt).to(DEV))
    torch.cuda.synchronize()
    assert tuple(out.shape) == (n, 2 * h, 2 * w, cout)
    _conv_bar(f"conv_transpose {(n, h, w, cin, cout)}", out.float().cpu(), ref, dtype)


# ---- output convolution ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_conv_out(dtype):
    k = _k()
    n, h, w = 2, 12, 20   # (one full and one partial tile along x)
    x = rnd(n, h, w, 64, dtype=dtype, seed=51).abs()   # behind a ReLU
    wt = rnd(1, 64, 7, 7, dtype=torch.float32, scale=3136 ** -0.5, seed=52)
    bias = torch.tensor([0.37])
    xp = F.pad(x.double().permute(0, 3, 1, 2), (3, 3, 3, 3), mode="reflect")
    exact = F.conv2d(xp, wt.double())[:, 0] + bias.double()
    bound = 3136 * 2.0 ** -24 * F.conv2d(xp.abs(), wt.double().abs())[:, 0]
    logits = torch.full((n, h, w), float("nan"), device=DEV)
    k.lineart_conv_out(x.to(DEV), wt[0].permute(1, 2, 0).contiguous().to(DEV), bias.to(DEV), logits)
    torch.cuda.synchronize()
    err = (logits.cpu().double() - exact).abs()
    print(f"conv_out {dtype}: worst err / bound = {(err / bound).max().item():.3f}")
    assert torch.isfinite(logits).all() and (err <= bound).all()


# ---- finish ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def finish_case():
    """n = 2 maps of 24 x 40 seeded N(0, 2.5^2) logits, and what the specification makes of them."""
    n, h, w = 2, 24, 40
    logits = (np.random.default_rng(4).standard_normal((n, h, w)) * 2.5).astype(np.float32)
    logits[0, 0, :4] = [-100.0, 100.0, 0.0, -0.0]
    want, scaled = lineart_ref.finish_ref(logits)
    decided = np.abs(scaled - np.rint(scaled)) > 1e-3
    return n, h, w, logits, want, decided


def test_finish_specification_leaves_few_pixels_undecided(finish_case):
    n, h, w, _, want, decided = finish_case
    share = 1.0 - decided.mean()
    print(f"share of pixels within 1e-3 of an integer: {share:.4f}")
    assert share <= 0.01
    assert want.min() < 40 and want.max() > 215  # the map uses its range
    assert want[0, 0, 0] == 255 and want[0, 0, 1] == 0 and want[0, 0, 2] == 128   # inverted: no line -> 255 - 0


@pytest.mark.parametrize("rep", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_finish_equals_the_numpy_specification(finish_case, rep, dtype):
    k = _k()
    n, h, w, logits, want, decided = finish_case
    dev = torch.from_numpy(logits).to(DEV)
    edges = torch.full((n, h, w), 3, dtype=torch.uint8, device=DEV)
    ctrl = torch.full((rep * n, 3, h, w), 7.0, dtype=dtype, device=DEV)
    k.lineart_finish(dev, edges=edges, control=ctrl, rep=rep)
    torch.cuda.synchronize()
    got = edges.cpu().numpy()
    diff = (got != want) & decided
    assert not diff.any(), f"{diff.sum()} pixels differ from the specification, first at {np.argwhere(diff)[0]}"
    assert (np.abs(got.astype(int) - want.astype(int)) <= 1).all()  # and the undecided ones by one level at most
    level = edges.cpu().float() / 255.0                          # control == map / 255 exactly in fp32 (rounded once more for fp16)
    c = ctrl.cpu()
    for r in range(rep):
        for ch in range(3):
            assert torch.equal(c[r * n:(r + 1) * n, ch], level.to(dtype))
    if rep == 2:
        assert torch.equal(c[:n], c[n:])
    only_e = torch.empty_like(edges)                             # either output alone: the same bytes
    k.lineart_finish(dev, edges=only_e)
    only_c = torch.empty_like(ctrl)
    k.lineart_finish(dev, control=only_c, rep=rep)
    assert torch.equal(only_e, edges) and torch.equal(only_c, ctrl)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def _rounded(sd, dtype):
    return {k: (v.to(dtype).float() if k.endswith(".weight") else v) for k, v in sd.items()}


@pytest.fixture(scope="module")
def e2e():
    """Two 64 x 128 frames, seeded weights rounded to fp16 (what the device holds), the fp32 reference's logits -- computed once --
    and the annotator."""
    from controlanimate_amd.annotators import LineartAnnotator
    sd = _rounded(lineart_ref.lineart_state_dict(seed=5, out_scale=3.0), torch.float16)
    frames = lineart_ref._frames()
    ref = lineart_ref.logits_ref(sd, frames)
    return {"sd": sd, "frames": frames, "logits": ref, "ann": LineartAnnotator(sd, DEV)}


def test_e2e_reference_logits_are_in_the_sigmoid_range(e2e):
    std = float(e2e["logits"].std())
    print(f"standard deviation of the reference logits: {std:.3f}")
    assert 0.5 <= std <= 4.0


def test_e2e_logits(e2e):
    got = e2e["ann"].logits(list(e2e["frames"]))
    torch.cuda.synchronize()
    assert tuple(got.shape) == (2, 64, 128) and got.dtype == torch.float32 and got.is_cuda
    got, ref = got.cpu(), e2e["logits"]
    rel = ((got - ref).norm() / ref.norm()).item()
    print(f"fp16 logits: relative L2 {rel:.3e}")
    assert torch.isfinite(got).all() and rel <= 1e-2


def test_e2e_bfloat16_runs_the_same_chain(e2e):
    from controlanimate_amd.annotators import LineartAnnotator
    sd = _rounded(lineart_ref.lineart_state_dict(seed=5, out_scale=3.0), torch.bfloat16)
    ref = lineart_ref.logits_ref(sd, e2e["frames"])
    assert 0.5 <= float(ref.std()) <= 4.0
    got = LineartAnnotator(sd, DEV, dtype=torch.bfloat16).logits(list(e2e["frames"])).cpu()
    rel = ((got - ref).norm() / ref.norm()).item()
    print(f"bf16 logits: relative L2 {rel:.3e}")
    assert torch.isfinite(got).all() and rel <= 8e-2  # 8 x the fp16 bar: bf16 carries 3 bits less


def test_e2e_map_is_the_finish_of_the_chains_own_logits(e2e):
    k, ann, frames = _k(), e2e["ann"], e2e["frames"]
    logits = ann.logits(torch.from_numpy(frames).to(DEV))
    alone = torch.empty((2, 64, 128), dtype=torch.uint8, device=DEV)
    k.lineart_finish(logits, edges=alone)
    got = ann.edges(list(frames))
    assert got.dtype == torch.uint8 and got.is_cuda and torch.equal(got, alone)
    assert got.min() < 40 and got.max() > 215
    # frame chunks: one frame per pass through the network gives the same bytes
    from controlanimate_amd.annotators import LineartAnnotator
    one = LineartAnnotator(e2e["sd"], DEV)
    one.max_activation_bytes = 64 * 128 * 288
    assert one.chunk_frames(64, 128) == 1 and torch.equal(one.edges(list(frames)), got)


def test_e2e_call_and_annotate_batch_contracts(e2e):
    from PIL import Image
    ann, frames = e2e["ann"], e2e["frames"]
    edges = ann.edges(list(frames)).cpu()
    pil = ann(Image.fromarray(frames[0]))
    assert isinstance(pil, Image.Image) and pil.mode == "RGB" and pil.size == (128, 64)
    a = np.asarray(pil)
    assert np.array_equal(a[..., 0], a[..., 1]) and np.array_equal(a[..., 0], a[..., 2]) and np.array_equal(a[..., 0], edges[0].numpy())
    arr = ann(frames[1])
    assert isinstance(arr, np.ndarray) and arr.shape == (64, 128, 3) and np.array_equal(arr[..., 2], edges[1].numpy())
    base = (edges.float() / 255.0)[:, None].expand(-1, 3, -1, -1)
    for dtype in (torch.float32, torch.float16):
        for rep in (1, 2):
            got = ann.annotate_batch([Image.fromarray(f) for f in frames], rep=rep, dtype=dtype)
            assert got.dtype == dtype and got.is_cuda and torch.equal(got.cpu(), torch.cat([base] * rep).to(dtype))
        t = torch.full((4, 3, 64, 128), 7.0, dtype=dtype, device=DEV)
        ptr = t.data_ptr()
        ret = ann.annotate_batch(list(frames), out=t, rep=2)
        assert ret is t and t.data_ptr() == ptr and torch.equal(t.cpu(), torch.cat([base] * 2).to(dtype))
    out = torch.empty((2, 64, 128), dtype=torch.uint8, device=DEV)
    assert ann.edges(torch.from_numpy(frames), out=out) is out and torch.equal(out.cpu(), edges)
    grey = ann.edges([Image.fromarray(frames[0][..., 0])]).cpu()                       # mode L: the three channels are the grey one
    assert torch.equal(grey, ann.edges([np.repeat(frames[0][..., :1], 3, axis=2)]).cpu())


def test_e2e_timed_stages_are_the_same_chain(e2e):
    from controlanimate_amd.lineart import STAGES
    ann, frames = e2e["ann"], e2e["frames"]
    plain = ann.edges(list(frames)).clone()
    ann.timings = {}
    try:
        timed = ann.edges(list(frames))
        torch.cuda.synchronize()
        assert {k: len(v) for k, v in ann.timings.items()} == STAGES == {"conv_in": 1, "instnorm": 11, "conv": 8, "convt": 2, "conv_out": 1, "finish": 1}
        assert all(a.elapsed_time(b) >= 0 for evs in ann.timings.values() for a, b in evs)
    finally:
        ann.timings = None
    assert torch.equal(timed, plain)


def test_e2e_chain_replays_in_a_captured_graph(e2e):
    """No launch of the chain waits for the host: captured once, it replays for new frames copied into the captured buffer."""
    ann, frames = e2e["ann"], e2e["frames"]
    eager = [ann.annotate_batch(torch.from_numpy(f).to(DEV), rep=2).clone() for f in (frames, frames[::-1].copy())]
    buf = torch.from_numpy(frames).to(DEV)
    out = torch.empty((4, 3, 64, 128), dtype=torch.float32, device=DEV)
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
    pipe = MultiControlNetResidualsPipeline([NAME], [1.0], use_lcm=False, controlnets=[net], device="cuda", annotators={"lineart": Counting()})
    pipe.prep_control_images(frames, do_classifier_free_guidance=cfg)
    rep = 2 if cfg else 1
    assert len(calls) == 1 and calls[0]["n"] == 2 and calls[0]["rep"] == rep and calls[0]["out"] is None and calls[0]["dtype"] == torch.float32
    got = pipe.prep_images[0]
    want = torch.cat([(ann.edges(frames).cpu().float() / 255.0)[:, None].expand(-1, 3, -1, -1)] * rep)  # (divided on the host: IEEE division)
    assert got.shape == (2 * rep, 3, 64, 128) and got.dtype == torch.float32 and got.is_cuda and got._cfg_doubled is cfg
    assert torch.equal(got.cpu(), want) and 0.05 < got.mean() < 0.95
    ptr = got.data_ptr()
    pipe.prep_control_images(frames[::-1], do_classifier_free_guidance=cfg)  # the next window goes into the tensor the ControlNets hold
    assert len(calls) == 2 and calls[1]["out"] is got and pipe.prep_images[0] is got and got.data_ptr() == ptr
    assert torch.equal(got[:2].cpu(), want[:2].flip(0))
    # the annotator itself plugs in under the same key
    direct = MultiControlNetResidualsPipeline([NAME], [1.0], use_lcm=False, controlnets=[net], device="cuda", annotators={"lineart": ann})
    direct.prep_control_images(frames[::-1], do_classifier_free_guidance=cfg)
    assert torch.equal(direct.prep_images[0], got)
