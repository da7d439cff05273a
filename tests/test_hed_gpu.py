"""GPU: the HED annotator (controlanimate_amd/hed.py, csrc/ca_hed.hip) against its specification (tests/hed_ref.py): the ReLU
epilogue of ca_conv3x3, ca_hed_prep / ca_hed_pool_side / ca_hed_fuse on their own, and the whole chain end to end.

Tolerances: the ReLU convolution uses the bar of tests/test_kernels_gpu.py's convolution test (relative L2 < 2.5 * 2^-10 for fp16, largest
error < 4 x that of the largest reference value); prep, the pooled tensor, control == edges / 255 and the chain's own fuse are exact;
a side map pixel is within the fp32 accumulation bound C * 2^-24 * sum_c |x * w| of a float64 dot; the uint8 map equals the numpy
specification wherever the specification's float64 edge * 255 is further than 1e-3 from an integer (the device's exp may differ
from numpy's in the last bits); the end-to-end side maps and mean logit meet the project's fp16 bar (relative L2 <= 1e-2, as the VAE).
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hed_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E2E_PROJ_SCALE = (0.04, 0.04, 0.04, 0.03, 0.03)  # x activations of standard deviation ~60 .. 120: logits of standard deviation ~2.5


def _k():
    from controlanimate_amd import kernels
    return kernels


def rnd(*shape, dtype=torch.float16, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


# ---- ReLU convolution --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("images,h,w,cin,cout", [(2, 16, 24, 64, 128), (1, 8, 8, 512, 512)])
def test_conv3x3_relu(images, h, w, cin, cout):
    k = _k()
    dtype = torch.float16
    x = rnd(images, h, w, cin, dtype=dtype, seed=11)
    wt = rnd(cout, cin, 3, 3, dtype=dtype, scale=(9 * cin) ** -0.5, seed=13)  # torch OIHW
    bias = rnd(cout, dtype=torch.float32, seed=14)
    ref = F.relu(F.conv2d(x.float().permute(0, 3, 1, 2), wt.float(), bias, padding=1)).permute(0, 2, 3, 1)
    assert 0.2 < (ref == 0).float().mean() < 0.8  # the activation clips about half of the outputs
    out = k.conv3x3(x.to(DEV), wt.permute(0, 2, 3, 1).contiguous().to(DEV), bias=bias.to(DEV), act=k.ACT_RELU)
    torch.cuda.synchronize()
    out = out.float().cpu()
    assert out.shape == ref.shape and torch.isfinite(out).all() and (out >= 0).all()
    rel = 2.5 * 2.0 ** -10
    rel_l2 = ((out - ref).norm() / ref.norm()).item()
    max_rel = ((out - ref).abs().max() / ref.abs().max()).item()
    print(f"conv3x3 relu {images}x{h}x{w} {cin}->{cout}: rel_l2={rel_l2:.3e} max_err/max_ref={max_rel:.3e} (tol {rel:.1e})")
    assert rel_l2 < rel and max_rel < 4 * rel
    # into a caller's tensor: the same bytes
    buf = torch.empty((images, h, w, cout), dtype=dtype, device=DEV)
    ret = k.conv3x3(x.to(DEV), wt.permute(0, 2, 3, 1).contiguous().to(DEV), bias=bias.to(DEV), act=k.ACT_RELU, out=buf)
    assert ret is buf and torch.equal(buf.float().cpu(), out)


# ---- ca_hed_prep -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_prep_is_bit_equal_to_the_torch_expression(dtype):
    k = _k()
    g = torch.Generator().manual_seed(1)
    frames = torch.randint(0, 256, (3, 5, 67, 3), generator=g, dtype=torch.uint8)  # 1005 pixels: more than one block, a partial last one
    frames[0, 0, 0] = torch.tensor([0, 255, 128], dtype=torch.uint8)
    norm = torch.tensor([122.6789, 116.6688, 104.0069])
    out = torch.full((3, 5, 67, 8), 7.0, dtype=dtype, device=DEV)
    k.hed_prep(frames.to(DEV), norm.to(DEV), out)
    torch.cuda.synchronize()
    want = torch.zeros((3, 5, 67, 8), dtype=dtype)
    want[..., :3] = (frames.float() - norm).to(dtype)
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))  # bits: the zero channels are +0


# ---- ca_hed_pool_side --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,pool", [((2, 6, 10, 64), True), ((1, 4, 8, 512), True), ((2, 6, 10, 64), False), ((1, 4, 8, 512), False),
                                        ((1, 2, 6, 72), True)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_pool_side(shape, pool, dtype):
    k = _k()
    n, h, w, c = shape  # (6 x 10: pooled height 3 is odd; 72 channels: 9 of a group's 16 lanes hold data)
    x = rnd(*shape, dtype=dtype, scale=30.0, seed=2)
    pw = rnd(c, dtype=torch.float32, scale=c ** -0.5, seed=3)
    pb = torch.tensor([0.37])
    side = torch.full((n, h, w), float("nan"), device=DEV)
    pooled = torch.full((n, h // 2, w // 2, c), float("nan"), dtype=dtype, device=DEV) if pool else None
    k.hed_pool_side(x.to(DEV), pw.to(DEV), pb.to(DEV), side, pooled)
    torch.cuda.synchronize()
    if pool:
        want = F.max_pool2d(x.float().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).to(dtype)
        assert torch.equal(pooled.cpu().view(torch.int16), want.contiguous().view(torch.int16))
    prod = x.double() * pw.double()
    exact = prod.sum(-1) + pb.double()
    bound = c * 2.0 ** -24 * prod.abs().sum(-1)
    err = (side.cpu().double() - exact).abs()
    print(f"pool_side {shape} {dtype}: worst err / bound = {(err / bound).max().item():.3f}")
    assert torch.isfinite(side).all() and (err <= bound).all()


# ---- ca_hed_fuse -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fuse_case():
    """n = 2 frames of 48 x 80 (the deep levels are 3 x 5), seeded N(0, 1.5^2) side maps, and what the specification makes of them."""
    n, h, w = 2, 48, 80
    rng = np.random.default_rng(4)
    sides = [(rng.standard_normal((n, h >> k, w >> k)) * 1.5).astype(np.float32) for k in range(5)]
    spec = [hed_ref.fuse_ref([s[i] for s in sides], h, w) for i in range(n)]
    edges = np.stack([s[0] for s in spec])
    scaled = np.stack([s[2] for s in spec])
    decided = np.abs(scaled - np.rint(scaled)) > 1e-3
    return n, h, w, sides, edges, decided


def test_fuse_specification_leaves_few_pixels_undecided(fuse_case):
    n, h, w, _, edges, decided = fuse_case
    share = 1.0 - decided.mean()
    print(f"share of pixels within 1e-3 of an integer: {share:.4f}")
    assert share <= 0.01
    assert edges.min() < 40 and edges.max() > 215  # the map uses its range


@pytest.mark.parametrize("rep", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_fuse_equals_the_numpy_specification(fuse_case, rep, dtype):
    k = _k()
    n, h, w, sides, want, decided = fuse_case
    dev = [torch.from_numpy(s).to(DEV) for s in sides]
    edges = torch.full((n, h, w), 3, dtype=torch.uint8, device=DEV)
    ctrl = torch.full((rep * n, 3, h, w), 7.0, dtype=dtype, device=DEV)
    k.hed_fuse(dev, edges=edges, control=ctrl, rep=rep)
    torch.cuda.synchronize()
    got = edges.cpu().numpy()
    diff = (got != want) & decided
    assert not diff.any(), f"{diff.sum()} pixels differ from the specification, first at {np.argwhere(diff)[0]}"
    assert (np.abs(got.astype(int) - want.astype(int)) <= 1).all()  # and the undecided ones by one level at most
    level = edges.cpu().float() / 255.0                          # control == edges / 255 exactly in fp32 (rounded once more for fp16)
    c = ctrl.cpu()
    for r in range(rep):
        for ch in range(3):
            assert torch.equal(c[r * n:(r + 1) * n, ch], level.to(dtype))
    if rep == 2:
        assert torch.equal(c[:n], c[n:])
    # either output alone: the same bytes
    only_e = torch.empty_like(edges)
    k.hed_fuse(dev, edges=only_e)
    only_c = torch.empty_like(ctrl)
    k.hed_fuse(dev, control=only_c, rep=rep)
    assert torch.equal(only_e, edges) and torch.equal(only_c, ctrl)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def _frames():
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:64, 0:128]
    out = []
    for i in range(2):
        a = np.zeros((64, 128, 3), np.float64)
        a[..., 0] = 128 + 100 * np.sin(xx / (5.0 + i)) * np.cos(yy / 7.0)
        a[..., 1] = (xx * 2 + yy * (3 + i)) % 256
        a[..., 2] = 255 * ((xx // 16 + yy // 16 + i) % 2)
        a += rng.normal(0, 12, a.shape)
        out.append(a.clip(0, 255).astype(np.uint8))
    return np.stack(out)


@pytest.fixture(scope="module")
def e2e():
    """Two 64 x 128 frames, seeded weights rounded to fp16 (what the device holds), the fp32 reference's side maps and mean logit --
    computed once -- and the annotator."""
    from controlanimate_amd.annotators import HedAnnotator
    sd = hed_ref.hed_state_dict(seed=5, proj_scale=E2E_PROJ_SCALE)
    sd = {k: (v.half().float() if ".convs." in k and k.endswith(".weight") else v) for k, v in sd.items()}  # (biases, projections and norm stay fp32 on the device)
    frames = _frames()
    sides = hed_ref.side_maps_ref(sd, frames)
    mean = np.stack([hed_ref.fuse_ref([s[i].numpy() for s in sides], 64, 128)[1] for i in range(2)])
    ann = HedAnnotator(sd, DEV, detect_resolution=64, image_resolution=64)
    return {"sd": sd, "frames": frames, "sides": sides, "mean": mean, "ann": ann}


def test_e2e_reference_logits_are_in_the_sigmoid_range(e2e):
    stds = [float(s.std()) for s in e2e["sides"]] + [float(e2e["mean"].std())]
    print("standard deviation of the reference's five side maps and of the mean logit:", [round(s, 3) for s in stds])
    assert all(0.5 <= s <= 4.0 for s in stds)


def test_e2e_side_maps_and_mean_logit(e2e):
    got = e2e["ann"].side_maps(list(e2e["frames"]))
    torch.cuda.synchronize()
    assert [tuple(s.shape) for s in got] == [(2, 64 >> k, 128 >> k) for k in range(5)] and all(s.dtype == torch.float32 and s.is_cuda for s in got)
    host = [s.cpu() for s in got]
    for k, (s, ref) in enumerate(zip(host, e2e["sides"])):
        rel = ((s - ref).norm() / ref.norm()).item()
        print(f"side map {k}: relative L2 {rel:.3e}")
        assert torch.isfinite(s).all() and rel <= 1e-2
    mean = np.stack([hed_ref.fuse_ref([s[i].numpy() for s in host], 64, 128)[1] for i in range(2)])
    rel = float(np.linalg.norm(mean - e2e["mean"]) / np.linalg.norm(e2e["mean"]))
    print(f"mean logit: relative L2 {rel:.3e}")
    assert rel <= 1e-2


def test_e2e_map_is_the_fuse_of_the_chains_own_side_maps(e2e):
    k, ann, frames = _k(), e2e["ann"], e2e["frames"]
    sides = ann.side_maps(torch.from_numpy(frames).to(DEV))
    alone = torch.empty((2, 64, 128), dtype=torch.uint8, device=DEV)
    k.hed_fuse(sides, edges=alone)
    got = ann.edges(list(frames))
    assert got.dtype == torch.uint8 and got.is_cuda and torch.equal(got, alone)
    # frame chunks: one frame per pass through the network gives the same bytes
    from controlanimate_amd.annotators import HedAnnotator
    one = HedAnnotator(e2e["sd"], DEV, detect_resolution=64, image_resolution=64)
    one.max_activation_bytes = 64 * 128 * 64 * 2
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


def test_e2e_bfloat16_runs_the_same_chain(e2e):
    from controlanimate_amd.annotators import HedAnnotator
    ann = HedAnnotator(e2e["sd"], DEV, dtype=torch.bfloat16, detect_resolution=64, image_resolution=64)
    got = [s.cpu() for s in ann.side_maps(list(e2e["frames"]))]
    for k, (s, ref) in enumerate(zip(got, e2e["sides"])):
        rel = ((s - ref).norm() / ref.norm()).item()
        print(f"bf16 side map {k}: relative L2 {rel:.3e}")
        assert torch.isfinite(s).all() and rel <= 8e-2  # 8 x the fp16 bar: bf16 carries 3 bits less (2^-8 against 2^-11 per rounding)


def test_e2e_timed_launches_are_the_same_chain(e2e):
    ann, frames = e2e["ann"], e2e["frames"]
    plain = ann.edges(list(frames)).clone()
    ann.timings = {}
    try:
        timed = ann.edges(list(frames))
        torch.cuda.synchronize()
        assert {k: len(v) for k, v in ann.timings.items()} == {"prep": 1, "conv": 13, "pool_side": 5, "fuse": 1}
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

    name = "lllyasviel/sd-controlnet-hed"
    net = ControlNetModel.from_config(controlnet_config(block_out_channels=(32, 64, 64, 64)))
    pipe = MultiControlNetResidualsPipeline([name], [1.0], use_lcm=False, controlnets=[net], device="cuda", annotators={"hed": Counting()})
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
    direct = MultiControlNetResidualsPipeline([name], [1.0], use_lcm=False, controlnets=[net], device="cuda", annotators={"hed": ann})
    direct.prep_control_images(frames[::-1], do_classifier_free_guidance=cfg)
    assert torch.equal(direct.prep_images[0], got)
