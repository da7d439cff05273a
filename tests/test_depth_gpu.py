"""GPU: the depth annotator (controlanimate_amd/depth.py, csrc/ca_depth.hip) against its specification (tests/depth_ref.py) and the fixture
made from transformers' and Pillow's own modules (tests/golden/dpt_tiny*.npz; the GPU tests read the fixture, not transformers).

Bars: ca_resize_pil_u8 equals Pillow byte for byte; the depth-to-space transposed convolutions, the readout GEMM and ca_dpt_head meet the
siblings' relative L2 < 2.5 * eps (eps = 2^-10 for fp16, 2^-8 for bf16) against fp32 torch on the same rounded operands; the bicubic tail is
within 1e-5 (largest error over largest reference value) of torch's with its max / min exact; ca_depth_finish equals the numpy specification
wherever the scaled value is further than 1e-3 from an integer or the depth is exactly zero (elsewhere within one level); the end-to-end predicted_depth meets the
project's bars per frame (relative L2 <= 1e-2 for fp16, <= 8e-2 for bf16), with the fused and with the composed head; the uint8 map may differ
from the fp32 fixture's by at most one level more than a plain torch fp16 run of depth_ref does.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
CONV_BAR = {torch.float16: 2.5 * 2.0 ** -10, torch.bfloat16: 2.5 * 2.0 ** -8}  # tests/test_kernels_gpu.py: close()
E2E_BAR = {torch.float16: 1e-2, torch.bfloat16: 8e-2}
RESIZE_SHAPES = [((64, 96), 96), ((40, 56), 96), ((512, 768), 384), ((384, 384), 384)]


def _k():
    from controlanimate_amd import kernels
    return kernels


def rnd(*shape, dtype=torch.float16, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def _bar(what, out, ref, dtype):
    rel = CONV_BAR[dtype]
    rel_l2 = ((out - ref).norm() / ref.norm()).item()
    print(f"{what} {dtype}: rel_l2={rel_l2:.3e} (tol {rel:.1e})")
    assert torch.isfinite(out).all() and rel_l2 < rel
    return rel_l2


def _packed(module, dtype):
    from controlanimate_amd.layers import WeightArena
    arena = WeightArena()
    module.pack(arena, dtype)
    arena.finalize(DEV)
    return module


def _smooth_frames(n, h, w, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for _ in range(n):
        img = np.stack([np.sin(2 * np.pi * (rng.uniform(0.5, 4) * y / h + rng.uniform(0.5, 4) * x / w) + rng.uniform(0, 6)) for _c in range(3)], -1)
        img += rng.normal(0, 0.15, img.shape)
        out.append(np.clip((img * 0.5 + 0.5) * 255, 0, 255).astype(np.uint8))
    return np.stack(out)


# ---- the resampler ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resample", [2, 3], ids=["bilinear", "bicubic"])
@pytest.mark.parametrize("src,size", RESIZE_SHAPES)
def test_resize_equals_pillow(src, size, resample):
    from PIL import Image
    from controlanimate_amd.depth import pil_coeffs
    K = _k()
    h, w = src
    frames = _smooth_frames(3, h, w, seed=h)
    want = np.stack([np.asarray(Image.fromarray(f).resize((size, size), resample=resample)) for f in frames])
    tabs = [torch.from_numpy(a).to(DEV) for a in pil_coeffs(w, size, resample) + pil_coeffs(h, size, resample)]
    got = K.resize_pil_u8(torch.from_numpy(frames).to(DEV), size, size, *tabs).cpu().numpy()
    diff = int((got != want).sum())
    print(f"resize {src} -> {size} resample {resample}: {diff} differing bytes")
    assert diff == 0


def test_patches_are_the_normalised_unfold():
    K = _k()
    frames = torch.from_numpy(_smooth_frames(2, 96, 96, seed=3)).to(DEV)
    got = K.dpt_patches(frames, 16, torch.float16).float()
    pv = (frames.float().permute(0, 3, 1, 2) / 255 - 0.5) / 0.5
    want = F.unfold(pv, 16, stride=16).transpose(1, 2).reshape(2 * 36, 768)
    assert (got - want).abs().max() <= 2.0 ** -11


# ---- reassemble --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("plane", [(6, 6), (5, 7)])
@pytest.mark.parametrize("k,c", [(4, 16), (2, 32), (4, 256), (2, 256)])
def test_conv_transpose_as_gemm_and_depth_to_space(k, c, plane, dtype):
    from controlanimate_amd.depth import _ConvTransposeK
    K = _k()
    gh, gw = plane
    n, t = 2, gh * gw + 1                                            # a class-token row in front of every image's rows, skipped by the scatter
    m = _ConvTransposeK(c, k)
    with torch.no_grad():
        m.weight.copy_(rnd(c, c, k, k, dtype=dtype, scale=c ** -0.5, seed=1).float())
        m.bias.copy_(rnd(c, dtype=torch.float32, scale=0.1, seed=2))
    _packed(m, dtype)
    x = rnd(n * t, c, dtype=dtype, seed=3).to(DEV)
    q = K.gemm(x, m.w.t, bias=m.b.t)
    got = K.depth_to_space(q, n, gh, gw, k, c, rows_per_image=t, row0=1)
    xi = x.float().view(n, t, c)[:, 1:].reshape(n, gh, gw, c).permute(0, 3, 1, 2)
    want = F.conv_transpose2d(xi, m.weight.to(DEV), m.bias.to(DEV), stride=k).permute(0, 2, 3, 1)
    assert got.shape == (n, gh * k, gw * k, c)
    _bar(f"convT k={k} c={c} {plane}", got.float(), want, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [32, 256])
def test_readout_gemm_with_the_class_token_as_row_bias(c, dtype):
    from controlanimate_amd.depth import _Readout
    K = _k()
    n, t = 3, 37
    m = _Readout(2 * c, c)
    with torch.no_grad():
        m.weight.copy_(rnd(c, 2 * c, dtype=dtype, scale=(2 * c) ** -0.5, seed=4).float())
        m.bias.copy_(rnd(c, dtype=torch.float32, scale=0.1, seed=5))
    _packed(m, dtype)
    hidden = rnd(n * t, c, dtype=dtype, seed=6).to(DEV)
    rb = K.gemm(hidden.view(n, t * c)[:, :c], m.w_cls.t, bias=m.b.t, out_f32=True)
    got = K.gemm(hidden, m.w_tok.t, rowbias=rb, rows_per_group=t, act=K.ACT_GELU).view(n, t, c)[:, 1:]
    h3 = hidden.float().view(n, t, c)
    tok, cls = h3[:, 1:], h3[:, :1]
    want = F.gelu(F.linear(torch.cat([tok, cls.expand_as(tok)], -1), m.weight.to(DEV), m.bias.to(DEV)))
    _bar(f"readout c={c}", got.float(), want, dtype)


# ---- the head ------------------------------------------------------------------------------------------------------------------------
def _head_case(cmid, plane, dtype, n=3):
    h, w = plane
    x = rnd(n, h, w, cmid, dtype=dtype, seed=10).to(DEV)
    w2 = rnd(32, cmid, 3, 3, dtype=dtype, scale=(9 * cmid) ** -0.5, seed=11).to(DEV)
    b2 = rnd(32, dtype=torch.float32, scale=0.3, seed=12).to(DEV)
    w3 = rnd(32, dtype=torch.float32, scale=32 ** -0.5, seed=13).to(DEV)
    b3 = torch.tensor([1.0], device=DEV)
    up = F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True)
    mid = F.relu(F.conv2d(up, w2.float(), b2, padding=1))
    pre = F.conv2d(mid, w3.view(1, 32, 1, 1), b3)[:, 0]
    return x, w2.permute(0, 2, 3, 1).contiguous(), b2, w3, b3, pre


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("plane", [(5, 7), (16, 24), (33, 20)])
@pytest.mark.parametrize("cmid", [32, 128])
def test_dpt_head_fused_and_composed(cmid, plane, dtype):
    K = _k()
    x, w2, b2, w3, b3, pre = _head_case(cmid, plane, dtype)
    clipped = (pre <= 0).float().mean().item()
    assert clipped < 0.3, f"the inputs clip {clipped:.2f} of the outputs"   # a condition on the inputs, checked in fp32
    want = F.relu(pre)
    assert K.dpt_head_supported(cmid)
    fused = K.dpt_head(x, w2, b2, w3, b3, fused=True)
    composed = K.dpt_head(x, w2, b2, w3, b3, fused=False)
    border = torch.ones_like(pre, dtype=torch.bool)
    border[:, 2:-2, 2:-2] = False
    for name, got in (("fused", fused), ("composed", composed)):
        assert got.shape == pre.shape and got.dtype == torch.float32
        for region, mask in (("border", border), ("interior", ~border)):
            _bar(f"head {name} cmid={cmid} {plane} {region} (clipped {clipped:.2f})", got[mask], want[mask], dtype)
        live = pre > 0.05                                                # away from the clip the output IS the pre-ReLU value
        _bar(f"head {name} cmid={cmid} {plane} pre-ReLU", got[live], pre[live], dtype)
    _bar(f"head fused against composed cmid={cmid} {plane}", fused, composed, dtype)


def test_dpt_head_widths():
    K = _k()
    assert [K.dpt_head_supported(c) for c in (32, 64, 128, 16, 96, 256)] == [True, True, True, False, False, False]
    x, w2, b2, w3, b3, pre = _head_case(64, (9, 11), torch.float16, n=1)
    _bar("head fused cmid=64", K.dpt_head(x, w2, b2, w3, b3, fused=True), F.relu(pre), torch.float16)
    x, w2, b2, w3, b3, pre = _head_case(16, (9, 11), torch.float16, n=1)   # a width the fused kernel does not take: the composed form serves it
    _bar("head composed cmid=16", K.dpt_head(x, w2, b2, w3, b3), F.relu(pre), torch.float16)


# ---- the tail --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    data, sd = R.load_fixture()
    return {"data": data, "sd": sd}


@pytest.mark.parametrize("n,src,dst", [(3, 96, (64, 96)), (3, 96, (200, 136)), (1, 384, (512, 768))])
def test_bicubic_tail_against_torch(fixture, n, src, dst):
    K = _k()
    if src == 96:
        d = torch.from_numpy(fixture["data"]["predicted_depth"]).to(DEV)
    else:
        d = F.relu(rnd(n, src, src, dtype=torch.float32, seed=20)).to(DEV)
    mm = torch.empty((n, 2), dtype=torch.float32, device=DEV)
    got, keys = K.resize_bicubic_f32(d, *dst, minmax=mm)
    want = F.interpolate(d[:, None], size=dst, mode="bicubic", align_corners=False)[:, 0]
    err = ((got - want).abs().max() / want.abs().max()).item()
    print(f"bicubic {src} -> {dst}: max_err/max_ref={err:.3e}")
    assert err < 1e-5
    assert torch.equal(mm[:, 0], got.amax((1, 2))) and torch.equal(mm[:, 1], got.amin((1, 2)))
    assert (mm[:, 1] < 0).all()                                            # the undershoot: why a float-as-integer maximum would be wrong


@pytest.mark.parametrize("rep", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("mode", ["max", "minmax"])
def test_finish_equals_the_numpy_specification(fixture, mode, dtype, rep):
    K = _k()
    post = fixture["data"]["post"]
    post = np.concatenate([post, np.zeros_like(post[:1])])                 # and an all-zero frame
    n, h, w = post.shape
    d = torch.from_numpy(post).to(DEV)
    _, keys = K.resize_bicubic_f32(d, h, w)                                # same size: the identity, and the keys of these very values
    lv = torch.empty((n, h, w), dtype=torch.uint8, device=DEV)
    ctrl = torch.empty((rep * n, 3, h, w), dtype=dtype, device=DEV)
    K.depth_finish(d, keys, mode, map=lv, control=ctrl, rep=rep)
    got = lv.cpu().numpy()
    for i in range(n - 1):
        scaled = (R.scaled_max if mode == "max" else R.scaled_minmax)(post[i])
        want = R.quantize_max(post[i])[0] if mode == "max" else R.quantize_minmax(post[i])
        near = (np.abs(scaled - np.rint(scaled)) < 1e-3) & (post[i] != 0)    # (an exact zero of the map is zero under any rounding: it must match)
        assert near.mean() <= 0.01
        assert np.array_equal(got[i][~near], want[~near]), i
        assert np.abs(got[i].astype(int) - want.astype(int)).max() <= 1
        if mode == "max" and i < 3:
            sat = scaled <= -1
            assert sat.sum() > 0 and (got[i][sat] == 0).all()
    assert (got[3] == 0).all()
    want_ctrl = torch.cat([(lv.cpu().float() / 255.0)[:, None].expand(-1, 3, -1, -1)] * rep).to(dtype)   # (divided on the host: IEEE division)
    assert torch.equal(ctrl.cpu(), want_ctrl)


# ---- end to end on the tiny model ------------------------------------------------------------------------------------------------------
def _annotator(sd, dtype, normalize="max", cfg=R.TINY_CONFIG, resample=3):
    from controlanimate_amd.depth import DepthAnnotator, DPTForDepthEstimation
    with torch.device(DEV):
        model = DPTForDepthEstimation(**cfg)
    model.load_state_dict({k: v.to(DEV) for k, v in sd.items()}, strict=True)
    model.to(dtype)
    return DepthAnnotator(model, cfg["image_size"], resample, normalize, device=DEV)


@pytest.fixture(scope="module")
def tiny(fixture):
    return {dt: _annotator(fixture["sd"], dt) for dt in DTYPES}


def _per_frame(got, want):
    return [((got[i] - want[i]).norm() / want[i].norm()).item() for i in range(len(want))]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_e2e_predicted_depth(fixture, tiny, dtype, fused, monkeypatch):
    from controlanimate_amd.context import dispatch
    monkeypatch.setattr(dispatch, "dpt_head_fused", fused)
    ann, data = tiny[dtype], fixture["data"]
    ann.model.taps = []
    got = ann.predicted_depth(list(data["frames"]))
    taps, ann.model.taps = ann.model.taps, None
    want = torch.from_numpy(data["predicted_depth"]).to(DEV)
    rels = _per_frame(got, want)
    tap_rels = [((t.float() - torch.from_numpy(data[f"tap{j}"]).to(DEV)).norm() / torch.from_numpy(data[f"tap{j}"]).norm()).item() for j, t in enumerate(taps)]
    print(f"e2e {dtype} fused={fused}: per-frame rel_l2 {['%.2e' % r for r in rels]}, taps {['%.2e' % r for r in tap_rels]}")
    assert torch.isfinite(got).all() and max(rels) <= E2E_BAR[dtype]
    assert max(tap_rels) <= E2E_BAR[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_e2e_seven_frames_as_four_and_three(fixture, tiny, dtype):
    ann, data = tiny[dtype], fixture["data"]
    frames = [data["frames"][i % 3] for i in range(7)]
    ann.chunk_frames = 4
    try:
        got = ann.predicted_depth(frames)
    finally:
        ann.chunk_frames = 16
    want = torch.from_numpy(data["predicted_depth"]).to(DEV)[[i % 3 for i in range(7)]]
    rels = _per_frame(got, want)
    print(f"e2e 4 + 3 {dtype}: {['%.2e' % r for r in rels]}")
    assert max(rels) <= E2E_BAR[dtype]


def test_e2e_uint8_map_against_a_torch_fp16_run(fixture, tiny):
    """The yardstick is measured first: the largest level difference between a plain torch fp16 run of depth_ref (and the fp32 tail) and
    the fp32 fixture.  The product may exceed it by one level at most.  (Recorded in profiles/depth_bench.json by tools/bench_depth.py.)"""
    data, sd = fixture["data"], fixture["sd"]
    h, w = data["frames"].shape[1:3]
    pv = torch.from_numpy(data["pixel_values_r3"]).to(DEV)
    with torch.no_grad():
        d16 = R.forward({k: v.to(DEV).half() for k, v in sd.items()}, R.TINY_CONFIG, pv.half())[0].float()
    post16 = F.interpolate(d16[:, None], size=(h, w), mode="bicubic", align_corners=False)[:, 0].cpu().numpy()
    for mode, ann in (("max", tiny[torch.float16]), ("minmax", _annotator(sd, torch.float16, "minmax"))):
        q = (lambda p: R.quantize_max(p)[0]) if mode == "max" else R.quantize_minmax
        want = np.stack([q(p) for p in data["post"]]).astype(int)
        torch16 = max(np.abs(q(post16[i]).astype(int) - want[i]).max() for i in range(3))
        got = ann.depth(list(data["frames"])).cpu().numpy().astype(int)
        ours = np.abs(got - want).max()
        print(f"uint8 map {mode}: largest level difference torch fp16 {torch16}, product {ours}")
        assert ours <= torch16 + 1
        if mode == "minmax":
            print(f"   against the recorded pipeline image: {np.abs(got - data['pipeline_depth'].astype(int)).max()}")


def test_e2e_call_and_batch_contracts(fixture, tiny):
    from PIL import Image
    ann, frames = tiny[torch.float16], fixture["data"]["frames"]
    lv = ann.depth(list(frames))
    assert lv.dtype == torch.uint8 and tuple(lv.shape) == (3, 64, 96) and lv.is_cuda and 100 <= len(torch.unique(lv[0]))
    ctrl = ann.annotate_batch(torch.from_numpy(frames).to(DEV), rep=2, dtype=torch.float16)
    assert tuple(ctrl.shape) == (6, 3, 64, 96) and torch.equal(ctrl[:3], ctrl[3:]) and torch.equal(ctrl[:3, 0].cpu(), (lv.cpu().float() / 255).half())
    img = ann(Image.fromarray(frames[1]))
    assert isinstance(img, Image.Image) and img.mode == "RGB" and img.size == (96, 64)
    assert np.array_equal(np.asarray(img)[:, :, 2], lv[1].cpu().numpy())
    assert isinstance(ann(frames[1]), np.ndarray)
    with pytest.raises(TypeError):
        ann.depth([frames[0].astype(np.float32)])
    with pytest.raises(ValueError):
        ann.depth([frames[0], frames[1][:32]])
    ann.timings = {}
    ann.depth(list(frames))
    timed, ann.timings = ann.timings, None
    torch.cuda.synchronize()
    assert set(timed) == {"resize", "vit", "reassemble", "fusion", "head", "tail"}


def test_e2e_chain_replays_in_a_captured_graph(fixture, tiny):
    """No launch of the chain waits for the host: captured once (a linear chain, no parallel branches), it replays for new frames copied
    into the captured buffer, to the same bits as eager."""
    ann, frames = tiny[torch.float16], fixture["data"]["frames"]
    eager = [ann.annotate_batch(torch.from_numpy(f).to(DEV), rep=2).clone() for f in (frames, frames[::-1].copy())]
    buf = torch.from_numpy(frames).to(DEV)
    out = torch.empty((6, 3, 64, 96), dtype=torch.float32, device=DEV)
    ann.annotate_batch(buf, out=out, rep=2)   # warm-up: the weights and the tables are on the device before the capture
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


@pytest.mark.parametrize("name", ["lllyasviel/sd-controlnet-depth", "lllyasviel/control_v11f1p_sd15_depth"])
def test_prep_control_images_leaves_the_doubled_tensor(fixture, tiny, name):
    from PIL import Image
    from controlanimate_amd.configs import controlnet_config
    from controlanimate_amd.controlnet import ControlNetModel
    from controlanimate_amd.controlresiduals_pipeline import MultiControlNetResidualsPipeline
    ann, frames = tiny[torch.float16], [Image.fromarray(f) for f in fixture["data"]["frames"]]
    net = ControlNetModel.from_config(controlnet_config(block_out_channels=(32, 64, 64, 64)))
    pipe = MultiControlNetResidualsPipeline([name], [1.0], use_lcm=False, controlnets=[net], device="cuda", annotators={"depth": ann})
    pipe.prep_control_images(frames, do_classifier_free_guidance=True)
    got = pipe.prep_images[0]
    want = ann.annotate_batch(frames, rep=2)
    assert got.shape == (6, 3, 64, 96) and got.is_cuda and got._cfg_doubled is True
    assert torch.equal(got, want.to(got.dtype)) and 0.05 < got.mean() < 0.95


# ---- one full-width pass -------------------------------------------------------------------------------------------------------------
def test_full_width_frame_against_the_fp32_specification():
    """One frame through DPT-large-shaped seeded weights generated on the device, against depth_ref in fp32 on the device: the same 1e-2
    bar, and no fp16 intermediate is non-finite."""
    cfg = R.LARGE_CONFIG
    sd = {k: v.half().float() for k, v in R.seeded_state_dict(cfg, seed=1, device=DEV).items()}
    ann = _annotator(sd, torch.float16, cfg=cfg)
    frame = torch.from_numpy(_smooth_frames(1, 384, 384, seed=9)).to(DEV)
    ann.model.taps, ann.model.stored = [], []
    got = ann.predicted_depth(frame)
    kept = ann.model.taps + ann.model.stored
    ann.model.taps = ann.model.stored = None
    pv = (frame.float().permute(0, 3, 1, 2) / 255 - 0.5) / 0.5
    with torch.no_grad():
        want, taps = R.forward(sd, cfg, pv)
    rel = ((got - want).norm() / want.norm()).item()
    largest = max(t.float().abs().max().item() for t in kept)
    print(f"full width: rel_l2={rel:.3e}, zero share {(want == 0).float().mean().item():.2f}, largest fp16 intermediate {largest:.1f}, "
          f"largest fp32 hidden state {max(t.abs().max().item() for t in taps):.1f}")
    assert len(kept) == 4 + 10 and all(torch.isfinite(t).all() for t in kept)
    assert torch.isfinite(got).all() and want.max() > 0 and rel <= 1e-2
