"""GPU: the M-LSD annotator (controlanimate_amd/mlsd.py, csrc/ca_mlsd.hip) against its specification (tests/mlsd_ref.py): ReLU6 in the
GEMM and convolution epilogues, the depthwise convolution, the align-corners upsample into half of a concatenation, the dilated
convolution, block B's ReLU-then-add, the decode and the line drawing on their own, and the whole chain end to end.

Tolerances: GEMMs and convolutions use the bar of tests/test_lineart_gpu.py (relative L2 < 2.5 * eps, eps = 2^-10 for fp16 and 2^-8 for
bf16, largest error < 4 x that of the largest reference value); the upsample is within relative L2 2^-10 (fp16) / 2^-7 (bf16) of a float64
reference on the same rounded input (the InstanceNorm bar: twice the output's half-ulp), its corners bit-equal to the source corners and
the other half of the concatenation bit-unchanged; the decode's segments and the drawn bytes equal the numpy specification exactly on
inputs that mlsd_ref.decided() accepts; control == map / 255 exactly; the end-to-end tpMap meets the project's fp16 bar (relative L2 <=
1e-2 over channels 0..4; bf16 8e-2).  A CPU emulation of the chain that stores every activation in fp16 (mlsd_ref.tpmap_emulated) gave
3.4e-3 (bf16: 2.1e-2) on this file's seed at centre logits of standard deviation 2, 2.9 x (3.9 x) under the bar; the device measured
3.2e-3 (2.5e-2).  tests/test_mlsd_cpu.py prints the emulation's figure for its own seed (1.9e-3 / 1.2e-2).
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlsd_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAME = "lllyasviel/control_v11p_sd15_mlsd"
CONV_BAR = {torch.float16: 2.5 * 2.0 ** -10, torch.bfloat16: 2.5 * 2.0 ** -8}  # tests/test_lineart_gpu.py
E2E_SEED = 11  # a seed whose device tpMap is `decided` (no decision of the decode within rounding of its threshold)


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


# ---- ReLU6 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_relu6_gemm(dtype):
    k = _k()
    a, w = rnd(77, 16, dtype=dtype, scale=3.0, seed=1), rnd(24, 16, dtype=dtype, seed=2)
    bias = rnd(24, dtype=torch.float32, seed=3)
    pre = a.float() @ w.float().t() + bias
    assert pre.max() > 8 and pre.min() < -8                       # values beyond both ends of [0, 6]
    out = k.gemm(a.to(DEV), w.to(DEV), bias=bias.to(DEV), act=k.ACT_RELU6)
    torch.cuda.synchronize()
    got = out.float().cpu()
    assert got.max() == 6.0 and got.min() == 0.0
    _conv_bar("gemm relu6 77x24x16", got, pre.clamp(0, 6), dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_relu6_stem_convolution(dtype):
    k = _k()
    x = rnd(2, 12, 20, 8, dtype=dtype, seed=4)
    wt = rnd(32, 8, 3, 3, dtype=dtype, scale=0.6, seed=5)
    bias = rnd(32, dtype=torch.float32, seed=6)
    pre = F.conv2d(F.pad(x.float().permute(0, 3, 1, 2), (0, 1, 0, 1)), wt.float(), bias, stride=2).permute(0, 2, 3, 1)
    assert pre.max() > 7 and pre.min() < -7
    out = k.conv3x3(x.to(DEV), wt.permute(0, 2, 3, 1).contiguous().to(DEV), bias=bias.to(DEV), stride=2, pad_asym=True, act=k.ACT_RELU6)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (2, 6, 10, 32)
    got = out.float().cpu()
    assert got.max() == 6.0 and got.min() == 0.0
    _conv_bar("stem 2x12x20x8->32 s2", got, pre.clamp(0, 6), dtype)


# ---- depthwise -------------------------------------------------------------------------------------------------------------------
DW_CASES = [((2, 5, 7, 16), 1), ((1, 6, 10, 96), 1), ((1, 6, 10, 96), 2), ((1, 9, 70, 384), 1), ((1, 40, 72, 576), 1), ((1, 40, 72, 576), 2)]


@pytest.mark.parametrize("relu6", [True, False])
@pytest.mark.parametrize("shape,stride", DW_CASES)   # (5 x 7: one partial strip; 9 x 70: two strips; 40 x 72 x 576: many blocks, every channel group)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_depthwise(shape, stride, relu6, dtype):
    from controlanimate_amd.mlsd import pack_depthwise
    k = _k()
    n, h, w, c = shape
    x = rnd(*shape, dtype=dtype, scale=2.0, seed=11)
    wt = rnd(c, 1, 3, 3, dtype=dtype, scale=0.8, seed=12)
    bias = rnd(c, dtype=torch.float32, seed=13)
    xin = x.float().permute(0, 3, 1, 2)
    if stride == 2:
        pre = F.conv2d(F.pad(xin, (0, 1, 0, 1)), wt.float(), bias, stride=2, groups=c)
    else:
        pre = F.conv2d(xin, wt.float(), bias, padding=1, groups=c)
    ref = (pre.clamp(0, 6) if relu6 else pre).permute(0, 2, 3, 1)
    assert pre.max() > 6.5 and pre.min() < -0.5
    out = torch.full((n, h // stride, w // stride, c), float("nan"), dtype=dtype, device=DEV)
    k.dwconv3x3(x.to(DEV), pack_depthwise(wt).to(DEV), bias.to(DEV), stride=stride, relu6=relu6, out=out)
    torch.cuda.synchronize()
    _conv_bar(f"depthwise {shape} s{stride} relu6={relu6}", out.float().cpu(), ref, dtype)


def test_depthwise_rejects_odd_sizes_at_stride_2():
    from controlanimate_amd._capi import CAHipError
    from controlanimate_amd.mlsd import pack_depthwise
    k = _k()
    for shape in ((1, 5, 8, 16), (1, 6, 7, 16)):
        x = rnd(*shape).to(DEV)
        with pytest.raises(CAHipError, match="even"):
            k.dwconv3x3(x, pack_depthwise(rnd(16, 1, 3, 3)).to(DEV), torch.zeros(16, device=DEV), stride=2)


# ---- upsample --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(3, 5), (4, 8)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_upsample_writes_one_half_of_the_concatenation(h, w, dtype):
    k = _k()
    n = 2
    x = rnd(n, h, w, 64, dtype=dtype, seed=21)
    sentinel = torch.full((n, 2 * h, 2 * w, 128), -7.25, dtype=dtype)
    out = sentinel.clone().to(DEV)
    k.upsample2x_bilinear_ac(x.to(DEV), out, col0=64)
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(got[..., :64].view(torch.int16), sentinel[..., :64].view(torch.int16))            # the other half: bit-unchanged
    ref = F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2.0, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    up = got[..., 64:]
    rel = ((up.double() - ref).norm() / ref.norm()).item()
    tol = 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7
    print(f"upsample {h}x{w} {dtype}: relative L2 {rel:.3e} (tol {tol:.2e})")
    assert torch.isfinite(up).all() and rel <= tol
    for (oy, ox), (iy, ix) in (((0, 0), (0, 0)), ((0, 2 * w - 1), (0, w - 1)), ((2 * h - 1, 0), (h - 1, 0)), ((2 * h - 1, 2 * w - 1), (h - 1, w - 1))):
        assert torch.equal(up[:, oy, ox].view(torch.int16), x[:, iy, ix].view(torch.int16))              # corners: exactly the source corners


# ---- dilated convolution ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", [(1, 7, 9), (2, 12, 20), (1, 33, 18)])   # (7 x 9: smaller than the dilation's reach; 33 x 18: partial tiles both ways)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_dilated_convolution(n, h, w, dtype):
    k = _k()
    x = rnd(n, h, w, 64, dtype=dtype, seed=31)
    wt = rnd(64, 64, 3, 3, dtype=dtype, scale=(2.0 / 576) ** 0.5, seed=32)
    g = torch.Generator().manual_seed(33)
    wt = (wt.float() * (1.0 + torch.arange(64).view(64, 1, 1, 1) / 64.0) * (1.0 + torch.rand(1, 64, 3, 3, generator=g))).to(dtype)   # asymmetric in every index
    bias = rnd(64, dtype=torch.float32, seed=34)
    pre = F.conv2d(x.float().permute(0, 3, 1, 2), wt.float(), bias, padding=5, dilation=5).permute(0, 2, 3, 1)
    for relu in (True, False):
        out = torch.full((n, h, w, 64), float("nan"), dtype=dtype, device=DEV)
        k.conv3x3_dil(x.to(DEV), wt.permute(0, 2, 3, 1).contiguous().to(DEV), bias.to(DEV), relu=relu, out=out)
        torch.cuda.synchronize()
        _conv_bar(f"dilated {(n, h, w)} relu={relu}", out.float().cpu(), pre.clamp_min(0) if relu else pre, dtype)


# ---- block B: ReLU, then the skip ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_block_b_relu_then_add(dtype):
    k = _k()
    n, h, w = 2, 6, 10
    x = rnd(n, h, w, 128, dtype=dtype, seed=41)
    w1 = rnd(128, 128, 3, 3, dtype=dtype, scale=(2.0 / 1152) ** 0.5, seed=42)
    w2 = rnd(64, 128, 3, 3, dtype=dtype, scale=(2.0 / 1152) ** 0.5, seed=43)
    b1, b2 = rnd(128, dtype=torch.float32, scale=0.3, seed=44), rnd(64, dtype=torch.float32, scale=0.3, seed=45)
    xin = x.float().permute(0, 3, 1, 2)
    t = (F.conv2d(xin, w1.float(), b1, padding=1).clamp_min(0)).to(dtype).float()
    s = (t + xin).to(dtype).float()
    assert (s < 0).any()                                          # add-then-ReLU would have cut these
    ref = F.conv2d(s, w2.float(), b2, padding=1).clamp_min(0).permute(0, 2, 3, 1)
    xd = x.to(DEV)
    td = k.conv3x3(xd, w1.permute(0, 2, 3, 1).contiguous().to(DEV), bias=b1.to(DEV), act=k.ACT_RELU)
    k.add_bcast(td, xd, out=td)
    torch.cuda.synchronize()
    _conv_bar("block B conv1(x) + x", td.float().cpu(), s.permute(0, 2, 3, 1), dtype)
    out = k.conv3x3(td, w2.permute(0, 2, 3, 1).contiguous().to(DEV), bias=b2.to(DEV), act=k.ACT_RELU)
    torch.cuda.synchronize()
    _conv_bar("block B", out.float().cpu(), ref, dtype)


# ---- decode ----------------------------------------------------------------------------------------------------------------------
def _rows(a):
    return sorted(map(tuple, np.asarray(a).reshape(-1, 4).tolist()))


@pytest.mark.parametrize("name", ["few", "plateau", "many", "short", "saturated"])
def test_decode_equals_the_numpy_specification(name):
    k = _k()
    tp = mlsd_ref.saturated_case() if name == "saturated" else mlsd_ref.decode_cases()[name]
    assert name == "saturated" or mlsd_ref.decided(tp)
    want = mlsd_ref.decode_ref(tp)
    both = torch.from_numpy(np.stack([tp, tp[::-1, ::-1].copy()])).to(DEV)            # a second frame: the first one turned by 180 degrees
    seg, cnt = k.mlsd_decode(both, 0.1, 0.1)
    torch.cuda.synchronize()
    seg, cnt = seg.cpu().numpy(), cnt.cpu().numpy()
    assert seg.shape == (2, 200, 4) and seg.dtype == np.int32 and cnt.tolist()[0] == len(want)
    assert _rows(seg[0, :cnt[0]]) == _rows(want)                                       # the set
    if name != "plateau":
        assert np.array_equal(seg[0, :cnt[0]], want)                                   # and, scores being distinct (or the index deciding), the rank order
    assert (seg[0, cnt[0]:] == 0).all()
    if name != "saturated":                                                            # (turned, a plateau's ties fall to other pixels)
        assert cnt[1] == len(mlsd_ref.decode_ref(tp[::-1, ::-1])) and _rows(seg[1, :cnt[1]]) == _rows(mlsd_ref.decode_ref(tp[::-1, ::-1]))
    again, cnt2 = k.mlsd_decode(both, 0.1, 0.1)
    assert torch.equal(again.cpu(), torch.from_numpy(seg)) and torch.equal(cnt2.cpu(), torch.from_numpy(cnt))     # the same bits twice


def test_decode_thresholds_are_arguments():
    k = _k()
    tp = mlsd_ref.decode_cases()["many"]
    for thr_v, thr_d in ((0.7, 0.1), (0.1, 6.0)):
        assert mlsd_ref.decided(tp, thr_v, thr_d)
        want = mlsd_ref.decode_ref(tp, thr_v, thr_d)
        seg, cnt = k.mlsd_decode(torch.from_numpy(tp[None]).to(DEV), thr_v, thr_d)
        assert 0 < len(want) < 200 and int(cnt[0]) == len(want) and _rows(seg[0, :len(want)].cpu().numpy()) == _rows(want)


# ---- draw ------------------------------------------------------------------------------------------------------------------------
def _segments(cases, names):
    seg = np.zeros((len(names), 200, 4), np.int32)
    cnt = np.zeros((len(names),), np.int32)
    for i, nm in enumerate(names):
        seg[i, :len(cases[nm])] = cases[nm]
        cnt[i] = len(cases[nm])
    return seg, cnt


@pytest.mark.parametrize("rep", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_draw_equals_the_numpy_specification(rep, dtype):
    k = _k()
    cases = mlsd_ref.draw_cases()
    names = list(cases)
    assert len(cases["empty"]) == 0 and len(cases["random200"]) == 200                 # count = 0 and count = 200
    seg, cnt = _segments(cases, names)
    seg[names.index("axes"), 4:] = 77                                                  # entries past the count are not drawn
    h, w, n = 64, 128, len(names)
    want = np.stack([mlsd_ref.draw_ref(cases[nm], h, w) for nm in names])
    edges = torch.full((n, h, w), 3, dtype=torch.uint8, device=DEV)
    ctrl = torch.full((rep * n, 3, h, w), 7.0, dtype=dtype, device=DEV)
    k.mlsd_draw(torch.from_numpy(seg).to(DEV), torch.from_numpy(cnt).to(DEV), h, w, edges=edges, control=ctrl, rep=rep)
    torch.cuda.synchronize()
    got = edges.cpu().numpy()
    for i, nm in enumerate(names):
        assert np.array_equal(got[i], want[i]), f"{nm}: {(got[i] != want[i]).sum()} pixels differ, first at {np.argwhere(got[i] != want[i])[:1]}"
    assert want[names.index("empty")].sum() == 0 and want[names.index("outside")].sum() > 0
    level = edges.cpu().float() / 255.0
    c = ctrl.cpu()
    for r in range(rep):
        for ch in range(3):
            assert torch.equal(c[r * n:(r + 1) * n, ch], level.to(dtype))
    assert set(c.unique().tolist()) == {0.0, 1.0}
    only_e = k.mlsd_draw(torch.from_numpy(seg).to(DEV), torch.from_numpy(cnt).to(DEV), h, w)
    assert torch.equal(only_e, edges)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def _rounded(sd, dtype):
    return {k: (v.to(dtype).float() if v.dim() == 4 else v) for k, v in sd.items()}


def _ann(sd, **kw):
    from controlanimate_amd.annotators import MlsdAnnotator
    return MlsdAnnotator(sd, DEV, detect_resolution=64, image_resolution=64, **kw)


@pytest.fixture(scope="module")
def e2e():
    """Two 64 x 128 frames, seeded weights rounded to fp16 (what the device holds), the fp32 reference's tpMap -- computed once -- and the
    annotator."""
    sd = _rounded(mlsd_ref.mlsd_state_dict(seed=E2E_SEED), torch.float16)
    frames = mlsd_ref.frames_fixture()
    return {"sd": sd, "frames": frames, "tp": mlsd_ref.tpmap_ref(sd, frames)[..., :5], "ann": _ann(sd)}


def test_e2e_tpmap(e2e):
    got = e2e["ann"].tpmap(list(e2e["frames"]))
    torch.cuda.synchronize()
    assert tuple(got.shape) == (2, 32, 64, 8) and got.dtype == torch.float32 and got.is_cuda
    got, ref = got.cpu(), e2e["tp"]
    assert (got[..., 5:] == 0).all()
    rel = ((got[..., :5] - ref).norm() / ref.norm()).item()
    per = [((got[..., c] - ref[..., c]).norm() / ref[..., c].norm()).item() for c in range(5)]
    print(f"fp16 tpMap: relative L2 {rel:.3e} (per channel {np.array2string(np.array(per), precision=2)}); reference centre std {float(ref[..., 0].std()):.2f}")
    assert torch.isfinite(got).all() and rel <= 1e-2


def test_e2e_bfloat16_runs_the_same_chain(e2e):
    sd = _rounded(mlsd_ref.mlsd_state_dict(seed=E2E_SEED), torch.bfloat16)
    ref = mlsd_ref.tpmap_ref(sd, e2e["frames"])[..., :5]
    got = _ann(sd, dtype=torch.bfloat16).tpmap(list(e2e["frames"])).cpu()[..., :5]
    rel = ((got - ref).norm() / ref.norm()).item()
    print(f"bf16 tpMap: relative L2 {rel:.3e}")
    assert torch.isfinite(got).all() and rel <= 8e-2  # 8 x the fp16 bar: bf16 carries 3 bits less


def test_e2e_map_is_the_drawing_of_the_decode_of_the_chains_own_tpmap(e2e):
    k, ann, frames = _k(), e2e["ann"], e2e["frames"]
    tp = ann.tpmap(torch.from_numpy(frames).to(DEV))
    seg, cnt = k.mlsd_decode(tp, 0.1, 0.1)
    alone = k.mlsd_draw(seg, cnt, 64, 128)
    got = ann.edges(list(frames))
    assert got.dtype == torch.uint8 and got.is_cuda and torch.equal(got, alone)
    share = (got == 255).float().mean().item()
    print(f"segments per frame {cnt.tolist()}, share of line pixels {share:.3f}")
    assert set(got.unique().tolist()) == {0, 255} and 0.005 < share < 0.9          # neither empty nor full
    # the specification's decode of that tpMap: the device's segments, then its map
    tph, segh, cnth = tp.cpu().numpy(), seg.cpu().numpy(), cnt.cpu().numpy()
    for i in range(2):
        assert mlsd_ref.decided(tph[i]), f"frame {i}: the device tpMap of seed {E2E_SEED} has a decision within rounding of its threshold"
        want = mlsd_ref.decode_ref(tph[i])
        assert cnth[i] == len(want) and np.array_equal(segh[i, :cnth[i]], want)
        assert np.array_equal(got[i].cpu().numpy(), mlsd_ref.detect_ref(tph[i]))
    # frame chunks: one frame per pass through the network gives the same bytes
    one = _ann(e2e["sd"])
    one.max_activation_bytes = 64 * 128 * 64
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
    from controlanimate_amd.mlsd import STAGES
    ann, frames = e2e["ann"], e2e["frames"]
    plain = ann.edges(list(frames)).clone()
    ann.timings = {}
    try:
        timed = ann.edges(list(frames))
        torch.cuda.synchronize()
        assert {k: len(v) for k, v in ann.timings.items()} == STAGES == {"prep": 1, "stem": 1, "pointwise": 33, "depthwise": 13, "upsample": 3, "conv": 9,
                                                                          "add": 4, "dilated": 1, "head": 1, "decode": 1, "draw": 1}
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
    assert 0.005 < out.mean() < 0.9


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
    pipe = MultiControlNetResidualsPipeline([NAME], [1.0], use_lcm=False, controlnets=[net], device="cuda", annotators={"mlsd": Counting()})
    pipe.prep_control_images(frames, do_classifier_free_guidance=cfg)
    rep = 2 if cfg else 1
    assert len(calls) == 1 and calls[0]["n"] == 2 and calls[0]["rep"] == rep and calls[0]["out"] is None and calls[0]["dtype"] == torch.float32
    got = pipe.prep_images[0]
    want = torch.cat([(ann.edges(frames).cpu().float() / 255.0)[:, None].expand(-1, 3, -1, -1)] * rep)
    assert got.shape == (2 * rep, 3, 64, 128) and got.dtype == torch.float32 and got.is_cuda and got._cfg_doubled is cfg
    assert torch.equal(got.cpu(), want) and 0.005 < got.mean() < 0.9
    ptr = got.data_ptr()
    pipe.prep_control_images(frames[::-1], do_classifier_free_guidance=cfg)  # the next window goes into the tensor the ControlNets hold
    assert len(calls) == 2 and calls[1]["out"] is got and pipe.prep_images[0] is got and got.data_ptr() == ptr
    assert torch.equal(got[:2].cpu(), want[:2].flip(0))
    # the annotator itself plugs in under the same key, for the other ControlNet name too
    direct = MultiControlNetResidualsPipeline(["lllyasviel/sd-controlnet-mlsd"], [1.0], use_lcm=False, controlnets=[net], device="cuda", annotators={"mlsd": ann})
    direct.prep_control_images(frames[::-1], do_classifier_free_guidance=cfg)
    assert torch.equal(direct.prep_images[0], got)
