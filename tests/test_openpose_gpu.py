"""GPU: the OpenPose body annotator (controlanimate_amd/openpose.py, csrc/ca_openpose.hip) against its specification (tests/pose_ref.py).

Discrete decisions are tested where they are exact (peaks, matching, assembly, rasterisation: equality with the numpy / float64
specification on the same fp32 maps), numerics where they are continuous (the convolutions, the resampling, the network): no test
compares a drawing across a rounding difference.

Tolerances: ca_conv7x7 and its im2col + ca_gemm form use the bar of tests/test_lineart_gpu.py (relative L2 < 2.5 * eps, eps = 2^-10 for
fp16 and 2^-8 for bf16, largest error < 4 x that of the largest reference value) against fp32 F.conv2d on the same rounded operands; an
image gives the same bits alone and inside a batch (the direct form, whose reduction is never split; ca_gemm's split-K depends on the
number of rows, so the other form is not asked that).  ca_pose_prep is byte-exact.  ca_pose_maps: max |err| <= 2^-17 max |ref| against the
float64 specification (fp32 accumulation of at most 35 + 23 products per output with sum |w| <= 2 per axis: 2^-24 * 58 * 2).  The 57
low-resolution maps meet the project's bar against the fp32 reference: relative L2 <= 1e-2 (fp16) / 8e-2 (bf16); the CPU emulation that
stores every activation in fp16 gave 1.1e-3 on this file's seed (tests/test_openpose_cpu.py prints it); the device measured 6.3e-4
(bf16: 5.0e-3), and 6.4e-4 between the two forms of the 7x7 convolutions.  ca_pose_maps measured 2.5e-7 of the largest value."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ("lllyasviel/control_v11p_sd15_openpose", "lllyasviel/sd-controlnet-openpose")
CONV_BAR = {torch.float16: 2.5 * 2.0 ** -10, torch.bfloat16: 2.5 * 2.0 ** -8}  # tests/test_lineart_gpu.py
E2E_BAR = {torch.float16: 1e-2, torch.bfloat16: 8e-2}
E2E_SEED = 0  # a seed whose device maps are `decided` (no decision of the decode within rounding of its threshold)
H, W = R.PLANT_H, R.PLANT_W


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


# ---- the 7x7 convolution ----------------------------------------------------------------------------------------------------------
def _conv7_case(n, h, w, cin, cout, dtype, seed, groups=1):
    xs, ws, bs = [], [], []
    for g in range(groups):
        x = rnd(n, h, w, cin, dtype=dtype, seed=seed + 10 * g)
        if n > 1:
            x[1:] = x[1:] * 100   # a halo read across the image border would show
        xs.append(x)
        ws.append(rnd(cout, 7, 7, cin, dtype=dtype, scale=(49 * cin) ** -0.5, seed=seed + 10 * g + 1))
        bs.append(rnd(cout, dtype=torch.float32, seed=seed + 10 * g + 2))
    return xs, ws, bs


def _conv7_ref(x, w, b, relu):
    y = F.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), b, padding=3).permute(0, 2, 3, 1)
    return F.relu(y) if relu else y


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "im2col_gemm"])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", [(1, 3, 5, 128, 128), (2, 9, 11, 192, 128)])
def test_conv7x7(shape, dtype, relu, direct):
    k = _k()
    xs, ws, bs = _conv7_case(*shape, dtype, seed=3)
    out = k.conv7x7([xs[0].to(DEV)], [ws[0].to(DEV)], biases=[bs[0].to(DEV)], relu=relu, direct=direct)[0]
    torch.cuda.synchronize()
    ref = _conv7_ref(xs[0], ws[0], bs[0], relu)
    for i in range(shape[0]):   # per image: the second one holds values 100 x larger
        _conv_bar(f"conv7x7 {shape} image {i} relu={relu} direct={direct}", out[i].float().cpu(), ref[i], dtype)
    if direct and shape[0] > 1:   # the same image alone: the same bits (the second one then runs in the blocks the first one had)
        for i in range(shape[0]):
            alone = k.conv7x7([xs[0][i:i + 1].to(DEV)], [ws[0].to(DEV)], biases=[bs[0].to(DEV)], relu=relu, direct=True)[0]
            assert torch.equal(alone[0], out[i]), i


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "im2col_gemm"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_conv7x7_grouped_into_column_ranges(dtype, direct):
    """Two problems with different inputs and weights in one call; the inputs are column ranges of 192-wide tensors, the outputs are
    column ranges of a 256-wide one whose other columns stay untouched."""
    k = _k()
    xs, ws, bs = _conv7_case(2, 9, 11, 128, 128, dtype, seed=5, groups=2)
    wide = torch.zeros((2, 2, 9, 11, 192), dtype=dtype)   # (the problems of a call share one pixel stride)
    wide[0, ..., 64:], wide[1, ..., 64:] = xs[0], xs[1]
    wide_d = wide.to(DEV)
    x1 = wide_d[1, ..., 64:]
    wide_d = wide_d[0]
    out = torch.full((2, 9, 11, 256), 7.0, dtype=dtype, device=DEV)
    k.conv7x7([wide_d[..., 64:], x1], [w.to(DEV) for w in ws], biases=[b.to(DEV) for b in bs], relu=True, outs=[out[..., :128], out[..., 128:]], direct=direct)
    torch.cuda.synchronize()
    for g in range(2):
        ref = _conv7_ref(xs[g], ws[g], bs[g], True)
        for i in range(2):   # per image: the second one holds values 100 x larger
            _conv_bar(f"conv7x7 grouped problem {g} image {i} direct={direct}", out[i, ..., g * 128:(g + 1) * 128].float().cpu(), ref[i], dtype)
    assert out.shape[3] == 256   # (both halves written: nothing of the 7.0 fill is left)
    assert not bool((out == 7.0).all(dim=3).any())


def test_conv7x7_rejects_bad_arguments():
    k = _k()
    x, w = rnd(1, 4, 4, 24).to(DEV), rnd(64, 7, 7, 24).to(DEV)
    from controlanimate_amd._capi import CAHipError
    with pytest.raises(CAHipError, match="ca_conv7x7"):
        k.conv7x7([x], [w], direct=True)   # cin % 32


# ---- prep -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(192, 256), (256, 320), (512, 768)])
def test_pose_prep_is_byte_exact(hw):
    from controlanimate_amd import openpose as O
    k = _k()
    frames = R.frames_fixture(1, *hw, seed=4)
    g = O.geometry(*hw)
    assert hw != (512, 768) or (g["ws"], g["wp"]) == (276, 280)
    tables = tuple(torch.from_numpy(a).to(DEV) for a in (*O.area_tables(hw[1], g["ws"], g["scale"]), *O.area_tables(hw[0], g["hs"], g["scale"])))
    out = torch.empty((1, g["hp"], g["wp"], 8), dtype=torch.float16, device=DEV)
    k.pose_prep(torch.from_numpy(frames).to(DEV), tables, g["hs"], g["ws"], out)
    torch.cuda.synchronize()
    got = ((out[0, :, :, :3].float().cpu() + 0.5) * 256).numpy()
    want = R.input_bytes(frames[0]).astype(np.float32)
    assert np.array_equal(got, want), f"{(got != want).sum()} bytes differ, max {np.abs(got - want).max()}"
    assert float(out[..., 3:].abs().max()) == 0.0


# ---- maps ---------------------------------------------------------------------------------------------------------------------------
def _device_maps(ann, low_paf, low_heat, h, w):
    """ca_pose_maps on one frame's low-resolution output through the annotator's own tables."""
    k = _k()
    ws = ann.workspace(1, h, w)
    hl, wl = low_heat.shape[1:]
    low = torch.zeros((1, hl, wl, 64))
    low[0, :, :, :38], low[0, :, :, 40:59] = torch.as_tensor(low_paf).permute(1, 2, 0), torch.as_tensor(low_heat).permute(1, 2, 0)
    k.pose_maps(low.to(DEV), ws["mx"], ws["my"], ws["raw"], ws["smooth"], ws["paf"], ws["maps_ws"])
    torch.cuda.synchronize()
    return ws["raw"][0].cpu().numpy(), ws["smooth"][0].cpu().numpy(), ws["paf"][0].cpu().numpy()


@pytest.fixture(scope="module")
def annotator():
    from controlanimate_amd.openpose import OpenposeAnnotator
    fr = R.frames_fixture()
    return OpenposeAnnotator(R.e2e_state_dict(E2E_SEED, fr), device=DEV, detect_resolution=256, image_resolution=256)


@pytest.mark.parametrize("hw", [(192, 256), (256, 320)])
def test_pose_maps(hw):
    from controlanimate_amd.openpose import OpenposeAnnotator
    ann = OpenposeAnnotator(R.pose_state_dict(1), device=DEV, detect_resolution=hw[0], image_resolution=hw[0])
    g = R.geometry(*hw)
    gen = np.random.default_rng(2)
    paf, heat = gen.standard_normal((38, g["hl"], g["wl"])).astype(np.float32), gen.standard_normal((19, g["hl"], g["wl"])).astype(np.float32)
    got = _device_maps(ann, paf, heat, *hw)
    for name, a, b in zip(("raw", "smooth", "paf"), got, R.maps_ref(paf, heat, *hw)):
        err, top = np.abs(a - b).max(), np.abs(b).max()
        print(f"ca_pose_maps {hw} {name}: max|err| / max|ref| = {err / top:.3e} (bar {2.0 ** -17:.3e})")
        assert err <= 2.0 ** -17 * top
    const = _device_maps(ann, np.full_like(paf, 0.75), np.full_like(heat, 0.75), *hw)
    for a in const:
        assert np.abs(a - 0.75).max() <= 2.0 ** -17 * 0.75


# ---- decode ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES)
def test_decode_of_planted_maps_equals_the_specification(case):
    k = _k()
    raw, smooth, paf, _ = R.planted(case)
    ok, why = R.decided(raw, smooth, paf)
    assert ok, why
    want = R.decode_ref(raw, smooth, paf)
    b = k.pose_decode(*(torch.from_numpy(a)[None].to(DEV) for a in (raw, smooth, paf)))
    torch.cuda.synchronize()
    assert int(b["people"][0]) == want["people"] and int(b["overflow"][0]) == want["overflow"]
    assert [int(c) for c in b["counts"][0]] == [len(p) for p in want["peaks"]]
    assert [int(c) for c in b["conn_n"][0]] == [len(c) for c in want["connections"]]
    assert np.array_equal(b["keypoints"][0].cpu().numpy(), want["keypoints"])
    assert np.array_equal(b["coords"][0].cpu().numpy(), want["coords"])
    if case == "crowd_overflow":
        assert want["overflow"] == R.OVERFLOW_PEAKS and want["people"] == 1


def test_people_cap_on_the_device():
    """64 two-part rows from limb 0, then limb 4 (left shoulder -- elbow) of nobody: the 65th row is dropped and the bit set; before that
    connection is added, a found == 1 extension of row 63 sets nothing."""
    k = _k()
    peaks = [[(10 + 3 * i, 20, np.float32(1.0)) for i in range(R.MAX_PEAKS)] if q in (1, 2) else [] for q in range(18)]
    peaks[8], peaks[5], peaks[6] = [(50, 60, np.float32(1.0))], [(70, 90, np.float32(1.0))], [(70, 120, np.float32(1.0))]
    conns = [[(i, i, 1.0) for i in range(R.MAX_PEAKS)] if q == 0 else [] for q in range(19)]
    conns[6] = [(63, 0, 1.0)]
    for extra, bit in ((False, 0), (True, R.OVERFLOW_PEOPLE)):
        if extra:
            conns[4] = [(0, 0, 1.0)]
        want = R.assemble_ref(peaks, conns, H, W)
        assert want[3] == bit
        b = k.pose_decode_buffers(1, DEV)
        for name in ("peaks", "scores", "counts", "overflow", "conn_ij", "conn_score", "conn_n"):
            b[name].zero_()
        for q, pk in enumerate(peaks):
            b["counts"][0, q] = len(pk)
            for i, (x, y, sc) in enumerate(pk):
                b["peaks"][0, q, i, 0], b["peaks"][0, q, i, 1], b["scores"][0, q, i] = x, y, float(sc)
        for q, cn in enumerate(conns):
            b["conn_n"][0, q] = len(cn)
            for c, (i, j, sc) in enumerate(cn):
                b["conn_ij"][0, q, c, 0], b["conn_ij"][0, q, c, 1], b["conn_score"][0, q, c] = i, j, sc
        k.pose_assemble(b, H, W)
        torch.cuda.synchronize()
        assert int(b["overflow"][0]) == bit and int(b["people"][0]) == want[2]
        assert np.array_equal(b["keypoints"][0].cpu().numpy(), want[0]) and np.array_equal(b["coords"][0].cpu().numpy(), want[1])


# ---- draw ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rep", [1, 2])
def test_draw_equals_the_specification(rep):
    from controlanimate_amd.openpose import sin_table
    k = _k()
    cases = R.draw_cases()
    coords = torch.from_numpy(np.stack([c[0] for c in cases.values()])).to(DEV)
    people = torch.tensor([c[1] for c in cases.values()], dtype=torch.int32, device=DEV)
    n = len(cases)
    sk = torch.empty((n, H, W, 3), dtype=torch.uint8, device=DEV)
    ctrl = torch.empty((rep * n, 3, H, W), dtype=torch.float32, device=DEV)
    k.pose_draw(coords, people, torch.from_numpy(sin_table()).to(DEV), H, W, skeleton=sk, control=ctrl, rep=rep)
    ctrl16 = torch.empty((rep * n, 3, H, W), dtype=torch.float16, device=DEV)
    k.pose_draw(coords, people, torch.from_numpy(sin_table()).to(DEV), H, W, control=ctrl16, rep=rep)
    torch.cuda.synchronize()
    for i, (name, (co, p)) in enumerate(cases.items()):
        want = R.draw_ref(co, p, H, W)
        got = sk[i].cpu().numpy()
        assert np.array_equal(got, want), f"{name}: {(got != want).any(axis=2).sum()} pixels differ"
    want_ctrl = (sk.cpu().permute(0, 3, 1, 2).float() / 255).repeat(rep, 1, 1, 1)   # (the true quotient: divided on the host)
    assert torch.equal(ctrl.cpu(), want_ctrl) and torch.equal(ctrl16.cpu(), want_ctrl.half())


# ---- end to end --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e():
    fr = R.frames_fixture()
    sd = R.e2e_state_dict(E2E_SEED, fr)
    return fr, sd, R.lowres_ref(sd, fr)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_lowres_maps_meet_the_bar(e2e, dtype):
    from controlanimate_amd.openpose import OpenposeAnnotator
    fr, sd, (paf, heat) = e2e
    sd = {k_: v.to(dtype).float() for k_, v in sd.items()}   # seeded weights rounded to the device dtype
    paf, heat = R.lowres_ref(sd, fr)
    ann = OpenposeAnnotator(sd, device=DEV, dtype=dtype, detect_resolution=256, image_resolution=256)
    low = ann.lowres(fr).cpu()
    got = torch.cat([low[..., :38], low[..., 40:59]], 3).permute(0, 3, 1, 2)
    ref = torch.cat([paf, heat], 1)
    per = ((got - ref).flatten(2).norm(dim=2) / ref.flatten(2).norm(dim=2)).max(0).values
    print(f"per-channel relative L2 {dtype}: " + " ".join(f"{v:.1e}" for v in per.tolist()))
    rel = ((got - ref).norm() / ref.norm()).item()
    print(f"low-resolution maps {dtype}: relative L2 {rel:.3e} (bar {E2E_BAR[dtype]:.0e})")
    assert rel <= E2E_BAR[dtype]
    assert float(low[..., 38:40].abs().max()) == 0.0 and float(low[..., 59:].abs().max()) == 0.0


def test_skeleton_end_to_end(e2e, annotator):
    from controlanimate_amd.context import dispatch
    k = _k()
    fr, sd, _ = e2e
    sk = annotator.skeleton(fr)
    raw, smooth, paf = annotator.maps(fr)
    kp, people, overflow = annotator.poses(fr)
    # the stand-alone kernels on the chain's own maps
    b = k.pose_decode(raw, smooth, paf)
    alone = k.pose_draw(b["coords"], b["people"], annotator.workspace(2, 256, 320)["sin"], 256, 320)
    torch.cuda.synchronize()
    assert torch.equal(alone, sk) and torch.equal(b["keypoints"], kp) and torch.equal(b["people"], people) and torch.equal(b["overflow"], overflow)
    # ... and the specification on them
    for i in range(2):
        maps = [t[i].cpu().numpy() for t in (raw, smooth, paf)]
        ok, why = R.decided(*maps)
        assert ok, f"frame {i}: {why}"
        want = R.decode_ref(*maps)
        print(f"frame {i}: {want['people']} people, peaks per part {[len(p) for p in want['peaks']]}")
        assert int(people[i]) == want["people"] and np.array_equal(kp[i].cpu().numpy(), want["keypoints"])
        assert np.array_equal(sk[i].cpu().numpy(), R.draw_ref(want["coords"], want["people"], 256, 320))
    assert int(people.sum()) > 0 and int(sk.max()) > 0
    # one frame per chunk: the same bytes
    g = R.geometry(256, 320)
    annotator.max_activation_bytes = g["hl"] * g["wl"] * 49 * 192 * 2   # what one frame's largest operand takes
    try:
        assert annotator.chunk_frames(256, 320) == 1
        assert torch.equal(annotator.skeleton(fr), sk)
    finally:
        del annotator.max_activation_bytes
    # the other form of the 7x7 convolutions: maps within the bar of each other
    low = annotator.lowres(fr)
    was = dispatch.pose_conv7_direct
    try:
        dispatch.pose_conv7_direct = not was
        other = annotator.lowres(fr)
    finally:
        dispatch.pose_conv7_direct = was
    rel = ((other - low).norm() / low.norm()).item()
    print(f"pose_conv7_direct on / off: relative L2 {rel:.3e}")
    assert rel <= E2E_BAR[torch.float16]


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "im2col_gemm"])
def test_chain_replays_in_a_captured_graph(e2e, annotator, monkeypatch, direct):
    """No launch of the chain waits for the host, the skeleton assembly included: captured once, it replays for new frames copied into
    the captured buffer -- with either form of the 7x7 convolutions."""
    from controlanimate_amd.context import dispatch
    monkeypatch.setattr(dispatch, "pose_conv7_direct", direct)
    fr = e2e[0]
    eager = [annotator.annotate_batch(torch.from_numpy(f).to(DEV), rep=2).clone() for f in (fr, fr[::-1].copy())]
    assert not torch.equal(eager[0], eager[1])
    buf = torch.from_numpy(fr).to(DEV)
    out = torch.empty((4, 3, 256, 320), dtype=torch.float32, device=DEV)
    annotator.annotate_batch(buf, out=out, rep=2)   # warm-up: the workspace and the weights are on the device before the capture
    out.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        annotator.annotate_batch(buf, out=out, rep=2)
    for i in (0, 1, 0):
        buf.copy_(torch.from_numpy(fr if i == 0 else fr[::-1].copy()).to(DEV))
        graph.replay()
        assert torch.equal(out, eager[i]), i
    assert out.max() > 0


def test_a_larger_chunk_than_the_plan_replans(e2e):
    from controlanimate_amd.openpose import OpenposeAnnotator
    fr, sd, _ = e2e
    ann = OpenposeAnnotator(sd, device=DEV, detect_resolution=256, image_resolution=256)
    g = R.geometry(256, 320)
    ann.max_activation_bytes = g["hl"] * g["wl"] * 49 * 192 * 2   # one frame per pass
    small = ann.skeleton(fr)
    del ann.max_activation_bytes                                   # both frames in one pass: larger buffers than were planned
    assert ann.chunk_frames(256, 320) >= 2 and torch.equal(ann.skeleton(fr), small) and int(small.max()) > 0


# ---- contracts and routing ---------------------------------------------------------------------------------------------------------
def test_call_and_annotate_batch_contracts(e2e, annotator):
    from PIL import Image
    fr, _, _ = e2e
    sk = annotator.skeleton(fr)
    out = annotator(fr[0])
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and np.array_equal(out, sk[0].cpu().numpy())
    pil = annotator(Image.fromarray(fr[0]))
    assert isinstance(pil, Image.Image) and pil.mode == "RGB" and np.array_equal(np.asarray(pil), out)
    ctrl = annotator.annotate_batch(list(fr), rep=2)
    assert tuple(ctrl.shape) == (4, 3, 256, 320) and ctrl.dtype == torch.float32
    want = (sk.cpu().permute(0, 3, 1, 2).float() / 255).repeat(2, 1, 1, 1)   # (the true quotient: divided on the host)
    assert torch.equal(ctrl.cpu(), want)
    half = torch.empty((2, 3, 256, 320), dtype=torch.float16, device=DEV)
    assert annotator.annotate_batch(torch.from_numpy(fr).to(DEV), out=half) is half and torch.equal(half.cpu(), want[:2].half())
    timings = {}
    annotator.timings = timings
    try:
        annotator.skeleton(fr)
        torch.cuda.synchronize()
    finally:
        annotator.timings = None
    assert {name: len(v) for name, v in timings.items()} == annotator.STAGES


@pytest.mark.parametrize("name", NAMES)
def test_pipeline_routes_the_key(name, annotator):
    from controlanimate_amd.controlresiduals_pipeline import MultiControlNetResidualsPipeline
    pipe = MultiControlNetResidualsPipeline.__new__(MultiControlNetResidualsPipeline)
    pipe.annotators = {"openpose": annotator}
    assert pipe._annotator_for(name) is annotator
    assert pipe._batch_annotator(name, [np.zeros((256, 320, 3), np.uint8)]) == annotator.annotate_batch
