"""GPU: controlanimate_amd/face_align.py against the specification tests/retinaface_ref.py.  The real geometry (a full-width ResNet-50) at
tiny frames: n = 3 frames of 64 x 96 and of 96 x 64, level maps 8 x 12 / 4 x 6 / 2 x 3 -- the smallest at which every level, both
orientations and the odd n can go wrong.  Weights are seeded and rounded to fp16 once, so the specification and the device hold the same.

The decode is exact: the device's own fp32 head tensors go to the numpy specification, which must then find the same faces.  The planted
head tensors (`planted_cases`) need no network; tests/test_face_align_cpu.py checks with the specification alone that each does what its
name says."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import retinaface_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONV_BAR = {torch.float16: 2.5 * 2.0 ** -10, torch.bfloat16: 2.5 * 2.0 ** -8}  # tests/test_openpose_gpu.py
E2E_BAR = {torch.float16: 1e-2, torch.bfloat16: 8e-2}                           # tests/test_openpose_gpu.py
# the tiny golden body through the device chain (relative L2 of the three taps against the recorded fp32 ones): measured 9.1e-4 / 1.1e-3 /
# 1.1e-3 in fp16 and 6.9e-3 / 8.4e-3 / 8.2e-3 in bf16; ten times that would be 1.1e-2 / 8.4e-2, the siblings' E2E_BAR is tighter and is kept
GOLDEN_BAR = {torch.float16: 1e-2, torch.bfloat16: 8e-2}
SEED, MAX_FACES = 0, 4
SIZES = ((64, 96), (96, 64))
PLANT_HW, PLANT_CONF = (256, 256), 0.5
TINY = (8, (32, 64, 128, 256), 128)


def _fa():
    from controlanimate_amd import face_align
    return face_align


def _k():
    from controlanimate_amd import kernels
    return kernels


def smooth_frames(n, h, w, seed=0) -> np.ndarray:
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for i in range(n):
        chans = [127.5 + 100.0 * np.sin(0.09 * (i + 1) * xx + 0.07 * (c + 1) * yy + 0.7 * c + i + seed) * np.cos(0.05 * (c + 2) * xx - 0.04 * yy) for c in range(3)]
        out.append(np.stack(chans, -1))
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(np.stack(out) + rng.normal(0, 6, (n, h, w, 3))), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=1)
def full_sd() -> dict:
    """The seeded full-width state dict, every tensor rounded to fp16 (what the device packs from)."""
    return {k: v.half().float() for k, v in R.seeded_state_dict(_fa().retinaface_key_shapes(), SEED).items()}


@functools.lru_cache(maxsize=4)
def reference_heads(hw, bgr=False):
    """The fp32 specification's (class, boxes, landmarks) for the seeded frames of one size: computed once, never changed."""
    with torch.no_grad():
        return tuple(t.numpy() for t in R.network(full_sd(), smooth_frames(3, *hw, seed=hw[1]), bgr))


@functools.lru_cache(maxsize=8)
def aligner(dtype, conf=0.97, upscale=1):
    return _fa().FaceAligner(full_sd(), max_faces=MAX_FACES, conf_threshold=conf, dtype=dtype, device=DEV, upscale_factor=upscale)


def _conv_bar(what, out, ref, dtype):
    rel = CONV_BAR[dtype]
    rel_l2 = ((out - ref).norm() / ref.norm()).item()
    max_rel = ((out - ref).abs().max() / ref.abs().max()).item()
    print(f"{what} {dtype}: rel_l2={rel_l2:.3e} max_err/max_ref={max_rel:.3e} (tol {rel:.1e})")
    assert torch.isfinite(out).all() and rel_l2 < rel and max_rel < 4 * rel


def _ulp_close(a, b, ulps=1):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= ulps * np.spacing(np.maximum(np.abs(a), np.abs(b)))))


# ---- the small kernels -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("hw", [(64, 96), (96, 64), (34, 46), (40, 264)])
def test_stem_against_conv2d(hw, dtype, bgr):
    """The whole output, border rows and columns included: the zero padding lies in the mean-subtracted image."""
    fa, K = _fa(), _k()
    h, w = hw
    frames = smooth_frames(3, h, w, seed=7)
    frames[1, :4] = 255            # a border of large values: a padding tap that contributed -mean * w would show
    frames[2, :, -4:] = 0
    sd = full_sd()
    wt, bias = fa.fold_bn(sd, "body.conv1", "body.bn1")
    ref = F.relu(F.conv2d(R.preprocess(frames, bgr), wt, bias, 2, 3)).permute(0, 2, 3, 1)
    out = torch.empty((3, h // 2, w // 2, 64), dtype=dtype, device=DEV)
    K.rface_stem(torch.from_numpy(frames).to(DEV), fa.pack_stem(wt, dtype).to(DEV), bias.to(DEV), out, bgr)
    out = out.float().cpu()
    _conv_bar(f"stem {hw} bgr={bgr}", out, ref, dtype)
    edge = torch.cat([(out - ref)[:, 0].flatten(), (out - ref)[:, -1].flatten(), (out - ref)[:, :, 0].flatten(), (out - ref)[:, :, -1].flatten()])
    assert edge.abs().max() < 4 * CONV_BAR[dtype] * ref.abs().max()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", [(3, 32, 48, 64), (2, 7, 9, 8), (1, 1, 1, 16)])
def test_maxpool3x3s2_exact(shape, dtype):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(shape, generator=g).to(dtype)
    x[0] = -x[0].abs() - 1       # an all-negative plane: a zero padding would win
    want = F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    got = _k().maxpool3x3s2(x.to(DEV)).float().cpu()
    assert got.shape == want.shape and torch.equal(got, want) and (got[0] < 0).all()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_subsample2_and_add_up2(dtype):
    K = _k()
    g = torch.Generator().manual_seed(2)
    x = torch.randn((3, 7, 10, 24), generator=g).to(dtype)
    assert torch.equal(K.subsample2(x.to(DEV)).cpu(), x[:, ::2, ::2].contiguous())
    a, b = torch.randn((3, 8, 12, 40), generator=g).to(dtype), torch.randn((3, 4, 6, 40), generator=g).to(dtype)
    want = (a.float() + F.interpolate(b.float().permute(0, 3, 1, 2), size=(8, 12), mode="nearest").permute(0, 2, 3, 1)).to(dtype)
    assert torch.equal(K.add_up2(a.to(DEV), b.to(DEV)).cpu(), want)
    ad = a.to(DEV)
    assert torch.equal(K.add_up2(ad, b.to(DEV), ad).cpu(), want)       # in place


# ---- the network -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("hw", SIZES)
def test_network_heads_against_the_fp32_specification(hw, dtype):
    """The fp32 head tensors (class logits, boxes, landmarks) of the full-width network against the fp32 specification, relative L2, at the
    siblings' E2E_BAR (fp16 1e-2, bf16 8e-2)."""
    fa = _fa()
    frames = smooth_frames(3, *hw, seed=hw[1])
    got = fa.unpack_heads(aligner(dtype).heads(frames))
    for name, g, r in zip(("class", "boxes", "landmarks"), got, reference_heads(hw)):
        assert g.shape == r.shape and np.isfinite(g).all()
        rel = float(np.linalg.norm(g.astype(np.float64) - r) / np.linalg.norm(r))
        print(f"{name} {hw} {dtype}: relative L2 {rel:.3e} (bar {E2E_BAR[dtype]:.0e})")
        assert rel <= E2E_BAR[dtype]


def test_network_bgr_reverses_the_channels_on_the_way_in():
    hw = SIZES[0]
    frames = smooth_frames(3, *hw, seed=hw[1])
    al = aligner(torch.float16)
    got = [t.cpu() for t in al.heads(np.ascontiguousarray(frames[..., ::-1]), bgr=True)]
    want = [t.cpu() for t in al.heads(frames)]
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_golden_body_through_the_device_chain(dtype):
    """The recorded transformers taps (fp32) against the device chain at the tiny widths of the fixture."""
    fa = _fa()
    z = np.load(os.path.join(ROOT, "tests", "golden", "retinaface_body_tiny.npz"))
    geo = fa.Geometry(*TINY)
    sd = R.seeded_state_dict(fa.retinaface_key_shapes(geo), 3)
    sd.update({k[2:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith("w:")})
    al = fa.FaceAligner(sd, geometry=geo, dtype=dtype, device=DEV)
    taps = al.body_taps(z["frames"])[1:]
    for i, t in enumerate(taps):
        want = torch.from_numpy(z[f"tap{i}"]).permute(0, 2, 3, 1)
        rel = ((t.float().cpu() - want).norm() / want.norm()).item()
        print(f"golden tap{i} {dtype}: relative L2 {rel:.3e} (bar {GOLDEN_BAR[dtype]:.0e})")
        assert rel <= GOLDEN_BAR[dtype]


# ---- the decode, exact -----------------------------------------------------------------------------------------------------------------------
def _check_decode(out, levels, h, w, conf, **kw):
    """The device's dets / count / overflow against the specification on the same fp32 head tensors, frame by frame."""
    cls, box, ldm = _fa().unpack_heads(levels)
    dets, count, overflow = out["dets"].cpu().numpy(), out["count"].cpu().numpy(), out["overflow"].cpu().numpy()
    for i in range(cls.shape[0]):
        want = R.detect(cls[i], box[i], ldm[i], h, w, conf_threshold=conf, max_faces=MAX_FACES, **kw)
        assert count[i] == want["count"] and overflow[i] == want["overflow"], (i, count[i], want["count"], overflow[i], want["overflow"])
        # the same faces in the same order: a row of dets within one fp32 ulp (exp) of the specification's decode of ITS kept prior
        assert _ulp_close(dets[i], want["dets"]), (i, dets[i], want["dets"])
        assert not dets[i, want["count"]:].any()
    return count


@pytest.mark.parametrize("hw", SIZES)
def test_decode_of_the_devices_own_heads_is_exact(hw):
    h, w = hw
    al = aligner(torch.float16, 0.5)
    levels = al.heads(smooth_frames(3, h, w, seed=w))
    cand = int((R.scores(_fa().unpack_heads(levels)[0]) > np.float32(0.5)).sum())
    print(f"{hw}: {cand} of {3 * R.prior_count(h, w)} priors above 0.5")
    assert cand > 3 * R.prior_count(h, w) // 8            # seeded weights pass a good share of the priors
    for kw in ({}, {"only_center_face": True}, {"only_keep_largest": True}):
        out = al.decode(levels, h, w, **kw)
        _check_decode(out, levels, h, w, 0.5, **kw)


def _landmarks(x1, y1, x2, y2):
    w, h = x2 - x1, y2 - y1
    return [x1 + 0.3 * w, y1 + 0.4 * h, x1 + 0.7 * w, y1 + 0.4 * h, x1 + 0.5 * w, y1 + 0.6 * h, x1 + 0.35 * w, y1 + 0.8 * h, x1 + 0.65 * w, y1 + 0.8 * h]


def _plant(case, pri, idx, box, logit, pts=None):
    """Writes head values into prior idx such that it decodes to the corner box and the landmark points (pixels) with score sigmoid(logit)."""
    h, w = PLANT_HW
    cx, cy, sw, sh = pri[idx]
    x1, y1, x2, y2 = box
    case["cls"][idx] = [0.0, logit]
    case["box"][idx] = [((x1 + x2) / 2 / w - cx) / (0.1 * sw), ((y1 + y2) / 2 / h - cy) / (0.1 * sh), math.log((x2 - x1) / w / sw) / 0.2, math.log((y2 - y1) / h / sh) / 0.2]
    pts = _landmarks(*box) if pts is None else pts
    case["ldm"][idx] = [(pts[t] / (h if t & 1 else w) - (cy if t & 1 else cx)) / (0.1 * (sh if t & 1 else sw)) for t in range(10)]
    case.setdefault("planted", []).append(idx)


@functools.lru_cache(maxsize=1)
def planted_cases() -> dict:
    """name -> dict(cls [P, 2], box [P, 4], ldm [P, 10] float32, planted: the prior indices in the order they were planted, kw: detect's flags)
    on a 256 x 256 frame; every prior that is not planted is background (score 2e-9)."""
    h, w = PLANT_HW
    pri = R.priors(h, w)
    p = len(pri)
    n0 = 2 * 32 * 32                                       # level 1 starts here; its cell (i, j) has the priors n0 + 2 (16 i + j) + {0, 1}

    def blank():
        cls = np.zeros((p, 2), np.float32)
        cls[:, 0], cls[:, 1] = 10.0, -10.0
        return {"cls": cls, "box": np.zeros((p, 4), np.float32), "ldm": np.zeros((p, 10), np.float32)}

    def at(i, j, a=1):
        return n0 + 2 * (16 * i + j) + a

    cases = {}
    # two 101-pixel squares (py_cpu_nms counts x2 - x1 + 1) shifted by d overlap by (101 - d) / (101 + d)
    for name, iou in (("overlap_039", 0.39), ("overlap_041", 0.41)):
        d = 101 * (1 - iou) / (1 + iou)
        c = cases[name] = blank()
        _plant(c, pri, at(6, 6), (50, 50, 150, 150), 3.0)
        _plant(c, pri, at(6, 9), (50 + d, 50, 150 + d, 150), 2.0)
    c = cases["score_tie"] = blank()
    _plant(c, pri, at(8, 8), (60, 60, 140, 140), 2.5)
    _plant(c, pri, at(5, 5), (60, 60, 140, 140), 2.5)
    for name, dist in (("eyes_49", 4.9), ("eyes_51", 5.1)):
        c = cases[name] = blank()
        pts = _landmarks(80, 80, 120, 120)
        pts[0:4] = [100.0, 100.0, 100.0 + dist, 100.0]
        _plant(c, pri, at(6, 6, 0), (80, 80, 120, 120), 3.0, pts)
    c = cases["too_many_faces"] = blank()
    for r in range(MAX_FACES + 1):
        x = 10 + 48 * r
        _plant(c, pri, at(3 * (r % 2) + 2, 3 * r + 1, 0), (x, 30 + 90 * (r % 2), x + 40, 70 + 90 * (r % 2)), 4.0 - 0.5 * r)
    cases["no_face"] = blank()
    c = cases["center_of_two"] = blank()
    _plant(c, pri, at(3, 3), (20, 20, 80, 80), 3.0)
    _plant(c, pri, at(8, 8), (100, 100, 160, 160), 2.0)
    c["kw"] = {"only_center_face": True}
    c = cases["largest_of_two"] = blank()
    _plant(c, pri, at(3, 3, 0), (20, 20, 60, 60), 3.0)
    _plant(c, pri, at(9, 9), (100, 100, 200, 200), 2.0)
    c["kw"] = {"only_keep_largest": True}
    # every prior of level 0 a candidate with a seeded score: twice CA_RFACE_MAX_CAND
    c = cases["candidate_overflow"] = blank()
    rng = np.random.default_rng(8)
    c["cls"][:n0, 0], c["cls"][:n0, 1] = 0.0, 0.5 + 3.0 * rng.random(n0)
    c["ldm"][:n0] = rng.normal(0, 1, (n0, 10))
    c["ldm"][:n0, 0], c["ldm"][:n0, 2] = -4.0, 4.0          # the eyes 0.8 prior sizes apart
    c["planted"] = []
    return cases


def test_planted_head_tensors():
    """Overlaps of 0.39 and 0.41, an exact score tie, eye distances 4.9 and 5.1, max_faces + 1 faces, no face, only_center_face and
    only_keep_largest with two faces, more than CA_RFACE_MAX_CAND candidates: each frame's faces are the specification's."""
    fa = _fa()
    h, w = PLANT_HW
    cases = planted_cases()
    al = aligner(torch.float16, PLANT_CONF)
    seen = {}
    for kw in ({}, {"only_center_face": True}, {"only_keep_largest": True}):
        names = [k for k, c in cases.items() if c.get("kw", {}) == kw]
        levels = [torch.from_numpy(t).to(DEV) for t in fa.pack_heads(*(np.stack([cases[k][f] for k in names]) for f in ("cls", "box", "ldm")), h, w)]
        out = al.decode(levels, h, w, **kw)
        count = _check_decode(out, levels, h, w, PLANT_CONF, **kw)
        seen.update({k: (int(count[i]), int(out["overflow"][i])) for i, k in enumerate(names)})
    assert seen["overlap_039"] == (2, 0) and seen["overlap_041"] == (1, 0) and seen["score_tie"] == (1, 0)
    assert seen["eyes_49"] == (0, 0) and seen["eyes_51"] == (1, 0) and seen["no_face"] == (0, 0)
    assert seen["too_many_faces"] == (MAX_FACES, R.OVERFLOW_FACES) and seen["center_of_two"] == (1, 0) and seen["largest_of_two"] == (1, 0)
    assert seen["candidate_overflow"][1] & R.OVERFLOW_CAND


# ---- fit and warp ----------------------------------------------------------------------------------------------------------------------------
def _planted_dets(h, w):
    """dets [3, MAX_FACES, 15] and count [3]: landmarks that are the template under a rotation, a shift that leaves part of the crop outside
    the frame, scales below and above 1."""
    dets, count = np.zeros((3, MAX_FACES, 15), np.float32), np.array([2, 0, 3], np.int32)
    rng = np.random.default_rng(6)

    def put(f, r, scale, theta, tx, ty):
        rot = scale * np.array([[math.cos(theta), -math.sin(theta)], [math.sin(theta), math.cos(theta)]])
        pts = (R.TEMPLATE - 256.0) @ rot.T + [tx, ty] + rng.normal(0, 0.3, (5, 2))     # (not an exact similarity: the fit has residuals)
        dets[f, r, 5:] = pts.reshape(-1)
        dets[f, r, :5] = [pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max(), 0.99]

    put(0, 0, 0.08, 0.5, w * 0.5, h * 0.5)          # a rotated face in the middle, shrunk frame -> crop scale 12.5: above 1
    put(0, 1, 0.2, -0.3, w * 0.9, h * 0.2)          # near the corner: most of the crop lies outside the frame
    put(2, 0, 0.15, 0.0, w * 0.3, h * 0.6)
    put(2, 1, 2.5, 2.0, w * 0.5, h * 0.5)           # a face larger than the frame: crop scale 0.4, below 1
    put(2, 2, 0.1, -1.2, -5.0, h * 0.5)             # centred left of the frame
    return dets, count


@pytest.mark.parametrize("upscale", [1, 2])
@pytest.mark.parametrize("hw", SIZES)
def test_fit_against_the_specification(hw, upscale):
    h, w = hw
    dets, count = _planted_dets(h, w)
    al = aligner(torch.float16, 0.97, upscale)
    aff = torch.empty((3, MAX_FACES, 2, 3), dtype=torch.float64, device=DEV)
    inv = torch.empty_like(aff)
    _k().face_align(torch.from_numpy(dets).to(DEV), torch.from_numpy(count).to(DEV), al.upscale_factor, aff, inv)
    aff, inv = aff.cpu().numpy(), inv.cpu().numpy()
    for f in range(3):
        for r in range(MAX_FACES):
            if r >= count[f]:
                assert not aff[f, r].any() and not inv[f, r].any()
                continue
            m = R.similarity_fit(dets[f, r, 5:].astype(np.float64).reshape(5, 2))
            assert np.abs(aff[f, r] - m).max() <= 1e-9 * np.abs(m).max()
            mi = R.inverse_affine(m, upscale)
            assert np.abs(inv[f, r] - mi).max() <= 1e-9 * np.abs(mi).max()


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("hw", SIZES)
def test_warp_byte_for_byte(hw, bgr):
    """The crops against the specification's warp of the device's own matrices: a rotated face, a face partly outside the frame (the
    border value shows), scales below and above 1, an empty frame, empty slots."""
    h, w = hw
    frames = smooth_frames(3, h, w, seed=5)
    dets, count = _planted_dets(h, w)
    al = aligner(torch.float16)
    aff = torch.empty((3, MAX_FACES, 2, 3), dtype=torch.float64, device=DEV)
    cnt = torch.from_numpy(count).to(DEV)
    _k().face_align(torch.from_numpy(dets).to(DEV), cnt, 1.0, aff, torch.empty_like(aff))
    faces = al.warp(torch.from_numpy(frames).to(DEV), aff, cnt, bgr=bgr).cpu().numpy()
    assert faces.shape == (3 * MAX_FACES, 512, 512, 3)
    aff = aff.cpu().numpy()
    border = np.array(R.BORDER[::-1] if bgr else R.BORDER, np.uint8)
    shows = 0
    for f in range(3):
        for r in range(MAX_FACES):
            got = faces[f * MAX_FACES + r]
            if r >= count[f]:
                assert (got == border).all()
                continue
            want = R.warp_affine(frames[f], aff[f, r], bgr=bgr)
            assert np.array_equal(got, want), (f, r, int((got != want).sum()))
            shows += int((want == border).all(axis=2).sum() > 1000)
            assert len(np.unique(want.reshape(-1, 3), axis=0)) > 50          # the frame shows too
    assert shows >= 3


# ---- contracts -------------------------------------------------------------------------------------------------------------------------------
def test_align_end_to_end_allocates_nothing_twice_and_is_bit_identical_under_a_graph():
    hw = SIZES[0]
    al = aligner(torch.float16, 0.5)
    dev_frames = torch.from_numpy(smooth_frames(3, *hw, seed=hw[1])).to(DEV)
    first = {k: v.clone() for k, v in al.align(dev_frames).items()}
    assert first["faces"].shape == (3 * MAX_FACES, 512, 512, 3) and first["faces"].dtype == torch.uint8 and first["affine"].dtype == torch.float64
    assert first["count"].shape == (3,) and first["dets"].shape == (3, MAX_FACES, 15) and first["inverse_affine"].shape == (3, MAX_FACES, 2, 3)
    assert all(v.is_cuda for v in first.values()) and int(first["count"].sum()) > 0
    # the whole chain against the specification fed with the device's heads and matrices
    levels = al.heads(dev_frames)
    _check_decode(first, levels, *hw, 0.5)
    crops = first["faces"].cpu().numpy()
    for f in range(3):
        for r in range(int(first["count"][f])):
            assert np.array_equal(crops[f * MAX_FACES + r], R.warp_affine(dev_frames[f].cpu().numpy(), first["affine"][f, r].cpu().numpy()))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    second = al.align(dev_frames)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert all(torch.equal(second[k], first[k]) for k in first)
    # PIL frames and arrays take the same path
    from PIL import Image
    third = al.align([Image.fromarray(a) for a in dev_frames.cpu().numpy()])
    assert all(torch.equal(third[k], first[k]) for k in first)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = al.align(dev_frames)
    for v in captured.values():
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(captured[k], first[k]) for k in first)


def test_chunked_passes_give_the_same_heads():
    """max_activation_bytes below a window's need: the frames go through the network in several passes, as in the hand stage."""
    hw = SIZES[1]
    frames = smooth_frames(3, *hw, seed=hw[1])
    al = _fa().FaceAligner(full_sd(), max_faces=MAX_FACES, dtype=torch.float16, device=DEV)
    al.max_activation_bytes = 2 * hw[0] * hw[1] * al._bytes_per_pixel       # two frames per pass
    assert al.chunk_frames(*hw) == 2
    got = [t.cpu() for t in al.heads(frames)]
    want = [t.cpu() for t in aligner(torch.float16).heads(frames)]
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_face_helper_drives_face_restorer_enhance():
    """FaceRestorer.enhance(has_aligned=False, paste_back=False) with the adapter: the crops are the aligner's, nothing from facexlib."""
    fa = _fa()
    hw = SIZES[0]
    frame = smooth_frames(3, *hw, seed=hw[1])[0]
    al = aligner(torch.float16, 0.5)
    want = {k: v.clone() for k, v in al.align([frame]).items()}
    n = int(want["count"][0])
    assert n > 0
    helper = fa.FaceHelper(al)

    class Restorer:                        # enhance's control flow needs restore_aligned only
        from controlanimate_amd.gfpgan import FaceRestorer
        enhance = FaceRestorer.enhance

        def restore_aligned(self, faces):
            return torch.from_numpy(np.stack(faces)).flip(-1)

    cropped, restored, img = Restorer().enhance(frame, has_aligned=False, paste_back=False, face_helper=helper)
    assert img is None and len(cropped) == len(restored) == n
    assert all(np.array_equal(c, w) for c, w in zip(cropped, want["faces"][:n].cpu().numpy()))
    assert all(np.array_equal(r, c[..., ::-1]) for r, c in zip(restored, cropped))
    assert np.array_equal(np.stack(helper.affine_matrices), want["affine"][0, :n].cpu().numpy())
    helper.get_inverse_affine()
    assert np.array_equal(np.stack(helper.inverse_affine_matrices), want["inverse_affine"][0, :n].cpu().numpy())
    with pytest.raises(NotImplementedError):
        Restorer().enhance(frame, has_aligned=False, paste_back=True, face_helper=helper)
