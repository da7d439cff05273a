"""GPU: the hand stage of the OpenPose annotator (controlanimate_amd/openpose_hand.py, csrc/ca_openpose_hand.hip) against its
specification (tests/hand_ref.py).  Discrete results (boxes, slots, overflow bits, crops, peaks, points) are compared exactly; the maps
within the bar of the body's full-resolution maps (tests/test_openpose_gpu.py: 2^-17 of the largest reference value); the network meets
the bars of the face tests (CONV_BAR for the 7x7 convolution at cin = 160 and for every layer at side 184, E2E_BAR for the 22 maps at
sides 184 and 736).  The drawing
is compared byte for byte."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hand_ref as HR  # noqa: E402
import pose_ref as R  # noqa: E402

from controlanimate_amd import openpose_hand as OH  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAPS_BAR = 2.0 ** -17   # tests/test_openpose_gpu.py::test_pose_maps


def _k():
    from controlanimate_amd import kernels
    return kernels


# ---- boxes ---------------------------------------------------------------------------------------------------------------------------
def _device_boxes(people_list, h, w, max_hands, overflow_in=None):
    k = _k()
    kp = torch.from_numpy(HR.keypoints_of(people_list))[None].contiguous().to(DEV)
    buf = k.hand_buffers(1, max_hands, DEV)
    k.hand_boxes(kp, torch.tensor([len(people_list)], dtype=torch.int32, device=DEV), h, w, buf, overflow_in)
    torch.cuda.synchronize()
    return buf


def _check_boxes(people_list, h, w, max_hands):
    buf = _device_boxes(people_list, h, w, max_hands)
    boxes, slots, over = HR.boxes_ref(HR.keypoints_of(people_list), len(people_list), h, w, max_hands)
    assert np.array_equal(buf["boxes"][0].cpu().numpy(), boxes)
    assert int(buf["overflow"][0]) == over
    got = buf["slots"][0].cpu().numpy()
    for i in range(max_hands):
        if i < len(slots):
            p, hd, box, ok = slots[i]
            assert tuple(got[i]) == (p, *box, hd, OH.MODE_RESIZE if ok else OH.MODE_NONE, 0, 0)
        else:
            assert tuple(got[i]) == (-1, 0, 0, 0, 0, OH.MODE_NONE, 0, 0)
    return slots, over


@pytest.mark.parametrize("case", sorted(HR.BOX_CASES))
def test_boxes_equal_the_specification(case):
    (h, w), people = HR.BOX_CASES[case]
    _check_boxes(people, h, w, 2)


def test_three_people_and_two_slots():
    """Four hands on three people, two slots: the first person's left then right hand are taken, the bit is set; with eight slots all four
    are taken in order and the bit is clear.  An incoming overflow word is kept."""
    (h, w), people = HR.BOX_CASES["three_people"]
    slots, over = _check_boxes(people, h, w, 2)
    assert [(s[0], s[1]) for s in slots] == [(0, 0), (0, 1)] and over == HR.OVERFLOW_HANDS
    slots, over = _check_boxes(people, h, w, 8)
    assert [(s[0], s[1]) for s in slots] == [(0, 0), (0, 1), (1, 1), (2, 0)] and over == 0
    buf = _device_boxes(people, h, w, 2, overflow_in=torch.tensor([3], dtype=torch.int32, device=DEV))
    assert int(buf["overflow"][0]) == 3 | HR.OVERFLOW_HANDS


def test_unrestated_side_sets_the_resize_bit():
    """A 552-pixel box (3 x 184) on a 1024 x 1024 frame: the slot is taken, its mode is NONE, the bit is set."""
    people = [HR.arm((500, 500), (500, 132), (500, 100))]   # width 1.5 * 368 = 552
    slots, over = _check_boxes(people, 1024, 1024, 2)
    assert slots[0][2][2] == 552 and not slots[0][3] and over == HR.OVERFLOW_HAND_RESIZE


# ---- maps ----------------------------------------------------------------------------------------------------------------------------
def test_hand_maps():
    """Random fp32 network outputs at the four sizes, one slot, both planes, against the specification's float64 result.  Measured on an
    MI355X: max|err| / max|ref| = 2.754e-07 (raw), 4.216e-07 (smooth); the bar is the body's 2^-17 = 7.6e-06."""
    k = _k()
    gen = np.random.default_rng(3)
    heats = [gen.standard_normal((HR.HAND_MAPS, m, m)).astype(np.float32) for m in OH.MAP_SIDES]
    dev = []
    for h in heats:
        t = torch.zeros((1, h.shape[1], h.shape[2], OH.HEAT_COLS))
        t[0, :, :, :HR.HAND_MAPS] = torch.from_numpy(h).permute(1, 2, 0)
        dev.append(t.to(DEV))
    buf = k.hand_buffers(1, 1, DEV)
    mats = torch.from_numpy(OH.map_matrices()).to(DEV)
    k.hand_maps(dev, mats, buf["raw"], buf["smooth"])
    torch.cuda.synchronize()
    for name, got, ref in zip(("raw", "smooth"), (buf["raw"], buf["smooth"]), HR.maps_ref(heats)):
        err, top = np.abs(got[0].cpu().numpy() - ref).max(), np.abs(ref).max()
        print(f"ca_hand_maps {name}: max|err| / max|ref| = {err / top:.3e} (bar {MAPS_BAR:.3e})")
        assert err <= MAPS_BAR * top
    const = [torch.full_like(t, 0.75) for t in dev]
    k.hand_maps(const, mats, buf["raw"], buf["smooth"])
    torch.cuda.synchronize()
    for t in (buf["raw"], buf["smooth"]):
        assert (t.cpu() - 0.75).abs().max().item() <= MAPS_BAR * 0.75


# ---- decode --------------------------------------------------------------------------------------------------------------------------
def _device_decode(raw, smooth, box=(0, 0, HR.WSIZE), h=512, w=512):
    """raw, smooth float32 [slots, 21, 128, 128] -> (peaks [slots, 21, 2], mass [slots, 21], points [slots, 21, 2]); slot i belongs to
    the left hand of person i of one frame, every slot has the same box."""
    k = _k()
    slots = raw.shape[0]
    buf = k.hand_buffers(1, slots, DEV)
    sl = np.zeros((1, slots, 8), np.int32)
    for i in range(slots):
        sl[0, i] = (i, *box, 0, OH.MODE_RESIZE, 0, 0)
    buf["slots"].copy_(torch.from_numpy(sl))
    k.hand_peaks(torch.from_numpy(raw).to(DEV), torch.from_numpy(smooth).to(DEV), buf, h, w)
    torch.cuda.synchronize()
    return buf["peaks"].cpu().numpy(), buf["mass"].cpu().numpy(), buf["points"][0, :slots, 0].cpu().numpy()


@pytest.fixture(scope="module")
def planted():
    cases = HR.decode_cases()
    assert len(cases) <= HR.HAND_PARTS
    raw, smooth = np.zeros((1, HR.HAND_PARTS, HR.WSIZE, HR.WSIZE), np.float32), np.zeros((1, HR.HAND_PARTS, HR.WSIZE, HR.WSIZE), np.float32)
    for i, (r, s, _) in enumerate(cases.values()):
        raw[0, i], smooth[0, i] = r, s
    return cases, raw, smooth, _device_decode(raw, smooth, box=(7, 9, 300))


def test_decode_of_planted_planes_is_exact(planted):
    """The empty plane, the corners, the full plane, the diagonal join, the serpentine, 4096 isolated pixels, equal masses, the heavier
    component against the taller peak, tied maxima, a negative winner: the peak, the winner's mass (exact sums) and the frame point."""
    cases, raw, smooth, (peaks, mass, points) = planted
    box = (7, 9, 300)
    for i, (name, (r, s, want)) in enumerate(cases.items()):
        pk, masses = HR.decode_ref(r, s)
        assert pk == want, name
        assert tuple(peaks[0, i]) == want, (name, peaks[0, i], want)
        assert mass[0, i] == (max(masses) if masses else 0.0), name
        assert tuple(points[0, i]) == HR.to_frame(want, box), name
    for i in range(len(cases), HR.HAND_PARTS):   # the unused parts are empty planes
        assert tuple(peaks[0, i]) == (0, 0) and tuple(points[0, i]) == (-1, -1)


def test_decode_of_random_maps(planted):
    """Blobs on noise, two slots: wherever the specification's two best masses differ by more than 1e-6 relative the peak and the frame
    point are the specification's, the winner's mass agrees within the rounding of a double sum, and under 5 % of the cases are left out; a second run gives
    bit-identical sums."""
    raw, smooth = HR.random_planes()
    box = (40, 60, 201)
    peaks, mass, points = _device_decode(raw, smooth, box=box)
    left_out = 0
    for s in range(raw.shape[0]):
        pts, pks, margins = HR.peaks_ref(raw[s], smooth[s], box)
        for p in range(HR.HAND_PARTS):
            if margins[p] <= 1e-6:
                left_out += 1
                continue
            assert tuple(peaks[s, p]) == tuple(pks[p]) and tuple(points[s, p]) == tuple(pts[p]), (s, p)
            masses = HR.decode_ref(raw[s, p], smooth[s, p])[1]
            if masses:   # two double sums of at most 2^14 terms in different orders
                assert abs(mass[s, p] - max(masses)) <= 2.0 ** 14 * 2.0 ** -53 * np.abs(raw[s, p].astype(np.float64)).sum()
    assert left_out < 0.05 * raw.shape[0] * HR.HAND_PARTS
    again = _device_decode(raw, smooth, box=box)
    assert np.array_equal(mass.view(np.int64), again[1].view(np.int64)) and np.array_equal(peaks, again[0])
    cases, praw, psmooth, first = planted
    second = _device_decode(praw, psmooth, box=(7, 9, 300))
    assert np.array_equal(first[1].view(np.int64), second[1].view(np.int64))


def test_skipped_and_empty_slots_give_no_points():
    k = _k()
    raw, smooth = HR.random_planes(slots=2)
    buf = k.hand_buffers(1, 2, DEV)
    buf["slots"].copy_(torch.tensor([[[3, 10, 10, 552, 1, OH.MODE_NONE, 0, 0], [-1, 0, 0, 0, 0, OH.MODE_NONE, 0, 0]]], dtype=torch.int32))
    k.hand_peaks(torch.from_numpy(raw).to(DEV), torch.from_numpy(smooth).to(DEV), buf, 1024, 1024)
    torch.cuda.synchronize()
    assert (buf["points"] == -1).all()


# ---- crop ----------------------------------------------------------------------------------------------------------------------------
from test_openpose_face_gpu import CONV_BAR, E2E_BAR  # noqa: E402  (the bars of the face tests)
# boxes on a 512 x 512 frame, (x, y, side): every border is touched; 368 takes the 2x path at side 184, 512 is the whole frame
CROP_BOXES = [(0, 0, 20), (491, 491, 21), (327, 0, 185), (0, 144, 368), (143, 100, 369), (0, 0, 512), None]


def _slot_rows(boxes):
    out = np.zeros((len(boxes), 8), np.int32)
    for i, b in enumerate(boxes):
        out[i] = (-1, 0, 0, 0, 0, OH.MODE_NONE, 0, 0) if b is None else (i, *b, i % 2, OH.MODE_RESIZE, 0, 0)
    return out


def _tables(side, side_max):
    return {k: (torch.from_numpy(v).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in OH.resize_tables(side, side_max).items()}


@pytest.fixture(scope="module")
def crop_case():
    frame = np.random.default_rng(7).integers(0, 256, (1, 512, 512, 3), dtype=np.uint8)
    want = [None if b is None else HR.hand_input_bytes(frame[0], b) for b in CROP_BOXES]
    return frame, want


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_hand_crop_is_byte_exact(crop_case, dtype):
    """Crop sides 20, 21, 185, 368, 369 and 512 and an empty slot, all four scales, byte for byte; the same crops in two passes, as a
    chunked network takes them, read the blurred crops the first pass wrote."""
    k = _k()
    frame, want = crop_case
    n = len(CROP_BOXES)
    frames, slots = torch.from_numpy(frame).to(DEV), torch.from_numpy(_slot_rows(CROP_BOXES)[None]).to(DEV)
    assert [tuple(HR.resize_choice(b[2], s) for s in HR.SIDES) for b in CROP_BOXES[3:5]] == [("area2x", "lanczos4", "lanczos4", "lanczos4"), ("area", "area", "lanczos4", "lanczos4")]
    blurred = torch.zeros((n, 512, 512, 3), dtype=torch.uint8, device=DEV)
    for si, side in enumerate(HR.SIDES):
        out = torch.full((n, side, side, 8), 3.0, dtype=dtype, device=DEV)
        k.hand_crop(frames, slots, _tables(side, 512), blurred, out, blur=si == 0)
        parts = torch.full((n, side, side, 8), 3.0, dtype=dtype, device=DEV)
        k.hand_crop(frames, slots, _tables(side, 512), blurred, parts[:3], first=0, blur=False)
        k.hand_crop(frames, slots, _tables(side, 512), blurred, parts[3:], first=3, blur=False)
        torch.cuda.synchronize()
        assert torch.equal(out, parts)
        got = out.float().cpu()
        assert float(got[..., 3:].abs().max()) == 0.0
        for s, box in enumerate(CROP_BOXES):
            if box is None:
                assert float(got[s].abs().max()) == 0.0   # the constant input
                continue
            have = ((got[s, :, :, :3] + 0.5) * 256).numpy()
            ref = want[s][si].astype(np.float32)
            assert np.array_equal(have, ref), f"side {side} crop {s} {box}: {(have != ref).sum()} bytes differ, max {np.abs(have - ref).max()}"


# ---- the 7x7 convolution at the hand network's width -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_conv7x7_at_cin_160(dtype):
    import torch.nn.functional as F
    k = _k()
    g = torch.Generator().manual_seed(11)
    x = torch.randn((1, 5, 7, 160), generator=g).to(dtype)
    w = (torch.randn((128, 7, 7, 160), generator=g) * (49 * 160) ** -0.5).to(dtype)
    b = torch.randn(128, generator=g)
    out = k.conv7x7([x.to(DEV)], [w.to(DEV)], biases=[b.to(DEV)], relu=True, direct=True)[0].float().cpu()
    ref = F.relu(F.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), b, padding=3)).permute(0, 2, 3, 1)
    rel_l2, max_rel = ((out - ref).norm() / ref.norm()).item(), ((out - ref).abs().max() / ref.abs().max()).item()
    print(f"conv7x7 cin=160 {dtype}: rel_l2={rel_l2:.3e} max_err/max_ref={max_rel:.3e} (tol {CONV_BAR[dtype]:.1e})")
    assert torch.isfinite(out).all() and rel_l2 < CONV_BAR[dtype] and max_rel < 4 * CONV_BAR[dtype]


# ---- the network and the stage ---------------------------------------------------------------------------------------------------------
ARMS = [{**HR.arm((200, 300), (180, 260), (170, 200)), **HR.arm((300, 310), (320, 250), (330, 200), left=False)}]   # boxes (165, 272, 82) and (245, 282, 94)


@pytest.fixture(scope="module")
def stage_case():
    """One 512 x 512 frame, one person with both arms planted, seeded hand weights whose last biases are set on the two crops at side 184."""
    frame = R.frames_fixture(1, 512, 512, seed=3)
    kp = HR.keypoints_of(ARMS)[None]
    boxes, slots, over = HR.boxes_ref(kp[0], 1, 512, 512, 2)
    assert [s[2] for s in slots] == [(165, 272, 82), (245, 282, 94)] and over == 0
    inputs = [HR.hand_input_bytes(frame[0], s[2]) for s in slots]
    sd = HR.e2e_hand_state_dict(0, np.stack([i[0] for i in inputs]))
    return frame, kp, boxes, slots, inputs, sd


def _run_stage(ann, frame, kp):
    ws = ann._hand.run(torch.from_numpy(frame).to(DEV), torch.from_numpy(kp).to(DEV), torch.tensor([1], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    return ws


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_handnet_meets_the_bar(stage_case, dtype):
    """Two crops from planted body keypoints, through the internal entry: the 22 maps at sides 184 and 736 against the
    fp32 reference on the specification's input, weights rounded to the device type first."""
    from controlanimate_amd.openpose import OpenposeAnnotator
    frame, kp, boxes, slots, inputs, sd = stage_case
    sd = {k_: v.to(dtype).float() for k_, v in sd.items()}
    ann = OpenposeAnnotator(R.pose_state_dict(0), device=DEV, dtype=dtype, hand=sd)
    ws = _run_stage(ann, frame, kp)
    assert np.array_equal(ws["buf"]["boxes"][0].cpu().numpy(), boxes)
    for si in (0, 3):
        got = ws["heat"][si].cpu()
        ref = HR.heat_ref(sd, np.stack([i[si] for i in inputs])).permute(0, 2, 3, 1)
        rel = ((got[..., :HR.HAND_MAPS] - ref).norm() / ref.norm()).item()
        print(f"hand maps side {HR.SIDES[si]} {dtype}: relative L2 {rel:.3e} (bar {E2E_BAR[dtype]:.0e})")
        assert rel <= E2E_BAR[dtype]
        assert float(got[..., HR.HAND_MAPS:].abs().max()) == 0.0   # the pad columns


def test_hand_stage_end_to_end(stage_case):
    """The device's own network maps through the specification's map average (within the maps' bar) and the device's own planes through
    the specification's decode (equal points wherever the two best masses differ by more than 1e-6 relative); the launch counts; one
    crop per pass through the network gives the same bytes."""
    from controlanimate_amd.openpose import OpenposeAnnotator
    frame, kp, boxes, slots, inputs, sd = stage_case
    ann = OpenposeAnnotator(R.pose_state_dict(0), device=DEV, hand=sd)
    ws = _run_stage(ann, frame, kp)
    b = ws["buf"]
    heat = [t.cpu().numpy().copy() for t in ws["heat"]]
    raw, smooth, points = b["raw"].cpu().numpy().copy(), b["smooth"].cpu().numpy().copy(), b["points"][0].cpu().numpy().copy()
    assert int(b["overflow"][0]) == 0
    compared = with_point = 0
    for s, (person, hd, box, ok) in enumerate(slots):
        for name, got, ref in zip(("raw", "smooth"), (raw[s], smooth[s]), HR.maps_ref([h[s].transpose(2, 0, 1)[:HR.HAND_MAPS] for h in heat])):
            assert np.abs(got - ref).max() <= MAPS_BAR * np.abs(ref).max(), (s, name)
        pts, pks, margins = HR.peaks_ref(raw[s], smooth[s], box)
        for part in range(HR.HAND_PARTS):
            if margins[part] > 1e-6:
                assert tuple(points[person, hd, part]) == tuple(pts[part]) and tuple(b["peaks"][s, part].cpu().numpy()) == tuple(pks[part]), (s, part)
                compared += 1
                with_point += int(pts[part][0] > 0)
    print(f"hand stage: {compared} of {2 * HR.HAND_PARTS} parts compared, {with_point} with a point")
    assert compared >= HR.HAND_PARTS and with_point >= 5
    assert (points[1:] == -1).all()
    # ... and the image: the planted body, the device's hand points, against the specification's drawing
    from controlanimate_amd.openpose import sin_table
    sk = _k().pose_draw_hands(torch.from_numpy(kp).to(DEV), torch.tensor([1], dtype=torch.int32, device=DEV), torch.from_numpy(sin_table()).to(DEV), b["points"], None,
                              ws["xmap"], ws["ymap"], 512, 512)
    want = HR.draw_ref(kp[0], 1, points, None, 512, 512)
    assert np.array_equal(sk[0].cpu().numpy(), want) and (want == np.array(HR.HAND_CIRCLE_COLOR, np.uint8)).all(axis=2).sum() > 200
    timings = {}
    ann.timings = timings
    try:
        _run_stage(ann, frame, kp)
    finally:
        ann.timings = None
    assert {name: len(v) for name, v in timings.items()} == OH.HAND_STAGES
    ann.max_activation_bytes = 736 * 736 * 64 * 2
    try:
        assert ann._hand.chunk_crops(736, True) == 1 and ann._hand.chunk_crops(184, True) == 16
        again = _run_stage(ann, frame, kp)
        assert all(np.array_equal(t.cpu().numpy(), h) for t, h in zip(again["heat"], heat)) and np.array_equal(again["buf"]["points"][0].cpu().numpy(), points)
    finally:
        del ann.max_activation_bytes


# ---- the annotator ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e():
    import face_ref as FR
    from controlanimate_amd.openpose import OpenposeAnnotator
    fr = R.frames_fixture()
    body = R.e2e_state_dict(0, fr)
    hand, face = HR.hand_state_dict(0), FR.face_state_dict(0)
    return fr, body, hand, face, OpenposeAnnotator(body, device=DEV, detect_resolution=256, image_resolution=256, hand=hand, face=face)


def test_hands_of_the_chains_own_keypoints(e2e):
    """256 x 320 frames through the whole annotator: the boxes, slots and overflow word are the specification's on the chain's own keypoints,
    points only for hands that got a slot; the image is the specification's drawing of the device's bodies, hand points and face points,
    with and without the face stage; poses() and faces() keep their results; without `hand=` (or with include_hand=False) every byte is
    what it is without a hand network."""
    import face_ref as FR
    from controlanimate_amd.openpose import OpenposeAnnotator
    fr, body, hand, face, ann = e2e
    h, w = fr.shape[1:3]
    kp, people, overflow = ann.poses(fr)
    fpoints, fboxes, fover = ann.faces(fr)
    points, boxes, hover = ann.hands(fr)
    sk = ann.skeleton(fr)
    ctrl = ann.annotate_batch(fr, rep=2)
    torch.cuda.synchronize()
    assert tuple(points.shape) == (2, R.MAX_PEOPLE, 2, HR.HAND_PARTS, 2) and tuple(boxes.shape) == (2, R.MAX_PEOPLE, 2, 4)
    coords = ann.workspace(2, h, w)["decode"]["coords"].cpu().numpy()
    hand_only = OpenposeAnnotator(body, device=DEV, detect_resolution=256, image_resolution=256, hand=hand)
    sk_hand_only = hand_only.skeleton(fr)
    slots_seen = 0
    for i in range(2):
        want_boxes, slots, over = HR.boxes_ref(kp[i].cpu().numpy(), int(people[i]), h, w, 2)
        print(f"frame {i}: {int(people[i])} people, hand slots {slots}, overflow {over}")
        slots_seen += len(slots)
        assert np.array_equal(boxes[i].cpu().numpy(), want_boxes) and int(hover[i]) == (over | int(overflow[i]))
        taken = np.zeros((R.MAX_PEOPLE, 2), bool)
        for person, hd, box, ok in slots:
            taken[person, hd] = ok
        assert (points[i].cpu().numpy()[~taken] == -1).all()
        assert np.array_equal(sk[i].cpu().numpy(), HR.draw_ref(coords[i], int(people[i]), points[i].cpu().numpy(), fpoints[i].cpu().numpy(), h, w)), i
        assert np.array_equal(sk_hand_only[i].cpu().numpy(), HR.draw_ref(coords[i], int(people[i]), points[i].cpu().numpy(), None, h, w)), i
    assert slots_seen >= 2, "a test that can pass with zero hands is not accepted"
    assert torch.equal(ctrl.cpu(), (sk.cpu().permute(0, 3, 1, 2).float() / 255).repeat(2, 1, 1, 1))
    assert torch.equal(hand_only.hands(fr)[0], points)
    timings = {}
    ann.timings = timings
    try:
        ann.skeleton(fr)
        torch.cuda.synchronize()
    finally:
        ann.timings = None
    assert {name: len(v) for name, v in timings.items()} == ann.STAGES and set(OH.HAND_STAGES) <= set(ann.STAGES)
    for kw in ({}, {"face": face}):
        off = OpenposeAnnotator(body, device=DEV, detect_resolution=256, image_resolution=256, hand=hand, include_hand=False, **kw)
        without = OpenposeAnnotator(body, device=DEV, detect_resolution=256, image_resolution=256, **kw)
        assert off._hand is None and torch.equal(off.skeleton(fr), without.skeleton(fr)) and torch.equal(off.annotate_batch(fr, rep=2), without.annotate_batch(fr, rep=2))
        assert all(torch.equal(a, b) for a, b in zip(without.poses(fr), (kp, people, overflow)))
        if kw:
            assert all(torch.equal(a, b) for a, b in zip(without.faces(fr), (fpoints, fboxes, fover)))


def test_body_hands_and_faces_replay_in_a_captured_graph(e2e):
    """The whole chain -- body, hands, faces and their drawing -- captured once and replayed on two inputs: the eager results."""
    fr, body, hand, face, ann = e2e
    eager = [ann.annotate_batch(torch.from_numpy(f).to(DEV), rep=2).clone() for f in (fr, fr[::-1].copy())]
    assert not torch.equal(eager[0], eager[1])
    buf = torch.from_numpy(fr).to(DEV)
    out = torch.empty((4, 3, 256, 320), dtype=torch.float32, device=DEV)
    ann.annotate_batch(buf, out=out, rep=2)   # warm-up: the workspaces and the weights are on the device before the capture
    out.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ann.annotate_batch(buf, out=out, rep=2)
    for i in (0, 1, 0):
        buf.copy_(torch.from_numpy(fr if i == 0 else fr[::-1].copy()).to(DEV))
        graph.replay()
        assert torch.equal(out, eager[i]), i
    blue = (out[:2, 2] == 1.0) & (out[:2, 0] == 0.0) & (out[:2, 1] == 0.0)
    assert int(blue.sum()) > 50   # the hands' circles went through


# ---- draw ------------------------------------------------------------------------------------------------------------------------------
def _planted_hands():
    """Hand points of the two people of pose_ref's draw case 'two' (192 x 256).  Person 0's left hand holds the edge shapes: horizontal,
    vertical, 45 degrees, shallow, zero length, a point with x = 0 (not drawn), the corner (W - 1, H - 1), edges along the right, left and
    top borders; its right hand and person 1's hands lie across the bodies."""
    pts = -np.ones((R.MAX_PEOPLE, 2, HR.HAND_PARTS, 2), np.int32)
    left = {0: (60, 40), 1: (100, 40), 2: (100, 90), 3: (130, 120), 4: (200, 128), 5: (60, 40), 6: (0, 50), 7: (255, 191), 8: (255, 100), 9: (1, 1), 10: (1, 150),
            11: (120, 1), 12: (250, 1), 13: (61, 43), 14: (66, 44), 17: (40, 0), 18: (30, 30)}
    for q, xy in left.items():
        pts[0, 0, q] = xy
    for q in range(HR.HAND_PARTS):
        pts[0, 1, q] = (30 + q * 10, 60 + (q * 37) % 100)
        pts[1, 0, q] = (140 + (q % 7) * 9, 30 + (q // 7) * 40)
        pts[1, 1, q] = (90 + (q * 53) % 120, 100 + (q * 29) % 80)
    pts[1, 1, 4] = (-1, -1)
    return pts


def _planted_faces():
    pts = -np.ones((R.MAX_PEOPLE, 71, 2), np.int32)
    for q in range(71):
        pts[0, q] = (40 + (q % 12) * 14, 35 + (q // 12) * 15)    # over person 0's own hands
        pts[1, q] = (135 + (q % 9) * 8, 28 + (q // 9) * 10)
    return pts


@pytest.mark.parametrize("with_faces", [False, True])
@pytest.mark.parametrize("rep", [1, 2])
def test_draw_with_hands_equals_the_specification(rep, with_faces):
    """Byte for byte on planted points: every edge shape, a second person's body over the first person's hands, a face over the same
    person's hands, with and without face points; the control tensor is the image / 255."""
    import face_ref as FR
    from controlanimate_amd.openpose import sin_table
    from controlanimate_amd.openpose_face import pixel_map
    k = _k()
    h, w = R.PLANT_H, R.PLANT_W
    coords, people = R.draw_cases()["two"]
    hands, faces = _planted_hands(), _planted_faces() if with_faces else None
    want = HR.draw_ref(coords, people, hands, faces, h, w)
    # the order matters here: hands drawn after both bodies, or faces before the hands, give another image
    late = R.draw_ref(coords, people, h, w)
    for n in range(people):
        for hd in (0, 1):
            HR.draw_hand(late, hands[n, hd])
        if with_faces:
            FR.draw_face(late, faces[n])
    assert not np.array_equal(want, late)
    if with_faces:
        swapped = np.zeros_like(want)
        for n in range(people):
            FR.draw_body(swapped, coords[n])
            FR.draw_face(swapped, faces[n])
            for hd in (0, 1):
                HR.draw_hand(swapped, hands[n, hd])
        assert not np.array_equal(want, swapped)
    colors = {tuple(int(c) for c in col) for col in HR.edge_colors()}
    seen = {tuple(int(c) for c in px) for px in want.reshape(-1, 3)}
    assert len(colors & seen) >= 12 and (0, 0, 255) in seen
    args = (torch.from_numpy(coords)[None].to(DEV), torch.tensor([people], dtype=torch.int32, device=DEV), torch.from_numpy(sin_table()).to(DEV),
            torch.from_numpy(hands)[None].to(DEV), None if faces is None else torch.from_numpy(faces)[None].to(DEV),
            torch.from_numpy(pixel_map(w)).to(DEV), torch.from_numpy(pixel_map(h)).to(DEV))
    sk = torch.empty((1, h, w, 3), dtype=torch.uint8, device=DEV)
    ctrl = torch.empty((rep, 3, h, w), dtype=torch.float32, device=DEV)
    k.pose_draw_hands(*args, h, w, skeleton=sk, control=ctrl, rep=rep)
    ctrl16 = torch.empty((rep, 3, h, w), dtype=torch.float16, device=DEV)
    k.pose_draw_hands(*args, h, w, control=ctrl16, rep=rep)
    torch.cuda.synchronize()
    got = sk[0].cpu().numpy()
    assert np.array_equal(got, want), f"{(got != want).any(axis=2).sum()} pixels differ"
    want_ctrl = (sk.cpu().permute(0, 3, 1, 2).float() / 255).repeat(rep, 1, 1, 1)
    assert torch.equal(ctrl.cpu(), want_ctrl) and torch.equal(ctrl16.cpu(), want_ctrl.half())


def test_draw_without_hand_points_is_the_drawing_with_faces():
    """No hand point at all: ca_pose_draw_hands gives ca_pose_draw_faces' bytes, and ca_pose_draw's without face points."""
    from controlanimate_amd.openpose import sin_table
    from controlanimate_amd.openpose_face import pixel_map
    k = _k()
    h, w = R.PLANT_H, R.PLANT_W
    coords, people = R.draw_cases()["two"]
    c, p, sin = torch.from_numpy(coords)[None].to(DEV), torch.tensor([people], dtype=torch.int32, device=DEV), torch.from_numpy(sin_table()).to(DEV)
    xm, ym = torch.from_numpy(pixel_map(w)).to(DEV), torch.from_numpy(pixel_map(h)).to(DEV)
    none = torch.full((1, R.MAX_PEOPLE, 2, HR.HAND_PARTS, 2), -1, dtype=torch.int32, device=DEV)
    faces = torch.from_numpy(_planted_faces())[None].to(DEV)
    assert torch.equal(k.pose_draw_hands(c, p, sin, none, faces, xm, ym, h, w), k.pose_draw_faces(c, p, sin, faces, xm, ym, h, w))
    assert torch.equal(k.pose_draw_hands(c, p, sin, none, None, xm, ym, h, w), k.pose_draw(c, p, sin, h, w))


@pytest.mark.parametrize("name", ("lllyasviel/control_v11p_sd15_openpose", "lllyasviel/sd-controlnet-openpose"))
def test_pipeline_routes_the_annotator_with_a_hand_network(name, e2e):
    from controlanimate_amd.controlresiduals_pipeline import MultiControlNetResidualsPipeline
    fr, body, hand, face, ann = e2e
    pipe = MultiControlNetResidualsPipeline.__new__(MultiControlNetResidualsPipeline)
    pipe.annotators, pipe.controlnet_names, pipe.use_lcm, pipe.prep_images, pipe.device = {"openpose": ann}, [name], False, None, torch.device(DEV)
    assert pipe._annotator_for(name) is ann
    pipe.prep_control_images(list(fr))
    assert len(pipe.prep_images) == 1 and torch.equal(pipe.prep_images[0], ann.annotate_batch(list(fr), rep=2))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_every_layer_at_side_184(stage_case, dtype):
    """One slot at side 184, layer by layer through the stage's own packed weights and launches: every layer's output against the fp32
    torch layer on the device's own input to it (CONV_BAR), the concatenation's layout and Mconv1's permutation included."""
    import torch.nn.functional as F
    k = _k()
    frame, kp, boxes, slots, inputs, sd = stage_case
    wts = OH.pack_hand_weights(sd, dtype)

    def bar(what, out, ref):
        rel_l2, max_rel = ((out - ref).norm() / ref.norm()).item(), ((out - ref).abs().max() / ref.abs().max()).item()
        assert torch.isfinite(out).all() and rel_l2 < CONV_BAR[dtype] and max_rel < 4 * CONV_BAR[dtype], (what, rel_l2, max_rel)
        return rel_l2

    def nchw(t):
        return t.float().cpu().permute(0, 3, 1, 2)

    x = torch.zeros((1, 184, 184, 8))
    x[0, :, :, :3] = torch.from_numpy(inputs[0][0].astype(np.float32) / 256 - 0.5)
    x = x.to(dtype).to(DEV)
    worst = 0.0
    for layer, wb in zip(OH.FRONT, wts["front"]):
        if layer == "pool":
            y = k.maxpool2x2(x, torch.empty((1, x.shape[1] // 2, x.shape[2] // 2, x.shape[3]), dtype=dtype, device=DEV))
            assert torch.equal(nchw(y), F.max_pool2d(nchw(x), 2))
        else:
            y = k.conv3x3(x, wb[0].to(DEV), bias=wb[1].to(DEV), act=k.ACT_RELU, out=torch.empty((*x.shape[:3], wb[0].shape[0]), dtype=dtype, device=DEV), split_k=False)
            worst = max(worst, bar(layer[0], nchw(y), F.relu(F.conv2d(nchw(x), wb[0].float().permute(0, 3, 1, 2), wb[1], padding=1))))
        x = y
    rows = 23 * 23
    feat = x.view(rows, 128)
    cat = torch.zeros((1, 23, 23, OH.CAT), dtype=dtype, device=DEV)
    cat2d = cat.view(rows, OH.CAT)
    k.copy_cols(feat, cat2d, 0)
    heat_cols = cat2d[:, 128:128 + OH.HEAT_COLS]

    def lin(what, a, wb, relu, out, out_f32=False):
        k.gemm(a, wb[0].to(DEV), bias=wb[1].to(DEV), act=k.ACT_RELU if relu else k.ACT_NONE, out=out, out_f32=out_f32)
        ref = a.float().cpu() @ wb[0].float().t() + wb[1]
        return bar(what, out.float().cpu(), F.relu(ref) if relu else ref)

    fc = torch.empty((rows, 512), dtype=dtype, device=DEV)
    worst = max(worst, lin("conv6_1_CPM", feat, wts["stage1"]["fc"], True, fc), lin("conv6_2_CPM", fc, wts["stage1"]["out"], False, heat_cols))
    assert torch.equal(cat2d[:, :128], feat) and float(cat2d[:, 150:].abs().max()) == 0.0
    final = torch.empty((rows, OH.HEAT_COLS), dtype=torch.float32, device=DEV)
    for t, stage in enumerate(wts["stages"]):
        a = cat
        for i in range(5):
            w7, b7 = stage["conv7"][i]
            y = k.conv7x7([a], [w7.to(DEV)], biases=[b7.to(DEV)], relu=True, direct=True)[0]
            if i == 0:   # the module's convolution on cat([heat 22, features 128]) with the checkpoint's own weight
                ref = F.relu(F.conv2d(torch.cat([nchw(a)[:, 128:150], nchw(a)[:, :128]], 1), sd[f"Mconv1_stage{t + 2}.weight"].to(dtype).float(), b7, padding=3))
            else:
                ref = F.relu(F.conv2d(nchw(a), w7.float().permute(0, 3, 1, 2), b7, padding=3))
            worst = max(worst, bar(f"Mconv{i + 1}_stage{t + 2}", nchw(y), ref))
            a = y
        fc = torch.empty((rows, 128), dtype=dtype, device=DEV)
        worst = max(worst, lin(f"Mconv6_stage{t + 2}", a.view(rows, 128), stage["fc"], True, fc))
        last = t == len(wts["stages"]) - 1
        worst = max(worst, lin(f"Mconv7_stage{t + 2}", fc, stage["out"], False, final if last else heat_cols, out_f32=last))
    assert float(final[:, HR.HAND_MAPS:].abs().max()) == 0.0
    print(f"hand network at side 184, every layer {dtype}: worst relative L2 {worst:.3e} (bar {CONV_BAR[dtype]:.1e})")
