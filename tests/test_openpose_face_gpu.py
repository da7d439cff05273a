"""GPU: the face stage of the OpenPose annotator (controlanimate_amd/openpose_face.py, csrc/ca_openpose_face.hip, ca_pose_draw_faces)
against its specification (tests/face_ref.py).

Discrete decisions are tested where they are exact: the boxes, the resized crops (byte for byte), the drawing.  The peaks are an arg-max over
a bilinear upsampling that need not be bit-equal to torch's: they are compared where the specification's answer is `decided` with
PEAK_TOL = 1e-5 (the bilinear value is four products and three sums in fp32 on values below 1: under 1e-6), and on a planted exact tie.
The network meets the bars of tests/test_openpose_gpu.py (CONV_BAR for the 7x7 convolution at cin = 224, E2E_BAR for the 71 maps)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import face_ref as FR  # noqa: E402
import pose_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ("lllyasviel/control_v11p_sd15_openpose", "lllyasviel/sd-controlnet-openpose")
CONV_BAR = {torch.float16: 2.5 * 2.0 ** -10, torch.bfloat16: 2.5 * 2.0 ** -8}  # tests/test_openpose_gpu.py
E2E_BAR = {torch.float16: 1e-2, torch.bfloat16: 8e-2}
PEAK_TOL = 1e-5
BH, BW = FR.BOX_H, FR.BOX_W   # 448 x 512
MODES = {"lanczos4": 1, "area": 2, "skipped": 0}


def _k():
    from controlanimate_amd import kernels
    return kernels


def _tables(side_max):
    from controlanimate_amd import openpose_face as OF
    t = OF.resize_tables(side_max)
    return {k: (torch.from_numpy(v).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in t.items()}


def _slot_rows(slots, h, w, max_faces):
    """face_ref's slots [(person, box, choice)] of one frame -> int32 [max_faces, 8] as ca_face_boxes writes them."""
    out = np.zeros((max_faces, 8), np.int32)
    out[:, 0] = -1
    for i, (person, box, choice) in enumerate(slots):
        hc, wc = FR.crop_shape(box, h, w)
        out[i] = (person, *box, hc, wc, MODES[choice], 0)
    return out


# ---- boxes ---------------------------------------------------------------------------------------------------------------------------
FLAGGED = {0: (200, 324), 14: (125, 324)}   # width 225: the box (0, 99, 450), a 349 x 450 crop -- INTER_AREA while the rows grow


def test_face_boxes_equal_the_specification():
    k = _k()
    frames = [[p] for p in FR.BOX_CASES.values()]
    frames.append([FR.head(100, 100), FR.head(300, 120, eye=8), {0: (50, 300)}, FR.head(400, 300)])   # three boxes, max_faces = 2
    frames.append([FLAGGED, FR.head(300, 120)])
    frames.append([])
    kp = np.stack([FR.keypoints_of(f) for f in frames])
    people = np.array([len(f) for f in frames], np.int32)
    over_in = np.zeros(len(frames), np.int32)
    over_in[0] = R.OVERFLOW_PEAKS
    buf = k.face_buffers(len(frames), 2, DEV)
    k.face_boxes(torch.from_numpy(kp).to(DEV), torch.from_numpy(people).to(DEV), BH, BW, buf, torch.from_numpy(over_in).to(DEV))
    torch.cuda.synchronize()
    for i, f in enumerate(frames):
        boxes, slots, over = FR.boxes_ref(kp[i], len(f), BH, BW, 2)
        assert np.array_equal(buf["boxes"][i].cpu().numpy(), boxes), i
        assert np.array_equal(buf["slots"][i].cpu().numpy(), _slot_rows(slots, BH, BW, 2)), i
        assert int(buf["overflow"][i]) == (over | int(over_in[i])), i
    n = len(FR.BOX_CASES)
    assert int(buf["overflow"][n]) == FR.OVERFLOW_FACES and [int(v) for v in buf["slots"][n, :, 0]] == [0, 1]
    assert int(buf["overflow"][n + 1]) == FR.OVERFLOW_FACE_RESIZE and int(buf["slots"][n + 1, 0, 6]) == 0 and int(buf["slots"][n + 1, 1, 6]) == 1
    assert int(buf["overflow"][0]) == R.OVERFLOW_PEAKS   # the body's bits pass through
    no_in = k.face_buffers(len(frames), 2, DEV)
    k.face_boxes(torch.from_numpy(kp).to(DEV), torch.from_numpy(people).to(DEV), BH, BW, no_in)
    assert int(no_in["overflow"][0]) == 0 and torch.equal(no_in["boxes"], buf["boxes"])


# ---- crop ----------------------------------------------------------------------------------------------------------------------------
# boxes on a 448 x 512 frame: (x, y, side) -> the crop's shape and OpenCV's choice
CROP_BOXES = [(30, 40, 20),      # 20 x 20: both axes grow
              (200, 100, 100),   # 100 x 100
              (5, 3, 440),       # 440 x 440: INTER_AREA, both shrink
              (300, 20, 400),    # 400 x 212, clamped at the right border: k >= 1 (LANCZOS4) while the rows shrink
              (50, 30, 384),     # 384 x 384: a copy
              (0, 0, 448),       # 448 x 448: INTER_AREA
              (0, 99, 450),      # 349 x 450: flagged, zeros
              None]              # an empty slot


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_face_crop_is_byte_exact(dtype):
    k = _k()
    gen = np.random.default_rng(7)
    frames = gen.integers(0, 256, (2, BH, BW, 3), dtype=np.uint8)
    choices = [None if b is None else FR.resize_choice(*FR.crop_shape(b, BH, BW)) for b in CROP_BOXES]
    assert choices == ["lanczos4", "lanczos4", "area", "lanczos4", "lanczos4", "area", "skipped", None]
    assert FR.crop_shape(CROP_BOXES[3], BH, BW) == (400, 212)
    slots = np.stack([_slot_rows([(j, b, c) for j, (b, c) in enumerate(zip(CROP_BOXES[i:i + 4], choices[i:i + 4])) if b is not None], BH, BW, 4) for i in (0, 4)])
    out = torch.full((8, 384, 384, 8), 3.0, dtype=dtype, device=DEV)
    k.face_crop(torch.from_numpy(frames).to(DEV), torch.from_numpy(slots).to(DEV), _tables(BW), out)
    # the same crops in two passes, as a chunked network takes them
    parts = torch.full((8, 384, 384, 8), 3.0, dtype=dtype, device=DEV)
    k.face_crop(torch.from_numpy(frames).to(DEV), torch.from_numpy(slots).to(DEV), _tables(BW), parts[:3], first=0)
    k.face_crop(torch.from_numpy(frames).to(DEV), torch.from_numpy(slots).to(DEV), _tables(BW), parts[3:], first=3)
    torch.cuda.synchronize()
    assert torch.equal(out, parts)
    got = out.float().cpu()
    assert float(got[..., 3:].abs().max()) == 0.0
    for s, box in enumerate(CROP_BOXES):
        want = None if box is None else FR.face_input_bytes(frames[s // 4], box)
        if want is None:
            assert float(got[s].abs().max()) == 0.0, s   # the constant input
            continue
        have = ((got[s, :, :, :3] + 0.5) * 256).numpy()
        assert np.array_equal(have, want.astype(np.float32)), f"crop {s} {box}: {(have != want).sum()} bytes differ, max {np.abs(have - want).max()}"


# ---- the 7x7 convolution at the face network's width -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_conv7x7_at_cin_224(dtype):
    k = _k()
    g = torch.Generator().manual_seed(11)
    x = torch.randn((1, 5, 7, 224), generator=g).to(dtype)
    w = (torch.randn((128, 7, 7, 224), generator=g) * (49 * 224) ** -0.5).to(dtype)
    b = torch.randn(128, generator=g)
    out = k.conv7x7([x.to(DEV)], [w.to(DEV)], biases=[b.to(DEV)], relu=True, direct=True)[0].float().cpu()
    ref = F.relu(F.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), b, padding=3)).permute(0, 2, 3, 1)
    rel_l2, max_rel = ((out - ref).norm() / ref.norm()).item(), ((out - ref).abs().max() / ref.abs().max()).item()
    print(f"conv7x7 cin=224 {dtype}: rel_l2={rel_l2:.3e} max_err/max_ref={max_rel:.3e} (tol {CONV_BAR[dtype]:.1e})")
    assert torch.isfinite(out).all() and rel_l2 < CONV_BAR[dtype] and max_rel < 4 * CONV_BAR[dtype]


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weights():
    """The body's end-to-end weights and face weights whose last biases are set on two fixed crops of the frames (face_ref.e2e_face_state_dict)."""
    fr = R.frames_fixture()
    body = R.e2e_state_dict(0, fr)
    calib = np.stack([FR.lanczos4_resize_ref(np.ascontiguousarray(f[:, :256, ::-1]), 384, 384) for f in fr])
    return fr, body, FR.e2e_face_state_dict(0, calib)


@pytest.fixture(scope="module")
def annotator(weights):
    from controlanimate_amd.openpose import OpenposeAnnotator
    fr, body, face = weights
    return OpenposeAnnotator(body, device=DEV, detect_resolution=256, image_resolution=256, face=face)


PLANTED_HEADS = [FR.head(90, 80, eye=10, ear=18), FR.head(230, 150, eye=5, ear=9)]   # boxes (60, 50, 60) and (215, 135, 30) on 256 x 320


# ---- the network -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_facenet_meets_the_bar(weights, dtype):
    """Two crops from planted body keypoints, through the internal entry: the 71 maps against the fp32 reference on the specification's
    input, weights rounded to the device type first."""
    from controlanimate_amd.openpose import OpenposeAnnotator
    fr, body, face = weights
    face = {k_: v.to(dtype).float() for k_, v in face.items()}
    ann = OpenposeAnnotator(body, device=DEV, dtype=dtype, detect_resolution=256, image_resolution=256, face=face)
    kp = FR.keypoints_of(PLANTED_HEADS)[None]
    boxes, slots, over = FR.boxes_ref(kp[0], 2, 256, 320, 2)
    assert [s[1] for s in slots] == [(60, 50, 60), (215, 135, 30)] and over == 0
    ws = ann._faces_from(torch.from_numpy(fr[:1]).to(DEV), torch.from_numpy(kp).to(DEV), torch.tensor([2], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    got = ws["heat"].cpu()
    ref = FR.heat_ref(face, np.stack([FR.face_input_bytes(fr[0], s[1]) for s in slots])).permute(0, 2, 3, 1)
    rel = ((got[..., :71] - ref).norm() / ref.norm()).item()
    print(f"face maps {dtype}: relative L2 {rel:.3e} (bar {E2E_BAR[dtype]:.0e})")
    assert rel <= E2E_BAR[dtype]
    assert float(got[..., 71].abs().max()) == 0.0   # the pad column
    assert np.array_equal(ws["buf"]["boxes"][0].cpu().numpy(), boxes)


# ---- peaks -----------------------------------------------------------------------------------------------------------------------------
PEAK_BOXES = [(40, 30, 64), (451, 50, 97), (150, 100, 300)]   # crops of 64 x 64, 97 x 61 and 300 x 300 on 448 x 512


def test_face_peaks_on_planted_maps():
    k = _k()
    heat = FR.planted_heat()
    assert [FR.crop_shape(b, BH, BW) for b in PEAK_BOXES] == [(64, 64), (97, 61), (300, 300)]
    # persons 5, 0 and 9 own the first three slots.  The others hold a hot map that must not be read: an empty slot; person 7's, whose crop
    # shape is skipped (mode 0: the promise of OVERFLOW_FACE_RESIZE is "no points"); person 8's, whose crop would leave the frame
    persons = (5, 0, 9)
    slots = _slot_rows([(p, b, "lanczos4") for p, b in zip(persons, PEAK_BOXES)] + [(7, (0, 99, 450), "skipped")], BH, BW, 6)
    assert list(slots[3]) == [7, 0, 99, 450, 349, 450, 0, 0] and slots[4, 0] == -1
    slots[4], slots[3] = slots[3].copy(), slots[4].copy()
    slots[5] = (8, BW - 50, 20, 100, 100, 100, 1, 0)
    slots = slots[None]
    dev_heat = torch.zeros((6, 48, 48, 72))
    dev_heat[:3, :, :, :71] = torch.from_numpy(heat).permute(1, 2, 0)
    dev_heat[3:, :, :, :71] = torch.from_numpy(heat[FR.PLANT_BLOB])[None, :, :, None]   # every part with a clear peak inside the crop
    points = torch.zeros((1, 64, 71, 2), dtype=torch.int32, device=DEV)
    k.face_peaks(dev_heat.to(DEV), torch.from_numpy(slots).to(DEV), points, BH, BW)
    torch.cuda.synchronize()
    got = points[0].cpu().numpy()
    for p, box in zip(persons, PEAK_BOXES):
        ok, why = FR.decided(heat, box, BH, BW, PEAK_TOL, ties=(FR.PLANT_TIE,))
        assert ok, why
        want = FR.peaks_ref(heat, box, BH, BW)
        hc, wc = FR.crop_shape(box, BH, BW)
        up = FR.upsample_ref(heat[FR.PLANT_TIE:FR.PLANT_TIE + 1], hc, wc)[0]
        ys, xs = np.nonzero(up == np.float32(FR.TIE_VALUE))
        assert up.max() == np.float32(FR.TIE_VALUE) and len(ys) >= 2 and ys.min() < hc // 2 < ys.max()   # an exact tie, in both blocks
        assert tuple(want[FR.PLANT_TIE]) == (xs[0] + box[0], ys[0] + box[1])                              # ... that goes to the first
        assert tuple(want[FR.PLANT_UNDER]) == (-1, -1) and want[FR.PLANT_COLUMN0][0] == -1 and want[FR.PLANT_COLUMN0][1] > 0
        assert want[FR.PLANT_ROW0][1] == -1 and want[FR.PLANT_ROW0][0] > 0 and (want[FR.PLANT_BLOB] > 0).all()
        assert np.array_equal(got[p], want), (box, got[p][:6].tolist(), want[:6].tolist())
    rest = np.delete(got, persons, axis=0)
    assert (rest == -1).all()   # rows 7 and 8 among them
    # the skipped slot is the only reason: the same slot with a mode reads its hot map
    live = slots.copy()
    live[0, 4, 6] = 2
    k.face_peaks(dev_heat.to(DEV), torch.from_numpy(live).to(DEV), points, BH, BW)
    torch.cuda.synchronize()
    assert (points[0, 7].cpu().numpy() != -1).any() and (points[0, 8].cpu().numpy() == -1).all()


def test_a_skipped_crop_shape_gives_the_bit_and_no_points(weights):
    """The FLAGGED head (a 349 x 450 crop: INTER_AREA while the rows grow) and an ordinary one through the internal entry, on a 448 x 512
    frame: the bit, no point for the flagged person, points for the other, and a drawing whose only white dots are the other's."""
    from controlanimate_amd.openpose import OpenposeAnnotator, sin_table
    k = _k()
    fr, body, face = weights
    ann = OpenposeAnnotator(body, device=DEV, detect_resolution=448, image_resolution=448, face=face)
    frame = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (1, BH, BW, 3), dtype=np.uint8)).to(DEV)
    kp = FR.keypoints_of([FLAGGED, FR.head(300, 120, eye=12, ear=20)])[None]
    ws = ann._faces_from(frame, torch.from_numpy(kp).to(DEV), torch.tensor([2], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    b = ws["buf"]
    assert int(b["overflow"][0]) == FR.OVERFLOW_FACE_RESIZE
    assert [int(v) for v in b["boxes"][0, 0]] == [0, 99, 450, 0] and int(b["slots"][0, 0, 6]) == 0 and int(b["slots"][0, 1, 6]) == 1
    pts = b["points"][0].cpu().numpy()
    assert (pts[0] == -1).all() and (pts[2:] == -1).all() and (pts[1, :, 0] > 0).sum() >= 10
    coords, people, sin = torch.from_numpy(kp).to(DEV), torch.tensor([2], dtype=torch.int32, device=DEV), torch.from_numpy(sin_table()).to(DEV)
    sk = k.pose_draw_faces(coords, people, sin, b["points"], ws["xmap"], ws["ymap"], BH, BW)
    only_other = b["points"].clone()
    only_other[0, 0] = -1
    torch.cuda.synchronize()
    assert np.array_equal(sk[0].cpu().numpy(), FR.draw_ref(kp[0], 2, pts, BH, BW))
    assert torch.equal(sk, k.pose_draw_faces(coords, people, sin, only_other, ws["xmap"], ws["ymap"], BH, BW))
    assert not torch.equal(sk, k.pose_draw(coords, people, sin, BH, BW))


# ---- draw ------------------------------------------------------------------------------------------------------------------------------
def _planted_points():
    """Face points of the two people of pose_ref's draw case 'two' (192 x 256): the first person's dots lie where the second person's limbs
    pass, some points are absent, on the border, or have a coordinate 0."""
    pts = -np.ones((R.MAX_PEOPLE, 71, 2), np.int32)
    for q in range(71):
        pts[0, q] = (70 + (q % 12) * 9, 20 + (q // 12) * 11)
        pts[1, q] = (150 + (q % 9) * 7, 100 + (q // 9) * 9)
    pts[0, 3], pts[0, 4], pts[0, 5] = (-1, -1), (0, 40), (40, 0)          # absent; x = 0 and y = 0 are not drawn
    pts[1, 0], pts[1, 1], pts[1, 2] = (255, 191), (1, 1), (254, 2)          # discs that leave the frame
    pts[1, 7] = (-1, 57)
    return pts


@pytest.mark.parametrize("rep", [1, 2])
def test_draw_with_faces_equals_the_specification(rep):
    from controlanimate_amd.openpose import sin_table
    from controlanimate_amd.openpose_face import pixel_map
    k = _k()
    h, w = R.PLANT_H, R.PLANT_W
    coords, people = R.draw_cases()["two"]
    pts = _planted_points()
    want = FR.draw_ref(coords, people, pts, h, w)
    late = R.draw_ref(coords, people, h, w)
    for n in range(people):
        FR.draw_face(late, pts[n])
    assert not np.array_equal(want, late)   # the second body covers some of the first person's dots: the order matters here
    white = (want == 255).all(axis=2).sum()
    assert white > 71 * 20
    args = (torch.from_numpy(coords)[None].to(DEV), torch.tensor([people], dtype=torch.int32, device=DEV), torch.from_numpy(sin_table()).to(DEV))
    maps = (torch.from_numpy(pixel_map(w)).to(DEV), torch.from_numpy(pixel_map(h)).to(DEV))
    sk = torch.empty((1, h, w, 3), dtype=torch.uint8, device=DEV)
    ctrl = torch.empty((rep, 3, h, w), dtype=torch.float32, device=DEV)
    k.pose_draw_faces(*args, torch.from_numpy(pts)[None].to(DEV), *maps, h, w, skeleton=sk, control=ctrl, rep=rep)
    ctrl16 = torch.empty((rep, 3, h, w), dtype=torch.float16, device=DEV)
    k.pose_draw_faces(*args, torch.from_numpy(pts)[None].to(DEV), *maps, h, w, control=ctrl16, rep=rep)
    torch.cuda.synchronize()
    got = sk[0].cpu().numpy()
    assert np.array_equal(got, want), f"{(got != want).any(axis=2).sum()} pixels differ"
    want_ctrl = (sk.cpu().permute(0, 3, 1, 2).float() / 255).repeat(rep, 1, 1, 1)
    assert torch.equal(ctrl.cpu(), want_ctrl) and torch.equal(ctrl16.cpu(), want_ctrl.half())


def test_draw_without_face_points_is_ca_pose_draw():
    from controlanimate_amd.openpose import sin_table
    k = _k()
    h, w = R.PLANT_H, R.PLANT_W
    cases = R.draw_cases()
    coords = torch.from_numpy(np.stack([c[0] for c in cases.values()])).to(DEV)
    people = torch.tensor([c[1] for c in cases.values()], dtype=torch.int32, device=DEV)
    sin = torch.from_numpy(sin_table()).to(DEV)
    a = k.pose_draw(coords, people, sin, h, w)
    b = k.pose_draw_faces(coords, people, sin, None, None, None, h, w)
    none = torch.full((len(cases), 64, 71, 2), -1, dtype=torch.int32, device=DEV)
    from controlanimate_amd.openpose_face import pixel_map
    c = k.pose_draw_faces(coords, people, sin, none, torch.from_numpy(pixel_map(w)).to(DEV), torch.from_numpy(pixel_map(h)).to(DEV), h, w)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c) and int(a.max()) > 0


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_faces_end_to_end(weights, annotator):
    """From the chain's own keypoints (tests/test_openpose_face_cpu.py checks with the fp32 reference that the seeded body weights give a
    face box in every frame; the device's own boxes are asserted below)."""
    from controlanimate_amd.openpose import OpenposeAnnotator
    k = _k()
    fr, body, face = weights
    h, w = fr.shape[1:3]
    kp, people, overflow = annotator.poses(fr)
    points, boxes, fover = annotator.faces(fr)
    sk = annotator.skeleton(fr)
    ctrl = annotator.annotate_batch(fr, rep=2)
    torch.cuda.synchronize()
    ws = annotator.workspace(2, h, w)
    fws = annotator._face.workspace(2, h, w, torch.device(DEV))
    coords, heat, slots_dev = ws["decode"]["coords"].cpu().numpy(), fws["heat"].cpu(), fws["buf"]["slots"]
    crops = torch.empty((4, 384, 384, 8), dtype=torch.float16, device=DEV)
    k.face_crop(torch.from_numpy(fr).to(DEV), slots_dev, fws["tables"], crops)
    crops = crops.float().cpu()
    compared = drawn = 0
    for i in range(2):
        want_boxes, slots, over = FR.boxes_ref(kp[i].cpu().numpy(), int(people[i]), h, w, 2)
        print(f"frame {i}: {int(people[i])} people, slots {slots}, overflow {over}")
        assert len(slots) >= 1, "a test that can pass with zero faces is not accepted"
        assert np.array_equal(boxes[i].cpu().numpy(), want_boxes) and int(fover[i]) == (over | int(overflow[i]))
        assert np.array_equal(slots_dev[i].cpu().numpy(), _slot_rows(slots, h, w, 2))
        want_points = -np.ones((R.MAX_PEOPLE, 71, 2), np.int32)
        for s, (person, box, choice) in enumerate(slots):
            img = FR.face_input_bytes(fr[i], box)
            if img is None:
                continue
            have = ((crops[i * 2 + s, :, :, :3] + 0.5) * 256).numpy()
            assert np.array_equal(have, img.astype(np.float32)), (i, s)
            maps = heat[i * 2 + s, :, :, :71].permute(2, 0, 1).numpy()
            bad = FR.undecided_parts(maps, box, h, w, PEAK_TOL)
            ref_pts = FR.peaks_ref(maps, box, h, w)
            got_pts = points[i, person].cpu().numpy()
            for part in range(71):
                if part not in bad:
                    assert tuple(got_pts[part]) == tuple(ref_pts[part]), (i, s, part)
                    compared += 1
            drawn += int((got_pts[:, 0] > 0).sum())
            print(f"frame {i} slot {s}: {71 - len(bad)} parts decided, {int((ref_pts[:, 0] >= 0).sum())} with a point")
        got_all = points[i].cpu().numpy()
        taken = [s[0] for s in slots]
        assert (np.delete(got_all, taken, axis=0) == -1).all()
        assert np.array_equal(sk[i].cpu().numpy(), FR.draw_ref(coords[i], int(people[i]), got_all, h, w)), i
    assert compared >= 71 and drawn >= 10   # most parts are decided, and dots are drawn
    want_ctrl = (sk.cpu().permute(0, 3, 1, 2).float() / 255).repeat(2, 1, 1, 1)
    assert torch.equal(ctrl.cpu(), want_ctrl)
    # poses() is what it was: the same annotator without the face stage
    plain = OpenposeAnnotator(body, device=DEV, detect_resolution=256, image_resolution=256)
    kp0, people0, over0 = plain.poses(fr)
    assert torch.equal(kp0, kp) and torch.equal(people0, people) and torch.equal(over0, overflow)
    body_only = plain.skeleton(fr)
    assert not torch.equal(body_only, sk) and torch.equal(body_only, OpenposeAnnotator(body, device=DEV, detect_resolution=256, image_resolution=256, face=face,
                                                                                         include_face=False).skeleton(fr))
    # one crop per pass through the network: the same bytes
    annotator.max_activation_bytes = 384 * 384 * 64 * 2
    try:
        assert annotator._face.chunk_crops(True) == 1
        assert torch.equal(annotator.skeleton(fr), sk)
    finally:
        del annotator.max_activation_bytes
    timings = {}
    annotator.timings = timings
    try:
        annotator.skeleton(fr)
        torch.cuda.synchronize()
    finally:
        annotator.timings = None
    assert {name: len(v) for name, v in timings.items()} == annotator.STAGES


def test_chain_with_faces_replays_in_a_captured_graph(weights, annotator):
    fr = weights[0]
    eager = [annotator.annotate_batch(torch.from_numpy(f).to(DEV), rep=2).clone() for f in (fr, fr[::-1].copy())]
    assert not torch.equal(eager[0], eager[1])
    buf = torch.from_numpy(fr).to(DEV)
    out = torch.empty((4, 3, 256, 320), dtype=torch.float32, device=DEV)
    annotator.annotate_batch(buf, out=out, rep=2)   # warm-up: the workspaces and the weights are on the device before the capture
    out.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        annotator.annotate_batch(buf, out=out, rep=2)
    for i in (0, 1, 0):
        buf.copy_(torch.from_numpy(fr if i == 0 else fr[::-1].copy()).to(DEV))
        graph.replay()
        assert torch.equal(out, eager[i]), i
    assert float(out.max()) == 1.0   # white dots


@pytest.mark.parametrize("name", NAMES)
def test_pipeline_routes_the_annotator_with_faces(name, weights, annotator):
    from controlanimate_amd.controlresiduals_pipeline import MultiControlNetResidualsPipeline
    fr = weights[0]
    pipe = MultiControlNetResidualsPipeline.__new__(MultiControlNetResidualsPipeline)
    pipe.annotators, pipe.controlnet_names, pipe.use_lcm, pipe.prep_images, pipe.device = {"openpose": annotator}, [name], False, None, torch.device(DEV)
    assert pipe._annotator_for(name) is annotator
    pipe.prep_control_images(list(fr))
    assert len(pipe.prep_images) == 1 and torch.equal(pipe.prep_images[0], annotator.annotate_batch(list(fr), rep=2))
    assert float(pipe.prep_images[0].min(dim=1).values.max()) == 1.0   # a white pixel: the dots went through
