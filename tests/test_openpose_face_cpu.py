"""CPU: the host side of the OpenPose face stage (controlanimate_amd/openpose_face.py) against its specification (tests/face_ref.py): key
names and rejections, the box rule, the resize tables applied in numpy against the reference's direct resize (byte for byte), the disc,
the pixel maps, the weight packing, the reference network's shape, and that the end-to-end fixture of tests/test_openpose_face_gpu.py
has a face in every frame."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import face_ref as FR  # noqa: E402
import pose_ref as R  # noqa: E402

from controlanimate_amd import openpose_face as OF  # noqa: E402
from controlanimate_amd.openpose import OpenposeAnnotator  # noqa: E402


@pytest.fixture(scope="module")
def body_sd():
    return R.pose_state_dict(0)


@pytest.fixture(scope="module")
def face_sd():
    return FR.face_state_dict(0)


# ---- keys and rejections -------------------------------------------------------------------------------------------------------------
def test_key_shapes_are_the_reference_modules():
    assert OF.face_key_shapes() == FR.key_shapes()
    assert OF.bare_keys({k: 0 for k in FR.key_shapes(True)}).keys() == FR.key_shapes().keys()
    assert (OF.FACE_SIZE, OF.FACE_HEAT, OF.FACE_PARTS, OF.MIN_SIDE) == (FR.FACE_SIZE, FR.FACE_HEAT, FR.FACE_PEAK_MAPS, FR.MIN_SIDE)
    assert (OF.OVERFLOW_FACES, OF.OVERFLOW_FACE_RESIZE) == (FR.OVERFLOW_FACES, FR.OVERFLOW_FACE_RESIZE) == (4, 8)


def test_rejections(body_sd, face_sd, tmp_path):
    a = OpenposeAnnotator(body_sd, face=face_sd)
    assert a._face is not None and a._face.max_faces == 2 and set(OF.FACE_STAGES) <= set(a.STAGES)
    assert OpenposeAnnotator(body_sd, face=FR.face_state_dict(0, prefixed=True))._face is not None
    assert OpenposeAnnotator(body_sd, face=face_sd, include_face=False)._face is None
    plain = OpenposeAnnotator(body_sd)
    assert plain._face is None and plain.STAGES == OpenposeAnnotator.STAGES and not set(OF.FACE_STAGES) & set(plain.STAGES)
    with pytest.raises(NotImplementedError, match="no face network"):
        OpenposeAnnotator(body_sd, include_face=True)
    with pytest.raises(NotImplementedError, match="no face network"):
        plain.faces([np.zeros((512, 512, 3), np.uint8)])
    with pytest.raises(NotImplementedError):
        OpenposeAnnotator(body_sd, face=face_sd, include_hand=True)
    missing = dict(face_sd)
    del missing["Mconv3_stage4.bias"]
    with pytest.raises(KeyError, match="Mconv3_stage4.bias"):
        OpenposeAnnotator(body_sd, face=missing)
    with pytest.raises(ValueError, match="unexpected tensor 'conv9.weight'"):
        OpenposeAnnotator(body_sd, face={**face_sd, "conv9.weight": torch.zeros(1)})
    with pytest.raises(ValueError, match="Mconv1_stage2.weight"):
        OpenposeAnnotator(body_sd, face={**face_sd, "Mconv1_stage2.weight": torch.zeros(128, 185, 7, 7)})
    with pytest.raises(ValueError, match="max_faces"):
        OpenposeAnnotator(body_sd, face=face_sd, max_faces=0)
    with pytest.raises(FileNotFoundError, match="facenet.pth"):
        OpenposeAnnotator(body_sd, face=str(tmp_path))
    torch.save(body_sd, tmp_path / "body_pose_model.pth")
    with pytest.raises(FileNotFoundError, match="facenet.pth"):
        OpenposeAnnotator.from_pretrained(str(tmp_path), face=str(tmp_path))
    torch.save(face_sd, tmp_path / "facenet.pth")
    assert OpenposeAnnotator.from_pretrained(str(tmp_path), face=str(tmp_path), max_faces=3)._face.max_faces == 3
    assert OpenposeAnnotator.from_pretrained(str(tmp_path), face=str(tmp_path / "facenet.pth"))._face is not None


def test_wiring():
    from controlanimate_amd import _build, _capi
    assert "ca_openpose_face.hip" in _build.SOURCES and "-ffp-contract=off" in _build.EXTRA["ca_openpose_face.hip"]
    for name in ("ca_face_boxes", "ca_face_crop", "ca_face_peaks", "ca_pose_draw_faces"):
        assert name in _capi.SYMBOLS
    assert _capi.ABI_VERSION == 16
    assert sum(OF.FACE_STAGES.values()) == 59


def test_entry_points_reject_bad_arguments_without_a_gpu():
    import ctypes as C
    from controlanimate_amd import _build, _capi
    _build.build(verbose=False)
    lib = _capi.lib()
    fake = C.c_void_p(0x1000)

    def expect(rc, who):
        assert rc < 0 and who.encode() in lib.ca_last_error(), (rc, lib.ca_last_error())

    expect(lib.ca_face_boxes(None, fake, None, fake, fake, fake, 1, 256, 320, 2, None), "ca_face_boxes")
    expect(lib.ca_face_boxes(fake, fake, None, fake, fake, fake, 1, 256, 320, 0, None), "ca_face_boxes")          # max_faces
    expect(lib.ca_face_boxes(fake, fake, None, fake, fake, fake, 1, 256, 4096, 2, None), "ca_face_boxes")         # w
    expect(lib.ca_face_boxes(fake, fake, C.c_void_p(0x1002), fake, fake, fake, 1, 256, 320, 2, None), "ca_face_boxes")   # alignment
    crop = [fake] * 8
    expect(lib.ca_face_crop(*([None] + crop[1:]), 1, 256, 320, 2, 0, 2, 384, 1, None), "ca_face_crop")
    expect(lib.ca_face_crop(*crop, 1, 256, 320, 2, 1, 2, 384, 1, None), "ca_face_crop")      # first + crops > slots
    expect(lib.ca_face_crop(*crop, 1, 512, 768, 2, 0, 2, 512, 1, None), "ca_face_crop")      # side_max < w
    expect(lib.ca_face_crop(*crop, 1, 256, 320, 2, 0, 2, 384, 7, None), "ca_face_crop")      # dtype
    expect(lib.ca_face_crop(*crop, 1, 256, 320, 2, 0, 2, 4096, 1, None), "ca_face_crop")     # side_max
    expect(lib.ca_face_peaks(fake, None, fake, 1, 2, 256, 320, None), "ca_face_peaks")
    expect(lib.ca_face_peaks(fake, fake, fake, 0, 2, 256, 320, None), "ca_face_peaks")       # images
    expect(lib.ca_face_peaks(fake, fake, fake, 1, 65, 256, 320, None), "ca_face_peaks")      # max_faces
    draw = [fake] * 9
    expect(lib.ca_pose_draw_faces(*([None] + draw[1:]), 1, 256, 320, 1, 2, None), "ca_pose_draw_faces")
    expect(lib.ca_pose_draw_faces(fake, fake, fake, fake, None, fake, fake, fake, fake, 1, 256, 320, 1, 2, None), "ca_pose_draw_faces")   # points without xmap
    expect(lib.ca_pose_draw_faces(*draw, 1, 256, 320, 3, 2, None), "ca_pose_draw_faces")     # rep
    expect(lib.ca_pose_draw_faces(*draw, 1, 256, 320, 1, 0, None), "ca_pose_draw_faces")     # control_dtype
    expect(lib.ca_pose_draw_faces(fake, fake, fake, fake, fake, fake, fake, None, None, 1, 256, 320, 1, 2, None), "ca_pose_draw_faces")   # no output


# ---- the box rule --------------------------------------------------------------------------------------------------------------------
H, W = FR.BOX_H, FR.BOX_W
BOX_WANT = {   # worked by hand from the rule (H = 448, W = 512)
    "eyes_only": (164, 164, 72),          # width = 3 * max(10, 12) = 36
    "ear_only": (155, 155, 90),           # width = 1.5 * 30 = 45
    "eye_beats_ear": (170, 170, 60),      # max(3 * 10, 1.5 * 15) = 30
    "no_nose": None,
    "nose_alone": None,                   # none of the four other points
    "clamped_left_top": (0, 0, 90),       # width 45: x and y clamp to 0, the side stays 90
    "half_pixel": (77, 77, 45),           # width 22.5: x = y = 77.5
    "right_rectangular": (454, 164, 72),  # width 36, x + width = 490 <= W: the side stays 72 though only 58 columns are left
    "bottom_rectangular": (164, 394, 72), # the same below: 54 rows are left
    "clamped_right_bottom": (0, 0, 448),  # width 600: x = y = 0, x + width > W -> 512, y + width > H -> 448
    "clamped_bottom": (0, 0, 448),        # width 480 <= W: width1 stays 960, width2 = H
    "side_18": None,                      # width 9
    "side_21": (189, 189, 21),            # width 10.5: x = y = 189.5
}


def test_box_rule_on_hand_written_keypoints():
    assert set(BOX_WANT) == set(FR.BOX_CASES)
    for name, people in FR.BOX_CASES.items():
        got = FR.face_box(FR.keypoints_of([people])[0], H, W)
        assert got == BOX_WANT[name], (name, got, BOX_WANT[name])
    assert FR.crop_shape(BOX_WANT["right_rectangular"], H, W) == (72, 58) and FR.crop_shape(BOX_WANT["bottom_rectangular"], H, W) == (54, 72)
    assert FR.crop_shape(BOX_WANT["clamped_right_bottom"], H, W) == (448, 448)


def test_box_threshold_19_9_against_20():
    """The rule compares the final side with 20.  Integer keypoints reach 18 and 21 only (above); the reference takes any pixel keypoints."""
    kp = FR.keypoints_of([{0: (0, 200), 17: (0, 200)}])[0].astype(np.float64)
    kp[17] = (19.9 / 3.0, 200)        # width = 1.5 * 6.633 = 9.95: the side is 19.9
    assert FR.face_box(kp, H, W) is None
    kp[17] = (20.0 / 3.0, 200)        # the side is 20 (or an ulp more)
    assert FR.face_box(kp, H, W) == (0, 190, 20)
    kp[17] = (6.625, 200)             # exactly representable: 19.875 and 20.25
    assert FR.face_box(kp, H, W) is None
    kp[17] = (6.75, 200)
    assert FR.face_box(kp, H, W) == (0, 189, 20)


def test_smallest_crop_side():
    """An unclamped box has x + width = nose.x <= W - 1 and width >= 10, so W - int(x) >= 11; a clamped one has x = 0 and side W."""
    kp = FR.keypoints_of([{0: (W - 1, 0), 14: (W - 1, 0)}])[0].astype(np.float64)
    kp[14] = (W - 1, 10.0 / 3.0)   # an eye that gives width 10: the narrowest box, as far right as a nose can be
    box = FR.face_box(kp, H, W)
    assert box == (W - 11, 0, 20) and FR.crop_shape(box, H, W) == (20, 11)
    assert FR.MIN_SIDE == OF.MIN_SIDE == 11
    box = FR.face_box(FR.keypoints_of([{0: (W - 1, 100), 16: (W - 8, 100)}])[0], H, W)   # integer keypoints: width 10.5
    assert box == (W - 12, 89, 21) and FR.crop_shape(box, H, W) == (21, 12)


def test_boxes_ref_slots_and_overflow():
    people = [FR.head(100, 100), FR.head(300, 120, eye=8), {0: (50, 300)}, FR.head(400, 300)]
    kp = FR.keypoints_of(people)
    boxes, slots, over = FR.boxes_ref(kp, 4, H, W, 2)
    assert [s[0] for s in slots] == [0, 1] and over == FR.OVERFLOW_FACES
    assert boxes[2, 2] == 0 and boxes[3, 2] > 0 and list(boxes[:4, 3]) == [0, 1, -1, -1]
    boxes, slots, over = FR.boxes_ref(kp, 4, H, W, 3)
    assert [s[0] for s in slots] == [0, 1, 3] and over == 0
    assert FR.boxes_ref(kp, 1, H, W, 3)[1] == [(0, FR.face_box(kp[0], H, W), "lanczos4")]


# ---- the resize ------------------------------------------------------------------------------------------------------------------------
def apply_tables(crop: np.ndarray, tables: dict) -> np.ndarray:
    """What ca_face_crop computes for a BGR uint8 crop [Hc, Wc, 3], in numpy, through the per-side tables."""
    hc, wc = crop.shape[:2]
    mode = OF.resize_mode(hc, wc)
    assert mode != OF.MODE_NONE
    if mode == OF.MODE_LANCZOS4:
        xo, xa = tables["lz_ofs"][wc - OF.MIN_SIDE], tables["lz_coef"][wc - OF.MIN_SIDE].astype(np.int64)
        yo, yb = tables["lz_ofs"][hc - OF.MIN_SIDE], tables["lz_coef"][hc - OF.MIN_SIDE].astype(np.int64)
        src = crop.astype(np.int64)
        hor = sum(src[:, np.clip(xo + k, 0, wc - 1)] * xa[:, k][None, :, None] for k in range(8))
        out = sum(hor[np.clip(yo + k, 0, hc - 1)] * yb[:, k][:, None, None] for k in range(8))
        return np.clip((out + (1 << 21)) >> 22, 0, 255).astype(np.uint8)
    i, j = wc - OF.FACE_SIZE, hc - OF.FACE_SIZE
    xo, xc, xw = tables["ar_ofs"][i], tables["ar_cnt"][i], tables["ar_w"][i]
    yo, yc, yw = tables["ar_ofs"][j], tables["ar_cnt"][j], tables["ar_w"][j]
    src = crop.astype(np.float32)
    hor = np.zeros((hc, OF.FACE_SIZE, 3), np.float32)
    for k in range(8):
        live = (k < xc)[None, :, None]
        hor = np.where(live, hor + xw[:, k][None, :, None] * src[:, np.minimum(xo + k, wc - 1)], hor)
    out = np.zeros((OF.FACE_SIZE, OF.FACE_SIZE, 3), np.float32)
    for k in range(8):
        live = (k < yc)[:, None, None]
        out = np.where(live, out + yw[:, k][:, None, None] * hor[np.minimum(yo + k, hc - 1)], out)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


# (Hc, Wc): every listed side (the smallest = 11, 100, 383, 384, 385, 500, 768) on an axis, with LANCZOS4 and -- from 384 on -- with AREA
RESIZE_SHAPES = [(11, 11), (100, 100), (383, 385), (385, 383), (384, 384), (20, 748), (384, 500), (500, 385), (768, 500), (500, 768), (440, 440)]


@pytest.mark.parametrize("shape", RESIZE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_resize_tables_equal_the_direct_resize(shape):
    tables = OF.resize_tables(768)
    assert tables["side_max"] == 768 and tables["lz_ofs"].shape == (768 - OF.MIN_SIDE + 1, 384) and tables["ar_w"].shape == (385, 384, 8)
    gen = np.random.default_rng(shape[0] * 1000 + shape[1])
    frame = gen.integers(0, 256, (shape[0], shape[1], 3), dtype=np.uint8)   # RGB; the box takes all of it
    want = FR.face_input_bytes(frame, (0, 0, max(shape)))
    got = apply_tables(np.ascontiguousarray(frame[:, :, ::-1]), tables)
    assert want.shape == (384, 384, 3) and np.array_equal(got, want), f"{(got != want).sum()} bytes differ"
    if shape == (384, 384):
        assert np.array_equal(want, frame[:, :, ::-1])   # LANCZOS4 at scale 1 copies


def test_resize_tables_equal_the_scalar_tables_on_a_sweep_of_sides():
    """The vectorised tables are the scalar ones bit for bit: every 23rd side up to 2048 (and the ends), LANCZOS4 and AREA."""
    from controlanimate_amd.upscaler import lanczos4_tables
    tables = OF.resize_tables(2048)
    sides = sorted(set(range(OF.MIN_SIDE, 2049, 23)) | {OF.MIN_SIDE, 757, 758, 2048})
    for s in sides:
        ofs, coef = lanczos4_tables(s, 384)
        assert np.array_equal(ofs, tables["lz_ofs"][s - OF.MIN_SIDE]) and np.array_equal(coef, tables["lz_coef"][s - OF.MIN_SIDE]), s
    for s in sorted({x for x in sides if x >= 384} | {384, 385}):
        scale = float(s) / 384   # as cv2.resize computes it from the two sizes
        ofs = np.array([r[0][0] for r in R.area_tab(s, 384, scale)], np.int32)
        i = s - 384
        assert np.array_equal(ofs, tables["ar_ofs"][i]), s
        for d, row in enumerate(R.area_tab(s, 384, scale)):
            assert tables["ar_cnt"][i][d] == len(row) and [t[0] for t in row] == list(range(row[0][0], row[0][0] + len(row))), (s, d)
            assert np.array_equal(tables["ar_w"][i][d][:len(row)], np.array([t[1] for t in row], np.float32)) and not tables["ar_w"][i][d][len(row):].any(), (s, d)


def test_resize_tables_check_the_source_row_span(monkeypatch):
    """ca_face_crop keeps SPAN_ROWS source rows per pair of output rows: tables that need more are refused on the host."""
    assert OF.SPAN_ROWS == 13
    OF.resize_tables.cache_clear()
    try:
        monkeypatch.setattr(OF, "SPAN_ROWS", 11)   # LANCZOS4 spans at most 10 rows, AREA 5 up to side 768 and 12 at side 2048
        OF.resize_tables(768)
        with pytest.raises(NotImplementedError, match="source rows"):
            OF.resize_tables(2048)
    finally:
        OF.resize_tables.cache_clear()


def test_skipped_shapes_are_recognised():
    for hc, wc, want in ((768, 768, "skipped"), (768, 384, "skipped"), (384, 1152, "skipped"), (400, 380, "skipped"), (300, 600, "skipped"),
                         (384, 384, "lanczos4"), (400, 368, "lanczos4"), (384, 385, "area"), (768, 500, "area"), (767, 768, "area"), (20, 20, "lanczos4")):
        assert FR.resize_choice(hc, wc) == want, (hc, wc)
        assert OF.resize_mode(hc, wc) == {"skipped": OF.MODE_NONE, "lanczos4": OF.MODE_LANCZOS4, "area": OF.MODE_AREA}[want], (hc, wc)
    assert FR.face_input_bytes(np.zeros((768, 768, 3), np.uint8), (0, 0, 768)) is None


# ---- the drawing's tables --------------------------------------------------------------------------------------------------------------
def test_disc_rows():
    assert FR.disc_rows(3) == {0: 3, -1: 2, 1: 2, -2: 2, 2: 2, -3: 0, 3: 0}
    canvas = np.zeros((9, 9, 3), np.uint8)
    FR.disc(canvas, 4, 4, 3, (255, 255, 255))
    assert [int(r) for r in (canvas[..., 0] > 0).sum(1)] == [0, 1, 5, 5, 7, 5, 5, 1, 0]
    # the same algorithm gives pose_ref's radius-4 circle
    a, b = np.zeros((11, 11, 3), np.uint8), np.zeros((11, 11, 3), np.uint8)
    FR.disc(a, 5, 5, 4, (1, 2, 3)), R.circle4(b, 5, 5, (1, 2, 3))
    assert np.array_equal(a, b)


@pytest.mark.parametrize("side", [320, 768])
def test_pixel_maps(side):
    got, want = OF.pixel_map(side), FR.pixel_map_ref(side)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert got[0] == 0 and (np.abs(got - np.arange(side)) <= 1).all()
    print(f"side {side}: {(got != np.arange(side)).sum()} pixels move by the float32 round trip")


# ---- packing and the network -------------------------------------------------------------------------------------------------------------
def test_mconv1_packing_reproduces_the_layer(face_sd):
    gen = torch.Generator().manual_seed(3)
    heat, feat = torch.randn((1, 71, 6, 9), generator=gen), torch.randn((1, 128, 6, 9), generator=gen)
    w, b = face_sd["Mconv1_stage3.weight"], face_sd["Mconv1_stage3.bias"]
    want = F.conv2d(torch.cat([heat, feat], 1), w, b, padding=3)
    packed = OF.pack_mconv1(w)   # [128, 7, 7, 224] on [features | heat | zeros]
    assert tuple(packed.shape) == (128, 7, 7, OF.CAT)
    cat = torch.cat([feat, heat, torch.full((1, OF.CAT - 199, 6, 9), 1e3)], 1)   # whatever the pad columns hold, their weights are zero
    got = F.conv2d(cat, packed.permute(0, 3, 1, 2), b, padding=3)
    assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max())
    assert float(packed[..., 199:].abs().max()) == 0.0
    host = OF.pack_face_weights(face_sd, torch.float16)
    assert tuple(host["front"][0][0].shape) == (64, 3, 3, 8) and float(host["front"][0][0][..., 3:].abs().max()) == 0.0
    assert tuple(host["stage1"]["out"][0].shape) == (72, 512) and float(host["stage1"]["out"][0][71].abs().max()) == 0.0 and float(host["stage1"]["out"][1][71]) == 0.0
    assert tuple(host["stages"][4]["out"][0].shape) == (72, 128) and len(host["stages"]) == 5 and len(host["stages"][0]["conv7"]) == 5


@pytest.fixture(scope="module")
def e2e():
    """The end-to-end fixture of tests/test_openpose_face_gpu.py: the body's frames and seeded weights, decoded by the fp32 reference."""
    fr = R.frames_fixture()
    sd = R.e2e_state_dict(0, fr)
    paf, heat = R.lowres_ref(sd, fr)
    out = []
    for i in range(len(fr)):
        raw, smooth, full = (m.astype(np.float32) for m in R.maps_ref(paf[i].numpy(), heat[i].numpy(), *fr.shape[1:3]))
        out.append(R.decode_ref(raw, smooth, full))
    return fr, out


def test_e2e_fixture_has_a_face_in_every_frame(e2e):
    fr, decoded = e2e
    for i, d in enumerate(decoded):
        boxes, slots, over = FR.boxes_ref(d["keypoints"], d["people"], *fr.shape[1:3], 2)
        print(f"frame {i}: {d['people']} people, slots {slots}, overflow {over}")
        assert len(slots) >= 1 and all(s[2] != "skipped" for s in slots)


def test_reference_network_shape(face_sd, e2e):
    fr, decoded = e2e
    _, slots, _ = FR.boxes_ref(decoded[0]["keypoints"], decoded[0]["people"], *fr.shape[1:3], 2)
    img = FR.face_input_bytes(fr[0], slots[0][1])
    assert img.shape == (384, 384, 3) and img.dtype == np.uint8
    heat = FR.heat_ref(face_sd, img[None])
    assert tuple(heat.shape) == (1, FR.FACE_MAPS, FR.FACE_HEAT, FR.FACE_HEAT) and bool(torch.isfinite(heat).all())
    pts = FR.peaks_ref(heat[0].numpy(), slots[0][1], *fr.shape[1:3])
    assert pts.shape == (71, 2) and pts.dtype == np.int32
