"""CPU: the host side of the OpenPose hand stage (controlanimate_amd/openpose_hand.py) against its specification (tests/hand_ref.py), and
the specification against what is installed (scipy's labelling and Gaussian, matplotlib's hsv_to_rgb): key names and rejections, the box
rule, the resize choice, the composed axis matrices, the planted decode cases, the weight packing."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hand_ref as HR  # noqa: E402
import pose_ref as R  # noqa: E402

from controlanimate_amd import openpose_hand as OH  # noqa: E402


@pytest.fixture(scope="module")
def hand_sd():
    return HR.hand_state_dict(0)


# ---- keys and rejections -------------------------------------------------------------------------------------------------------------
def test_key_shapes_are_the_reference_modules():
    assert OH.hand_key_shapes() == HR.key_shapes()
    assert OH.bare_keys({k: 0 for k in HR.key_shapes(True)}).keys() == HR.key_shapes().keys()
    assert (OH.HAND_PARTS, OH.HAND_MAPS, OH.MAP_SIZE, OH.SIDES, OH.MIN_BOX) == (HR.HAND_PARTS, HR.HAND_MAPS, HR.WSIZE, HR.SIDES, HR.MIN_BOX)
    assert (OH.OVERFLOW_HANDS, OH.OVERFLOW_HAND_RESIZE) == (HR.OVERFLOW_HANDS, HR.OVERFLOW_HAND_RESIZE) == (16, 32)
    assert OH.HAND_EDGES == HR.EDGES and len(OH.HAND_EDGES) == 20
    assert all(s % HR.STRIDE == 0 for s in OH.SIDES) and OH.MAP_SIDES == (23, 46, 69, 92)   # nothing is ever padded


def test_state_dict_rejections(hand_sd):
    OH.check_hand_state_dict(hand_sd)
    OH.check_hand_state_dict(OH.bare_keys(HR.hand_state_dict(0, prefixed=True)))
    missing = dict(hand_sd)
    del missing["Mconv3_stage4.bias"]
    with pytest.raises(KeyError, match="Mconv3_stage4.bias"):
        OH.check_hand_state_dict(missing)
    with pytest.raises(ValueError, match="unexpected tensor 'conv9.weight'"):
        OH.check_hand_state_dict({**hand_sd, "conv9.weight": torch.zeros(1)})
    with pytest.raises(ValueError, match="Mconv1_stage2.weight"):   # the face network's 199 input channels
        OH.check_hand_state_dict({**hand_sd, "Mconv1_stage2.weight": torch.zeros(128, 199, 7, 7)})
    with pytest.raises(FileNotFoundError, match="hand_pose_model.pth"):
        OH.load_hand_state_dict(os.path.join(os.path.dirname(__file__), "golden"))


def test_weight_packing(hand_sd):
    w = pack = OH.pack_hand_weights(hand_sd, torch.float16)
    assert w["front"][0][0].shape == (64, 3, 3, 8) and w["stage1"]["out"][0].shape == (OH.HEAT_COLS, 512) and w["stage1"]["out"][1].shape == (OH.HEAT_COLS,)
    assert (pack["stage1"]["out"][0][HR.HAND_MAPS:] == 0).all() and (pack["stage1"]["out"][1][HR.HAND_MAPS:] == 0).all()
    m1 = hand_sd["Mconv1_stage2.weight"]
    p = OH.pack_mconv1(m1)
    assert p.shape == (128, 7, 7, OH.CAT)
    assert torch.equal(p[..., :128], m1[:, HR.HAND_MAPS:].permute(0, 2, 3, 1)) and torch.equal(p[..., 128:150], m1[:, :HR.HAND_MAPS].permute(0, 2, 3, 1))
    assert (p[..., 150:] == 0).all()
    # the packed Mconv1 on the packed concatenation is the module's convolution on cat([heat, features])
    gen = torch.Generator().manual_seed(1)
    heat, feat = torch.randn(1, HR.HAND_MAPS, 9, 9, generator=gen), torch.randn(1, 128, 9, 9, generator=gen)
    ref = torch.nn.functional.conv2d(torch.cat([heat, feat], 1), m1, padding=3)
    cat = torch.cat([feat, heat, torch.zeros(1, OH.CAT - 150, 9, 9)], 1)
    got = torch.nn.functional.conv2d(cat, p.permute(0, 3, 1, 2), padding=3)
    assert (got - ref).abs().max() <= 1e-4 * ref.abs().max()


# ---- the specification against what is installed -----------------------------------------------------------------------------------------
def test_labelling_is_scipys():
    ndi = pytest.importorskip("scipy.ndimage")
    gen = np.random.default_rng(0)
    planes = [gen.random((HR.WSIZE, HR.WSIZE)) > t for t in (0.3, 0.5, 0.6, 0.8)] + [c[1] > 0 for c in HR.decode_cases().values()]
    for b in planes:
        want, n = ndi.label(b, structure=np.ones((3, 3)))
        got, m = HR.label_ref(b)
        assert m == n and np.array_equal(got, want)


def test_smoothing_is_scipys():
    ndi = pytest.importorskip("scipy.ndimage")
    a = np.random.default_rng(1).standard_normal((HR.WSIZE, HR.WSIZE))
    assert np.abs(R.gaussian_ref(a) - ndi.gaussian_filter(a, sigma=3)).max() <= 1e-13
    from controlanimate_amd.openpose import gaussian_matrix
    g = gaussian_matrix(HR.WSIZE)
    assert np.abs(g @ a @ g.T - ndi.gaussian_filter(a, sigma=3)).max() <= 1e-13


def test_colours_are_matplotlibs():
    colors = pytest.importorskip("matplotlib.colors")
    want = np.array([np.rint(colors.hsv_to_rgb([ie / 20.0, 1.0, 1.0]) * 255) for ie in range(20)]).astype(np.uint8)
    assert np.array_equal(HR.edge_colors(), want)


def test_colours():
    c = HR.edge_colors()
    assert np.array_equal(OH.hand_colors(), c)
    assert tuple(c[0]) == (255, 0, 0) and tuple(c[1]) == (255, 77, 0) and tuple(c[7]) == (0, 255, 25)


# ---- boxes -----------------------------------------------------------------------------------------------------------------------------
def test_box_cases():
    def hands(name, max_hands=8):
        (h, w), people = HR.BOX_CASES[name]
        return HR.boxes_ref(HR.keypoints_of(people), len(people), h, w, max_hands)

    assert [(s[0], s[1]) for s in hands("left_only")[1]] == [(0, 0)]
    assert [(s[0], s[1]) for s in hands("right_only")[1]] == [(0, 1)]
    assert [(s[0], s[1]) for s in hands("both")[1]] == [(0, 0), (0, 1)]
    assert hands("none")[1] == [] and hands("short_arm")[1] == [] and hands("width_under_20")[1] == []
    assert hands("clamped_left")[1][0][2][0] == 0 and hands("clamped_top")[1][0][2][1] == 0
    x, y, side = hands("clamped_right")[1][0][2]
    assert 767 <= x + side <= 768   # (both are truncated)
    x, y, side = hands("clamped_bottom")[1][0][2]
    assert 767 <= y + side <= 768
    assert hands("width_at_20")[1][0][2] == (492, 193, 20)
    assert hands("elbow_shoulder_rules")[1][0][2][2] == 135
    boxes, slots, over = hands("three_people", 2)
    assert [(s[0], s[1]) for s in slots] == [(0, 0), (0, 1)] and over == HR.OVERFLOW_HANDS
    assert boxes[1, 1, 2] > 0 and boxes[1, 1, 3] == -1 and boxes[2, 0, 2] > 0 and boxes[2, 0, 3] == -1
    assert [(s[0], s[1]) for s in hands("three_people")[1]] == [(0, 0), (0, 1), (1, 1), (2, 0)] and hands("three_people")[2] == 0


def test_random_boxes_are_full_squares():
    """hand_boxes asserts that every crop is the full w x w square; random arms near every border exercise it."""
    gen = np.random.default_rng(2)
    kept = 0
    for _ in range(2000):
        h, w = ((512, 512), (512, 768), (768, 512))[int(gen.integers(3))]
        pts = [(int(gen.integers(w)), int(gen.integers(h))) for _ in range(3)]
        kept += len(HR.hand_boxes(HR.keypoints_of([HR.arm(*pts)])[0], h, w))
    assert kept > 500


# ---- the resize choice -----------------------------------------------------------------------------------------------------------------
def test_resize_choice():
    want = {20: ("lanczos4",) * 4, 183: ("lanczos4",) * 4, 184: ("lanczos4",) * 4, 185: ("area", "lanczos4", "lanczos4", "lanczos4"),
            367: ("area", "lanczos4", "lanczos4", "lanczos4"), 368: ("area2x", "lanczos4", "lanczos4", "lanczos4"),
            369: ("area", "area", "lanczos4", "lanczos4"), 512: ("area", "area", "lanczos4", "lanczos4")}
    for w, modes in want.items():
        assert tuple(HR.resize_choice(w, s) for s in HR.SIDES) == modes, w
        assert tuple(OH.resize_mode(w, s) for s in OH.SIDES) == modes, w
    for w in range(HR.MIN_BOX, 2049):
        for s in HR.SIDES:
            assert OH.resize_mode(w, s).replace("none", "skipped") == HR.resize_choice(w, s)
        assert OH.resize_restated(w) == HR.restated(w)
    # the 2x path is reached by (w, side) = (368, 184) among restated crops; (736, 368), (1104, 552), (1472, 736) meet 4x / 6x / 8x at side 184
    assert [(w, s) for w in range(HR.MIN_BOX, 2049) for s in HR.SIDES if HR.restated(w) and HR.resize_choice(w, s) == "area2x"] == [(368, 184)]
    # a box is never wider than the frame's smaller side: nothing is skipped below 552, so never at 512; 576 and up can meet 552
    assert OH.unrestated_sides(512) == [] and OH.unrestated_sides(551) == [] and OH.unrestated_sides(576) == [552]
    assert OH.unrestated_sides(768) == [552, 736] and OH.unrestated_sides(2048) == [184 * k for k in range(3, 12)]


# ---- the maps --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", OH.MAP_SIDES)
def test_axis_matrix_is_the_two_resizes_in_turn(m):
    """A_s against the x8 LANCZOS4 resize and the INTER_AREA resize to 128 applied one after the other in float64 (the specification's
    own matrices), and a constant stays constant."""
    a = OH.axis_matrix(m)
    v = np.random.default_rng(m).standard_normal((m, 5))
    step = HR.area_rows(8 * m, HR.WSIZE) @ (R.lanczos_rows(m, 8 * m, 1.0 / 8) @ v)
    assert a.shape == (HR.WSIZE, m) and np.abs(a @ v - step).max() <= 1e-12
    assert np.abs(a.sum(1) - 1).max() <= 1e-12


def test_map_matrices_layout():
    from controlanimate_amd.openpose import gaussian_matrix
    mats = OH.map_matrices()
    assert mats.shape == (2, sum(OH.MAP_SIDES), HR.WSIZE) and mats.dtype == np.float32 and mats.flags["C_CONTIGUOUS"]
    row = 0
    for m in OH.MAP_SIDES:
        a = OH.axis_matrix(m)
        assert np.array_equal(mats[0, row:row + m], a.T.astype(np.float32))
        assert np.array_equal(mats[1, row:row + m], (gaussian_matrix(HR.WSIZE) @ a).T.astype(np.float32))
        row += m


def test_maps_ref_of_a_constant():
    avg, smooth = HR.maps_ref([np.full((HR.HAND_MAPS, m, m), 0.75, np.float32) for m in OH.MAP_SIDES])
    assert avg.shape == (HR.HAND_PARTS, HR.WSIZE, HR.WSIZE) and np.abs(avg - 0.75).max() <= 1e-6 and np.abs(smooth - 0.75).max() <= 1e-6


# ---- the decode ------------------------------------------------------------------------------------------------------------------------
def test_planted_decode_cases():
    cases = HR.decode_cases()
    assert {"empty", "corners", "full", "diagonal", "serpentine", "isolated", "equal_masses", "heavier_wins", "negative"} <= set(cases)
    for name, (raw, smooth, want) in cases.items():
        before = raw.copy()
        pk, masses = HR.decode_ref(raw, smooth)
        assert pk == want and np.array_equal(raw, before), name
    assert len(HR.decode_ref(*cases["serpentine"][:2])[1]) == 1 and len(HR.decode_ref(*cases["isolated"][:2])[1]) == 4096
    assert len(HR.decode_ref(*cases["diagonal"][:2])[1]) == 2
    m = HR.decode_ref(*cases["equal_masses"][:2])[1]
    assert m[0] == m[1] == 4.0


def test_random_planes_are_decided():
    """The seeded inputs of the device test: fewer than 5 % of the planes have their two best masses within 1e-6 relative."""
    raw, smooth = HR.random_planes()
    margins = [HR.mass_margin(HR.decode_ref(raw[s, p], smooth[s, p])[1]) for s in range(raw.shape[0]) for p in range(HR.HAND_PARTS)]
    assert sum(m <= 1e-6 for m in margins) < 0.05 * len(margins)
    assert sum(np.isfinite(m) for m in margins) >= len(margins) // 2   # most planes have several components


def test_to_frame():
    assert HR.to_frame((0, 0), (7, 9, 300)) == (-1, -1) and HR.to_frame((1, 0), (7, 9, 300)) == (9, -1)
    assert HR.to_frame((1, 127), (0, 0, 20)) == (-1, 19) and HR.to_frame((127, 64), (3, 4, 512)) == (511, 260)


# ---- the annotator's constructor ---------------------------------------------------------------------------------------------------------
def test_annotator_rejections(hand_sd):
    from controlanimate_amd.openpose import OpenposeAnnotator
    body = R.pose_state_dict(0)
    a = OpenposeAnnotator(body, hand=hand_sd)
    assert a._hand is not None and a._hand.max_hands == 2 and a.STAGES == {**OpenposeAnnotator.STAGES, **OH.HAND_STAGES}   # drawn by default
    assert OpenposeAnnotator(body, hand=hand_sd, include_hand=True)._hand is not None
    off = OpenposeAnnotator(body, hand=hand_sd, include_hand=False)
    assert off._hand is None and off.STAGES == OpenposeAnnotator.STAGES
    assert OpenposeAnnotator(body, hand=HR.hand_state_dict(0, prefixed=True), max_hands=4)._hand.max_hands == 4
    plain = OpenposeAnnotator(body)
    assert plain._hand is None
    with pytest.raises(NotImplementedError, match="no hand network"):
        plain.hands([np.zeros((512, 512, 3), np.uint8)])
    with pytest.raises(NotImplementedError, match="include_hand"):
        OpenposeAnnotator(body, include_hand=True)
    with pytest.raises(NotImplementedError, match="no hand network"):
        off.hands([np.zeros((512, 512, 3), np.uint8)])
    missing = dict(hand_sd)
    del missing["conv6_2_CPM.weight"]
    with pytest.raises(KeyError, match="conv6_2_CPM.weight"):
        OpenposeAnnotator(body, hand=missing)
    with pytest.raises(ValueError, match="conv6_2_CPM.weight"):   # the face network's 71 maps
        OpenposeAnnotator(body, hand={**hand_sd, "conv6_2_CPM.weight": torch.zeros(71, 512, 1, 1)})
    for bad in (0, -1, 129):
        with pytest.raises(ValueError, match="max_hands"):
            OpenposeAnnotator(body, hand=hand_sd, max_hands=bad)
    with pytest.raises(FileNotFoundError, match="hand_pose_model.pth"):
        OpenposeAnnotator(body, hand=os.path.join(os.path.dirname(__file__), "golden"))


# ---- the crop's tables -------------------------------------------------------------------------------------------------------------------
def test_blur_taps_are_the_specifications():
    assert np.array_equal(OH.blur_taps(), HR.blur_taps()) and len(OH.blur_taps()) == 7 and abs(OH.blur_taps().sum() - 1) < 1e-15


@pytest.mark.parametrize("side", OH.SIDES)
def test_resize_tables_stay_inside_the_crop(side):
    """For every box side up to 768: the LANCZOS4 rows are upscaler.lanczos4_tables's, the INTER_AREA rows have 1 .. 16 consecutive taps
    inside the crop (what ca_hand_crop reads), and a table row applied in numpy is the specification's resize, byte for byte."""
    from controlanimate_amd.upscaler import lanczos4_tables
    import face_ref as FR
    t = OH.resize_tables(side, 768)
    assert t["lz_ofs"].shape == (min(side, 768) - 19, side) and t["lz_coef"].shape == (min(side, 768) - 19, side, 8)
    for w in (20, 21, min(side, 768) - 1, min(side, 768)):
        ofs, coef = lanczos4_tables(w, side)
        assert np.array_equal(t["lz_ofs"][w - 20], ofs) and np.array_equal(t["lz_coef"][w - 20], coef)
    if side < 768:
        assert t["ar_ofs"].shape == (768 - side, side) and t["ar_w"].shape == (768 - side, side, OH.AREA_TAPS)
        ws = np.arange(side + 1, 769)[:, None]
        assert (t["ar_cnt"] >= 1).all() and (t["ar_cnt"] <= OH.AREA_TAPS).all() and (t["ar_ofs"] >= 0).all() and (t["ar_ofs"] + t["ar_cnt"] <= ws).all()
        w = side + 1 if side != 184 else 369
        gen = np.random.default_rng(side)
        img = gen.integers(0, 256, (w, w, 3), dtype=np.uint8)
        ofs, cnt, wt = (t[k][w - side - 1] for k in ("ar_ofs", "ar_cnt", "ar_w"))
        src = img.astype(np.float32)
        hor = np.zeros((w, side, 3), np.float32)
        for d in range(side):
            acc = np.zeros((w, 3), np.float32)
            for j in range(cnt[d]):
                acc = acc + wt[d, j] * src[:, ofs[d] + j]
            hor[:, d] = acc
        out = np.zeros((side, side, 3), np.float32)
        for d in range(side):
            acc = np.zeros((side, 3), np.float32)
            for j in range(cnt[d]):
                acc = acc + wt[d, j] * hor[ofs[d] + j]
            out[d] = acc
        assert np.array_equal(np.clip(np.rint(out), 0, 255).astype(np.uint8), FR.area_resize_ref(img, side, side))
    else:
        assert t["ar_ofs"] is None


def test_area_tables_reach_the_widest_admitted_box():
    """2048 / 184 = 11.1 source pixels per output pixel: 13 taps at the most, within the 16 the kernel takes."""
    from controlanimate_amd.openpose_face import area_side_tables
    ofs, cnt, w = area_side_tables(np.array([2047, 2048]), 184, OH.AREA_TAPS)
    assert cnt.max() == 13


def test_blur_reference():
    """A constant stays constant, an impulse spreads as the outer product of the taps, and the border is BORDER_REFLECT_101."""
    assert (HR.gaussian_blur_ref(np.full((20, 20, 3), 77, np.uint8)) == 77).all()
    t = HR.blur_taps()
    imp = np.zeros((21, 21, 1), np.uint8)
    imp[10, 10] = 255
    assert np.array_equal(HR.gaussian_blur_ref(imp)[7:14, 7:14, 0], np.rint(255 * np.outer(t, t)).astype(np.uint8))
    edge = np.zeros((20, 20, 1), np.uint8)
    edge[:, 1] = 200   # reflect 101: column -1 is column 1
    assert HR.gaussian_blur_ref(edge)[5, 0, 0] == int(np.rint(200 * 2 * t[4]))


# ---- the drawing -------------------------------------------------------------------------------------------------------------------------
def test_thick_line_reference():
    """A horizontal thickness-2 line is three rows (the corners at y -+ 1 round to the rows above and below) with the end circles' pixels
    one column beyond; a zero-length line is the radius-1 circle: a plus of five pixels; nothing is written outside the canvas."""
    c = np.zeros((9, 20, 3), np.uint8)
    HR.thick_line2(c, 4, 4, 14, 4, [9, 9, 9])
    on = c[..., 0] > 0
    assert on[3:6, 4:15].all() and on[4, 3] and on[4, 15] and not on[:3].any() and not on[6:].any() and on.sum() == 35
    c = np.zeros((9, 9, 3), np.uint8)
    HR.thick_line2(c, 4, 4, 4, 4, [9, 9, 9])
    assert (c[..., 0] > 0).sum() == 5 and c[4, 3:6, 0].all() and c[3, 4, 0] and c[5, 4, 0]
    c = np.zeros((6, 6, 3), np.uint8)
    HR.thick_line2(c, 1, 1, 5, 5, [9, 9, 9])
    HR.thick_line2(c, 5, 1, 5, 5, [9, 9, 9])
    assert c[..., 0].any()
    assert HR.clip_line(10, 10, -5, 5, 5, 5) == (True, 0, 5, 5, 5) and not HR.clip_line(10, 10, -5, -5, -1, -1)[0]
