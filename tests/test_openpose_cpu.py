"""CPU: the OpenPose body annotator's host side (controlanimate_amd/openpose.py) and its specification (tests/pose_ref.py): the key table
against a real nn module, both key forms, the error types, the resampling tables, the Gaussian, the planted cases of the decode (each must
decode to exactly its planted keypoints and be `decided`, so the GPU tests skip nothing), the properties of the drawing, the scope
rejections, the key routing, the end-to-end fixture's peak counts, and the CPU emulation of the chain in fp16 / bf16 whose relative L2
against the fp32 maps is the expectation the device result is read against."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_ref as R  # noqa: E402

from controlanimate_amd import openpose as O  # noqa: E402
from controlanimate_amd.openpose import OpenposeAnnotator  # noqa: E402

H, W = R.PLANT_H, R.PLANT_W


@pytest.fixture(scope="module")
def sd():
    return R.pose_state_dict(0)


def test_key_table_equals_the_modules_state_dict(sd):
    assert O.pose_key_shapes() == R.key_shapes() and len(O.pose_key_shapes()) == 184
    prefixed = R.pose_state_dict(0, prefixed=True)
    assert "model0.conv1_1.weight" in prefixed and "model3_2.Mconv1_stage3_L2.weight" in prefixed
    assert set(O.bare_keys(prefixed)) == set(sd)
    O.check_state_dict(O.bare_keys(prefixed))
    a, b = OpenposeAnnotator(sd), OpenposeAnnotator(prefixed)
    assert torch.equal(a._host["stages"][1][1]["conv7"][0][0], b._host["stages"][1][1]["conv7"][0][0])


def test_state_dict_errors_name_the_tensor(sd):
    missing = {k: v for k, v in sd.items() if k != "Mconv7_stage6_L2.bias"}
    with pytest.raises(KeyError, match="Mconv7_stage6_L2.bias"):
        OpenposeAnnotator(missing)
    with pytest.raises(ValueError, match="unexpected tensor 'conv9_9.weight'"):
        OpenposeAnnotator({**sd, "conv9_9.weight": torch.zeros(1)})
    with pytest.raises(ValueError, match="Mconv1_stage2_L1.weight"):
        OpenposeAnnotator({**sd, "Mconv1_stage2_L1.weight": torch.zeros(128, 128, 7, 7)})


def test_mconv1_weights_follow_the_concatenation_layout(sd):
    a = OpenposeAnnotator(sd, dtype=torch.bfloat16)
    w, _ = a._host["stages"][0][0]["conv7"][0]     # [128, 7, 7, 192]: features | L1, 2 zeros | L2, 5 zeros
    src = sd["Mconv1_stage2_L1.weight"].permute(0, 2, 3, 1).to(torch.bfloat16)
    assert torch.equal(w[..., :128], src[..., 57:]) and torch.equal(w[..., 128:166], src[..., :38]) and torch.equal(w[..., 168:187], src[..., 38:57])
    assert float(w[..., 166:168].abs().max()) == 0 and float(w[..., 187:].abs().max()) == 0
    out_w, out_b = a._host["stages"][0][1]["out"]
    assert tuple(out_w.shape) == (24, 128) and float(out_w[19:].abs().max()) == 0 and float(out_b[19:].abs().max()) == 0
    assert tuple(a._host["front"][0][0].shape) == (64, 3, 3, 8) and float(a._host["front"][0][0][..., 3:].abs().max()) == 0


@pytest.mark.parametrize("hw", [(192, 256), (256, 320), (512, 512), (512, 768), (768, 512)])
def test_resampling_rows_sum_to_one(hw):
    g = O.geometry(*hw)
    assert g == R.geometry(*hw) and g["hs"] == 184 and g["scale"] < 1
    for full, res in ((hw[1], g["ws"]), (hw[0], g["hs"])):
        ofs, cnt, w64 = O.area_tables(full, res, g["scale"], np.float64)
        assert np.abs(w64.sum(1) - 1).max() < 1e-12 and cnt.min() >= 1 and cnt.max() <= O.AREA_TAPS
        ofs32, cnt32, w32 = O.area_tables(full, res, g["scale"])
        assert np.array_equal(w32, w64.astype(np.float32)) and ofs.min() >= 0 and (ofs + cnt).max() <= full
        tab = R.area_tab(full, res, 1.0 / g["scale"])   # the specification's own table
        assert [len(r) for r in tab] == list(cnt32) and [r[0][0] for r in tab] == list(ofs32)
        assert all(np.array_equal(np.array([x[1] for x in r], np.float32), w32[d, :len(r)]) for d, r in enumerate(tab))
    ax, gax = O.axis_matrices(hw[1], g["ws"], g["wp"])
    ay, gay = O.axis_matrices(hw[0], g["hs"], g["hp"])
    for m in (ax, gax, ay, gay):
        assert np.abs(m.sum(1) - 1).max() < 1e-12 and np.abs(m).sum(1).max() <= 2.0


def test_composite_matrices_equal_the_steps():
    h, w = 192, 256
    g = R.geometry(h, w)
    gen = np.random.default_rng(0)
    paf, heat = gen.standard_normal((38, g["hl"], g["wl"])), gen.standard_normal((19, g["hl"], g["wl"]))
    raw, smooth, full = R.maps_ref(paf, heat, h, w)
    ax, gax = O.axis_matrices(w, g["ws"], g["wp"])
    ay, gay = O.axis_matrices(h, g["hs"], g["hp"])
    assert np.abs(ay @ heat[:18] @ ax.T - raw).max() < 1e-12 and np.abs(gay @ heat[:18] @ gax.T - smooth).max() < 1e-12
    assert np.abs(ay @ paf @ ax.T - full).max() < 1e-12
    const = R.maps_ref(np.full_like(paf, 0.75), np.full_like(heat, 0.75), h, w)
    assert all(np.abs(c - 0.75).max() < 1e-12 for c in const)


def test_gaussian_taps():
    g = O.gaussian_taps()
    assert len(g) == 25 and abs(g.sum() - 1) < 1e-15 and np.array_equal(g, g[::-1]) and np.array_equal(g, R.gaussian_taps())
    assert abs(g[12] / g[11] - np.exp(0.5 / 9)) < 1e-12
    m = O.gaussian_matrix(40)
    x = np.random.default_rng(1).standard_normal((40, 40))
    assert np.abs(m @ x @ m.T - R.gaussian_ref(x)).max() < 1e-13
    step = np.zeros(40)
    step[0] = 1.0   # reflect (d c b a | a b c d): the first sample is its own mirror image
    assert abs((m @ step)[0] - (g[12] + g[11])) < 1e-15 and abs((m @ step)[3] - (g[12 - 3] + g[12 - 4])) < 1e-15


@pytest.mark.parametrize("case", R.CASES)
def test_planted_case_decodes_to_its_keypoints_and_is_decided(case):
    raw, smooth, paf, people = R.planted(case)
    ok, why = R.decided(raw, smooth, paf)
    assert ok, why
    d = R.decode_ref(raw, smooth, paf)
    got = sorted(tuple(map(tuple, d["coords"][n])) for n in range(d["people"]))
    want = sorted(tuple(map(tuple, R.expected_coords(people)[n])) for n in range(len(people)))
    assert got == want
    assert np.array_equal(d["keypoints"][:d["people"]], d["coords"][:d["people"]])   # (no coordinate of these loses a pixel in x / W * W)
    assert (d["keypoints"][d["people"]:] == -1).all()
    assert d["overflow"] == (R.OVERFLOW_PEAKS if case == "crowd_overflow" else 0)
    if case == "crowd_overflow":
        assert len(d["peaks"][0]) == R.MAX_PEAKS and d["peaks"][0][0][:2] == people[0][0]
    if case == "merge":
        assert sum(len(c) for c in d["connections"]) == 5 and len(d["connections"][17]) == 1
    if case == "weak":
        assert all(len(d["connections"][k]) == 1 for k in range(19))   # everything connects; the 0.4 rule deletes the row


def test_people_cap_sets_the_overflow_bit():
    peaks = [[(10 + 3 * i, 20, np.float32(1.0)) for i in range(R.MAX_PEAKS)] if q in (1, 2, 5) else [] for q in range(18)]
    conns = [[(i, i, 1.0) for i in range(R.MAX_PEAKS)] if k == 0 else [] for k in range(19)]
    conns[1] = [(0, 0, 1.0)]
    kp, co, people, over = R.assemble_ref(peaks, conns, H, W)
    assert over == 0 and people == 0   # 64 rows of two parts, one of three: all deleted, no 65th row was needed
    peaks[8], conns[6] = [(50, 60, np.float32(1.0))], [(63, 0, 1.0)]
    assert R.assemble_ref(peaks, conns, H, W)[3] == 0   # found == 1: extends row 63
    peaks[9], peaks[10] = [(50, 80, np.float32(1.0))], [(50, 99, np.float32(1.0))]
    conns[8] = [(0, 0, 1.0)]                            # knee -- ankle of nobody: a 65th row
    assert R.assemble_ref(peaks, conns, H, W)[3] == R.OVERFLOW_PEOPLE


def test_the_float_round_trip_can_lose_a_pixel():
    lost = [(x, w) for w in (256, 320, 512, 768) for x in range(w) if int(x / float(w) * w) != x]
    assert all(int(x / float(w) * w) == x - 1 for x, w in lost)
    print(f"x / float(W) * W truncates below x at {len(lost)} of {256 + 320 + 512 + 768} coordinates")


def test_drawing_properties():
    cases = R.draw_cases()
    one = R.draw_ref(*cases["one"], H, W)
    co = cases["one"][0][0]
    (ax, ay), (bx, by) = co[1], co[2]           # limb 0: neck -- right shoulder, colour int(255 * 0.6), 0, 0
    mid = one[(ay + by) // 2, (ax + bx) // 2 - 8]
    assert tuple(one[(ay + by) // 2, (3 * ax + bx) // 4]) in ((153, 0, 0), (153, 51, 0)) and (153, 0, 0) in {tuple(p) for p in one.reshape(-1, 3)}
    assert mid.max() > 0
    for q in range(18):                           # a circle lies over the limbs: a keypoint's own pixel has the keypoint's full colour
        x, y = co[q]
        later = [p for p in range(q + 1, 18) if abs(co[p][0] - x) <= 4 and abs(co[p][1] - y) <= 4]
        if not later:
            assert tuple(one[y, x]) == tuple(R.COLORS[q])
    two = R.draw_ref(*cases["two"], H, W)        # a later person over an earlier one
    second_only = R.draw_ref(cases["two"][0][1:], 1, H, W)
    covered = second_only.max(axis=2) > 0
    assert np.array_equal(two[covered], second_only[covered]) and (two[~covered] == R.draw_ref(cases["two"][0][:1], 1, H, W)[~covered]).all()
    edge = R.draw_ref(*cases["leaves_frame"], H, W)   # clipped at the border, drawn up to it
    assert edge[:, 0].max() > 0 and edge[0, :].max() > 0 and edge[:, W - 1].max() > 0
    zero = R.draw_ref(*cases["zero_length"], H, W)
    assert (zero.max(axis=2) > 0).sum() >= 37 and tuple(zero[80, 100]) in {tuple(c) for c in R.COLORS}
    # the pieces: the circle's rows, the polygon of a zero-size ellipse, a convex fill
    c = np.zeros((9, 9), np.uint8)
    R.circle4(c, 4, 4, 1)
    assert [int(r.sum()) for r in c] == [1, 5, 7, 7, 9, 7, 7, 5, 1]
    assert R.ellipse2poly(5, 6, 0, 0, 0) == [(5, 6), (5, 6)]
    poly = R.ellipse2poly(20, 20, 10, 4, 30)
    sq = np.zeros((40, 40), np.uint8)
    R.fill_convex_poly(sq, poly, 1)
    assert 100 < sq.sum() < 160 and sq[20, 20] == 1 and all(sq[y, x] == 1 for x, y in poly)
    rows = [np.flatnonzero(r) for r in sq if r.any()]
    assert all(len(r) == r[-1] - r[0] + 1 for r in rows)   # every row is one run: convex
    assert np.array_equal(O.sin_table(), R.SIN_TABLE) and R.SIN_TABLE[90] == 1 and R.SIN_TABLE[1] == np.float32(0.0174524)


def test_scope_rejections(sd):
    for kw in ({"include_hand": True}, {"include_face": True}, {"detect_resolution": 512, "image_resolution": 768}, {"detect_resolution": 128, "image_resolution": 128},
               {"detect_resolution": 500, "image_resolution": 500}):
        with pytest.raises(NotImplementedError):
            OpenposeAnnotator(sd, **kw)
    with pytest.raises(TypeError):
        OpenposeAnnotator(sd, dtype=torch.float32)
    a = OpenposeAnnotator(sd)
    for h, w in ((512, 512), (512, 768), (768, 512)):
        a._check_size(h, w)
    # all of these are refused before the device is touched (there is none here)
    for shape in ((512, 520), (448, 512), (512, 2112), (512, 4096)):
        with pytest.raises(NotImplementedError):
            a.skeleton([np.zeros((*shape, 3), np.uint8)])
    with pytest.raises(NotImplementedError):
        OpenposeAnnotator(sd, detect_resolution=1472, image_resolution=1472).skeleton([np.zeros((1472, 1472, 3), np.uint8)])   # H % 184 == 0
    with pytest.raises(TypeError):
        a.skeleton([np.zeros((512, 512, 3), np.float32)])
    with pytest.raises(ValueError):
        a.skeleton([np.zeros((512, 512, 3), np.uint8), np.zeros((512, 768, 3), np.uint8)])
    with pytest.raises(ValueError):
        a.annotate_batch([np.zeros((512, 512, 3), np.uint8)], rep=3)
    with pytest.raises(FileNotFoundError, match="body_pose_model.pth"):
        OpenposeAnnotator.from_pretrained("/nonexistent")


def test_from_pretrained_reads_a_local_file(tmp_path, sd):
    torch.save(R.pose_state_dict(0, prefixed=True), tmp_path / "body_pose_model.pth")
    a = OpenposeAnnotator.from_pretrained(tmp_path)
    assert torch.equal(a._host["front"][3][0], OpenposeAnnotator(sd)._host["front"][3][0])


def test_key_routing():
    from controlanimate_amd import annotators
    from controlanimate_amd.controlresiduals_pipeline import MultiControlNetResidualsPipeline
    assert annotators.OpenposeAnnotator is OpenposeAnnotator
    pipe = MultiControlNetResidualsPipeline.__new__(MultiControlNetResidualsPipeline)
    marker = object()
    pipe.annotators = {"openpose": marker, "canny": annotators.canny}
    for name in ("lllyasviel/control_v11p_sd15_openpose", "lllyasviel/sd-controlnet-openpose"):
        assert pipe._annotator_for(name) is marker
    assert pipe._annotator_for("lllyasviel/control_v11p_sd15_mlsd") is None
    pipe.annotators = {"canny": annotators.canny}
    assert pipe._annotator_for("lllyasviel/control_v11p_sd15_openpose") is None   # without the key: as before


def test_build_lists_the_source_and_the_switch():
    from controlanimate_amd import _build, _capi
    from controlanimate_amd.context import dispatch
    assert "ca_openpose.hip" in _build.SOURCES and "-ffp-contract=off" in _build.EXTRA["ca_openpose.hip"] and isinstance(dispatch.pose_conv7_direct, bool)
    assert (_capi.CA_POSE_MAX_PEAKS, _capi.CA_POSE_MAX_PEOPLE) == (O.MAX_PEAKS, O.MAX_PEOPLE) == (R.MAX_PEAKS, R.MAX_PEOPLE) == (64, 64)
    assert sum(O.STAGES.values()) == 77


@pytest.fixture(scope="module")
def e2e():
    fr = R.frames_fixture()
    sd = R.e2e_state_dict(0, fr)   # the seed of tests/test_openpose_gpu.py
    return fr, sd, R.lowres_ref(sd, fr)


def test_e2e_fixture_has_peaks_on_every_part(e2e):
    fr, sd, (paf, heat) = e2e
    for i in range(len(fr)):
        raw, smooth, full = (m.astype(np.float32) for m in R.maps_ref(paf[i].numpy(), heat[i].numpy(), *fr.shape[1:3]))
        d = R.decode_ref(raw, smooth, full)
        counts = [len(p) for p in d["peaks"]]
        print(f"frame {i}: peaks per part {counts}, {d['people']} people")
        assert min(counts) >= 1 and max(counts) <= R.MAX_PEAKS and d["overflow"] == 0 and d["people"] >= 1


@pytest.mark.parametrize("dtype,bar", [(torch.float16, 1e-2), (torch.bfloat16, 8e-2)])
def test_emulated_chain_against_fp32(e2e, dtype, bar):
    fr, sd, (paf, heat) = e2e
    sd = {k: v.to(dtype).float() for k, v in sd.items()}
    ref = torch.cat(R.lowres_ref(sd, fr), 1)
    emu = torch.cat(R.lowres_emulated(sd, fr, dtype), 1)
    rel = ((emu - ref).norm() / ref.norm()).item()
    print(f"emulated chain {dtype}: relative L2 {rel:.3e} against the fp32 maps (the device's bar: {bar:.0e})")
    assert rel <= bar
