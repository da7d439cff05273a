"""CPU: the face detector's specification (tests/retinaface_ref.py) against itself, against arithmetic done by hand and -- the one pin --
against transformers' ResNetModel through the recorded fixture; the state-dict, size and error checks of controlanimate_amd/face_align.py;
and that each planted case of tests/test_face_align_gpu.py does what its name says, by the specification alone."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import retinaface_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "retinaface_body_tiny.npz")
# the specification against the fixture, fp32 against fp32: measured 0.0 on the three taps (relative L2) -- the same torch operators in the
# same order.  Ten times that holds only on the build that recorded the fixture; the bar is what another summation order inside a
# convolution costs in fp32 (the 1e-5 of tests/test_normalbae_cpu.py's pin)
TAP_BAR = 1e-5


def load_fixture():
    z = np.load(GOLDEN)
    sd = {k[2:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith("w:")}
    return z["frames"], [torch.from_numpy(z[f"tap{i}"]) for i in range(3)], sd, list(z["versions"])


# ---- priors, fold, decode ----------------------------------------------------------------------------------------------------------------
def test_prior_count_and_first_and_last_prior_of_each_level():
    assert R.prior_count(512, 768) == (64 * 96 + 32 * 48 + 16 * 24) * 2 == 16128
    p = R.priors(512, 768)
    assert p.shape == (16128, 4) and p.dtype == np.float64
    start = 0
    for (fh, fw), step, sizes in zip(R.level_shapes(512, 768), R.STEPS, R.MIN_SIZES):
        n = 2 * fh * fw
        first, last = p[start], p[start + n - 1]
        assert first.tolist() == [0.5 * step / 768, 0.5 * step / 512, sizes[0] / 768, sizes[0] / 512]
        assert last.tolist() == [(fw - 0.5) * step / 768, (fh - 0.5) * step / 512, sizes[1] / 768, sizes[1] / 512]
        assert p[start + 1].tolist() == [0.5 * step / 768, 0.5 * step / 512, sizes[1] / 768, sizes[1] / 512]     # the cell's second prior
        assert p[start + 2, 0] == 1.5 * step / 768 and p[start + 2, 1] == 0.5 * step / 512                        # row-major: x runs first
        start += n
    assert start == 16128
    assert R.prior_count(64, 96) == 252 and R.level_shapes(64, 96) == [(8, 12), (4, 6), (2, 3)]
    assert R.level_shapes(60, 100) == [(8, 13), (4, 7), (2, 4)]                                                   # ceil


def test_bn_fold_is_an_identity_in_float64():
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(3)
    w = torch.randn((6, 4, 3, 3), generator=g, dtype=torch.float64)
    gamma, beta, mean = (torch.randn((6,), generator=g, dtype=torch.float64) for _ in range(3))
    var = 0.5 + torch.rand((6,), generator=g, dtype=torch.float64)
    x = torch.randn((2, 4, 5, 7), generator=g, dtype=torch.float64)
    want = F.batch_norm(F.conv2d(x, w, None, 1, 1), mean, var, gamma, beta, False, 0.0, R.BN_EPS)
    wf, bf = R.fold_bn(w, gamma, beta, mean, var)
    got = F.conv2d(x, wf, bf, 1, 1)
    assert ((got - want).norm() / want.norm()).item() < 1e-14


def test_decode_on_a_hand_worked_prior():
    # 64 x 96: the prior of level 0, cell (i = 2, j = 3), second size: cx = 3.5 * 8 / 96, cy = 2.5 * 8 / 64, s = 32
    idx = 2 * (2 * 12 + 3) + 1
    pri = R.priors(64, 96)[idx:idx + 1]
    assert pri[0].tolist() == [28 / 96, 20 / 64, 32 / 96, 32 / 64]
    box = np.array([[1.0, -2.0, 0.0, math.log(2.0) / 0.2]], np.float32)
    ldm = np.zeros((1, 10), np.float32)
    ldm[0, :4] = [5.0, 0.0, 0.0, -5.0]
    corners, pts = R.decode(box, ldm, pri, 64, 96)
    # centre (28 + 0.1 * 32, 20 - 0.2 * 32) = (31.2, 13.6); size (32, 32 * exp(fp32(log 2 / 0.2) * 0.2) ~ 64)
    hgt = 32 * math.exp(float(np.float32(math.log(2.0) / 0.2)) * 0.2)
    want = [31.2 - 16, 13.6 - hgt / 2, 31.2 + 16, 13.6 + hgt / 2]
    assert np.allclose(corners[0], want, rtol=0, atol=2e-5) and corners.dtype == np.float32
    assert np.allclose(pts[0, :4], [28 + 0.5 * 32, 20, 28, 20 - 0.5 * 32], rtol=0, atol=2e-5)
    assert np.allclose(pts[0, 4:], [28, 20] * 3, rtol=0, atol=2e-5)
    assert R.scores(np.array([[0.0, 0.0], [0.0, math.log(3.0)]], np.float32)).tolist() == [0.5, float(np.float32(1.0 / (1.0 + math.exp(-float(np.float32(math.log(3.0)))))))]


def test_nms_against_a_brute_force_restatement():
    rng = np.random.default_rng(5)
    for trial in range(4):
        n = 60
        xy = rng.uniform(0, 80, (n, 2))
        wh = rng.uniform(5, 40, (n, 2))
        boxes = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        iou = np.array([[R.iou_plus1(a, b) for b in boxes] for a in boxes])
        alive, keep = np.ones(n, bool), []
        for i in range(n):               # O(n^2): a kept box kills every later box that overlaps it by more than the threshold
            if alive[i]:
                keep.append(i)
                alive[i + 1:] &= ~(iou[i, i + 1:] > 0.4)
        assert R.nms(boxes, 0.4) == keep and 1 < len(keep) < n
    assert R.iou_plus1([0, 0, 9, 9], [0, 0, 9, 9]) == 1.0 and R.iou_plus1([0, 0, 9, 9], [20, 20, 29, 29]) == 0.0
    assert R.iou_plus1([0, 0, 9, 9], [5, 0, 14, 9]) == 50 / 150


def test_order_breaks_ties_by_the_lower_prior_index():
    sc = np.array([0.5, 0.9, 0.9, 0.7, 0.9], np.float32)
    idx = np.array([10, 40, 20, 30, 5])
    assert idx[R.order(sc, idx)].tolist() == [5, 20, 40, 30, 10]


# ---- fit, inverse, warp ------------------------------------------------------------------------------------------------------------------
def _design(src):
    a = np.zeros((10, 4))
    for i, (x, y) in enumerate(src):
        a[2 * i], a[2 * i + 1] = [x, -y, 1, 0], [y, x, 0, 1]
    return a


def test_similarity_fit_against_lstsq_and_a_known_transform():
    rng = np.random.default_rng(9)
    for _ in range(5):
        src = rng.uniform(0, 700, (5, 2))
        sol = np.linalg.lstsq(_design(src), R.TEMPLATE.reshape(-1), rcond=None)[0]
        want = np.array([[sol[0], -sol[1], sol[2]], [sol[1], sol[0], sol[3]]])
        got = R.similarity_fit(src)
        assert np.abs(got - want).max() / np.abs(want).max() < 1e-12
    # the five points are the template moved by a known similarity: the fit is its inverse, to round-off
    s, th, t = 0.37, 0.6, np.array([211.0, -35.0])
    rot = s * np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
    src = R.TEMPLATE @ rot.T + t
    got = R.similarity_fit(src)
    inv = np.linalg.inv(rot)
    assert np.allclose(got[:, :2], inv, rtol=0, atol=1e-12) and np.allclose(got[:, 2], -inv @ t, rtol=0, atol=1e-9)
    assert np.allclose(R.similarity_fit(R.TEMPLATE), [[1, 0, 0], [0, 1, 0]], rtol=0, atol=1e-12)


def test_inverse_against_numpy():
    rng = np.random.default_rng(2)
    for up in (1, 2):
        m = rng.normal(size=(2, 3)) * [1, 1, 100]
        want = np.linalg.inv(np.vstack([m, [0, 0, 1]]))[:2] * up
        assert np.allclose(R.inverse_affine(m, up), want, rtol=1e-12, atol=1e-12)


def test_warp_identity_and_integer_shift():
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (600, 520, 3), dtype=np.uint8)
    ident = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    assert np.array_equal(R.warp_affine(img, ident), img[:512, :512])
    small = img[:100, :90]
    out = R.warp_affine(small, np.array([[1.0, 0, 7], [0, 1.0, 3]]))      # the image moves right by 7 and down by 3
    want = np.empty((512, 512, 3), np.uint8)
    want[:] = R.BORDER
    want[3:103, 7:97] = small
    assert np.array_equal(out, want)
    # bgr: the border value turns with the channels, the pixels stay
    out = R.warp_affine(small, np.array([[1.0, 0, 7], [0, 1.0, 3]]), bgr=True)
    want[:] = R.BORDER[::-1]
    want[3:103, 7:97] = small
    assert np.array_equal(out, want)
    # a half-pixel shift of a two-level image: the fixed-point weights are exact halves, the result rounds half up
    cols = np.zeros((4, 8, 3), np.uint8)
    cols[:, 1::2] = 101
    out = R.warp_affine(cols, np.array([[1.0, 0, 0.5], [0, 1.0, 0]]))
    assert out[1, 1:7].tolist() == [[51] * 3] * 6       # (0 + 101 + 1) >> 1


# ---- the pin ---------------------------------------------------------------------------------------------------------------------------------
def test_specification_body_reproduces_the_transformers_fixture():
    frames, taps, sd, versions = load_fixture()
    assert os.path.getsize(GOLDEN) < 1 << 20
    with torch.no_grad():
        got = R.body(sd, R.preprocess(frames))
    assert [tuple(t.shape) for t in got] == [(3, 64, 8, 12), (3, 128, 4, 6), (3, 256, 2, 3)] == [tuple(t.shape) for t in taps]
    rels = [((a - b).norm() / b.norm()).item() for a, b in zip(got, taps)]
    print(f"specification against {versions}: {['%.2e' % r for r in rels]}")
    assert max(rels) <= TAP_BAR
    # the fixture's names are the product's: the body part of the tiny geometry's tensor list
    from controlanimate_amd import face_align as fa
    want = {k: s for k, s in fa.retinaface_key_shapes(fa.Geometry(8, (32, 64, 128, 256), 128)).items() if k.startswith("body.")}
    assert {k: tuple(v.shape) for k, v in sd.items()} == want


# ---- the product's host side ---------------------------------------------------------------------------------------------------------------
TINY = (8, (32, 64, 128, 256), 128)


def _tiny_sd(seed=0):
    from controlanimate_amd import face_align as fa
    return R.seeded_state_dict(fa.retinaface_key_shapes(fa.Geometry(*TINY)), seed)


def test_key_shapes_count_and_names():
    from controlanimate_amd import face_align as fa
    shapes = fa.retinaface_key_shapes()
    convs = [k for k in shapes if len(shapes[k]) == 4]
    # 1 + 16 * 3 + 4 shortcuts in the body, 3 + 2 in the FPN, 15 in the SSH modules, 9 heads
    assert len(convs) == 53 + 5 + 15 + 9
    assert shapes["body.layer4.0.downsample.0.weight"] == (2048, 1024, 1, 1) and shapes["body.layer1.0.conv1.weight"] == (64, 64, 1, 1)
    assert shapes["fpn.output1.0.weight"] == (256, 512, 1, 1) and shapes["ssh2.conv7x7_3.0.weight"] == (64, 64, 3, 3)
    assert shapes["ssh1.conv3X3.0.weight"] == (128, 256, 3, 3) and shapes["LandmarkHead.2.conv1x1.weight"] == (20, 256, 1, 1)
    assert shapes["ClassHead.0.conv1x1.bias"] == (4,) and shapes["BboxHead.1.conv1x1.weight"] == (8, 256, 1, 1)
    n = sum(int(np.prod(s)) for k, s in shapes.items() if not k.rsplit(".", 1)[1].startswith("running_"))
    assert 27.0e6 < n < 27.6e6       # RetinaFace-ResNet50 is published with about 27.3 M parameters


def test_state_dict_checks_name_the_tensor():
    from controlanimate_amd import face_align as fa
    geo = fa.Geometry(*TINY)
    sd = _tiny_sd()
    fa.check_state_dict(sd, geo)
    fa.FaceAligner({"module." + k: v for k, v in sd.items()}, geometry=geo)           # `module.` is stripped
    fa.FaceAligner({**sd, "body.bn1.num_batches_tracked": torch.tensor(0)}, geometry=geo)
    with pytest.raises(KeyError, match="ssh2.conv5X5_1.0.weight"):
        fa.check_state_dict({k: v for k, v in sd.items() if k != "ssh2.conv5X5_1.0.weight"}, geo)
    with pytest.raises(ValueError, match="body.layer9"):
        fa.check_state_dict({**sd, "body.layer9.0.conv1.weight": torch.zeros(1)}, geo)
    with pytest.raises(ValueError, match="fpn.merge1.0.weight"):
        fa.check_state_dict({**sd, "fpn.merge1.0.weight": torch.zeros((128, 128, 1, 1))}, geo)
    with pytest.raises(ValueError, match="body.conv1.weight"):
        fa.FaceAligner(sd)                                                            # the tiny widths against the full geometry: a wrong shape


def test_constructor_and_size_errors_fire_before_the_device(monkeypatch, tmp_path):
    from controlanimate_amd import face_align as fa
    geo = fa.Geometry(*TINY)
    sd = _tiny_sd()
    al = fa.FaceAligner(sd, geometry=geo)
    assert al.max_faces == 4 and al.conf_threshold == 0.97 and al.nms_threshold == 0.4 and al.eye_dist_threshold == 5 and al.dtype == torch.float16
    assert fa.FaceAligner.STAGES == fa.STAGES and al.timings is None
    monkeypatch.setattr(al, "_device", lambda: (_ for _ in ()).throw(AssertionError("the device was touched")))
    for h, w in ((500, 768), (512, 760), (16, 32)):
        with pytest.raises(NotImplementedError):
            al._check_size(h, w)
        with pytest.raises(NotImplementedError):
            al.align([np.zeros((h, w, 3), np.uint8)])
    for h, w in ((512, 512), (512, 768), (768, 512), (1024, 1536), (2048, 3072), (64, 96)):
        al._check_size(h, w)
    with pytest.raises(TypeError):
        al.align([np.zeros((64, 96, 3), np.float32)])
    with pytest.raises(ValueError):
        al.align([np.zeros((64, 96, 3), np.uint8), np.zeros((96, 64, 3), np.uint8)])
    with pytest.raises(TypeError):
        fa.FaceAligner(sd, geometry=geo, dtype=torch.float32)
    with pytest.raises(ValueError):
        fa.FaceAligner(sd, geometry=geo, max_faces=65)
    with pytest.raises(ValueError):
        fa.FaceAligner(sd, geometry=geo, conf_threshold=1.0)
    with pytest.raises(NotImplementedError, match="slope"):
        fa.FaceAligner(sd, geometry=fa.Geometry(8, (32, 64, 128, 256), 64))           # facexlib's LeakyReLU(0.1)
    assert fa.leaky_slope(64) == 0.1 and fa.leaky_slope(256) == 0.0 and R.leaky_slope(64) == 0.1 and R.leaky_slope(65) == 0.0
    with pytest.raises(FileNotFoundError):
        fa.FaceAligner.from_pretrained(str(tmp_path))
    torch.save(sd, tmp_path / fa.WEIGHTS_NAME)
    assert fa.FaceAligner.from_pretrained(str(tmp_path), geometry=geo, max_faces=2).max_faces == 2
    # the chunking of the hand stage: as many frames per pass as keep the largest operand within max_activation_bytes
    full = fa.FaceAligner.__new__(fa.FaceAligner)
    full._bytes_per_pixel = 32
    assert full.chunk_frames(2048, 3072) == 10 and full.chunk_frames(512, 768) == 170


def test_no_cpu_fallback(monkeypatch):
    from controlanimate_amd import _capi, face_align as fa
    al = fa.FaceAligner(_tiny_sd(), geometry=fa.Geometry(*TINY))
    monkeypatch.setattr(_capi, "_lib", None)
    monkeypatch.setattr(_capi, "LIB_PATH", "/nonexistent/libcontrolanimate_hip.so")
    with pytest.raises(_capi.CAHipUnavailable):
        al.align([np.zeros((64, 96, 3), np.uint8)])


def test_face_helper_surface_and_paste_back_raises():
    from controlanimate_amd import face_align as fa
    from controlanimate_amd import gfpgan
    assert gfpgan.FaceAligner is fa.FaceAligner and gfpgan.FaceHelper is fa.FaceHelper
    helper = fa.FaceHelper(fa.FaceAligner(_tiny_sd(), geometry=fa.Geometry(*TINY)))
    for name in ("clean_all", "read_image", "get_face_landmarks_5", "align_warp_face", "add_restored_face", "get_inverse_affine", "paste_faces_to_input_image"):
        assert callable(getattr(helper, name))
    assert helper.cropped_faces == [] and helper.restored_faces == []
    with pytest.raises(NotImplementedError, match=re.escape("paste-back (ParseNet mask, inverse warp, blend) is not built yet")):
        helper.paste_faces_to_input_image()
    helper.add_restored_face(np.zeros((512, 512, 3), np.uint8))
    assert len(helper.restored_faces) == 1
    helper.clean_all()
    assert helper.restored_faces == []
    with pytest.raises(ValueError):
        helper.get_face_landmarks_5()


def test_pack_heads_round_trip_and_layout():
    from controlanimate_amd import face_align as fa
    rng = np.random.default_rng(1)
    p = R.prior_count(64, 96)
    cls, box, ldm = (rng.normal(size=(3, p, k)).astype(np.float32) for k in (2, 4, 10))
    levels = fa.pack_heads(cls, box, ldm, 64, 96)
    assert [t.shape for t in levels] == [(3, 8, 12, 32), (3, 4, 6, 32), (3, 2, 3, 32)]
    back = fa.unpack_heads(levels)
    assert all(np.array_equal(a, b) for a, b in zip(back, (cls, box, ldm)))
    # prior 2 * 96 + 1 of frame 1 is the second prior of level 1's cell 0: class at columns 2, 3, box at 8 .. 11, landmarks at 22 .. 31
    k = 2 * 96 + 1
    assert levels[1][1, 0, 0, 2:4].tolist() == cls[1, k].tolist() and levels[1][1, 0, 0, 8:12].tolist() == box[1, k].tolist()
    assert levels[1][1, 0, 0, 22:32].tolist() == ldm[1, k].tolist()


def test_abi_constants_and_symbols():
    from controlanimate_amd import _capi as capi, face_align as fa
    header = open(os.path.join(ROOT, "include", "controlanimate_hip.h")).read()
    assert capi.ABI_VERSION == 16
    for name, val in (("CA_RFACE_MAX_CAND", 1024), ("CA_RFACE_HEAD_COLS", 32), ("CA_RFACE_DET_COLS", 15), ("CA_RFACE_MAX_FACES", 64), ("CA_RFACE_OVERFLOW_CAND", 1),
                      ("CA_RFACE_OVERFLOW_FACES", 2), ("CA_RFACE_CENTER", 1), ("CA_RFACE_LARGEST", 2), ("CA_FACE_ALIGN_SIZE", 512)):
        assert getattr(capi, name) == val and re.search(rf"#define {name} {val}\b", header)
    assert (fa.MAX_CAND, fa.HEAD_COLS, fa.DET_COLS, fa.FACE_SIZE) == (1024, 32, 15, 512) == (R.MAX_CAND, 32, 15, R.FACE_SIZE)
    assert (fa.OVERFLOW_CAND, fa.OVERFLOW_FACES) == (R.OVERFLOW_CAND, R.OVERFLOW_FACES) == (1, 2)
    for name in ("ca_rface_stem", "ca_maxpool3x3s2", "ca_subsample2", "ca_add_up2", "ca_rface_decode_workspace_bytes", "ca_rface_decode", "ca_face_align", "ca_face_warp"):
        assert name in capi.SYMBOLS and re.search(rf"\b{name}\s*\(", header)


def test_entry_points_reject_bad_arguments_without_a_gpu():
    import ctypes as C
    from controlanimate_amd import _build, _capi as capi
    _build.build(verbose=False)
    lib = capi.lib()
    fake = C.c_void_p(0x1000)

    def expect(rc, who):
        assert rc < 0 and who.encode() in lib.ca_last_error(), (rc, lib.ca_last_error())

    expect(lib.ca_rface_stem(fake, fake, fake, fake, 1, 63, 64, 64, 0, 1, None), "ca_rface_stem")          # odd height
    expect(lib.ca_rface_stem(fake, fake, fake, fake, 1, 64, 63, 64, 0, 1, None), "ca_rface_stem")          # odd width
    expect(lib.ca_rface_stem(fake, fake, fake, fake, 1, 64, 64, 72, 0, 1, None), "ca_rface_stem")          # cout
    expect(lib.ca_rface_stem(fake, fake, fake, fake, 1, 64, 64, 64, 2, 1, None), "ca_rface_stem")          # bgr
    expect(lib.ca_rface_stem(None, fake, fake, fake, 1, 64, 64, 64, 0, 1, None), "ca_rface_stem")
    expect(lib.ca_maxpool3x3s2(fake, fake, 1, 8, 8, 12, 1, None), "ca_maxpool3x3s2")                       # c % 8
    expect(lib.ca_maxpool3x3s2(fake, fake, 1, 8, 8, 16, 5, None), "ca_maxpool3x3s2")                       # dtype
    expect(lib.ca_subsample2(fake, C.c_void_p(0x1004), 1, 8, 8, 16, 1, None), "ca_subsample2")             # alignment
    expect(lib.ca_add_up2(fake, fake, fake, 1, 7, 8, 16, 1, None), "ca_add_up2")                           # odd height
    assert lib.ca_rface_decode_workspace_bytes(3, 64, 96) == 3 * 252 * 8 and lib.ca_rface_decode_workspace_bytes(16, 512, 768) == 16 * 16128 * 8
    assert lib.ca_rface_decode_workspace_bytes(0, 64, 96) == 0
    dec = lambda **kw: lib.ca_rface_decode(fake, fake, fake, kw.get("n", 1), 64, 96, kw.get("conf", 0.97), 0.4, 5.0, kw.get("flags", 0), kw.get("mf", 4), fake,  # noqa: E731
                                           kw.get("wsb", 252 * 8), fake, fake, fake, None)
    expect(dec(conf=1.0), "ca_rface_decode")
    expect(dec(flags=4), "ca_rface_decode")
    expect(dec(mf=65), "ca_rface_decode")
    expect(dec(wsb=252 * 8 - 1), "ca_rface_decode")
    expect(lib.ca_face_align(fake, fake, 1, 0, 1.0, fake, fake, None), "ca_face_align")                    # max_faces
    expect(lib.ca_face_align(fake, fake, 1, 4, 0.0, fake, fake, None), "ca_face_align")                    # upscale
    expect(lib.ca_face_warp(fake, fake, fake, fake, 1, 40000, 64, 4, 0, None), "ca_face_warp")             # h >= 32768
    expect(lib.ca_face_warp(fake, fake, fake, fake, 1, 64, 96, 4, 3, None), "ca_face_warp")                # bgr
    expect(lib.ca_face_warp(fake, None, fake, fake, 1, 64, 96, 4, 0, None), "ca_face_warp")


# ---- the GPU tests' planted cases, by the specification alone -----------------------------------------------------------------------------
def test_planted_cases_do_what_their_names_say():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_face_align_gpu as G
    h, w = G.PLANT_HW
    cases = G.planted_cases()
    assert set(cases) == {"overlap_039", "overlap_041", "score_tie", "eyes_49", "eyes_51", "too_many_faces", "no_face", "center_of_two", "largest_of_two",
                          "candidate_overflow"}

    def run(name, **kw):
        c = cases[name]
        return R.detect(c["cls"], c["box"], c["ldm"], h, w, conf_threshold=G.PLANT_CONF, max_faces=G.MAX_FACES, **{**c.get("kw", {}), **kw})

    def overlap(name):
        c = cases[name]
        idx = c["planted"]
        corners, _ = R.decode(c["box"][idx], c["ldm"][idx], R.priors(h, w)[idx], h, w)
        return R.iou_plus1(corners[0], corners[1])

    assert abs(overlap("overlap_039") - 0.39) < 5e-3 and overlap("overlap_039") < 0.4 - 1e-3 and run("overlap_039")["count"] == 2
    assert abs(overlap("overlap_041") - 0.41) < 5e-3 and overlap("overlap_041") > 0.4 + 1e-3 and run("overlap_041")["count"] == 1
    assert run("overlap_041")["priors"] == [cases["overlap_041"]["planted"][0]]        # the better score stays
    tie = cases["score_tie"]
    sc = R.scores(tie["cls"])
    a, b = tie["planted"]
    assert sc[a] == sc[b] and a > b and run("score_tie")["priors"] == [b]              # two overlapping boxes, equal scores: the lower index wins
    for name, want in (("eyes_49", 0), ("eyes_51", 1)):
        c = cases[name]
        _, pts = R.decode(c["box"][c["planted"]], c["ldm"][c["planted"]], R.priors(h, w)[c["planted"]], h, w)
        d = math.hypot(float(pts[0, 0]) - float(pts[0, 2]), float(pts[0, 1]) - float(pts[0, 3]))
        assert abs(d - (4.9 if want == 0 else 5.1)) < 1e-3 and run(name)["count"] == want
    many = run("too_many_faces")
    assert many["count"] == G.MAX_FACES and many["overflow"] == R.OVERFLOW_FACES and len(cases["too_many_faces"]["planted"]) == G.MAX_FACES + 1
    assert many["priors"] == cases["too_many_faces"]["planted"][:G.MAX_FACES]          # planted in the order of their scores
    none = run("no_face")
    assert none["count"] == 0 and none["overflow"] == 0 and not none["dets"].any()
    two = cases["center_of_two"]
    assert run("center_of_two", only_center_face=False)["count"] == 2
    assert run("center_of_two")["priors"] == [two["planted"][1]]                       # the SECOND by score is the one nearer the centre
    assert run("largest_of_two")["priors"] == [cases["largest_of_two"]["planted"][1]]  # ... and the larger
    over = run("candidate_overflow")
    assert over["overflow"] & R.OVERFLOW_CAND and int((R.scores(cases["candidate_overflow"]["cls"]) > np.float32(G.PLANT_CONF)).sum()) > R.MAX_CAND
