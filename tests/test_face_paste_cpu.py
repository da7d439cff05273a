"""CPU: the paste-back stage (controlanimate_amd/face_paste.py, csrc/ca_facepaste.hip) as far as it goes without a GPU -- the ABI and its
argument checks, the state-dict check and the BatchNorm fold, the specification's own properties (tests/facepaste_ref.py), the FaceHelper /
FaceRestorer.enhance plumbing with a stub paster, the missing CPU fallback, and the margin condition of the GPU label test on the fp32
specification alone."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import facepaste_ref as P  # noqa: E402
import facepaste_cases as CS  # noqa: E402
from test_capi_symbols import declared_functions  # noqa: E402
from controlanimate_amd import face_paste as FP  # noqa: E402  (every test of this file is about that module: none runs without it)

NEW = ["ca_parse_prep", "ca_conv3x3_reflect", "ca_parse_mask", "ca_parse_labels", "ca_ring_fill", "ca_mask_blur", "ca_face_paste"]


@pytest.fixture(scope="module")
def capi():
    from controlanimate_amd import _build, _capi
    _build.build(verbose=False)
    return _capi


def _fp():
    from controlanimate_amd import face_paste
    return face_paste


# ---- 1. the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree(capi):
    lib = capi.lib()
    names = declared_functions()
    for n in NEW:
        assert n in names and n in capi.SYMBOLS and hasattr(lib, n), n
    assert sorted(capi.SYMBOLS) == names and lib.ca_abi_version() == capi.ABI_VERSION == 16


def test_every_new_entry_point_rejects_bad_arguments_without_a_gpu(capi):
    lib = capi.lib()
    fake, fake2, odd = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x1004)

    def expect(rc, who):
        assert rc < 0 and who.encode() in lib.ca_last_error(), (rc, who, lib.ca_last_error())

    who = "ca_parse_prep"
    expect(lib.ca_parse_prep(None, fake, 1, 512, 1, 0, 1, None), who)
    expect(lib.ca_parse_prep(fake, None, 1, 512, 1, 0, 1, None), who)
    expect(lib.ca_parse_prep(fake, fake2, 0, 512, 1, 0, 1, None), who)          # no faces
    expect(lib.ca_parse_prep(fake, fake2, 1, 512, 2, 0, 1, None), who)          # reverse
    expect(lib.ca_parse_prep(fake, fake2, 1, 512, 1, 0, 7, None), who)          # dtype
    expect(lib.ca_parse_prep(fake, odd, 1, 512, 1, 0, 1, None), who)            # alignment
    expect(lib.ca_parse_prep(fake, fake2, 200, 512, 1, 0, 1, None), who)        # out of 3.3 GB

    who = "ca_conv3x3_reflect"

    def conv(x=fake, wt=fake, bias=fake, res=None, y=fake2, n=1, h=8, w=8, cin=64, cout=64, stride=1, up2=0, leaky=0, f32=0, rings=0, dt=1):
        return lib.ca_conv3x3_reflect(x, wt, bias, res, y, n, h, w, cin, cout, stride, up2, leaky, f32, rings, dt, None)

    for kw in (dict(x=None), dict(wt=None), dict(bias=None), dict(y=None), dict(cin=48), dict(cin=3), dict(cout=19), dict(cout=512), dict(stride=3), dict(stride=0),
               dict(stride=2, up2=1), dict(up2=2), dict(h=1), dict(w=1), dict(leaky=2), dict(f32=2), dict(rings=8), dict(rings=4), dict(dt=3), dict(x=odd),
               dict(bias=C.c_void_p(0x1002)), dict(y=fake), dict(res=fake2), dict(n=64, h=1024, w=1024, cin=256)):
        expect(conv(**kw), who)

    who = "ca_parse_mask"
    expect(lib.ca_parse_mask(None, fake, fake, fake2, 1, 512, 512, 64, 19, 0, 1, None), who)
    expect(lib.ca_parse_mask(fake, fake, fake, None, 1, 512, 512, 64, 19, 0, 1, None), who)
    expect(lib.ca_parse_mask(fake, fake, fake, fake2, 1, 512, 512, 48, 19, 0, 1, None), who)      # cin
    expect(lib.ca_parse_mask(fake, fake, fake, fake2, 1, 512, 512, 64, 20, 0, 1, None), who)      # classes
    expect(lib.ca_parse_mask(fake, fake, fake, fake2, 1, 512, 512, 64, 19, 2, 1, None), who)      # ring
    expect(lib.ca_parse_mask(fake, fake, fake, fake2, 1, 512, 512, 64, 19, 0, 0, None), who)      # dtype
    expect(lib.ca_parse_mask(odd, fake, fake, fake2, 1, 512, 512, 64, 19, 0, 1, None), who)

    who = "ca_parse_labels"
    expect(lib.ca_parse_labels(None, fake, None, 16, 32, 19, None), who)
    expect(lib.ca_parse_labels(fake, None, None, 16, 32, 19, None), who)
    expect(lib.ca_parse_labels(fake, fake2, None, 0, 32, 19, None), who)
    expect(lib.ca_parse_labels(fake, fake2, None, 16, 18, 19, None), who)       # fewer columns than classes
    expect(lib.ca_parse_labels(fake, fake2, None, 16, 32, 5, None), who)

    who = "ca_ring_fill"
    expect(lib.ca_ring_fill(None, 1, 8, 8, 64, 0, 1, None), who)
    expect(lib.ca_ring_fill(fake, 1, 8, 8, 60, 0, 1, None), who)                # channels
    expect(lib.ca_ring_fill(fake, 1, 8, 8, 64, 2, 1, None), who)                # mode
    expect(lib.ca_ring_fill(fake, 1, 1, 8, 64, 0, 1, None), who)                # one row cannot reflect
    expect(lib.ca_ring_fill(fake, 1, 8, 8, 64, 0, 9, None), who)
    expect(lib.ca_ring_fill(odd, 1, 8, 8, 64, 0, 1, None), who)

    who = "ca_mask_blur"
    expect(lib.ca_mask_blur(None, fake, fake, fake2, 1, 512, 51, None), who)
    expect(lib.ca_mask_blur(fake, None, fake, fake2, 1, 512, 51, None), who)
    expect(lib.ca_mask_blur(fake, fake, fake, fake2, 1, 256, 51, None), who)    # a mask that is not 512 x 512
    expect(lib.ca_mask_blur(fake, fake, fake, fake2, 1, 513, 51, None), who)
    expect(lib.ca_mask_blur(fake, fake, fake, fake2, 1, 512, 101, None), who)   # the half table is wanted
    expect(lib.ca_mask_blur(fake, fake, fake, fake2, 0, 512, 51, None), who)
    expect(lib.ca_mask_blur(fake, fake, fake2, fake2, 1, 512, 51, None), who)   # workspace is out
    expect(lib.ca_mask_blur(fake, odd, fake, fake2, 1, 512, 51, None), who)

    who = "ca_face_paste"

    def paste(bg=fake, res=fake, m=fake, inv=fake, cnt=fake, out=fake2, n=1, h=64, w=96, mf=2, up=1.0):
        return lib.ca_face_paste(bg, res, m, inv, cnt, out, n, h, w, mf, C.c_double(up), None)

    for kw in (dict(bg=None), dict(res=None), dict(m=None), dict(inv=None), dict(cnt=None), dict(out=None), dict(n=0), dict(h=0), dict(w=40000), dict(mf=0), dict(mf=65),
               dict(up=0.0), dict(up=-1.0), dict(m=odd), dict(inv=odd), dict(cnt=C.c_void_p(0x1002)), dict(n=4096, mf=64)):
        expect(paste(**kw), who)


# ---- 2. the state dict ------------------------------------------------------------------------------------------------------------------------
def test_key_table_matches_the_specification_at_both_geometries():
    fp = _fp()
    assert fp.parsenet_key_shapes(fp.PARSENET) == P.key_shapes(**P.FULL)
    assert fp.parsenet_key_shapes(fp.Geometry(**CS.SMALL)) == P.key_shapes(**CS.SMALL)
    names = [b[0] for b in fp.blocks_of(fp.PARSENET)]
    assert names[:4] == [f"encoder.{i}" for i in range(1, 5)] and names[4:14] == [f"body.{i}" for i in range(10)] and names[14:] == [f"decoder.{i}" for i in range(4)]
    assert [(b[1], b[2]) for b in fp.blocks_of(fp.PARSENET) if b[3] != "none"] == [(64, 128), (128, 256), (256, 256), (256, 256), (256, 256), (256, 256), (256, 128), (128, 64)]
    assert tuple(fp.MASK_COLORMAP) == tuple(int(v) for v in P.MASK_COLORMAP)


def test_state_dict_check_names_the_tensor():
    fp = _fp()
    geo = fp.Geometry(**CS.SMALL)
    sd = CS.small_sd()
    fp.check_state_dict(sd, geo)
    with_img = dict(sd)
    with_img["out_img_conv.conv2d.weight"], with_img["out_img_conv.conv2d.bias"] = torch.zeros(3, 32, 3, 3), torch.zeros(3)
    with_img["body.0.conv1.norm.norm.num_batches_tracked"] = torch.tensor(0)
    fp.check_state_dict(with_img, geo)                              # accepted and ignored
    assert "out_img" not in str(fp.pack_network(with_img, geo, torch.float16).keys())
    missing = {k: v for k, v in sd.items() if k != "decoder.1.conv2.norm.norm.running_var"}
    with pytest.raises(KeyError, match="decoder.1.conv2.norm.norm.running_var"):
        fp.check_state_dict(missing, geo)
    with pytest.raises(ValueError, match="surplus.weight"):
        fp.check_state_dict({**sd, "surplus.weight": torch.zeros(1)}, geo)
    with pytest.raises(ValueError, match="encoder.1.shortcut_func.conv2d.weight"):
        fp.check_state_dict({**sd, "encoder.1.shortcut_func.conv2d.weight": torch.zeros(64, 32, 1, 1)}, geo)
    with pytest.raises(KeyError):
        fp.FacePaster(missing, geometry=geo)
    with pytest.raises(ValueError):
        fp.FacePaster(sd, geometry=fp.Geometry(96, 32, 2, (32, 64)))
    with pytest.raises(TypeError):
        fp.FacePaster(sd, geometry=geo, dtype=torch.float32)


def test_from_pretrained_reads_a_local_file_or_directory(tmp_path):
    fp = _fp()
    torch.save(CS.small_sd(), tmp_path / fp.WEIGHTS_NAME)
    for path in (tmp_path, tmp_path / fp.WEIGHTS_NAME):
        p = fp.FacePaster.from_pretrained(path, geometry=fp.Geometry(**CS.SMALL))
        assert p.geometry.in_size == 128
    with pytest.raises(FileNotFoundError):
        fp.FacePaster.from_pretrained(tmp_path / "absent")


def test_batchnorm_fold_equals_the_unfused_network():
    """The folded fp32 weights (what the device packs from) through plain reflected convolutions against the specification's Conv + BatchNorm."""
    import torch.nn.functional as F
    fp = _fp()
    geo = fp.Geometry(**CS.SMALL)
    sd = CS.small_sd()
    faces = CS.small_faces()

    def conv(x, name, stride=1, up=False, leaky=False):
        w, b = fp.fold_bn(sd, name)
        if up:
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        y = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w, b, stride)
        return F.leaky_relu(y, 0.2) if leaky else y

    with torch.no_grad():
        x = conv(P.preprocess(faces), "encoder.0")
        feat = None
        for name, cin, cout, scale in fp.blocks_of(geo):
            if scale == "none" and feat is None:
                feat = x
            idn = conv(x, name + ".shortcut_func", 2 if scale == "down" else 1, scale == "up") if fp.has_shortcut(cin, cout, scale) else x
            y = conv(x, name + ".conv1", 1, scale == "up", True)
            x = idn + conv(y, name + ".conv2", 2 if scale == "down" else 1)
            if name == f"body.{geo.res_depth - 1}":
                x = feat + x
        got = conv(x, "out_mask_conv")
    want = CS.small_logits()
    assert got.shape == want.shape == (3, 19, 128, 128)
    assert ((got - want).abs().max() / want.abs().max()).item() < 1e-5


def test_packing_pads_the_first_and_the_last_layer():
    fp = _fp()
    geo = fp.Geometry(**CS.SMALL)
    host = fp.pack_network(CS.small_sd(), geo, torch.float16)
    w0, b0 = host["in"]
    assert tuple(w0.shape) == (32, 3, 3, 32) and w0.dtype == torch.float16 and (w0[..., 3:] == 0).all() and b0.dtype == torch.float32
    wm, bm = host["mask"]
    assert tuple(wm.shape) == (32, 3, 3, 32) and (wm[19:] == 0).all() and (bm[19:] == 0).all() and bm[:19].abs().min() > 0
    assert len(host["blocks"]) == 6 and [("shortcut" in b) for b in host["blocks"]] == [True, True, False, False, True, True]
    assert fp._bytes_per_face_pixel(fp.PARSENET) == 256 and fp._bytes_per_face_pixel(geo) == 128


# ---- 3. the specification's own properties ---------------------------------------------------------------------------------------------------
def test_blur_of_a_constant_mask_is_the_constant():
    k = P.gaussian_taps()
    assert len(k) == 101 and abs(k.sum() - 1) < 1e-15 and np.array_equal(k, k[::-1]) and np.array_equal(P.half_taps(), _fp().gaussian_half_taps())
    b = P.gaussian_blur(P.gaussian_blur(np.full((512, 512), 255.0)))
    assert np.abs(b - 255.0).max() / 255.0 < 1e-12
    s = P.soft_mask(np.full((512, 512), 255, np.uint8))
    assert (s[:10] == 0).all() and (s[-10:] == 0).all() and (s[:, :10] == 0).all() and (s[:, -10:] == 0).all() and np.abs(s[10:-10, 10:-10] - 1).max() < 1e-12


def test_blur_equals_scipy_correlate1d_mirror():
    from scipy.ndimage import correlate1d
    a = CS.blur_masks()[0].astype(np.float64)
    k = P.gaussian_taps()
    assert np.array_equal(k[50:], FP.gaussian_half_taps())          # the table the device is handed
    for axis in (-1, -2):
        ref, got = correlate1d(a, k, axis=axis, mode="mirror"), P.blur_axis(a, axis)
        assert np.abs(ref - got).max() / np.abs(ref).max() < 1e-12
    ref2 = correlate1d(correlate1d(a, k, axis=-1, mode="mirror"), k, axis=-2, mode="mirror")
    assert np.abs(ref2 - P.gaussian_blur(a)).max() / np.abs(ref2).max() < 1e-12


def test_identity_paste_reproduces_the_face_inside_the_border():
    assert FP.FACE_SIZE == P.FACE_SIZE == 512
    rng = np.random.default_rng(5)
    face = rng.integers(0, 256, (512, 512, 3), dtype=np.uint8)
    bg = rng.integers(0, 256, (512, 512, 3), dtype=np.uint8)
    soft = P.soft_mask(np.full((512, 512), 255, np.uint8))
    soft = (soft > 0.5).astype(np.float64)      # exactly 1 inside the zeroed border, 0 on it
    out = P.paste(bg, face[None], soft[None], np.array([[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]]), 1)
    assert np.array_equal(out[10:-10, 10:-10], face[10:-10, 10:-10])
    edge = np.ones((512, 512), bool)
    edge[10:-10, 10:-10] = False
    assert np.array_equal(out[edge], bg[edge])
    assert np.array_equal(P.paste(bg, face[:0], soft[:0], np.zeros((0, 2, 3)), 1), bg)
    # the warps alone: identity is the image; the double path agrees with the byte path on bytes
    eye = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    assert np.array_equal(P.warp_u8(face, eye, 512, 512), face)
    assert np.array_equal(P.warp_f64(face[..., 0].astype(np.float64), eye, 512, 512), face[..., 0].astype(np.float64))


def c_size() -> int:
    return CS.planted_soft_masks().shape[1]


def test_planted_paste_cases_do_what_their_names_say():
    """The GPU paste test's cases, on the specification alone: overlapping faces depend on the order, faces hang over every edge, the
    count-0 frame is its background, the offset applies once at f = 2."""
    assert FP.FACE_SIZE == c_size() == 512
    for f in (1, 2):
        c = CS.paste_case((64, 96), f)
        outs = [P.paste(c["background"][i], c["restored"][i * 3:i * 3 + c["count"][i]], c["masks"][i * 3:i * 3 + c["count"][i]],
                        c["inverse"][i, :c["count"][i]], f) for i in range(3)]
        assert list(c["count"]) == [0, 1, 3]
        assert np.array_equal(outs[0], c["background"][0])
        assert (outs[1] != c["background"][1]).any() and (outs[2] != c["background"][2]).any()
        order = [1, 0, 2]
        swapped = P.paste(c["background"][2], c["restored"][6:9][order], c["masks"][6:9][order], c["inverse"][2][order], f)
        assert (swapped != outs[2]).any()                                  # two faces overlap: the order shows
        h, w = outs[2].shape[:2]
        changed = (outs[2] != c["background"][2]).any(axis=2)
        assert changed[0].any() and changed[-1].any() and changed[:, 0].any() and changed[:, -1].any()   # a face hangs over each edge
        if f == 2:
            no_offset = c["inverse"][1, :1].copy()
            twice = no_offset.copy()
            twice[:, :, 2] += 1.0
            assert (P.paste(c["background"][1], c["restored"][3:4], c["masks"][3:4], twice, 1) == outs[1]).all()


# ---- 4. the plumbing ---------------------------------------------------------------------------------------------------------------------------
class StubPaster:
    def __init__(self):
        self.calls = []

    def paste(self, background, restored, inverse_affine, count, upscale_factor=1, bgr=False, out=None, frame_size=None):
        self.calls.append((tuple(background.shape), tuple(restored.shape), tuple(inverse_affine.shape), count.tolist(), upscale_factor, bgr, frame_size))
        return torch.full((1, int(frame_size[0] * upscale_factor), int(frame_size[1] * upscale_factor), 3), 7, dtype=torch.uint8)


class StubAligner:
    upscale_factor = 2.0
    max_faces = 4

    def align(self, frames, **kw):
        n = 2
        return {"faces": torch.arange(n, dtype=torch.uint8).view(n, 1, 1, 1).expand(n, 512, 512, 3).contiguous(), "count": torch.tensor([n], dtype=torch.int32),
                "dets": torch.zeros(1, 4, 15), "affine": torch.zeros(1, 4, 2, 3, dtype=torch.float64),
                "inverse_affine": torch.arange(24, dtype=torch.float64).view(1, 4, 2, 3), "overflow": torch.zeros(1, dtype=torch.int32)}


def test_face_helper_keeps_its_message_without_a_paster_and_forwards_with_one():
    from controlanimate_amd.face_align import FaceHelper
    from controlanimate_amd.gfpgan import FaceRestorer
    frame = np.zeros((64, 96, 3), np.uint8)
    plain = FaceHelper(StubAligner())
    with pytest.raises(NotImplementedError) as e:
        plain.paste_faces_to_input_image()
    assert str(e.value) == "paste-back (ParseNet mask, inverse warp, blend) is not built yet"
    stub = StubPaster()
    helper = FaceHelper(StubAligner(), bgr=True, paster=stub)

    class Restorer:
        enhance = FaceRestorer.enhance

        def restore_aligned(self, faces):
            return torch.from_numpy(np.stack(faces)) + 1

    cropped, restored, img = Restorer().enhance(frame, has_aligned=False, paste_back=True, face_helper=helper)
    assert len(cropped) == len(restored) == 2 and img.shape == (128, 192, 3) and (img == 7).all()
    (bg, res, inv, count, f, bgr, size), = stub.calls
    assert bg == (1, 64, 96, 3) and res == (2, 512, 512, 3) and inv == (1, 2, 2, 3) and count == [2] and f == 2.0 and bgr is True and size == (64, 96)
    with pytest.raises(NotImplementedError):
        helper.paste_faces_to_input_image(save_path="x.png")
    up = np.zeros((128, 192, 3), np.uint8)
    helper.paste_faces_to_input_image(upsample_img=up)
    assert stub.calls[-1][0] == (1, 128, 192, 3)
    fresh = FaceHelper(StubAligner(), paster=stub)
    with pytest.raises(ValueError):
        fresh.paste_faces_to_input_image()


def test_face_enhancer_is_exported_and_checks_the_upscale():
    from controlanimate_amd import gfpgan
    fp = _fp()
    assert gfpgan.FaceEnhancer is fp.FaceEnhancer and gfpgan.FacePaster is fp.FacePaster
    fe = fp.FaceEnhancer(StubAligner(), None, None)
    with pytest.raises(ValueError, match="upscale_factor"):
        fe.enhance_frames([np.zeros((64, 96, 3), np.uint8)], upscale=1)
    assert callable(fe.as_face_enhancer())


# ---- 5. no CPU fallback ------------------------------------------------------------------------------------------------------------------------
def test_no_cpu_fallback_when_the_library_is_missing(monkeypatch):
    from controlanimate_amd import _capi
    fp = _fp()
    p = fp.FacePaster(CS.small_sd(), geometry=fp.Geometry(**CS.SMALL))
    monkeypatch.setattr(_capi, "_lib", None)
    monkeypatch.setattr(_capi, "LIB_PATH", "/nonexistent/libcontrolanimate_hip.so")
    with pytest.raises(_capi.CAHipUnavailable):
        p.labels(CS.small_faces())
    full = fp.FacePaster.__new__(fp.FacePaster)
    full.geometry, full.device = fp.PARSENET, None
    with pytest.raises(_capi.CAHipUnavailable):
        full.blur(torch.zeros((1, 512, 512), dtype=torch.uint8))
    with pytest.raises(TypeError):
        p.labels(torch.zeros((1, 128, 128, 3)))
    with pytest.raises(ValueError):
        p.labels(torch.zeros((1, 64, 64, 3), dtype=torch.uint8))


# ---- 6. the label test's margin condition ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_margin_condition_of_the_gpu_label_test_holds_on_the_specification(dtype):
    """GPU item: labels must agree wherever the specification's top-two margin exceeds four times the device's maximum logit error, and at
    most 5 % of the pixels may fall below that margin.  Here with the error bound of tests/facepaste_cases.py (LOGIT_ERR), which the GPU
    test holds its own measurement to."""
    seed, cb = CS.LABEL_CASE[dtype]
    FP.check_state_dict(CS.small_sd(seed, cb), FP.Geometry(**CS.SMALL))      # the fixture is one the device accepts
    lg = CS.small_logits(False, seed, cb)
    margin = P.top2_margin(lg)
    left_out = float((margin <= 4 * CS.LOGIT_ERR[dtype]).mean())
    labels = P.labels_of(lg)
    share = np.bincount(labels.ravel(), minlength=19) / labels.size
    print(f"{dtype}: {left_out:.2%} of the pixels within 4 x {CS.LOGIT_ERR[dtype]} of a tie; {int((share > 0.01).sum())} classes above 1 %, the largest {share.max():.0%}")
    assert left_out <= 0.05
    assert (share > 0.01).sum() >= 2 and share.max() < 0.99                     # the labels are not one constant
    if dtype == torch.float16:                                                  # the other tests' fixture: many classes, a mask with both values
        assert (share > 0.01).sum() >= 8 and share.max() < 0.5 and 0.05 < (P.MASK_COLORMAP[labels] == 255).mean() < 0.95
