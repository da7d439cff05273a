"""CPU: the specification of the HED annotator (tests/hed_ref.py: the 37 tensors of the network, the INTER_LINEAR restatement),
HedAnnotator's loading and input checks, and the argument checks of the entry points added to ABI v16 for it (no launch, no GPU)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hed_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ca_hed_prep", "ca_hed_pool_side", "ca_hed_fuse"]


@pytest.fixture(scope="module")
def capi():
    from controlanimate_amd import _build, _capi
    _build.build(verbose=False)
    return _capi


@pytest.fixture(scope="module")
def sd():
    return hed_ref.hed_state_dict(seed=3)


# ---- the specification -------------------------------------------------------------------------------------------------------------
def test_reference_net_has_the_37_tensors():
    want = {"norm": (1, 3, 1, 1)}
    for b, (cin, cout, layers) in enumerate(((3, 64, 2), (64, 128, 2), (128, 256, 3), (256, 512, 3), (512, 512, 3)), start=1):
        for i in range(layers):
            want[f"block{b}.convs.{i}.weight"] = (cout, cin if i == 0 else cout, 3, 3)
            want[f"block{b}.convs.{i}.bias"] = (cout,)
        want[f"block{b}.projection.weight"] = (1, cout, 1, 1)
        want[f"block{b}.projection.bias"] = (1,)
    assert len(want) == 37
    got = {k: tuple(v.shape) for k, v in hed_ref.ControlNetHED().state_dict().items()}
    assert got == want
    assert hed_ref.hed_key_shapes() == want
    assert {k: tuple(v.shape) for k, v in hed_ref.hed_state_dict().items()} == want
    from controlanimate_amd.hed import hed_key_shapes
    assert hed_key_shapes() == want


def test_reference_net_side_maps_have_the_five_resolutions(sd):
    frames = np.random.default_rng(0).integers(0, 256, (2, 32, 48, 3), dtype=np.uint8)
    sides = hed_ref.side_maps_ref(sd, frames)
    assert [tuple(s.shape) for s in sides] == [(2, 32 >> k, 48 >> k) for k in range(5)]


def test_bilinear_is_the_identity_at_scale_1():
    a = np.random.default_rng(1).standard_normal((7, 13)).astype(np.float32)
    assert np.array_equal(hed_ref.resize_linear_f32(a, 7, 13), a)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_bilinear_keeps_a_constant_map_constant(k):
    a = np.full((3, 5), np.float32(0.3) * 7, np.float32)
    out = hed_ref.resize_linear_f32(a, 3 << k, 5 << k)
    assert out.shape == (3 << k, 5 << k) and np.array_equal(out, np.full_like(out, a[0, 0]))


def test_bilinear_reproduces_a_linear_ramp_in_the_interior_at_x2():
    h, w = 6, 9
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    a = (2 * xx + 3 * yy + 1).astype(np.float32)  # small integers and quarter steps: every product and sum is exact
    out = hed_ref.resize_linear_f32(a, 2 * h, 2 * w)
    dy, dx = np.mgrid[0:2 * h, 0:2 * w].astype(np.float64)
    want = 2 * ((dx + 0.5) / 2 - 0.5) + 3 * ((dy + 0.5) / 2 - 0.5) + 1  # the ramp at the source coordinate of each destination pixel
    assert np.array_equal(out[1:-1, 1:-1].astype(np.float64), want[1:-1, 1:-1])
    assert out[0, 0] == a[0, 0] and out[-1, -1] == a[-1, -1]  # outside the first / last sample the border replicates


def test_fuse_ref_quantises_by_truncation():
    z = [np.zeros((16 >> k, 16 >> k), np.float32) for k in range(5)]
    edge, mean, scaled = hed_ref.fuse_ref(z, 16, 16)
    assert np.all(mean == 0) and np.all(scaled == 127.5) and np.all(edge == 127)  # sigmoid(0) * 255 = 127.5 -> 127
    big = [np.full_like(s, 40.0) for s in z]
    assert np.all(hed_ref.fuse_ref(big, 16, 16)[0] == 255)                         # 1 + exp(-40) is 1 in float64
    assert np.all(hed_ref.fuse_ref([-s for s in big], 16, 16)[0] == 0)


def test_detector_identity_sizes_and_scope(sd):
    assert hed_ref.resize_image_size(512, 768, 512)[:2] == (512, 768)
    assert hed_ref.resize_image_size(576, 768, 512)[:2] == (512, 704)
    assert hed_ref.resize_image_size(64, 128, 64) == (64, 128, "area")
    img = np.random.default_rng(2).integers(0, 256, (64, 128, 3), dtype=np.uint8)
    out = hed_ref.hed_detect(sd, img, 64, 64)
    assert out.shape == (64, 128, 3) and out.dtype == np.uint8 and np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 0], out[..., 2])
    with pytest.raises(NotImplementedError):
        hed_ref.hed_detect(sd, img, 128, 128)


# ---- HedAnnotator: loading ---------------------------------------------------------------------------------------------------------
def test_from_pretrained_round_trips_a_saved_state_dict(sd, tmp_path):
    import torch
    from controlanimate_amd.annotators import HedAnnotator
    f = tmp_path / "ControlNetHED.pth"
    torch.save(hed_ref.hed_net(sd).state_dict(), f)
    for src in (f, str(f), tmp_path):  # the file, or the directory that holds it
        ann = HedAnnotator.from_pretrained(src)
        assert ann.dtype == torch.float16 and ann.detect_resolution == 512 and ann.image_resolution == 512
        assert torch.equal(ann._host["norm"], sd["norm"].reshape(3))
        convs, pw, pb = ann._host["blocks"][0]
        w0, b0 = convs[0]
        assert tuple(w0.shape) == (64, 3, 3, 8) and w0.dtype == torch.float16                      # [cout][3][3][cin], cin zero-padded to 8
        assert torch.equal(w0[..., :3], sd["block1.convs.0.weight"].permute(0, 2, 3, 1).half()) and not w0[..., 3:].any()
        assert torch.equal(b0, sd["block1.convs.0.bias"]) and b0.dtype == torch.float32
        w1, _ = ann._host["blocks"][2][0][1]
        assert tuple(w1.shape) == (256, 3, 3, 256) and torch.equal(w1, sd["block3.convs.1.weight"].permute(0, 2, 3, 1).half())
        assert torch.equal(pw, sd["block1.projection.weight"].reshape(64)) and torch.equal(pb, sd["block1.projection.bias"])
        assert [len(b[0]) for b in ann._host["blocks"]] == [2, 2, 3, 3, 3]
    bf = HedAnnotator.from_pretrained(f, dtype=torch.bfloat16, detect_resolution=64, image_resolution=64)
    assert bf._host["blocks"][4][0][2][0].dtype == torch.bfloat16 and bf.detect_resolution == 64
    with pytest.raises(FileNotFoundError):
        HedAnnotator.from_pretrained(tmp_path / "nowhere")
    with pytest.raises(TypeError):
        HedAnnotator(sd, dtype=torch.float32)


def test_state_dict_checks_name_the_offender(sd):
    import torch
    from controlanimate_amd.annotators import HedAnnotator
    missing = {k: v for k, v in sd.items() if k != "block4.convs.2.bias"}
    with pytest.raises(KeyError, match=re.escape("block4.convs.2.bias")):
        HedAnnotator(missing)
    wrong = dict(sd)
    wrong["block2.projection.weight"] = torch.zeros(1, 64, 1, 1)
    with pytest.raises(ValueError, match=re.escape("block2.projection.weight")):
        HedAnnotator(wrong)
    wrong = dict(sd)
    wrong["norm"] = torch.zeros(3)
    with pytest.raises(ValueError, match="norm"):
        HedAnnotator(wrong)
    extra = dict(sd)
    extra["block6.convs.0.weight"] = torch.zeros(1)
    with pytest.raises(ValueError, match=re.escape("block6.convs.0.weight")):
        HedAnnotator(extra)


# ---- HedAnnotator: input checks before the device -------------------------------------------------------------------------------
def test_annotator_checks_types_sizes_and_scope_before_the_device(capi, sd, monkeypatch):
    import torch
    from PIL import Image
    from controlanimate_amd.annotators import HedAnnotator
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "LIB_PATH", "/nonexistent/libcontrolanimate_hip.so")   # touching the device would raise CAHipUnavailable
    ann = HedAnnotator(sd, detect_resolution=64, image_resolution=64)
    u8, f32 = np.zeros((64, 128, 3), np.uint8), np.zeros((64, 128, 3), np.float32)
    for call in (ann, lambda x: ann.edges([x]), lambda x: ann.annotate_batch([x]), lambda x: ann.side_maps([x])):
        with pytest.raises(TypeError):
            call(f32)
    with pytest.raises(TypeError):
        ann.edges(torch.zeros((1, 64, 128, 3), dtype=torch.float32))
    with pytest.raises(ValueError):
        ann.edges([u8, np.zeros((64, 64, 3), np.uint8)])
    with pytest.raises(ValueError):
        ann.annotate_batch([np.zeros((64, 128, 4), np.uint8)])
    with pytest.raises(ValueError, match="RGBA"):
        ann.annotate_batch([Image.new("RGBA", (128, 64))])
    with pytest.raises(ValueError):
        ann.annotate_batch([u8], rep=3)
    with pytest.raises(TypeError):
        ann.annotate_batch([u8], dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        ann.annotate_batch([u8], out=torch.zeros((1, 3, 64, 128), dtype=torch.float64))
    with pytest.raises(ValueError):
        ann.edges([])
    # sizes for which a resize_image call of the detector is not the identity
    std = HedAnnotator(sd)
    with pytest.raises(NotImplementedError, match="576 x 768"):
        std.edges([np.zeros((576, 768, 3), np.uint8)])
    with pytest.raises(NotImplementedError):
        std.annotate_batch(torch.zeros((2, 576, 768, 3), dtype=torch.uint8))
    with pytest.raises(NotImplementedError):
        std([np.zeros((64, 128, 3), np.uint8)][0])                                      # detect_resolution != the shorter side
    with pytest.raises(NotImplementedError):
        HedAnnotator(sd, detect_resolution=64, image_resolution=128).edges([u8])         # image_resolution != detect_resolution
    with pytest.raises(NotImplementedError):
        HedAnnotator(sd, detect_resolution=72, image_resolution=72).edges([np.zeros((72, 128, 3), np.uint8)])   # 72 % 64
    # in scope (mode L and RGB alike): the device comes next, and there is none
    for ok in (u8, Image.new("RGB", (128, 64)), Image.new("L", (128, 64))):
        with pytest.raises(capi.CAHipUnavailable):
            ann.edges([ok])
    with pytest.raises(capi.CAHipUnavailable):
        ann(u8)
    with pytest.raises(capi.CAHipUnavailable):
        std.annotate_batch([np.zeros((512, 768, 3), np.uint8)])


def test_annotator_needs_a_gpu(capi, sd, monkeypatch):
    import torch
    from controlanimate_amd.annotators import HedAnnotator
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    ann = HedAnnotator(sd, detect_resolution=64, image_resolution=64)
    with pytest.raises(capi.CAHipUnavailable):
        ann.annotate_batch([np.zeros((64, 64, 3), np.uint8)])
    with pytest.raises(capi.CAHipUnavailable):
        HedAnnotator(sd, "cuda", detect_resolution=64, image_resolution=64).edges(torch.zeros((1, 64, 64, 3), dtype=torch.uint8))


def test_chunking_keeps_the_largest_activation_addressable(sd):
    from controlanimate_amd.annotators import HedAnnotator
    ann = HedAnnotator(sd)
    per_frame = 512 * 768 * 64 * 2
    assert ann.chunk_frames(512, 768) == (0x7FFFFF00 - 1) // per_frame == 42      # a 16-frame window is one pass
    assert ann.chunk_frames(512, 768) * per_frame < 0x7FFFFF00
    ann.max_activation_bytes = 3 * per_frame + 5
    assert ann.chunk_frames(512, 768) == 3
    ann.max_activation_bytes = per_frame - 1
    with pytest.raises(ValueError):
        ann.chunk_frames(512, 768)


# ---- the entry points --------------------------------------------------------------------------------------------------------------
def test_abi_is_still_16_and_header_binding_library_agree(capi):
    assert capi.ABI_VERSION == 16 and capi.CA_ACT_RELU == 4
    lib = capi.lib()
    assert lib.ca_abi_version() == 16
    header = open(os.path.join(ROOT, "include", "controlanimate_hip.h")).read()
    assert re.search(r"#define\s+CA_ABI_VERSION\s+16\b", header) and re.search(r"#define\s+CA_ACT_RELU\s+4\b", header)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert name in capi.SYMBOLS and getattr(lib, name) is not None
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert decl, f"{name} is not declared in the header"
        assert len([a for a in decl.group(1).split(",") if a.strip()]) == len(capi.SYMBOLS[name][1]), name   # one binding type per C parameter
    from controlanimate_amd import kernels as K
    assert K.ACT_RELU == 4 and callable(K.hed_prep) and callable(K.hed_pool_side) and callable(K.hed_fuse)
    from controlanimate_amd import _build
    assert "ca_hed.hip" in _build.SOURCES


def test_entry_points_reject_bad_arguments_without_a_launch(capi):
    lib = capi.lib()
    fake, odd = C.c_void_p(0x1000), C.c_void_p(0x1004)  # never dereferenced: validation fails first
    F16, BF16, F32 = capi.CA_F16, capi.CA_BF16, capi.CA_F32

    def expect(rc, who):
        assert rc < 0 and who.encode() in lib.ca_last_error(), (rc, lib.ca_last_error())

    pr = "ca_hed_prep"
    expect(lib.ca_hed_prep(None, fake, fake, 2, 8, 8, F16, None), pr)
    expect(lib.ca_hed_prep(fake, None, fake, 2, 8, 8, F16, None), pr)
    expect(lib.ca_hed_prep(fake, fake, None, 2, 8, 8, F16, None), pr)
    expect(lib.ca_hed_prep(fake, fake, fake, 0, 8, 8, F16, None), pr)
    expect(lib.ca_hed_prep(fake, fake, fake, 2, 0, 8, F16, None), pr)
    expect(lib.ca_hed_prep(fake, fake, fake, 2, 8, -1, F16, None), pr)
    expect(lib.ca_hed_prep(fake, fake, fake, 2, 8, 8, F32, None), pr)                    # the activations are fp16 / bf16
    expect(lib.ca_hed_prep(fake, fake, odd, 2, 8, 8, BF16, None), pr)                    # 16-byte stores
    expect(lib.ca_hed_prep(fake, fake, fake, 1 << 15, 1 << 8, 1 << 8, F16, None), pr)    # images * h * w = 2^31

    ps = "ca_hed_pool_side"
    expect(lib.ca_hed_pool_side(None, fake, fake, fake, fake, 2, 8, 8, 64, F16, None), ps)
    expect(lib.ca_hed_pool_side(fake, None, fake, fake, fake, 2, 8, 8, 64, F16, None), ps)
    expect(lib.ca_hed_pool_side(fake, fake, None, fake, fake, 2, 8, 8, 64, F16, None), ps)
    expect(lib.ca_hed_pool_side(fake, fake, fake, None, None, 2, 8, 8, 64, F16, None), ps)   # the side map is always written
    expect(lib.ca_hed_pool_side(fake, fake, fake, fake, fake, 2, 7, 8, 64, F16, None), ps)   # odd h
    expect(lib.ca_hed_pool_side(fake, fake, fake, fake, None, 2, 8, 9, 64, F16, None), ps)   # odd w, also without the pool
    expect(lib.ca_hed_pool_side(fake, fake, fake, fake, fake, 2, 8, 8, 68, F16, None), ps)   # C % 8
    expect(lib.ca_hed_pool_side(fake, fake, fake, fake, fake, 2, 8, 8, 56, F16, None), ps)   # C < 64
    expect(lib.ca_hed_pool_side(fake, fake, fake, fake, fake, 2, 8, 8, 520, F16, None), ps)  # C > 512
    expect(lib.ca_hed_pool_side(fake, fake, fake, fake, fake, 0, 8, 8, 64, F16, None), ps)
    expect(lib.ca_hed_pool_side(fake, fake, fake, fake, fake, 2, 8, 8, 64, F32, None), ps)
    expect(lib.ca_hed_pool_side(odd, fake, fake, fake, fake, 2, 8, 8, 64, F16, None), ps)
    expect(lib.ca_hed_pool_side(fake, fake, fake, odd, fake, 2, 8, 8, 64, F16, None), ps)    # 8-byte stores to the side map
    expect(lib.ca_hed_pool_side(fake, fake, fake, fake, odd, 2, 8, 8, 64, BF16, None), ps)
    expect(lib.ca_hed_pool_side(fake, fake, fake, fake, fake, 1 << 15, 1 << 8, 1 << 8, 64, F16, None), ps)

    fu = "ca_hed_fuse"
    s = [fake] * 5
    expect(lib.ca_hed_fuse(*s, 2, 16, 16, None, None, 1, F32, None), fu)                  # neither output
    for k in range(5):
        expect(lib.ca_hed_fuse(*[None if i == k else fake for i in range(5)], 2, 16, 16, fake, None, 1, F32, None), fu)
    expect(lib.ca_hed_fuse(*s, 2, 24, 16, fake, None, 1, F32, None), fu)                  # H % 16
    expect(lib.ca_hed_fuse(*s, 2, 16, 40, fake, None, 1, F32, None), fu)                  # W % 16
    expect(lib.ca_hed_fuse(*s, 0, 16, 16, fake, None, 1, F32, None), fu)
    expect(lib.ca_hed_fuse(*s, 2, 0, 16, fake, None, 1, F32, None), fu)
    expect(lib.ca_hed_fuse(*s, 2, 16, 16, fake, fake, 0, F32, None), fu)
    expect(lib.ca_hed_fuse(*s, 2, 16, 16, fake, fake, 3, F16, None), fu)                  # rep is 1 or 2
    expect(lib.ca_hed_fuse(*s, 2, 16, 16, fake, fake, 1, BF16, None), fu)                 # the control tensor is fp32 or fp16
    expect(lib.ca_hed_fuse(*s, 2, 16, 16, fake, fake, 1, 3, None), fu)
    expect(lib.ca_hed_fuse(*s, 2, 16, 16, None, C.c_void_p(0x1008), 1, F32, None), fu)    # four-element stores
    expect(lib.ca_hed_fuse(*s, 2, 16, 16, C.c_void_p(0x1002), None, 1, F32, None), fu)
    expect(lib.ca_hed_fuse(odd, fake, fake, fake, fake, 2, 16, 16, fake, None, 1, F32, None), fu)
    expect(lib.ca_hed_fuse(*s, 1 << 15, 1 << 8, 1 << 8, fake, None, 1, F32, None), fu)


def test_relu_convolutions_keep_the_plan_they_had(capi):
    """CA_ACT_RELU widens no streaming kernel's plan condition: a ReLU convolution gets the plan of the same convolution with SiLU
    (an activation the planner already knew), at the thirteen HED shapes of a 16 x 512 x 768 window."""
    lib = capi.lib()
    fake = C.c_void_p(0x1000)

    def plan(cin, cout, h, w, act):
        a = capi.ConvArgs(x=fake, w=fake, y=fake, bias=fake, images=16, hin=h, win=w, cin1=cin, cout=cout, stride=1, alpha=1.0, post_scale=1.0,
                          act=act, dtype=capi.CA_F16)
        buf = C.create_string_buffer(64)
        assert lib.ca_conv3x3_plan_name(C.byref(a), buf, 64) == 0, lib.ca_last_error()
        return buf.value.decode()

    h, w, names = 512, 768, []
    for b, (cin, cout, layers) in enumerate(hed_ref.HED_BLOCKS):
        for i in range(layers):
            ci = (8 if b == 0 else cin) if i == 0 else cout
            names.append(plan(ci, cout, h, w, capi.CA_ACT_RELU))
            assert names[-1] == plan(ci, cout, h, w, capi.CA_ACT_SILU)
        h, w = h // 2, w // 2
    assert len(names) == 13 and not any(n.startswith(("pq", "ps", "ar", "wres", "wino")) for n in names)
    print("HED convolution plans at 16x512x768:", names)
