"""CPU: the GFPGAN face restorer's host side (controlanimate_amd/gfpgan.py) and its specification (tests/gfpgan_ref.py): the identity
the device path rests on, in float64; the state-dict rules; final_linear's column permutation; the packed style parameters; the input
checks, which come before the device is touched; GFPGANer.enhance's control flow around a caller-supplied face helper; the fixture of
the finish test against its cap; the ABI additions and their argument validation."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gfpgan_ref as R  # noqa: E402
import rrdb_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "controlanimate_hip.h")
SEED = 5


@pytest.fixture(scope="module")
def capi():
    from controlanimate_amd import _build, _capi
    _build.build(verbose=False)
    return _capi


@pytest.fixture(scope="module")
def net16():
    return R.make_net(16, SEED)


# ---- the specification is self-consistent ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("demodulate", [True, False])
@pytest.mark.parametrize("upsample", [False, True])
def test_factored_modulated_convolution_equals_the_published_form(upsample, demodulate, scaled):
    """demod[n, o] * conv(W, s[n, i] * x) with demod from Wsq = sum_k W^2 -- and the form with s scaled by its per-image maximum --
    equal ModulatedConv2d in float64."""
    torch.manual_seed(SEED)
    k = 3 if demodulate else 1
    m = R.ModulatedConv2d(24, 16, k, 32, demodulate=demodulate, sample_mode="upsample" if upsample else None).double()
    with torch.no_grad():
        m.modulation.weight.copy_(torch.randn(24, 32, dtype=torch.float64) * 0.3)
    x, style = torch.randn(3, 24, 6, 10, dtype=torch.float64), torch.randn(3, 32, dtype=torch.float64)
    with torch.no_grad():
        want = m(x, style)
        got = R.factored_modconv(x, m.modulation(style), m.weight[0], demodulate=demodulate, upsample=upsample, scaled=scaled)
    err = ((got - want).abs().max() / want.abs().max()).item()
    print(f"factored form up={upsample} demod={demodulate} scaled={scaled}: largest relative error {err:.2e}")
    assert err < 1e-13


def test_half_resize_is_the_2x2_mean():
    x = torch.randn(2, 5, 6, 10)
    assert torch.equal(R.resize2(x, False), F.avg_pool2d(x, 2))


def test_parameter_count_at_512():
    from controlanimate_amd.gfpgan import gfpgan_key_shapes
    shapes = gfpgan_key_shapes(512)
    assert sum(int(np.prod(s)) for s in shapes.values()) == 84339239
    assert shapes["final_linear.weight"] == (16 * 512, 4096) and shapes["conv_body_first.weight"] == (32, 3, 1, 1)
    assert shapes["stylegan_decoder.style_convs.13.modulated_conv.weight"] == (1, 64, 64, 3, 3)
    assert shapes["condition_scale.6.2.weight"] == (32, 32, 3, 3)


# ---- state-dict rules ---------------------------------------------------------------------------------------------------------------
def test_state_dict_names_and_shapes_round_trip(net16):
    from controlanimate_amd.gfpgan import IGNORED_PREFIXES, GFPGANv1Clean, gfpgan_key_shapes
    sd = net16.state_dict()
    assert any(k.startswith("toRGB.") for k in sd) and any(k.startswith("stylegan_decoder.style_mlp.") for k in sd)
    assert any(k.startswith("stylegan_decoder.noises.") for k in sd)          # the three ignored families are in the published dict
    used = {k: tuple(v.shape) for k, v in sd.items() if not k.startswith(IGNORED_PREFIXES)}
    assert used == gfpgan_key_shapes(16)
    box = GFPGANv1Clean(16).load_state_dict(sd)                               # accepted with the ignored families present
    back = box.state_dict()
    assert set(back) == set(used) and all(torch.equal(back[k], sd[k]) for k in back)
    R.GFPGANv1Clean(16).load_state_dict({**sd, **back})                       # and the published module takes them back


def test_missing_unexpected_and_misshapen_tensors_are_named(net16):
    from controlanimate_amd.gfpgan import GFPGANv1Clean
    sd = dict(net16.state_dict())
    gone = "stylegan_decoder.style_convs.1.modulated_conv.modulation.bias"
    bad = {k: v for k, v in sd.items() if k != gone}
    bad["conv_body_up.0.conv3.weight"] = torch.zeros(1)
    with pytest.raises(KeyError) as e:
        GFPGANv1Clean(16).load_state_dict(bad)
    assert "missing" in str(e.value) and gone in str(e.value) and "unexpected" in str(e.value) and "conv_body_up.0.conv3.weight" in str(e.value)
    sd["final_conv.bias"] = torch.zeros(7)
    with pytest.raises(ValueError) as e:
        GFPGANv1Clean(16).load_state_dict(sd)
    assert "final_conv.bias" in str(e.value)
    with pytest.raises(NotImplementedError):
        GFPGANv1Clean(512, channel_multiplier=1)


def test_weight_file_wrappers_and_missing_file(net16, tmp_path):
    from controlanimate_amd.gfpgan import FaceRestorer
    from controlanimate_amd.local_models import GFPGAN_V13_PATH, load_gfpgan_state_dict
    assert GFPGAN_V13_PATH.endswith("GFPGANv1.3.pth")
    sd = net16.state_dict()
    for wrap in ("params_ema", "params", None):
        p = str(tmp_path / f"{wrap}.pth")
        torch.save({wrap: sd, "other": 1} if wrap else sd, p)
        got = load_gfpgan_state_dict(p)
        assert set(got) == set(sd) and torch.equal(got["final_conv.bias"], sd["final_conv.bias"])
    p = str(tmp_path / "both.pth")
    torch.save({"params": {"x": torch.zeros(1)}, "params_ema": sd}, p)
    assert set(load_gfpgan_state_dict(p)) == set(sd)                           # params_ema before params
    r = FaceRestorer(p, out_size=16)
    assert torch.equal(r.net.params["final_conv.bias"], sd["final_conv.bias"])
    with pytest.raises(FileNotFoundError) as e:
        FaceRestorer(str(tmp_path / "nope.pth"))
    assert "nope.pth" in str(e.value)


# ---- packing --------------------------------------------------------------------------------------------------------------------------
def test_final_linear_nhwc_permutation_reproduces_the_nchw_result():
    from controlanimate_amd.gfpgan import permute_final_linear
    g = torch.Generator().manual_seed(SEED)
    w, feat = torch.randn(40, 256 * 16, generator=g, dtype=torch.float64), torch.randn(3, 256, 4, 4, generator=g, dtype=torch.float64)
    want = feat.reshape(3, -1) @ w.t()                                         # the NCHW flattening, as feat.view(n, -1) upstream
    got = feat.permute(0, 2, 3, 1).reshape(3, -1) @ permute_final_linear(w).t()
    assert torch.equal(got, want) or (got - want).abs().max() < 1e-12
    assert not torch.allclose(feat.permute(0, 2, 3, 1).reshape(3, -1) @ w.t(), want)   # (without it the result is another one)
    with pytest.raises(ValueError):
        permute_final_linear(w[:, :100])


def test_packed_style_parameters_reproduce_modulation_and_demodulation(net16):
    """The flat parameter block and the descriptors of ca_gfp_styles, evaluated as the header states them in float64, give each layer's
    modulation(latent) and, with Wsq, its demodulation."""
    from controlanimate_amd.gfpgan import GFPGANv1Clean
    box = GFPGANv1Clean(16).load_state_dict(net16.state_dict()).prepare("cpu", torch.float16)
    P = box.packed
    params, desc = P["style_params"].double(), P["desc"]
    assert len(desc) == 6 * (2 * 2 + 1 + 3) and box.num_latent == 6 and box.num_layers == 5
    lat = torch.randn(2, box.num_latent, 512, dtype=torch.float64, generator=torch.Generator().manual_seed(SEED))
    dec = net16.stylegan_decoder
    mods = [dec.style_conv1, dec.to_rgb1, dec.style_convs[0], dec.style_convs[1], dec.to_rgbs[0], dec.style_convs[2], dec.style_convs[3], dec.to_rgbs[1]]
    assert [desc[6 * i] for i in range(8)] == [0, 1, 1, 2, 3, 3, 4, 5]          # the latent of each layer, as the decoder's loop takes them
    end = 0
    for i, mod in enumerate(mods):
        li, cin, cout, w_off, wsq_off, out_off = desc[6 * i:6 * i + 6]
        mc = mod.modulated_conv
        assert cin == mc.in_channels and cout == (mc.out_channels if mc.demodulate else 0) and out_off == end
        end = out_off + cin + cout
        s = lat[:, li] @ params[w_off:w_off + 512 * cin].view(512, cin) + params[w_off + 512 * cin:w_off + 513 * cin]
        want = lat[:, li] @ mc.modulation.weight.detach().double().t() + mc.modulation.bias.detach().double()
        assert (s - want).abs().max() < 1e-12
        if cout:
            wsq = params[wsq_off:wsq_off + cin * cout].view(cin, cout)
            w16 = mc.weight[0].detach().half().double()
            demod = torch.rsqrt((s * s) @ wsq + 1e-8)
            want_d = torch.rsqrt((w16[None] * s[:, None, :, None, None]).pow(2).sum([2, 3, 4]) + 1e-8)
            assert ((demod - want_d).abs() / want_d).max() < 2.0 ** -24   # Wsq is stored in fp32 (2^-24 per term); the rsqrt halves it
            assert torch.equal(P["layers"][i]["w"], mc.weight[0].detach().permute(0, 2, 3, 1).half())
    assert end == P["style_stride"]
    assert torch.equal(P["const"], dec.constant_input.weight.detach().permute(0, 2, 3, 1).half())


# ---- FaceRestorer: errors before the device ------------------------------------------------------------------------------------------
class _Touched(Exception):
    pass


@pytest.fixture()
def restorer(net16, monkeypatch):
    from controlanimate_amd.gfpgan import FaceRestorer
    r = FaceRestorer(net16.state_dict(), out_size=16)

    def touched(self=None):
        raise _Touched()
    monkeypatch.setattr(r, "_device", touched)
    return r


def test_type_shape_and_scope_errors_come_before_the_device(restorer):
    from PIL import Image
    r = restorer
    ok = np.zeros((16, 16, 3), np.uint8)
    noises = [torch.zeros(s) for s in r.net.noise_shapes(1)]
    assert [tuple(t.shape) for t in noises] == [(1, 4, 4), (1, 8, 8), (1, 8, 8), (1, 16, 16), (1, 16, 16)]
    for faces in ([ok], [Image.fromarray(ok)], torch.zeros(1, 16, 16, 3, dtype=torch.uint8), np.zeros((2, 16, 16, 3), np.uint8)):
        with pytest.raises(_Touched):                       # valid input reaches the device step
            r.restore_aligned(faces, noises if not isinstance(faces, np.ndarray) else None)
    with pytest.raises(TypeError):
        r.restore_aligned([ok.astype(np.float32)])
    with pytest.raises(TypeError):
        r.restore_aligned(torch.zeros(1, 16, 16, 3))
    with pytest.raises(TypeError):
        r.restore_aligned("face.png")
    with pytest.raises(ValueError):
        r.restore_aligned([np.zeros((16, 16), np.uint8)])
    with pytest.raises(ValueError):
        r.restore_aligned([])
    with pytest.raises(ValueError):
        r.restore_aligned([ok, np.zeros((8, 8, 3), np.uint8)])
    with pytest.raises(ValueError):
        r.restore_aligned(torch.zeros(16, 16, 3, dtype=torch.uint8))
    with pytest.raises(NotImplementedError) as e:           # enhance would cv2.resize: not restated
        r.restore_aligned([np.zeros((24, 24, 3), np.uint8)])
    assert "16 x 16" in str(e.value)
    with pytest.raises(ValueError):
        r.restore_aligned([ok], noises[:-1])
    with pytest.raises(ValueError):
        r.pre_clamp([ok], noises[:-1] + [torch.zeros(1, 8, 8)])
    with pytest.raises(TypeError):
        r.restore_aligned([ok], noises[:-1] + [torch.zeros(1, 16, 16, dtype=torch.float64)])
    with pytest.raises(ValueError):
        r.restore_aligned([ok], noises, out=torch.zeros(1, 16, 16, 3))
    with pytest.raises(ValueError):                         # right type and shape, but on the host: also before the device step
        r.restore_aligned([ok], noises, out=torch.zeros(1, 16, 16, 3, dtype=torch.uint8))


def test_constructor_checks(net16):
    from controlanimate_amd.gfpgan import FaceRestorer
    with pytest.raises(TypeError):
        FaceRestorer(net16.state_dict(), dtype=torch.float32, out_size=16)
    with pytest.raises(ValueError):
        FaceRestorer(net16.state_dict(), max_faces_per_launch=0, out_size=16)
    with pytest.raises(NotImplementedError):
        FaceRestorer(net16.state_dict(), out_size=24)


def test_no_cpu_fallback(net16, monkeypatch):
    from controlanimate_amd import _capi
    from controlanimate_amd.gfpgan import FaceRestorer
    r = FaceRestorer(net16.state_dict(), out_size=16, device="cpu")
    with pytest.raises(_capi.CAHipUnavailable):
        r.restore_aligned([np.zeros((16, 16, 3), np.uint8)])
    monkeypatch.setattr(_capi, "_lib", None)
    monkeypatch.setattr(_capi, "LIB_PATH", "/nonexistent/libcontrolanimate_hip.so")
    with pytest.raises(_capi.CAHipUnavailable):
        FaceRestorer(net16.state_dict(), out_size=16).restore_aligned([np.zeros((16, 16, 3), np.uint8)])


# ---- enhance: GFPGANer's control flow around a caller-supplied helper -----------------------------------------------------------------
def test_enhance_drives_the_helper_in_gfpganers_order(restorer, monkeypatch):
    r = restorer
    seen = []

    def fake_restore(faces, noises=None, generator=None, out=None):
        seen.append(len(faces))
        return torch.stack([torch.from_numpy(255 - np.asarray(f)) for f in faces])
    monkeypatch.setattr(r, "restore_aligned", fake_restore)
    frame = np.random.RandomState(SEED).randint(0, 256, (40, 64, 3), dtype=np.uint8)
    helper = R.FakeHelper(16, [(2, 3), (20, 40)])
    cropped, restored, img = r.enhance(frame, has_aligned=False, only_center_face=False, paste_back=True, face_helper=helper)
    assert helper.calls == ["clean_all", "read_image", ("get_face_landmarks_5", False, 5), "align_warp_face", "add_restored_face", "add_restored_face",
                            ("get_inverse_affine", None), ("paste_faces_to_input_image", False)]
    assert seen == [2]                                            # all cropped faces of the frame in ONE pass
    assert len(cropped) == 2 and len(restored) == 2 and np.array_equal(img[2:18, 3:19], 255 - frame[2:18, 3:19]) and np.array_equal(img[0], frame[0])

    class Bg:
        scale = 2

        def enhance(self, img, outscale=None):
            self.outscale = outscale
            return np.repeat(np.repeat(img, 2, 0), 2, 1), None
    bg = Bg()
    out = r.as_face_enhancer(helper)(frame, bg_upsampler=bg)
    assert bg.outscale == 2 and out.shape == (80, 128, 3) and helper.calls[-1] == ("paste_faces_to_input_image", True) and seen == [2, 2]
    _, _, none = r.enhance(frame, paste_back=False, only_center_face=True, face_helper=helper)
    assert none is None and ("get_face_landmarks_5", True, 5) in helper.calls and helper.calls[-1] == "add_restored_face"
    cropped, restored, none = r.enhance(frame[:16, :16], has_aligned=True)
    assert none is None and len(cropped) == 1 and np.array_equal(restored[0], 255 - frame[:16, :16]) and seen[-1] == 1
    helper0 = R.FakeHelper(16, [])
    r.enhance(frame, face_helper=helper0)
    assert "add_restored_face" not in helper0.calls and seen[-1] == 1   # a frame without faces does not run the net


def test_enhance_without_a_helper_names_what_is_missing(restorer):
    frame = np.zeros((40, 64, 3), np.uint8)
    with pytest.raises(NotImplementedError) as e:
        restorer.enhance(frame)
    assert "face_helper" in str(e.value) and "detection" in str(e.value) and "paste" in str(e.value)
    with pytest.raises(NotImplementedError):
        restorer.as_face_enhancer(None)


def test_upscaler_still_raises_without_a_callable():
    from controlanimate_amd.upscaler import Upscaler
    sd = rrdb_ref.rrdb_state_dict(seed=1)
    with pytest.raises(NotImplementedError):
        Upscaler(2, state_dict=sd)                            # the reference's default use_face_enhancer=True
    with pytest.raises(NotImplementedError):
        Upscaler(2, use_face_enhancer=True, state_dict=sd)


# ---- the container and the finish fixture ------------------------------------------------------------------------------------------------
def test_container_round_trip_and_channel_reversal():
    faces = R.make_faces(16, 2, SEED)
    x = R.container_in(faces)
    assert x.shape == (2, 3, 16, 16) and x.dtype == torch.float32 and x.min() >= -1 and x.max() <= 1
    assert torch.equal(x[:, 0], R.container_in(faces, reverse_channels=False)[:, 2])
    assert np.array_equal(R.container_out(x), faces.numpy())      # the identity network: uint8 in = uint8 out, channels back in place
    assert R.container_out(torch.tensor([-3.0, 0.0, 7.0]).view(1, 3, 1, 1), reverse_channels=False).ravel().tolist() == [0, 128, 255]  # 127.5 -> 128: half to even


def test_finish_fixture_keeps_its_share_of_near_ties_under_the_cap():
    """At most 1 % of the unclamped values of the finish test's fixture lie within 1e-3 of a half-integer before the rounding (a locally
    uniform value has 0.2 % there)."""
    x = R.make_finish_fixture(SEED + 6)
    pre = R.pre_round64(x)
    unclamped = (x.abs() < 1).permute(0, 2, 3, 1).numpy()[..., ::-1]
    share = R.in_band(pre)[unclamped].mean()
    print(f"finish fixture: {unclamped.mean():.3f} unclamped, {share:.4%} of them within {R.BAND} of a half-integer")
    assert 0.5 < unclamped.mean() < 0.9 and 0 < share <= 0.01
    assert (x.abs() > 1).any() and (x == 1).any() and (x == -1).any()


# ---- the ABI additions ---------------------------------------------------------------------------------------------------------------
def test_abi_additions(capi):
    header = open(HEADER).read()
    assert capi.ABI_VERSION == 16 and capi.CA_ACT_LEAKY02 == 6 and re.search(r"#define CA_ACT_LEAKY02 6\b", header)
    assert re.search(r"#define CA_ACT_RELU6 5\b", header) and re.search(r"#define CA_ACT_RELU 4\b", header)      # the existing codes keep their values
    for name in ("ca_gfp_prep", "ca_resample2x", "ca_gfp_styles", "ca_modconv3x3", "ca_gfp_modulate", "ca_gfp_style_epilogue", "ca_gfp_to_rgb", "ca_gfp_finish"):
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name)


def test_modconv_args_struct_matches_c_layout(capi, tmp_path):
    import subprocess
    st = capi.ModconvArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){", 'printf("size %zu\\n", sizeof(ca_modconv_args));']
    lines += [f'printf("{f} %zu\\n", offsetof(ca_modconv_args, {f}));' for f, _ in st._fields_]
    lines.append("return 0;}")
    src, exe = str(tmp_path / "l.c"), str(tmp_path / "l")
    open(src, "w").write("\n".join(lines))
    subprocess.check_call(["gcc", "-o", exe, src])
    got = dict(l.split() for l in subprocess.check_output([exe], text=True).strip().splitlines())
    assert int(got["size"]) == C.sizeof(st)
    for f, _ in st._fields_:
        assert int(got[f]) == getattr(st, f).offset, f


def test_entry_points_reject_bad_arguments_without_a_gpu(capi):
    """Validation comes before any launch, and the message names the entry point (this runs on a machine without a GPU)."""
    lib = capi.lib()
    fake, f2 = C.c_void_p(0x1000), C.c_void_p(0x2000)

    def expect(rc, who):
        assert rc < 0 and who.encode() in lib.ca_last_error(), (rc, lib.ca_last_error())

    expect(lib.ca_gfp_prep(None, fake, fake, fake, 1, 8, 8, 32, 1, 1, None), "ca_gfp_prep")
    expect(lib.ca_gfp_prep(fake, fake, fake, fake, 1, 8, 8, 12, 1, 1, None), "ca_gfp_prep")              # cout % 8
    expect(lib.ca_gfp_prep(fake, fake, fake, fake, 1, 8, 8, 32, 2, 1, None), "ca_gfp_prep")              # the flag
    expect(lib.ca_gfp_prep(fake, fake, fake, fake, 1, 8, 8, 32, 1, 7, None), "ca_gfp_prep")              # dtype
    expect(lib.ca_resample2x(fake, fake, 1, 8, 8, 64, 1, 1, None), "ca_resample2x")                      # in place
    expect(lib.ca_resample2x(fake, f2, 1, 7, 8, 64, 0, 1, None), "ca_resample2x")                        # odd plane halves
    expect(lib.ca_resample2x(fake, f2, 1, 8, 8, 12, 1, 1, None), "ca_resample2x")                        # c % 8
    expect(lib.ca_resample2x(fake, f2, 1, 8, 8, 64, 2, 1, None), "ca_resample2x")
    expect(lib.ca_resample2x(fake, f2, 4096, 1024, 1024, 64, 1, 1, None), "ca_resample2x")               # 2^31 bytes

    def desc(*v):
        return (C.c_int32 * len(v))(*v)
    ok = (0, 64, 64, 0, 513 * 64, 0)
    total = 513 * 64 + 64 * 64
    expect(lib.ca_gfp_styles(None, fake, total, desc(*ok), 1, fake, 128, 1, 2, None), "ca_gfp_styles")
    expect(lib.ca_gfp_styles(fake, fake, total, desc(*ok), 0, fake, 128, 1, 2, None), "ca_gfp_styles")   # no layer
    expect(lib.ca_gfp_styles(fake, fake, total, desc(*ok), 33, fake, 128, 1, 2, None), "ca_gfp_styles")
    expect(lib.ca_gfp_styles(fake, fake, total, desc(2, *ok[1:]), 1, fake, 128, 1, 2, None), "ca_gfp_styles")             # latent index
    expect(lib.ca_gfp_styles(fake, fake, total, desc(0, 48, *ok[2:]), 1, fake, 128, 1, 2, None), "ca_gfp_styles")         # cin
    expect(lib.ca_gfp_styles(fake, fake, total - 1, desc(*ok), 1, fake, 128, 1, 2, None), "ca_gfp_styles")                # Wsq leaves params
    expect(lib.ca_gfp_styles(fake, fake, total, desc(*ok), 1, fake, 127, 1, 2, None), "ca_gfp_styles")                    # out leaves its row
    expect(lib.ca_gfp_styles(fake, fake, total, desc(*ok[:5], 1), 1, fake, 128, 1, 2, None), "ca_gfp_styles")

    def mc(**kw):
        base = dict(x=0x1000, wt=0x2000, s=0x3000, demod=0x4000, noise=0x5000, bias=0x6000, y=0x7000, s_stride=128, demod_stride=128, images=2, h=4, w=4, cin=64, cout=64,
                    upsample=0, x_shared=0, noise_weight=0.1, dtype=1)
        base.update(kw)
        return C.byref(capi.ModconvArgs(**base))
    expect(lib.ca_modconv3x3(None, None), "ca_modconv3x3")
    expect(lib.ca_modconv3x3(mc(noise=None), None), "ca_modconv3x3")
    expect(lib.ca_modconv3x3(mc(cin=96), None), "ca_modconv3x3")
    expect(lib.ca_modconv3x3(mc(cout=32), None), "ca_modconv3x3")
    expect(lib.ca_modconv3x3(mc(sft_scale=0x8000), None), "ca_modconv3x3")                              # scale without shift
    expect(lib.ca_modconv3x3(mc(upsample=2), None), "ca_modconv3x3")
    expect(lib.ca_modconv3x3(mc(y=0x1000), None), "ca_modconv3x3")                                      # in place
    expect(lib.ca_modconv3x3(mc(x=0x1008), None), "ca_modconv3x3")                                      # alignment
    expect(lib.ca_modconv3x3(mc(dtype=2), None), "ca_modconv3x3")
    expect(lib.ca_modconv3x3(mc(images=64, h=512, w=512, upsample=1), None), "ca_modconv3x3")           # 2^31 bytes
    expect(lib.ca_modconv3x3(mc(noise_weight=float("nan")), None), "ca_modconv3x3")
    expect(lib.ca_gfp_modulate(fake, fake, 64, fake, 2, 4, 4, 64, 0, 0, 1, None), "ca_gfp_modulate")                     # in place
    expect(lib.ca_gfp_modulate(fake, fake, 64, f2, 2, 4, 4, 96, 0, 0, 1, None), "ca_gfp_modulate")                       # c
    expect(lib.ca_gfp_modulate(fake, fake, 64, f2, 2, 4, 4, 64, 2, 0, 1, None), "ca_gfp_modulate")                       # the flag
    expect(lib.ca_gfp_modulate(fake, fake, 64, f2, 64, 512, 512, 64, 1, 0, 1, None), "ca_gfp_modulate")                  # 2^31 bytes
    expect(lib.ca_gfp_modulate(fake, None, 64, f2, 2, 4, 4, 64, 0, 0, 1, None), "ca_gfp_modulate")
    expect(lib.ca_gfp_style_epilogue(fake, fake, 64, None, 0.1, fake, None, None, fake, 2, 4, 4, 64, 1, None), "ca_gfp_style_epilogue")
    expect(lib.ca_gfp_style_epilogue(fake, fake, 64, fake, 0.1, fake, fake, None, fake, 2, 4, 4, 64, 1, None), "ca_gfp_style_epilogue")   # scale without shift
    expect(lib.ca_gfp_style_epilogue(fake, fake, 64, fake, 0.1, fake, None, None, fake, 2, 4, 4, 32, 1, None), "ca_gfp_style_epilogue")   # c
    expect(lib.ca_gfp_style_epilogue(fake, fake, 64, fake, float("nan"), fake, None, None, fake, 2, 4, 4, 64, 1, None), "ca_gfp_style_epilogue")
    expect(lib.ca_gfp_style_epilogue(fake, fake, 64, fake, 0.1, fake, None, None, fake, 2, 4, 4, 64, 5, None), "ca_gfp_style_epilogue")   # dtype
    expect(lib.ca_gfp_to_rgb(fake, fake, fake, 0, fake, None, None, 1, 4, 4, 64, 1, None), "ca_gfp_to_rgb")
    expect(lib.ca_gfp_to_rgb(fake, fake, fake, 0, fake, None, f2, 1, 4, 4, 48, 1, None), "ca_gfp_to_rgb")       # cin
    expect(lib.ca_gfp_to_rgb(fake, fake, fake, 0, fake, fake, f2, 1, 5, 4, 64, 1, None), "ca_gfp_to_rgb")       # odd plane with a previous image
    expect(lib.ca_gfp_to_rgb(fake, fake, fake, 0, fake, f2, f2, 1, 4, 4, 64, 1, None), "ca_gfp_to_rgb")         # out is prev
    expect(lib.ca_gfp_finish(None, fake, 16, 1, None), "ca_gfp_finish")
    expect(lib.ca_gfp_finish(fake, fake, 0, 1, None), "ca_gfp_finish")
    expect(lib.ca_gfp_finish(fake, fake, 16, 3, None), "ca_gfp_finish")
