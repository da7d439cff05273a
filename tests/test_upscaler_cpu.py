"""CPU: the Real-ESRGAN upscaler's host side -- weight loading (basicsr key names, params_ema before params, strict key check),
output sizes and the reference's scale assertion, the ABI v14 struct layout and argument validation, the LANCZOS4 tables and
properties of the resize restatement (tests/rrdb_ref.py)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rrdb_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "controlanimate_hip.h")


@pytest.fixture(scope="module")
def capi():
    from controlanimate_amd import _build, _capi
    _build.build(verbose=False)
    return _capi


@pytest.fixture(scope="module")
def sd():
    return rrdb_ref.rrdb_state_dict(seed=1)


def test_state_dict_keys_are_basicsr_names(sd):
    from controlanimate_amd.upscaler import RRDBNet
    keys = set(RRDBNet().state_dict().keys())
    assert keys == set(sd.keys())
    assert "body.5.rdb3.conv5.weight" in keys and "conv_last.bias" in keys and len(keys) == 2 * (1 + 6 * 15 + 5)


def test_load_params_ema_before_params(sd, tmp_path):
    from controlanimate_amd.local_models import load_realesrgan_state_dict
    from controlanimate_amd.upscaler import Upscaler
    other = rrdb_ref.rrdb_state_dict(seed=2)
    for name, payload, want in (("ema.pth", {"params_ema": sd}, sd), ("params.pth", {"params": other}, other),
                                ("both.pth", {"params": other, "params_ema": sd}, sd)):
        p = str(tmp_path / name)
        torch.save(payload, p)
        got = load_realesrgan_state_dict(p)
        assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want), name
        up = Upscaler(4, use_face_enhancer=False, model_path=p)
        assert torch.equal(up.model.conv_last.bias, want["conv_last.bias"])
        assert torch.equal(up.model.body[3].rdb2.conv4.weight, want["body.3.rdb2.conv4.weight"])


def test_wrong_or_missing_keys_name_both_lists(sd, tmp_path):
    from controlanimate_amd.upscaler import Upscaler
    bad = dict(sd)
    bad["conv_lastx.weight"] = bad.pop("conv_last.weight")
    p = str(tmp_path / "bad.pth")
    torch.save({"params_ema": bad}, p)
    with pytest.raises(KeyError) as e:
        Upscaler(4, use_face_enhancer=False, model_path=p)
    msg = str(e.value)
    assert "missing" in msg and "conv_last.weight" in msg and "unexpected" in msg and "conv_lastx.weight" in msg
    with pytest.raises(FileNotFoundError) as e:
        Upscaler(4, use_face_enhancer=False, model_path=str(tmp_path / "nope.pth"))
    assert "nope.pth" in str(e.value)


def test_output_sizes_and_scale_assertion(sd):
    from PIL import Image
    from controlanimate_amd.upscaler import Upscaler, output_size
    assert output_size(768, 512, 2) == (1536, 1024)
    assert output_size(768, 512, 3) == (2304, 1536)
    assert output_size(768, 512, 4) == (3072, 2048)
    assert output_size(768, 512, 1.5) == (1152, 768)
    assert output_size(77, 51, 1.5) == (115, 76)   # int() truncation, as vid2vid.py:118-119 and enhance()
    img = Image.new("RGB", (8, 8))
    for bad in (1, 8):
        up = Upscaler(bad, use_face_enhancer=False, state_dict=sd)
        with pytest.raises(AssertionError):
            up(img)
        with pytest.raises(AssertionError):
            up.upscale_frames([img])


def test_face_enhancer_is_a_hook_not_a_fallback(sd):
    from controlanimate_amd.upscaler import Upscaler
    with pytest.raises(NotImplementedError):
        Upscaler(2, state_dict=sd)                      # the reference's default use_face_enhancer=True
    seen = {}

    def fe(arr, bg_upsampler):
        seen["bg"], seen["shape"] = bg_upsampler, arr.shape
        return arr

    from PIL import Image
    up = Upscaler(2, use_face_enhancer=True, upscale_first=True, state_dict=sd, face_enhancer=fe)
    assert up.upscale_first is False                    # forced, as upscaler.py:23 does
    out = up(Image.new("RGB", (6, 4), (10, 20, 30)))
    assert seen["bg"] is up and seen["shape"] == (4, 6, 3) and out.size == (6, 4)


def test_upscaler_from_config(sd, tmp_path):
    from controlanimate_amd.upscaler import Upscaler, upscaler_from_config
    assert upscaler_from_config({"upscale": 1, "use_face_enhancer": 1}) is None
    p = str(tmp_path / "w.pth")
    torch.save({"params_ema": sd}, p)
    up = upscaler_from_config({"upscale": 2, "use_face_enhancer": 0, "upscale_first": 1}, model_path=p)
    assert isinstance(up, Upscaler) and up.scale == 2.0 and not up.use_face_enhancer
    with pytest.raises(NotImplementedError):
        upscaler_from_config({"upscale": 4, "use_face_enhancer": 1}, model_path=p)


def test_narrow_args_struct_matches_c_layout(capi):
    st = capi.ConvNarrowArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(ca_conv3x3_narrow_args));']
    for fname, _ in st._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(ca_conv3x3_narrow_args, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-o", exe, src])
        got = dict(l.split() for l in subprocess.check_output([exe], text=True).strip().splitlines())
    assert int(got["size"]) == C.sizeof(st)
    for fname, _ in st._fields_:
        assert int(got[fname]) == getattr(st, fname).offset, fname


def test_new_entry_points_reject_bad_arguments_without_a_gpu(capi):
    lib = capi.lib()
    fake, fake2 = C.c_void_p(0x1000), C.c_void_p(0x2000)

    def expect(rc, who):
        assert rc < 0 and who.encode() in lib.ca_last_error(), (rc, lib.ca_last_error())

    def args(**kw):
        base = dict(x=fake, w=fake, y=fake2, ldx=192, ldy=192, images=1, hin=8, win=8, cin=64, cout=32, channel_offset=64,
                    s0=1.0, dtype=1)
        base.update(kw)
        return capi.ConvNarrowArgs(**base)

    buf = C.create_string_buffer(64)
    assert lib.ca_conv3x3_narrow_plan_name(C.byref(args()), buf, 64) == 0 and buf.value == b"convn_n32m128"
    assert lib.ca_conv3x3_narrow_plan_name(C.byref(args(cout=64, channel_offset=0)), buf, 64) == 0 and buf.value == b"convn_n64m64"
    assert lib.ca_conv3x3_narrow_plan_name(C.byref(args(cout=3, channel_offset=0, out_u8=1)), buf, 64) == 0 and buf.value == b"convn_n16m128"
    for who in ("ca_conv3x3_narrow", "ca_conv3x3_narrow_plan_name"):
        fn = lib.ca_conv3x3_narrow if who == "ca_conv3x3_narrow" else (lambda a, s: lib.ca_conv3x3_narrow_plan_name(a, buf, 64))
        expect(fn(None, None), "ca_conv3x3_narrow")
        expect(fn(C.byref(args(cin=60, ldx=64)), None), "ca_conv3x3_narrow")                   # cin % 8
        expect(fn(C.byref(args(ldx=56)), None), "ca_conv3x3_narrow")                           # ldx < cin
        expect(fn(C.byref(args(channel_offset=168)), None), "ca_conv3x3_narrow")               # channel_offset + cout > ldy
        expect(fn(C.byref(args(dtype=5)), None), "ca_conv3x3_narrow")                          # dtype
        expect(fn(C.byref(args(cout=48)), None), "ca_conv3x3_narrow")                          # cout
        expect(fn(C.byref(args(cout=3, channel_offset=0)), None), "ca_conv3x3_narrow")         # cout 3 without out_u8
        expect(fn(C.byref(args(out_u8=1)), None), "ca_conv3x3_narrow")                         # out_u8 with cout 32
        expect(fn(C.byref(args(upsample=2)), None), "ca_conv3x3_narrow")
        expect(fn(C.byref(args(r1=fake, ld_r1=30)), None), "ca_conv3x3_narrow")                # residual stride
        expect(fn(C.byref(args(images=4096, hin=1024, win=1024, upsample=1)), None), "ca_conv3x3_narrow")  # >= 2^31 pixels
        expect(fn(C.byref(args(x=None)), None), "ca_conv3x3_narrow")
    expect(lib.ca_conv3x3_narrow_plan_name(C.byref(args()), None, 0), "ca_conv3x3_narrow_plan_name")
    expect(lib.ca_rgb8_to_nhwc(fake, fake2, 1, 8, 8, 7, None), "ca_rgb8_to_nhwc")              # dtype
    expect(lib.ca_rgb8_to_nhwc(fake, fake2, 0, 8, 8, 1, None), "ca_rgb8_to_nhwc")
    expect(lib.ca_rgb8_to_nhwc(None, fake2, 1, 8, 8, 1, None), "ca_rgb8_to_nhwc")
    expect(lib.ca_resize_lanczos4_u8(fake, fake2, 1, 8, 8, 4, 4, fake, fake, fake, None, None), "ca_resize_lanczos4_u8")  # table
    expect(lib.ca_resize_lanczos4_u8(fake, fake2, 1, 8, 0, 4, 4, fake, fake, fake, fake, None), "ca_resize_lanczos4_u8")  # size


def test_lanczos4_tables_equal_the_restatement():
    from controlanimate_amd.upscaler import lanczos4_tables
    for src, dst in ((3072, 1536), (2048, 1024), (256, 192), (96, 115), (40, 40), (17, 5)):
        ofs, coef = lanczos4_tables(src, dst)
        idx, ref = rrdb_ref._axis(src, dst)
        assert np.array_equal(coef.astype(np.int64), ref), (src, dst)
        assert np.array_equal(np.clip(ofs[:, None] + np.arange(8), 0, src - 1), idx), (src, dst)


def test_lanczos4_restatement_properties():
    rng = np.random.default_rng(3)
    const = np.full((21, 34, 3), 137, dtype=np.uint8)
    for dw, dh in ((17, 10), (51, 31), (68, 42)):
        out = rrdb_ref.resize_lanczos4_ref(const, dw, dh)
        assert out.shape == (dh, dw, 3) and np.all(out == 137)
    img = rng.integers(0, 256, size=(19, 23, 3), dtype=np.uint8)
    assert np.array_equal(rrdb_ref.resize_lanczos4_ref(img, 23, 19), img)           # x1: identity
    yy, xx = np.mgrid[0:16, 0:24]
    smooth = np.stack([120 + 50 * np.sin(xx / 14.0 + c) + 40 * np.cos(yy / 12.0 - c) + 2 * c for c in range(3)], -1)
    smooth = np.round(smooth).astype(np.uint8)                                        # a band-limited image (noise is not kept by Lanczos)
    up = smooth.repeat(2, axis=0).repeat(2, axis=1)                                    # nearest x2
    down = rrdb_ref.resize_lanczos4_ref(up, 24, 16)
    assert np.abs(down.astype(int) - smooth.astype(int)).max() <= 1
