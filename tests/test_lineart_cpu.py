"""CPU: the specification of the lineart annotator (tests/lineart_ref.py: the 24 tensors of the network), LineartAnnotator's loading
and input checks, the phase form of the transposed convolution, the biases that cancel, the annotator lookup of the ControlNet
pipeline, and the argument checks of the entry points added to ABI v16 for it (no launch, no GPU)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lineart_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ca_lineart_conv_in", "ca_instnorm_partials_floats", "ca_instnorm_stats", "ca_instnorm_apply", "ca_convt3x3s2_gather", "ca_lineart_conv_out",
       "ca_lineart_finish"]


@pytest.fixture(scope="module")
def capi():
    from controlanimate_amd import _build, _capi
    _build.build(verbose=False)
    return _capi


@pytest.fixture(scope="module")
def sd():
    return lineart_ref.lineart_state_dict(seed=3)


# ---- the specification -------------------------------------------------------------------------------------------------------------
def test_key_table_has_24_tensors_and_4290945_parameters(sd):
    from controlanimate_amd.lineart import lineart_key_shapes
    want = lineart_key_shapes()
    assert len(want) == 24 and sum(int(np.prod(s)) for s in want.values()) == 4290945
    net = lineart_ref.Generator()
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == want          # the restated network has exactly these tensors
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert want["model3.0.weight"] == (256, 128, 3, 3) and want["model3.0.bias"] == (128,)   # transposed: [Cin, Cout, 3, 3]
    assert want["model3.3.weight"] == (128, 64, 3, 3) and want["model4.1.weight"] == (1, 64, 7, 7)


def test_state_dict_checks_name_the_offender(sd):
    from controlanimate_amd.lineart import LineartAnnotator, check_state_dict
    check_state_dict(sd)
    missing = {k: v for k, v in sd.items() if k != "model2.1.conv_block.5.bias"}
    with pytest.raises(KeyError, match=re.escape("model2.1.conv_block.5.bias")):
        check_state_dict(missing)
    with pytest.raises(KeyError):
        LineartAnnotator(missing)
    extra = dict(sd, **{"model5.0.weight": torch.zeros(1)})
    with pytest.raises(ValueError, match=re.escape("model5.0.weight")):
        LineartAnnotator(extra)
    wrong = dict(sd, **{"model3.0.weight": torch.zeros(128, 256, 3, 3)})                   # a Conv2d layout where ConvTranspose2d's is due
    with pytest.raises(ValueError, match=re.escape("model3.0.weight")):
        LineartAnnotator(wrong)
    with pytest.raises(TypeError):
        LineartAnnotator(sd, dtype=torch.float32)


def test_file_selection_and_missing_files(sd, tmp_path):
    from controlanimate_amd.annotators import LineartAnnotator
    fine, coarse = dict(sd), dict(sd, **{"model4.1.bias": sd["model4.1.bias"] + 1.0})
    torch.save(fine, tmp_path / "sk_model.pth")
    torch.save(coarse, tmp_path / "sk_model2.pth")
    a = LineartAnnotator.from_pretrained(tmp_path)
    b = LineartAnnotator.from_pretrained(str(tmp_path), coarse=True)
    c = LineartAnnotator(tmp_path / "sk_model2.pth")                                       # a file is taken as it is
    assert not a.coarse and b.coarse
    assert torch.equal(a._host["out_b"], sd["model4.1.bias"]) and torch.equal(b._host["out_b"], sd["model4.1.bias"] + 1.0)
    assert torch.equal(c._host["out_b"], b._host["out_b"])
    assert torch.equal(LineartAnnotator(str(tmp_path), coarse=True)._host["out_b"], b._host["out_b"])
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(FileNotFoundError, match=re.escape(str(empty / "sk_model.pth"))):
        LineartAnnotator.from_pretrained(empty)
    with pytest.raises(FileNotFoundError, match=re.escape(str(empty / "sk_model2.pth"))):
        LineartAnnotator.from_pretrained(empty, coarse=True)
    with pytest.raises(FileNotFoundError, match="nowhere.pth"):
        LineartAnnotator(str(tmp_path / "nowhere.pth"))


# ---- LineartAnnotator: input checks before the device --------------------------------------------------------------------------------
def test_annotator_checks_types_sizes_and_scope_before_the_device(capi, sd, monkeypatch):
    from PIL import Image
    from controlanimate_amd.annotators import LineartAnnotator
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "LIB_PATH", "/nonexistent/libcontrolanimate_hip.so")   # touching the device would raise CAHipUnavailable
    ann = LineartAnnotator(sd)
    u8, f32 = np.zeros((64, 128, 3), np.uint8), np.zeros((64, 128, 3), np.float32)
    for call in (ann, lambda x: ann.edges([x]), lambda x: ann.annotate_batch([x]), lambda x: ann.logits([x])):
        with pytest.raises(TypeError):
            call(f32)
    with pytest.raises(TypeError):
        ann.edges(torch.zeros((1, 64, 128, 3), dtype=torch.float32))
    with pytest.raises(ValueError):
        ann.edges([u8, np.zeros((64, 64, 3), np.uint8)])
    with pytest.raises(ValueError, match="RGBA"):
        ann.annotate_batch([Image.new("RGBA", (128, 64))])
    with pytest.raises(ValueError):
        ann.annotate_batch([u8], rep=3)
    with pytest.raises(TypeError):
        ann.annotate_batch([u8], dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ann.edges([])
    with pytest.raises(NotImplementedError, match="72 x 128"):
        ann.edges([np.zeros((72, 128, 3), np.uint8)])
    with pytest.raises(NotImplementedError):
        ann.annotate_batch(torch.zeros((2, 72, 128, 3), dtype=torch.uint8))
    with pytest.raises(NotImplementedError):
        ann(np.zeros((128, 72), np.uint8))
    # in scope (mode L and RGB alike, any multiple of 64): the device comes next, and there is none
    for ok in (u8, Image.new("RGB", (128, 64)), Image.new("L", (128, 64)), np.zeros((576, 768, 3), np.uint8)):
        with pytest.raises(capi.CAHipUnavailable):
            ann.edges([ok])
    with pytest.raises(capi.CAHipUnavailable):
        ann(u8)


def test_annotator_needs_a_gpu(capi, sd, monkeypatch):
    from controlanimate_amd.annotators import LineartAnnotator
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(capi.CAHipUnavailable):
        LineartAnnotator(sd).annotate_batch([np.zeros((64, 64, 3), np.uint8)])


def test_chunking_keeps_the_largest_operand_addressable(sd):
    from controlanimate_amd.annotators import LineartAnnotator
    ann = LineartAnnotator(sd)
    per_frame = (512 // 2) * (768 // 2) * 9 * 64 * 2      # the taps of the second transposed convolution
    assert ann.chunk_frames(512, 768) == (0x7FFFFF00 - 1) // per_frame == 18      # a 16-frame window is one pass
    assert ann.chunk_frames(512, 768) * per_frame < 0x7FFFFF00
    ann.max_activation_bytes = per_frame - 1
    with pytest.raises(ValueError):
        ann.chunk_frames(512, 768)


# ---- the transposed convolution's phase form -------------------------------------------------------------------------------------------
def test_pack_convt_phases_reproduces_conv_transpose2d():
    from controlanimate_amd.lineart import pack_convt_phases
    g = torch.Generator().manual_seed(0)
    cin, cout, h, w = 6, 4, 5, 7
    x = torch.randn(2, cin, h, w, generator=g)
    wt = torch.randn(cin, cout, 3, 3, generator=g)
    ref = F.conv_transpose2d(x, wt, stride=2, padding=1, output_padding=1)
    W = pack_convt_phases(wt)
    assert tuple(W.shape) == (3, 3, cout, cin) and W.is_contiguous()
    xp = F.pad(x, (0, 1, 0, 1))                                      # x[H] = x[.][W] = 0

    def tap(ky, kx, dy, dx):                                         # W[ky][kx] . x[i + dy, j + dx] for every (i, j)
        return torch.einsum("oc,nchw->nohw", W[ky][kx], xp[:, :, dy:dy + h, dx:dx + w])

    out = torch.zeros(2, cout, 2 * h, 2 * w)
    out[:, :, 0::2, 0::2] = tap(1, 1, 0, 0)
    out[:, :, 0::2, 1::2] = tap(1, 2, 0, 0) + tap(1, 0, 0, 1)
    out[:, :, 1::2, 0::2] = tap(2, 1, 0, 0) + tap(0, 1, 1, 0)
    out[:, :, 1::2, 1::2] = tap(2, 2, 0, 0) + tap(2, 0, 0, 1) + tap(0, 2, 1, 0) + tap(0, 0, 1, 1)
    assert ref.shape == out.shape and (out - ref).abs().max().item() <= 1e-5
    with pytest.raises(ValueError):
        pack_convt_phases(torch.zeros(4, 4, 2, 2))


def test_pack_conv_in_orders_a_tile_row_contiguously():
    from controlanimate_amd.lineart import pack_conv_in
    w = torch.arange(64 * 3 * 49, dtype=torch.float32).view(64, 3, 7, 7)
    p = pack_conv_in(w)
    assert tuple(p.shape) == (64, 160) and (p[:, 147:] == 0).all()
    for o, c, ky, kx in ((0, 0, 0, 0), (5, 2, 3, 6), (63, 1, 6, 0)):
        assert p[o, ky * 21 + kx * 3 + c] == w[o, c, ky, kx]


# ---- biases in front of a non-affine InstanceNorm cancel -------------------------------------------------------------------------------
def test_only_the_last_bias_reaches_the_result(sd):
    frames = lineart_ref.frames_fixture()[:1]
    full = lineart_ref.logits_ref(sd, frames)
    bare = {k: (torch.zeros_like(v) if k.endswith(".bias") and k != "model4.1.bias" else v) for k, v in sd.items()}
    assert any(v.abs().max() > 0.01 for k, v in sd.items() if k.endswith(".bias") and k != "model4.1.bias")
    got = lineart_ref.logits_ref(bare, frames)
    rel = ((got - full).norm() / full.norm()).item()
    print(f"all biases zero but model4.1.bias: relative L2 {rel:.3e}")
    assert rel <= 1e-4
    moved = lineart_ref.logits_ref(dict(sd, **{"model4.1.bias": sd["model4.1.bias"] + 0.5}), frames)
    assert torch.allclose(moved, full + 0.5, atol=1e-5)


def test_detector_restatement(sd):
    frames = lineart_ref.frames_fixture()
    out = lineart_ref.lineart_detect(sd, frames[0])
    assert out.dtype == np.uint8 and out.shape == (64, 128, 3) and np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 0], out[..., 2])
    want, _ = lineart_ref.finish_ref(lineart_ref.logits_ref(sd, frames[:1])[0].numpy())
    assert (np.abs(out[..., 0].astype(int) - want.astype(int)) <= 1).all()
    grey = lineart_ref.lineart_detect(sd, frames[0][..., 0])
    assert np.array_equal(grey, lineart_ref.lineart_detect(sd, np.repeat(frames[0][..., :1], 3, axis=2)))
    with pytest.raises(NotImplementedError):
        lineart_ref.lineart_detect(sd, np.zeros((72, 128, 3), np.uint8))
    m, s = lineart_ref.finish_ref(np.array([-100.0, 0.0, 100.0, 0.0079], np.float32))
    assert m.tolist() == [255, 128, 0, 127] and abs(s[1] - 127.5) < 1e-9   # 255 - trunc(127.5) = 128; sigmoid(0.0079) * 255 = 128.004 -> 127


# ---- the annotator lookup --------------------------------------------------------------------------------------------------------------
def _pipe(annotators):
    from controlanimate_amd.controlresiduals_pipeline import MultiControlNetResidualsPipeline
    pipe = MultiControlNetResidualsPipeline.__new__(MultiControlNetResidualsPipeline)   # the lookup alone: no nets, no device
    pipe.annotators = dict(annotators)
    return pipe


class _Tag:
    def __init__(self, tag):
        self.tag = tag

    def __call__(self, image):
        return (self.tag, image)

    def annotate_batch(self, frames, out=None, rep=1, dtype=None):
        return (self.tag, "batch")


LINEART, ANIME = "lllyasviel/control_v11p_sd15_lineart", "lllyasviel/control_v11p_sd15s2_lineart_anime"


@pytest.mark.parametrize("order", [("lineart", "lineart_anime"), ("lineart_anime", "lineart")])
def test_lookup_longest_contained_key_wins(order):
    tags = {"lineart": _Tag("a"), "lineart_anime": _Tag("b")}
    pipe = _pipe({k: tags[k] for k in order})
    img = np.zeros((8, 8, 3), np.uint8)
    assert pipe.prepare_controlnet_input_image(LINEART, img)[0] == "a"
    assert pipe.prepare_controlnet_input_image(ANIME, img)[0] == "b"
    assert pipe._batch_annotator(LINEART, [img])([img])[0] == "a"
    assert pipe._batch_annotator(ANIME, [img])([img])[0] == "b"


def test_lookup_lineart_alone_does_not_serve_lineart_anime():
    pipe = _pipe({"lineart": _Tag("a")})
    img = np.zeros((8, 8, 3), np.uint8)
    assert pipe.prepare_controlnet_input_image(ANIME, img) is img          # taken as already annotated
    assert pipe._batch_annotator(ANIME, [img]) is None
    assert pipe.prepare_controlnet_input_image(LINEART, img)[0] == "a"
    assert pipe._batch_annotator(LINEART, [img]) is not None
    other = _pipe({"lineart": _Tag("a"), "anime": _Tag("c")})                 # another contained key still serves the name
    assert other.prepare_controlnet_input_image(ANIME, img)[0] == "c" and other._batch_annotator(ANIME, [img])([img])[0] == "c"
    assert other.prepare_controlnet_input_image(LINEART, img)[0] == "a"


def test_lookup_single_keys_behave_as_before():
    from controlanimate_amd.annotators import canny
    pipe = _pipe({"canny": canny, "hed": _Tag("h")})
    img = np.zeros((8, 8, 3), np.uint8)
    out = pipe.prepare_controlnet_input_image("lllyasviel/sd-controlnet-canny", img)
    assert isinstance(out, np.ndarray) and out.shape == (8, 8, 3) and out is not img
    assert pipe.prepare_controlnet_input_image("lllyasviel/sd-controlnet-hed", img)[0] == "h"
    assert pipe._batch_annotator("lllyasviel/sd-controlnet-hed", [img])([img])[0] == "h"
    assert pipe._batch_annotator("lllyasviel/sd-controlnet-canny", [img]) is None            # the plain function has no annotate_batch
    assert pipe.prepare_controlnet_input_image("lllyasviel/sd-controlnet-openpose", img) is img
    assert pipe._batch_annotator("lllyasviel/sd-controlnet-hed", [torch.zeros(3, 8, 8)]) is None
    t = torch.zeros(3, 8, 8)
    assert pipe.prepare_controlnet_input_image("lllyasviel/sd-controlnet-hed", t) is t


# ---- the entry points --------------------------------------------------------------------------------------------------------------
def test_abi_is_still_16_and_header_binding_library_agree(capi):
    assert capi.ABI_VERSION == 16
    lib = capi.lib()
    assert lib.ca_abi_version() == 16
    header = open(os.path.join(ROOT, "include", "controlanimate_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert name in capi.SYMBOLS and getattr(lib, name) is not None
        decl = re.search(r"\b(?:int|int64_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert decl, f"{name} is not declared in the header"
        assert len([a for a in decl.group(1).split(",") if a.strip()]) == len(capi.SYMBOLS[name][1]), name   # one binding type per C parameter
    from controlanimate_amd import kernels as K
    for fn in ("lineart_conv_in", "instance_norm", "conv_transpose3x3s2", "lineart_conv_out", "lineart_finish"):
        assert callable(getattr(K, fn))
    from controlanimate_amd import _build
    assert "ca_lineart.hip" in _build.SOURCES


def test_instnorm_partials_size(capi):
    lib = capi.lib()
    assert lib.ca_instnorm_partials_floats(2, 6, 10, 64) == 2 * 1 * 2 * 64                  # one chunk of 4096 pixels
    assert lib.ca_instnorm_partials_floats(16, 128, 192, 256) == 16 * 24 * 2 * 256          # 1024 pixels per chunk at 256 channels
    assert lib.ca_instnorm_partials_floats(1, 65, 63, 64) == 1 * 1 * 2 * 64                 # 4095 pixels
    assert lib.ca_instnorm_partials_floats(1, 64, 64, 64) == 1 * 1 * 2 * 64 and lib.ca_instnorm_partials_floats(1, 64, 65, 64) == 2 * 2 * 64
    assert lib.ca_instnorm_partials_floats(1, 8, 8, 96) == 0 and lib.ca_instnorm_partials_floats(0, 8, 8, 64) == 0


def test_entry_points_reject_bad_arguments_without_a_launch(capi):
    lib = capi.lib()
    fake, odd = C.c_void_p(0x1000), C.c_void_p(0x1004)  # never dereferenced: validation fails first

    def expect(rc, who):
        assert rc < 0 and who.encode() in lib.ca_last_error(), (rc, lib.ca_last_error())

    who = "ca_lineart_conv_in"
    expect(lib.ca_lineart_conv_in(None, fake, fake, 1, 8, 8, 1, None), who)
    expect(lib.ca_lineart_conv_in(fake, fake, fake, 1, 3, 8, 1, None), who)                 # reflection by 3 needs 4 rows
    expect(lib.ca_lineart_conv_in(fake, fake, fake, 0, 8, 8, 1, None), who)
    expect(lib.ca_lineart_conv_in(fake, fake, fake, 1, 8, 8, 2, None), who)                 # dtype
    expect(lib.ca_lineart_conv_in(fake, fake, odd, 1, 8, 8, 1, None), who)                  # alignment
    expect(lib.ca_lineart_conv_in(fake, fake, fake, 64, 8192, 8192, 1, None), who)          # 2^32 pixels
    who = "ca_instnorm_stats"
    expect(lib.ca_instnorm_stats(None, fake, 1, 8, 8, 64, 0, 1, None), who)
    expect(lib.ca_instnorm_stats(fake, None, 1, 8, 8, 64, 0, 1, None), who)
    expect(lib.ca_instnorm_stats(fake, fake, 1, 8, 8, 96, 0, 1, None), who)                 # c
    expect(lib.ca_instnorm_stats(fake, fake, 1, 8, 8, 64, 2, 1, None), who)                 # in_ring
    expect(lib.ca_instnorm_stats(odd, fake, 1, 8, 8, 64, 0, 1, None), who)
    expect(lib.ca_instnorm_stats(fake, fake, 1, 8, 8, 64, 0, 5, None), who)
    who = "ca_instnorm_apply"
    expect(lib.ca_instnorm_apply(fake, fake, None, None, 1, 8, 8, 64, 0, 0, 0, 0, 1e-5, 1, None), who)     # y
    expect(lib.ca_instnorm_apply(fake, fake, odd, fake, 1, 8, 8, 64, 0, 0, 0, 0, 1e-5, 1, None), who)      # residual alignment
    expect(lib.ca_instnorm_apply(fake, fake, None, fake, 1, 8, 8, 512, 0, 0, 0, 0, 1e-5, 1, None), who)    # c
    expect(lib.ca_instnorm_apply(fake, fake, None, fake, 1, 8, 8, 64, 0, 0, 2, 0, 1e-5, 1, None), who)     # out_pad
    expect(lib.ca_instnorm_apply(fake, fake, None, fake, 1, 1, 8, 64, 0, 0, 1, 0, 1e-5, 1, None), who)     # one row cannot be reflected
    expect(lib.ca_instnorm_apply(fake, fake, None, fake, 1, 8, 8, 64, 0, 0, 0, 0, 0.0, 1, None), who)      # eps
    who = "ca_convt3x3s2_gather"
    expect(lib.ca_convt3x3s2_gather(None, fake, 1, 8, 8, 64, 1, None), who)
    expect(lib.ca_convt3x3s2_gather(fake, fake, 1, 8, 8, 60, 1, None), who)                 # cout % 8
    expect(lib.ca_convt3x3s2_gather(fake, fake, 1, 0, 8, 64, 1, None), who)
    expect(lib.ca_convt3x3s2_gather(fake, fake, 32, 4096, 4096, 64, 1, None), who)          # 2^31 output pixels
    expect(lib.ca_convt3x3s2_gather(fake, odd, 1, 8, 8, 64, 1, None), who)
    who = "ca_lineart_conv_out"
    expect(lib.ca_lineart_conv_out(fake, fake, None, fake, 1, 8, 8, 1, None), who)          # bias
    expect(lib.ca_lineart_conv_out(fake, fake, fake, fake, 1, 8, 3, 1, None), who)
    expect(lib.ca_lineart_conv_out(odd, fake, fake, fake, 1, 8, 8, 1, None), who)
    expect(lib.ca_lineart_conv_out(fake, fake, fake, fake, 1, 8, 8, 9, None), who)
    who = "ca_lineart_finish"
    expect(lib.ca_lineart_finish(None, 1, 8, 8, fake, None, 1, 2, None), who)
    expect(lib.ca_lineart_finish(fake, 1, 8, 8, None, None, 1, 2, None), who)               # neither output
    expect(lib.ca_lineart_finish(fake, 1, 3, 5, fake, None, 1, 2, None), who)               # h * w % 4
    expect(lib.ca_lineart_finish(fake, 1, 8, 8, fake, None, 3, 2, None), who)               # rep
    expect(lib.ca_lineart_finish(fake, 1, 8, 8, None, fake, 1, 0, None), who)               # a bf16 control tensor
    expect(lib.ca_lineart_finish(fake, 1, 8, 8, None, odd, 1, 2, None), who)                # alignment
