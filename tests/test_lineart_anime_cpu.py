"""CPU: the specification of the lineart_anime annotator (tests/lineart_anime_ref.py: the 32 tensors of the U-Net),
LineartAnimeAnnotator's loading and input checks, the pack functions against torch, the annotator lookup of the ControlNet pipeline,
the numpy finish, and the argument checks of the entry points added to ABI v16 for it (no launch, no GPU)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lineart_anime_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ca_lanime_conv_in", "ca_conv4x4s2", "ca_im2col4x4s2", "ca_convt4x4s2", "ca_instnorm_act_partials_floats", "ca_instnorm_act", "ca_lanime_conv_out", "ca_lanime_finish"]


@pytest.fixture(scope="module")
def capi():
    from controlanimate_amd import _build, _capi
    _build.build(verbose=False)
    return _capi


@pytest.fixture(scope="module")
def sd():
    return lineart_anime_ref.lineart_anime_state_dict(seed=3)


# ---- the specification -------------------------------------------------------------------------------------------------------------
def test_key_table_has_32_tensors_and_54405505_parameters(sd):
    from controlanimate_amd.lineart_anime import conv_keys, lineart_anime_key_shapes
    want = lineart_anime_key_shapes()
    assert len(want) == 32 and sum(int(np.prod(s)) for s in want.values()) == 54405505
    net = lineart_anime_ref.UnetGenerator()
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == want          # the restated network has exactly these tensors
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert conv_keys(0) == ("model.model.0", "model.model.3")
    assert conv_keys(1) == ("model.model.1.model.1", "model.model.1.model.5")
    assert conv_keys(3) == ("model.model.1.model.3.model.3.model.1", "model.model.1.model.3.model.3.model.5")
    assert conv_keys(7) == ("model.model.1" + ".model.3" * 6 + ".model.1", "model.model.1" + ".model.3" * 6 + ".model.3")
    assert want["model.model.0.weight"] == (64, 3, 4, 4) and want["model.model.3.weight"] == (128, 1, 4, 4) and want["model.model.3.bias"] == (1,)
    assert want["model.model.1.model.5.weight"] == (256, 64, 4, 4)                          # transposed: [Cin = 2 x 128, Cout, 4, 4]
    assert want[conv_keys(7)[1] + ".weight"] == (512, 512, 4, 4) and want[conv_keys(6)[1] + ".weight"] == (1024, 512, 4, 4)


def test_state_dict_checks_name_the_offender(sd):
    from controlanimate_amd.lineart_anime import LineartAnimeAnnotator, check_state_dict
    check_state_dict(sd)
    gone = "model.model.1.model.3.model.5.bias"
    missing = {k: v for k, v in sd.items() if k != gone}
    with pytest.raises(KeyError, match=re.escape(gone)):
        check_state_dict(missing)
    with pytest.raises(KeyError):
        LineartAnimeAnnotator(missing)
    extra = dict(sd, **{"model.model.4.weight": torch.zeros(1)})
    with pytest.raises(ValueError, match=re.escape("model.model.4.weight")):
        LineartAnimeAnnotator(extra)
    wrong = dict(sd, **{"model.model.1.model.5.weight": torch.zeros(64, 256, 4, 4)})        # a Conv2d layout where ConvTranspose2d's is due
    with pytest.raises(ValueError, match=re.escape("model.model.1.model.5.weight")):
        LineartAnimeAnnotator(wrong)
    with pytest.raises(TypeError):
        LineartAnimeAnnotator(sd, dtype=torch.float32)


def test_module_prefix_is_accepted_and_files_are_local(sd, tmp_path):
    from controlanimate_amd.annotators import LineartAnimeAnnotator
    prefixed = {"module." + k: v for k, v in sd.items()}
    a = LineartAnimeAnnotator(prefixed)
    assert torch.equal(a._host["out_b"], sd["model.model.3.bias"])
    torch.save(prefixed, tmp_path / "netG.pth")
    b = LineartAnimeAnnotator.from_pretrained(tmp_path)
    c = LineartAnimeAnnotator(str(tmp_path / "netG.pth"))
    for x in (b, c):
        assert torch.equal(x._host["in_b"], sd["model.model.0.bias"]) and torch.equal(x._host["conv_in"], a._host["conv_in"])
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(FileNotFoundError, match=re.escape(str(empty / "netG.pth"))):
        LineartAnimeAnnotator.from_pretrained(empty)
    with pytest.raises(FileNotFoundError, match="nowhere.pth"):
        LineartAnimeAnnotator(str(tmp_path / "nowhere.pth"))


def test_only_three_biases_are_kept(sd):
    from controlanimate_amd.lineart_anime import LineartAnimeAnnotator, conv_keys
    h = LineartAnimeAnnotator(sd)._host
    assert torch.equal(h["in_b"], sd["model.model.0.bias"]) and torch.equal(h["inner_b"], sd[conv_keys(7)[0] + ".bias"])
    assert torch.equal(h["out_b"], sd["model.model.3.bias"])
    assert sorted(k for k in h if k.endswith("_b")) == ["in_b", "inner_b", "out_b"]
    assert len(h["down"]) == 7 and len(h["up"]) == 7 and tuple(h["out_w"].shape) == (4, 4, 128) and h["out_w"].dtype == torch.float32
    assert tuple(h["up"][0].shape) == (4, 64, 2, 2, 256) and tuple(h["up"][6].shape) == (4, 512, 2, 2, 512) and tuple(h["down"][6].shape) == (512, 4, 4, 512)


# ---- the pack functions against torch ----------------------------------------------------------------------------------------------------
def test_pack_convt4x4_phases_reproduces_conv_transpose2d():
    from controlanimate_amd.lineart_anime import pack_convt4x4_phases
    g = torch.Generator().manual_seed(0)
    cin, cout, h, w = 6, 4, 5, 7
    x = torch.randn(2, cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cin, cout, 4, 4, generator=g, dtype=torch.float64)
    ref = F.conv_transpose2d(x, wt, stride=2, padding=1)
    W = pack_convt4x4_phases(wt)
    assert tuple(W.shape) == (4, cout, 2, 2, cin) and W.is_contiguous() and W.dtype == torch.float64
    xp = F.pad(x, (1, 1, 1, 1))                                      # zero outside the image; source (y - 1 + a, x - 1 + b) = xp[y + a, x + b]
    out = torch.zeros(2, cout, 2 * h, 2 * w, dtype=torch.float64)
    for py in range(2):
        for px in range(2):
            acc = torch.zeros(2, cout, h, w, dtype=torch.float64)
            for dy in range(2):
                for dx in range(2):
                    acc += torch.einsum("oc,nchw->nohw", W[py * 2 + px, :, dy, dx, :], xp[:, :, py + dy:py + dy + h, px + dx:px + dx + w])
            out[:, :, py::2, px::2] = acc
    assert ref.shape == out.shape and (out - ref).abs().max().item() <= 1e-12
    with pytest.raises(ValueError):
        pack_convt4x4_phases(torch.zeros(4, 4, 3, 3))


def test_pack_conv4x4_and_conv_in_orders():
    from controlanimate_amd.lineart_anime import pack_conv4x4, pack_conv_in
    w = torch.arange(64 * 3 * 16, dtype=torch.float32).view(64, 3, 4, 4)
    p = pack_conv_in(w)
    assert tuple(p.shape) == (64, 64) and (p[:, 48:] == 0).all()
    for o, c, ky, kx in ((0, 0, 0, 0), (5, 2, 3, 1), (63, 1, 2, 3)):
        assert p[o, ky * 12 + kx * 3 + c] == w[o, c, ky, kx]
    g = torch.Generator().manual_seed(1)
    wt = torch.randn(8, 5, 4, 4, generator=g, dtype=torch.float64)
    x = torch.randn(1, 5, 6, 8, generator=g, dtype=torch.float64)
    q = pack_conv4x4(wt)
    assert tuple(q.shape) == (8, 4, 4, 5) and q.is_contiguous()
    cols = F.unfold(x, 4, padding=1, stride=2).view(1, 5, 16, 3 * 4)                      # [n, cin, ky * 4 + kx, pixels]
    out = torch.einsum("okc,nckp->nop", q.reshape(8, 16, 5), cols).view(1, 8, 3, 4)
    assert (out - F.conv2d(x, wt, stride=2, padding=1)).abs().max().item() <= 1e-12
    with pytest.raises(ValueError):
        pack_conv4x4(torch.zeros(4, 4, 3, 3))
    with pytest.raises(ValueError):
        pack_conv_in(torch.zeros(64, 3, 7, 7))


def test_conv_in_padding_lies_in_the_normalised_image():
    """(sum over valid taps of w * byte) / 127.5 - (sum over valid taps of w) is the convolution of the zero-padded normalised
    image -- what ca_lanime_conv_in computes; padding the BYTE image with 0 instead would feed -1 at the border."""
    g = torch.Generator().manual_seed(2)
    wt = torch.randn(4, 3, 4, 4, generator=g, dtype=torch.float64)
    img = torch.randint(0, 256, (1, 3, 6, 8), generator=g).double()
    ref = F.conv2d(img / 127.5 - 1.0, wt, stride=2, padding=1)
    got = F.conv2d(img, wt, stride=2, padding=1) / 127.5 - F.conv2d(torch.ones_like(img), wt, stride=2, padding=1)
    assert (got - ref).abs().max().item() <= 1e-12
    wrong = F.conv2d(F.pad(img, (1, 1, 1, 1)) / 127.5 - 1.0, wt, stride=2)
    assert (wrong - ref)[..., 0, :].abs().max().item() > 0.1 and (wrong - ref)[..., 1:-1, 1:-1].abs().max().item() <= 1e-12


# ---- LineartAnimeAnnotator: input checks before the device ----------------------------------------------------------------------------
def test_annotator_checks_types_sizes_and_scope_before_the_device(capi, sd, monkeypatch):
    from PIL import Image
    from controlanimate_amd.annotators import LineartAnimeAnnotator
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "LIB_PATH", "/nonexistent/libcontrolanimate_hip.so")   # touching the device would raise CAHipUnavailable
    ann = LineartAnimeAnnotator(sd)
    u8, f32 = np.zeros((256, 512, 3), np.uint8), np.zeros((256, 512, 3), np.float32)
    for call in (ann, lambda x: ann.edges([x]), lambda x: ann.annotate_batch([x]), lambda x: ann.pre_tanh([x])):
        with pytest.raises(TypeError):
            call(f32)
    with pytest.raises(TypeError):
        ann.edges(torch.zeros((1, 256, 512, 3), dtype=torch.float32))
    with pytest.raises(ValueError):
        ann.edges([u8, np.zeros((256, 256, 3), np.uint8)])
    with pytest.raises(ValueError, match="RGBA"):
        ann.annotate_batch([Image.new("RGBA", (512, 256))])
    with pytest.raises(ValueError):
        ann.annotate_batch([u8], rep=3)
    with pytest.raises(TypeError):
        ann.annotate_batch([u8], dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ann.edges([])
    with pytest.raises(NotImplementedError, match="320 x 512"):
        ann.edges([np.zeros((320, 512, 3), np.uint8)])                                 # in LineartAnnotator's scope (% 64), not in this one's
    with pytest.raises(NotImplementedError):
        ann.annotate_batch(torch.zeros((2, 256, 576, 3), dtype=torch.uint8))
    with pytest.raises(NotImplementedError):
        ann(np.zeros((128, 256), np.uint8))
    # in scope (mode L and RGB alike, any multiple of 256): the device comes next, and there is none
    for ok in (u8, Image.new("RGB", (512, 256)), Image.new("L", (256, 256)), np.zeros((512, 768, 3), np.uint8), np.zeros((768, 512, 3), np.uint8)):
        with pytest.raises(capi.CAHipUnavailable):
            ann.edges([ok])
    with pytest.raises(capi.CAHipUnavailable):
        ann(u8)


def test_annotator_needs_a_gpu(capi, sd, monkeypatch):
    from controlanimate_amd.annotators import LineartAnimeAnnotator
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(capi.CAHipUnavailable, match="LineartAnimeAnnotator"):
        LineartAnimeAnnotator(sd).annotate_batch([np.zeros((256, 256, 3), np.uint8)])


def test_chunking_keeps_the_largest_operand_addressable(sd):
    from controlanimate_amd.annotators import LineartAnimeAnnotator
    ann = LineartAnimeAnnotator(sd)
    per_frame = (512 // 2) * (768 // 2) * 128 * 2          # the concatenation buffer C_0
    assert ann.chunk_frames(512, 768) == (0x7FFFFF00 - 1) // per_frame == 85      # a 16-frame window is one pass
    assert ann.chunk_frames(512, 768) * per_frame < 0x7FFFFF00
    ann.max_activation_bytes = per_frame - 1
    with pytest.raises(ValueError):
        ann.chunk_frames(512, 768)


def test_im2col_buffer_serves_every_chunk_up_to_the_largest():
    """kernels.conv4x4s2 picks the gather form from the rows of the chunk it gets, so a short last chunk gathers at levels that run on
    the tile kernel at the full chunk: 95 frames of 512 x 768 are 85 + 10, and level 4 (16 x 24 pixels from 512 channels) has 3840 rows
    in the tail.  The buffer of a workspace holds what any chunk of 1 .. m frames needs."""
    from controlanimate_amd.kernels import CONV4X4S2_GEMM_ROWS
    from controlanimate_amd.lineart_anime import CHANNELS, cols_elems

    def need(k, h, w):   # what a chunk of k frames gathers at most
        rows = [(i, k * (h >> (i + 1)) * (w >> (i + 1))) for i in range(1, 8)]
        return max([r * 16 * CHANNELS[i - 1] for i, r in rows if r < CONV4X4S2_GEMM_ROWS], default=0)

    assert need(85, 512, 768) == 2040 * 16 * 512 and need(10, 512, 768) == 3840 * 16 * 512 > need(85, 512, 768)
    for h, w, ms in ((512, 768, (1, 10, 16, 85)), (256, 256, (1, 2, 3, 4, 5, 16, 63, 64, 341)), (768, 512, (7, 85)), (1024, 1024, (1, 31))):
        for m in ms:
            worst = max(need(k, h, w) for k in range(1, m + 1))
            assert cols_elems(m, h, w) == worst, (h, w, m)                              # enough for every chunk, and no more
    assert cols_elems(85, 512, 768) == 42 * 96 * 16 * 512 > need(10, 512, 768)          # a 42-frame chunk at level 5: 4032 rows


# ---- the detector's last step ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def finish_case():
    return lineart_anime_ref.finish_case()


def test_finish_specification_leaves_few_pixels_undecided(finish_case):
    n, h, w, _, want, decided = finish_case
    share = 1.0 - decided.mean()
    print(f"share of pixels within 1e-3 of an integer: {share:.4f}")
    assert share <= 0.01
    assert want.min() < 40 and want.max() > 215  # the map uses its range
    assert want[0, 0, 0] == 255 and want[0, 0, 1] == 0 and want[0, 0, 2] == 128   # inverted: tanh = -1 -> line 0 -> 255; tanh(0) -> trunc(127.5) = 127 -> 128
    m, s = lineart_anime_ref.finish_ref(np.array([0.5, -0.5], np.float32))
    assert m.tolist() == [255 - 186, 255 - 68] and abs(s[0] - (np.tanh(0.5) * 127.5 + 127.5)) < 1e-12   # 186.42 -> 186; 68.58 -> 68


def test_detector_restatement_and_in_place_activations(sd):
    """The restated detector on one 256 x 256 frame; and the skip tensors are what the storage convention says: the block below
    sees LeakyReLU(d_0), the last transposed convolution sees ReLU(d_0) -- the effect of the in-place activations."""
    frames = lineart_anime_ref.frames_fixture(256, 256, 1)
    out = lineart_anime_ref.lineart_anime_detect(sd, frames[0])
    assert out.dtype == np.uint8 and out.shape == (256, 256, 3) and np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 0], out[..., 2])
    pre = lineart_anime_ref.pre_tanh_ref(sd, frames)
    want, _ = lineart_anime_ref.finish_ref(pre[0].numpy())
    assert (np.abs(out[..., 0].astype(int) - want.astype(int)) <= 1).all()
    emul = lineart_anime_ref.emulate_pre_tanh(sd, frames, torch.float32)                   # the chain as the device orders it, unrounded
    rel = ((emul - pre).norm() / pre.norm()).item()
    print(f"the chain in the device's order, fp32, against the nn.Module network: relative L2 {rel:.3e}")
    assert rel <= 1e-4
    with pytest.raises(NotImplementedError):
        lineart_anime_ref.lineart_anime_detect(sd, np.zeros((320, 256, 3), np.uint8))


# ---- the annotator lookup --------------------------------------------------------------------------------------------------------------
class _Tag:
    def __init__(self, tag):
        self.tag = tag

    def __call__(self, image):
        return (self.tag, image)

    def annotate_batch(self, frames, out=None, rep=1, dtype=None):
        return (self.tag, "batch")


LINEART, ANIME = "lllyasviel/control_v11p_sd15_lineart", "lllyasviel/control_v11p_sd15s2_lineart_anime"


def _pipe(annotators):
    from controlanimate_amd.controlresiduals_pipeline import MultiControlNetResidualsPipeline
    pipe = MultiControlNetResidualsPipeline.__new__(MultiControlNetResidualsPipeline)   # the lookup alone: no nets, no device
    pipe.annotators = dict(annotators)
    return pipe


@pytest.mark.parametrize("order", [("lineart", "lineart_anime"), ("lineart_anime", "lineart")])
def test_lookup_serves_the_anime_net_from_its_own_key_only(sd, order):
    from controlanimate_amd.annotators import LineartAnimeAnnotator
    ann = LineartAnimeAnnotator(sd)
    tags = {"lineart": _Tag("a"), "lineart_anime": ann}
    pipe = _pipe({k: tags[k] for k in order})
    img = np.zeros((8, 8, 3), np.uint8)
    assert pipe._annotator_for(ANIME) is ann and pipe._annotator_for(LINEART) is tags["lineart"]
    assert pipe.prepare_controlnet_input_image(LINEART, img)[0] == "a"
    assert pipe._batch_annotator(ANIME, [img]) is not None and pipe._batch_annotator(LINEART, [img])([img])[0] == "a"
    alone = _pipe({"lineart": _Tag("a")})                                                 # with `lineart` alone the anime net has no annotator
    assert alone._annotator_for(ANIME) is None and alone._batch_annotator(ANIME, [img]) is None
    assert alone.prepare_controlnet_input_image(ANIME, img) is img


# ---- the entry points --------------------------------------------------------------------------------------------------------------
def test_abi_is_still_16_and_header_binding_library_agree(capi):
    assert capi.ABI_VERSION == 16
    lib = capi.lib()
    assert lib.ca_abi_version() == 16
    header = open(os.path.join(ROOT, "include", "controlanimate_hip.h")).read()
    assert "#define CA_ABI_VERSION 16" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert name in capi.SYMBOLS and getattr(lib, name) is not None
        decl = re.search(r"\b(?:int|int64_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert decl, f"{name} is not declared in the header"
        assert len([a for a in decl.group(1).split(",") if a.strip()]) == len(capi.SYMBOLS[name][1]), name   # one binding type per C parameter
    from controlanimate_amd import kernels as K
    for fn in ("lanime_conv_in", "conv4x4s2", "conv_transpose4x4s2", "instance_norm_act", "lanime_conv_out", "lanime_finish"):
        assert callable(getattr(K, fn))
    from controlanimate_amd import _build
    assert "ca_lineart_anime.hip" in _build.SOURCES


def test_instnorm_act_partials_size_and_the_old_entry_points_are_unchanged(capi):
    lib = capi.lib()
    # a chunk is 262144 / c pixels, halved down to 16384 / c while images * chunks < 256
    assert lib.ca_instnorm_act_partials_floats(2, 2, 2, 512) == 2 * 1 * 2 * 512               # one chunk: the one-launch form
    assert lib.ca_instnorm_act_partials_floats(16, 4, 6, 512) == 16 * 1 * 2 * 512             # 24 pixels of 32 per chunk
    assert lib.ca_instnorm_act_partials_floats(16, 16, 24, 512) == 16 * 12 * 2 * 512          # 384 pixels in chunks of 32: 192 blocks
    assert lib.ca_instnorm_act_partials_floats(16, 32, 48, 512) == 16 * 24 * 2 * 512          # 1536 pixels in chunks of 64: 384 blocks
    assert lib.ca_instnorm_act_partials_floats(16, 256, 384, 64) == 16 * 24 * 2 * 64          # 98304 pixels in chunks of 4096: 384 blocks
    assert lib.ca_instnorm_act_partials_floats(1, 70, 66, 64) == 1 * 19 * 2 * 64              # 4620 pixels in chunks of 256
    assert lib.ca_instnorm_act_partials_floats(1, 8, 8, 96) == 0 and lib.ca_instnorm_act_partials_floats(0, 8, 8, 64) == 0
    assert lib.ca_instnorm_partials_floats(1, 8, 8, 512) == 0                                 # the lineart annotator's entry points still stop at 256


def test_entry_points_reject_bad_arguments_without_a_launch(capi):
    lib = capi.lib()
    fake, odd, odd4 = C.c_void_p(0x1000), C.c_void_p(0x1004), C.c_void_p(0x1002)  # never dereferenced: validation fails first

    def expect(rc, who):
        assert rc < 0 and who.encode() in lib.ca_last_error(), (rc, lib.ca_last_error())

    who = "ca_lanime_conv_in"
    expect(lib.ca_lanime_conv_in(None, fake, fake, fake, fake, 1, 8, 8, 1, None), who)
    expect(lib.ca_lanime_conv_in(fake, fake, None, fake, fake, 1, 8, 8, 1, None), who)            # bias
    expect(lib.ca_lanime_conv_in(fake, fake, fake, fake, None, 1, 8, 8, 1, None), who)            # c0
    expect(lib.ca_lanime_conv_in(fake, fake, fake, fake, fake, 1, 7, 8, 1, None), who)            # odd height
    expect(lib.ca_lanime_conv_in(fake, fake, fake, fake, fake, 0, 8, 8, 1, None), who)
    expect(lib.ca_lanime_conv_in(fake, fake, fake, fake, fake, 1, 8, 8, 2, None), who)            # dtype
    expect(lib.ca_lanime_conv_in(fake, fake, fake, odd, fake, 1, 8, 8, 1, None), who)             # alignment
    expect(lib.ca_lanime_conv_in(fake, fake, odd4, fake, fake, 1, 8, 8, 1, None), who)
    expect(lib.ca_lanime_conv_in(fake, fake, fake, fake, fake, 64, 8192, 8192, 1, None), who)     # 2^32 pixels
    expect(lib.ca_lanime_conv_in(fake, fake, fake, fake, fake, 64, 1024, 1024, 1, None), who)     # c0 of 4 GiB
    who = "ca_conv4x4s2"
    expect(lib.ca_conv4x4s2(None, fake, None, fake, 1, 8, 8, 64, 128, 0, 1, None), who)
    expect(lib.ca_conv4x4s2(fake, None, None, fake, 1, 8, 8, 64, 128, 0, 1, None), who)
    expect(lib.ca_conv4x4s2(fake, fake, None, None, 1, 8, 8, 64, 128, 0, 1, None), who)
    expect(lib.ca_conv4x4s2(fake, fake, None, fake, 1, 8, 9, 64, 128, 0, 1, None), who)           # odd width
    expect(lib.ca_conv4x4s2(fake, fake, None, fake, 1, 8, 8, 96, 128, 0, 1, None), who)           # cin
    expect(lib.ca_conv4x4s2(fake, fake, None, fake, 1, 8, 8, 64, 64, 0, 1, None), who)            # cout
    expect(lib.ca_conv4x4s2(fake, fake, None, fake, 1, 8, 8, 64, 128, 2, 1, None), who)           # relu
    expect(lib.ca_conv4x4s2(fake, fake, None, fake, 1, 8, 8, 64, 128, 0, 3, None), who)           # dtype
    expect(lib.ca_conv4x4s2(odd, fake, None, fake, 1, 8, 8, 64, 128, 0, 1, None), who)
    expect(lib.ca_conv4x4s2(fake, fake, odd4, fake, 1, 8, 8, 64, 128, 0, 1, None), who)           # bias alignment
    expect(lib.ca_conv4x4s2(fake, fake, None, fake, 64, 1024, 1024, 64, 128, 0, 1, None), who)    # x of 8 GiB
    who = "ca_im2col4x4s2"
    expect(lib.ca_im2col4x4s2(None, fake, 1, 8, 8, 64, 1, None), who)
    expect(lib.ca_im2col4x4s2(fake, None, 1, 8, 8, 64, 1, None), who)
    expect(lib.ca_im2col4x4s2(fake, fake, 1, 8, 7, 64, 1, None), who)                             # odd width
    expect(lib.ca_im2col4x4s2(fake, fake, 1, 8, 8, 60, 1, None), who)                             # cin % 8
    expect(lib.ca_im2col4x4s2(fake, fake, 1, 8, 8, 2048, 1, None), who)
    expect(lib.ca_im2col4x4s2(fake, odd, 1, 8, 8, 64, 1, None), who)
    expect(lib.ca_im2col4x4s2(fake, fake, 1, 8, 8, 64, 2, None), who)
    expect(lib.ca_im2col4x4s2(fake, fake, 16, 512, 512, 512, 1, None), who)                       # cols of 16 GiB
    who = "ca_convt4x4s2"
    expect(lib.ca_convt4x4s2(None, fake, fake, 1, 8, 8, 256, 64, 1, None), who)
    expect(lib.ca_convt4x4s2(fake, fake, fake, 1, 0, 8, 256, 64, 1, None), who)
    expect(lib.ca_convt4x4s2(fake, fake, fake, 1, 8, 8, 128, 64, 1, None), who)                   # cin
    expect(lib.ca_convt4x4s2(fake, fake, fake, 1, 8, 8, 256, 32, 1, None), who)                   # cout
    expect(lib.ca_convt4x4s2(fake, fake, odd, 1, 8, 8, 256, 64, 1, None), who)
    expect(lib.ca_convt4x4s2(fake, fake, fake, 1, 8, 8, 256, 64, 7, None), who)
    expect(lib.ca_convt4x4s2(fake, fake, fake, 16, 1024, 1024, 256, 64, 1, None), who)            # y of 8 GiB
    who = "ca_instnorm_act"
    ok = (fake, 1, 0, 64, None, 0, 0, 0)
    expect(lib.ca_instnorm_act(None, fake, *ok, 1, 8, 8, 64, 1e-5, 1, None), who)
    expect(lib.ca_instnorm_act(fake, None, *ok, 1, 8, 8, 64, 1e-5, 1, None), who)
    expect(lib.ca_instnorm_act(fake, fake, None, 1, 0, 64, None, 0, 0, 0, 1, 8, 8, 64, 1e-5, 1, None), who)       # y0
    expect(lib.ca_instnorm_act(fake, fake, *ok, 1, 8, 8, 96, 1e-5, 1, None), who)                                 # c
    expect(lib.ca_instnorm_act(fake, fake, *ok, 1, 8, 8, 1024, 1e-5, 1, None), who)
    expect(lib.ca_instnorm_act(fake, fake, fake, 3, 0, 64, None, 0, 0, 0, 1, 8, 8, 64, 1e-5, 1, None), who)       # act
    expect(lib.ca_instnorm_act(fake, fake, fake, 1, 64, 64, None, 0, 0, 0, 1, 8, 8, 64, 1e-5, 1, None), who)      # off + c > stride
    expect(lib.ca_instnorm_act(fake, fake, fake, 1, 4, 128, None, 0, 0, 0, 1, 8, 8, 64, 1e-5, 1, None), who)      # off % 8
    expect(lib.ca_instnorm_act(fake, fake, fake, 1, 0, 64, fake, 2, 64, 100, 1, 8, 8, 64, 1e-5, 1, None), who)    # second stride
    expect(lib.ca_instnorm_act(fake, fake, fake, 1, 0, 64, fake, 5, 0, 64, 1, 8, 8, 64, 1e-5, 1, None), who)      # second act
    expect(lib.ca_instnorm_act(fake, fake, fake, 1, 0, 64, odd, 1, 0, 64, 1, 8, 8, 64, 1e-5, 1, None), who)       # alignment
    expect(lib.ca_instnorm_act(fake, fake, *ok, 1, 8, 8, 64, 0.0, 1, None), who)                                  # eps
    expect(lib.ca_instnorm_act(fake, fake, *ok, 1, 8, 8, 64, 1e-5, 4, None), who)                                 # dtype
    expect(lib.ca_instnorm_act(fake, fake, *ok, 0, 8, 8, 64, 1e-5, 1, None), who)
    who = "ca_lanime_conv_out"
    expect(lib.ca_lanime_conv_out(fake, fake, None, fake, 1, 8, 8, 1, None), who)                 # bias
    expect(lib.ca_lanime_conv_out(fake, fake, fake, fake, 1, 8, 0, 1, None), who)
    expect(lib.ca_lanime_conv_out(odd, fake, fake, fake, 1, 8, 8, 1, None), who)
    expect(lib.ca_lanime_conv_out(fake, fake, fake, odd, 1, 8, 8, 1, None), who)                  # out is stored two floats at a time
    expect(lib.ca_lanime_conv_out(fake, fake, fake, fake, 1, 8, 8, 9, None), who)
    who = "ca_lanime_finish"
    expect(lib.ca_lanime_finish(None, 1, 8, 8, fake, None, 1, 2, None), who)
    expect(lib.ca_lanime_finish(fake, 1, 8, 8, None, None, 1, 2, None), who)               # neither output
    expect(lib.ca_lanime_finish(fake, 1, 3, 5, fake, None, 1, 2, None), who)               # h * w % 4
    expect(lib.ca_lanime_finish(fake, 1, 8, 8, fake, None, 3, 2, None), who)               # rep
    expect(lib.ca_lanime_finish(fake, 1, 8, 8, None, fake, 1, 0, None), who)               # a bf16 control tensor
    expect(lib.ca_lanime_finish(fake, 1, 8, 8, None, odd, 1, 2, None), who)                # alignment
