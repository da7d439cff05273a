"""CPU: the specification of the softedge annotator (tests/softedge_ref.py), SoftedgeAnnotator's key table, the folding of the three
pixel-difference operators, zero padding, the BGR reversal folded into the weight, loading and input checks, the annotator lookup of the
ControlNet pipeline, the fp16 / bf16 storage emulation, and the argument checks of the entry points added to ABI v16 for it (no launch,
no GPU)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import softedge_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ca_softedge_prep", "ca_relu", "ca_dwconv_k", "ca_maxpool2x2", "ca_pdc_block_supported", "ca_pdc_block", "ca_cdcm_dil4", "ca_csam_reduce",
       "ca_softedge_fuse"]


@pytest.fixture(scope="module")
def capi():
    from controlanimate_amd import _build, _capi
    _build.build(verbose=False)
    return _capi


@pytest.fixture(scope="module")
def sd():
    return R.softedge_state_dict(seed=0)


# ---- the key table ---------------------------------------------------------------------------------------------------------------
def test_key_table_is_the_restated_network(sd):
    from controlanimate_amd.softedge import blocks, softedge_key_shapes
    want = softedge_key_shapes()
    assert set(want) == set(sd) and all(tuple(sd[k].shape) == s for k, s in want.items())
    assert len(want) == 1 + 15 * 2 + 3 * 2 + 4 * (2 + 4 + 2 + 1 + 2) + 2 == 83
    assert [(n, t) for n, t, *_ in blocks()] == R.BLOCKS
    assert [t for _, t in R.BLOCKS] == ["ad", "rd", "cv"] + ["cd", "ad", "rd", "cv"] * 3
    assert [(cin, cout, s) for _, _, cin, cout, s in blocks() if s] == [(60, 120, True), (120, 240, True), (240, 240, True)]
    assert want["init_block.weight"] == (60, 3, 3, 3) and want["block2_1.conv1.weight"] == (60, 1, 3, 3) and want["block2_1.shortcut.bias"] == (120,)
    assert want["dilations.3.conv1.weight"] == (24, 240, 1, 1) and want["attentions.0.conv2.weight"] == (1, 4, 3, 3) and want["classifier.weight"] == (1, 4, 1, 1)


def test_state_dict_checks_name_the_offender(sd):
    from controlanimate_amd.softedge import check_state_dict, strip_state_dict
    check_state_dict(sd)
    wrapped = {"epoch": 20, "state_dict": {"module." + k: v for k, v in sd.items()}}
    bare = strip_state_dict(wrapped)
    assert set(bare) == set(sd) and all(bare[k] is sd[k] for k in sd)
    assert set(strip_state_dict(sd)) == set(sd)                                     # the bare dict is accepted as well
    missing = dict(sd)
    del missing["block3_1.shortcut.bias"]
    with pytest.raises(KeyError, match="block3_1.shortcut.bias"):
        check_state_dict(missing)
    with pytest.raises(ValueError, match="unexpected tensor 'block1_1.shortcut.weight'"):
        check_state_dict(dict(sd, **{"block1_1.shortcut.weight": torch.zeros(60, 60, 1, 1)}))
    with pytest.raises(ValueError, match=r"'dilations.2.conv2_3.weight' has shape \(24, 24, 1, 1\)"):
        check_state_dict(dict(sd, **{"dilations.2.conv2_3.weight": torch.zeros(24, 24, 1, 1)}))
    with pytest.raises(ValueError, match="not a state dict"):
        strip_state_dict([1, 2])
    with pytest.raises(KeyError):                                                   # the converted form has other tensors: not this
        check_state_dict({k: v for k, v in sd.items() if "conv1" not in k})


# ---- folding ---------------------------------------------------------------------------------------------------------------------
def test_fold_pdc_on_hand_written_cases():
    from controlanimate_amd.softedge import fold_pdc
    w = torch.arange(1.0, 10.0, dtype=torch.float64).view(1, 1, 3, 3)          # 1 2 3 / 4 5 6 / 7 8 9
    assert torch.equal(fold_pdc(w, "cv"), w)
    assert fold_pdc(w, "cd").view(-1).tolist() == [1, 2, 3, 4, 5 - 45, 6, 7, 8, 9]
    # ad: position i minus the weight at [3, 0, 1, 6, 4, 2, 7, 8, 5][i]: 1-4, 2-1, 3-2, 4-7, 5-5, 6-3, 7-8, 8-9, 9-6
    assert fold_pdc(w, "ad").view(-1).tolist() == [-3, 1, 1, -3, 0, 3, -1, -1, 3]
    # rd: the outer ring of the 5 x 5 takes w.flat[1:] = 2 .. 9 in reading order, the inner ring their negatives, the centre zero
    assert fold_pdc(w, "rd").view(5, 5).tolist() == [[2, 0, 3, 0, 4],
                                                     [0, -2, -3, -4, 0],
                                                     [5, -5, 0, -6, 6],
                                                     [0, -7, -8, -9, 0],
                                                     [7, 0, 8, 0, 9]]
    assert R.AD_PERM == [3, 0, 1, 6, 4, 2, 7, 8, 5] and R.RD_PLUS == [0, 2, 4, 10, 14, 20, 22, 24] and R.RD_MINUS == [6, 7, 8, 11, 13, 16, 17, 18]
    with pytest.raises(ValueError):
        fold_pdc(w, "xd")
    with pytest.raises(ValueError):
        fold_pdc(torch.zeros(1, 1, 5, 5), "cd")


@pytest.mark.parametrize("kind", ["cd", "ad", "rd", "cv"])
@pytest.mark.parametrize("groups", [1, 6])
def test_fold_pdc_equals_the_run_time_operator(kind, groups):
    from controlanimate_amd.softedge import fold_pdc
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 6, 9, 11, generator=g, dtype=torch.float64)
    w = torch.randn(6 if groups == 6 else 4, 6 // groups, 3, 3, generator=g, dtype=torch.float64)
    want = R.pdc_conv(x, w, kind, groups=groups)
    k = fold_pdc(w, kind)
    got = F.conv2d(x, k, padding=k.shape[-1] // 2, groups=groups)
    rel = ((got - want).abs().max() / want.abs().max()).item()
    assert k.dtype == torch.float64 and tuple(k.shape[2:]) == ((5, 5) if kind == "rd" else (3, 3)) and rel <= 1e-12, rel


def test_folded_network_equals_the_specification(sd):
    """folded_layers as plain convolutions (what the device chain runs) against the run-time operators, in float64."""
    from controlanimate_amd.softedge import folded_layers
    frames = R.frames_fixture()
    d = {k: v.double() for k, v in sd.items()}
    want = R.network_ref(d, R.to_input(frames).double())
    lay = folded_layers(d)
    assert lay["init"].dtype == torch.float32                                      # fp32 on the host ...
    lay = folded_layers_f64(d)                                                     # ... evaluated here in float64 to separate folding from rounding
    x = R.to_input(frames).double().flip(1)                                        # RGB: the reversal is in the weight
    x = F.conv2d(x, lay["init"], padding=1)
    feats = []
    for blk in lay["blocks"]:
        if "shortcut" in blk:
            feats.append(x)
            x = F.max_pool2d(x, 2, 2)
        k = blk["dw"].shape[-1]
        y = F.conv2d(F.relu(F.conv2d(x, blk["dw"], padding=k // 2, groups=x.shape[1])), blk["pw"])
        x = y + (F.conv2d(x, *blk["shortcut"]) if "shortcut" in blk else x)
    feats.append(x)
    for a, b in zip(feats, want["features"]):
        assert ((a - b).abs().max() / b.abs().max()).item() <= 1e-12


def folded_layers_f64(d):
    from controlanimate_amd import softedge as S
    init = S.fold_pdc(d["init_block.weight"], "cd")[:, [2, 1, 0]]
    out = {"init": init, "blocks": []}
    for name, kind, _, _, strided in S.blocks():
        blk = {"dw": S.fold_pdc(d[f"{name}.conv1.weight"], kind), "pw": d[f"{name}.conv2.weight"]}
        if strided:
            blk["shortcut"] = (d[f"{name}.shortcut.weight"], d[f"{name}.shortcut.bias"])
        out["blocks"].append(blk)
    return out


def test_bgr_reversal_folded_into_the_weight_equals_reversing_the_input(sd):
    from controlanimate_amd.softedge import fold_pdc, folded_layers
    frames = R.frames_fixture()
    rgb = torch.from_numpy(frames.astype(np.float32) / 255.0).permute(0, 3, 1, 2).contiguous()
    lay = folded_layers(sd)
    assert torch.equal(lay["init"], fold_pdc(sd["init_block.weight"], "cd")[:, [2, 1, 0]])
    with torch.backends.mkldnn.flags(enabled=False):                               # one summation order for both
        a = F.conv2d(rgb, lay["init"], padding=1)
        b = F.conv2d(R.to_input(frames), fold_pdc(sd["init_block.weight"], "cd"), padding=1)
    assert torch.allclose(a, b, rtol=0, atol=1e-5) and torch.equal(R.to_input(frames), rgb.flip(1))


# ---- zero padding ------------------------------------------------------------------------------------------------------------------
def test_zero_padding_leaves_the_network_bit_unchanged_and_the_pad_lanes_zero(sd):
    """The fp32 specification on the padded state dict (60 -> 64, 120 -> 128, 240 -> 256, 24 -> 32, input 3 -> 8).  Run without oneDNN:
    its blocked convolutions choose their summation order by the channel count, which moves last bits (2e-7 on the logit) for reasons that
    have nothing to do with the padding; torch's own kernels add the extra zeros without a trace."""
    from controlanimate_amd.softedge import PADDED, pad_state_dict
    padded = pad_state_dict(sd)
    assert tuple(padded["init_block.weight"].shape) == (64, 8, 3, 3) and tuple(padded["block2_1.conv1.weight"].shape) == (64, 1, 3, 3)
    assert tuple(padded["block3_1.shortcut.weight"].shape) == (256, 128, 1, 1) and tuple(padded["block3_1.shortcut.bias"].shape) == (256,)
    assert tuple(padded["dilations.0.conv1.weight"].shape) == (32, 64, 1, 1) and tuple(padded["dilations.1.conv2_4.weight"].shape) == (32, 32, 3, 3)
    assert tuple(padded["attentions.2.conv1.weight"].shape) == (4, 32, 1, 1) and tuple(padded["attentions.2.conv2.weight"].shape) == (1, 4, 3, 3)
    assert tuple(padded["conv_reduces.3.conv.weight"].shape) == (1, 32, 1, 1) and tuple(padded["classifier.weight"].shape) == (1, 4, 1, 1)
    assert float(padded["block3_1.shortcut.bias"][240:].abs().max()) == 0 and float(padded["dilations.0.conv1.bias"][24:].abs().max()) == 0
    x = R.to_input(R.frames_fixture())
    with torch.backends.mkldnn.flags(enabled=False):
        a = R.network_ref(sd, x)
        b = R.network_ref(padded, F.pad(x, (0, 0, 0, 0, 0, 5)))
    assert torch.equal(a["logit"], b["logit"]) and all(torch.equal(s, t) for s, t in zip(a["sides"], b["sides"]))
    for f, g, c in zip(a["features"], b["features"], (60, 120, 240, 240)):
        assert g.shape[1] == PADDED[c] and torch.equal(f, g[:, :c]) and float(g[:, c:].abs().max()) == 0
    for f, g in zip(a["cdcm"], b["cdcm"]):
        assert g.shape[1] == 32 and torch.equal(f, g[:, :24]) and float(g[:, 24:].abs().max()) == 0


def test_packing(sd):
    from controlanimate_amd.annotators import SoftedgeAnnotator
    from controlanimate_amd.softedge import fold_pdc, pack_depthwise
    ann = SoftedgeAnnotator(sd)
    h = ann._host
    assert tuple(h["init"].shape) == (64, 3, 3, 8) and h["init"].dtype == torch.float16 and float(h["init"][60:].abs().max()) == 0 and float(h["init"][..., 3:].abs().max()) == 0
    assert [tuple(b["dw"].shape) for b in h["blocks"][:4]] == [(9, 64), (25, 64), (9, 64), (9, 64)]          # ad, rd, cv, then cd behind the pool
    assert tuple(h["blocks"][3]["pw"].shape) == (128, 128) and tuple(h["blocks"][3]["bias"].shape) == (128,) and "bias" not in h["blocks"][0]
    assert tuple(h["blocks"][7]["pw"].shape) == (256, 256) and tuple(h["blocks"][8]["pw"].shape) == (256, 256) and tuple(h["blocks"][11]["pw"].shape) == (256, 512)
    rd = fold_pdc(sd["block1_2.conv1.weight"], "rd")
    assert torch.equal(h["blocks"][1]["dw"][:, :60], pack_depthwise(rd).to(torch.float16)) and float(h["blocks"][1]["dw"][:, 60:].abs().max()) == 0
    assert float(h["blocks"][1]["dw"][12].abs().max()) == 0 and float(h["blocks"][1]["dw"][1].abs().max()) == 0   # the centre and a gap of the 5 x 5
    lv = h["levels"][1]
    assert tuple(lv["cdcm1"][0].shape) == (32, 128) and tuple(lv["cdcm2"].shape) == (4, 32, 3, 3, 32) and tuple(lv["w1"].shape) == (4, 32)
    assert tuple(lv["w2"].shape) == (3, 3, 4) and tuple(lv["wr"].shape) == (32,) and lv["w1"].dtype == torch.float32
    assert torch.equal(lv["cdcm2"][2, :24, 1, 2, :24], sd["dilations.1.conv2_3.weight"][:, :, 1, 2].to(torch.float16))
    assert h["classifier"].tolist() == sd["classifier.weight"].reshape(-1).tolist() + sd["classifier.bias"].tolist()
    with pytest.raises(ValueError):
        pack_depthwise(torch.zeros(8, 1, 4, 4))
    with pytest.raises(TypeError):
        SoftedgeAnnotator(sd, dtype=torch.float32)
    for kw in ({"scribble": True}, {"apply_filter": True}):
        with pytest.raises(NotImplementedError):
            SoftedgeAnnotator(sd, **kw)


# ---- the emulation and the decided share -----------------------------------------------------------------------------------------------
def test_storage_emulation_gives_the_error_the_gpu_bar_is_judged_against(sd):
    frames = R.frames_fixture()
    rounded = {k: (v.to(torch.float16).float() if v.dim() == 4 else v) for k, v in sd.items()}
    ref = R.logits_ref(rounded, frames)
    for dtype, bar in ((torch.float16, 1e-2), (torch.bfloat16, 8e-2)):
        em = R.logits_emulated(rounded, frames, dtype)["logit"]
        rel = ((em - ref).norm() / ref.norm()).item()
        print(f"emulated {dtype} storage: relative L2 of the fused logit {rel:.3e} (the GPU bar {bar:.0e}); reference std {float(ref.std()):.2f}")
        assert rel <= bar / 2                                                      # else the seeded weights are badly scaled
    assert 1.5 < float(ref.std()) < 2.5
    feats = R.network_ref(rounded, R.to_input(frames))["features"]
    assert all(0.3 < float(f.std()) < 3.0 for f in feats)                          # fifteen blocks without normalisation stay O(1)


def test_almost_every_pixel_of_the_fixture_is_decided(sd):
    z = R.logits_ref(sd, R.frames_fixture()).numpy()
    share = 1.0 - R.decided(z).mean()
    print(f"pixels within 1e-3 of a byte boundary: {100 * share:.2f} % (about 0.2 % expected of a smooth distribution)")
    assert share <= 0.01
    assert R.decided(np.array([0.0]))[0] and not R.decided(np.array([np.log(128 / 127)]))[0]      # 127.5, and exactly 128
    m = R.tail_ref(np.array([-20.0, 0.0, np.log(128 / 127) + 1e-4, 20.0], np.float32))
    assert m.tolist() == [0, 127, 128, 255] and m.dtype == np.uint8                 # (sigmoid(20) is 1 in fp32)
    assert R.tail_ref(np.array([-1.0, 0.0, 1.0, 20.0], np.float32), safe=True).tolist() == [0, 127, 255, 255]


def test_detector_restatement(sd):
    frames = R.frames_fixture()
    out = R.detect_ref(sd, frames[0])
    assert out.shape == (64, 128, 3) and out.dtype == np.uint8 and np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 0], out[..., 2])
    assert len(np.unique(out)) > 100
    grey = R.detect_ref(sd, frames[0][..., 0])
    assert np.array_equal(grey, R.detect_ref(sd, np.repeat(frames[0][..., :1], 3, axis=2)))
    assert not np.array_equal(out, R.detect_ref(sd, frames[0][..., ::-1].copy()))   # the channel order matters


# ---- loading ---------------------------------------------------------------------------------------------------------------------
def test_loader_is_file_only(sd, tmp_path):
    from controlanimate_amd.annotators import SoftedgeAnnotator
    torch.save({"epoch": 20, "state_dict": {"module." + k: v for k, v in sd.items()}}, tmp_path / "table5_pidinet.pth")
    a = SoftedgeAnnotator.from_pretrained(tmp_path)
    b = SoftedgeAnnotator(str(tmp_path / "table5_pidinet.pth"), safe=True)
    c = SoftedgeAnnotator(sd)
    assert torch.equal(a._host["init"], c._host["init"]) and torch.equal(b._host["levels"][3]["cdcm2"], c._host["levels"][3]["cdcm2"]) and b.safe and not a.safe
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(FileNotFoundError, match=re.escape(str(empty / "table5_pidinet.pth"))):
        SoftedgeAnnotator.from_pretrained(empty)
    with pytest.raises(FileNotFoundError, match="nothing is ever downloaded"):
        SoftedgeAnnotator("lllyasviel/Annotators")
    src = open(os.path.join(ROOT, "controlanimate_amd", "softedge.py")).read()
    assert "weights_only=True" in src and not re.search(r"hf_hub|huggingface_hub|urllib|requests|http", src)


# ---- SoftedgeAnnotator: input checks before the device -------------------------------------------------------------------------------------
def test_annotator_checks_types_sizes_and_scope_before_the_device(capi, sd, monkeypatch):
    from PIL import Image
    from controlanimate_amd.annotators import SoftedgeAnnotator
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "LIB_PATH", "/nonexistent/libcontrolanimate_hip.so")   # touching the device would raise CAHipUnavailable
    ann = SoftedgeAnnotator(sd)
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
    with pytest.raises(NotImplementedError, match="128 x 96"):
        ann.annotate_batch(torch.zeros((2, 128, 96, 3), dtype=torch.uint8))
    with pytest.raises(NotImplementedError):
        ann(np.zeros((128, 72), np.uint8))
    for ok in (u8, Image.new("RGB", (128, 64)), Image.new("L", (64, 192)), np.zeros((512, 768, 3), np.uint8)):
        with pytest.raises(capi.CAHipUnavailable):
            ann.edges([ok])
    with pytest.raises(capi.CAHipUnavailable):
        ann(u8)


def test_annotator_needs_a_gpu(capi, sd, monkeypatch):
    from controlanimate_amd.annotators import SoftedgeAnnotator
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(capi.CAHipUnavailable):
        SoftedgeAnnotator(sd).annotate_batch([np.zeros((64, 64, 3), np.uint8)])


def test_chunking_keeps_the_largest_operand_addressable(sd):
    from controlanimate_amd.annotators import SoftedgeAnnotator
    from controlanimate_amd.softedge import STAGES, stages
    ann = SoftedgeAnnotator(sd)
    per_frame = 512 * 768 * 64 * 2      # a 64-channel tensor at full resolution
    assert ann.chunk_frames(512, 768) == (0x7FFFFF00 - 1) // per_frame == 42      # a 16-frame window is one pass
    ann.max_activation_bytes = per_frame - 1
    with pytest.raises(ValueError):
        ann.chunk_frames(512, 768)
    assert STAGES in (stages(True), stages(False)) and stages(True)["block"] == 3 and stages(False)["block"] == 0
    assert stages(False)["depthwise"] == 15 and stages(False)["pointwise"] == 19 and sum(stages(True).values()) == sum(stages(False).values()) - 3


# ---- the annotator lookup --------------------------------------------------------------------------------------------------------------
def test_lookup_softedge_serves_the_controlnet_name():
    from controlanimate_amd.controlresiduals_pipeline import MultiControlNetResidualsPipeline

    class Tag:
        def __call__(self, image):
            return ("s", image)

        def annotate_batch(self, frames, out=None, rep=1, dtype=None):
            return ("s", "batch")

    pipe = MultiControlNetResidualsPipeline.__new__(MultiControlNetResidualsPipeline)   # the lookup alone: no nets, no device
    tag = Tag()
    pipe.annotators = {"softedge": tag}
    img = np.zeros((8, 8, 3), np.uint8)
    name = "lllyasviel/control_v11p_sd15_softedge"
    assert pipe._annotator_for(name) is tag
    assert pipe.prepare_controlnet_input_image(name, img)[0] == "s"
    assert pipe._batch_annotator(name, [img])([img])[0] == "s"
    assert pipe.prepare_controlnet_input_image("lllyasviel/sd-controlnet-openpose", img) is img


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
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    from controlanimate_amd import kernels as K
    for fn in ("softedge_prep", "relu", "dwconv_k", "maxpool2x2", "pdc_block", "pdc_block_supported", "cdcm_dil4", "csam_reduce", "softedge_fuse"):
        assert callable(getattr(K, fn))
    from controlanimate_amd import _build
    from controlanimate_amd.context import dispatch
    assert "ca_softedge.hip" in _build.SOURCES and isinstance(dispatch.pdc_block_fused, bool)
    assert lib.ca_pdc_block_supported(64, 3) == 1 and lib.ca_pdc_block_supported(64, 5) == 1
    assert lib.ca_pdc_block_supported(128, 3) == 0 and lib.ca_pdc_block_supported(64, 7) == 0


def test_entry_points_reject_bad_arguments_without_a_launch(capi):
    lib = capi.lib()
    fake, far, odd = C.c_void_p(0x1000), C.c_void_p(0x40000000), C.c_void_p(0x1004)  # never dereferenced: validation fails first

    def expect(rc, who):
        assert rc < 0 and who.encode() in lib.ca_last_error(), (rc, lib.ca_last_error())

    who = "ca_softedge_prep"
    expect(lib.ca_softedge_prep(None, fake, 1, 8, 8, 1, None), who)
    expect(lib.ca_softedge_prep(fake, fake, 0, 8, 8, 1, None), who)
    expect(lib.ca_softedge_prep(fake, fake, 1, 8, 8, 2, None), who)                          # dtype
    expect(lib.ca_softedge_prep(fake, odd, 1, 8, 8, 1, None), who)
    expect(lib.ca_softedge_prep(fake, fake, 64, 8192, 8192, 1, None), who)                   # 2^32 pixels
    who = "ca_relu"
    expect(lib.ca_relu(fake, None, 64, 1, None), who)
    expect(lib.ca_relu(fake, fake, 60, 1, None), who)                                        # numel % 8
    expect(lib.ca_relu(fake, odd, 64, 1, None), who)
    who = "ca_dwconv_k"
    expect(lib.ca_dwconv_k(fake, fake, None, 1, 8, 8, 64, 3, 1, 1, None), who)
    expect(lib.ca_dwconv_k(fake, fake, far, 1, 8, 8, 264, 3, 1, 1, None), who)               # c > 256
    expect(lib.ca_dwconv_k(fake, fake, far, 1, 8, 8, 60, 3, 1, 1, None), who)                # c % 8
    expect(lib.ca_dwconv_k(fake, fake, far, 1, 8, 8, 64, 4, 1, 1, None), who)                # ksize
    expect(lib.ca_dwconv_k(fake, fake, far, 1, 8, 8, 64, 7, 1, 1, None), who)
    expect(lib.ca_dwconv_k(fake, fake, far, 1, 8, 8, 64, 3, 2, 1, None), who)                # relu
    expect(lib.ca_dwconv_k(fake, fake, far, 1, 8, 8, 64, 3, 1, 2, None), who)                # dtype
    expect(lib.ca_dwconv_k(fake, fake, fake, 1, 8, 8, 64, 3, 1, 1, None), who)               # in place
    expect(lib.ca_dwconv_k(fake, fake, C.c_void_p(0x1100), 1, 8, 8, 64, 3, 1, 1, None), who)  # overlapping
    who = "ca_maxpool2x2"
    expect(lib.ca_maxpool2x2(fake, None, 1, 8, 8, 64, 1, None), who)
    expect(lib.ca_maxpool2x2(fake, far, 1, 7, 8, 64, 1, None), who)
    expect(lib.ca_maxpool2x2(fake, far, 1, 8, 9, 64, 1, None), who)
    expect(lib.ca_maxpool2x2(fake, far, 1, 8, 8, 60, 1, None), who)
    who = "ca_pdc_block"
    expect(lib.ca_pdc_block(fake, fake, None, far, 1, 8, 8, 64, 3, 1, None), who)
    expect(lib.ca_pdc_block(fake, fake, fake, far, 1, 8, 8, 128, 3, 1, None), who)           # c
    expect(lib.ca_pdc_block(fake, fake, fake, far, 1, 8, 8, 64, 4, 1, None), who)            # ksize
    expect(lib.ca_pdc_block(fake, fake, fake, fake, 1, 8, 8, 64, 3, 1, None), who)           # in place
    expect(lib.ca_pdc_block(fake, fake, fake, C.c_void_p(0x1100), 1, 8, 8, 64, 5, 1, None), who)   # overlapping
    expect(lib.ca_pdc_block(fake, odd, fake, far, 1, 8, 8, 64, 3, 1, None), who)
    expect(lib.ca_pdc_block(fake, fake, fake, far, 1, 8, 8, 64, 3, 2, None), who)            # dtype
    who = "ca_cdcm_dil4"
    expect(lib.ca_cdcm_dil4(fake, None, far, 1, 8, 8, 32, 1, None), who)
    expect(lib.ca_cdcm_dil4(fake, fake, far, 1, 8, 8, 64, 1, None), who)                     # c
    expect(lib.ca_cdcm_dil4(fake, fake, fake, 1, 8, 8, 32, 1, None), who)                    # in place
    expect(lib.ca_cdcm_dil4(fake, fake, far, 0, 8, 8, 32, 1, None), who)
    who = "ca_csam_reduce"
    t, r, s = C.c_void_p(0x100000), C.c_void_p(0x200000), C.c_void_p(0x300000)
    expect(lib.ca_csam_reduce(fake, fake, fake, fake, fake, None, t, r, s, 1, 8, 8, 32, 1, None), who)
    expect(lib.ca_csam_reduce(fake, fake, fake, fake, fake, fake, t, r, s, 1, 8, 8, 24, 1, None), who)   # c
    expect(lib.ca_csam_reduce(fake, fake, fake, fake, fake, fake, t, r, t, 1, 8, 8, 32, 1, None), who)   # side over the scratch
    expect(lib.ca_csam_reduce(odd, fake, fake, fake, fake, fake, t, r, s, 1, 8, 8, 32, 1, None), who)
    who = "ca_softedge_fuse"
    expect(lib.ca_softedge_fuse(fake, fake, fake, None, fake, 1, 64, 128, 0, None, fake, None, 1, 2, None), who)   # a side map
    expect(lib.ca_softedge_fuse(fake, fake, fake, fake, None, 1, 64, 128, 0, None, fake, None, 1, 2, None), who)   # the classifier
    expect(lib.ca_softedge_fuse(fake, fake, fake, fake, fake, 1, 64, 128, 0, None, None, None, 1, 2, None), who)   # no output
    expect(lib.ca_softedge_fuse(fake, fake, fake, fake, fake, 1, 60, 128, 0, None, fake, None, 1, 2, None), who)   # h % 8
    expect(lib.ca_softedge_fuse(fake, fake, fake, fake, fake, 1, 64, 128, 2, None, fake, None, 1, 2, None), who)   # safe
    expect(lib.ca_softedge_fuse(fake, fake, fake, fake, fake, 1, 64, 128, 0, None, fake, None, 3, 2, None), who)   # rep
    expect(lib.ca_softedge_fuse(fake, fake, fake, fake, fake, 1, 64, 128, 0, None, fake, fake, 1, 0, None), who)   # a bf16 control tensor
    expect(lib.ca_softedge_fuse(fake, fake, fake, fake, fake, 1, 64, 128, 0, None, fake, odd, 1, 2, None), who)    # alignment
