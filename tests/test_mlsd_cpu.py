"""CPU: the specification of the M-LSD annotator (tests/mlsd_ref.py), MlsdAnnotator's key table, BatchNorm folding, loading and input
checks, the numpy line iterator on hand-worked lines, the numpy decode against the torch formulation, the annotator lookup of the
ControlNet pipeline, and the argument checks of the entry points added to ABI v16 for it (no launch, no GPU)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlsd_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ca_mlsd_prep", "ca_dwconv3x3", "ca_upsample2x_bilinear_ac", "ca_conv3x3_dil", "ca_mlsd_decode_workspace_bytes", "ca_mlsd_decode", "ca_mlsd_draw"]


@pytest.fixture(scope="module")
def capi():
    from controlanimate_amd import _build, _capi
    _build.build(verbose=False)
    return _capi


@pytest.fixture(scope="module")
def sd():
    return mlsd_ref.mlsd_state_dict(seed=3)   # out_scale=None: centre logits of standard deviation 2


# ---- the key table ---------------------------------------------------------------------------------------------------------------
def test_key_table_is_the_restated_network(sd):
    from controlanimate_amd.mlsd import backbone_blocks, mlsd_key_shapes
    want = mlsd_key_shapes()
    net = mlsd_ref.MobileV2_MLSD_Large()
    assert {k: tuple(v.shape) for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")} == want
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert want["backbone.features.0.0.weight"] == (32, 4, 3, 3) and want["backbone.features.1.conv.0.0.weight"] == (32, 1, 3, 3)
    assert want["backbone.features.2.conv.0.0.weight"] == (96, 16, 1, 1) and want["backbone.features.13.conv.2.weight"] == (96, 576, 1, 1)
    assert want["block15.conv1.0.weight"] == (64, 96, 1, 1) and want["block15.conv2.0.weight"] == (64, 64, 1, 1)
    assert want["block21.conv2.0.weight"] == (64, 16, 1, 1) and want["block22.conv1.0.weight"] == (128, 128, 3, 3)
    assert want["block23.conv3.weight"] == (16, 64, 1, 1) and "backbone.features.14.conv.0.0.weight" not in want
    blocks = backbone_blocks()
    assert len(blocks) == 13 and [b[0] for b in blocks] == list(range(1, 14))
    assert [b[4] for b in blocks] == [1, 2, 1, 2, 1, 1, 2, 1, 1, 1, 1, 1, 1] and max(b[2] for b in blocks) == 576
    assert [b[0] for b in blocks if b[6]] == [3, 5, 6, 8, 9, 10, 12, 13]      # the blocks with a skip


def test_state_dict_checks_name_the_offender(sd):
    from controlanimate_amd.mlsd import MlsdAnnotator, check_state_dict
    check_state_dict(sd)
    missing = {k: v for k, v in sd.items() if k != "block18.conv2.1.running_var"}
    with pytest.raises(KeyError, match=re.escape("block18.conv2.1.running_var")):
        check_state_dict(missing)
    with pytest.raises(KeyError):
        MlsdAnnotator(missing)
    with pytest.raises(ValueError, match=re.escape("block24.conv1.0.weight")):
        MlsdAnnotator(dict(sd, **{"block24.conv1.0.weight": torch.zeros(1)}))
    with pytest.raises(ValueError, match=re.escape("block23.conv3.weight")):
        MlsdAnnotator(dict(sd, **{"block23.conv3.weight": torch.zeros(9, 64, 1, 1)}))
    # layers past features.13 that a checkpoint may keep, and the BatchNorm counters, are ignored
    extra = dict(sd, **{"backbone.features.14.conv.0.0.weight": torch.zeros(576, 96, 1, 1), "backbone.features.0.1.num_batches_tracked": torch.tensor(7),
                        "block15.conv1.1.num_batches_tracked": torch.tensor(7)})
    check_state_dict(extra)
    a, b = MlsdAnnotator(extra), MlsdAnnotator(sd)
    assert torch.equal(a._host["head"][0], b._host["head"][0]) and torch.equal(a._host["stem"][0], b._host["stem"][0])
    with pytest.raises(TypeError):
        MlsdAnnotator(sd, dtype=torch.float32)
    with pytest.raises(NotImplementedError):
        MlsdAnnotator(sd, detect_resolution=512, image_resolution=768)
    with pytest.raises(ValueError):
        MlsdAnnotator(sd, thr_v=1.5)


def test_packing(sd):
    from controlanimate_amd.mlsd import MlsdAnnotator, fold_bn, pack_depthwise
    ann = MlsdAnnotator(sd)
    stem = ann._host["stem"][0]
    assert tuple(stem.shape) == (32, 3, 3, 8) and (stem[..., 4:] == 0).all() and stem.dtype == torch.float16
    w, _ = fold_bn(sd, "backbone.features.0.0", "backbone.features.0.1")
    assert torch.equal(stem[..., :4], w.permute(0, 2, 3, 1).to(torch.float16))
    head_w, head_b = ann._host["head"]
    assert tuple(head_w.shape) == (8, 64) and (head_w[5:] == 0).all() and (head_b[5:] == 0).all()
    assert torch.equal(head_w[:5], sd["block23.conv3.weight"].reshape(16, 64)[7:12].to(torch.float16)) and torch.equal(head_b[:5], sd["block23.conv3.bias"][7:12])
    dw = torch.arange(16 * 9, dtype=torch.float32).view(16, 1, 3, 3)
    p = pack_depthwise(dw)
    assert tuple(p.shape) == (9, 16) and p.is_contiguous() and p[5, 3] == dw[3, 0, 1, 2]
    with pytest.raises(ValueError):
        pack_depthwise(torch.zeros(16, 2, 3, 3))


def test_bn_folding_equals_the_unfolded_network(sd):
    frames = mlsd_ref.frames_fixture()
    ref = mlsd_ref.tpmap_ref(sd, frames)[..., :5]
    got = mlsd_ref.tpmap_emulated(sd, frames, torch.float32)
    rel = ((got - ref).norm() / ref.norm()).item()
    std = [float(ref[..., c].std()) for c in range(5)]
    print(f"folded against unfolded fp32 network: relative L2 {rel:.3e}; reference std per channel {np.round(std, 2)}")
    assert rel <= 1e-5
    assert 1.9 <= std[0] <= 2.1 and all(0.5 <= s <= 8.0 for s in std[1:])


def test_fp16_storage_emulation_gives_the_error_the_gpu_bar_is_judged_against(sd):
    """Prints the tpMap error of the chain with every stored activation rounded to fp16 / bf16 (weights folded, then rounded) against the
    fp32 network with the weights rounded to that type: 1.9e-3 (fp16) and 1.2e-2 (bf16) when this was written, 5.4 x and 6.6 x under
    the bars of tests/test_mlsd_gpu.py (1e-2 / 8e-2).  On the GPU test's seed 11 the emulation gives 3.4e-3 / 2.1e-2 and the device measured
    3.2e-3 / 2.5e-2."""
    frames = mlsd_ref.frames_fixture()
    for dtype, bar in ((torch.float16, 1e-2), (torch.bfloat16, 8e-2)):
        rounded = {k: (v.to(dtype).float() if v.dim() == 4 else v) for k, v in sd.items()}
        ref = mlsd_ref.tpmap_ref(rounded, frames)[..., :5]
        got = mlsd_ref.tpmap_emulated(rounded, frames, dtype)
        rel = ((got - ref).norm() / ref.norm()).item()
        print(f"{dtype} storage emulation: relative L2 {rel:.3e} (GPU bar {bar:.0e}, {bar / rel:.1f} x under)")
        assert rel <= bar


# ---- loading ---------------------------------------------------------------------------------------------------------------------
def test_loader_is_file_only(sd, tmp_path):
    from controlanimate_amd.annotators import MlsdAnnotator
    torch.save(sd, tmp_path / "mlsd_large_512_fp32.pth")
    a = MlsdAnnotator.from_pretrained(tmp_path)
    b = MlsdAnnotator(str(tmp_path / "mlsd_large_512_fp32.pth"), thr_v=0.2)
    c = MlsdAnnotator(sd)
    assert torch.equal(a._host["head"][0], c._host["head"][0]) and torch.equal(b._host["C"][0][0], c._host["C"][0][0]) and b.thr_v == 0.2
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(FileNotFoundError, match=re.escape(str(empty / "mlsd_large_512_fp32.pth"))):
        MlsdAnnotator.from_pretrained(empty)
    with pytest.raises(FileNotFoundError, match="nothing is ever downloaded"):
        MlsdAnnotator("lllyasviel/Annotators")
    src = open(os.path.join(ROOT, "controlanimate_amd", "mlsd.py")).read()
    assert not re.search(r"hf_hub|huggingface_hub|urllib|requests|http", src)


# ---- MlsdAnnotator: input checks before the device -------------------------------------------------------------------------------------
def test_annotator_checks_types_sizes_and_scope_before_the_device(capi, sd, monkeypatch):
    from PIL import Image
    from controlanimate_amd.annotators import MlsdAnnotator
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "LIB_PATH", "/nonexistent/libcontrolanimate_hip.so")   # touching the device would raise CAHipUnavailable
    ann = MlsdAnnotator(sd, detect_resolution=64, image_resolution=64)
    u8, f32 = np.zeros((64, 128, 3), np.uint8), np.zeros((64, 128, 3), np.float32)
    for call in (ann, lambda x: ann.edges([x]), lambda x: ann.annotate_batch([x]), lambda x: ann.tpmap([x])):
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
    with pytest.raises(NotImplementedError, match="128 x 128"):                     # min(H, W) != detect_resolution: the detector would resample
        ann.annotate_batch(torch.zeros((2, 128, 128, 3), dtype=torch.uint8))
    with pytest.raises(NotImplementedError):
        ann(np.zeros((128, 72), np.uint8))
    big = MlsdAnnotator(sd)                                                         # the defaults: 512
    with pytest.raises(NotImplementedError, match="detect_resolution"):
        big.edges([u8])
    for ok in (np.zeros((512, 512, 3), np.uint8), np.zeros((512, 768, 3), np.uint8), np.zeros((768, 512), np.uint8)):
        with pytest.raises(capi.CAHipUnavailable):
            big.edges([ok])
    for ok in (u8, Image.new("RGB", (128, 64)), Image.new("L", (64, 192))):
        with pytest.raises(capi.CAHipUnavailable):
            ann.edges([ok])
    with pytest.raises(capi.CAHipUnavailable):
        ann(u8)


def test_annotator_needs_a_gpu(capi, sd, monkeypatch):
    from controlanimate_amd.annotators import MlsdAnnotator
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(capi.CAHipUnavailable):
        MlsdAnnotator(sd, detect_resolution=64, image_resolution=64).annotate_batch([np.zeros((64, 64, 3), np.uint8)])


def test_chunking_keeps_the_largest_operand_addressable(sd):
    from controlanimate_amd.annotators import MlsdAnnotator
    ann = MlsdAnnotator(sd)
    per_frame = (512 // 2) * (768 // 2) * 128 * 2      # the 128-channel concatenation at half resolution
    assert ann.chunk_frames(512, 768) == (0x7FFFFF00 - 1) // per_frame == 85      # a 16-frame window is one pass
    ann.max_activation_bytes = per_frame - 1
    with pytest.raises(ValueError):
        ann.chunk_frames(512, 768)


# ---- draw_ref on hand-worked lines -------------------------------------------------------------------------------------------------------
def _px(x1, y1, x2, y2, w=16, h=12):
    return mlsd_ref.line_pixels(w, h, x1, y1, x2, y2)


def test_draw_ref_axis_aligned_and_diagonal():
    assert _px(2, 3, 6, 3) == [(2, 3), (3, 3), (4, 3), (5, 3), (6, 3)]
    assert _px(6, 3, 2, 3) == [(2, 3), (3, 3), (4, 3), (5, 3), (6, 3)]                      # walked left to right
    assert _px(4, 1, 4, 5) == [(4, 1), (4, 2), (4, 3), (4, 4), (4, 5)]
    assert _px(4, 5, 4, 1) == [(4, 5), (4, 4), (4, 3), (4, 2), (4, 1)]                      # dx == 0: no swap, the walk goes up
    assert _px(1, 1, 5, 5) == [(1, 1), (2, 2), (3, 3), (4, 4), (5, 5)]
    assert _px(1, 5, 5, 1) == [(1, 5), (2, 4), (3, 3), (4, 2), (5, 1)]
    assert _px(7, 7, 7, 7) == [(7, 7)]                                                     # zero length: one pixel


def test_draw_ref_shallow_and_steep_in_all_sign_combinations():
    # shallow, dx = 6, dy = 2: err = 2 at the first pixel, then -2 (the minor axis advances after this pixel), 6, 2, -2 (advances), 6, 2
    assert _px(0, 0, 6, 2) == [(0, 0), (1, 0), (2, 1), (3, 1), (4, 1), (5, 2), (6, 2)]
    assert _px(0, 2, 6, 0) == [(0, 2), (1, 2), (2, 1), (3, 1), (4, 1), (5, 0), (6, 0)]
    # steep, dx = 2, dy = 6: the roles are swapped
    assert _px(0, 0, 2, 6) == [(0, 0), (0, 1), (1, 2), (1, 3), (1, 4), (2, 5), (2, 6)]
    assert _px(0, 6, 2, 0) == [(0, 6), (0, 5), (1, 4), (1, 3), (1, 2), (2, 1), (2, 0)]
    # reversed endpoints: the iterator starts from the left point, so the pixels are the same
    for a, b in (((0, 0), (6, 2)), ((0, 2), (6, 0)), ((0, 0), (2, 6)), ((0, 6), (2, 0)), ((1, 9), (14, 3)), ((3, 11), (5, 0))):
        assert sorted(_px(*a, *b)) == sorted(_px(*b, *a)), (a, b)
    m1, m2 = mlsd_ref.draw_ref([[1, 9, 14, 3]], 12, 16), mlsd_ref.draw_ref([[14, 3, 1, 9]], 12, 16)
    assert np.array_equal(m1, m2) and m1.sum() == 255 * 14 and set(np.unique(m1)) == {0, 255}


def test_draw_ref_clipping():
    # both ends outside on opposite sides: a horizontal line through the image
    assert _px(-5, 4, 30, 4) == [(x, 4) for x in range(16)]
    # the diagonal y = x - 3 from (-4, -7) to (20, 17): clipped to (3, 0) .. (14, 11)
    assert _px(-4, -7, 20, 17) == [(3 + i, i) for i in range(12)]
    # fully outside draws nothing: both left, both below, and a line that misses the corner
    assert _px(-9, 2, -1, 8) == [] and _px(3, 12, 9, 40) == [] and _px(-6, 3, 3, -8) == []
    assert mlsd_ref.draw_ref([[-9, 2, -1, 8], [3, 12, 9, 40]], 12, 16).sum() == 0
    # one end far outside: (2, 2) -> (2 + 10^6, 2 + 5 * 10^5), slope 1/2.  First y is moved to the bottom edge 11: x2 += trunc(-499991 * 10^6 /
    # (5 * 10^5)) = -999982 -> (20, 11); then x to the right edge 15 with the UPDATED end point: y2 += trunc(-5 * 9 / 18) = -2 -> (15, 9)
    ok, x1, y1, x2, y2 = mlsd_ref.clip_line(16, 12, 2, 2, 1000002, 500002)
    assert ok and (x1, y1, x2, y2) == (2, 2, 15, 9)
    px = _px(2, 2, 1000002, 500002)
    assert px[0] == (2, 2) and px[-1] == (15, 9) and len(px) == 14
    # clipLine truncates toward zero: from (-3, 0) to (5, 3) the left edge is met at y = trunc(3 * 3 / 8) = 1
    assert mlsd_ref.clip_line(16, 12, -3, 0, 5, 3) == (True, 0, 1, 5, 3)


# ---- decode_ref ------------------------------------------------------------------------------------------------------------------------
def test_decode_cases_are_decided_and_equal_the_torch_formulation():
    cases = mlsd_ref.decode_cases()
    assert set(cases) == {"few", "plateau", "many", "short"}
    for name, tp in cases.items():
        assert tp.shape == (32, 64, 8) and tp.dtype == np.float32
        assert mlsd_ref.decided(tp), name
        got, torch_way = mlsd_ref.decode_ref(tp), mlsd_ref.decode_topk_torch(tp)
        if name == "plateau":   # equal scores: torch.topk's order among them is its own
            assert sorted(map(tuple, got)) == sorted(map(tuple, torch_way))
        else:
            assert np.array_equal(got, torch_way), name


def test_decode_ref_properties():
    cases = mlsd_ref.decode_cases()
    assert len(mlsd_ref.decode_ref(cases["few"])) == 40                                    # fewer than 200 candidates: all of them
    tp = cases["few"]
    first = mlsd_ref.decode_ref(tp)[0]                                                     # the highest peak: i = 39 at (y 11, x 56)
    assert tuple(first) == tuple(int(2.0 * (p + float(d))) for p, d in ((56, tp[11, 56, 1]), (11, tp[11, 56, 2]), (56, tp[11, 56, 3]), (11, tp[11, 56, 4])))
    plateau = mlsd_ref.decode_ref(cases["plateau"])                                        # every pixel of the 3 x 4 plateau, and the ramp's maximum alone
    assert len(plateau) == 13
    many = cases["many"]
    kept = mlsd_ref.decode_ref(many)
    assert len(kept) == 200
    peaks = np.sort(many[..., 0][many[..., 0] > -7.0])[::-1]
    assert len(peaks) == 336
    cut = peaks[199]                                                                       # the dropped ones are the 136 lowest
    want = [(y, x) for y, x in zip(*np.nonzero(many[..., 0] >= cut))]
    assert len(want) == 200
    order = sorted(want, key=lambda p: -many[p[0], p[1], 0])
    assert [tuple(r) for r in kept[:5]] == [tuple(mlsd_ref._endpoint(q, many[y, x, c]) for q, c in ((x, 1), (y, 2), (x, 3), (y, 4))) for y, x in order[:5]]
    short = mlsd_ref.decode_ref(cases["short"])                                            # four of the top 200 have dist <= thr_d: dropped, not replaced
    assert len(short) == 196
    assert mlsd_ref.decided(many) and not mlsd_ref.decided(np.where(np.arange(8) == 0, np.float32(np.log(0.1 / 0.9)), many).astype(np.float32))
    sat = mlsd_ref.saturated_case()                                                        # one plateau of heat 1.0: the first 200 pixels by index
    got = mlsd_ref.decode_ref(sat)
    assert len(got) == 200 and tuple(got[64]) == tuple(mlsd_ref._endpoint(q, sat[1, 0, c]) for q, c in ((0, 1), (1, 2), (0, 3), (1, 4)))


def test_detector_restatement(sd):
    frames = mlsd_ref.frames_fixture()
    out = mlsd_ref.mlsd_detect(sd, frames[0])
    assert out.dtype == np.uint8 and out.shape == (64, 128, 3) and np.array_equal(out[..., 0], out[..., 1]) and set(np.unique(out)) <= {0, 255}
    assert 0 < (out[..., 0] == 255).mean() < 0.9
    x = mlsd_ref.to_input(frames[:1])
    assert tuple(x.shape) == (1, 4, 64, 128) and torch.all(x[:, 3] == np.float32(1 / 127.5 - 1.0))
    with pytest.raises(NotImplementedError):
        mlsd_ref.mlsd_detect(sd, np.zeros((72, 128, 3), np.uint8))


# ---- the annotator lookup --------------------------------------------------------------------------------------------------------------
def test_lookup_mlsd_serves_both_controlnet_names():
    from controlanimate_amd.controlresiduals_pipeline import MultiControlNetResidualsPipeline

    class Tag:
        def __call__(self, image):
            return ("m", image)

        def annotate_batch(self, frames, out=None, rep=1, dtype=None):
            return ("m", "batch")

    pipe = MultiControlNetResidualsPipeline.__new__(MultiControlNetResidualsPipeline)   # the lookup alone: no nets, no device
    pipe.annotators = {"mlsd": Tag()}
    img = np.zeros((8, 8, 3), np.uint8)
    for name in ("lllyasviel/control_v11p_sd15_mlsd", "lllyasviel/sd-controlnet-mlsd"):
        assert pipe.prepare_controlnet_input_image(name, img)[0] == "m"
        assert pipe._batch_annotator(name, [img])([img])[0] == "m"
    assert pipe.prepare_controlnet_input_image("lllyasviel/sd-controlnet-openpose", img) is img


# ---- the entry points --------------------------------------------------------------------------------------------------------------
def test_abi_is_still_16_and_header_binding_library_agree(capi):
    assert capi.ABI_VERSION == 16 and capi.CA_ACT_RELU6 == 5 and capi.CA_MLSD_TOPK == 200
    lib = capi.lib()
    assert lib.ca_abi_version() == 16
    header = open(os.path.join(ROOT, "include", "controlanimate_hip.h")).read()
    assert re.search(r"#define CA_ACT_RELU6 5\b", header) and re.search(r"#define CA_MLSD_TOPK 200\b", header)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert name in capi.SYMBOLS and getattr(lib, name) is not None
        decl = re.search(r"\b(?:int|int64_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert decl, f"{name} is not declared in the header"
        assert len([a for a in decl.group(1).split(",") if a.strip()]) == len(capi.SYMBOLS[name][1]), name   # one binding type per C parameter
    from controlanimate_amd import kernels as K
    for fn in ("mlsd_prep", "dwconv3x3", "upsample2x_bilinear_ac", "conv3x3_dil", "mlsd_decode", "mlsd_draw", "mlsd_decode_workspace_bytes"):
        assert callable(getattr(K, fn))
    assert K.ACT_RELU6 == 5
    from controlanimate_amd import _build
    assert "ca_mlsd.hip" in _build.SOURCES


def test_entry_points_reject_bad_arguments_without_a_launch(capi):
    lib = capi.lib()
    fake, odd = C.c_void_p(0x1000), C.c_void_p(0x1004)  # never dereferenced: validation fails first

    def expect(rc, who):
        assert rc < 0 and who.encode() in lib.ca_last_error(), (rc, lib.ca_last_error())

    who = "ca_mlsd_prep"
    expect(lib.ca_mlsd_prep(None, fake, 1, 8, 8, 1, None), who)
    expect(lib.ca_mlsd_prep(fake, fake, 0, 8, 8, 1, None), who)
    expect(lib.ca_mlsd_prep(fake, fake, 1, 8, 8, 2, None), who)                              # dtype
    expect(lib.ca_mlsd_prep(fake, odd, 1, 8, 8, 1, None), who)
    expect(lib.ca_mlsd_prep(fake, fake, 64, 8192, 8192, 1, None), who)                       # 2^32 pixels
    who = "ca_dwconv3x3"
    expect(lib.ca_dwconv3x3(fake, fake, None, fake, 1, 8, 8, 32, 1, 1, 1, None), who)        # bias
    expect(lib.ca_dwconv3x3(fake, fake, fake, fake, 1, 8, 8, 8, 1, 1, 1, None), who)         # c < 16
    expect(lib.ca_dwconv3x3(fake, fake, fake, fake, 1, 8, 8, 584, 1, 1, 1, None), who)       # c > 576
    expect(lib.ca_dwconv3x3(fake, fake, fake, fake, 1, 8, 8, 36, 1, 1, 1, None), who)        # c % 8
    expect(lib.ca_dwconv3x3(fake, fake, fake, fake, 1, 8, 8, 32, 3, 1, 1, None), who)        # stride
    expect(lib.ca_dwconv3x3(fake, fake, fake, fake, 1, 7, 8, 32, 2, 1, 1, None), who)        # stride 2 on an odd height
    expect(lib.ca_dwconv3x3(fake, fake, fake, fake, 1, 8, 9, 32, 2, 1, 1, None), who)        # ... and width
    expect(lib.ca_dwconv3x3(fake, fake, fake, fake, 1, 8, 8, 32, 1, 2, 1, None), who)        # relu6
    expect(lib.ca_dwconv3x3(fake, odd, fake, fake, 1, 8, 8, 32, 1, 1, 1, None), who)
    who = "ca_upsample2x_bilinear_ac"
    expect(lib.ca_upsample2x_bilinear_ac(fake, None, 1, 4, 4, 64, 128, 64, 1, None), who)
    expect(lib.ca_upsample2x_bilinear_ac(fake, fake, 1, 4, 4, 64, 128, 72, 1, None), who)    # col0 + c > ld
    expect(lib.ca_upsample2x_bilinear_ac(fake, fake, 1, 4, 4, 64, 128, 4, 1, None), who)     # col0 % 8
    expect(lib.ca_upsample2x_bilinear_ac(fake, fake, 1, 4, 4, 60, 128, 0, 1, None), who)     # c % 8
    expect(lib.ca_upsample2x_bilinear_ac(fake, fake, 32, 4096, 4096, 64, 128, 0, 1, None), who)   # 2^31 output pixels
    expect(lib.ca_upsample2x_bilinear_ac(fake, fake, 1, 4, 4, 64, 128, 64, 3, None), who)
    who = "ca_conv3x3_dil"
    expect(lib.ca_conv3x3_dil(fake, fake, fake, None, 1, 8, 8, 64, 5, 1, 1, None), who)
    expect(lib.ca_conv3x3_dil(fake, fake, fake, C.c_void_p(0x2000), 1, 8, 8, 128, 5, 1, 1, None), who)   # c
    expect(lib.ca_conv3x3_dil(fake, fake, fake, C.c_void_p(0x2000), 1, 8, 8, 64, 2, 1, 1, None), who)    # dilation
    expect(lib.ca_conv3x3_dil(fake, fake, fake, fake, 1, 8, 8, 64, 5, 1, 1, None), who)                  # in place
    expect(lib.ca_conv3x3_dil(fake, fake, fake, C.c_void_p(0x2000), 1, 8, 8, 64, 5, 2, 1, None), who)    # relu
    assert lib.ca_mlsd_decode_workspace_bytes(2, 32, 64) == 2 * 32 * 64 * 8 and lib.ca_mlsd_decode_workspace_bytes(16, 256, 384) == 16 * 256 * 384 * 8
    assert lib.ca_mlsd_decode_workspace_bytes(0, 32, 64) == 0 and lib.ca_mlsd_decode_workspace_bytes(64, 8192, 8192) == 0
    who = "ca_mlsd_decode"
    expect(lib.ca_mlsd_decode(None, 1, 32, 64, 0.1, 0.1, fake, 1 << 20, fake, fake, None), who)
    expect(lib.ca_mlsd_decode(fake, 1, 32, 64, 0.1, 0.1, fake, 32 * 64 * 8 - 1, fake, fake, None), who)  # workspace too small
    expect(lib.ca_mlsd_decode(fake, 1, 32, 64, -0.1, 0.1, fake, 1 << 20, fake, fake, None), who)         # thr_v
    expect(lib.ca_mlsd_decode(fake, 1, 32, 64, 0.1, float("nan"), fake, 1 << 20, fake, fake, None), who)
    expect(lib.ca_mlsd_decode(fake, 1, 32, 64, 0.1, 0.1, fake, 1 << 20, None, fake, None), who)
    expect(lib.ca_mlsd_decode(odd, 1, 32, 64, 0.1, 0.1, fake, 1 << 20, fake, fake, None), who)
    who = "ca_mlsd_draw"
    expect(lib.ca_mlsd_draw(fake, fake, 1, 64, 128, None, None, 1, 2, None), who)                        # the map
    expect(lib.ca_mlsd_draw(fake, None, 1, 64, 128, fake, None, 1, 2, None), who)
    expect(lib.ca_mlsd_draw(fake, fake, 1, 3, 5, fake, None, 1, 2, None), who)                           # h * w % 4
    expect(lib.ca_mlsd_draw(fake, fake, 1, 64, 128, fake, None, 3, 2, None), who)                        # rep
    expect(lib.ca_mlsd_draw(fake, fake, 1, 64, 128, fake, fake, 1, 0, None), who)                        # a bf16 control tensor
    expect(lib.ca_mlsd_draw(fake, fake, 1, 64, 128, fake, odd, 1, 2, None), who)                         # alignment
