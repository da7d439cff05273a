"""CPU: the NormalBae annotator's specification (tests/normalbae_ref.py) against transformers' EfficientNetModel through the recorded
fixture, the tensor list, the state-dict and frame checks of controlanimate_amd/normalbae.py, the detector's tail, and the condition on
the seeded inputs that the GPU tests rely on.

test_tail_truncates and test_seeded_inputs_keep_every_normalisation_away_from_zero check the specification and the GPU tests' inputs alone:
they need tests/normalbae_ref.py and no product code (the second reads its seed and frames from tests/test_normalbae_gpu.py)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normalbae_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_SEED = 0   # tests/test_normalbae_gpu.py: SEED.  Seeds 0 and 1 were tried on the CPU; both hold the condition below with a margin (the
#                smallest norm / median over the four stages: tiny 0.37 / 0.49, B5 0.40 / 0.52); 0 is the one used.


def _count(shapes, params_only=False):
    return sum(int(np.prod(s)) for k, s in shapes.items() if not (params_only and k.rsplit(".", 1)[1].startswith("running_")))


def test_specification_encoder_reproduces_the_transformers_fixture():
    """fp32 against fp32: only the summation order differs (1e-5, the figure of tests/test_depth_gpu.py's fp32 check)."""
    frames, taps, sd, versions = R.load_fixture()
    enc = R.Encoder(R.TINY).eval()
    missing = enc.load_state_dict({k[len("encoder."):]: v for k, v in sd.items()}, strict=False)
    assert not missing.unexpected_keys and all(k.endswith("num_batches_tracked") for k in missing.missing_keys)
    with torch.no_grad():
        feats = enc(R.preprocess(frames))
    assert len(feats) == 12
    got = [feats[i] for i in (4, 5, 6, 8, 11)]
    # the tap indices, by shape: stages 0, 1, 2 and 4 at 1/2, 1/4, 1/8, 1/16 and conv_head's output at 1/32
    assert [tuple(t.shape) for t in got] == [(3, 8, 32, 48), (3, 16, 16, 24), (3, 24, 8, 12), (3, 56, 4, 6), (3, 640, 2, 3)]
    assert [tuple(t.shape) for t in taps] == [tuple(t.shape) for t in got]
    rels = [((a - b).norm() / b.norm()).item() for a, b in zip(got, taps)]
    print(f"specification against {versions}: {['%.2e' % r for r in rels]}")
    assert max(rels) <= 1e-5


def test_b5_tap_shapes_and_stride_table():
    from controlanimate_amd import normalbae as nb
    assert tuple(nb.B5) == tuple(R.B5) and nb.blocks_of(nb.B5) == R.blocks_of(R.B5) and nb.TAP_STAGES == R.TAP_STAGES
    assert nb.decoder_widths(nb.B5) == ([24, 40, 64, 176], [1024, 512, 256, 128])
    feats_c = [R.B5.stages[s][0] for s in R.TAP_STAGES] + [R.B5.head]
    assert feats_c == [24, 40, 64, 176, 2048]
    blocks = R.blocks_of(R.B5)
    assert len(blocks) == 39 and [b[7] for b in blocks if b[1] == 0] == [12, 6, 10, 16, 32, 44, 76]   # the SE widths of each stage's first block
    enc = R.Encoder(R.B5).eval()
    with torch.no_grad():
        feats = enc(torch.zeros(1, 3, 64, 64))
    assert [tuple(feats[i].shape[1:]) for i in (4, 5, 6, 8, 11)] == [(24, 32, 32), (40, 16, 16), (64, 8, 8), (176, 4, 4), (2048, 2, 2)]


def test_key_shapes_count_against_transformers_b5():
    from transformers import EfficientNetConfig, EfficientNetModel
    from controlanimate_amd import normalbae as nb
    model = EfficientNetModel(EfficientNetConfig(width_coefficient=1.6, depth_coefficient=2.2, hidden_dim=2048))
    hf = sum(p.numel() for p in model.parameters())
    assert hf == 28_340_784 and len(model.encoder.blocks) == 39
    shapes = R.key_shapes(R.B5)
    assert shapes == nb.normalbae_key_shapes(nb.B5) and R.key_shapes(R.TINY) == nb.normalbae_key_shapes(nb.Geometry(*R.TINY))
    enc = {k: s for k, s in shapes.items() if k.startswith("encoder.")}
    assert _count(enc, params_only=True) == hf - 2 * 2048          # the detector drops top_bn (bn2 behind conv_head): weight and bias
    # the decoder, derived: conv2, four UpSampleBN (two 3x3 convolutions with bias, two BatchNorms with weight and bias), res8, three MLPs
    conv2 = 2048 * 2048 + 2048
    ups = sum(9 * cin * c + c + 2 * c + 9 * c * c + c + 2 * c for cin, c in ((2048 + 176, 1024), (1024 + 64, 512), (512 + 40, 256), (256 + 24, 128)))
    res8 = 9 * 512 * 4 + 4
    mlps = sum((c + 4) * 128 + 128 + 2 * (128 * 128 + 128) + 128 * 4 + 4 for c in (512, 256, 128))
    dec = {k: s for k, s in shapes.items() if k.startswith("decoder.")}
    assert _count(dec, params_only=True) == conv2 + ups + res8 + mlps == 44_081_552
    assert len(shapes) == 808


def test_check_state_dict_names_the_tensor():
    from controlanimate_amd import normalbae as nb
    geo = nb.Geometry(*R.TINY)
    sd = {k: torch.zeros(s) for k, s in nb.normalbae_key_shapes(geo).items()}
    nb.check_state_dict(sd, geo)
    nb.check_state_dict({**sd, "encoder.original_model.bn2.weight": torch.zeros(640), "encoder.original_model.classifier.weight": torch.zeros(3, 640),
                         "encoder.original_model.bn1.num_batches_tracked": torch.zeros(())}, geo)      # what the detector never runs is ignored
    gone = dict(sd)
    del gone["decoder.up2._net.3.weight"]
    with pytest.raises(KeyError, match=r"decoder\.up2\._net\.3\.weight"):
        nb.check_state_dict(gone, geo)
    with pytest.raises(ValueError, match=r"unexpected tensor 'decoder\.up5\._net\.0\.weight'"):
        nb.check_state_dict({**sd, "decoder.up5._net.0.weight": torch.zeros(1)}, geo)
    with pytest.raises(ValueError, match=r"encoder\.original_model\.blocks\.3\.1\.se\.conv_reduce\.weight.*expected"):
        nb.check_state_dict({**sd, "encoder.original_model.blocks.3.1.se.conv_reduce.weight": torch.zeros(12, 240, 1, 1)}, geo)
    # the checkpoint's layout: {"model": state dict}, DataParallel's prefix stripped
    ann = nb.NormalBaeAnnotator({"model": {"module." + k: v for k, v in R.tiny_state_dict(0).items()}}, detect_resolution=64, geometry=geo)
    assert ann._bytes_per_pixel == 256


def test_scope_and_frame_errors_fire_before_the_device(monkeypatch):
    from controlanimate_amd import normalbae as nb
    geo = nb.Geometry(*R.TINY)
    sd = R.tiny_state_dict(0)
    ann = nb.NormalBaeAnnotator(sd, geometry=geo)       # detect_resolution = 512
    monkeypatch.setattr(ann, "_device", lambda: (_ for _ in ()).throw(AssertionError("the device was touched")))
    for h, w in ((512, 520), (500, 512), (576, 768)):
        with pytest.raises(NotImplementedError):
            ann._check_size(h, w)
        with pytest.raises(NotImplementedError):
            ann.normals([np.zeros((h, w, 3), np.uint8)])
    ann._check_size(512, 768)
    ann._check_size(768, 512)
    ann._check_size(512, 512)
    with pytest.raises(TypeError):
        ann.normals([np.zeros((512, 512, 3), np.float32)])
    with pytest.raises(ValueError):
        ann.normals([np.zeros((512, 512, 3), np.uint8), np.zeros((512, 768, 3), np.uint8)])
    with pytest.raises(ValueError):
        ann.normals([np.zeros((512, 512, 4), np.uint8)])
    with pytest.raises(TypeError):
        ann.annotate_batch(torch.zeros((1, 512, 512, 3), dtype=torch.float32))
    with pytest.raises(NotImplementedError):
        nb.NormalBaeAnnotator(sd, geometry=geo, detect_resolution=500)
    with pytest.raises(TypeError):
        nb.NormalBaeAnnotator(sd, geometry=geo, dtype=torch.float32)


def test_tail_truncates():
    v = np.array([-1.0, 1.0, 0.0, 0.2, 0.999, -0.999, 2.0, -2.0], np.float32)
    lv = R.tail(torch.from_numpy(np.tile(v, 3).reshape(1, 3, 1, 8)))[0, 0, :, 0]
    want = [0, 255, 127, 153, 254, 0, 255, 0]     # 127.5 -> 127 and 254.87 -> 254: truncation; rounding would give 128 and 255
    assert lv.tolist() == want


@pytest.mark.parametrize("geo", ["tiny", "b5"])
def test_seeded_inputs_keep_every_normalisation_away_from_zero(geo):
    """The condition on the GPU tests' inputs, in fp32: with the seeded weights (rounded to fp16, as the GPU tests use them) the norm of xyz
    in front of each of the four normalisations stays above a quarter of its median over all pixels.  Without it the four cascaded
    normalisations would make parity a test of the seed."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_normalbae_gpu as G
    assert G.SEED == GPU_SEED
    g, sd = (R.TINY, R.tiny_state_dict(GPU_SEED)) if geo == "tiny" else (R.B5, R.seeded_state_dict(R.B5, GPU_SEED))
    net = R.load(g, {k: v.half().float() for k, v in sd.items()})
    for hw in ((64, 64), (64, 128)):
        raws = []
        with torch.no_grad():
            feats = net.encoder(R.preprocess(G._smooth_frames(3, hw[0], hw[1], seed=hw[1])))
            net.decoder(feats, raws)
        ratios = [float(r[:, :3].norm(dim=1).min() / r[:, :3].norm(dim=1).median()) for r in raws]
        peak = max(float(f.abs().max()) for f in feats[1:])
        print(f"{geo} {hw}: smallest norm / median per stage {['%.2f' % r for r in ratios]}; largest encoder activation {peak:.1f}")
        assert len(raws) == 4 and min(ratios) > 0.25 and peak < 100      # activations stay O(1)


def test_abi_constants_and_symbols():
    from controlanimate_amd import _capi as capi
    header = open(os.path.join(ROOT, "include", "controlanimate_hip.h")).read()
    assert capi.ABI_VERSION == 16 and capi.CA_ACT_LEAKY001 == 7 and re.search(r"#define CA_ACT_LEAKY001 7\b", header)
    assert re.search(r"#define CA_ACT_LEAKY02 6\b", header) and re.search(r"#define CA_ACT_RELU 4\b", header)      # the existing codes keep their values
    for name in ("ca_nbae_stem", "ca_dwconv_same", "ca_dwconv_same_partials_floats", "ca_se_gate", "ca_scale_channels", "ca_nbae_cat_pred", "ca_nbae_normalize",
                 "ca_nbae_finish"):
        assert name in capi.SYMBOLS and re.search(rf"\b{name}\s*\(", header)


def test_entry_points_reject_bad_arguments_without_a_gpu():
    import ctypes as C
    from controlanimate_amd import _build, _capi as capi
    _build.build(verbose=False)
    lib = capi.lib()
    fake = C.c_void_p(0x1000)

    def expect(rc, who):
        assert rc < 0 and who.encode() in lib.ca_last_error(), (rc, lib.ca_last_error())

    expect(lib.ca_nbae_stem(fake, fake, fake, fake, 1, 63, 64, 48, 1, None), "ca_nbae_stem")                     # odd height
    expect(lib.ca_nbae_stem(fake, fake, fake, fake, 1, 64, 64, 72, 1, None), "ca_nbae_stem")                     # cout
    expect(lib.ca_dwconv_same(fake, fake, fake, C.c_void_p(0x100000), fake, fake, 1, 8, 8, 3080, 3, 1, 1, None), "ca_dwconv_same")   # c > 3072
    expect(lib.ca_dwconv_same(fake, fake, fake, C.c_void_p(0x100000), fake, fake, 1, 8, 8, 48, 7, 1, 1, None), "ca_dwconv_same")     # ksize
    expect(lib.ca_dwconv_same(fake, fake, fake, C.c_void_p(0x100000), fake, fake, 1, 8, 8, 48, 3, 3, 1, None), "ca_dwconv_same")     # stride
    expect(lib.ca_dwconv_same(fake, fake, fake, fake, fake, fake, 1, 8, 8, 48, 3, 1, 1, None), "ca_dwconv_same")                     # y overlaps x
    assert lib.ca_dwconv_same_partials_floats(1, 8, 8, 44, 1) == 0 and lib.ca_dwconv_same_partials_floats(3, 8, 12, 48, 1) > 0
    expect(lib.ca_se_gate(fake, fake, fake, fake, fake, fake, 1, 48, 300, 1.0, None), "ca_se_gate")              # r > 256
    expect(lib.ca_scale_channels(fake, fake, fake, 1, 16, 44, 1, None), "ca_scale_channels")                     # c % 8
    expect(lib.ca_nbae_cat_pred(fake, fake, 1, 4, 6, 12, 0, 1, None), "ca_nbae_cat_pred")                        # ld % 8
    expect(lib.ca_nbae_normalize(fake, 6, fake, 16, 0.01, None), "ca_nbae_normalize")                            # ld % 4
    expect(lib.ca_nbae_finish(fake, 1, 3, 5, fake, None, 1, 2, None), "ca_nbae_finish")                          # h * w % 4
    expect(lib.ca_nbae_finish(fake, 1, 4, 4, None, None, 1, 2, None), "ca_nbae_finish")                          # no output
