"""CPU: the depth annotator's specification (tests/depth_ref.py) against the fixture made from transformers' and Pillow's own modules
(tests/golden/dpt_tiny*.npz, tests/golden/make_dpt_golden.py) and against Pillow / torch themselves; the product's state-dict surface,
scope checks, routing and argument validation (controlanimate_amd/depth.py, csrc/ca_depth.hip).  No GPU is needed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_ref as R  # noqa: E402

RESIZE_SHAPES = [((64, 96), 96), ((40, 56), 96), ((512, 768), 384), ((384, 384), 384)]


@pytest.fixture(scope="module")
def fixture():
    data, sd = R.load_fixture()
    return {"data": data, "sd": sd}


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(np.asarray(b, np.float64)))


def test_reference_forward_equals_the_fixture(fixture):
    data, sd = fixture["data"], fixture["sd"]
    with torch.no_grad():
        depth, taps = R.forward(sd, R.TINY_CONFIG, torch.from_numpy(data["pixel_values_r3"]))
    rels = [_rel(depth.numpy(), data["predicted_depth"])] + [_rel(t.numpy(), data[f"tap{j}"]) for j, t in enumerate(taps)]
    print("relative L2 (predicted_depth, taps):", ["%.2e" % r for r in rels])
    assert max(rels) < 1e-5
    assert data["predicted_depth"].shape == (3, 96, 96) and data["tap0"].shape == (3, 37, 32)


def test_fixture_conditions(fixture):
    data = fixture["data"]
    assert sum(v.numel() for v in fixture["sd"].values()) == 855969
    for i in range(3):
        d, p = data["predicted_depth"][i], data["post"][i]
        assert d.max() > 0 and (d == 0).mean() <= 0.5 and (p < 0).any()
        assert len(np.unique(R.quantize_max(p)[0])) >= 100
    assert max(np.abs(data[f"tap{j}"]).max() for j in range(4)) < 100


def test_product_state_dict_keys_and_shapes_equal_the_fixtures(fixture):
    from controlanimate_amd.depth import DPTForDepthEstimation
    model = DPTForDepthEstimation(**R.TINY_CONFIG)
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    want = {k: tuple(v.shape) for k, v in fixture["sd"].items()}
    assert len(want) == 142 and got == want and want == R.key_shapes(R.TINY_CONFIG)
    model.load_state_dict(fixture["sd"], strict=True)
    assert model.dtype == torch.float16 and model.bfloat16().dtype == torch.bfloat16
    with pytest.raises(RuntimeError):
        model.prepare("cpu")                                             # the execution path has no CPU fallback


@pytest.mark.parametrize("resample", [2, 3], ids=["bilinear", "bicubic"])
@pytest.mark.parametrize("src,size", RESIZE_SHAPES)
def test_numpy_resampler_equals_pillow(src, size, resample):
    from PIL import Image
    from controlanimate_amd.depth import pil_coeffs
    h, w = src
    rng = np.random.default_rng(h + resample)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([127 + 120 * np.sin(0.11 * x + 0.07 * y + c) for c in range(3)], -1) + rng.normal(0, 12, (h, w, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    want = np.asarray(Image.fromarray(img).resize((size, size), resample=resample))
    got = R.pil_resize(img, size, size, resample)
    assert int((got != want).sum()) == 0
    for n_in in (h, w):                                                   # the product builds the same tables
        for a, b in zip(pil_coeffs(n_in, size, resample), R.pil_coeffs(n_in, size, resample)):
            assert a.dtype == np.int32 and np.array_equal(a, b)


@pytest.mark.parametrize("resample", [2, 3])
def test_preprocess_equals_the_image_processor(fixture, resample):
    data = fixture["data"]
    got = R.preprocess(data["frames"], 96, resample)
    assert np.abs(got - data[f"pixel_values_r{resample}"]).max() <= 2.0 ** -23   # the same bytes; the normalisation to fp32 round-off


@pytest.mark.parametrize("src,dst", [((96, 96), (64, 96)), ((96, 96), (200, 136)), ((48, 80), (17, 23))])
def test_bicubic_restatement_matches_torch(src, dst):
    d = torch.randn(2, *src, generator=torch.Generator().manual_seed(1)).relu()
    want = F.interpolate(d[:, None], size=dst, mode="bicubic", align_corners=False)[:, 0].numpy()
    got = R.bicubic_resize(d.numpy(), *dst)
    assert np.abs(got - want).max() / np.abs(want).max() < 1e-6


def test_bicubic_restatement_matches_the_post_processing(fixture):
    data = fixture["data"]
    got = R.bicubic_resize(data["predicted_depth"], 64, 96)
    assert np.abs(got - data["post"]).max() / np.abs(data["post"]).max() < 1e-6


def test_quantisations_match_numpy(fixture):
    post = fixture["data"]["post"]
    for p in post:
        q, sat = R.quantize_max(p)
        plain = (p * 255 / p.max())
        assert sat.sum() > 0 and (q[sat] == 0).all()                       # the deliberate deviation: saturated, where numpy's cast wraps on x86
        assert np.array_equal(q[~sat], plain[~sat].astype(np.int64).astype(np.uint8)) and np.array_equal(sat, plain <= -1)
        # what the GPU finish test leaves to one level: a scaled value within 1e-3 of an integer.  An exact zero of the map (7 .. 14 % of
        # these frames, zero under any rounding) is not among them: it must come out as level 0
        near = (np.abs(R.scaled_max(p) - np.rint(R.scaled_max(p))) < 1e-3) & (p != 0)
        assert near.mean() <= 0.01
        d = (p - p.min()) / (p.max() - p.min())
        assert np.array_equal(R.quantize_minmax(p), (d * 255).astype("uint8"))
        near = (np.abs(R.scaled_minmax(p) - np.rint(R.scaled_minmax(p))) < 1e-3) & (p != 0)
        assert near.mean() <= 0.01
    zero = np.zeros((8, 12), np.float32)
    assert not R.quantize_max(zero)[0].any() and not R.quantize_minmax(zero).any()
    assert not R.quantize_minmax(np.full((4, 4), 3.0, np.float32)).any()


def test_minmax_equals_the_recorded_pipeline_image(fixture):
    data = fixture["data"]
    got = np.stack([R.quantize_minmax(p) for p in data["post"]])
    assert np.array_equal(got, data["pipeline_depth"])


def test_routing_serves_both_depth_controlnets():
    from controlanimate_amd.controlresiduals_pipeline import MultiControlNetResidualsPipeline
    pipe = MultiControlNetResidualsPipeline.__new__(MultiControlNetResidualsPipeline)
    marker = object()
    pipe.annotators = {"canny": object(), "depth": marker}
    for name in ("lllyasviel/sd-controlnet-depth", "lllyasviel/control_v11f1p_sd15_depth"):
        assert pipe._annotator_for(name) is marker
    assert pipe._annotator_for("lllyasviel/control_v11p_sd15_openpose") is None
    from controlanimate_amd import annotators
    assert annotators.DepthAnnotator.__module__ == "controlanimate_amd.depth"


@pytest.mark.parametrize("bad", [dict(is_hybrid=True), dict(backbone_config={"model_type": "beit"}), dict(readout_type="add"), dict(readout_type="ignore"),
                                 dict(reassemble_factors=[4, 2, 1, 1]), dict(use_batch_norm_in_fusion_residual=True), dict(add_projection=True),
                                 dict(hidden_act="relu"), dict(image_size=104), dict(patch_size=12, image_size=96), dict(qkv_bias=False)],
                         ids=lambda d: ",".join(d))
def test_unsupported_configs_raise(bad):
    from controlanimate_amd.depth import DPTForDepthEstimation
    cfg = dict(R.TINY_CONFIG)
    cfg.update(bad)
    with pytest.raises(NotImplementedError):
        DPTForDepthEstimation(**cfg)


@pytest.mark.parametrize("bad", [dict(do_resize=False), dict(size={"height": 96, "width": 128}), dict(size={"height": 384, "width": 384}),
                                 dict(keep_aspect_ratio=True), dict(ensure_multiple_of=32), dict(do_pad=True), dict(image_mean=[0.485, 0.456, 0.406]),
                                 dict(image_std=[0.229, 0.224, 0.225]), dict(resample=0), dict(resample=1)], ids=lambda d: ",".join(d))
def test_unsupported_processor_settings_raise(bad):
    from controlanimate_amd.depth import check_processor
    pp = {"do_resize": True, "size": {"height": 96, "width": 96}, "resample": 3, "image_mean": [0.5] * 3, "image_std": [0.5] * 3}
    assert check_processor(pp, 96) == 3
    pp.update(bad)
    with pytest.raises(NotImplementedError):
        check_processor(pp, 96)


def test_annotator_constructor_and_from_pretrained(tmp_path, fixture):
    import json
    from controlanimate_amd.depth import DepthAnnotator, DPTForDepthEstimation
    model = DPTForDepthEstimation(**R.TINY_CONFIG)
    with pytest.raises(NotImplementedError):
        DepthAnnotator(model, 128, 3)                                      # a size other than the trained grid's
    with pytest.raises(NotImplementedError):
        DepthAnnotator(model, 96, 1)                                       # Lanczos
    with pytest.raises(ValueError):
        DepthAnnotator(model, 96, 3, normalize="mean")
    ann = DepthAnnotator(model, 96, 2, "minmax")
    assert ann.resample == 2 and ann.normalize == "minmax" and ann.size == 96
    with pytest.raises(TypeError):
        ann.depth([np.zeros((8, 8, 3), np.float32)])                       # before the device is touched
    with pytest.raises(ValueError):
        ann.depth([np.zeros((8, 8, 3), np.uint8), np.zeros((8, 9, 3), np.uint8)])
    # a local directory in transformers' layout; nothing is downloaded
    (tmp_path / "config.json").write_text(json.dumps(dict(R.TINY_CONFIG, model_type="dpt", architectures=["DPTForDepthEstimation"])))
    (tmp_path / "preprocessor_config.json").write_text(json.dumps({"do_resize": True, "size": {"height": 96, "width": 96}, "resample": 3, "do_rescale": True,
                                                                   "rescale_factor": 1 / 255, "do_normalize": True, "image_mean": [0.5] * 3, "image_std": [0.5] * 3,
                                                                   "keep_aspect_ratio": False, "ensure_multiple_of": 1, "do_pad": False}))
    torch.save(fixture["sd"], tmp_path / "pytorch_model.bin")
    ann = DepthAnnotator.from_pretrained(tmp_path, dtype=torch.bfloat16, normalize="minmax")
    assert ann.model.dtype == torch.bfloat16 and ann.resample == 3 and ann.size == 96
    assert torch.equal(ann.model.state_dict()["head.head.4.weight"], fixture["sd"]["head.head.4.weight"])
    (tmp_path / "preprocessor_config.json").write_text(json.dumps({"size": {"height": 96, "width": 96}, "keep_aspect_ratio": True}))
    with pytest.raises(NotImplementedError):
        DepthAnnotator.from_pretrained(tmp_path)
    with pytest.raises(FileNotFoundError):
        DepthAnnotator.from_pretrained(tmp_path / "absent")


def test_abi_version_and_bad_arguments_without_a_gpu():
    from controlanimate_amd import _build, _capi
    _build.build(verbose=False)
    lib = _capi.lib()
    assert _capi.ABI_VERSION == 16 and lib.ca_abi_version() == 16
    fake, fake2, fake3 = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)

    def expect(rc, who):
        assert rc < 0 and who.encode() in lib.ca_last_error(), (rc, lib.ca_last_error())

    expect(lib.ca_resize_pil_u8(None, fake2, fake3, 1, 8, 8, 4, 4, fake, fake, 3, fake, fake, 3, None), "ca_resize_pil_u8")
    expect(lib.ca_resize_pil_u8(fake, fake2, fake3, 1, 8, 0, 4, 4, fake, fake, 3, fake, fake, 3, None), "ca_resize_pil_u8")      # an empty source
    expect(lib.ca_resize_pil_u8(fake, fake2, fake3, 1, 8, 8, 4, 4, fake, fake, 0, fake, fake, 3, None), "ca_resize_pil_u8")      # ksize
    expect(lib.ca_resize_pil_u8(fake, fake, fake3, 1, 8, 8, 4, 4, fake, fake, 3, fake, fake, 3, None), "ca_resize_pil_u8")       # tmp is src
    expect(lib.ca_dpt_patches(fake, None, 1, 96, 16, 1, None), "ca_dpt_patches")
    expect(lib.ca_dpt_patches(fake, fake2, 1, 96, 12, 1, None), "ca_dpt_patches")                                               # patch % 8
    expect(lib.ca_dpt_patches(fake, fake2, 1, 100, 16, 1, None), "ca_dpt_patches")                                              # size % patch
    expect(lib.ca_dpt_patches(fake, fake2, 1, 96, 16, 7, None), "ca_dpt_patches")                                               # dtype
    expect(lib.ca_depth_to_space(fake, fake2, 1, 6, 6, 3, 16, 144, 36, 0, 1, None), "ca_depth_to_space")                        # k
    expect(lib.ca_depth_to_space(fake, fake2, 1, 6, 6, 2, 12, 48, 36, 0, 1, None), "ca_depth_to_space")                         # cout % 8
    expect(lib.ca_depth_to_space(fake, fake2, 1, 6, 6, 2, 16, 32, 36, 0, 1, None), "ca_depth_to_space")                         # ldx < k k cout
    expect(lib.ca_depth_to_space(fake, fake2, 1, 6, 6, 2, 16, 64, 36, 1, 1, None), "ca_depth_to_space")                         # row0 + gh gw > rows
    expect(lib.ca_depth_to_space(fake, fake, 1, 6, 6, 2, 16, 64, 36, 0, 1, None), "ca_depth_to_space")                          # in place
    assert [lib.ca_dpt_head_supported(c) for c in (32, 64, 128, 0, 48, 256)] == [1, 1, 1, 0, 0, 0]
    expect(lib.ca_dpt_head(fake, fake, fake, fake, fake, None, 1, 8, 8, 128, 1, None), "ca_dpt_head")
    expect(lib.ca_dpt_head(fake, fake, fake, fake, fake, fake, 1, 8, 8, 256, 1, None), "ca_dpt_head")                           # cmid
    expect(lib.ca_dpt_head(fake, fake, fake, fake, fake, fake, 1, 0, 8, 128, 1, None), "ca_dpt_head")                           # h
    expect(lib.ca_dpt_head(fake, fake, fake, fake, fake, fake, 1, 8, 8, 128, 5, None), "ca_dpt_head")                           # dtype
    expect(lib.ca_dpt_head(C.c_void_p(0x1008), fake, fake, fake, fake, fake, 1, 8, 8, 128, 1, None), "ca_dpt_head")             # alignment
    expect(lib.ca_dpt_logit(fake, fake, fake, None, 64, None), "ca_dpt_logit")
    expect(lib.ca_dpt_logit(fake, fake, fake, fake, 0, None), "ca_dpt_logit")
    expect(lib.ca_resize_bicubic_f32(fake, fake2, None, None, 1, 8, 8, 4, 4, None), "ca_resize_bicubic_f32")
    expect(lib.ca_resize_bicubic_f32(fake, fake2, fake3, None, 1, 8, 8, 0, 4, None), "ca_resize_bicubic_f32")
    expect(lib.ca_resize_bicubic_f32(fake, fake, fake3, None, 1, 8, 8, 4, 4, None), "ca_resize_bicubic_f32")                    # in place
    expect(lib.ca_depth_finish(fake, fake2, 1, 8, 8, 2, fake3, None, 1, 2, None), "ca_depth_finish")                            # mode
    expect(lib.ca_depth_finish(fake, fake2, 1, 8, 8, 0, None, None, 1, 2, None), "ca_depth_finish")                             # no output
    expect(lib.ca_depth_finish(fake, fake2, 1, 8, 8, 0, fake3, None, 3, 2, None), "ca_depth_finish")                            # rep
    expect(lib.ca_depth_finish(fake, fake2, 1, 8, 8, 0, fake3, fake3, 1, 0, None), "ca_depth_finish")                           # control dtype
    expect(lib.ca_depth_finish(None, fake2, 1, 8, 8, 0, fake3, None, 1, 2, None), "ca_depth_finish")
