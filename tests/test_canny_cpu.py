"""CPU: the ABI v16 canny entry points (symbols, argument checks, workspace query; no launch, no GPU), CannyAnnotator's input
checks, and the whole-window route of prep_control_images with a stub annotator."""
import ctypes as C

import numpy as np
import pytest

NEW = ["ca_canny_workspace_bytes", "ca_canny_tile_w", "ca_canny_tile_h", "ca_canny_classify", "ca_canny_link", "ca_canny_link_stage", "ca_canny_emit"]


@pytest.fixture(scope="module")
def capi():
    from controlanimate_amd import _build, _capi
    _build.build(verbose=False)
    return _capi


def test_abi_v16_and_symbols(capi):
    assert capi.ABI_VERSION == 16
    lib = capi.lib()
    assert lib.ca_abi_version() == 16
    for name in NEW:
        assert name in capi.SYMBOLS and getattr(lib, name) is not None
    from controlanimate_amd import kernels as K
    assert (lib.ca_canny_tile_h(), lib.ca_canny_tile_w()) == (K.CANNY_TILE_H, K.CANNY_TILE_W)


def test_workspace_query(capi):
    lib = capi.lib()
    sizes = [lib.ca_canny_workspace_bytes(n, h, w) for n, h, w in ((1, 1, 1), (1, 70, 133), (3, 70, 133), (16, 512, 768), (16, 1024, 768))]
    assert sizes[0] > 0 and sizes == sorted(set(sizes))                       # positive, strictly growing with images * h * w
    assert 6 * 16 * 512 * 768 <= sizes[3] < 6 * 16 * 512 * 768 + 4096         # label + class + flag per pixel
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (1 << 15, 1 << 8, 1 << 8), (2, 1 << 15, 1 << 15)):
        assert lib.ca_canny_workspace_bytes(*bad) == 0
    assert lib.ca_canny_workspace_bytes(1, 1 << 15, (1 << 16) - 1) > 0       # images * h * w = 2^31 - 2^15: the last sizes that fit


def test_entry_points_reject_bad_arguments_without_a_launch(capi):
    lib = capi.lib()
    fake, ws = C.c_void_p(0x1000), C.c_void_p(0x2000)  # never dereferenced: validation fails first
    odd = C.c_void_p(0x2004)
    need = lib.ca_canny_workspace_bytes(2, 8, 8)
    F16, F32 = capi.CA_F16, capi.CA_F32

    def expect(rc, who):
        assert rc < 0 and who.encode() in lib.ca_last_error(), (rc, lib.ca_last_error())

    cl = "ca_canny_classify"
    expect(lib.ca_canny_classify(None, 2, 8, 8, 3, 100, 200, ws, need, None), cl)
    expect(lib.ca_canny_classify(fake, 0, 8, 8, 3, 100, 200, ws, need, None), cl)
    expect(lib.ca_canny_classify(fake, 2, 0, 8, 3, 100, 200, ws, need, None), cl)
    expect(lib.ca_canny_classify(fake, 2, 8, 0, 3, 100, 200, ws, need, None), cl)
    expect(lib.ca_canny_classify(fake, 2, 8, 8, 2, 100, 200, ws, need, None), cl)
    expect(lib.ca_canny_classify(fake, 2, 8, 8, 4, 100, 200, ws, need, None), cl)
    expect(lib.ca_canny_classify(fake, 2, 8, 8, 0, 100, 200, ws, need, None), cl)
    expect(lib.ca_canny_classify(fake, 2, 8, 8, 3, 201, 200, ws, need, None), cl)
    expect(lib.ca_canny_classify(fake, 2, 8, 8, 3, 100, 200, None, need, None), cl)
    expect(lib.ca_canny_classify(fake, 2, 8, 8, 3, 100, 200, ws, need - 1, None), cl)
    expect(lib.ca_canny_classify(fake, 2, 8, 8, 3, 100, 200, odd, need, None), cl)
    expect(lib.ca_canny_classify(fake, 1 << 15, 1 << 8, 1 << 8, 3, 100, 200, ws, 1 << 40, None), cl)   # images * h * w = 2^31

    ln = "ca_canny_link"
    expect(lib.ca_canny_link(0, 8, 8, ws, need, None), ln)
    expect(lib.ca_canny_link(2, -1, 8, ws, need, None), ln)
    expect(lib.ca_canny_link(2, 8, 0, ws, need, None), ln)
    expect(lib.ca_canny_link(2, 8, 8, None, need, None), ln)
    expect(lib.ca_canny_link(2, 8, 8, ws, need - 1, None), ln)
    expect(lib.ca_canny_link(2, 8, 8, odd, need, None), ln)
    expect(lib.ca_canny_link(2, 1 << 15, 1 << 15, ws, 1 << 40, None), ln)

    st = "ca_canny_link_stage"
    expect(lib.ca_canny_link_stage(0, 8, 8, ws, need, 0, None), st)
    expect(lib.ca_canny_link_stage(2, 0, 8, ws, need, 1, None), st)
    expect(lib.ca_canny_link_stage(2, 8, -3, ws, need, 2, None), st)
    expect(lib.ca_canny_link_stage(2, 8, 8, None, need, 0, None), st)
    expect(lib.ca_canny_link_stage(2, 8, 8, ws, need - 1, 1, None), st)
    expect(lib.ca_canny_link_stage(2, 8, 8, odd, need, 2, None), st)
    expect(lib.ca_canny_link_stage(2, 8, 8, ws, need, 3, None), st)                      # label, merge, flatten: 0, 1, 2
    expect(lib.ca_canny_link_stage(2, 8, 8, ws, need, -1, None), st)
    expect(lib.ca_canny_link_stage(2, 1 << 15, 1 << 15, ws, 1 << 40, 0, None), st)

    em = "ca_canny_emit"
    expect(lib.ca_canny_emit(2, 8, 8, ws, need, None, None, 1, F32, None), em)           # neither output
    expect(lib.ca_canny_emit(0, 8, 8, ws, need, fake, None, 1, F32, None), em)
    expect(lib.ca_canny_emit(2, 0, 8, ws, need, fake, None, 1, F32, None), em)
    expect(lib.ca_canny_emit(2, 8, 0, ws, need, fake, None, 1, F32, None), em)
    expect(lib.ca_canny_emit(2, 8, 8, None, need, fake, None, 1, F32, None), em)
    expect(lib.ca_canny_emit(2, 8, 8, ws, need - 1, fake, None, 1, F32, None), em)
    expect(lib.ca_canny_emit(2, 8, 8, ws, need, fake, fake, 0, F32, None), em)
    expect(lib.ca_canny_emit(2, 8, 8, ws, need, fake, fake, 3, F16, None), em)
    expect(lib.ca_canny_emit(2, 8, 8, ws, need, fake, fake, 1, 3, None), em)             # unknown output dtype
    expect(lib.ca_canny_emit(2, 8, 8, ws, need, fake, fake, 1, -1, None), em)
    expect(lib.ca_canny_emit(2, 8, 8, ws, need, fake, fake, 1, capi.CA_BF16, None), em)  # the control tensor is fp32 or fp16
    expect(lib.ca_canny_emit(2, 8, 8, ws, need, None, C.c_void_p(0x1002), 1, F32, None), em)   # float32 at an odd address
    expect(lib.ca_canny_emit(1 << 15, 1 << 8, 1 << 8, ws, 1 << 40, fake, None, 1, F32, None), em)


def test_annotator_checks_types_before_the_device_and_has_no_cpu_fallback(capi, monkeypatch):
    import torch
    from controlanimate_amd.annotators import CannyAnnotator
    u8, f32 = np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 3), np.float32)
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "LIB_PATH", "/nonexistent/libcontrolanimate_hip.so")   # touching the device would raise CAHipUnavailable
    ann = CannyAnnotator()
    for call in (ann, lambda x: ann.edges([x]), lambda x: ann.annotate_batch([x])):
        with pytest.raises(TypeError):
            call(f32)
    with pytest.raises(TypeError):
        ann.edges(torch.zeros((1, 8, 8, 3), dtype=torch.float32))
    with pytest.raises(ValueError):
        ann.edges([u8, np.zeros((8, 9, 3), np.uint8)])
    with pytest.raises(ValueError):
        ann.annotate_batch([np.zeros((8, 8, 4), np.uint8)])
    with pytest.raises(ValueError):
        ann.annotate_batch([u8], rep=3)
    with pytest.raises(TypeError):
        ann.annotate_batch([u8], dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        ann.annotate_batch([u8], out=torch.zeros((1, 3, 8, 8), dtype=torch.float64))
    from PIL import Image
    with pytest.raises(ValueError, match="RGBA"):
        ann.annotate_batch([Image.new("RGBA", (8, 8))])
    with pytest.raises(ValueError):
        CannyAnnotator(low=300, high=200)
    with pytest.raises(capi.CAHipUnavailable):
        ann.edges([u8])
    with pytest.raises(capi.CAHipUnavailable):
        ann(u8)


def test_annotator_needs_a_gpu(capi, monkeypatch):
    import torch
    from controlanimate_amd.annotators import CannyAnnotator
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    u8 = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(capi.CAHipUnavailable):
        CannyAnnotator().annotate_batch([u8])
    with pytest.raises(capi.CAHipUnavailable):
        CannyAnnotator("cuda").edges(torch.zeros((1, 8, 8, 3), dtype=torch.uint8))


# ---- prep_control_images ---------------------------------------------------------------------------------------------------------

NAME = "lllyasviel/control_v11p_sd15_canny"


class _StubBatchAnnotator:
    """Has annotate_batch, records its calls, computes with the host function."""

    def __init__(self):
        self.batch_calls, self.single_calls = [], 0

    def __call__(self, image):
        from controlanimate_amd.annotators import canny
        self.single_calls += 1
        return canny(image)

    def annotate_batch(self, frames, out=None, rep=1, dtype=None):
        import torch
        from controlanimate_amd.annotators import canny_edges
        self.batch_calls.append({"n": len(frames), "out": out, "rep": rep, "dtype": dtype})
        e = torch.from_numpy(np.stack([canny_edges(np.asarray(f)) for f in frames])).to(dtype) / 255.0
        ctrl = torch.cat([e[:, None].expand(-1, 3, -1, -1)] * rep).contiguous()
        if out is not None:
            out.copy_(ctrl)
            return out
        return ctrl


def _pipe(annotators=None, use_lcm=False):
    from controlanimate_amd.configs import controlnet_config
    from controlanimate_amd.controlnet import ControlNetModel
    from controlanimate_amd.controlresiduals_pipeline import MultiControlNetResidualsPipeline
    net = ControlNetModel.from_config(controlnet_config(block_out_channels=(32, 64, 64, 64)))
    return MultiControlNetResidualsPipeline([NAME], [1.0], use_lcm=use_lcm, controlnets=[net], device="cpu", annotators=annotators)


def _frames(n=3, h=16, w=24):
    from PIL import Image
    out = []
    for i in range(n):
        a = np.zeros((h, w, 3), np.uint8)
        a[:, 6 + 3 * i:] = 255
        a[h // 2:, :, 1] = 40 * i
        out.append(Image.fromarray(a))
    return out


def _today(frames, doubled):
    import torch
    from controlanimate_amd.annotators import canny
    from controlanimate_amd.controlresiduals_pipeline import _image_to_chw01
    ctrl = torch.stack([_image_to_chw01(canny(f)) for f in frames])
    return torch.cat([ctrl] * 2) if doubled else ctrl


@pytest.mark.parametrize("cfg,guess,lcm,rep", [(True, False, False, 2), (True, True, False, 1), (False, False, False, 1), (True, False, True, 1)])
def test_prep_control_images_calls_annotate_batch_once(cfg, guess, lcm, rep):
    import torch
    stub = _StubBatchAnnotator()
    pipe, frames = _pipe({"canny": stub}, use_lcm=lcm), _frames()
    pipe.prep_control_images(frames, do_classifier_free_guidance=cfg, guess_mode=guess)
    assert stub.single_calls == 0 and len(stub.batch_calls) == 1
    call = stub.batch_calls[0]
    assert call["n"] == 3 and call["rep"] == rep and call["out"] is None and call["dtype"] == torch.float32
    got = pipe.prep_images[0]
    assert got._cfg_doubled is (rep == 2) and got.dtype == torch.float32
    assert torch.equal(got, _today(frames, rep == 2)) and got.sum() > 0
    # the next window goes into the tensor the ControlNets already hold
    nxt = _frames()[::-1]
    pipe.prep_control_images(nxt, do_classifier_free_guidance=cfg, guess_mode=guess)
    assert len(stub.batch_calls) == 2 and stub.batch_calls[1]["out"] is got
    assert pipe.prep_images[0] is got and got._cfg_doubled is (rep == 2) and torch.equal(got, _today(nxt, rep == 2))
    # another frame count does not fit: a new tensor
    pipe.prep_control_images(nxt[:2], do_classifier_free_guidance=cfg, guess_mode=guess)
    assert stub.batch_calls[2]["out"] is None and pipe.prep_images[0].shape[0] == 2 * rep


def test_prep_control_images_keeps_todays_path_for_everything_else():
    import torch
    frames = _frames()
    # a plain callable: per frame, as today; the default annotator is the host function
    from controlanimate_amd.annotators import canny
    calls = []
    plain = _pipe({"canny": lambda im: (calls.append(1), canny(im))[1]})
    plain.prep_control_images(frames)
    assert len(calls) == 3 and torch.equal(plain.prep_images[0], _today(frames, True)) and plain.prep_images[0]._cfg_doubled is True
    default = _pipe()
    assert default.annotators["canny"] is canny
    default.prep_control_images(frames)
    assert torch.equal(default.prep_images[0], plain.prep_images[0])
    # tensors are already annotated: the batch annotator is not asked, neither per frame nor per list
    stub = _StubBatchAnnotator()
    pipe = _pipe({"canny": stub})
    tens = [torch.rand(3, 16, 24) for _ in range(3)]
    pipe.prep_control_images(tens, do_classifier_free_guidance=False)
    assert not stub.batch_calls and stub.single_calls == 0 and torch.equal(pipe.prep_images[0], torch.stack(tens))
    # a dict source dispatches per name
    pipe.prep_control_images({NAME: frames})
    assert len(stub.batch_calls) == 1 and stub.batch_calls[0]["rep"] == 2 and torch.equal(pipe.prep_images[0], _today(frames, True))
    pipe.prep_control_images({NAME: tens}, do_classifier_free_guidance=False)
    assert len(stub.batch_calls) == 1 and torch.equal(pipe.prep_images[0], torch.stack(tens))


def test_chains_twin_keeps_the_annotator_object():
    from controlanimate_amd.chains import clone_residuals_pipeline
    stub = _StubBatchAnnotator()
    twin = clone_residuals_pipeline(_pipe({"canny": stub}))
    assert twin.annotators["canny"] is stub
    twin.prep_control_images(_frames())
    assert len(stub.batch_calls) == 1 and stub.single_calls == 0
