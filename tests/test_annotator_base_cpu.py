"""CPU: what the annotators share (controlanimate_amd/annotator_base.py) -- the buffer plan, a pass through a network and the weight
packers on CPU tensors, the frame intake and the
`out` contracts through a toy subclass (the order of the checks, their messages as HedAnnotator raised them before the base existed,
and that none of them touches the device), and the state-dict check.  No GPU, no library."""
import numpy as np
import pytest
import torch

from controlanimate_amd.annotator_base import (AnnotatorBase, BufferPlan, PackedNetwork, bn_key_shapes, check_state_dict, fold_bn, pack_conv, pack_depthwise,
                                               pack_pointwise, to_device)


# ---- BufferPlan --------------------------------------------------------------------------------------------------------------------
def _ws():
    return {"pool": [], "plan": [], "planned": False}


def _pass(ws):
    """A take / give sequence with reuse: -> the data pointers in take order."""
    plan = BufferPlan(ws, torch.float16, "cpu")
    a = plan.take(2, 8, 8, 4)
    b = plan.take(2, 4, 4, 8)
    plan.give(a)
    c = plan.take(2, 8, 8, 2)      # fits into a's buffer
    d = plan.take(3, 5)
    plan.give(b), plan.give(c)
    e = plan.take(2, 4, 4, 8)
    plan.give(d), plan.give(e)
    assert a.shape == (2, 8, 8, 4) and c.shape == (2, 8, 8, 2) and a.dtype == torch.float16 and c.data_ptr() == a.data_ptr()
    ws["planned"] = True
    return [t.data_ptr() for t in (a, b, c, d, e)]


def test_buffer_plan_replays_the_first_pass():
    ws = _ws()
    first = _pass(ws)
    pool = [slot[0].data_ptr() for slot in ws["pool"]]
    assert len(pool) == 3 and ws["plan"] == [0, 1, 0, 2, 1] and not any(slot[1] for slot in ws["pool"])
    for _ in range(2):
        assert _pass(ws) == first
        assert [slot[0].data_ptr() for slot in ws["pool"]] == pool and ws["plan"] == [0, 1, 0, 2, 1]


def test_buffer_plan_starts_over_after_an_abandoned_first_pass():
    ws = _ws()
    plan = BufferPlan(ws, torch.float16, "cpu")
    plan.take(4, 4)
    plan.take(100)                 # ... and the pass ends here, without ws["planned"]
    assert ws["plan"] == [0, 1] and all(slot[1] for slot in ws["pool"])
    first = _pass(ws)              # the plan is made anew and every buffer is free again: the 16-element one serves the 15-element take
    assert ws["plan"] == [2, 3, 2, 0, 3] and len(ws["pool"]) == 4 and not any(slot[1] for slot in ws["pool"])
    assert _pass(ws) == first


def test_buffer_plan_give_rejects_a_foreign_tensor_and_take_is_best_fit():
    ws = _ws()
    plan = BufferPlan(ws, torch.float32, "cpu")
    big, small, mid = plan.take(1000), plan.take(10), plan.take(100)
    with pytest.raises(AssertionError, match="not a pool buffer"):
        plan.give(torch.zeros(10))
    for t in (big, small, mid):
        plan.give(t)
    assert plan.take(50).data_ptr() == mid.data_ptr()       # the smallest free buffer that is large enough, not the first
    assert plan.take(50).data_ptr() == big.data_ptr()       # mid is taken now
    assert plan.take(5).data_ptr() == small.data_ptr()
    assert len(ws["pool"]) == 3
    assert plan.take(5).numel() == 5 and len(ws["pool"]) == 4   # nothing free: a new buffer


# ---- NetPass -------------------------------------------------------------------------------------------------------------------------
class ToyNet(PackedNetwork):
    dtype = torch.float16

    def __init__(self):
        self._ws, self.made = {}, 0

    def _device(self):
        return torch.device("cpu")

    def workspace(self, n):
        def make(dev):
            self.made += 1
            return {"out": torch.empty(n, device=dev)}
        return self._workspace(n, make)


def _net_pass(net, ws, fail=False):
    """The take / give sequence of _pass through a NetPass -> the data pointers in take order."""
    with net._pass(ws, "cpu") as p:
        a = p.take(2, 8, 8, 4)
        b = p.take(2, 4, 4, 8)
        p.give(a)
        c = p.take(2, 8, 8, 2)
        if fail:
            raise RuntimeError("a launch failed")
        d = p.launch("stage", lambda x, out: out, c, out=p.take(3, 5))
        p.give(b), p.give(c)
        e = p.take(2, 4, 4, 8)
        p.give(d), p.give(e)
        assert not ws["planned"] or p.replay       # the flag is set when the block is left, not inside it
    return [t.data_ptr() for t in (a, b, c, d, e)]


def test_workspace_cache_and_chunks():
    net = ToyNet()
    ws = net.workspace(3)
    assert net.workspace(3) is ws and net.made == 1 and net.workspace(4) is not ws and net.made == 2
    assert ws["pool"] == [] and ws["plan"] == [] and ws["planned"] is False and tuple(ws["out"].shape) == (3,)
    assert net._workspace("tuple", lambda dev: (1, 2)) == (1, 2)        # only a dict gets the plan's entries
    assert list(net._chunks(7, 3)) == [(0, slice(0, 3)), (3, slice(3, 6)), (6, slice(6, 7))]
    assert list(net._chunks(0, 3)) == [] and list(net._chunks(3, 5)) == [(0, slice(0, 3))]


def test_net_pass_replays_the_first_pass_and_allocates_nothing():
    net = ToyNet()
    ws = net.workspace(1)
    first = _net_pass(net, ws)
    pool = [slot[0].data_ptr() for slot in ws["pool"]]
    assert ws["planned"] is True and len(pool) == 3 and ws["plan"] == [0, 1, 0, 2, 1] and first[2] == first[0]
    for _ in range(2):
        assert _net_pass(net, ws) == first
        assert [slot[0].data_ptr() for slot in ws["pool"]] == pool and ws["plan"] == [0, 1, 0, 2, 1]


def test_net_pass_that_raises_leaves_planned_false_and_the_next_pass_plans_again():
    net = ToyNet()
    ws = net.workspace(1)
    with pytest.raises(RuntimeError, match="a launch failed"):
        _net_pass(net, ws, fail=True)
    assert ws["planned"] is False and ws["plan"] == [0, 1, 0]
    first = _net_pass(net, ws)                     # plans anew, on the buffers that are there
    assert ws["planned"] is True and ws["plan"] == [0, 1, 0, 2, 1] and len(ws["pool"]) == 3
    assert _net_pass(net, ws) == first
    with pytest.raises(RuntimeError):              # a replay that raises does not unplan
        _net_pass(net, ws, fail=True)
    assert ws["planned"] is True and _net_pass(net, ws) == first


def test_net_pass_launches_are_the_nets_stages():
    net = ToyNet()
    seen = []
    net._timed = lambda name, fn, *a, **kw: (seen.append(name), fn(*a, **kw))[1]
    with net._pass(net.workspace(1), "cpu") as p:
        assert p.launch("prep", lambda x, k=0: x + k, 1, k=2) == 3
    assert seen == ["prep"]


def test_pointwise_hands_the_gemm_pixel_views(monkeypatch):
    from controlanimate_amd import kernels as K
    calls = []
    monkeypatch.setattr(K, "gemm", lambda a, w, **kw: calls.append((a, w, kw)))
    net = ToyNet()
    ws = net.workspace(1)
    wt, bias = torch.zeros(32, 64, dtype=torch.float16), torch.zeros(32)
    x, res, a2 = torch.zeros(2, 8, 8, 64, dtype=torch.float16), torch.zeros(2, 8, 8, 32, dtype=torch.float16), torch.zeros(2, 8, 8, 16, dtype=torch.float16)
    wide = torch.zeros(2, 8, 8, 128, dtype=torch.float16)
    with net._pass(ws, "cpu") as p:
        y = p.pointwise("pw", x, (wt, bias), act=K.ACT_RELU, residual=res, a2=a2)
        a, w, kw = calls[-1]
        assert tuple(y.shape) == (2, 8, 8, 32) and y.dtype == torch.float16 and y.data_ptr() == ws["pool"][0][0].data_ptr()
        assert tuple(a.shape) == (128, 64) and a.data_ptr() == x.data_ptr() and w is wt and kw["bias"] is bias and kw["act"] == K.ACT_RELU
        assert tuple(kw["out"].shape) == (128, 32) and kw["out"].data_ptr() == y.data_ptr() and kw["out"].is_contiguous() and kw["out_f32"] is False
        assert tuple(kw["residual"].shape) == (128, 32) and kw["residual"].data_ptr() == res.data_ptr()
        assert tuple(kw["a2"].shape) == (128, 16) and kw["a2"].data_ptr() == a2.data_ptr()
        # out2d: a column slice of a wider tensor is handed over as it is (its row stride stays 128), nothing is taken, None comes back
        out2d = wide.view(128, 128)[:, 64:96]
        assert p.pointwise("pw", x, (wt, None), out2d=out2d, out_f32=True) is None and len(ws["pool"]) == 1
        a, w, kw = calls[-1]
        assert kw["out"] is out2d and kw["out"].stride() == (128, 1) and kw["out"].data_ptr() == wide.data_ptr() + 64 * 2
        assert kw["bias"] is None and kw["residual"] is None and kw["a2"] is None and kw["act"] == K.ACT_NONE and kw["out_f32"] is True
        # pixels x C in, pixels x N out
        y2 = p.pointwise("pw", x.view(128, 64), (wt, bias))
        assert tuple(y2.shape) == (128, 32) and tuple(calls[-1][2]["out"].shape) == (128, 32) and len(calls) == 3


def test_conv3x3_takes_its_own_output(monkeypatch):
    from controlanimate_amd import kernels as K
    calls = []
    monkeypatch.setattr(K, "conv3x3", lambda x, w, **kw: (calls.append((x, w, kw)), kw["out"])[1])
    net = ToyNet()
    wt, bias, x = torch.zeros(32, 3, 3, 64, dtype=torch.float16), torch.zeros(32), torch.zeros(2, 9, 8, 64, dtype=torch.float16)
    with net._pass(net.workspace(1), "cpu") as p:
        y = p.conv3x3("conv", x, (wt, bias), stride=2, act=K.ACT_RELU, pad_asym=True)
        assert tuple(y.shape) == (2, 5, 4, 32) and calls[-1][2] == {"bias": bias, "stride": 2, "act": K.ACT_RELU, "out": y, "pad_asym": True}
        assert tuple(p.conv3x3("conv", x, (wt, None)).shape) == (2, 9, 8, 32) and calls[-1][2]["stride"] == 1 and calls[-1][2]["act"] == K.ACT_NONE


# ---- the packers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [True, False])
def test_fold_bn_equals_eval_mode_batchnorm_in_float64(with_bias):
    g = torch.Generator().manual_seed(3)
    conv = torch.nn.Conv2d(5, 7, 3, padding=1, bias=with_bias)
    bn = torch.nn.BatchNorm2d(7, eps=1e-3)
    with torch.no_grad():
        for t in (bn.weight, bn.bias, bn.running_mean):
            t.copy_(torch.randn(7, generator=g))
        bn.running_var.copy_(torch.rand(7, generator=g) + 0.5)
    sd = {**{"c." + k: v for k, v in conv.state_dict().items()}, **{"n." + k: v for k, v in bn.state_dict().items()}}
    assert set(bn_key_shapes("n", 7)) == set(sd) - {"c.weight", "c.bias", "n.num_batches_tracked"} and bn_key_shapes("n", 7)["n.running_var"] == (7,)
    w, b = fold_bn(sd, "c", "n", 1e-3)
    assert w.dtype == b.dtype == torch.float32 and tuple(w.shape) == (7, 5, 3, 3) and tuple(b.shape) == (7,)
    x = torch.randn(2, 5, 6, 6, generator=g).double()
    with torch.no_grad():
        want = bn.double().eval()(conv.double()(x))
        got = torch.nn.functional.conv2d(x, w.double(), b.double(), padding=1)
    # fp32 folding against float64: a few fp32 roundings of values of order 1 .. 10
    assert float((got - want).abs().max()) < 1e-5
    lin_w, _ = fold_bn({**sd, "c.weight": sd["c.weight"][:, :, 0, 0:1].reshape(7, 5, 1)}, "c", "n", 1e-3)      # a Conv1d weight folds too
    assert tuple(lin_w.shape) == (7, 5, 1)


def test_pack_conv_and_pointwise_pad_with_zeros():
    g = torch.Generator().manual_seed(5)
    w, b = torch.randn(5, 3, 3, 3, generator=g), torch.randn(5, generator=g)
    pw_, pb = pack_conv((w, b), torch.float16, cin_pad=8, cout_pad=8)
    assert tuple(pw_.shape) == (8, 3, 3, 8) and pw_.dtype == torch.float16 and pw_.is_contiguous() and pb.dtype == torch.float32 and pb.is_contiguous()
    assert torch.equal(pw_[:5, :, :, :3], w.permute(0, 2, 3, 1).to(torch.float16)) and torch.equal(pb[:5], b)
    assert float(pw_[5:].abs().max()) == 0 and float(pw_[..., 3:].abs().max()) == 0 and float(pb[5:].abs().max()) == 0
    plain, none = pack_conv((w, None), torch.bfloat16, cin_pad=2, cout_pad=4)       # a pad below the size pads nothing; no bias stays None
    assert tuple(plain.shape) == (5, 3, 3, 3) and plain.dtype == torch.bfloat16 and none is None
    w7 = torch.randn(4, 6, 7, 7, generator=g)
    assert torch.equal(pack_conv((w7, None), torch.float32)[0], w7.permute(0, 2, 3, 1).contiguous())
    lw, lb = pack_pointwise((torch.randn(5, 6, 1, 1, generator=g), b), torch.float16, cout_pad=8)
    assert tuple(lw.shape) == (8, 6) and lw.is_contiguous() and float(lw[5:].abs().max()) == 0 and torch.equal(lb[:5], b) and float(lb[5:].abs().max()) == 0
    lw1, _ = pack_pointwise((torch.ones(5, 6, 1), None), torch.float16)
    assert tuple(lw1.shape) == (5, 6) and lw1.dtype == torch.float16


def test_pack_depthwise_rejects_what_the_three_modules_rejected():
    dw = torch.arange(16 * 9, dtype=torch.float32).view(16, 1, 3, 3)
    p = pack_depthwise(dw, (3,))
    assert tuple(p.shape) == (9, 16) and p.is_contiguous() and p[5, 3] == dw[3, 0, 1, 2]
    assert tuple(pack_depthwise(torch.zeros(8, 1, 5, 5), (3, 5)).shape) == (25, 8)
    for bad, ksizes, text in ((torch.zeros(16, 2, 3, 3), (3,), "[C, 1, 3, 3]"), (torch.zeros(16, 1, 5, 5), (3,), "[C, 1, 3, 3]"),
                              (torch.zeros(16, 9), (3,), "[C, 1, 3, 3]"), (torch.zeros(8, 1, 4, 4), (3, 5), "[C, 1, 3, 3] or [C, 1, 5, 5]"),
                              (torch.zeros(8, 1, 3, 5), (3, 5), "[C, 1, 3, 3] or [C, 1, 5, 5]"), (torch.zeros(8, 2, 5, 5), (3, 5), "[C, 1, 3, 3] or [C, 1, 5, 5]")):
        with pytest.raises(ValueError) as e:
            pack_depthwise(bad, ksizes)
        assert str(e.value) == f"a depthwise weight {text} is expected, got {tuple(bad.shape)}"
    from controlanimate_amd import mlsd, normalbae, softedge
    for mod, bad, text in ((mlsd, torch.zeros(16, 1, 5, 5), "[C, 1, 3, 3]"), (softedge, torch.zeros(8, 1, 4, 4), "[C, 1, 3, 3] or [C, 1, 5, 5]"),
                           (normalbae, torch.zeros(8, 1, 4, 4), "[C, 1, k, k] with k = 3 or 5")):
        with pytest.raises(ValueError) as e:
            mod.pack_depthwise(bad)
        assert str(e.value) == f"a depthwise weight {text} is expected, got {tuple(bad.shape)}"


# ---- a toy annotator ---------------------------------------------------------------------------------------------------------------
class Toy(AnnotatorBase):
    _bytes_per_pixel = 4

    def __init__(self):
        self.device_calls, self.runs = 0, []

    def _device(self):
        self.device_calls += 1
        return torch.device("cpu")

    def _check_size(self, h, w):
        if h % 8 or w % 8:
            raise NotImplementedError(f"Toy takes multiples of 8; got {h} x {w}")

    def edges(self, frames, out=None):
        return self._uint8_out(frames, out)

    def _run(self, src, edges, control, rep):
        self.runs.append((tuple(src.shape), edges, control, rep))
        if edges is not None:
            edges.copy_(src[..., 0] if edges.dim() == 3 else src)


class ToyGrey(Toy):
    _grey_to_rgb = False


U8 = np.zeros((8, 8, 3), np.uint8)
FRAME_MSG = "a frame must be [H, W] or [H, W, C] with C = 1 or 3 (PIL mode L or RGB: convert RGBA or palette frames with .convert('RGB') first), got "


def _raises(kind, message, call, toy, device_calls=0):
    before = toy.device_calls
    with pytest.raises(kind) as e:
        call()
    assert str(e.value) == message
    assert toy.device_calls - before == device_calls and not toy.runs


def test_intake_checks_come_before_the_device_with_hed_messages():
    from PIL import Image
    toy = Toy()
    for call in (toy.edges, toy.annotate_batch, toy._frames):
        _raises(TypeError, "frames must be uint8, got torch.float32", lambda: call(torch.zeros((1, 8, 8, 3))), toy)
        _raises(TypeError, "frames must be uint8, got float32", lambda: call([np.zeros((8, 8, 3), np.float32)]), toy)
        _raises(ValueError, "frames tensor must be [n, H, W] or [n, H, W, C] with C = 1 or 3, got (1, 8, 8, 4)",
                lambda: call(torch.zeros((1, 8, 8, 4), dtype=torch.uint8)), toy)
        _raises(ValueError, "frames tensor must be [n, H, W] or [n, H, W, C] with C = 1 or 3, got (8, 8)", lambda: call(torch.zeros((8, 8), dtype=torch.uint8)), toy)
        _raises(ValueError, FRAME_MSG + "(8, 8, 4)", lambda: call([np.zeros((8, 8, 4), np.uint8)]), toy)
        _raises(ValueError, FRAME_MSG + "(8, 8, 4) from PIL mode RGBA", lambda: call([Image.new("RGBA", (8, 8))]), toy)
        _raises(ValueError, "no frames", lambda: call([]), toy)
        _raises(ValueError, "all frames of a call must share one size", lambda: call([U8, np.zeros((8, 16, 3), np.uint8)]), toy)
        _raises(NotImplementedError, "Toy takes multiples of 8; got 12 x 8", lambda: call([np.zeros((12, 8, 3), np.uint8)]), toy)
        _raises(NotImplementedError, "Toy takes multiples of 8; got 8 x 12", lambda: call(torch.zeros((2, 8, 12, 3), dtype=torch.uint8)), toy)
    _raises(TypeError, "frames must be uint8, got float32", lambda: toy(np.zeros((8, 8, 3), np.float32)), toy)
    assert toy.device_calls == 0


def test_the_order_of_the_checks():
    toy = Toy()
    f32, odd = np.zeros((12, 8, 3), np.float32), np.zeros((12, 8, 3), np.uint8)
    bad_out = torch.zeros((1, 3, 8, 8), dtype=torch.float64)
    # annotate_batch: rep, then the control tensor's dtype (given or out's), then the frames -- all before the device
    _raises(ValueError, "rep=3 (1 or 2)", lambda: toy.annotate_batch([f32], rep=3, dtype=torch.bfloat16), toy)
    _raises(ValueError, "rep=0 (1 or 2)", lambda: toy.annotate_batch([U8], rep=0), toy)
    _raises(TypeError, "the control tensor is float32 or float16, got torch.bfloat16", lambda: toy.annotate_batch([f32], dtype=torch.bfloat16), toy)
    _raises(TypeError, "the control tensor is float32 or float16, got torch.float64", lambda: toy.annotate_batch([f32], out=bad_out), toy)
    _raises(TypeError, "frames must be uint8, got float32", lambda: toy.annotate_batch([f32]), toy)
    # the frames: dtype, then shape, then one size, then the scope
    _raises(TypeError, "frames must be uint8, got float32", lambda: toy._frames([np.zeros((8, 8, 4), np.float32)]), toy)
    _raises(ValueError, FRAME_MSG + "(12, 8, 4)", lambda: toy._frames([odd, np.zeros((12, 8, 4), np.uint8)]), toy)
    _raises(ValueError, "all frames of a call must share one size", lambda: toy._frames([odd, U8]), toy)
    # `out` is compared with the frames on their device, so its shape, device and layout checks are the only ones behind the device
    _raises(ValueError, "out must be a contiguous torch.float32 tensor (2, 3, 8, 8) on cpu", lambda: toy.annotate_batch([U8], out=torch.zeros((1, 3, 8, 8)), rep=2), toy, 1)
    _raises(ValueError, "out must be a contiguous torch.float16 tensor (1, 3, 8, 8) on cpu",
            lambda: toy.annotate_batch([U8], out=torch.zeros((1, 3, 8, 8)), dtype=torch.float16), toy, 1)
    _raises(ValueError, "out must be a contiguous torch.float32 tensor (1, 3, 8, 8) on cpu",
            lambda: toy.annotate_batch([U8], out=torch.zeros((1, 8, 8, 3)).permute(0, 3, 1, 2)), toy, 1)
    _raises(ValueError, "out must be a contiguous uint8 tensor (1, 8, 8) on cpu", lambda: toy.edges([U8], out=torch.zeros((1, 8, 8))), toy, 1)
    _raises(ValueError, "out must be a contiguous uint8 tensor (1, 8, 8, 3) on cpu",
            lambda: toy._uint8_out([U8], torch.zeros((1, 8, 8), dtype=torch.uint8), channels_last=3), toy, 1)
    _raises(TypeError, "frames must be uint8, got float32", lambda: toy.edges([f32], out=torch.zeros((1, 8, 8))), toy)


def test_outputs_and_what_run_is_asked_for():
    toy = Toy()
    empty = torch.zeros((0, 8, 8, 3), dtype=torch.uint8)
    out = toy.annotate_batch(empty, rep=2)
    assert tuple(out.shape) == (0, 3, 8, 8) and out.dtype == torch.float32 and tuple(toy.edges(empty).shape) == (0, 8, 8) and not toy.runs
    frames = [U8, U8 + 1, U8 + 2]
    out = toy.annotate_batch(frames, rep=2)
    assert tuple(out.shape) == (6, 3, 8, 8) and out.dtype == torch.float32
    assert toy.runs == [((3, 8, 8, 3), None, out, 2)] and toy.runs[0][2] is out
    given = torch.empty((3, 3, 8, 8), dtype=torch.float16)
    assert toy.annotate_batch(frames, out=given) is given and toy.runs[1][2] is given and toy.runs[1][3] == 1
    assert toy.annotate_batch(frames, dtype=torch.float16).dtype == torch.float16
    e = toy.edges(frames)
    assert e.dtype == torch.uint8 and tuple(e.shape) == (3, 8, 8) and toy.runs[-1][1] is e and toy.runs[-1][2] is None and toy.runs[-1][3] == 1
    assert [int(x) for x in e[:, 0, 0]] == [0, 1, 2]
    assert tuple(toy._uint8_out(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), None, channels_last=3).shape) == (2, 8, 8, 3)
    # a grey frame is repeated to three channels, unless the class keeps C as given
    for grey in ([np.zeros((8, 8), np.uint8)], torch.zeros((1, 8, 8), dtype=torch.uint8), torch.zeros((1, 8, 8, 1), dtype=torch.uint8)):
        assert tuple(Toy()._frames(grey).shape) == (1, 8, 8, 3) and tuple(ToyGrey()._frames(grey).shape) == (1, 8, 8, 1)
    assert Toy()._frames(torch.zeros((1, 8, 8, 1), dtype=torch.uint8)).is_contiguous()


def test_call_returns_what_came_in():
    from PIL import Image
    toy = Toy()
    img = np.full((8, 8, 3), 7, np.uint8)
    arr = toy(img)
    assert isinstance(arr, np.ndarray) and arr.shape == (8, 8, 3) and arr.dtype == np.uint8 and (arr == 7).all()
    pil = toy(Image.fromarray(img))
    assert isinstance(pil, Image.Image) and pil.mode == "RGB" and pil.size == (8, 8) and np.array_equal(np.asarray(pil), arr)
    assert isinstance(toy(Image.new("L", (8, 8))), Image.Image)


def test_chunking_and_the_device_weights():
    toy = Toy()
    assert toy.chunk_frames(8, 8) == (0x7FFFFF00 - 1) // 256
    toy.max_activation_bytes = 3 * 256 + 5
    assert toy.chunk_frames(8, 8) == 3
    toy.max_activation_bytes = 255
    with pytest.raises(ValueError) as e:
        toy.chunk_frames(8, 8)
    assert str(e.value) == "a 8 x 8 frame alone exceeds what the kernels address (256 > 255 bytes)"
    del toy.max_activation_bytes
    assert toy.max_activation_bytes == 0x7FFFFF00 - 1
    toy._host = {"a": [(torch.ones(2), None)], "b": {"c": torch.zeros(3)}}
    moved = toy._weights(torch.device("cpu"))
    assert isinstance(moved["a"][0], tuple) and moved["a"][0][1] is None and torch.equal(moved["b"]["c"], torch.zeros(3))
    assert toy._weights(torch.device("cpu")) is moved                    # moved once per device
    assert toy._weights(torch.device("meta")) is not moved and toy._weights(torch.device("meta"))["b"]["c"].device.type == "meta"
    assert to_device(None, "cpu") is None


# ---- check_state_dict ----------------------------------------------------------------------------------------------------------------
def test_check_state_dict_raises_the_hed_messages():
    want = {"norm": (1, 3, 1, 1), "block1.convs.0.weight": (64, 3, 3, 3)}
    hint = "norm, block1..5.convs.*.weight|bias, block1..5.projection.weight|bias"
    sd = {k: torch.zeros(s) for k, s in want.items()}
    check_state_dict(sd, want, "HED", hint)
    with pytest.raises(KeyError) as e:
        check_state_dict({"norm": sd["norm"], "extra": 0}, want, "HED", hint)      # a missing tensor is named before an unexpected one
    assert e.value.args[0] == f"HED state dict: 'block1.convs.0.weight' is missing (2 tensors expected: {hint})"
    with pytest.raises(ValueError) as e:
        check_state_dict({**sd, "block6.convs.0.weight": torch.zeros(1), "norm": torch.zeros(3)}, want, "HED", hint)   # ... and that before a shape
    assert str(e.value) == "HED state dict: unexpected tensor 'block6.convs.0.weight'"
    with pytest.raises(ValueError) as e:
        check_state_dict({**sd, "norm": torch.zeros(3)}, want, "HED", hint)
    assert str(e.value) == "HED state dict: 'norm' has shape (3,), expected (1, 3, 1, 1)"
    check_state_dict({**sd, "num_batches_tracked": 0}, want, "HED", hint, ignore=lambda k: k.endswith("tracked"))


def test_hed_raises_through_the_shared_check():
    from controlanimate_amd.hed import check_state_dict as check_hed, hed_key_shapes
    sd = {k: torch.zeros(s) for k, s in hed_key_shapes().items()}
    check_hed(sd)
    del sd["block4.convs.2.bias"]
    with pytest.raises(KeyError) as e:
        check_hed(sd)
    assert e.value.args[0] == ("HED state dict: 'block4.convs.2.bias' is missing (37 tensors expected: norm, block1..5.convs.*.weight|bias, "
                               "block1..5.projection.weight|bias)")
