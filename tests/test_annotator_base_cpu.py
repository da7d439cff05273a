"""CPU: what the annotators share (controlanimate_amd/annotator_base.py) -- the buffer plan on CPU tensors, the frame intake and the
`out` contracts through a toy subclass (the order of the checks, their messages as HedAnnotator raised them before the base existed,
and that none of them touches the device), and the state-dict check.  No GPU, no library."""
import numpy as np
import pytest
import torch

from controlanimate_amd.annotator_base import AnnotatorBase, BufferPlan, check_state_dict, to_device


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
