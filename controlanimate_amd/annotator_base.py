"""What every model that runs as a packed tree shares on the host: the weight packers, the state-dict check and the weights-file
helpers; `PackedNetwork` (the packed weights' move to the device, the chunking rule, the workspace cache), `NetPass` (one pass through
a network: the buffer plan, the timed launches, the 1x1 and 3x3 layers), `FrameIntake` and `AnnotatorBase` (the `out` contracts).  See
DESIGN.md, "The annotator base".  The hot paths are the kernels under csrc/; here only `NetPass.pointwise` / `.conv3x3` name one.

A new annotator derives from `AnnotatorBase` and supplies: `__init__` (checks the state dict and packs it with the packers below into
`self._host`, sets `self.device`, `self.dtype` and `self._ws = {}`), `workspace(n, h, w)` (its own buffers, through `_workspace`),
`_check_size(h, w)` (NotImplementedError out of scope), `_network(src, ws, i0)` (`with self._pass(ws, src.device) as p:` and then
`p.take`, `p.give`, `p.launch(stage, kernel, ...)`, `p.pointwise`, `p.conv3x3` in the network's own order) and `_run(src, map, control,
rep)` (`for i0, sl in self._chunks(n, self.chunk_frames(h, w))`), the class attributes `WEIGHTS_NAME` and `_bytes_per_pixel`, and a
one-line public `edges(frames, out=None)` (or what its map is called) over `_uint8_out`.  A model that is no annotator derives from
`PackedNetwork` (with `FrameIntake` when it takes frames).

Importing this module imports neither torch, PIL nor the library: those are imported where they are used.
"""
from __future__ import annotations

import math
import os

import numpy as np


def check_state_dict(sd, want: dict, label: str, hint: str, ignore=None) -> None:
    """KeyError naming a tensor of `want` (name -> shape) that `sd` lacks, ValueError naming one that is unexpected (unless ignore(name))
    or has the wrong shape.  label: what the messages call the state dict; hint: what follows "N tensors expected: "."""
    for k in want:
        if k not in sd:
            raise KeyError(f"{label} state dict: '{k}' is missing ({len(want)} tensors expected: {hint})")
    for k in sd:
        if k not in want and not (ignore is not None and ignore(k)):
            raise ValueError(f"{label} state dict: unexpected tensor '{k}'")
    for k, shape in want.items():
        if tuple(sd[k].shape) != shape:
            raise ValueError(f"{label} state dict: '{k}' has shape {tuple(sd[k].shape)}, expected {shape}")


def weights_path(path, name: str) -> str:
    """path: the file, or a directory that holds `name` -> the file's path.  Nothing is ever downloaded."""
    path = os.fspath(path)
    if os.path.isdir(path):
        path = os.path.join(path, name)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path}: no such file (a local {name}, or a directory that holds it; nothing is ever downloaded)")
    return path


def load_state_dict(path, name: str) -> dict:
    """torch.load(weights_only=True) of weights_path(path, name); ValueError when the file holds no dict."""
    import torch
    path = weights_path(path, name)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: not a state dict")
    return sd


def to_device(tree, dev):
    """A tree of tensors (dicts, lists, tuples, None) with every tensor moved to `dev`."""
    import torch
    if tree is None:
        return None
    if isinstance(tree, torch.Tensor):
        return tree.to(dev)
    if isinstance(tree, dict):
        return {k: to_device(v, dev) for k, v in tree.items()}
    return type(tree)(to_device(v, dev) for v in tree)


# ---- packers: a (weight, bias) pair `wb` in PyTorch layout -> what the kernels read ------------------------------------------------------
def bn_key_shapes(prefix: str, c: int) -> dict:
    """The four tensors of a BatchNorm over c channels that is read in eval mode: name -> shape."""
    return {f"{prefix}.weight": (c,), f"{prefix}.bias": (c,), f"{prefix}.running_mean": (c,), f"{prefix}.running_var": (c,)}


def fold_bn(sd, conv: str, bn: str, eps: float):
    """(weight, bias) in fp32 of the convolution `conv` followed by the eval-mode BatchNorm `bn` (key prefixes in `sd`): w * g / sqrt(var +
    eps) per output channel, (b - mean) * g / sqrt(var + eps) + beta, with b zeros when the convolution has no bias."""
    import torch
    w = sd[conv + ".weight"].detach().float()
    b = sd[conv + ".bias"].detach().float() if conv + ".bias" in sd else torch.zeros(w.shape[0])
    scale = sd[bn + ".weight"].detach().float() / torch.sqrt(sd[bn + ".running_var"].detach().float() + eps)
    return w * scale.view(-1, *([1] * (w.dim() - 1))), (b - sd[bn + ".running_mean"].detach().float()) * scale + sd[bn + ".bias"].detach().float()


def _pad_rows(t, rows: int):
    """t with zero rows behind it up to `rows` of them (as it is when it has that many), contiguous; None stays None."""
    import torch
    if t is None:
        return None
    if rows > t.shape[0]:
        t = torch.cat([t, t.new_zeros((rows - t.shape[0], *t.shape[1:]))])
    return t.contiguous()


def pack_conv(wb, dtype, cin_pad: int = 0, cout_pad: int = 0):
    """Conv2d (weight [Cout, Cin, k, k], bias or None) -> ([Cout', k, k, Cin'] of dtype, contiguous fp32 bias [Cout']): zero-padded to
    cin_pad input and cout_pad output channels where it has fewer."""
    import torch
    w = wb[0].detach().float().permute(0, 2, 3, 1)
    if cin_pad > w.shape[3]:
        w = torch.nn.functional.pad(w, (0, cin_pad - w.shape[3]))
    return _pad_rows(w, cout_pad).to(dtype), _pad_rows(None if wb[1] is None else wb[1].detach().float(), cout_pad)


def pack_pointwise(wb, dtype, cout_pad: int = 0):
    """1x1 convolution (weight [Cout, Cin, 1(, 1)], bias or None) -> ([Cout', Cin] of dtype, contiguous fp32 bias [Cout']): the GEMM's
    operands, zero-padded to cout_pad rows where it has fewer."""
    w = wb[0].detach().float()
    return _pad_rows(w.reshape(w.shape[0], -1), cout_pad).to(dtype), _pad_rows(None if wb[1] is None else wb[1].detach().float(), cout_pad)


def pack_depthwise(w, ksizes, expected=None):
    """Depthwise weight [C, 1, k, k] with k out of `ksizes` -> [k * k, C]: tap ky * k + kx of every channel.  expected: how the ValueError
    words the shapes (default "[C, 1, 3, 3] or [C, 1, 5, 5]" for ksizes (3, 5))."""
    if w.dim() != 4 or w.shape[1] != 1 or w.shape[2] != w.shape[3] or w.shape[2] not in ksizes:
        raise ValueError(f"a depthwise weight {expected or ' or '.join(f'[C, 1, {k}, {k}]' for k in ksizes)} is expected, got {tuple(w.shape)}")
    return w.detach().reshape(w.shape[0], -1).t().contiguous()


class BufferPlan:
    """The activation buffers of one pass through a network, out of a workspace's pool (ws["pool"]: [[flat buffer, taken]]; ws["plan"]: the
    slot of the i-th take of a pass, fixed by the first pass; ws["planned"]).  The layers take and give buffers in a fixed order; the first
    pass allocates them and every later pass gets the same ones in the same order, so nothing is allocated after it and a captured graph
    stays valid.  The caller sets ws["planned"] when a pass has finished (a first pass that did not finish starts over)."""

    def __init__(self, ws: dict, dtype, device):
        self.pool, self.plan, self.replay, self.cursor = ws["pool"], ws["plan"], ws["planned"], 0
        self.dtype, self.device = dtype, device
        if not self.replay:
            self.plan.clear()
        for slot in self.pool:
            slot[1] = False

    def take(self, *shape):
        import torch
        numel = math.prod(shape)
        pool = self.pool
        if self.replay:
            slot = pool[self.plan[self.cursor]]
            self.cursor += 1
            assert not slot[1] and slot[0].numel() >= numel
        else:
            free = [i for i, sl in enumerate(pool) if not sl[1] and sl[0].numel() >= numel]
            if not free:
                pool.append([torch.empty(numel, dtype=self.dtype, device=self.device), False])
                free = [len(pool) - 1]
            self.plan.append(min(free, key=lambda i: pool[i][0].numel()))
            slot = pool[self.plan[-1]]
        slot[1] = True
        return slot[0][:numel].view(*shape)

    def give(self, t) -> None:
        for slot in self.pool:
            if slot[0].data_ptr() == t.data_ptr():
                slot[1] = False
                return
        raise AssertionError("not a pool buffer")


class HipStages:
    """A host object that launches stages on the GPU: the device it runs on, and events around its stages when someone times them."""

    device = None
    timings = None  # a dict: receives (start, end) torch events per launch under its stage's name (the keys of the module's STAGES) -- tools/bench_*.py
    _no_gpu_hint = "(there is no CPU fallback)"

    def _device(self):
        import torch
        from . import _capi
        _capi.lib()  # CAHipUnavailable when the extension is not built
        if not torch.cuda.is_available():
            raise _capi.CAHipUnavailable(f"{type(self).__name__} needs a GPU {self._no_gpu_hint}")
        return torch.device(self.device if self.device is not None else "cuda")

    def _stage(self, name):
        import torch
        if self.timings is None:
            return None
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        self.timings.setdefault(name, []).append(ev)
        ev[0].record()
        return ev

    def _timed(self, name, fn, *args, **kw):
        """fn(*args, **kw) as one launch of the stage `name`."""
        ev = self._stage(name)
        out = fn(*args, **kw)
        if ev:
            ev[1].record()
        return out


class PackedNetwork(HipStages):
    """A model whose weights are packed once on the host into a tree `self._host` and that runs in passes over chunks of its input, on
    buffers kept per input shape in `self._ws`: see the module's head for what a subclass supplies."""

    WEIGHTS_NAME = None
    # the largest operand of a chunk of frames (`_bytes_per_pixel` bytes per frame pixel) stays below what the kernels address with 32-bit
    # byte offsets; a plain class attribute, so that an instance can lower it
    max_activation_bytes = 0x7FFFFF00 - 1
    _bytes_per_pixel = None
    _addressed_by = "the kernels"
    _host = None
    _dev = None

    # ---- the weights file --------------------------------------------------------------------------------------------------------
    @classmethod
    def _weights_path(cls, path) -> str:
        return weights_path(path, cls.WEIGHTS_NAME)

    @classmethod
    def _load(cls, path):
        return load_state_dict(path, cls.WEIGHTS_NAME)

    @classmethod
    def from_pretrained(cls, path, **kwargs):
        """path: the local weights file (the class's WEIGHTS_NAME) or a directory that holds it (no network access, ever)."""
        return cls(cls._load(path), **kwargs)

    def _weights(self, dev):
        """self._host on `dev`: moved once, and again only when another device is asked for."""
        if self._dev is None or self._dev[0] != dev:
            self._dev = (dev, to_device(self._host, dev))
        return self._dev[1]

    # ---- chunking ----------------------------------------------------------------------------------------------------------------
    def chunk_frames(self, h: int, w: int) -> int:
        """Frames per pass through the network: as many as keep the largest operand within max_activation_bytes."""
        per_frame = h * w * self._bytes_per_pixel
        if per_frame > self.max_activation_bytes:
            raise ValueError(f"a {h} x {w} frame alone exceeds what {self._addressed_by} address ({per_frame} > {self.max_activation_bytes} bytes)")
        return self.max_activation_bytes // per_frame

    @staticmethod
    def _chunks(n: int, step: int):
        """(i0, slice(i0, i1)) of the passes over n items, `step` of them at a time."""
        for i0 in range(0, n, step):
            yield i0, slice(i0, min(i0 + step, n))

    # ---- device state ------------------------------------------------------------------------------------------------------------
    def _workspace(self, key, make, dev=None):
        """The buffers of a call, cached under `key`: what make(device) returns, and in a dict the pool, plan and flag of a NetPass."""
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = make(self._device() if dev is None else dev)
            if isinstance(ws, dict):
                ws.update(pool=[], plan=[], planned=False)
        return ws

    def _pass(self, ws: dict, device):
        """`with self._pass(ws, device) as p:` -- one pass through the network on the workspace's pool."""
        return NetPass(self, ws, device)


class NetPass(BufferPlan):
    """One pass through a network: the buffer plan of the workspace `ws`, the launches as stages of `net`, and the two layers every
    network has.  Gives stay explicit and each network keeps its own order: a captured graph is valid only if every pass repeats it.
    Leaving the `with` block sets ws["planned"]; an exception leaves it as it was, so a first pass that failed plans again."""

    def __init__(self, net, ws: dict, device):
        from . import kernels
        super().__init__(ws, net.dtype, device)
        self.ws, self.launch, self.K = ws, net._timed, kernels   # launch(stage, fn, *args, **kw): fn(*args, **kw) as one launch of `stage`

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.ws["planned"] = True
        return False

    def pointwise(self, stage, x, wb, act=0, residual=None, a2=None, out2d=None, out_f32=False):
        """1x1 convolution of x [..., C] (NHWC, or pixels x C) as a GEMM over its pixels, wb = (weight [N, K], bias).  The output is taken
        here, in x's leading shape, and returned -- or written to out2d, a [pixels, N] view (possibly a column slice of a wider tensor),
        and None returned.  residual and a2 (a second source of the same pixels, behind x along K) are viewed [pixels, .] likewise.
        act: a CA_ACT_* code (0: none)."""
        c = x.shape[-1]
        m = x.numel() // c
        y = None
        if out2d is None:
            y = self.take(*x.shape[:-1], wb[0].shape[0])
            out2d = y.view(m, -1)
        self.launch(stage, self.K.gemm, x.view(m, c), wb[0], a2=None if a2 is None else a2.view(m, -1), bias=wb[1], act=act,
                    residual=None if residual is None else residual.view(m, -1), out=out2d, out_f32=out_f32)
        return y

    def conv3x3(self, stage, x, wb, stride=1, act=0, **kw):
        """3x3 convolution (padding 1) of NHWC x into an output taken here, wb = (weight [Cout, 3, 3, Cin], bias); kw: ca_conv3x3's further
        arguments."""
        n, h, w, _ = x.shape
        return self.launch(stage, self.K.conv3x3, x, wb[0], bias=wb[1], stride=stride, act=act,
                           out=self.take(n, (h - 1) // stride + 1, (w - 1) // stride + 1, wb[0].shape[0]), **kw)


class FrameIntake:
    """The frames of a call for a class with `_device()`: uint8, one size, in the class's scope -- checked before the device is touched."""

    _grey_to_rgb = True   # a one-channel frame is repeated to three channels, as the detectors' HWC3 does

    # ---- input checks ------------------------------------------------------------------------------------------------------------
    def _check_size(self, h: int, w: int) -> None:
        """NotImplementedError for a frame size out of the annotator's scope (here: every size is in scope)."""

    def _frames(self, frames):
        """-> uint8 device tensor [n, H, W, 3] ([n, H, W, C], C = 1 or 3, where _grey_to_rgb is off).  The type, size and scope checks
        come before the device is touched.  A PIL image is taken as np.asarray gives it, so its mode must be L or RGB."""
        import torch
        if isinstance(frames, torch.Tensor):
            if frames.dtype != torch.uint8:
                raise TypeError(f"frames must be uint8, got {frames.dtype}")
            if frames.dim() == 3:
                frames = frames[..., None]
            if frames.dim() != 4 or frames.shape[3] not in (1, 3):
                raise ValueError(f"frames tensor must be [n, H, W] or [n, H, W, C] with C = 1 or 3, got {tuple(frames.shape)}")
            self._check_size(frames.shape[1], frames.shape[2])
            dev = self._device()
            if self._grey_to_rgb and frames.shape[3] == 1:
                frames = frames.expand(-1, -1, -1, 3)
            return frames.to(dev).contiguous()
        host = []
        for fr in frames:
            a = np.asarray(fr)
            if a.dtype != np.uint8:
                raise TypeError(f"frames must be uint8, got {a.dtype}")
            if a.ndim == 2:
                a = a[:, :, None]
            if a.ndim != 3 or a.shape[2] not in (1, 3):
                raise ValueError(f"a frame must be [H, W] or [H, W, C] with C = 1 or 3 (PIL mode L or RGB: convert RGBA or palette "
                                 f"frames with .convert('RGB') first), got {a.shape}" + (f" from PIL mode {fr.mode}" if hasattr(fr, "mode") else ""))
            host.append(a)
        if not host:
            raise ValueError("no frames")
        if any(a.shape != host[0].shape for a in host):
            raise ValueError("all frames of a call must share one size")
        self._check_size(host[0].shape[0], host[0].shape[1])
        dev = self._device()
        stack = np.stack(host)
        if self._grey_to_rgb and stack.shape[3] == 1:
            stack = np.repeat(stack, 3, axis=3)
        return torch.from_numpy(stack).to(dev)


class AnnotatorBase(FrameIntake, PackedNetwork):
    """The host side of an annotator for a window of frames: see the module's head for what a subclass supplies."""

    # ---- outputs -----------------------------------------------------------------------------------------------------------------
    def _uint8_out(self, frames, out, channels_last=None):
        """The annotator's uint8 map of `frames` on the device, [n, H, W] (or [n, H, W, channels_last]), written into `out` when given."""
        import torch
        src = self._frames(frames)
        n, h, w, _ = src.shape
        shape = (n, h, w) if channels_last is None else (n, h, w, channels_last)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=src.device)
        elif out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != src.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous uint8 tensor {shape} on {src.device}")
        if n:
            self._run(src, out, None, 1)
        return out

    def annotate_batch(self, frames, out=None, rep: int = 1, dtype=None):
        """-> the control tensor [rep * n, 3, H, W] on the device, map / 255 (three equal channels for a one-channel map); rep = 2 writes
        the n frames twice (torch.cat([ctrl] * 2) of classifier-free guidance).  Written into `out` (and `out` returned) when given."""
        import torch
        if rep not in (1, 2):
            raise ValueError(f"rep={rep} (1 or 2)")
        want = out.dtype if out is not None and dtype is None else (dtype if dtype is not None else torch.float32)
        if want not in (torch.float32, torch.float16):
            raise TypeError(f"the control tensor is float32 or float16, got {want}")
        src = self._frames(frames)
        n, h, w, _ = src.shape
        if out is None:
            out = torch.empty((rep * n, 3, h, w), dtype=want, device=src.device)
        elif tuple(out.shape) != (rep * n, 3, h, w) or out.device != src.device or not out.is_contiguous() or out.dtype != want:
            raise ValueError(f"out must be a contiguous {want} tensor {(rep * n, 3, h, w)} on {src.device}")
        if n:
            self._run(src, None, out, rep)
        return out

    def __call__(self, image):
        """PIL in, PIL RGB with three equal channels out; an array in, an array out (the contract of `annotators.canny`)."""
        try:
            from PIL import Image
        except Exception:  # pragma: no cover
            Image = None
        e = self._uint8_out([image], None)[0].cpu().numpy()
        rgb = np.repeat(e[:, :, None], 3, axis=2)
        return Image.fromarray(rgb) if Image is not None and not isinstance(image, np.ndarray) else rgb
