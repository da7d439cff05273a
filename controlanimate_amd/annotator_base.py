"""What every GPU annotator shares on the host: the frame intake, the `out` contracts, the stage timing, the packed weights' move to
the device, the chunking rule, the weights-file helpers, the buffer plan and the state-dict check.  See DESIGN.md, "The annotator
base".  The hot paths are the kernels under csrc/; nothing here launches one.

A new annotator derives from `AnnotatorBase` and supplies: `__init__` (checks and packs the weights into `self._host`, sets
`self.device`, `self.dtype` and `self._ws = {}`), `workspace(n, h, w)`, `_check_size(h, w)` (NotImplementedError out of scope),
`_network(...)` and `_run(src, map, control, rep)`, the class attributes `WEIGHTS_NAME` and `_bytes_per_pixel`, and a one-line
public `edges(frames, out=None)` (or what its map is called) over `_uint8_out`.

Importing this module imports neither torch, PIL nor the library: those are imported where they are used.
"""
from __future__ import annotations

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


def device_weights(self, dev):
    """self._host on `dev`: moved once, and again only when another device is asked for (the `_weights` of every class that packs its
    weights on the host into a tree `_host` and starts with `_dev = None`)."""
    if self._dev is None or self._dev[0] != dev:
        self._dev = (dev, to_device(self._host, dev))
    return self._dev[1]


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
        numel = int(np.prod(shape))
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


class AnnotatorBase(HipStages):
    """The host side of an annotator for a window of frames: see the module's head for what a subclass supplies."""

    WEIGHTS_NAME = None
    # the largest operand of a chunk of frames (`_bytes_per_pixel` bytes per frame pixel) stays below what the kernels address with 32-bit
    # byte offsets; a plain class attribute, so that an instance can lower it
    max_activation_bytes = 0x7FFFFF00 - 1
    _bytes_per_pixel = None
    _addressed_by = "the kernels"
    _grey_to_rgb = True   # a one-channel frame is repeated to three channels, as the detectors' HWC3 does
    _dev = None
    _weights = device_weights

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

    # ---- chunking ----------------------------------------------------------------------------------------------------------------
    def chunk_frames(self, h: int, w: int) -> int:
        """Frames per pass through the network: as many as keep the largest operand within max_activation_bytes."""
        per_frame = h * w * self._bytes_per_pixel
        if per_frame > self.max_activation_bytes:
            raise ValueError(f"a {h} x {w} frame alone exceeds what {self._addressed_by} address ({per_frame} > {self.max_activation_bytes} bytes)")
        return self.max_activation_bytes // per_frame

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
