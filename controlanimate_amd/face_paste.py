"""The paste-back behind gfpgan.FaceRestorer: the back half of facexlib's FaceRestoreHelper as GFPGANer.enhance(img, paste_back=True) drives it
(modules/upscaler.py:70 of the reference) -- ParseNet on every restored 512 x 512 face, the parsing mask's colour map, two Gaussian blurs, the
inverse warp and the blend -- for a whole window, ending in the uint8 frames `[n, h_up, w_up, 3]` on the device.  Opt-in: nothing calls it
unless a `FacePaster` is handed to `face_align.FaceHelper(aligner, paster=...)` or to `FaceEnhancer`.

    network  ParseNet(in_size 512, base_ch 64, parsing_ch 19, res_depth 10, LeakyReLU(0.2), BatchNorm, ch_range [32, 256]): a plain 3 -> 64
             convolution, four 'down' residual blocks to 256 channels at 32 x 32, ten plain blocks, feat + body(feat), four 'up' blocks back to
             64 channels at 512 x 512, a 64 -> 19 convolution; every convolution 3 x 3 behind ReflectionPad2d(1); BatchNorm folded on the host
    mask     argmax over the 19 maps (the first maximum), MASK_COLORMAP -> 0 / 255; cv2.GaussianBlur((101, 101), 11) twice in float64; the
             outer 10 rows and columns zeroed; / 255
    paste    per face in order: cv2.warpAffine of the restored face and of the mask with the inverse affine (+ 0.5 f on its translation when
             f > 1), img = m face + (1 - m) img in float64; one astype(uint8) at the end

It runs as (the names are the keys of `FacePaster.timings`; launches per pass of a chunk of faces with ca_conv3x3_reflect everywhere -- the
ring route below swaps the stride-1 layers for ca_ring_fill + ca_conv3x3):

    prep      1   ca_parse_prep: ((byte / 255) - 0.5) / 0.5, the channels reversed unless bgr, padded to 32 channels
    encoder  13   ca_conv3x3_reflect: the plain convolution, then per 'down' block the stride-2 shortcut, conv1 and the stride-2 conv2 with the
                  shortcut as its residual
    body     21   per plain block two ca_conv3x3_reflect (the block's input as conv2's residual); ca_add_bcast for feat + body(feat)
    decoder  12   per 'up' block the shortcut and conv1 on the nearest x2 source (ca_conv3x3_reflect(up2): the x2 plane is never written) and
                  conv2 with the shortcut as its residual
    mask      1   ca_parse_mask: the last layer, the argmax and the colour map in one launch (the 19 fp32 planes never reach memory);
                  `logits` / `labels` run the composed form instead: ca_conv3x3_reflect with fp32 output + ca_parse_labels
    blur      4   ca_mask_blur: row, column, row, column pass through LDS
    paste     1   ca_face_paste (+ ca_resize_lanczos4_u8 in front when the background is not h_up x w_up yet)

THE RING ROUTE.  `context.dispatch.parse_conv_reflect = True` runs every convolution on ca_conv3x3_reflect, as listed above.  False (the
default), or a collection of plane sizes, stores the activations of those levels as ringed tensors [n, P + 2, P + 2, C] and runs their
stride-1 convolutions on the tuned, zero-padded ca_conv3x3 over the whole ringed tensor (its interior is right), with ca_ring_fill
refilling the ring in front of each; the stride-2 and x2 layers, the first (3-channel) layer and the mask launch read and write the ringed
tensors' interiors with ca_conv3x3_reflect.  Measured (tools/bench_facepaste.py, profiles/facepaste_bench.json): the ring
route takes 0.59 - 0.80 of the new kernel's time per stride-1 layer from 64 x 64 up and the same at 32 x 32; the whole network 30.75 ms
against 34.96 ms for 32 faces.

UNPINNED.  The specification is tests/facepaste_ref.py, restated from memory of facexlib's published code and of OpenCV's GaussianBlur /
warpAffine: facexlib and OpenCV are absent here and no parsing_parsenet.pth is available.  Not settled by memory: the checkpoint's key names,
the summation order inside OpenCV's blur (the specification fixes k0 x0 + sum k_i (x_-i + x_+i), i ascending), and flags=3 of the mask's warp
(taken as bilinear).  The reference runs ParseNet in fp32; this runs fp16 / bf16 activations with fp32 sums, so a pixel whose two best maps
are closer than the activation error can take either label.  The range of fp16 activations on the trained checkpoint is unmeasured;
dtype=torch.bfloat16 is the escape.

Scope: use_parse=True only; 3-channel uint8 frames; no save_path; no CPU fallback (CAHipUnavailable).  ParseNet and the blur run on all
n * max_faces slots (an empty slot holds the aligner's border crop; the paste kernel never reads it), so nothing is read back to the host.
"""
from __future__ import annotations

import math
import os
from typing import NamedTuple

import numpy as np

from . import annotator_base as _base
from .annotator_base import PackedNetwork, bn_key_shapes as _bn, check_state_dict as _check_state_dict, pack_conv

WEIGHTS_NAME = "parsing_parsenet.pth"
STAGES = ("prep", "encoder", "body", "decoder", "mask", "blur", "paste")
PARSING_CH, CPAD, MIN_FEAT, FACE_SIZE = 19, 32, 32, 512
BN_EPS = 1e-5
BLUR_KSIZE, BLUR_SIGMA = 101, 11.0
MASK_COLORMAP = (0, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 0, 255, 0, 0, 0)


class Geometry(NamedTuple):
    in_size: int        # the faces' side (= out_size)
    base_ch: int
    res_depth: int
    ch_range: tuple     # (lowest, highest) width


PARSENET = Geometry(512, 64, 10, (32, 256))


def check_geometry(geo) -> None:
    steps = math.log2(geo.in_size / MIN_FEAT) if geo.in_size >= MIN_FEAT else -1
    ok = (steps >= 1 and steps == int(steps) and geo.res_depth >= 1 and len(geo.ch_range) == 2
          and all(c in (32, 64, 128, 256) for c in (geo.base_ch, *geo.ch_range)) and geo.ch_range[0] <= geo.base_ch <= geo.ch_range[1])
    if not ok:
        raise ValueError(f"geometry out of the kernels' range (in_size 32 * 2^k with k >= 1, res_depth >= 1, base_ch and ch_range out of 32, 64, 128, 256): {geo}")


def blocks_of(geo=PARSENET):
    """[(name, cin, cout, scale)] of the residual blocks in order (encoder.1 .., body.0 .., decoder.0 ..), widths clipped to ch_range."""
    lo, hi = geo.ch_range
    steps = int(round(math.log2(geo.in_size // MIN_FEAT)))

    def clip(c):
        return max(lo, min(hi, c))

    out, head = [], geo.base_ch
    for i in range(steps):
        out.append((f"encoder.{i + 1}", clip(head), clip(head * 2), "down"))
        head *= 2
    for i in range(geo.res_depth):
        out.append((f"body.{i}", clip(head), clip(head), "none"))
    for i in range(steps):
        out.append((f"decoder.{i}", clip(head), clip(head // 2), "up"))
        head //= 2
    return out


def has_shortcut(cin: int, cout: int, scale: str) -> bool:
    return not (scale == "none" and cin == cout)


def parsenet_key_shapes(geo=PARSENET) -> dict:
    """Every tensor of parsing_parsenet.pth that the chain uses (facexlib's names, from memory): name -> shape."""
    out = {"encoder.0.conv2d.weight": (geo.base_ch, 3, 3, 3), "encoder.0.conv2d.bias": (geo.base_ch,)}
    for name, cin, cout, scale in blocks_of(geo):
        if has_shortcut(cin, cout, scale):
            out[f"{name}.shortcut_func.conv2d.weight"], out[f"{name}.shortcut_func.conv2d.bias"] = (cout, cin, 3, 3), (cout,)
        out[f"{name}.conv1.conv2d.weight"] = (cout, cin, 3, 3)
        out.update(_bn(f"{name}.conv1.norm.norm", cout))
        out[f"{name}.conv2.conv2d.weight"] = (cout, cout, 3, 3)
        out.update(_bn(f"{name}.conv2.norm.norm", cout))
    out["out_mask_conv.conv2d.weight"], out["out_mask_conv.conv2d.bias"] = (PARSING_CH, blocks_of(geo)[-1][2], 3, 3), (PARSING_CH,)
    return out


def _ignored(k: str) -> bool:
    # out_img_conv is in the checkpoint and its result is discarded by facexlib's caller: accepted, never run; BatchNorm's step counter is never read
    return k.startswith("out_img_conv.") or k.endswith("num_batches_tracked")


def check_state_dict(sd, geo=PARSENET) -> None:
    """KeyError naming a missing tensor, ValueError naming one that is unexpected or has the wrong shape."""
    _check_state_dict(sd, parsenet_key_shapes(geo), "parsenet", "encoder.0, encoder.1 .. / body.N / decoder.N .{shortcut_func, conv1, conv2} and out_mask_conv",
                      ignore=_ignored)


def fold_bn(sd, conv: str):
    """(weight, bias) in fp32 of the ConvLayer `conv`: its bias-free convolution followed by its eval-mode BatchNorm when it has one, else
    the convolution's own weight and bias."""
    if conv + ".norm.norm.weight" not in sd:
        return sd[conv + ".conv2d.weight"].detach().float(), sd[conv + ".conv2d.bias"].detach().float()
    return _base.fold_bn(sd, conv + ".conv2d", conv + ".norm.norm", BN_EPS)


def pack_network(sd, geo, dtype) -> dict:
    """The packed weights of the chain as a tree of host tensors: BatchNorm folded in fp32, rounded once to dtype."""
    out = {"in": pack_conv(fold_bn(sd, "encoder.0"), dtype, cin_pad=CPAD), "blocks": [],
           "mask": pack_conv(fold_bn(sd, "out_mask_conv"), dtype, cout_pad=CPAD)}
    for name, cin, cout, scale in blocks_of(geo):
        blk = {"conv1": pack_conv(fold_bn(sd, name + ".conv1"), dtype), "conv2": pack_conv(fold_bn(sd, name + ".conv2"), dtype)}
        if has_shortcut(cin, cout, scale):
            blk["shortcut"] = pack_conv(fold_bn(sd, name + ".shortcut_func"), dtype)
        out["blocks"].append(blk)
    return out


def gaussian_half_taps(ksize: int = BLUR_KSIZE, sigma: float = BLUR_SIGMA) -> np.ndarray:
    """cv2.getGaussianKernel(ksize, sigma) in float64 -- exp(-x^2 / (2 sigma^2)) divided by the sum taken in index order -- from its centre
    tap on: float64 [(ksize + 1) / 2], what ca_mask_blur takes.  No exp runs on the device."""
    r = (ksize - 1) // 2
    e = np.array([math.exp(-(i - r) * (i - r) / (2.0 * sigma * sigma)) for i in range(ksize)], np.float64)
    s = 0.0
    for v in e:
        s += v
    return np.ascontiguousarray((e * (1.0 / s))[r:])


def _bytes_per_face_pixel(geo) -> int:
    """The largest activation of a face, in bytes per pixel of the (ringed) in_size plane: 16-bit elements."""
    worst, level = max(CPAD, geo.base_ch), 1          # level: the plane's side is in_size / level
    for _, cin, cout, scale in blocks_of(geo):
        if scale == "down":
            worst = max(worst, cout / level ** 2)     # conv1's output, before the stride
            level *= 2
        elif scale == "up":
            level //= 2
        worst = max(worst, cout / level ** 2)
    return int(math.ceil(2 * worst))


class FacePaster(PackedNetwork):
    """`FacePaster.from_pretrained(path).paste(background, restored, inverse_affine, count)`: ParseNet, the mask blur and the blend on the HIP
    kernels.  Non-uint8 input raises TypeError, wrong shapes ValueError -- before the device is touched; without the library or a GPU a call
    raises CAHipUnavailable (there is no CPU fallback)."""

    WEIGHTS_NAME = WEIGHTS_NAME
    STAGES = STAGES

    def __init__(self, state_dict_or_path, dtype=None, device=None, geometry=PARSENET):
        import torch
        dtype = torch.float16 if dtype is None else dtype
        if dtype not in (torch.float16, torch.bfloat16):
            raise TypeError(f"dtype must be torch.float16 or torch.bfloat16, got {dtype}")
        geometry = Geometry(*geometry)
        check_geometry(geometry)
        sd = self._load(state_dict_or_path) if isinstance(state_dict_or_path, (str, os.PathLike)) else state_dict_or_path
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
        check_state_dict(sd, geometry)
        self.device, self.dtype, self.geometry = device, dtype, geometry
        self._bytes_per_pixel = _bytes_per_face_pixel(geometry)
        self._host = pack_network(sd, geometry, dtype)
        self._host["taps"] = torch.from_numpy(gaussian_half_taps())
        self._ws, self._tables, self._resized_bg = {}, {}, {}

    @classmethod
    def from_pretrained(cls, path, dtype=None, device=None, **kwargs):
        """path: a local parsing_parsenet.pth or a directory that holds it (no network access, ever)."""
        return cls(cls._load(path), dtype=dtype, device=device, **kwargs)

    # ---- input checks ----------------------------------------------------------------------------------------------------------
    def _faces(self, faces):
        """-> uint8 device tensor [m, S, S, 3]; the checks come before the device is touched."""
        import torch
        s = self.geometry.in_size
        if not isinstance(faces, torch.Tensor):
            arrs = [np.asarray(f) for f in faces]
            if not arrs:
                raise ValueError("no faces")
            if any(a.dtype != np.uint8 for a in arrs):
                raise TypeError(f"faces must be uint8, got {sorted({str(a.dtype) for a in arrs})}")
            if any(a.shape != (s, s, 3) for a in arrs):
                raise ValueError(f"a face is {s} x {s} x 3, got {sorted({a.shape for a in arrs})}")
            faces = torch.from_numpy(np.stack(arrs))
        if faces.dtype != torch.uint8:
            raise TypeError(f"faces must be uint8, got {faces.dtype}")
        if faces.dim() != 4 or tuple(faces.shape[1:]) != (s, s, 3) or faces.shape[0] < 1:
            raise ValueError(f"a face tensor is uint8 [m, {s}, {s}, 3], got {tuple(faces.shape)}")
        return faces.to(self._device()).contiguous()

    # ---- device state ----------------------------------------------------------------------------------------------------------
    def ring_levels(self) -> frozenset:
        """The plane sizes whose activations are ringed tensors (their stride-1 convolutions take the ring route), from the dispatch switch."""
        from .context import dispatch
        sw = dispatch.parse_conv_reflect
        if sw is True:
            return frozenset()
        levels = {self.geometry.in_size >> k for k in range(int(math.log2(self.geometry.in_size // MIN_FEAT)) + 1)}
        return frozenset(levels) if sw is False else frozenset(int(p) for p in sw) & levels

    def workspace(self, m: int) -> dict:
        """The buffers of a call with m faces, cached per (m, ring levels): the masks, the blur's scratch and output, and a pool of activation
        buffers that the layers of a pass take and give back in a fixed order (the first pass allocates them, every later pass reuses them)."""
        import torch
        s = self.geometry.in_size
        return self._workspace((m, self.ring_levels()), lambda dev: {
            "mask": torch.empty((m, s, s), dtype=torch.uint8, device=dev), "labels": None, "logits": None,
            "blur": torch.empty((m, s, s), dtype=torch.float64, device=dev), "soft": torch.empty((m, s, s), dtype=torch.float64, device=dev)})

    # ---- the chain -------------------------------------------------------------------------------------------------------------
    def _trunk(self, p, src, bgr: bool):
        """ParseNet up to the decoder's output for the faces `src` (a chunk) on the pass `p` -> x [m, S, S, head channels] or ringed.  The
        caller gives x back."""
        from . import kernels as K
        wts = self._weights(src.device)
        rings = self.ring_levels()
        m, s = src.shape[0], src.shape[1]
        launch = p.launch
        filled = set()      # the ringed buffers whose ring holds the reflection of their present interior

        def take(side, c):
            return p.take(m, side + 2, side + 2, c) if side in rings else p.take(m, side, side, c)

        def conv(stage, x, side, wb, stride=1, up2=False, leaky=False, residual=None, reflect=False):
            """One ConvLayer on the plane of side `side` -> (y, its side).  reflect: ca_conv3x3_reflect whatever the level's route."""
            po = 2 * side if up2 else (side - 1) // stride + 1
            y = take(po, wb[0].shape[0])
            if side in rings and stride == 1 and not up2 and not reflect:
                if x.data_ptr() not in filled:
                    launch(stage, K.ring_fill, x)
                    filled.add(x.data_ptr())
                launch(stage, K.conv3x3, x, wb[0], bias=wb[1], residual=residual, act=K.ACT_LEAKY02 if leaky else K.ACT_NONE, out=y, split_k=False)
            else:
                launch(stage, K.conv3x3_reflect, x, wb[0], wb[1], stride=stride, up2=up2, leaky=leaky, residual=residual, out=y, in_ring=side in rings,
                       out_ring=po in rings, res_ring=po in rings)
            filled.discard(y.data_ptr())
            return y, po

        def give(t):
            filled.discard(t.data_ptr())
            p.give(t)

        x0 = take(s, CPAD)
        launch("prep", K.parse_prep, src, x0, not bgr, s in rings)
        x, side = conv("encoder", x0, s, wts["in"], reflect=True)   # K = 32 of which 3 channels are live: ca_conv3x3 measured 2.2x slower on it
        give(x0)
        feat = None
        for (name, cin, cout, scale), blk in zip(blocks_of(self.geometry), wts["blocks"]):
            stage = name.split(".")[0]
            if scale == "none" and feat is None:
                feat = x
            idn = x
            if "shortcut" in blk:
                idn, _ = conv(stage, x, side, blk["shortcut"], stride=2 if scale == "down" else 1, up2=scale == "up")
            y, py = conv(stage, x, side, blk["conv1"], up2=scale == "up", leaky=True)
            z, pz = conv(stage, y, py, blk["conv2"], stride=2 if scale == "down" else 1, residual=idn)
            give(y)
            if idn is not x:
                give(idn)
            if x is not feat:
                give(x)
            x, side = z, pz
            if name == f"body.{self.geometry.res_depth - 1}":
                launch("body", K.add_bcast, feat, x, x)      # feat + body(feat), in place (ringed buffers: the rings are rewritten before they are read)
                give(feat)
        return x

    def _masks_u8(self, src, ws, bgr: bool, composed: bool = False):
        """The 0 / 255 masks of all faces into ws["mask"], in chunks; composed: through fp32 logits (kept in ws["logits"]) and ws["labels"]."""
        import torch
        from . import kernels as K
        m, s = src.shape[0], src.shape[1]
        passes = -(-m // self.chunk_frames(s + 2, s + 2))
        wts = self._weights(src.device)
        if composed and ws["logits"] is None:
            ws["logits"] = torch.empty((m, s, s, CPAD), dtype=torch.float32, device=src.device)
            ws["labels"] = torch.empty((m, s, s), dtype=torch.uint8, device=src.device)
        ring = s in self.ring_levels()
        for _, sl in self._chunks(m, -(-m // passes)):      # an even split
            with self._pass(ws, src.device) as p:
                x = self._trunk(p, src[sl], bgr)
                if composed:
                    p.launch("mask", K.conv3x3_reflect, x, wts["mask"][0], wts["mask"][1], out_f32=True, out=ws["logits"][sl], in_ring=ring)
                    p.launch("mask", K.parse_labels, ws["logits"][sl], ws["labels"][sl], ws["mask"][sl])
                else:
                    p.launch("mask", K.parse_mask, x, wts["mask"][0], wts["mask"][1], ws["mask"][sl], ring)
                p.give(x)
        return ws["mask"]

    # ---- the public surface ------------------------------------------------------------------------------------------------------
    def logits(self, faces, bgr: bool = False):
        """-> the 19 parsing maps, float32 [m, S, S, 19] on the device (the composed form; a new tensor).  A view for tests and tools: the
        fp32 maps of ALL m faces are kept, [m, S, S, 32] whatever the chunking (33.5 MB per face at 512 x 512), plus the copy returned."""
        src = self._faces(faces)
        ws = self.workspace(src.shape[0])
        self._masks_u8(src, ws, bool(bgr), composed=True)
        return ws["logits"][..., :PARSING_CH].clone()

    def labels(self, faces, bgr: bool = False):
        """-> the parsing labels, uint8 [m, S, S] on the device (the composed form: fp32 logits, then the first maximum; a new tensor).  Keeps
        the fp32 maps of all m faces like `logits`."""
        src = self._faces(faces)
        ws = self.workspace(src.shape[0])
        self._masks_u8(src, ws, bool(bgr), composed=True)
        return ws["labels"].clone()

    def hard_masks(self, faces, bgr: bool = False, composed: bool = False):
        """-> MASK_COLORMAP[labels], uint8 [m, S, S] of 0 / 255 on the device: ca_parse_mask's one launch, or the composed form (a new tensor)."""
        src = self._faces(faces)
        return self._masks_u8(src, self.workspace(src.shape[0]), bool(bgr), composed=composed).clone()

    def blur(self, mask_u8, out=None, ws=None):
        """uint8 masks [m, 512, 512] on the device -> the float64 soft masks: blurred twice, the border zeroed, / 255 (tests plant masks here)."""
        import torch
        from . import kernels as K
        if mask_u8.dtype != torch.uint8 or mask_u8.dim() != 3 or tuple(mask_u8.shape[1:]) != (FACE_SIZE, FACE_SIZE):
            raise ValueError(f"masks are uint8 [m, {FACE_SIZE}, {FACE_SIZE}], got {mask_u8.dtype} {tuple(mask_u8.shape)}")
        dev = self._device()
        mask_u8 = mask_u8.to(dev).contiguous()
        if out is None:
            out = torch.empty(mask_u8.shape, dtype=torch.float64, device=dev)
        if ws is None:
            ws = torch.empty(mask_u8.shape, dtype=torch.float64, device=dev)
        return self._timed("blur", K.mask_blur, mask_u8, self._weights(dev)["taps"], ws, out)

    def masks(self, faces, bgr: bool = False):
        """-> the float64 blurred masks [m, 512, 512] on the device (the workspace's tensor: the next call on m faces overwrites it)."""
        if self.geometry.in_size != FACE_SIZE:
            raise NotImplementedError(f"the blur and the paste take {FACE_SIZE} x {FACE_SIZE} masks; this geometry's are {self.geometry.in_size}")
        src = self._faces(faces)
        ws = self.workspace(src.shape[0])
        return self.blur(self._masks_u8(src, ws, bool(bgr)), ws["soft"], ws["blur"])

    def _resized(self, background, h_up: int, w_up: int):
        """cv2.resize(background, (w_up, h_up), INTER_LANCZOS4) on the device, into a buffer kept per shape (a second call on the same shapes
        allocates nothing); at equal size the tensor itself (no launch)."""
        import torch
        from . import kernels as K
        from .upscaler import lanczos4_tables
        n, h, w, _ = background.shape
        if (h, w) == (h_up, w_up):
            return background
        tabs = []
        for src, dst in ((w, w_up), (h, h_up)):
            if (src, dst) not in self._tables:
                ofs, coef = lanczos4_tables(src, dst)
                self._tables[(src, dst)] = (torch.from_numpy(ofs).to(background.device), torch.from_numpy(coef).to(background.device))
            tabs.append(self._tables[(src, dst)])
        key = (n, h, w, h_up, w_up)
        if key not in self._resized_bg:
            self._resized_bg[key] = torch.empty((n, h_up, w_up, 3), dtype=torch.uint8, device=background.device)
        return self._timed("paste", K.resize_lanczos4_u8, background, h_up, w_up, tabs[0][0], tabs[0][1], tabs[1][0], tabs[1][1], out=self._resized_bg[key])

    def paste_masks(self, background, restored, masks, inverse_affine, count, upscale_factor: float = 1, out=None, frame_size=None):
        """The blend alone, with the soft masks given (float64 [n * max_faces, 512, 512]; tests plant them).  See `paste`."""
        import torch
        from . import kernels as K
        for name, t, dt in (("background", background, torch.uint8), ("restored", restored, torch.uint8), ("masks", masks, torch.float64),
                            ("inverse_affine", inverse_affine, torch.float64), ("count", count, torch.int32)):
            if not isinstance(t, torch.Tensor) or t.dtype != dt:
                raise TypeError(f"{name} must be a {dt} tensor, got {getattr(t, 'dtype', type(t).__name__)}")
        if background.dim() != 4 or background.shape[3] != 3 or background.shape[0] < 1:
            raise ValueError(f"background is uint8 [n, H, W, 3], got {tuple(background.shape)}")
        n = background.shape[0]
        if inverse_affine.dim() != 4 or inverse_affine.shape[0] != n or tuple(inverse_affine.shape[2:]) != (2, 3) or tuple(count.shape) != (n,):
            raise ValueError(f"inverse_affine is float64 [n, max_faces, 2, 3] and count int32 [n] with n = {n}, got {tuple(inverse_affine.shape)} and {tuple(count.shape)}")
        mf = inverse_affine.shape[1]
        if tuple(restored.shape) != (n * mf, FACE_SIZE, FACE_SIZE, 3) or tuple(masks.shape) != (n * mf, FACE_SIZE, FACE_SIZE):
            raise ValueError(f"restored is uint8 [{n * mf}, 512, 512, 3] and masks float64 [{n * mf}, 512, 512], got {tuple(restored.shape)} and {tuple(masks.shape)}")
        f = float(upscale_factor)
        if f <= 0:
            raise ValueError(f"upscale_factor={upscale_factor} (> 0)")
        h, w = frame_size if frame_size is not None else background.shape[1:3]
        h_up, w_up = int(h * f), int(w * f)
        if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (n, h_up, w_up, 3) or not out.is_contiguous()
                                or not out.is_cuda):
            raise ValueError(f"out: a contiguous uint8 tensor {(n, h_up, w_up, 3)} on the device")
        dev = self._device()
        bg = self._resized(background.to(dev).contiguous(), h_up, w_up)
        if out is None:
            out = torch.empty((n, h_up, w_up, 3), dtype=torch.uint8, device=dev)
        return self._timed("paste", K.face_paste, bg, restored.to(dev).contiguous(), masks.to(dev).contiguous(), inverse_affine.to(dev).contiguous(),
                           count.to(dev).contiguous(), out, f)

    def paste(self, background, restored, inverse_affine, count, upscale_factor: float = 1, bgr: bool = False, out=None, frame_size=None):
        """-> uint8 [n, h_up, w_up, 3] on the device (written into `out` when given), (h_up, w_up) = (int(h f), int(w f)).

        background: uint8 [n, H, W, 3] -- the frames themselves, or their upsampled version (facexlib's upsample_img); it is resized with
        INTER_LANCZOS4 when it is not h_up x w_up yet.  frame_size = (h, w) of the frames the faces were found in (default: the
        background's own size).  restored: uint8 [n * max_faces, 512, 512, 3], slot f * max_faces + r, in the caller's channel order;
        inverse_affine float64 [n, max_faces, 2, 3] and count int32 [n] as `FaceAligner.align` returns them (the aligner's upscale_factor
        must be this call's: its inverse matrices are already scaled by it).  The matrices are only read.  bgr: as in `FaceAligner.align`.
        Nothing is read back to the host; a second call on the same shapes allocates nothing but `out`."""
        import torch
        if not isinstance(restored, torch.Tensor) or restored.dtype != torch.uint8:
            raise TypeError(f"restored must be a uint8 tensor, got {getattr(restored, 'dtype', type(restored).__name__)}")
        return self.paste_masks(background, restored, self.masks(restored, bgr), inverse_affine, count, upscale_factor, out, frame_size)


class FaceEnhancer:
    """The reference's use_face_enhancer for a whole window on device tensors: `FaceAligner.align`, `FaceRestorer.restore_aligned` on all
    n * max_faces slots, `FacePaster.paste` -- no host read in between.  `restorer` needs `restore_aligned(faces) -> uint8 [m, 512, 512, 3]`."""

    def __init__(self, aligner, restorer, paster, bgr: bool = False):
        self.aligner, self.restorer, self.paster, self.bgr = aligner, restorer, paster, bool(bgr)

    def enhance_frames(self, frames, background=None, upscale=None, out=None, **restore_kwargs):
        """frames: what `FaceAligner.align` takes -> uint8 [n, h_up, w_up, 3] on the device.  background: the frames' upsampled version
        (e.g. `Upscaler.enhance_batch`'s output), default the frames.  upscale: the aligner's upscale_factor (the inverse matrices carry it);
        any other value raises."""
        f = self.aligner.upscale_factor if upscale is None else float(upscale)
        if f != self.aligner.upscale_factor:
            raise ValueError(f"upscale={upscale} but the aligner was built with upscale_factor={self.aligner.upscale_factor}: its inverse matrices carry that factor")
        src = self.aligner._frames(frames)
        al = self.aligner.align(src, bgr=self.bgr)
        restored = self.restorer.restore_aligned(al["faces"], **restore_kwargs)
        return self.paster.paste(src if background is None else background, restored, al["inverse_affine"], al["count"], f, self.bgr, out, tuple(src.shape[1:3]))

    def as_face_enhancer(self):
        """-> `(rgb_uint8, bg_upsampler=None) -> uint8 array`, the signature of `Upscaler`'s face_enhancer hook: the reference's configuration is
        `Upscaler(scale, face_enhancer=FaceEnhancer(aligner, restorer, paster).as_face_enhancer())` with the aligner built at
        upscale_factor = scale."""
        import torch

        def face_enhancer(rgb_uint8, bg_upsampler=None):
            frame = np.asarray(rgb_uint8)
            bg = None
            if bg_upsampler is not None:
                bg = torch.from_numpy(np.ascontiguousarray(bg_upsampler.enhance(frame, outscale=self.aligner.upscale_factor)[0]))[None]
            return self.enhance_frames([frame], background=bg)[0].cpu().numpy()

        return face_enhancer
