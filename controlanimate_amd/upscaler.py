"""Real-ESRGAN upscaling of the emitted frames (modules/upscaler.py; scripts/vid2vid.py:116-119,236-242) on the HIP path.

The reference builds `RRDBNet(num_in_ch=3, num_out_ch=3, num_feat=64, num_block=6, num_grow_ch=32, scale=4)` (basicsr, the
"anime-6B" model) and runs it through `RealESRGANer(scale=4, tile=0, pre_pad=0, half=True).enhance(np.asarray(pil_image),
outscale=scale)`.  That data flow is replicated here (realesrgan / basicsr / OpenCV are not installed, so it is restated from their
published sources and UNPINNED against them):

  * enhance() treats its input as BGR and converts BGR -> RGB; the reference hands it an RGB array, so the net sees the channels
    REVERSED and its output is reversed back (`output_img[[2, 1, 0]]`): ca_rgb8_to_nhwc / conv_last's out_u8 epilogue;
  * input / 255 in fp32, then fp16; the net in fp16; output clamp(0, 1) * 255 rounded half to even (numpy's .round()) to uint8;
  * outscale != 4: cv2.resize(..., (int(w * outscale), int(h * outscale)), interpolation=cv2.INTER_LANCZOS4) on the uint8 result
    -- OpenCV's integer path for 8-bit data, restated in `lanczos4_tables` (host, O(W + H)) + ca_resize_lanczos4_u8 (device).

Every convolution is ca_conv3x3_narrow (ABI v14): the dense blocks write x1 .. x4 into channel slices of one 192-channel concat
buffer (no torch.cat), LeakyReLU(0.2) and the residual scalings `x5 * 0.2 + x` / `rdb3 * 0.2 + x` are epilogue terms, the nearest
x2 upsamplings are folded into the gather of conv_up1 / conv_up2.  There is no CPU path.

GFPGAN face restoration (use_face_enhancer) is a detector + aligner + restoration network + paste-back of its own.  The network is
built for ALIGNED 512 x 512 faces in gfpgan.py (GFPGANv1Clean on the HIP kernels, no CPU fallback, UNPINNED against gfpgan and real
weights); face detection and the 5-point warp (face_align.py) and the parsing-mask paste-back (face_paste.py) are built, opt-in and
UNPINNED against facexlib.  The call that gives the reference's behaviour is `Upscaler(scale, face_enhancer=FaceEnhancer(aligner,
restorer, paster).as_face_enhancer())` with the aligner built at upscale_factor = scale, or `FaceRestorer(weights).as_face_enhancer(
face_helper)` with `FaceHelper(aligner, paster=paster)` or a caller-supplied helper that has facexlib.FaceRestoreHelper's methods; any
other `face_enhancer` callable works as before.  Nothing here changes: without a callable, use_face_enhancer=True still raises.
"""
from __future__ import annotations

import math
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import kernels as K
from .layers import WeightArena

try:
    from PIL import Image
except Exception:  # pragma: no cover
    Image = None

NETSCALE = 4
NUM_FEAT, NUM_GROW, NUM_BLOCK = 64, 32, 6


def _conv(cin: int, cout: int) -> nn.Conv2d:
    return nn.Conv2d(cin, cout, 3, 1, 1)  # parameter container with basicsr's names (weight, bias); never called


class ResidualDenseBlock(nn.Module):
    def __init__(self, nf: int = NUM_FEAT, gc: int = NUM_GROW):
        super().__init__()
        self.conv1, self.conv2, self.conv3 = _conv(nf, gc), _conv(nf + gc, gc), _conv(nf + 2 * gc, gc)
        self.conv4, self.conv5 = _conv(nf + 3 * gc, gc), _conv(nf + 4 * gc, nf)


class RRDB(nn.Module):
    def __init__(self, nf: int = NUM_FEAT, gc: int = NUM_GROW):
        super().__init__()
        self.rdb1, self.rdb2, self.rdb3 = ResidualDenseBlock(nf, gc), ResidualDenseBlock(nf, gc), ResidualDenseBlock(nf, gc)


class RRDBNet(nn.Module):
    """basicsr.archs.rrdbnet_arch.RRDBNet for scale = 4 (parameter names and forward), executed by the HIP kernels after
    `prepare(device, dtype)`.  Activations are NHWC."""

    def __init__(self, num_in_ch: int = 3, num_out_ch: int = 3, num_feat: int = NUM_FEAT, num_block: int = NUM_BLOCK,
                 num_grow_ch: int = NUM_GROW, scale: int = NETSCALE):
        super().__init__()
        if (num_in_ch, num_out_ch, num_feat, num_grow_ch, scale) != (3, 3, NUM_FEAT, NUM_GROW, NETSCALE):
            raise NotImplementedError("only the anime-6B shape family (3 -> 3 channels, num_feat 64, num_grow_ch 32, scale 4) is built")
        self.conv_first = _conv(3, num_feat)
        self.body = nn.Sequential(*[RRDB(num_feat, num_grow_ch) for _ in range(num_block)])
        self.conv_body = _conv(num_feat, num_feat)
        self.conv_up1, self.conv_up2 = _conv(num_feat, num_feat), _conv(num_feat, num_feat)
        self.conv_hr, self.conv_last = _conv(num_feat, num_feat), _conv(num_feat, 3)
        self._packed = None
        self.dtype = None

    def load_state_dict(self, state_dict, strict: bool = True):  # noqa: D401 -- strict check names both lists
        own = set(self.state_dict().keys())
        got = set(state_dict.keys())
        missing, unexpected = sorted(own - got), sorted(got - own)
        if strict and (missing or unexpected):
            raise KeyError(f"RRDBNet state dict does not match: missing keys {missing}, unexpected keys {unexpected}")
        self._packed = None
        return super().load_state_dict(state_dict, strict=strict)

    def _convs(self):
        yield "conv_first", self.conv_first
        for i, blk in enumerate(self.body):
            for r in ("rdb1", "rdb2", "rdb3"):
                for c in range(1, 6):
                    yield f"body.{i}.{r}.conv{c}", getattr(getattr(blk, r), f"conv{c}")
        for n in ("conv_body", "conv_up1", "conv_up2", "conv_hr", "conv_last"):
            yield n, getattr(self, n)

    @staticmethod
    def pack_weight(weight: torch.Tensor, cin_in: int) -> torch.Tensor:
        """[cout, cin, 3, 3] -> [round_up(cout, 16), 3, 3, round_up(max(cin, cin_in), 32)] zero padded (ca_conv3x3_narrow_args.w)."""
        cout, cin = weight.shape[:2]
        cin_p = (max(cin, cin_in) + 31) // 32 * 32
        out = torch.zeros(((cout + 15) // 16 * 16, 3, 3, cin_p), dtype=torch.float32)
        out[:cout, :, :, :cin] = weight.detach().float().permute(0, 2, 3, 1)
        return out

    def prepare(self, device, dtype: torch.dtype = torch.float16) -> "RRDBNet":
        """Packs every weight once into one device WeightArena (as vae.py does)."""
        arena = WeightArena()
        packed = {}
        for name, conv in self._convs():
            cin_in = 8 if name == "conv_first" else conv.in_channels
            w = self.pack_weight(conv.weight, cin_in)
            pw = arena.add(w.shape, dtype, lambda w=w: w)
            pb = arena.add((conv.out_channels,), torch.float32, lambda b=conv.bias: b.detach().float())
            packed[name] = (pw, pb, cin_in, conv.out_channels)
        arena.finalize(torch.device(device))
        self._packed = {n: (pw.t, pb.t, cin, cout) for n, (pw, pb, cin, cout) in packed.items()}
        self._arena, self.dtype = arena, dtype
        return self

    def _run(self, name, x, y, **kw):
        w, b, cin, cout = self._packed[name]
        return K.conv3x3_narrow(x, w, y, cin=cin, cout=cout, bias=b, **kw)

    def forward_nhwc(self, x8: torch.Tensor, float_out: bool = False) -> torch.Tensor:
        """x8: [n, H, W, 8] (ca_rgb8_to_nhwc).  Returns uint8 [n, 4H, 4W, 3] in the caller's channel order (conv_last's output
        reversed back), or -- float_out -- conv_last's raw output [n, 4H, 4W, 16] in the net's own channel order (channels 0..2)."""
        if self._packed is None:
            raise RuntimeError("RRDBNet.prepare(device, dtype) first")
        n, h, w, _ = x8.shape
        dev, dt = x8.device, self.dtype
        nf, gc = NUM_FEAT, NUM_GROW
        feat = torch.empty((n, h, w, nf), device=dev, dtype=dt)
        self._run("conv_first", x8, feat)
        cat = [torch.empty((n, h, w, nf + 4 * gc), device=dev, dtype=dt) for _ in range(3)]
        self._run("conv_first", x8, cat[0])  # the body's input also lives in the first 64 channels of a concat buffer

        def rdb(prefix, a, b, rrdb_in=None):
            for c in range(1, 5):
                self._run(f"{prefix}.conv{c}", a, a, channel_offset=nf + (c - 1) * gc, leaky_relu=True)
            if rrdb_in is None:  # x5 * 0.2 + x
                self._run(f"{prefix}.conv5", a, b, s0=0.2, r1=a, s1=1.0)
            else:  # (x5 * 0.2 + x) * 0.2 + x_rrdb, written over x_rrdb in place (same lane reads, then writes)
                self._run(f"{prefix}.conv5", a, b, s0=0.04, r1=a, s1=0.2, r2=rrdb_in, s2=1.0)

        p = 0
        for i in range(len(self.body)):
            q, r = (p + 1) % 3, (p + 2) % 3
            rdb(f"body.{i}.rdb1", cat[p], cat[q])
            rdb(f"body.{i}.rdb2", cat[q], cat[r])
            rdb(f"body.{i}.rdb3", cat[r], cat[p], rrdb_in=cat[p])
        body = cat[p]
        feat2 = torch.empty((n, h, w, nf), device=dev, dtype=dt)
        self._run("conv_body", body, feat2, r1=feat, s1=1.0)  # feat + conv_body(body(feat))
        del body, cat, feat
        up1 = torch.empty((n, 2 * h, 2 * w, nf), device=dev, dtype=dt)
        self._run("conv_up1", feat2, up1, upsample=True, leaky_relu=True)
        del feat2
        up2 = torch.empty((n, 4 * h, 4 * w, nf), device=dev, dtype=dt)
        self._run("conv_up2", up1, up2, upsample=True, leaky_relu=True)
        del up1
        hr = torch.empty((n, 4 * h, 4 * w, nf), device=dev, dtype=dt)
        self._run("conv_hr", up2, hr, leaky_relu=True)
        del up2
        if float_out:
            wl, bl, cin, _ = self._packed["conv_last"]
            out = torch.empty((n, 4 * h, 4 * w, 16), device=dev, dtype=dt)
            bias16 = torch.zeros(16, device=dev, dtype=torch.float32)
            bias16[:3] = bl
            return K.conv3x3_narrow(hr, wl, out, cin=cin, cout=16, bias=bias16)
        out = torch.empty((n, 4 * h, 4 * w, 3), device=dev, dtype=torch.uint8)
        return self._run("conv_last", hr, out, out_u8=True)


# ---- OpenCV INTER_LANCZOS4, 8-bit data -----------------------------------------------------------------------------------------

_S45 = 0.70710678118654752440084436210485
_CS = ((1.0, 0.0), (-_S45, -_S45), (0.0, 1.0), (_S45, -_S45), (-1.0, 0.0), (_S45, _S45), (0.0, -1.0), (-_S45, _S45))


def _lanczos4_coeffs(x: np.float32) -> List[np.float32]:
    """OpenCV's interpolateLanczos4(x, coeffs): float / double arithmetic as in its C++ (float inputs, double trig)."""
    f32 = np.float32
    y0 = float(-(x + f32(3))) * math.pi * 0.25
    s0, c0 = math.sin(y0), math.cos(y0)
    coeffs, total = [], f32(0)
    for i in range(8):
        y0_ = f32(x + f32(3)) - f32(i)
        if abs(y0_) >= f32(1e-6):
            y = float(-y0_) * math.pi * 0.25
            c = f32((_CS[i][0] * s0 + _CS[i][1] * c0) / (y * y))
        else:
            c = f32(1e30)
        coeffs.append(c)
        total = f32(total + c)
    inv = f32(f32(1) / total)
    return [f32(c * inv) for c in coeffs]


def lanczos4_tables(src: int, dst: int):
    """Per destination index d of one axis of cv2.resize(src -> dst, INTER_LANCZOS4) on uint8: (ofs int32 [dst] = floor(f) - 3,
    coef int16 [dst, 8] = saturate_cast<short>(lanczos4(f - floor(f))[k] * 2048)) with f = float((d + 0.5) * src / dst - 0.5)."""
    scale = 1.0 / (float(dst) / float(src))
    ofs = np.empty(dst, dtype=np.int32)
    coef = np.empty((dst, 8), dtype=np.int16)
    for d in range(dst):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(math.floor(f))
        f = np.float32(f - np.float32(s))
        ofs[d] = s - 3
        for k, c in enumerate(_lanczos4_coeffs(f)):
            coef[d, k] = int(np.clip(np.rint(np.float32(c * np.float32(2048))), -32768, 32767))
    return ofs, coef


def output_size(w: int, h: int, outscale: float):
    """(width, height) of RealESRGANer.enhance's result: (int(w * outscale), int(h * outscale)) (also the ffmpeg writer size of
    scripts/vid2vid.py:118-119)."""
    return int(w * outscale), int(h * outscale)


class Upscaler:
    """modules/upscaler.py:17-74 on the HIP path: `Upscaler(scale)(pil_image) -> PIL.Image`.

    The net's weights come from `state_dict`, or a local `.pth` (`model_path`, default the reference's
    weights/RealESRGAN_x4plus_anime_6B.pth; local_models.load_realesrgan_state_dict).  They are packed on the first call.
    `face_enhancer(rgb_uint8_array, bg_upsampler=self) -> uint8 array` stands in for GFPGANer.enhance(...)[2]; `self.enhance` is
    then the background upsampler it may call, as RealESRGANer is for GFPGAN.  `upscale_first` is forced to False, as the reference
    does (upscaler.py:23).  `max_frames_per_launch` bounds how many frames one pass of the net takes (each frame's 4x activations
    are 2 x 805 MB at 512 x 768); the kernels address with 64-bit pointers, so any count within their 2^31-pixel limit works."""

    def __init__(self, scale, use_face_enhancer: bool = True, upscale_first: bool = False, *, model_path: Optional[str] = None,
                 state_dict: Optional[dict] = None, device=None, face_enhancer: Optional[Callable] = None,
                 dtype: torch.dtype = torch.float16, max_frames_per_launch: int = 8):
        self.scale = scale
        self.use_face_enhancer = use_face_enhancer
        self.upscale_first = False  # the reference ignores its argument (upscaler.py:23)
        if use_face_enhancer and face_enhancer is None:
            raise NotImplementedError("use_face_enhancer=True: GFPGAN face restoration is not built in this project; pass a "
                                      "face_enhancer callable or use_face_enhancer=False")  # (gfpgan.FaceRestorer.as_face_enhancer(helper) is such a callable)
        self.face_enhancer = face_enhancer
        self.model = RRDBNet(num_in_ch=3, num_out_ch=3, num_feat=64, num_block=6, num_grow_ch=32, scale=NETSCALE)
        if state_dict is None:
            from .local_models import REALESRGAN_ANIME_6B_PATH, load_realesrgan_state_dict
            state_dict = load_realesrgan_state_dict(model_path or REALESRGAN_ANIME_6B_PATH)
        self.model.load_state_dict(state_dict)
        self.device = device
        self.dtype = dtype
        self.max_frames_per_launch = max(1, int(max_frames_per_launch))
        self._tables = {}

    def _net(self) -> RRDBNet:
        if self.model._packed is None:
            dev = torch.device(self.device) if self.device is not None else torch.device("cuda", torch.cuda.current_device())
            if dev.type != "cuda":
                raise RuntimeError("the upscaler runs on the HIP kernels only (no CPU path)")
            self.model.prepare(dev, self.dtype)
            self.device = dev
        return self.model

    def _resize_tables(self, src: int, dst: int):
        key = (src, dst)
        if key not in self._tables:
            ofs, coef = lanczos4_tables(src, dst)
            self._tables[key] = (torch.from_numpy(ofs).to(self.device), torch.from_numpy(coef).to(self.device))
        return self._tables[key]

    def enhance_batch(self, frames: torch.Tensor, outscale: Optional[float] = None) -> torch.Tensor:
        """uint8 [n, h, w, 3] (any device) -> uint8 [n, H', W', 3] on the device: RealESRGANer.enhance per frame, in passes of at most
        `max_frames_per_launch` frames."""
        net = self._net()
        frames = frames.to(self.device).contiguous()
        n, h, w, _ = frames.shape
        outs = []
        step = self.max_frames_per_launch
        chunks = -(-n // step)
        per = -(-n // chunks)  # even split
        for s in range(0, n, per):
            outs.append(net.forward_nhwc(K.rgb8_to_nhwc(frames[s:s + per].contiguous(), self.dtype)))
        out = outs[0] if len(outs) == 1 else torch.cat(outs)
        if outscale is not None and float(outscale) != float(NETSCALE):
            dw, dh = output_size(w, h, outscale)
            xofs, alpha = self._resize_tables(NETSCALE * w, dw)
            yofs, beta = self._resize_tables(NETSCALE * h, dh)
            out = K.resize_lanczos4_u8(out, dh, dw, xofs, alpha, yofs, beta)
        return out

    def enhance(self, img: np.ndarray, outscale: Optional[float] = None):
        """RealESRGANer.enhance(img, outscale) for a uint8 H x W x 3 array -> (uint8 array, None)."""
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"the upscaler takes uint8 H x W x 3 frames, got {img.dtype} {img.shape}")
        out = self.enhance_batch(torch.from_numpy(np.array(img, copy=True))[None], outscale)
        return out[0].cpu().numpy(), None

    def __call__(self, pil_image):
        assert self.scale > 1 and self.scale < 8, 'Error: Invalid scale value.'
        if self.use_face_enhancer:
            output = np.asarray(pil_image)  # upscale_first is always False (see __init__)
            output = np.asarray(self.face_enhancer(output, bg_upsampler=self))
        else:
            output, _ = self.enhance(np.asarray(pil_image), outscale=self.scale)
        return Image.fromarray(output) if Image is not None else output

    def upscale_frames(self, frames: Sequence) -> List:
        """`[self(f) for f in frames]`, byte for byte, with the frames of one size going through the net together."""
        assert self.scale > 1 and self.scale < 8, 'Error: Invalid scale value.'
        frames = list(frames)
        if self.use_face_enhancer or not frames:
            return [self(f) for f in frames]
        arrs = [np.asarray(f) for f in frames]
        out: List = [None] * len(arrs)
        by_shape = {}
        for i, a in enumerate(arrs):
            by_shape.setdefault(a.shape, []).append(i)
        for shape, idx in by_shape.items():
            if len(shape) != 3 or shape[2] != 3:
                raise ValueError(f"the upscaler takes uint8 H x W x 3 frames, got {shape}")
            batch = torch.from_numpy(np.stack([arrs[i] for i in idx]))
            res = self.enhance_batch(batch, self.scale).cpu().numpy()
            for j, i in enumerate(idx):
                out[i] = Image.fromarray(res[j]) if Image is not None else res[j]
        return out


def upscaler_from_config(config, model_path: Optional[str] = None, device=None, face_enhancer: Optional[Callable] = None,
                         **kw) -> Optional[Upscaler]:
    """scripts/vid2vid.py:58-59,236-237: `upscale > 1` builds an Upscaler from `use_face_enhancer` and `upscale_first`; upscale <= 1
    builds nothing (None)."""
    from .controlanimate_pipeline import _get
    upscale = float(_get(config, "upscale", 1) or 1)
    assert upscale >= 1, "Upscale factor should be greater than or equal to one."
    if upscale <= 1:
        return None
    return Upscaler(upscale, use_face_enhancer=bool(_get(config, "use_face_enhancer", 0)),
                    upscale_first=bool(_get(config, "upscale_first", 0)), model_path=model_path, device=device,
                    face_enhancer=face_enhancer, **kw)
