"""GFPGAN face restoration (modules/upscaler.py:53-70: with `use_face_enhancer` every emitted frame passes through
`GFPGANer(arch='clean', channel_multiplier=2).enhance(...)`) on the HIP path, for ALIGNED 512 x 512 faces.

The network is `GFPGANv1Clean(out_size=512, num_style_feat=512, channel_multiplier=2, narrow=1, different_w=True, input_is_latent=True,
sft_half=True)`: a U-Net whose features modulate (SFT) a StyleGAN2 decoder -- 84.3 M parameters on this path, about 0.35 TFLOP per
face, two thirds of it modulated convolution.  It runs as (the names are the keys of `FaceRestorer.timings`):

    prep      ca_gfp_prep: uint8 faces -> LeakyReLU(conv_body_first((x / 255 - 0.5) / 0.5)), the channel reversal a flag
    encoder   per ResBlock: ca_conv3x3 (CA_ACT_LEAKY02), ca_resample2x (the bilinear x1/2 = 2x2 mean, or x2), ca_conv3x3, ca_resample2x
              of the input, ca_gemm (the 1x1 skip, the main path as its residual operand); final_conv; final_linear as ca_gemm over the
              NHWC flattening (its columns permuted at pack time), fp32 latents; the up blocks start with ca_add_bcast (feat + skip)
    sft       the condition_scale / condition_shift branches: two ca_conv3x3 each
    styles    ca_gfp_styles: ONE launch for the 2 L - 1 StyleConv (s / max|s| and demod') and the L ToRGB (s) of every image
    modconv   kernels.modconv3x3, one per StyleConv: demod[n, o] * conv(W, s[n, i] * x) keeps one weight for the batch.  At 512 x 512
              output pixels ca_modconv3x3, one launch: the upsampling layer computes the bilinear x2 from the low-resolution halo in LDS;
              noise, bias, LeakyReLU and SFT in the epilogue.  On the smaller planes, where ca_conv3x3's tiles are faster (measured per
              level), the same arithmetic as three launches: ca_gfp_modulate, ca_conv3x3 without split-K, ca_gfp_style_epilogue
    to_rgb    ca_gfp_to_rgb: the 1x1 modulated convolution to 3 channels + bias + the bilinear x2 of the previous fp32 image
    finish    ca_gfp_finish: clamp(-1, 1), (x + 1) / 2 * 255, half-to-even rounding, channel reversal -> uint8

No device-to-host read and no atomics anywhere: with explicit noises the chain can be captured in a hipGraph, and two runs give the
same bits.  There is no CPU fallback: without the library or a GPU a call raises CAHipUnavailable.

Scope.  `restore_aligned` is `GFPGANer.enhance(..., has_aligned=True)` for faces that already are 512 x 512 (enhance would cv2.resize
any other size, which is not restated: NotImplementedError).  Face detection (RetinaFace), the 5-point warp and the parsing-mask
paste-back are facexlib.FaceRestoreHelper's and live beside this module (face_align.py and face_paste.py: built, opt-in, UNPINNED):
`enhance(has_aligned=False)` and `as_face_enhancer` drive an object with that class's methods, `face_align.FaceHelper(aligner,
paster=face_paste.FacePaster(...))` or the caller's own; `face_paste.FaceEnhancer` runs the three stages for a whole window.

The specification is tests/gfpgan_ref.py.  gfpgan, basicsr, facexlib and OpenCV are third-party packages that are absent here and
no GFPGANv1.3.pth is available: key names and parity with them are UNPINNED, and the real-weight path of `as_face_enhancer` is
unmeasured.
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Sequence

import numpy as np
import torch

from .layers import Packed, WeightArena

OUT_SIZE = 512
STYLE_FEAT = 512
IGNORED_PREFIXES = ("toRGB.", "stylegan_decoder.style_mlp.", "stylegan_decoder.noises.")  # unused on this path: accepted and dropped
STAGES = ("prep", "encoder", "sft", "styles", "modconv", "to_rgb", "finish")


def unet_channels(size: int) -> int:
    """Width of the U-Net and of the SFT maps at plane `size` (channel_multiplier 2, narrow 1)."""
    return {128: 128, 256: 64, 512: 32}.get(size, 256)


def stylegan_channels(size: int) -> int:
    return {128: 256, 256: 128, 512: 64}.get(size, 512)


def _log_size(out_size: int) -> int:
    log = int(math.log2(out_size))
    if 2 ** log != out_size or not 8 <= out_size <= 512:
        raise NotImplementedError(f"out_size must be a power of two in 8 .. 512, got {out_size}")
    return log


def gfpgan_key_shapes(out_size: int = OUT_SIZE) -> Dict[str, tuple]:
    """name -> shape of every tensor this path reads (84,339,239 parameters at out_size 512)."""
    log = _log_size(out_size)
    out: Dict[str, tuple] = {}

    def conv(name, cin, cout, k, bias=True):
        out[name + ".weight"] = (cout, cin, k, k)
        if bias:
            out[name + ".bias"] = (cout,)

    def resblock(name, cin, cout):
        conv(name + ".conv1", cin, cin, 3)
        conv(name + ".conv2", cin, cout, 3)
        conv(name + ".skip", cin, cout, 1, bias=False)

    def modconv(name, cin, cout, k):
        out[name + ".modulated_conv.weight"] = (1, cout, cin, k, k)
        out[name + ".modulated_conv.modulation.weight"] = (cin, STYLE_FEAT)
        out[name + ".modulated_conv.modulation.bias"] = (cin,)

    def styleconv(name, cin, cout):
        modconv(name, cin, cout, 3)
        out[name + ".weight"] = (1,)
        out[name + ".bias"] = (1, cout, 1, 1)

    def torgb(name, cin):
        modconv(name, cin, 3, 1)
        out[name + ".bias"] = (1, 3, 1, 1)

    c = unet_channels(out_size)
    conv("conv_body_first", 3, c, 1)
    for j, i in enumerate(range(log, 2, -1)):
        resblock(f"conv_body_down.{j}", c, unet_channels(2 ** (i - 1)))
        c = unet_channels(2 ** (i - 1))
    conv("final_conv", c, unet_channels(4), 3)
    c = unet_channels(4)
    for j, i in enumerate(range(3, log + 1)):
        cu = unet_channels(2 ** i)
        resblock(f"conv_body_up.{j}", c, cu)
        c = cu
        for branch in ("condition_scale", "condition_shift"):
            conv(f"{branch}.{j}.0", cu, cu, 3)
            conv(f"{branch}.{j}.2", cu, cu, 3)
    out["final_linear.weight"] = ((2 * log - 2) * STYLE_FEAT, unet_channels(4) * 16)
    out["final_linear.bias"] = ((2 * log - 2) * STYLE_FEAT,)
    d = "stylegan_decoder."
    out[d + "constant_input.weight"] = (1, stylegan_channels(4), 4, 4)
    styleconv(d + "style_conv1", stylegan_channels(4), stylegan_channels(4))
    torgb(d + "to_rgb1", stylegan_channels(4))
    c = stylegan_channels(4)
    for j, i in enumerate(range(3, log + 1)):
        cs = stylegan_channels(2 ** i)
        styleconv(f"{d}style_convs.{2 * j}", c, cs)
        styleconv(f"{d}style_convs.{2 * j + 1}", cs, cs)
        torgb(f"{d}to_rgbs.{j}", cs)
        c = cs
    return out


def permute_final_linear(weight: torch.Tensor, channels: int = 256) -> torch.Tensor:
    """final_linear.weight [N, channels * 16], whose columns follow the NCHW flattening c * 16 + y * 4 + x of the [channels, 4, 4] map, ->
    the same weight for the NHWC flattening (y * 4 + x) * channels + c."""
    n = weight.shape[0]
    if tuple(weight.shape) != (n, channels * 16):
        raise ValueError(f"final_linear.weight [N, {channels * 16}] is expected, got {tuple(weight.shape)}")
    return weight.detach().reshape(n, channels, 16).permute(0, 2, 1).reshape(n, channels * 16).contiguous()


class GFPGANv1Clean:
    """The parameter container of the network under the published names (gfpgan.archs.gfpganv1_clean_arch.GFPGANv1Clean with
    basicsr's StyleGAN2GeneratorCSFT as `stylegan_decoder`), executed by the HIP kernels after `prepare(device, dtype)`."""

    def __init__(self, out_size: int = OUT_SIZE, num_style_feat: int = STYLE_FEAT, channel_multiplier: int = 2, narrow: float = 1, different_w: bool = True,
                 input_is_latent: bool = True, sft_half: bool = True):
        if (num_style_feat, channel_multiplier, narrow, different_w, input_is_latent, sft_half) != (STYLE_FEAT, 2, 1, True, True, True):
            raise NotImplementedError("only the reference's configuration is built: num_style_feat 512, channel_multiplier 2, narrow 1, different_w, "
                                      "input_is_latent, sft_half")
        self.out_size = out_size
        self.log_size = _log_size(out_size)
        self.num_latent = 2 * self.log_size - 2
        self.num_layers = 2 * (self.log_size - 2) + 1   # StyleConv layers = noise maps
        self.shapes = gfpgan_key_shapes(out_size)
        self.params: Dict[str, torch.Tensor] = {}
        self.packed = None
        self.dtype = None

    def noise_shapes(self, n: int) -> List[tuple]:
        return [(n, 2 ** ((i + 5) // 2), 2 ** ((i + 5) // 2)) for i in range(self.num_layers)]

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return dict(self.params)

    def load_state_dict(self, state_dict, strict: bool = True):
        """Strict: KeyError naming the missing and the unexpected keys, ValueError naming a tensor of the wrong shape.  `toRGB.*`,
        `stylegan_decoder.style_mlp.*` and `stylegan_decoder.noises.*` are accepted and dropped (unused on this path)."""
        got = {k: v for k, v in state_dict.items() if not k.startswith(IGNORED_PREFIXES)}
        missing = sorted(k for k in self.shapes if k not in got)
        unexpected = sorted(k for k in got if k not in self.shapes)
        if missing or (strict and unexpected):
            raise KeyError(f"GFPGANv1Clean state dict does not match: missing keys {missing}, unexpected keys {unexpected}")
        for k, shape in self.shapes.items():
            if tuple(got[k].shape) != shape:
                raise ValueError(f"GFPGANv1Clean state dict: '{k}' has shape {tuple(got[k].shape)}, expected {shape}")
        self.params = {k: got[k].detach().float().cpu().contiguous() for k in self.shapes}
        self.packed = None
        return self

    # ---- packing ---------------------------------------------------------------------------------------------------------------
    def prepare(self, device, dtype: torch.dtype = torch.float16) -> "GFPGANv1Clean":
        """Packs every weight once into one device WeightArena (as upscaler.RRDBNet does)."""
        if dtype not in (torch.float16, torch.bfloat16):
            raise TypeError(f"dtype must be torch.float16 or torch.bfloat16, got {dtype}")
        if not self.params:
            raise RuntimeError("GFPGANv1Clean.load_state_dict(...) first")
        sd, arena = self.params, WeightArena()
        f32 = torch.float32

        def add(t, dt):
            t = t.contiguous()
            return arena.add(tuple(t.shape), dt, lambda t=t: t)

        def conv3(name):
            return {"w": add(sd[name + ".weight"].permute(0, 2, 3, 1), dtype), "b": add(sd[name + ".bias"], f32)}

        def resblock(name):
            w = sd[name + ".skip.weight"]
            return {"c1": conv3(name + ".conv1"), "c2": conv3(name + ".conv2"), "skip": add(w.reshape(w.shape[0], w.shape[1]), dtype)}

        levels = self.log_size - 2
        P = {"first_w": add(sd["conv_body_first.weight"].reshape(-1, 3), f32), "first_b": add(sd["conv_body_first.bias"], f32),
             "down": [resblock(f"conv_body_down.{j}") for j in range(levels)], "final": conv3("final_conv"),
             "lin_w": add(permute_final_linear(sd["final_linear.weight"], unet_channels(4)), dtype), "lin_b": add(sd["final_linear.bias"], f32),
             "up": [resblock(f"conv_body_up.{j}") for j in range(levels)],
             "cond": [[(conv3(f"{b}.{j}.0"), conv3(f"{b}.{j}.2")) for b in ("condition_scale", "condition_shift")] for j in range(levels)]}
        d = "stylegan_decoder."
        P["const"] = add(sd[d + "constant_input.weight"].permute(0, 2, 3, 1), dtype)
        # the modulated layers in the order the decoder runs them; latent i feeds layer i
        names = [(d + "style_conv1", True), (d + "to_rgb1", False)]
        for j in range(levels):
            names += [(f"{d}style_convs.{2 * j}", True), (f"{d}style_convs.{2 * j + 1}", True), (f"{d}to_rgbs.{j}", False)]
        latent_of, idx = [0, 1], 1
        for j in range(levels):
            latent_of += [idx, idx + 1, idx + 2]
            idx += 2
        chunks, desc, layers, p_off, o_off = [], [], [], 0, 0
        for (name, is_conv), li in zip(names, latent_of):
            w = sd[name + ".modulated_conv.weight"][0]                       # [cout, cin, k, k]
            cout, cin = (w.shape[0], w.shape[1]) if is_conv else (0, w.shape[1])
            mod = torch.cat([sd[name + ".modulated_conv.modulation.weight"].t().reshape(-1), sd[name + ".modulated_conv.modulation.bias"].reshape(-1)])
            chunks.append(mod)
            w_off, p_off = p_off, p_off + mod.numel()
            wsq_off = 0
            if is_conv:
                wsq = w.to(dtype).float().pow(2).sum([2, 3]).t().reshape(-1)     # of the weight as the MFMA reads it: [cin, cout]
                chunks.append(wsq)
                wsq_off, p_off = p_off, p_off + wsq.numel()
                layer = {"w": add(w.permute(0, 2, 3, 1), dtype), "b": add(sd[name + ".bias"].reshape(-1), f32), "nw": float(sd[name + ".weight"].reshape(-1)[0])}
            else:
                layer = {"w": add(w.reshape(3, cin), f32), "b": add(sd[name + ".bias"].reshape(-1), f32)}
            layer.update(cin=cin, cout=cout, off=o_off)
            layers.append(layer)
            desc += [li, cin, cout, w_off, wsq_off, o_off]
            o_off += cin + cout
        P["style_params"] = add(torch.cat(chunks), f32)
        arena.finalize(torch.device(device))

        def resolve(v):
            if isinstance(v, dict):
                return {k: resolve(x) for k, x in v.items()}
            if isinstance(v, (list, tuple)):
                return type(v)(resolve(x) for x in v)
            return v.t if isinstance(v, Packed) else v

        P = resolve(P)
        P["layers"], P["desc"], P["style_stride"] = resolve(layers), desc, o_off
        self.packed, self._arena, self.dtype = P, arena, dtype
        return self

    # ---- the chain ---------------------------------------------------------------------------------------------------------------
    def forward(self, faces: torch.Tensor, noises: Sequence[torch.Tensor], reverse_channels: bool = True, timed=None) -> torch.Tensor:
        """faces: uint8 [n, S, S, 3] on the device; noises: num_layers float32 [n, h, w] -> the image before the clamp, float32 [n, S, S, 3]
        in the net's own channel order."""
        from . import kernels as K
        if self.packed is None:
            raise RuntimeError("GFPGANv1Clean.prepare(device, dtype) first")
        P, dt, dev = self.packed, self.dtype, faces.device
        n, S = faces.shape[0], self.out_size
        run = timed if timed is not None else (lambda name, fn, *a, **kw: fn(*a, **kw))

        def conv(x, c, act=K.ACT_LEAKY02):
            return K.conv3x3(x, c["w"], bias=c["b"], act=act)

        def resblock(x, blk, up):
            t = K.resample2x(conv(x, blk["c1"]), up)
            main = conv(t, blk["c2"])
            xr = K.resample2x(x, up)
            m, h, w, cout = main.shape
            return K.gemm(xr.view(m * h * w, xr.shape[3]), blk["skip"], residual=main.view(m * h * w, cout)).view(m, h, w, cout)

        feat = run("prep", K.gfp_prep, faces, P["first_w"], P["first_b"], torch.empty((n, S, S, P["first_w"].shape[0]), dtype=dt, device=dev), reverse_channels)
        skips = []
        for blk in P["down"]:
            feat = run("encoder", resblock, feat, blk, False)
            skips.insert(0, feat)
        # final_conv writes the first n rows of final_linear's A operand, whose row count is padded to a multiple of 16
        rows = (n + 15) // 16 * 16
        c4 = P["final"]["w"].shape[0]
        flat = torch.zeros((rows, 16 * c4), dtype=dt, device=dev)
        feat = run("encoder", K.conv3x3, feat, P["final"]["w"], bias=P["final"]["b"], act=K.ACT_LEAKY02, out=flat[:n].view(n, 4, 4, c4))
        latents = run("encoder", K.gemm, flat, P["lin_w"], bias=P["lin_b"], out_f32=True)[:n].view(n, self.num_latent, STYLE_FEAT)
        conds = []
        for j, blk in enumerate(P["up"]):
            feat = run("encoder", resblock, run("encoder", K.add_bcast, feat, skips[j]), blk, True)
            for a, b in P["cond"][j]:
                conds.append(run("sft", lambda a=a, b=b, feat=feat: conv(conv(feat, a), b, K.ACT_NONE)))
        styles = run("styles", K.gfp_styles, latents, P["style_params"], P["desc"], torch.empty((n, P["style_stride"]), dtype=torch.float32, device=dev))

        def sd_of(layer):
            o, cin, cout = layer["off"], layer["cin"], layer["cout"]
            return styles[:, o:o + cin], styles[:, o + cin:o + cin + cout]

        L = P["layers"]
        s, dm = sd_of(L[0])
        out = run("modconv", K.modconv3x3, P["const"], L[0]["w"], s, dm, noises[0], L[0]["b"], L[0]["nw"], images=n)
        img = run("to_rgb", K.gfp_to_rgb, out, L[1]["w"], sd_of(L[1])[0], L[1]["b"], torch.empty((n, 4, 4, 3), dtype=torch.float32, device=dev))
        for j in range(self.log_size - 2):
            c1, c2, rgb = L[2 + 3 * j], L[3 + 3 * j], L[4 + 3 * j]
            s, dm = sd_of(c1)
            out = run("modconv", K.modconv3x3, out, c1["w"], s, dm, noises[1 + 2 * j], c1["b"], c1["nw"], upsample=True, sft=(conds[2 * j], conds[2 * j + 1]))
            s, dm = sd_of(c2)
            out = run("modconv", K.modconv3x3, out, c2["w"], s, dm, noises[2 + 2 * j], c2["b"], c2["nw"])
            side = out.shape[1]
            img = run("to_rgb", K.gfp_to_rgb, out, rgb["w"], sd_of(rgb)[0], rgb["b"], torch.empty((n, side, side, 3), dtype=torch.float32, device=dev), prev=img)
        return img


def _as_u8_faces(faces, size: int) -> torch.Tensor:
    """PIL images / uint8 arrays / a uint8 tensor -> uint8 tensor [n, size, size, 3]; TypeError, ValueError or NotImplementedError before
    any device work."""
    if isinstance(faces, torch.Tensor):
        t = faces
        if t.dtype != torch.uint8:
            raise TypeError(f"faces must be uint8, got {t.dtype}")
        if t.dim() != 4 or t.shape[3] != 3 or t.shape[0] < 1:
            raise ValueError(f"a face tensor is uint8 [n, {size}, {size}, 3], got {tuple(t.shape)}")
    else:
        if isinstance(faces, np.ndarray) and faces.ndim == 4:
            faces = list(faces)
        if not isinstance(faces, (list, tuple)):
            raise TypeError(f"faces: a list of PIL images or uint8 arrays, or a uint8 tensor [n, {size}, {size}, 3]; got {type(faces).__name__}")
        if not faces:
            raise ValueError("faces is empty")
        arrs = []
        for f in faces:
            if isinstance(f, torch.Tensor):
                f = f.cpu().numpy()
            a = np.asarray(f)
            if a.dtype != np.uint8:
                raise TypeError(f"faces must be uint8, got {a.dtype}")
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"a face is H x W x 3, got {a.shape}")
            arrs.append(a)
        if len({a.shape for a in arrs}) != 1:
            raise ValueError(f"faces of different sizes: {sorted({a.shape for a in arrs})}")
        t = torch.from_numpy(np.ascontiguousarray(np.stack(arrs)))
    if t.shape[1] != size or t.shape[2] != size:
        raise NotImplementedError(f"aligned faces are {size} x {size}; got {t.shape[1]} x {t.shape[2]} (GFPGANer.enhance would cv2.resize, which is not restated)")
    return t


class FaceRestorer:
    """`FaceRestorer(weights).restore_aligned(faces)`: GFPGANer(arch='clean', channel_multiplier=2) for aligned faces on the HIP kernels.
    `state_dict_or_path`: a state dict, or a local GFPGANv1.3.pth (local_models.load_gfpgan_state_dict; nothing is downloaded).
    `reverse_channels`: GFPGANer.enhance takes BGR and the reference hands it RGB, so the net sees the channels reversed and its output is
    reversed back; False feeds the net the caller's order.  `max_faces_per_launch` bounds one pass of the net (a face's largest activation
    is 33.5 MB; an operand stays below 2^31 bytes, so at most 63)."""

    def __init__(self, state_dict_or_path, device=None, dtype: torch.dtype = torch.float16, reverse_channels: bool = True, max_faces_per_launch: int = 16,
                 out_size: int = OUT_SIZE):
        if dtype not in (torch.float16, torch.bfloat16):
            raise TypeError(f"dtype must be torch.float16 or torch.bfloat16, got {dtype}")
        if not 1 <= int(max_faces_per_launch) <= 63:
            raise ValueError(f"max_faces_per_launch must be in 1 .. 63, got {max_faces_per_launch}")
        if isinstance(state_dict_or_path, (str, os.PathLike)):
            from .local_models import load_gfpgan_state_dict
            state_dict_or_path = load_gfpgan_state_dict(os.fspath(state_dict_or_path))
        self.net = GFPGANv1Clean(out_size).load_state_dict(state_dict_or_path)
        self.device, self.dtype = device, dtype
        self.reverse_channels = bool(reverse_channels)
        self.max_faces_per_launch = int(max_faces_per_launch)
        self.passes = 0          # passes of the net so far (tests, tools)
        self.timings = None      # a dict: receives (start, end) torch events per stage under the keys of STAGES -- tools/bench_gfpgan.py
        self._noise = {}

    # ---- device state ----------------------------------------------------------------------------------------------------------
    def _device(self) -> torch.device:
        from . import _capi
        _capi.lib()  # CAHipUnavailable when the extension is not built
        if not torch.cuda.is_available():
            raise _capi.CAHipUnavailable("FaceRestorer needs a GPU (there is no CPU fallback)")
        dev = torch.device(self.device if self.device is not None else "cuda")
        if dev.type != "cuda":
            raise _capi.CAHipUnavailable(f"FaceRestorer runs on the HIP kernels only (no CPU fallback), got device {dev}")
        if self.net.packed is None:
            self.net.prepare(dev, self.dtype)
        return dev

    def _check_noises(self, noises, n: int):
        want = self.net.noise_shapes(n)
        if not isinstance(noises, (list, tuple)) or len(noises) != len(want):
            raise ValueError(f"noises: a list of {len(want)} float32 tensors [n, h, w] (one at 4 x 4, then two per level), got "
                             f"{len(noises) if isinstance(noises, (list, tuple)) else type(noises).__name__}")
        for i, (t, shape) in enumerate(zip(noises, want)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
                raise TypeError(f"noise {i} must be a float32 tensor, got {getattr(t, 'dtype', type(t).__name__)}")
            if tuple(t.shape) != shape:
                raise ValueError(f"noise {i} has shape {tuple(t.shape)}, expected {shape}")

    def _draw_noises(self, n: int, dev, generator):
        """randomize_noise=True: the maps are drawn on the device by torch, into buffers cached per n, from `generator` (a generator of the
        device, or None for the default one)."""
        if n not in self._noise:
            self._noise[n] = [torch.empty(s, dtype=torch.float32, device=dev) for s in self.net.noise_shapes(n)]
        for t in self._noise[n]:
            t.normal_(generator=generator)
        return self._noise[n]

    def _timed(self, name, fn, *a, **kw):
        if self.timings is None:
            return fn(*a, **kw)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(*a, **kw)
        e1.record()
        self.timings.setdefault(name, []).append((e0, e1))
        return out

    def _run(self, faces, noises, generator, want_u8: bool, out=None):
        size = self.net.out_size
        t = _as_u8_faces(faces, size)
        n = t.shape[0]
        if noises is not None:
            self._check_noises(noises, n)
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (n, size, size, 3) or not out.is_contiguous() or not out.is_cuda:
                raise ValueError(f"out: a contiguous uint8 tensor {(n, size, size, 3)} on the device")
        dev = self._device()
        t = t.to(dev).contiguous()
        if noises is None:
            noises = self._draw_noises(n, dev, generator)
        else:
            noises = [x.to(dev).contiguous() for x in noises]
        from . import kernels as K
        step = self.max_faces_per_launch
        pres = []
        for i0 in range(0, n, step):
            pres.append(self.net.forward(t[i0:i0 + step], [x[i0:i0 + step] for x in noises], self.reverse_channels, timed=self._timed))
            self.passes += 1
        pre = pres[0] if len(pres) == 1 else torch.cat(pres)
        if not want_u8:
            return pre
        if out is None:
            out = torch.empty((n, size, size, 3), dtype=torch.uint8, device=dev)
        return self._timed("finish", K.gfp_finish, pre, out, self.reverse_channels)

    # ---- the public surface ------------------------------------------------------------------------------------------------------
    def restore_aligned(self, faces, noises=None, generator=None, out=None) -> torch.Tensor:
        """-> uint8 [n, 512, 512, 3] on the device, in the caller's channel order.  faces: a list of PIL images or uint8 arrays, or a uint8
        tensor [n, 512, 512, 3].  noises=None draws the decoder's noise maps on the device from `generator` (randomize_noise=True, what
        GFPGANer does); a list of 15 float32 tensors [n, h, w] (4 x 4, then two per level from 8 to 512) is used as given."""
        return self._run(faces, noises, generator, True, out)

    def pre_clamp(self, faces, noises) -> torch.Tensor:
        """-> float32 [n, 512, 512, 3]: the net's image before the clamp and the quantisation, in the net's own channel order (tests)."""
        return self._run(faces, noises, None, False)

    def enhance(self, img, has_aligned: bool = False, only_center_face: bool = False, paste_back: bool = True, weight: float = 0.5, face_helper=None,
                bg_upsampler=None, upscale: float = 2):
        """GFPGANer.enhance's control flow and return triple (cropped_faces, restored_faces, restored_img).  has_aligned=True needs no
        helper.  Otherwise `face_helper` is an object with facexlib.FaceRestoreHelper's methods (detection, warp and paste-back are
        face_align.FaceHelper's, the paste-back with a face_paste.FacePaster); all cropped faces of the frame go through the net in ONE pass.  `weight` is accepted as GFPGANer accepts it (the clean
        architecture ignores it)."""
        if has_aligned:
            arr = np.asarray(img)
            cropped = [arr]
            restored = [r for r in self.restore_aligned([arr]).cpu().numpy()]
            return cropped, restored, None
        if face_helper is None:
            raise NotImplementedError("enhance(has_aligned=False) needs a face_helper with facexlib.FaceRestoreHelper's methods (clean_all, read_image, "
                                      "get_face_landmarks_5, align_warp_face, cropped_faces, add_restored_face, get_inverse_affine, "
                                      "paste_faces_to_input_image): face detection (RetinaFace), the 5-point warp and the parsing-mask paste-back are "
                                      "not built in this project")
        face_helper.clean_all()
        face_helper.read_image(img)
        face_helper.get_face_landmarks_5(only_center_face=only_center_face, eye_dist_threshold=5)
        face_helper.align_warp_face()
        cropped = list(face_helper.cropped_faces)
        if cropped:
            for r in self.restore_aligned(cropped).cpu().numpy():
                face_helper.add_restored_face(r)
        if paste_back:
            bg_img = bg_upsampler.enhance(img, outscale=upscale)[0] if bg_upsampler is not None else None
            face_helper.get_inverse_affine(None)
            restored_img = face_helper.paste_faces_to_input_image(upsample_img=bg_img)
            return face_helper.cropped_faces, face_helper.restored_faces, restored_img
        return face_helper.cropped_faces, face_helper.restored_faces, None

    def as_face_enhancer(self, face_helper):
        """-> `(rgb_uint8, bg_upsampler=None) -> uint8 array`, the signature of `Upscaler`'s face_enhancer hook: the reference's
        `face_enhancer.enhance(output, has_aligned=False, only_center_face=False, paste_back=True)[2]` with the background upsampled by
        `bg_upsampler` at its own `scale` (GFPGANer(upscale=scale)).  The reference's behaviour is then
        `Upscaler(scale, face_enhancer=restorer.as_face_enhancer(helper))`.  With real weights and facexlib this path is unmeasured and
        unpinned."""
        if face_helper is None:
            raise NotImplementedError("as_face_enhancer needs a face_helper (see FaceRestorer.enhance)")

        def face_enhancer(rgb_uint8, bg_upsampler=None):
            upscale = getattr(bg_upsampler, "scale", 2) if bg_upsampler is not None else 2
            return self.enhance(rgb_uint8, has_aligned=False, only_center_face=False, paste_back=True, face_helper=face_helper, bg_upsampler=bg_upsampler,
                                upscale=upscale)[2]

        return face_enhancer


# what stands in front of `restore_aligned` for frames that are not aligned yet: detection, fit and warp (face_align.py)
from .face_align import FaceAligner, FaceHelper  # noqa: E402,F401
# ... and what stands behind it: ParseNet, the mask blur and the blend back into the frame (face_paste.py; opt-in)
from .face_paste import FaceEnhancer, FacePaster  # noqa: E402,F401
