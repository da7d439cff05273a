"""The specification of the depth annotator (controlanimate_amd/depth.py): test infrastructure, never imported by the product.

  * `forward(sd, cfg, pixel_values)`: transformers' DPTForDepthEstimation (the plain-ViT DPT: readout "project", reassemble factors
    (4, 2, 1, 0.5), no batch norm) as a functional torch restatement over the checkpoint's own keys, in the dtype of `pixel_values`;
    returns (predicted_depth [n, S, S], the hidden states after the backbone_out_indices layers).
  * `pil_coeffs` / `pil_resize`: Pillow's Image.resize for uint8 (Resample.c: two passes, 22-bit fixed-point coefficients, the
    intermediate rounded and clipped to uint8), in numpy.
  * `preprocess`: DPTImageProcessor with do_resize to a square, mean = std = 0.5.
  * `bicubic_resize`: torch's interpolate(mode="bicubic", align_corners=False) (A = -0.75, clamped indices), in numpy float32.
  * `quantize_max` / `quantize_minmax`: the two uint8 maps.  "max" is the formula of the depth-estimation pipeline of transformers 4.34.1,
    (d * 255 / d.max()).astype(uint8), restated and not run; "minmax" the one of the installed pipeline.  Both truncate toward zero; a
    scaled value <= -1 (the bicubic undershoot under "max") SATURATES to 0 here, where numpy's cast is platform-defined (it wraps on
    x86): `quantize_max` also returns the mask of those pixels.  A frame with max = 0 (or max = min) gives an all-zero map.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

TINY_CONFIG = dict(hidden_size=32, num_hidden_layers=4, num_attention_heads=2, intermediate_size=64, image_size=96, patch_size=16,
                   backbone_out_indices=[0, 1, 2, 3], neck_hidden_sizes=[16, 32, 64, 64], fusion_hidden_size=64)
LARGE_CONFIG = dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096, image_size=384, patch_size=16,
                    backbone_out_indices=[5, 11, 17, 23], neck_hidden_sizes=[256, 512, 1024, 1024], fusion_hidden_size=256)
LAYER_NORM_EPS = 1e-12
REASSEMBLE_FACTORS = (4, 2, 1, 0.5)


def key_shapes(cfg: dict) -> dict:
    """name -> shape of every tensor of the DPTForDepthEstimation checkpoint of `cfg` (142 for the tiny config)."""
    c, inter, p = cfg["hidden_size"], cfg["intermediate_size"], cfg["patch_size"]
    tokens = (cfg["image_size"] // p) ** 2 + 1
    fh = cfg["fusion_hidden_size"]
    out = {"dpt.embeddings.cls_token": (1, 1, c), "dpt.embeddings.position_embeddings": (1, tokens, c),
           "dpt.embeddings.patch_embeddings.projection.weight": (c, 3, p, p), "dpt.embeddings.patch_embeddings.projection.bias": (c,)}

    def lin(name, n, k):
        out[name + ".weight"], out[name + ".bias"] = (n, k), (n,)

    def conv(name, co, ci, k, bias=True):
        out[name + ".weight"] = (co, ci, k, k)
        if bias:
            out[name + ".bias"] = (co,)

    for i in range(cfg["num_hidden_layers"]):
        pre = f"dpt.encoder.layer.{i}."
        for nm in ("query", "key", "value"):
            lin(pre + "attention.attention." + nm, c, c)
        lin(pre + "attention.output.dense", c, c)
        lin(pre + "intermediate.dense", inter, c)
        lin(pre + "output.dense", c, inter)
        for nm in ("layernorm_before", "layernorm_after"):
            out[pre + nm + ".weight"], out[pre + nm + ".bias"] = (c,), (c,)
    out["dpt.layernorm.weight"], out["dpt.layernorm.bias"] = (c,), (c,)
    for i, (ch, f) in enumerate(zip(cfg["neck_hidden_sizes"], REASSEMBLE_FACTORS)):
        pre = f"neck.reassemble_stage.layers.{i}."
        conv(pre + "projection", ch, c, 1)
        if f > 1:
            conv(pre + "resize", ch, ch, int(f))   # ConvTranspose2d: [Cin, Cout, k, k]
        elif f < 1:
            conv(pre + "resize", ch, ch, 3)
    for i in range(4):
        lin(f"neck.reassemble_stage.readout_projects.{i}.0", c, 2 * c)
    for i, ch in enumerate(cfg["neck_hidden_sizes"]):
        conv(f"neck.convs.{i}", fh, ch, 3, bias=False)
    for i in range(4):
        pre = f"neck.fusion_stage.layers.{i}."
        conv(pre + "projection", fh, fh, 1)
        for r in ("residual_layer1", "residual_layer2"):
            conv(pre + r + ".convolution1", fh, fh, 3)
            conv(pre + r + ".convolution2", fh, fh, 3)
    conv("head.head.0", fh // 2, fh, 3)
    conv("head.head.2", 32, fh // 2, 3)
    conv("head.head.4", 1, 32, 1)
    return out


def seeded_state_dict(cfg: dict, seed: int = 0, device="cpu", dtype=torch.float32) -> dict:
    """Seeded weights of the shapes of `cfg`, generated on `device`, scaled so that activations stay O(1): matrices and convolutions
    normal with std 1 / sqrt(fan_in), LayerNorm weights 1 + 0.1 N, biases 0.05 N, the last bias 0.1 (the ReLU then clips little)."""
    g = torch.Generator(device=device).manual_seed(seed)
    sd = {}
    for k, shape in key_shapes(cfg).items():
        if "layernorm" in k and k.endswith(".weight"):
            t = 1 + 0.1 * torch.randn(shape, generator=g, device=device)
        elif k.endswith(".bias"):
            t = 0.05 * torch.randn(shape, generator=g, device=device)
        elif k.endswith("cls_token") or k.endswith("position_embeddings"):
            t = 0.5 * torch.randn(shape, generator=g, device=device)
        else:
            fan_in = math.prod(shape[1:]) if "resize" not in k or len(shape) != 4 or shape[2] == 3 else shape[0]
            t = torch.randn(shape, generator=g, device=device) * fan_in ** -0.5
        sd[k] = t.to(dtype)
    sd["head.head.4.bias"] = torch.full((1,), 0.1, device=device, dtype=dtype)
    sd["head.head.4.weight"] = sd["head.head.4.weight"].abs() * 0.5
    return sd


# ---- the network -------------------------------------------------------------------------------------------------------------------
def vit(sd, cfg, pixel_values):
    """-> the hidden states after every encoder layer, each [n, tokens, C]."""
    c, heads = cfg["hidden_size"], cfg["num_attention_heads"]
    n = pixel_values.shape[0]
    x = F.conv2d(pixel_values, sd["dpt.embeddings.patch_embeddings.projection.weight"], sd["dpt.embeddings.patch_embeddings.projection.bias"],
                 stride=cfg["patch_size"]).flatten(2).transpose(1, 2)
    x = torch.cat([sd["dpt.embeddings.cls_token"].expand(n, -1, -1), x], 1) + sd["dpt.embeddings.position_embeddings"]
    t = x.shape[1]
    hidden = []
    for i in range(cfg["num_hidden_layers"]):
        p = f"dpt.encoder.layer.{i}."
        h = F.layer_norm(x, (c,), sd[p + "layernorm_before.weight"], sd[p + "layernorm_before.bias"], LAYER_NORM_EPS)
        q, k, v = (F.linear(h, sd[p + f"attention.attention.{nm}.weight"], sd[p + f"attention.attention.{nm}.bias"]).view(n, t, heads, c // heads).transpose(1, 2)
                   for nm in ("query", "key", "value"))
        a = torch.softmax(q @ k.transpose(-1, -2) * (c // heads) ** -0.5, -1) @ v
        a = a.transpose(1, 2).reshape(n, t, c)
        x = F.linear(a, sd[p + "attention.output.dense.weight"], sd[p + "attention.output.dense.bias"]) + x
        h = F.layer_norm(x, (c,), sd[p + "layernorm_after.weight"], sd[p + "layernorm_after.bias"], LAYER_NORM_EPS)
        h = F.gelu(F.linear(h, sd[p + "intermediate.dense.weight"], sd[p + "intermediate.dense.bias"]))
        x = F.linear(h, sd[p + "output.dense.weight"], sd[p + "output.dense.bias"]) + x
        hidden.append(x)
    return hidden


def _rcu(sd, p, x):
    h = F.conv2d(F.relu(x), sd[p + "convolution1.weight"], sd[p + "convolution1.bias"], padding=1)
    return F.conv2d(F.relu(h), sd[p + "convolution2.weight"], sd[p + "convolution2.bias"], padding=1) + x


def head_tail(sd, x):
    """head.head.1 .. 5 on the output of head.head.0: align-corners x2, 3x3 + ReLU, 1x1 + ReLU -> [n, 2h, 2w]."""
    x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    x = F.relu(F.conv2d(x, sd["head.head.2.weight"], sd["head.head.2.bias"], padding=1))
    return F.relu(F.conv2d(x, sd["head.head.4.weight"], sd["head.head.4.bias"]))[:, 0]


def forward(sd, cfg, pixel_values):
    c = cfg["hidden_size"]
    g = cfg["image_size"] // cfg["patch_size"]
    n = pixel_values.shape[0]
    hidden = vit(sd, cfg, pixel_values)
    taps = [hidden[i] for i in cfg["backbone_out_indices"]]
    feats = []
    for i, h in enumerate(taps):
        cls, tok = h[:, :1], h[:, 1:]
        pre = f"neck.reassemble_stage.readout_projects.{i}.0."
        tok = F.gelu(F.linear(torch.cat([tok, cls.expand_as(tok)], -1), sd[pre + "weight"], sd[pre + "bias"]))
        x = tok.transpose(1, 2).reshape(n, c, g, g)
        pre = f"neck.reassemble_stage.layers.{i}."
        x = F.conv2d(x, sd[pre + "projection.weight"], sd[pre + "projection.bias"])
        f = REASSEMBLE_FACTORS[i]
        if f > 1:
            x = F.conv_transpose2d(x, sd[pre + "resize.weight"], sd[pre + "resize.bias"], stride=int(f))
        elif f < 1:
            x = F.conv2d(x, sd[pre + "resize.weight"], sd[pre + "resize.bias"], stride=2, padding=1)
        feats.append(F.conv2d(x, sd[f"neck.convs.{i}.weight"], None, padding=1))
    fused = None
    for j, x in enumerate(feats[::-1]):
        pre = f"neck.fusion_stage.layers.{j}."
        h = x if fused is None else fused + _rcu(sd, pre + "residual_layer1.", x)
        h = _rcu(sd, pre + "residual_layer2.", h)
        h = F.interpolate(h, scale_factor=2, mode="bilinear", align_corners=True)
        fused = F.conv2d(h, sd[pre + "projection.weight"], sd[pre + "projection.bias"])
    x = F.conv2d(fused, sd["head.head.0.weight"], sd["head.head.0.bias"], padding=1)
    return head_tail(sd, x), taps


# ---- Pillow's resampler ------------------------------------------------------------------------------------------------------------
PIL_BILINEAR, PIL_BICUBIC = 2, 3
PRECISION_BITS = 32 - 8 - 2


def _bilinear_filter(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic_filter(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def pil_coeffs(in_size: int, out_size: int, resample: int):
    """precompute_coeffs + normalize_coeffs_8bpc -> (bounds int32 [out, 2] = (first source index, taps), coefficients int32 [out, ksize])."""
    filt, support = {PIL_BILINEAR: (_bilinear_filter, 1.0), PIL_BICUBIC: (_bicubic_filter, 2.0)}[resample]
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [filt((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        for x, v in enumerate(w):
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    return bounds, kk


def _pil_pass(a: np.ndarray, bounds, kk, axis: int) -> np.ndarray:
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((len(bounds),) + a.shape[1:], np.uint8)
    for i, (xmin, xmax) in enumerate(bounds):
        ssum = np.tensordot(kk[i, :xmax].astype(np.int64), a[xmin:xmin + xmax], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        out[i] = np.clip(ssum >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def pil_resize(img: np.ndarray, dh: int, dw: int, resample: int) -> np.ndarray:
    """uint8 [H, W, C] -> uint8 [dh, dw, C]: Image.fromarray(img).resize((dw, dh), resample), horizontal pass first."""
    h, w = img.shape[:2]
    if (h, w) == (dh, dw):
        return img.copy()
    if w != dw:
        img = _pil_pass(img, *pil_coeffs(w, dw, resample), axis=1)
    if h != dh:
        img = _pil_pass(img, *pil_coeffs(h, dh, resample), axis=0)
    return img


def preprocess(frames, size: int, resample: int) -> np.ndarray:
    """uint8 frames [H, W, 3] -> pixel_values float32 [n, 3, size, size]."""
    out = [((pil_resize(np.asarray(f), size, size, resample).astype(np.float32) * np.float32(1 / 255)) - np.float32(0.5)) / np.float32(0.5) for f in frames]
    return np.stack(out).transpose(0, 3, 1, 2)


# ---- the tail ------------------------------------------------------------------------------------------------------------------------
def _cubic_taps(in_size: int, out_size: int):
    a = np.float32(-0.75)
    scale = np.float32(in_size) / np.float32(out_size)
    # scale * (dst + 0.5) - 0.5 with ONE rounding: torch's kernels are compiled with contraction, and a source coordinate that is one ulp
    # off moves an upsampled value by 3e-6 of the largest one
    src = (np.float64(scale) * (np.arange(out_size, dtype=np.float64) + 0.5) - 0.5).astype(np.float32)
    i0 = np.floor(src)
    t = (src - i0).astype(np.float32)

    def c1(x):
        return ((a + 2) * x - (a + 3)) * x * x + 1

    def c2(x):
        return ((a * x - 5 * a) * x + 8 * a) * x - 4 * a

    w = np.stack([c2(t + 1), c1(t), c1(1 - t), c2((1 - t) + 1)], 1).astype(np.float32)
    idx = np.clip(i0.astype(np.int64)[:, None] + np.arange(-1, 3)[None], 0, in_size - 1)
    return idx, w


def bicubic_resize(d: np.ndarray, dh: int, dw: int) -> np.ndarray:
    """float32 [n, h, w] -> float32 [n, dh, dw]."""
    d = np.asarray(d, np.float32)
    iy, wy = _cubic_taps(d.shape[1], dh)
    ix, wx = _cubic_taps(d.shape[2], dw)
    rows = (d[:, :, ix] * wx[None, None]).sum(-1, dtype=np.float32)          # [n, h, dw]
    return (rows[:, iy] * wy[None, :, :, None]).sum(2, dtype=np.float32)     # [n, dh, dw]


def _trunc_u8(v: np.ndarray):
    """Truncation toward zero into 0 .. 255; values <= -1 saturate to 0 (the deviation from numpy's cast), NaN counts as 0."""
    v = np.nan_to_num(v, nan=0.0)
    return np.clip(np.trunc(v), 0, 255).astype(np.uint8)


def scaled_max(d: np.ndarray) -> np.ndarray:
    d = np.asarray(d, np.float32)
    mx = d.max()
    return np.zeros_like(d) if not mx > 0 else (d * np.float32(255)) / mx


def scaled_minmax(d: np.ndarray) -> np.ndarray:
    d = np.asarray(d, np.float32)
    mx, mn = d.max(), d.min()
    return np.zeros_like(d) if not mx > mn else ((d - mn) / (mx - mn)) * np.float32(255)


def quantize_max(d: np.ndarray):
    """One frame float32 [H, W] -> (uint8 [H, W], the mask of the pixels whose scaled value is <= -1: saturated to 0 here)."""
    v = scaled_max(d)
    return _trunc_u8(v), v <= -1


def quantize_minmax(d: np.ndarray) -> np.ndarray:
    return _trunc_u8(scaled_minmax(d))


def load_fixture():
    """tests/golden/dpt_tiny*.npz (made by tests/golden/make_dpt_golden.py) -> (the recorded arrays, the state dict as float32 tensors)."""
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    data = dict(np.load(os.path.join(here, "dpt_tiny.npz")))
    sd = {}
    for part in ("dpt_tiny_w0.npz", "dpt_tiny_w1.npz"):
        for k, v in np.load(os.path.join(here, part)).items():
            sd[k[2:]] = torch.from_numpy(v.astype(np.float32))
    return data, sd
