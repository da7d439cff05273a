"""Test helpers: fp32 CPU restatements of the Real-ESRGAN path the upscaler replicates.

  * `rrdb_forward`: basicsr's RRDBNet.forward for scale 4 (RRDB = three ResidualDenseBlocks, `x5 * 0.2 + x` and
    `out * 0.2 + x`, LeakyReLU(0.2), nearest x2 upsamplings before conv_up1 / conv_up2), written with torch.nn.functional on
    the CPU from the published architecture;
  * `enhance_ref`: RealESRGANer.enhance(img, outscale) for a uint8 H x W x 3 array (half=True, tile=0, pre_pad=0): BGR -> RGB
    (the reference passes RGB, so the net sees the channels reversed), /255, fp16 input, net, clamp(0, 1), channels back,
    (x * 255).round() to uint8, then cv2.resize(INTER_LANCZOS4) when outscale != 4;
  * `resize_lanczos4_ref`: OpenCV's INTER_LANCZOS4 integer path for 8-bit data (11-bit coefficients, separable horizontal then
    vertical sums, rounding shift by 22, saturation, edge replication).

basicsr, realesrgan and OpenCV are not installed here: none of this has a reference-produced fixture, it is UNPINNED against
those packages.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F


def rrdb_state_dict(seed: int = 0, num_block: int = 6) -> dict:
    """Seeded RRDBNet weights: kaiming-normal x 0.1 (basicsr's default_init_weights scale for RRDB blocks) and asymmetric
    per-channel biases, so that a channel-order mistake shows."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(name, cin, cout, scale=0.1):
        w = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (cin * 9)) * scale
        b = (torch.arange(cout, dtype=torch.float32) / max(cout - 1, 1) - 0.3) * 0.05 + torch.randn(cout, generator=g) * 0.01
        sd[name + ".weight"], sd[name + ".bias"] = w, b

    conv("conv_first", 3, 64, 1.0)
    for i in range(num_block):
        for r in ("rdb1", "rdb2", "rdb3"):
            for c in range(1, 6):
                conv(f"body.{i}.{r}.conv{c}", 64 + 32 * (c - 1), 32 if c < 5 else 64)
    for n in ("conv_body", "conv_up1", "conv_up2", "conv_hr"):
        conv(n, 64, 64, 1.0)
    conv("conv_last", 64, 3, 1.0)
    sd["conv_last.bias"] = torch.tensor([0.30, 0.45, 0.60])  # strongly asymmetric: a swapped channel order shows at once
    return sd


def rrdb_forward(sd: dict, x: torch.Tensor, num_block: int = 6) -> torch.Tensor:
    def conv(n, t):
        return F.conv2d(t, sd[n + ".weight"].float(), sd[n + ".bias"].float(), padding=1)

    def lrelu(t):
        return F.leaky_relu(t, 0.2)

    def rdb(p, x0):
        x1 = lrelu(conv(p + ".conv1", x0))
        x2 = lrelu(conv(p + ".conv2", torch.cat((x0, x1), 1)))
        x3 = lrelu(conv(p + ".conv3", torch.cat((x0, x1, x2), 1)))
        x4 = lrelu(conv(p + ".conv4", torch.cat((x0, x1, x2, x3), 1)))
        x5 = conv(p + ".conv5", torch.cat((x0, x1, x2, x3, x4), 1))
        return x5 * 0.2 + x0

    feat = conv("conv_first", x)
    body = feat
    for i in range(num_block):
        out = rdb(f"body.{i}.rdb3", rdb(f"body.{i}.rdb2", rdb(f"body.{i}.rdb1", body)))
        body = out * 0.2 + body
    feat = feat + conv("conv_body", body)
    feat = lrelu(conv("conv_up1", F.interpolate(feat, scale_factor=2, mode="nearest")))
    feat = lrelu(conv("conv_up2", F.interpolate(feat, scale_factor=2, mode="nearest")))
    return conv("conv_last", lrelu(conv("conv_hr", feat)))


def enhance_ref(img: np.ndarray, sd: dict, outscale: float = 4.0):
    """-> (uint8 result, float net output [3, 4H, 4W] in the net's channel order before clamp / quantisation)."""
    h, w = img.shape[:2]
    x = img.astype(np.float32) / 255.0
    x = x[:, :, ::-1]  # cv2.cvtColor(img, COLOR_BGR2RGB) on what is really RGB
    t = torch.from_numpy(np.ascontiguousarray(np.transpose(x, (2, 0, 1))))[None].half().float()
    with torch.no_grad():
        raw = rrdb_forward(sd, t)[0]
    out = raw.clamp(0, 1).numpy()
    out = np.transpose(out[[2, 1, 0], :, :], (1, 2, 0))
    u8 = (out * 255.0).round().astype(np.uint8)
    if outscale != 4:
        u8 = resize_lanczos4_ref(u8, int(w * outscale), int(h * outscale))
    return u8, raw


def _coeffs(x: np.float32):
    f32 = np.float32
    s45 = 0.70710678118654752440084436210485
    cs = [(1, 0), (-s45, -s45), (0, 1), (s45, -s45), (-1, 0), (s45, s45), (0, -1), (-s45, s45)]
    y0 = float(-(x + f32(3))) * math.pi * 0.25
    s0, c0 = math.sin(y0), math.cos(y0)
    c = np.zeros(8, dtype=np.float32)
    total = f32(0)
    for i in range(8):
        d = f32(f32(x + f32(3)) - f32(i))
        if abs(d) >= f32(1e-6):
            y = float(-d) * math.pi * 0.25
            c[i] = f32((cs[i][0] * s0 + cs[i][1] * c0) / (y * y))
        else:
            c[i] = f32(1e30)
        total = f32(total + c[i])
    inv = f32(f32(1.0) / total)
    return (c * inv).astype(np.float32)


def _axis(src: int, dst: int):
    scale = 1.0 / (dst / src)
    idx = np.zeros((dst, 8), dtype=np.int64)
    coef = np.zeros((dst, 8), dtype=np.int64)
    for d in range(dst):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = math.floor(f)
        f = np.float32(f - np.float32(s))
        idx[d] = np.clip(np.arange(s - 3, s + 5), 0, src - 1)
        coef[d] = np.clip(np.rint(_coeffs(f) * np.float32(2048)), -32768, 32767).astype(np.int64)
    return idx, coef


def resize_lanczos4_ref(img: np.ndarray, dw: int, dh: int) -> np.ndarray:
    """cv2.resize(img, (dw, dh), interpolation=cv2.INTER_LANCZOS4) for uint8 H x W x C."""
    sh, sw = img.shape[:2]
    xi, xa = _axis(sw, dw)
    yi, ya = _axis(sh, dh)
    src = img.astype(np.int64)
    hbuf = np.zeros((sh, dw) + img.shape[2:], dtype=np.int64)
    for k in range(8):
        hbuf += src[:, xi[:, k]] * (xa[:, k][:, None] if img.ndim == 3 else xa[:, k])
    acc = np.zeros((dh, dw) + img.shape[2:], dtype=np.int64)
    for k in range(8):
        acc += hbuf[yi[:, k]] * ya[:, k].reshape((dh,) + (1,) * (img.ndim - 1))
    return np.clip((acc + (1 << 21)) >> 22, 0, 255).astype(np.uint8)
