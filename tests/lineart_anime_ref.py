"""Test helpers: the specification of the lineart_anime annotator (controlanimate_amd/lineart_anime.py), restated on the CPU.

  * `UnetGenerator`: the fp32 torch network, written from the published pix2pix UnetGenerator(3, 1, num_downs=8, ngf=64,
    norm_layer=InstanceNorm2d(affine=False, track_running_stats=False), use_dropout=False) as controlnet_aux's LineartAnimeDetector
    builds it, from real nn modules WITH their in-place activations (their effect is part of the behaviour: the skip tensor that a
    block concatenates has been through its own LeakyReLU(0.2, inplace) and then goes through the parent's ReLU(inplace)).  Every
    convolution has a bias.  Its state dict has the 32 keys of netG.pth (54,405,505 parameters).
  * `lineart_anime_detect`: LineartAnimeDetector.__call__ in numpy for sizes at which all of its resamplings are the identity
    (detect_resolution = image_resolution = min(H, W), H and W multiples of 256): a grey frame repeated to three channels,
    x = float32(uint8) / 127.5 - 1.0 as NCHW, line = model(x)[0, 0] * 127.5 + 127.5, clip(0, 255) truncated to uint8,
    map = 255 - line, three equal channels.
  * `finish_ref`: that last step from the pre-tanh values (the network's output before the tanh).
  * `emulate_pre_tanh`: the chain with every activation and weight stored in fp16 / bf16 and fp32 accumulation (what the device
    computes, on the CPU), for the error figures quoted in tests/test_lineart_anime_gpu.py.

controlnet_aux and OpenCV are not installed here and no netG.pth is available: none of this has a fixture produced by those
packages, key names and parity are UNPINNED against them.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

CHANNELS = (64, 128, 256, 512, 512, 512, 512, 512)


def _norm(c: int) -> nn.Module:
    return nn.InstanceNorm2d(c, affine=False, track_running_stats=False)


class UnetSkipConnectionBlock(nn.Module):
    """X -------------------identity----------------------
       |-- downsampling -- |submodule| -- upsampling --|"""

    def __init__(self, outer_nc: int, inner_nc: int, input_nc=None, submodule=None, outermost: bool = False, innermost: bool = False):
        super().__init__()
        self.outermost = outermost
        if input_nc is None:
            input_nc = outer_nc
        downconv = nn.Conv2d(input_nc, inner_nc, kernel_size=4, stride=2, padding=1, bias=True)
        downrelu, downnorm = nn.LeakyReLU(0.2, True), _norm(inner_nc)
        uprelu, upnorm = nn.ReLU(True), _norm(outer_nc)
        if outermost:
            upconv = nn.ConvTranspose2d(inner_nc * 2, outer_nc, kernel_size=4, stride=2, padding=1)
            model = [downconv, submodule, uprelu, upconv, nn.Tanh()]
        elif innermost:
            upconv = nn.ConvTranspose2d(inner_nc, outer_nc, kernel_size=4, stride=2, padding=1, bias=True)
            model = [downrelu, downconv, uprelu, upconv, upnorm]
        else:
            upconv = nn.ConvTranspose2d(inner_nc * 2, outer_nc, kernel_size=4, stride=2, padding=1, bias=True)
            model = [downrelu, downconv, downnorm, submodule, uprelu, upconv, upnorm]
        self.model = nn.Sequential(*model)

    def forward(self, x):
        if self.outermost:
            return self.model(x)
        return torch.cat([x, self.model(x)], 1)


class UnetGenerator(nn.Module):
    def __init__(self, input_nc: int = 3, output_nc: int = 1, num_downs: int = 8, ngf: int = 64):
        super().__init__()
        block = UnetSkipConnectionBlock(ngf * 8, ngf * 8, innermost=True)
        for _ in range(num_downs - 5):
            block = UnetSkipConnectionBlock(ngf * 8, ngf * 8, submodule=block)
        block = UnetSkipConnectionBlock(ngf * 4, ngf * 8, submodule=block)
        block = UnetSkipConnectionBlock(ngf * 2, ngf * 4, submodule=block)
        block = UnetSkipConnectionBlock(ngf, ngf * 2, submodule=block)
        self.model = UnetSkipConnectionBlock(output_nc, ngf, input_nc=input_nc, submodule=block, outermost=True)

    def pre_tanh(self, x):
        """The output before the tanh."""
        return self.model.model[:-1](x)

    def forward(self, x):
        return self.model(x)


def lineart_anime_state_dict(seed: int = 0, out_scale: float = 1.0) -> dict:
    """Seeded weights: He-normal convolutions (fan-in of the convolution; of the equivalent 2x2 convolution for the transposed ones:
    an output pixel of a 4x4 stride-2 transposed convolution sees 4 of the 16 taps) with small asymmetric biases; the last
    transposed convolution's weight scaled by out_scale (the pre-tanh values' spread)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in UnetGenerator().state_dict().items():
        if k.endswith(".weight"):
            transposed = k.endswith((".model.3.weight", ".model.5.weight"))   # a block's last-but-one / last-but-two module: its upconv
            fan_in = v.shape[0] * 4 if transposed else v.shape[1] * 16
            w = torch.randn(v.shape, generator=g) * math.sqrt(2.0 / fan_in)
            sd[k] = w * out_scale if k == "model.model.3.weight" else w
        else:
            n = v.shape[0]
            sd[k] = (torch.arange(n, dtype=torch.float32) / max(n - 1, 1) - 0.4) * 0.1 + torch.randn(n, generator=g) * 0.02
    return sd


def strip_module_prefix(sd: dict) -> dict:
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}


def lineart_anime_net(sd: dict) -> UnetGenerator:
    net = UnetGenerator()
    net.load_state_dict({k: v.float() for k, v in strip_module_prefix(sd).items()}, strict=True)
    return net.eval()


def to_input(frames: np.ndarray) -> torch.Tensor:
    """uint8 [n, H, W, 3] -> float32 [n, 3, H, W] = float32(uint8) / 127.5 - 1.0."""
    a = torch.from_numpy(np.ascontiguousarray(frames)).float()
    return (a / 127.5 - 1.0).permute(0, 3, 1, 2).contiguous()


def pre_tanh_ref(sd: dict, frames: np.ndarray) -> torch.Tensor:
    """uint8 RGB [n, H, W, 3] -> float32 pre-tanh values [n, H, W] (the fp32 net on the CPU)."""
    with torch.no_grad():
        return lineart_anime_net(sd).pre_tanh(to_input(frames))[:, 0].contiguous()


def finish_ref(pre: np.ndarray):
    """float32 pre-tanh values -> (the uint8 map 255 - uint8(clip(tanh * 127.5 + 127.5, 0, 255)), the float64 value
    tanh * 127.5 + 127.5 before clip and truncation).  The detector's own arithmetic is float32 (torch's tanh, * 127.5 + 127.5 on
    the float32 tensor): the map is computed so."""
    t = np.asarray(pre, dtype=np.float32)
    line = (torch.tanh(torch.from_numpy(t)) * 127.5 + 127.5).numpy()
    level = line.clip(0, 255).astype(np.uint8)
    scaled = np.tanh(t.astype(np.float64)) * 127.5 + 127.5
    return (255 - level).astype(np.uint8), scaled


def lineart_anime_detect(sd: dict, image: np.ndarray) -> np.ndarray:
    """LineartAnimeDetector.__call__(image, detect_resolution=min(H, W), image_resolution=min(H, W)) for a uint8 [H, W] or [H, W, 3]
    array with H % 256 == W % 256 == 0 -> uint8 [H, W, 3] with three equal channels."""
    img = np.asarray(image)
    assert img.dtype == np.uint8
    if img.ndim == 2:
        img = np.repeat(img[:, :, None], 3, axis=2)
    assert img.ndim == 3 and img.shape[2] == 3
    if img.shape[0] % 256 or img.shape[1] % 256:
        raise NotImplementedError(f"{img.shape[:2]}: the detector's resamplings are restated only where they are the identity")
    with torch.no_grad():
        line = (lineart_anime_net(sd)(to_input(img[None]))[0, 0] * 127.5 + 127.5).numpy()
    level = line.clip(0, 255).astype(np.uint8)
    return np.repeat((255 - level)[:, :, None], 3, axis=2)


def emulate_pre_tanh(sd: dict, frames: np.ndarray, dtype) -> torch.Tensor:
    """The chain as the device runs it, on the CPU: weights and every stored activation rounded to `dtype`, convolutions and
    InstanceNorm statistics in fp32, biases only where no InstanceNorm follows, the last transposed convolution with fp32 weights."""
    sd = strip_module_prefix(sd)

    def r(t):
        return t.to(dtype).float()

    def keys(i):
        p = ("model" if i == 0 else "model.model.1" + ".model.3" * (i - 1)) + ".model."
        return (p + "0", p + "3") if i == 0 else (p + "1", p + ("3" if i == 7 else "5"))

    def inorm(t):
        return F.instance_norm(t, eps=1e-5)

    with torch.no_grad():
        d = F.conv2d(to_input(frames), r(sd[keys(0)[0] + ".weight"]), sd[keys(0)[0] + ".bias"].float(), stride=2, padding=1)
        leaky, skips = r(F.leaky_relu(d, 0.2)), [r(F.relu(d))]
        for i in range(1, 7):
            d = inorm(r(F.conv2d(leaky, r(sd[keys(i)[0] + ".weight"]), stride=2, padding=1)))
            leaky = r(F.leaky_relu(d, 0.2))
            skips.append(r(F.relu(d)))
        x = r(F.relu(F.conv2d(leaky, r(sd[keys(7)[0] + ".weight"]), sd[keys(7)[0] + ".bias"].float(), stride=2, padding=1)))
        for i in range(7, 0, -1):
            u = r(F.relu(inorm(r(F.conv_transpose2d(x, r(sd[keys(i)[1] + ".weight"]), stride=2, padding=1)))))
            x = torch.cat([skips[i - 1], u], 1)
        out = F.conv_transpose2d(x, sd[keys(0)[1] + ".weight"].float(), sd[keys(0)[1] + ".bias"].float(), stride=2, padding=1)
    return out[:, 0].contiguous()


def frames_fixture(h: int = 256, w: int = 256, n: int = 2, seed: int = 7) -> np.ndarray:
    """n RGB frames of h x w with smooth, periodic and blocky content plus noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for i in range(n):
        a = np.zeros((h, w, 3), np.float64)
        a[..., 0] = 128 + 100 * np.sin(xx / (9.0 + i)) * np.cos(yy / 13.0)
        a[..., 1] = (xx * 2 + yy * (3 + i)) % 256
        a[..., 2] = 255 * ((xx // 32 + yy // 32 + i) % 2)
        a += rng.normal(0, 12, a.shape)
        out.append(a.clip(0, 255).astype(np.uint8))
    return np.stack(out)


def finish_case():
    """n = 2 maps of 24 x 40 seeded N(0, 0.75^2) pre-tanh values (the spread of the seeded network's) with the extremes and both zeros in
    front, what the specification makes of them, and where it is decided (float64 tanh * 127.5 + 127.5 further than 1e-3 from an integer)
    -> (n, h, w, pre, want, decided)."""
    n, h, w = 2, 24, 40
    pre = (np.random.default_rng(4).standard_normal((n, h, w)) * 0.75).astype(np.float32)
    pre[0, 0, :4] = [-100.0, 100.0, 0.0, -0.0]
    want, scaled = finish_ref(pre)
    return n, h, w, pre, want, np.abs(scaled - np.rint(scaled)) > 1e-3
