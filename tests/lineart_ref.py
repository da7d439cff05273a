"""Test helpers: the specification of the lineart annotator (controlanimate_amd/lineart.py), restated on the CPU.

  * `Generator`: the fp32 torch network, written from the published "informative drawings" Generator(3, 1, n_residual_blocks=3) as
    controlnet_aux's LineartDetector builds it: ReflectionPad2d(3) + Conv2d(3, 64, 7) + InstanceNorm2d + ReLU; two stride-2
    convolutions; three residual blocks of reflection-padded 3x3 convolutions; two transposed convolutions; ReflectionPad2d(3) +
    Conv2d(64, 1, 7) + Sigmoid.  InstanceNorm2d is torch's default: affine=False, eps=1e-5, biased variance.  Its state dict has the
    24 keys of sk_model.pth / sk_model2.pth.
  * `lineart_detect`: LineartDetector.__call__ in numpy for sizes at which both of its resamplings are the identity
    (detect_resolution = image_resolution = min(H, W), H and W multiples of 64): a grey frame repeated to three channels,
    x = uint8 / 255.0 as NCHW float32, line = model(x)[0][0], map = 255 - uint8(clip(line * 255.0, 0, 255)), three equal channels.
  * `finish_ref`: that last step from the logits (the network's output before the sigmoid).

controlnet_aux and OpenCV are not installed here and no sk_model.pth is available: none of this has a fixture produced by those
packages, it is UNPINNED against them.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn as nn

N_RES_BLOCKS = 3


class ResidualBlock(nn.Module):
    def __init__(self, in_features: int):
        super().__init__()
        self.conv_block = nn.Sequential(nn.ReflectionPad2d(1), nn.Conv2d(in_features, in_features, 3), nn.InstanceNorm2d(in_features), nn.ReLU(inplace=True),
                                        nn.ReflectionPad2d(1), nn.Conv2d(in_features, in_features, 3), nn.InstanceNorm2d(in_features))

    def forward(self, x):
        return x + self.conv_block(x)


class Generator(nn.Module):
    def __init__(self, input_nc: int = 3, output_nc: int = 1, n_residual_blocks: int = N_RES_BLOCKS, sigmoid: bool = True):
        super().__init__()
        self.model0 = nn.Sequential(nn.ReflectionPad2d(3), nn.Conv2d(input_nc, 64, 7), nn.InstanceNorm2d(64), nn.ReLU(inplace=True))
        self.model1 = nn.Sequential(nn.Conv2d(64, 128, 3, stride=2, padding=1), nn.InstanceNorm2d(128), nn.ReLU(inplace=True),
                                    nn.Conv2d(128, 256, 3, stride=2, padding=1), nn.InstanceNorm2d(256), nn.ReLU(inplace=True))
        self.model2 = nn.Sequential(*[ResidualBlock(256) for _ in range(n_residual_blocks)])
        self.model3 = nn.Sequential(nn.ConvTranspose2d(256, 128, 3, stride=2, padding=1, output_padding=1), nn.InstanceNorm2d(128), nn.ReLU(inplace=True),
                                    nn.ConvTranspose2d(128, 64, 3, stride=2, padding=1, output_padding=1), nn.InstanceNorm2d(64), nn.ReLU(inplace=True))
        model4 = [nn.ReflectionPad2d(3), nn.Conv2d(64, output_nc, 7)]
        if sigmoid:
            model4.append(nn.Sigmoid())
        self.model4 = nn.Sequential(*model4)

    def features(self, x):
        """The 64 channels the last convolution reads."""
        return self.model3(self.model2(self.model1(self.model0(x))))

    def logits(self, x):
        """The output before the sigmoid."""
        out = self.features(x)
        return self.model4[1](self.model4[0](out))

    def forward(self, x):
        return self.model4(self.features(x))


def lineart_state_dict(seed: int = 0, out_scale: float = 1.0) -> dict:
    """Seeded weights: He-normal convolutions (fan-in of the convolution; of the equivalent convolution for the transposed ones) with
    small asymmetric biases; model4.1.weight scaled by out_scale (the logits' spread)."""
    g = torch.Generator().manual_seed(seed)
    net = Generator()
    sd = {}
    for k, v in net.state_dict().items():
        if k.endswith(".weight"):
            fan_in = (v.shape[0] if k.startswith("model3.") else v.shape[1]) * v.shape[2] * v.shape[3]
            if k.startswith("model3."):
                fan_in //= 4  # a stride-2 transposed convolution: an output pixel sees 9 / 4 taps on average
            w = torch.randn(v.shape, generator=g) * math.sqrt(2.0 / fan_in)
            sd[k] = w * out_scale if k == "model4.1.weight" else w
        else:
            n = v.shape[0]
            sd[k] = (torch.arange(n, dtype=torch.float32) / max(n - 1, 1) - 0.4) * 0.1 + torch.randn(n, generator=g) * 0.02
    return sd


def lineart_net(sd: dict) -> Generator:
    net = Generator()
    net.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return net.eval()


def to_input(frames: np.ndarray) -> torch.Tensor:
    """uint8 [n, H, W, 3] -> float32 [n, 3, H, W] = uint8 / 255.0."""
    a = np.ascontiguousarray(frames).astype(np.float32) / 255.0
    return torch.from_numpy(a).permute(0, 3, 1, 2).contiguous()


def logits_ref(sd: dict, frames: np.ndarray) -> torch.Tensor:
    """uint8 RGB [n, H, W, 3] -> float32 logits [n, H, W] (the fp32 net on the CPU)."""
    with torch.no_grad():
        return lineart_net(sd).logits(to_input(frames))[:, 0].contiguous()


def finish_ref(logits: np.ndarray):
    """float32 logits -> (the uint8 map 255 - uint8(clip(sigmoid * 255.0, 0, 255)), the float64 value sigmoid * 255 before clip and
    truncation).  The detector's own arithmetic is float32 (torch's sigmoid, numpy's float32 * 255.0): the map is computed so."""
    lg = np.asarray(logits, dtype=np.float32)
    line = torch.sigmoid(torch.from_numpy(lg)).numpy()
    level = (line * 255.0).clip(0, 255).astype(np.uint8)
    scaled = (1.0 / (1.0 + np.exp(-lg.astype(np.float64)))) * 255.0
    return (255 - level).astype(np.uint8), scaled


def lineart_detect(sd: dict, image: np.ndarray) -> np.ndarray:
    """LineartDetector.__call__(image, detect_resolution=min(H, W), image_resolution=min(H, W)) for a uint8 [H, W] or [H, W, 3] array
    with H % 64 == W % 64 == 0 -> uint8 [H, W, 3] with three equal channels."""
    img = np.asarray(image)
    assert img.dtype == np.uint8
    if img.ndim == 2:
        img = np.repeat(img[:, :, None], 3, axis=2)
    assert img.ndim == 3 and img.shape[2] == 3
    if img.shape[0] % 64 or img.shape[1] % 64:
        raise NotImplementedError(f"{img.shape[:2]}: the detector's resamplings are restated only where they are the identity")
    with torch.no_grad():
        line = lineart_net(sd)(to_input(img[None]))[0][0].numpy()
    level = (line * 255.0).clip(0, 255).astype(np.uint8)
    return np.repeat((255 - level)[:, :, None], 3, axis=2)


def frames_fixture():
    """Two 64 x 128 RGB frames with smooth, periodic and blocky content plus noise."""
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:64, 0:128]
    out = []
    for i in range(2):
        a = np.zeros((64, 128, 3), np.float64)
        a[..., 0] = 128 + 100 * np.sin(xx / (5.0 + i)) * np.cos(yy / 7.0)
        a[..., 1] = (xx * 2 + yy * (3 + i)) % 256
        a[..., 2] = 255 * ((xx // 16 + yy // 16 + i) % 2)
        a += rng.normal(0, 12, a.shape)
        out.append(a.clip(0, 255).astype(np.uint8))
    return np.stack(out)


_frames = frames_fixture
