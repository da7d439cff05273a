"""Test helpers: the specification of the HED annotator (controlanimate_amd/hed.py), restated on the CPU.

  * `ControlNetHED`: the fp32 torch network, written from the published ControlNetHED_Apache2 (controlnet_aux, Apache-2.0): a
    learned per-channel `norm` subtracted from float RGB in 0..255, five blocks of 3x3 convolutions + ReLU (blocks 2..5 start with
    a 2x2 / stride-2 max pool), a 1x1 `projection` to one channel per block.  Its state dict has the 37 keys of ControlNetHED.pth.
  * `hed_detect`: HEDdetector.__call__(image, detect_resolution, image_resolution) in numpy: resize_image, the net, every side map
    resized to the input's size with cv2.resize(INTER_LINEAR) on float32, the float32 mean, the float64 sigmoid, x 255, clip,
    truncation to uint8, three equal channels, resize to resize_image(input, image_resolution)'s size.
  * `resize_linear_f32`: OpenCV's INTER_LINEAR for float32 data as OpenCV computes the coordinates and weights
    (f = (d + 0.5) * src / dst - 0.5, s = floor(f), f -= s; s < 0 -> s = 0, f = 0; s >= src - 1 -> s = src - 1, f = 0; weights 1 - f
    and f in float32; columns combined first, then rows; every product and every sum rounded to float32).

controlnet_aux and OpenCV are not installed here and no ControlNetHED.pth is available: none of this has a fixture produced by
those packages, it is UNPINNED against them.  The two `resize_image` resamplings of 8-bit images (INTER_LANCZOS4 / INTER_AREA on the
way in, INTER_LINEAR on the way out) are restated only where they are the identity, which is the scope of HedAnnotator.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

HED_BLOCKS = ((3, 64, 2), (64, 128, 2), (128, 256, 3), (256, 512, 3), (512, 512, 3))  # (in, out, layers) of block1 .. block5


def hed_key_shapes() -> dict:
    """The 37 tensors of ControlNetHED.pth: name -> shape."""
    out = {"norm": (1, 3, 1, 1)}
    for b, (cin, cout, layers) in enumerate(HED_BLOCKS, start=1):
        for i in range(layers):
            out[f"block{b}.convs.{i}.weight"] = (cout, cin if i == 0 else cout, 3, 3)
            out[f"block{b}.convs.{i}.bias"] = (cout,)
        out[f"block{b}.projection.weight"] = (1, cout, 1, 1)
        out[f"block{b}.projection.bias"] = (1,)
    return out


class DoubleConvBlock(torch.nn.Module):
    def __init__(self, input_channel: int, output_channel: int, layer_number: int):
        super().__init__()
        self.convs = torch.nn.Sequential()
        self.convs.append(torch.nn.Conv2d(input_channel, output_channel, kernel_size=(3, 3), stride=(1, 1), padding=1))
        for _ in range(1, layer_number):
            self.convs.append(torch.nn.Conv2d(output_channel, output_channel, kernel_size=(3, 3), stride=(1, 1), padding=1))
        self.projection = torch.nn.Conv2d(output_channel, 1, kernel_size=(1, 1), stride=(1, 1), padding=0)

    def forward(self, x, down_sampling: bool = False):
        h = x
        if down_sampling:
            h = F.max_pool2d(h, kernel_size=(2, 2), stride=(2, 2))
        for conv in self.convs:
            h = F.relu(conv(h))
        return h, self.projection(h)


class ControlNetHED(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.norm = torch.nn.Parameter(torch.zeros(size=(1, 3, 1, 1)))
        for b, (cin, cout, layers) in enumerate(HED_BLOCKS, start=1):
            setattr(self, f"block{b}", DoubleConvBlock(cin, cout, layers))

    def forward(self, x):
        """x: float RGB in 0..255, [n, 3, H, W] -> the five side maps [n, 1, H >> k, W >> k]."""
        h = x - self.norm
        sides = []
        for b in range(1, 6):
            h, p = getattr(self, f"block{b}")(h, down_sampling=b > 1)
            sides.append(p)
        return tuple(sides)


def hed_state_dict(seed: int = 0, proj_scale=(1.0, 1.0, 1.0, 1.0, 1.0)) -> dict:
    """Seeded weights: He-normal convolutions with small asymmetric biases, a `norm` near the usual RGB means with fractional parts
    (so that the subtraction rounds), projections N(0, 1 / C) x proj_scale[block] with a bias of their own."""
    g = torch.Generator().manual_seed(seed)
    sd = {"norm": torch.tensor([122.6789, 116.6688, 104.0069]).view(1, 3, 1, 1) + torch.randn(1, 3, 1, 1, generator=g)}
    for b, (cin, cout, layers) in enumerate(HED_BLOCKS, start=1):
        for i in range(layers):
            ci = cin if i == 0 else cout
            sd[f"block{b}.convs.{i}.weight"] = torch.randn(cout, ci, 3, 3, generator=g) * math.sqrt(2.0 / (ci * 9))
            sd[f"block{b}.convs.{i}.bias"] = (torch.arange(cout, dtype=torch.float32) / (cout - 1) - 0.4) * 0.1 + torch.randn(cout, generator=g) * 0.02
        sd[f"block{b}.projection.weight"] = torch.randn(1, cout, 1, 1, generator=g) * (proj_scale[b - 1] / math.sqrt(cout))
        sd[f"block{b}.projection.bias"] = torch.randn(1, generator=g) * 0.1
    return sd


def hed_net(sd: dict) -> ControlNetHED:
    net = ControlNetHED()
    net.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return net.eval()


def side_maps_ref(sd: dict, frames: np.ndarray):
    """uint8 RGB [n, H, W, 3] -> the five side maps as float32 tensors [n, H >> k, W >> k] (the fp32 net on the CPU)."""
    x = torch.from_numpy(np.ascontiguousarray(frames)).permute(0, 3, 1, 2).float()
    with torch.no_grad():
        return [s[:, 0].contiguous() for s in hed_net(sd)(x)]


# ---- cv2.resize(INTER_LINEAR) on float32 ------------------------------------------------------------------------------------------
def _linear_axis(src: int, dst: int):
    """-> (index of the first sample, index of the second, weight of the first, weight of the second) per destination index."""
    scale = src / dst
    s0 = np.zeros(dst, np.int64)
    w1 = np.zeros(dst, np.float32)
    for d in range(dst):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = math.floor(f)
        f = np.float32(f - np.float32(s))
        if s < 0:
            s, f = 0, np.float32(0)
        if s >= src - 1:
            s, f = src - 1, np.float32(0)
        s0[d], w1[d] = s, f
    s1 = np.minimum(s0 + 1, src - 1)
    return s0, s1, (np.float32(1) - w1).astype(np.float32), w1


def resize_linear_f32(src: np.ndarray, dh: int, dw: int) -> np.ndarray:
    """cv2.resize(src, (dw, dh), interpolation=cv2.INTER_LINEAR) for a float32 [h, w] map."""
    a = np.asarray(src, dtype=np.float32)
    assert a.ndim == 2
    xa, xb, wx0, wx1 = _linear_axis(a.shape[1], dw)
    ya, yb, wy0, wy1 = _linear_axis(a.shape[0], dh)
    rows = (a[:, xa] * wx0[None, :]).astype(np.float32) + (a[:, xb] * wx1[None, :]).astype(np.float32)   # columns first
    rows = rows.astype(np.float32)
    out = (rows[ya] * wy0[:, None]).astype(np.float32) + (rows[yb] * wy1[:, None]).astype(np.float32)  # then rows
    return out.astype(np.float32)


def fuse_ref(sides, h: int, w: int):
    """The five side maps of ONE frame (float32 [h >> k, w >> k]) -> (uint8 edge map [h, w], the float32 mean logit, the float64
    value edge * 255 before clip and truncation)."""
    acc = resize_linear_f32(sides[0], h, w)
    for s in sides[1:]:
        acc = (acc + resize_linear_f32(s, h, w)).astype(np.float32)
    mean = (acc / np.float32(5)).astype(np.float32)
    edge = 1.0 / (1.0 + np.exp(-mean.astype(np.float64)))
    scaled = edge * 255.0
    return scaled.clip(0, 255).astype(np.uint8), mean, scaled


# ---- HEDdetector -----------------------------------------------------------------------------------------------------------------
def resize_image_size(h: int, w: int, resolution: int):
    """resize_image's target size and interpolation for an h x w image: k = resolution / min(h, w), both sides round(side * k / 64) * 64,
    LANCZOS4 when k > 1, else AREA."""
    k = float(resolution) / min(h, w)
    return int(np.round(h * k / 64.0)) * 64, int(np.round(w * k / 64.0)) * 64, ("lanczos4" if k > 1 else "area")


def _resize_u8_identity(img: np.ndarray, h: int, w: int, what: str) -> np.ndarray:
    if img.shape[:2] != (h, w):
        raise NotImplementedError(f"{what}: {img.shape[:2]} -> {(h, w)} is a resampling of an 8-bit image, which is not restated here (identity only)")
    return img


def hed_detect(sd: dict, image: np.ndarray, detect_resolution: int = 512, image_resolution: int = 512) -> np.ndarray:
    """HEDdetector.__call__ for a uint8 RGB [H, W, 3] array -> uint8 [H', W', 3] with three equal channels."""
    img = np.asarray(image)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    dh, dw, _ = resize_image_size(img.shape[0], img.shape[1], detect_resolution)
    x = _resize_u8_identity(img, dh, dw, "resize_image(input, detect_resolution)")
    sides = side_maps_ref(sd, x[None])
    edge, _, _ = fuse_ref([s[0].numpy() for s in sides], dh, dw)
    rgb = np.repeat(edge[:, :, None], 3, axis=2)
    oh, ow, _ = resize_image_size(img.shape[0], img.shape[1], image_resolution)
    return _resize_u8_identity(rgb, oh, ow, "the final INTER_LINEAR resize")
