"""The specification of the NormalBae annotator: the NNET surface-normal network (an EfficientNet encoder in geffnet's naming, the
decoder with its three per-pixel refinement stages) as fp32 torch modules, and the detector's pre- and post-processing in numpy.

Restated from memory of controlnet_aux 0.0.6 (NormalBaeDetector) and of the NNET code it vendors; neither package nor a scannet.pt is
available here, so the topology, the key names and parity with them are UNPINNED.  What IS pinned: the encoder's arithmetic, against
transformers' EfficientNetModel through tests/golden/normalbae_tiny.npz (tests/golden/make_normalbae_golden.py; the mapping of
transformers' key names to geffnet's lives there and in the tests).

The geometry is a parameter: B5 is tf_efficientnet_b5_ap as the detector builds it, TINY serves the tests.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
ENCODER_BN_EPS = 1e-3
MIN_KAPPA = 0.01
TAP_STAGES = (0, 1, 2, 4)      # features[4], [5], [6], [8] of the module-by-module list; features[11] is conv_head's output
HEAD_BIAS = (0.5, -0.4, 0.8, 0.2)   # seeded_state_dict: the bias of every head's last layer (see its docstring)


class Geometry(NamedTuple):
    stem: int
    stages: tuple      # per stage (width, repeats, kernel, stride, expansion)
    head: int          # conv_head's width
    decoder: int       # conv2's width; up1 .. up4 give decoder / 2, / 4, / 8, / 16
    hidden: int = 128  # the width of the refinement MLPs


B5 = Geometry(48, ((24, 3, 3, 1, 1), (40, 5, 3, 2, 6), (64, 5, 5, 2, 6), (128, 7, 3, 2, 6), (176, 7, 5, 1, 6), (304, 9, 5, 2, 6), (512, 3, 3, 1, 6)), 2048, 2048)
# transformers' EfficientNetConfig(width_coefficient=0.5, depth_coefficient=0.35): 10 blocks, both kernel sizes, both strides, a repeated block
TINY = Geometry(16, ((8, 1, 3, 1, 1), (16, 1, 3, 2, 6), (24, 1, 5, 2, 6), (40, 2, 3, 2, 6), (56, 2, 5, 1, 6), (96, 2, 5, 2, 6), (160, 1, 3, 1, 6)), 640, 256)


def blocks_of(geo: Geometry):
    """[(stage, index in stage, cin, cout, kernel, stride, expansion, se width)] of every block: the squeeze width is a quarter of the
    block's INPUT channels."""
    out, cin = [], geo.stem
    for s, (width, repeats, kernel, stride, expand) in enumerate(geo.stages):
        for b in range(repeats):
            out.append((s, b, cin, width, kernel, stride if b == 0 else 1, expand, max(1, cin // 4)))
            cin = width
    return out


def swish(x):
    return x * torch.sigmoid(x)


def same_pad(size: int, k: int, s: int):
    """TensorFlow SAME: (before, after)."""
    total = max((-(-size // s) - 1) * s + k - size, 0)
    return total // 2, total - total // 2


class Conv2dSame(nn.Conv2d):
    def forward(self, x):
        k, s = self.kernel_size[0], self.stride[0]
        (t, b), (l, r) = same_pad(x.shape[2], k, s), same_pad(x.shape[3], k, s)
        return F.conv2d(F.pad(x, (l, r, t, b)), self.weight, self.bias, self.stride, 0, 1, self.groups)


class SqueezeExcite(nn.Module):
    def __init__(self, c, r):
        super().__init__()
        self.conv_reduce = nn.Conv2d(c, r, 1)
        self.conv_expand = nn.Conv2d(r, c, 1)

    def forward(self, x):
        return x * torch.sigmoid(self.conv_expand(swish(self.conv_reduce(x.mean((2, 3), keepdim=True)))))


def _bn(c):
    return nn.BatchNorm2d(c, eps=ENCODER_BN_EPS)


class DepthwiseSeparable(nn.Module):   # expansion 1
    def __init__(self, cin, cout, k, stride, r):
        super().__init__()
        self.skip = stride == 1 and cin == cout
        self.conv_dw, self.bn1 = Conv2dSame(cin, cin, k, stride, groups=cin, bias=False), _bn(cin)
        self.se = SqueezeExcite(cin, r)
        self.conv_pw, self.bn2 = nn.Conv2d(cin, cout, 1, bias=False), _bn(cout)

    def forward(self, x):
        y = self.bn2(self.conv_pw(self.se(swish(self.bn1(self.conv_dw(x))))))
        return y + x if self.skip else y


class InvertedResidual(nn.Module):
    def __init__(self, cin, cout, k, stride, expand, r):
        super().__init__()
        mid = cin * expand
        self.skip = stride == 1 and cin == cout
        self.conv_pw, self.bn1 = nn.Conv2d(cin, mid, 1, bias=False), _bn(mid)
        self.conv_dw, self.bn2 = Conv2dSame(mid, mid, k, stride, groups=mid, bias=False), _bn(mid)
        self.se = SqueezeExcite(mid, r)
        self.conv_pwl, self.bn3 = nn.Conv2d(mid, cout, 1, bias=False), _bn(cout)

    def forward(self, x):
        y = swish(self.bn1(self.conv_pw(x)))
        y = self.se(swish(self.bn2(self.conv_dw(y))))
        y = self.bn3(self.conv_pwl(y))
        return y + x if self.skip else y


class EfficientNet(nn.Module):
    """geffnet's GenEfficientNet without the pool and the classifier (`encoder.original_model`)."""

    def __init__(self, geo: Geometry):
        super().__init__()
        self.conv_stem, self.bn1 = Conv2dSame(3, geo.stem, 3, 2, bias=False), _bn(geo.stem)
        stages = [[] for _ in geo.stages]
        for s, _, cin, cout, k, stride, expand, r in blocks_of(geo):
            stages[s].append(DepthwiseSeparable(cin, cout, k, stride, r) if expand == 1 else InvertedResidual(cin, cout, k, stride, expand, r))
        self.blocks = nn.Sequential(*[nn.Sequential(*st) for st in stages])
        self.conv_head = nn.Conv2d(geo.stages[-1][0], geo.head, 1, bias=False)


class Encoder(nn.Module):
    def __init__(self, geo: Geometry):
        super().__init__()
        self.original_model = EfficientNet(geo)

    def forward(self, x):
        """The module-by-module feature list: [x, conv_stem, bn1, act1, blocks.0 .. blocks.6, conv_head] (the detector's encoder goes on
        through bn2 and act2, which the decoder never reads)."""
        m = self.original_model
        feats = [x]
        feats.append(m.conv_stem(feats[-1]))
        feats.append(m.bn1(feats[-1]))
        feats.append(swish(feats[-1]))
        for stage in m.blocks:
            feats.append(stage(feats[-1]))
        feats.append(m.conv_head(feats[-1]))
        return feats


class UpSampleBN(nn.Module):
    def __init__(self, skip_input, output_features):
        super().__init__()
        self._net = nn.Sequential(nn.Conv2d(skip_input, output_features, 3, 1, 1), nn.BatchNorm2d(output_features), nn.LeakyReLU(),
                                  nn.Conv2d(output_features, output_features, 3, 1, 1), nn.BatchNorm2d(output_features), nn.LeakyReLU())

    def forward(self, x, concat_with):
        up = F.interpolate(x, size=concat_with.shape[2:], mode="bilinear", align_corners=True)
        return self._net(torch.cat([up, concat_with], 1))


def norm_normalize(out):
    x, y, z, k = torch.split(out, 1, dim=1)
    norm = torch.sqrt(x ** 2.0 + y ** 2.0 + z ** 2.0) + 1e-10
    return torch.cat([x / norm, y / norm, z / norm, F.elu(k) + 1.0 + MIN_KAPPA], 1)


def _mlp(cin, hidden):
    return nn.Sequential(nn.Conv1d(cin, hidden, 1), nn.ReLU(), nn.Conv1d(hidden, hidden, 1), nn.ReLU(), nn.Conv1d(hidden, hidden, 1), nn.ReLU(),
                         nn.Conv1d(hidden, 4, 1))


def refine_stage(mlp, feat, pred, raw_out=None):
    """One refinement stage: feat [B, C, h, w] and pred [B, 4, h, w] x2 (bilinear, align_corners), concatenated, through the per-pixel MLP,
    normalised -> [B, 4, 2h, 2w].  raw_out: a list that receives the MLP's output before the normalisation."""
    f = F.interpolate(feat, scale_factor=2, mode="bilinear", align_corners=True)
    p = F.interpolate(pred, scale_factor=2, mode="bilinear", align_corners=True)
    x = torch.cat([f, p], 1)
    b, c, h, w = x.shape
    raw = mlp(x.view(b, c, -1)).view(b, 4, h, w)
    if raw_out is not None:
        raw_out.append(raw)
    return norm_normalize(raw)


class Decoder(nn.Module):
    def __init__(self, geo: Geometry):
        super().__init__()
        d = geo.decoder
        taps = [geo.stages[s][0] for s in TAP_STAGES]
        self.conv2 = nn.Conv2d(geo.head, d, 1)
        self.up1 = UpSampleBN(d + taps[3], d // 2)
        self.up2 = UpSampleBN(d // 2 + taps[2], d // 4)
        self.up3 = UpSampleBN(d // 4 + taps[1], d // 8)
        self.up4 = UpSampleBN(d // 8 + taps[0], d // 16)
        self.out_conv_res8 = nn.Conv2d(d // 4, 4, 3, 1, 1)
        self.out_conv_res4 = _mlp(d // 4 + 4, geo.hidden)
        self.out_conv_res2 = _mlp(d // 8 + 4, geo.hidden)
        self.out_conv_res1 = _mlp(d // 16 + 4, geo.hidden)

    def forward(self, feats, raws=None):
        """-> [res8, res4, res2, res1] (the test-time path: every pixel is refined).  raws: a list that receives the four pre-normalisation
        outputs."""
        b0, b1, b2, b3, b4 = feats[4], feats[5], feats[6], feats[8], feats[11]
        x_d0 = self.conv2(b4)
        x_d1 = self.up1(x_d0, b3)
        x_d2 = self.up2(x_d1, b2)
        x_d3 = self.up3(x_d2, b1)
        x_d4 = self.up4(x_d3, b0)
        raw8 = self.out_conv_res8(x_d2)
        if raws is not None:
            raws.append(raw8)
        res8 = norm_normalize(raw8)
        res4 = refine_stage(self.out_conv_res4, x_d2, res8, raws)
        res2 = refine_stage(self.out_conv_res2, x_d3, res4, raws)
        res1 = refine_stage(self.out_conv_res1, x_d4, res2, raws)
        return [res8, res4, res2, res1]


class NNET(nn.Module):
    def __init__(self, geo: Geometry = B5):
        super().__init__()
        self.geometry = geo
        self.encoder, self.decoder = Encoder(geo), Decoder(geo)

    def forward(self, img, raws=None):
        return self.decoder(self.encoder(img), raws)


def key_shapes(geo: Geometry = B5) -> dict:
    """Every tensor of the checkpoint's "model" entry that the detector runs: name -> shape (num_batches_tracked left out)."""
    return {k: tuple(v.shape) for k, v in NNET(geo).state_dict().items() if not k.endswith("num_batches_tracked")}


def seeded_state_dict(geo: Geometry = B5, seed: int = 0) -> dict:
    """A state dict whose weights keep activations O(1): convolutions N(0, gain / fan_in) (gain 2 in front of swish / ReLU / LeakyReLU, 1
    elsewhere), BatchNorm tensors real with non-trivial running statistics, nothing folded.  The last layer of every head (out_conv_res8,
    out_conv_resN.6) has small weights and the fixed bias HEAD_BIAS, so that the norm of xyz in front of each of the four normalisations
    stays away from zero (tests/test_normalbae_cpu.py asserts it for the seeds the GPU tests use)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in key_shapes(geo).items():
        leaf = k.rsplit(".", 1)[1]
        is_bn = len(shape) == 1 and (k.rsplit(".", 1)[0] + ".running_var") in key_shapes_cache(geo)
        if is_bn:
            if leaf == "weight":
                t = 0.8 + 0.4 * torch.rand(shape, generator=g)
            elif leaf == "running_var":
                t = 0.6 + 0.8 * torch.rand(shape, generator=g)
            else:   # bias, running_mean
                t = 0.2 * torch.randn(shape, generator=g)
        elif leaf == "bias":
            t = 0.1 * torch.randn(shape, generator=g)
        else:
            fan_in = int(np.prod(shape[1:]))
            last = k.startswith("decoder.out_conv_res8") or k.endswith(".6.weight")
            linear = "conv_pwl" in k or "se.conv_expand" in k or k.startswith("encoder.original_model.blocks.0.") and "conv_pw." in k or k == "decoder.conv2.weight"
            gain = 0.25 if last else (1.0 if linear else 2.0)
            t = torch.randn(shape, generator=g) * (gain / fan_in) ** 0.5
        sd[k] = t
    for k in sd:
        if k == "decoder.out_conv_res8.bias" or (k.startswith("decoder.out_conv_res") and k.endswith(".6.bias")):
            sd[k] = torch.tensor(HEAD_BIAS)
    return sd


_KEY_SHAPES = {}


def key_shapes_cache(geo: Geometry) -> dict:
    if geo not in _KEY_SHAPES:
        _KEY_SHAPES[geo] = key_shapes(geo)
    return _KEY_SHAPES[geo]


def load(geo: Geometry, sd: dict) -> NNET:
    net = NNET(geo).eval()
    net.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return net


# ---- the detector around the network ----------------------------------------------------------------------------------------------------
def preprocess(frames: np.ndarray) -> torch.Tensor:
    """uint8 [n, H, W, 3] -> float32 [n, 3, H, W]: / 255, then the ImageNet normalisation (torchvision's Normalize: subtract, divide)."""
    x = torch.from_numpy(np.ascontiguousarray(frames)).float().permute(0, 3, 1, 2) / 255.0
    mean = torch.tensor(IMAGENET_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD).view(1, 3, 1, 1)
    return (x - mean) / std


def tail(normal: torch.Tensor) -> np.ndarray:
    """The last prediction's xyz, float32 [n, 3, H, W] -> the detector's uint8 map [n, H, W, 3]: truncation, not rounding."""
    normal = ((normal + 1) * 0.5).clip(0, 1)
    normal = normal.permute(0, 2, 3, 1).cpu().numpy()
    return (normal * 255.0).clip(0, 255).astype(np.uint8)


def detect(net: NNET, frames: np.ndarray) -> np.ndarray:
    """NormalBaeDetector at detect_resolution = image_resolution = min(H, W) with sides that are multiples of 64 (no resampling)."""
    with torch.no_grad():
        pred = net(preprocess(frames))[-1]
    return tail(pred[:, :3].float())


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------
def load_fixture():
    """tests/golden/normalbae_tiny*.npz -> (frames uint8 [3, 64, 96, 3], [five recorded fp32 NCHW tensors], the encoder's state dict under
    geffnet's names in fp32 (fp16 values), the recorded versions).  The key mapping is tests/golden/make_normalbae_golden.hf_to_geffnet."""
    import importlib.util
    import os
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_normalbae_golden", os.path.join(golden, "make_normalbae_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    z = np.load(os.path.join(golden, "normalbae_tiny.npz"))
    sd = {}
    for i in (0, 1):
        w = np.load(os.path.join(golden, f"normalbae_tiny_w{i}.npz"))
        for k in w.files:
            sd[mk.hf_to_geffnet(k[2:])] = torch.from_numpy(w[k].astype(np.float32))
    return z["frames"], [torch.from_numpy(z[f"tap{i}"]) for i in range(5)], sd, [str(v) for v in z["versions"]]


def tiny_state_dict(seed: int = 0) -> dict:
    """The TINY network's state dict: the fixture's encoder (pinned to transformers) and a seeded decoder."""
    sd = seeded_state_dict(TINY, seed)
    enc = load_fixture()[2]
    assert set(enc) <= set(sd)
    sd.update(enc)
    return sd
