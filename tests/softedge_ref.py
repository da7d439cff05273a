"""The specification of the softedge annotator (controlanimate_amd/softedge.py): controlnet_aux's PidiNetDetector as the reference
calls it (modules/controlresiduals_pipeline.py:62, 134-138: detect_resolution = image_resolution = min(h, w), safe = False), restated
from memory of the published code (pidinet/model.py: PiDiNet(60, carv4, dil = 24, sa = True), unconverted; pidinet/__init__.py) --
UNPINNED: controlnet_aux and OpenCV are absent here and no table5_pidinet.pth is available.

    network   init_block (a `cd` pixel-difference convolution 3 -> 60), fifteen PDCBlocks; the operator types are (cd, ad, rd, cv) x 4
              -- block1_1..3 at 60 channels, block2_1..4 at 120, block3_1..4 and block4_1..4 at 240, the first block of levels 2 .. 4
              behind MaxPool2d(2, 2) with a biased 1x1 shortcut --, per level a CDCM, a CSAM and a 1x1 reduction to one channel, the
              four maps resized bilinearly (align_corners = False) to the frame, a 1x1 classifier over their concatenation, a sigmoid
    detector  RGB uint8 -> BGR / 255 -> network -> edge (fp32) -> [safe: trunc(edge * 3) / 2] -> (edge * 255).clip(0, 255).astype(uint8)

The difference operators are evaluated here at RUN time, the way the published functions do (softedge.fold_pdc folds them; the CPU
tests compare the two).  The network is written functionally over a state dict and reads every width from the tensors' shapes, so the
zero-padded dict of softedge.pad_state_dict runs through the same code.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

LAYER_TYPES = ("cd", "ad", "rd", "cv") * 4           # carv4: layer 0 is init_block, layers 1 .. 15 the blocks in order
BLOCKS = [(f"block{lv}_{j}", LAYER_TYPES[i + 1]) for i, (lv, j) in enumerate([(1, 1), (1, 2), (1, 3)] + [(lv, j) for lv in (2, 3, 4) for j in (1, 2, 3, 4)])]
AD_PERM = [3, 0, 1, 6, 4, 2, 7, 8, 5]
RD_PLUS = [0, 2, 4, 10, 14, 20, 22, 24]
RD_MINUS = [6, 7, 8, 11, 13, 16, 17, 18]


# ---- the three pixel-difference operators, as the published createConvFunc builds them ---------------------------------------------------
def pdc_conv(x: torch.Tensor, w: torch.Tensor, kind: str, groups: int = 1) -> torch.Tensor:
    if kind == "cv":
        return F.conv2d(x, w, padding=1, groups=groups)
    if kind == "cd":
        wc = w.sum(dim=[2, 3], keepdim=True)
        return F.conv2d(x, w, padding=1, groups=groups) - F.conv2d(x, wc, padding=0, groups=groups)
    if kind == "ad":
        shape = w.shape
        flat = w.view(shape[0], shape[1], -1)
        return F.conv2d(x, (flat - flat[:, :, AD_PERM]).view(shape), padding=1, groups=groups)
    if kind == "rd":
        shape = w.shape
        buf = torch.zeros(shape[0], shape[1], 25, dtype=w.dtype)
        flat = w.view(shape[0], shape[1], -1)
        buf[:, :, RD_PLUS] = flat[:, :, 1:]
        buf[:, :, RD_MINUS] = -flat[:, :, 1:]
        buf[:, :, 12] = 0
        return F.conv2d(x, buf.view(shape[0], shape[1], 5, 5), padding=2, groups=groups)
    raise ValueError(kind)


def pdc_block(sd: dict, name: str, kind: str, x: torch.Tensor) -> torch.Tensor:
    strided = f"{name}.shortcut.weight" in sd
    if strided:
        x = F.max_pool2d(x, 2, 2)
    y = pdc_conv(x, sd[f"{name}.conv1.weight"], kind, groups=x.shape[1])
    y = F.conv2d(F.relu(y), sd[f"{name}.conv2.weight"])
    if strided:
        x = F.conv2d(x, sd[f"{name}.shortcut.weight"], sd[f"{name}.shortcut.bias"])
    return y + x


def cdcm(sd: dict, i: int, x: torch.Tensor) -> torch.Tensor:
    p = f"dilations.{i}"
    x = F.conv2d(F.relu(x), sd[f"{p}.conv1.weight"], sd[f"{p}.conv1.bias"])
    x1, x2, x3, x4 = (F.conv2d(x, sd[f"{p}.conv2_{k + 1}.weight"], padding=d, dilation=d) for k, d in enumerate((5, 7, 9, 11)))
    return x1 + x2 + x3 + x4


def csam(sd: dict, i: int, x: torch.Tensor) -> torch.Tensor:
    p = f"attentions.{i}"
    y = F.conv2d(F.relu(x), sd[f"{p}.conv1.weight"], sd[f"{p}.conv1.bias"])
    y = torch.sigmoid(F.conv2d(y, sd[f"{p}.conv2.weight"], padding=1))
    return x * y


def side_map(sd: dict, i: int, f: torch.Tensor) -> torch.Tensor:
    """CSAM, then the 1x1 reduction: [n, 1, h, w] at the level's own resolution."""
    return F.conv2d(csam(sd, i, f), sd[f"conv_reduces.{i}.conv.weight"], sd[f"conv_reduces.{i}.conv.bias"])


def fuse_ref(sides, classifier_w: torch.Tensor, classifier_b: torch.Tensor, size) -> torch.Tensor:
    """The four side maps [n, 1, h >> k, w >> k] -> the fused logit [n, h, w]."""
    up = [F.interpolate(s, size, mode="bilinear", align_corners=False) for s in sides]
    return F.conv2d(torch.cat(up, dim=1), classifier_w, classifier_b)[:, 0]


def network_ref(sd: dict, x: torch.Tensor) -> dict:
    """x [n, 3 (or the padded 8), H, W] in the state dict's dtype -> {"features": the four block outputs, "cdcm": the four CDCM outputs,
    "sides": the four side maps [n, h_k, w_k] at their own resolution, "logit": the fused logit [n, H, W]}."""
    with torch.no_grad():
        h, w = x.shape[2:]
        x = pdc_conv(x, sd["init_block.weight"], "cd")
        feats = []
        for name, kind in BLOCKS:
            if name.endswith("_1") and name != "block1_1":
                feats.append(x)
            x = pdc_block(sd, name, kind, x)
        feats.append(x)
        cd = [cdcm(sd, i, f) for i, f in enumerate(feats)]
        sides = [side_map(sd, i, f) for i, f in enumerate(cd)]
        logit = fuse_ref(sides, sd["classifier.weight"], sd["classifier.bias"], (h, w))
        return {"features": feats, "cdcm": cd, "sides": [s[:, 0] for s in sides], "logit": logit}


def to_input(frames: np.ndarray) -> torch.Tensor:
    """uint8 RGB [n, H, W, 3] -> float32 BGR / 255 [n, 3, H, W]."""
    return torch.from_numpy(np.ascontiguousarray(frames[..., ::-1]).astype(np.float32) / 255.0).permute(0, 3, 1, 2).contiguous()


def logits_ref(sd: dict, frames: np.ndarray) -> torch.Tensor:
    return network_ref({k: v.float() for k, v in sd.items()}, to_input(frames))["logit"]


# ---- the detector's tail ---------------------------------------------------------------------------------------------------------------
def tail_ref(logit, safe: bool = False) -> np.ndarray:
    """fused logit float32 [..] -> the detector's uint8 map."""
    edge = torch.sigmoid(torch.as_tensor(np.ascontiguousarray(logit), dtype=torch.float32)).numpy()
    if safe:
        edge = (edge * np.float32(3.0)).astype(np.int32).astype(np.float32) / np.float32(2.0)
    return (edge * np.float32(255.0)).clip(0, 255).astype(np.uint8)


def decided(z, safe: bool = False) -> np.ndarray:
    """The pixels whose byte does not hang on the last bits of the fp32 arithmetic: 255 * sigmoid(z) lies farther than 1e-3 from an
    integer (with safe: 3 * sigmoid(z) farther than 1e-5 from an integer -- the steps of trunc(edge * 3))."""
    s = 1.0 / (1.0 + np.exp(-np.asarray(z, dtype=np.float64)))
    v, tol = (3.0 * s, 1e-5) if safe else (255.0 * s, 1e-3)
    return np.abs(v - np.round(v)) > tol


def detect_ref(sd: dict, image: np.ndarray, safe: bool = False) -> np.ndarray:
    """One RGB (or grey) uint8 frame -> [H, W, 3] uint8, three equal channels."""
    if image.ndim == 2:
        image = image[:, :, None]
    if image.shape[2] == 1:
        image = np.repeat(image, 3, axis=2)
    m = tail_ref(logits_ref(sd, image[None])[0].numpy(), safe)
    return np.repeat(m[:, :, None], 3, axis=2)


# ---- seeded weights -----------------------------------------------------------------------------------------------------------------------
# Fifteen residual blocks without normalisation: the branch W2 . relu(dw(x)) must stay a fraction of x.  A folded difference kernel
# built from taps of standard deviation s has energy 16 s^2 (cd, ad, rd; 9 s^2 for cv), so DW = 0.25 keeps a white input's variance;
# PW / sqrt(cin) with PW = 0.5 behind the ReLU gives a branch of about a quarter of x's variance or less per block.  The init_block sees
# differences of an image in [0, 1]: INIT lifts them to O(1).  The shortcut is variance-preserving; the CDCM / CSAM / reduction scales
# are He-style (the reduction three times that); the classifier mixes the four side maps with weights near CLS = 2, which puts the fused
# logit's standard deviation on the fixture at about 2 (2.06 at seed 0).
SCALES = {"init": 6.0, "dw": 0.25, "pw": 0.5, "shortcut": 1.0, "bias": 0.1, "cdcm1": 1.4, "cdcm2": 1.0, "csam1": 1.4, "csam2": 0.5, "reduce": 3.0, "cls": 2.0}
WIDTHS = (60, 120, 240, 240)


def softedge_state_dict(seed: int = 0, scales: dict | None = None) -> dict:
    sc = dict(SCALES, **(scales or {}))
    g = torch.Generator().manual_seed(seed)

    def rn(*shape, std=1.0):
        return torch.randn(*shape, generator=g) * std

    sd = {"init_block.weight": rn(60, 3, 3, 3, std=sc["init"] / 27 ** 0.5)}
    cin = 60
    for name, _ in BLOCKS:
        lv, j = int(name[5]), int(name[7])
        cout = WIDTHS[lv - 1]
        strided = j == 1 and lv > 1
        sd[f"{name}.conv1.weight"] = rn(cin, 1, 3, 3, std=sc["dw"])
        sd[f"{name}.conv2.weight"] = rn(cout, cin, 1, 1, std=sc["pw"] / cin ** 0.5)
        if strided:
            sd[f"{name}.shortcut.weight"] = rn(cout, cin, 1, 1, std=sc["shortcut"] / cin ** 0.5)
            sd[f"{name}.shortcut.bias"] = rn(cout, std=sc["bias"])
        cin = cout
    for i, c in enumerate(WIDTHS):
        sd[f"dilations.{i}.conv1.weight"] = rn(24, c, 1, 1, std=sc["cdcm1"] / c ** 0.5)
        sd[f"dilations.{i}.conv1.bias"] = rn(24, std=sc["bias"])
        for k in range(4):
            sd[f"dilations.{i}.conv2_{k + 1}.weight"] = rn(24, 24, 3, 3, std=sc["cdcm2"] / (4 * 9 * 24) ** 0.5)
        sd[f"attentions.{i}.conv1.weight"] = rn(4, 24, 1, 1, std=sc["csam1"] / 24 ** 0.5)
        sd[f"attentions.{i}.conv1.bias"] = rn(4, std=sc["bias"])
        sd[f"attentions.{i}.conv2.weight"] = rn(1, 4, 3, 3, std=sc["csam2"] / 6.0)
        sd[f"conv_reduces.{i}.conv.weight"] = rn(1, 24, 1, 1, std=sc["reduce"] / 24 ** 0.5)
        sd[f"conv_reduces.{i}.conv.bias"] = rn(1, std=sc["bias"])
    sd["classifier.weight"] = sc["cls"] * (1.0 + 0.25 * rn(1, 4, 1, 1))
    sd["classifier.bias"] = rn(1, std=sc["bias"])
    return sd


def frames_fixture(h: int = 64, w: int = 128, n: int = 2, seed: int = 5) -> np.ndarray:
    """n RGB frames of h x w with smooth, periodic and blocky content plus noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for k in range(n):
        base = 127 + 80 * np.sin(xx / (5.0 + 3 * k)) * np.cos(yy / (7.0 - 2 * k))
        img = np.stack([base, 255 - base, 60 + 150.0 * xx / w], axis=2)
        img[h // 4 + 8 * k:5 * h // 8, w // 5:w // 2 + 16 * k] = (220, 40 + 100 * k, 90)
        img += rng.normal(0, 12, img.shape)
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return np.stack(out)


# ---- the device chain on the CPU, every stored activation rounded -------------------------------------------------------------------------------
def logits_emulated(sd: dict, frames: np.ndarray, dtype=torch.float16) -> dict:
    """The chain of SoftedgeAnnotator with torch fp32 arithmetic and every tensor the device stores in `dtype` (the weights as it packs
    them, the prepared frames, every block's depthwise result and output, the CDCM's two tensors) rounded to it; the CSAM, the side maps
    and the fuse stay fp32, as on the device.  -> {"sides": [n, h_k, w_k] x 4, "logit": [n, H, W]}."""
    from controlanimate_amd import softedge as S

    def r(t):
        return t.to(dtype).float()

    with torch.no_grad():
        lay = S.folded_layers(sd)
        x = r(torch.from_numpy(frames.astype(np.float32) / 255.0).permute(0, 3, 1, 2).contiguous())
        h, w = x.shape[2:]
        x = r(F.conv2d(x, r(lay["init"]), padding=1))                     # the weight's input channels already in RGB order
        feats = []
        for blk in lay["blocks"]:
            if "shortcut" in blk:
                feats.append(x)
                x = F.max_pool2d(x, 2, 2)
            k = blk["dw"].shape[-1]
            d = r(F.relu(F.conv2d(x, r(blk["dw"]), padding=k // 2, groups=x.shape[1])))
            y = F.conv2d(d, r(blk["pw"]))
            if "shortcut" in blk:
                x = r(y + F.conv2d(x, r(blk["shortcut"][0]), blk["shortcut"][1]))
            else:
                x = r(r(y) + x)                                           # ca_gemm's residual epilogue and ca_pdc_block round the product first
        feats.append(x)
        sides = []
        for lv, f in zip(lay["levels"], feats):
            t = r(F.conv2d(r(F.relu(f)), r(lv["cdcm1"][0]), lv["cdcm1"][1]))
            t = r(sum(F.conv2d(t, r(wd), padding=d, dilation=d) for wd, d in zip(lv["cdcm2"], (5, 7, 9, 11))))
            a = F.conv2d(F.relu(t), lv["csam1"][0], lv["csam1"][1])
            a = torch.sigmoid(F.conv2d(a, lv["csam2"], padding=1))
            sides.append(a * F.conv2d(t, lv["reduce"][0]) + lv["reduce"][1])
        logit = fuse_ref(sides, lay["classifier"][0], lay["classifier"][1], (h, w))
        return {"sides": [s[:, 0] for s in sides], "logit": logit}
