"""The specification of the M-LSD annotator (controlanimate_amd/mlsd.py): MobileV2_MLSD_Large as an fp32 torch network built from a state
dict, and the detector around it in numpy -- the input of four channels, the decode (deccode_output_score_and_ptss(tp, 200, 3) followed by
pred_lines) and cv2.line as OpenCV's clipLine + 8-connected LineIterator.  Restated from memory of the published code (controlnet_aux's
mlsd: models/mbv2_mlsd_large.py, utils.py; OpenCV's drawing.cpp): controlnet_aux and OpenCV are absent here and no checkpoint is available,
so key names and arithmetic are UNPINNED.  Scope: min(H, W) == detect_resolution == image_resolution, H % 64 == W % 64 == 0, where every
resampling of the detector is the identity.

torch.topk leaves the order among equal scores unspecified; the specification here is score descending, then flat index ascending.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

TOPK = 200


# ---- the network ---------------------------------------------------------------------------------------------------------------------
class ConvBNReLU(nn.Sequential):
    def __init__(self, cin, cout, kernel_size=3, stride=1, groups=1):
        self.stride = stride
        padding = 0 if stride == 2 else (kernel_size - 1) // 2
        super().__init__(nn.Conv2d(cin, cout, kernel_size, stride, padding, groups=groups, bias=False), nn.BatchNorm2d(cout), nn.ReLU6(inplace=True))

    def forward(self, x):
        if self.stride == 2:
            x = F.pad(x, (0, 1, 0, 1), "constant", 0)
        for m in self:
            x = m(x)
        return x


class InvertedResidual(nn.Module):
    def __init__(self, cin, cout, stride, t):
        super().__init__()
        hid = cin * t
        self.skip = stride == 1 and cin == cout
        layers = [ConvBNReLU(cin, hid, kernel_size=1)] if t != 1 else []
        layers += [ConvBNReLU(hid, hid, stride=stride, groups=hid), nn.Conv2d(hid, cout, 1, 1, 0, bias=False), nn.BatchNorm2d(cout)]
        self.conv = nn.Sequential(*layers)

    def forward(self, x):
        return x + self.conv(x) if self.skip else self.conv(x)


class Backbone(nn.Module):
    def __init__(self):
        super().__init__()
        feats, cin = [ConvBNReLU(4, 32, stride=2)], 32
        for t, c, n, s in ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1)):
            for i in range(n):
                feats.append(InvertedResidual(cin, c, s if i == 0 else 1, t))
                cin = c
        self.features = nn.Sequential(*feats)

    def forward(self, x):
        taps = []
        for i, f in enumerate(self.features):
            x = f(x)
            if i in (1, 3, 6, 10, 13):
                taps.append(x)
        return taps


def _cbr(cin, cout, k, **kw):
    return nn.Sequential(nn.Conv2d(cin, cout, k, **kw), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))


class BlockTypeA(nn.Module):
    def __init__(self, in_c1, in_c2, out_c1, out_c2, upscale=True):
        super().__init__()
        self.conv1, self.conv2, self.upscale = _cbr(in_c2, out_c2, 1), _cbr(in_c1, out_c1, 1), upscale

    def forward(self, a, b):
        b, a = self.conv1(b), self.conv2(a)
        if self.upscale:
            b = F.interpolate(b, scale_factor=2.0, mode="bilinear", align_corners=True)
        return torch.cat((a, b), dim=1)


class BlockTypeB(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv1, self.conv2 = _cbr(cin, cin, 3, padding=1), _cbr(cin, cout, 3, padding=1)

    def forward(self, x):
        return self.conv2(self.conv1(x) + x)


class BlockTypeC(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv1, self.conv2 = _cbr(cin, cin, 3, padding=5, dilation=5), _cbr(cin, cin, 3, padding=1)
        self.conv3 = nn.Conv2d(cin, cout, 1)

    def forward(self, x):
        return self.conv3(self.conv2(self.conv1(x)))


class MobileV2_MLSD_Large(nn.Module):
    def __init__(self):
        super().__init__()
        self.backbone = Backbone()
        self.block15, self.block16 = BlockTypeA(64, 96, 64, 64, upscale=False), BlockTypeB(128, 64)
        self.block17, self.block18 = BlockTypeA(32, 64, 64, 64), BlockTypeB(128, 64)
        self.block19, self.block20 = BlockTypeA(24, 64, 64, 64), BlockTypeB(128, 64)
        self.block21, self.block22 = BlockTypeA(16, 64, 64, 64), BlockTypeB(128, 64)
        self.block23 = BlockTypeC(64, 16)

    def forward(self, x):
        c1, c2, c3, c4, c5 = self.backbone(x)
        x = self.block16(self.block15(c4, c5))
        x = self.block18(self.block17(c3, x))
        x = self.block20(self.block19(c2, x))
        x = self.block22(self.block21(c1, x))
        return self.block23(x)[:, 7:, :, :]


def mlsd_state_dict(seed: int = 0, out_scale=None) -> dict:
    """Seeded weights: He-normal convolutions, BatchNorm with non-trivial statistics (gamma 0.7 .. 1.3, beta and running mean N(0, 0.1^2),
    running variance 0.5 .. 1.5); block23.conv3.weight scaled by out_scale (the spread of the centre logits and of the displacements).
    out_scale=None: the scale that gives the centre logits of frames_fixture() a standard deviation of 2 (the displacements are then a
    few pixels) -- the spread of the unscaled network varies with the seed."""
    g = torch.Generator().manual_seed(seed)
    net = MobileV2_MLSD_Large()
    sd = {}
    for k, v in net.state_dict().items():
        if k.endswith("num_batches_tracked"):
            continue
        if v.dim() == 4:
            fan_in = v.shape[1] * v.shape[2] * v.shape[3]
            sd[k] = torch.randn(v.shape, generator=g) * (2.0 / fan_in) ** 0.5
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
        elif k.endswith("running_mean"):
            sd[k] = torch.randn(v.shape, generator=g) * 0.1
        elif k.endswith(".weight"):   # BatchNorm gamma
            sd[k] = 0.7 + 0.6 * torch.rand(v.shape, generator=g)
        else:                         # BatchNorm beta, convolution bias
            sd[k] = torch.randn(v.shape, generator=g) * 0.1
    if out_scale is None:
        out_scale = 2.0 / float(tpmap_ref(sd, frames_fixture())[..., 0].std())
    sd["block23.conv3.weight"] = sd["block23.conv3.weight"] * out_scale
    return sd


def mlsd_net(sd: dict) -> MobileV2_MLSD_Large:
    net = MobileV2_MLSD_Large()
    net.load_state_dict({k: v.float() for k, v in sd.items()}, strict=False)
    return net.eval()


def to_input(frames: np.ndarray) -> torch.Tensor:
    """uint8 [n, H, W, 3] -> float32 [n, 4, H, W]: RGB and a channel of ones, x / 127.5 - 1 on all four."""
    a = np.ascontiguousarray(frames)
    four = np.concatenate([a, np.ones(a.shape[:3] + (1,), a.dtype)], axis=3).astype(np.float32)
    return torch.from_numpy(four / 127.5 - 1.0).permute(0, 3, 1, 2).contiguous()


def tpmap_ref(sd: dict, frames: np.ndarray) -> torch.Tensor:
    """uint8 RGB [n, H, W, 3] -> float32 [n, H/2, W/2, 9] channels-last: the network's output channels 7 .. 15 (0 the centre logit, 1 .. 4
    the displacements)."""
    with torch.no_grad():
        return mlsd_net(sd)(to_input(frames)).permute(0, 2, 3, 1).contiguous()


# ---- decode --------------------------------------------------------------------------------------------------------------------------
def _sigmoid32(x: np.ndarray) -> np.ndarray:
    return torch.sigmoid(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))).numpy()


def _nms_heat(center: np.ndarray):
    """float32 logits [h, w] -> (heat float32, keep bool): heat == max_pool2d(heat, 3, stride 1, padding 1), which pads with -inf."""
    heat = _sigmoid32(center)
    p = np.pad(heat, 1, mode="constant", constant_values=-np.inf)
    h, w = heat.shape
    mx = np.max(np.stack([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)]), axis=0)
    return heat, heat == mx


def _endpoint(pix: int, disp) -> int:
    v = 2.0 * (float(pix) + float(disp))       # float64 from the fp32 displacement
    if v != v:
        return 0
    return int(max(-1073741824.0, min(1073741824.0, v)))   # pinned as the device pins it (2^30: far outside any image)


def decode_ref(tp: np.ndarray, thr_v: float = 0.1, thr_d: float = 0.1):
    """tp float32 [h, w, >= 5] (channel 0 the centre logit, 1 .. 4 = dx_s, dy_s, dx_e, dy_e) -> int array [count, 4] of (xs, ys, xe, ye) at
    full resolution, in rank order (score descending, flat index ascending)."""
    tp = np.asarray(tp, dtype=np.float32)
    h, w = tp.shape[:2]
    heat, keep = _nms_heat(tp[..., 0])
    flat = (heat * keep).reshape(-1)
    order = np.lexsort((np.arange(flat.size), -flat.astype(np.float64)))[:TOPK]     # top 200 of all pixels
    out = []
    for idx in order:
        score = flat[idx]
        y, x = int(idx) // w, int(idx) % w
        dxs, dys, dxe, dye = tp[y, x, 1:5]
        dist = np.sqrt((dxs - dxe) * (dxs - dxe) + (dys - dye) * (dys - dye))       # float32
        if score > np.float32(thr_v) and dist > np.float32(thr_d):
            out.append([_endpoint(x, dxs), _endpoint(y, dys), _endpoint(x, dxe), _endpoint(y, dye)])
    return np.asarray(out, dtype=np.int64).reshape(-1, 4)


def decode_topk_torch(tp: np.ndarray, thr_v: float = 0.1, thr_d: float = 0.1):
    """The same through the published formulation (torch.sigmoid, F.max_pool2d, torch.topk): equal to decode_ref on tie-free input."""
    t = torch.from_numpy(np.asarray(tp, dtype=np.float32))
    h, w = t.shape[:2]
    heat = torch.sigmoid(t[..., 0])[None, None]
    hmax = F.max_pool2d(heat, (3, 3), stride=1, padding=1)
    heat = (heat * (hmax == heat).float()).reshape(-1)
    scores, indices = torch.topk(heat, TOPK, dim=-1, largest=True)
    yy, xx = torch.div(indices, w, rounding_mode="floor"), torch.fmod(indices, w)
    disp = t[..., 1:5].numpy()
    start, end = disp[..., :2], disp[..., 2:]
    dist_map = np.sqrt(np.sum((start - end) ** 2, axis=-1))
    out = []
    for y, x, score in zip(yy.numpy(), xx.numpy(), scores.numpy()):
        if score > thr_v and dist_map[y, x] > thr_d:
            dxs, dys, dxe, dye = disp[y, x]
            out.append([x + dxs, y + dys, x + dxe, y + dye])
    lines = 2 * np.array(out, dtype=np.float64).reshape(-1, 4)
    return np.array([[int(v) for v in ln] for ln in lines], dtype=np.int64).reshape(-1, 4)


def decided(tp: np.ndarray, thr_v: float = 0.1, thr_d: float = 0.1) -> bool:
    """True when no decision of the decode hangs on the last bits: no kept score within 1e-4 of thr_v, no distance of a top-200 point
    within 1e-4 of thr_d, a relative gap of at least 1e-5 between the scores ranked 200 and 201, no two 3x3 neighbours with unequal
    logits whose heats differ by less than 1e-6 (where at least one of the two reaches thr_v - 1e-4: which of two pixels below the
    threshold suppresses the other decides nothing, neither can become a point), no endpoint within 1e-3 of an integer."""
    tp = np.asarray(tp, dtype=np.float32)
    h, w = tp.shape[:2]
    heat, keep = _nms_heat(tp[..., 0])
    if np.any(keep & (np.abs(heat - np.float32(thr_v)) < 1e-4)):
        return False
    lg = np.pad(tp[..., 0], 1, mode="constant", constant_values=np.nan)
    hp = np.pad(heat, 1, mode="constant", constant_values=np.nan)
    for dy in range(3):
        for dx in range(3):
            a, b = lg[dy:dy + h, dx:dx + w], hp[dy:dy + h, dx:dx + w]
            with np.errstate(invalid="ignore"):
                if np.any((a != tp[..., 0]) & ~np.isnan(a) & (np.abs(b.astype(np.float64) - heat) < 1e-6) & (np.maximum(b, heat) > thr_v - 1e-4)):
                    return False
    flat = (heat * keep).reshape(-1).astype(np.float64)
    order = np.lexsort((np.arange(flat.size), -flat))
    if flat.size > TOPK:
        s200, s201 = flat[order[TOPK - 1]], flat[order[TOPK]]
        if s200 > thr_v and s201 > thr_v and (s200 - s201) < 1e-5 * s200:
            return False
    for idx in order[:TOPK]:
        if not flat[idx] > thr_v:
            break
        y, x = int(idx) // w, int(idx) % w
        d = tp[y, x, 1:5].astype(np.float64)
        if abs(np.hypot(d[0] - d[2], d[1] - d[3]) - thr_d) < 1e-4:
            return False
        for pix, disp in ((x, d[0]), (y, d[1]), (x, d[2]), (y, d[3])):
            v = 2.0 * (pix + disp)
            if abs(v - np.rint(v)) < 1e-3:
                return False
    return True


# ---- draw ----------------------------------------------------------------------------------------------------------------------------
def clip_line(w: int, h: int, x1: int, y1: int, x2: int, y2: int):
    """OpenCV's clipLine(Size(w, h), pt1, pt2) -> (inside, x1, y1, x2, y2).  int() truncates toward zero, as the (int64) cast does."""
    right, bottom = w - 1, h - 1
    c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8
    c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += int(float(a - y1) * float(x2 - x1) / float(y2 - y1))
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += int(float(a - y2) * float(x2 - x1) / float(y2 - y1))
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += int(float(a - x1) * float(y2 - y1) / float(x2 - x1))
                x1 = a
                c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += int(float(a - x2) * float(y2 - y1) / float(x2 - x1))
                x2 = a
                c2 = 0
    return (c1 | c2) == 0, x1, y1, x2, y2


def line_pixels(w: int, h: int, x1: int, y1: int, x2: int, y2: int):
    """The (x, y) pixels cv2.line(img, (x1, y1), (x2, y2), color, 1) sets on a w x h image: clipLine, then LineIterator(connectivity 8,
    leftToRight)."""
    ok, x1, y1, x2, y2 = clip_line(w, h, int(x1), int(y1), int(x2), int(y2))
    if not ok:
        return []
    dx, dy = x2 - x1, y2 - y1
    if dx < 0:
        dx, dy, x1, y1 = -dx, -dy, x2, y2
    ystep = -1 if dy < 0 else 1
    dy = abs(dy)
    vert = dy > dx
    if vert:
        dx, dy = dy, dx
    err, plus, minus = dx - 2 * dy, 2 * dx, -2 * dy
    px, py, out = x1, y1, []
    for _ in range(dx + 1):
        out.append((px, py))
        neg = err < 0
        err += minus + (plus if neg else 0)
        if vert:
            px += 1 if neg else 0
            py += ystep
        else:
            py += ystep if neg else 0
            px += 1
    return out


def draw_ref(segments, h: int, w: int) -> np.ndarray:
    """int (xs, ys, xe, ye) rows -> the uint8 map [h, w] with 255 on every line."""
    m = np.zeros((h, w), np.uint8)
    for xs, ys, xe, ye in np.asarray(segments, dtype=np.int64).reshape(-1, 4):
        for x, y in line_pixels(w, h, int(xs), int(ys), int(xe), int(ye)):
            m[y, x] = 255
    return m


def detect_ref(tp: np.ndarray, thr_v: float = 0.1, thr_d: float = 0.1) -> np.ndarray:
    """tpMap [h, w, >= 5] of one frame -> the detector's uint8 map [2h, 2w]."""
    h, w = tp.shape[:2]
    return draw_ref(decode_ref(tp, thr_v, thr_d), 2 * h, 2 * w)


def mlsd_detect(sd: dict, image: np.ndarray, resolution: int = 64, thr_v: float = 0.1, thr_d: float = 0.1) -> np.ndarray:
    """MLSDdetector.__call__(image, thr_v, thr_d, detect_resolution=resolution, image_resolution=resolution) for a uint8 [H, W] or
    [H, W, 3] array in scope -> uint8 [H, W, 3] with three equal channels."""
    img = np.asarray(image)
    if img.ndim == 2:
        img = np.repeat(img[:, :, None], 3, axis=2)
    h, w = img.shape[:2]
    if min(h, w) != resolution or h % 64 or w % 64:
        raise NotImplementedError(f"min(H, W) == {resolution} with H % 64 == W % 64 == 0 is the scope, got {h} x {w}")
    m = detect_ref(tpmap_ref(sd, img[None])[0].numpy(), thr_v, thr_d)
    return np.repeat(m[:, :, None], 3, axis=2)


# ---- fixtures shared by the CPU and GPU tests ---------------------------------------------------------------------------------------------
def frames_fixture():
    """Two 64 x 128 RGB frames with smooth, periodic and blocky content plus noise."""
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:64, 0:128]
    out = []
    for k in range(2):
        base = 127 + 80 * np.sin(xx / (5.0 + 3 * k)) * np.cos(yy / (7.0 - 2 * k))
        img = np.stack([base, 255 - base, 60 + 1.2 * xx], axis=2)
        img[16 + 8 * k:40, 24:72 + 16 * k] = (220, 40 + 100 * k, 90)
        img += rng.normal(0, 12, img.shape)
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return np.stack(out)


def _nudge(tp: np.ndarray) -> np.ndarray:
    """Moves every displacement whose endpoint would fall within 2e-3 of an integer by 0.01 (the constructed cases stay `decided`)."""
    h, w = tp.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    for ch, pix in ((1, xx), (2, yy), (3, xx), (4, yy)):
        for _ in range(3):
            v = 2.0 * (pix + tp[..., ch].astype(np.float64))
            bad = np.abs(v - np.rint(v)) < 2e-3
            tp[..., ch] = np.where(bad, tp[..., ch] + np.float32(0.01), tp[..., ch])
    return tp


def decode_cases() -> dict:
    """The constructed 32 x 64 tpMaps [32, 64, 8] of the decode tests (CPU: against the torch formulation and `decided`; GPU: against
    decode_ref): name -> tpMap."""
    h, w = 32, 64
    rng = np.random.default_rng(5)

    def blank():
        tp = np.zeros((h, w, 8), np.float32)
        tp[..., 0] = -8.0                                                 # heat 3.4e-4: one plateau far below thr_v
        tp[..., 1:5] = (rng.standard_normal((h, w, 4)) * 3.0).astype(np.float32)
        return tp

    cases = {}
    tp = blank()                                         # fewer than 200 candidates: 40 isolated peaks with distinct scores
    for i in range(40):
        tp[3 * (i // 10) + 2, 6 * (i % 10) + 2, 0] = 0.5 + 0.07 * i
    cases["few"] = _nudge(tp)
    tp = blank()                                         # exactly a plateau: a 3 x 4 block of one logit keeps every pixel, plus a ramp beside it
    tp[10:13, 20:24, 0] = 2.0
    tp[20, 5:9, 0] = [1.0, 1.5, 2.5, 2.2]              # a ramp: only its maximum stays
    cases["plateau"] = _nudge(tp)
    tp = blank()                                         # more than 200 isolated peaks: 16 x 21 = 336 with distinct scores; the lowest are dropped
    scores = rng.permutation(336).astype(np.float32)
    for i in range(336):
        tp[2 * (i // 21), 3 * (i % 21), 0] = -1.5 + 0.012 * scores[i]
    cases["many"] = _nudge(tp)
    tp = cases["many"].copy()                            # top-200 points with start == end are dropped and not replaced
    flat = tp[..., 0].reshape(-1)
    for idx in np.argsort(-flat)[[0, 7, 50, 199]]:
        y, x = idx // w, idx % w
        tp[y, x, 3:5] = tp[y, x, 1:3] + np.float32(0.01)
    cases["short"] = _nudge(tp)
    return cases


def saturated_case() -> np.ndarray:
    """A 32 x 64 tpMap whose every centre logit is 40: one plateau of heat exactly 1.0, h * w candidates, the top 200 decided by the index
    alone.  (Not `decided` by the letter -- ranks 200 and 201 are equal -- but equal logits give equal heats in any arithmetic.)"""
    tp = np.zeros((32, 64, 8), np.float32)
    tp[..., 0] = 40.0
    tp[..., 1:5] = (np.random.default_rng(6).standard_normal((32, 64, 4)) * 3.0).astype(np.float32)
    return _nudge(tp)


def draw_cases() -> dict:
    """Segment lists on a 64 x 128 (h x w) map: name -> int array [k, 4] of (xs, ys, xe, ye)."""
    h, w = 64, 128
    rng = np.random.default_rng(9)
    cases = {
        "axes": [[5, 10, 60, 10], [7, 3, 7, 50], [10, 10, 40, 40], [40, 12, 12, 40]],
        "octants": [[64 + a * dx, 32 + a * dy, 64 + b * dx, 32 + b * dy] for dx, dy in ((9, 4), (9, -4), (-9, 4), (-9, -4), (4, 9), (4, -9), (-4, 9), (-4, -9))
                    for a, b in ((0, 3), (3, 0))],
        "zero": [[30, 30, 30, 30], [0, 0, 0, 0], [127, 63, 127, 63]],
        "through": [[-20, 10, 150, 50], [30, -15, 90, 80], [-5, 70, 140, -9]],
        "outside": [[-10, 5, -3, 60], [130, 0, 200, 63], [5, -9, 100, -1], [0, 64, 127, 90], [-5, 30, 30, -40]],
        "far": [[20, 20, 100000, 70000], [-300000, -5, 60, 31], [64, 32, 64, -1000000], [1073741824, 1073741824, 3, 3]],
    }
    cases["random200"] = rng.integers(-40, 170, size=(200, 4)).tolist()
    cases["empty"] = []
    return {k: np.asarray(v, dtype=np.int64).reshape(-1, 4) for k, v in cases.items()}


# ---- the chain with every stored activation rounded to the device type -----------------------------------------------------------------
def tpmap_emulated(sd: dict, frames: np.ndarray, dtype=torch.float16) -> torch.Tensor:
    """The BatchNorm-folded chain of controlanimate_amd/mlsd.py on the CPU, in fp32 arithmetic, with the weights and every activation the
    device stores rounded to `dtype` (dtype=torch.float32: the folded network itself) -> float32 [n, H/2, W/2, 5]."""
    from controlanimate_amd.mlsd import backbone_blocks, folded_layers
    f = folded_layers(sd)

    def r(t):
        return t.to(dtype).float()

    def conv(x, wb, act=None, **kw):
        y = F.conv2d(x, r(wb[0]), wb[1], **kw)
        return y if act is None else (y.clamp(0, 6) if act == "relu6" else y.clamp_min(0))

    with torch.no_grad():
        x = r(to_input(frames))
        x = r(conv(F.pad(x, (0, 1, 0, 1)), f["stem"], "relu6", stride=2))
        taps = {}
        for (idx, _, hid, _, stride, expands, skips), blk in zip(backbone_blocks(), f["features"]):
            t = r(conv(x, blk["expand"], "relu6")) if expands else x
            t = r(conv(F.pad(t, (0, 1, 0, 1)) if stride == 2 else t, blk["dw"], "relu6", stride=stride, padding=0 if stride == 2 else 1, groups=hid))
            y = conv(t, blk["project"])
            x = r(y + x if skips else y)
            if idx in (1, 3, 6, 10, 13):
                taps[idx] = x
        x = taps[13]
        for level, (a, up) in enumerate(((taps[10], False), (taps[6], True), (taps[3], True), (taps[1], True))):
            (w1, w2), (b1, b2) = f["A"][level], f["B"][level]
            b = r(conv(x, w1, "relu"))
            if up:
                b = r(F.interpolate(b, scale_factor=2.0, mode="bilinear", align_corners=True))
            cat = torch.cat((r(conv(a, w2, "relu")), b), dim=1)
            t = r(r(conv(cat, b1, "relu", padding=1)) + cat)
            x = r(conv(t, b2, "relu", padding=1))
        c1, c2, c3 = f["C"]
        x = r(conv(x, c1, "relu", padding=5, dilation=5))
        x = r(conv(x, c2, "relu", padding=1))
        return conv(x, (c3[0][7:12], c3[1][7:12])).permute(0, 2, 3, 1).contiguous()
