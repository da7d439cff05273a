"""The specification of the OpenPose body annotator (controlanimate_amd/openpose.py): the fp32 torch network, and the detector's resizes,
Gaussian, peak finder, connection scoring, assembly and rasterisers in numpy / float64.  Restated from memory of the published code
(controlnet_aux 0.0.6 open_pose/{__init__,body,util}.py, pytorch-openpose's bodypose_model, OpenCV's resize, ellipse2Poly, fillConvexPoly
and circle, scipy's gaussian_filter) and UNPINNED: controlnet_aux, OpenCV and scipy are third-party packages that are absent here, and
no body_pose_model.pth is available.

Deviations from the published code, all deliberate and the device's too: at most MAX_PEAKS peaks per part (the first in row-major order)
and MAX_PEOPLE subset rows, with a bit in `overflow` where a cap was exceeded; a connection whose ends are shared by three or more rows is
skipped (the published code raises IndexError); a row of a LANCZOS4 matrix is renormalised in float64 (OpenCV's eight float coefficients
sum to 1 within 1e-7 only); the limb length is sqrt(d * d + e * e) where the published code writes (d ** 2 + e ** 2) ** 0.5; the body
skeleton only (no hands, no faces)."""
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from mlsd_ref import line_pixels   # cv2.line: clipLine + the 8-connected LineIterator

MAX_PEAKS, MAX_PEOPLE = 64, 64
OVERFLOW_PEAKS, OVERFLOW_PEOPLE = 1, 2
THRE1, THRE2, MID_NUM = 0.1, 0.05, 10
LIMB_SEQ = [[2, 3], [2, 6], [3, 4], [4, 5], [6, 7], [7, 8], [2, 9], [9, 10], [10, 11], [2, 12], [12, 13], [13, 14], [2, 1], [1, 15], [15, 17], [1, 16], [16, 18],
            [3, 17], [6, 18]]
MAP_IDX = [[31, 32], [39, 40], [33, 34], [35, 36], [41, 42], [43, 44], [19, 20], [21, 22], [23, 24], [25, 26], [27, 28], [29, 30], [47, 48], [49, 50], [53, 54],
           [51, 52], [55, 56], [37, 38], [45, 46]]
COLORS = [[255, 0, 0], [255, 85, 0], [255, 170, 0], [255, 255, 0], [170, 255, 0], [85, 255, 0], [0, 255, 0], [0, 255, 85], [0, 255, 170], [0, 255, 255],
          [0, 170, 255], [0, 85, 255], [0, 0, 255], [85, 0, 255], [170, 0, 255], [255, 0, 255], [255, 0, 170], [255, 0, 85]]
FRONT = (("conv1_1", 3, 64), ("conv1_2", 64, 64), "pool1_stage1", ("conv2_1", 64, 128), ("conv2_2", 128, 128), "pool2_stage1", ("conv3_1", 128, 256),
         ("conv3_2", 256, 256), ("conv3_3", 256, 256), ("conv3_4", 256, 256), "pool3_stage1", ("conv4_1", 256, 512), ("conv4_2", 512, 512),
         ("conv4_3_CPM", 512, 256), ("conv4_4_CPM", 256, 128))


# ---- the network ---------------------------------------------------------------------------------------------------------------------
def _seq(layers, no_relu):
    mods = OrderedDict()
    for l in layers:
        if isinstance(l, str):
            mods[l] = nn.MaxPool2d(2, 2, 0)
        else:
            name, cin, cout, k = l
            mods[name] = nn.Conv2d(cin, cout, k, 1, k // 2)
            if name not in no_relu:
                mods["relu_" + name] = nn.ReLU(inplace=False)
    return nn.Sequential(mods)


class BodyPose(nn.Module):
    """pytorch-openpose's bodypose_model: model0, model1_1 / model1_2, ..., model6_1 / model6_2."""

    def __init__(self):
        super().__init__()
        self.model0 = _seq([l if isinstance(l, str) else (*l, 3) for l in FRONT], ())
        for br, c in ((1, 38), (2, 19)):
            s1 = [(f"conv5_{i}_CPM_L{br}", 128, 128, 3) for i in (1, 2, 3)] + [(f"conv5_4_CPM_L{br}", 128, 512, 1), (f"conv5_5_CPM_L{br}", 512, c, 1)]
            setattr(self, f"model1_{br}", _seq(s1, (f"conv5_5_CPM_L{br}",)))
            for t in range(2, 7):
                st = ([(f"Mconv1_stage{t}_L{br}", 185, 128, 7)] + [(f"Mconv{i}_stage{t}_L{br}", 128, 128, 7) for i in (2, 3, 4, 5)] +
                      [(f"Mconv6_stage{t}_L{br}", 128, 128, 1), (f"Mconv7_stage{t}_L{br}", 128, c, 1)])
                setattr(self, f"model{t}_{br}", _seq(st, (f"Mconv7_stage{t}_L{br}",)))

    def forward(self, x):
        feat = self.model0(x)
        l1, l2 = self.model1_1(feat), self.model1_2(feat)
        for t in range(2, 7):
            cat = torch.cat([l1, l2, feat], 1)
            l1, l2 = getattr(self, f"model{t}_1")(cat), getattr(self, f"model{t}_2")(cat)
        return l1, l2


def key_shapes(prefixed: bool = False) -> dict:
    """name -> shape of the module's own state_dict, under the module-prefixed names or the checkpoint's bare ones."""
    sd = BodyPose().state_dict()
    return {(k if prefixed else k.split(".", 1)[1]): tuple(v.shape) for k, v in sd.items()}


def pose_state_dict(seed: int = 0, prefixed: bool = False) -> dict:
    """Seeded weights (no trained checkpoint exists here): He-scaled so that activations keep their size through the 49 layers."""
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for k, shape in key_shapes(True).items():
        if k.endswith(".weight"):
            fan_in = shape[1] * shape[2] * shape[3]
            last = "conv5_5" in k or "Mconv7" in k
            out[k] = torch.randn(shape, generator=gen) * math.sqrt((1.0 if last else 2.0) / fan_in)
        else:
            out[k] = torch.randn(shape, generator=gen) * 0.05
    return out if prefixed else {k.split(".", 1)[1]: v for k, v in out.items()}


def pose_net(sd: dict) -> BodyPose:
    net = BodyPose().eval()
    names = {k.split(".", 1)[1]: k for k in net.state_dict()}
    net.load_state_dict({names[k.split(".", 1)[1] if k.startswith("model") else k]: v.float() for k, v in sd.items()})
    return net


# ---- the input -------------------------------------------------------------------------------------------------------------------------
def geometry(h: int, w: int) -> dict:
    scale = 0.5 * 368 / h
    hs, ws = int(round(h * scale)), int(round(w * scale))
    hp, wp = (hs + 7) // 8 * 8, (ws + 7) // 8 * 8
    return {"scale": scale, "hs": hs, "ws": ws, "hp": hp, "wp": wp, "hl": hp // 8, "wl": wp // 8}


def area_tab(src: int, dst: int, scale: float):
    """computeResizeAreaTab: [(source index, float32 weight), ...] per destination index."""
    tab = []
    for d in range(dst):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, src - f1)
        s1, s2 = int(math.ceil(f1)), int(math.floor(f2))
        s2 = min(s2, src - 1)
        s1 = min(s1, s2)
        row = []
        if s1 - f1 > 1e-3:
            row.append((s1 - 1, np.float32((s1 - f1) / cell)))
        row += [(s, np.float32(1.0 / cell)) for s in range(s1, s2)]
        if f2 - s2 > 1e-3:
            row.append((s2, np.float32(min(min(f2 - s2, 1.0), cell) / cell)))
        tab.append(row)
    return tab


def area_resize_ref(img: np.ndarray, fx: float) -> np.ndarray:
    """cv2.resize(img, (0, 0), fx=fx, fy=fx, interpolation=INTER_AREA) of a uint8 [H, W, C] image, fx < 1 and 1 / fx no integer: the
    horizontal weighted sums first (left to right), then their vertical sum (top to bottom), float32 throughout, rounded half to even."""
    h, w, c = img.shape
    dh, dw = int(round(h * fx)), int(round(w * fx))
    xt, yt = area_tab(w, dw, 1.0 / fx), area_tab(h, dh, 1.0 / fx)
    src = img.astype(np.float32)
    hor = np.zeros((h, dw, c), np.float32)
    for d, row in enumerate(xt):
        acc = np.zeros((h, c), np.float32)
        for s, a in row:
            acc = acc + a * src[:, s]
        hor[:, d] = acc
    out = np.zeros((dh, dw, c), np.float32)
    for d, row in enumerate(yt):
        acc = np.zeros((dw, c), np.float32)
        for s, b in row:
            acc = acc + b * hor[s]
        out[d] = acc
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def input_bytes(frame: np.ndarray) -> np.ndarray:
    """uint8 RGB [H, W, 3] -> the padded uint8 BGR image the network sees [hp, wp, 3] (the padding is 128)."""
    g = geometry(*frame.shape[:2])
    small = area_resize_ref(np.ascontiguousarray(frame[:, :, ::-1]), g["scale"])
    assert small.shape[:2] == (g["hs"], g["ws"])
    return np.pad(small, ((0, g["hp"] - g["hs"]), (0, g["wp"] - g["ws"]), (0, 0)), constant_values=128)


def to_input(frames: np.ndarray) -> torch.Tensor:
    """uint8 RGB [n, H, W, 3] -> float32 [n, 3, hp, wp]: x / 256 - 0.5."""
    x = np.stack([input_bytes(f) for f in frames]).astype(np.float32) / np.float32(256) - np.float32(0.5)
    return torch.from_numpy(x).permute(0, 3, 1, 2).contiguous()


def lowres_ref(sd: dict, frames: np.ndarray):
    """-> (PAF [n, 38, hl, wl], heat [n, 19, hl, wl]), float32: the fp32 network on the specification's input."""
    with torch.no_grad():
        return pose_net(sd)(to_input(frames))


def lowres_emulated(sd: dict, frames: np.ndarray, dtype=torch.float16):
    """The same with the weights and every activation rounded to `dtype` (fp32 accumulation): what the device chain stores.  The last
    layer's output stays fp32, as the device's does."""
    def r(t):
        return t.to(dtype).float()

    def conv(x, name, relu=True, rnd=True):
        w = sd[name + ".weight"]
        y = F.conv2d(x, r(w.float()), sd[name + ".bias"].float(), padding=w.shape[2] // 2)
        y = F.relu(y) if relu else y
        return r(y) if rnd else y

    with torch.no_grad():
        x = r(to_input(frames))
        for l in FRONT:
            x = F.max_pool2d(x, 2) if isinstance(l, str) else conv(x, l[0])
        feat, outs = x, []
        for br in (1, 2):
            a = feat
            for i in (1, 2, 3, 4):
                a = conv(a, f"conv5_{i}_CPM_L{br}")
            outs.append(conv(a, f"conv5_5_CPM_L{br}", relu=False))
        for t in range(2, 7):
            cat, outs = torch.cat([outs[0], outs[1], feat], 1), []
            for br in (1, 2):
                a = cat
                for i in range(1, 7):
                    a = conv(a, f"Mconv{i}_stage{t}_L{br}")
                outs.append(conv(a, f"Mconv7_stage{t}_L{br}", relu=False, rnd=t < 6))
        return outs[0], outs[1]


# ---- back to the frame -----------------------------------------------------------------------------------------------------------------
def lanczos_rows(src: int, dst: int, scale: float) -> np.ndarray:
    """cv2.resize(INTER_LANCZOS4) of float data along one axis, float64 [dst, src] (clamped indices; the row renormalised)."""
    from controlanimate_amd.upscaler import _lanczos4_coeffs
    m = np.zeros((dst, src))
    for d in range(dst):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(math.floor(f))
        for k, c in enumerate(_lanczos4_coeffs(np.float32(f - np.float32(s)))):
            m[d, int(np.clip(s - 3 + k, 0, src - 1))] += float(c)
    return m / m.sum(1, keepdims=True)


def gaussian_taps():
    x = np.arange(-12, 13, dtype=np.float64)
    phi = np.exp(-0.5 / 9.0 * x ** 2)
    return phi / phi.sum()


def gaussian_ref(a: np.ndarray) -> np.ndarray:
    """scipy.ndimage.gaussian_filter(a, sigma=3) of a float64 [.., H, W] array along its last two axes, mode 'reflect'."""
    g = gaussian_taps()
    for axis in (-2, -1):
        n = a.shape[axis]
        idx = (np.arange(-12, n + 12)) % (2 * n)
        idx = np.where(idx < n, idx, 2 * n - 1 - idx)
        p = np.take(a, idx, axis=axis)
        a = sum(g[t] * np.take(p, np.arange(t, t + n), axis=axis) for t in range(25))
    return a


def maps_ref(paf_low: np.ndarray, heat_low: np.ndarray, h: int, w: int):
    """One frame's network output (PAF [38, hl, wl], heat [19, hl, wl]) -> float64 (raw heat [18, h, w], smoothed heat [18, h, w], PAF
    [38, h, w]), step by step: x8 LANCZOS4, crop, LANCZOS4 to the frame; the Gaussian on the heat maps of parts 0 .. 17."""
    g = geometry(h, w)

    def back(m):
        m = np.asarray(m, np.float64)
        up = lanczos_rows(g["hl"], g["hp"], 0.125) @ m @ lanczos_rows(g["wl"], g["wp"], 0.125).T
        up = up[:, :g["hs"], :g["ws"]]
        return lanczos_rows(g["hs"], h, 1.0 / (float(h) / g["hs"])) @ up @ lanczos_rows(g["ws"], w, 1.0 / (float(w) / g["ws"])).T

    raw = back(heat_low[:18])
    return raw, gaussian_ref(raw), back(paf_low)


# ---- decode ----------------------------------------------------------------------------------------------------------------------------
class Margins:
    """Collects how close every threshold comparison of a decode came, relative to the larger of the two sides."""

    def __init__(self):
        self.worst, self.what, self.ties = np.inf, "", []

    def note(self, value, threshold, what, scale=None):
        """scale: the size of the terms the value was computed from, for a threshold of zero (where value / max(|value|, 0) is always 1)."""
        m = abs(value - threshold) / (scale if scale is not None else max(abs(value), abs(threshold), 1e-300))
        if m < self.worst:
            self.worst, self.what = m, f"{what}: {value!r} against {threshold!r}"


def peaks_ref(raw: np.ndarray, smooth: np.ndarray, margins=None):
    """-> ([per part: [(x, y, score), ...]], overflow bit): capped at MAX_PEAKS per part in row-major order."""
    out, over = [], 0
    for part in range(18):
        one = np.asarray(smooth[part])
        z = np.zeros_like(one)
        up, down, left, right = z.copy(), z.copy(), z.copy(), z.copy()
        up[1:, :], down[:-1, :], left[:, 1:], right[:, :-1] = one[:-1, :], one[1:, :], one[:, :-1], one[:, 1:]
        o64 = one.astype(np.float64)
        binary = (one >= up) & (one >= down) & (one >= left) & (one >= right) & (o64 > THRE1)
        if margins is not None:
            i = np.argmin(np.abs(o64 - THRE1))
            margins.note(float(o64.flat[i]), THRE1, f"peak threshold of part {part}")
        ys, xs = np.nonzero(binary)
        if len(ys) > MAX_PEAKS:
            over = OVERFLOW_PEAKS
        out.append([(int(x), int(y), raw[part][y, x]) for y, x in zip(ys[:MAX_PEAKS], xs[:MAX_PEAKS])])
    return out, over


def connect_ref(paf: np.ndarray, peaks, h: int, margins=None):
    """-> per limb [(i, j, score), ...]: indices into the two parts' peak lists, in the order the greedy matching made them."""
    out = []
    for k in range(19):
        ca, cb = peaks[LIMB_SEQ[k][0] - 1], peaks[LIMB_SEQ[k][1] - 1]
        mid = [paf[MAP_IDX[k][0] - 19], paf[MAP_IDX[k][1] - 19]]
        cands = []
        for i, a in enumerate(ca):
            for j, b in enumerate(cb):
                vx, vy = b[0] - a[0], b[1] - a[1]
                norm = max(0.001, math.sqrt(vx * vx + vy * vy))
                ux, uy = vx / norm, vy / norm
                sx, sy = np.linspace(a[0], b[0], num=MID_NUM), np.linspace(a[1], b[1], num=MID_NUM)
                pts = [np.float64(mid[0][int(round(sy[s])), int(round(sx[s]))]) * ux + np.float64(mid[1][int(round(sy[s])), int(round(sx[s]))]) * uy
                       for s in range(MID_NUM)]
                score = sum(pts) / len(pts) + min(0.5 * h / norm - 1, 0)
                if margins is not None:
                    for p in pts:
                        margins.note(float(p), THRE2, f"limb {k} sample")
                    prior = min(0.5 * h / norm - 1, 0)   # score = mean + prior against 0: the margin is absolute, in units of its terms
                    scale = max(abs(sum(pts) / len(pts)), abs(prior), max(abs(p) for p in pts))
                    if scale > 0:   # (every term exactly zero -- two peaks on one pixel: 0.0 > 0 is no matter of rounding)
                        margins.note(float(score), 0.0, f"limb {k} score", scale=scale)
                if len([p for p in pts if p > THRE2]) > 0.8 * len(pts) and score > 0:
                    cands.append((i, j, float(score)))
        if margins is not None and len({c[2] for c in cands}) != len(cands):
            margins.ties.append(k)
        cands = sorted(cands, key=lambda c: c[2], reverse=True)
        conn, used_a, used_b = [], set(), set()
        for i, j, s in cands:
            if i not in used_a and j not in used_b:
                conn.append((i, j, s))
                used_a.add(i), used_b.add(j)
                if len(conn) >= min(len(ca), len(cb)):
                    break
        out.append(conn)
    return out


def assemble_ref(peaks, conns, h: int, w: int, margins=None):
    """-> (keypoints int [MAX_PEOPLE, 18, 2], coords likewise, people, overflow bit).  A peak's id is (part, index)."""
    rows, over = [], 0   # [ids (list of 18, None when absent), score, count]
    for k in range(19):
        a, b = LIMB_SEQ[k][0] - 1, LIMB_SEQ[k][1] - 1
        for i, j, s in conns[k]:
            found = [r for r in range(len(rows)) if rows[r][0][a] == (a, i) or rows[r][0][b] == (b, j)]
            sb = np.float64(peaks[b][j][2])
            if len(found) == 1:
                r = rows[found[0]]
                if r[0][b] != (b, j):
                    r[0][b] = (b, j)
                    r[2] += 1
                    r[1] = r[1] + (sb + s)
            elif len(found) == 2:
                r1, r2 = rows[found[0]], rows[found[1]]
                if not any(x is not None and y is not None for x, y in zip(r1[0], r2[0])):
                    r1[0] = [x if x is not None else y for x, y in zip(r1[0], r2[0])]
                    r1[1] = (r1[1] + r2[1]) + s
                    r1[2] += r2[2]
                    del rows[found[1]]
                else:
                    r1[0][b] = (b, j)
                    r1[2] += 1
                    r1[1] = r1[1] + (sb + s)
            elif not found and k < 17:
                if len(rows) < MAX_PEOPLE:
                    ids = [None] * 18
                    ids[a], ids[b] = (a, i), (b, j)
                    rows.append([ids, ((0.0 + np.float64(peaks[a][i][2])) + sb) + s, 2])
                else:
                    over = OVERFLOW_PEOPLE
    kept = []
    for ids, score, count in rows:
        if margins is not None and count >= 4:
            margins.note(float(score / count), 0.4, "score / parts")
        if not (count < 4 or score / count < 0.4):
            kept.append(ids)
    kp, co = -np.ones((MAX_PEOPLE, 18, 2), np.int32), -np.ones((MAX_PEOPLE, 18, 2), np.int32)
    for n, ids in enumerate(kept):
        for q, id_ in enumerate(ids):
            if id_ is not None:
                x, y = peaks[id_[0]][id_[1]][:2]
                co[n, q] = (x, y)
                kp[n, q] = (int(x / float(w) * w), int(y / float(h) * h))
    return kp, co, len(kept), over


def decode_ref(raw, smooth, paf, margins=None) -> dict:
    """One frame's maps (raw / smooth [18, h, w], paf [38, h, w]) -> keypoints, coords, people, overflow."""
    h, w = raw.shape[1:]
    peaks, o1 = peaks_ref(raw, smooth, margins)
    conns = connect_ref(paf, peaks, h, margins)
    kp, co, people, o2 = assemble_ref(peaks, conns, h, w, margins)
    return {"keypoints": kp, "coords": co, "people": people, "overflow": o1 | o2, "peaks": peaks, "connections": conns}


def decided(raw, smooth, paf, tol: float = 1e-9):
    """(True, "") when no comparison of the decode lies within tol (relative) of its threshold and no two connection scores of a limb
    tie; else (False, which one)."""
    m = Margins()
    decode_ref(raw, smooth, paf, m)
    if m.ties:
        return False, f"connection scores of limb(s) {m.ties} tie"
    if m.worst <= tol:
        return False, m.what
    return True, ""


# ---- draw ------------------------------------------------------------------------------------------------------------------------------
SIN_TABLE = np.round(np.sin(np.deg2rad(np.arange(451, dtype=np.float64))), 7).astype(np.float32)   # OpenCV's SinTable: seven decimals, float


def ellipse2poly(cx: int, cy: int, aw: int, ah: int, angle: int):
    """cv2.ellipse2Poly((cx, cy), (aw, ah), angle, 0, 360, 1): the double-precision points rounded half to even, consecutive equal points
    dropped; a single point becomes two."""
    while angle < 0:
        angle += 360
    while angle > 360:
        angle -= 360
    alpha, beta = float(SIN_TABLE[450 - angle]), float(SIN_TABLE[angle])
    pts = []
    for i in range(0, 361):
        x, y = aw * float(SIN_TABLE[450 - i]), ah * float(SIN_TABLE[i])
        p = (int(np.rint((cx + x * alpha) - y * beta)), int(np.rint((cy + x * beta) + y * alpha)))
        if not pts or p != pts[-1]:
            pts.append(p)
    if len(pts) == 1:
        pts = [(cx, cy), (cx, cy)]
    return pts


def _tdiv(a: int, b: int) -> int:   # C++ integer division truncates toward zero
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def fill_convex_poly(canvas: np.ndarray, pts, color) -> None:
    """cv2.fillConvexPoly(canvas, pts, color) (line_type 8, shift 0): the outline with cv2.line, then the rows between the two edge chains
    that leave the topmost vertex, x in 16.16 fixed point."""
    h, w = canvas.shape[:2]
    n = len(pts)
    for i in range(n):
        p0, p1 = pts[i - 1], pts[i]
        for x, y in line_pixels(w, h, p0[0], p0[1], p1[0], p1[1]):
            canvas[y, x] = color
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    xmin, xmax, ymin, ymax = min(xs), max(xs), min(ys), max(ys)
    imin = ys.index(ymin)
    if n < 3 or xmax < 0 or ymax < 0 or xmin >= w or ymin >= h:
        return
    ymax = min(ymax, h - 1)
    edge = [{"idx": imin, "di": 1, "ye": ymin, "x": -65536, "dx": 0}, {"idx": imin, "di": n - 1, "ye": ymin, "x": -65536, "dx": 0}]
    edges, y = n, ymin
    while True:
        for e in edge:
            if y >= e["ye"]:
                idx0, di = e["idx"], e["di"]
                idx = idx0 + di
                if idx >= n:
                    idx -= n
                while True:
                    had = edges
                    edges -= 1
                    if not had > 0:
                        break
                    ty = ys[idx]
                    if ty > y:
                        x0, x1 = xs[idx0] << 16, xs[idx] << 16
                        e["ye"], e["dx"], e["x"], e["idx"] = ty, _tdiv((x1 - x0) * 2 + (ty - y), 2 * (ty - y)), x0, idx
                        break
                    idx0 = idx
                    idx += di
                    if idx >= n:
                        idx -= n
        if edges < 0:
            break
        if y >= 0:
            left, right = (1, 0) if edge[0]["x"] > edge[1]["x"] else (0, 1)
            x1, x2 = (edge[left]["x"] + 32768) >> 16, (edge[right]["x"] + 32768) >> 16
            if x2 >= 0 and x1 < w:
                canvas[y, max(x1, 0):min(x2, w - 1) + 1] = color
        edge[0]["x"] += edge[0]["dx"]
        edge[1]["x"] += edge[1]["dx"]
        y += 1
        if y > ymax:
            break


def circle4(canvas: np.ndarray, cx: int, cy: int, color) -> None:
    """cv2.circle(canvas, (cx, cy), 4, color, -1): the rows the midpoint algorithm fills, clipped."""
    h, w = canvas.shape[:2]
    err, dx, dy, plus, minus = 0, 4, 0, 1, 7
    while dx >= dy:
        for yy, half in ((cy - dy, dx), (cy + dy, dx), (cy - dx, dy), (cy + dx, dy)):
            if 0 <= yy < h and cx + half >= 0 and cx - half < w:
                canvas[yy, max(cx - half, 0):min(cx + half, w - 1) + 1] = color
        dy += 1
        err += plus
        plus += 2
        mask = -1 if err > 0 else 0
        err -= minus & mask
        dx += mask
        minus -= mask & 2


def draw_ref(coords: np.ndarray, people: int, h: int, w: int) -> np.ndarray:
    """draw_bodypose of the first `people` rows of coords [.., 18, 2] (the peaks' own pixels, -1 when absent) -> uint8 RGB [h, w, 3]."""
    canvas = np.zeros((h, w, 3), np.uint8)
    for n in range(people):
        kp = [None if coords[n, q, 0] < 0 else (int(coords[n, q, 0]) / float(w), int(coords[n, q, 1]) / float(h)) for q in range(18)]
        for (k1, k2), color in zip(LIMB_SEQ[:17], COLORS):
            a, b = kp[k1 - 1], kp[k2 - 1]
            if a is None or b is None:
                continue
            Y, X = np.array([a[0], b[0]]) * float(w), np.array([a[1], b[1]]) * float(h)
            mX, mY = np.mean(X), np.mean(Y)
            length = math.sqrt((X[0] - X[1]) * (X[0] - X[1]) + (Y[0] - Y[1]) * (Y[0] - Y[1]))
            angle = math.degrees(math.atan2(X[0] - X[1], Y[0] - Y[1]))
            poly = ellipse2poly(int(mY), int(mX), int(length / 2), 4, int(angle))
            fill_convex_poly(canvas, poly, [int(float(c) * 0.6) for c in color])
        for p, color in zip(kp, COLORS):
            if p is not None:
                circle4(canvas, int(p[0] * w), int(p[1] * h), color)
    return canvas


# ---- planted maps ------------------------------------------------------------------------------------------------------------------------
PLANT_H, PLANT_W = 192, 256
# a standing figure in a unit box: (x, y) of parts 0 .. 17
FIGURE = [(0.50, 0.14), (0.50, 0.30), (0.36, 0.30), (0.30, 0.46), (0.27, 0.62), (0.64, 0.30), (0.70, 0.46), (0.73, 0.62), (0.43, 0.60), (0.42, 0.76),
          (0.41, 0.92), (0.57, 0.60), (0.58, 0.76), (0.59, 0.92), (0.45, 0.09), (0.55, 0.09), (0.39, 0.13), (0.61, 0.13)]


def figure(x0: float, y0: float, bw: float, bh: float, parts=None) -> dict:
    """part -> (x, y) integer pixels of the figure in the box."""
    return {q: (int(round(x0 + FIGURE[q][0] * bw)), int(round(y0 + FIGURE[q][1] * bh))) for q in (range(18) if parts is None else parts)}


def plant(people, h: int = PLANT_H, w: int = PLANT_W, amp=1.0, paf_amp=1.0, extra=()):
    """Full-resolution float32 maps (raw = smoothed heat [18, h, w], PAF [38, h, w]) of planted skeletons: a Gaussian blob (sigma 2.5) of
    height `amp` at every keypoint, the unit vector times paf_amp within 2.5 pixels of every limb whose two ends the person has.
    people: [{part: (x, y)}]; amp / paf_amp: one value or one per person; extra: [(part, x, y)] further blobs."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    heat, paf = np.zeros((18, h, w)), np.zeros((38, h, w))
    amps = amp if isinstance(amp, (list, tuple)) else [amp] * len(people)
    pamps = paf_amp if isinstance(paf_amp, (list, tuple)) else [paf_amp] * len(people)
    blobs = [(q, x, y, amps[n]) for n, p in enumerate(people) for q, (x, y) in p.items()] + [(q, x, y, 1.0) for q, x, y in extra]
    for q, x, y, a in blobs:
        heat[q] = np.maximum(heat[q], a * np.exp(-((xx - x) ** 2 + (yy - y) ** 2) / (2 * 2.5 ** 2)))
    for n, p in enumerate(people):
        for k, (k1, k2) in enumerate(LIMB_SEQ):
            if k1 - 1 in p and k2 - 1 in p:
                (ax, ay), (bx, by) = p[k1 - 1], p[k2 - 1]
                vx, vy = bx - ax, by - ay
                norm = math.hypot(vx, vy)
                if norm == 0:
                    continue
                ux, uy = vx / norm, vy / norm
                t = np.clip(((xx - ax) * ux + (yy - ay) * uy), 0, norm)
                dist = np.hypot(xx - (ax + t * ux), yy - (ay + t * uy))
                band = dist <= 2.5
                paf[MAP_IDX[k][0] - 19][band], paf[MAP_IDX[k][1] - 19][band] = pamps[n] * ux, pamps[n] * uy
    heat = heat.astype(np.float32)
    return heat, heat.copy(), paf.astype(np.float32)


def planted(case: str):
    """-> (raw, smooth, paf, expected): the maps of a case and the people the decode must find, [{part: (x, y)}] in subset order."""
    if case == "one":
        p = [figure(60, 8, 130, 170)]
        return (*plant(p), p)
    if case == "two_crossing":   # the second figure stands 22 pixels to the right: arms and legs cross, every part has two candidates
        p = [figure(40, 8, 130, 170), figure(62, 12, 124, 163)]   # (another size and PAF height: no two scores of a limb tie)
        return (*plant(p, paf_amp=[1.0, 0.9]), p)
    if case == "partial":        # neck, right arm and left shoulder stay; neck, hip and knee of another do not
        p = [figure(20, 8, 130, 170, (1, 2, 3, 4, 5)), figure(120, 8, 130, 170, (1, 8, 9))]
        return (*plant(p), p[:1])
    if case == "merge":          # right arm and head without a neck: two rows until limb 17 (shoulder -- ear) joins them
        p = [figure(60, 8, 130, 170, (2, 3, 4, 0, 14, 16))]
        return (*plant(p), p)
    if case == "weak":           # everything passes its own threshold, the person's score / parts does not reach 0.4
        p = [figure(60, 8, 130, 170)]
        return (*plant(p, amp=0.15, paf_amp=0.1), [])
    if case == "crowd_overflow":  # 96 noses below a small figure whose own nose comes first in row-major order
        p = [figure(10, 4, 80, 100)]
        extra = [(0, x, y) for y in range(125, 190, 12) for x in range(8, 256, 16)]
        return (*plant(p, extra=extra), p)
    if case == "empty":
        return (*plant([]), [])
    raise KeyError(case)


CASES = ("one", "two_crossing", "partial", "merge", "weak", "crowd_overflow", "empty")


def expected_coords(people) -> np.ndarray:
    co = -np.ones((MAX_PEOPLE, 18, 2), np.int32)
    for n, p in enumerate(people):
        for q, xy in p.items():
            co[n, q] = xy
    return co


def draw_cases() -> dict:
    """name -> (coords [MAX_PEOPLE, 18, 2], people) at PLANT_H x PLANT_W: planted poses for the rasteriser."""
    out = {"one": (expected_coords([figure(60, 8, 130, 170)]), 1),
           "two": (expected_coords([figure(40, 8, 130, 170), figure(62, 12, 124, 163)]), 2)}
    edge = figure(-58, -20, 130, 170, (1, 2, 3, 4, 8, 9, 10))     # the right arm and leg touch the left border, the wrist the bottom
    edge = {q: (min(max(x, 0), PLANT_W - 1), min(max(y, 0), PLANT_H - 1)) for q, (x, y) in edge.items()}
    out["leaves_frame"] = (expected_coords([edge, {1: (254, 2), 2: (255, 90), 5: (200, 0), 0: (255, 0)}]), 2)
    out["zero_length"] = (expected_coords([{1: (100, 80), 2: (100, 80), 5: (101, 80), 3: (100, 81)}]), 1)
    out["axes"] = (expected_coords([{1: (100, 80), 2: (60, 80), 5: (140, 80), 8: (100, 150), 0: (100, 30), 11: (130, 110)}]), 1)
    return out


def frames_fixture(n: int = 2, h: int = 256, w: int = 320, seed: int = 0) -> np.ndarray:
    """Smooth random uint8 RGB frames [n, h, w, 3]."""
    gen = torch.Generator().manual_seed(seed)
    low = torch.rand((n, 3, h // 16, w // 16), generator=gen)
    img = F.interpolate(low, size=(h, w), mode="bicubic", align_corners=False) + 0.05 * torch.randn((n, 3, h, w), generator=gen)
    return (img.clamp(0, 1) * 255).round().byte().permute(0, 2, 3, 1).contiguous().numpy()


def e2e_state_dict(seed: int, frames: np.ndarray, quantile: float = 0.97):
    """Seeded weights whose last heat biases (Mconv7_stage6_L2.bias) put the `quantile` of every part's own pre-bias map in the fp32
    reference at the peak threshold, and whose last PAF biases are +0.3 (limbs that point down and to the right then connect)."""
    sd = pose_state_dict(seed)
    sd["Mconv7_stage6_L2.bias"] = torch.zeros(19)
    sd["Mconv7_stage6_L1.bias"] = torch.full((38,), 0.3)
    _, heat = lowres_ref(sd, frames)
    q = torch.quantile(heat.permute(1, 0, 2, 3).reshape(19, -1), quantile, dim=1)
    sd["Mconv7_stage6_L2.bias"] = (THRE1 - q).float()
    return sd
