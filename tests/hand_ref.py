"""The specification of the hand stage of the OpenPose annotator (controlanimate_amd/openpose_hand.py): the wrist boxes, the blurred
four-scale input, the fp32 torch handpose_model, the four-scale map average, the connected-component decode and the drawing, in numpy
/ torch on the CPU.  Restated from memory of the published code (controlnet_aux 0.0.6 open_pose/{__init__,hand,util}.py, OpenCV's
GaussianBlur and resize, scipy.ndimage.gaussian_filter, skimage.measure.label, matplotlib's hsv_to_rgb) and UNPINNED: controlnet_aux,
OpenCV and scikit-image are third-party packages that are absent here, and no hand_pose_model.pth is available (weights are seeded).  The
body's part is tests/pose_ref.py, the face's tests/face_ref.py.

What is from memory and how it was decided:
  * util.handDetect, Hand.__call__ and the network's layers are as the issue that asked for this stage states them; nothing in them is
    known here to differ from the published code.
  * cv2.GaussianBlur(crop, (0, 0), 0.8) on uint8: OpenCV's uint8 path uses a fixed-point kernel whose rounding is not restated with
    confidence, so gaussian_blur_ref uses the FLOAT taps exp(-i^2 / (2 sigma^2)), i = -3 .. 3, normalised, float64 sums over both axes and
    ONE rounding (half to even) to uint8 at the end, BORDER_REFLECT_101 inside the crop.
  * INTER_AREA at the exact ratio 2 is OpenCV's integer fast path (a + b + c + d + 2) >> 2; any other exact integer ratio is not restated
    and the hand is skipped (OVERFLOW_HAND_RESIZE).
  * the drawing's cv2.line(thickness = 2) is OpenCV's ThickLine, Line2, clipLine and FillConvexPoly at shift 16, from memory of
    modules/imgproc/src/drawing.cpp; the end circles of radius 1 and the keypoint circles of radius 4 are the midpoint algorithm of
    face_ref.disc.
  * labelling is restated as a raster-order flood fill; tests compare it with scipy.ndimage.label(structure=ones((3, 3))), whose label
    order is skimage's.

Deviation (deliberate, the device's too): at most `max_hands` hands per frame, the first boxes in person order, left before right
(OVERFLOW_HANDS)."""
import math

import numpy as np
import torch
import torch.nn as nn

import face_ref as FR
import pose_ref as R

# ---- the numbers of the published code, one line each ------------------------------------------------------------------------------------
LEFT, RIGHT = (5, 6, 7), (2, 3, 4)          # util.handDetect: shoulder, elbow, wrist
RATIO_WRIST_ELBOW = 0.33
MIN_BOX = 20
BOXSIZE, STRIDE, SCALE_SEARCH = 368, 8, (0.5, 1.0, 1.5, 2.0)
SIDES = tuple(int(s * BOXSIZE) for s in SCALE_SEARCH)   # 184, 368, 552, 736
WSIZE = 128
HAND_MAPS, HAND_PARTS = 22, 21              # the network's channels; Hand.__call__ reads maps 0 .. 20
BLUR_SIGMA = 0.8
THRE = 0.05
ZERO_COORD = 1e-6
OVERFLOW_HANDS, OVERFLOW_HAND_RESIZE = 16, 32
EDGES = ((0, 1), (1, 2), (2, 3), (3, 4), (0, 5), (5, 6), (6, 7), (7, 8), (0, 9), (9, 10), (10, 11), (11, 12), (0, 13), (13, 14), (14, 15), (15, 16),
         (0, 17), (17, 18), (18, 19), (19, 20))


# ---- the boxes ---------------------------------------------------------------------------------------------------------------------------
def hand_boxes(kp, h: int, w: int):
    """util.handDetect for one person.  kp: [18, 2] integer pixel keypoints, a negative x for a missing part -> [(x, y, side, is_left)],
    left before right, in Python float arithmetic.

    The crop img[y : y + side, x : x + side] is always the full square: width was cut to W - x where x + width > W, so x + width <= W,
    and int(x) + int(width) <= x + width; the same with H.  Asserted here."""
    kp = np.asarray(kp)
    out = []
    for parts, is_left in ((LEFT, True), (RIGHT, False)):
        if any(kp[q][0] < 0 or kp[q][1] < 0 for q in parts):
            continue
        (x1, y1), (x2, y2), (x3, y3) = ((int(kp[q][0]), int(kp[q][1])) for q in parts)
        x = x3 + RATIO_WRIST_ELBOW * (x3 - x2)
        y = y3 + RATIO_WRIST_ELBOW * (y3 - y2)
        distance_wrist_elbow = math.sqrt((x3 - x2) ** 2 + (y3 - y2) ** 2)
        distance_elbow_shoulder = math.sqrt((x2 - x1) ** 2 + (y2 - y1) ** 2)
        width = 1.5 * max(distance_wrist_elbow, 0.9 * distance_elbow_shoulder)
        x -= width / 2
        y -= width / 2
        if x < 0:
            x = 0
        if y < 0:
            y = 0
        width1 = width
        width2 = width
        if x + width > w:
            width1 = w - x
        if y + width > h:
            width2 = h - y
        width = min(width1, width2)
        if width >= MIN_BOX:
            box = (int(x), int(y), int(width), is_left)
            assert box[0] + box[2] <= w and box[1] + box[2] <= h
            out.append(box)
    return out


def resize_choice(w: int, side: int) -> str:
    """util.smart_resize of a w x w crop to side x side: k = side / w; INTER_AREA when k < 1 ('area', or 'area2x' on the integer fast path
    at w == 2 side, 'skipped' at any other exact integer ratio), else 'lanczos4'."""
    if float(side + side) / float(w + w) < 1:
        if w % side == 0:
            return "area2x" if w // side == 2 else "skipped"
        return "area"
    return "lanczos4"


def restated(w: int) -> bool:
    return all(resize_choice(w, s) != "skipped" for s in SIDES)


def boxes_ref(keypoints: np.ndarray, people: int, h: int, w: int, max_hands: int):
    """One frame: keypoints [MAX_PEOPLE, 18, 2] -> (boxes int32 [MAX_PEOPLE, 2, 4] = (x, y, side, slot), left then right; slots [(person,
    hand (0 left, 1 right), (x, y, side), restated)] of at most max_hands entries; overflow bits)."""
    boxes = np.zeros((R.MAX_PEOPLE, 2, 4), np.int32)
    boxes[:, :, 3] = -1
    slots, over = [], 0
    for p in range(people):
        for x, y, side, is_left in hand_boxes(keypoints[p], h, w):
            hd = 0 if is_left else 1
            boxes[p, hd, :3] = (x, y, side)
            if len(slots) >= max_hands:
                over |= OVERFLOW_HANDS
                continue
            ok = restated(side)
            if not ok:
                over |= OVERFLOW_HAND_RESIZE
            boxes[p, hd, 3] = len(slots)
            slots.append((p, hd, (x, y, side), ok))
    return boxes, slots, over


# ---- the input ---------------------------------------------------------------------------------------------------------------------------
def blur_taps() -> np.ndarray:
    """getGaussianKernel for sigma 0.8 on uint8: ksize = cvRound(0.8 * 6 + 1) | 1 = 7 float taps (see the head: not the fixed-point path)."""
    k = int(round(BLUR_SIGMA * 6 + 1)) | 1
    assert k == 7
    i = np.arange(k, dtype=np.float64) - (k - 1) / 2
    t = np.exp(-(i * i) / (2.0 * BLUR_SIGMA * BLUR_SIGMA))
    return t / t.sum()


def gaussian_blur_ref(crop: np.ndarray) -> np.ndarray:
    """uint8 [w, w, C] -> uint8: rows then columns in float64, BORDER_REFLECT_101 (dcb | abcd | cba) inside the crop, one rounding."""
    t = blur_taps()
    r = len(t) // 2
    a = crop.astype(np.float64)
    for axis in (1, 0):
        n = a.shape[axis]
        idx = np.arange(-r, n + r)
        idx = np.abs(idx)
        idx = np.where(idx >= n, 2 * (n - 1) - idx, idx)
        p = np.take(a, idx, axis=axis)
        a = sum(t[k] * np.take(p, np.arange(k, k + n), axis=axis) for k in range(len(t)))
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def area2x_ref(img: np.ndarray) -> np.ndarray:
    """INTER_AREA at the exact ratio 2 on uint8: (a + b + c + d + 2) >> 2."""
    s = img.astype(np.int32)
    return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def hand_input_bytes(frame: np.ndarray, box):
    """uint8 RGB frame [H, W, 3] and a box (x, y, side) -> the four uint8 BGR images the network sees ([184, 184, 3] .. [736, 736, 3]), or
    None for a skipped side."""
    x, y, side = box[:3]
    if not restated(side):
        return None
    crop = gaussian_blur_ref(np.ascontiguousarray(frame[y:y + side, x:x + side, ::-1]))
    out = []
    for s in SIDES:
        choice = resize_choice(side, s)
        out.append(area2x_ref(crop) if choice == "area2x" else (FR.area_resize_ref if choice == "area" else FR.lanczos4_resize_ref)(crop, s, s))
    return out


# ---- the network -----------------------------------------------------------------------------------------------------------------------
class HandPose(nn.Module):
    """pytorch-openpose's handpose_model: model1_0 (conv1_1 .. conv5_3_CPM), model1_1 (conv6_1_CPM, conv6_2_CPM), model2 .. model6."""

    def __init__(self):
        super().__init__()
        self.model1_0 = R._seq([l if isinstance(l, str) else (*l, 3) for l in FR.FRONT], ())
        self.model1_1 = R._seq([("conv6_1_CPM", 128, 512, 1), ("conv6_2_CPM", 512, HAND_MAPS, 1)], ("conv6_2_CPM",))
        for t in range(2, 7):
            st = ([(f"Mconv1_stage{t}", 128 + HAND_MAPS, 128, 7)] + [(f"Mconv{i}_stage{t}", 128, 128, 7) for i in (2, 3, 4, 5)] +
                  [(f"Mconv6_stage{t}", 128, 128, 1), (f"Mconv7_stage{t}", 128, HAND_MAPS, 1)])
            setattr(self, f"model{t}", R._seq(st, (f"Mconv7_stage{t}",)))

    def forward(self, x):
        feat = self.model1_0(x)
        out = self.model1_1(feat)
        for t in range(2, 7):
            out = getattr(self, f"model{t}")(torch.cat([out, feat], 1))
        return out


def key_shapes(prefixed: bool = False) -> dict:
    sd = HandPose().state_dict()
    return {(k if prefixed else k.split(".", 1)[1]): tuple(v.shape) for k, v in sd.items()}


def hand_state_dict(seed: int = 0, prefixed: bool = False) -> dict:
    """Seeded weights (no trained checkpoint exists here): He-scaled so that activations keep their size through the 50 layers."""
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for k, shape in key_shapes(True).items():
        if k.endswith(".weight"):
            fan_in = shape[1] * shape[2] * shape[3]
            last = "conv6_2" in k or "Mconv7" in k
            out[k] = torch.randn(shape, generator=gen) * math.sqrt((1.0 if last else 2.0) / fan_in)
        else:
            out[k] = torch.randn(shape, generator=gen) * 0.05
    return out if prefixed else {k.split(".", 1)[1]: v for k, v in out.items()}


# ---- the maps --------------------------------------------------------------------------------------------------------------------------
def area_rows(src: int, dst: int) -> np.ndarray:
    """cv2.resize(INTER_AREA) of float data along one axis as a float64 matrix [dst, src] of OpenCV's float32 weights, the row
    renormalised (scale = src / dst, as cv2.resize computes it from the two sizes; no integer here)."""
    m = np.zeros((dst, src))
    for d, row in enumerate(R.area_tab(src, dst, float(src) / dst)):
        for s, a in row:
            m[d, s] += float(a)
    return m / m.sum(1, keepdims=True)


def maps_ref(heats):
    """The network's maps of the four scales ([22, m, m] each, m = 23, 46, 69, 92) -> float64 (heatmap_avg [21, 128, 128], its
    gaussian_filter(sigma = 3)): per scale smart_resize_k(fx = fy = 8) (INTER_LANCZOS4 per channel, a float32 result), smart_resize to
    128 x 128 (INTER_AREA, a float32 result), divided by 4 and summed in float64."""
    avg = np.zeros((HAND_PARTS, WSIZE, WSIZE), np.float64)
    for heat in heats:
        hm = np.asarray(heat, np.float64)[:HAND_PARTS]
        m = hm.shape[1]
        lz, ar = R.lanczos_rows(m, STRIDE * m, 1.0 / STRIDE), area_rows(STRIDE * m, WSIZE)
        up = (lz @ hm @ lz.T).astype(np.float32).astype(np.float64)
        small = (ar @ up @ ar.T).astype(np.float32).astype(np.float64)
        avg += small / len(heats)
    return avg, R.gaussian_ref(avg)


# ---- the decode ------------------------------------------------------------------------------------------------------------------------
def label_ref(binary: np.ndarray):
    """skimage.measure.label(binary, return_num=True, connectivity=2): the 8-connected components, numbered from 1 in raster order of
    their first pixel -> (labels int32, count)."""
    h, w = binary.shape
    lab = np.zeros((h, w), np.int32)
    count = 0
    for y0, x0 in zip(*np.nonzero(binary)):
        if lab[y0, x0]:
            continue
        count += 1
        lab[y0, x0] = count
        stack = [(int(y0), int(x0))]
        while stack:
            y, x = stack.pop()
            for yy in range(max(y - 1, 0), min(y + 2, h)):
                for xx in range(max(x - 1, 0), min(x + 2, w)):
                    if binary[yy, xx] and not lab[yy, xx]:
                        lab[yy, xx] = count
                        stack.append((yy, xx))
    return lab, count


def decode_ref(raw: np.ndarray, smooth: np.ndarray):
    """One part's planes [128, 128] -> ((x, y) on the 128 grid, masses of the components in label order).  raw is not modified."""
    map_ori = np.array(raw, np.float64)
    binary = np.ascontiguousarray(np.asarray(smooth, np.float64) > THRE, dtype=np.uint8)
    if np.sum(binary) == 0:
        return (0, 0), []
    label_img, label_numbers = label_ref(binary)
    masses = [float(np.sum(map_ori[label_img == i])) for i in range(1, label_numbers + 1)]
    max_index = int(np.argmax(masses)) + 1
    label_img[label_img != max_index] = 0
    map_ori[label_img == 0] = 0
    y, x = np.unravel_index(map_ori.argmax(), map_ori.shape)   # util.npmax: the first maximum in row-major order
    return (int(x), int(y)), masses


def mass_margin(masses) -> float:
    """How far apart the two best masses are, relative to the larger magnitude (inf with fewer than two components)."""
    if len(masses) < 2:
        return math.inf
    a, b = sorted(masses, reverse=True)[:2]
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def to_frame(peak, box):
    """Hand.__call__'s scaling and detect_hands' shift: x = int(float(x) * float(w) / 128.0); -1 if x < 1e-6 else x + box_x."""
    (x, y), (bx, by, side) = peak, box[:3]
    x = int(float(x) * float(side) / float(WSIZE))
    y = int(float(y) * float(side) / float(WSIZE))
    return (-1 if x < ZERO_COORD else x + bx, -1 if y < ZERO_COORD else y + by)


def peaks_ref(raw: np.ndarray, smooth: np.ndarray, box):
    """[21, 128, 128] planes of one hand -> (points int32 [21, 2] in frame pixels, peaks int32 [21, 2] on the 128 grid, the margins)."""
    pts, pks, margins = np.zeros((HAND_PARTS, 2), np.int32), np.zeros((HAND_PARTS, 2), np.int32), []
    for part in range(HAND_PARTS):
        pk, masses = decode_ref(raw[part], smooth[part])
        pks[part], pts[part] = pk, to_frame(pk, box)
        margins.append(mass_margin(masses))
    return pts, pks, margins


# ---- the drawing's colours ---------------------------------------------------------------------------------------------------------------
def hsv_to_rgb(h: float, s: float, v: float):
    """matplotlib.colors.hsv_to_rgb for one colour."""
    i = int(h * 6.0)
    f = h * 6.0 - i
    p, q, t = v * (1.0 - s), v * (1.0 - s * f), v * (1.0 - s * (1.0 - f))
    return ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))[i % 6]


def edge_colors() -> np.ndarray:
    """util.draw_handpose: hsv_to_rgb([ie / 20, 1, 1]) * 255 through cv2's scalar cast (saturate_cast<uchar>(double): half to even)."""
    return np.array([[int(np.rint(c * 255.0)) for c in hsv_to_rgb(ie / float(len(EDGES)), 1.0, 1.0)] for ie in range(len(EDGES))], np.uint8)


# ---- planted inputs ----------------------------------------------------------------------------------------------------------------------
def arm(wrist, elbow, shoulder, left=True) -> dict:
    """{part: (x, y)} of one arm."""
    parts = LEFT if left else RIGHT
    return {parts[0]: shoulder, parts[1]: elbow, parts[2]: wrist}


def keypoints_of(people_list) -> np.ndarray:
    """[{part: (x, y)}, ...] -> int32 [MAX_PEOPLE, 18, 2], -1 for what is missing."""
    kp = -np.ones((R.MAX_PEOPLE, 18, 2), np.int32)
    for p, parts in enumerate(people_list):
        for q, xy in parts.items():
            kp[p, q] = xy
    return kp


# (frame h, w), the people of a frame.  Wrist straight below the elbow by 16: width 24, x = wrist.x - 12, y = wrist.y + 5.28 - 12.
BOX_CASES = {
    "left_only": ((512, 512), [arm((200, 300), (180, 260), (170, 200))]),
    "right_only": ((512, 512), [arm((300, 300), (320, 250), (330, 200), left=False)]),
    "both": ((512, 512), [{**arm((200, 300), (180, 260), (170, 200)), **arm((300, 310), (320, 250), (330, 200), left=False)}]),
    "none": ((512, 512), [{5: (170, 200), 6: (180, 260), 2: (330, 200), 4: (300, 300)}]),
    "clamped_left": ((512, 512), [arm((5, 300), (30, 280), (60, 200))]),
    "clamped_top": ((512, 512), [arm((200, 4), (210, 40), (220, 100))]),
    "clamped_right": ((512, 768), [arm((760, 300), (720, 290), (660, 250))]),
    "clamped_bottom": ((768, 512), [arm((200, 760), (190, 700), (180, 640))]),
    "width_at_20": ((512, 512), [arm((504, 200), (504, 184), (504, 180))]),        # x = 492, cut to 512 - 492 = 20: kept
    "width_under_20": ((512, 512), [arm((505, 200), (505, 184), (505, 180))]),     # x = 493, cut to 19: dropped
    "short_arm": ((512, 512), [arm((200, 300), (200, 290), (200, 280))]),          # width 15: dropped
    "elbow_shoulder_rules": ((512, 512), [arm((200, 300), (200, 290), (200, 190))]),   # 0.9 * 100 > 10: width 135
    "two_people": ((512, 512), [arm((100, 300), (90, 250), (80, 200)), {**arm((300, 300), (290, 250), (280, 200)), **arm((400, 300), (410, 250), (420, 200), left=False)}]),
    "three_people": ((512, 512), [{**arm((60, 300), (50, 250), (40, 200)), **arm((140, 300), (150, 250), (160, 200), left=False)},
                                  arm((300, 300), (290, 250), (280, 200), left=False), arm((440, 300), (430, 250), (420, 200))]),
}


def _blob(cy: float, cx: float, amp: float, sigma: float) -> np.ndarray:
    y, x = np.mgrid[0:WSIZE, 0:WSIZE].astype(np.float64)
    return amp * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2.0 * sigma * sigma))


def decode_cases() -> dict:
    """name -> (raw, smooth, expected (x, y)): planted float32 [128, 128] plane pairs.  smooth is 1 on the binary plane and 0 off it; the
    values of raw are small integers or powers of two, so every sum is exact in any order."""
    n = WSIZE
    cases = {}

    def case(name, raw, binary, want):
        cases[name] = (raw.astype(np.float32), binary.astype(np.float32), want)

    gen = np.random.default_rng(5)
    case("empty", gen.standard_normal((n, n)), np.zeros((n, n)), (0, 0))
    b, r = np.zeros((n, n)), np.zeros((n, n))
    for (y, x), v in zip(((0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1)), (1, 2, 4, 3)):
        b[y, x], r[y, x] = 1, v
    case("corners", r, b, (0, n - 1))
    r = np.ones((n, n))
    r[77, 101] = r[90, 3] = 2
    case("full", r, np.ones((n, n)), (101, 77))
    b, r = np.zeros((n, n)), np.zeros((n, n))
    b[10:21, 10:21] = b[21:31, 21:31] = 1    # 121 + 100 pixels that touch at (20, 20) / (21, 21) only
    b[60:70, 40:55] = 1                      # 150 pixels
    r[b > 0] = 1
    r[25, 27], r[63, 50] = 2, 4              # 222 against 153: the joined pair wins, though the third blob holds the taller peak
    case("diagonal", r, b, (27, 25))
    b = np.zeros((n, n))
    b[0::2] = 1
    b[1::4, n - 1] = b[3::4, 0] = 1
    r = np.where(b > 0, 1.0, 0.0)
    r[126, 5] = 2
    case("serpentine", r, b, (5, 126))
    b = np.zeros((n, n))
    b[0::2, 0::2] = 1
    r = b.copy()
    r[40, 80] = r[90, 20] = 2                # two heaviest components of equal mass: the first label wins
    case("isolated", r, b, (80, 40))
    b, r = np.zeros((n, n)), np.zeros((n, n))
    b[30, 30:34], r[30, 30:34] = 1, (0.5, 0.5, 1, 2)
    b[50, 50], r[50, 50] = 1, 4              # masses 4 and 4: the first label wins, though the second holds the taller peak
    case("equal_masses", r, b, (33, 30))
    b, r = np.zeros((n, n)), np.zeros((n, n))
    b[20, 100] = 1
    r[20, 100] = 5
    b[70:75, 10:16] = r[70:75, 10:16] = 1    # 30 against 5: the heavier wins; its maxima tie, the first in row-major order is taken
    case("heavier_wins", r, b, (10, 70))
    b, r = np.zeros((n, n)), np.zeros((n, n))
    b[0:4, 0:4], r[0:4, 0:4] = 1, -1         # the winner's maximum is below 0: the first zero of the zeroed plane, outside it
    case("negative", r, b, (4, 0))
    return cases


def random_planes(slots: int = 2, seed: int = 11):
    """-> (raw, smooth) float32 [slots, 21, 128, 128]: a few blobs of random place, size and height per plane on low noise, and its sigma-3
    Gaussian: several components above 0.05, some of them close in mass."""
    gen = np.random.default_rng(seed)
    raw = np.zeros((slots, HAND_PARTS, WSIZE, WSIZE), np.float64)
    for s in range(slots):
        for p in range(HAND_PARTS):
            a = 0.01 * gen.standard_normal((WSIZE, WSIZE))
            for _ in range(int(gen.integers(1, 6))):
                a += _blob(gen.uniform(0, WSIZE), gen.uniform(0, WSIZE), gen.uniform(0.2, 1.0), gen.uniform(1.5, 6.0))
            raw[s, p] = a
    raw = raw.astype(np.float32)
    return raw, R.gaussian_ref(raw.astype(np.float64)).astype(np.float32)


# ---- the network's fixtures --------------------------------------------------------------------------------------------------------------
def hand_net(sd: dict) -> HandPose:
    net = HandPose().eval()
    names = {k.split(".", 1)[1]: k for k in net.state_dict()}
    net.load_state_dict({names[k.split(".", 1)[1] if k.startswith("model") else k]: v.float() for k, v in sd.items()})
    return net


def heat_ref(sd: dict, images: np.ndarray) -> torch.Tensor:
    """uint8 BGR [n, side, side, 3] -> the fp32 network's stage-6 output [n, 22, side / 8, side / 8]."""
    with torch.no_grad():
        return hand_net(sd)(FR.to_input(images))


def e2e_hand_state_dict(seed: int, images: np.ndarray, quantile: float = 0.9):
    """Seeded weights whose last biases (Mconv7_stage6.bias) put the `quantile` of every part's own pre-bias map in the fp32 reference on
    `images` (uint8 BGR [n, 184, 184, 3]) at the threshold 0.05: most parts have components above it."""
    sd = hand_state_dict(seed)
    sd["Mconv7_stage6.bias"] = torch.zeros(HAND_MAPS)
    heat = heat_ref(sd, images)
    q = torch.quantile(heat.permute(1, 0, 2, 3).reshape(HAND_MAPS, -1), quantile, dim=1)
    sd["Mconv7_stage6.bias"] = (THRE - q).float()
    return sd


# ---- the drawing -------------------------------------------------------------------------------------------------------------------------
# util.draw_handpose: per hand 20 edges cv2.line(canvas, (x1, y1), (x2, y2), colour, thickness=2) where all four coordinates are > 0.01,
# then 21 cv2.circle(canvas, (x, y), 4, (0, 0, 255), thickness=-1) where both are.  OpenCV's ThickLine, Line2, clipLine and FillConvexPoly
# (shift 16) are restated from memory of modules/imgproc/src/drawing.cpp.
XY_SHIFT, XY_ONE = 16, 1 << 16
HAND_CIRCLE_RADIUS, HAND_CIRCLE_COLOR, DRAW_EPS = 4, (0, 0, 255), 0.01


def clip_line(wd: int, ht: int, x1: int, y1: int, x2: int, y2: int):
    """cv::clipLine(Size2l, Point2l&, Point2l&) -> (inside, x1, y1, x2, y2)."""
    right, bottom = wd - 1, ht - 1
    if wd <= 0 or ht <= 0:
        return False, x1, y1, x2, y2
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


def _put(canvas, x, y, color):
    if 0 <= x < canvas.shape[1] and 0 <= y < canvas.shape[0]:
        canvas[y, x] = color


def line2(canvas: np.ndarray, x1: int, y1: int, x2: int, y2: int, color) -> None:
    """OpenCV's Line2: endpoints at 16 fractional bits, one pixel per step of the longer axis."""
    h, w = canvas.shape[:2]
    ok, x1, y1, x2, y2 = clip_line(w << XY_SHIFT, h << XY_SHIFT, x1, y1, x2, y2)
    if not ok:
        return
    dx, dy = x2 - x1, y2 - y1
    ax, ay = abs(dx), abs(dy)
    if ax > ay:
        if dx < 0:
            x1, x2, y1, y2, dy = x2, x1, y2, y1, -dy
        x_step, y_step = XY_ONE, R._tdiv(dy * XY_ONE, ax | 1)
        ecount = (x2 - x1) >> XY_SHIFT
    else:
        if dy < 0:
            x1, x2, y1, y2, dx = x2, x1, y2, y1, -dx
        x_step, y_step = R._tdiv(dx * XY_ONE, ay | 1), XY_ONE
        ecount = (y2 - y1) >> XY_SHIFT
    x1 += XY_ONE >> 1
    y1 += XY_ONE >> 1
    _put(canvas, (x2 + (XY_ONE >> 1)) >> XY_SHIFT, (y2 + (XY_ONE >> 1)) >> XY_SHIFT, color)
    if ax > ay:
        x1 >>= XY_SHIFT
        while ecount >= 0:
            _put(canvas, x1, y1 >> XY_SHIFT, color)
            x1 += 1
            y1 += y_step
            ecount -= 1
    else:
        y1 >>= XY_SHIFT
        while ecount >= 0:
            _put(canvas, x1 >> XY_SHIFT, y1, color)
            x1 += x_step
            y1 += 1
            ecount -= 1


def fill_convex_poly16(canvas: np.ndarray, pts, color) -> None:
    """cv::FillConvexPoly(img, pts, npts, color, line_type 8, shift 16): pose_ref.fill_convex_poly with the vertices at 16 fractional bits
    (the outline through Line2, a vertex's row (y + 32768) >> 16, x as it is)."""
    h, w = canvas.shape[:2]
    n, delta = len(pts), XY_ONE >> 1
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    for i in range(n):
        line2(canvas, xs[i - 1], ys[i - 1], xs[i], ys[i], color)
    imin = ys.index(min(ys))
    xmin, xmax, ymin, ymax = (min(xs) + delta) >> XY_SHIFT, (max(xs) + delta) >> XY_SHIFT, (min(ys) + delta) >> XY_SHIFT, (max(ys) + delta) >> XY_SHIFT
    if n < 3 or xmax < 0 or ymax < 0 or xmin >= w or ymin >= h:
        return
    ymax = min(ymax, h - 1)
    edge = [{"idx": imin, "di": 1, "ye": ymin, "x": -XY_ONE, "dx": 0}, {"idx": imin, "di": n - 1, "ye": ymin, "x": -XY_ONE, "dx": 0}]
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
                    ty = (ys[idx] + delta) >> XY_SHIFT
                    if ty > y:
                        e["ye"], e["dx"], e["x"], e["idx"] = ty, R._tdiv((xs[idx] - xs[idx0]) * 2 + (ty - y), 2 * (ty - y)), xs[idx0], idx
                        break
                    idx0 = idx
                    idx += di
                    if idx >= n:
                        idx -= n
        if edges < 0:
            break
        if y >= 0:
            left, right = (1, 0) if edge[0]["x"] > edge[1]["x"] else (0, 1)
            x1, x2 = (edge[left]["x"] + delta) >> XY_SHIFT, (edge[right]["x"] + delta) >> XY_SHIFT
            if x2 >= 0 and x1 < w:
                canvas[y, max(x1, 0):min(x2, w - 1) + 1] = color
        edge[0]["x"] += edge[0]["dx"]
        edge[1]["x"] += edge[1]["dx"]
        y += 1
        if y > ymax:
            break


def thick_line2(canvas: np.ndarray, x1: int, y1: int, x2: int, y2: int, color) -> None:
    """cv2.line(canvas, (x1, y1), (x2, y2), color, thickness=2): OpenCV's ThickLine."""
    p0x, p0y, p1x, p1y = x1 << XY_SHIFT, y1 << XY_SHIFT, x2 << XY_SHIFT, y2 << XY_SHIFT
    thickness = 2 << (XY_SHIFT - 1)
    dx, dy = (p0x - p1x) * (1.0 / XY_ONE), (p1y - p0y) * (1.0 / XY_ONE)
    r = dx * dx + dy * dy
    if abs(r) > 2.220446049250313e-16:
        r = thickness / math.sqrt(r)
        dpx, dpy = int(np.rint(dy * r)), int(np.rint(dx * r))   # cvRound
        fill_convex_poly16(canvas, [(p0x + dpx, p0y + dpy), (p0x - dpx, p0y - dpy), (p1x - dpx, p1y - dpy), (p1x + dpx, p1y + dpy)], color)
    for cx, cy in ((x1, y1), (x2, y2)):   # Circle(center, (thickness + 32768) >> 16 = 1, filled)
        FR.disc(canvas, cx, cy, (thickness + (XY_ONE >> 1)) >> XY_SHIFT, color)


def draw_hand(canvas: np.ndarray, points_h: np.ndarray) -> None:
    """util.draw_handpose of one hand's points [21, 2] (frame pixels, -1 for none)."""
    h, w = canvas.shape[:2]
    xy = [(int(np.float32(np.float32(np.float32(px) / np.float32(w)) * np.float32(w))), int(np.float32(np.float32(np.float32(py) / np.float32(h)) * np.float32(h))))
          for px, py in np.asarray(points_h)]
    colors = edge_colors()
    for ie, (e1, e2) in enumerate(EDGES):
        (x1, y1), (x2, y2) = xy[e1], xy[e2]
        if x1 > DRAW_EPS and y1 > DRAW_EPS and x2 > DRAW_EPS and y2 > DRAW_EPS:
            thick_line2(canvas, x1, y1, x2, y2, [int(c) for c in colors[ie]])
    for x, y in xy:
        if x > DRAW_EPS and y > DRAW_EPS:
            FR.disc(canvas, x, y, HAND_CIRCLE_RADIUS, HAND_CIRCLE_COLOR)


def draw_ref(coords: np.ndarray, people: int, hand_points, face_points, h: int, w: int) -> np.ndarray:
    """draw_poses: person by person the body, the left hand, the right hand (hand_points [.., 2, 21, 2]), the face (face_points [.., 71, 2]
    or None) -> uint8 RGB [h, w, 3]."""
    canvas = np.zeros((h, w, 3), np.uint8)
    for n in range(people):
        FR.draw_body(canvas, coords[n])
        for hd in (0, 1):
            draw_hand(canvas, hand_points[n, hd])
        if face_points is not None:
            FR.draw_face(canvas, face_points[n])
    return canvas
