"""The specification of the face stage of the OpenPose annotator (controlanimate_amd/openpose_face.py): the box rule, the crop's resize,
the fp32 torch FaceNet, the peaks and the drawing with faces, in numpy / torch on the CPU.  Restated from memory of the published code
(controlnet_aux 0.0.6 open_pose/{__init__,face,util}.py, OpenCV's resize and circle) and UNPINNED: controlnet_aux and OpenCV are
third-party packages that are absent here, and no facenet.pth is available.  The body's part is tests/pose_ref.py.

Deviations from the published code, all deliberate and the device's too: at most `max_faces` faces per frame (the first people with a box,
OVERFLOW_FACES); a crop whose resize takes an OpenCV path that is not restated -- INTER_AREA chosen while one axis grows, or both scales
exact integers with one of them at least 2 (the integer fast path) -- is skipped (OVERFLOW_FACE_RESIZE; the bit is set for faces that
were taken only); hands are not drawn."""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import pose_ref as R

# ---- the numbers of the published code, one line each ------------------------------------------------------------------------------------
NOSE, EYES, EARS = 0, (14, 15), (16, 17)
EYE_FACTOR, EAR_FACTOR = 3.0, 1.5           # util.faceDetect: width = max(3.0 * eye distance, 1.5 * ear distance)
MIN_BOX = 20                                # ... a box narrower than this is dropped
FACE_SIZE = 384                             # Face.__call__: every crop is resized to 384 x 384
FACE_HEAT = 48                              # ... and the network answers at 1 / 8
FACE_MAPS, FACE_PEAK_MAPS = 71, 71          # FaceNet's output channels; compute_peaks_from_heatmaps reads all of them
PEAK_THRESHOLD = np.float32(0.05)           # heatmaps > 0.05 on a float32 array
ZERO_COORD = 1e-6                           # a local coordinate below this becomes -1
DOT_RADIUS, DOT_COLOR, DRAW_EPS = 3, (255, 255, 255), 0.01   # util.draw_facepose
OVERFLOW_FACES, OVERFLOW_FACE_RESIZE = 4, 8
MIN_SIDE = 11   # the smallest side of a crop: see face_box
FRONT = (("conv1_1", 3, 64), ("conv1_2", 64, 64), "pool1", ("conv2_1", 64, 128), ("conv2_2", 128, 128), "pool2", ("conv3_1", 128, 256),
         ("conv3_2", 256, 256), ("conv3_3", 256, 256), ("conv3_4", 256, 256), "pool3", ("conv4_1", 256, 512), ("conv4_2", 512, 512),
         ("conv4_3", 512, 512), ("conv4_4", 512, 512), ("conv5_1", 512, 512), ("conv5_2", 512, 512), ("conv5_3_CPM", 512, 128))


# ---- the box -----------------------------------------------------------------------------------------------------------------------------
def face_box(kp, h: int, w: int):
    """util.faceDetect for one person.  kp: [18, 2] pixel keypoints, a negative x for a missing part.  -> (x, y, side) or None.

    The smallest crop side: x + width > W happens only where x was clamped to 0 (else x + width is the nose's own x <= W - 1), and then the
    side is W.  Every other box has side int(2 * width) >= 20 and W - int(x) >= W - x = W - nose.x + width >= 1 + 10, so its crop keeps at
    least MIN_SIDE = 11 columns (12 from integer keypoints, whose widths are multiples of 1.5).  Asserted here."""
    kp = np.asarray(kp)
    if kp[NOSE][0] < 0:
        return None
    x0, y0 = float(kp[NOSE][0]), float(kp[NOSE][1])
    width, found = 0.0, False
    for parts, factor in ((EYES, EYE_FACTOR), (EARS, EAR_FACTOR)):
        for q in parts:
            if kp[q][0] >= 0:
                d = max(abs(x0 - float(kp[q][0])), abs(y0 - float(kp[q][1])))
                width, found = max(width, factor * d), True
    if not found:
        return None
    x, y = max(x0 - width, 0.0), max(y0 - width, 0.0)
    width1 = width2 = width * 2
    if x + width > w:   # (the published test: width, not 2 * width)
        width1 = w - x
    if y + width > h:
        width2 = h - y
    width = min(width1, width2)
    if width >= MIN_BOX:
        box = (int(x), int(y), int(width))
        hc, wc = crop_shape(box, h, w)
        assert min(hc, wc) >= MIN_SIDE
        return box
    return None


def crop_shape(box, h: int, w: int):
    x, y, side = box
    return min(side, h - y), min(side, w - x)


def resize_choice(hc: int, wc: int) -> str:
    """util.smart_resize to 384 x 384: 'area' when k = (384 + 384) / (Hc + Wc) < 1, else 'lanczos4'; 'skipped' for the two shapes whose
    OpenCV path is not restated."""
    k = float(FACE_SIZE + FACE_SIZE) / float(hc + wc)
    if k < 1:
        if hc < FACE_SIZE or wc < FACE_SIZE:
            return "skipped"   # INTER_AREA while an axis grows: OpenCV's other path
        if hc % FACE_SIZE == 0 and wc % FACE_SIZE == 0 and max(hc, wc) >= 2 * FACE_SIZE:
            return "skipped"   # both scales exact integers, one of them at least 2: the integer fast path
        return "area"
    return "lanczos4"


def boxes_ref(keypoints: np.ndarray, people: int, h: int, w: int, max_faces: int):
    """One frame: keypoints [MAX_PEOPLE, 18, 2] -> (boxes int32 [MAX_PEOPLE, 4] = (x, y, side, slot), slots [(person, box, choice)] of at
    most max_faces entries in person order, overflow bits)."""
    boxes = np.zeros((R.MAX_PEOPLE, 4), np.int32)
    boxes[:, 3] = -1
    slots, over = [], 0
    for p in range(people):
        box = face_box(keypoints[p], h, w)
        if box is None:
            continue
        boxes[p, :3] = box
        if len(slots) >= max_faces:
            over |= OVERFLOW_FACES
            continue
        choice = resize_choice(*crop_shape(box, h, w))
        if choice == "skipped":
            over |= OVERFLOW_FACE_RESIZE
        boxes[p, 3] = len(slots)
        slots.append((p, box, choice))
    return boxes, slots, over


# ---- the input ---------------------------------------------------------------------------------------------------------------------------
def lanczos4_resize_ref(img: np.ndarray, dh: int, dw: int) -> np.ndarray:
    """cv2.resize(img, (dw, dh), interpolation=INTER_LANCZOS4) of a uint8 [H, W, C] image: OpenCV's 11-bit fixed point, the integer
    horizontal sums first, then their vertical sum, (sum + 2^21) >> 22, indices clamped to the image."""
    from controlanimate_amd.upscaler import lanczos4_tables
    h, w, c = img.shape
    xofs, alpha = lanczos4_tables(w, dw)
    yofs, beta = lanczos4_tables(h, dh)
    src = img.astype(np.int64)
    hor = np.zeros((h, dw, c), np.int64)
    for k in range(8):
        hor += src[:, np.clip(xofs + k, 0, w - 1)] * alpha[:, k].astype(np.int64)[None, :, None]
    out = np.zeros((dh, dw, c), np.int64)
    for k in range(8):
        out += hor[np.clip(yofs + k, 0, h - 1)] * beta[:, k].astype(np.int64)[:, None, None]
    return np.clip((out + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def area_resize_ref(img: np.ndarray, dh: int, dw: int) -> np.ndarray:
    """cv2.resize(img, (dw, dh), interpolation=INTER_AREA) of a uint8 [H, W, C] image with H >= dh and W >= dw and not both scales
    integers: pose_ref.area_resize_ref with one scale per axis (scale = source size / destination size, as cv2.resize computes it)."""
    h, w, c = img.shape
    xt, yt = R.area_tab(w, dw, float(w) / dw), R.area_tab(h, dh, float(h) / dh)
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


def face_input_bytes(frame: np.ndarray, box):
    """uint8 RGB frame [H, W, 3] and a box -> the uint8 BGR image [384, 384, 3] the network sees, or None for a skipped shape."""
    x, y, side = box
    crop = np.ascontiguousarray(frame[y:y + side, x:x + side, ::-1])
    choice = resize_choice(*crop.shape[:2])
    if choice == "skipped":
        return None
    return (area_resize_ref if choice == "area" else lanczos4_resize_ref)(crop, FACE_SIZE, FACE_SIZE)


def to_input(images: np.ndarray) -> torch.Tensor:
    """uint8 BGR [n, 384, 384, 3] -> float32 [n, 3, 384, 384]: x / 256 - 0.5."""
    x = np.asarray(images).astype(np.float32) / np.float32(256) - np.float32(0.5)
    return torch.from_numpy(x).permute(0, 3, 1, 2).contiguous()


# ---- the network -----------------------------------------------------------------------------------------------------------------------
class FaceNet(nn.Module):
    """controlnet_aux's FaceNet: model1_0 (conv1_1 .. conv5_3_CPM), model1_1 (conv6_1_CPM, conv6_2_CPM), model2 .. model6."""

    def __init__(self):
        super().__init__()
        self.model1_0 = R._seq([l if isinstance(l, str) else (*l, 3) for l in FRONT], ())
        self.model1_1 = R._seq([("conv6_1_CPM", 128, 512, 1), ("conv6_2_CPM", 512, FACE_MAPS, 1)], ("conv6_2_CPM",))
        for t in range(2, 7):
            st = ([(f"Mconv1_stage{t}", 128 + FACE_MAPS, 128, 7)] + [(f"Mconv{i}_stage{t}", 128, 128, 7) for i in (2, 3, 4, 5)] +
                  [(f"Mconv6_stage{t}", 128, 128, 1), (f"Mconv7_stage{t}", 128, FACE_MAPS, 1)])
            setattr(self, f"model{t}", R._seq(st, (f"Mconv7_stage{t}",)))

    def forward(self, x):
        feat = self.model1_0(x)
        out = self.model1_1(feat)
        for t in range(2, 7):
            out = getattr(self, f"model{t}")(torch.cat([out, feat], 1))
        return out


def key_shapes(prefixed: bool = False) -> dict:
    sd = FaceNet().state_dict()
    return {(k if prefixed else k.split(".", 1)[1]): tuple(v.shape) for k, v in sd.items()}


def face_state_dict(seed: int = 0, prefixed: bool = False) -> dict:
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


def face_net(sd: dict) -> FaceNet:
    net = FaceNet().eval()
    names = {k.split(".", 1)[1]: k for k in net.state_dict()}
    net.load_state_dict({names[k.split(".", 1)[1] if k.startswith("model") else k]: v.float() for k, v in sd.items()})
    return net


def heat_ref(sd: dict, images: np.ndarray) -> torch.Tensor:
    """uint8 BGR [n, 384, 384, 3] -> the fp32 network's stage-6 output [n, 71, 48, 48]."""
    with torch.no_grad():
        return face_net(sd)(to_input(images))


# ---- peaks -------------------------------------------------------------------------------------------------------------------------------
def upsample_ref(heat, hc: int, wc: int) -> np.ndarray:
    """[C, 48, 48] -> float32 [C, Hc, Wc]: F.interpolate(mode='bilinear', align_corners=True)."""
    t = torch.as_tensor(np.asarray(heat), dtype=torch.float32)[None]
    return F.interpolate(t, size=(hc, wc), mode="bilinear", align_corners=True)[0].numpy()


def peaks_ref(heat, box, h: int, w: int) -> np.ndarray:
    """compute_peaks_from_heatmaps on the upsampled maps of one face and the shift to the frame -> int32 [71, 2] (x, y), -1 for none."""
    hc, wc = crop_shape(box, h, w)
    up = upsample_ref(heat, hc, wc)
    out = -np.ones((FACE_PEAK_MAPS, 2), np.int32)
    for part in range(FACE_PEAK_MAPS):
        m = up[part]
        above = m > PEAK_THRESHOLD
        if not above.any():
            continue
        best = int(np.argmax(np.where(above, m, -np.inf)))   # the first row-major position of the maximum
        y, x = divmod(best, wc)
        out[part] = (-1 if x < ZERO_COORD else x + box[0], -1 if y < ZERO_COORD else y + box[1])
    return out


def undecided_parts(heat, box, h: int, w: int, tol: float, ties=()) -> dict:
    """{part: why} of the parts whose answer a rounding could change: the winner of the upsampled map must beat every pixel farther than 2
    pixels from it, every other pixel near it, and the threshold, by more than tol (a map that stays below the threshold must stay below it
    by more than tol).  Parts listed in `ties` are planted exact ties and are not asked."""
    hc, wc = crop_shape(box, h, w)
    up = upsample_ref(heat, hc, wc).astype(np.float64)
    yy, xx = np.mgrid[0:hc, 0:wc]
    out = {}
    for part in range(FACE_PEAK_MAPS):
        if part in ties:
            continue
        m = up[part]
        top = m.max()
        if abs(top - float(PEAK_THRESHOLD)) <= tol:
            out[part] = f"maximum {top!r} within {tol} of the threshold"
        if top <= float(PEAK_THRESHOLD):
            continue
        y, x = divmod(int(np.argmax(m)), wc)
        far = np.maximum(np.abs(yy - y), np.abs(xx - x)) > 2
        if far.any() and top - m[far].max() <= tol:
            out[part] = f"runner-up {m[far].max()!r} within {tol} of the maximum {top!r}"
        elif np.sum(top - m[~far] <= tol) > 1:
            out[part] = f"a neighbour of the maximum {top!r} lies within {tol} of it"
    return out


def decided(heat, box, h: int, w: int, tol: float, ties=()):
    """(True, "") when no part of undecided_parts is left; else (False, which one)."""
    bad = undecided_parts(heat, box, h, w, tol, ties)
    return (not bad, "; ".join(f"part {k}: {v}" for k, v in bad.items()))


# planted 48 x 48 maps: part -> what it shows
PLANT_UNDER, PLANT_COLUMN0, PLANT_TIE, PLANT_BLOB, PLANT_ROW0 = 0, 1, 2, 3, 4
TIE_VALUE = 0.5   # a power of two: inside a 2 x 2 block of equal nodes (1 - l) * v + l * v is v exactly, in any order of the bilinear sum


def _blob(cy: float, cx: float, amp: float, sigma: float = 3.0) -> np.ndarray:
    yy, xx = np.mgrid[0:FACE_HEAT, 0:FACE_HEAT].astype(np.float64)
    return (amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sigma * sigma))).astype(np.float32)


def planted_heat() -> np.ndarray:
    """float32 [71, 48, 48]: part 0 stays under the threshold; part 1 has its maximum in local column 0 (x becomes -1); part 2 is an exact
    tie between two 2 x 2 blocks of nodes of TIE_VALUE, where the interpolation is exact -- the first in row-major order wins; part 3 is
    an ordinary peak; part 4 has its maximum in local row 0 (y becomes -1); the other parts are zero (no point)."""
    heat = np.zeros((FACE_MAPS, FACE_HEAT, FACE_HEAT), np.float32)
    heat[PLANT_UNDER] = _blob(24.3, 17.6, 0.04)
    heat[PLANT_COLUMN0] = _blob(20.3, 0.0, 0.8)
    heat[PLANT_TIE, 10:12, 30:32] = TIE_VALUE
    heat[PLANT_TIE, 30:32, 8:10] = TIE_VALUE
    heat[PLANT_BLOB] = _blob(31.4, 12.7, 0.6)
    heat[PLANT_ROW0] = _blob(0.0, 33.4, 0.7)
    return heat


# ---- draw --------------------------------------------------------------------------------------------------------------------------------
def pixel_map_ref(side: int) -> np.ndarray:
    """draw_facepose's x of a pixel coordinate p: the point is stored as float32(p) / side in float32 and multiplied back in float32."""
    return np.array([int(np.float32(np.float32(np.float32(p) / np.float32(side)) * np.float32(side))) for p in range(side)], np.int32)


def disc_rows(radius: int):
    """cv2.circle(filled): {dy: half width} of the rows the midpoint algorithm fills."""
    rows = {}
    err, dx, dy, plus, minus = 0, radius, 0, 1, 2 * radius - 1
    while dx >= dy:
        for yy, half in ((-dy, dx), (dy, dx), (-dx, dy), (dx, dy)):
            rows[yy] = max(rows.get(yy, 0), half)
        dy += 1
        err += plus
        plus += 2
        mask = -1 if err > 0 else 0
        err -= minus & mask
        dx += mask
        minus -= mask & 2
    return rows


def disc(canvas: np.ndarray, cx: int, cy: int, radius: int, color) -> None:
    h, w = canvas.shape[:2]
    for dy, half in disc_rows(radius).items():
        yy = cy + dy
        if 0 <= yy < h and cx + half >= 0 and cx - half < w:
            canvas[yy, max(cx - half, 0):min(cx + half, w - 1) + 1] = color


def draw_body(canvas: np.ndarray, coords_n: np.ndarray) -> None:
    """pose_ref.draw_ref's body of one person (coords_n [18, 2], -1 when absent) onto the canvas."""
    h, w = canvas.shape[:2]
    kp = [None if coords_n[q, 0] < 0 else (int(coords_n[q, 0]) / float(w), int(coords_n[q, 1]) / float(h)) for q in range(18)]
    for (k1, k2), color in zip(R.LIMB_SEQ[:17], R.COLORS):
        a, b = kp[k1 - 1], kp[k2 - 1]
        if a is None or b is None:
            continue
        Y, X = np.array([a[0], b[0]]) * float(w), np.array([a[1], b[1]]) * float(h)
        mX, mY = np.mean(X), np.mean(Y)
        length = math.sqrt((X[0] - X[1]) * (X[0] - X[1]) + (Y[0] - Y[1]) * (Y[0] - Y[1]))
        angle = math.degrees(math.atan2(X[0] - X[1], Y[0] - Y[1]))
        poly = R.ellipse2poly(int(mY), int(mX), int(length / 2), 4, int(angle))
        R.fill_convex_poly(canvas, poly, [int(float(c) * 0.6) for c in color])
    for p, color in zip(kp, R.COLORS):
        if p is not None:
            R.circle4(canvas, int(p[0] * w), int(p[1] * h), color)


def draw_face(canvas: np.ndarray, points_n: np.ndarray) -> None:
    """util.draw_facepose of one person's points [71, 2] (frame pixels, -1 for none)."""
    h, w = canvas.shape[:2]
    for px, py in np.asarray(points_n):
        x = int(np.float32(np.float32(np.float32(px) / np.float32(w)) * np.float32(w)))
        y = int(np.float32(np.float32(np.float32(py) / np.float32(h)) * np.float32(h)))
        if x > DRAW_EPS and y > DRAW_EPS:
            disc(canvas, x, y, DOT_RADIUS, DOT_COLOR)


def draw_ref(coords: np.ndarray, people: int, points, h: int, w: int) -> np.ndarray:
    """draw_poses: person by person the body, then the face (points [.., 71, 2] or None) -> uint8 RGB [h, w, 3].  A later person's body
    covers an earlier person's dots."""
    canvas = np.zeros((h, w, 3), np.uint8)
    for n in range(people):
        draw_body(canvas, coords[n])
        if points is not None:
            draw_face(canvas, points[n])
    return canvas


# ---- hand-written keypoints for the box rule, {part: (x, y)} at BOX_H x BOX_W (the expected boxes are in tests/test_openpose_face_cpu.py) ------
BOX_H, BOX_W = 448, 512
BOX_CASES = {
    "eyes_only": {0: (200, 200), 14: (190, 195), 15: (212, 194)},
    "ear_only": {0: (200, 200), 17: (230, 190)},
    "eye_beats_ear": {0: (200, 200), 14: (190, 200), 16: (185, 200)},
    "no_nose": {14: (190, 195), 15: (212, 194), 16: (180, 200), 17: (220, 200)},
    "nose_alone": {0: (200, 200), 1: (200, 260)},
    "clamped_left_top": {0: (20, 30), 15: (35, 28)},
    "half_pixel": {0: (100, 100), 16: (85, 100)},
    "right_rectangular": {0: (490, 200), 14: (478, 200)},
    "bottom_rectangular": {0: (200, 430), 15: (212, 430)},
    "clamped_right_bottom": {0: (100, 200), 15: (300, 200)},
    "clamped_bottom": {0: (250, 220), 14: (90, 220)},
    "side_18": {0: (200, 200), 14: (197, 199)},
    "side_21": {0: (200, 200), 16: (193, 200)},
}


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------------
def e2e_face_state_dict(seed: int, images: np.ndarray, quantile: float = 0.9):
    """Seeded weights whose last biases (Mconv7_stage6.bias) put the `quantile` of every part's own pre-bias map in the fp32 reference on
    `images` (uint8 BGR [n, 384, 384, 3]) at the peak threshold: most parts have a peak, and it is a clear one."""
    sd = face_state_dict(seed)
    sd["Mconv7_stage6.bias"] = torch.zeros(FACE_MAPS)
    heat = heat_ref(sd, images)
    q = torch.quantile(heat.permute(1, 0, 2, 3).reshape(FACE_MAPS, -1), quantile, dim=1)
    sd["Mconv7_stage6.bias"] = (float(PEAK_THRESHOLD) - q).float()
    return sd


def head(x: int, y: int, eye: int = 6, ear: int = 12, parts=(0, 14, 15, 16, 17)) -> dict:
    """Body keypoints of a head: the nose at (x, y), the eyes `eye` pixels to its sides and above, the ears `ear` pixels to its sides."""
    full = {0: (x, y), 14: (x - eye, y - eye // 2), 15: (x + eye, y - eye // 2), 16: (x - ear, y), 17: (x + ear, y)}
    return {q: full[q] for q in parts}


def keypoints_of(people_list) -> np.ndarray:
    """[{part: (x, y)}] -> int32 [MAX_PEOPLE, 18, 2], -1 for none."""
    return R.expected_coords(people_list)
