"""The hand half of the OpenPose detector's hand_and_face=True (modules/controlresiduals_pipeline.py:113 of the reference), driven by
openpose.OpenposeAnnotator when it is given a hand network: the 21 keypoints of the hands of the first `max_hands` wrist boxes of a
frame (`OpenposeAnnotator.hands()`), drawn into the body's drawing after that person's body and before that person's face.

The detector's hand part, as the reference calls it:

    box      util.handDetect per person, from the pixel keypoints shoulder, elbow, wrist = (5, 6, 7) for the left hand and (2, 3, 4) for the
             right one, a hand where all three exist: x = wrist.x + 0.33 (wrist.x - elbow.x), y likewise; width = 1.5 max(|wrist - elbow|,
             0.9 |elbow - shoulder|); x -= width / 2, y -= width / 2, each clamped below at 0; width1 = W - x if x + width > W else width,
             width2 likewise with H; width = min(width1, width2); the box is (int(x), int(y), int(width)) when width >= 20, left before
             right, people in order.  The crop img[y : y + w, x : x + w] is always the full w x w square
    input    cv2.GaussianBlur(crop, (0, 0), 0.8), then per side 184, 368, 552, 736 util.smart_resize (INTER_AREA when w > side, else
             INTER_LANCZOS4), byte / 256 - 0.5
    network  handpose_model: FaceNet's layers with 22 maps: the VGG front end through conv5_3_CPM (128 features at 1/8); conv6_1_CPM 1x1 ->
             512, conv6_2_CPM 1x1 -> 22; stages 2 .. 6 on cat([previous 22, features 128]): five 7x7 to 128, 1x1 128 -> 128, 1x1 128 -> 22
    maps     per scale the 22 maps resized x8 (float32 INTER_LANCZOS4), then to 128 x 128 (float32 INTER_AREA), divided by 4 and summed
    decode   per map 0 .. 20: gaussian_filter(sigma = 3) > 0.05, its 8-connected components (skimage.measure.label), the component with the
             largest sum of the unsmoothed map, the first row-major maximum of the map zeroed outside it; x = int(float(x) * float(w) /
             128.0); a local coordinate 0 makes that axis -1, else the box origin is added
    draw     util.draw_handpose per hand: x = int(float32(float32(px) / W) * W), y likewise; 20 edges cv2.line(thickness = 2) in the colours
             hsv_to_rgb([ie / 20, 1, 1]) * 255 where all four coordinates are > 0.01, then 21 cv2.circle(radius 4, (0, 0, 255), filled)

It runs as (the names are further keys of the annotator's `timings`, the numbers the launches per pass of n * max_hands slots):

    hand_boxes      1    ca_hand_boxes: keypoints and people -> boxes, max_hands slots per frame, the overflow bits
    hand_crop       4    ca_hand_crop, once per side (736 first: it also blurs the crops): the blurred crop resized through host-made
                         tables (the face stage's builders, made for the side)
    hand_conv       60   ca_conv3x3 with CA_ACT_RELU (15 per side)
    hand_pool       12   ca_maxpool2x2
    hand_copy       4    ca_copy_cols: the features into columns 0 .. 127 of the 160-wide concatenation [features 128 | heat 22 + 10 zeros]
    hand_pointwise  48   ca_gemm: the 1x1 layers; a stage's last one (22 rows padded to 24) writes into the concatenation, the sixth
                         stage's into the fp32 maps [slots, m, m, 24], m = side / 8
    hand_conv7      100  ca_conv7x7 (cin = 160 for Mconv1, whose weights are permuted to the concatenation's layout)
    hand_maps       1    ca_hand_maps: the four-scale average and its Gaussian, [slots, 21, 128, 128] each, through composed axis matrices
    hand_peaks      1    ca_hand_peaks: the decode (union-find labelling in LDS, component masses as double sums in a fixed order)
    draw            1    ca_pose_draw_hands in place of ca_pose_draw / ca_pose_draw_faces (csrc/ca_openpose.hip: OpenCV's ThickLine -- the
                         four corners at 16 fractional bits through FillConvexPoly, a radius-1 circle at each end)

Memory: at side 736 a slot's 64-channel plane is 69 MB, so with the default chunk (30 slots per pass) the activation pool holds three to
four buffers of about 2 GB each; a 16-frame window at max_hands = 2 (32 slots) takes about 8 GB of activations, freed with the annotator.
Lower `max_activation_bytes` on the annotator to trade passes for memory.

The specification is tests/hand_ref.py, restated from memory of controlnet_aux 0.0.6 open_pose/{__init__,hand,util}.py and UNPINNED:
controlnet_aux, OpenCV and scikit-image are absent here and no hand_pose_model.pth is available, so the stage's fp16 range on trained
weights is unmeasured (bf16 is the escape, as for the body and the face).

Two caps (deliberate): OVERFLOW_HANDS -- more boxes in a frame than max_hands, the first max_hands are taken; OVERFLOW_HAND_RESIZE -- a
crop side at which INTER_AREA meets an exact integer ratio other than 2 (OpenCV's integer fast path, restated for 2 only) is skipped, the
hand gets no points: w = 184 k with k >= 3, so only frames whose smaller side is at least 552 (576 and up among the admitted sizes)."""
from __future__ import annotations

import functools
import os

import numpy as np

from . import openpose as _body
from .annotator_base import check_state_dict
from .openpose import bare_keys
from .openpose_face import FRONT, pixel_map

WEIGHTS_NAME = "hand_pose_model.pth"
HAND_PARTS, HAND_MAPS, HEAT_COLS, MAP_SIZE, MIN_BOX = 21, 22, 24, 128, 20
SIDES = (184, 368, 552, 736)            # [0.5, 1.0, 1.5, 2.0] * 368: all multiples of the stride, nothing is ever padded
MAP_SIDES = tuple(s // 8 for s in SIDES)
CAT = 160   # the concatenation's columns: features 128 | heat 22 + 10 zeros
OVERFLOW_HANDS, OVERFLOW_HAND_RESIZE = 16, 32
MODE_NONE, MODE_RESIZE = 0, 1
HAND_EDGES = ((0, 1), (1, 2), (2, 3), (3, 4), (0, 5), (5, 6), (6, 7), (7, 8), (0, 9), (9, 10), (10, 11), (11, 12), (0, 13), (13, 14), (14, 15), (15, 16),
              (0, 17), (17, 18), (18, 19), (19, 20))


def hand_key_shapes() -> dict:
    """Every tensor of hand_pose_model.pth: bare layer name -> shape."""
    out = {}

    def add(name, cout, cin, k):
        out[f"{name}.weight"], out[f"{name}.bias"] = (cout, cin, k, k), (cout,)

    for layer in FRONT:
        if layer != "pool":
            add(layer[0], layer[2], layer[1], 3)
    add("conv6_1_CPM", 512, 128, 1)
    add("conv6_2_CPM", HAND_MAPS, 512, 1)
    for t in range(2, 7):
        add(f"Mconv1_stage{t}", 128, 128 + HAND_MAPS, 7)
        for i in (2, 3, 4, 5):
            add(f"Mconv{i}_stage{t}", 128, 128, 7)
        add(f"Mconv6_stage{t}", 128, 128, 1)
        add(f"Mconv7_stage{t}", HAND_MAPS, 128, 1)
    return out


def check_hand_state_dict(sd) -> None:
    """KeyError naming a missing tensor, ValueError naming one that is unexpected or has the wrong shape (bare names)."""
    check_state_dict(sd, hand_key_shapes(), "openpose hand", "the layers of handpose_model")


def load_hand_state_dict(path) -> dict:
    return HandStage._load(path)


# ---- the resize choice on the host -------------------------------------------------------------------------------------------------------
def resize_mode(w: int, side: int) -> str:
    """util.smart_resize's choice for a w x w crop at one side: 'lanczos4' when w <= side, else INTER_AREA -- 'area' through the
    general tables, 'area2x' on OpenCV's fast path (a + b + c + d + 2) >> 2 when w == 2 side, 'none' at any other exact integer ratio
    (the fast path is not restated there: the hand is skipped, OVERFLOW_HAND_RESIZE)."""
    if w <= side:
        return "lanczos4"
    if w % side:
        return "area"
    return "area2x" if w == 2 * side else "none"


def resize_restated(w: int) -> bool:
    """Whether a w x w crop is resized at all four sides by a restated path (what ca_hand_boxes writes into a slot's mode)."""
    return all(resize_mode(w, s) != "none" for s in SIDES)


def unrestated_sides(resolution: int) -> list:
    """The box sides a frame whose smaller side is `resolution` can give (20 .. resolution) that are skipped: none below 552."""
    return [w for w in range(MIN_BOX, resolution + 1) if not resize_restated(w)]


# ---- host-side tables ------------------------------------------------------------------------------------------------------------------
def area_matrix(src: int, dst: int) -> np.ndarray:
    """cv2.resize(INTER_AREA) of float data along one axis, src -> dst with scale = src / dst no integer, as a float64 matrix [dst, src]
    of OpenCV's float32 weights (a row renormalised in float64, so that a constant map stays constant)."""
    from .openpose_face import area_side_tables
    ofs, cnt, w = (t[0] for t in area_side_tables([src], dst))
    m = np.zeros((dst, src), np.float64)
    for d in range(dst):
        m[d, ofs[d]:ofs[d] + cnt[d]] = w[d, :cnt[d]]
    return m / m.sum(axis=1, keepdims=True)


def axis_matrix(m: int) -> np.ndarray:
    """A [128, m] float64: the x8 INTER_LANCZOS4 resize of m network samples (scale 1 / 8, replicated border) followed by the INTER_AREA
    resize of the 8 m samples to 128."""
    from .openpose import lanczos4_matrix
    return area_matrix(8 * m, MAP_SIZE) @ lanczos4_matrix(m, 8 * m, 1.0 / 8.0)


@functools.lru_cache(maxsize=1)
def map_matrices() -> np.ndarray:
    """float32 [2, 230, 128] for ca_hand_maps: plane 0 the transposed A_s ([m, 128]) of the four scales behind each other, plane 1 the
    transposed G A_s with G the sigma-3 Gaussian (scipy's 'reflect') on 128 samples."""
    from .openpose import gaussian_matrix
    g = gaussian_matrix(MAP_SIZE)
    a = [axis_matrix(m) for m in MAP_SIDES]
    return np.ascontiguousarray(np.stack([np.concatenate([x.T for x in a]), np.concatenate([(g @ x).T for x in a])]), dtype=np.float32)


def hand_colors() -> np.ndarray:
    """draw_handpose's 20 edge colours, uint8 [20, 3] RGB: matplotlib.colors.hsv_to_rgb([ie / 20, 1, 1]) * 255 through OpenCV's scalar
    cast (rounds half to even)."""
    out = np.zeros((len(HAND_EDGES), 3), np.uint8)
    for ie in range(len(HAND_EDGES)):
        h6 = ie / float(len(HAND_EDGES)) * 6.0
        i = int(h6)
        f = h6 - i
        p, q, t, v = 0.0, 1.0 - f, 1.0 - (1.0 - f), 1.0
        rgb = ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))[i % 6]
        out[ie] = [int(np.rint(c * 255.0)) for c in rgb]
    return out


# ---- packing -----------------------------------------------------------------------------------------------------------------------------
def pack_mconv1(w):
    """Mconv1's weight [128, 150, 7, 7] on input channels [heat 22 | features 128] -> [128, 7, 7, 160] on [features 128 | heat 22, 10 zeros]."""
    return _body.pack_mconv1(w, ((HAND_MAPS, CAT - 128),))


def pack_hand_weights(sd, dtype) -> dict:
    return _body.pack_crop_cpm_weights(sd, dtype, FRONT, HAND_MAPS, HEAT_COLS, CAT - 128)


# ---- the crop's tables -------------------------------------------------------------------------------------------------------------------
BLUR_SIGMA, AREA_TAPS = 0.8, 16


def blur_taps() -> np.ndarray:
    """The taps of cv2.GaussianBlur(crop, (0, 0), 0.8) as the specification restates it: ksize = cvRound(0.8 * 6 + 1) | 1 = 7 float taps
    exp(-i^2 / (2 sigma^2)), normalised (float64 [7])."""
    k = int(round(BLUR_SIGMA * 6 + 1)) | 1
    i = np.arange(k, dtype=np.float64) - (k - 1) / 2
    t = np.exp(-(i * i) / (2.0 * BLUR_SIGMA * BLUR_SIGMA))
    return t / t.sum()


@functools.lru_cache(maxsize=8)
def resize_tables(side: int, side_max: int) -> dict:
    """ca_hand_crop's tables for one network side and boxes up to side_max (the frame's smaller side) wide: INTER_LANCZOS4 for w = 20 ..
    min(side, side_max) and INTER_AREA for w = side + 1 .. side_max (None when there is none), one row of `side` entries per w; the face
    stage's tables made for this destination size (bit for bit upscaler.lanczos4_tables / openpose.area_tables), and the blur's taps."""
    from .openpose_face import area_side_tables, lanczos4_side_tables
    lz_ofs, lz_coef = lanczos4_side_tables(np.arange(MIN_BOX, min(side, side_max) + 1), side)
    out = {"taps": blur_taps(), "lz_ofs": lz_ofs, "lz_coef": lz_coef, "ar_ofs": None, "ar_cnt": None, "ar_w": None}
    if side_max > side:
        out["ar_ofs"], out["ar_cnt"], out["ar_w"] = area_side_tables(np.arange(side + 1, side_max + 1), side, AREA_TAPS)
    return out


HAND_STAGES = {"hand_boxes": 1, "hand_crop": 4, "hand_conv": 60, "hand_pool": 12, "hand_copy": 4, "hand_pointwise": 48, "hand_conv7": 100, "hand_maps": 1,
               "hand_peaks": 1}


class HandStage(_body.CropStage):
    """The hand stage of one OpenposeAnnotator (`owner`: its dtype, max_activation_bytes and timings are used).  `run` starts from given
    keypoints and people tensors, so tests can plant them."""

    WEIGHTS_NAME = WEIGHTS_NAME

    def __init__(self, owner, state_dict_or_path, max_hands: int = 2):
        if not 1 <= int(max_hands) <= 128:
            raise ValueError(f"max_hands={max_hands} (1 .. 128)")
        sd = self._load(state_dict_or_path) if isinstance(state_dict_or_path, (str, os.PathLike)) else state_dict_or_path
        sd = bare_keys(sd)
        check_hand_state_dict(sd)
        self.owner, self.max_hands = owner, int(max_hands)
        self._host = pack_hand_weights(sd, owner.dtype)   # packed once, on the host
        self._ws = {}

    def chunk_crops(self, side: int, direct: bool) -> int:
        """Crops per pass through the network at one side: as many as keep the largest 16-bit operand (conv1's output -- 69 MB a crop at
        side 736 -- or the im2col tensor of the alternative form of the 7x7 convolutions) within the owner's max_activation_bytes."""
        m = side // 8
        per_crop = max(side * side * 64 * 2, 0 if direct else m * m * 49 * CAT * 2)
        limit = self.max_activation_bytes
        if per_crop > limit:
            raise ValueError(f"a hand crop alone exceeds what the kernels address ({per_crop} > {limit} bytes)")
        return limit // per_crop

    def workspace(self, n: int, h: int, w: int, dev) -> dict:
        """The buffers of a call with n frames of h x w pixels, cached per (n, h, w): the tables of the four sides and the axis matrices on
        the device, the boxes / slots / points / planes, the blurred crops, the network's four fp32 outputs, and one pool of activation
        buffers with a take / give plan per side (the largest side runs first, the others reuse its buffers)."""
        import torch
        from . import kernels as K

        def make(dev):
            total, side_max = n * self.max_hands, min(h, w)
            tables = [{k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in resize_tables(s, side_max).items()} for s in SIDES]
            return {"tables": tables, "mats": torch.from_numpy(map_matrices()).to(dev), "buf": K.hand_buffers(n, self.max_hands, dev),
                    "blurred": torch.empty((total, side_max, side_max, 3), dtype=torch.uint8, device=dev),
                    "heat": [torch.empty((total, m, m, HEAT_COLS), dtype=torch.float32, device=dev) for m in MAP_SIDES],
                    "xmap": torch.from_numpy(pixel_map(w)).to(dev), "ymap": torch.from_numpy(pixel_map(h)).to(dev)}

        ws = self._workspace((n, h, w, str(dev)), make, dev)
        if "net" not in ws:   # one pool, and a plan per side on it
            ws["net"] = [{"pool": ws["pool"], "plan": [], "planned": False} for _ in SIDES]
        return ws

    def _network(self, src, ws, k: int, c0: int, nc: int, direct: bool, blur: bool) -> None:
        """Crops c0 .. c0 + nc - 1 at side SIDES[k]: the blurred, resized input and the network, the 24 map columns into ws["heat"][k]."""
        from . import kernels as K
        side, hl = SIDES[k], MAP_SIDES[k]

        def crop(out):
            return K.hand_crop(src, ws["buf"]["slots"], ws["tables"][k], ws["blurred"], out, first=c0, blur=blur)

        self._cpm_network(ws["net"][k], self._weights(src.device), "hand", FRONT, crop, nc, side, hl, CAT,
                          ws["heat"][k][c0:c0 + nc].view(nc * hl * hl, HEAT_COLS), direct)

    def run(self, src, keypoints, people, overflow_in=None, direct: bool = True) -> dict:
        """frames uint8 [n, H, W, 3] on the device, keypoints int32 [n, 64, 18, 2], people int32 [n] (and the overflow so far, int32 [n]) ->
        the stage's workspace: ["buf"] holds boxes, slots, points, peaks, mass, overflow and the raw / smooth planes, ["heat"] the maps."""
        from . import kernels as K
        n, h, w, _ = src.shape
        ws = self.workspace(n, h, w, src.device)
        total = n * self.max_hands
        self._timed("hand_boxes", K.hand_boxes, keypoints, people, h, w, ws["buf"], overflow_in)
        for k in reversed(range(len(SIDES))):   # the largest side first: it blurs the crops, and its buffers serve the smaller sides
            net, step = ws["net"][k], self.chunk_crops(SIDES[k], direct)
            if net["planned"] and (bool(net.get("direct", True)) != bool(direct) or min(step, total) > net.get("chunk", 0)):
                net["plan"], net["planned"] = [], False   # the other form of the 7x7 convolutions, or a larger chunk than was planned
            net["direct"] = bool(direct)
            net["chunk"] = max(net.get("chunk", 0), min(step, total)) if net["planned"] else min(step, total)
            for c0, sl in self._chunks(total, step):
                self._network(src, ws, k, c0, sl.stop - c0, direct, blur=k == len(SIDES) - 1)
        self._timed("hand_maps", K.hand_maps, ws["heat"], ws["mats"], ws["buf"]["raw"], ws["buf"]["smooth"])
        self._timed("hand_peaks", K.hand_peaks, ws["buf"]["raw"], ws["buf"]["smooth"], ws["buf"], h, w)
        return ws
