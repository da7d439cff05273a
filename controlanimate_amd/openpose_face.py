"""The face half of the OpenPose detector's hand_and_face=True (modules/controlresiduals_pipeline.py:113 of the reference), driven by
openpose.OpenposeAnnotator when it is given a face network: the 71 face points of every detected person (one per
map of FaceNet, as the specification reads them: FACE_PEAK_MAPS = 71), drawn as white dots into the
body's drawing.  The hand half is openpose_hand.py (its crops go through the table builders here, made for its four sides).

The detector's face part, as the reference calls it:

    box      util.faceDetect per person, from the pixel keypoints nose 0, eyes 14 / 15, ears 16 / 17: no box without the nose or without
             any of the other four; width = max(3.0 |eye - nose|_inf, 1.5 |ear - nose|_inf); x = max(nose.x - width, 0), y likewise;
             width1 = width2 = 2 width; if x + width > W: width1 = W - x (the published test uses width, not 2 width), y likewise;
             width = min(width1, width2); the box is (int(x), int(y), int(width)) when width >= 20.  The crop is the numpy slice
             img[y : y + w, x : x + w], so it can be rectangular: Hc = min(w, H - y), Wc = min(w, W - x), each at least MIN_SIDE = 11
    input    the BGR crop, cv2.resize to 384 x 384 with INTER_AREA when k = 768 / (Hc + Wc) < 1, else INTER_LANCZOS4 (util.smart_resize),
             x / 256 - 0.5
    network  FaceNet: a VGG-19 front end (conv1_1 .. conv5_2, conv5_3_CPM; 3x3 + ReLU, three 2x2 max pools) to 128 features at 1/8; stage 1
             conv6_1_CPM 1x1 128 -> 512 + ReLU, conv6_2_CPM 1x1 512 -> 71; stages 2 .. 6 on cat([previous 71, features 128]): five 7x7 to
             128 channels, 1x1 128 -> 128, all with ReLU, 1x1 128 -> 71
    peaks    stage 6 at 48 x 48, F.interpolate(bilinear, align_corners=True) to (Hc, Wc); per map 0 .. 70 the first row-major position of the
             maximum over the pixels above 0.05 (none: no point); a local coordinate 0 makes that axis -1; else the box origin is added
    draw     per person the body, then per face point x = int(float32(float32(px) / W) * W), y likewise; cv2.circle(radius 3, white,
             filled) when x > 0.01 and y > 0.01

It runs as (the names are further keys of the annotator's `timings`, the numbers the launches per pass):

    face_boxes      1   ca_face_boxes: keypoints and people -> boxes, max_faces slots per frame in person order, the overflow bits
    face_crop       1   ca_face_crop: frames and slots -> [n * max_faces, 384, 384, 8]; the resize is byte-exact through host-made tables
                        indexed by the crop's side (resize_tables: LANCZOS4 for every side, AREA for sides >= 384; no sine on the device)
    face_conv       15  ca_conv3x3 with CA_ACT_RELU
    face_pool       3   ca_maxpool2x2
    face_copy       1   ca_copy_cols: the features into columns 0 .. 127 of the 224-wide concatenation [features 128 | heat 71 + 25 zeros]
    face_pointwise  12  ca_gemm: the 1x1 layers; a stage's last one (71 rows padded to 72) writes into the concatenation, the sixth
                        stage's into the fp32 maps [n * max_faces, 48, 48, 72]
    face_conv7      25  ca_conv7x7 (cin = 224 for Mconv1, whose weights are permuted to the concatenation's layout)
    face_peaks      1   ca_face_peaks: the bilinear value of every crop pixel on the fly, the arg-max with the lowest index
    draw            1   ca_pose_draw_faces in place of ca_pose_draw

The network always runs on n * max_faces crops: an empty slot gets a constant input and its peaks are ignored, nothing is read back to
size the batch, so the chain with faces still captures into a hipGraph.

The specification is tests/face_ref.py, restated from memory of controlnet_aux 0.0.6 open_pose/{__init__,face,util}.py and UNPINNED:
controlnet_aux and OpenCV are absent here and no facenet.pth is available, so the stage's fp16 range on trained weights is unmeasured.

Two caps and one deviation (deliberate): OVERFLOW_FACES -- more people with a box than max_faces, the first max_faces in person order are
taken; OVERFLOW_FACE_RESIZE -- a crop shape whose resize takes an OpenCV path that is not restated (INTER_AREA chosen while one axis
grows; both scales exact integers with one of them at least 2: the integer fast path) is skipped, the face gets no points.
"""
from __future__ import annotations

import functools
import math
import os

import numpy as np

from . import openpose as _body
from .annotator_base import check_state_dict
from .openpose import bare_keys  # noqa: F401  (one function for the three checkpoints)

WEIGHTS_NAME = "facenet.pth"
FACE_SIZE, FACE_HEAT, FACE_PARTS, FACE_MAPS, MIN_SIDE, TAPS = 384, 48, 71, 72, 11, 8
SPAN_ROWS = 13   # source rows under two output rows that ca_face_crop keeps in LDS (kRowsIn)
CAT = 224   # the concatenation's columns: features 128 | heat 71 + 25 zeros
OVERFLOW_FACES, OVERFLOW_FACE_RESIZE = 4, 8
MODE_NONE, MODE_LANCZOS4, MODE_AREA = 0, 1, 2
FACE_STAGES = {"face_boxes": 1, "face_crop": 1, "face_conv": 15, "face_pool": 3, "face_copy": 1, "face_pointwise": 12, "face_conv7": 25, "face_peaks": 1}

FRONT = (("conv1_1", 3, 64), ("conv1_2", 64, 64), "pool", ("conv2_1", 64, 128), ("conv2_2", 128, 128), "pool", ("conv3_1", 128, 256),
         ("conv3_2", 256, 256), ("conv3_3", 256, 256), ("conv3_4", 256, 256), "pool", ("conv4_1", 256, 512), ("conv4_2", 512, 512),
         ("conv4_3", 512, 512), ("conv4_4", 512, 512), ("conv5_1", 512, 512), ("conv5_2", 512, 512), ("conv5_3_CPM", 512, 128))


def face_key_shapes() -> dict:
    """Every tensor of facenet.pth: layer name -> shape."""
    out = {}

    def add(name, cout, cin, k):
        out[f"{name}.weight"], out[f"{name}.bias"] = (cout, cin, k, k), (cout,)

    for layer in FRONT:
        if layer != "pool":
            add(layer[0], layer[2], layer[1], 3)
    add("conv6_1_CPM", 512, 128, 1)
    add("conv6_2_CPM", FACE_PARTS, 512, 1)
    for t in range(2, 7):
        add(f"Mconv1_stage{t}", 128, 128 + FACE_PARTS, 7)
        for i in (2, 3, 4, 5):
            add(f"Mconv{i}_stage{t}", 128, 128, 7)
        add(f"Mconv6_stage{t}", 128, 128, 1)
        add(f"Mconv7_stage{t}", FACE_PARTS, 128, 1)
    return out


def check_face_state_dict(sd) -> None:
    """KeyError naming a missing tensor, ValueError naming one that is unexpected or has the wrong shape (bare names)."""
    check_state_dict(sd, face_key_shapes(), "openpose face", "the layers of FaceNet")


# ---- the resize choice on the host (what ca_face_boxes writes into a slot) --------------------------------------------------------------
def resize_mode(hc: int, wc: int) -> int:
    """util.smart_resize's choice for an Hc x Wc crop: MODE_AREA when k = 768 / (Hc + Wc) < 1, else MODE_LANCZOS4; MODE_NONE for the two
    shapes whose OpenCV path is not restated (the face is skipped, OVERFLOW_FACE_RESIZE)."""
    if hc + wc > 2 * FACE_SIZE:
        if hc < FACE_SIZE or wc < FACE_SIZE:
            return MODE_NONE   # INTER_AREA while an axis grows
        if hc % FACE_SIZE == 0 and wc % FACE_SIZE == 0:
            return MODE_NONE   # both scales integers, one of them >= 2: the integer fast path
        return MODE_AREA
    return MODE_LANCZOS4


# ---- host-side tables ------------------------------------------------------------------------------------------------------------------
_S45 = 0.70710678118654752440084436210485
_CS = np.array(((1.0, 0.0), (-_S45, -_S45), (0.0, 1.0), (_S45, -_S45), (-1.0, 0.0), (_S45, _S45), (0.0, -1.0), (-_S45, _S45)), np.float64)


def lanczos4_side_tables(sides, dst: int = FACE_SIZE):
    """upscaler.lanczos4_tables(side, dst) for every side of `sides` at once: (ofs int32 [len, dst], coef int16 [len, dst, 8]), bit for bit
    (the same float / double operations in numpy; the one sine and cosine of an entry come from math, as there: numpy's need not be
    bit-equal to them)."""
    f32 = np.float32
    sides = np.asarray(sides, np.float64)
    scale = 1.0 / (float(dst) / sides)
    f = ((np.arange(dst, dtype=np.float64)[None, :] + 0.5) * scale[:, None] - 0.5).astype(f32)
    s = np.floor(f)
    x = (f - s).astype(f32)
    x3 = x + f32(3)
    y0 = (-x3).astype(np.float64) * math.pi * 0.25
    flat = y0.ravel().tolist()
    s0 = np.array([math.sin(v) for v in flat], np.float64).reshape(y0.shape)
    c0 = np.array([math.cos(v) for v in flat], np.float64).reshape(y0.shape)
    coeffs = np.empty(x.shape + (8,), f32)
    total = np.zeros(x.shape, f32)
    for i in range(8):
        yi = (x3 - f32(i)).astype(f32)
        y = (-yi).astype(np.float64) * math.pi * 0.25
        with np.errstate(divide="ignore", invalid="ignore"):
            c = ((_CS[i][0] * s0 + _CS[i][1] * c0) / (y * y)).astype(f32)
        c = np.where(np.abs(yi) >= f32(1e-6), c, f32(1e30)).astype(f32)
        coeffs[..., i] = c
        total = (total + c).astype(f32)
    inv = (f32(1) / total).astype(f32)
    coeffs = (coeffs * inv[..., None]).astype(f32)
    coef = np.clip(np.rint((coeffs * f32(2048)).astype(f32)), -32768, 32767).astype(np.int16)
    return (s.astype(np.int64) - 3).astype(np.int32), coef


def area_side_tables(sides, dst: int = FACE_SIZE, taps: int = TAPS):
    """openpose.area_tables(side, dst, dst / side) for every side >= dst of `sides` at once: (ofs int32 [len, dst], cnt int32 [len, dst],
    w float32 [len, dst, taps]) with scale = side / dst, as cv2.resize computes it from the two sizes (taps: 8 here; the hand stage, whose
    smallest input is 184 pixels, takes up to 16)."""
    sides = np.asarray(sides, np.int64)
    assert (sides >= dst).all()
    src = sides.astype(np.float64)[:, None]
    scale = src / float(dst)
    f1 = np.arange(dst, dtype=np.float64)[None, :] * scale
    f2 = f1 + scale
    cell = np.minimum(scale, src - f1)
    s1, s2 = np.ceil(f1).astype(np.int64), np.floor(f2).astype(np.int64)
    s2 = np.minimum(s2, sides[:, None] - 1)
    s1 = np.minimum(s1, s2)
    first = (s1 - f1 > 1e-3)
    last = (f2 - s2 > 1e-3)
    full = s2 - s1
    cnt = first.astype(np.int64) + full + last
    if cnt.max() > taps or cnt.min() < 1:
        raise NotImplementedError(f"INTER_AREA to {dst}: {cnt.min()} .. {cnt.max()} taps (1 .. {taps} are taken)")
    wfirst = ((s1 - f1) / cell).astype(np.float32)
    wfull = (1.0 / cell).astype(np.float32)
    wlast = (np.minimum(np.minimum(f2 - s2, 1.0), cell) / cell).astype(np.float32)
    j = np.arange(taps)[None, None, :] - first[..., None]   # index among the full taps; -1: the first partial tap
    w = np.where(j < 0, wfirst[..., None], np.where(j < full[..., None], wfull[..., None], np.where((j == full[..., None]) & last[..., None], wlast[..., None], 0)))
    w = np.where(np.arange(taps)[None, None, :] < cnt[..., None], w, 0).astype(np.float32)
    return (s1 - first).astype(np.int32), cnt.astype(np.int32), np.ascontiguousarray(w)


@functools.lru_cache(maxsize=4)
def resize_tables(side_max: int) -> dict:
    """One table per admissible crop side of an axis, for frames whose larger side is side_max: INTER_LANCZOS4 for MIN_SIDE .. side_max,
    INTER_AREA for FACE_SIZE .. side_max (11.7 MB at side_max = 768).  Built once per side_max.  ca_face_crop keeps the horizontal sums of
    the source rows under a pair of output rows in LDS, SPAN_ROWS of them: that every table a slot can use stays within it is checked here
    (LANCZOS4 is chosen when Hc + Wc <= 768 only, so its sides beyond 768 - MIN_SIDE are never used)."""
    side_max = max(int(side_max), FACE_SIZE)
    lz_ofs, lz_coef = lanczos4_side_tables(np.arange(MIN_SIDE, side_max + 1))
    ar_ofs, ar_cnt, ar_w = area_side_tables(np.arange(FACE_SIZE, side_max + 1))
    used = min(side_max, 2 * FACE_SIZE - MIN_SIDE) - MIN_SIDE + 1
    top = np.arange(MIN_SIDE, MIN_SIDE + used)[:, None] - 1
    lz_span = np.clip(lz_ofs[:used, 1::2] + TAPS - 1, 0, top) - np.clip(lz_ofs[:used, 0::2], 0, top) + 1
    ar_span = (ar_ofs[:, 1::2] + ar_cnt[:, 1::2] - 1) - ar_ofs[:, 0::2] + 1
    if max(int(lz_span.max()), int(ar_span.max())) > SPAN_ROWS:
        raise NotImplementedError(f"resize tables up to side {side_max}: a pair of output rows spans {int(lz_span.max())} (LANCZOS4) / "
                                  f"{int(ar_span.max())} (AREA) source rows, ca_face_crop holds {SPAN_ROWS}")
    return {"lz_ofs": lz_ofs, "lz_coef": lz_coef, "ar_ofs": ar_ofs, "ar_cnt": ar_cnt, "ar_w": ar_w, "side_max": side_max}


def pixel_map(side: int) -> np.ndarray:
    """draw_facepose's coordinate of a pixel p of an axis of `side` pixels, int32 [side]: int(float32(float32(p) / side) * side)."""
    p = np.arange(side, dtype=np.float32)
    return ((p / np.float32(side)).astype(np.float32) * np.float32(side)).astype(np.float32).astype(np.int32)


# ---- packing -----------------------------------------------------------------------------------------------------------------------------
def pack_mconv1(w):
    """Mconv1's weight [128, 199, 7, 7] on input channels [heat 71 | features 128] -> [128, 7, 7, 224] on [features 128 | heat 71, 25 zeros]."""
    return _body.pack_mconv1(w, ((FACE_PARTS, CAT - 128),))


def pack_face_weights(sd, dtype) -> dict:
    return _body.pack_crop_cpm_weights(sd, dtype, FRONT, FACE_PARTS, FACE_MAPS, CAT - 128)


class FaceStage(_body.CropStage):
    """The face stage of one OpenposeAnnotator (`owner`: its dtype, max_activation_bytes and timings are used).  `run` starts from given
    keypoints and people tensors, so tests -- and a later hand stage -- can plant them."""

    WEIGHTS_NAME = WEIGHTS_NAME

    def __init__(self, owner, state_dict_or_path, max_faces: int = 2):
        if not 1 <= int(max_faces) <= 64:
            raise ValueError(f"max_faces={max_faces} (1 .. 64)")
        sd = self._load(state_dict_or_path) if isinstance(state_dict_or_path, (str, os.PathLike)) else state_dict_or_path
        sd = bare_keys(sd)
        check_face_state_dict(sd)
        self.owner, self.max_faces = owner, int(max_faces)
        self._host = pack_face_weights(sd, owner.dtype)   # packed once, on the host
        self._ws = {}

    def chunk_crops(self, direct: bool) -> int:
        """Crops per pass through the network: as many as keep the largest 16-bit operand (conv1's output, or the im2col tensor of the
        alternative form of the 7x7 convolutions) within the owner's max_activation_bytes."""
        per_crop = max(FACE_SIZE * FACE_SIZE * 64 * 2, 0 if direct else FACE_HEAT * FACE_HEAT * 49 * CAT * 2)
        limit = self.max_activation_bytes
        if per_crop > limit:
            raise ValueError(f"a face crop alone exceeds what the kernels address ({per_crop} > {limit} bytes)")
        return limit // per_crop

    def workspace(self, n: int, h: int, w: int, dev) -> dict:
        """The buffers of a call with n frames of h x w pixels, cached per (n, h, w): the resize tables and pixel maps on the device, the
        boxes / slots / points / overflow, the network's fp32 output, and the pool of activation buffers with its take / give plan."""
        import torch
        from . import kernels as K

        def make(dev):
            tables = {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in resize_tables(max(h, w)).items()}
            return {"tables": tables, "xmap": torch.from_numpy(pixel_map(w)).to(dev), "ymap": torch.from_numpy(pixel_map(h)).to(dev),
                    "buf": K.face_buffers(n, self.max_faces, dev),
                    "heat": torch.empty((n * self.max_faces, FACE_HEAT, FACE_HEAT, FACE_MAPS), dtype=torch.float32, device=dev)}

        return self._workspace((n, h, w, str(dev)), make, dev)

    def _network(self, src, ws, c0: int, nc: int, direct: bool) -> None:
        """Crops c0 .. c0 + nc - 1 of the frames `src`: the resized input and the network, the 72 maps into ws["heat"][c0 : c0 + nc]."""
        from . import kernels as K

        def crop(out):
            return K.face_crop(src, ws["buf"]["slots"], ws["tables"], out, first=c0)

        self._cpm_network(ws, self._weights(src.device), "face", FRONT, crop, nc, FACE_SIZE, FACE_HEAT, CAT,
                          ws["heat"][c0:c0 + nc].view(nc * FACE_HEAT * FACE_HEAT, FACE_MAPS), direct)

    def run(self, src, keypoints, people, overflow_in=None, direct: bool = True) -> dict:
        """frames uint8 [n, H, W, 3] on the device, keypoints int32 [n, 64, 18, 2], people int32 [n] (and the body's overflow int32 [n]) ->
        the stage's workspace: ["buf"] holds boxes, slots, points and overflow, ["heat"] the maps, ["xmap"] / ["ymap"] the draw's tables."""
        from . import kernels as K
        n, h, w, _ = src.shape
        ws = self.workspace(n, h, w, src.device)
        total = n * self.max_faces
        step = self.chunk_crops(direct)
        if ws["planned"] and (bool(ws.get("direct", True)) != bool(direct) or min(step, total) > ws.get("chunk", 0)):
            ws["pool"], ws["plan"], ws["planned"] = [], [], False   # the other form of the 7x7 convolutions, or a larger chunk than was planned
        ws["direct"] = bool(direct)
        ws["chunk"] = max(ws.get("chunk", 0), min(step, total)) if ws["planned"] else min(step, total)
        self._timed("face_boxes", K.face_boxes, keypoints, people, h, w, ws["buf"], overflow_in)
        for c0, sl in self._chunks(total, step):
            self._network(src, ws, c0, sl.stop - c0, direct)
        self._timed("face_peaks", K.face_peaks, ws["heat"], ws["buf"]["slots"], ws["buf"]["points"], h, w)
        return ws
