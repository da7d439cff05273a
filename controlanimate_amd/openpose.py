"""The OpenPose body annotator of the reference's sample configs (SampleConfig.yaml, SampleConfigLCMLoRA.yaml and SampleConfigIPAdapter.yaml
list lllyasviel/control_v11p_sd15_openpose as their first ControlNet; their control frames come from controlnet_aux's OpenposeDetector,
modules/controlresiduals_pipeline.py:57, 107-113) on the GPU, for a whole window of frames at once.

The reference calls the detector with hand_and_face=True, which additionally runs a hand network and a face network on crops around
the detected body.  Without further weights this annotator draws the BODY skeleton only.  Given a face network
(`OpenposeAnnotator(body, face=<state dict or facenet.pth>)`) it also draws the 71 face points of the first `max_faces` people of a
frame: the face stage is openpose_face.py (its head describes it; `faces()` returns its points and boxes).  Given a hand network
(`hand=<state dict or hand_pose_model.pth>`) it also draws the hands of the first `max_hands` wrist boxes of a frame (20 edges and 21
circles each): the hand stage is openpose_hand.py (`hands()` returns its points and boxes).  With both networks the drawing is the
reference's hand_and_face=True: per person the body, the left hand, the right hand, the face.  `include_hand=True` without a hand
network raises NotImplementedError, and so does `include_face=True` without a face network.

The detector's body part, as the reference calls it (detect_resolution = image_resolution = 512):

    input    BGR, cv2.resize(fx = fy = 0.5 * 368 / H, INTER_AREA), padded right and below to multiples of 8 with 128, x / 256 - 0.5
    network  bodypose_model: a VGG-19 front end (conv1_1 .. conv4_2, conv4_3_CPM, conv4_4_CPM; 3x3 + ReLU, three 2x2 max pools) to 128
             features at 1/8; stage 1 with two branches L1 (38 PAF channels) and L2 (19 heat channels): three 3x3 128 -> 128, 1x1 128 -> 512,
             1x1 512 -> 38 | 19; stages 2 .. 6 on cat([L1, L2, features]) (185 channels): five 7x7 to 128 channels, 1x1 128 -> 128, 1x1 128 ->
             38 | 19; ReLU after every layer but a stage's last
    maps     both outputs resized x8 (INTER_LANCZOS4), cropped by the padding, resized to H x W (INTER_LANCZOS4)
    peaks    per part 0 .. 17: gaussian_filter(sigma = 3) (reflect), a peak where the smoothed value is >= its four neighbours (zero outside)
             and > 0.1, in row-major order, the score read from the unsmoothed map
    limbs    19 part pairs: per candidate pair 10 samples of the PAF along the segment, mean(paf . unit) + min(0.5 H / norm - 1, 0), kept
             when more than 80 % of the samples exceed 0.05 and the score is positive; sorted by score (stable), matched greedily
    people   the subset table (found == 1, found == 2 merge / extend, new row for the first 17 limbs); rows with fewer than 4 parts or
             score / parts < 0.4 deleted; keypoints x / float(W), y / float(H)
    draw     per person 17 limbs (cv2.ellipse2Poly + fillConvexPoly, colour int(c * 0.6)), then 18 circles of radius 4

It runs as (the names are the keys of `timings`, the numbers the launches of that name per pass in the default form):

    prep       1   ca_pose_prep: uint8 frames -> 8 channels (conv1_1's weight is zero-padded to 8 input channels)
    conv       18  ca_conv3x3 with CA_ACT_RELU: the front end and the three 3x3 layers of each branch of stage 1
    pool       3   ca_maxpool2x2
    copy       1   ca_copy_cols: the features into columns 0 .. 127 of the 192-wide concatenation [features | L1, 2 zeros | L2, 5 zeros]
                   (Mconv1's weights are permuted and zero-padded to that layout; every later stage output is written there by its GEMM
                   through ldc and a column offset: no torch.cat)
    pointwise  24  ca_gemm: the 1x1 layers; a stage's last one writes into the concatenation, the sixth stage's into the fp32 maps
    conv7      25  ca_conv7x7: Mconv1 .. Mconv5 of BOTH branches in one launch each (context.dispatch.pose_conv7_direct; off:
                   ca_im2col7x7 + ca_gemm per branch)
    maps       1   ca_pose_maps -> raw heat, smoothed heat and PAF at full resolution, fp32
    peaks      1   ca_pose_peaks
    connect    1   ca_pose_connect
    assemble   1   ca_pose_assemble
    draw       1   ca_pose_draw -> the uint8 skeleton and / or the control tensor the ControlNets hold

No device-to-host read anywhere, the skeleton assembly included: the chain can be captured in a hipGraph.

The specification is tests/pose_ref.py (the fp32 torch network and the numpy / float64 decode and rasterisers).  Key names and arithmetic
are restated from memory of the published code (controlnet_aux 0.0.6 open_pose/{__init__,body,util}.py, pytorch-openpose's
bodypose_model, OpenCV's resize, ellipse2Poly, fillConvexPoly and circle) and are UNPINNED: controlnet_aux, OpenCV and scipy are
third-party packages that are absent here, and no body_pose_model.pth is available.

Two caps the published code does not have (deliberate): at most CA_POSE_MAX_PEAKS = 64 peaks per part and frame (the first 64 in
row-major order) and at most CA_POSE_MAX_PEOPLE = 64 rows of the subset table.  Where either is exceeded the bit is set in `overflow`
and the result is the specification's under the same cap.  Where three or more rows share a connection's end the published code raises
an IndexError; here the connection is skipped.

Scope of sizes: min(H, W) == detect_resolution == image_resolution, H and W multiples of 64, H >= 192 (the image resize is then always
the INTER_AREA branch) and H no multiple of 184 (OpenCV's integer-scale fast path rounds differently); H, W <= 2048.  At the default 512
that admits 512 x 512, 512 x 768 and 768 x 512.  Anything else raises NotImplementedError.
"""
from __future__ import annotations

import math
import os
import re

import numpy as np

from .annotator_base import AnnotatorBase, PackedNetwork, check_state_dict as _check_state_dict, pack_conv, pack_pointwise

WEIGHTS_NAME = "body_pose_model.pth"
MAX_PEAKS, MAX_PEOPLE, AREA_TAPS = 64, 64, 8
OVERFLOW_PEAKS, OVERFLOW_PEOPLE = 1, 2
OVERFLOW_FACES, OVERFLOW_FACE_RESIZE = 4, 8   # the face stage (openpose_face.py)
OVERFLOW_HANDS, OVERFLOW_HAND_RESIZE = 16, 32   # the hand stage (openpose_hand.py)
BOXSIZE, STRIDE = 368, 8
STAGES = {"prep": 1, "conv": 18, "pool": 3, "copy": 1, "pointwise": 24, "conv7": 25, "maps": 1, "peaks": 1, "connect": 1, "assemble": 1, "draw": 1}

# the front end: (name, cin, cout) or "pool"
FRONT = (("conv1_1", 3, 64), ("conv1_2", 64, 64), "pool", ("conv2_1", 64, 128), ("conv2_2", 128, 128), "pool", ("conv3_1", 128, 256),
         ("conv3_2", 256, 256), ("conv3_3", 256, 256), ("conv3_4", 256, 256), "pool", ("conv4_1", 256, 512), ("conv4_2", 512, 512),
         ("conv4_3_CPM", 512, 256), ("conv4_4_CPM", 256, 128))
BRANCH_OUT = {1: 38, 2: 19}


def pose_key_shapes() -> dict:
    """Every tensor of body_pose_model.pth: bare layer name -> shape."""
    out = {}

    def add(name, cout, cin, k):
        out[f"{name}.weight"], out[f"{name}.bias"] = (cout, cin, k, k), (cout,)

    for layer in FRONT:
        if layer != "pool":
            add(layer[0], layer[2], layer[1], 3)
    for br, c in BRANCH_OUT.items():
        for i in (1, 2, 3):
            add(f"conv5_{i}_CPM_L{br}", 128, 128, 3)
        add(f"conv5_4_CPM_L{br}", 512, 128, 1)
        add(f"conv5_5_CPM_L{br}", c, 512, 1)
        for t in range(2, 7):
            add(f"Mconv1_stage{t}_L{br}", 128, 185, 7)
            for i in (2, 3, 4, 5):
                add(f"Mconv{i}_stage{t}_L{br}", 128, 128, 7)
            add(f"Mconv6_stage{t}_L{br}", 128, 128, 1)
            add(f"Mconv7_stage{t}_L{br}", c, 128, 1)
    return out


_PREFIX = re.compile(r"^model\d+(_\d+)?\.")


def bare_keys(sd) -> dict:
    """The checkpoint under its bare layer names: 'model0.conv1_1.weight' / 'model3_2.Mconv1_stage3_L2.weight' lose the module prefix
    (the body's, the face's and the hand's checkpoints alike)."""
    return {_PREFIX.sub("", k): v for k, v in sd.items()}


def check_state_dict(sd) -> None:
    """KeyError naming a missing tensor, ValueError naming one that is unexpected or has the wrong shape (bare names)."""
    _check_state_dict(sd, pose_key_shapes(), "openpose", "the layers of bodypose_model")


# ---- packing (the body's network and the face and hand stages') ----------------------------------------------------------------------
def pack_mconv1(w, heads):
    """Mconv1's weight [128, maps + 128, 7, 7] on input channels [each head's maps | features 128] -> [128, 7, 7, 128 + columns] on
    [features 128 | each head's maps, zero-padded to its columns of the concatenation]; heads: ((maps, columns), ...)."""
    import torch
    maps = sum(m for m, _ in heads)
    z = torch.zeros((w.shape[0], 128 + sum(c for _, c in heads), 7, 7), dtype=w.dtype)
    z[:, 0:128] = w[:, maps:maps + 128]
    src, dst = 0, 128
    for m, c in heads:
        z[:, dst:dst + m] = w[:, src:src + m]
        src, dst = src + m, dst + c
    return z.permute(0, 2, 3, 1).contiguous()


def cpm_packers(sd, dtype, heads):
    """(conv, lin, mconv1): the layers of a CPM network out of the state dict `sd` (bare names) as (weight in `dtype`, fp32 bias) in the
    kernels' layouts; heads: the concatenation's layout behind the features, as pack_mconv1 takes it."""
    def wb(name):
        return sd[name + ".weight"].detach().float(), sd[name + ".bias"].detach().float().contiguous()

    def conv(name, pad_in=0):  # [Cout, Cin, k, k] -> [Cout, k, k, Cin (+ pad_in zero channels)]
        w, b = wb(name)
        return pack_conv((w, b), dtype, cin_pad=w.shape[1] + pad_in)

    def lin(name, pad_out=0):  # [Cout, Cin, 1, 1] -> [Cout + pad_out zero rows, Cin]
        w, b = wb(name)
        return pack_pointwise((w, b), dtype, cout_pad=w.shape[0] + pad_out)

    def mconv1(name):
        w, b = wb(name)
        return pack_mconv1(w, heads).to(dtype), b

    return conv, lin, mconv1


def pack_crop_cpm_weights(sd, dtype, front, maps: int, rows: int, columns: int) -> dict:
    """The one-branch CPM network of the face and hand stages, packed: `maps` heat maps, written as `rows` GEMM rows (zero-padded: the
    GEMM stores 16-byte chunks) into `columns` columns of the concatenation behind the 128 features."""
    conv, lin, mconv1 = cpm_packers(sd, dtype, ((maps, columns),))
    pad = rows - maps
    return {"front": [None if l == "pool" else conv(l[0], 5 if l[0] == "conv1_1" else 0) for l in front],
            "stage1": {"fc": lin("conv6_1_CPM"), "out": lin("conv6_2_CPM", pad)},
            "stages": [{"conv7": [mconv1(f"Mconv1_stage{t}")] + [conv(f"Mconv{i}_stage{t}") for i in (2, 3, 4, 5)],
                        "fc": lin(f"Mconv6_stage{t}"), "out": lin(f"Mconv7_stage{t}", pad)} for t in range(2, 7)]}


class CropStage(PackedNetwork):
    """A stage of one OpenposeAnnotator (`owner`) that runs a one-branch CPM network on crops around its keypoints: it runs in the
    owner's dtype, on its device, within its max_activation_bytes, and its launches are stages of the owner's `timings`.  The four are
    read through to the owner and cannot be set on the stage: set them on the annotator."""

    dtype = property(lambda self: self.owner.dtype)
    device = property(lambda self: self.owner.device)
    timings = property(lambda self: self.owner.timings)
    max_activation_bytes = property(lambda self: self.owner.max_activation_bytes)

    def _cpm_network(self, ws, wts, prefix: str, front, crop, nc: int, side: int, hl: int, cat_cols: int, out2d, direct: bool) -> None:
        """The CPM network for `nc` crops of side x side pixels, from the crop launch onward: the front end, the feature copy into the
        concatenation [features 128 | heat | zeros] of `cat_cols` columns at hl x hl, stage 1 and the five 7x7 stages, the last of which
        writes the fp32 view out2d [nc * hl * hl, heat columns].  crop(out): the stage's crop launch into out [nc, side, side, 8];
        prefix: "face" / "hand", in front of the stage names; ws: the dict that holds the pool and its plan (the buffer plan and the
        per-stage launch counts depend on the order of the takes, gives and launches below)."""
        from . import kernels as K
        with self._pass(ws, out2d.device) as p:   # the body's buffer plan: the same buffers in the same order on every pass
            take, give, launch = p.take, p.give, p.launch

            def pw(x2d, wb, act, out2d, out_f32=False):
                p.pointwise(prefix + "_pointwise", x2d, wb, act, out2d=out2d, out_f32=out_f32)

            x = launch(prefix + "_crop", crop, take(nc, side, side, 8))
            for layer, wb in zip(front, wts["front"]):
                if layer == "pool":
                    y = launch(prefix + "_pool", K.maxpool2x2, x, take(nc, x.shape[1] // 2, x.shape[2] // 2, x.shape[3]))
                else:   # split_k=False: the order of an output's sum is then the same whatever the number of crops
                    y = p.conv3x3(prefix + "_conv", x, wb, act=K.ACT_RELU, split_k=False)
                give(x)
                x = y
            feat = x
            rows = nc * hl * hl
            cat = take(nc, hl, hl, cat_cols)
            cat2d = cat.view(rows, cat_cols)
            cat2d.zero_()   # the columns behind the heat maps are read (against zero weights) and never written
            launch(prefix + "_copy", K.copy_cols, feat.view(rows, 128), cat2d, 0)
            heat_cols = cat2d[:, 128:128 + out2d.shape[1]]
            fc = take(rows, 512)
            pw(feat, wts["stage1"]["fc"], K.ACT_RELU, fc)
            give(feat)
            pw(fc, wts["stage1"]["out"], K.ACT_NONE, heat_cols)
            give(fc)
            cols = None if direct else take(rows, 49 * cat_cols)
            for t, stage in enumerate(wts["stages"]):
                a = cat
                for i in range(5):
                    y = take(nc, hl, hl, 128)
                    launch(prefix + "_conv7", K.conv7x7, [a], [stage["conv7"][i][0]], biases=[stage["conv7"][i][1]], relu=True, outs=[y], direct=direct, cols=cols)
                    if i:
                        give(a)
                    a = y
                fc = take(rows, 128)
                pw(a, stage["fc"], K.ACT_RELU, fc)
                give(a)
                if t == len(wts["stages"]) - 1:
                    pw(fc, stage["out"], K.ACT_NONE, out2d, out_f32=True)
                else:
                    pw(fc, stage["out"], K.ACT_NONE, heat_cols)
                give(fc)
            if cols is not None:
                give(cols)
            give(cat)


# ---- host-side tables ------------------------------------------------------------------------------------------------------------

def geometry(h: int, w: int) -> dict:
    """The sizes of Body.__call__ for an h x w frame: the scale, the resized size (cvRound of the product), the padded size, the maps' size."""
    scale = 0.5 * BOXSIZE / h
    hs, ws = int(round(h * scale)), int(round(w * scale))
    hp, wp = -(-hs // STRIDE) * STRIDE, -(-ws // STRIDE) * STRIDE
    return {"scale": scale, "hs": hs, "ws": ws, "hp": hp, "wp": wp, "hl": hp // STRIDE, "wl": wp // STRIDE}


def area_tables(src: int, dst: int, fx: float, dtype=np.float32):
    """OpenCV's computeResizeAreaTab for one axis of cv2.resize(fx = fx, INTER_AREA), src -> dst pixels, scale = 1 / fx: per destination
    index the first source index, the number of taps and their float32 weights (ofs int32 [dst], cnt int32 [dst], w float32 [dst, 8]).
    dtype=np.float64 gives the weights before OpenCV stores them as float: those sum to 1 within 1e-12."""
    scale = 1.0 / fx
    ofs, cnt, wgt = np.zeros(dst, np.int32), np.zeros(dst, np.int32), np.zeros((dst, AREA_TAPS), dtype)
    for d in range(dst):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, src - f1)
        s1, s2 = int(math.ceil(f1)), int(math.floor(f2))
        s2 = min(s2, src - 1)
        s1 = min(s1, s2)
        taps = []
        if s1 - f1 > 1e-3:
            taps.append((s1 - 1, dtype((s1 - f1) / cell)))
        for s in range(s1, s2):
            taps.append((s, dtype(1.0 / cell)))
        if f2 - s2 > 1e-3:
            taps.append((s2, dtype(min(min(f2 - s2, 1.0), cell) / cell)))
        if not taps or len(taps) > AREA_TAPS or any(b[0] != a[0] + 1 for a, b in zip(taps, taps[1:])) or taps[0][0] < 0 or taps[-1][0] >= src:
            raise NotImplementedError(f"INTER_AREA {src} -> {dst}: {len(taps)} taps at index {d} (1 .. {AREA_TAPS} consecutive ones are taken)")
        ofs[d], cnt[d] = taps[0][0], len(taps)
        wgt[d, :len(taps)] = [t[1] for t in taps]
    return ofs, cnt, wgt


def lanczos4_matrix(src: int, dst: int, scale: float) -> np.ndarray:
    """cv2.resize(INTER_LANCZOS4) of float data along one axis as a float64 matrix [dst, src]: f = float((d + 0.5) * scale - 0.5), eight
    float32 coefficients at floor(f) - 3 .. + 4, indices clamped to the axis (the clamped taps add up in the edge columns).  OpenCV's
    eight float coefficients sum to 1 within 1e-7 only; a row is renormalised in float64, so that a constant map stays constant."""
    from .upscaler import _lanczos4_coeffs
    m = np.zeros((dst, src), np.float64)
    for d in range(dst):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(math.floor(f))
        for k, c in enumerate(_lanczos4_coeffs(np.float32(f - np.float32(s)))):
            m[d, min(max(s - 3 + k, 0), src - 1)] += float(c)
    return m / m.sum(axis=1, keepdims=True)


def gaussian_taps(sigma: float = 3.0, truncate: float = 4.0) -> np.ndarray:
    """scipy.ndimage.gaussian_filter1d's weights: radius int(truncate * sigma + 0.5) = 12, exp(-x^2 / (2 sigma^2)) normalised to sum 1."""
    r = int(truncate * sigma + 0.5)
    x = np.arange(-r, r + 1, dtype=np.float64)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def gaussian_matrix(n: int) -> np.ndarray:
    """The sigma-3 filter along an axis of n samples with scipy's mode 'reflect' (d c b a | a b c d | d c b a) as a float64 matrix [n, n]."""
    g = gaussian_taps()
    r = len(g) // 2
    m = np.zeros((n, n), np.float64)
    for i in range(n):
        for t in range(-r, r + 1):
            j = (i + t) % (2 * n)
            j = j if j < n else 2 * n - 1 - j
            m[i, j] += g[t + r]
    return m


def axis_matrices(full: int, resized: int, padded: int):
    """(A, G A) float64 [full, padded / 8] of one axis: A = R2 . crop . R1 with R1 the x8 LANCZOS4 resize of the padded / 8 network
    samples (cv2.resize(fx = 8): scale 1 / 8), the crop to the resized size, R2 the LANCZOS4 resize to the frame (scale = 1 / (full /
    resized)); G the Gaussian."""
    low = padded // STRIDE
    r1 = lanczos4_matrix(low, padded, 1.0 / float(STRIDE))
    r2 = lanczos4_matrix(resized, full, 1.0 / (float(full) / float(resized)))
    a = r2 @ r1[:resized]
    return a, gaussian_matrix(full) @ a


def sin_table() -> np.ndarray:
    """OpenCV's SinTable: sin of 0 .. 450 degrees as float literals of seven decimals."""
    return np.round(np.sin(np.deg2rad(np.arange(451, dtype=np.float64))), 7).astype(np.float32)


class OpenposeAnnotator(AnnotatorBase):
    """`OpenposeAnnotator(weights)(image)` has the contract of `annotators.canny(image)` (PIL in, PIL RGB out; an array in, an array out),
    so it plugs into `MultiControlNetResidualsPipeline(annotators={"openpose": OpenposeAnnotator.from_pretrained(path)})`, whose
    `prep_control_images` then calls `annotate_batch` once per list of frames.  Nothing makes it a default: the weights are the user's
    file.  It draws the body skeleton, and the faces when a face network is given (see the module's head).  Non-uint8 input raises TypeError, frames of different sizes
    ValueError, sizes out of scope NotImplementedError -- all before the device is touched; without the library or a GPU a call raises
    CAHipUnavailable (there is no CPU fallback).  `from_pretrained(path, face=<a local facenet.pth or a directory that holds it>)` adds the
    face stage, `hand=<a local hand_pose_model.pth or its directory>` the hand stage (hands())."""

    WEIGHTS_NAME = WEIGHTS_NAME
    STAGES = STAGES

    def __init__(self, state_dict_or_path, device=None, dtype=None, detect_resolution: int = 512, image_resolution: int = 512,
                 include_hand=None, include_face=None, face=None, max_faces: int = 2, hand=None, max_hands: int = 2):
        import torch
        dtype = torch.float16 if dtype is None else dtype
        if dtype not in (torch.float16, torch.bfloat16):
            raise TypeError(f"dtype must be torch.float16 or torch.bfloat16, got {dtype}")
        include_hand = hand is not None if include_hand is None else bool(include_hand)   # with `hand` given, hands are drawn by default
        if include_hand and hand is None:
            raise NotImplementedError("include_hand=True, but no hand network was given: pass hand=<state dict, hand_pose_model.pth or the "
                                      "directory that holds it> (nothing is ever downloaded)")
        include_face = face is not None if include_face is None else bool(include_face)   # with `face` given, faces are drawn by default
        if include_face and face is None:
            raise NotImplementedError("include_face=True, but no face network was given: pass face=<state dict, facenet.pth or the directory "
                                      "that holds it> (nothing is ever downloaded)")
        if detect_resolution != image_resolution or detect_resolution < 192 or detect_resolution % 64:
            raise NotImplementedError(f"OpenposeAnnotator takes detect_resolution == image_resolution, a multiple of 64 and >= 192; got "
                                      f"{detect_resolution} and {image_resolution}")
        sd = self._load(state_dict_or_path) if isinstance(state_dict_or_path, (str, os.PathLike)) else state_dict_or_path
        sd = bare_keys(sd)
        check_state_dict(sd)
        self.device, self.dtype, self.resolution = device, dtype, int(detect_resolution)
        # Mconv1's input channels [L1 38 | L2 19 | features 128] -> [features 128 | L1 38, 2 zeros | L2 19, 5 zeros]
        conv, lin, mconv1 = cpm_packers(sd, dtype, ((38, 40), (19, 24)))
        pad_n = {1: 2, 2: 5}  # 38 -> 40, 19 -> 24 output columns: the GEMM stores 16-byte chunks
        # packed once, on the host
        self._host = {"front": [None if l == "pool" else conv(l[0], 5 if l[0] == "conv1_1" else 0) for l in FRONT],
                      "stage1": [{"conv": [conv(f"conv5_{i}_CPM_L{br}") for i in (1, 2, 3)], "fc": lin(f"conv5_4_CPM_L{br}"),
                                  "out": lin(f"conv5_5_CPM_L{br}", pad_n[br])} for br in (1, 2)],
                      "stages": [[{"conv7": [mconv1(f"Mconv1_stage{t}_L{br}")] + [conv(f"Mconv{i}_stage{t}_L{br}") for i in (2, 3, 4, 5)],
                                   "fc": lin(f"Mconv6_stage{t}_L{br}"), "out": lin(f"Mconv7_stage{t}_L{br}", pad_n[br])} for br in (1, 2)]
                                 for t in range(2, 7)]}
        self._ws = {}   # (`timings` receives events under the keys of STAGES -- tools/bench_openpose.py)
        self._tables = {}
        self._face = None
        if include_face:
            from .openpose_face import FACE_STAGES, FaceStage
            self._face = FaceStage(self, face, max_faces)   # (its key and shape checks come before the device is touched, like the body's)
            self.STAGES = {**STAGES, **FACE_STAGES}
        self._hand = None
        if include_hand:
            from .openpose_hand import HAND_STAGES, HandStage
            self._hand = HandStage(self, hand, max_hands)   # (key and shape checks before the device is touched)
            self.STAGES = {**self.STAGES, **HAND_STAGES}

    # ---- device state ----------------------------------------------------------------------------------------------------------
    def host_tables(self, h: int, w: int) -> dict:
        """The host-side tables of an h x w frame (cached): the geometry, the AREA tables of both axes, the float64 composite matrices
        (ax, gax [w, wl]; ay, gay [h, hl]) and OpenCV's sine table."""
        key = (h, w)
        if key not in self._tables:
            g = geometry(h, w)
            ax, gax = axis_matrices(w, g["ws"], g["wp"])
            ay, gay = axis_matrices(h, g["hs"], g["hp"])
            self._tables[key] = {"geometry": g, "area_x": area_tables(w, g["ws"], g["scale"]), "area_y": area_tables(h, g["hs"], g["scale"]),
                                 "ax": ax, "gax": gax, "ay": ay, "gay": gay, "sin": sin_table()}
        return self._tables[key]

    def chunk_frames(self, h: int, w: int) -> int:
        """Frames per pass through the network: as many as keep the largest 16-bit operand (conv1's output, or the im2col tensor of the
        alternative form of the 7x7 convolutions) within max_activation_bytes."""
        g = geometry(h, w)
        per_frame = max(g["hp"] * g["wp"] * 64 * 2, g["hl"] * g["wl"] * 49 * 192 * 2)
        if per_frame > self.max_activation_bytes:
            raise ValueError(f"a {h} x {w} frame alone exceeds what the kernels address ({per_frame} > {self.max_activation_bytes} bytes)")
        return self.max_activation_bytes // per_frame

    def workspace(self, n: int, h: int, w: int) -> dict:
        """The buffers of a call with n frames of h x w pixels, cached per (n, h, w): the device tables, the network's fp32 output
        [n, hl, wl, 64], the three full-resolution maps, the decode's buffers, the draw's index plane, and a pool of activation buffers
        that the layers of a pass take and give back in a fixed order (contents are never assumed; the first pass allocates them and
        every later pass reuses the same ones)."""
        import torch
        from . import kernels as K

        def make(dev):
            t = self.host_tables(h, w)
            g = t["geometry"]
            f32 = dict(dtype=torch.float32, device=dev)
            tables = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (*t["area_x"], *t["area_y"]))
            return {"geometry": g, "area": tables,
                    "mx": torch.from_numpy(np.stack([t["ax"], t["gax"]]).astype(np.float32)).to(dev),
                    "my": torch.from_numpy(np.stack([t["ay"], t["gay"]]).astype(np.float32)).to(dev),
                    "sin": torch.from_numpy(t["sin"]).to(dev),
                    "low": torch.empty((n, g["hl"], g["wl"], 64), **f32),
                    "raw": torch.empty((n, 18, h, w), **f32), "smooth": torch.empty((n, 18, h, w), **f32), "paf": torch.empty((n, 38, h, w), **f32),
                    "maps_ws": torch.empty(K.pose_maps_workspace_bytes(n, g["hl"], w), dtype=torch.uint8, device=dev),
                    "decode": K.pose_decode_buffers(n, dev), "index": torch.empty((n, h, w), dtype=torch.int32, device=dev)}

        return self._workspace((n, h, w), make)

    # ---- input checks ----------------------------------------------------------------------------------------------------------
    def _check_size(self, h: int, w: int) -> None:
        r = self.resolution
        if min(h, w) != r or h % 64 or w % 64 or h < 192 or h % 184 == 0 or max(h, w) > 2048:
            raise NotImplementedError(
                f"OpenposeAnnotator takes frames with min(H, W) == detect_resolution == image_resolution (= {r}), H % 64 == W % 64 == 0, "
                f"192 <= H, H % 184 != 0 and H, W <= 2048; got {h} x {w}")

    # ---- the chain -------------------------------------------------------------------------------------------------------------
    def _network(self, src, ws, i0: int) -> None:
        """The network for the frames `src` (a chunk): PAF and heat into ws["low"][i0 : i0 + len(src)]."""
        from . import kernels as K
        from .context import dispatch
        wts = self._weights(src.device)
        n = src.shape[0]
        g = ws["geometry"]
        with self._pass(ws, src.device) as p:
            take, give, launch = p.take, p.give, p.launch

            def conv3(x, wb):   # split_k=False: the order of an output's sum is then the same whatever the number of frames
                return p.conv3x3("conv", x, wb, act=K.ACT_RELU, split_k=False)

            def pw(x, wb, act, out2d, out_f32=False):
                p.pointwise("pointwise", x, wb, act, out2d=out2d, out_f32=out_f32)

            x = launch("prep", K.pose_prep, src, ws["area"], g["hs"], g["ws"], take(n, g["hp"], g["wp"], 8))
            for layer, wb in zip(FRONT, wts["front"]):
                if layer == "pool":
                    y = launch("pool", K.maxpool2x2, x, take(n, x.shape[1] // 2, x.shape[2] // 2, x.shape[3]))
                else:
                    y = conv3(x, wb)
                give(x)
                x = y
            feat = x
            hl, wl = g["hl"], g["wl"]
            rows = n * hl * wl
            cat = take(n, hl, wl, 192)
            cat2d = cat.view(rows, 192)
            launch("copy", K.copy_cols, feat.view(rows, 128), cat2d, 0)
            col = {0: (128, 168), 1: (168, 192)}     # the columns of L1 (38 + 2) and L2 (19 + 5) in the concatenation
            low2d = ws["low"][i0:i0 + n].view(rows, 64)
            lcol = {0: (0, 40), 1: (40, 64)}         # ... and in the fp32 output
            for br, s1 in enumerate(wts["stage1"]):
                a = feat
                for wb in s1["conv"]:
                    y = conv3(a, wb)
                    if a is not feat:
                        give(a)
                    a = y
                fc = take(rows, 512)
                pw(a, s1["fc"], K.ACT_RELU, fc)
                give(a)
                pw(fc, s1["out"], K.ACT_NONE, cat2d[:, col[br][0]:col[br][1]])
                give(fc)
            give(feat)
            direct = bool(dispatch.pose_conv7_direct)
            cols = None if direct else take(rows, 49 * 192)
            for t, stage in enumerate(wts["stages"]):
                xs = [cat, cat]
                for i in range(5):
                    outs = [take(n, hl, wl, 128), take(n, hl, wl, 128)]
                    launch("conv7", K.conv7x7, xs, [stage[0]["conv7"][i][0], stage[1]["conv7"][i][0]], biases=[stage[0]["conv7"][i][1], stage[1]["conv7"][i][1]],
                           relu=True, outs=outs, direct=direct, cols=cols)
                    if i:
                        give(xs[0]), give(xs[1])
                    xs = outs
                last = t == len(wts["stages"]) - 1
                for br in (0, 1):
                    fc = take(rows, 128)
                    pw(xs[br], stage[br]["fc"], K.ACT_RELU, fc)
                    give(xs[br])
                    if last:
                        pw(fc, stage[br]["out"], K.ACT_NONE, low2d[:, lcol[br][0]:lcol[br][1]], out_f32=True)
                    else:
                        pw(fc, stage[br]["out"], K.ACT_NONE, cat2d[:, col[br][0]:col[br][1]])
                    give(fc)
            if cols is not None:
                give(cols)
            give(cat)

    def _run(self, src, skeleton, control, rep, decode=True, face=None, hand=None):
        """face, hand: run that stage (None: when there is one and something is drawn)."""
        from . import kernels as K
        n, h, w, _ = src.shape
        ws = self.workspace(n, h, w)
        if ws["planned"] and bool(ws.get("direct", True)) != bool(self._direct()):
            ws["pool"], ws["plan"], ws["planned"] = [], [], False   # the other form of the 7x7 convolutions takes other buffers
        ws["direct"] = self._direct()
        step = self.chunk_frames(h, w)
        if ws["planned"] and min(step, n) > ws.get("chunk", 0):
            ws["pool"], ws["plan"], ws["planned"] = [], [], False   # a larger chunk than the plan was made for (max_activation_bytes grew)
        ws["chunk"] = max(ws.get("chunk", 0), min(step, n)) if ws["planned"] else min(step, n)
        for i0, sl in self._chunks(n, step):
            self._network(src[sl], ws, i0)
        self._timed("maps", K.pose_maps, ws["low"], ws["mx"], ws["my"], ws["raw"], ws["smooth"], ws["paf"], ws["maps_ws"])
        if decode:
            K.pose_decode(ws["raw"], ws["smooth"], ws["paf"], ws["decode"], stage=self._stage)
        drawn = skeleton is not None or control is not None
        fws = hws = None
        if self._face is not None and decode and (drawn if face is None else face):
            fws = self._faces_from(src, ws["decode"]["keypoints"], ws["decode"]["people"], ws["decode"]["overflow"])
        if self._hand is not None and decode and (drawn if hand is None else hand):   # (its overflow word carries the face stage's bits on)
            over = fws["buf"]["overflow"] if fws is not None else ws["decode"]["overflow"]
            hws = self._hand.run(src, ws["decode"]["keypoints"], ws["decode"]["people"], over, direct=self._direct())
        if drawn:
            ev = self._stage("draw")
            d = ws["decode"]
            if hws is not None:
                K.pose_draw_hands(d["coords"], d["people"], ws["sin"], hws["buf"]["points"], None if fws is None else fws["buf"]["points"], hws["xmap"], hws["ymap"],
                                  h, w, index=ws["index"], skeleton=skeleton, control=control, rep=rep)
            elif fws is None:
                K.pose_draw(d["coords"], d["people"], ws["sin"], h, w, index=ws["index"], skeleton=skeleton, control=control, rep=rep)
            else:
                K.pose_draw_faces(d["coords"], d["people"], ws["sin"], fws["buf"]["points"], fws["xmap"], fws["ymap"], h, w, index=ws["index"],
                                  skeleton=skeleton, control=control, rep=rep)
            if ev:
                ev[1].record()
        return ws

    def _faces_from(self, src, keypoints, people, overflow=None):
        """The face stage from given keypoints int32 [n, MAX_PEOPLE, 18, 2] and people int32 [n] on the device (the internal entry: tests
        plant them, a hand stage would start the same way) -> the stage's workspace (openpose_face.FaceStage.run)."""
        if self._face is None:
            raise NotImplementedError("no face network was given (OpenposeAnnotator(..., face=<state dict or facenet.pth>))")
        return self._face.run(src, keypoints, people, overflow, direct=self._direct())

    @staticmethod
    def _direct() -> bool:
        from .context import dispatch
        return bool(dispatch.pose_conv7_direct)

    def lowres(self, frames):
        """-> float32 [n, hl, wl, 64] on the device, as a new tensor: the network's sixth-stage output at 1/8 of the padded input, PAF in
        columns 0 .. 37, heat in 40 .. 58 (the other columns are zero)."""
        src = self._frames(frames)
        return self._run(src, None, None, 1, decode=False)["low"].clone()

    def maps(self, frames):
        """-> (raw heat [n, 18, H, W], smoothed heat [n, 18, H, W], PAF [n, 38, H, W]), float32 on the device, as new tensors."""
        src = self._frames(frames)
        ws = self._run(src, None, None, 1, decode=False)
        return ws["raw"].clone(), ws["smooth"].clone(), ws["paf"].clone()

    def poses(self, frames):
        """-> (keypoints int32 [n, MAX_PEOPLE, 18, 2] = (x, y) pixels, -1 for a missing part or an unused row; people int32 [n];
        overflow int32 [n]: OVERFLOW_PEAKS | OVERFLOW_PEOPLE where a cap was exceeded), on the device, as new tensors."""
        src = self._frames(frames)
        d = self._run(src, None, None, 1)["decode"]
        return d["keypoints"].clone(), d["people"].clone(), d["overflow"].clone()

    def faces(self, frames):
        """-> (points int32 [n, MAX_PEOPLE, 71, 2] = (x, y) frame pixels of the face keypoints of the person of that row of poses(), -1 for
        none; boxes int32 [n, MAX_PEOPLE, 4] = (x, y, side, slot) of util.faceDetect, side 0 for no box, slot -1 for a face that was not
        taken; overflow int32 [n]: poses()'s bits and OVERFLOW_FACES | OVERFLOW_FACE_RESIZE), on the device, as new tensors."""
        if self._face is None:
            raise NotImplementedError("no face network was given (OpenposeAnnotator(..., face=<state dict or facenet.pth>))")
        src = self._frames(frames)
        self._run(src, None, None, 1, face=True, hand=False)
        b = self._face.workspace(*src.shape[:3], src.device)["buf"]
        return b["points"].clone(), b["boxes"].clone(), b["overflow"].clone()

    def hands(self, frames):
        """-> (points int32 [n, MAX_PEOPLE, 2, 21, 2] = (x, y) frame pixels of the hand keypoints of the person of that row of poses(), left
        then right, -1 for a missing coordinate; boxes int32 [n, MAX_PEOPLE, 2, 4] = (x, y, side, slot) of util.handDetect, side 0 for no box,
        slot -1 for a hand that was not taken; overflow int32 [n]: poses()'s bits and OVERFLOW_HANDS | OVERFLOW_HAND_RESIZE), on the device,
        as new tensors."""
        if self._hand is None:
            raise NotImplementedError("no hand network was given (OpenposeAnnotator(..., hand=<state dict or hand_pose_model.pth>))")
        src = self._frames(frames)
        self._run(src, None, None, 1, face=False, hand=True)
        b = self._hand.workspace(*src.shape[:3], src.device)["buf"]
        return b["points"].clone(), b["boxes"].clone(), b["overflow"].clone()

    def skeleton(self, frames, out=None):
        """frames: a list of PIL images / uint8 arrays of one size, or a uint8 tensor [n, H, W, C] (no host copy when it is on the
        device) -> uint8 device tensor [n, H, W, 3] (RGB: the detector's drawing on black, with the face dots when there is a face
        network), written into `out` when given."""
        return self._uint8_out(frames, out, channels_last=3)

    def __call__(self, image):
        try:
            from PIL import Image
        except Exception:  # pragma: no cover
            Image = None
        rgb = self.skeleton([image])[0].cpu().numpy()
        return Image.fromarray(rgb) if Image is not None and not isinstance(image, np.ndarray) else rgb
