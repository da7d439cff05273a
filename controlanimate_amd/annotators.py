"""Host-side ControlNet annotators ("canny first").

`canny(image, low, high)` restates OpenCV's cv2.Canny(img, 100, 200) as the reference calls it
(modules/controlresiduals_pipeline.py:48-55: 8-bit RGB input, aperture 3, L1 gradient norm) in numpy:
3x3 Sobel with replicated borders; for colour input the channel with the largest |dx| + |dy| at each pixel;
non-maximum suppression with OpenCV's fixed-point tan(22.5 deg) sector test; hysteresis (strong > high,
weak > low connected through the 8-neighbourhood).  OpenCV is a THIRD-PARTY dependency that is absent here, so
this restatement is UNPINNED (no cv2 output to compare with); tests check the algorithmic properties.
Of the learned detectors (controlnet_aux / transformers models, :56-61) HED, the sample config's, is rebuilt: `HedAnnotator` (hed.py,
re-exported here) runs ControlNetHED for a whole window on the GPU from a local ControlNetHED.pth, opt-in through
`annotators={"hed": HedAnnotator.from_pretrained(path)}`.  So is lineart, the IP-Adapter sample config's: `LineartAnnotator`
(lineart.py, re-exported here) runs the "informative drawings" generator of controlnet_aux's LineartDetector from a local
sk_model.pth / sk_model2.pth, opt-in through `annotators={"lineart": LineartAnnotator.from_pretrained(path)}`.  So is mlsd, which every
sample config with ControlNets lists: `MlsdAnnotator` (mlsd.py, re-exported here) runs MobileV2_MLSD_Large, the top-200 decode and the
line drawing of controlnet_aux's MLSDdetector from a local mlsd_large_512_fp32.pth, opt-in through
`annotators={"mlsd": MlsdAnnotator.from_pretrained(path)}` (it serves control_v11p_sd15_mlsd and sd-controlnet-mlsd alike).  So is
softedge, the IP-Adapter sample config's sixth ControlNet: `SoftedgeAnnotator` (softedge.py, re-exported here) runs PiDiNet and the tail of
controlnet_aux's PidiNetDetector from a local table5_pidinet.pth, opt-in through `annotators={"softedge":
SoftedgeAnnotator.from_pretrained(path)}`.  So is lineart_anime, which every sample config lists: `LineartAnimeAnnotator`
(lineart_anime.py, re-exported here) runs the pix2pix U-Net of controlnet_aux's LineartAnimeDetector from a local netG.pth, opt-in
through `annotators={"lineart_anime": LineartAnimeAnnotator.from_pretrained(path)}`.  So is depth, the transformers depth-estimation
pipeline (Intel/dpt-large): `DepthAnnotator` (depth.py, re-exported here) runs DPTForDepthEstimation, the image processor's Pillow resize
and the pipeline's post-processing from a local model directory, opt-in through `annotators={"depth":
DepthAnnotator.from_pretrained(local_dir)}` (the key serves sd-controlnet-depth and control_v11f1p_sd15_depth alike); it is pinned
against transformers' and Pillow's own modules.  So is openpose, the first ControlNet of three sample configs: `OpenposeAnnotator`
(openpose.py, re-exported here) runs bodypose_model, the skeleton decode and the drawing of controlnet_aux's OpenposeDetector on the
device from a local body_pose_model.pth, opt-in through `annotators={"openpose": OpenposeAnnotator.from_pretrained(path)}` (the key serves
control_v11p_sd15_openpose and sd-controlnet-openpose alike).  Given a face network (`face=<facenet.pth>`) it also draws the face
keypoints of the reference's hand_and_face=True (openpose_face.py); without one it draws the BODY skeleton only.  Given a hand network
(`hand=<hand_pose_model.pth>`) it draws the hands too (openpose_hand.py); with both, the drawing is the reference's hand_and_face=True.
So is normalbae, the last of the reference's nine branches: `NormalBaeAnnotator` (normalbae.py, re-exported here) runs the EfficientNet-B5
encoder, the decoder and the per-pixel refinement stages of controlnet_aux's NormalBaeDetector from a local scannet.pt, opt-in through
`annotators={"normalbae": NormalBaeAnnotator.from_pretrained(path)}`; its encoder is pinned against transformers' EfficientNetModel.
(The face restorer of the emitted frames is not an annotator and lives in gfpgan.py: GFPGANv1Clean for aligned 512 x 512 faces on the HIP
kernels, around a caller-supplied helper for detection, warp and paste-back; UNPINNED against gfpgan and real weights; no CPU fallback.)

`CannyAnnotator` is the same function for a whole window of frames on the GPU (ABI v16, csrc/ca_canny.hip): opt-in through
`annotators={"canny": CannyAnnotator(device)}`; `canny` stays the default.  `canny_edges` is its specification: the device result
equals it byte for byte.
"""
from __future__ import annotations

import numpy as np

try:
    from PIL import Image
except Exception:  # pragma: no cover
    Image = None

from .annotator_base import AnnotatorBase  # noqa: E402
from .hed import HedAnnotator  # noqa: E402,F401  (the learned HED detector on the GPU; torch is imported when it is used)
from .lineart import LineartAnnotator  # noqa: E402,F401  (the learned lineart detector on the GPU, likewise)
from .lineart_anime import LineartAnimeAnnotator  # noqa: E402,F401  (the learned anime line detector on the GPU, likewise)
from .mlsd import MlsdAnnotator  # noqa: E402,F401  (the learned straight-line detector on the GPU, likewise)
from .softedge import SoftedgeAnnotator  # noqa: E402,F401  (the learned soft-edge detector on the GPU, likewise)
from .openpose import OpenposeAnnotator  # noqa: E402,F401  (the learned body-pose detector on the GPU, likewise)
from .normalbae import NormalBaeAnnotator  # noqa: E402,F401  (the learned surface-normal detector on the GPU, likewise)


def __getattr__(name):
    # DepthAnnotator (the DPT depth estimator on the GPU) is re-exported on first use: depth.py builds on clip.py's packed-model classes,
    # which import torch, and this module stays importable without it
    if name == "DepthAnnotator":
        from .depth import DepthAnnotator
        return DepthAnnotator
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _sobel(ch: np.ndarray):
    p = np.pad(ch.astype(np.int32), 1, mode="edge")
    dx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    dy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    return dx, dy


def canny_edges(img: np.ndarray, low: float = 100, high: float = 200) -> np.ndarray:
    """img: [H,W] or [H,W,C] uint8 -> [H,W] uint8 edge map (0 / 255)."""
    a = np.asarray(img)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, c = a.shape
    dx = np.zeros((h, w), np.int32)
    dy = np.zeros((h, w), np.int32)
    mag = np.full((h, w), -1, np.int32)
    for k in range(c):  # the channel with the largest L1 gradient wins
        gx, gy = _sobel(a[:, :, k])
        m = np.abs(gx) + np.abs(gy)
        take = m > mag
        dx[take], dy[take], mag[take] = gx[take], gy[take], m[take]
    low_i, high_i = int(np.floor(low)), int(np.floor(high))
    # non-maximum suppression along the quantised gradient direction (OpenCV: TG22 = tan(22.5) * 2^15)
    pm = np.pad(mag, 1, mode="constant")
    ax, ay = np.abs(dx).astype(np.int64), np.abs(dy).astype(np.int64) << 15
    tg22x = ax * 13573
    tg67x = tg22x + (ax << 16)
    c0 = pm[1:-1, 1:-1]
    left, right = pm[1:-1, :-2], pm[1:-1, 2:]
    up, down = pm[:-2, 1:-1], pm[2:, 1:-1]
    horiz = ay < tg22x                      # gradient ~ horizontal: compare with left / right
    vert = ay > tg67x                       # ~ vertical: compare with up / down
    s = np.where((dx ^ dy) < 0, -1, 1)      # diagonal: sign decides which diagonal
    ul, dr = pm[:-2, :-2], pm[2:, 2:]
    ur, dl = pm[:-2, 2:], pm[2:, :-2]
    d1, d2 = np.where(s > 0, ul, ur), np.where(s > 0, dr, dl)
    keep = np.where(horiz, (c0 > left) & (c0 >= right), np.where(vert, (c0 > up) & (c0 >= down), (c0 > d1) & (c0 > d2)))
    cand = keep & (mag > low_i)
    strong = cand & (mag > high_i)
    # hysteresis: grow the strong set through weak candidates (8-neighbourhood) to a fixed point
    out = strong.copy()
    while True:
        p = np.pad(out, 1, mode="constant")
        nb = (p[:-2, :-2] | p[:-2, 1:-1] | p[:-2, 2:] | p[1:-1, :-2] | p[1:-1, 2:] | p[2:, :-2] | p[2:, 1:-1] | p[2:, 2:])
        grown = out | (cand & nb)
        if grown.sum() == out.sum():
            break
        out = grown
    return (out * 255).astype(np.uint8)


def canny(image, low: float = 100, high: float = 200):
    """The reference's canny_processor (:48-55): PIL RGB -> PIL RGB whose three channels are the edge map."""
    e = canny_edges(np.asarray(image), low, high)
    rgb = np.repeat(e[:, :, None], 3, axis=2)
    return Image.fromarray(rgb) if Image is not None and not isinstance(image, np.ndarray) else rgb


class CannyAnnotator(AnnotatorBase):
    """`canny` on the GPU for a whole window at once: `CannyAnnotator(device)(image)` has the contract of `canny(image)` (PIL RGB in,
    PIL RGB with three equal channels out; an array in, an array out), so it is a drop-in for `annotators={"canny": ...}`, and
    `MultiControlNetResidualsPipeline.prep_control_images` calls `annotate_batch` once per list of frames instead of the callable
    once per frame.  All frames of a call share one size and go through ONE fixed set of five launches (classify; label, merge,
    flatten; emit) with no device-to-host read, so the chain can be captured in a hipGraph.  Non-uint8 input raises TypeError,
    frames of different sizes ValueError; without the library or a GPU a call raises CAHipUnavailable (no CPU fallback: `canny` is
    the host function)."""

    _no_gpu_hint = "(no CPU fallback; annotators.canny is the host function)"
    _grey_to_rgb = False   # C = 1 or 3 as given, as `canny` takes it: the kernel picks the channel with the largest gradient

    def __init__(self, device=None, low: float = 100, high: float = 200):
        self.device = device
        self.low, self.high = int(np.floor(low)), int(np.floor(high))
        if self.low > self.high:
            raise ValueError(f"low={low} > high={high}")
        self._ws = {}   # (`timings` receives events under classify, label, merge, flatten, emit -- tools/bench_canny.py)

    def workspace(self, n: int, h: int, w: int):
        """The scratch tensor of a call with n frames of h x w pixels (cached per (n, h, w); contents are never assumed)."""
        import torch
        from . import kernels as K
        key = (n, h, w)
        if key not in self._ws:
            self._ws[key] = torch.empty(K.canny_workspace_bytes(n, h, w), dtype=torch.uint8, device=self._device())
        return self._ws[key]

    def _run(self, frames, edges, control, rep):
        from . import kernels as K
        n, h, w, _ = frames.shape
        ws = self.workspace(n, h, w)
        self._timed("classify", K.canny_classify, frames, self.low, self.high, ws)
        if self.timings is None:
            K.canny_link(n, h, w, ws)
        else:  # the same three launches, one at a time, with events around each
            for stage in K.CANNY_LINK_STAGES:
                self._timed(stage, K.canny_link_stage, n, h, w, ws, stage)
        self._timed("emit", K.canny_emit, n, h, w, ws, edges=edges, control=control, rep=rep)

    def edges(self, frames, out=None):
        """frames: a list of PIL images / uint8 arrays of one size, or a uint8 tensor [n, H, W, C] (no host copy when it is on the
        device) -> uint8 device tensor [n, H, W] with 0 / 255, written into `out` when given."""
        return self._uint8_out(frames, out)
