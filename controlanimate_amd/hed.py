"""The HED edge annotator of the reference's sample config (configs/prompts/SampleConfig.yaml: lllyasviel/sd-controlnet-hed, whose
control frames come from controlnet_aux's HEDdetector, modules/controlresiduals_pipeline.py:58, 116-117) on the GPU, for a whole
window of frames at once.

The network (ControlNetHED_Apache2: a learned per-channel `norm` subtracted from float RGB in 0..255; five blocks of 3x3
convolutions + ReLU, 3->64 x2, 64->128 x2, 128->256 x3, 256->512 x3, 512->512 x3, blocks 2..5 behind a 2x2 max pool; a 1x1
projection to a one-channel side map per block) runs as: ca_hed_prep (uint8 -> NHWC with 8 channels), thirteen ca_conv3x3 with
CA_ACT_RELU on two ping-pong buffers, ca_hed_pool_side after each block (the side map and the pooled tensor in one pass over the
block's output), and one ca_hed_fuse (the five bilinear resizes, mean, sigmoid, quantisation -> the uint8 map and / or the control
tensor the ControlNets hold).  No device-to-host read anywhere: the chain can be captured in a hipGraph.

The specification is tests/hed_ref.py (the fp32 torch network and the numpy detector, restated from the published code).
controlnet_aux and OpenCV are third-party packages that are absent here, and no ControlNetHED.pth is available: parity with them is
UNPINNED.  In particular the fp16 range on the trained checkpoint is unmeasured -- the activations of a VGG fed 0..255 inputs can
reach the thousands (fp16 overflows at 65504, and the MFMA accumulates in fp32 but stores fp16): `dtype=torch.bfloat16` is the
escape.

Scope of sizes: frames for which both of the detector's `resize_image` calls are the identity, min(H, W) == detect_resolution ==
image_resolution with H and W multiples of 64 (512 x 512, 512 x 768: the sizes this project measures).  Anything else raises
NotImplementedError: the INTER_AREA / INTER_LANCZOS4 resamplings of the detector are not rebuilt.
"""
from __future__ import annotations

import os

from .annotator_base import AnnotatorBase, check_state_dict as _check_state_dict, pack_conv

HED_BLOCKS = ((3, 64, 2), (64, 128, 2), (128, 256, 3), (256, 512, 3), (512, 512, 3))  # (in, out, layers) of block1 .. block5
WEIGHTS_NAME = "ControlNetHED.pth"
_CIN_PAD = 8  # ca_conv3x3 takes input channels in multiples of 8: the first convolution's weight is zero-padded, ca_hed_prep writes zeros


def hed_key_shapes() -> dict:
    """The 37 tensors of ControlNetHED.pth: name -> shape."""
    out = {"norm": (1, 3, 1, 1)}
    for b, (cin, cout, layers) in enumerate(HED_BLOCKS, start=1):
        for i in range(layers):
            out[f"block{b}.convs.{i}.weight"] = (cout, cin if i == 0 else cout, 3, 3)
            out[f"block{b}.convs.{i}.bias"] = (cout,)
        out[f"block{b}.projection.weight"] = (1, cout, 1, 1)
        out[f"block{b}.projection.bias"] = (1,)
    return out


def check_state_dict(sd) -> None:
    """KeyError naming a missing tensor, ValueError naming one that is unexpected or has the wrong shape."""
    _check_state_dict(sd, hed_key_shapes(), "HED", "norm, block1..5.convs.*.weight|bias, block1..5.projection.weight|bias")


class HedAnnotator(AnnotatorBase):
    """`HedAnnotator(weights)(image)` has the contract of `annotators.canny(image)` (PIL RGB in, PIL RGB with three equal channels out;
    an array in, an array out), so it plugs into `MultiControlNetResidualsPipeline(annotators={"hed": HedAnnotator.from_pretrained(path)})`,
    whose `prep_control_images` then calls `annotate_batch` once per list of frames.  Nothing makes it a default: the weights are the
    user's file.  Non-uint8 input raises TypeError, frames of different sizes ValueError, sizes out of scope NotImplementedError -- all
    before the device is touched; without the library or a GPU a call raises CAHipUnavailable (there is no CPU fallback)."""

    WEIGHTS_NAME = WEIGHTS_NAME
    # the largest activation of a chunk of frames (block 1's output, 64 channels at full size) stays below what ca_conv3x3's kernels
    # address with 32-bit byte offsets (conv_prepare: operands below 0x7FFFFF00 bytes keep every plan available)
    _bytes_per_pixel = 64 * 2
    _addressed_by = "the convolutions"

    def __init__(self, state_dict_or_path, device=None, dtype=None, detect_resolution: int = 512, image_resolution: int = 512):
        import torch
        dtype = torch.float16 if dtype is None else dtype
        if dtype not in (torch.float16, torch.bfloat16):
            raise TypeError(f"dtype must be torch.float16 or torch.bfloat16, got {dtype}")
        sd = self._load(state_dict_or_path) if isinstance(state_dict_or_path, (str, os.PathLike)) else state_dict_or_path
        check_state_dict(sd)
        self.device, self.dtype = device, dtype
        self.detect_resolution, self.image_resolution = int(detect_resolution), int(image_resolution)
        # packed once, on the host: [cout][3][3][cin] in `dtype` (cin zero-padded to 8 for the first), fp32 biases, projections as fp32 rows
        self._host = {"norm": sd["norm"].detach().float().reshape(3).contiguous(), "blocks": []}
        for b, (cin, cout, layers) in enumerate(HED_BLOCKS, start=1):
            convs = [pack_conv((sd[f"block{b}.convs.{i}.weight"], sd[f"block{b}.convs.{i}.bias"]), dtype, cin_pad=_CIN_PAD) for i in range(layers)]
            self._host["blocks"].append((convs, sd[f"block{b}.projection.weight"].detach().float().reshape(cout).contiguous(),
                                         sd[f"block{b}.projection.bias"].detach().float().reshape(1).contiguous()))
        self._ws = {}   # (`timings` receives events under "prep", "conv", "pool_side", "fuse" -- tools/bench_hed.py)

    # ---- device state ----------------------------------------------------------------------------------------------------------
    def workspace(self, n: int, h: int, w: int):
        """(two ping-pong activation buffers for a chunk of frames, the five float32 side maps [n, h >> k, w >> k]) of a call with n frames
        of h x w pixels, cached per (n, h, w); contents are never assumed."""
        import torch
        return self._workspace((n, h, w), lambda dev: (
            [torch.empty(min(n, self.chunk_frames(h, w)) * h * w * 64, dtype=self.dtype, device=dev) for _ in range(2)],
            [torch.empty((n, h >> k, w >> k), dtype=torch.float32, device=dev) for k in range(5)]))

    # ---- input checks ----------------------------------------------------------------------------------------------------------
    def _check_size(self, h: int, w: int) -> None:
        if not (min(h, w) == self.detect_resolution == self.image_resolution and h % 64 == 0 and w % 64 == 0):
            raise NotImplementedError(
                f"HedAnnotator takes frames for which both resize_image calls of the detector are the identity: min(H, W) == detect_resolution == "
                f"image_resolution and H % 64 == W % 64 == 0; got {h} x {w} with detect_resolution={self.detect_resolution}, "
                f"image_resolution={self.image_resolution} (the INTER_AREA / INTER_LANCZOS4 resamplings are not rebuilt)")

    # ---- the chain -------------------------------------------------------------------------------------------------------------
    def _network(self, src, bufs, sides, i0: int) -> None:
        """The network for the frames `src` (a chunk), side maps into sides[k][i0 : i0 + len(src)]."""
        from . import kernels as K
        wts = self._weights(src.device)
        n, h, w, _ = src.shape
        cur, other = bufs

        def view(buf, hh, ww, c):
            return buf[: n * hh * ww * c].view(n, hh, ww, c)

        x = self._timed("prep", K.hed_prep, src, wts["norm"], view(cur, h, w, _CIN_PAD))
        hh, ww = h, w
        for k, (convs, pw, pb) in enumerate(wts["blocks"]):
            for wt, bias in convs:
                cur, other = other, cur
                x = self._timed("conv", K.conv3x3, x, wt, bias=bias, act=K.ACT_RELU, out=view(cur, hh, ww, wt.shape[0]))
            last = k == len(wts["blocks"]) - 1
            pooled = None if last else view(other, hh // 2, ww // 2, x.shape[3])
            self._timed("pool_side", K.hed_pool_side, x, pw, pb, sides[k][i0:i0 + n], pooled)
            if not last:
                cur, other = other, cur
                x, hh, ww = pooled, hh // 2, ww // 2

    def _run(self, src, edges, control, rep):
        from . import kernels as K
        n, h, w, _ = src.shape
        bufs, sides = self.workspace(n, h, w)
        for i0, sl in self._chunks(n, self.chunk_frames(h, w)):
            self._network(src[sl], bufs, sides, i0)
        if edges is not None or control is not None:
            self._timed("fuse", K.hed_fuse, sides, edges=edges, control=control, rep=rep)
        return sides

    def side_maps(self, frames):
        """-> the five float32 side maps [n, H >> k, W >> k] on the device (the logits before resize, mean and sigmoid), as new tensors."""
        src = self._frames(frames)
        return [s.clone() for s in self._run(src, None, None, 1)]

    def edges(self, frames, out=None):
        """frames: a list of PIL images / uint8 arrays of one size, or a uint8 tensor [n, H, W, C] (no host copy when it is on the
        device) -> uint8 device tensor [n, H, W] (the detector's map, 0 .. 255), written into `out` when given."""
        return self._uint8_out(frames, out)
