"""The M-LSD straight-line annotator of the reference's sample configs (SampleConfig.yaml, SampleConfigLCMLoRA.yaml and
SampleConfigIPAdapter.yaml list lllyasviel/control_v11p_sd15_mlsd, the last one sd-controlnet-mlsd as well; their control frames come
from controlnet_aux's MLSDdetector, modules/controlresiduals_pipeline.py:56, 101-105) on the GPU, for a whole window of frames at once.

The detector, as the reference calls it (thr_v = 0.1, thr_d = 0.1, detect_resolution = image_resolution = 512):

    input    [H, W, 4]: RGB and a channel of ones, x / 127.5 - 1 on all four
    network  MobileV2_MLSD_Large: a MobileNetV2 backbone (features.0 .. 13; ConvBNReLU = Conv2d, BatchNorm, ReLU6, with F.pad(x, (0, 1, 0, 1))
             and padding 0 at stride 2; InvertedResidual = [1x1 expansion], depthwise 3x3, linear 1x1, skip when the shapes allow), taps
             c1 .. c5 after features 1, 3, 6, 10, 13, and a decoder of blocks A (two 1x1 convolutions + BN + ReLU, one side upsampled x2
             bilinearly with align_corners, concatenated), B (conv2(conv1(x) + x), 3x3 + BN + ReLU each) and C (3x3 with dilation 5, 3x3,
             1x1 to 16 channels) at half resolution; channels 7 .. 11 of the 16 are read: the centre logit and (dx_s, dy_s, dx_e, dy_e)
    decode   sigmoid, 3x3 maximum test that keeps plateaus, the top 200 of the map, score > thr_v, then |start - end| > thr_d (a dropped
             point is not replaced), endpoints 2 * (pixel + displacement) in float64 truncated by int()
    draw     cv2.line(map, start, end, 255, 1) on a zeroed map; three equal channels

It runs as (the names are the keys of `timings`, the numbers the stages of that name per pass):

    prep       1   ca_mlsd_prep: uint8 frames -> 8 channels (the stem's weight is zero-padded to 8 input channels)
    stem       1   ca_conv3x3, stride 2, pad_asym, CA_ACT_RELU6
    pointwise  33  ca_gemm with the folded bias: CA_ACT_RELU6 (expansions), none + residual (projections), CA_ACT_RELU (block A, whose
                   conv2 writes columns 0 .. 63 of the 128-wide concatenation through ldc = 128)
    depthwise  13  ca_dwconv3x3
    upsample   3   ca_upsample2x_bilinear_ac into columns 64 .. 127 of the concatenation
    conv       9   ca_conv3x3 with CA_ACT_RELU: the two convolutions of every block B and the second of block C
    add        4   ca_add_bcast: block B's conv1(x) + x is ReLU THEN add, which the convolution's residual epilogue (add, then activation)
                   does not compute -- one more pass over a 128-channel tensor at the block's resolution
    dilated    1   ca_conv3x3_dil
    head       1   ca_gemm, N = 8: rows 7 .. 11 of block23.conv3, zero-padded, fp32 output -- the tpMap [n, H/2, W/2, 8]
    decode     1   ca_mlsd_decode -> segments int32 [n, 200, 4], count int32 [n]
    draw       1   ca_mlsd_draw -> the uint8 map and / or the control tensor the ControlNets hold

Eval-mode BatchNorm (eps 1e-5) is folded into the convolution before it once, on the host, in fp32.  No device-to-host read anywhere:
the chain can be captured in a hipGraph.

The specification is tests/mlsd_ref.py (the fp32 torch network, the numpy decode and line iterator).  Key names and arithmetic are
restated from memory of the published code (mbv2_mlsd_large.py, utils.py of controlnet_aux's mlsd, OpenCV's clipLine / LineIterator)
and are UNPINNED: controlnet_aux and OpenCV are third-party packages that are absent here, and no mlsd_large_512_fp32.pth is available.
torch.topk's order among equal scores is unspecified; here it is score descending, then flat index ascending.

Scope of sizes: min(H, W) == detect_resolution == image_resolution with H and W multiples of 64, for which both resize_image calls, the
INTER_AREA resize inside pred_lines and the final INTER_LINEAR resize are the identity (512 x 512, 512 x 768, 768 x 512 at the default
512); anything else raises NotImplementedError.  MobileV2_MLSD_Tiny is not part of this.
"""
from __future__ import annotations

import os

from . import annotator_base as _base
from .annotator_base import AnnotatorBase, bn_key_shapes as _bn, check_state_dict as _check_state_dict, pack_conv, pack_pointwise

WEIGHTS_NAME = "mlsd_large_512_fp32.pth"
EPS = 1e-5
TOPK = 200
# (t, c, n, s) of the backbone behind features.0, as far as the taps reach (features.1 .. features.13)
SETTINGS = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1))
TAPS = (1, 3, 6, 10, 13)
STAGES = {"prep": 1, "stem": 1, "pointwise": 33, "depthwise": 13, "upsample": 3, "conv": 9, "add": 4, "dilated": 1, "head": 1, "decode": 1, "draw": 1}


def backbone_blocks():
    """[(features index, cin, hidden, cout, stride, expands, skips)] of features.1 .. features.13."""
    out, cin, idx = [], 32, 1
    for t, c, n, s in SETTINGS:
        for i in range(n):
            stride = s if i == 0 else 1
            out.append((idx, cin, cin * t, c, stride, t != 1, stride == 1 and cin == c))
            cin, idx = c, idx + 1
    return out


def mlsd_key_shapes() -> dict:
    """Every tensor of mlsd_large_512_fp32.pth that the chain uses: name -> shape."""
    out = {"backbone.features.0.0.weight": (32, 4, 3, 3), **_bn("backbone.features.0.1", 32)}
    for idx, cin, hid, c, _, expands, _ in backbone_blocks():
        p, j = f"backbone.features.{idx}.conv", 0
        if expands:
            out[f"{p}.0.0.weight"] = (hid, cin, 1, 1)
            out.update(_bn(f"{p}.0.1", hid))
            j = 1
        out[f"{p}.{j}.0.weight"] = (hid, 1, 3, 3)
        out.update(_bn(f"{p}.{j}.1", hid))
        out[f"{p}.{j + 1}.weight"] = (c, hid, 1, 1)
        out.update(_bn(f"{p}.{j + 2}", c))

    def conv_bn(prefix, cout, cin, k):
        out[f"{prefix}.0.weight"], out[f"{prefix}.0.bias"] = (cout, cin, k, k), (cout,)
        out.update(_bn(f"{prefix}.1", cout))

    for blk, (c_a, c_b) in ((15, (64, 96)), (17, (32, 64)), (19, (24, 64)), (21, (16, 64))):   # A(a, b): conv1 takes b, conv2 takes a
        conv_bn(f"block{blk}.conv1", 64, c_b, 1)
        conv_bn(f"block{blk}.conv2", 64, c_a, 1)
        conv_bn(f"block{blk + 1}.conv1", 128, 128, 3)
        conv_bn(f"block{blk + 1}.conv2", 64, 128, 3)
    conv_bn("block23.conv1", 64, 64, 3)
    conv_bn("block23.conv2", 64, 64, 3)
    out["block23.conv3.weight"], out["block23.conv3.bias"] = (16, 64, 1, 1), (16,)
    return out


def check_state_dict(sd) -> None:
    """KeyError naming a missing tensor, ValueError naming one that is unexpected or has the wrong shape.  num_batches_tracked and any
    further backbone. key (layers past features.13 that a checkpoint may keep) are ignored."""
    _check_state_dict(sd, mlsd_key_shapes(), "mlsd", "backbone.features.0 .. 13 and block15 .. block23 of MobileV2_MLSD_Large",
                      ignore=lambda k: k.endswith("num_batches_tracked") or k.startswith("backbone."))


def fold_bn(sd, conv: str, bn: str):
    """(weight, bias) in fp32 of the convolution `conv` followed by the eval-mode BatchNorm `bn`: w * g / sqrt(var + eps) per output
    channel, (b - mean) * g / sqrt(var + eps) + beta."""
    return _base.fold_bn(sd, conv, bn, EPS)


def folded_layers(sd) -> dict:
    """The network as fp32 (weight, bias) pairs in PyTorch layout, BatchNorm folded: what the device chain and the folding test read.
    "stem"; "features": [{"expand"?, "dw", "project"}]; "A": [(conv1, conv2)] and "B": [(conv1, conv2)] for blocks 15 / 17 / 19 / 21 and
    16 / 18 / 20 / 22; "C": (conv1, conv2, conv3)."""
    out = {"stem": fold_bn(sd, "backbone.features.0.0", "backbone.features.0.1"), "features": [], "A": [], "B": []}
    for idx, _, _, _, _, expands, _ in backbone_blocks():
        p, j, blk = f"backbone.features.{idx}.conv", 0, {}
        if expands:
            blk["expand"] = fold_bn(sd, f"{p}.0.0", f"{p}.0.1")
            j = 1
        blk["dw"] = fold_bn(sd, f"{p}.{j}.0", f"{p}.{j}.1")
        blk["project"] = fold_bn(sd, f"{p}.{j + 1}", f"{p}.{j + 2}")
        out["features"].append(blk)
    for blk in (15, 17, 19, 21):
        out["A"].append(tuple(fold_bn(sd, f"block{blk}.conv{k}.0", f"block{blk}.conv{k}.1") for k in (1, 2)))
        out["B"].append(tuple(fold_bn(sd, f"block{blk + 1}.conv{k}.0", f"block{blk + 1}.conv{k}.1") for k in (1, 2)))
    out["C"] = (fold_bn(sd, "block23.conv1.0", "block23.conv1.1"), fold_bn(sd, "block23.conv2.0", "block23.conv2.1"),
                (sd["block23.conv3.weight"].detach().float(), sd["block23.conv3.bias"].detach().float()))
    return out


def pack_depthwise(w):
    """Depthwise weight [C, 1, 3, 3] -> [9, C]: tap ky * 3 + kx of every channel (ca_dwconv3x3)."""
    return _base.pack_depthwise(w, (3,))


class MlsdAnnotator(AnnotatorBase):
    """`MlsdAnnotator(weights)(image)` has the contract of `annotators.canny(image)` (PIL in, PIL RGB with three equal channels out; an
    array in, an array out), so it plugs into `MultiControlNetResidualsPipeline(annotators={"mlsd": MlsdAnnotator.from_pretrained(path)})`,
    whose `prep_control_images` then calls `annotate_batch` once per list of frames.  Nothing makes it a default: the weights are the
    user's file.  Non-uint8 input raises TypeError, frames of different sizes ValueError, sizes out of scope NotImplementedError -- all
    before the device is touched; without the library or a GPU a call raises CAHipUnavailable (there is no CPU fallback)."""

    # the largest operand of a chunk of frames (the 128-channel concatenation at half resolution: 64 bytes per frame pixel) stays below
    # what the GEMM and convolution kernels address with 32-bit byte offsets
    _bytes_per_pixel = 64
    WEIGHTS_NAME = WEIGHTS_NAME

    def __init__(self, state_dict_or_path, device=None, dtype=None, detect_resolution: int = 512, image_resolution: int = 512,
                 thr_v: float = 0.1, thr_d: float = 0.1):
        import torch
        dtype = torch.float16 if dtype is None else dtype
        if dtype not in (torch.float16, torch.bfloat16):
            raise TypeError(f"dtype must be torch.float16 or torch.bfloat16, got {dtype}")
        if detect_resolution != image_resolution or detect_resolution < 64 or detect_resolution % 64:
            raise NotImplementedError(f"MlsdAnnotator takes detect_resolution == image_resolution, a multiple of 64 (no resampling); got "
                                      f"{detect_resolution} and {image_resolution}")
        if not (0.0 <= thr_v < 1.0) or not (0.0 <= thr_d < float("inf")):
            raise ValueError(f"thr_v={thr_v} (0 <= thr_v < 1), thr_d={thr_d} (>= 0)")
        sd = self._load(state_dict_or_path) if isinstance(state_dict_or_path, (str, os.PathLike)) else state_dict_or_path
        check_state_dict(sd)
        self.device, self.dtype = device, dtype
        self.resolution, self.thr_v, self.thr_d = int(detect_resolution), float(thr_v), float(thr_d)
        f = folded_layers(sd)
        # packed once, on the host
        self._host = {
            "stem": pack_conv(f["stem"], dtype, cin_pad=8),   # 4 -> 8 input channels, the new ones zero
            "features": [{k: ((pack_depthwise(v[0]).to(dtype), v[1].contiguous()) if k == "dw" else pack_pointwise(v, dtype)) for k, v in blk.items()}
                         for blk in f["features"]],
            "A": [(pack_pointwise(a, dtype), pack_pointwise(b, dtype)) for a, b in f["A"]],
            "B": [(pack_conv(a, dtype), pack_conv(b, dtype)) for a, b in f["B"]],
            "C": (pack_conv(f["C"][0], dtype), pack_conv(f["C"][1], dtype)),
            "head": pack_pointwise((f["C"][2][0][7:12], f["C"][2][1][7:12]), dtype, cout_pad=8),   # rows 7 .. 11 of conv3, 5 -> 8 rows
        }
        self._ws = {}   # (`timings` receives events under the keys of STAGES -- tools/bench_mlsd.py)

    # ---- device state ----------------------------------------------------------------------------------------------------------
    def workspace(self, n: int, h: int, w: int) -> dict:
        """The buffers of a call with n frames of h x w pixels, cached per (n, h, w): the tpMap float32 [n, h/2, w/2, 8], the segments, the
        counts, the candidate list of the decode, the map that is drawn when only the control tensor is asked for, and a pool of
        activation buffers that the layers of a pass take and give back in a fixed order (contents are never assumed; the first pass
        allocates them -- the largest chunk comes first -- and every later pass reuses the same ones)."""
        import torch
        from . import kernels as K
        return self._workspace((n, h, w), lambda dev: {
            "tp": torch.empty((n, h // 2, w // 2, 8), dtype=torch.float32, device=dev),
            "segments": torch.empty((n, TOPK, 4), dtype=torch.int32, device=dev),
            "count": torch.empty((n,), dtype=torch.int32, device=dev),
            "decode": torch.empty(K.mlsd_decode_workspace_bytes(n, h // 2, w // 2), dtype=torch.uint8, device=dev),
            "map": torch.empty((n, h, w), dtype=torch.uint8, device=dev)})

    # ---- input checks ----------------------------------------------------------------------------------------------------------
    def _check_size(self, h: int, w: int) -> None:
        r = self.resolution
        if min(h, w) != r or h % 64 or w % 64:
            raise NotImplementedError(
                f"MlsdAnnotator takes frames with min(H, W) == detect_resolution == image_resolution (= {r}) and H % 64 == W % 64 == 0, for "
                f"which every resampling of the detector is the identity; got {h} x {w}")

    # ---- the chain -------------------------------------------------------------------------------------------------------------
    def _network(self, src, ws, i0: int) -> None:
        """The network for the frames `src` (a chunk), the tpMap into ws["tp"][i0 : i0 + len(src)]."""
        from . import kernels as K
        wts = self._weights(src.device)
        n, h, w, _ = src.shape
        with self._pass(ws, src.device) as p:   # the same buffers in the same order on every pass
            take, give, launch, pw = p.take, p.give, p.launch, p.pointwise
            x = launch("prep", K.mlsd_prep, src, take(n, h, w, 8))
            y = p.conv3x3("stem", x, wts["stem"], stride=2, act=K.ACT_RELU6, pad_asym=True)
            give(x)
            x, taps = y, {}
            for (idx, _, hid, c, stride, expands, skips), blk in zip(backbone_blocks(), wts["features"]):
                t = pw("pointwise", x, blk["expand"], K.ACT_RELU6) if expands else x
                hh, ww = t.shape[1] // stride, t.shape[2] // stride
                d = launch("depthwise", K.dwconv3x3, t, blk["dw"][0], blk["dw"][1], stride=stride, relu6=True, out=take(n, hh, ww, hid))
                if expands:
                    give(t)
                y = pw("pointwise", d, blk["project"], residual=x if skips else None)
                give(d)
                if idx - 1 in TAPS:   # x is the output of features[idx - 1]: a tap stays until its block A has read it
                    taps[idx - 1] = x
                else:
                    give(x)
                x = y
                if idx == TAPS[-1]:
                    taps[idx] = x
            c1, c2, c3, c4, c5 = (taps[i] for i in TAPS)
            x = c5
            for level, (a, up) in enumerate(((c4, False), (c3, True), (c2, True), (c1, True))):
                (w1, w2), (b1, b2) = wts["A"][level], wts["B"][level]
                nn, hh, ww, _ = a.shape
                cat = take(nn, hh, ww, 128)
                cat2d = cat.view(nn * hh * ww, 128)
                pw("pointwise", a, w2, K.ACT_RELU, out2d=cat2d[:, :64])
                if up:
                    t = pw("pointwise", x, w1, K.ACT_RELU)
                    launch("upsample", K.upsample2x_bilinear_ac, t, cat, 64)
                    give(t)
                else:
                    pw("pointwise", x, w1, K.ACT_RELU, out2d=cat2d[:, 64:])
                give(a)
                give(x)
                t = p.conv3x3("conv", cat, b1, act=K.ACT_RELU)
                launch("add", K.add_bcast, t, cat, out=t)   # ReLU, then the skip
                give(cat)
                x = p.conv3x3("conv", t, b2, act=K.ACT_RELU)
                give(t)
            (d1, d2) = wts["C"]
            t = launch("dilated", K.conv3x3_dil, x, d1[0], d1[1], dilation=5, relu=True, out=take(*x.shape))
            give(x)
            x = p.conv3x3("conv", t, d2, act=K.ACT_RELU)
            give(t)
            pw("head", x, wts["head"], out2d=ws["tp"][i0:i0 + n].view(-1, 8), out_f32=True)
            give(x)

    def _run(self, src, edges, control, rep):
        from . import kernels as K
        n, h, w, _ = src.shape
        ws = self.workspace(n, h, w)
        for i0, sl in self._chunks(n, self.chunk_frames(h, w)):
            self._network(src[sl], ws, i0)
        if edges is not None or control is not None:
            self._timed("decode", K.mlsd_decode, ws["tp"], self.thr_v, self.thr_d, segments=ws["segments"], count=ws["count"], ws=ws["decode"])
            self._timed("draw", K.mlsd_draw, ws["segments"], ws["count"], h, w, edges=edges if edges is not None else ws["map"], control=control, rep=rep)
        return ws["tp"]

    def tpmap(self, frames):
        """-> float32 [n, H/2, W/2, 8] on the device, as a new tensor: channel 0 the centre logit, channels 1 .. 4 the displacements
        (dx_s, dy_s, dx_e, dy_e) -- channels 7 .. 11 of the network's output; channels 5 .. 7 are zero."""
        src = self._frames(frames)
        return self._run(src, None, None, 1).clone()

    def edges(self, frames, out=None):
        """frames: a list of PIL images / uint8 arrays of one size, or a uint8 tensor [n, H, W, C] (no host copy when it is on the
        device) -> uint8 device tensor [n, H, W] (the detector's map: 0, lines 255), written into `out` when given."""
        return self._uint8_out(frames, out)
