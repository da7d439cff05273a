"""The softedge annotator of the reference's SampleConfigIPAdapter.yaml (it lists lllyasviel/control_v11p_sd15_softedge, whose control
frames come from controlnet_aux's PidiNetDetector, modules/controlresiduals_pipeline.py:62, 134-138) on the GPU, for a whole window of
frames at once.

The detector, as the reference calls it (detect_resolution = image_resolution = min(h, w), safe = False):

    input    RGB uint8, reversed to BGR, / 255
    network  PiDiNet(60, carv4, dil = 24, sa = True), unconverted: init_block (a `cd` pixel-difference convolution 3 -> 60) and fifteen
             PDCBlocks y = x + conv2(relu(conv1(x))) -- conv1 a depthwise pixel-difference convolution of type cd, ad, rd, cv in turn,
             conv2 1x1 -- at 60, 120, 240, 240 channels; the first block of levels 2 .. 4 sits behind MaxPool2d(2, 2) and has a biased
             1x1 shortcut.  Per level a CDCM (ReLU, 1x1 to 24, four 3x3 convolutions of dilation 5 / 7 / 9 / 11 summed), a CSAM
             (x * sigmoid(conv3x3(conv1x1(relu(x)))), one attention value per pixel) and a 1x1 reduction to one map; the four maps are
             resized bilinearly (align_corners = False) to the frame and mixed by a 1x1 classifier; the result is its sigmoid
    tail     optional safe step trunc(edge * 3) / 2, then (edge * 255).clip(0, 255).astype(uint8); three equal channels

The three difference operators are linear in x: fold_pdc turns each into a plain 3x3 (cd, ad) or 5x5 (rd) kernel once, on the host, in
fp32, and the BGR reversal becomes the order of init_block's input channels.  Channels are zero-padded once (60 -> 64, 120 -> 128,
240 -> 256, 24 -> 32, the input to 8; pad_state_dict): depthwise taps, rows and columns of every 1x1 and the shortcut biases of the
pad lanes are zero, so the lanes stay exactly zero through the chain.  It runs as (the keys of `timings`; STAGES holds the counts):

    prep       ca_softedge_prep: uint8 frames -> 8 channels
    init       ca_conv3x3 on the folded init_block weight, no bias, no activation
    block      ca_pdc_block: a stride-1 block at C = 64 in ONE launch (context.dispatch.pdc_block_fused; off, or at C = 128 / 256, the
               block is `depthwise` (ca_dwconv_k with ReLU) + `pointwise` (ca_gemm with the skip as its residual))
    pool       ca_maxpool2x2 in front of the first block of levels 2 .. 4; that block is `depthwise` + ONE `pointwise` GEMM over the
               K-concatenation [relu(dw(p)) | p] with [W2 | W_shortcut] and the shortcut's bias: no shortcut launch, no add
    relu       ca_relu in front of a CDCM (the next block reads the un-rectified tensor, so this is nobody's epilogue)
    pointwise  ... and the CDCM's 1x1 convolution with its bias
    cdcm       ca_cdcm_dil4: the four dilated convolutions as one MFMA accumulation
    csam       ca_csam_reduce: attention and reduction -> the fp32 side map
    fuse       ca_softedge_fuse: resize, classifier, sigmoid, safe step, quantisation -> the uint8 map and / or the control tensor

No device-to-host read anywhere; after the first pass nothing is allocated: the chain can be captured in a hipGraph.

The specification is tests/softedge_ref.py.  Key names and arithmetic are restated from memory of the published code (pidinet/model.py
and pidinet/__init__.py of controlnet_aux) and are UNPINNED: controlnet_aux and OpenCV are third-party packages that are absent here,
and no table5_pidinet.pth is available.  float16 is the default activation type and its range on the trained checkpoint is UNMEASURED
(the network has no normalisation layer: fifteen residual blocks can grow); dtype=torch.bfloat16 is the escape.

Scope of sizes: H and W multiples of 64 with detect_resolution = image_resolution = min(H, W), for which resize_image and the final
INTER_LINEAR resize are the identity; anything else raises NotImplementedError.  scribble and apply_filter are not part of this, nor is
the converted (convert_pidinet) checkpoint form.
"""
from __future__ import annotations

import os

from . import annotator_base as _base
from .annotator_base import AnnotatorBase, check_state_dict as _check_state_dict, pack_conv, pack_pointwise

WEIGHTS_NAME = "table5_pidinet.pth"
LAYER_TYPES = ("cd", "ad", "rd", "cv") * 4       # carv4; layer 0 is init_block
WIDTHS = (60, 120, 240, 240)
DIL = 24
PADDED = {3: 8, 60: 64, 120: 128, 240: 256, 24: 32}
AD_PERM = (3, 0, 1, 6, 4, 2, 7, 8, 5)
RD_PLUS = (0, 2, 4, 10, 14, 20, 22, 24)
RD_MINUS = (6, 7, 8, 11, 13, 16, 17, 18)


def blocks():
    """[(name, operator type, cin, cout, strided)] of the fifteen PDCBlocks in order."""
    out, cin, i = [], 60, 1
    for lv, count in ((1, 3), (2, 4), (3, 4), (4, 4)):
        for j in range(1, count + 1):
            cout = WIDTHS[lv - 1]
            out.append((f"block{lv}_{j}", LAYER_TYPES[i], cin, cout, lv > 1 and j == 1))
            cin, i = cout, i + 1
    return out


def stages(fused: bool = True) -> dict:
    """Launch groups per pass through the network, by the keys of `timings`."""
    one = 3 if fused else 0
    return {"prep": 1, "init": 1, "block": one, "pool": 3, "depthwise": 15 - one, "pointwise": 19 - one, "relu": 4, "cdcm": 4, "csam": 4, "fuse": 1}


STAGES = stages(True)


def softedge_key_shapes() -> dict:
    """Every tensor of table5_pidinet.pth (without the module. prefix): name -> shape."""
    out = {"init_block.weight": (60, 3, 3, 3)}
    for name, _, cin, cout, strided in blocks():
        out[f"{name}.conv1.weight"] = (cin, 1, 3, 3)
        out[f"{name}.conv2.weight"] = (cout, cin, 1, 1)
        if strided:
            out[f"{name}.shortcut.weight"] = (cout, cin, 1, 1)
            out[f"{name}.shortcut.bias"] = (cout,)
    for i, c in enumerate(WIDTHS):
        out[f"dilations.{i}.conv1.weight"], out[f"dilations.{i}.conv1.bias"] = (DIL, c, 1, 1), (DIL,)
        for k in range(1, 5):
            out[f"dilations.{i}.conv2_{k}.weight"] = (DIL, DIL, 3, 3)
        out[f"attentions.{i}.conv1.weight"], out[f"attentions.{i}.conv1.bias"] = (4, DIL, 1, 1), (4,)
        out[f"attentions.{i}.conv2.weight"] = (1, 4, 3, 3)
        out[f"conv_reduces.{i}.conv.weight"], out[f"conv_reduces.{i}.conv.bias"] = (1, DIL, 1, 1), (1,)
    out["classifier.weight"], out["classifier.bias"] = (1, 4, 1, 1), (1,)
    return out


def strip_state_dict(obj) -> dict:
    """The checkpoint as torch.load gives it ({"state_dict": {...}, ...} with module.-prefixed keys) or the bare dict -> the bare dict."""
    if isinstance(obj, dict) and "state_dict" in obj and isinstance(obj["state_dict"], dict):
        obj = obj["state_dict"]
    if not isinstance(obj, dict):
        raise ValueError("softedge state dict: not a state dict")
    return {(k[len("module."):] if isinstance(k, str) and k.startswith("module.") else k): v for k, v in obj.items()}


def check_state_dict(sd) -> None:
    """KeyError naming a missing tensor, ValueError naming one that is unexpected or has the wrong shape."""
    _check_state_dict(sd, softedge_key_shapes(), "softedge", "PiDiNet(60, carv4, dil=24, sa=True), unconverted")


def fold_pdc(w, kind: str):
    """A pixel-difference weight [.., .., 3, 3] of type `kind` -> the plain kernel that computes the same function of x in w's dtype:
    cd  conv(x, w) - conv1x1(x, sum w): the centre tap minus the sum of all nine                                  -> 3 x 3
    ad  conv(x, w - w.flat[[3, 0, 1, 6, 4, 2, 7, 8, 5]]): every outer tap minus its clockwise neighbour's weight   -> 3 x 3
    rd  flat positions 0 2 4 10 14 20 22 24 of a 5 x 5 take w.flat[1:], positions 6 7 8 11 13 16 17 18 take -w.flat[1:], the rest
        (the centre included) are zero                                                                              -> 5 x 5
    cv  w itself."""
    import torch
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise ValueError(f"a weight [.., .., 3, 3] is expected, got {tuple(w.shape)}")
    w = w.detach()
    if kind == "cv":
        return w.clone()
    if kind == "cd":
        out = w.clone()
        out[:, :, 1, 1] = w[:, :, 1, 1] - w.sum(dim=(2, 3))
        return out
    flat = w.reshape(w.shape[0], w.shape[1], 9)
    if kind == "ad":
        return (flat - flat[:, :, list(AD_PERM)]).reshape(w.shape)
    if kind == "rd":
        buf = torch.zeros(w.shape[0], w.shape[1], 25, dtype=w.dtype)
        buf[:, :, list(RD_PLUS)] = flat[:, :, 1:]
        buf[:, :, list(RD_MINUS)] = -flat[:, :, 1:]
        return buf.reshape(w.shape[0], w.shape[1], 5, 5)
    raise ValueError(f"operator type '{kind}' (cd, ad, rd or cv)")


def pad_state_dict(sd) -> dict:
    """The state dict with every channel count zero-padded (3 -> 8, 60 -> 64, 120 -> 128, 240 -> 256, 24 -> 32; 4 and 1 stay): the
    same network on the first channels, exact zeros on the rest."""
    import torch
    out = {}
    for k, v in sd.items():
        v = v.detach()
        depthwise = ".conv1.weight" in k and k.startswith("block")
        shape = list(v.shape)
        shape[0] = PADDED.get(shape[0], shape[0])
        if v.dim() == 4 and not depthwise:
            shape[1] = PADDED.get(shape[1], shape[1])
        p = torch.zeros(shape, dtype=v.dtype)
        p[tuple(slice(0, s) for s in v.shape)] = v
        out[k] = p
    return out


def folded_layers(sd) -> dict:
    """The network as fp32 plain convolutions in PyTorch layout, of whatever widths `sd` has: "init" [C, cin, 3, 3] with its first three
    input channels in RGB order (the detector's BGR reversal folded in); "blocks": [{"dw" [C, 1, k, k], "pw" [Cout, C, 1, 1],
    "shortcut"? (w, b)}]; "levels": [{"cdcm1" (w, b), "cdcm2" [4 weights], "csam1" (w, b), "csam2" w, "reduce" (w, b)}];
    "classifier" (w, b)."""
    f = {k: v.detach().float() for k, v in sd.items()}
    init = fold_pdc(f["init_block.weight"], "cd")
    order = [2, 1, 0] + list(range(3, init.shape[1]))
    out = {"init": init[:, order].contiguous(), "blocks": [], "levels": []}
    for name, kind, _, _, strided in blocks():
        blk = {"dw": fold_pdc(f[f"{name}.conv1.weight"], kind), "pw": f[f"{name}.conv2.weight"]}
        if strided:
            blk["shortcut"] = (f[f"{name}.shortcut.weight"], f[f"{name}.shortcut.bias"])
        out["blocks"].append(blk)
    for i in range(4):
        out["levels"].append({"cdcm1": (f[f"dilations.{i}.conv1.weight"], f[f"dilations.{i}.conv1.bias"]),
                              "cdcm2": [f[f"dilations.{i}.conv2_{k}.weight"] for k in range(1, 5)],
                              "csam1": (f[f"attentions.{i}.conv1.weight"], f[f"attentions.{i}.conv1.bias"]),
                              "csam2": f[f"attentions.{i}.conv2.weight"],
                              "reduce": (f[f"conv_reduces.{i}.conv.weight"], f[f"conv_reduces.{i}.conv.bias"])})
    out["classifier"] = (f["classifier.weight"], f["classifier.bias"])
    return out


def pack_depthwise(w):
    """Depthwise weight [C, 1, k, k] -> [k * k, C]: tap ky * k + kx of every channel (ca_dwconv_k, ca_pdc_block)."""
    return _base.pack_depthwise(w, (3, 5))


class SoftedgeAnnotator(AnnotatorBase):
    """`SoftedgeAnnotator(weights)(image)` has the contract of `annotators.canny(image)` (PIL in, PIL RGB with three equal channels out;
    an array in, an array out), so it plugs into `MultiControlNetResidualsPipeline(annotators={"softedge":
    SoftedgeAnnotator.from_pretrained(path)})`, whose `prep_control_images` then calls `annotate_batch` once per list of frames.  Nothing
    makes it a default: the weights are the user's file.  Non-uint8 input raises TypeError, frames of different sizes ValueError, sizes
    out of scope NotImplementedError -- all before the device is touched; without the library or a GPU a call raises CAHipUnavailable
    (there is no CPU fallback)."""

    # the largest operand of a chunk of frames (a 64-channel tensor at full resolution: 128 bytes per frame pixel) stays below what the
    # GEMM and convolution kernels address with 32-bit byte offsets
    _bytes_per_pixel = 128
    WEIGHTS_NAME = WEIGHTS_NAME

    def __init__(self, state_dict_or_path, device=None, dtype=None, safe: bool = False, scribble: bool = False, apply_filter: bool = False):
        import torch
        dtype = torch.float16 if dtype is None else dtype
        if dtype not in (torch.float16, torch.bfloat16):
            raise TypeError(f"dtype must be torch.float16 or torch.bfloat16, got {dtype}")
        if scribble or apply_filter:
            raise NotImplementedError("SoftedgeAnnotator: scribble and apply_filter are not part of this (the reference calls the detector without them)")
        sd = self._load(state_dict_or_path) if isinstance(state_dict_or_path, (str, os.PathLike)) else strip_state_dict(state_dict_or_path)
        check_state_dict(sd)
        self.device, self.dtype, self.safe = device, dtype, bool(safe)
        f = folded_layers(pad_state_dict(sd))

        def lin(w):   # [Cout, Cin, 1, 1] -> [Cout, Cin]
            return w.reshape(w.shape[0], -1).contiguous()

        blks = []
        for blk in f["blocks"]:
            b = {"dw": pack_depthwise(blk["dw"]).to(dtype)}
            if "shortcut" in blk:   # one GEMM over [relu(dw(p)) | p]
                b["pw"] = torch.cat([lin(blk["pw"]), lin(blk["shortcut"][0])], dim=1).contiguous().to(dtype)
                b["bias"] = blk["shortcut"][1].contiguous()
            else:
                b["pw"] = lin(blk["pw"]).to(dtype)
            blks.append(b)
        levels = []
        for lv in f["levels"]:
            levels.append({"cdcm1": pack_pointwise(lv["cdcm1"], dtype),
                           "cdcm2": torch.stack([w.permute(0, 2, 3, 1) for w in lv["cdcm2"]]).contiguous().to(dtype),   # [4, cout, ky, kx, cin]
                           "w1": lin(lv["csam1"][0]), "b1": lv["csam1"][1].contiguous(),
                           "w2": lv["csam2"].permute(0, 2, 3, 1)[0].contiguous(),                                     # [ky, kx, 4]
                           "wr": lv["reduce"][0].reshape(-1).contiguous(), "br": lv["reduce"][1].contiguous()})
        # packed once, on the host
        self._host = {"init": pack_conv((f["init"], None), dtype)[0], "blocks": blks, "levels": levels,
                      "classifier": torch.cat([f["classifier"][0].reshape(-1), f["classifier"][1].reshape(-1)]).contiguous()}
        self._ws = {}   # (`timings` receives events under the keys of STAGES -- tools/bench_softedge.py)

    @classmethod
    def _load(cls, path):   # (the checkpoint keeps its state dict under "state_dict": a non-dict is strip_state_dict's ValueError)
        import torch
        return strip_state_dict(torch.load(cls._weights_path(path), map_location="cpu", weights_only=True))

    # ---- device state ----------------------------------------------------------------------------------------------------------
    def workspace(self, n: int, h: int, w: int) -> dict:
        """The buffers of a call with n frames of h x w pixels, cached per (n, h, w): the four fp32 side maps [n, h >> k, w >> k], the
        fused logit, the CSAM's fp32 scratch (five floats per pixel of a chunk), the map that is written when only the control tensor is
        asked for, and a pool of activation buffers that the layers of a pass take and give back in a fixed order (contents are never
        assumed; the first pass allocates them and every later pass reuses the same ones)."""
        import torch
        return self._workspace((n, h, w), lambda dev: {
            "sides": [torch.empty((n, h >> k, w >> k), dtype=torch.float32, device=dev) for k in range(4)],
            "logit": torch.empty((n, h, w), dtype=torch.float32, device=dev),
            "scratch": torch.empty(5 * min(n, self.chunk_frames(h, w)) * h * w, dtype=torch.float32, device=dev), "fused": None})

    # ---- input checks ----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_size(h: int, w: int) -> None:
        if h < 64 or w < 64 or h % 64 or w % 64:
            raise NotImplementedError(
                f"SoftedgeAnnotator takes frames with H % 64 == W % 64 == 0 (detect_resolution = image_resolution = min(H, W), for which "
                f"every resampling of the detector is the identity); got {h} x {w}")

    # ---- the chain -------------------------------------------------------------------------------------------------------------
    def _network(self, src, ws, i0: int) -> None:
        """The network for the frames `src` (a chunk), the side maps into ws["sides"][k][i0 : i0 + len(src)]."""
        from . import kernels as K
        from .context import dispatch
        wts = self._weights(src.device)
        n, h, w, _ = src.shape
        fused = bool(dispatch.pdc_block_fused)
        if ws["fused"] != fused:   # the other form takes other buffers: plan again
            ws["planned"], ws["fused"] = False, fused
        with self._pass(ws, src.device) as p:   # the same buffers in the same order on every pass
            take, give, launch, pw = p.take, p.give, p.launch, p.pointwise

            def side(level, x):
                lv = wts["levels"][level]
                r = launch("relu", K.relu, x, take(*x.shape))
                t = pw("pointwise", r, lv["cdcm1"])
                give(r)
                f = launch("cdcm", K.cdcm_dil4, t, lv["cdcm2"], take(*t.shape))
                give(t)
                launch("csam", K.csam_reduce, f, lv["w1"], lv["b1"], lv["w2"], lv["wr"], lv["br"], side=ws["sides"][level][i0:i0 + n], scratch=ws["scratch"])
                give(f)

            x = launch("prep", K.softedge_prep, src, take(n, h, w, 8))
            y = p.conv3x3("init", x, (wts["init"], None))
            give(x)
            x, level = y, 0
            for (_, _, _, cout, strided), blk in zip(blocks(), wts["blocks"]):
                nn, hh, ww, cc = x.shape
                if strided:
                    side(level, x)
                    level += 1
                    pl = launch("pool", K.maxpool2x2, x, take(nn, hh // 2, ww // 2, cc))
                    give(x)
                    d = launch("depthwise", K.dwconv_k, pl, blk["dw"], relu=True, out=take(*pl.shape))
                    y = pw("pointwise", d, (blk["pw"], blk["bias"]), a2=pl)
                    give(d)
                    give(pl)
                elif fused and K.pdc_block_supported(cc, 3 if blk["dw"].shape[0] == 9 else 5):
                    y = launch("block", K.pdc_block, x, blk["dw"], blk["pw"], out=take(nn, hh, ww, cc), fused=True)
                    give(x)
                else:
                    d = launch("depthwise", K.dwconv_k, x, blk["dw"], relu=True, out=take(nn, hh, ww, cc))
                    y = pw("pointwise", d, (blk["pw"], None), residual=x)
                    give(d)
                    give(x)
                x = y
            side(level, x)
            give(x)

    def _run(self, src, edges, control, rep, logit=False):
        from . import kernels as K
        n, h, w, _ = src.shape
        ws = self.workspace(n, h, w)
        for i0, sl in self._chunks(n, self.chunk_frames(h, w)):
            self._network(src[sl], ws, i0)
        self._timed("fuse", K.softedge_fuse, ws["sides"], self._weights(src.device)["classifier"], safe=self.safe, logit=ws["logit"] if logit else None,
                    edges=edges, control=control, rep=rep)
        return ws

    def logits(self, frames) -> dict:
        """-> {"sides": the four side maps float32 [n, H >> k, W >> k] at their own resolution, "logit": the fused logit float32
        [n, H, W]} on the device, as new tensors (for tests)."""
        src = self._frames(frames)
        ws = self._run(src, None, None, 1, logit=True)
        return {"sides": [s.clone() for s in ws["sides"]], "logit": ws["logit"].clone()}

    def edges(self, frames, out=None):
        """frames: a list of PIL images / uint8 arrays of one size, or a uint8 tensor [n, H, W, C] (no host copy when it is on the
        device) -> uint8 device tensor [n, H, W] (the detector's map), written into `out` when given."""
        return self._uint8_out(frames, out)
