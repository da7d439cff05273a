"""The normalbae annotator (SampleConfigIPAdapter.yaml of the reference lists lllyasviel/control_v11p_sd15_normalbae, whose control
frames come from controlnet_aux's NormalBaeDetector, modules/controlresiduals_pipeline.py:97-150) on the GPU, for a whole window of
frames at once: surface normals as an RGB map.

The network is NNET (Bae et al.): a tf_efficientnet_b5_ap encoder without pool and classifier, and a decoder whose last three stages
are per-pixel MLPs over bilinearly upsampled features.  In geffnet's naming, with c = the block's input channels:

    stem        conv_stem 3 -> 48, 3x3 stride 2 SAME; bn1; swish                                                       (1/2)
    stage 0     3 x DepthwiseSeparable: conv_dw k3, bn1, swish, se(c / 4), conv_pw, bn2 (+ x)             24 ch        (1/2)   tap
    stage 1..6  InvertedResidual: conv_pw c -> 6c, bn1, swish, conv_dw k SAME, bn2, swish, se(c / 4), conv_pwl, bn3 (+ x where stride 1
                and in = out): 5 x k3 s2 -> 40 (1/4, tap), 5 x k5 s2 -> 64 (1/8, tap), 7 x k3 s2 -> 128 (1/16), 7 x k5 -> 176 (1/16, tap),
                9 x k5 s2 -> 304 (1/32), 3 x k3 -> 512 (1/32)
    head        conv_head 512 -> 2048, 1x1: its output BEFORE bn2 and the activation is the fifth tap                  (1/32)
    decoder     conv2 2048 -> 2048 (1x1, bias); up1 .. up4: bilinear x2 (align_corners) to the skip's size, cat(up, skip), twice (3x3 conv,
                BN, LeakyReLU(0.01)): 2224 -> 1024, 1088 -> 512, 552 -> 256, 280 -> 128
    res8        out_conv_res8 3x3 512 -> 4 on x_d2 (1/8), norm_normalize
    res4, 2, 1  cat(up(x_d2 | x_d3 | x_d4), up(previous prediction)) -> per-pixel MLP (C + 4) -> 128 -> 128 -> 128 -> 4 (ReLU), norm_normalize
    norm_normalize: xyz / (sqrt(x^2 + y^2 + z^2) + 1e-10), kappa = elu(k) + 1 + 0.01

BatchNorm (eps 1e-3 in the encoder, 1e-5 in the decoder) is folded on the host in fp32 and the result rounded once.  It runs as (the
names are the keys of `timings`):

    stem     ca_nbae_stem: uint8 frames -> 48 channels at half size, the ImageNet normalisation and the SAME padding folded in
    encoder  per block ca_gemm (expansion, CA_ACT_SILU), ca_dwconv_same (depthwise + swish + the pooled sums of what it stored),
             ca_se_gate, ca_scale_channels (in place), ca_gemm (projection, with the block's residual); conv_head is a ca_gemm
    decoder  ca_gemm (conv2, in column blocks of 1024), ca_upsample2x_bilinear_ac, ca_conv3x3 with the skip as its second source
             (CA_ACT_LEAKY001), out_conv_res8 as ca_conv3x3 with Cout padded to 8 and fp32 output, ca_nbae_normalize
    refine   per stage ca_nbae_refine (context.dispatch.nbae_refine_fused, C = 128 / 256 / 512): one launch, the interpolated row and the
             128-wide hidden activations in LDS, four layers on the MFMA, norm_normalize; or the composed form: ca_upsample2x_bilinear_ac,
             ca_nbae_cat_pred (the fp32 prediction interpolated in fp32 into the eight columns of the MLP's second source), three ca_gemm
             (CA_ACT_RELU), a fourth with fp32 output, ca_nbae_normalize
    finish   ca_nbae_finish: xyz -> the uint8 map and / or the control tensor

The four-channel predictions stay fp32 from stage to stage.  No device-to-host read anywhere: the chain can be captured in a hipGraph.

The specification is tests/normalbae_ref.py (the fp32 torch network and the numpy tail, restated from the published code).
controlnet_aux, geffnet and OpenCV are third-party packages that are absent here, and no scannet.pt is available: key names and parity
with them are UNPINNED.  The encoder's arithmetic is pinned against transformers' EfficientNetModel (tests/golden/normalbae_tiny.npz).
The range of the fp16 activations on the trained weights is unmeasured (no checkpoint here); dtype=torch.bfloat16 is the escape.

Scope of sizes: min(H, W) == detect_resolution == image_resolution and H % 64 == W % 64 == 0 (512 x 512, 512 x 768, 768 x 512 at the
default 512), for which every resampling of the detector is the identity; anything else raises NotImplementedError.  No CPU fallback.
"""
from __future__ import annotations

import os
from typing import NamedTuple

import numpy as np

from . import annotator_base as _base
from .annotator_base import AnnotatorBase, bn_key_shapes as _bn, check_state_dict as _check_state_dict, fold_bn, pack_conv, pack_pointwise

WEIGHTS_NAME = "scannet.pt"
ENCODER_BN_EPS, DECODER_BN_EPS = 1e-3, 1e-5
TAP_STAGES = (0, 1, 2, 4)
STAGES = ("stem", "encoder", "decoder", "refine", "finish")   # the keys of `timings`
UP_MAX_C = 1024   # ca_upsample2x_bilinear_ac takes up to 1024 channels per launch: conv2 runs in column blocks of that


class Geometry(NamedTuple):
    stem: int
    stages: tuple      # per stage (width, repeats, kernel, stride, expansion)
    head: int          # conv_head's width
    decoder: int       # conv2's width; up1 .. up4 give decoder / 2, / 4, / 8, / 16
    hidden: int = 128  # the width of the refinement MLPs


B5 = Geometry(48, ((24, 3, 3, 1, 1), (40, 5, 3, 2, 6), (64, 5, 5, 2, 6), (128, 7, 3, 2, 6), (176, 7, 5, 1, 6), (304, 9, 5, 2, 6), (512, 3, 3, 1, 6)), 2048, 2048)


def check_geometry(geo) -> None:
    ok = (len(geo.stages) == 7 and 8 <= geo.stem <= 64 and geo.stem % 8 == 0 and geo.head % 8 == 0 and geo.decoder % 128 == 0 and geo.hidden % 8 == 0
          and [s[3] for s in geo.stages] == [1, 2, 2, 2, 1, 2, 1] and all(s[0] % 8 == 0 and s[1] >= 1 and s[2] in (3, 5) and s[4] >= 1 for s in geo.stages)
          and max(s[0] * s[4] for s in geo.stages) <= 3072 and max(s[0] for s in geo.stages) // 4 <= 256)
    if not ok:
        raise ValueError(f"geometry out of the kernels' range (seven stages with strides 1, 2, 2, 2, 1, 2, 1, widths multiples of 8, expanded width <= 3072, "
                         f"decoder a multiple of 128): {geo}")


def blocks_of(geo):
    """[(stage, index in stage, cin, cout, kernel, stride, expansion, se width)]: the squeeze width is a quarter of the block's input."""
    out, cin = [], geo.stem
    for s, (width, repeats, kernel, stride, expand) in enumerate(geo.stages):
        for b in range(repeats):
            out.append((s, b, cin, width, kernel, stride if b == 0 else 1, expand, max(1, cin // 4)))
            cin = width
    return out


def decoder_widths(geo):
    """(the taps' widths at 1/2, 1/4, 1/8, 1/16; x_d1 .. x_d4's widths)."""
    return [geo.stages[s][0] for s in TAP_STAGES], [geo.decoder >> i for i in (1, 2, 3, 4)]


def normalbae_key_shapes(geo=B5) -> dict:
    """Every tensor of scannet.pt's "model" entry that the chain uses: name -> shape."""
    e = "encoder.original_model"
    out = {f"{e}.conv_stem.weight": (geo.stem, 3, 3, 3), **_bn(f"{e}.bn1", geo.stem)}
    for s, b, cin, cout, k, _, expand, r in blocks_of(geo):
        p, mid = f"{e}.blocks.{s}.{b}", cin * expand
        se = {f"{p}.se.conv_reduce.weight": (r, mid, 1, 1), f"{p}.se.conv_reduce.bias": (r,), f"{p}.se.conv_expand.weight": (mid, r, 1, 1),
              f"{p}.se.conv_expand.bias": (mid,)}
        if expand == 1:
            out[f"{p}.conv_dw.weight"] = (cin, 1, k, k)
            out.update(_bn(f"{p}.bn1", cin))
            out.update(se)
            out[f"{p}.conv_pw.weight"] = (cout, cin, 1, 1)
            out.update(_bn(f"{p}.bn2", cout))
        else:
            out[f"{p}.conv_pw.weight"] = (mid, cin, 1, 1)
            out.update(_bn(f"{p}.bn1", mid))
            out[f"{p}.conv_dw.weight"] = (mid, 1, k, k)
            out.update(_bn(f"{p}.bn2", mid))
            out.update(se)
            out[f"{p}.conv_pwl.weight"] = (cout, mid, 1, 1)
            out.update(_bn(f"{p}.bn3", cout))
    out[f"{e}.conv_head.weight"] = (geo.head, geo.stages[-1][0], 1, 1)
    taps, xd = decoder_widths(geo)
    out["decoder.conv2.weight"], out["decoder.conv2.bias"] = (geo.decoder, geo.head, 1, 1), (geo.decoder,)
    cin = geo.decoder
    for i in range(4):
        p = f"decoder.up{i + 1}._net"
        out[f"{p}.0.weight"], out[f"{p}.0.bias"] = (xd[i], cin + taps[3 - i], 3, 3), (xd[i],)
        out.update(_bn(f"{p}.1", xd[i]))
        out[f"{p}.3.weight"], out[f"{p}.3.bias"] = (xd[i], xd[i], 3, 3), (xd[i],)
        out.update(_bn(f"{p}.4", xd[i]))
        cin = xd[i]
    out["decoder.out_conv_res8.weight"], out["decoder.out_conv_res8.bias"] = (4, xd[1], 3, 3), (4,)
    for name, c in (("res4", xd[1]), ("res2", xd[2]), ("res1", xd[3])):
        p = f"decoder.out_conv_{name}"
        for j, (co, ci) in zip((0, 2, 4, 6), ((geo.hidden, c + 4), (geo.hidden, geo.hidden), (geo.hidden, geo.hidden), (4, geo.hidden))):
            out[f"{p}.{j}.weight"], out[f"{p}.{j}.bias"] = (co, ci, 1), (co,)
    return out


def strip_module_prefix(sd) -> dict:
    """The state dict without the `module.` prefix of a DataParallel checkpoint (what the detector strips)."""
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}


def _ignored(k: str) -> bool:
    # what the detector's encoder holds but never runs on the way to the decoder's taps: bn2 behind conv_head, the classifier
    e = "encoder.original_model."
    return k.endswith("num_batches_tracked") or k.startswith(e + "bn2.") or k.startswith(e + "classifier.")


def check_state_dict(sd, geo=B5) -> None:
    """KeyError naming a missing tensor, ValueError naming one that is unexpected or has the wrong shape."""
    _check_state_dict(sd, normalbae_key_shapes(geo), "normalbae", "encoder.original_model.{conv_stem, bn1, blocks.S.B, conv_head} and "
                      "decoder.{conv2, up1 .. up4, out_conv_res8, out_conv_res4 / 2 / 1}", ignore=_ignored)


def pack_depthwise(w):
    """Depthwise weight [C, 1, k, k] -> [k * k, C]: tap ky * k + kx of every channel (ca_dwconv_same)."""
    return _base.pack_depthwise(w, (3, 5), "[C, 1, k, k] with k = 3 or 5")


def pack_stem(w):
    """conv_stem weight [cout, 3, 3, 3] (BatchNorm folded) -> float32 [27, cout]: row (ky * 3 + kx) * 3 + channel (ca_nbae_stem)."""
    if w.dim() != 4 or tuple(w.shape[1:]) != (3, 3, 3):
        raise ValueError(f"a Conv2d weight [cout, 3, 3, 3] is expected, got {tuple(w.shape)}")
    return w.detach().float().permute(2, 3, 1, 0).reshape(27, w.shape[0]).contiguous()


def pack_network(sd, geo, dtype) -> dict:
    """The packed weights of the chain as a tree of host tensors (BatchNorm folded in fp32, rounded once to dtype where a kernel reads dtype)."""
    e = "encoder.original_model"

    def plain(name):
        return sd[name + ".weight"].detach().float(), sd[name + ".bias"].detach().float()

    stem = fold_bn(sd, f"{e}.conv_stem", f"{e}.bn1", ENCODER_BN_EPS)
    out = {"stem": (pack_stem(stem[0]), stem[1].contiguous()), "blocks": []}
    for s, b, cin, cout, k, stride, expand, r in blocks_of(geo):
        p, blk = f"{e}.blocks.{s}.{b}", {}
        if expand == 1:
            dw, proj = fold_bn(sd, f"{p}.conv_dw", f"{p}.bn1", ENCODER_BN_EPS), fold_bn(sd, f"{p}.conv_pw", f"{p}.bn2", ENCODER_BN_EPS)
        else:
            blk["expand"] = pack_pointwise(fold_bn(sd, f"{p}.conv_pw", f"{p}.bn1", ENCODER_BN_EPS), dtype)
            dw, proj = fold_bn(sd, f"{p}.conv_dw", f"{p}.bn2", ENCODER_BN_EPS), fold_bn(sd, f"{p}.conv_pwl", f"{p}.bn3", ENCODER_BN_EPS)
        blk["dw"] = (pack_depthwise(dw[0]).to(dtype), dw[1].contiguous())
        wr, br = plain(f"{p}.se.conv_reduce")
        we, be = plain(f"{p}.se.conv_expand")
        blk["se"] = (wr.reshape(r, -1).contiguous(), br.contiguous(), we.reshape(-1, r).t().contiguous(), be.contiguous())
        blk["project"] = pack_pointwise(proj, dtype)
        out["blocks"].append(blk)
    out["head"] = pack_pointwise((sd[f"{e}.conv_head.weight"], None), dtype)
    w2, b2 = plain("decoder.conv2")
    w2 = w2.reshape(geo.decoder, geo.head)
    out["conv2"] = [(w2[i:i + UP_MAX_C].contiguous().to(dtype), b2[i:i + UP_MAX_C].contiguous()) for i in range(0, geo.decoder, UP_MAX_C)]
    out["up"] = []
    for i in range(4):
        p = f"decoder.up{i + 1}._net"
        out["up"].append(tuple(pack_conv(fold_bn(sd, f"{p}.{j}", f"{p}.{j + 1}", DECODER_BN_EPS), dtype) for j in (0, 3)))
    out["res8"] = pack_conv(plain("decoder.out_conv_res8"), dtype, cout_pad=8)   # Cout 4 -> 8, the new ones zero
    mlps = [[plain(f"decoder.out_conv_{name}.{j}") for j in (0, 2, 4, 6)] for name in ("res4", "res2", "res1")]
    out["mlp"] = [pack_mlp(m, dtype) for m in mlps]
    out["mlp_frag"] = [pack_mlp_frag(m, dtype) for m in mlps]   # (None per stage whose widths ca_nbae_refine is not built for)
    return out


def pack_mlp(layers, dtype) -> list:
    """The four (weight [Cout, Cin, 1], bias) pairs of a refinement stage's MLP (C + 4) -> hidden -> hidden -> hidden -> 4 as ca_gemm reads
    them: [Cout, Cin] of dtype and fp32 bias, the first layer's K padded from C + 4 to C + 8 and the last layer's N from 4 to 8 with zeros."""
    import torch
    F = torch.nn.functional
    (w0, b0), (w1, b1), (w2, b2), (w3, b3) = [(w.detach().float().reshape(w.shape[0], -1), b.detach().float()) for w, b in layers]
    if w3.shape[0] != 4 or w0.shape[1] % 8 != 4 or not (w0.shape[0] == w1.shape[1] == w1.shape[0] == w2.shape[1] == w2.shape[0] == w3.shape[1]) or w0.shape[0] % 8:
        raise ValueError(f"an MLP (C + 4) -> hidden -> hidden -> hidden -> 4 with C and hidden multiples of 8 is expected, got {[tuple(w.shape) for w, _ in layers]}")
    return [(F.pad(w0, (0, 4)).contiguous().to(dtype), b0.contiguous()), (w1.contiguous().to(dtype), b1.contiguous()), (w2.contiguous().to(dtype), b2.contiguous()),
            (F.pad(w3, (0, 0, 0, 4)).contiguous().to(dtype), F.pad(b3, (0, 4)).contiguous())]


def pack_mlp_frag(layers, dtype):
    """The same four (weight, bias) pairs as ca_nbae_refine reads them, or None where it is not built for the widths (C in 128 / 256 / 512,
    hidden 128): ([four MFMA-fragment tensors of dtype], [four fp32 biases]).  Fragment (ks, t) of a weight [N, K] (K padded with zeros to
    a multiple of 32; the first layer's C + 4 to the multiple at or above C + 8; the last layer's N = 4 to 16) is 64 lanes x 8 elements:
    element ((ks * N / 16 + t) * 64 + lane) * 8 + e = W[t * 16 + lane % 16][ks * 32 + lane // 16 * 8 + e]."""
    import torch
    F = torch.nn.functional
    ws = [w.detach().float().reshape(w.shape[0], -1) for w, _ in layers]
    c, hidden = ws[0].shape[1] - 4, ws[0].shape[0]
    if c not in (128, 256, 512) or hidden != 128 or ws[3].shape[0] != 4:
        return None
    kp = (c + 8 + 31) // 32 * 32
    ws[0] = F.pad(ws[0], (0, kp - (c + 4)))
    ws[3] = F.pad(ws[3], (0, 0, 0, 12))
    frags = []
    for w in ws:
        n, k = w.shape
        frags.append(w.reshape(n // 16, 16, k // 32, 4, 8).permute(2, 0, 3, 1, 4).contiguous().reshape(-1).to(dtype))
    return frags, [b.detach().float().contiguous() for _, b in layers]


def refine_stage(feat, pred, layers, out=None, raw=None, take=None, give=None, timed=None, frag=None):
    """One refinement stage: feat [n, h, w, C] and the fp32 prediction pred [n, h, w, 4] -> out fp32 [n, 2h, 2w, 4].  With frag
    (pack_mlp_frag's) and context.dispatch.nbae_refine_fused: one launch of ca_nbae_refine.  Else the composed form:
    ca_upsample2x_bilinear_ac, ca_nbae_cat_pred, three ca_gemm (CA_ACT_RELU), a fourth with fp32 output, ca_nbae_normalize.  layers:
    pack_mlp's; raw: fp32 scratch of n * 2h * 2w * 8 floats; take / give: a BufferPlan's (None: fresh tensors); timed: HipStages._timed."""
    import torch
    from . import kernels as K
    from .context import dispatch
    n, h, w, c = feat.shape
    m = n * 4 * h * w
    if frag is not None and dispatch.nbae_refine_fused:
        out = torch.empty((n, 2 * h, 2 * w, 4), dtype=torch.float32, device=feat.device) if out is None else out
        run = timed or (lambda name, fn, *a, **kw: fn(*a, **kw))
        return run("refine", K.nbae_refine, feat, pred, frag[0], frag[1], out)
    take = take or (lambda *shape: torch.empty(shape, dtype=feat.dtype, device=feat.device))
    give = give or (lambda t: None)
    timed = timed or (lambda name, fn, *a, **kw: fn(*a, **kw))
    out = torch.empty((n, 2 * h, 2 * w, 4), dtype=torch.float32, device=feat.device) if out is None else out
    raw = torch.empty(m * 8, dtype=torch.float32, device=feat.device) if raw is None else raw
    f = timed("refine", K.upsample2x_bilinear_ac, feat, take(n, 2 * h, 2 * w, c))
    pc = timed("refine", K.nbae_cat_pred, pred, take(n, 2 * h, 2 * w, 8))
    x = take(m, layers[0][0].shape[0])
    timed("refine", K.gemm, f.view(m, c), layers[0][0], a2=pc.view(m, 8), bias=layers[0][1], act=K.ACT_RELU, out=x)
    give(f)
    give(pc)
    for wb in layers[1:3]:
        y = take(m, wb[0].shape[0])
        timed("refine", K.gemm, x, wb[0], bias=wb[1], act=K.ACT_RELU, out=y)
        give(x)
        x = y
    raw = raw[:m * 8].view(m, 8)
    timed("refine", K.gemm, x, layers[3][0], bias=layers[3][1], out_f32=True, out=raw)
    give(x)
    return timed("refine", K.nbae_normalize, raw, out)


class NormalBaeAnnotator(AnnotatorBase):
    """`NormalBaeAnnotator(weights)(image)`: PIL in, PIL RGB out (the normal map: x, y, z as red, green, blue); an array in, an array out.
    `normals(frames, out=None)` gives the uint8 map [n, H, W, 3] on the device, `annotate_batch(frames, out=, rep=, dtype=)` the control
    tensor, so it plugs into `MultiControlNetResidualsPipeline(annotators={"normalbae": NormalBaeAnnotator.from_pretrained(path)})`, whose
    `prep_control_images` then calls `annotate_batch` once per list of frames.  Nothing makes it a default: the weights are the user's
    file.  Non-uint8 input raises TypeError, frames of different sizes ValueError, sizes out of scope NotImplementedError -- all before
    the device is touched; without the library or a GPU a call raises CAHipUnavailable (there is no CPU fallback)."""

    WEIGHTS_NAME = WEIGHTS_NAME
    STAGES = STAGES

    def __init__(self, state_dict_or_path, device=None, dtype=None, detect_resolution: int = 512, geometry=B5):
        import torch
        dtype = torch.float16 if dtype is None else dtype
        if dtype not in (torch.float16, torch.bfloat16):
            raise TypeError(f"dtype must be torch.float16 or torch.bfloat16, got {dtype}")
        if detect_resolution < 64 or detect_resolution % 64:
            raise NotImplementedError(f"NormalBaeAnnotator takes a detect_resolution (= image_resolution) that is a multiple of 64; got {detect_resolution}")
        check_geometry(geometry)
        sd = self._load(state_dict_or_path) if isinstance(state_dict_or_path, (str, os.PathLike)) else state_dict_or_path
        if isinstance(sd.get("model"), dict):   # scannet.pt: {"model": state dict, ...}
            sd = sd["model"]
        sd = strip_module_prefix(sd)
        check_state_dict(sd, geometry)
        self.device, self.dtype, self.geometry, self.resolution = device, dtype, geometry, int(detect_resolution)
        # the largest operand of a chunk of frames, in bytes per frame pixel: the full-resolution planes of the last refinement stage (the
        # upsampled x_d4 and the hidden activations), the concatenation of up4 at half size, the widest expansion of the encoder at its size
        _, xd = decoder_widths(geometry)
        per_pixel = [2 * max(xd[3], geometry.hidden), 2 * 2 * xd[3] / 4]
        for s, _, cin, _, _, _, expand, _ in blocks_of(geometry):
            per_pixel.append(2 * cin * expand / 4 ** (1 + sum(st[3] == 2 for st in geometry.stages[:s])))   # (the expansion lies in front of the stride)
        self._bytes_per_pixel = int(np.ceil(max(per_pixel)))
        self._host = pack_network(sd, geometry, dtype)
        self._ws = {}   # (`timings` receives events under the keys of STAGES -- tools/bench_normalbae.py)

    @classmethod
    def from_pretrained(cls, path, detect_resolution: int = 512, dtype=None, geometry=B5, **kwargs):
        """path: a local scannet.pt or a directory that holds it (no network access, ever)."""
        return cls(cls._load(path), detect_resolution=detect_resolution, dtype=dtype, geometry=geometry, **kwargs)

    # ---- device state ----------------------------------------------------------------------------------------------------------
    def workspace(self, n: int, h: int, w: int) -> dict:
        """The buffers of a call with n frames of h x w pixels, cached per (n, h, w): the fp32 predictions ("pred": the last stage's, for all n
        frames; "pred8", "pred4", "pred2" and "raw" for a chunk), the squeeze-and-excite scratch ("sums", "gate", "partials") and a pool of
        activation buffers that the layers of a pass take and give back in a fixed order (contents are never assumed; the first pass
        allocates them and every later pass reuses the same ones)."""
        import torch
        from . import kernels as K
        from .context import dispatch

        def make(dev):
            m = min(n, self.chunk_frames(h, w))
            geo = self.geometry
            cmax, partials, hh, ww = 8, 1, h // 2, w // 2
            for _, _, cin, _, _, stride, expand, _ in blocks_of(geo):
                cmax = max(cmax, cin * expand)
                partials = max(partials, K.dwconv_same_partials_floats(m, hh, ww, cin * expand, stride))
                hh, ww = hh // stride, ww // stride

            def f32(*shape):
                return torch.empty(shape, dtype=torch.float32, device=dev)

            return {"pred": f32(n, h, w, 4), "pred8": f32(m, h // 8, w // 8, 4), "pred4": f32(m, h // 4, w // 4, 4), "pred2": f32(m, h // 2, w // 2, 4),
                    "raw": f32(m * h * w * 8), "sums": f32(m * cmax), "gate": f32(m * cmax), "partials": f32(partials)}

        # (the two forms of the refinement stages take different buffers: a plan each)
        return self._workspace((n, h, w, bool(dispatch.nbae_refine_fused)), make)

    # ---- input checks ----------------------------------------------------------------------------------------------------------
    def _check_size(self, h: int, w: int) -> None:
        r = self.resolution
        if min(h, w) != r or h % 64 or w % 64:
            raise NotImplementedError(
                f"NormalBaeAnnotator takes frames with min(H, W) == detect_resolution == image_resolution (= {r}) and H % 64 == W % 64 == 0, for "
                f"which every resampling of the detector is the identity; got {h} x {w}")

    # ---- the chain -------------------------------------------------------------------------------------------------------------
    def _network(self, src, ws, i0: int, taps_out=None) -> None:
        """The network for the frames `src` (a chunk), the last prediction into ws["pred"][i0 : i0 + len(src)].  taps_out: a list that receives
        clones of the five encoder taps (tests)."""
        from . import kernels as K
        wts = self._weights(src.device)
        geo = self.geometry
        n, h, w, _ = src.shape
        with self._pass(ws, src.device) as p:   # the same buffers in the same order on every pass
            take, give, launch, pw = p.take, p.give, p.launch, p.pointwise
            x = launch("stem", K.nbae_stem, src, wts["stem"][0], wts["stem"][1], take(n, h // 2, w // 2, geo.stem))
            taps = []
            for (s, b, cin, cout, _, stride, expand, _), blk in zip(blocks_of(geo), wts["blocks"]):
                t = pw("encoder", x, blk["expand"], K.ACT_SILU) if expand != 1 else x
                _, hh, ww, mid = t.shape
                ho, wo = K.same_out(hh, stride), K.same_out(ww, stride)
                sums, gate = ws["sums"][:n * mid].view(n, mid), ws["gate"][:n * mid].view(n, mid)
                d, _ = launch("encoder", K.dwconv_same, t, blk["dw"][0], blk["dw"][1], stride=stride, out=take(n, ho, wo, mid), sums=sums, partials=ws["partials"])
                if expand != 1:
                    give(t)
                launch("encoder", K.se_gate, sums, *blk["se"], ho * wo, out=gate)
                launch("encoder", K.scale_channels, d, gate, out=d)
                y = pw("encoder", d, blk["project"], residual=x if (stride == 1 and cin == cout) else None)
                give(d)
                if not any(x is tp for tp in taps):   # a tap stays until the decoder has read it
                    give(x)
                x = y
                if b == geo.stages[s][1] - 1 and s in TAP_STAGES:
                    taps.append(x)
            head = pw("encoder", x, wts["head"])
            give(x)
            if taps_out is not None:
                taps_out.extend(tp.clone() for tp in taps + [head])
            # ---- decoder
            parts = [pw("decoder", head, wb) for wb in wts["conv2"]]
            give(head)
            xd = []
            for i, (c1, c2) in enumerate(wts["up"]):
                skip = taps[3 - i]
                nn, hh, ww, _ = skip.shape
                up = take(nn, hh, ww, sum(pt.shape[3] for pt in parts))
                col = 0
                for pt in parts:
                    launch("decoder", K.upsample2x_bilinear_ac, pt, up, col)
                    col += pt.shape[3]
                t = p.conv3x3("decoder", up, c1, act=K.ACT_LEAKY001, x2=skip)
                give(up)
                give(skip)
                if i < 2:   # conv2's output and x_d1 are done; x_d2 and x_d3 stay for their refinement stages
                    for pt in parts:
                        give(pt)
                y = p.conv3x3("decoder", t, c2, act=K.ACT_LEAKY001)
                give(t)
                xd.append(y)
                parts = [y]
            nn, h8, w8, _ = xd[1].shape
            raw8 = ws["raw"][:nn * h8 * w8 * 8].view(nn, h8, w8, 8)
            launch("decoder", K.conv3x3, xd[1], wts["res8"][0], bias=wts["res8"][1], out_f32=True, out=raw8)
            pred = launch("decoder", K.nbae_normalize, raw8.view(-1, 8), ws["pred8"][:nn])
            # ---- the three refinement stages
            outs = (ws["pred4"][:nn], ws["pred2"][:nn], ws["pred"][i0:i0 + nn])
            for feat, layers, frag, out in zip(xd[1:], wts["mlp"], wts["mlp_frag"], outs):
                pred = refine_stage(feat, pred, layers, out=out, raw=ws["raw"], take=take, give=give, timed=launch, frag=frag)
                give(feat)

    def _run(self, src, map, control, rep):
        from . import kernels as K
        n, h, w, _ = src.shape
        ws = self.workspace(n, h, w)
        for i0, sl in self._chunks(n, self.chunk_frames(h, w)):
            self._network(src[sl], ws, i0)
        if map is not None or control is not None:
            self._timed("finish", K.nbae_finish, ws["pred"], map=map, control=control, rep=rep)
        return ws["pred"]

    def prediction(self, frames):
        """-> float32 [n, H, W, 4] on the device, as a new tensor: the last stage's unit normal (x, y, z) and kappa."""
        src = self._frames(frames)
        return self._run(src, None, None, 1).clone()

    def encoder_taps(self, frames):
        """-> the five tensors the decoder reads (NHWC, new tensors): the outputs of stages 0, 1, 2 and 4 and conv_head's (tests)."""
        src = self._frames(frames)
        n, h, w, _ = src.shape
        if n > self.chunk_frames(h, w):
            raise ValueError("encoder_taps takes what fits one pass")
        taps = []
        self._network(src, self.workspace(n, h, w), 0, taps_out=taps)
        return taps

    def normals(self, frames, out=None):
        """frames: a list of PIL images / uint8 arrays of one size, or a uint8 tensor [n, H, W, C] (no host copy when it is on the
        device) -> uint8 device tensor [n, H, W, 3] (the detector's map), written into `out` when given."""
        return self._uint8_out(frames, out, channels_last=3)

    def __call__(self, image):
        """PIL in, PIL RGB out; an array in, an array out."""
        try:
            from PIL import Image
        except Exception:  # pragma: no cover
            Image = None
        rgb = self.normals([image])[0].cpu().numpy()
        return Image.fromarray(rgb) if Image is not None and not isinstance(image, np.ndarray) else rgb
