"""The depth annotator (the reference builds transformers.pipeline('depth-estimation'), whose default model is Intel/dpt-large, for every
ControlNet whose name contains "depth": modules/controlresiduals_pipeline.py:63, 94, 141-144) on the GPU, for a whole window of frames at
once.  The reference's own branch cannot run as written (:63 stores `depth_estimate_processor` while :94 and :141 read `depth_estimator`,
and :144 concatenates `image` instead of `o_image`); its evident intent is built: the pipeline's ['depth'] image, replicated to three
channels.

The chain, for frames of any size H x W (the names are the keys of `timings`):

    resize     ca_resize_pil_u8: Pillow's Image.resize to S x S (S = config.image_size), bilinear or bicubic, byte for byte
    vit        ca_dpt_patches (uint8 -> (x / 255 - 0.5) / 0.5 as patch rows) + the patch-embedding GEMM, then per layer what clip.CLIPEncoderLayer
               runs: ca_layernorm -> q|k|v ca_gemm -> ca_attention -> output GEMM (+ residual) -> ca_layernorm -> GEMM + erf-GELU -> GEMM
               (+ residual).  The hidden states after the backbone_out_indices layers are kept; DPT applies no final LayerNorm to them
    reassemble the readout GELU(W[:, :C] token + (W[:, C:] cls + b)) as a small GEMM over the n class tokens (a per-image row bias) and ONE
               ca_gemm(rowbias=, rows_per_group=tokens, act=GELU) over all rows (the torch.cat never exists; the class-token row of each image
               is computed along and skipped afterwards); the 1x1 projection; ConvTranspose2d(k = stride = 4 / 2) as one GEMM with N = k k Cout
               + ca_depth_to_space (no zero-stuffed tensor), a gather for the third stage, ca_conv3x3(stride 2) for the fourth
    fusion     neck.convs (ca_conv3x3 without bias); a pre-activation unit is ca_relu, ca_conv3x3(act=RELU), ca_conv3x3(residual=x); the 1x1
               projection runs BEFORE the align-corners x2 (its weights sum to 1, so a bias commutes with it: a quarter of the GEMM), then
               ca_upsample2x_bilinear_ac
    head       ca_conv3x3 (F -> F / 2), then kernels.dpt_head: the composed form (ca_upsample2x_bilinear_ac, ca_conv3x3 with ReLU and fp32
               output, ca_dpt_logit), or with context.dispatch.dpt_head_fused ca_dpt_head, one launch for the x2, the 3x3 -> 32 + ReLU and
               the 1x1 -> 1 + ReLU that never writes the upsampled plane -- 2.5x slower as measured, so not the default; float32 [n, S, S]
    tail       ca_resize_bicubic_f32 (torch's bicubic, align_corners False) back to H x W with the per-frame max / min kept on the device,
               ca_depth_finish: the uint8 map and / or the control tensor

No device-to-host read anywhere and no parallel branches: the chain can be captured in a hipGraph.  The head's logits and the whole tail are
float32; the rest runs in float16 (default) or bfloat16.  The activation range of the trained Intel/dpt-large in float16 is UNMEASURED (no
checkpoint is available here): dtype=torch.bfloat16 is the escape.

`normalize="max"` (default) is the depth-estimation pipeline of the reference's pinned transformers 4.34.1, (d * 255 / d.max()).astype(uint8),
restated and not run; "minmax" the installed one (5.15), ((d - min) / (max - min) * 255).astype(uint8).  Both truncate toward zero.  Under
"max" the bicubic undershoot makes a few percent of the pixels negative; numpy's cast of a value <= -1 to uint8 is platform-defined (it wraps
on x86), here it SATURATES to 0 -- a deliberate deviation.  An all-zero frame gives an all-zero map.

The specification is tests/depth_ref.py, pinned against the modules of transformers 5.15 and Pillow 12.2 by tests/golden/dpt_tiny*.npz.
Scope (anything else raises NotImplementedError): the plain-ViT DPT -- is_hybrid False, no backbone_config, readout_type "project",
reassemble_factors (4, 2, 1, 0.5), no batch norm in the fusion units, add_projection False, hidden_act "gelu"; processor settings do_resize
to a square size == image_size, keep_aspect_ratio False, ensure_multiple_of 1, do_pad False, mean = std = 0.5, resample 2 or 3.  The grid
then equals the trained one: the position embedding is never interpolated and the fusion layers never meet unequal shapes.  There is no
CPU fallback.
"""
from __future__ import annotations

import json
import math
import os
from types import SimpleNamespace

import numpy as np
import torch
from torch import nn

from .annotator_base import AnnotatorBase, HipStages
from .clip import _PackedModel
from .layers import HipConv1x1, HipConv3x3, HipLayerNorm, HipLinear, WeightArena, _f32, pack_concat_bias, pack_concat_rows

REASSEMBLE_FACTORS = (4, 2, 1, 0.5)
DPT_CONFIG = dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096, image_size=384, patch_size=16,
                  backbone_out_indices=(5, 11, 17, 23), neck_hidden_sizes=(256, 512, 1024, 1024), fusion_hidden_size=256, layer_norm_eps=1e-12,
                  head_in_index=-1)   # Intel/dpt-large
PIL_BILINEAR, PIL_BICUBIC = 2, 3
STAGES = ("resize", "vit", "reassemble", "fusion", "head", "tail")


def check_config(cfg: dict) -> None:
    """NotImplementedError for a DPTConfig outside the plain-ViT scope (the keys that are absent count as transformers' defaults)."""
    def no(what):
        raise NotImplementedError(f"DepthAnnotator runs the plain-ViT DPT only: {what}")

    if cfg.get("is_hybrid", False):
        no("is_hybrid=True (DPT-hybrid)")
    if cfg.get("backbone_config") is not None or cfg.get("backbone") is not None:
        no("a backbone_config / backbone (BEiT, Swin, DINOv2 ... backbones)")
    if cfg.get("readout_type", "project") != "project":
        no(f"readout_type={cfg.get('readout_type')!r} ('project')")
    if tuple(cfg.get("reassemble_factors", REASSEMBLE_FACTORS)) != REASSEMBLE_FACTORS:
        no(f"reassemble_factors={cfg.get('reassemble_factors')} ((4, 2, 1, 0.5))")
    if cfg.get("use_batch_norm_in_fusion_residual", False):
        no("use_batch_norm_in_fusion_residual=True")
    if cfg.get("use_bias_in_fusion_residual", None) is False:
        no("use_bias_in_fusion_residual=False")
    if cfg.get("add_projection", False):
        no("add_projection=True")
    if cfg.get("hidden_act", "gelu") != "gelu":
        no(f"hidden_act={cfg.get('hidden_act')!r} ('gelu')")
    if not cfg.get("qkv_bias", True):
        no("qkv_bias=False")
    if cfg.get("num_channels", 3) != 3:
        no(f"num_channels={cfg.get('num_channels')} (3)")
    if cfg.get("head_in_index", -1) != -1:
        no(f"head_in_index={cfg.get('head_in_index')} (-1)")
    full = dict(DPT_CONFIG)
    full.update(cfg)
    c, p, s = full["hidden_size"], full["patch_size"], full["image_size"]
    if isinstance(s, (list, tuple)) or isinstance(p, (list, tuple)) or p % 8 or s % p:
        no(f"image_size={s} patch_size={p} (a square image, patch_size a multiple of 8 that divides it)")
    if (s // p) % 2:
        no(f"an odd token grid {s // p} (the stride-2 stage and the x2 stages must meet at equal shapes)")
    if len(full["backbone_out_indices"]) != 4 or len(full["neck_hidden_sizes"]) != 4:
        no("four backbone_out_indices and four neck_hidden_sizes are expected")
    if c % full["num_attention_heads"] or (c // full["num_attention_heads"]) % 8 or c % 8 or full["intermediate_size"] % 8:
        no(f"hidden_size={c} with {full['num_attention_heads']} heads (widths and the head dimension must be multiples of 8)")
    if any(ch % 8 for ch in full["neck_hidden_sizes"]) or full["fusion_hidden_size"] % 16:
        no(f"neck_hidden_sizes={full['neck_hidden_sizes']} fusion_hidden_size={full['fusion_hidden_size']} (multiples of 8 / 16)")


def check_processor(pp: dict, image_size: int) -> int:
    """NotImplementedError for DPTImageProcessor settings outside the scope; -> the resample code (2 bilinear, 3 bicubic)."""
    def no(what):
        raise NotImplementedError(f"DepthAnnotator: image processor setting out of scope: {what}")

    if not pp.get("do_resize", True):
        no("do_resize=False")
    size = pp.get("size", {"height": 384, "width": 384})
    if isinstance(size, int):
        size = {"height": size, "width": size}
    if size.get("height") != image_size or size.get("width") != image_size:
        no(f"size={size} (a square equal to config.image_size = {image_size})")
    if pp.get("keep_aspect_ratio", False):
        no("keep_aspect_ratio=True")
    if pp.get("ensure_multiple_of", 1) != 1:
        no(f"ensure_multiple_of={pp.get('ensure_multiple_of')} (1)")
    if pp.get("do_pad", False):
        no("do_pad=True")
    if not pp.get("do_rescale", True) or not pp.get("do_normalize", True) or pp.get("do_reduce_labels", False):
        no("do_rescale / do_normalize must be on, do_reduce_labels off")
    if abs(pp.get("rescale_factor", 1 / 255) - 1 / 255) > 1e-12:
        no(f"rescale_factor={pp.get('rescale_factor')} (1 / 255)")
    for k in ("image_mean", "image_std"):
        v = pp.get(k, [0.5, 0.5, 0.5])
        if [float(x) for x in v] != [0.5, 0.5, 0.5]:
            no(f"{k}={v} (0.5, 0.5, 0.5)")
    resample = int(pp.get("resample", PIL_BICUBIC))
    if resample not in (PIL_BILINEAR, PIL_BICUBIC):
        no(f"resample={resample} (2 bilinear or 3 bicubic)")
    return resample


# ---- Pillow's coefficient tables (Resample.c: precompute_coeffs + normalize_coeffs_8bpc), in float64 on the host ------------------------
def _bilinear_filter(x: float) -> float:
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic_filter(x: float, a: float = -0.5) -> float:
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def pil_coeffs(in_size: int, out_size: int, resample: int):
    """-> (bounds int32 [out, 2]: first source index and number of taps; coefficients int32 [out, ksize] with 22 fractional bits).  The
    support is stretched by the scale when shrinking; the taps are normalised, then rounded half away from zero."""
    filt, support = {PIL_BILINEAR: (_bilinear_filter, 1.0), PIL_BICUBIC: (_bicubic_filter, 2.0)}[resample]
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [filt((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        for x, v in enumerate(w):
            kk[xx, x] = int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22))
    return bounds, kk


# ---- the packed model ---------------------------------------------------------------------------------------------------------------
class _PatchProjection(nn.Module):
    """Conv2d(3, C, P, stride P) as a GEMM over ca_dpt_patches' rows."""

    def __init__(self, c: int, patch: int):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(c, 3, patch, patch) * (3 * patch * patch) ** -0.5)
        self.bias = nn.Parameter(torch.zeros(c))
        self.w = self.b = None

    def pack(self, arena: WeightArena, dtype):
        c = self.weight.shape[0]
        self.w = arena.add((c, self.weight[0].numel()), dtype, lambda: _f32(self.weight).reshape(c, -1))
        self.b = arena.add((c,), torch.float32, lambda: _f32(self.bias))


class _PatchEmbeddings(nn.Module):
    def __init__(self, c, patch):
        super().__init__()
        self.projection = _PatchProjection(c, patch)


class _Embeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        tokens = (cfg.image_size // cfg.patch_size) ** 2 + 1
        self.cls_token = nn.Parameter(torch.randn(1, 1, cfg.hidden_size) * 0.3)
        self.position_embeddings = nn.Parameter(torch.randn(1, tokens, cfg.hidden_size) * 0.3)
        self.patch_embeddings = _PatchEmbeddings(cfg.hidden_size, cfg.patch_size)


class _SelfAttention(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.query, self.key, self.value = HipLinear(c, c), HipLinear(c, c), HipLinear(c, c)


class _Dense(nn.Module):
    def __init__(self, k, n):
        super().__init__()
        self.dense = HipLinear(k, n)


class _Attention(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.attention = _SelfAttention(c)
        self.output = _Dense(c, c)


class DPTViTLayer(nn.Module):
    """A ViT layer under transformers' DPT names, run as clip.CLIPEncoderLayer runs its own."""

    def __init__(self, cfg):
        super().__init__()
        c = cfg.hidden_size
        self.heads = cfg.num_attention_heads
        self.attention = _Attention(c)
        self.intermediate = _Dense(c, cfg.intermediate_size)
        self.output = _Dense(cfg.intermediate_size, c)
        self.layernorm_before = HipLayerNorm(c, cfg.layer_norm_eps)
        self.layernorm_after = HipLayerNorm(c, cfg.layer_norm_eps)
        self.wqkv = self.bqkv = None

    def pack(self, arena: WeightArena, dtype):
        a = self.attention.attention
        mods = [a.query, a.key, a.value]
        self.wqkv = pack_concat_rows(arena, dtype, mods)
        self.bqkv = pack_concat_bias(arena, mods)
        for m in (self.attention.output.dense, self.intermediate.dense, self.output.dense, self.layernorm_before, self.layernorm_after):
            m.pack(arena, dtype)

    def run(self, x: torch.Tensor, batch: int, tokens: int) -> torch.Tensor:
        from . import kernels as K
        qkv = K.gemm(self.layernorm_before.run(x), self.wqkv.t, bias=self.bqkv.t)
        o = K.attention_spatial(qkv, batch, tokens, self.heads)
        x = self.attention.output.dense.run(o, residual=x)
        h = self.intermediate.dense.run(self.layernorm_after.run(x), act=K.ACT_GELU)
        return self.output.dense.run(h, residual=x)


class _Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layer = nn.ModuleList([DPTViTLayer(cfg) for _ in range(cfg.num_hidden_layers)])


class _DPTModel(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.embeddings = _Embeddings(cfg)
        self.encoder = _Encoder(cfg)
        self.layernorm = HipLayerNorm(cfg.hidden_size, cfg.layer_norm_eps)   # a checkpoint key; DPT's taps never pass through it


class _ConvTransposeK(nn.Module):
    """ConvTranspose2d(C, C, kernel = stride = k) as a GEMM with N = k k C (columns (ky, kx, co)) + ca_depth_to_space."""

    def __init__(self, c: int, k: int):
        super().__init__()
        self.k, self.c = k, c
        self.weight = nn.Parameter(torch.randn(c, c, k, k) * c ** -0.5)
        self.bias = nn.Parameter(torch.zeros(c))
        self.w = self.b = None

    def pack(self, arena: WeightArena, dtype):
        k, c = self.k, self.c
        self.w = arena.add((k * k * c, c), dtype, lambda: _f32(self.weight).permute(2, 3, 1, 0).reshape(k * k * c, c))
        self.b = arena.add((k * k * c,), torch.float32, lambda: _f32(self.bias).repeat(k * k))


class _ReassembleLayer(nn.Module):
    def __init__(self, hidden: int, channels: int, factor):
        super().__init__()
        self.factor = factor
        self.projection = HipConv1x1(hidden, channels)
        if factor > 1:
            self.resize = _ConvTransposeK(channels, int(factor))
        elif factor < 1:
            self.resize = HipConv3x3(channels, channels, stride=2)


class _Readout(HipLinear):
    """Linear(2C, C) over cat(token, cls): the token half is a GEMM weight, the class-token half becomes a per-image row bias."""

    def pack(self, arena: WeightArena, dtype):
        c = self.out_features
        self.w_tok = arena.add((c, c), dtype, lambda: _f32(self.weight)[:, :c])
        self.w_cls = arena.add((c, c), dtype, lambda: _f32(self.weight)[:, c:])
        self.b = arena.add((c,), torch.float32, lambda: _f32(self.bias))


class _ReassembleStage(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layers = nn.ModuleList([_ReassembleLayer(cfg.hidden_size, ch, f) for ch, f in zip(cfg.neck_hidden_sizes, REASSEMBLE_FACTORS)])
        self.readout_projects = nn.ModuleList([nn.Sequential(_Readout(2 * cfg.hidden_size, cfg.hidden_size)) for _ in range(4)])


class _Conv3x3NoBias(nn.Module):
    def __init__(self, cin: int, cout: int):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(cout, cin, 3, 3) * (9 * cin) ** -0.5)
        self.w = None

    def pack(self, arena: WeightArena, dtype):
        co, ci = self.weight.shape[:2]
        self.w = arena.add((co, 3, 3, ci), dtype, lambda: _f32(self.weight).permute(0, 2, 3, 1))


class _ResidualLayer(nn.Module):
    def __init__(self, f: int):
        super().__init__()
        self.convolution1, self.convolution2 = HipConv3x3(f, f), HipConv3x3(f, f)

    def run(self, x: torch.Tensor) -> torch.Tensor:
        from . import kernels as K
        t = self.convolution1.run(K.relu(x), act=K.ACT_RELU)
        return self.convolution2.run(t, residual=x)


class _FusionLayer(nn.Module):
    def __init__(self, f: int):
        super().__init__()
        self.projection = HipConv1x1(f, f)
        self.residual_layer1, self.residual_layer2 = _ResidualLayer(f), _ResidualLayer(f)


class _FusionStage(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layers = nn.ModuleList([_FusionLayer(cfg.fusion_hidden_size) for _ in range(4)])


class _Neck(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.reassemble_stage = _ReassembleStage(cfg)
        self.convs = nn.ModuleList([_Conv3x3NoBias(ch, cfg.fusion_hidden_size) for ch in cfg.neck_hidden_sizes])
        self.fusion_stage = _FusionStage(cfg)


class _LastConv(nn.Module):
    """Conv2d(32, 1, 1): float32 operands of the head's last step."""

    def __init__(self):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(1, 32, 1, 1) * 32 ** -0.5)
        self.bias = nn.Parameter(torch.zeros(1))
        self.w = self.b = None

    def pack(self, arena: WeightArena, dtype):
        self.w = arena.add((32,), torch.float32, lambda: _f32(self.weight).reshape(32))
        self.b = arena.add((1,), torch.float32, lambda: _f32(self.bias))


class _Head(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        f = cfg.fusion_hidden_size
        self.head = nn.ModuleDict({"0": HipConv3x3(f, f // 2), "2": HipConv3x3(f // 2, 32), "4": _LastConv()})


class DPTForDepthEstimation(_PackedModel):
    """transformers' DPTForDepthEstimation (plain ViT) with its checkpoint keys, packed for the HIP kernels; the prepare() / dtype contract of
    clip._PackedModel.  `predicted_depth(frames_u8)` takes the RESIZED uint8 frames [n, S, S, 3] on the device (the normalisation is part of
    the patch kernel) and returns float32 [n, S, S]."""

    def __init__(self, **config):
        super().__init__()
        check_config(config)
        cfg = dict(DPT_CONFIG)
        cfg.update({k: v for k, v in config.items() if k in DPT_CONFIG})
        self.config = SimpleNamespace(**cfg)
        self.dpt = _DPTModel(self.config)
        self.neck = _Neck(self.config)
        self.head = _Head(self.config)
        self._init_exec()
        self.timings = None   # a dict: receives (start, end) torch events per stage under the keys of STAGES -- tools/bench_depth.py
        self.taps = None      # a list: receives the hidden states after the backbone_out_indices layers (tests)
        self.stored = None    # a list: receives every other stored activation of a pass: the planes, the fusion inputs, the fused map, the head's input

    @classmethod
    def from_config(cls, config=None, **kw):
        cfg = dict(config or {})
        cfg.update(kw)
        return cls(**cfg)

    def _pack_extra(self, arena: WeightArena):
        emb = self.dpt.embeddings
        dtype = self.act_dtype
        self.pos = arena.add(tuple(emb.position_embeddings.shape[1:]), torch.float32, lambda: _f32(emb.position_embeddings)[0])
        self.cls = arena.add((1, emb.cls_token.shape[2]), dtype, lambda: _f32(emb.cls_token)[0])

    _stage = HipStages._stage   # (events per stage into `timings`, as the annotators record them)

    # ---- stages -----------------------------------------------------------------------------------------------------------------------
    def _vit(self, frames_u8: torch.Tensor):
        """-> the hidden states [n * tokens, C] after the backbone_out_indices layers."""
        from . import kernels as K
        cfg = self.config
        n = frames_u8.shape[0]
        proj = self.dpt.embeddings.patch_embeddings.projection
        tok = K.gemm(K.dpt_patches(frames_u8, cfg.patch_size, self.act_dtype), proj.w.t, bias=proj.b.t)
        g2 = tok.shape[0] // n
        t = g2 + 1
        # the class token in front and the position table: device-side indexing, as clip's embeddings (plumbing)
        x = (torch.cat([self.cls.t.expand(n, 1, -1), tok.view(n, g2, -1)], 1).float() + self.pos.t).to(self.act_dtype).reshape(n * t, -1).contiguous()
        taps, want = [], set(cfg.backbone_out_indices)
        for i, layer in enumerate(self.dpt.encoder.layer):
            x = layer.run(x, n, t)
            if i in want:
                taps.append(x)
            if len(taps) == len(want):
                break
        return taps, t

    def _reassemble(self, i: int, hidden: torch.Tensor, n: int, t: int) -> torch.Tensor:
        from . import kernels as K
        cfg = self.config
        c, g = cfg.hidden_size, cfg.image_size // cfg.patch_size
        ro = self.neck.reassemble_stage.readout_projects[i][0]
        layer = self.neck.reassemble_stage.layers[i]
        cls_rows = hidden.view(n, t * c)[:, :c]                                       # the n class tokens: a strided view, no copy
        rb = K.gemm(cls_rows, ro.w_cls.t, bias=ro.b.t, out_f32=True)                  # [n, C]: W[:, C:] cls + b
        r = K.gemm(hidden, ro.w_tok.t, rowbias=rb, rows_per_group=t, act=K.ACT_GELU)  # all n * t rows; row 0 of each image is never read again
        p = layer.projection.run(r)
        ch = layer.projection.out_channels
        if layer.factor > 1:
            k = layer.resize.k
            q = K.gemm(p, layer.resize.w.t, bias=layer.resize.b.t)
            return K.depth_to_space(q, n, g, g, k, ch, rows_per_image=t, row0=1)
        y = K.depth_to_space(p, n, g, g, 1, ch, rows_per_image=t, row0=1)
        return y if layer.factor == 1 else layer.resize.run(y)

    def _fusion(self, feats) -> torch.Tensor:
        from . import kernels as K
        fused = None
        for layer, x in zip(self.neck.fusion_stage.layers, feats[::-1]):
            h = x if fused is None else K.add_bcast(layer.residual_layer1.run(x), fused)
            h = layer.residual_layer2.run(h)
            n, hh, ww, f = h.shape
            p = layer.projection.run(h.view(n * hh * ww, f)).view(n, hh, ww, f)       # before the x2: bilinear weights sum to 1
            fused = K.upsample2x_bilinear_ac(p, torch.empty((n, 2 * hh, 2 * ww, f), dtype=p.dtype, device=p.device))
        return fused

    @torch.no_grad()
    def predicted_depth(self, frames_u8: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
        from . import kernels as K
        cfg = self.config
        s = cfg.image_size
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or tuple(frames_u8.shape[1:]) != (s, s, 3):
            raise ValueError(f"expected uint8 [n, {s}, {s}, 3], got {frames_u8.dtype} {tuple(frames_u8.shape)}")
        self._ready(frames_u8.device)
        n = frames_u8.shape[0]
        ev = self._stage("vit")
        taps, t = self._vit(frames_u8.contiguous())
        if ev:
            ev[1].record()
        if self.taps is not None:
            self.taps.extend(x.view(n, t, -1) for x in taps)
        ev = self._stage("reassemble")
        planes = [self._reassemble(i, h, n, t) for i, h in enumerate(taps)]
        if ev:
            ev[1].record()
        ev = self._stage("fusion")
        feats = [K.conv3x3(p, conv.w.t) for p, conv in zip(planes, self.neck.convs)]
        fused = self._fusion(feats)
        if ev:
            ev[1].record()
        ev = self._stage("head")
        hd = self.head.head
        x = hd["0"].run(fused)
        if self.stored is not None:
            self.stored.extend(planes + feats + [fused, x])
        out = K.dpt_head(x, hd["2"].w.t, hd["2"].b.t, hd["4"].w.t, hd["4"].b.t, out=out)
        if ev:
            ev[1].record()
        return out


# ---- the annotator --------------------------------------------------------------------------------------------------------------------
class DepthAnnotator(AnnotatorBase):
    """`DepthAnnotator(model, size, resample, normalize)` for a packed DPTForDepthEstimation with seeded or loaded weights;
    `DepthAnnotator.from_pretrained(local_dir)` for a local Intel/dpt-large style directory.  The surface of the sibling annotators:
    `annotate_batch(frames, out=, rep=, dtype=)` writes the ControlNets' control tensor [rep * n, 3, H, W] in [0, 1]; `depth(frames)` is the
    uint8 map [n, H, W] on the device; `predicted_depth(frames)` float32 [n, S, S]; `__call__(image)` a PIL RGB image with three equal
    channels (an array in, an array out).  Frames: PIL RGB images, uint8 arrays [H, W, 3] of one size, or a uint8 tensor [n, H, W, 3] (no host
    copy when it is on the device).  It plugs into `MultiControlNetResidualsPipeline(annotators={"depth": ann})`, whose key "depth" serves
    every ControlNet name that contains it.  Non-uint8 input raises TypeError, frames of different sizes ValueError, a config or processor
    setting out of scope NotImplementedError -- all before the device is touched; without the library or a GPU a call raises
    CAHipUnavailable (there is no CPU fallback)."""

    chunk_frames = 16   # frames per pass through the network (the tail and the finish run once for all)

    def __init__(self, model: DPTForDepthEstimation, size: int = None, resample: int = PIL_BICUBIC, normalize: str = "max", device=None):
        if not isinstance(model, DPTForDepthEstimation):
            raise TypeError("model must be a controlanimate_amd.depth.DPTForDepthEstimation")
        size = model.config.image_size if size is None else size
        self.resample = check_processor({"size": {"height": size, "width": size}, "resample": resample}, model.config.image_size)
        if normalize not in ("max", "minmax"):
            raise ValueError(f"normalize={normalize!r} ('max' or 'minmax')")
        self.model, self.size, self.normalize, self.device = model, size, normalize, device
        self._tables = {}   # (`timings` receives events under the keys of STAGES -- tools/bench_depth.py)

    @classmethod
    def from_pretrained(cls, local_dir, device=None, dtype=torch.float16, normalize: str = "max"):
        """local_dir: a local directory with config.json, preprocessor_config.json and model.safetensors / pytorch_model.bin (nothing is
        ever downloaded)."""
        from .local_models import load_dir_config, load_dir_state_dict
        local_dir = os.fspath(local_dir)
        if not os.path.isdir(local_dir):
            raise FileNotFoundError(f"{local_dir}: no such directory (a local copy of the model; nothing is ever downloaded)")
        if dtype not in (torch.float16, torch.bfloat16):
            raise TypeError(f"dtype must be torch.float16 or torch.bfloat16, got {dtype}")
        cfg = load_dir_config(local_dir)
        pp_path = os.path.join(local_dir, "preprocessor_config.json")
        if not os.path.isfile(pp_path):
            raise FileNotFoundError(f"{pp_path} does not exist")
        with open(pp_path) as fh:
            pp = json.load(fh)
        check_config(cfg)
        image_size = cfg.get("image_size", DPT_CONFIG["image_size"])
        resample = check_processor(pp, image_size)
        model = DPTForDepthEstimation.from_config(cfg)
        model.load_state_dict(load_dir_state_dict(local_dir), strict=True)
        model.to(dtype)
        return cls(model, image_size, resample, normalize, device=device)

    # ---- input checks ----------------------------------------------------------------------------------------------------------
    def _frames(self, frames) -> torch.Tensor:
        """-> uint8 device tensor [n, H, W, 3].  The type and size checks come before the device is touched.  (Its own intake: three
        channels only, as the pipeline's image processor takes them, with its own messages.)"""
        if isinstance(frames, torch.Tensor):
            if frames.dtype != torch.uint8:
                raise TypeError(f"frames must be uint8, got {frames.dtype}")
            if frames.dim() != 4 or frames.shape[3] != 3:
                raise ValueError(f"frames tensor must be [n, H, W, 3], got {tuple(frames.shape)}")
            return frames.to(self._device()).contiguous()
        host = []
        for fr in frames:
            a = np.asarray(fr)
            if a.dtype != np.uint8:
                raise TypeError(f"frames must be uint8, got {a.dtype}")
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"a frame must be [H, W, 3] (PIL mode RGB: convert other modes with .convert('RGB') first), got {a.shape}"
                                 + (f" from PIL mode {fr.mode}" if hasattr(fr, "mode") else ""))
            host.append(a)
        if not host:
            raise ValueError("no frames")
        if any(a.shape != host[0].shape for a in host):
            raise ValueError("all frames of a call must share one size")
        dev = self._device()
        return torch.from_numpy(np.stack(host)).to(dev)

    def tables(self, h: int, w: int, dev):
        """The resampler's bounds and coefficients for frames of h x w pixels, on the device; cached per size."""
        key = (h, w, str(dev))
        if key not in self._tables:
            xb, xk = pil_coeffs(w, self.size, self.resample)
            yb, yk = pil_coeffs(h, self.size, self.resample)
            self._tables[key] = tuple(torch.from_numpy(a).to(dev) for a in (xb, xk, yb, yk))
        return self._tables[key]

    # ---- the chain -------------------------------------------------------------------------------------------------------------
    def _predict(self, src: torch.Tensor) -> torch.Tensor:
        from . import kernels as K
        n, h, w, _ = src.shape
        s = self.size
        self.model.timings = self.timings
        small = self._timed("resize", K.resize_pil_u8, src, s, s, *self.tables(h, w, src.device))
        depth = torch.empty((n, s, s), dtype=torch.float32, device=src.device)
        for i0 in range(0, n, self.chunk_frames):
            self.model.predicted_depth(small[i0:i0 + self.chunk_frames], out=depth[i0:i0 + self.chunk_frames])
        return depth

    def _run(self, src, map, control, rep):
        from . import kernels as K
        n, h, w, _ = src.shape
        depth = self._predict(src)
        ev = self._stage("tail")
        full, keys = K.resize_bicubic_f32(depth, h, w)
        K.depth_finish(full, keys, self.normalize, map=map, control=control, rep=rep)
        if ev:
            ev[1].record()

    def predicted_depth(self, frames) -> torch.Tensor:
        """-> float32 [n, S, S] on the device: the model's output for the resized frames."""
        return self._predict(self._frames(frames))

    def depth(self, frames, out=None) -> torch.Tensor:
        """-> the uint8 depth map [n, H, W] on the device, written into `out` when given."""
        return self._uint8_out(frames, out)
