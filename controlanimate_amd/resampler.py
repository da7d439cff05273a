"""The perceiver Resampler of IP-Adapter Plus on the HIP layers: num_queries learned latents attend, layer after layer, to the
projected CLIP hidden states and to themselves, and leave as the image-prompt tokens.

Follows the reference's modules/resampler.py (Resampler :81-147, PerceiverAttention :34-78, FeedForward :13-20); the state-dict keys
and shapes are that module's, so the `image_proj` section of ip-adapter-plus_sd15.bin loads strictly:
  latents [1, nq, dim], proj_in, proj_out, norm_out,
  layers.{i}.0.{norm1, norm2}.{weight, bias}, layers.{i}.0.{to_q, to_kv, to_out}.weight,
  layers.{i}.1.0.{weight, bias} (LayerNorm), layers.{i}.1.{1, 3}.weight (Linear; .2 is the GELU)

Execution (one path):
  xp = proj_in(x); one row_stats(xp) -- xp never changes, so the statistics of every layer's norm1(xp) are the same -- and ONE
  LayerNorm-folded GEMM gives the image-side K|V of ALL layers [B n1, depth 2 inner] (norm1_l folded into the rows of to_kv_l);
  per layer: row_stats(latents), one folded GEMM norm2 -> q | k | v of the latents, ca_perceiver_attn (one fp32 softmax over the
  image rows -- a column slice of the big buffer -- and the latent rows together), to_out (+ residual), row_stats, FF1 (LayerNorm
  folded, erf GELU in the epilogue), FF2 (+ residual); then proj_out and norm_out.
The reference scales q and k by dim_head ** -0.25 each; the kernel applies dim_head ** -0.5 once, in fp32, to the logits.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from . import kernels as K
from .layers import HipLayerNorm, HipLinear, LnFold, WeightArena, _f32


class PerceiverAttention(nn.Module):
    def __init__(self, dim: int, dim_head: int, heads: int):
        super().__init__()
        self.heads, self.inner = heads, dim_head * heads
        self.norm1 = HipLayerNorm(dim)
        self.norm2 = HipLayerNorm(dim)
        self.to_q = HipLinear(dim, self.inner, bias=False)
        self.to_kv = HipLinear(dim, 2 * self.inner, bias=False)
        self.to_out = HipLinear(self.inner, dim, bias=False)
        self.fold: Optional[LnFold] = None

    def pack(self, arena: WeightArena, dtype):
        self.fold = LnFold(arena, dtype, self.norm2, [self.to_q, self.to_kv])  # latent side: q | k | v
        self.to_out.pack(arena, dtype)


def _feed_forward(dim: int, mult) -> nn.ModuleList:
    inner = int(dim * mult)
    return nn.ModuleList([HipLayerNorm(dim), HipLinear(dim, inner, bias=False), nn.Identity(), HipLinear(inner, dim, bias=False)])


class _ImageKV:
    """norm1_l -> to_kv_l of every layer l as ONE folded weight [depth 2 inner, dim] (the algebra of layers.LnFold, one LayerNorm per
    row block): W' = cat_l(W_l diag(gamma_l)), colsum of the ROUNDED W', bias' = cat_l(W_l beta_l)."""

    def __init__(self, arena: WeightArena, dtype, attns):
        n = sum(a.to_kv.weight.shape[0] for a in attns)
        k = attns[0].to_kv.weight.shape[1]
        self.eps = attns[0].norm1.eps

        def w_fold():
            return torch.cat([_f32(a.to_kv.weight) * _f32(a.norm1.weight)[None, :] for a in attns], 0)

        self.w = arena.add((n, k), dtype, w_fold)
        self.cs = arena.add((n,), torch.float32, lambda: w_fold().to(dtype).float().sum(1))
        self.b = arena.add((n,), torch.float32, lambda: torch.cat([_f32(a.to_kv.weight) @ _f32(a.norm1.bias) for a in attns], 0))


class Resampler(nn.Module):
    def __init__(self, dim=1024, depth=8, dim_head=64, heads=16, num_queries=8, embedding_dim=768, output_dim=1024, ff_mult=4,
                 max_seq_len: int = 257, apply_pos_emb: bool = False, num_latents_mean_pooled: int = 0):
        super().__init__()
        if apply_pos_emb:
            raise NotImplementedError("Resampler(apply_pos_emb=True): IPAdapterPlus does not use it and it is not implemented")
        if num_latents_mean_pooled > 0:
            raise NotImplementedError("Resampler(num_latents_mean_pooled > 0): IPAdapterPlus does not use it and it is not implemented")
        self.dim, self.depth, self.heads, self.inner = dim, depth, heads, dim_head * heads
        self.num_queries, self.embedding_dim, self.output_dim = num_queries, embedding_dim, output_dim
        self.latents = nn.Parameter(torch.randn(1, num_queries, dim) / dim ** 0.5)
        self.proj_in = HipLinear(embedding_dim, dim)
        self.proj_out = HipLinear(dim, output_dim)
        self.norm_out = HipLayerNorm(output_dim)
        self.layers = nn.ModuleList([nn.ModuleList([PerceiverAttention(dim, dim_head, heads), _feed_forward(dim, ff_mult)])
                                     for _ in range(depth)])
        self.arena: Optional[WeightArena] = None
        self.act_dtype = torch.float16

    def prepare(self, device, dtype=None):
        if dtype is not None:
            self.act_dtype = dtype
        arena = WeightArena()
        dt = self.act_dtype
        self.proj_in.pack(arena, dt)
        self.kv_image = _ImageKV(arena, dt, [attn for attn, _ in self.layers])
        self.ff_folds = []
        for attn, ff in self.layers:
            attn.pack(arena, dt)
            self.ff_folds.append(LnFold(arena, dt, ff[0], [ff[1]]))
            ff[3].pack(arena, dt)
        self.proj_out.pack(arena, dt)
        self.norm_out.pack(arena, dt)
        self.lat = arena.add((self.num_queries, self.dim), dt, lambda: _f32(self.latents)[0])
        arena.finalize(device)
        self.arena = arena
        return self

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [B, n1, embedding_dim] (CLIP hidden states) -> [B, num_queries, output_dim]."""
        if x.dim() != 3 or x.shape[2] != self.embedding_dim:
            raise ValueError(f"expected [B, tokens, {self.embedding_dim}], got {tuple(x.shape)}")
        if self.arena is None or self.arena.buffer.device != x.device:
            self.prepare(x.device)
        b, n1, _ = x.shape
        nq, inner = self.num_queries, self.inner
        xp = self.proj_in.run(x.to(self.act_dtype).reshape(b * n1, -1).contiguous())
        kvi = self.kv_image
        kv_x = K.gemm(xp, kvi.w.t, bias=kvi.b.t, ln=(K.row_stats(xp, kvi.eps), kvi.cs.t)).view(b, n1, self.depth * 2 * inner)
        lat = K.repeat_batch(self.lat.t, b)  # [b * nq, dim]
        for i, (attn, ff) in enumerate(self.layers):
            f = attn.fold
            qkv = K.gemm(lat, f.w.t, bias=f.b.t, ln=(K.row_stats(lat, f.eps), f.cs.t)).view(b, nq, 3 * inner)
            c0 = i * 2 * inner
            o = K.perceiver_attn(qkv[:, :, :inner], kv_x[:, :, c0:c0 + inner], kv_x[:, :, c0 + inner:c0 + 2 * inner],
                                 qkv[:, :, inner:2 * inner], qkv[:, :, 2 * inner:], attn.heads)
            lat = attn.to_out.run(o.view(b * nq, inner), residual=lat)
            f = self.ff_folds[i]
            h = K.gemm(lat, f.w.t, bias=f.b.t, ln=(K.row_stats(lat, f.eps), f.cs.t), act=K.ACT_GELU)
            lat = ff[3].run(h, residual=lat)
        return self.norm_out.run(self.proj_out.run(lat)).view(b, nq, self.output_dim)
