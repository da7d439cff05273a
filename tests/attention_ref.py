"""Plain fp64 CPU restatement of ca_attention, and the key-mask patterns the attention tests share
(tests/test_attention_plans_gpu.py runs them on the kernels, tests/test_attention_ref_cpu.py checks this file against torch).

    out = old + out_scale * softmax(scale * q k^T  [hidden keys -> -inf]) v

A key is hidden by the key mask (0 = invisible, per batch element) or, with causal, when j > i.  A query with no visible key
contributes zeros (include/controlanimate_hip.h: "A query whose keys are ALL masked gets zeros"), so an accumulating call leaves
`old` there."""
from __future__ import annotations

import torch


def split_heads(x: torch.Tensor, batch: int, n: int, heads: int, d: int) -> torch.Tensor:
    """[batch * n, heads * d] rows -> [batch, heads, n, d]."""
    return x.reshape(batch, n, heads, d).transpose(1, 2)


def merge_heads(x: torch.Tensor) -> torch.Tensor:
    """[batch, heads, n, d] -> [batch * n, heads * d] rows."""
    b, h, n, d = x.shape
    return x.transpose(1, 2).reshape(b * n, h * d)


def visible(nq: int, nk: int, key_mask=None, causal: bool = False, batch: int = 1) -> torch.Tensor:
    """bool [batch, nq, nk]: True where query i may look at key j."""
    vis = torch.ones(batch, nq, nk, dtype=torch.bool)
    if key_mask is not None:
        assert tuple(key_mask.shape) == (batch, nk)
        vis &= key_mask.bool()[:, None, :]
    if causal:
        assert nq == nk
        vis &= torch.ones(nq, nk, dtype=torch.bool).tril()[None]
    return vis


def attention_ref(q, k, v, *, scale=None, causal=False, key_mask=None, out_scale=1.0, old=None):
    """q [B, H, nq, d], k / v [B, H, nk, d] (any float dtype, taken as they are), key_mask [B, nk] (0 = hidden),
    old [B, H, nq, d] or None  ->  fp64 [B, H, nq, d]."""
    b, h, nq, d = q.shape
    nk = k.shape[2]
    scale = d ** -0.5 if scale is None else scale
    vis = visible(nq, nk, key_mask, causal, b)
    out = torch.zeros(b, h, nq, d, dtype=torch.float64)
    for z in range(b):  # (per batch element: the score matrix of a big launch stays small)
        s = (q[z].double() @ k[z].double().transpose(-1, -2)) * scale
        s = s.masked_fill(~vis[z][None], float("-inf"))
        m = s.amax(-1, keepdim=True)
        m = torch.where(torch.isinf(m), torch.zeros_like(m), m)  # nothing visible: exp(-inf - 0) = 0 everywhere
        p = torch.exp(s - m)
        l = p.sum(-1, keepdim=True)
        out[z] = torch.where(l > 0, (p @ v[z].double()) / l.clamp_min(1e-300), torch.zeros_like(l))
    out = out * out_scale
    if old is not None:
        out = out + old.double()
    return out


# ------------------------------------------------------------------------------------------------ key-mask patterns
# uint8 [batch, nk], 1 = visible.  They differ per batch element, so a kernel that indexed the mask with the wrong batch stride
# or batch index reads another element's pattern.

def _mask(batch: int, nk: int, hidden) -> torch.Tensor:
    m = torch.ones(batch, nk, dtype=torch.uint8)
    for z, keys in enumerate(hidden):
        m[z, list(keys)] = 0
    return m


def mask_clip77() -> torch.Tensor:
    """2 x 77 (the CLIP product length): holes inside the full 64-key tile and a run in the ragged tail.
     Key 0 stays visible in both, so the pattern also leaves every causal row something to look at."""
    return _mask(2, 77, [[3, 4, 5, 40, *range(64, 71)], [1, 2, 41, *range(70, 77)]])


def mask_whole_tiles200() -> torch.Tensor:
    """3 x 200: each image hides one WHOLE 64-key tile -- the first, a middle one, the ragged tail (192..199)."""
    return _mask(3, 200, [range(0, 64), range(64, 128), range(192, 200)])


def mask_cross70(images: int = 6) -> torch.Tensor:
    """images x 70 (a text cross-attention length): about a third of the keys hidden at random, image 2 also its whole
    ragged tail (64..69), image 3 its whole first tile."""
    g = torch.Generator().manual_seed(70)
    m = (torch.rand(images, 70, generator=g) > 0.33).to(torch.uint8)
    m[:, 7] = 1  # every image keeps a key
    m[2, 64:] = 0
    m[3, :64] = 0
    m[3, 66] = 1
    return m


def mask_first_image_hidden(nk: int) -> torch.Tensor:
    """2 x nk: image 0 sees NO key at all; image 1 has a few holes."""
    return _mask(2, nk, [range(nk), [0, 5, nk // 2, nk - 1]])


def mask_key0_hidden(nk: int) -> torch.Tensor:
    """2 x nk, for causal launches: image 0 hides key 0, so its query 0 -- and only that one -- has nothing visible."""
    return _mask(2, nk, [[0], [3, nk - 2]])
