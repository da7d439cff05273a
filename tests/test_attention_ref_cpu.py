"""CPU: the fp64 attention restatement the kernel parity tests trust (tests/attention_ref.py, used by
tests/test_attention_plans_gpu.py) against torch's scaled_dot_product_attention in fp64, on the key-mask patterns those tests use."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_ref as R  # noqa: E402

# name -> (mask, nq): CLIP's 77 tokens, whole 64-key tiles hidden at 200 tokens, text cross-attention (300 queries, 70 keys)
PATTERNS = {
    "clip77": (R.mask_clip77, 77),
    "whole_tiles200": (R.mask_whole_tiles200, 200),
    "cross70": (R.mask_cross70, 300),
}


def _qkv(batch, nq, nk, heads=2, d=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(batch, heads, nq, d, generator=g, dtype=torch.float64),
            torch.randn(batch, heads, nk, d, generator=g, dtype=torch.float64),
            torch.randn(batch, heads, nk, d, generator=g, dtype=torch.float64))


# (cross70 has nq != nk: ca_attention rejects a causal launch of it)
@pytest.mark.parametrize("name,causal", [("clip77", False), ("clip77", True), ("whole_tiles200", False), ("whole_tiles200", True),
                                         ("cross70", False)])
def test_reference_agrees_with_torch_sdpa(name, causal):
    make, nq = PATTERNS[name]
    mask = make()
    batch, nk = mask.shape
    q, k, v = _qkv(batch, nq, nk, seed=nk)
    vis = R.visible(nq, nk, mask, causal, batch)
    ref = F.scaled_dot_product_attention(q, k, v, attn_mask=vis[:, None])
    out = R.attention_ref(q, k, v, causal=causal, key_mask=mask)
    rows = vis.any(-1)  # [batch, nq]: torch gives NaN where a query sees nothing
    if causal and name == "whole_tiles200":  # (causal + a hidden first tile: rows that see nothing exist)
        assert not rows.all()
    sel = rows[:, None, :, None].expand_as(out)
    assert torch.isfinite(ref[sel]).all()
    assert (out[sel] - ref[sel]).abs().max().item() < 1e-12
    assert (out[~sel] == 0).all()


def test_reference_without_mask_and_with_scale():
    q, k, v = _qkv(2, 50, 70, seed=3)
    ref = F.scaled_dot_product_attention(q, k, v, scale=0.3)
    assert (R.attention_ref(q, k, v, scale=0.3) - ref).abs().max().item() < 1e-12
    q, k, v = _qkv(2, 70, 70, seed=4)
    ref = F.scaled_dot_product_attention(q, k, v, is_causal=True)
    assert (R.attention_ref(q, k, v, causal=True) - ref).abs().max().item() < 1e-12


def test_all_hidden_rows_are_zero_where_torch_gives_nan():
    for nk in (77, 200):
        mask = R.mask_first_image_hidden(nk)
        q, k, v = _qkv(2, nk, nk, seed=5)
        out = R.attention_ref(q, k, v, key_mask=mask)
        # the textbook formula (what scaled_dot_product_attention computed before torch special-cased such rows): 0 / 0
        vis = R.visible(nk, nk, mask, False, 2)[:, None]
        tor = torch.softmax((q @ k.transpose(-1, -2) * 8 ** -0.5).masked_fill(~vis, float("-inf")), -1) @ v
        assert torch.isnan(tor[0]).all() and torch.isfinite(tor[1]).all()
        assert (tor[1] - F.scaled_dot_product_attention(q, k, v, attn_mask=vis)[1]).abs().max().item() < 1e-12
        assert (out[0] == 0).all() and torch.isfinite(out).all()
        assert (out[1] - tor[1]).abs().max().item() < 1e-12
        # accumulating: the softmax term of a hidden row is zero, the previous contents stay
        old = torch.randn(out.shape, dtype=torch.float64)
        acc = R.attention_ref(q, k, v, key_mask=mask, out_scale=0.4, old=old)
        assert torch.equal(acc[0], old[0])
        assert (acc[1] - (old[1] + 0.4 * tor[1])).abs().max().item() < 1e-12
    mask = R.mask_key0_hidden(77)
    q, k, v = _qkv(2, 77, 77, seed=6)
    out = R.attention_ref(q, k, v, key_mask=mask, causal=True)
    assert (out[0, :, 0] == 0).all() and (out[0, :, 1:].abs().sum(-1) > 0).all() and (out[1].abs().sum(-1) > 0).all()


def test_layout_helpers_round_trip():
    x = torch.arange(3 * 5 * 2 * 4, dtype=torch.float64).reshape(15, 8)
    h = R.split_heads(x, 3, 5, 2, 4)
    assert h.shape == (3, 2, 5, 4) and h[1, 1, 2, 3] == x[1 * 5 + 2, 1 * 4 + 3]
    assert torch.equal(R.merge_heads(h), x)


def test_kernel_case_masks_leave_every_row_a_visible_key():
    """The patterns meant for cases that compare EVERY row with the reference: no row may be all hidden, or such a case would
    quietly turn into the all-hidden one."""
    assert R.visible(77, 77, R.mask_clip77(), False, 2).any(-1).all()
    assert R.visible(77, 77, R.mask_clip77(), True, 2).any(-1).all()           # (causal: key 0 is visible in both images)
    assert R.visible(200, 200, R.mask_whole_tiles200(), False, 3).any(-1).all()
    assert R.visible(300, 70, R.mask_cross70(), False, 6).any(-1).all()
    m = R.mask_clip77()
    assert not torch.equal(m[0], m[1]) and m.dtype == torch.uint8
    # and the patterns reach what they are meant to: whole tiles of 64 keys hidden, the ragged tail hidden
    t = R.mask_whole_tiles200()
    assert t[0, :64].sum() == 0 and t[1, 64:128].sum() == 0 and t[2, 192:].sum() == 0 and t.sum() == 600 - 64 - 64 - 8
    c = R.mask_cross70()
    assert c[2, 64:].sum() == 0 and c[3, :64].sum() == 0 and 0 < (c == 0).sum() < c.numel() // 2
