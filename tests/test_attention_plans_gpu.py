"""GPU: ca_attention against a plain fp64 restatement (tests/attention_ref.py) on EVERY kernel attn_plan() can reach --
attn_generic, attn_tiny16 / 32, attn_dma, attn_dma_fold, attn_dma40, attn_dma80, attn_short -- with the features each of them
carries its own copy of: the key mask (alone, with causal, hiding whole tiles, hiding everything), accumulate + out_scale,
cross / temporal addressing, row strides wider than the logical width, and the running-maximum rescale.

Every case records the plan label of its launch and asserts it, so a later dispatch change cannot quietly move a case onto
another kernel.  Inputs are rounded to the activation dtype first; tolerances are those of test_kernels_gpu.py's attention tests."""
import contextlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_ref as R  # noqa: E402
from test_kernels_gpu import DEV, DTYPES, close, rnd  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = {torch.bfloat16: 8e-3, torch.float16: 3e-3}
TOL_ACC = {torch.bfloat16: 1e-2, torch.float16: 4e-3}  # accumulating launches (test_attention_cross_and_ip)


def _k():
    from controlanimate_amd import kernels
    return kernels


@contextlib.contextmanager
def planned(*labels):
    """The launches inside run on exactly these kernels."""
    K = _k()
    K._plan_sink = seen = []
    try:
        yield
        torch.cuda.synchronize()
    finally:
        K._plan_sink = None
    assert seen == list(labels), f"planned {labels}, ran {seen}"


def spatial_raw(qkv, images, tokens, heads, d, out, **kw):
    """attention_spatial through attention_raw: qkv / out may be column slices of wider buffers, and accumulate, out_scale,
    causal and key_mask pass through."""
    c = heads * d
    ld, lo = qkv.stride(0), out.stride(0)
    _k().attention_raw(qkv, qkv, qkv, out, q_off=0, k_off=c, v_off=2 * c, o_off=0, q_strides=(tokens * ld, 0, ld),
                       o_strides=(tokens * lo, 0, lo), k_strides=(tokens * ld, 0, ld), inner_count=1, kv_inner_count=1, kv_div=1,
                       batches=images, heads=heads, head_dim=d, nq=tokens, nk=tokens, scale=d ** -0.5, **kw)
    return out


def temporal_raw(qkv, b, frames, tokens, heads, d, out, **kw):
    """attention_temporal through attention_raw (rows in (b f n) order, the sequence runs over f)."""
    c = heads * d
    ld, lo = qkv.stride(0), out.stride(0)
    _k().attention_raw(qkv, qkv, qkv, out, q_off=0, k_off=c, v_off=2 * c, o_off=0, q_strides=(frames * tokens * ld, ld, tokens * ld),
                       o_strides=(frames * tokens * lo, lo, tokens * lo), k_strides=(frames * tokens * ld, ld, tokens * ld),
                       inner_count=tokens, kv_inner_count=tokens, kv_div=1, batches=b * tokens, heads=heads, head_dim=d,
                       nq=frames, nk=frames, scale=d ** -0.5, **kw)
    return out


def spatial_heads(qkv, images, tokens, heads, d):
    """CPU [images * tokens, 3C] -> q, k, v as [images, heads, tokens, d]."""
    return [R.split_heads(t, images, tokens, heads, d) for t in qkv.split(heads * d, dim=1)]


def temporal_heads(x, b, frames, tokens, heads, d):
    """CPU [(b f n), parts * C] -> `parts` tensors [b * tokens, heads, frames, d]."""
    parts = x.shape[1] // (heads * d)
    t = x.reshape(b, frames, tokens, parts, heads, d).permute(3, 0, 2, 4, 1, 5).reshape(parts, b * tokens, heads, frames, d)
    return list(t)


def temporal_rows(x, b, frames, tokens):
    """[b * tokens, heads, frames, d] -> [(b f n), C]."""
    bn, heads, _, d = x.shape
    return x.reshape(b, tokens, heads, frames, d).permute(0, 3, 1, 2, 4).reshape(b * frames * tokens, heads * d)


def cross_heads(q, kv, b, f, tokens, heads, d, rows_per_batch, row_offset, nk, kv_mod=0):
    """CPU q [b f tokens, C], kv [kv batches * rows_per_batch, 2C] -> q, k, v per image, as attention_cross addresses them."""
    c = heads * d
    images = b * f
    kvb = kv.shape[0] // rows_per_batch
    idx = [(z // f) % (kv_mod or images) for z in range(images)]
    kh = kv[:, :c].reshape(kvb, rows_per_batch, heads, d)[:, row_offset:row_offset + nk].transpose(1, 2)[idx]
    vh = kv[:, c:].reshape(kvb, rows_per_batch, heads, d)[:, row_offset:row_offset + nk].transpose(1, 2)[idx]
    return R.split_heads(q, images, tokens, heads, d), kh, vh


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


def cdiv(a, b):
    return -(-a // b)


# ================================================================================================ A. key mask (attn_generic)
def _masked_self(mask, tokens, heads, d, dtype, causal, seed, rel=None, strided_mask=False):
    K = _k()
    images = mask.shape[0]
    qkv = rnd(images * tokens, 3 * heads * d, dtype=dtype, seed=seed)
    ref = R.attention_ref(*spatial_heads(qkv, images, tokens, heads, d), causal=causal, key_mask=mask)
    if strided_mask:  # a [:, :tokens] slice of a wider buffer: key_mask_stride > nk; what lies behind the slice says "hidden"
        buf = torch.zeros(images, 96, dtype=torch.uint8)
        buf[:, :tokens] = mask
        mdev = buf.to(DEV)[:, :tokens]
        assert mdev.stride(0) == 96
    else:
        mdev = mask.to(DEV)
    with planned("attn_generic"):
        out = K.attention_spatial(qkv.to(DEV), images, tokens, heads, causal=causal, key_mask=mdev)
    close(out, R.merge_heads(ref), dtype, f"masked self-attention {images}x{tokens}x{heads}x{d} causal={causal}", rel=rel or TOL[dtype])
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [False, True])
def test_key_mask_clip_shape_77_tokens(causal, dtype):
    """A1 / A2: 2 x 77 tokens, 12 heads of 64 (sum_row = 0, prefetch instantiation): one full 64-key tile through the masked
    branch plus a ragged masked tail, the mask a slice with row stride 96; A2 adds causal -- the CLIP product launch."""
    _masked_self(R.mask_clip77(), 77, 12, 64, dtype, causal, seed=101, strided_mask=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,d", [(2, 40), (1, 160)])
def test_key_mask_hides_a_whole_tile(heads, d, dtype):
    """A3 / A4: 3 x 200 tokens; image 0 hides the whole FIRST 64-key tile (the reference maximum has seen nothing when tile 1
    arrives), image 1 a whole middle tile, image 2 the whole ragged tail.  d = 40: row sums come from the ones row (sum_row = 1);
    d = 160: DK32 = 5, the instantiation without register prefetch."""
    _masked_self(R.mask_whole_tiles200(), 200, heads, d, dtype, False, seed=103)


@pytest.mark.parametrize("dtype", DTYPES)
def test_key_mask_routes_text_cross_attention_to_generic(dtype):
    """A5: 6 images (b = 2, f = 3) x 300 queries, 70 keys, 8 heads of 40 is attn_short's shape -- but that kernel knows no mask."""
    K = _k()
    b, f, tokens, heads, d, nk = 2, 3, 300, 8, 40, 70
    c = heads * d
    mask = R.mask_cross70(b * f)
    q = rnd(b * f * tokens, c, dtype=dtype, seed=105)
    kv = rnd(b * nk, 2 * c, dtype=dtype, seed=106)
    ref = R.attention_ref(*cross_heads(q, kv, b, f, tokens, heads, d, nk, 0, nk), key_mask=mask)
    with planned("attn_generic"):
        out = K.attention_cross(q.to(DEV), kv.to(DEV), b * f, tokens, heads, nk, nk, f, key_mask=mask.to(DEV))
    close(out, R.merge_heads(ref), dtype, "masked cross-attention", rel=TOL[dtype])
    with planned("attn_short"):  # (the same launch without the mask: the shape is the short kernel's)
        K.attention_cross(q.to(DEV), kv.to(DEV), b * f, tokens, heads, nk, nk, f)


@pytest.mark.parametrize("dtype", DTYPES)
def test_key_mask_of_ones_changes_nothing(dtype):
    """A6: an all-visible mask takes the masked branch of the same kernel and must give the same bits."""
    K = _k()
    images, tokens, heads, d = 2, 100, 2, 80
    qkv = rnd(images * tokens, 3 * heads * d, dtype=dtype, seed=107).to(DEV)
    with planned("attn_generic", "attn_generic"):
        plain = K.attention_spatial(qkv, images, tokens, heads)
        masked = K.attention_spatial(qkv, images, tokens, heads, key_mask=torch.ones(images, tokens, dtype=torch.uint8, device=DEV))
    assert torch.equal(bits(plain), bits(masked))
    ref = R.attention_ref(*spatial_heads(qkv.cpu(), images, tokens, heads, d))
    close(masked, R.merge_heads(ref), dtype, "all-ones mask", rel=TOL[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tokens,d", [(77, 64), (200, 64), (77, 40), (200, 40)])
def test_query_with_every_key_hidden_gets_zeros(tokens, d, dtype):
    """A7: image 0 sees no key at all: its rows are exactly zero (the header's promise), image 1's rows are right."""
    out = _masked_self(R.mask_first_image_hidden(tokens), tokens, 2, d, dtype, False, seed=109)
    assert torch.isfinite(out.float()).all()
    assert (out[:tokens].float() == 0).all(), "rows without a visible key are not zero"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tokens,d", [(77, 64), (200, 40)])
def test_causal_query_0_with_key_0_hidden_gets_zeros(tokens, d, dtype):
    """A7: causal, image 0 hides key 0 -- query 0, and only that one, has nothing visible; it shares its wave with rows that do."""
    out = _masked_self(R.mask_key0_hidden(tokens), tokens, 2, d, dtype, True, seed=111)
    assert (out[0].float() == 0).all(), "query 0 has no visible key and is not zero"
    assert (out[1:].float().abs().sum(1) > 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_accumulate_leaves_rows_with_every_key_hidden_alone(dtype):
    """A8: accumulate + out_scale = 0.4 with image 0 all hidden: those rows keep their previous contents bit for bit."""
    images, tokens, heads, d = 2, 77, 2, 64
    mask = R.mask_first_image_hidden(tokens)
    qkv = rnd(images * tokens, 3 * heads * d, dtype=dtype, seed=113)
    old = rnd(images * tokens, heads * d, dtype=dtype, scale=0.1, seed=114)
    old[5, 3] = -0.0  # (a rewrite as old + 0 would turn this into +0)
    ref = R.attention_ref(*spatial_heads(qkv, images, tokens, heads, d), key_mask=mask, out_scale=0.4,
                          old=R.split_heads(old, images, tokens, heads, d))
    out = old.to(DEV)
    with planned("attn_generic"):
        spatial_raw(qkv.to(DEV), images, tokens, heads, d, out, key_mask=mask.to(DEV), accumulate=True, out_scale=0.4)
    assert torch.equal(bits(out[:tokens]), bits(old[:tokens])), "accumulate touched rows that have no visible key"
    close(out, R.merge_heads(ref), dtype, "masked accumulate", rel=TOL_ACC[dtype])


# ================================================================================================ B. plans without a parity test
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tokens,d,plan", [(300, 16, "attn_dma_fold"), (300, 24, "attn_dma_fold"), (300, 56, "attn_dma_fold"),
                                           (300, 8, "attn_dma"), (300, 32, "attn_dma"), (300, 48, "attn_dma"),
                                           # exactly four KV tiles, no ragged one
                                           (256, 24, "attn_dma_fold"), (256, 48, "attn_dma")])
def test_self_attention_on_the_dma_plans(tokens, d, plan, dtype):
    """2 images x 300 tokens x 2 heads: q-blocks of 128 + 128 + 44, four full KV tiles and a ragged one."""
    K = _k()
    images, heads = 2, 2
    qkv = rnd(images * tokens, 3 * heads * d, dtype=dtype, seed=120 + d)
    ref = R.attention_ref(*spatial_heads(qkv, images, tokens, heads, d))
    with planned(plan):
        out = K.attention_spatial(qkv.to(DEV), images, tokens, heads)
    close(out, R.merge_heads(ref), dtype, f"{plan} d={d} tokens={tokens}", rel=TOL[dtype])


# ================================================================================================ C. features per kernel
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,d,plan", [(8, 40, "attn_dma40"), (8, 80, "attn_dma80"), (2, 24, "attn_dma_fold"), (2, 64, "attn_dma")])
def test_accumulate_and_out_scale_on_the_dma_kernels(heads, d, plan, dtype):
    """C1: out = old + 0.4 * attention into a pre-filled output (k_attn_dma's own epilogue), 1 x 300 tokens."""
    images, tokens = 1, 300
    qkv = rnd(images * tokens, 3 * heads * d, dtype=dtype, seed=130 + d)
    old = rnd(images * tokens, heads * d, dtype=dtype, scale=0.1, seed=131)
    ref = R.attention_ref(*spatial_heads(qkv, images, tokens, heads, d), out_scale=0.4, old=R.split_heads(old, images, tokens, heads, d))
    out = old.to(DEV)
    with planned(plan):
        spatial_raw(qkv.to(DEV), images, tokens, heads, d, out, accumulate=True, out_scale=0.4)
    close(out, R.merge_heads(ref), dtype, f"accumulate on {plan}", rel=TOL_ACC[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("frames,d,plan", [(16, 80, "attn_tiny16"), (32, 160, "attn_tiny32")])
def test_accumulate_and_out_scale_on_the_tiny_kernels(frames, d, plan, dtype):
    """C1: the one-wave instantiations of k_attn, temporal layout: b = 1, 5 tokens, 8 heads."""
    b, tokens, heads = 1, 5, 8
    qkv = rnd(b * frames * tokens, 3 * heads * d, dtype=dtype, seed=140 + d)
    old = rnd(b * frames * tokens, heads * d, dtype=dtype, scale=0.1, seed=141)
    ref = R.attention_ref(*temporal_heads(qkv, b, frames, tokens, heads, d), out_scale=0.4,
                          old=temporal_heads(old, b, frames, tokens, heads, d)[0])
    out = old.to(DEV)
    with planned(plan):
        temporal_raw(qkv.to(DEV), b, frames, tokens, heads, d, out, accumulate=True, out_scale=0.4)
    close(out, temporal_rows(ref, b, frames, tokens), dtype, f"accumulate on {plan}", rel=TOL_ACC[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("qc", [16, 8])
@pytest.mark.parametrize("tokens,d,rows,strip", [(256, 40, 77, 0), (272, 80, 81, 4)])
def test_short_kernel_out_scale_in_both_chunk_sizes(tokens, d, rows, strip, qc, dtype):
    """C2: k_attn_short with out_scale = 0.5.  The launcher gives a block QC = 16 query tiles per item when
    images * ceil(ceil(tokens / 16) / 16) reaches the CU count, else 8; the plan label is "attn_short" for both, so the image count
    is chosen by that arithmetic.  On a 256-CU MI355X: qc = 16 -> 256 images x 256 tokens (one chunk each) and 128 images x 272
    tokens (17 query tiles: a full chunk and one that holds a single tile); qc = 8 -> 4 images of either.
    272 tokens / 81 rows: K / V are the first 77 rows of an 81-row buffer (the image-prompt strip follows them)."""
    K = _k()
    heads, f = 8, 4
    c = heads * d
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    chunks16 = cdiv(cdiv(tokens, 16), 16)
    b = cdiv(cus, chunks16 * f) if qc == 16 else 1
    images = b * f
    assert (images * chunks16 >= cus) == (qc == 16), (images, chunks16, cus)
    nk = rows - strip
    q = rnd(images * tokens, c, dtype=dtype, seed=150)
    kv = rnd(b * rows, 2 * c, dtype=dtype, seed=151)
    ref = R.attention_ref(*cross_heads(q, kv, b, f, tokens, heads, d, rows, 0, nk), out_scale=0.5)
    with planned("attn_short"):
        out = K.attention_cross(q.to(DEV), kv.to(DEV), images, tokens, heads, nk, rows, f, out_scale=0.5)
    close(out, R.merge_heads(ref), dtype, f"attn_short qc={qc} d={d}", rel=TOL[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b,kv_mod,d,plan", [(2, 0, 40, "attn_dma40"), (2, 0, 80, "attn_dma80"), (4, 2, 40, "attn_dma40")])
def test_cross_layout_on_the_dma_kernels(b, kv_mod, d, plan, dtype):
    """C3: K / V of an image are rows 4 .. 263 of its batch element's 300 in a [kv batches * 300, 2C] buffer (k_row != q_row,
    kv_div = 3, nq = 200 != nk = 260).  Last case: 12 images over TWO K / V batches -- the batch index wraps (kv_mod = 2)."""
    K = _k()
    f, tokens, heads, rows, off, nk = 3, 200, 2, 300, 4, 260
    c = heads * d
    q = rnd(b * f * tokens, c, dtype=dtype, seed=160 + d)
    kv = rnd((kv_mod or b) * rows, 2 * c, dtype=dtype, seed=161)
    ref = R.attention_ref(*cross_heads(q, kv, b, f, tokens, heads, d, rows, off, nk, kv_mod))
    with planned(plan):
        out = K.attention_cross(q.to(DEV), kv.to(DEV), b * f, tokens, heads, nk, rows, f, kv_row_offset=off, kv_mod=kv_mod)
    close(out, R.merge_heads(ref), dtype, f"cross layout on {plan}", rel=TOL[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
def test_temporal_layout_on_a_dma_kernel(dtype):
    """C4: 260 frames of 3 tokens: inner_count = 3, the rows of a sequence are 3 apart."""
    K = _k()
    b, frames, tokens, heads, d = 1, 260, 3, 2, 40
    qkv = rnd(b * frames * tokens, 3 * heads * d, dtype=dtype, seed=170)
    ref = R.attention_ref(*temporal_heads(qkv, b, frames, tokens, heads, d))
    with planned("attn_dma40"):
        out = K.attention_temporal(qkv.to(DEV), b, frames, tokens, heads)
    close(out, temporal_rows(ref, b, frames, tokens), dtype, "temporal on attn_dma40", rel=TOL[dtype])


def _widened(x, left, extra, fill):
    """x as the column slice [:, left : left + width] of a buffer `extra` columns wider, the rest filled with `fill`."""
    wide = torch.full((x.shape[0], x.shape[1] + extra), fill, dtype=x.dtype)
    wide[:, left:left + x.shape[1]] = x
    return wide.to(DEV), left, x.shape[1]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("images,tokens,heads,d,plan", [(2, 100, 2, 80, "attn_generic"), (1, 300, 2, 40, "attn_dma40"),
                                                        (1, 300, 2, 80, "attn_dma80"), (3, 13, 2, 40, "attn_tiny16")])
def test_strided_views_self_attention(images, tokens, heads, d, plan, dtype):
    """C5: q | k | v are columns 64 .. 64 + 3C of a buffer 128 columns wider (NaN around them: nothing outside the logical width
    may reach the result) and the output goes into columns 32 .. 32 + C of a zero-filled wider buffer, which stays zero elsewhere."""
    c = heads * d
    qkv = rnd(images * tokens, 3 * c, dtype=dtype, seed=180 + d)
    ref = R.attention_ref(*spatial_heads(qkv, images, tokens, heads, d))
    wide, left, w = _widened(qkv, 64, 128, float("nan"))
    owide = torch.zeros(images * tokens, c + 64, dtype=dtype, device=DEV)
    with planned(plan):
        spatial_raw(wide[:, left:left + w], images, tokens, heads, d, owide[:, 32:32 + c])
    assert (bits(owide[:, :32]) == 0).all() and (bits(owide[:, 32 + c:]) == 0).all(), "wrote outside the output slice"
    close(owide[:, 32:32 + c], R.merge_heads(ref), dtype, f"strided views on {plan}", rel=TOL[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_views_short_kernel(dtype):
    """C5: k_attn_short computes its buffer-resource bounds from the row strides: q and the output are both column slices."""
    K = _k()
    b, f, tokens, heads, d, nk = 2, 2, 272, 8, 40, 77
    c = heads * d
    q = rnd(b * f * tokens, c, dtype=dtype, seed=190)
    kv = rnd(b * nk, 2 * c, dtype=dtype, seed=191)
    ref = R.attention_ref(*cross_heads(q, kv, b, f, tokens, heads, d, nk, 0, nk))
    wide, left, w = _widened(q, 64, 128, float("nan"))
    owide = torch.zeros(b * f * tokens, c + 64, dtype=dtype, device=DEV)
    with planned("attn_short"):
        K.attention_cross(wide[:, left:left + w], kv.to(DEV), b * f, tokens, heads, nk, nk, f, out=owide[:, 32:32 + c])
    assert (bits(owide[:, :32]) == 0).all() and (bits(owide[:, 32 + c:]) == 0).all(), "wrote outside the output slice"
    close(owide[:, 32:32 + c], R.merge_heads(ref), dtype, "strided views on attn_short", rel=TOL[dtype])


# ================================================================================================ D. running-maximum rescale
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("late", [True, False])
@pytest.mark.parametrize("tokens,d,plan", [(200, 160, "attn_generic"), (300, 40, "attn_dma40"), (300, 80, "attn_dma80"),
                                           (300, 56, "attn_dma_fold")])
def test_spiked_key_moves_the_running_maximum(tokens, d, plan, late, dtype):
    """The construction of test_attention_online_softmax_rescale on the kernels that keep the reference maximum differently:
    the FOLD kernels carry a QUANTISED maximum inside the Q fragment, attn_dma80 has its own loop.
    late: key 195 (KV tile 3) is 6 x query 3 and key 70 (tile 1) is 4 x query 9 -- the reference moves late and O is rescaled.
    not late (the mirror): the same spikes sit in tile 0 (keys 5, 20), every later score of those queries is far below the
    reference -- the side of the deferred maximum where p underflows instead of reaching 256."""
    K = _k()
    images, heads = 1, 2
    c = heads * d
    qkv = rnd(images * tokens, 3 * c, dtype=dtype, seed=42).float()
    hi, lo = (195, 70) if late else (5, 20)
    qkv[hi, c:2 * c] = qkv[3, 0:c] * 6.0
    qkv[lo, c:2 * c] = qkv[9, 0:c] * 4.0
    qkv = qkv.to(dtype)
    ref = R.attention_ref(*spatial_heads(qkv, images, tokens, heads, d))
    with planned(plan):
        out = K.attention_spatial(qkv.to(DEV), images, tokens, heads)
    close(out, R.merge_heads(ref), dtype, f"spike late={late} on {plan}", rel=TOL[dtype])
