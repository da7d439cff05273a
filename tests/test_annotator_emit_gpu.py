"""GPU: the control-tensor contract of csrc/ca_annot.h on all eight finish entries (ca_canny_emit, ca_hed_fuse, ca_lineart_finish,
ca_lanime_finish, ca_mlsd_draw, ca_softedge_fuse, ca_depth_finish, ca_nbae_finish), through their wrappers in kernels.py.

What each annotator's own suite asserts -- the uint8 map against its specification -- is not repeated here.  This file pins what the
entries share: the control tensor [rep * images, 3, H, W] equals map / 255 cast to its dtype bit for bit in every channel and both rep
halves (NormalBae: per channel; canny: 0.0 / 1.0), the map does not depend on whether the control tensor is written with it, a control
tensor written alone equals the one written with the map, and nothing outside the outputs is touched (they lie inside larger filled
buffers whose margins are compared).

Planes: images = 3 at the smallest plane the entry's own checks admit -- h * w = 4 for the four-pixels-per-thread finishes, so every
thread lands in another image; 8 x 8 for softedge (four levels), 16 x 16 for HED (five levels), one pixel for the scalar depth finish --
and one larger plane whose pixel count is no power of two; canny also takes a plane with h * w % 4 != 0 (its scalar tail).  Inputs are
seeded values that reach both clamps, with a NaN where the kernel documents that a NaN counts as 0.  Exact comparisons throughout: the
reference is IEEE division of the map's own bytes on the host.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 3
PAD = 64          # elements of margin on either side of an output
FILL = {torch.uint8: 0x5A, torch.float32: 7.0, torch.float16: 7.0}

PLANES = {"canny": [(2, 2), (4, 6), (3, 5)], "hed": [(16, 16), (16, 48)], "lineart": [(2, 2), (4, 6)], "lanime": [(2, 2), (4, 6)],
          "mlsd": [(2, 2), (4, 6)], "softedge": [(8, 8), (8, 24)], "depth": [(1, 1), (3, 5)], "nbae": [(2, 2), (4, 6)]}
CASES = [(e, hw) for e, planes in PLANES.items() for hw in planes]


def _k():
    from controlanimate_amd import kernels
    return kernels


def _randn(seed, *shape, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def _guarded(shape, dtype):
    """(buffer, view): the view of `shape` lies PAD elements inside the filled flat buffer (PAD elements keep 16-byte alignment)."""
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * PAD,), FILL[dtype], dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + numel].view(shape)


def _margins_untouched(buf):
    fill = torch.full((PAD,), FILL[buf.dtype], dtype=buf.dtype)
    return torch.equal(buf[:PAD].cpu(), fill) and torch.equal(buf[-PAD:].cpu(), fill)


def _bits(t):
    return t.cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _runner(entry, h, w):
    """run(map, control, rep) for one entry on its seeded inputs, and the map's shape."""
    k = _k()
    shape = (N, h, w)
    if entry == "canny":
        frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (N, h, w, 3), dtype=np.uint8)).to(DEV)
        ws = torch.empty(k.canny_workspace_bytes(N, h, w), dtype=torch.uint8, device=DEV)
        k.canny_classify(frames, 100, 200, ws)
        k.canny_link(N, h, w, ws)
        return (lambda m, c, rep: k.canny_emit(N, h, w, ws, edges=m, control=c, rep=rep)), shape
    if entry == "hed":
        sides = [_randn(k_, N, h >> k_, w >> k_, scale=6.0) for k_ in range(5)]
        return (lambda m, c, rep: k.hed_fuse(sides, edges=m, control=c, rep=rep)), shape
    if entry in ("lineart", "lanime"):
        x = _randn(1, N, h, w, scale=12.0)    # sigmoid / tanh reach 0 and 1 in float64 beyond +-37 / +-19
        x[0].view(-1)[0], x[2].view(-1)[3] = 40.0, -40.0
        x[1].view(-1)[1] = float("nan")       # (a NaN counts as 0 before the inversion)
        fn = k.lineart_finish if entry == "lineart" else k.lanime_finish
        return (lambda m, c, rep: fn(x, edges=m, control=c, rep=rep)), shape
    if entry == "mlsd":
        g = torch.Generator().manual_seed(2)
        seg = torch.randint(-3, max(h, w) + 3, (N, k.MLSD_TOPK, 4), generator=g, dtype=torch.int32).to(DEV)   # inside, across and outside the plane
        seg[:, 0] = torch.tensor([0, 0, w - 1, h - 1], dtype=torch.int32)                                       # the diagonal: drawn and not drawn pixels
        count = torch.tensor([1, 0, 2], dtype=torch.int32, device=DEV)
        return (lambda m, c, rep: k.mlsd_draw(seg, count, h, w, edges=m, control=c, rep=rep)), shape
    if entry == "softedge":
        sides = [_randn(10 + k_, N, h >> k_, w >> k_, scale=4.0) for k_ in range(4)]
        cls = torch.tensor([1.0, 0.5, -0.75, 0.25, 0.1], dtype=torch.float32, device=DEV)
        return (lambda m, c, rep: k.softedge_fuse(sides, cls, edges=m, control=c, rep=rep)), shape
    if entry == "depth":
        d = _randn(3, N, h, w, scale=3.0)
        _, keys = k.resize_bicubic_f32(d, h, w)   # same size: the identity, and the keys of these very values
        if h * w > 1:
            d = d.clone()
            d[1].view(-1)[2] = float("nan")   # (after the keys: a NaN counts as 0 in the finish)
        return (lambda m, c, rep: k.depth_finish(d, keys, "minmax", map=m, control=c, rep=rep)), shape
    assert entry == "nbae"
    pred = _randn(4, N, h, w, 4, scale=0.9)       # (v + 1) / 2 leaves [0, 1] on both sides
    pred[2, 0, 1, 1] = float("nan")
    return (lambda m, c, rep: k.nbae_finish(pred, map=m, control=c, rep=rep)), (N, h, w, 3)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("rep", [1, 2])
@pytest.mark.parametrize("entry,hw", CASES, ids=[f"{e}-{h}x{w}" for e, (h, w) in CASES])
def test_control_is_the_map_over_255_and_nothing_else_is_written(entry, hw, rep, dtype):
    h, w = hw
    run, map_shape = _runner(entry, h, w)
    ctrl_shape = (rep * N, 3, h, w)

    mbuf, m = _guarded(map_shape, torch.uint8)
    cbuf, c = _guarded(ctrl_shape, dtype)
    run(m, c, rep)
    torch.cuda.synchronize()
    assert _margins_untouched(mbuf) and _margins_untouched(cbuf)
    levels = m.cpu()
    if entry != "depth" or h * w > 1:
        assert levels.min() < levels.max()                                    # the inputs do produce more than one level
    per_channel = levels.permute(0, 3, 1, 2) if entry == "nbae" else levels[:, None].expand(-1, 3, -1, -1)
    want = torch.cat([per_channel.float() / 255.0] * rep).to(dtype)           # IEEE division on the host, then one rounding to fp16
    assert torch.equal(_bits(c), _bits(want))
    if entry == "canny":
        assert set(levels.unique().tolist()) <= {0, 255} and set(c.cpu().float().unique().tolist()) <= {0.0, 1.0}

    mbuf1, m1 = _guarded(map_shape, torch.uint8)                                # the map alone
    run(m1, None, rep)
    torch.cuda.synchronize()
    assert _margins_untouched(mbuf1) and torch.equal(m1.cpu(), levels)

    if entry != "mlsd":                                                         # the control tensor alone (ca_mlsd_draw always draws into a map)
        cbuf1, c1 = _guarded(ctrl_shape, dtype)
        run(None, c1, rep)
        torch.cuda.synchronize()
        assert _margins_untouched(cbuf1) and torch.equal(_bits(c1), _bits(c))
