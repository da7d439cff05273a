"""GPU: the NormalBae annotator (controlanimate_amd/normalbae.py, csrc/ca_normalbae.hip) against its specification (tests/normalbae_ref.py)
and against torch in the same test: the SAME-padded depthwise convolution with its pooled sums, the stem, the squeeze-and-excite gate, the
channel scaling, LeakyReLU(0.01) in the GEMM and convolution epilogues, a refinement stage, the uint8 finish, and the chain end to end on
the tiny geometry (the encoder pinned to transformers through tests/golden/normalbae_tiny*.npz) and on the B5 geometry (seeded weights).

Every input is rounded to dtype first; the reference is fp32 (float64 for the gate) torch on those values.

Tolerances.  Depthwise: the fp32 result rounded once, within one unit in the last place of dtype, plus the error of an fp32 sum of 9 / 25
products in another order (2^-21 of the sum of the products' magnitudes) plus the hardware swish (2^-21 relative).  One unit alone cannot
hold against ANY correct fp32 evaluation: where the exact pre-rounding value lies within that fp32 error of a rounding boundary of dtype,
two correct sums round to neighbours, and where the 9 / 25 products cancel, their fp32 sum in another order differs by more than a unit of
the small result; the two extra terms are exactly those two effects and nothing else.  Sums: 1e-5 relative -- to the sum of the
magnitudes, since a pool whose terms cancel has no relative accuracy in fp32 in any order of summation.  Stem, LeakyReLU GEMM / convolution: the bar of tests/test_lineart_gpu.py (relative L2 < 2.5 eps, eps = 2^-10 /
2^-8, largest error < 4 x that of the largest reference value).  Gate: 1e-5 relative to float64.  Scale and finish: exact.  Refinement
stage and end to end: the siblings' E2E bars (relative L2 <= 1e-2 fp16, 8e-2 bf16).  The uint8 map: at most one level more than a plain
torch fp16 run of the specification on the same frames (the rule of tests/test_depth_gpu.py).
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normalbae_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAME = "lllyasviel/control_v11p_sd15_normalbae"
DTYPES = [torch.float16, torch.bfloat16]
CONV_BAR = {torch.float16: 2.5 * 2.0 ** -10, torch.bfloat16: 2.5 * 2.0 ** -8}  # tests/test_lineart_gpu.py
E2E_BAR = {torch.float16: 1e-2, torch.bfloat16: 8e-2}
MANT = {torch.float16: (10, -24), torch.bfloat16: (7, -133)}   # (explicit mantissa bits, log2 of the smallest subnormal)
SEED = 0   # tests/test_normalbae_cpu.py asserts the norm condition for this seed


def _k():
    from controlanimate_amd import kernels
    return kernels


def rnd(*shape, dtype=torch.float16, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def _conv_bar(what, out, ref, dtype):
    rel = CONV_BAR[dtype]
    rel_l2 = ((out - ref).norm() / ref.norm()).item()
    max_rel = ((out - ref).abs().max() / ref.abs().max()).item()
    print(f"{what} {dtype}: rel_l2={rel_l2:.3e} max_err/max_ref={max_rel:.3e} (tol {rel:.1e})")
    assert torch.isfinite(out).all() and rel_l2 < rel and max_rel < 4 * rel


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def _smooth_frames(n, h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for _ in range(n):
        a = rng.uniform(0.02, 0.12, (3, 4))
        ph = rng.uniform(0, 6.28, (3, 2))
        out.append(np.stack([127.5 + 100 * np.sin(a[c, 0] * xx + a[c, 1] * yy + ph[c, 0]) * np.cos(a[c, 2] * xx - a[c, 3] * yy + ph[c, 1]) for c in range(3)], -1))
    return np.clip(np.rint(np.stack(out)), 0, 255).astype(np.uint8)


# ---- ca_dwconv_same -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [48, 144, 1056])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("ksize", [3, 5])
def test_dwconv_same(ksize, stride, c, dtype):
    k = _k()
    for h, w in ((2, 2), (4, 6), (8, 12)):
        x = rnd(3, h, w, c, dtype=dtype, seed=h)
        wt = rnd(c, 1, ksize, ksize, dtype=dtype, scale=0.4, seed=10 + ksize)
        bias = rnd(c, dtype=torch.float32, scale=0.3, seed=3)
        xn = x.float().permute(0, 3, 1, 2)
        (pt, pb), (pl, pr) = R.same_pad(h, ksize, stride), R.same_pad(w, ksize, stride)
        xp = F.pad(xn, (pl, pr, pt, pb))
        pre = F.conv2d(xp, wt.float(), bias, stride=stride, groups=c)
        mag = F.conv2d(xp.abs(), wt.float().abs(), bias.abs(), stride=stride, groups=c)
        want = (pre * torch.sigmoid(pre)).permute(0, 2, 3, 1)
        wpack = wt.reshape(c, ksize * ksize).t().contiguous()
        out, sums = k.dwconv_same(x.to(DEV), wpack.to(DEV), bias.to(DEV), stride=stride)
        out2, sums2 = k.dwconv_same(x.to(DEV), wpack.to(DEV), bias.to(DEV), stride=stride)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (3, -(-h // stride), -(-w // stride), c) == tuple(want.shape)
        assert torch.equal(out, out2) and torch.equal(sums, sums2)          # two runs: the same bits
        got = out.float().cpu()
        bits, low = MANT[dtype]
        once = want.to(dtype).float()
        ulp = torch.ldexp(torch.ones_like(once), (torch.frexp(once)[1] - 1 - bits).clamp(min=low))   # the spacing of dtype at the rounded reference
        # swish' is at most 1.1: the sum's reordering error passes through it almost unchanged
        tol = ulp + 1.1 * 2.0 ** -21 * mag.permute(0, 2, 3, 1) + 2.0 ** -21 * want.abs()
        err = (got - once).abs()
        print(f"dwconv_same k{ksize} s{stride} c{c} {h}x{w} {dtype}: max err / tol {float((err / tol).max()):.3f}")
        assert torch.isfinite(got).all() and (err <= tol).all()
        ssum = got.double().sum((1, 2))
        sabs = got.double().abs().sum((1, 2))
        assert ((sums.cpu().double() - ssum).abs() <= 1e-5 * sabs + 1e-30).all()


# ---- ca_nbae_stem ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cout", [48, 16])
def test_stem(cout, dtype):
    k = _k()
    frames = _smooth_frames(1, 64, 96, seed=5)
    frames[0, -1, :, :] = 255   # the last row and column meet the padding: make them matter
    frames[0, :, -1, :] = 255
    wt = rnd(cout, 3, 3, 3, dtype=dtype, scale=0.3, seed=1).float()
    bias = rnd(cout, dtype=torch.float32, scale=0.2, seed=2)
    x = R.preprocess(frames)
    pre = F.conv2d(F.pad(x, (0, 1, 0, 1)), wt, bias, stride=2)
    want = (pre * torch.sigmoid(pre)).permute(0, 2, 3, 1)
    out = torch.empty((1, 32, 48, cout), dtype=dtype, device=DEV)
    k.nbae_stem(torch.from_numpy(frames).to(DEV), wt.permute(2, 3, 1, 0).reshape(27, cout).contiguous().to(DEV), bias.to(DEV), out)
    torch.cuda.synchronize()
    got = out.float().cpu()
    _conv_bar(f"stem 64x96 -> {cout}", got, want, dtype)
    for name, sl in (("first row", (0, slice(None))), ("last row", (-1, slice(None))), ("first column", (slice(None), 0)), ("last column", (slice(None), -1))):
        _conv_bar(f"stem {name}", got[0][sl], want[0][sl], dtype)
    sym = F.conv2d(F.pad(x, (1, 0, 1, 0)), wt, bias, stride=2)   # the padding on the wrong side is told apart
    assert _rel((sym * torch.sigmoid(sym)).permute(0, 2, 3, 1), want) > 0.1


# ---- ca_se_gate -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,r", [(48, 12), (144, 6), (1824, 76)])
def test_se_gate(c, r):
    k = _k()
    n, pixels = 3, 35
    sums = rnd(n, c, dtype=torch.float32, scale=20.0, seed=1)
    wr, br = rnd(r, c, dtype=torch.float32, scale=c ** -0.5, seed=2), rnd(r, dtype=torch.float32, scale=0.3, seed=3)
    we, be = rnd(c, r, dtype=torch.float32, scale=r ** -0.5, seed=4), rnd(c, dtype=torch.float32, scale=0.3, seed=5)
    mean = sums.double() / pixels
    v = mean @ wr.double().t() + br.double()
    want = torch.sigmoid((v * torch.sigmoid(v)) @ we.double().t() + be.double())
    got = k.se_gate(sums.to(DEV), wr.to(DEV), br.to(DEV), we.t().contiguous().to(DEV), be.to(DEV), pixels)
    torch.cuda.synchronize()
    err = ((got.cpu().double() - want).abs() / want).max().item()
    print(f"se_gate c={c} r={r}: max relative error {err:.2e}; gate in [{want.min():.3f}, {want.max():.3f}]")
    assert tuple(got.shape) == (n, c) and err <= 1e-5


# ---- ca_scale_channels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_scale_channels(dtype):
    k = _k()
    x = rnd(3, 5, 7, 144, dtype=dtype, scale=2.0, seed=1)
    gate = torch.rand(3, 144, generator=torch.Generator().manual_seed(2))
    want = (x.float() * gate[:, None, None, :]).to(dtype)
    xd = x.to(DEV)
    out = k.scale_channels(xd, gate.to(DEV))
    assert torch.equal(out.cpu(), want) and torch.equal(xd.cpu(), x)
    k.scale_channels(xd, gate.to(DEV), out=xd)   # in place
    assert torch.equal(xd.cpu(), want)


# ---- CA_ACT_LEAKY001 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_leaky001_gemm(dtype):
    k = _k()
    a, w = rnd(77, 16, dtype=dtype, scale=3.0, seed=1), rnd(24, 16, dtype=dtype, seed=2)
    bias = rnd(24, dtype=torch.float32, seed=3)
    pre = a.float() @ w.float().t() + bias
    assert pre.min() < -8
    want = F.leaky_relu(pre, 0.01)
    got = k.gemm(a.to(DEV), w.to(DEV), bias=bias.to(DEV), act=k.ACT_LEAKY001).float().cpu()
    _conv_bar("gemm leaky 0.01 77x24x16", got, want, dtype)
    i = pre.argmin()
    assert abs(got.flatten()[i] - 0.01 * pre.flatten()[i]) < 0.02 * abs(0.01 * pre.flatten()[i])      # slope 0.2 would give twenty times that
    assert abs(got.flatten()[i] - 0.2 * pre.flatten()[i]) > abs(0.1 * pre.flatten()[i])


@pytest.mark.parametrize("dtype", DTYPES)
def test_leaky001_convolution(dtype):
    k = _k()
    x = rnd(2, 6, 10, 16, dtype=dtype, seed=4)
    wt = rnd(24, 16, 3, 3, dtype=dtype, scale=0.4, seed=5)
    bias = rnd(24, dtype=torch.float32, seed=6)
    pre = F.conv2d(x.float().permute(0, 3, 1, 2), wt.float(), bias, padding=1).permute(0, 2, 3, 1)
    assert pre.min() < -8
    got = k.conv3x3(x.to(DEV), wt.permute(0, 2, 3, 1).contiguous().to(DEV), bias=bias.to(DEV), act=k.ACT_LEAKY001).float().cpu()
    _conv_bar("conv3x3 leaky 0.01", got, F.leaky_relu(pre, 0.01), dtype)
    i = pre.argmin()
    assert abs(got.flatten()[i] - 0.01 * pre.flatten()[i]) < 0.02 * abs(0.01 * pre.flatten()[i])


# ---- a refinement stage ---------------------------------------------------------------------------------------------------------------
def _refine_case(c, dtype):
    """feat, pred, the MLP's fp32 (weight, bias) pairs on dtype-rounded values, the specification's output [3, 4, 8, 12] and raw."""
    g = torch.Generator().manual_seed(c)
    mlp = R._mlp(c + 4, 128).eval()
    sd = {}
    for name, p in mlp.state_dict().items():
        if name.endswith("weight"):
            t = torch.randn(p.shape, generator=g) * ((0.25 if name.startswith("6") else 2.0) / p.shape[1]) ** 0.5
        else:
            t = torch.tensor(R.HEAD_BIAS) if name.startswith("6") else 0.1 * torch.randn(p.shape, generator=g)
        sd[name] = t.to(dtype).float()
    mlp.load_state_dict(sd)
    feat = rnd(3, c, 4, 6, dtype=dtype, seed=c + 1).float()
    pred = R.norm_normalize(torch.randn(3, 4, 4, 6, generator=g))
    raws = []
    with torch.no_grad():
        want = R.refine_stage(mlp, feat, pred, raws)
    layers = [(sd[f"{j}.weight"], sd[f"{j}.bias"]) for j in (0, 2, 4, 6)]
    return feat, pred, layers, mlp, want, raws[0]


def _run_refine(feat, pred, layers, dtype, fused, monkeypatch):
    """-> (the stage's output [3, 4, 8, 12] on the host, the launch labels it recorded)."""
    from controlanimate_amd import kernels as K, normalbae as nb
    from controlanimate_amd.context import dispatch
    monkeypatch.setattr(dispatch, "nbae_refine_fused", fused)
    packed = [(w.to(DEV), b.to(DEV)) for w, b in nb.pack_mlp(layers, dtype)]
    frag = nb.pack_mlp_frag(layers, dtype)
    assert frag is not None
    frag = ([f.to(DEV) for f in frag[0]], [b.to(DEV) for b in frag[1]])
    labels = []
    monkeypatch.setattr(K, "_plan_sink", labels)
    got = nb.refine_stage(feat.permute(0, 2, 3, 1).contiguous().to(dtype).to(DEV), pred.permute(0, 2, 3, 1).contiguous().to(DEV), packed, frag=frag)
    torch.cuda.synchronize()
    monkeypatch.setattr(K, "_plan_sink", None)
    return got.cpu().permute(0, 3, 1, 2), labels


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [128, 256, 512])
def test_refine_stage(c, dtype, monkeypatch):
    feat, pred, layers, mlp, want, raw = _refine_case(c, dtype)
    nrm = raw[:, :3].norm(dim=1)
    assert nrm.min() > 0.25 * nrm.median()        # the condition on the inputs: no normalisation of a vanishing vector
    with torch.no_grad():   # align_corners: an output corner is the MLP of the source's corner
        src = torch.cat([feat, pred], 1)[:, :, [0, 0, -1, -1], [0, -1, 0, -1]]
        corner = R.norm_normalize(mlp(src).view(3, 4, 2, 2)).view(3, 4, 4)
    outs = {}
    for fused in (True, False):
        got, labels = _run_refine(feat, pred, layers, dtype, fused, monkeypatch)
        # the switch really selects the path: one launch labelled nbae_refine, or four GEMMs and no such label
        assert labels == [f"nbae_refine_c{c}"] if fused else (len(labels) == 4 and not any("nbae_refine" in x for x in labels)), labels
        rx, rk = _rel(got[:, :3], want[:, :3]), _rel(got[:, 3], want[:, 3])
        print(f"refine C={c} {dtype} {'fused' if fused else 'composed'}: xyz rel_l2 {rx:.2e}, kappa {rk:.2e}")
        assert tuple(got.shape) == (3, 4, 8, 12) and torch.isfinite(got).all() and rx <= E2E_BAR[dtype] and rk <= E2E_BAR[dtype]
        assert _rel(got[:, :, [0, 0, -1, -1], [0, -1, 0, -1]], corner) <= E2E_BAR[dtype]
        outs[fused] = got
    both = _rel(outs[True][:, :3], outs[False][:, :3]), _rel(outs[True][:, 3], outs[False][:, 3])
    print(f"refine C={c} {dtype} fused against composed: xyz {both[0]:.2e}, kappa {both[1]:.2e}")
    assert max(both) <= E2E_BAR[dtype]             # no looser than each against the specification


# ---- ca_nbae_finish -------------------------------------------------------------------------------------------------------------------
def test_finish_bytes():
    k = _k()
    one = np.float32(1.0)
    below = np.nextafter(one, np.float32(0), dtype=np.float32)    # 1 - 2^-24
    planted = [-1.0, 1.0, 0.0, below, -below, 1.5, -1.5, 7.0, -3.0, 1e-8, -1e-8]
    # values v whose (v + 1) * 0.5 * 255 lands within an fp32 ulp below an integer level
    for level in (1, 2, 37, 128, 200, 254, 255):
        t = np.nextafter(np.float32(level) / np.float32(255.0), np.float32(0), dtype=np.float32)
        for t2 in (t, np.nextafter(t, np.float32(0), dtype=np.float32), np.float32(level) / np.float32(255.0)):
            planted.append(float(np.float32(t2) * np.float32(2.0) - one))
    rng = np.random.default_rng(3)
    vals = np.concatenate([np.array(planted, np.float32), rng.uniform(-1.2, 1.2, 3 * 8 * 16 * 3 - len(planted)).astype(np.float32)])
    xyz = vals.reshape(3, 8, 16, 3)
    pred = np.concatenate([xyz, np.ones((3, 8, 16, 1), np.float32)], -1)
    want = R.tail(torch.from_numpy(xyz).permute(0, 3, 1, 2))
    assert want.shape == (3, 8, 16, 3) and want.min() == 0 and want.max() == 255
    p = torch.from_numpy(pred).to(DEV)
    m = torch.empty((3, 8, 16, 3), dtype=torch.uint8, device=DEV)
    for dt in (torch.float32, torch.float16):
        ctrl = torch.empty((6, 3, 8, 16), dtype=dt, device=DEV)
        k.nbae_finish(p, map=m, control=ctrl, rep=2)
        torch.cuda.synchronize()
        assert np.array_equal(m.cpu().numpy(), want)
        assert torch.equal(ctrl[:3], ctrl[3:])
        assert torch.equal(ctrl[:3].cpu(), (torch.from_numpy(want).permute(0, 3, 1, 2).float() / 255).to(dt))
    ctrl1 = torch.empty((3, 3, 8, 16), dtype=torch.float32, device=DEV)
    k.nbae_finish(p, control=ctrl1)
    assert torch.equal(ctrl1.cpu(), torch.from_numpy(want).permute(0, 3, 1, 2).float() / 255)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets():
    """Per geometry: the state dict (fp16 values), the fp32 specification, annotators per dtype, and per frame size the frames and the
    specification's feature list and predictions -- computed once, shared, never changed."""
    from controlanimate_amd import normalbae as nb
    out = {}
    for name, geo, sd in (("tiny", R.TINY, R.tiny_state_dict(SEED)), ("b5", R.B5, R.seeded_state_dict(R.B5, SEED))):
        sd = {k: v.half().float() for k, v in sd.items()}
        net = R.load(geo, sd).to(DEV)
        entry = {"sd": sd, "net": net, "geo": geo, "ann": {}, "cases": {}}
        for dtype in DTYPES:
            entry["ann"][dtype] = nb.NormalBaeAnnotator(sd, device=DEV, dtype=dtype, detect_resolution=64, geometry=nb.Geometry(*geo))
        for hw in ((64, 64), (64, 128)):
            frames = _smooth_frames(3, hw[0], hw[1], seed=hw[1])
            with torch.no_grad():
                x = R.preprocess(frames).to(DEV)
                feats = net.encoder(x)
                preds = net.decoder(feats)
                pred16 = net.half()(x.half())[-1].float()
                net.float()
            entry["cases"][hw] = {"frames": frames, "taps": [feats[i] for i in (4, 5, 6, 8, 11)], "pred": preds[-1], "pred16": pred16}
        out[name] = entry
    return out


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", [(64, 64), (64, 128)])
@pytest.mark.parametrize("geo", ["tiny", "b5"])
def test_e2e(nets, geo, hw, dtype, fused, monkeypatch):
    """(The tiny geometry's refinement widths, 64 / 32 / 16, are none that ca_nbae_refine is built for: both settings run the composed form there.)"""
    from controlanimate_amd import kernels as K
    from controlanimate_amd.context import dispatch
    monkeypatch.setattr(dispatch, "nbae_refine_fused", fused)
    labels = []
    monkeypatch.setattr(K, "_plan_sink", labels)
    e = nets[geo]
    ann, case = e["ann"][dtype], e["cases"][hw]
    frames = torch.from_numpy(case["frames"]).to(DEV)
    taps = ann.encoder_taps(frames)
    tap_rels = [_rel(t.permute(0, 3, 1, 2), want) for t, want in zip(taps, case["taps"])]
    got = ann.prediction(frames).permute(0, 3, 1, 2)
    rels = [_rel(got[i, :3], case["pred"][i, :3]) for i in range(3)]
    assert sum("nbae_refine" in x for x in labels) == (6 if fused and geo == "b5" else 0)      # encoder_taps and prediction: three stages each
    print(f"e2e {geo} {hw} {dtype} fused={fused}: taps {['%.2e' % r for r in tap_rels]}, xyz per frame {['%.2e' % r for r in rels]}")
    assert torch.isfinite(got).all() and max(tap_rels) <= E2E_BAR[dtype] and max(rels) <= E2E_BAR[dtype]
    if dtype == torch.float16:
        want = R.tail(case["pred"][:, :3]).astype(int)
        torch16 = np.abs(R.tail(case["pred16"][:, :3]).astype(int) - want).max()
        ours = np.abs(ann.normals(frames).cpu().numpy().astype(int) - want).max()
        print(f"   uint8 map: largest level difference torch fp16 {torch16}, product {ours}")
        assert ours <= torch16 + 1


def test_tiny_encoder_taps_against_the_transformers_fixture(nets):
    frames, taps, _, versions = R.load_fixture()
    for dtype in DTYPES:
        ann = nets["tiny"]["ann"][dtype]
        got = []   # (64 x 96 is no size of the detector's scope: the network alone takes any multiple of 32)
        ann._network(torch.from_numpy(frames).to(DEV), ann.workspace(3, 64, 96), 0, taps_out=got)
        rels = [_rel(t.permute(0, 3, 1, 2).cpu(), want) for t, want in zip(got, taps)]
        print(f"taps against {versions[0]} {dtype}: {['%.2e' % r for r in rels]}")
        assert max(rels) <= E2E_BAR[dtype]


def test_contracts(nets):
    from PIL import Image
    e = nets["tiny"]
    ann, frames = e["ann"][torch.float16], e["cases"][(64, 128)]["frames"]
    m = ann.normals(list(frames))
    assert m.dtype == torch.uint8 and tuple(m.shape) == (3, 64, 128, 3) and m.is_cuda
    out = torch.zeros((3, 64, 128, 3), dtype=torch.uint8, device=DEV)
    assert ann.normals(torch.from_numpy(frames), out=out) is out and torch.equal(out, m)
    with pytest.raises(ValueError):
        ann.normals(list(frames), out=torch.zeros((3, 64, 128), dtype=torch.uint8, device=DEV))
    ctrl = ann.annotate_batch(torch.from_numpy(frames).to(DEV), rep=2, dtype=torch.float16)
    assert tuple(ctrl.shape) == (6, 3, 64, 128) and ctrl.dtype == torch.float16 and torch.equal(ctrl[:3], ctrl[3:])
    assert torch.equal(ctrl[:3].cpu(), (m.cpu().permute(0, 3, 1, 2).float() / 255).half())
    assert not torch.equal(ctrl[:, 0], ctrl[:, 1]) and not torch.equal(ctrl[:, 1], ctrl[:, 2])
    img = ann(Image.fromarray(frames[1]))
    assert isinstance(img, Image.Image) and img.mode == "RGB" and img.size == (128, 64) and np.array_equal(np.asarray(img), m[1].cpu().numpy())
    arr = ann(frames[1])
    assert isinstance(arr, np.ndarray) and np.array_equal(arr, m[1].cpu().numpy())
    grey = frames[0][:, :, 0]
    assert torch.equal(ann.normals([grey]), ann.normals([np.repeat(grey[:, :, None], 3, 2)]))
    ann.timings = {}
    ann.normals(list(frames))
    timed, ann.timings = ann.timings, None
    torch.cuda.synchronize()
    assert set(timed) == set(ann.STAGES) == {"stem", "encoder", "decoder", "refine", "finish"}


def test_second_call_allocates_nothing(nets):
    ann, frames = nets["tiny"]["ann"][torch.float16], torch.from_numpy(nets["tiny"]["cases"][(64, 64)]["frames"]).to(DEV)
    out = torch.empty((3, 64, 64, 3), dtype=torch.uint8, device=DEV)
    first = ann.normals(frames, out=out).clone()
    ws = ann.workspace(3, 64, 64)
    pool = [(s[0].data_ptr(), s[0].numel()) for s in ws["pool"]]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    ann.normals(frames, out=out)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert [(s[0].data_ptr(), s[0].numel()) for s in ws["pool"]] == pool and torch.equal(out, first)


def test_chain_replays_in_a_captured_graph(nets):
    """No launch of the chain waits for the host: captured once, it replays for new frames copied into the captured buffer, to the eager bits."""
    ann, frames = nets["tiny"]["ann"][torch.float16], nets["tiny"]["cases"][(64, 64)]["frames"]
    eager = [ann.annotate_batch(torch.from_numpy(f).to(DEV), rep=2).clone() for f in (frames, frames[::-1].copy())]
    buf = torch.from_numpy(frames).to(DEV)
    out = torch.empty((6, 3, 64, 64), dtype=torch.float32, device=DEV)
    ann.annotate_batch(buf, out=out, rep=2)   # warm-up: the weights and the buffers are on the device before the capture
    out.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ann.annotate_batch(buf, out=out, rep=2)
    for i in (0, 1, 0):
        buf.copy_(torch.from_numpy(frames if i == 0 else frames[::-1].copy()).to(DEV))
        graph.replay()
        assert torch.equal(out, eager[i]), i
    assert 0.05 < out.mean() < 0.95


def test_chunked_passes_give_the_same_bits(nets):
    from controlanimate_amd import normalbae as nb
    e = nets["tiny"]
    frames = torch.from_numpy(e["cases"][(64, 64)]["frames"]).to(DEV)
    whole = e["ann"][torch.float16].normals(frames)
    ann = nb.NormalBaeAnnotator(e["sd"], device=DEV, dtype=torch.float16, detect_resolution=64, geometry=nb.Geometry(*e["geo"]))
    ann.max_activation_bytes = 2 * 64 * 64 * ann._bytes_per_pixel   # two frames per pass: three frames need two passes
    assert ann.chunk_frames(64, 64) == 2
    assert torch.equal(ann.normals(frames), whole)


def test_prep_control_images_leaves_the_doubled_tensor(nets):
    from PIL import Image
    from controlanimate_amd.configs import controlnet_config
    from controlanimate_amd.controlnet import ControlNetModel
    from controlanimate_amd.controlresiduals_pipeline import MultiControlNetResidualsPipeline
    ann, frames = nets["tiny"]["ann"][torch.float16], [Image.fromarray(f) for f in nets["tiny"]["cases"][(64, 128)]["frames"]]
    net = ControlNetModel.from_config(controlnet_config(block_out_channels=(32, 64, 64, 64)))
    pipe = MultiControlNetResidualsPipeline([NAME], [1.0], use_lcm=False, controlnets=[net], device="cuda", annotators={"normalbae": ann})
    pipe.prep_control_images(frames, do_classifier_free_guidance=True)
    got = pipe.prep_images[0]
    want = ann.annotate_batch(frames, rep=2)
    assert got.shape == (6, 3, 64, 128) and got.is_cuda and got._cfg_doubled is True
    assert torch.equal(got, want.to(got.dtype)) and 0.05 < got.mean() < 0.95
