"""GPU: the Real-ESRGAN upscaler (ABI v14) -- ca_conv3x3_narrow against fp32 torch for every layer shape of RRDBNet anime-6B, the
whole net and RealESRGANer.enhance's data flow against the CPU restatement (tests/rrdb_ref.py), the LANCZOS4 resize bit for bit,
the batched path, a full-size 512 x 768 frame and the opt-in hook of the window loop."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rrdb_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


@pytest.fixture(scope="module")
def sd():
    return rrdb_ref.rrdb_state_dict(seed=11)


@pytest.fixture(scope="module")
def up4(sd):
    from controlanimate_amd.upscaler import Upscaler
    return Upscaler(4, use_face_enhancer=False, state_dict=sd, device=DEV)


@pytest.fixture(scope="module")
def up2(sd, up4):
    from controlanimate_amd.upscaler import Upscaler
    u = Upscaler(2, use_face_enhancer=False, state_dict=sd, device=DEV)
    u.model = up4.model  # the same packed net
    return u


def _frame(h, w, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 90 * np.sin(xx / (5.0 + c) + yy / 9.0) for c in range(3)], -1) + rng.normal(0, 12, (h, w, 3))
    base[..., 2] = base[..., 2] * 0.5 + 60  # channels differ: a swapped order shows
    return Image.fromarray(np.clip(base, 0, 255).astype(np.uint8))


# (cin, cout, upsample) of every layer of the net; conv_first reads the 8-channel input of ca_rgb8_to_nhwc
SHAPES = [(8, 64, False), (64, 32, False), (96, 32, False), (128, 32, False), (160, 32, False), (192, 64, False), (64, 64, False),
          (64, 64, True), (64, 32, True), (192, 32, True), (64, 16, False)]


@pytest.mark.parametrize("cin,cout,upsample", SHAPES)
def test_narrow_conv_matches_torch(cin, cout, upsample):
    from controlanimate_amd import kernels as K
    from controlanimate_amd.upscaler import RRDBNet
    g = torch.Generator().manual_seed(cin * 7 + cout + int(upsample))
    n, h, w = 2, 37, 53
    ldx, ldy, off = cin + 24, cout + 40, 20          # read the first cin of a wider buffer, write a slice of a wider one
    xf = torch.randn(n, h, w, ldx, generator=g).half()
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    ho, wo = (2 * h, 2 * w) if upsample else (h, w)
    r1 = torch.randn(n, ho, wo, cout + 8, generator=g).half()
    r2 = torch.randn(n, ho, wo, cout, generator=g).half()
    xin = xf[..., :cin].float().permute(0, 3, 1, 2)
    if upsample:
        xin = F.interpolate(xin, scale_factor=2, mode="nearest")
    conv = F.conv2d(xin, wt.half().float(), bias, padding=1).permute(0, 2, 3, 1)
    wp = RRDBNet.pack_weight(wt, cin).half().to(DEV)
    for lrelu, res in ((False, False), (True, False), (True, True)):
        y = torch.full((n, ho, wo, ldy), float("nan"), dtype=torch.float16, device=DEV)
        kw = dict(r1=r1.to(DEV), s1=0.2, r2=r2.to(DEV), s2=1.0, s0=0.04) if res else {}
        K.conv3x3_narrow(xf.to(DEV), wp, y, cin=cin, cout=cout, bias=bias.to(DEV), channel_offset=off, upsample=upsample,
                         leaky_relu=lrelu, **kw)
        torch.cuda.synchronize()
        ref = F.leaky_relu(conv, 0.2) if lrelu else conv
        if res:
            ref = 0.04 * ref + 0.2 * r1[..., :cout].float() + r2.float()
        got = y.cpu()
        assert _rel(got[..., off:off + cout], ref) < 2e-3, (lrelu, res, _rel(got[..., off:off + cout], ref))
        assert torch.isnan(got[..., :off]).all() and torch.isnan(got[..., off + cout:]).all()


def _u8_close(got, ref):
    """The uint8 bar.  An fp16 net (the reference runs half=True too) stores every layer output in fp16; restated on the CPU with fp16
    rounding after every layer, this 64 x 96 case lands at rel-L2 1.24e-3 from fp32, uint8 max |d| 5, 95.4 % of bytes equal and
    99.87 % within 2 -- the floor of ANY fp16 execution, not of this kernel.  So: max |d| <= 8, >= 93 % equal, >= 99.5 % within 2."""
    d = np.abs(got.astype(int) - ref.astype(int))
    return d.max() <= 8 and np.mean(d == 0) >= 0.93 and np.mean(d <= 2) >= 0.995, (d.max(), np.mean(d == 0), np.mean(d <= 2))


def test_full_net_matches_restatement(sd, up4):
    from controlanimate_amd import kernels as K
    img = np.asarray(_frame(64, 96, 1))
    ref_u8, ref_raw = rrdb_ref.enhance_ref(img, sd, 4.0)
    net = up4._net()
    x8 = K.rgb8_to_nhwc(torch.from_numpy(img.copy())[None].to(DEV).contiguous(), torch.float16)
    raw = net.forward_nhwc(x8, float_out=True)[0, :, :, :3].permute(2, 0, 1).float().cpu()
    rel = _rel(raw, ref_raw)
    got_u8, _ = up4.enhance(img, outscale=4)
    d = np.abs(got_u8.astype(int) - ref_u8.astype(int))
    print(f"RRDBNet 64x96: float rel-L2 {rel:.2e}; uint8 max |d| {d.max()}, equal {np.mean(d == 0) * 100:.2f} %, "
          f"within 2 {np.mean(d <= 2) * 100:.2f} %")
    assert got_u8.shape == (256, 384, 3)
    assert rel < 5e-3
    ok, stats = _u8_close(got_u8, ref_u8)
    assert ok, stats


def test_call_scale_2_and_4_with_exact_resize(sd, up4, up2):
    fr = _frame(48, 80, 2)
    o4, o2 = np.asarray(up4(fr)), np.asarray(up2(fr))
    assert o4.shape == (192, 320, 3) and o2.shape == (96, 160, 3)
    assert np.array_equal(o2, rrdb_ref.resize_lanczos4_ref(o4, 160, 96))   # the device resize, bit for bit
    ref4, _ = rrdb_ref.enhance_ref(np.asarray(fr), sd, 4.0)
    ref2, _ = rrdb_ref.enhance_ref(np.asarray(fr), sd, 2.0)
    for got, ref in ((o4, ref4), (o2, ref2)):
        ok, stats = _u8_close(got, ref)
        assert ok, stats
    from controlanimate_amd.upscaler import Upscaler
    up15 = Upscaler(1.5, use_face_enhancer=False, state_dict=sd, device=DEV)
    up15.model = up4.model
    o15 = np.asarray(up15(fr))
    assert o15.shape == (72, 120, 3) and np.array_equal(o15, rrdb_ref.resize_lanczos4_ref(o4, 120, 72))


def test_upscale_frames_equals_calls(up2):
    frames = [_frame(40, 56, 10 + i) for i in range(5)]
    up2.max_frames_per_launch = 2
    try:
        batched = up2.upscale_frames(frames)
    finally:
        up2.max_frames_per_launch = 8
    for b, f in zip(batched, frames):
        assert np.array_equal(np.asarray(b), np.asarray(up2(f)))


def test_full_size_frame(up4):
    from controlanimate_amd import kernels as K
    frames = [_frame(512, 768, 20), _frame(512, 768, 21)]
    x8 = K.rgb8_to_nhwc(torch.from_numpy(np.array(frames[0]))[None].to(DEV).contiguous(), torch.float16)
    raw = up4._net().forward_nhwc(x8, float_out=True)
    assert raw.shape == (1, 2048, 3072, 16) and bool(torch.isfinite(raw[..., :3]).all())
    del raw, x8
    up4.max_frames_per_launch = 2
    one = up4.upscale_frames(frames)           # one pass over both frames
    up4.max_frames_per_launch = 1
    try:
        chunked = up4.upscale_frames(frames)   # one pass per frame
    finally:
        up4.max_frames_per_launch = 8
    for a, b in zip(one, chunked):
        assert np.asarray(a).shape == (2048, 3072, 3) and np.array_equal(np.asarray(a), np.asarray(b))
    torch.cuda.empty_cache()


def test_run_windows_with_upscaler(up2):
    from controlanimate_amd import vid2vid as V
    frames = [_frame(24, 32, 40 + i) for i in range(12)]

    def run(**kw):
        calls = []

        def animate(batch, last_output_frames, cfg):
            calls.append((None if last_output_frames is None else [np.asarray(f).copy() for f in last_output_frames]))
            return [V.Image.fromarray(255 - np.asarray(b)) for b in batch]

        cfg = V.WindowConfig(frame_count=6, overlap_length=2, loop_back_frames=True)
        out = [list(w) for w in V.run_windows(iter(frames), animate, cfg, **kw)]
        return out, calls

    today, calls0 = run()
    none, calls1 = run(upscaler=None)
    upw, calls2 = run(upscaler=up2)
    assert len(today) == len(none) == len(upw) > 1
    for a, b, c in zip(today, none, upw):
        assert [np.asarray(x).tobytes() for x in a] == [np.asarray(x).tobytes() for x in b]
        assert len(a) == len(c)
        for x, y in zip(a, c):
            assert np.array_equal(np.asarray(y), np.asarray(up2(x))) and np.asarray(y).shape == (48, 64, 3)
    for c0, c2 in zip(calls0, calls2):   # what the next window sees (its last_output_frames) is the un-upscaled frame
        assert (c0 is None and c2 is None) or all(np.array_equal(p, q) for p, q in zip(c0, c2))
