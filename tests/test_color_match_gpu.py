"""GPU: the colour-match kernels (ABI v15, csrc/ca_color.hip) each against numpy, then ColorMatcher against the host
vid2vid.match_colors.

Bound of the end-to-end comparison (tests 5 and 7): no value differs by more than 1 level and at most 1e-4 of the values of a
frame differ at all.  It is a condition, not a measurement: the float64 staging differs from the host in 0 values on the CPU
(tests/test_color_match_cpu.py), a float32 one in <= 9.3e-6 of them; a wrong table, rank or channel order changes whole regions,
a flipped tie or .5 rounding a handful of values.  The observed count is printed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_LEVELS, MAX_FRACTION = 1, 1e-4


@pytest.fixture(scope="module")
def K():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from controlanimate_amd import kernels
    return kernels


def _frame(h, w, seed, pil=True):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 90 * np.sin(xx / (5.0 + c) + yy / 9.0 + seed) for c in range(3)], -1) + rng.normal(0, 12, (h, w, 3))
    base[..., 2] = base[..., 2] * 0.5 + 60  # channels differ: a swapped order shows
    a = np.clip(base, 0, 255).astype(np.uint8)
    return Image.fromarray(a) if pil else a


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ws(K, images, pixels, fill=None):
    import torch
    ws = torch.empty(K.color_match_workspace_bytes(images, pixels), dtype=torch.uint8, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    return ws


def _within_bound(got, want, what):
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    assert got.shape == want.shape, what
    diff = np.abs(got - want)
    n_diff, worst = int((diff != 0).sum()), int(diff.max())
    print(f"{what}: {n_diff} of {diff.size} values differ, largest difference {worst}")
    assert worst <= MAX_LEVELS, (what, worst)
    assert n_diff <= MAX_FRACTION * diff.size, (what, n_diff, diff.size)
    return n_diff


# ---- 1. histogram -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("images,pixels", [(3, 64 * 96), (2, 5003), (1, 1), (2, 700001)])
def test_hist_equals_bincount(K, images, pixels):
    import torch
    rng = np.random.default_rng(pixels)
    a = rng.integers(0, 256, (images, pixels, 3), dtype=np.uint8)
    a[0, :, 1] = 77  # a constant channel: every lane hits one bin
    a[-1] = 200      # a constant image
    hist = torch.full((images, 3, 256), -1, dtype=torch.int32, device="cuda")
    K.hist_u8x3(_dev(a), hist)
    want = np.stack([[np.bincount(a[i, :, c], minlength=256) for c in range(3)] for i in range(images)])
    assert np.array_equal(hist.cpu().numpy(), want)


# ---- 2. moments ---------------------------------------------------------------------------------------------------------------

def test_moments_against_numpy_and_bitwise_repeatable(K):
    import torch
    from controlanimate_amd.color_match import centred_moments
    rng = np.random.default_rng(2)
    images, pixels = 3, 256 * 320 + 17
    a = np.stack([_frame(256, 321, s, pil=False).reshape(-1, 3)[:pixels] for s in range(images)])
    lut = rng.normal(100, 40, (images, 3, 256))
    mean = np.stack([[lut[i, c][a[i, :, c]].mean() for c in range(3)] for i in range(images)])
    ad, lutd, meand = _dev(a), _dev(lut), _dev(mean)
    runs = []
    for fill in (0x00, 0xFF):
        out = torch.full((images, 6), float("nan"), dtype=torch.float64, device="cuda")
        K.color_moments_f64(ad, lutd, meand, out, _ws(K, images, pixels, fill))
        runs.append(out.cpu().numpy())
    assert runs[0].tobytes() == runs[1].tobytes(), "two runs must agree bit for bit"
    want = np.stack([centred_moments(a[i], lut[i], mean[i]) for i in range(images)])
    scale = np.abs(want).max(axis=1, keepdims=True)  # s01 may cancel to near zero: relative to the image's largest moment
    rel = np.abs(runs[0] - want) / scale
    print("moments: largest relative error", rel.max())
    assert rel.max() <= 1e-12


# ---- 3. sort ------------------------------------------------------------------------------------------------------------------

def _sort_case(K, keys):
    """keys float64 [segments, n]; guard words before and after both key buffers."""
    import torch
    segments, n = keys.shape
    guard = 64
    buf_in = torch.full((guard + segments * n + guard,), 1234.5, dtype=torch.float64, device="cuda")
    buf_out = torch.full((guard + segments * n + guard,), -4321.5, dtype=torch.float64, device="cuda")
    kin = buf_in[guard:guard + segments * n].view(segments, n)
    kout = buf_out[guard:guard + segments * n].view(segments, n)
    kin.copy_(_dev(keys))
    K.sort_f64_segments(kin, kout, _ws(K, (segments + 2) // 3, n, 0xFF))
    torch.cuda.synchronize()
    got = kout.cpu().numpy()
    assert np.array_equal(got, np.sort(keys, axis=1)), (segments, n)
    assert np.array_equal(kin.cpu().numpy(), keys), "the input keys must stay untouched"
    for b, v in ((buf_in, 1234.5), (buf_out, -4321.5)):
        assert bool((b[:guard] == v).all()) and bool((b[-guard:] == v).all()), "guard words overwritten"


def test_sort_normal_data_full_size(K):
    rng = np.random.default_rng(3)
    _sort_case(K, rng.normal(0.0, 100.0, (6, 393216)))


@pytest.mark.parametrize("n", [1, 255, 257, 4099, 12289])
def test_sort_odd_sizes(K, n):
    rng = np.random.default_rng(n)
    _sort_case(K, rng.normal(0.0, 1.0, (4, n)))


def test_sort_degenerate_orders(K):
    n = 9001
    rng = np.random.default_rng(4)
    asc = np.sort(rng.normal(0, 1, n))
    keys = np.stack([np.full(n, 3.25), rng.choice([-1.5, 2.0], n), asc, asc[::-1].copy(), np.zeros(n)])
    _sort_case(K, keys)


def test_sort_many_exponents_both_signs(K):
    rng = np.random.default_rng(5)
    n = 20011
    keys = rng.choice([-1.0, 1.0], (3, n)) * 10.0 ** rng.uniform(-300, 300, (3, n))
    keys[0, :7] = [0.0, 5e-324, -5e-324, 1.7976931348623157e308, -1.7976931348623157e308, 1.0, -1.0]
    _sort_case(K, keys)


def test_sort_in_place(K):
    import torch
    rng = np.random.default_rng(6)
    keys = rng.normal(0, 1, (3, 5000))
    k = _dev(keys)
    K.sort_f64_segments(k, k, _ws(K, 1, 5000))
    torch.cuda.synchronize()
    assert np.array_equal(k.cpu().numpy(), np.sort(keys, axis=1))


# ---- 4. rank map + finish -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("ties", [False, True])
def test_rank_map_and_finish_against_numpy(K, normalize, ties):
    import torch
    from controlanimate_amd.color_match import finish_u8, rank_map
    rng = np.random.default_rng(7)
    images, pixels = 2, 96 * 131
    y = rng.normal(0.4, 0.3, (images, 3, pixels))
    if ties:
        y = np.round(y * 20) / 20  # a few dozen distinct values: almost all ties
    knots = []
    for c, k in enumerate((256, 1, 37)):  # full, single-knot (constant reference channel) and sparse channels
        cnt = rng.integers(1, 50, k)
        knots.append((np.cumsum(cnt).astype(np.float64) / cnt.sum(), np.sort(rng.choice(256, k, replace=False)).astype(np.float64) / 255.0))
    kq, kv = np.zeros((3, 256)), np.zeros((3, 256))
    for c, (q, v) in enumerate(knots):
        kq[c, :len(q)], kv[c, :len(q)] = q, v
    ws = _ws(K, images, pixels, 0xFF)
    yd = _dev(y)
    srt = torch.empty_like(yd)
    K.sort_f64_segments(yd, srt, ws)
    o = torch.empty_like(yd)
    K.color_rank_map_f64(yd, srt, o, _dev(kq), _dev(kv), torch.tensor([len(k[0]) for k in knots], dtype=torch.int32, device="cuda"), ws)
    out = torch.empty((images, pixels, 3), dtype=torch.uint8, device="cuda")
    K.color_finish_u8(o, out, normalize, ws)
    torch.cuda.synchronize()
    want_o = np.stack([[rank_map(y[i, c], np.sort(y[i, c]), *knots[c]) for c in range(3)] for i in range(images)])
    assert np.array_equal(o.cpu().numpy(), want_o), "rank map must equal the numpy expression bit for bit"
    want = np.stack([finish_u8(want_o[i].T, normalize) for i in range(images)])
    assert np.array_equal(out.cpu().numpy(), want)


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("h,w", [(512, 512), (512, 768)])
def test_color_matcher_against_host(K, h, w, normalize):
    from controlanimate_amd.color_match import ColorMatcher
    from controlanimate_amd.vid2vid import match_colors
    frames = [_frame(h, w, s) for s in range(4)]
    ref = _frame(h, w, 11)
    got = ColorMatcher(normalize=normalize)(frames, ref)
    want = match_colors(frames, ref, normalize=normalize)
    assert len(got) == 4 and all(type(g) is type(f) for g, f in zip(got, frames))
    for i, (g, x) in enumerate(zip(got, want)):
        _within_bound(g, x, f"{h}x{w} normalize={normalize} frame {i}")


@pytest.mark.parametrize("normalize", [True, False])
def test_color_matcher_special_frames(K, normalize):
    from controlanimate_amd.color_match import ColorMatcher
    from controlanimate_amd.vid2vid import match_colors
    h, w = 96, 128
    ref = _frame(80, 112, 12, pil=False)  # another size than the frames
    poster = _frame(h, w, 1, pil=False) // 32 * 32 + 16
    const = np.full((h, w, 3), 77, np.uint8)
    low = np.clip(_frame(h, w, 2, pil=False), 20, 230)
    frames = [poster, const, low]
    got = ColorMatcher(normalize=normalize)(frames, ref)
    want = match_colors(frames, ref, normalize=normalize)
    for name, g, x in zip(("posterised", "constant", "low contrast"), got, want):
        assert isinstance(g, np.ndarray)
        _within_bound(g, x, f"{name} normalize={normalize}")
    # a constant reference (hi == lo branch of the reference's table, single-knot interpolation)
    cref = np.full((h, w, 3), 50, np.uint8)
    _within_bound(ColorMatcher(normalize=normalize)([low], cref)[0], match_colors([low], cref, normalize=normalize)[0], f"constant reference normalize={normalize}")
    # rank-deficient covariance (two flat colours): the host algorithm is ill-conditioned there; only finite, uint8, right shape
    two = np.zeros((h, w, 3), np.uint8)
    two[:, : w // 2] = (200, 40, 90)
    two[:, w // 2:] = (20, 180, 60)
    out = ColorMatcher(normalize=normalize)([two], ref)[0]
    assert out.dtype == np.uint8 and out.shape == (h, w, 3)


# ---- 6. tensor route, repeatability, scratch ------------------------------------------------------------------------------------

def test_tensor_route_repeatable_and_scratch_independent(K):
    import torch
    from controlanimate_amd.color_match import ColorMatcher
    h, w = 120, 200
    frames = [_frame(h, w, s) for s in range(3)]
    ref = _frame(h, w, 13)
    cm = ColorMatcher()
    pil = np.stack([np.asarray(f) for f in cm(frames, ref)])
    t_in = _dev(np.stack([np.asarray(f) for f in frames]))
    t_out = cm(t_in, _dev(np.asarray(ref)))
    assert isinstance(t_out, torch.Tensor) and t_out.is_cuda and t_out.dtype == torch.uint8 and tuple(t_out.shape) == (3, h, w, 3)
    assert np.array_equal(t_out.cpu().numpy(), pil)
    assert np.array_equal(cm(t_in, _dev(np.asarray(ref))).cpu().numpy(), pil), "two calls must give identical bytes"
    cm.workspace(3, h * w).fill_(0xFF)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        again = cm(t_in, _dev(np.asarray(ref)))
    side.synchronize()
    assert np.array_equal(again.cpu().numpy(), pil), "no stage may read scratch it did not write"


def test_float_frames_are_refused(K):
    from controlanimate_amd.color_match import ColorMatcher
    with pytest.raises(TypeError):
        ColorMatcher()([np.zeros((8, 8, 3), np.float32)], np.zeros((8, 8, 3), np.uint8))


# ---- 7. the window loop -------------------------------------------------------------------------------------------------------

def test_run_windows_with_color_matcher(K):
    from controlanimate_amd.color_match import ColorMatcher
    from controlanimate_amd.vid2vid import WindowConfig, run_windows

    def animate(batch, last, cfg):
        return [_frame(64, 64, 100 * cfg.epoch + i) for i in range(len(batch))]

    def run(hook):
        cfg = WindowConfig(frame_count=8, overlap_length=4)
        return [f for win in run_windows(None, animate, cfg, total_frames=16, match_colors=hook) for f in win]

    from controlanimate_amd import vid2vid
    assert len(list(run_windows(None, animate, WindowConfig(frame_count=8, overlap_length=4), total_frames=16, match_colors=None))) == 3
    got, want = run(ColorMatcher()), run(vid2vid.match_colors)
    assert len(got) == len(want) == 16
    total = 0
    for i, (g, x) in enumerate(zip(got, want)):
        # blended frames mix two matched frames: the bound holds per frame all the same (a 1-level difference stays <= 1 level)
        total += _within_bound(g, x, f"window frame {i}")
    print("run_windows: differing values in total", total)
