"""CPU: the staged statement of the colour match (controlanimate_amd/color_match.py) against the host vid2vid.match_colors, its
table stages against vid2vid's helpers, and the argument checks of the ABI v15 entry points (no launch, no GPU)."""
import ctypes as C

import numpy as np
import pytest


def _frame(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 90 * np.sin(xx / (5.0 + c) + yy / 9.0 + seed) for c in range(3)], -1) + rng.normal(0, 12, (h, w, 3))
    base[..., 2] = base[..., 2] * 0.5 + 60  # channels differ: a swapped order shows
    return np.clip(base, 0, 255).astype(np.uint8)


def _equal(frames, ref, normalize):
    from controlanimate_amd.color_match import match_colors_staged
    from controlanimate_amd.vid2vid import match_colors
    got, want = match_colors_staged(frames, ref, normalize), match_colors(frames, ref, normalize=normalize)
    assert len(got) == len(want) == len(frames)
    for g, x in zip(got, want):
        assert type(g) is type(x)
        g, x = np.asarray(g), np.asarray(x)
        assert g.dtype == np.uint8 and np.array_equal(g, x), int((g != x).sum())


# ---- 1. byte for byte ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("h,w", [(64, 96), (256, 320)])
def test_staged_equals_host(h, w, normalize):
    _equal([_frame(h, w, 1), _frame(h, w, 2)], _frame(h, w, 9), normalize)


@pytest.mark.parametrize("normalize", [True, False])
def test_staged_equals_host_on_special_frames(normalize):
    h, w = 64, 96
    plain, low = _frame(h, w, 3), np.clip(_frame(h, w, 4), 20, 230)
    _equal([plain], low, normalize)                                  # low-contrast reference
    _equal([low], plain, normalize)                                  # low-contrast source
    _equal([plain, low], _frame(48, 80, 5), normalize)               # a reference of another size
    _equal([_frame(h, w, 6) // 32 * 32 + 16], plain, normalize)      # posterised: stage 4 is almost all ties, full-rank covariance
    _equal([np.full((h, w, 3), 77, np.uint8)], plain, normalize)     # constant frame (hi == lo)
    _equal([plain], np.full((h, w, 3), 50, np.uint8), normalize)     # constant reference


def test_staged_keeps_pil_frames():
    from PIL import Image
    _equal([Image.fromarray(_frame(32, 48, 1))], Image.fromarray(_frame(32, 48, 2)), True)


def test_rank_deficient_frame_is_finite():
    """Two flat colours: the host algorithm itself is ill-conditioned there (an inverse of a square root clamped at machine
    epsilon); no equality is claimed, only a uint8 result of the right shape."""
    from controlanimate_amd.color_match import match_colors_staged
    two = np.zeros((32, 48, 3), np.uint8)
    two[:, :24], two[:, 24:] = (200, 40, 90), (20, 180, 60)
    out = match_colors_staged([two], _frame(32, 48, 1))[0]
    assert out.dtype == np.uint8 and out.shape == two.shape


# ---- 2. the table stages against the existing helpers ---------------------------------------------------------------------------

@pytest.mark.parametrize("normalize", [True, False])
def test_first_match_table_equals_hist_match(normalize):
    from controlanimate_amd import color_match as cm
    from controlanimate_amd.vid2vid import _hist_match
    a, r = np.clip(_frame(64, 96, 1), 30, 200), _frame(48, 64, 2)
    ha, hr = cm.hist_u8x3(a), cm.hist_u8x3(r)
    ta, tr = cm.norm_table(*cm.range_from_hist(ha), normalize), cm.norm_table(*cm.range_from_hist(hr), normalize)
    assert cm.range_from_hist(ha) == (int(a.min()), int(a.max()))
    lut = cm.first_match_table(ha, ta, cm.reference_knots(hr, tr))
    got = np.stack([lut[c][a[..., c]] for c in range(3)], -1)
    assert np.array_equal(got, _hist_match(ta[a], tr[r]))


def test_mkl_matrix_and_moments_equal_mkl():
    from controlanimate_amd import color_match as cm
    from controlanimate_amd.vid2vid import _mkl
    a, r = _frame(64, 96, 3), _frame(48, 64, 4)
    rng = np.random.default_rng(0)
    lut = np.sort(rng.normal(120, 50, (3, 256)), axis=1)
    ident = np.stack([np.arange(256, dtype=np.float64)] * 3)
    ha, hr = cm.hist_u8x3(a), cm.hist_u8x3(r)
    mx, my = cm.mean_from_hist(ha, lut), cm.mean_from_hist(hr, ident)
    x = np.stack([lut[c][a[..., c]] for c in range(3)], -1)
    assert np.allclose(mx, x.reshape(-1, 3).mean(0), rtol=1e-13, atol=0)
    cs = cm.covariance(cm.centred_moments(a, lut, mx), a.shape[0] * a.shape[1])
    cr = cm.covariance(cm.centred_moments(r, ident, my), r.shape[0] * r.shape[1])
    assert np.allclose(cs, np.cov(x.reshape(-1, 3), rowvar=False), rtol=1e-12, atol=0)
    got = (x.reshape(-1, 3) - mx) @ cm.mkl_matrix(cs, cr) + my
    want = _mkl(x, r.astype(np.float64)).reshape(-1, 3)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


# ---- 3. argument checks ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def capi():
    from controlanimate_amd import _build, _capi
    _build.build(verbose=False)
    return _capi


def test_entry_points_reject_bad_arguments_without_a_launch(capi):
    lib = capi.lib()
    fake, fake2 = C.c_void_p(0x1000), C.c_void_p(0x2000)  # never dereferenced: validation fails first
    odd = C.c_void_p(0x1004)

    def expect(rc, who):
        assert rc < 0 and who.encode() in lib.ca_last_error(), (rc, lib.ca_last_error())

    need = lib.ca_color_match_workspace_bytes(16, 512 * 768)
    assert need >= 48 * 512 * 768 * 8 and need < 48 * 512 * 768 * 8 + (16 << 20)    # the second key buffer + small counters
    assert lib.ca_color_match_workspace_bytes(0, 100) == 0 and lib.ca_color_match_workspace_bytes(1, 0) == 0
    assert lib.ca_color_match_workspace_bytes(1, (1 << 30) + 1) == 0
    small = lib.ca_color_match_workspace_bytes(1, 100)

    expect(lib.ca_hist_u8x3(None, fake, 1, 100, None), "ca_hist_u8x3")
    expect(lib.ca_hist_u8x3(fake, None, 1, 100, None), "ca_hist_u8x3")
    expect(lib.ca_hist_u8x3(fake, fake2, 0, 100, None), "ca_hist_u8x3")
    expect(lib.ca_hist_u8x3(fake, fake2, 1, 0, None), "ca_hist_u8x3")

    expect(lib.ca_color_moments_f64(None, fake, fake, fake, 1, 100, fake2, small, None), "ca_color_moments_f64")
    expect(lib.ca_color_moments_f64(fake, fake, fake, None, 1, 100, fake2, small, None), "ca_color_moments_f64")
    expect(lib.ca_color_moments_f64(fake, fake, fake, fake, 1, 0, fake2, small, None), "ca_color_moments_f64")
    expect(lib.ca_color_moments_f64(fake, fake, fake, fake, 1, 100, None, small, None), "ca_color_moments_f64")
    expect(lib.ca_color_moments_f64(fake, fake, fake, fake, 1, 100, fake2, small - 1, None), "ca_color_moments_f64")
    expect(lib.ca_color_moments_f64(fake, odd, fake, fake, 1, 100, fake2, small, None), "ca_color_moments_f64")

    expect(lib.ca_color_transform_f64(fake, fake, fake, fake, fake, None, 1, 100, None), "ca_color_transform_f64")
    expect(lib.ca_color_transform_f64(fake, fake, fake, None, fake, fake2, 1, 100, None), "ca_color_transform_f64")
    expect(lib.ca_color_transform_f64(fake, fake, fake, fake, fake, fake2, 0, 100, None), "ca_color_transform_f64")
    expect(lib.ca_color_transform_f64(fake, fake, fake, fake, fake, odd, 1, 100, None), "ca_color_transform_f64")

    expect(lib.ca_sort_f64_segments(None, fake, 3, 100, fake2, small, None), "ca_sort_f64_segments")
    expect(lib.ca_sort_f64_segments(fake, None, 3, 100, fake2, small, None), "ca_sort_f64_segments")
    expect(lib.ca_sort_f64_segments(fake, fake, 0, 100, fake2, small, None), "ca_sort_f64_segments")
    expect(lib.ca_sort_f64_segments(fake, fake, 3, 0, fake2, small, None), "ca_sort_f64_segments")
    expect(lib.ca_sort_f64_segments(fake, fake, 3, 100, None, small, None), "ca_sort_f64_segments")
    expect(lib.ca_sort_f64_segments(fake, fake, 3, 100, fake2, small - 1, None), "ca_sort_f64_segments")
    expect(lib.ca_sort_f64_segments(fake, fake, 4, 100, fake2, small, None), "ca_sort_f64_segments")        # 4 segments need the bytes of 2 images

    expect(lib.ca_color_rank_map_f64(None, fake, fake2, fake, fake, fake, 1, 100, fake2, small, None), "ca_color_rank_map_f64")
    expect(lib.ca_color_rank_map_f64(fake, fake2, fake, fake, fake, None, 1, 100, fake2, small, None), "ca_color_rank_map_f64")
    expect(lib.ca_color_rank_map_f64(fake, fake2, fake2, fake, fake, fake, 1, 100, fake2, small, None), "ca_color_rank_map_f64")  # o aliases sorted
    expect(lib.ca_color_rank_map_f64(fake, fake2, fake, fake, fake, fake, 1, 100, fake2, small - 1, None), "ca_color_rank_map_f64")
    expect(lib.ca_color_rank_map_f64(fake, fake2, fake, fake, fake, fake, 1, 0, fake2, small, None), "ca_color_rank_map_f64")

    expect(lib.ca_color_finish_u8(None, fake, 1, 100, 1, fake2, small, None), "ca_color_finish_u8")
    expect(lib.ca_color_finish_u8(fake, None, 1, 100, 1, fake2, small, None), "ca_color_finish_u8")
    expect(lib.ca_color_finish_u8(fake, fake2, 1, 100, 2, fake2, small, None), "ca_color_finish_u8")
    expect(lib.ca_color_finish_u8(fake, fake2, 1, 100, 1, None, 0, None), "ca_color_finish_u8")              # normalize needs the min / max partials
    expect(lib.ca_color_finish_u8(fake, fake2, 1, 100, 1, fake2, small - 1, None), "ca_color_finish_u8")
    expect(lib.ca_color_finish_u8(fake, fake2, 0, 100, 0, None, 0, None), "ca_color_finish_u8")


def test_color_matcher_refuses_float_frames_and_has_no_cpu_fallback(capi, monkeypatch):
    import torch
    from controlanimate_amd.color_match import ColorMatcher
    u8, f32 = np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 3), np.float32)
    with pytest.raises(TypeError):
        ColorMatcher()([f32], u8)
    with pytest.raises(TypeError):
        ColorMatcher()([u8], f32)
    with pytest.raises(TypeError):
        ColorMatcher()(torch.zeros((1, 8, 8, 3), dtype=torch.float32), u8)
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "LIB_PATH", "/nonexistent/libcontrolanimate_hip.so")
    with pytest.raises(capi.CAHipUnavailable):
        ColorMatcher()([u8], u8)


def test_color_matcher_needs_a_gpu(capi):
    import torch
    from controlanimate_amd.color_match import ColorMatcher
    if torch.cuda.is_available():
        return  # covered by tests/test_color_match_gpu.py
    u8 = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(capi.CAHipUnavailable):
        ColorMatcher()([u8], u8)


# ---- 4. the window loop ---------------------------------------------------------------------------------------------------------

def test_run_windows_with_the_staged_hook():
    from controlanimate_amd.color_match import match_colors_staged
    from controlanimate_amd.vid2vid import WindowConfig, match_colors, run_windows

    def animate(batch, last, cfg):
        return [_frame(32, 48, 100 * cfg.epoch + i) for i in range(len(batch))]

    def run(hook):
        cfg = WindowConfig(frame_count=4, overlap_length=2)
        return list(run_windows(None, animate, cfg, total_frames=6, match_colors=hook))

    got, want = run(match_colors_staged), run(match_colors)
    assert [len(w) for w in got] == [len(w) for w in want] == [2, 4]
    for gw, ww in zip(got, want):
        for g, x in zip(gw, ww):
            assert np.array_equal(np.asarray(g), np.asarray(x))
