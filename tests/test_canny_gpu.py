"""GPU: CannyAnnotator (ABI v16, csrc/ca_canny.hip) against the host annotators.canny_edges.  Every comparison is exact
(np.array_equal, 0 differing pixels): the algorithm is integer.  The inputs are the smallest at which each part can go wrong; the
facts that make them hard (growth depth, strong / promoted / dropped counts, weak-only chains) are recomputed from the host
function and asserted before the device is compared, so a weakened input cannot pass silently."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from controlanimate_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def ann(K):
    from controlanimate_amd.annotators import CannyAnnotator
    return CannyAnnotator("cuda")


def _host(img, low=100, high=200):
    from controlanimate_amd.annotators import canny_edges
    return canny_edges(img, low, high)


def _facts(img, low=100, high=200):
    """(strong, candidates, edges, growth depth) of the host function: with low = high every candidate is strong, so the two
    masks come from canny_edges itself; the depth is the number of sweeps of its hysteresis loop."""
    strong, cand = _host(img, high, high) > 0, _host(img, low, low) > 0
    out, depth = strong.copy(), 0
    while True:
        p = np.pad(out, 1)
        nb = p[:-2, :-2] | p[:-2, 1:-1] | p[:-2, 2:] | p[1:-1, :-2] | p[1:-1, 2:] | p[2:, :-2] | p[2:, 1:-1] | p[2:, 2:]
        grown = out | (cand & nb)
        if grown.sum() == out.sum():
            break
        out, depth = grown, depth + 1
    assert np.array_equal(out, _host(img, low, high) > 0)
    return int(strong.sum()), int(cand.sum()), int(out.sum()), depth


def snake(h, w, seeded=True):
    """Bands of 30, 6 px high, every 16 rows from row 4, columns 4 .. w - 4, joined alternately at the right and the left end by a
    6-px column of 30: one long chain of weak candidates.  seeded: columns 12..14 of the first band are 240 (the only strong pixels)."""
    img = np.zeros((h, w), np.uint8)
    rows = list(range(4, h - 6, 16))
    for i, r in enumerate(rows):
        img[r:r + 6, 4:w - 4] = 30
        if i + 1 < len(rows):
            cols = slice(w - 10, w - 4) if i % 2 == 0 else slice(4, 10)
            img[r:rows[i + 1] + 6, cols] = 30
    if seeded:
        img[4:10, 12:15] = 240
    return img


def smoothed_noise(h, w, c=3, seed=7, passes=2):
    a = np.random.default_rng(seed).integers(0, 256, (h, w, c) if c else (h, w)).astype(np.float64)
    for _ in range(passes):
        a = (a + np.roll(a, 1, 0) + np.roll(a, -1, 0) + np.roll(a, 1, 1) + np.roll(a, -1, 1)) / 5.0
    span = a.max() - a.min()
    return ((a - a.min()) / (span if span else 1.0) * 255.0).astype(np.uint8)


def structured(h, w, seed=0):
    """Smoothed noise plus shapes: soft texture with long weak chains, hard outlines that seed them."""
    rng = np.random.default_rng(seed)
    a = smoothed_noise(h, w, 3, seed=seed + 100, passes=3).astype(np.float64)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(6):
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(min(h, w) // 12 + 2, min(h, w) // 4 + 3)
        m = (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
        a[m] = a[m] * 0.5 + rng.integers(0, 256, 3) * 0.5
    for _ in range(4):
        y0, x0 = rng.integers(0, h), rng.integers(0, w)
        m = (yy >= y0) & (yy < y0 + h // 5 + 1) & (xx >= x0) & (xx < x0 + w // 4 + 1)
        a[m] = a[m] * 0.7 + rng.integers(0, 256, 3) * 0.3
    a += 20.0 * np.sin((xx + 2 * yy) / 23.0)[..., None]
    return np.clip(a, 0, 255).astype(np.uint8)


def _equal(ann, frames, low=None, high=None):
    """Device edges of the list `frames` == host, frame by frame; returns the device result."""
    from controlanimate_amd.annotators import CannyAnnotator
    a = ann if low is None else CannyAnnotator("cuda", low, high)
    got = a.edges(frames).cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == (len(frames),) + np.asarray(frames[0]).shape[:2]
    for i, f in enumerate(frames):
        want = _host(f, a.low, a.high)
        assert np.array_equal(got[i], want), (i, int((got[i] != want).sum()))
    return got


# ---- hysteresis --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w,depth,edges", [(70, 133, 512, 1064), (150, 201, 1787, 3618)])
def test_seeded_snake(ann, h, w, depth, edges):
    img, bare = snake(h, w), snake(h, w, seeded=False)
    s, c, e, d = _facts(img)
    assert (s, c, e, d) == (18, edges, edges, depth) and d >= 256
    sb, cb, eb, _ = _facts(bare)
    assert (sb, cb, eb) == (0, edges - 8, 0)
    got = _equal(ann, [img])
    assert int((got > 0).sum()) == edges
    assert not _equal(ann, [bare]).any()


@pytest.mark.parametrize("low,high", [(250, 500), (100, 200)])
def test_smoothed_noise(ann, low, high):
    """67 x 45 x 3, default_rng(7): at 250 / 500 the host gives 236 strong, 746 promoted and 161 dropped of 1143 candidates."""
    img = smoothed_noise(67, 45)
    s, c, e, _ = _facts(img, low, high)
    if (low, high) == (250, 500):
        assert min(s, e - s, c - e) >= 0.05 * c, (s, e - s, c - e, c)
    _equal(ann, [img], low, high)


def test_links_random_class_maps(K):
    """ca_canny_link alone on class bytes written by the test (the workspace layout of the header: labels, then class bytes, then
    flags): random maps near the percolation threshold have components that cross every kind of tile border many times."""
    import torch
    n, h, w = 3, 2 * K.CANNY_TILE_H + 5, 3 * K.CANNY_TILE_W + 7
    rng = np.random.default_rng(3)
    cls = np.zeros((n, h, w), np.uint8)
    for i, p in enumerate((0.35, 0.45, 0.6)):
        cls[i] = rng.random((h, w)) < p
        cls[i][(rng.random((h, w)) < 0.002) & (cls[i] > 0)] = 2
    want = np.zeros((n, h, w), np.uint8)
    for i in range(n):
        cand, out = cls[i] > 0, cls[i] == 2
        while True:
            p = np.pad(out, 1)
            nb = p[:-2, :-2] | p[:-2, 1:-1] | p[:-2, 2:] | p[1:-1, :-2] | p[1:-1, 2:] | p[2:, :-2] | p[2:, 1:-1] | p[2:, 2:]
            grown = out | (cand & nb)
            if grown.sum() == out.sum():
                break
            out = grown
        assert 0.05 * cand.sum() < out.sum() < 0.98 * cand.sum() or i == 2
        want[i] = out * 255
    total = n * h * w
    ws = torch.full((K.canny_workspace_bytes(n, h, w),), 0xAB, dtype=torch.uint8, device="cuda")
    ws[4 * total:5 * total] = torch.from_numpy(cls.reshape(-1)).cuda()
    got = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    K.canny_link(n, h, w, ws)
    K.canny_emit(n, h, w, ws, edges=got)
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("flip", [False, True])
def test_diagonal_link_across_a_tile_corner(ann, K, flip):
    """A 2-px band of 30 along a 45-degree line: two weak-only chains, 1 px wide, one of which steps from tile (0, 0) into the
    diagonally opposite tile through the corner alone.  Seeded by its first five rows, which are 60: inside the first tile."""
    th, tw = K.CANNY_TILE_H, K.CANNY_TILE_W
    assert (th, tw) == (16, 64)  # the offset below puts the chain on the corner (16, 64)
    h, w = 100, 3 * tw if flip else 200
    yy, xx = np.mgrid[0:h, 0:w]
    d = xx - yy - 46
    band = (d >= 0) & (d < 2)
    img = np.where(band, 30, 0).astype(np.uint8)
    img[band & (yy < 5)] = 60
    if flip:
        img = np.ascontiguousarray(img[:, ::-1])
    want = _host(img)
    strong, cand = _host(img, 200, 200) > 0, _host(img, 100, 100) > 0
    sy, sx = np.nonzero(strong)
    assert len(sy) > 0 and sy.max() < 8                                     # weak-only away from the seed
    a, b = ((th - 1, tw - 1), (th, tw)) if not flip else ((th - 1, w - tw), (th, w - tw - 1))
    other = ((a[0], b[1]), (b[0], a[1]))
    assert cand[a] and cand[b] and not cand[other[0]] and not cand[other[1]]  # the two are linked through the corner alone
    assert want[a] == 255 and want[b] == 255 and want[60:].any()             # and the host promotes the chain beyond it
    _equal(ann, [img])


# ---- gradient, suppression, borders ---------------------------------------------------------------------------------------------

def _shapes(K):
    th, tw = K.CANNY_TILE_H, K.CANNY_TILE_W
    return [(1, 1), (1, 9), (9, 1), (5, 7), (th, tw), (th + 1, tw), (th, tw + 1), (th + 1, tw + 1), (3 * th - 1, 3 * tw - 1)]


@pytest.mark.parametrize("c", [0, 3])
def test_shapes(ann, K, c):
    for h, w in _shapes(K):
        img = smoothed_noise(h, w, c, seed=h * 1000 + w, passes=1)
        if h * w > 100:
            assert _host(img).any()
        _equal(ann, [img])


def test_channel_choice(ann):
    green = np.zeros((24, 24, 3), np.uint8)
    green[:, 12:, 1] = 255                                                  # an edge only in green
    assert _equal(ann, [green]).any()
    # blue is red mirrored: the same gradient sizes with the opposite dx sign wherever the pattern is symmetric, and there the
    # first channel decides the sector and the diagonal
    r = (np.random.default_rng(0).random((8, 8)) < 0.5).astype(np.uint8) * 200
    two = np.zeros((8, 8, 3), np.uint8)
    two[..., 0], two[..., 2] = r, r[:, ::-1]
    swapped = np.ascontiguousarray(two[..., ::-1])
    assert not np.array_equal(_host(two), _host(swapped))                   # only ties make the order of the channels show
    _equal(ann, [two])
    _equal(ann, [swapped])


def test_batch_isolation_and_workspace_contents(ann):
    import torch
    h, w = 70, 133
    frames = [snake(h, w), snake(h, w, seeded=False), smoothed_noise(h, w, 0, seed=11)]
    got = _equal(ann, frames)
    assert got[0].any() and not got[1].any() and got[2].any()
    for i, f in enumerate(frames):
        assert np.array_equal(ann.edges([f]).cpu().numpy()[0], got[i])
    ws = ann.workspace(3, h, w)
    for fill in (0xFF, 0x00):
        ws.fill_(fill)
        assert np.array_equal(ann.edges(frames).cpu().numpy(), got)
    rgb = [np.repeat(f[:, :, None], 3, 2) for f in frames]
    assert np.array_equal(ann.edges(torch.from_numpy(np.stack(rgb)).cuda()).cpu().numpy(), got)


# ---- emit, capture, pipeline ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", [(40, 52), (37, 45)])   # h * w a multiple of 4 (packed stores) and not
def test_emit_control_tensor(ann, h, w):
    import torch
    from PIL import Image
    from controlanimate_amd.annotators import canny
    from controlanimate_amd.controlresiduals_pipeline import _image_to_chw01
    frames = [Image.fromarray(structured(h, w, seed=s)) for s in range(3)]
    base = torch.stack([_image_to_chw01(canny(f)) for f in frames])
    assert 0 < base.mean() < 1
    for dtype in (torch.float32, torch.float16):
        for rep in (1, 2):
            got = ann.annotate_batch(frames, rep=rep, dtype=dtype)
            assert got.dtype == dtype and got.is_cuda and torch.equal(got.cpu(), torch.cat([base] * rep).to(dtype))
    for dtype in (torch.float32, torch.float16):
        out = torch.full((6, 3, h, w), 7.0, dtype=dtype, device="cuda")
        ptr = out.data_ptr()
        ret = ann.annotate_batch(frames, out=out, rep=2, dtype=dtype)
        assert ret is out and out.data_ptr() == ptr and torch.equal(out.cpu(), torch.cat([base] * 2).to(dtype))
    one = ann(frames[0])
    assert isinstance(one, Image.Image) and np.array_equal(np.asarray(one), np.asarray(canny(frames[0])))
    arr = ann(np.asarray(frames[0]))
    assert isinstance(arr, np.ndarray) and np.array_equal(arr, np.asarray(one))


def test_edges_replay_in_a_captured_graph(ann):
    """No launch of the chain waits for the host: captured once, it replays for new input copied into the captured buffer."""
    import torch
    h, w = 70, 133
    a = np.stack([np.repeat(snake(h, w)[:, :, None], 3, 2), structured(h, w, 1)])
    b = np.stack([structured(h, w, 2), np.repeat(snake(h, w, seeded=False)[:, :, None], 3, 2)])
    buf = torch.from_numpy(a).cuda()
    out = torch.empty((2, h, w), dtype=torch.uint8, device="cuda")
    ann.edges(buf, out=out)   # warm-up: the workspace of this size exists before the capture
    out.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ann.edges(buf, out=out)
    for frames in (a, b, a):
        buf.copy_(torch.from_numpy(frames).cuda())
        graph.replay()
        got = out.cpu().numpy()
        for i in range(2):
            assert np.array_equal(got[i], _host(frames[i])), i
    assert out.any()


@pytest.mark.parametrize("cfg", [True, False])
def test_pipeline_with_the_device_annotator(cfg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from PIL import Image
    from controlanimate_amd.annotators import CannyAnnotator
    from controlanimate_amd.configs import controlnet_config
    from controlanimate_amd.controlnet import ControlNetModel
    from controlanimate_amd.controlresiduals_pipeline import MultiControlNetResidualsPipeline
    name = "lllyasviel/control_v11p_sd15_canny"
    net = ControlNetModel.from_config(controlnet_config(block_out_channels=(32, 64, 64, 64)))

    def pipe(annotators=None):
        return MultiControlNetResidualsPipeline([name], [1.0], use_lcm=False, controlnets=[net], device="cuda", annotators=annotators)

    frames = [Image.fromarray(structured(48, 72, seed=s)) for s in range(4)]
    nxt = [Image.fromarray(structured(48, 72, seed=10 + s)) for s in range(4)]
    host, dev = pipe(), pipe({"canny": CannyAnnotator("cuda")})
    host.prep_control_images(frames, do_classifier_free_guidance=cfg)
    dev.prep_control_images(frames, do_classifier_free_guidance=cfg)
    want, got = host.prep_images[0], dev.prep_images[0]
    assert got.shape == want.shape == ((8 if cfg else 4), 3, 48, 72) and got.dtype == want.dtype and got.device == want.device
    assert torch.equal(got, want) and 0 < got.mean() < 1 and got._cfg_doubled is cfg
    ptr = got.data_ptr()
    host.prep_control_images(nxt, do_classifier_free_guidance=cfg)
    dev.prep_control_images(nxt, do_classifier_free_guidance=cfg)
    assert dev.prep_images[0] is got and got.data_ptr() == ptr and got._cfg_doubled is cfg
    assert torch.equal(got, host.prep_images[0])


def test_full_size_frame(ann):
    img = structured(512, 768, seed=5)
    want = _host(img)
    s, c, e = int((_host(img, 200, 200) > 0).sum()), int((_host(img, 100, 100) > 0).sum()), int((want > 0).sum())
    assert s > 1000 and e - s > 1000 and c - e > 1000, (s, c, e)          # strong, promoted and dropped candidates all occur
    got = ann.edges([img]).cpu().numpy()[0]
    assert np.array_equal(got, want), int((got != want).sum())


def test_pipeline_on_another_device_than_the_annotator():
    """As the per-frame path's .to(self.device): the control tensor lands on the pipeline's device, window after window."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from PIL import Image
    from controlanimate_amd.annotators import CannyAnnotator
    from controlanimate_amd.configs import controlnet_config
    from controlanimate_amd.controlnet import ControlNetModel
    from controlanimate_amd.controlresiduals_pipeline import MultiControlNetResidualsPipeline
    name = "lllyasviel/control_v11p_sd15_canny"
    net = ControlNetModel.from_config(controlnet_config(block_out_channels=(32, 64, 64, 64)))
    host = MultiControlNetResidualsPipeline([name], [1.0], use_lcm=False, controlnets=[net], device="cpu")
    dev = MultiControlNetResidualsPipeline([name], [1.0], use_lcm=False, controlnets=[net], device="cpu", annotators={"canny": CannyAnnotator("cuda")})
    for seed in (0, 10):
        frames = [Image.fromarray(structured(48, 72, seed=seed + s)) for s in range(2)]
        host.prep_control_images(frames)
        dev.prep_control_images(frames)
        got = dev.prep_images[0]
        assert got.device.type == "cpu" and got._cfg_doubled is True and torch.equal(got, host.prep_images[0]) and 0 < got.mean() < 1


def test_timed_launches_are_the_same_chain(ann):
    """With `timings` set the three hysteresis launches go out one by one (ca_canny_link_stage): same bytes, five event pairs."""
    import torch
    h, w = 70, 133
    frames = [snake(h, w), snake(h, w, seeded=False), smoothed_noise(h, w, 0, seed=11)]
    ann.timings = {}
    try:
        _equal(ann, frames)
        torch.cuda.synchronize()
        assert list(ann.timings) == ["classify", "label", "merge", "flatten", "emit"]
        assert all(len(v) == 1 and v[0][0].elapsed_time(v[0][1]) >= 0 for v in ann.timings.values())
    finally:
        ann.timings = None
