"""The window loop's colour match ('hm-mkl-hm', vid2vid.match_colors) as device stages (ABI v15, csrc/ca_color.hip).

For uint8 frames `match_colors(frames, ref, normalize)` is, per frame `a` [H, W, 3]:

  1. type_norm: a 256-entry table N from the frame's (min, max) over all channels           -> `norm_table`
  2. first histogram match: source and reference are integer valued, so per channel it is a 256-entry float64 table
     LUT1_c[v] = interp(s_q[v]; r_q, r_val), from the two 256-bin histograms alone         -> `reference_knots`, `first_match_table`
  3. Monge-Kantorovich: mean (histogram x table, `mean_from_hist`) and covariance (six centred second moments, one pass over
     the pixels) of the LUT1 image, T from them and the reference's (`mkl_matrix`), y = (x - mx) @ T + my
  4. second histogram match: y is continuous; a pixel goes to interp(rank / n; r_q, r_val) with rank = the number of pixels of
     its frame and channel that are <= it: a sort per (frame, channel) and a binary search
  5. min-max stretch over the whole frame (normalize), round half to even, clip, uint8.

`match_colors_staged` is that chain in numpy: the CPU statement of what the kernels compute, used by the tests and as
documentation.  It is NOT a fallback: `ColorMatcher` runs stages 1-5 on the GPU (ca_hist_u8x3, ca_color_moments_f64,
ca_color_transform_f64, ca_sort_f64_segments, ca_color_rank_map_f64, ca_color_finish_u8) and raises `CAHipUnavailable` without
the library or a GPU.  The table / matrix functions below work on 16 x 3 x 256 numbers per window and stay on the host for both:
a `ColorMatcher` call therefore has two small device-to-host reads (the histograms; the moments) and two small uploads between
its launches, and nothing else crosses the bus when the frames are already a device tensor.

Everything after the tables is float64 on the device as on the host: float32 values in stage 3 / 4 already move visible
levels.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from .annotator_base import HipStages
from .vid2vid import _like, _to_np

# ---- table / matrix stages (host, shared by the device path and the tests) ----------------------------------------------------


def hist_u8x3(a: np.ndarray) -> np.ndarray:
    """int64 [3, 256]: per-channel byte histogram of a uint8 [..., 3] image (what ca_hist_u8x3 computes)."""
    a = a.reshape(-1, 3)
    return np.stack([np.bincount(a[:, c], minlength=256) for c in range(3)]).astype(np.int64)


def range_from_hist(hist: np.ndarray) -> Tuple[int, int]:
    """(min, max) of the image over all channels, from its [3, 256] histogram."""
    nz = np.nonzero(hist.sum(0))[0]
    return int(nz[0]), int(nz[-1])


def norm_table(lo: int, hi: int, normalize: bool = True) -> np.ndarray:
    """float64 [256]: type_norm of match_colors as a table over the byte value.  normalize: the min-max stretch to 0..255,
    rounded half to even; a constant image (hi == lo) is what the host code makes of it, v * 255.  Otherwise v / 255."""
    v = np.arange(256, dtype=np.float64)
    if not normalize:
        return v / 255.0
    if hi != lo:
        return np.round((v - float(lo)) / (float(hi) - float(lo)) * 255.0 + 0.0)
    return v * 255.0 + 0.0


def _distinct(table: np.ndarray, hist_c: np.ndarray):
    """The distinct table values over the non-empty bins of one channel (ascending), their pixel counts, the non-empty bins and
    each bin's index into the distinct values: np.unique(..., return_inverse, return_counts) of the table image."""
    nz = np.nonzero(hist_c)[0]
    vals, inv = np.unique(table[nz], return_inverse=True)
    cnt = np.zeros(len(vals), dtype=np.int64)
    np.add.at(cnt, inv.reshape(-1), hist_c[nz])
    return vals, cnt, nz, inv.reshape(-1)


def reference_knots(ref_hist: np.ndarray, ref_table: np.ndarray) -> List[Tuple[np.ndarray, np.ndarray]]:
    """Per channel (r_q, r_val): cumulative frequency and value of the reference's non-empty bins (_hist_match's r_q, r_val)."""
    knots = []
    for c in range(3):
        vals, cnt, _, _ = _distinct(ref_table, ref_hist[c])
        knots.append((np.cumsum(cnt).astype(np.float64) / int(ref_hist[c].sum()), vals))
    return knots


def first_match_table(src_hist: np.ndarray, src_table: np.ndarray, knots) -> np.ndarray:
    """float64 [3, 256]: LUT1_c[v] = the value _hist_match gives a pixel whose byte is v (0 for bytes the frame does not have)."""
    lut = np.zeros((3, 256), dtype=np.float64)
    for c in range(3):
        _, cnt, nz, inv = _distinct(src_table, src_hist[c])
        s_q = np.cumsum(cnt).astype(np.float64) / int(src_hist[c].sum())
        lut[c, nz] = np.interp(s_q, knots[c][0], knots[c][1])[inv]
    return lut


def mean_from_hist(hist: np.ndarray, lut: np.ndarray) -> np.ndarray:
    """float64 [3]: the per-channel mean of the image lut_c[a_c], from the histogram."""
    return (hist.astype(np.float64) * lut).sum(1) / hist.sum(1).astype(np.float64)


def centred_moments(a: np.ndarray, lut: np.ndarray, mean: np.ndarray) -> np.ndarray:
    """float64 [6] = (s00, s01, s02, s11, s12, s22), s_ij = sum (lut_i[a_i] - mean_i)(lut_j[a_j] - mean_j) over the pixels of
    the uint8 image `a` (numpy statement of ca_color_moments_f64; np.cov's numerator)."""
    a = a.reshape(-1, 3)
    d = np.stack([lut[c][a[:, c]] for c in range(3)], axis=1) - mean
    m = d.T @ d
    return np.array([m[0, 0], m[0, 1], m[0, 2], m[1, 1], m[1, 2], m[2, 2]])


def covariance(moments: np.ndarray, n: int) -> np.ndarray:
    """The symmetric 3x3 covariance (N - 1 normalisation, as np.cov) from the six moments."""
    s00, s01, s02, s11, s12, s22 = (float(v) for v in moments)
    return np.array([[s00, s01, s02], [s01, s11, s12], [s02, s12, s22]]) / float(n - 1)


def mkl_matrix(cs: np.ndarray, cr: np.ndarray) -> np.ndarray:
    """T = Cs^-1/2 (Cs^1/2 Cr Cs^1/2)^1/2 Cs^-1/2 with the eigh-based square roots and the eps clamp of vid2vid._mkl."""
    eps = np.finfo(np.float64).eps

    def sqrtm(a):
        w, v = np.linalg.eigh(a)
        return (v * np.sqrt(np.clip(w, eps, None))) @ v.T

    cs_h = sqrtm(cs)
    cs_hi = np.linalg.inv(cs_h)
    return cs_hi @ sqrtm(cs_h @ cr @ cs_h) @ cs_hi


def _as_u8(frame, what: str) -> np.ndarray:
    a = _to_np(frame)
    if a.dtype != np.uint8:
        raise TypeError(f"{what} must be uint8, got {a.dtype} (vid2vid.match_colors is the route for float images)")
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"{what} must be [H, W, 3], got {a.shape}")
    return a


class _Reference:
    """Stage 1 / 2 / 3 quantities of the reference frame, from its histogram (and, for `cr`, its moments)."""

    def __init__(self, hist: np.ndarray, normalize: bool):
        self.hist = hist
        self.n = int(hist[0].sum())
        self.table = norm_table(*range_from_hist(hist), normalize)
        self.lut = np.stack([self.table] * 3)
        self.knots = reference_knots(hist, self.table)
        self.mean = mean_from_hist(hist, self.lut)


def frame_tables(hist: np.ndarray, ref: _Reference, normalize: bool) -> Tuple[np.ndarray, np.ndarray]:
    """(LUT1 [3, 256], mean [3]) of one source frame from its histogram."""
    lut = first_match_table(hist, norm_table(*range_from_hist(hist), normalize), ref.knots)
    return lut, mean_from_hist(hist, lut)


def match_colors_staged(frames: Sequence, ref_frame, normalize: bool = True) -> List:
    """`vid2vid.match_colors` for uint8 frames as the five stages of the module docstring, in numpy.  Test infrastructure and
    documentation of the device path (same tables, same order of stages), not a fallback."""
    r = _as_u8(ref_frame, "ref_frame")
    ref = _Reference(hist_u8x3(r), normalize)
    cr = covariance(centred_moments(r, ref.lut, ref.mean), ref.n)
    out = []
    for fr in frames:
        a = _as_u8(fr, "frame")
        n = a.shape[0] * a.shape[1]
        flat = a.reshape(-1, 3)
        lut, mx = frame_tables(hist_u8x3(a), ref, normalize)
        t = mkl_matrix(covariance(centred_moments(a, lut, mx), n), cr)
        x = np.stack([lut[c][flat[:, c]] for c in range(3)], axis=1)
        y = (x - mx) @ t + ref.mean
        o = np.empty_like(y)
        for c in range(3):
            o[:, c] = rank_map(y[:, c], np.sort(y[:, c]), *ref.knots[c])
        out.append(_like(finish_u8(o, normalize).reshape(a.shape), fr))
    return out


def rank_map(y: np.ndarray, y_sorted: np.ndarray, r_q: np.ndarray, r_val: np.ndarray) -> np.ndarray:
    """Stage 4 for one (frame, channel): interp(rank / n; r_q, r_val), rank = the number of values <= the pixel's."""
    rank = np.searchsorted(y_sorted, y, side="right")
    return np.interp(rank.astype(np.float64) / y.size, r_q, r_val)


def finish_u8(o: np.ndarray, normalize: bool) -> np.ndarray:
    """Stage 5: min-max stretch over the whole frame (unchanged when constant), round half to even, clip, uint8."""
    if normalize:
        lo, hi = float(o.min()), float(o.max())
        if hi != lo:
            o = (o - lo) / (hi - lo)
    return np.clip(np.round(o * 255.0), 0, 255).astype(np.uint8)


# ---- device path ------------------------------------------------------------------------------------------------------------


class ColorMatcher(HipStages):
    """`match_colors` on the GPU: `ColorMatcher(device)(frames, ref_frame)` has the contract of `vid2vid.match_colors` for uint8
    input -- PIL images or HxWx3 uint8 arrays in, the same kind out, one result per frame -- and is a drop-in for the hooks
    `run_windows(..., match_colors=...)` and `run_video_sharded(..., match_colors_fn=...)`.  All frames of a call share one size
    and go through ONE set of launches; the reference (any size) is analysed once per call.  A uint8 torch tensor [n, H, W, 3] on the
    device is accepted too and then a tensor of that kind is returned, without a host copy of the frames.

    Per call: histograms (frames + reference) -> host tables -> moments -> host 3x3 matrices -> transform, sort, rank map, finish;
    i.e. two device-to-host reads of a few KB (which synchronise the stream) and two uploads of tables.  Non-uint8 input raises
    TypeError; without the library or a GPU the call raises CAHipUnavailable (there is no CPU fallback)."""

    _no_gpu_hint = "(no CPU fallback; vid2vid.match_colors is the host function)"

    def __init__(self, device=None, normalize: bool = True):
        self.device = device
        self.normalize = bool(normalize)
        self._ws = {}   # (`timings` receives events per stage -- tools/bench_color_match.py)

    def workspace(self, images: int, pixels: int):
        """The scratch tensor of a call with `images` frames of `pixels` pixels (cached; contents are never assumed)."""
        import torch
        from . import kernels as K
        key = (images, pixels)
        if key not in self._ws:
            self._ws = {key: torch.empty(K.color_match_workspace_bytes(images, pixels), dtype=torch.uint8, device=self._device())}
        return self._ws[key]

    def __call__(self, frames, ref_frame) -> List:
        import torch
        from . import kernels as K
        as_tensor = isinstance(frames, torch.Tensor)
        if as_tensor:
            if frames.dtype != torch.uint8:
                raise TypeError(f"frames must be uint8, got {frames.dtype}")
            if frames.dim() != 4 or frames.shape[3] != 3:
                raise ValueError(f"frames tensor must be [n, H, W, 3], got {tuple(frames.shape)}")
            host = None
        else:
            host = [_as_u8(fr, "frame") for fr in frames]
            if any(h.shape != host[0].shape for h in host):
                raise ValueError("all frames of a call must share one size")
        ref_is_tensor = isinstance(ref_frame, torch.Tensor)
        if ref_is_tensor:
            if ref_frame.dtype != torch.uint8:
                raise TypeError(f"ref_frame must be uint8, got {ref_frame.dtype}")
        else:
            ref_host = _as_u8(ref_frame, "ref_frame")
        dev = self._device()
        if not as_tensor and not host:
            return []
        src = frames.to(dev).contiguous() if as_tensor else torch.from_numpy(np.stack(host)).to(dev)
        ref = (ref_frame.to(dev) if ref_is_tensor else torch.from_numpy(np.array(ref_host)).to(dev)).reshape(1, -1, 3).contiguous()
        n, h, w, _ = src.shape
        if n == 0:
            return src
        pixels, ref_pixels = h * w, ref.shape[1]
        src = src.reshape(n, pixels, 3)
        ws, ws_ref = self.workspace(n, pixels), None
        f64 = dict(dtype=torch.float64, device=dev)

        ev = self._stage("hist")
        hist = torch.empty((n + 1, 3, 256), dtype=torch.int32, device=dev)
        K.hist_u8x3(src, hist[:n])
        K.hist_u8x3(ref, hist[n:])
        if ev:
            ev[1].record()
        hist_h = hist.cpu().numpy().astype(np.int64)                                           # device -> host read 1
        rf = _Reference(hist_h[n], self.normalize)
        tabs = [frame_tables(hist_h[i], rf, self.normalize) for i in range(n)]
        lut = torch.from_numpy(np.stack([t[0] for t in tabs] + [rf.lut])).to(dev)              # [n + 1, 3, 256]
        mean = torch.from_numpy(np.stack([t[1] for t in tabs] + [rf.mean])).to(dev)            # [n + 1, 3]
        kq, kv = np.zeros((3, 256)), np.zeros((3, 256))
        for c, (r_q, r_val) in enumerate(rf.knots):
            kq[c, :len(r_q)], kv[c, :len(r_q)] = r_q, r_val
        knots_q, knots_v = torch.from_numpy(kq).to(dev), torch.from_numpy(kv).to(dev)
        knots_n = torch.tensor([len(k[0]) for k in rf.knots], dtype=torch.int32).to(dev)

        ev = self._stage("moments")
        mom = torch.empty((n + 1, 6), **f64)
        K.color_moments_f64(src, lut[:n], mean[:n], mom[:n], ws)
        if ref_pixels == pixels:
            ws_ref = ws
        else:
            ws_ref = torch.empty(K.color_match_workspace_bytes(1, ref_pixels), dtype=torch.uint8, device=dev)
        K.color_moments_f64(ref, lut[n:], mean[n:], mom[n:], ws_ref)
        if ev:
            ev[1].record()
        mom_h = mom.cpu().numpy()                                                              # device -> host read 2
        cr = covariance(mom_h[n], ref_pixels)
        t = torch.from_numpy(np.stack([mkl_matrix(covariance(mom_h[i], pixels), cr) for i in range(n)])).to(dev)
        my = mean[n].contiguous()

        y = torch.empty((n, 3, pixels), **f64)
        srt = torch.empty((n, 3, pixels), **f64)
        out = torch.empty((n, pixels, 3), dtype=torch.uint8, device=dev)
        ev = self._stage("transform")
        K.color_transform_f64(src, lut[:n], mean[:n], t, my, y)
        if ev:
            ev[1].record()
        ev = self._stage("sort")
        K.sort_f64_segments(y, srt, ws)
        if ev:
            ev[1].record()
        ev = self._stage("rank_map")
        K.color_rank_map_f64(y, srt, y, knots_q, knots_v, knots_n, ws)
        if ev:
            ev[1].record()
        ev = self._stage("finish")
        K.color_finish_u8(y, out, self.normalize, ws)
        if ev:
            ev[1].record()
        out = out.reshape(n, h, w, 3)
        if as_tensor:
            return out
        out_h = out.cpu().numpy()
        return [_like(out_h[i], fr) for i, fr in enumerate(frames)]
