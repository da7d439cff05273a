"""Times the canny control images of one 16-frame window of 512x768 RGB frames: the host route of prep_control_images
(annotators.canny per frame, _image_to_chw01, torch.stack, copy to the device, torch.cat for the CFG halves) against
annotators.CannyAnnotator.annotate_batch(rep=2), on the same frames in the same run.

    python tools/bench_canny.py [--frames 16] [--runs 10] [--out profiles/canny_bench.json] [--once]

Host: --host-runs runs (default 3).  Device: warm, --runs calls each, PIL frames in (stack, one copy to the device, five launches)
and a uint8 device tensor in (five launches); the time of each of the five launches from events around it (the three hysteresis
launches go out one by one for that: ca_canny_link_stage), with the bytes each has to move at least.  Every figure is reported as median and [min, max].  Also counts the pixels in
which the device edge maps differ from the host's.  The frames are smoothed noise plus shapes: pure noise has no chains.
--once: one warm device call and nothing else (for a kernel trace)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def structured_frame(h: int, w: int, seed: int) -> np.ndarray:
    """uint8 [h, w, 3]: smoothed noise (soft texture: long chains of weak candidates) plus discs, boxes and a slow wave (hard
    outlines that seed them)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 3)).astype(np.float64)
    for _ in range(3):
        a = (a + np.roll(a, 1, 0) + np.roll(a, -1, 0) + np.roll(a, 1, 1) + np.roll(a, -1, 1)) / 5.0
    a = (a - a.min()) / (a.max() - a.min()) * 255.0
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


def stage_bytes(n: int, pixels: int, rep: int) -> dict:
    """Least traffic per launch: 3 bytes of RGB, 1 class byte, a 4-byte label and a 1-byte root flag per pixel; 12 bytes of float32
    control per pixel and CFG half.  The merge touches the pixels of tile borders only (top row, left and right column of 64 x 16
    tiles: 94 of 1024), class byte and label; its walks and the candidates' writes in flatten depend on the image and are not counted."""
    p = n * pixels
    return {"classify": p * (3 + 1),    # frames in, class bytes out
            "label": p * (1 + 4 + 1),   # class in, label and zeroed flag out
            "merge": p * 94 // 1024 * (1 + 4),
            "flatten": p * (1 + 4),     # class and label in
            "emit": p * (4 + rep * 12)}  # labels in, control out


def _spread(ms) -> dict:
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "runs": len(ms)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--out", default=os.path.join("profiles", "canny_bench.json"))
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    import torch
    from PIL import Image
    from controlanimate_amd.annotators import CannyAnnotator, canny, canny_edges
    from controlanimate_amd.controlresiduals_pipeline import _image_to_chw01

    h, w, n, rep = a.height, a.width, a.frames, 2
    arrays = [structured_frame(h, w, s) for s in range(n)]
    frames = [Image.fromarray(x) for x in arrays]
    ann = CannyAnnotator("cuda")
    out = ann.annotate_batch(frames, rep=rep, dtype=torch.float32)  # warm-up: allocations, module load
    torch.cuda.synchronize()
    if a.once:
        ann.annotate_batch(frames, out=out, rep=rep, dtype=torch.float32)
        torch.cuda.synchronize()
        return

    def host_route():
        ctrl = torch.stack([_image_to_chw01(canny(f)) for f in frames]).to("cuda")
        return torch.cat([ctrl] * rep)

    host_ms, annot_ms = [], []
    for _ in range(a.host_runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = host_route()
        torch.cuda.synchronize()
        host_ms.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    host_edges = [canny_edges(x) for x in arrays]
    annot_ms.append((time.perf_counter() - t0) * 1e3)

    t_in = torch.from_numpy(np.stack(arrays)).cuda()
    got_edges = ann.edges(t_in).cpu().numpy()
    differ = int(sum((g != x).sum() for g, x in zip(got_edges, host_edges)))
    control_equal = bool(torch.equal(out, want))

    pil_ms, tensor_ms = [], []
    for _ in range(a.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ann.annotate_batch(frames, out=out, rep=rep, dtype=torch.float32)
        torch.cuda.synchronize()
        pil_ms.append((time.perf_counter() - t0) * 1e3)
    ann.timings = {}
    for _ in range(a.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ann.annotate_batch(t_in, out=out, rep=rep, dtype=torch.float32)
        torch.cuda.synchronize()
        tensor_ms.append((time.perf_counter() - t0) * 1e3)
    need = stage_bytes(n, h * w, rep)
    stages = {}
    for name, evs in ann.timings.items():
        ms = [s.elapsed_time(e) for s, e in evs]
        stages[name] = {**_spread(ms), "min_bytes": need[name], "gb_per_s": round(need[name] / statistics.median(ms) / 1e6, 1)}
    ann.timings = None
    kernels_ms = sum(s["median_ms"] for s in stages.values())
    largest = max(stages, key=lambda k: stages[k]["median_ms"])
    link_ms = sum(stages[k]["median_ms"] for k in ("label", "merge", "flatten"))
    result = {
        "frames": n, "size": f"{h}x{w}", "rep": rep, "control_dtype": "float32", "device": torch.cuda.get_device_name(0),
        "edge_fraction": round(float(np.mean([(e > 0).mean() for e in host_edges])), 4),
        "host_route": {**_spread(host_ms), "what": "canny per frame + _image_to_chw01 + stack + copy + cat"},
        "host_canny_edges_only_ms": round(annot_ms[0], 1),
        "device_from_pil": _spread(pil_ms),
        "device_from_tensor": _spread(tensor_ms),
        "device_kernels_ms": round(kernels_ms, 4),
        "stages": stages,
        "largest_stage": largest,
        "hysteresis_ms": round(link_ms, 4),
        "merge_share_of_kernels": round(stages["merge"]["median_ms"] / kernels_ms, 3),
        "host_over_device_from_pil": round(statistics.median(host_ms) / statistics.median(pil_ms), 1),
        "host_over_device_from_tensor": round(statistics.median(host_ms) / statistics.median(tensor_ms), 1),
        "pixels": int(n * h * w),
        "pixels_that_differ_from_host": differ,
        "control_tensor_equals_host_route": control_equal,
    }
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
