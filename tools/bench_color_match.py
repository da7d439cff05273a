"""Times the colour match of one 16-frame window: host vid2vid.match_colors against color_match.ColorMatcher, on the same
frames in the same run, at 512x512 and 512x768.

    python tools/bench_color_match.py [--frames 16] [--runs 10] [--out profiles/color_match_bench.json] [--once]

Host: one run.  Device: warm, median of --runs calls, PIL frames in / PIL frames out (what run_windows hands the hook) and
device tensor in / out; per-stage device times from events around each stage's launches, with the bytes each stage has to move
at least and the rate that implies.  Also counts the values in which the two differ.
--once: one warm device call per size and nothing else (for a kernel trace)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _frame(h, w, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 90 * np.sin(xx / (5.0 + c) + yy / 9.0 + seed) for c in range(3)], -1) + rng.normal(0, 12, (h, w, 3))
    base[..., 2] = base[..., 2] * 0.5 + 60
    return Image.fromarray(np.clip(base, 0, 255).astype(np.uint8))


def stage_bytes(n: int, pixels: int) -> dict:
    """Least traffic per stage: uint8 frames are 3 bytes per pixel, float64 planes 24."""
    u8, f64 = n * pixels * 3, n * pixels * 24
    return {"hist": u8, "moments": u8, "transform": u8 + f64, "sort": 8 * 3 * f64,  # per pass: histogram read, scatter read + write
            "rank_map": 2 * f64, "finish": f64 + u8}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "color_match_bench.json"))
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    import torch
    from controlanimate_amd.color_match import ColorMatcher
    from controlanimate_amd.vid2vid import match_colors

    result = {"frames": a.frames, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for h, w in ((512, 512), (512, 768)):
        frames, ref = [_frame(h, w, s) for s in range(a.frames)], _frame(h, w, 99)
        cm = ColorMatcher()
        got = cm(frames, ref)  # warm-up: allocations, module load
        if a.once:
            cm(frames, ref)
            torch.cuda.synchronize()
            continue
        t0 = time.perf_counter()
        want = match_colors(frames, ref)
        host_ms = (time.perf_counter() - t0) * 1e3
        diff = [np.abs(np.asarray(g).astype(np.int64) - np.asarray(x)) for g, x in zip(got, want)]
        t_in = torch.from_numpy(np.stack([np.asarray(f) for f in frames])).cuda()
        r_in = torch.from_numpy(np.array(ref)).cuda()
        pil_ms, tensor_ms = [], []
        cm.timings = {}
        for _ in range(a.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cm(frames, ref)
            pil_ms.append((time.perf_counter() - t0) * 1e3)
        cm.timings = {}
        for _ in range(a.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cm(t_in, r_in)
            torch.cuda.synchronize()
            tensor_ms.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        need = stage_bytes(a.frames, h * w)
        stages = {}
        for name, evs in cm.timings.items():
            ms = statistics.median(s.elapsed_time(e) for s, e in evs)
            stages[name] = {"ms": round(ms, 4), "min_bytes": need[name], "gb_per_s": round(need[name] / ms / 1e6, 1)}
        cm.timings = None
        result["sizes"][f"{h}x{w}"] = {
            "host_match_colors_ms": round(host_ms, 1),
            "device_pil_in_pil_out_ms": round(statistics.median(pil_ms), 3),
            "device_tensor_in_tensor_out_ms": round(statistics.median(tensor_ms), 3),
            "device_kernels_ms": round(sum(s["ms"] for s in stages.values()), 3),
            "stages": stages,
            "values": int(sum(d.size for d in diff)),
            "values_that_differ_from_host": int(sum((d != 0).sum() for d in diff)),
            "largest_difference_levels": int(max(d.max() for d in diff)),
        }
    if a.once:
        return
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
