"""Times the HED control images of one 16-frame window of 512x768 RGB frames: annotators.HedAnnotator.annotate_batch(rep=2) from a
uint8 device tensor and from PIL frames, each launch of the chain from events around it, and -- in the same run, on the same seeded
weights and frames -- the same network as a torch fp16 channels_last chain on the GPU (conv2d + relu, max_pool2d, the 1x1
projections, F.interpolate(bilinear), mean, sigmoid, x 255, truncation, three channels, torch.cat for the CFG halves).

    python tools/bench_hed.py [--frames 16] [--runs 10] [--out profiles/hed_bench.json] [--no-torch] [--once]

Warm: two calls of every route before its timed window.  Every figure is median and [min, max] over --runs calls, a host clock around
work that ends in a device synchronise; the per-launch figures are device events.  FLOPs and least bytes per launch are computed from
the shapes.  The weights are seeded He-normal (tests/hed_ref.py's recipe): no trained checkpoint is available, so the figures say
nothing about fp16 range on one.  The result is written after the project's own figures and again after torch's, so a torch chain
that takes long to pick its algorithms does not lose the first half.
--once: one warm device call and nothing else (for a kernel trace)."""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HED_BLOCKS = ((3, 64, 2), (64, 128, 2), (128, 256, 3), (256, 512, 3), (512, 512, 3))


def seeded_state_dict(seed: int = 0) -> dict:
    import torch
    g = torch.Generator().manual_seed(seed)
    sd = {"norm": torch.tensor([122.6789, 116.6688, 104.0069]).view(1, 3, 1, 1)}
    for b, (cin, cout, layers) in enumerate(HED_BLOCKS, start=1):
        for i in range(layers):
            ci = cin if i == 0 else cout
            sd[f"block{b}.convs.{i}.weight"] = torch.randn(cout, ci, 3, 3, generator=g) * math.sqrt(2.0 / (ci * 9))
            sd[f"block{b}.convs.{i}.bias"] = torch.randn(cout, generator=g) * 0.02
        sd[f"block{b}.projection.weight"] = torch.randn(1, cout, 1, 1, generator=g) * (0.03 / math.sqrt(cout))
        sd[f"block{b}.projection.bias"] = torch.randn(1, generator=g) * 0.1
    return sd


def frame(h: int, w: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.zeros((h, w, 3), np.float64)
    a[..., 0] = 128 + 100 * np.sin(xx / (9.0 + seed)) * np.cos(yy / 13.0)
    a[..., 1] = (xx * 2 + yy * (3 + seed)) % 256
    a[..., 2] = 255 * ((xx // 32 + yy // 32 + seed) % 2)
    a += rng.normal(0, 12, a.shape)
    return a.clip(0, 255).astype(np.uint8)


def conv_shapes(h: int, w: int):
    """(cin as the network defines it, cout, h, w) of the thirteen convolutions."""
    out = []
    for cin, cout, layers in HED_BLOCKS:
        for i in range(layers):
            out.append((cin if i == 0 else cout, cout, h, w))
        h, w = h // 2, w // 2
    return out


def _spread(ms) -> dict:
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "runs": len(ms)}


def _timed(fn, runs: int):
    import torch
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def torch_chain(sd, dev, rep: int):
    """The same network as torch ops in fp16 channels_last on the device: frames uint8 [n, H, W, 3] -> float32 control [rep n, 3, H, W]."""
    import torch
    import torch.nn.functional as F
    cl = torch.channels_last
    norm = sd["norm"].to(dev)
    blocks = []
    for b, (_, _, layers) in enumerate(HED_BLOCKS, start=1):
        convs = [(sd[f"block{b}.convs.{i}.weight"].to(dev).half().contiguous(memory_format=cl), sd[f"block{b}.convs.{i}.bias"].to(dev).half()) for i in range(layers)]
        blocks.append((convs, sd[f"block{b}.projection.weight"].to(dev).half().contiguous(memory_format=cl), sd[f"block{b}.projection.bias"].to(dev).half()))

    @torch.no_grad()
    def run(frames_u8):
        n, h, w, _ = frames_u8.shape
        x = (frames_u8.permute(0, 3, 1, 2).float() - norm).half().contiguous(memory_format=cl)
        acc = None
        for k, (convs, pw, pb) in enumerate(blocks):
            if k:
                x = F.max_pool2d(x, 2, 2)
            for wt, bias in convs:
                x = F.relu(F.conv2d(x, wt, bias, padding=1))
            s = F.interpolate(F.conv2d(x, pw, pb).float(), size=(h, w), mode="bilinear", align_corners=False)
            acc = s if acc is None else acc + s
        level = (torch.sigmoid((acc / 5.0).double()) * 255.0).clamp(0, 255).to(torch.uint8)
        ctrl = (level.float() / 255.0).expand(-1, 3, -1, -1)
        return torch.cat([ctrl] * rep).contiguous(), level[:, 0]

    return run


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--out", default=os.path.join("profiles", "hed_bench.json"))
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    import torch
    from PIL import Image
    from controlanimate_amd import kernels as K
    from controlanimate_amd.annotators import HedAnnotator

    h, w, n, rep = a.height, a.width, a.frames, 2
    if not torch.cuda.is_available():
        raise SystemExit("bench_hed.py measures on the GPU: none found")
    sd = seeded_state_dict(0)
    arrays = [frame(h, w, s) for s in range(n)]
    frames = [Image.fromarray(x) for x in arrays]
    ann = HedAnnotator(sd, "cuda", detect_resolution=min(h, w), image_resolution=min(h, w))
    t_in = torch.from_numpy(np.stack(arrays)).cuda()
    K._plan_sink = plans = []
    out = ann.annotate_batch(t_in, rep=rep, dtype=torch.float32)  # warm-up: allocations, module load
    K._plan_sink = None
    ann.annotate_batch(frames, out=out, rep=rep)
    torch.cuda.synchronize()
    if a.once:
        ann.annotate_batch(t_in, out=out, rep=rep)
        torch.cuda.synchronize()
        return

    tensor_ms = _timed(lambda: ann.annotate_batch(t_in, out=out, rep=rep), a.runs)
    pil_ms = _timed(lambda: ann.annotate_batch(frames, out=out, rep=rep), a.runs)
    ann.timings = {}
    _timed(lambda: ann.annotate_batch(t_in, out=out, rep=rep), a.runs)
    timings, ann.timings = ann.timings, None
    px = n * h * w
    shapes = conv_shapes(h, w)
    per_call = {"prep": 1, "conv": 13, "pool_side": 5, "fuse": 1}
    stages = {}
    for name, evs in timings.items():
        ms = [s.elapsed_time(e) for s, e in evs]
        k = per_call[name]
        each = [[ms[r * k + i] for r in range(len(ms) // k)] for i in range(k)]  # launch i of the stage over the runs
        stages[name] = {"launches": k, "total": _spread([sum(ms[r * k:(r + 1) * k]) for r in range(len(ms) // k)]), "each_median_ms": [round(statistics.median(e), 4) for e in each]}
    conv_flop = [2 * 9 * ci * co * hh * ww * n for ci, co, hh, ww in shapes]
    stages["conv"]["plans"] = plans
    stages["conv"]["shapes"] = [f"{ci}->{co} @ {hh}x{ww}" for ci, co, hh, ww in shapes]
    stages["conv"]["tflop_per_s_each"] = [round(f / (m * 1e-3) / 1e12, 1) for f, m in zip(conv_flop, stages["conv"]["each_median_ms"])]
    stages["conv"]["tflop"] = round(sum(conv_flop) / 1e12, 3)
    stages["prep"]["min_bytes"] = px * (3 + 16)
    pool_bytes = [n * (h >> k) * (w >> k) * (c * 2 + 4 + (c * 2 // 4 if k < 4 else 0)) for k, (_, c, _) in enumerate(HED_BLOCKS)]
    stages["pool_side"]["min_bytes_each"] = pool_bytes
    stages["pool_side"]["gb_per_s_each"] = [round(b / m / 1e6, 1) for b, m in zip(pool_bytes, stages["pool_side"]["each_median_ms"])]
    stages["fuse"]["min_bytes"] = sum(n * (h >> k) * (w >> k) * 4 for k in range(5)) + px * rep * 12
    for name in ("prep", "fuse"):
        stages[name]["gb_per_s"] = round(stages[name]["min_bytes"] / stages[name]["total"]["median_ms"] / 1e6, 1)
    kernels_ms = sum(s["total"]["median_ms"] for s in stages.values())
    result = {
        "frames": n, "size": f"{h}x{w}", "rep": rep, "dtype": "float16", "control_dtype": "float32", "device": torch.cuda.get_device_name(0),
        "weights": "seeded He-normal (no trained checkpoint: fp16 range on one is unmeasured)",
        "device_from_tensor": _spread(tensor_ms),
        "device_from_pil": _spread(pil_ms),
        "device_kernels_ms": round(kernels_ms, 4),
        "stages": stages,
        "mean_level": round(float(ann.edges(t_in).float().mean()), 2),
    }

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")

    write()
    if not a.no_torch:
        run = torch_chain(sd, torch.device("cuda"), rep)
        t0 = time.perf_counter()
        for _ in range(2):
            want, want_level = run(t_in)
        torch.cuda.synchronize()
        result["torch_chain_warmup_s"] = round(time.perf_counter() - t0, 2)
        torch_ms = _timed(lambda: run(t_in), a.runs)
        again = _timed(lambda: ann.annotate_batch(t_in, out=out, rep=rep), a.runs)  # the project's route once more, after torch's: the spread between windows
        d = (ann.edges(t_in).int() - want_level.int()).abs()
        result["torch_fp16_channels_last_chain"] = {**_spread(torch_ms), "what": "conv2d + relu, max_pool2d, 1x1 conv2d, interpolate(bilinear), mean, sigmoid, cat"}
        result["device_from_tensor_after_torch"] = _spread(again)
        result["torch_over_device_from_tensor"] = round(statistics.median(torch_ms) / statistics.median(tensor_ms + again), 2)
        result["levels_that_differ_from_torch_chain"] = {"share": round(float((d > 0).float().mean()), 4), "max": int(d.max())}
        write()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
