"""Times the lineart control images of one 16-frame window of 512x768 RGB frames: annotators.LineartAnnotator.annotate_batch(rep=2)
from a uint8 device tensor and from PIL frames, each stage of the chain from events around it, and -- in the same run, on the same
seeded weights and frames -- the same network as a torch fp16 channels_last chain on the GPU (F.pad(reflect), conv2d, instance_norm,
relu, conv_transpose2d, sigmoid, x 255, truncation, three channels, torch.cat for the CFG halves), whole and per stage.

    python tools/bench_lineart.py [--frames 16] [--runs 10] [--out profiles/lineart_bench.json] [--no-torch] [--once]

Warm: two calls of every route before its timed window.  Every figure is median and [min, max] over --runs calls, a host clock around
work that ends in a device synchronise; the per-stage figures are device events (a stage's events enclose its launches: an
InstanceNorm is two, a transposed convolution a GEMM and a gather).  FLOPs are computed from the shapes.  The weights are seeded
He-normal as in tests/lineart_ref.py, with small random biases: no trained checkpoint is available.  The result is written after the project's own
figures and again after torch's, so a torch chain that takes long to pick its algorithms does not lose the first half.
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


def seeded_state_dict(seed: int = 0, out_scale: float = 3.0) -> dict:
    import torch
    from controlanimate_amd.lineart import lineart_key_shapes
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in lineart_key_shapes().items():
        if k.endswith(".weight"):
            fan_in = (shape[0] if k.startswith("model3.") else shape[1]) * shape[2] * shape[3]
            if k.startswith("model3."):
                fan_in //= 4
            sd[k] = torch.randn(shape, generator=g) * math.sqrt(2.0 / fan_in) * (out_scale if k == "model4.1.weight" else 1.0)
        else:
            sd[k] = torch.randn(shape, generator=g) * 0.02
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


def stage_flop(n: int, h: int, w: int) -> dict:
    """FLOPs of the stages of each name, in order (2 per multiply-add; the convolutions on reflection-padded tensors as the
    network defines them, without the ring)."""
    h2, w2, h4, w4 = h // 2, w // 2, h // 4, w // 4
    return {
        "conv_in": [2 * 147 * 64 * h * w * n],
        "conv": [2 * 9 * 64 * 128 * h2 * w2 * n, 2 * 9 * 128 * 256 * h4 * w4 * n] + [2 * 9 * 256 * 256 * h4 * w4 * n] * 6,
        "convt": [2 * 9 * 256 * 128 * h4 * w4 * n, 2 * 9 * 128 * 64 * h2 * w2 * n],
        "conv_out": [2 * 49 * 64 * h * w * n],
    }


def instnorm_bytes(n: int, h: int, w: int) -> list:
    """Least bytes of the eleven InstanceNorms (the input read twice, the output written once; the residual read where there is one)."""
    e = 2
    full, half, quarter = n * h * w * 64 * e, n * (h // 2) * (w // 2) * 128 * e, n * (h // 4) * (w // 4) * 256 * e
    return [3 * full, 3 * half, 3 * quarter] + [3 * quarter, 4 * quarter] * 3 + [3 * half, 3 * full]


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


def _stage_table(timings: dict, per_call: dict) -> dict:
    stages = {}
    for name, evs in timings.items():
        ms = [s.elapsed_time(e) for s, e in evs]
        k = per_call[name]
        each = [[ms[r * k + i] for r in range(len(ms) // k)] for i in range(k)]  # the i-th stage of that name over the runs
        stages[name] = {"stages": k, "total": _spread([sum(ms[r * k:(r + 1) * k]) for r in range(len(ms) // k)]),
                        "each_median_ms": [round(statistics.median(e), 4) for e in each]}
    return stages


def torch_chain(sd, dev, rep: int):
    """The same network as torch ops in fp16 channels_last on the device: frames uint8 [n, H, W, 3] -> float32 control [rep n, 3, H, W].
    `timings` (a dict, or None) receives events per stage under the annotator's stage names."""
    import torch
    import torch.nn.functional as F
    cl = torch.channels_last

    def wt(k):
        return sd[k + ".weight"].to(dev).half().contiguous(memory_format=cl), sd[k + ".bias"].to(dev).half()

    w_in, w_d0, w_d1, w_u0, w_u1, w_out = wt("model0.1"), wt("model1.0"), wt("model1.3"), wt("model3.0"), wt("model3.3"), wt("model4.1")
    res = [(wt(f"model2.{b}.conv_block.1"), wt(f"model2.{b}.conv_block.5")) for b in range(3)]

    @torch.no_grad()
    def run(frames_u8, timings=None):
        def st(name, fn):
            if timings is None:
                return fn()
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            timings.setdefault(name, []).append(ev)
            ev[0].record()
            out = fn()
            ev[1].record()
            return out

        def inorm(x, relu=True, residual=None):
            def f():
                y = F.instance_norm(x, eps=1e-5)
                if relu:
                    y = F.relu(y)
                return y if residual is None else residual + y
            return st("instnorm", f)

        x0 = (frames_u8.permute(0, 3, 1, 2).float() / 255.0).half().contiguous(memory_format=cl)
        x = st("conv_in", lambda: F.conv2d(F.pad(x0, (3, 3, 3, 3), mode="reflect"), *w_in))
        x = inorm(x)
        for w in (w_d0, w_d1):
            x = inorm(st("conv", lambda: F.conv2d(x, *w, stride=2, padding=1)))
        for (a, b) in res:
            y = inorm(st("conv", lambda: F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), *a)))
            x = inorm(st("conv", lambda: F.conv2d(F.pad(y, (1, 1, 1, 1), mode="reflect"), *b)), relu=False, residual=x)
        for w in (w_u0, w_u1):
            x = inorm(st("convt", lambda: F.conv_transpose2d(x, *w, stride=2, padding=1, output_padding=1)))
        logit = st("conv_out", lambda: F.conv2d(F.pad(x, (3, 3, 3, 3), mode="reflect"), *w_out).float())

        def finish():
            level = 255 - (torch.sigmoid(logit.double()) * 255.0).clamp(0, 255).to(torch.uint8)
            ctrl = (level.float() / 255.0).expand(-1, 3, -1, -1)
            return torch.cat([ctrl] * rep).contiguous(), level[:, 0]
        return st("finish", finish)

    return run


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--out", default=os.path.join("profiles", "lineart_bench.json"))
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    import torch
    from PIL import Image
    from controlanimate_amd import kernels as K
    from controlanimate_amd.annotators import LineartAnnotator
    from controlanimate_amd.lineart import STAGES

    h, w, n, rep = a.height, a.width, a.frames, 2
    if not torch.cuda.is_available():
        raise SystemExit("bench_lineart.py measures on the GPU: none found")
    sd = seeded_state_dict(0)
    arrays = [frame(h, w, s) for s in range(n)]
    frames = [Image.fromarray(x) for x in arrays]
    ann = LineartAnnotator(sd, "cuda")
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
    stages = _stage_table(timings, STAGES)
    flop = stage_flop(n, h, w)
    for name, fl in flop.items():
        stages[name]["tflop_per_s_each"] = [round(f / (m * 1e-3) / 1e12, 1) for f, m in zip(fl, stages[name]["each_median_ms"])]
        stages[name]["tflop"] = round(sum(fl) / 1e12, 3)
    stages["all_plans"] = plans  # ca_conv3x3 / ca_gemm kernel labels of one pass, in launch order
    nb = instnorm_bytes(n, h, w)
    stages["instnorm"]["min_bytes_each"] = nb
    stages["instnorm"]["gb_per_s_each"] = [round(b / m / 1e6, 1) for b, m in zip(nb, stages["instnorm"]["each_median_ms"])]
    kernels_ms = sum(s["total"]["median_ms"] for s in stages.values() if isinstance(s, dict))
    result = {
        "frames": n, "size": f"{h}x{w}", "rep": rep, "dtype": "float16", "control_dtype": "float32", "device": torch.cuda.get_device_name(0),
        "weights": "seeded He-normal (no trained checkpoint)",
        "transposed_convolution": "one GEMM with N = 9 * Cout + a gather per output phase (the only form built)",
        "device_from_tensor": _spread(tensor_ms),
        "device_from_pil": _spread(pil_ms),
        "device_stages_ms": round(kernels_ms, 4),
        "tflop_per_window": round(sum(sum(v) for v in flop.values()) / 1e12, 3),
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
        tt = {}
        _timed(lambda: run(t_in, tt), a.runs)
        again = _timed(lambda: ann.annotate_batch(t_in, out=out, rep=rep), a.runs)  # the project's route once more, after torch's: the spread between windows
        d = (ann.edges(t_in).int() - want_level.int()).abs()
        result["torch_fp16_channels_last_chain"] = {**_spread(torch_ms), "what": "pad(reflect), conv2d, instance_norm, relu, conv_transpose2d, sigmoid, cat",
                                                    "stages": _stage_table(tt, STAGES)}
        result["device_from_tensor_after_torch"] = _spread(again)
        result["torch_over_device_from_tensor"] = round(statistics.median(torch_ms) / statistics.median(tensor_ms + again), 2)
        result["torch_over_device_per_stage"] = {k: round(result["torch_fp16_channels_last_chain"]["stages"][k]["total"]["median_ms"] / stages[k]["total"]["median_ms"], 2)
                                                 for k in STAGES}
        result["levels_that_differ_from_torch_chain"] = {"share": round(float((d > 0).float().mean()), 4), "share_above_1": round(float((d > 1).float().mean()), 4), "max": int(d.max())}
        write()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
