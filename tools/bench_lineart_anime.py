"""Times the lineart_anime control images of one 16-frame window of 512x768 RGB frames:
annotators.LineartAnimeAnnotator.annotate_batch(rep=2) from a uint8 device tensor and from PIL frames, each stage of the chain from
events around it, and -- in the same run, on the same seeded weights and frames -- the same network as a torch fp16 channels_last
chain on the GPU (conv2d, leaky_relu, instance_norm, relu, cat, conv_transpose2d, tanh, truncation, three channels, torch.cat for the
CFG halves), whole and per stage.  For each level of the two MFMA kernels (ca_conv4x4s2, ca_convt4x4s2) it also times ca_conv3x3 on a
shape of equal work: the same plane, input and output channels, and 16 / 9 as many frames (rounded), so that both run the same
number of multiply-adds to within a frame; the figures beside each other are TFLOP/s.

    python tools/bench_lineart_anime.py [--frames 16] [--runs 10] [--out profiles/lineart_anime_bench.json] [--no-torch] [--once]

Warm: two calls of every route before its timed window.  Every figure is median and [min, max] over --runs calls, a host clock around
work that ends in a device synchronise; the per-stage figures are device events (a stage's events enclose its launches: an
InstanceNorm of more than one chunk of pixels is two).  FLOPs are computed from the shapes.  The weights are seeded He-normal as in
tests/lineart_anime_ref.py, with small random biases: no trained checkpoint is available.  The result is written after the project's
own figures and again after torch's, so a torch chain that takes long to pick its algorithms does not lose the first half.
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

from bench_lineart import _spread, _stage_table, _timed, frame  # noqa: E402


def seeded_state_dict(seed: int = 0) -> dict:
    import torch
    from controlanimate_amd.lineart_anime import lineart_anime_key_shapes
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in lineart_anime_key_shapes().items():
        if k.endswith(".weight"):
            transposed = k.endswith((".model.3.weight", ".model.5.weight"))
            fan_in = shape[0] * 4 if transposed else shape[1] * 16
            sd[k] = torch.randn(shape, generator=g) * math.sqrt(2.0 / fan_in)
        else:
            sd[k] = torch.randn(shape, generator=g) * 0.02
    return sd


def levels(h: int, w: int):
    """(h_i, w_i, c_i) of level i = 0 .. 7."""
    from controlanimate_amd.lineart_anime import CHANNELS
    return [(h >> (i + 1), w >> (i + 1), c) for i, c in enumerate(CHANNELS)]


def stage_flop(n: int, h: int, w: int) -> dict:
    """FLOPs of the stages of each name, in launch order (2 per multiply-add, padding taps counted)."""
    lv = levels(h, w)
    conv = [2 * 16 * lv[i - 1][2] * lv[i][2] * lv[i][0] * lv[i][1] * n for i in range(1, 8)]
    # up_i reads level i (K = 2 c_i, the innermost c_7) and writes c_{i-1} channels at level i - 1: 4 taps per output pixel
    convt = [2 * 4 * (lv[i][2] if i == 7 else 2 * lv[i][2]) * lv[i - 1][2] * lv[i - 1][0] * lv[i - 1][1] * n for i in range(7, 0, -1)]
    return {"conv_in": [2 * 48 * 64 * lv[0][0] * lv[0][1] * n], "conv": conv, "convt": convt, "conv_out": [2 * 4 * 128 * h * w * n]}


def instnorm_bytes(n: int, h: int, w: int) -> list:
    """Least bytes of the thirteen InstanceNorms, in launch order: the input read twice; on the way down two outputs written, on the
    way up one."""
    lv = levels(h, w)
    size = [n * a * b * c * 2 for a, b, c in lv]
    return [4 * size[i] for i in range(1, 7)] + [3 * size[i - 1] for i in range(7, 0, -1)]


def conv3x3_equal_work(n: int, h: int, w: int, runs: int) -> dict:
    """ca_conv3x3 (stride 1) on the plane, input and output channels of every level of the two MFMA kernels, with round(16 n / 9)
    frames: the same work to within a frame.  -> {"conv": [...], "convt": [...]} of {shape, median_ms, tflop_per_s, plan} in the
    stages' launch order; a shape ca_conv3x3 does not take is recorded with its error."""
    import torch
    from controlanimate_amd import kernels as K
    lv = levels(h, w)
    n3 = max(1, round(16 * n / 9))
    shapes = {"conv": [(lv[i][0], lv[i][1], lv[i - 1][2], lv[i][2]) for i in range(1, 8)],
              "convt": [(lv[i][0], lv[i][1], lv[i][2] if i == 7 else 2 * lv[i][2], lv[i - 1][2]) for i in range(7, 0, -1)]}
    out = {}
    g = torch.Generator().manual_seed(1)
    for name, lst in shapes.items():
        out[name] = []
        for (hh, ww, cin, cout) in lst:
            rec = {"shape": [n3, hh, ww, cin, cout]}
            try:
                x = torch.randn((n3, hh, ww, cin), generator=g).half().cuda()
                wt = (torch.randn((cout, 3, 3, cin), generator=g) * math.sqrt(2.0 / (9 * cin))).half().cuda()
                y = torch.empty((n3, hh, ww, cout), dtype=torch.float16, device="cuda")
                K._plan_sink = plans = []
                for _ in range(2):
                    K.conv3x3(x, wt, out=y)
                K._plan_sink = None
                ms = statistics.median(_timed(lambda: K.conv3x3(x, wt, out=y), runs))
                rec.update(median_ms=round(ms, 4), tflop_per_s=round(2 * 9 * cin * cout * hh * ww * n3 / (ms * 1e-3) / 1e12, 1), plan=plans[0] if plans else "?")
            except Exception as e:  # a shape outside ca_conv3x3's ranges
                K._plan_sink = None
                rec["error"] = str(e)[:200]
            out[name].append(rec)
    return out


def conv_forms(ann, n: int, h: int, w: int, runs: int) -> list:
    """Every level of kernels.conv4x4s2 alone in both of its forms, on the annotator's weights: {rows, form (the one the chain takes),
    tile_ms, gemm_ms} per level -- the measurement behind kernels.CONV4X4S2_GEMM_ROWS.  The gather form is skipped where its im2col
    tensor would pass 1 GiB."""
    import torch
    from controlanimate_amd import kernels as K
    lv = levels(h, w)
    wts = ann._weights(torch.device("cuda"))["down"]
    out = []
    for i in range(1, 8):
        x = torch.randn((n, lv[i - 1][0], lv[i - 1][1], lv[i - 1][2]), device="cuda").half()
        rows = n * lv[i][0] * lv[i][1]
        rec = {"level": i, "rows": rows, "form": "gemm" if rows < K.CONV4X4S2_GEMM_ROWS else "tile"}
        for form in ("tile", "gemm"):
            if form == "gemm" and rows * 16 * lv[i - 1][2] * 2 > 1 << 30:
                continue
            for _ in range(2):
                K.conv4x4s2(x, wts[i - 1], form=form)
            rec[form + "_ms"] = round(statistics.median(_timed(lambda: K.conv4x4s2(x, wts[i - 1], form=form), runs)), 4)
        out.append(rec)
    return out


def torch_chain(sd, dev, rep: int):
    """The same network as torch ops in fp16 channels_last on the device: frames uint8 [n, H, W, 3] -> float32 control [rep n, 3, H, W].
    `timings` (a dict, or None) receives events per stage under the annotator's stage names."""
    import torch
    import torch.nn.functional as F
    from controlanimate_amd.lineart_anime import conv_keys
    cl = torch.channels_last

    def wt(k):
        return sd[k + ".weight"].to(dev).half().contiguous(memory_format=cl), sd[k + ".bias"].to(dev).half()

    down = [wt(conv_keys(i)[0]) for i in range(8)]
    up = [wt(conv_keys(i)[1]) for i in range(8)]

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

        x0 = (frames_u8.permute(0, 3, 1, 2).float() / 127.5 - 1.0).half().contiguous(memory_format=cl)
        d = st("conv_in", lambda: F.conv2d(x0, *down[0], stride=2, padding=1))
        skips = [d]
        for i in range(1, 7):
            raw = st("conv", lambda: F.conv2d(F.leaky_relu(skips[-1], 0.2), *down[i], stride=2, padding=1))
            skips.append(st("instnorm", lambda: F.instance_norm(raw, eps=1e-5)))
        x = st("conv", lambda: F.relu(F.conv2d(F.leaky_relu(skips[-1], 0.2), *down[7], stride=2, padding=1)))
        for i in range(7, 0, -1):
            raw = st("convt", lambda: F.conv_transpose2d(x, *up[i], stride=2, padding=1))
            x = st("instnorm", lambda: F.relu(torch.cat([skips[i - 1], F.instance_norm(raw, eps=1e-5)], 1)))
        pre = st("conv_out", lambda: F.conv_transpose2d(x, *up[0], stride=2, padding=1).float())

        def finish():
            level = 255 - (torch.tanh(pre.double()) * 127.5 + 127.5).clamp(0, 255).to(torch.uint8)
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
    ap.add_argument("--out", default=os.path.join("profiles", "lineart_anime_bench.json"))
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    import torch
    from PIL import Image
    from controlanimate_amd.annotators import LineartAnimeAnnotator
    from controlanimate_amd.lineart_anime import STAGES

    h, w, n, rep = a.height, a.width, a.frames, 2
    if not torch.cuda.is_available():
        raise SystemExit("bench_lineart_anime.py measures on the GPU: none found")
    sd = seeded_state_dict(0)
    arrays = [frame(h, w, s) for s in range(n)]
    frames = [Image.fromarray(x) for x in arrays]
    ann = LineartAnimeAnnotator(sd, "cuda")
    t_in = torch.from_numpy(np.stack(arrays)).cuda()
    out = ann.annotate_batch(t_in, rep=rep, dtype=torch.float32)  # warm-up: allocations, module load
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
    nb = instnorm_bytes(n, h, w)
    stages["instnorm"]["min_bytes_each"] = nb
    stages["instnorm"]["gb_per_s_each"] = [round(b / m / 1e6, 1) for b, m in zip(nb, stages["instnorm"]["each_median_ms"])]
    kernels_ms = sum(s["total"]["median_ms"] for s in stages.values() if isinstance(s, dict))
    stages["conv"]["forms"] = conv_forms(ann, n, h, w, a.runs)
    ref3 = conv3x3_equal_work(n, h, w, a.runs)
    for name in ("conv", "convt"):
        stages[name]["ca_conv3x3_equal_work"] = ref3[name]
    result = {
        "frames": n, "size": f"{h}x{w}", "rep": rep, "dtype": "float16", "control_dtype": "float32", "device": torch.cuda.get_device_name(0),
        "weights": "seeded He-normal (no trained checkpoint)",
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
        result["torch_fp16_channels_last_chain"] = {**_spread(torch_ms), "what": "conv2d, leaky_relu, instance_norm, relu, cat, conv_transpose2d, tanh, cat",
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
