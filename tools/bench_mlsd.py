"""Times the M-LSD control images of one 16-frame window of 512x768 RGB frames: annotators.MlsdAnnotator.annotate_batch(rep=2) from a
uint8 device tensor and from PIL frames, each stage of the chain from events around it, and -- in the same run, on the same seeded
weights and frames -- the same network plus decode as a torch fp16 channels_last chain on the GPU (BatchNorm folded the same way;
conv2d, relu6 / relu, interpolate(align_corners), cat, sigmoid, max_pool2d, topk, the distance test; no drawing: torch has none).

    python tools/bench_mlsd.py [--frames 16] [--runs 10] [--out profiles/mlsd_bench.json] [--no-torch] [--once]

Warm: two calls of every route before its timed window.  Every figure is median and [min, max] over --runs calls, a host clock around
work that ends in a device synchronise; the per-stage figures are device events.  Beside them: the depthwise kernel's achieved bytes
per second (input read once, output written once) next to the plain-copy rate DESIGN.md section 7 records (5.2 TB/s), and the dilated
convolution's TFLOP/s next to ca_conv3x3's on 64 -> 64 channels at the same size.  The weights are seeded as in tests/mlsd_ref.py (no
trained checkpoint is available); the last layer is scaled so that a few dozen lines per frame come out.
--once: one warm device call and nothing else (for a kernel trace)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_TB_PER_S = 5.2


def seeded_state_dict(seed: int = 0, out_scale: float = 0.3) -> dict:
    import torch
    from controlanimate_amd.mlsd import mlsd_key_shapes
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in mlsd_key_shapes().items():
        if len(shape) == 4:
            sd[k] = torch.randn(shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5 * (out_scale if k == "block23.conv3.weight" else 1.0)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(shape, generator=g)
        elif k.endswith("running_mean"):
            sd[k] = torch.randn(shape, generator=g) * 0.1
        elif k.endswith(".weight"):
            sd[k] = 0.7 + 0.6 * torch.rand(shape, generator=g)
        else:
            sd[k] = torch.randn(shape, generator=g) * 0.1
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


def depthwise_bytes(n: int, h: int, w: int) -> list:
    """Least bytes of the thirteen depthwise convolutions, in order: the input read once, the output written once (fp16)."""
    from controlanimate_amd.mlsd import backbone_blocks
    out, hh, ww = [], h // 2, w // 2
    for _, _, hid, _, stride, _, _ in backbone_blocks():
        out.append(2 * n * hid * (hh * ww + (hh // stride) * (ww // stride)))
        hh, ww = hh // stride, ww // stride
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


def _events(fn, runs: int):
    import torch
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def _stage_table(timings: dict, per_call: dict) -> dict:
    stages = {}
    for name, evs in timings.items():
        ms = [s.elapsed_time(e) for s, e in evs]
        k = per_call[name]
        each = [[ms[r * k + i] for r in range(len(ms) // k)] for i in range(k)]
        stages[name] = {"stages": k, "total": _spread([sum(ms[r * k:(r + 1) * k]) for r in range(len(ms) // k)]),
                        "each_median_ms": [round(statistics.median(e), 4) for e in each]}
    return stages


def torch_chain(sd, dev, thr_v: float = 0.1, thr_d: float = 0.1):
    """The same network (BatchNorm folded, fp16, channels_last) and decode as torch ops on the device: frames uint8 [n, H, W, 3] ->
    (segments float [n, 200, 4], live mask [n, 200]); no host read."""
    import torch
    import torch.nn.functional as F
    from controlanimate_amd.mlsd import backbone_blocks, folded_layers
    cl = torch.channels_last
    f = folded_layers(sd)

    def wb(p):
        return p[0].to(dev).half().contiguous(memory_format=cl), p[1].to(dev).half()

    stem = wb(f["stem"])
    feats = [{k: wb(v) for k, v in blk.items()} for blk in f["features"]]
    blocks_a, blocks_b = [(wb(a), wb(b)) for a, b in f["A"]], [(wb(a), wb(b)) for a, b in f["B"]]
    c1, c2 = wb(f["C"][0]), wb(f["C"][1])
    head = wb((f["C"][2][0][7:12], f["C"][2][1][7:12]))
    meta = backbone_blocks()

    @torch.no_grad()
    def run(frames_u8):
        n = frames_u8.shape[0]
        x = torch.cat([frames_u8, torch.ones_like(frames_u8[..., :1])], dim=3).permute(0, 3, 1, 2).float() / 127.5 - 1.0
        x = x.half().contiguous(memory_format=cl)
        x = F.relu6(F.conv2d(F.pad(x, (0, 1, 0, 1)), *stem, stride=2))
        taps = {}
        for (idx, _, hid, _, stride, expands, skips), blk in zip(meta, feats):
            t = F.relu6(F.conv2d(x, *blk["expand"])) if expands else x
            t = F.relu6(F.conv2d(F.pad(t, (0, 1, 0, 1)) if stride == 2 else t, *blk["dw"], stride=stride, padding=0 if stride == 2 else 1, groups=hid))
            y = F.conv2d(t, *blk["project"])
            x = y + x if skips else y
            if idx in (1, 3, 6, 10, 13):
                taps[idx] = x
        x = taps[13]
        for level, (a, up) in enumerate(((taps[10], False), (taps[6], True), (taps[3], True), (taps[1], True))):
            (w1, w2), (b1, b2) = blocks_a[level], blocks_b[level]
            b = F.relu(F.conv2d(x, *w1))
            if up:
                b = F.interpolate(b, scale_factor=2.0, mode="bilinear", align_corners=True)
            cat = torch.cat((F.relu(F.conv2d(a, *w2)), b), dim=1)
            x = F.relu(F.conv2d(F.relu(F.conv2d(cat, *b1, padding=1)) + cat, *b2, padding=1))
        x = F.relu(F.conv2d(F.relu(F.conv2d(x, *c1, padding=5, dilation=5)), *c2, padding=1))
        tp = F.conv2d(x, *head).float()
        hh, ww = tp.shape[2], tp.shape[3]
        heat = torch.sigmoid(tp[:, :1])
        heat = (heat * (F.max_pool2d(heat, 3, stride=1, padding=1) == heat)).reshape(n, -1)
        scores, idx = torch.topk(heat, 200, dim=1)
        disp = tp[:, 1:5].reshape(n, 4, -1).gather(2, idx[:, None].expand(-1, 4, -1))
        yy, xx = torch.div(idx, ww, rounding_mode="floor"), idx % ww
        live = (scores > thr_v) & (torch.sqrt((disp[:, 0] - disp[:, 2]) ** 2 + (disp[:, 1] - disp[:, 3]) ** 2) > thr_d)
        seg = 2 * torch.stack([xx + disp[:, 0], yy + disp[:, 1], xx + disp[:, 2], yy + disp[:, 3]], dim=2)
        return seg, live

    return run


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--out", default=os.path.join("profiles", "mlsd_bench.json"))
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    import torch
    from PIL import Image
    from controlanimate_amd import kernels as K
    from controlanimate_amd.annotators import MlsdAnnotator
    from controlanimate_amd.mlsd import STAGES

    h, w, n, rep = a.height, a.width, a.frames, 2
    if not torch.cuda.is_available():
        raise SystemExit("bench_mlsd.py measures on the GPU: none found")
    sd = seeded_state_dict(0)
    arrays = [frame(h, w, s) for s in range(n)]
    frames = [Image.fromarray(x) for x in arrays]
    ann = MlsdAnnotator(sd, "cuda", detect_resolution=min(h, w), image_resolution=min(h, w))
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
    nb = depthwise_bytes(n, h, w)
    stages["depthwise"]["min_bytes_each"] = nb
    stages["depthwise"]["tb_per_s_each"] = [round(b / m / 1e9, 2) for b, m in zip(nb, stages["depthwise"]["each_median_ms"])]
    stages["depthwise"]["tb_per_s_all"] = round(sum(nb) / stages["depthwise"]["total"]["median_ms"] / 1e9, 2)
    stages["depthwise"]["plain_copy_tb_per_s"] = COPY_TB_PER_S
    # the dilated convolution next to ca_conv3x3 on 64 -> 64 channels at the same size
    x = torch.randn((n, h // 2, w // 2, 64), device="cuda").half()
    wt = (torch.randn((64, 3, 3, 64), device="cuda") * 0.06).half()
    bias = torch.zeros(64, device="cuda")
    y = torch.empty_like(x)
    for _ in range(2):
        K.conv3x3_dil(x, wt, bias, relu=True, out=y)
        K.conv3x3(x, wt, bias=bias, act=K.ACT_RELU, out=y)
    flop = 2 * 9 * 64 * 64 * n * (h // 2) * (w // 2)
    dil_ms = statistics.median(_events(lambda: K.conv3x3_dil(x, wt, bias, relu=True, out=y), a.runs))
    plain_ms = statistics.median(_events(lambda: K.conv3x3(x, wt, bias=bias, act=K.ACT_RELU, out=y), a.runs))
    seg_count = ann.workspace(n, h, w)["count"].tolist()
    kernels_ms = sum(s["total"]["median_ms"] for s in stages.values())
    result = {
        "frames": n, "size": f"{h}x{w}", "rep": rep, "dtype": "float16", "control_dtype": "float32", "device": torch.cuda.get_device_name(0),
        "weights": "seeded (no trained checkpoint)",
        "device_from_tensor": _spread(tensor_ms),
        "device_from_pil": _spread(pil_ms),
        "device_stages_ms": round(kernels_ms, 4),
        "device_network_and_decode_ms": round(kernels_ms - stages["draw"]["total"]["median_ms"], 4),
        "stages": stages,
        "all_plans": plans,  # ca_conv3x3 / ca_gemm kernel labels of one pass, in launch order
        "dilated_vs_conv3x3_64_to_64": {"size": f"{n}x{h // 2}x{w // 2}", "gflop": round(flop / 1e9, 2), "ca_conv3x3_dil_ms": round(dil_ms, 4),
                                        "ca_conv3x3_dil_tflop_per_s": round(flop / dil_ms / 1e9, 1), "ca_conv3x3_ms": round(plain_ms, 4),
                                        "ca_conv3x3_tflop_per_s": round(flop / plain_ms / 1e9, 1)},
        "segments_per_frame": seg_count,
        "share_of_line_pixels": round(float((ann.edges(t_in) == 255).float().mean()), 4),
    }

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")

    write()
    if not a.no_torch:
        run = torch_chain(sd, torch.device("cuda"))
        t0 = time.perf_counter()
        for _ in range(2):
            seg, live = run(t_in)
        torch.cuda.synchronize()
        result["torch_chain_warmup_s"] = round(time.perf_counter() - t0, 2)
        torch_ms = _timed(lambda: run(t_in), a.runs)
        again = _timed(lambda: ann.annotate_batch(t_in, out=out, rep=rep), a.runs)  # the project's route once more, after torch's
        result["torch_fp16_channels_last_network_and_decode"] = {**_spread(torch_ms), "what": "conv2d, relu6, relu, interpolate, cat, sigmoid, max_pool2d, topk"}
        result["device_from_tensor_after_torch"] = _spread(again)
        result["torch_over_device_from_tensor"] = round(statistics.median(torch_ms) / statistics.median(tensor_ms + again), 2)
        result["torch_segments_per_frame"] = live.sum(dim=1).tolist()
        write()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
