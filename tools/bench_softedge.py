"""Times the softedge control images of one 16-frame window of 512x768 RGB frames: annotators.SoftedgeAnnotator.annotate_batch(rep=2)
from a uint8 device tensor and from PIL frames, each stage of the chain from events around it, the three full-resolution blocks as
ca_pdc_block against their two-launch form (ca_dwconv_k + ca_gemm with the skip as residual), and -- in the same run, on the same
seeded weights and frames -- the same network as a torch fp16 channels_last chain on the GPU (the difference operators folded the same
way; conv2d, relu, max_pool2d, interpolate, sigmoid).

    python tools/bench_softedge.py [--frames 16] [--runs 10] [--out profiles/softedge_bench.json] [--no-torch] [--once]

Warm: two calls of every route before its timed window.  Every figure is median and [min, max] over --runs calls, a host clock around
work that ends in a device synchronise; the per-stage and per-kernel figures are device events.  Beside them: the achieved bytes per
second of ca_pdc_block and ca_dwconv_k against their least traffic (input read once, output written once) next to the plain-copy rate
DESIGN.md section 16 records (5.2 TB/s).  The weights are seeded as in tests/softedge_ref.py (no trained checkpoint is available).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
COPY_TB_PER_S = 5.2


def frame(h: int, w: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.zeros((h, w, 3), np.float64)
    a[..., 0] = 128 + 100 * np.sin(xx / (9.0 + seed)) * np.cos(yy / 13.0)
    a[..., 1] = (xx * 2 + yy * (3 + seed)) % 256
    a[..., 2] = 255 * ((xx // 32 + yy // 32 + seed) % 2)
    a += rng.normal(0, 12, a.shape)
    return a.clip(0, 255).astype(np.uint8)


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


def torch_chain(sd, dev):
    """The same network (difference operators folded, fp16, channels_last) as torch ops on the device: frames uint8 [n, H, W, 3] ->
    the uint8 map [n, H, W]; no host read."""
    import torch
    import torch.nn.functional as F
    from controlanimate_amd.softedge import folded_layers
    cl = torch.channels_last
    f = folded_layers(sd)

    def w4(t):
        return t.to(dev).half().contiguous(memory_format=cl)

    def b1(t):
        return t.to(dev).half()

    init = w4(f["init"])
    blks = [{"dw": w4(b["dw"]), "pw": w4(b["pw"]), "shortcut": (w4(b["shortcut"][0]), b1(b["shortcut"][1])) if "shortcut" in b else None} for b in f["blocks"]]
    levels = [{"cdcm1": (w4(lv["cdcm1"][0]), b1(lv["cdcm1"][1])), "cdcm2": [w4(t) for t in lv["cdcm2"]], "csam1": (w4(lv["csam1"][0]), b1(lv["csam1"][1])),
               "csam2": w4(lv["csam2"]), "reduce": (w4(lv["reduce"][0]), b1(lv["reduce"][1]))} for lv in f["levels"]]
    cls = (f["classifier"][0].to(dev), f["classifier"][1].to(dev))

    @torch.no_grad()
    def run(frames_u8):
        h, w = frames_u8.shape[1:3]
        x = (frames_u8.permute(0, 3, 1, 2).float() / 255.0).half().contiguous(memory_format=cl)
        x = F.conv2d(x, init, padding=1)
        feats = []
        for blk in blks:
            if blk["shortcut"] is not None:
                feats.append(x)
                x = F.max_pool2d(x, 2, 2)
            k = blk["dw"].shape[-1]
            y = F.conv2d(F.relu(F.conv2d(x, blk["dw"], padding=k // 2, groups=x.shape[1])), blk["pw"])
            x = y + (F.conv2d(x, *blk["shortcut"]) if blk["shortcut"] is not None else x)
        feats.append(x)
        sides = []
        for lv, ft in zip(levels, feats):
            t = F.conv2d(F.relu(ft), *lv["cdcm1"])
            t = sum(F.conv2d(t, wd, padding=d, dilation=d) for wd, d in zip(lv["cdcm2"], (5, 7, 9, 11)))
            a = torch.sigmoid(F.conv2d(F.conv2d(F.relu(t), *lv["csam1"]), lv["csam2"], padding=1))
            s = F.conv2d(t * a, *lv["reduce"]).float()
            sides.append(F.interpolate(s, (h, w), mode="bilinear", align_corners=False))
        edge = torch.sigmoid(F.conv2d(torch.cat(sides, dim=1), *cls))[:, 0]
        return (edge * 255.0).clamp(0, 255).to(torch.uint8)

    return run


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--out", default=os.path.join("profiles", "softedge_bench.json"))
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    import torch
    from PIL import Image
    import softedge_ref
    from controlanimate_amd import kernels as K
    from controlanimate_amd.annotators import SoftedgeAnnotator
    from controlanimate_amd.context import dispatch
    from controlanimate_amd.softedge import stages as stage_counts

    h, w, n, rep = a.height, a.width, a.frames, 2
    if not torch.cuda.is_available():
        raise SystemExit("bench_softedge.py measures on the GPU: none found")
    sd = softedge_ref.softedge_state_dict(0)
    arrays = [frame(h, w, s) for s in range(n)]
    frames = [Image.fromarray(x) for x in arrays]
    default_fused = bool(dispatch.pdc_block_fused)
    ann = SoftedgeAnnotator(sd, "cuda")
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
    stages = _stage_table(timings, stage_counts(default_fused))
    kernels_ms = sum(s["total"]["median_ms"] for s in stages.values())
    edges = ann.edges(t_in)
    result = {
        "frames": n, "size": f"{h}x{w}", "rep": rep, "dtype": "float16", "control_dtype": "float32", "device": torch.cuda.get_device_name(0),
        "weights": "seeded (no trained checkpoint)", "default_pdc_block_fused": default_fused,
        "device_from_tensor": _spread(tensor_ms),
        "device_from_pil": _spread(pil_ms),
        "device_stages_ms": round(kernels_ms, 4),
        "stages": stages,
        "all_plans": plans,  # ca_conv3x3 / ca_gemm kernel labels of one pass, in launch order
        "map_mean": round(float(edges.float().mean()), 2), "map_levels": int(edges.unique().numel()),
    }

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")

    write()
    # the whole chain under the other dispatch, same run
    other = SoftedgeAnnotator(sd, "cuda")
    try:
        dispatch.pdc_block_fused = not default_fused
        for _ in range(2):
            other.annotate_batch(t_in, out=out, rep=rep)
        other_ms = _timed(lambda: other.annotate_batch(t_in, out=out, rep=rep), a.runs)
    finally:
        dispatch.pdc_block_fused = default_fused
    again_ms = _timed(lambda: ann.annotate_batch(t_in, out=out, rep=rep), a.runs)
    fused_ms, two_ms = (tensor_ms + again_ms, other_ms) if default_fused else (other_ms, tensor_ms + again_ms)
    result["chain_pdc_block_fused"] = _spread(fused_ms)
    result["chain_two_launch"] = _spread(two_ms)
    result["chain_two_launch_over_fused"] = round(statistics.median(two_ms) / statistics.median(fused_ms), 3)
    del other
    # the three full-resolution blocks alone: ad and cv are 3x3, rd is 5x5
    wts = ann._weights(torch.device("cuda"))
    x = (torch.randn((n, h, w, 64), device="cuda") * 0.7).half()
    y, tmp = torch.empty_like(x), torch.empty_like(x)
    nbytes = 2 * x.numel() * 2
    blocks = {}
    for name, blk in zip(("block1_1 ad 3x3", "block1_2 rd 5x5", "block1_3 cv 3x3"), wts["blocks"][:3]):
        for _ in range(2):
            K.pdc_block(x, blk["dw"], blk["pw"], out=y, fused=True)
            K.pdc_block(x, blk["dw"], blk["pw"], out=y, fused=False, tmp=tmp)
        f_ms = _events(lambda: K.pdc_block(x, blk["dw"], blk["pw"], out=y, fused=True), a.runs)
        t_ms = _events(lambda: K.pdc_block(x, blk["dw"], blk["pw"], out=y, fused=False, tmp=tmp), a.runs)
        d_ms = _events(lambda: K.dwconv_k(x, blk["dw"], relu=True, out=tmp), a.runs)
        blocks[name] = {"ca_pdc_block": _spread(f_ms), "two_launches": _spread(t_ms), "ca_dwconv_k_alone": _spread(d_ms),
                        "two_over_fused": round(statistics.median(t_ms) / statistics.median(f_ms), 3),
                        "least_bytes": nbytes, "ca_pdc_block_tb_per_s": round(nbytes / statistics.median(f_ms) / 1e9, 2),
                        "ca_dwconv_k_tb_per_s": round(nbytes / statistics.median(d_ms) / 1e9, 2)}
    copy_ms = _events(lambda: y.copy_(x), a.runs)
    result["full_resolution_blocks"] = blocks
    result["full_resolution_blocks_sum"] = {"ca_pdc_block_ms": round(sum(b["ca_pdc_block"]["median_ms"] for b in blocks.values()), 4),
                                            "two_launches_ms": round(sum(b["two_launches"]["median_ms"] for b in blocks.values()), 4)}
    result["plain_copy"] = {"recorded_tb_per_s": COPY_TB_PER_S, "this_run_tb_per_s": round(nbytes / statistics.median(copy_ms) / 1e9, 2), "bytes": nbytes}
    del x, y, tmp
    write()
    if not a.no_torch:
        run = torch_chain(sd, torch.device("cuda"))
        t0 = time.perf_counter()
        for _ in range(2):
            m = run(t_in)
        torch.cuda.synchronize()
        result["torch_chain_warmup_s"] = round(time.perf_counter() - t0, 2)
        torch_ms = _timed(lambda: run(t_in), a.runs)
        again = _timed(lambda: ann.annotate_batch(t_in, out=out, rep=rep), a.runs)  # the project's route once more, after torch's
        result["torch_fp16_channels_last_network"] = {**_spread(torch_ms), "what": "conv2d, relu, max_pool2d, interpolate, sigmoid; no control tensor"}
        result["device_from_tensor_after_torch"] = _spread(again)
        result["torch_over_device_from_tensor"] = round(statistics.median(torch_ms) / statistics.median(tensor_ms + again), 2)
        result["torch_map_differs_by_more_than_2_levels"] = round(float(((m.int() - edges.int()).abs() > 2).float().mean()), 4)
        write()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
