"""Times the normalbae control images of one 16-frame window of 512x768 RGB frames, on seeded B5-shaped weights in fp16, in one process:
annotators.NormalBaeAnnotator.annotate_batch(rep=2) from a uint8 device tensor and from PIL frames, each stage of the chain from events
around its launches, ca_dwconv_same's moved bytes per second beside a plain device copy of as many bytes, each refinement stage on its
own as ca_nbae_refine (one launch) against the composed form (upsample, cat_pred, four GEMMs, normalize) with the bytes the latter's
intermediate planes write and read, the whole window under either setting of context.dispatch.nbae_refine_fused, and -- in
the same run, on the same weights and frames -- the specification (tests/normalbae_ref.py) as a torch fp16 channels_last chain.

    python tools/bench_normalbae.py [--frames 16] [--runs 10] [--out profiles/normalbae_bench.json] [--no-torch]

Warm: two calls of every route before its timed window.  Every figure is median and [min, max] over --runs calls, a host clock around
work that ends in a device synchronise; the per-stage figures are device events.  The weights are tests/normalbae_ref.seeded_state_dict:
no trained checkpoint is available.  The result is written after the project's own figures and again after torch's."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_lineart import _spread, _timed, frame  # noqa: E402


def _stage_totals(timings: dict, runs: int) -> dict:
    out = {}
    for name, evs in timings.items():
        ms = [s.elapsed_time(e) for s, e in evs]
        k = len(ms) // runs
        out[name] = {"launches": k, "total": _spread([sum(ms[r * k:(r + 1) * k]) for r in range(runs)])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normalbae_bench.json"))
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    import torch
    from PIL import Image
    import normalbae_ref as R
    from controlanimate_amd import kernels as K
    from controlanimate_amd import normalbae as nb

    dev = torch.device("cuda:0")
    n, h, w = a.frames, a.height, a.width
    sd = {k: v.half().float() for k, v in R.seeded_state_dict(R.B5, 0).items()}
    ann = nb.NormalBaeAnnotator(sd, device=dev, dtype=torch.float16, detect_resolution=min(h, w))
    frames = np.stack([frame(h, w, i) for i in range(n)])
    dev_frames = torch.from_numpy(frames).to(dev)
    pil = [Image.fromarray(f) for f in frames]
    out = torch.empty((2 * n, 3, h, w), dtype=torch.float16, device=dev)
    res = {"frames": n, "height": h, "width": w, "dtype": "float16", "runs": a.runs, "device": torch.cuda.get_device_name(0),
           "refine_default": "fused (ca_nbae_refine)" if __import__("controlanimate_amd.context", fromlist=["dispatch"]).dispatch.nbae_refine_fused else "composed",
           "passes": -(-n // ann.chunk_frames(h, w))}
    for _ in range(2):
        ann.annotate_batch(dev_frames, out=out, rep=2)
    res["annotate_batch_device"] = _spread(_timed(lambda: ann.annotate_batch(dev_frames, out=out, rep=2), a.runs))
    for _ in range(2):
        ann.annotate_batch(pil, out=out, rep=2)
    res["annotate_batch_pil"] = _spread(_timed(lambda: ann.annotate_batch(pil, out=out, rep=2), a.runs))
    ann.timings = {}
    for _ in range(a.runs):
        ann.annotate_batch(dev_frames, out=out, rep=2)
    torch.cuda.synchronize()
    timed, ann.timings = ann.timings, None
    res["stages"] = _stage_totals(timed, a.runs)
    print(json.dumps({k: res[k] for k in ("annotate_batch_device", "annotate_batch_pil", "stages")}), flush=True)

    # ---- ca_dwconv_same beside a plain copy: the widest depthwise layers of a window
    res["dwconv_same"] = []
    for (hh, ww, c, ks, stride) in ((h // 2, w // 2, 144, 3, 2), (h // 4, w // 4, 240, 5, 2), (h // 16, w // 16, 1056, 5, 1), (h // 32, w // 32, 3072, 3, 1)):
        x = torch.randn((n, hh, ww, c), device=dev).half()
        wt = (torch.randn((ks * ks, c), device=dev) * 0.3).half()
        bias = torch.zeros(c, device=dev)
        y, sums = K.dwconv_same(x, wt, bias, stride=stride)
        partials = torch.empty(K.dwconv_same_partials_floats(n, hh, ww, c, stride), dtype=torch.float32, device=dev)
        moved = (x.numel() + y.numel()) * 2
        src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        for _ in range(2):
            K.dwconv_same(x, wt, bias, stride=stride, out=y, sums=sums, partials=partials)
            dst.copy_(src)
        t_dw = _timed(lambda: K.dwconv_same(x, wt, bias, stride=stride, out=y, sums=sums, partials=partials), a.runs)
        t_cp = _timed(lambda: dst.copy_(src), a.runs)
        res["dwconv_same"].append({"plane": [hh, ww], "c": c, "ksize": ks, "stride": stride, "moved_bytes": moved, "dwconv": _spread(t_dw), "copy": _spread(t_cp),
                                   "dwconv_GBps": round(moved / statistics.median(t_dw) / 1e6, 1), "copy_GBps": round(moved / statistics.median(t_cp) / 1e6, 1)})
    print(json.dumps(res["dwconv_same"]), flush=True)

    # ---- the refinement stages on their own: the composed form against ca_nbae_refine (the composed form is forced through the switch)
    from controlanimate_amd.context import dispatch
    default_fused, dispatch.nbae_refine_fused = dispatch.nbae_refine_fused, False
    res["refine"] = []
    m = min(n, ann.chunk_frames(h, w))
    wts = ann._weights(dev)
    for level, (div, c) in enumerate(((8, 512), (4, 256), (2, 128))):
        feat = torch.randn((m, h // div, w // div, c), device=dev).half()
        pred = torch.nn.functional.normalize(torch.randn((m, h // div, w // div, 4), device=dev), dim=3)
        px = m * (2 * h // div) * (2 * w // div)
        bufs = {}

        def take(*shape):
            key = (shape, sum(1 for k in bufs if k[0] == shape and bufs[k][1]))
            if key not in bufs:
                bufs[key] = [torch.empty(shape, dtype=torch.float16, device=dev), False]
            bufs[key][1] = True
            return bufs[key][0]

        def give(t):
            for v in bufs.values():
                if v[0].data_ptr() == t.data_ptr():
                    v[1] = False

        o = torch.empty((m, 2 * h // div, 2 * w // div, 4), dtype=torch.float32, device=dev)
        raw = torch.empty(px * 8, dtype=torch.float32, device=dev)
        run = lambda: nb.refine_stage(feat, pred, wts["mlp"][level], out=o, raw=raw, take=take, give=give)  # noqa: E731
        frag = wts["mlp_frag"][level]
        o2 = torch.empty_like(o)
        run_fused = lambda: K.nbae_refine(feat, pred, frag[0], frag[1], o2)  # noqa: E731
        for _ in range(2):
            run()
            run_fused()
        tf = _timed(run_fused, a.runs)
        # planes the composed form writes and reads again: the upsampled features (C), the prediction columns (8), three hidden planes (128), raw (8 fp32)
        plane_bytes = px * ((c + 8 + 3 * 128) * 2 + 8 * 4)
        t = _timed(run, a.runs)
        res["refine"].append({"level": f"1/{div} -> 1/{div // 2}", "c": c, "pixels": px, "composed": _spread(t), "fused": _spread(tf),
                              "composed_over_fused": round(statistics.median(t) / statistics.median(tf), 3),
                              "fused_against_composed_rel_l2": float(((o2 - o).norm() / o.norm()).item()), "intermediate_bytes_each_way": plane_bytes,
                              "flop": 2 * px * ((c + 4) * 128 + 2 * 128 * 128 + 128 * 4)})
    res["refine_three_levels"] = {"composed_ms": round(sum(r["composed"]["median_ms"] for r in res["refine"]), 4),
                                  "fused_ms": round(sum(r["fused"]["median_ms"] for r in res["refine"]), 4)}
    print(json.dumps(res["refine"]), json.dumps(res["refine_three_levels"]), flush=True)
    dispatch.nbae_refine_fused = default_fused
    # the whole window under either setting of the switch
    res["annotate_batch_by_refine_form"] = {}
    for name, flag in (("fused", True), ("composed", False)):
        dispatch.nbae_refine_fused = flag
        for _ in range(2):
            ann.annotate_batch(dev_frames, out=out, rep=2)
        res["annotate_batch_by_refine_form"][name] = _spread(_timed(lambda: ann.annotate_batch(dev_frames, out=out, rep=2), a.runs))
    dispatch.nbae_refine_fused = default_fused
    print(json.dumps(res["annotate_batch_by_refine_form"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)

    if not a.no_torch:
        net = R.load(R.B5, sd).to(dev).half().to(memory_format=torch.channels_last)
        mean = torch.tensor(R.IMAGENET_MEAN, device=dev).view(1, 3, 1, 1)
        std = torch.tensor(R.IMAGENET_STD, device=dev).view(1, 3, 1, 1)

        def chain():
            with torch.no_grad():
                x = ((dev_frames.permute(0, 3, 1, 2).float() / 255.0 - mean) / std).half().contiguous(memory_format=torch.channels_last)
                outs = []
                for i0 in range(0, n, 4):     # four frames per pass: the full-resolution planes of torch's MLP stage
                    xyz = net(x[i0:i0 + 4])[-1][:, :3].float()
                    lv = (((xyz + 1) * 0.5).clip(0, 1) * 255.0).clip(0, 255).to(torch.uint8)
                    outs.append((lv.float() / 255).half())
                c = torch.cat(outs)
                return torch.cat([c, c])

        for _ in range(2):
            chain()
        res["torch_fp16_channels_last"] = _spread(_timed(chain, a.runs))
        res["torch_over_ours"] = round(res["torch_fp16_channels_last"]["median_ms"] / res["annotate_batch_device"]["median_ms"], 3)
        print(json.dumps({"torch_fp16_channels_last": res["torch_fp16_channels_last"], "torch_over_ours": res["torch_over_ours"]}), flush=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
