"""Times the depth control images of one 16-frame window of 512x768 RGB frames on DPT-large-shaped seeded weights:
annotators.DepthAnnotator.annotate_batch(rep=2) from a uint8 device tensor and from PIL frames, each stage of the chain (resize, vit,
reassemble, fusion, head, tail) from events around it, ca_dpt_head against the composed head (ca_upsample2x_bilinear_ac + ca_conv3x3 +
ca_dpt_logit) at 192^2 -> 384^2 with 128 channels, and -- in the same run, on the same weights and frames -- the same network as a torch
fp16 chain on the GPU: transformers' DPTForDepthEstimation where that package is importable, else tests/depth_ref.py in fp16; the resize
to 384 (torch's bicubic, not Pillow's: only its time counts) and the pipeline's tail in torch ops around it.  It also records, on the
tiny fixture (tests/golden/dpt_tiny*.npz), the largest uint8 level difference to the fp32 fixture of a plain torch fp16 run and of the
product, for both normalisations.

    python tools/bench_depth.py [--frames 16] [--runs 10] [--out profiles/depth_bench.json] [--no-torch]

Warm: two calls of every route before its timed window.  Every figure is median and [min, max] over --runs calls, a host clock around
work that ends in a device synchronise; the per-stage figures are device events.  The weights are seeded (depth_ref.seeded_state_dict): no
trained checkpoint is available, and the float16 activation range of the trained Intel/dpt-large is unmeasured.  No speed-up was promised in
advance; the torch chain of the same run is the yardstick."""
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


def _spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "runs": len(ms)}


def _timed(fn, runs, warm=2):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return _spread(out)


def frames_u8(n, h, w, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for _ in range(n):
        img = np.stack([np.sin(2 * np.pi * (rng.uniform(0.5, 4) * y / h + rng.uniform(0.5, 4) * x / w) + rng.uniform(0, 6)) for _c in range(3)], -1)
        img += rng.normal(0, 0.15, img.shape)
        out.append(np.clip((img * 0.5 + 0.5) * 255, 0, 255).astype(np.uint8))
    return np.stack(out)


def build_annotator(sd, cfg, dtype, dev, normalize="max"):
    import torch
    from controlanimate_amd.depth import DepthAnnotator, DPTForDepthEstimation
    with torch.device(dev):
        model = DPTForDepthEstimation(**cfg)
    model.load_state_dict({k: v.to(dev) for k, v in sd.items()}, strict=True)
    model.to(dtype)
    return DepthAnnotator(model, cfg["image_size"], 3, normalize, device=dev)


def torch_chain(sd, cfg, dev):
    """-> (name, fn(frames uint8 [n, H, W, 3] on the device) -> control tensor [2n, 3, H, W] float32)."""
    import torch
    import torch.nn.functional as F
    import depth_ref as R
    try:
        from transformers import DPTConfig, DPTForDepthEstimation
        with torch.device(dev):
            model = DPTForDepthEstimation(DPTConfig(**cfg)).eval()
        model.load_state_dict(sd, strict=True)
        model = model.half()
        name = "transformers DPTForDepthEstimation, fp16"

        def net(pv):
            return model(pixel_values=pv).predicted_depth
    except Exception as e:  # transformers is absent (or cannot build the module) on this machine
        half = {k: v.half() for k, v in sd.items()}
        name = f"tests/depth_ref.py forward, fp16 ({type(e).__name__}: transformers' module was not usable)"

        def net(pv):
            return R.forward(half, cfg, pv)[0]

    s = cfg["image_size"]

    @torch.no_grad()
    def run(frames):
        n, h, w, _ = frames.shape
        x = frames.permute(0, 3, 1, 2).float()
        x = F.interpolate(x, size=(s, s), mode="bicubic", align_corners=False).round().clamp(0, 255)
        pv = ((x / 255 - 0.5) / 0.5).half()
        d = net(pv).float()
        d = F.interpolate(d[:, None], size=(h, w), mode="bicubic", align_corners=False)[:, 0]
        lv = (d * 255 / d.amax((1, 2), keepdim=True)).clamp(0, 255).to(torch.uint8)
        ctrl = (lv.float() / 255)[:, None].expand(-1, 3, -1, -1)
        return torch.cat([ctrl] * 2)

    return name, run


def level_differences(dev):
    """On the tiny fixture: the largest uint8 level difference to the fp32 fixture of a plain torch fp16 run of depth_ref and of the product."""
    import torch
    import torch.nn.functional as F
    import depth_ref as R
    data, sd = R.load_fixture()
    h, w = data["frames"].shape[1:3]
    pv = torch.from_numpy(data["pixel_values_r3"]).to(dev)
    with torch.no_grad():
        d16 = R.forward({k: v.to(dev).half() for k, v in sd.items()}, R.TINY_CONFIG, pv.half())[0].float()
    post16 = F.interpolate(d16[:, None], size=(h, w), mode="bicubic", align_corners=False)[:, 0].cpu().numpy()
    out = {}
    for mode in ("max", "minmax"):
        q = (lambda p: R.quantize_max(p)[0]) if mode == "max" else R.quantize_minmax
        want = np.stack([q(p) for p in data["post"]]).astype(int)
        ann = build_annotator(sd, R.TINY_CONFIG, torch.float16, dev, mode)
        got = ann.depth(list(data["frames"])).cpu().numpy().astype(int)
        out[mode] = {"torch_fp16": int(max(np.abs(q(post16[i]).astype(int) - want[i]).max() for i in range(3))), "product_fp16": int(np.abs(got - want).max())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_bench.json"))
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    import torch
    from PIL import Image
    import depth_ref as R
    from controlanimate_amd import kernels as K
    from controlanimate_amd.context import dispatch

    dev = "cuda:0"
    cfg = R.LARGE_CONFIG
    sd = {k: v.half().float() for k, v in R.seeded_state_dict(cfg, seed=1, device=dev).items()}
    ann = build_annotator(sd, cfg, torch.float16, dev)
    host = frames_u8(args.frames, args.height, args.width)
    pil = [Image.fromarray(f) for f in host]
    buf = torch.from_numpy(host).to(dev)
    n = args.frames
    out = torch.empty((2 * n, 3, args.height, args.width), dtype=torch.float32, device=dev)
    res = {"frames": n, "size": f"{args.height}x{args.width}", "rep": 2, "dtype": "float16", "control_dtype": "float32",
           "device": torch.cuda.get_device_name(0), "weights": "seeded, DPT-large-shaped (no trained checkpoint; its fp16 range is unmeasured)",
           "fusion_projection": "before the align-corners x2"}

    def write():
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")

    # the head: fused against composed, at the real shape
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, 192, 192, 128, generator=g).half().to(dev)
    w2 = (torch.randn(32, 3, 3, 128, generator=g) * (9 * 128) ** -0.5).half().to(dev)
    b2, w3, b3 = (torch.randn(32, generator=g) * 0.1).to(dev), (torch.randn(32, generator=g) * 0.2).to(dev), torch.tensor([0.5], device=dev)
    hout = torch.empty((n, 384, 384), dtype=torch.float32, device=dev)
    up = torch.empty((n, 384, 384, 128), dtype=torch.float16, device=dev)
    mid = torch.empty((n, 384, 384, 32), dtype=torch.float32, device=dev)
    fused = _timed(lambda: K.dpt_head(x, w2, b2, w3, b3, out=hout, fused=True), args.runs)
    composed = _timed(lambda: K.dpt_head(x, w2, b2, w3, b3, out=hout, fused=False, up=up, mid=mid), args.runs)
    del x, up, mid, hout
    res["head_192_to_384_c128"] = {"fused_ca_dpt_head": fused, "composed": composed, "composed_over_fused": round(composed["median_ms"] / fused["median_ms"], 3),
                                   "default": "fused" if fused["median_ms"] <= composed["median_ms"] else "composed"}
    dispatch.dpt_head_fused = fused["median_ms"] <= composed["median_ms"]   # the whole-chain figures below run the faster form
    res["dispatch_dpt_head_fused"] = bool(dispatch.dpt_head_fused)
    write()

    res["device_from_tensor"] = _timed(lambda: ann.annotate_batch(buf, out=out, rep=2), args.runs)
    res["device_from_pil"] = _timed(lambda: ann.annotate_batch(pil, out=out, rep=2), args.runs)
    stages = {}
    for _ in range(args.runs):
        ann.timings = {}
        ann.annotate_batch(buf, out=out, rep=2)
        torch.cuda.synchronize()
        for k, evs in ann.timings.items():
            stages.setdefault(k, []).append(sum(a.elapsed_time(b) for a, b in evs))
    ann.timings = ann.model.timings = None
    res["stages"] = {k: _spread(v) for k, v in stages.items()}
    res["device_stages_ms"] = round(sum(v["median_ms"] for v in res["stages"].values()), 4)
    write()
    res["uint8_level_difference_to_fp32_fixture"] = level_differences(dev)
    write()
    if not args.no_torch:
        name, chain = torch_chain(sd, cfg, dev)
        res["torch_chain"] = dict(_timed(lambda: chain(buf), args.runs), what=name)
        res["torch_over_device"] = round(res["torch_chain"]["median_ms"] / res["device_from_tensor"]["median_ms"], 3)
        write()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
