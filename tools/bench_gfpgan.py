"""Times GFPGAN face restoration of 16 aligned 512 x 512 faces (one per frame of a window): gfpgan.FaceRestorer.restore_aligned from a
uint8 device tensor and from PIL frames (noise drawn on the device, as the reference's randomize_noise=True), each stage of the chain
from device events around it, and -- in the same run, on the same seeded weights and inputs -- the same network as a torch fp16
channels_last chain on the GPU whose modulated convolutions are written as upstream writes them (a per-sample weight and a grouped
convolution: tests/gfpgan_ref.py, the specification's modules).  For each StyleConv of the decoder it also times the two forms of
kernels.modconv3x3 -- "fused": ca_modconv3x3, one launch; "composed": ca_gfp_modulate -> ca_conv3x3 without split-K ->
ca_gfp_style_epilogue -- beside a bare ca_conv3x3 on the same plane and channels.  kernels.MODCONV_FUSED_MIN_PIXELS is set from these
figures.  The figures beside each other are TFLOP/s (2 per multiply-add, padding taps counted).

    python tools/bench_gfpgan.py [--faces 16] [--runs 10] [--out profiles/gfpgan_bench.json] [--no-torch]

Warm: two calls of every route before its timed window.  Every figure is median and [min, max] over --runs calls: a host clock around
work that ends in a device synchronise for the whole calls, device events for stages and kernels.  The weights are the seeded ones of
tests/gfpgan_ref.make_net: no trained checkpoint is available.  The result file is written after the project's own figures and again
after torch's, in the same process."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEV = "cuda:0"


def _spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def _host_timed(fn, runs):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return _spread(out)


def _event_timed(fn, runs):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return _spread(out)


def style_layers(size=512):
    """(input plane, cin, cout, upsample) of the decoder's StyleConv layers in launch order."""
    from controlanimate_amd.gfpgan import stylegan_channels as ch
    out = [(4, ch(4), ch(4), False)]
    s = 8
    while s <= size:
        out += [(s // 2, ch(s // 2), ch(s), True), (s, ch(s), ch(s), False)]
        s *= 2
    return out


def bench_project(args, result):
    import torch
    import gfpgan_ref as R
    from PIL import Image
    from controlanimate_amd import kernels as K
    from controlanimate_amd.gfpgan import STAGES, FaceRestorer
    n, runs = args.faces, args.runs
    sd = R.make_net(512, 5).state_dict()
    r = FaceRestorer(sd, device=DEV, dtype=torch.float16, max_faces_per_launch=max(n, 1))
    faces = R.make_faces(512, n, 7)
    dev_faces = faces.to(DEV)
    pil = [Image.fromarray(f) for f in faces.numpy()]
    gen = torch.Generator(device=DEV).manual_seed(3)
    result["faces"], result["runs"] = n, runs
    result["restore_aligned_ms"] = {"device_tensor": _host_timed(lambda: r.restore_aligned(dev_faces, generator=gen), runs),
                                    "pil_frames": _host_timed(lambda: r.restore_aligned(pil, generator=gen), runs)}
    per_call = {s: [] for s in STAGES}
    for _ in range(runs):
        r.timings = {}
        r.restore_aligned(dev_faces, generator=gen)
        torch.cuda.synchronize()
        for s in STAGES:
            per_call[s].append(sum(a.elapsed_time(b) for a, b in r.timings.get(s, [])))
    r.timings = None
    result["stages_ms"] = {s: _spread(v) for s, v in per_call.items()}
    result["stage_launches"] = "encoder counts its resamplings, 1x1 skips and adds; sft is 4 ca_conv3x3 per level; modconv is the 15 StyleConv"
    # ---- the StyleConv layers: fused, ca_conv3x3 on the same plane and channels, and the stand-in for the three-pass form
    g = torch.Generator().manual_seed(11)
    rows = []
    for plane, cin, cout, up in style_layers():
        hh = 2 * plane if up else plane
        x = torch.randn(n, plane, plane, cin, generator=g).half().to(DEV)
        xo = torch.randn(n, hh, hh, cin, generator=g).half().to(DEV) if up else x
        w = (torch.randn(cout, 3, 3, cin, generator=g) * (1.0 / (9 * cin)) ** 0.5).half().to(DEV)
        s, dm = (torch.rand(n, cin, generator=g) * 2 - 1).to(DEV), (torch.rand(n, cout, generator=g) + 0.5).to(DEV)
        noise, bias = torch.randn(n, hh, hh, generator=g).to(DEV), torch.zeros(cout, device=DEV)
        sft = tuple(torch.randn(n, hh, hh, cout // 2, generator=g).half().to(DEV) for _ in range(2)) if up else None
        y = torch.empty(n, hh, hh, cout, dtype=torch.float16, device=DEV)
        xs = torch.empty_like(xo)
        flop = 2.0 * 9 * cin * cout * hh * hh * n
        fused = _event_timed(lambda: K.modconv3x3(x, w, s, dm, noise, bias, 0.1, upsample=up, sft=sft, out=y, form="fused"), runs)
        comp = _event_timed(lambda: K.modconv3x3(x, w, s, dm, noise, bias, 0.1, upsample=up, sft=sft, out=y, form="composed", scratch=xs), runs)
        conv = _event_timed(lambda: K.conv3x3(xo, w, bias=bias, act=K.ACT_LEAKY02, out=y), runs)

        row = {"plane_out": hh, "cin": cin, "cout": cout, "upsample": up, "sft": sft is not None, "gflop": flop / 1e9,
               "fused_ms": fused, "composed_ms": comp, "conv3x3_ms": conv,
               "default_form": "fused" if hh * hh >= K.MODCONV_FUSED_MIN_PIXELS else "composed",
               "fused_tflops": flop / fused["median"] / 1e9, "composed_tflops": flop / comp["median"] / 1e9,
               "conv3x3_tflops": flop / conv["median"] / 1e9}
        rows.append(row)
        print(f"  {hh:4d}^2 {cin:3d}->{cout:3d} up={int(up)}: fused {fused['median']:.3f} [{fused['min']:.3f}, {fused['max']:.3f}] ms ({row['fused_tflops']:.0f} TF)  "
              f"composed {comp['median']:.3f} [{comp['min']:.3f}, {comp['max']:.3f}] ms ({row['composed_tflops']:.0f} TF)  conv3x3 {conv['median']:.3f} ms ({row['conv3x3_tflops']:.0f} TF)", flush=True)
        del x, xo, w, y, xs, sft, noise
    result["style_convs"] = rows


def bench_torch(args, result):
    import torch
    import gfpgan_ref as R
    n, runs = args.faces, args.runs
    net = R.make_net(512, 5).half().to(DEV)
    for p in net.parameters():                     # (the modulated weights are 5-D: only the ordinary convolutions' take the format)
        if p.dim() == 4:
            p.data = p.data.contiguous(memory_format=torch.channels_last)
    faces = R.make_faces(512, n, 7).to(DEV)
    noises = [t.to(DEV).half()[:, None] for t in R.make_noises(512, n, 8)]

    def chain():
        with torch.no_grad():
            x = (faces.float() / 255.0).flip(-1).sub(0.5).div(0.5).permute(0, 3, 1, 2).half().contiguous(memory_format=torch.channels_last)
            for t in noises:
                t.normal_()
            img = net(x, noises)
            return ((img.float().clamp(-1, 1) + 1) / 2 * 255).round().to(torch.uint8).permute(0, 2, 3, 1).flip(-1).contiguous()
    result["torch_fp16_channels_last_ms"] = _host_timed(chain, runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=16)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gfpgan_bench.json"))
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    import torch
    result = {}
    result.update({"device": torch.cuda.get_device_name(0), "dtype": "float16", "weights": "tests/gfpgan_ref.make_net(512, seed 5)"})

    def write():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
    bench_project(args, result)
    write()
    print(json.dumps({k: result[k] for k in ("restore_aligned_ms", "stages_ms")}), flush=True)
    if not args.no_torch:
        bench_torch(args, result)
        write()
        print(json.dumps({"torch_fp16_channels_last_ms": result["torch_fp16_channels_last_ms"]}), flush=True)


if __name__ == "__main__":
    main()
