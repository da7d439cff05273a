"""Times the Real-ESRGAN upscaler (RRDBNet anime-6B) on one window of the SampleConfig size: 16 frames of 512 x 768 to x4 and to x2.

    python tools/bench_upscaler.py [--frames 16] [--h 512] [--w 768] [--iters 3] [--no-torch] [--out profiles/upscaler_bench.json]

* HIP path: Upscaler.enhance_batch (ca_rgb8_to_nhwc, 97 ca_conv3x3_narrow launches per pass, ca_resize_lanczos4_u8 at x2), frames
  uint8 on the device, result left on the device.  HIP events around synchronised work, after one warm-up pass.
* torch chain: the same net as plain torch.nn.functional.conv2d in fp16 NCHW (MIOpen), with torch.cat for the dense blocks and
  F.interpolate for the upsamplings -- how the reference executes it (RealESRGANer, half=True) -- timed alternately with the HIP
  path in the same process.  Same frame chunking (8 frames per pass).
* FLOPs from the layer shapes (2 * pixels * cout * 9 * cin per convolution, real channel counts); share of the 2.5 PFLOP/s dense
  fp16 peak.  The bytes each pass must move (every activation written once and read by the layers behind it, L2-cold) are
  counted too, so that the script states which of the two bounds the pass.
One JSON line per measurement on stdout; all of them in --out.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F16 = 2.5e15   # dense fp16 MFMA, MI355X
HBM_BPS = 8.0e12    # HBM3E


def layer_shapes():
    """(name, cin, cout, resolution factor) of every convolution of RRDBNet(num_feat 64, num_block 6, num_grow_ch 32, scale 4)."""
    out = [("conv_first", 3, 64, 1)]
    for i in range(6):
        for r in ("rdb1", "rdb2", "rdb3"):
            for c in range(1, 6):
                out.append((f"body.{i}.{r}.conv{c}", 64 + 32 * (c - 1), 32 if c < 5 else 64, 1))
    out += [("conv_body", 64, 64, 1), ("conv_up1", 64, 64, 2), ("conv_up2", 64, 64, 4), ("conv_hr", 64, 64, 4), ("conv_last", 64, 3, 4)]
    return out


def flops_per_frame(h, w):
    return sum(2.0 * h * f * w * f * cout * 9 * cin for _, cin, cout, f in layer_shapes())


def bytes_per_frame(h, w):
    """fp16 activations written once + read once by each consumer (concat inputs re-read per dense layer)."""
    b = 0.0
    for name, cin, cout, f in layer_shapes():
        px = h * f * w * f
        px_in = px // 4 if name in ("conv_up1", "conv_up2") else px  # the x2 upsampling is folded into the gather
        b += 2.0 * (px * cout + px_in * cin)
    return b


def torch_chain(sd, x):
    """The net in fp16 NCHW with torch.nn.functional (MIOpen convolutions); x: [n, 3, H, W] fp16."""
    def conv(n, t):
        return F.conv2d(t, sd[n + ".weight"], sd[n + ".bias"], padding=1)

    def lrelu(t):
        return F.leaky_relu(t, 0.2)

    def rdb(p, x0):
        x1 = lrelu(conv(p + ".conv1", x0))
        x2 = lrelu(conv(p + ".conv2", torch.cat((x0, x1), 1)))
        x3 = lrelu(conv(p + ".conv3", torch.cat((x0, x1, x2), 1)))
        x4 = lrelu(conv(p + ".conv4", torch.cat((x0, x1, x2, x3), 1)))
        return conv(p + ".conv5", torch.cat((x0, x1, x2, x3, x4), 1)) * 0.2 + x0

    feat = conv("conv_first", x)
    body = feat
    for i in range(6):
        body = rdb(f"body.{i}.rdb3", rdb(f"body.{i}.rdb2", rdb(f"body.{i}.rdb1", body))) * 0.2 + body
    feat = feat + conv("conv_body", body)
    feat = lrelu(conv("conv_up1", F.interpolate(feat, scale_factor=2, mode="nearest")))
    feat = lrelu(conv("conv_up2", F.interpolate(feat, scale_factor=2, mode="nearest")))
    out = conv("conv_last", lrelu(conv("conv_hr", feat)))
    return (out.float().clamp_(0, 1) * 255).round().to(torch.uint8)


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--h", type=int, default=512)
    ap.add_argument("--w", type=int, default=768)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="alternating HIP / torch rounds")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from rrdb_ref import rrdb_state_dict
    from controlanimate_amd.upscaler import Upscaler
    dev = torch.device("cuda:0")
    sd = rrdb_state_dict(seed=0)
    up = Upscaler(4, use_face_enhancer=False, state_dict=sd, device=dev)
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (a.frames, a.h, a.w, 3), generator=g, dtype=torch.uint8).to(dev)
    sd16 = {k: v.to(dev).half() for k, v in sd.items()}
    x_nchw = frames.permute(0, 3, 1, 2).flip(1).half().div_(255).contiguous()
    fl = flops_per_frame(a.h, a.w) * a.frames
    by = bytes_per_frame(a.h, a.w) * a.frames
    results = []

    def emit(d):
        d.update(frames=a.frames, h=a.h, w=a.w, tflop=round(fl / 1e12, 2), gbytes=round(by / 1e9, 2),
                 floor_ms_flops=round(fl / PEAK_F16 * 1e3, 1), floor_ms_bytes=round(by / HBM_BPS * 1e3, 1))
        ms = d["ms_per_window"]
        d["tflops"] = round(fl / (ms * 1e-3) / 1e12, 1)
        d["share_of_peak"] = round(fl / (ms * 1e-3) / PEAK_F16, 3)
        d["bound"] = "flops" if d["floor_ms_flops"] > d["floor_ms_bytes"] else "bytes"
        print(json.dumps(d), flush=True)
        results.append(d)

    hip4 = lambda: up.enhance_batch(frames, 4)  # noqa: E731
    hip2 = lambda: up.enhance_batch(frames, 2)  # noqa: E731

    def tor():
        for s in range(0, a.frames, 8):
            torch_chain(sd16, x_nchw[s:s + 8])

    with torch.no_grad():
        hip4(), hip2()
        if not a.no_torch:
            tor()
        for r in range(a.rounds):
            emit({"path": "hip", "outscale": 4, "round": r, "ms_per_window": round(timed(hip4, a.iters), 2)})
            emit({"path": "hip", "outscale": 2, "round": r, "ms_per_window": round(timed(hip2, a.iters), 2)})
            if not a.no_torch:
                emit({"path": "torch_miopen_nchw_f16", "outscale": 4, "round": r, "ms_per_window": round(timed(tor, a.iters), 2)})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
