"""Times the paste-back of one 16-frame window of 512x768 frames at max_faces = 2 (32 face slots of 512x512), on seeded ParseNet weights in
fp16, in one process: face_paste.FacePaster.paste whole and replayed from a captured graph, each stage (prep, encoder, body, decoder, mask,
blur, paste) from events around its launches, the whole network under three settings of context.dispatch.parse_conv_reflect, every stride-1
layer shape of ParseNet on ca_conv3x3_reflect against the ring route (ca_ring_fill + ca_conv3x3 over the ringed tensor), ca_parse_mask
against its composed form, and -- in the same run, on the same weights and faces -- the same ParseNet (BatchNorm folded, as the device packs
it) as a torch fp16 channels_last chain up to the 19 maps.

    python tools/bench_facepaste.py [--frames 16] [--max-faces 2] [--runs 10] [--out profiles/facepaste_bench.json] [--no-torch]

Warm: two calls of every route before its timed window.  Every whole-call figure is median and [min, max] over --runs calls, a host clock
around work that ends in a device synchronise; the per-stage and per-layer figures are device events, the two routes of a layer alternating.
The restored faces, the matrices and the counts are planted (every slot holds a face): no trained checkpoint is available.  FLOP counts are
2 per multiply-add of the convolutions as the network defines them.  The result is written after the project's own figures and again after
torch's."""
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

from bench_lineart import _spread, _timed  # noqa: E402
from bench_normalbae import _stage_totals  # noqa: E402


def layer_table(fp, geo):
    """[(name, plane side of the input, cin, cout, stride, up2)] of every convolution of the network, in order."""
    out, p = [("encoder.0", geo.in_size, fp.CPAD, geo.base_ch, 1, False)], geo.in_size
    for name, cin, cout, scale in fp.blocks_of(geo):
        if fp.has_shortcut(cin, cout, scale):
            out.append((name + ".shortcut", p, cin, cout, 2 if scale == "down" else 1, scale == "up"))
        out.append((name + ".conv1", p, cin, cout, 1, scale == "up"))
        p1 = 2 * p if scale == "up" else p
        out.append((name + ".conv2", p1, cout, cout, 2 if scale == "down" else 1, False))
        p = p1 // 2 if scale == "down" else p1
    out.append(("out_mask_conv", p, out[-1][3], fp.PARSING_CH, 1, False))
    return out


def conv_flop(p, cin, cout, stride, up2) -> float:
    po = 2 * p if up2 else (p - 1) // stride + 1
    return 2.0 * po * po * 9 * cin * cout


def torch_chain(fp, sd, geo, dev):
    import torch
    F = torch.nn.functional

    def wb(name):
        w, b = fp.fold_bn(sd, name)
        return w.to(dev).half().contiguous(memory_format=torch.channels_last), b.to(dev).half()

    first, last = wb("encoder.0"), wb("out_mask_conv")
    blocks = [(name, scale, wb(name + ".shortcut_func") if fp.has_shortcut(cin, cout, scale) else None, wb(name + ".conv1"), wb(name + ".conv2"))
              for name, cin, cout, scale in fp.blocks_of(geo)]

    def conv(x, w, stride=1, up=False, leaky=False):
        if up:
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        y = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w[0], w[1], stride)
        return F.leaky_relu(y, 0.2) if leaky else y

    def run(faces_u8):
        with torch.no_grad():
            x = (((faces_u8.flip(-1).permute(0, 3, 1, 2).float() / 255.0) - 0.5) / 0.5).half().contiguous(memory_format=torch.channels_last)
            x = conv(x, first)
            feat = None
            for name, scale, sc, c1, c2 in blocks:
                if scale == "none" and feat is None:
                    feat = x
                idn = conv(x, sc, 2 if scale == "down" else 1, scale == "up") if sc is not None else x
                x = idn + conv(conv(x, c1, 1, scale == "up", True), c2, 2 if scale == "down" else 1)
                if name == f"body.{geo.res_depth - 1}":
                    x = feat + x
            return conv(x, last).float()

    return run


def _events(fn, runs):
    import torch
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--max-faces", type=int, default=2)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "facepaste_bench.json"))
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    import torch
    import facepaste_ref as P
    import facepaste_cases as CS
    from controlanimate_amd import face_paste as fp, kernels as K
    from controlanimate_amd.context import dispatch

    dev = torch.device("cuda:0")
    n, h, w, mf = a.frames, a.height, a.width, a.max_faces
    m = n * mf
    geo = fp.PARSENET
    sd = {k: v.half().float() for k, v in P.seeded_state_dict(P.FULL, 0).items()}
    paster = fp.FacePaster(sd, device=dev, dtype=torch.float16)
    rng = np.random.default_rng(0)
    base = CS.smooth_faces(4, 512, seed=1)
    restored = torch.from_numpy(np.stack([np.roll(base[i % 4], 17 * i, axis=1) for i in range(m)])).to(dev)
    frames = torch.from_numpy(rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)).to(dev)
    inv = np.zeros((n, mf, 2, 3))
    for i in range(n):
        for r in range(mf):
            s, ang = 0.45 + 0.02 * r, 0.1 * (r - 0.5)
            inv[i, r] = [[s * np.cos(ang), -s * np.sin(ang), 40.3 + 330 * r + 3 * i], [s * np.sin(ang), s * np.cos(ang), 120.7 + 5 * i]]
    inv = torch.from_numpy(inv).to(dev)
    count = torch.full((n,), mf, dtype=torch.int32, device=dev)
    out = torch.empty_like(frames)
    layers = layer_table(fp, geo)
    flop_face = sum(conv_flop(p, ci, co, st, up) for _, p, ci, co, st, up in layers)
    res = {"frames": n, "height": h, "width": w, "max_faces": mf, "faces": m, "dtype": "float16", "runs": a.runs, "device": torch.cuda.get_device_name(0),
           "passes": -(-m // paster.chunk_frames(514, 514)), "parsenet_gflop_per_face": round(flop_face / 1e9, 1), "parsenet_tflop_per_window": round(flop_face * m / 1e12, 2)}

    def call():
        return paster.paste(frames, restored, inv, count, out=out)

    for _ in range(2):
        call()
    res["paste_device"] = _spread(_timed(call, a.runs))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(2):
        graph.replay()
    res["paste_graph_replay"] = _spread(_timed(graph.replay, a.runs))
    paster.timings = {}
    for _ in range(a.runs):
        call()
    torch.cuda.synchronize()
    timed, paster.timings = paster.timings, None
    res["stages"] = _stage_totals(timed, a.runs)
    net_ms = sum(res["stages"][k]["total"]["median_ms"] for k in ("prep", "encoder", "body", "decoder", "mask"))
    res["parsenet_tflop_per_s"] = round(flop_face * m / net_ms / 1e9, 1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)

    def save(*keys):
        print(json.dumps({k: res[k] for k in keys}), flush=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    save("paste_device", "paste_graph_replay", "stages", "parsenet_tflop_per_s")

    # the network under both settings of the switch (the masks only), alternating
    def network():
        return paster._masks_u8(restored, paster.workspace(m), False)

    nets, default = {}, dispatch.parse_conv_reflect
    settings = {"network_reflect_kernel": True, "network_ring_route": False, "network_ring_route_64_128_256": (64, 128, 256)}
    for sw in settings.values():
        dispatch.parse_conv_reflect = sw
        for _ in range(2):
            network()
    for _ in range(a.runs):
        for name, sw in settings.items():
            dispatch.parse_conv_reflect = sw
            nets.setdefault(name, []).extend(_events(network, 1))
    dispatch.parse_conv_reflect = default
    res["default_parse_conv_reflect"] = default if isinstance(default, bool) else sorted(default)
    for name in settings:
        res[name] = _spread(nets[name])
    save("default_parse_conv_reflect", *settings)

    # every stride-1 layer shape: ca_conv3x3_reflect against ca_ring_fill + ca_conv3x3 on the ringed tensor
    per_layer, seen = [], set()
    for name, p, ci, co, st, up in layers[:-1]:
        if st != 1 or up or (p, ci, co) in seen:
            continue
        seen.add((p, ci, co))
        faces_here = min(m, max(1, int(0x7FFFFF00 // ((p + 2) * (p + 2) * max(ci, co) * 2))))
        x = torch.randn((faces_here, p, p, ci), device=dev, dtype=torch.float16)
        wt = (torch.randn((co, 3, 3, ci), device=dev) * (1.0 / (9 * ci)) ** 0.5).half()
        b = torch.zeros((co,), device=dev)
        y = torch.empty((faces_here, p, p, co), device=dev, dtype=torch.float16)
        xr = torch.zeros((faces_here, p + 2, p + 2, ci), device=dev, dtype=torch.float16)
        xr[:, 1:-1, 1:-1] = x
        yr = torch.empty((faces_here, p + 2, p + 2, co), device=dev, dtype=torch.float16)

        def direct():
            K.conv3x3_reflect(x, wt, b, leaky=True, out=y)

        def ring():
            K.ring_fill(xr)
            K.conv3x3(xr, wt, bias=b, act=K.ACT_LEAKY02, out=yr, split_k=False)

        for _ in range(2):
            direct(), ring()
        t = {"direct": [], "ring": []}
        for _ in range(a.runs):
            t["direct"].extend(_events(direct, 1))
            t["ring"].extend(_events(ring, 1))
        same = float(((y.float() - yr[:, 1:-1, 1:-1].float()).norm() / y.float().norm()).item())
        fl = conv_flop(p, ci, co, 1, False) * faces_here
        d, r = statistics.median(t["direct"]), statistics.median(t["ring"])
        per_layer.append({"layer": name, "plane": p, "cin": ci, "cout": co, "faces": faces_here, "gflop": round(fl / 1e9, 1), "ca_conv3x3_reflect": _spread(t["direct"]),
                          "ring_route": _spread(t["ring"]), "reflect_tflop_per_s": round(fl / d / 1e9, 1), "ring_tflop_per_s": round(fl / r / 1e9, 1),
                          "ring_over_reflect": round(r / d, 3), "rel_l2_between_routes": same})
        del x, y, xr, yr
    res["stride1_layers"] = per_layer
    save("stride1_layers")

    # the stride-2 and x2 layers (ca_conv3x3_reflect only)
    others, seen = [], set()
    for name, p, ci, co, st, up in layers:
        if (st == 1 and not up) or (p, ci, co, st, up) in seen:
            continue
        seen.add((p, ci, co, st, up))
        po = 2 * p if up else (p - 1) // st + 1
        faces_here = min(m, max(1, int(0x7FFFFF00 // max(p * p * ci * 2, po * po * co * 2))))
        x = torch.randn((faces_here, p, p, ci), device=dev, dtype=torch.float16)
        wt = (torch.randn((co, 3, 3, ci), device=dev) * (1.0 / (9 * ci)) ** 0.5).half()
        b = torch.zeros((co,), device=dev)
        y = torch.empty((faces_here, po, po, co), device=dev, dtype=torch.float16)

        def run():
            K.conv3x3_reflect(x, wt, b, stride=st, up2=up, out=y)

        for _ in range(2):
            run()
        t = _events(run, a.runs)
        fl = conv_flop(p, ci, co, st, up) * faces_here
        others.append({"layer": name, "plane": p, "cin": ci, "cout": co, "stride": st, "up2": up, "faces": faces_here, "gflop": round(fl / 1e9, 1), "ca_conv3x3_reflect": _spread(t),
                       "tflop_per_s": round(fl / statistics.median(t) / 1e9, 1)})
        del x, y
    res["stride2_and_up2_layers"] = others
    save("stride2_and_up2_layers")

    # the last layer: one launch against the composed form
    xh = torch.randn((m, 512, 512, geo.base_ch), device=dev, dtype=torch.float16)
    wts = paster._weights(dev)["mask"]
    mask = torch.empty((m, 512, 512), dtype=torch.uint8, device=dev)
    mask2, labels = torch.empty_like(mask), torch.empty_like(mask)
    logits = torch.empty((m, 512, 512, 32), dtype=torch.float32, device=dev)

    def fused():
        K.parse_mask(xh, wts[0], wts[1], mask)

    def composed():
        K.conv3x3_reflect(xh, wts[0], wts[1], out_f32=True, out=logits)
        K.parse_labels(logits, labels, mask2)

    for _ in range(2):
        fused(), composed()
    t = {"fused": [], "composed": []}
    for _ in range(a.runs):
        t["fused"].extend(_events(fused, 1))
        t["composed"].extend(_events(composed, 1))
    res["parse_mask"] = {"ca_parse_mask": _spread(t["fused"]), "composed": _spread(t["composed"]),
                         "composed_over_fused": round(statistics.median(t["composed"]) / statistics.median(t["fused"]), 3),
                         "pixels_that_differ": int((mask != mask2).sum().item()), "logit_bytes_not_written": int(logits.numel() * 4)}
    del xh, logits
    save("parse_mask")

    if not a.no_torch:
        chain = torch_chain(fp, sd, geo, dev)
        for _ in range(2):
            ref = chain(restored)
        res["torch_fp16_channels_last_network"] = _spread(_timed(lambda: chain(restored), a.runs))
        res["network_device"] = _spread(_timed(network, a.runs))
        res["torch_over_ours_network"] = round(res["torch_fp16_channels_last_network"]["median_ms"] / res["network_device"]["median_ms"], 3)
        ours = paster.logits(restored[:2])
        theirs = ref[:2].permute(0, 2, 3, 1)
        res["ours_against_torch_rel_l2_logits"] = float(((ours - theirs).norm() / theirs.norm()).item())
        save("torch_fp16_channels_last_network", "network_device", "torch_over_ours_network", "ours_against_torch_rel_l2_logits")


if __name__ == "__main__":
    main()
