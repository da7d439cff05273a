"""Times face detection and alignment of one 16-frame window of 512x768 RGB frames, on seeded full-width weights in fp16, in one process:
face_align.FaceAligner.align from a uint8 device tensor, from PIL frames and replayed from a captured graph, each stage of the chain (stem,
body, FPN+SSH, heads, decode, warp) from events around its launches, and -- in the same run, on the same weights and frames -- the same
network (BatchNorm folded, as the device packs it) as a torch fp16 channels_last chain up to the head tensors.

    python tools/bench_facealign.py [--frames 16] [--runs 10] [--out profiles/facealign_bench.json] [--no-torch]

Warm: two calls of every route before its timed window.  Every figure is median and [min, max] over --runs calls, a host clock around
work that ends in a device synchronise; the per-stage figures are device events.  The weights are tests/retinaface_ref.seeded_state_dict:
no trained checkpoint is available, so conf_threshold is 0.5 (seeded weights pass about half the priors: the decode sees the 1024-candidate
cap on every frame, its slowest case).  The result is written after the project's own figures and again after torch's."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_lineart import _spread, _timed, frame  # noqa: E402
from bench_normalbae import _stage_totals  # noqa: E402


def torch_chain(fa, sd, geo, dev):
    """The network with BatchNorm folded, fp16 weights in channels_last, as plain torch calls: uint8 frames [n, H, W, 3] -> the nine head tensors."""
    import torch
    F = torch.nn.functional

    def wb(conv, bn):
        w, b = fa.fold_bn(sd, conv, bn)
        return w.to(dev).half().contiguous(memory_format=torch.channels_last), b.to(dev).half()

    stem = wb("body.conv1", "body.bn1")
    blocks = []
    for li, b, _, _, _, stride in fa.blocks_of(geo):
        p = f"body.layer{li}.{b}"
        blocks.append((li, b, stride, wb(p + ".conv1", p + ".bn1"), wb(p + ".conv2", p + ".bn2"), wb(p + ".conv3", p + ".bn3"),
                       wb(p + ".downsample.0", p + ".downsample.1") if b == 0 else None))
    outs = [wb(f"fpn.output{k}.0", f"fpn.output{k}.1") for k in (1, 2, 3)]
    merges = [wb(f"fpn.merge{k}.0", f"fpn.merge{k}.1") for k in (1, 2)]
    ssh = [{name: wb(f"ssh{k}.{name}.0", f"ssh{k}.{name}.1") for name in fa.SSH_CONVS} for k in (1, 2, 3)]
    heads = [[(sd[f"{name}.{k}.conv1x1.weight"].to(dev).half().contiguous(memory_format=torch.channels_last), sd[f"{name}.{k}.conv1x1.bias"].to(dev).half())
              for name, _ in fa.HEADS] for k in range(3)]
    mean = torch.tensor([104.0, 117.0, 123.0], device=dev).view(1, 3, 1, 1)

    def run(frames_u8):
        with torch.no_grad():
            x = (frames_u8.permute(0, 3, 1, 2).float() - mean).half().contiguous(memory_format=torch.channels_last)
            x = F.max_pool2d(F.relu(F.conv2d(x, *stem, 2, 3)), 3, 2, 1)
            taps = []
            for li, b, stride, c1, c2, c3, down in blocks:
                y = F.relu(F.conv2d(x, *c1))
                y = F.relu(F.conv2d(y, *c2, stride, 1))
                y = F.conv2d(y, *c3)
                if down is not None:
                    x = F.conv2d(x, *down, stride)
                x = F.relu(y + x)
                if li > 1 and b == fa.LAYERS[li - 1] - 1:
                    taps.append(x)
            o = [F.relu(F.conv2d(t, *w)) for t, w in zip(taps, outs)]
            o[1] = F.relu(F.conv2d(o[1] + F.interpolate(o[2], size=o[1].shape[2:], mode="nearest"), *merges[1], 1, 1))
            o[0] = F.relu(F.conv2d(o[0] + F.interpolate(o[1], size=o[0].shape[2:], mode="nearest"), *merges[0], 1, 1))
            res = []
            for f, s, hd in zip(o, ssh, heads):
                c3 = F.conv2d(f, *s["conv3X3"], 1, 1)
                c51 = F.relu(F.conv2d(f, *s["conv5X5_1"], 1, 1))
                c5 = F.conv2d(c51, *s["conv5X5_2"], 1, 1)
                c7 = F.conv2d(F.relu(F.conv2d(c51, *s["conv7X7_2"], 1, 1)), *s["conv7x7_3"], 1, 1)
                f = F.relu(torch.cat([c3, c5, c7], 1))
                res.extend(F.conv2d(f, *w).float() for w in hd)
            return res

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "facealign_bench.json"))
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    import torch
    from PIL import Image
    import retinaface_ref as R
    from controlanimate_amd import face_align as fa

    dev = torch.device("cuda:0")
    n, h, w = a.frames, a.height, a.width
    geo = fa.RESNET50
    sd = {k: v.half().float() for k, v in R.seeded_state_dict(fa.retinaface_key_shapes(geo), 0).items()}
    al = fa.FaceAligner(sd, device=dev, dtype=torch.float16, conf_threshold=0.5)
    frames = np.stack([frame(h, w, i) for i in range(n)])
    dev_frames = torch.from_numpy(frames).to(dev)
    pil = [Image.fromarray(f) for f in frames]
    res = {"frames": n, "height": h, "width": w, "dtype": "float16", "runs": a.runs, "device": torch.cuda.get_device_name(0), "max_faces": al.max_faces,
           "conf_threshold": 0.5, "priors_per_frame": R.prior_count(h, w), "passes": -(-n // al.chunk_frames(h, w))}
    for _ in range(2):
        out = al.align(dev_frames)
    res["faces_found"] = out["count"].tolist()
    res["overflow"] = out["overflow"].tolist()
    res["align_device"] = _spread(_timed(lambda: al.align(dev_frames), a.runs))
    for _ in range(2):
        al.align(pil)
    res["align_pil"] = _spread(_timed(lambda: al.align(pil), a.runs))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        al.align(dev_frames)
    for _ in range(2):
        graph.replay()
    res["align_graph_replay"] = _spread(_timed(graph.replay, a.runs))
    al.timings = {}
    for _ in range(a.runs):
        al.align(dev_frames)
    torch.cuda.synchronize()
    timed, al.timings = al.timings, None
    res["stages"] = _stage_totals(timed, a.runs)
    # the network alone (up to the head tensors), what the torch chain below computes
    for _ in range(2):
        al.heads(dev_frames)
    res["network_device"] = _spread(_timed(lambda: al._heads(dev_frames, al.workspace(n, h, w), False), a.runs))
    print(json.dumps({k: res[k] for k in ("align_device", "align_pil", "align_graph_replay", "network_device", "stages", "faces_found", "overflow")}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)

    if not a.no_torch:
        chain = torch_chain(fa, sd, geo, dev)
        for _ in range(2):
            ref = chain(dev_frames)
        res["torch_fp16_channels_last_network"] = _spread(_timed(lambda: chain(dev_frames), a.runs))
        res["torch_over_ours_network"] = round(res["torch_fp16_channels_last_network"]["median_ms"] / res["network_device"]["median_ms"], 3)
        # the two fp16 chains against each other on the class logits of the finest level
        ours = al.heads(dev_frames)[0][..., :4]
        theirs = ref[0].permute(0, 2, 3, 1)
        res["ours_against_torch_rel_l2_class0"] = float(((ours - theirs).norm() / theirs.norm()).item())
        print(json.dumps({k: res[k] for k in ("torch_fp16_channels_last_network", "torch_over_ours_network", "ours_against_torch_rel_l2_class0")}), flush=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
