"""Times the OpenPose body annotator (controlanimate_amd/openpose.py) for a window of frames with seeded weights, with the 7x7
convolutions of its refinement stages in both forms (context.dispatch.pose_conv7_direct: ca_conv7x7 / ca_im2col7x7 + ca_gemm), and
prints one JSON line: the whole chain and the conv7 stage per form, median of --iters passes after one warm-up pass each.

    python tools/bench_openpose.py [--frames 16] [--height 512] [--width 768] [--iters 5] [--dtype fp16]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--dtype", choices=("fp16", "bf16"), default="fp16")
    a = ap.parse_args()
    import pose_ref
    from controlanimate_amd.context import dispatch
    from controlanimate_amd.openpose import OpenposeAnnotator
    res = min(a.height, a.width)
    ann = OpenposeAnnotator(pose_ref.pose_state_dict(0), device="cuda:0", dtype=torch.float16 if a.dtype == "fp16" else torch.bfloat16,
                            detect_resolution=res, image_resolution=res)
    frames = torch.from_numpy(pose_ref.frames_fixture(a.frames, a.height, a.width)).to("cuda:0")
    out = torch.empty((2 * a.frames, 3, a.height, a.width), dtype=torch.float16, device="cuda:0")
    default = bool(dispatch.pose_conv7_direct)
    result = {"frames": a.frames, "height": a.height, "width": a.width, "dtype": a.dtype, "weights": "seeded (no trained checkpoint)",
              "default_pose_conv7_direct": default}
    try:
        for direct in (True, False):
            dispatch.pose_conv7_direct = direct
            ann.annotate_batch(frames, out=out, rep=2)
            torch.cuda.synchronize()
            whole, conv7, stages = [], [], {}
            for _ in range(a.iters):
                ann.timings = {}
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                ann.annotate_batch(frames, out=out, rep=2)
                e.record()
                torch.cuda.synchronize()
                whole.append(s.elapsed_time(e))
                per = {k: sum(x.elapsed_time(y) for x, y in v) for k, v in ann.timings.items()}
                conv7.append(per["conv7"])
                for k, v in per.items():
                    stages.setdefault(k, []).append(v)
                ann.timings = None
            key = "direct" if direct else "im2col_gemm"
            result[f"chain_ms_{key}"] = round(statistics.median(whole), 3)
            result[f"conv7_ms_{key}"] = round(statistics.median(conv7), 3)
            result[f"stages_ms_{key}"] = {k: round(statistics.median(v), 3) for k, v in stages.items()}
    finally:
        dispatch.pose_conv7_direct = default
    print(json.dumps(result))


if __name__ == "__main__":
    main()
