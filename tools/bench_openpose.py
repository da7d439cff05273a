"""Times the OpenPose body annotator (controlanimate_amd/openpose.py) for a window of frames with seeded weights, with the 7x7
convolutions of its refinement stages in both forms (context.dispatch.pose_conv7_direct: ca_conv7x7 / ca_im2col7x7 + ca_gemm), and
prints one JSON line: the whole chain and the conv7 stage per form, median of --iters passes after one warm-up pass each.

    python tools/bench_openpose.py [--frames 16] [--height 512] [--width 768] [--iters 5] [--dtype fp16]

--face times the face stage (controlanimate_amd/openpose_face.py) instead, in one run: the window without and with the stage (the
chain's own keypoints; `slots_filled` says how many of its face slots held a face), the stage alone from planted keypoints that fill
every slot for max_faces = 1, 2 and 4 with the cost per face slot and the per-stage times, and the same FaceNet as a torch fp16
channels_last chain on the same number of crops.

    python tools/bench_openpose.py --face > profiles/openpose_face_bench.json

--hand times the hand stage (controlanimate_amd/openpose_hand.py) likewise: the window without and with the stage (the chain's own
keypoints), the stage alone from planted keypoints that fill every slot for max_hands = 1, 2 and 4 with the cost per hand slot and the
per-stage times, and the same handpose_model as a torch fp16 channels_last chain on the same number
of slots at the four sides.

    python tools/bench_openpose.py --hand > profiles/openpose_hand_bench.json
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


def _median_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    return round(statistics.median(times), 3)


def face_mode(a):
    import face_ref
    import pose_ref
    from controlanimate_amd.openpose import OpenposeAnnotator
    dev, dtype = "cuda:0", torch.float16 if a.dtype == "fp16" else torch.bfloat16
    res = min(a.height, a.width)
    body, face = pose_ref.pose_state_dict(0), face_ref.face_state_dict(0)
    frames = torch.from_numpy(pose_ref.frames_fixture(a.frames, a.height, a.width)).to(dev)
    out = torch.empty((2 * a.frames, 3, a.height, a.width), dtype=torch.float16, device=dev)
    result = {"frames": a.frames, "height": a.height, "width": a.width, "dtype": a.dtype, "weights": "seeded (no trained checkpoint)", "default_max_faces": 2}
    plain = OpenposeAnnotator(body, device=dev, dtype=dtype, detect_resolution=res, image_resolution=res)
    result["chain_ms_without_faces"] = _median_ms(lambda: plain.annotate_batch(frames, out=out, rep=2), a.iters)
    # two heads per frame whose boxes are 180 and 120 pixels wide, repeated to fill every slot
    heads = [face_ref.head(200, 200, eye=30, ear=50), face_ref.head(500, 300, eye=20, ear=36), face_ref.head(350, 120, eye=30, ear=50),
             face_ref.head(640, 150, eye=20, ear=36)]
    for mf in (1, 2, 4):
        ann = OpenposeAnnotator(body, device=dev, dtype=dtype, detect_resolution=res, image_resolution=res, face=face, max_faces=mf)
        with_faces = _median_ms(lambda: ann.annotate_batch(frames, out=out, rep=2), a.iters)
        _, boxes, _ = ann.faces(frames)
        kp = torch.from_numpy(np.stack([face_ref.keypoints_of(heads[:mf])] * a.frames)).to(dev)
        people = torch.full((a.frames,), mf, dtype=torch.int32, device=dev)
        stage = _median_ms(lambda: ann._faces_from(frames, kp, people), a.iters)
        filled = int((ann._face.workspace(a.frames, a.height, a.width, frames.device)["buf"]["slots"][:, :, 0] >= 0).sum())
        assert filled == a.frames * mf
        entry = {"crops": a.frames * mf, "chain_ms_with_faces": with_faces, "slots_filled_by_the_chain": int((boxes[:, :, 3] >= 0).sum()),
                 "face_stage_ms_all_slots_filled": stage, "ms_per_face_slot": round(stage / (a.frames * mf), 4)}
        ann.timings = {}
        ann._faces_from(frames, kp, people)
        torch.cuda.synchronize()
        entry["stages_ms"] = {k: round(sum(x.elapsed_time(y) for x, y in v), 3) for k, v in ann.timings.items()}
        ann.timings = None
        result[f"max_faces_{mf}"] = entry
        del ann
        torch.cuda.empty_cache()
    # the same network in torch: fp16 (or bf16), channels_last, on the default number of crops
    net = face_ref.face_net(face).to(dev).to(dtype).to(memory_format=torch.channels_last)
    x = torch.randn((a.frames * 2, 3, 384, 384), device=dev).to(dtype).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        result["torch_channels_last_facenet_ms"] = {"crops": a.frames * 2, "ms": _median_ms(lambda: net(x), a.iters)}
    net_ms = sum(v for k, v in result["max_faces_2"]["stages_ms"].items() if k in ("face_conv", "face_pool", "face_copy", "face_pointwise", "face_conv7"))
    result["hip_facenet_ms"] = {"crops": a.frames * 2, "ms": round(net_ms, 3)}
    print(json.dumps(result))


def hand_mode(a):
    import hand_ref
    import pose_ref
    from controlanimate_amd.openpose import OpenposeAnnotator
    from controlanimate_amd.openpose_hand import SIDES
    dev, dtype = "cuda:0", torch.float16 if a.dtype == "fp16" else torch.bfloat16
    res = min(a.height, a.width)
    body, hand = pose_ref.pose_state_dict(0), hand_ref.hand_state_dict(0)
    frames = torch.from_numpy(pose_ref.frames_fixture(a.frames, a.height, a.width)).to(dev)
    out = torch.empty((2 * a.frames, 3, a.height, a.width), dtype=torch.float16, device=dev)
    result = {"frames": a.frames, "height": a.height, "width": a.width, "dtype": a.dtype, "weights": "seeded (no trained checkpoint)", "default_max_hands": 2}
    plain = OpenposeAnnotator(body, device=dev, dtype=dtype, detect_resolution=res, image_resolution=res)
    result["chain_ms_without_hands"] = _median_ms(lambda: plain.annotate_batch(frames, out=out, rep=2), a.iters)
    # two people per frame with both arms: boxes of 82, 94, 82 and 94 pixels, taken in order until the slots are full
    people_list = [{**hand_ref.arm((200, 300), (180, 260), (170, 200)), **hand_ref.arm((300, 310), (320, 250), (330, 200), left=False)},
                   {**hand_ref.arm((500, 300), (480, 260), (470, 200)), **hand_ref.arm((600, 310), (620, 250), (630, 200), left=False)}]
    kp = torch.from_numpy(np.stack([hand_ref.keypoints_of(people_list)] * a.frames)).to(dev)
    people = torch.full((a.frames,), 2, dtype=torch.int32, device=dev)
    for mh in (1, 2, 4):
        ann = OpenposeAnnotator(body, device=dev, dtype=dtype, detect_resolution=res, image_resolution=res, hand=hand, max_hands=mh)
        whole = _median_ms(lambda: ann.annotate_batch(frames, out=out, rep=2), a.iters)
        _, boxes, _ = ann.hands(frames)
        stage = _median_ms(lambda: ann._hand.run(frames, kp, people), a.iters)
        filled = int((ann._hand.workspace(a.frames, a.height, a.width, frames.device)["buf"]["slots"][:, :, 0] >= 0).sum())
        assert filled == a.frames * mh
        entry = {"slots": a.frames * mh, "chain_ms_with_hands": whole, "slots_filled_by_the_chain": int((boxes[:, :, :, 3] >= 0).sum()),
                 "hand_stage_ms_all_slots_filled": stage, "ms_per_hand_slot": round(stage / (a.frames * mh), 4)}
        ann.timings = {}
        ann._hand.run(frames, kp, people)
        torch.cuda.synchronize()
        entry["stages_ms"] = {k: round(sum(x.elapsed_time(y) for x, y in v), 3) for k, v in ann.timings.items()}
        ann.timings = None
        result[f"max_hands_{mh}"] = entry
        del ann
        torch.cuda.empty_cache()
    # the same network in torch: fp16 (or bf16), channels_last, on the default number of slots at the same four sides
    net = hand_ref.hand_net(hand).to(dev).to(dtype).to(memory_format=torch.channels_last)
    xs = [torch.randn((a.frames * 2, 3, s, s), device=dev).to(dtype).contiguous(memory_format=torch.channels_last) for s in SIDES]
    with torch.no_grad():
        result["torch_channels_last_handnet_ms"] = {"slots": a.frames * 2, "ms": _median_ms(lambda: [net(x) for x in xs], a.iters)}
    net_ms = sum(v for k, v in result["max_hands_2"]["stages_ms"].items() if k in ("hand_conv", "hand_pool", "hand_copy", "hand_pointwise", "hand_conv7"))
    result["hip_handnet_ms"] = {"slots": a.frames * 2, "ms": round(net_ms, 3)}
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--dtype", choices=("fp16", "bf16"), default="fp16")
    ap.add_argument("--face", action="store_true", help="time the face stage (see the head of this file)")
    ap.add_argument("--hand", action="store_true", help="time the hand stage (see the head of this file)")
    a = ap.parse_args()
    if a.face:
        return face_mode(a)
    if a.hand:
        return hand_mode(a)
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
