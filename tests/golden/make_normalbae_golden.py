"""Writes tests/golden/normalbae_tiny.npz and normalbae_tiny_w0.npz / _w1.npz (the weights): the pin of the NormalBae annotator's encoder arithmetic against transformers.

    python tests/golden/make_normalbae_golden.py

transformers' EfficientNetModel at EfficientNetConfig(width_coefficient=0.5, depth_coefficient=0.35, hidden_dim=640) is the encoder of
tests/normalbae_ref.TINY: 10 blocks, a repeated block in every multi-block stage, both kernel sizes, both strides, an expansion-1
stage; its stride-2 depthwise layers sit behind ZeroPad2d((0, 1, 0, 1)) / ((1, 2, 1, 2)), which is TensorFlow-SAME padding for even
planes.  Recorded: three smooth 64 x 96 frames, the four tapped hidden states and the output of encoder.top_conv (a forward hook: before
top_bn) in fp32, the fp16-rounded weights that produced them (under transformers' names) and the library versions.

`hf_to_geffnet` maps transformers' key names to geffnet's, which the specification and the product use; the tests import it from here.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 7
WIDTH, DEPTH, HIDDEN = 0.5, 0.35, 640
REPEATS = (1, 1, 1, 2, 2, 2, 1)   # ceil(0.35 * (1, 2, 2, 3, 3, 4, 1)): the blocks per stage of the tiny encoder
TAPS_HIDDEN = (1, 2, 3, 7)        # hidden_states[k]: the output of the k-th block, 1-based (0 is the stem): the last blocks of stages 0, 1, 2, 4


def hf_to_geffnet(name: str, repeats=REPEATS):
    """transformers' EfficientNetModel key -> geffnet's key under encoder.original_model (None for what the detector never runs)."""
    e = "encoder.original_model."
    if name.startswith("embeddings.convolution."):
        return e + "conv_stem." + name.rsplit(".", 1)[1]
    if name.startswith("embeddings.batchnorm."):
        return e + "bn1." + name.rsplit(".", 1)[1]
    if name.startswith("encoder.top_conv."):
        return e + "conv_head." + name.rsplit(".", 1)[1]
    if name.startswith("encoder.top_bn."):
        return None
    parts = name.split(".")
    assert parts[0] == "encoder" and parts[1] == "blocks", name
    idx, stage = int(parts[2]), 0
    while idx >= repeats[stage]:
        idx -= repeats[stage]
        stage += 1
    sep = stage == 0   # expansion 1: geffnet's DepthwiseSeparableConv
    module, leaf = ".".join(parts[3:-1]), parts[-1]
    table = {"expansion.expand_conv": "conv_pw", "expansion.expand_bn": "bn1",
             "depthwise_conv.depthwise_conv": "conv_dw", "depthwise_conv.depthwise_norm": "bn1" if sep else "bn2",
             "squeeze_excite.reduce": "se.conv_reduce", "squeeze_excite.expand": "se.conv_expand",
             "projection.project_conv": "conv_pw" if sep else "conv_pwl", "projection.project_bn": "bn2" if sep else "bn3"}
    return f"{e}blocks.{stage}.{idx}.{table[module]}.{leaf}"


def frames() -> np.ndarray:
    """Three smooth 64 x 96 RGB frames."""
    yy, xx = np.mgrid[0:64, 0:96].astype(np.float64)
    out = []
    for i in range(3):
        chans = [127.5 + 110.0 * np.sin(0.05 * (i + 1) * xx + 0.07 * (c + 1) * yy + 0.9 * c + i) * np.cos(0.03 * (c + 2) * xx - 0.04 * yy) for c in range(3)]
        out.append(np.stack(chans, -1))
    return np.clip(np.rint(np.stack(out)), 0, 255).astype(np.uint8)


def main():
    import transformers
    from transformers import EfficientNetConfig, EfficientNetModel
    sys.path.insert(0, os.path.dirname(HERE))
    import normalbae_ref as ref

    torch.manual_seed(SEED)
    cfg = EfficientNetConfig(width_coefficient=WIDTH, depth_coefficient=DEPTH, hidden_dim=HIDDEN)
    model = EfficientNetModel(cfg).eval()
    g = torch.Generator().manual_seed(SEED)
    sd = model.state_dict()
    for k, v in sd.items():   # non-trivial BatchNorm statistics and affine terms; every tensor rounded to fp16
        if k.endswith("running_var"):
            v.copy_(0.6 + 0.8 * torch.rand(v.shape, generator=g))
        elif k.endswith("running_mean"):
            v.copy_(0.2 * torch.randn(v.shape, generator=g))
        elif v.dim() == 1 and v.dtype.is_floating_point and ("bn" in k or "norm" in k):
            v.copy_((0.8 + 0.4 * torch.rand(v.shape, generator=g)) if k.endswith("weight") else 0.2 * torch.randn(v.shape, generator=g))
        elif v.dim() == 4:      # (the library's initialisation makes activations vanish through ten blocks)
            fan_in = v.shape[1] * v.shape[2] * v.shape[3]
            v.copy_(torch.randn(v.shape, generator=g) * (2.0 / fan_in) ** 0.5)
        if v.dtype.is_floating_point:
            v.copy_(v.half().float())
    model.load_state_dict(sd)
    fr = frames()
    x = ref.preprocess(fr)
    top = []
    hook = model.encoder.top_conv.register_forward_hook(lambda m, i, o: top.append(o.detach()))
    with torch.no_grad():
        hs = model(pixel_values=x, output_hidden_states=True).hidden_states
    hook.remove()
    out = {"frames": fr, "versions": np.array([f"transformers {transformers.__version__}", f"torch {torch.__version__}", f"numpy {np.__version__}"])}
    for i, k in enumerate(TAPS_HIDDEN):
        out[f"tap{i}"] = hs[k].numpy().astype(np.float32)
    out["tap4"] = top[0].numpy().astype(np.float32)
    path = os.path.join(HERE, "normalbae_tiny.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items() if k.startswith("tap")})
    # the weights in two files (random fp16 does not compress; a committed file stays below 1 MiB): the blocks of stages 0 .. 5, the rest
    halves = ({}, {})
    for k, v in sd.items():
        if v.dtype.is_floating_point and hf_to_geffnet(k) is not None:
            late = k.startswith("encoder.top_conv") or (k.startswith("encoder.blocks.") and int(k.split(".")[2]) >= sum(REPEATS[:6]))
            halves[int(late)]["w:" + k] = v.numpy().astype(np.float16)
    for i, half in enumerate(halves):
        path = os.path.join(HERE, f"normalbae_tiny_w{i}.npz")
        np.savez_compressed(path, **half)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
