"""Writes tests/golden/retinaface_body_tiny.npz: the pin of the face detector's body arithmetic against transformers.

    python tests/golden/make_retinaface_golden.py

transformers' ResNetModel at ResNetConfig(layer_type="bottleneck", downsample_in_bottleneck=False, depths=[3, 4, 6, 3]) is torchvision's
ResNet v1.5: the stride on the 3x3 convolution of a bottleneck, a 1x1 convolution of the block's stride plus BatchNorm as the shortcut, a
7x7 stride-2 stem and a 3x3 stride-2 max pool with padding 1.  The widths are the smallest the device chain accepts (stem 8, layers 32, 64,
128, 256: every inner width a multiple of 8).  Recorded: three smooth 64 x 96 frames, the outputs of stages 2, 3 and 4 (what RetinaFace taps
behind layer2, layer3 and layer4) in fp32, the fp16-rounded weights that produced them under facexlib's `body.` names, and the library
versions.  Random fp16 does not compress, so the widths also keep the file below 1 MiB.
"""
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 11
STEM, WIDTHS, DEPTHS = 8, (32, 64, 128, 256), (3, 4, 6, 3)


def hf_to_facexlib(name: str):
    """transformers' ResNetModel key -> facexlib's key under `body.` (None for what has no counterpart)."""
    leaf = name.rsplit(".", 1)[1]
    if leaf == "num_batches_tracked":
        return None
    if name.startswith("embedder.embedder.convolution."):
        return "body.conv1." + leaf
    if name.startswith("embedder.embedder.normalization."):
        return "body.bn1." + leaf
    m = re.match(r"encoder\.stages\.(\d+)\.layers\.(\d+)\.(shortcut|layer\.(\d+))\.(convolution|normalization)\.", name)
    assert m, name
    p = f"body.layer{int(m.group(1)) + 1}.{m.group(2)}."
    if m.group(3) == "shortcut":
        return p + ("downsample.0." if m.group(5) == "convolution" else "downsample.1.") + leaf
    return p + ("conv" if m.group(5) == "convolution" else "bn") + str(int(m.group(4)) + 1) + "." + leaf


def frames() -> np.ndarray:
    """Three smooth 64 x 96 RGB frames."""
    yy, xx = np.mgrid[0:64, 0:96].astype(np.float64)
    out = []
    for i in range(3):
        chans = [127.5 + 110.0 * np.sin(0.06 * (i + 1) * xx + 0.05 * (c + 1) * yy + 0.7 * c + i) * np.cos(0.04 * (c + 2) * xx - 0.03 * yy) for c in range(3)]
        out.append(np.stack(chans, -1))
    return np.clip(np.rint(np.stack(out)), 0, 255).astype(np.uint8)


def main():
    import transformers
    from transformers import ResNetConfig, ResNetModel
    sys.path.insert(0, os.path.dirname(HERE))
    import retinaface_ref as ref

    torch.manual_seed(SEED)
    cfg = ResNetConfig(num_channels=3, embedding_size=STEM, hidden_sizes=list(WIDTHS), depths=list(DEPTHS), layer_type="bottleneck", hidden_act="relu",
                       downsample_in_first_stage=False, downsample_in_bottleneck=False)
    model = ResNetModel(cfg).eval()
    g = torch.Generator().manual_seed(SEED)
    sd = model.state_dict()
    for k, v in sd.items():   # non-trivial BatchNorm statistics and affine terms; every tensor rounded to fp16
        if k.endswith("running_var"):
            v.copy_(0.6 + 0.8 * torch.rand(v.shape, generator=g))
        elif k.endswith("running_mean"):
            v.copy_(0.2 * torch.randn(v.shape, generator=g))
        elif v.dim() == 1 and v.dtype.is_floating_point:
            v.copy_((0.8 + 0.4 * torch.rand(v.shape, generator=g)) if k.endswith("weight") else 0.2 * torch.randn(v.shape, generator=g))
            if k.endswith("layer.2.normalization.weight"):
                v.mul_(0.5)   # (the residual sum would otherwise double the variance per block)
        elif v.dim() == 4:
            fan_in = v.shape[1] * v.shape[2] * v.shape[3]
            v.copy_(torch.randn(v.shape, generator=g) * (2.0 / fan_in) ** 0.5)
            if k.startswith("embedder."):
                v.div_(64.0)   # (the input is bytes minus a mean: of the order of 100)
        if v.dtype.is_floating_point:
            v.copy_(v.half().float())
    model.load_state_dict(sd)
    fr = frames()
    with torch.no_grad():
        hs = model(pixel_values=ref.preprocess(fr), output_hidden_states=True).hidden_states
    out = {"frames": fr, "versions": np.array([f"transformers {transformers.__version__}", f"torch {torch.__version__}", f"numpy {np.__version__}"])}
    for i in range(3):
        out[f"tap{i}"] = hs[i + 2].numpy().astype(np.float32)
    for k, v in sd.items():
        name = hf_to_facexlib(k)
        if name is not None:
            out["w:" + name] = v.numpy().astype(np.float16)
    path = os.path.join(HERE, "retinaface_body_tiny.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items() if k.startswith("tap")}, [float(np.abs(out[f"tap{i}"]).mean()) for i in range(3)])


if __name__ == "__main__":
    main()
