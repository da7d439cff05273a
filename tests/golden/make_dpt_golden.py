"""Makes tests/golden/dpt_tiny.npz from transformers' own modules (DPTForDepthEstimation, DPTImageProcessorPil, DepthEstimationPipeline)
and Pillow: the fixture that pins controlanimate_amd/depth.py and tests/depth_ref.py.  Run from the repository root:

    python tests/golden/make_dpt_golden.py

The tiny config is depth_ref.TINY_CONFIG (855,969 parameters, 37 tokens, planes 24 / 12 / 6 / 3).  The weights are seeded, scaled so that
activations stay O(1) (transformers' own initialisation with initializer_range 0.2 reaches 3e7 at the output, which fp16 cannot hold) and
rounded to fp16 BEFORE the model runs, so the stored fp16 values are exactly the weights that produced the recorded outputs.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import depth_ref as R  # noqa: E402

SEED = 3
H, W = 64, 96


def frames():
    """Three smooth uint8 frames [H, W, 3]: sums of a few low-frequency waves and a ramp."""
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for _ in range(3):
        img = np.zeros((H, W, 3))
        for c in range(3):
            for _k in range(4):
                fy, fx, ph = rng.uniform(0.5, 3.0), rng.uniform(0.5, 3.0), rng.uniform(0, 2 * np.pi)
                img[:, :, c] += rng.uniform(0.3, 1.0) * np.sin(2 * np.pi * (fy * y / H + fx * x / W) + ph)
            img[:, :, c] += rng.uniform(-1, 1) * (x / W) + rng.uniform(-1, 1) * (y / H)
        img = (img - img.min()) / (img.max() - img.min())
        out.append(np.round(img * 255).astype(np.uint8))
    return np.stack(out)


def main():
    import transformers
    import PIL
    from PIL import Image
    from transformers import DPTConfig, DPTForDepthEstimation
    from transformers.models.dpt.image_processing_pil_dpt import DPTImageProcessorPil
    from transformers.pipelines import DepthEstimationPipeline

    cfg = DPTConfig(**R.TINY_CONFIG)
    model = DPTForDepthEstimation(cfg).eval()
    sd = R.seeded_state_dict(R.TINY_CONFIG, seed=SEED)
    # a signed last layer without a bias: a part of every map is clipped to zero next to steep rises, which is where the bicubic tail
    # undershoots (seeds 0 .. 7 were tried on the CPU against the conditions asserted below)
    sd["head.head.4.weight"] = torch.randn(sd["head.head.4.weight"].shape, generator=torch.Generator().manual_seed(SEED + 100)) * 32 ** -0.5
    sd["head.head.4.bias"] = torch.zeros(1)
    sd = {k: v.half().float() for k, v in sd.items()}
    assert sorted(sd) == sorted(model.state_dict()), "depth_ref.key_shapes and the module disagree"
    assert all(tuple(sd[k].shape) == tuple(v.shape) for k, v in model.state_dict().items())
    model.load_state_dict(sd, strict=True)
    assert sum(v.numel() for v in sd.values()) == 855969

    fr = frames()
    pil = [Image.fromarray(f) for f in fr]
    out = {"frames": fr, "versions": np.array([transformers.__version__, PIL.__version__])}
    size = R.TINY_CONFIG["image_size"]
    procs = {r: DPTImageProcessorPil(size={"height": size, "width": size}, resample=r) for r in (2, 3)}
    for r, p in procs.items():
        out[f"pixel_values_r{r}"] = np.asarray(p(images=pil, return_tensors="pt")["pixel_values"], dtype=np.float32)
    proc = procs[3]
    # one frame per pass, as the pipeline runs them: the recorded values are then the very ones behind the pipeline's image (a batch of
    # three differs from three batches of one in the last bits)
    with torch.no_grad():
        res = [model(pixel_values=torch.from_numpy(out["pixel_values_r3"][i:i + 1]), output_hidden_states=True) for i in range(3)]
    out["predicted_depth"] = np.concatenate([r.predicted_depth.numpy() for r in res])
    for j, i in enumerate(cfg.backbone_out_indices):
        out[f"tap{j}"] = np.concatenate([r.hidden_states[i + 1].numpy() for r in res])
        assert np.abs(out[f"tap{j}"]).max() < 100, "a hidden state passes 100"
    out["post"] = np.stack([proc.post_process_depth_estimation(r, target_sizes=[(H, W)])[0]["predicted_depth"].numpy() for r in res])
    pipe = DepthEstimationPipeline(model=model, image_processor=proc)
    piped = [pipe(im) for im in pil]
    out["pipeline_depth"] = np.stack([np.asarray(p["depth"]) for p in piped])
    assert out["pipeline_depth"].dtype == np.uint8 and out["pipeline_depth"].shape == (3, H, W)
    assert all(np.array_equal(p["predicted_depth"].numpy(), out["post"][i]) for i, p in enumerate(piped)), "the pipeline ran other values"
    assert np.array_equal(np.stack([R.quantize_minmax(p) for p in out["post"]]), out["pipeline_depth"])

    for i in range(3):  # conditions on the fixture
        d, p = out["predicted_depth"][i], out["post"][i]
        assert d.max() > 0
        assert (d == 0).mean() <= 0.5, f"frame {i}: {(d == 0).mean():.2f} of predicted_depth is zero"
        assert len(np.unique(R.quantize_max(p)[0])) >= 100, f"frame {i}: {len(np.unique(R.quantize_max(p)[0]))} levels"
        assert (p < 0).any(), f"frame {i}: no pixel below 0 after the bicubic"
        print(f"frame {i}: max {d.max():.4f}, zero share {(d == 0).mean():.3f}, levels {len(np.unique(R.quantize_max(p)[0]))}, "
              f"below zero {(p < 0).sum()}, lowest scaled {R.scaled_max(p).min():.3f}")
    # no committed file may pass 1 MiB: the fp16 weights go into two files beside the recorded data (depth_ref.load_fixture joins them)
    parts, total = [{}, {}], sum(v.numel() for v in sd.values())
    seen = 0
    for k, v in sd.items():
        parts[0 if seen < total // 2 else 1]["w:" + k] = v.half().numpy()
        seen += v.numel()
    for name, data in (("dpt_tiny.npz", out), ("dpt_tiny_w0.npz", parts[0]), ("dpt_tiny_w1.npz", parts[1])):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **data)
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
