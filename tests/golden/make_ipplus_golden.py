"""IP-Adapter Plus pinned by the reference's own Resampler (modules/resampler.py) and transformers' CLIPVisionModelWithProjection
(what modules/ip_adapter.py:368-380 composes: Resampler(hidden_states[-2]) of the image and of an all-zero image).  Container only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ipplus_golden.py

Writes resampler_tiny.npz, resampler_sd15.npz, resampler_sd15_keys.json, clip_vision_hidden_tiny.npz.  The generators below
(`draw_resampler_state`, `draw_sd15_input`) are imported by the tests, which re-draw what is too large to store.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

TINY = dict(dim=128, depth=2, dim_head=64, heads=2, num_queries=16, embedding_dim=64, output_dim=96, ff_mult=2)
SD15 = dict(dim=768, depth=4, dim_head=64, heads=12, num_queries=16, embedding_dim=1280, output_dim=768, ff_mult=4)
SD15_SEED = 20260
TINY_CLIP = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=3, num_attention_heads=4, image_size=28, patch_size=14,
                 projection_dim=32, hidden_act="gelu", layer_norm_eps=1e-5)


def draw_resampler_state(shapes: dict, g: torch.Generator) -> dict:
    """A Resampler state dict drawn in the order of `shapes` (key -> shape): matrices N(0, 1 / fan_in), LayerNorm weights 1 + 0.1 N,
    every other vector 0.1 N (no LayerNorm is an identity), latents N(0, 1 / dim).  Rounded to fp16 values, kept as fp32."""
    sd = {}
    for key, shape in shapes.items():
        shape = tuple(shape)
        t = torch.randn(shape, generator=g)
        if key == "latents":
            t = t * shape[-1] ** -0.5
        elif len(shape) == 2:
            t = t * shape[1] ** -0.5
        elif key.endswith("weight"):
            t = 1 + 0.1 * t
        else:
            t = 0.1 * t
        sd[key] = t.half().float()
    return sd


def draw_sd15_input(g: torch.Generator) -> torch.Tensor:
    """The SD1.5-width input [2, 257, 1280], drawn AFTER the weights from the same generator (2.6 MB: not stored)."""
    return torch.randn(2, 257, SD15["embedding_dim"], generator=g).half().float()


def checksum(tensors) -> float:
    return float(sum(t.double().abs().sum() for t in tensors))


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    import _refstub

    _refstub.install()
    from modules.resampler import Resampler  # (reference)
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection

    torch.manual_seed(0)
    # ---- the tiny CLIP vision encoder: all hidden states
    clip = CLIPVisionModelWithProjection(CLIPVisionConfig(**TINY_CLIP)).eval()
    g = torch.Generator().manual_seed(7)
    csd = {}
    for k, v in clip.state_dict().items():
        if not v.dtype.is_floating_point:
            continue
        t = torch.randn(v.shape, generator=g)
        if v.dim() == 1:
            t = (1 + 0.1 * t) if ("norm" in k and k.endswith("weight")) else 0.1 * t
        else:
            t = t * (v[0].numel() ** -0.5)
        csd[k] = t.half().float()
    clip.load_state_dict(csd, strict=False)
    px = torch.randn(1, 3, 28, 28, generator=g).half().float()
    with torch.no_grad():
        hs = clip(px, output_hidden_states=True).hidden_states
        hs0 = clip(torch.zeros_like(px), output_hidden_states=True).hidden_states
    assert len(hs) == 4

    # ---- the tiny Resampler: weights stored (fp16 values)
    ref = Resampler(**TINY).eval()
    g = torch.Generator().manual_seed(11)
    tsd = draw_resampler_state({k: v.shape for k, v in ref.state_dict().items()}, g)
    ref.load_state_dict(tsd)
    x = torch.randn(2, 257, 64, generator=g).half().float()
    with torch.no_grad():
        y = ref(x)
        y_small = ref(hs[-2])
        tokens, uncond = ref(hs[-2]), ref(hs0[-2])
    np.savez_compressed(os.path.join(HERE, "resampler_tiny.npz"), x=x.numpy().astype(np.float16), y=y.numpy(),
                        x_small=hs[-2].numpy(), y_small=y_small.numpy(), **{"w." + k: v.numpy().astype(np.float16) for k, v in tsd.items()})
    # keys of transformers 4.x checkpoints ("vision_model." prefix), whatever the installed version writes
    np.savez_compressed(os.path.join(HERE, "clip_vision_hidden_tiny.npz"), pixel_values=px.numpy(),
                        **{f"hidden_states.{i}": h.numpy() for i, h in enumerate(hs)}, tokens=tokens.numpy(), uncond=uncond.numpy(),
                        **{"w." + (k if k.startswith(("vision_model.", "visual_projection.")) else "vision_model." + k): v.numpy() for k, v in csd.items()})

    # ---- SD1.5 width: weights and input re-drawn by the test
    ref = Resampler(**SD15).eval()
    shapes = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    g = torch.Generator().manual_seed(SD15_SEED)
    sd = draw_resampler_state(shapes, g)
    ref.load_state_dict(sd)
    x = draw_sd15_input(g)
    with torch.no_grad():
        y = ref(x)
        y64 = ref.double()(x.double()).float()
    print("fp32 vs fp64 rel", float((y - y64).norm() / y64.norm()))  # (the stored fp32 reference's own error: ~1e-6)
    np.savez_compressed(os.path.join(HERE, "resampler_sd15.npz"), y=y.numpy(), weight_seed=SD15_SEED, checksum=checksum(list(sd.values()) + [x]))
    with open(os.path.join(HERE, "resampler_sd15_keys.json"), "w") as fh:
        json.dump({k: list(v) for k, v in shapes.items()}, fh, indent=0)
    for f in ("resampler_tiny.npz", "resampler_sd15.npz", "resampler_sd15_keys.json", "clip_vision_hidden_tiny.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)))
