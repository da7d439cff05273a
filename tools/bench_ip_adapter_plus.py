"""Times what IP-Adapter Plus adds to a window and to a denoising step, against the plain adapter, in ONE process with the repeats
alternated (every figure: median and [min, max] over --runs):

  image prompt per window   IPAdapter.get_image_embeds(pil_image): ViT-H/14 forward + ImageProjModel                  (plain)
                            IPAdapterPlus.get_image_embeds(pil_image): 31 ViT-H layers + Resampler, the zero image's state cached
                            the same with the cache dropped before every call (a second 31-layer pass per window)
  Resampler alone           [2, 257, 1280] -> [2, 16, 768]
  ca_perceiver_attn alone   2 x 12 heads, 16 queries, 257 + 16 keys (from events around 20 launches)
  UNet step                 full width, 16 frames of 64x64 latents, CFG batch 2, eager call: context 77 + 4 and 77 + 16 tokens

    python tools/bench_ip_adapter_plus.py [--runs 10] [--out profiles/ip_adapter_plus_bench.json] [--no-unet]

Weights are seeded random values at the real shapes (no checkpoint is read); times do not depend on the values."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"


def _spread(ms) -> dict:
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "runs": len(ms)}


class _NoUnet:
    """What IPAdapter needs of a pipeline when only the image prompt is timed."""
    config = SimpleNamespace(cross_attention_dim=768, block_out_channels=(320, 640, 1280, 1280))
    attn_processors: dict = {}

    def set_attn_processor(self, procs):
        pass


def full_unet(num_tokens: int):
    """The full-width UNet3D with IP processors for `num_tokens` image tokens (tests/test_workload_configs_gpu.py _full_unet)."""
    import torch
    from controlanimate_amd.configs import unet_config
    from controlanimate_amd.ip_adapter import IPAdapter
    from controlanimate_amd.unet import UNet3DConditionModel
    torch.manual_seed(0)
    with torch.device(DEV):
        unet = UNet3DConditionModel.from_config(unet_config("v2"))
    g = torch.Generator().manual_seed(1)
    for p in unet.parameters():
        if p.dim() > 1 and float(p.detach().abs().max()) == 0.0:
            p.data.copy_((torch.randn(p.shape, generator=g) * 0.02).to(DEV))
    ipa = IPAdapter(SimpleNamespace(unet=unet), None, None, DEV, num_tokens=num_tokens)
    for proc in unet.attn_processors.values():
        if hasattr(proc, "to_k_ip"):
            for lin in (proc.to_k_ip, proc.to_v_ip):
                lin.weight.data.copy_((torch.randn(lin.weight.shape, generator=g) * lin.weight.shape[1] ** -0.5).to(DEV))
    ipa.set_scale(0.4)
    return unet.prepare(DEV, torch.float16)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "ip_adapter_plus_bench.json"))
    ap.add_argument("--no-unet", action="store_true")
    a = ap.parse_args()
    import torch
    from PIL import Image
    from controlanimate_amd import kernels as K
    from controlanimate_amd.clip import CLIPVisionModelWithProjection
    from controlanimate_amd.ip_adapter import IPAdapter, IPAdapterPlus
    if not torch.cuda.is_available():
        raise SystemExit("bench_ip_adapter_plus needs the GPU: there is nothing to time without one")

    torch.manual_seed(0)
    with torch.device(DEV):
        enc = CLIPVisionModelWithProjection()  # ViT-H/14: 32 layers of 1280, 257 tokens
    enc.prepare(DEV, torch.float16)
    pipe = SimpleNamespace(unet=_NoUnet())
    plain = IPAdapter(pipe, enc, None, DEV, num_tokens=4)
    plus = IPAdapterPlus(pipe, enc, None, DEV, num_tokens=16)
    img = Image.fromarray(np.random.default_rng(0).integers(0, 255, (512, 512, 3), dtype=np.uint8))
    states = torch.randn(2, 257, 1280, device=DEV, dtype=torch.float16)
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(2, 16, 3 * 768, generator=g).to(DEV, torch.float16)
    kvx = torch.randn(2, 257, 4 * 2 * 768, generator=g).to(DEV, torch.float16)
    o = torch.empty(2, 16, 768, device=DEV, dtype=torch.float16)

    def attn20():
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(20):
            K.perceiver_attn(qkv[:, :, :768], kvx[:, :, 1536:2304], kvx[:, :, 2304:3072], qkv[:, :, 768:1536], qkv[:, :, 1536:], 12, out=o)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / 20

    def drop_cache_then_plus():
        plus._zero_state = None
        return plus.get_image_embeds(pil_image=img)

    work = {"image_prompt_plain": lambda: plain.get_image_embeds(pil_image=img),
            "image_prompt_plus_zero_cached": lambda: plus.get_image_embeds(pil_image=img),
            "image_prompt_plus_zero_not_cached": drop_cache_then_plus,
            "resampler": lambda: plus.image_proj_model(states)}
    if not a.no_unet:
        lat = torch.randn(1, 4, 16, 64, 64, device=DEV)
        for nt in (4, 16):
            unet = full_unet(nt)
            x2 = K.latents_to_nhwc(lat, unet.conv_in.cin_pad, 2, 1.0, torch.float16)  # [(2 f), h, w, 8]: the CFG halves share the latents
            ehs = torch.randn(2, 77 + nt, 768, device=DEV)
            work[f"unet_step_{nt}_image_tokens"] = (lambda u=unet, x=x2, c=ehs: u.forward_nhwc(x, 2, 16, 500, c, None, None, cfg_identical_halves=True))
    for fn in work.values():  # warm every shape: code objects, arenas, the K/V caches of the prompt
        for _ in range(2):
            fn()
    attn20()
    torch.cuda.synchronize()
    ms = {k: [] for k in work}
    attn_ms = []
    for _ in range(a.runs):  # alternated: every repeat visits every variant once
        for name, fn in work.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
        attn_ms.append(attn20())
    t0 = time.perf_counter()
    from controlanimate_amd.clip import clip_preprocess
    clip_preprocess(img, 224)
    pre_ms = (time.perf_counter() - t0) * 1e3
    result = {"device": torch.cuda.get_device_name(0), "dtype": "float16", "timing": "host clock around a call that ends in a device synchronise",
              "image": "512x512 RGB (PIL), clip_preprocess on the host included in the image_prompt_* figures",
              "host_clip_preprocess_ms": round(pre_ms, 3),
              **{k: _spread(v) for k, v in ms.items()},
              "perceiver_attn": {**_spread(attn_ms), "what": "2 x 12 heads, nq 16, 257 + 16 keys; device events around 20 launches, per launch"}}
    if not a.no_unet:
        result["unet_step"] = "full width, 16 frames, 64x64 latents, CFG batch 2, forward_nhwc without ControlNet residuals, eager (no hipGraph), per call"
        result["unet_step_16_over_4_tokens"] = round(statistics.median(ms["unet_step_16_image_tokens"]) / statistics.median(ms["unet_step_4_image_tokens"]), 4)
    result["plus_zero_cache_saves_ms"] = round(statistics.median(ms["image_prompt_plus_zero_not_cached"]) - statistics.median(ms["image_prompt_plus_zero_cached"]), 3)
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
