"""IP-Adapter Plus on the GPU: ca_perceiver_attn against fp32 torch on the same rounded operands; the Resampler against the
reference module's fixtures (tests/golden/make_ipplus_golden.py); the CLIP vision encoder's hidden states against transformers';
IPAdapterPlus.get_image_embeds end to end; the UNet and the fused cross-attention with 16 image tokens; the facade."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
DEV = "cuda:0"
SMALL = (64, 128, 256, 256)
ATTN_TOL = {torch.bfloat16: 8e-3, torch.float16: 3e-3}   # tests/test_attention_plans_gpu.py TOL
TOL = {torch.bfloat16: 2.5e-2, torch.float16: 1e-2}      # tests/test_unet_gpu.py TOL
D = 64


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm()).item()


# ---- ca_perceiver_attn -----------------------------------------------------------------------------------------------------------
class Operands:
    """q | k | v of the latents in one [B, n_l, 3 inner] buffer (the layer's GEMM), the image side as layer `layer` of an all-layers
    buffer [B, n_x, 4 * 2 * inner] (row stride 4 * 2 * inner), the output as a column slice of a wider buffer."""

    def __init__(self, batches, heads, nq, n_x, n_l, dtype, seed=3, layer=2):
        g = torch.Generator().manual_seed(seed)
        self.heads, self.inner, self.nq = heads, heads * D, nq
        inner = self.inner
        self.qkv = torch.randn(batches, max(nq, n_l), 3 * inner, generator=g).to(DEV, dtype)
        self.kvx = torch.randn(batches, n_x, 4 * 2 * inner, generator=g).to(DEV, dtype)
        self.owide = torch.zeros(batches, nq, inner + 64, device=DEV, dtype=dtype)
        self.q = self.qkv[:, :nq, :inner]
        self.lk, self.lv = self.qkv[:, :n_l, inner:2 * inner], self.qkv[:, :n_l, 2 * inner:]
        c0 = layer * 2 * inner
        self.xk, self.xv = self.kvx[:, :, c0:c0 + inner], self.kvx[:, :, c0 + inner:c0 + 2 * inner]
        self.out = self.owide[:, :, 32:32 + inner]

    def run(self):
        from controlanimate_amd import kernels as K
        self.owide.fill_(7.0)
        o = K.perceiver_attn(self.q, self.xk, self.xv, self.lk, self.lv, self.heads, out=self.out)
        torch.cuda.synchronize()
        assert bool((self.owide[:, :, :32] == 7.0).all()) and bool((self.owide[:, :, 32 + self.inner:] == 7.0).all()), "wrote outside its columns"
        return o.clone()

    def reference(self):
        b = self.q.shape[0]
        split = lambda t: t.float().view(b, t.shape[1], self.heads, D).transpose(1, 2)
        k = torch.cat([split(self.xk), split(self.lk)], 2)   # image rows, then latent rows
        v = torch.cat([split(self.xv), split(self.lv)], 2)
        p = torch.softmax(split(self.q) @ k.transpose(-1, -2) * D ** -0.5, dim=-1)
        return (p @ v).transpose(1, 2).reshape(b, self.nq, self.inner)


CASES = [(2, 12, 16, 257, 16),   # the product shape: 273 keys = 17 tiles + 1 key
         (1, 2, 16, 5, 16),      # 21 keys: fewer tiles than waves, empty partials in the merge
         (3, 2, 4, 257, 4),      # padded query rows, latent source shorter than a tile
         (1, 1, 16, 16, 16),     # both sources exactly one tile
         (1, 1, 1, 1, 1)]        # minimum


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("batches,heads,nq,n_x,n_l", CASES)
def test_perceiver_attn_against_fp32(batches, heads, nq, n_x, n_l, dtype):
    ops = Operands(batches, heads, nq, n_x, n_l, dtype)
    out = ops.run()
    r = rel(out, ops.reference())
    print(f"perceiver_attn {batches}x{heads} nq={nq} n_x={n_x} n_l={n_l} {dtype}: rel_l2 {r:.3e}")
    assert bool(torch.isfinite(out.float()).all()) and r < ATTN_TOL[dtype], r
    assert torch.equal(out, ops.run()), "two runs differ"


def _spiked(dtype):
    """The product shape with a +30 logit on the LAST key of source L for every query of every head (q_0 = 8, k_0 = 30:
    8 * 30 / sqrt(64) = 30): the last tile's maximum jumps, every partial before it is rescaled."""
    ops = Operands(2, 12, 16, 257, 16, dtype, seed=5)
    ops.q[:, :, 0::D] = 8.0
    ops.lk[:, -1, 0::D] = 30.0
    return ops


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_perceiver_attn_spike_in_the_last_latent_key(dtype):
    ops = _spiked(dtype)
    out, ref = ops.run(), ops.reference()
    r = rel(out, ref)
    print(f"spike {dtype}: rel_l2 {r:.3e}")
    assert r < ATTN_TOL[dtype], r
    # the spike dominates: the output is (nearly) that key's value row
    assert rel(out, ops.lv[:, -1:, :].expand(-1, 16, -1)) < 0.05


def test_perceiver_attn_join_order():
    """Keys and values are joined X first, then L, and stay paired: swapping two rows inside X changes nothing beyond rounding;
    giving the spiked key another source's value row changes the result to what fp32 says for THAT arrangement."""
    dtype = torch.float16
    ops = _spiked(dtype)
    base = ops.run()
    rows = ops.kvx[:, 3].clone()
    ops.kvx[:, 3] = ops.kvx[:, 200]
    ops.kvx[:, 200] = rows
    swapped = ops.run()
    assert rel(swapped, base) < ATTN_TOL[dtype] and rel(swapped, ops.reference()) < ATTN_TOL[dtype]
    v_l = ops.lv[:, -1].clone()
    ops.lv[:, -1] = ops.xv[:, 0]
    ops.xv[:, 0] = v_l
    moved, ref = ops.run(), ops.reference()
    assert rel(moved, ref) < ATTN_TOL[dtype], rel(moved, ref)
    assert rel(moved, base) > 0.5, "the value row of the spiked key did not matter"


# ---- Resampler -------------------------------------------------------------------------------------------------------------------
def _golden():
    sys.path.insert(0, G)
    import make_ipplus_golden as M
    return M


def _tiny_resampler(dtype):
    from controlanimate_amd.resampler import Resampler
    M = _golden()
    fx = np.load(os.path.join(G, "resampler_tiny.npz"))
    m = Resampler(**M.TINY)
    m.load_state_dict({k[2:]: torch.from_numpy(fx[k].astype(np.float32)) for k in fx.files if k.startswith("w.")}, strict=True)
    return m.to(DEV).prepare(DEV, dtype), fx


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_resampler_tiny_against_the_reference(dtype):
    from controlanimate_amd import kernels as K
    m, fx = _tiny_resampler(dtype)
    sink = []
    K._plan_sink = sink
    try:
        y = m(torch.from_numpy(fx["x"].astype(np.float32)).to(DEV))
    finally:
        K._plan_sink = None
    y_small = m(torch.from_numpy(fx["x_small"]).to(DEV))
    torch.cuda.synchronize()
    r, rs = rel(y, torch.from_numpy(fx["y"])), rel(y_small, torch.from_numpy(fx["y_small"]))
    print(f"resampler tiny {dtype}: [2,257,64] rel_l2 {r:.3e}, [1,5,64] rel_l2 {rs:.3e}")
    assert y.shape == (2, 16, 96) and y.dtype == dtype and r < TOL[dtype] and rs < TOL[dtype], (r, rs)
    # launches: before the first attention proj_in, ONE GEMM for the image-side K|V of all layers, the layer's own q|k|v; between two
    # attentions to_out, FF1, FF2 and the next layer's q|k|v -- no image-side K|V GEMM per layer
    at = [i for i, p in enumerate(sink) if p == "perceiver_attn"]
    assert len(at) == 2 and at[0] == 3 and at[1] - at[0] - 1 == 4, sink
    assert len(sink) == 2 + 3 + 4 + 3 + 1, sink  # ... and to_out, FF1, FF2, proj_out after the last


def test_resampler_sd15_width_against_the_reference():
    from controlanimate_amd.resampler import Resampler
    M = _golden()
    fx = np.load(os.path.join(G, "resampler_sd15.npz"))
    shapes = json.load(open(os.path.join(G, "resampler_sd15_keys.json")))
    g = torch.Generator().manual_seed(int(fx["weight_seed"]))
    sd = M.draw_resampler_state(shapes, g)
    x = M.draw_sd15_input(g)
    assert abs(M.checksum(list(sd.values()) + [x]) - float(fx["checksum"])) < 1e-6 * float(fx["checksum"]), "the generator drew other values"
    m = Resampler(**M.SD15)
    m.load_state_dict(sd, strict=True)
    y = m.to(DEV).prepare(DEV, torch.float16)(x.to(DEV))
    torch.cuda.synchronize()
    r = rel(y, torch.from_numpy(fx["y"]))
    print(f"resampler SD1.5 width fp16: rel_l2 {r:.3e}")
    assert y.shape == (2, 16, 768) and r < TOL[torch.float16], r


# ---- CLIP vision hidden states ---------------------------------------------------------------------------------------------------
def _tiny_clip(dtype=torch.float16):
    from controlanimate_amd.clip import CLIPVisionModelWithProjection
    M = _golden()
    fx = np.load(os.path.join(G, "clip_vision_hidden_tiny.npz"))
    enc = CLIPVisionModelWithProjection(**M.TINY_CLIP)
    enc.load_state_dict({k[2:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("w.")}, strict=True)
    return enc.to(DEV).prepare(DEV, dtype), fx


def test_clip_vision_hidden_states_against_transformers():
    enc, fx = _tiny_clip()
    px = torch.from_numpy(fx["pixel_values"]).to(DEV)
    out = enc(px, output_hidden_states=True)
    assert len(out.hidden_states) == 4
    assert torch.equal(out.hidden_states[-1], out.last_hidden_state)
    for i, h in enumerate(out.hidden_states):
        r = rel(h, torch.from_numpy(fx[f"hidden_states.{i}"]))
        print(f"hidden_states[{i}] rel_l2 {r:.3e}")
        assert r < 5e-3, (i, r)
    assert torch.equal(enc.penultimate_hidden_state(px), out.hidden_states[-2])
    plain = enc(px)
    assert len(plain) == 2 and plain.hidden_states is None
    assert torch.equal(plain.image_embeds, out.image_embeds) and torch.equal(plain.last_hidden_state, out.last_hidden_state)


# ---- IPAdapterPlus ---------------------------------------------------------------------------------------------------------------
class _Unet:
    config = SimpleNamespace(cross_attention_dim=96, block_out_channels=(64,))
    attn_processors = {}

    def set_attn_processor(self, procs):
        pass


def test_ip_adapter_plus_image_embeds_end_to_end_and_zero_image_cache():
    from controlanimate_amd.ip_adapter import IPAdapterPlus
    from controlanimate_amd.resampler import Resampler
    M = _golden()
    enc, fx = _tiny_clip()
    rfx = np.load(os.path.join(G, "resampler_tiny.npz"))
    ip = IPAdapterPlus(SimpleNamespace(unet=_Unet()), enc, None, DEV, num_tokens=16)
    ip.image_proj_model = Resampler(**M.TINY).to(DEV)  # (init_proj's is 12 heads of 64 at cross_attention_dim: the fixture's is smaller)
    ip.image_proj_model.load_state_dict({k[2:]: torch.from_numpy(rfx[k].astype(np.float32)) for k in rfx.files if k.startswith("w.")})
    calls = []
    embed = enc._embed
    enc._embed = lambda px: (calls.append(float(px.abs().sum())), embed(px))[1]
    states = enc.penultimate_hidden_state(torch.from_numpy(fx["pixel_values"]).to(DEV))
    calls.clear()
    tokens, uncond = ip.get_image_embeds(clip_image_embeds=states)
    torch.cuda.synchronize()
    rt, ru = rel(tokens, torch.from_numpy(fx["tokens"])), rel(uncond, torch.from_numpy(fx["uncond"]))
    print(f"IPAdapterPlus tokens rel_l2 {rt:.3e}, uncond rel_l2 {ru:.3e}")
    assert tokens.shape == uncond.shape == (1, 16, 96) and rt < 1e-2 and ru < 1e-2, (rt, ru)
    assert calls == [0.0], "one encoder pass, over the all-zero image"
    t2, u2 = ip.get_image_embeds(clip_image_embeds=states)
    assert calls == [0.0], "the zero image went through the encoder again"
    assert torch.equal(t2, tokens) and torch.equal(u2, uncond)
    enc.prepare(DEV, torch.float16)  # a new arena: the cached state belongs to the old one
    ip.get_image_embeds(clip_image_embeds=states)
    assert calls == [0.0, 0.0]
    # through the PIL path: the image's own pass, no second zero pass
    from PIL import Image
    img = Image.fromarray(np.random.default_rng(0).integers(0, 255, (40, 32, 3), dtype=np.uint8))
    t3, u3 = ip.get_image_embeds(pil_image=img)
    assert len(calls) == 3 and calls[2] > 0 and torch.equal(u3, uncond) and not torch.equal(t3, tokens)
    with pytest.raises(ValueError):
        ip.get_image_embeds(clip_image_embeds=torch.zeros(1, 64, device=DEV))


# ---- the per-step side with 16 image tokens --------------------------------------------------------------------------------------
def test_unet_with_16_image_tokens_against_the_oracle():
    """93-token context (77 text + 16 image tokens): IP processors with num_tokens = 16 on the UNet, the token-stripping processor
    with 16 on a ControlNet; UNet eps against the fp32 oracle computed here."""
    from controlanimate_amd.attention_processor import AttnProcessor2_0, CNAttnProcessor2_0, IPAttnProcessor2_0
    from controlanimate_amd.configs import controlnet_config, unet_config
    from controlanimate_amd.controlnet import ControlNetModel
    from controlanimate_amd.controlresiduals_pipeline import MultiControlNetResidualsPipeline
    from controlanimate_amd.unet import UNet3DConditionModel
    from oracle.controlnet import ControlNetConfig, controlnet_forward, init_controlnet_weights
    from oracle.unet3d import UNet3DConfig, init_unet3d_weights, unet3d_forward
    ucfg = UNet3DConfig.v2(block_out_channels=SMALL)
    uw = init_unet3d_weights(ucfg, seed=171)
    unet = UNet3DConditionModel.from_config(unet_config("v2", block_out_channels=SMALL))
    unet.load_state_dict(uw)
    unet = unet.to(DEV)
    f, h, w, nt = 4, 8, 16, 16
    g = torch.Generator().manual_seed(172)
    sample = torch.randn(1, 4, f, h, w, generator=g)
    ehs = torch.cat([torch.randn(1, 77, 768, generator=g) * 0.5, torch.randn(1, nt, 768, generator=g)], dim=1)
    assert ehs.shape[1] == 93
    hint = torch.rand(f, 3, 8 * h, 8 * w, generator=g)
    procs, ip_oracle = {}, {}
    for name in unet.attn_processors.keys():
        if "attn2" in name and "temporal_transformer" not in name:
            hidden = unet.get_submodule(name[: -len(".processor")]).to_q.out_features
            pr = IPAttnProcessor2_0(hidden_size=hidden, cross_attention_dim=768, scale=0.4, num_tokens=nt)
            pr.to_k_ip.weight.data.copy_(torch.randn(hidden, 768, generator=g) * 768 ** -0.5)
            pr.to_v_ip.weight.data.copy_(torch.randn(hidden, 768, generator=g) * 768 ** -0.5)
            procs[name] = pr
            ip_oracle[name[: -len(".processor")]] = dict(to_k_ip=pr.to_k_ip.weight.data.clone(), to_v_ip=pr.to_v_ip.weight.data.clone(),
                                                         scale=0.4, num_tokens=nt)
        else:
            procs[name] = AttnProcessor2_0()
    unet.set_attn_processor(procs)
    unet.prepare(DEV, torch.float16)
    ccfg = ControlNetConfig(block_out_channels=SMALL)
    cw = init_controlnet_weights(ccfg, seed=173)
    net = ControlNetModel.from_config(controlnet_config(block_out_channels=SMALL))
    net.load_state_dict(cw)
    net.set_attn_processor(CNAttnProcessor2_0(num_tokens=nt))
    net = net.to(DEV).prepare(DEV, torch.float16)
    with torch.no_grad():
        x2d = sample.permute(0, 2, 1, 3, 4).reshape(f, 4, h, w)
        d, m = controlnet_forward(cw, ccfg, x2d, 300, ehs.expand(f, -1, -1), hint, conditioning_scale=0.9, guess_mode=False, strip_tokens=nt)
        to5 = lambda t: t.reshape(1, f, *t.shape[1:]).permute(0, 2, 1, 3, 4)
        ref = unet3d_forward(uw, ucfg, sample, 300, ehs, down_block_additional_residuals=[to5(t) for t in d],
                             mid_block_additional_residual=to5(m), ip=ip_oracle)
    cn = MultiControlNetResidualsPipeline(["a"], [0.9], use_lcm=False, controlnets=[net], device=DEV)
    cn.prep_control_images({"a": [x for x in hint]}, do_classifier_free_guidance=False, guess_mode=False)
    down, mid = cn(sample.to(DEV), 300, ehs.to(DEV), f, do_classifier_free_guidance=False, guess_mode=False)
    out = unet(sample.to(DEV), 300, ehs.to(DEV), down_block_additional_residuals=down, mid_block_additional_residual=mid).sample
    torch.cuda.synchronize()
    r = rel(out, ref)
    print("UNet, 16 image tokens: eps rel_l2 %.3e" % r)
    assert out.shape == ref.shape and r < TOL[torch.float16], r


def test_xattn_fused_at_the_plus_shape():
    """The fused cross-attention of the 64x64-latent level with the image-prompt branch at 16 tokens: 8 images of 2048 tokens, context
    93 = 77 text + 16 image tokens; it runs as xattn_ip_out128 and meets tools/xattn_check.py's fp16 bound."""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import xattn_check as X
    from controlanimate_amd import kernels as K
    dt = torch.float16
    images, tokens, L, nk, nip, fpk, kvb, sc = 8, 2048, 93, 77, 16, 4, 2, 0.6
    x, wq, gamma, beta, kv = X.make(images, tokens, L, kvb, dt)
    kvip = X.make(images, tokens, L, kvb, dt, seed=23)[4]
    wo, bo = X.make_out(dt)
    ref = X.reference_ip(x, wq, gamma, beta, kv, kvip, images, tokens, L, nk, nip, fpk, kvb, dt, sc) @ wo.float().t() + bo[None, :] + x.float()
    sink = []
    K._plan_sink = sink
    try:
        out = X.fused_ip_out(x, wq, gamma, beta, kv, kvip, images, tokens, L, nk, nip, fpk, kvb, wo, bo, sc)
    finally:
        K._plan_sink = None
    assert out is not None, "the library did not take the launch"
    torch.cuda.synchronize()
    r = rel(out, ref)
    print(f"xattn_fused images={images} tokens={tokens} L={L} nk_ip={nip}: rel_l2 {r:.3e}")
    assert sink == ["xattn_ip_out128"], sink
    assert r < 2e-3, r


# ---- facade ----------------------------------------------------------------------------------------------------------------------
def test_facade_builds_plus_from_the_checkpoint_and_runs_a_window():
    from PIL import Image
    from test_facade_gpu import _IP_CFG, _components
    from controlanimate_amd.controlanimate_pipeline import ControlAnimatePipeline
    from controlanimate_amd.ip_adapter import IPAdapterPlus
    from controlanimate_amd.resampler import Resampler
    enc, _ = _tiny_clip()
    comps = _components()
    unet = comps["unet"]
    torch.manual_seed(2025)
    proj = Resampler(dim=768, depth=4, dim_head=64, heads=12, num_queries=16, embedding_dim=64, output_dim=768, ff_mult=4)
    ip_sd = {}
    for i, name in enumerate(k for k in unet.attn_processors if "attn2" in k):
        hidden = unet.get_submodule(name[: -len(".processor")]).to_q.out_features
        ip_sd[f"{2 * i + 1}.to_k_ip.weight"] = torch.randn(hidden, 768) * 768 ** -0.5
        ip_sd[f"{2 * i + 1}.to_v_ip.weight"] = torch.randn(hidden, 768) * 768 ** -0.5
    ckpt = {"image_proj": {k: v.clone() for k, v in proj.state_dict().items()}, "ip_adapter": ip_sd}
    cfg = dict(_IP_CFG, steps=2)
    pipe = ControlAnimatePipeline(cfg, dict(comps, image_encoder=enc, ip_adapter_ckpt=ckpt), device=DEV)
    ip = pipe.pipeline.ip_adapter
    assert isinstance(ip, IPAdapterPlus) and ip.num_tokens == 16 and isinstance(ip.image_proj_model, Resampler)
    assert torch.equal(ip.image_proj_model.latents.data.cpu(), ckpt["image_proj"]["latents"])
    assert all(p.num_tokens == 16 for p in pipe.multicontrolnetresiduals_pipeline.controlnets[0].attn_processors.values())
    assert any(b.data_ptr() == ip.image_proj_model.latents.data_ptr() for b in pipe.weight_buffers())
    # eager, ControlNet on the main stream: the Python-level calls below are then the calls of every step
    pipe.pipeline.use_hip_graph = False
    pipe.pipeline.overlap_controlnet = False
    seen = {"ctx": [], "res": []}
    cn, un = pipe.multicontrolnetresiduals_pipeline, pipe.pipeline.unet
    res_nhwc, fwd_nhwc = cn.residuals_nhwc, un.forward_nhwc

    def rec_res(x, tt, prompt, *a, **k):
        down, mid = res_nhwc(x, tt, prompt, *a, **k)
        seen["res"].append([t.clone() for t in list(down) + [mid]])
        return down, mid

    def rec_fwd(x, rep, f, tt, prompt, *a, **k):
        seen["ctx"].append(int(prompt.shape[1]))
        return fwd_nhwc(x, rep, f, tt, prompt, *a, **k)

    cn.residuals_nhwc, un.forward_nhwc = rec_res, rec_fwd
    rng = np.random.default_rng(0)
    frames = [Image.fromarray(rng.integers(0, 255, (64, 64, 3), dtype=np.uint8)) for _ in range(8)]
    prev_a = [Image.fromarray(rng.integers(0, 255, (64, 64, 3), dtype=np.uint8))]
    prev_b = [Image.fromarray(rng.integers(0, 255, (64, 64, 3), dtype=np.uint8))]
    out_a = pipe.animate(frames, prev_a, cfg)
    first_a = seen["res"][0]
    seen["res"].clear()
    out_b = pipe.animate(frames, prev_b, cfg)
    first_b = seen["res"][0]
    assert len(out_a) == 8 and seen["ctx"] and set(seen["ctx"]) == {93}, seen["ctx"]
    # only the image tokens differ between the two windows: the ControlNet strips them, its first-step residuals are the same bits
    assert all(torch.equal(a, b) for a, b in zip(first_a, first_b))
    assert not np.array_equal(np.asarray(out_a[0]), np.asarray(out_b[0])), "the image prompt did not reach the UNet"
