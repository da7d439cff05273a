"""IP-Adapter Plus without a GPU: the new C entry point is exported, bound and rejects bad arguments before any launch; the ctypes
struct equals the C layout; the Resampler's state dict is the reference module's; the facade picks the variant from the checkpoint;
the zero image tokens of a first window follow num_tokens."""
import ctypes as C
import json
import os
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "controlanimate_hip.h")
G = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def capi():
    from controlanimate_amd import _build, _capi
    _build.build(verbose=False)
    return _capi


def test_perceiver_attn_is_exported_and_bound_at_abi_16(capi):
    lib = capi.lib()
    assert "ca_perceiver_attn" in capi.SYMBOLS and hasattr(lib, "ca_perceiver_attn")
    assert "ca_perceiver_attn" in open(HEADER).read()
    assert capi.ABI_VERSION == 16 and lib.ca_abi_version() == 16
    from controlanimate_amd import _build, kernels
    assert "ca_perceiver.hip" in _build.SOURCES and callable(kernels.perceiver_attn)


def _args(capi, **over):
    fake = 0x10000  # never dereferenced on the host: validation fails first
    kw = dict(q=fake, x=fake, l=fake, o=fake, q_row=384, q_batch=16 * 384, x_row=1024, x_batch=257 * 1024, x_v_off=128, l_row=384,
              l_batch=16 * 384, l_v_off=128, o_row=128, o_batch=16 * 128, batches=2, heads=2, head_dim=64, nq=16, n_x=257, n_l=16,
              scale=0.125, dtype=1)
    kw.update(over)
    return capi.PerceiverAttnArgs(**kw)


@pytest.mark.parametrize("over", [dict(head_dim=40), dict(nq=0), dict(nq=17), dict(n_x=0), dict(n_l=0), dict(x=0x10008), dict(o=0x10002),
                                  dict(l_row=380), dict(x_batch=257 * 1024 + 4), dict(o_row=132), dict(dtype=7), dict(q=None)],
                         ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_perceiver_attn_rejects_bad_arguments_before_any_launch(capi, over):
    lib = capi.lib()
    rc = lib.ca_perceiver_attn(C.byref(_args(capi, **over)), None)
    assert rc < 0 and b"ca_perceiver_attn" in lib.ca_last_error(), (rc, lib.ca_last_error())


def test_perceiver_attn_rejects_null_args(capi):
    lib = capi.lib()
    assert lib.ca_perceiver_attn(None, None) < 0 and b"ca_perceiver_attn" in lib.ca_last_error()


def test_perceiver_attn_struct_matches_c_layout(capi):
    st, cname = capi.PerceiverAttnArgs, "ca_perceiver_attn_args"
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){", f'printf("{cname} %zu\\n", sizeof({cname}));']
    lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in st._fields_]
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-o", exe, src])
        got = dict(l.split() for l in subprocess.check_output([exe], text=True).strip().splitlines())
    assert int(got[cname]) == C.sizeof(st)
    for f, _ in st._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(st, f).offset, f


# ---- Resampler -------------------------------------------------------------------------------------------------------------------
SD15 = dict(dim=768, depth=4, dim_head=64, heads=12, num_queries=16, embedding_dim=1280, output_dim=768, ff_mult=4)
TINY = dict(dim=128, depth=2, dim_head=64, heads=2, num_queries=16, embedding_dim=64, output_dim=96, ff_mult=2)


def tiny_state():
    fx = np.load(os.path.join(G, "resampler_tiny.npz"))
    return {k[2:]: torch.from_numpy(fx[k].astype(np.float32)) for k in fx.files if k.startswith("w.")}


def test_resampler_state_dict_is_the_reference_modules():
    from controlanimate_amd.resampler import Resampler
    want = json.load(open(os.path.join(G, "resampler_sd15_keys.json")))
    got = {k: list(v.shape) for k, v in Resampler(**SD15).state_dict().items()}
    assert list(got) == list(want) and got == want
    m = Resampler(**TINY)
    sd = tiny_state()
    assert m.load_state_dict(sd, strict=True) is not None
    assert torch.equal(m.latents.data, sd["latents"]) and torch.equal(m.layers[1][1][3].weight.data, sd["layers.1.1.3.weight"])


def test_resampler_unsupported_flags_raise():
    from controlanimate_amd.resampler import Resampler
    with pytest.raises(NotImplementedError):
        Resampler(**TINY, apply_pos_emb=True)
    with pytest.raises(NotImplementedError):
        Resampler(**TINY, num_latents_mean_pooled=4)


# ---- facade ----------------------------------------------------------------------------------------------------------------------
def test_variant_follows_the_checkpoint():
    from controlanimate_amd.controlanimate_pipeline import ip_adapter_variant
    from controlanimate_amd.ip_adapter import IPAdapter, IPAdapterPlus
    plus = {"image_proj": {"latents": torch.zeros(1, 16, 768), "proj_in.weight": torch.zeros(768, 1280)}, "ip_adapter": {}}
    plain = {"image_proj": {"proj.weight": torch.zeros(4 * 768, 1024), "proj.bias": torch.zeros(4 * 768)}, "ip_adapter": {}}
    full = {"image_proj": {"proj.0.weight": torch.zeros(1280, 1280), "proj.2.weight": torch.zeros(768, 1280)}, "ip_adapter": {}}
    assert ip_adapter_variant(plus, 768) == (IPAdapterPlus, 16)
    assert ip_adapter_variant(plain, 768) == (IPAdapter, 4)
    assert ip_adapter_variant({"image_proj": {"latents": torch.zeros(1, 8, 768)}}, 768) == (IPAdapterPlus, 8)
    with pytest.raises(NotImplementedError, match="IPAdapterFull"):
        ip_adapter_variant(full, 768)
    assert issubclass(IPAdapterPlus, IPAdapter)


def _stub_pipeline(num_tokens):
    from controlanimate_amd.configs import NOISE_SCHEDULER_KWARGS
    from controlanimate_amd.controlanimation_pipeline import ControlAnimationPipeline
    from controlanimate_amd.schedulers import get_scheduler
    pipe = ControlAnimationPipeline(vae=None, text_encoder=None, tokenizer=None, unet=None, scheduler=get_scheduler("LCMScheduler", **NOISE_SCHEDULER_KWARGS))
    pipe.ip_adapter = SimpleNamespace(num_tokens=num_tokens)
    return pipe


@pytest.mark.parametrize("num_tokens", [4, 16])
def test_zero_image_tokens_of_a_first_window_follow_num_tokens(num_tokens):
    """A window without a previous frame and without a fixed image prompt: the context grows by num_tokens zero rows (the reference
    hard-codes 4, which is right for its plain adapter only)."""
    pipe = _stub_pipeline(num_tokens)
    pos, neg = torch.randn(1, 77, 768), torch.randn(1, 77, 768)
    p2, n2 = pipe._append_image_tokens(pos, neg, torch.device("cpu"), None, 0.4, {})
    assert p2.shape == n2.shape == (1, 77 + num_tokens, 768)
    assert torch.equal(p2[:, :77], pos) and torch.equal(n2[:, :77], neg)
    assert not p2[:, 77:].any() and not n2[:, 77:].any()


def test_plus_needs_the_hip_encoder():
    from controlanimate_amd.ip_adapter import IPAdapterPlus

    class _Unet:
        config = SimpleNamespace(cross_attention_dim=768, block_out_channels=(64,))
        attn_processors = {}

        def set_attn_processor(self, procs):
            pass

    pipe = SimpleNamespace(unet=_Unet())
    with pytest.raises(TypeError, match="CLIPVisionModelWithProjection"):
        IPAdapterPlus(pipe, lambda pil: torch.zeros(1, 1024), None, "cpu")
    ip = IPAdapterPlus(pipe, None, None, "cpu")
    assert ip.num_tokens == 16 and type(ip.image_proj_model).__name__ == "Resampler"
    with pytest.raises(RuntimeError, match="image_encoder"):
        ip.get_image_embeds(clip_image_embeds=torch.zeros(1, 257, 1280))
    ip.image_encoder = SimpleNamespace(penultimate_hidden_state=None, config=SimpleNamespace(image_size=224), arena=None)
    with pytest.raises(ValueError, match="penultimate hidden states"):
        ip.get_image_embeds(clip_image_embeds=torch.zeros(1, 1024))
