"""The lineart annotator of the reference's IP-Adapter sample config (configs/prompts/SampleConfigIPAdapter.yaml:
lllyasviel/control_v11p_sd15_lineart, whose control frames come from controlnet_aux's LineartDetector,
modules/controlresiduals_pipeline.py:60, 125-129) on the GPU, for a whole window of frames at once.

The network is the "informative drawings" Generator(3, 1, n_residual_blocks=3), 24 tensors and 4,290,945 parameters, with
IN = InstanceNorm2d(affine=False, eps=1e-5):

    model0: ReflectionPad2d(3), Conv2d(3, 64, 7), IN, ReLU
    model1: Conv2d(64, 128, 3, stride=2, padding=1), IN, ReLU, Conv2d(128, 256, 3, stride=2, padding=1), IN, ReLU
    model2: 3 x ResidualBlock: x + [ReflectionPad2d(1), Conv2d(256, 256, 3), IN, ReLU, ReflectionPad2d(1), Conv2d(256, 256, 3), IN](x)
    model3: ConvTranspose2d(256, 128, 3, stride=2, padding=1, output_padding=1), IN, ReLU, ConvTranspose2d(128, 64, 3, 2, 1, 1), IN, ReLU
    model4: ReflectionPad2d(3), Conv2d(64, 1, 7), Sigmoid

It runs as (the names are the keys of `timings`, the numbers the stages of that name per pass):

    conv_in   1   ca_lineart_conv_in: uint8 frames -> 64 channels, reflection padding and / 255 folded in (MFMA, K = 147 in 160)
    instnorm  11  ca_instnorm_stats + ca_instnorm_apply (two launches): ReLU / residual add / reflection-padded output as the layer needs
    conv      8   ca_conv3x3: the two stride-2 convolutions, and the six 256 -> 256 convolutions on tensors the InstanceNorm before
                  them wrote reflection-padded by one pixel -- the zero-padded convolution of the padded tensor is right in its interior,
                  and the InstanceNorm after it ignores the ring
    convt     2   one ca_gemm with N = 9 * Cout (every tap of every input pixel) + ca_convt3x3s2_gather (the sum per output phase)
    conv_out  1   ca_lineart_conv_out: 64 -> 1, 7x7 behind reflection padding, fp32 logits
    finish    1   ca_lineart_finish: 255 - trunc(sigmoid * 255) -> the uint8 map and / or the control tensor the ControlNets hold

A bias in front of a non-affine InstanceNorm cancels exactly: only model4.1.bias reaches the device.  No device-to-host read
anywhere: the chain can be captured in a hipGraph.

The specification is tests/lineart_ref.py (the fp32 torch network and the numpy detector, restated from the published code).
controlnet_aux and OpenCV are third-party packages that are absent here, and no sk_model.pth is available: parity with them is
UNPINNED.  Every convolution but the last is followed by an InstanceNorm, so activations stay of order one in fp16.

Scope of sizes: the reference calls the detector with detect_resolution = image_resolution = min(H, W) on frames floored to
multiples of 64, for which both of the detector's resamplings are the identity.  H % 64 == 0 and W % 64 == 0 is therefore the
scope; anything else raises NotImplementedError.  The lineart_anime detector is a different network: lineart_anime.py.
"""
from __future__ import annotations

import os

from .annotator_base import AnnotatorBase, check_state_dict as _check_state_dict, load_state_dict, pack_conv

WEIGHTS_NAME,WEIGHTS_NAME_COARSE = "sk_model.pth", "sk_model2.pth"
N_RES_BLOCKS = 3
EPS = 1e-5
# stages per pass through the network, which is what `timings` counts: 24 stages, 37 launches (an InstanceNorm is two launches, a
# transposed convolution a GEMM and a gather)
STAGES = {"conv_in": 1, "instnorm": 11, "conv": 8, "convt": 2, "conv_out": 1, "finish": 1}


def lineart_key_shapes() -> dict:
    """The 24 tensors of sk_model.pth / sk_model2.pth: name -> shape (4,290,945 parameters)."""
    convs = {"model0.1": (64, 3, 7, 7), "model1.0": (128, 64, 3, 3), "model1.3": (256, 128, 3, 3)}
    for b in range(N_RES_BLOCKS):
        convs[f"model2.{b}.conv_block.1"] = (256, 256, 3, 3)
        convs[f"model2.{b}.conv_block.5"] = (256, 256, 3, 3)
    convs["model3.0"] = (256, 128, 3, 3)  # ConvTranspose2d: [Cin, Cout, 3, 3]
    convs["model3.3"] = (128, 64, 3, 3)
    convs["model4.1"] = (1, 64, 7, 7)
    out = {}
    for k, shape in convs.items():
        out[k + ".weight"] = shape
        out[k + ".bias"] = (shape[1] if k.startswith("model3.") else shape[0],)
    return out


def check_state_dict(sd) -> None:
    """KeyError naming a missing tensor, ValueError naming one that is unexpected or has the wrong shape."""
    _check_state_dict(sd, lineart_key_shapes(), "lineart",
                      "model0.1, model1.{0,3}, model2.{0,1,2}.conv_block.{1,5}, model3.{0,3}, model4.1, each with .weight and .bias")


def pack_conv_in(w):
    """model0.1.weight [64, 3, 7, 7] -> [64, 160] float32: column ky * 21 + kx * 3 + c, columns 147 .. 159 zero (ca_lineart_conv_in)."""
    import torch
    return torch.nn.functional.pad(w.detach().float().permute(0, 2, 3, 1).reshape(64, 147), (0, 13)).contiguous()


def pack_convt_phases(w):
    """ConvTranspose2d weight [Cin, Cout, 3, 3] -> [3, 3, Cout, Cin]: W[ky][kx] as the [Cout, Cin] matrix of one tap.  With
    k = 3, stride 2, padding 1, output_padding 1 and x[H] = x[.][W] = 0 the four output phases are
        out[2i, 2j]     = W[1][1] x[i, j]
        out[2i, 2j+1]   = W[1][2] x[i, j] + W[1][0] x[i, j+1]
        out[2i+1, 2j]   = W[2][1] x[i, j] + W[0][1] x[i+1, j]
        out[2i+1, 2j+1] = W[2][2] x[i, j] + W[2][0] x[i, j+1] + W[0][2] x[i+1, j] + W[0][0] x[i+1, j+1]
    -- viewed as [9 * Cout, Cin] it is the weight of the one GEMM that computes every tap (kernels.conv_transpose3x3s2)."""
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise ValueError(f"a ConvTranspose2d weight [Cin, Cout, 3, 3] is expected, got {tuple(w.shape)}")
    return w.detach().permute(2, 3, 1, 0).contiguous()


class LineartAnnotator(AnnotatorBase):
    """`LineartAnnotator(weights)(image)` has the contract of `annotators.canny(image)` (PIL in, PIL RGB with three equal channels
    out; an array in, an array out), so it plugs into `MultiControlNetResidualsPipeline(annotators={"lineart":
    LineartAnnotator.from_pretrained(path)})`, whose `prep_control_images` then calls `annotate_batch` once per list of frames.
    Nothing makes it a default: the weights are the user's file.  Non-uint8 input raises TypeError, frames of different sizes
    ValueError, sizes out of scope NotImplementedError -- all before the device is touched; without the library or a GPU a call
    raises CAHipUnavailable (there is no CPU fallback)."""

    # the largest operand of a chunk of frames (the 9 x 64 taps of the second transposed convolution at half size: 288 bytes per
    # frame pixel) stays below what the GEMM and convolution kernels address with 32-bit byte offsets
    _bytes_per_pixel = 288
    WEIGHTS_NAME = WEIGHTS_NAME

    def __init__(self, state_dict_or_path, device=None, dtype=None, coarse: bool = False):
        import torch
        dtype = torch.float16 if dtype is None else dtype
        if dtype not in (torch.float16, torch.bfloat16):
            raise TypeError(f"dtype must be torch.float16 or torch.bfloat16, got {dtype}")
        self.coarse = bool(coarse)
        sd = self._load(state_dict_or_path, self.coarse) if isinstance(state_dict_or_path, (str, os.PathLike)) else state_dict_or_path
        check_state_dict(sd)
        self.device, self.dtype = device, dtype

        def conv(key):
            return pack_conv((sd[key + ".weight"], None), dtype)[0]

        # packed once, on the host; every bias but the last cancels in the InstanceNorm behind it
        self._host = {
            "conv_in": pack_conv_in(sd["model0.1.weight"]).to(dtype),
            "down": [conv("model1.0"), conv("model1.3")],
            "res": [(conv(f"model2.{b}.conv_block.1"), conv(f"model2.{b}.conv_block.5")) for b in range(N_RES_BLOCKS)],
            "up": [pack_convt_phases(sd["model3.0.weight"].float()).to(dtype), pack_convt_phases(sd["model3.3.weight"].float()).to(dtype)],
            "out_w": sd["model4.1.weight"].detach().float()[0].permute(1, 2, 0).contiguous(),
            "out_b": sd["model4.1.bias"].detach().float().reshape(1).contiguous(),
        }
        self._ws = {}   # (`timings` receives events under the keys of STAGES -- tools/bench_lineart.py)

    @classmethod
    def _load(cls, path, coarse: bool = False):
        return load_state_dict(path, WEIGHTS_NAME_COARSE if coarse else cls.WEIGHTS_NAME)

    @classmethod
    def from_pretrained(cls, path, coarse: bool = False, **kwargs):
        """path: a local sk_model.pth (sk_model2.pth with coarse=True) or a directory that holds it (no network access, ever)."""
        return cls(cls._load(path, coarse), coarse=coarse, **kwargs)

    # ---- device state ----------------------------------------------------------------------------------------------------------
    def workspace(self, n: int, h: int, w: int):
        """(three activation buffers for a chunk of frames, the tap buffer of the transposed convolutions, the InstanceNorm partial
        sums, the float32 logits [n, h, w]) of a call with n frames of h x w pixels, cached per (n, h, w); contents are never assumed."""
        import torch
        from . import _capi

        def make(dev):
            m = min(n, self.chunk_frames(h, w))
            lib = _capi.lib()
            floats = max(int(lib.ca_instnorm_partials_floats(m, h >> s, w >> s, c)) for s, c in ((0, 64), (1, 128), (2, 256)))
            return ([torch.empty(m * h * w * 64, dtype=self.dtype, device=dev) for _ in range(3)],
                    torch.empty(m * h * w * 144, dtype=self.dtype, device=dev),
                    torch.empty(floats, dtype=torch.float32, device=dev),
                    torch.empty((n, h, w), dtype=torch.float32, device=dev))

        return self._workspace((n, h, w), make)

    # ---- input checks ----------------------------------------------------------------------------------------------------------
    def _check_size(self, h: int, w: int) -> None:
        if h < 64 or w < 64 or h % 64 or w % 64:
            raise NotImplementedError(
                f"LineartAnnotator takes frames with H % 64 == W % 64 == 0 (what the reference produces, and for which both resamplings of "
                f"the detector are the identity at detect_resolution = image_resolution = min(H, W)); got {h} x {w}")

    # ---- the chain -------------------------------------------------------------------------------------------------------------
    def _network(self, src, ws, i0: int) -> None:
        """The network for the frames `src` (a chunk), logits into ws[3][i0 : i0 + len(src)]."""
        from . import kernels as K
        wts = self._weights(src.device)
        n, h, w, _ = src.shape
        bufs, taps, partials, logits = ws
        a, b, c = bufs

        def view(buf, hh, ww, ch):
            return buf[: n * hh * ww * ch].view(n, hh, ww, ch)

        timed = self._timed

        def norm(x, out, **kw):
            return timed("instnorm", K.instance_norm, x, out=out, partials=partials, eps=EPS, **kw)

        x = timed("conv_in", K.lineart_conv_in, src, wts["conv_in"], view(a, h, w, 64))
        x = norm(x, view(b, h, w, 64), relu=True)
        hh, ww = h, w
        for i, wt in enumerate(wts["down"]):
            hh, ww = hh // 2, ww // 2
            x = timed("conv", K.conv3x3, x, wt, stride=2, out=view(a, hh, ww, wt.shape[0]))
            last = i == len(wts["down"]) - 1  # the residual blocks take their input reflection-padded
            x = norm(x, view(b, hh + 2, ww + 2, 256) if last else view(b, hh, ww, wt.shape[0]), relu=True, out_pad=last)
        p, q, r = b, a, c  # p holds the block's input (padded), q and r are free
        for i, (w1, w2) in enumerate(wts["res"]):
            xp = view(p, hh + 2, ww + 2, 256)
            y = timed("conv", K.conv3x3, xp, w1, out=view(q, hh + 2, ww + 2, 256))
            z = norm(y, view(r, hh + 2, ww + 2, 256), relu=True, in_ring=True, out_pad=True)
            y = timed("conv", K.conv3x3, z, w2, out=view(q, hh + 2, ww + 2, 256))
            last = i == len(wts["res"]) - 1
            x = norm(y, view(r, hh, ww, 256) if last else view(r, hh + 2, ww + 2, 256), in_ring=True, residual=xp, res_ring=True, out_pad=not last)
            p, r = r, p
        for wt in wts["up"]:  # x lies in p
            cout = wt.shape[2]
            y = timed("convt", K.conv_transpose3x3s2, x, wt, taps=taps[: n * hh * ww * 9 * cout].view(n * hh * ww, 9 * cout),
                      out=view(q, 2 * hh, 2 * ww, cout))
            hh, ww = 2 * hh, 2 * ww
            x = norm(y, view(r, hh, ww, cout), relu=True)
            p, r = r, p
        timed("conv_out", K.lineart_conv_out, x, wts["out_w"], wts["out_b"], logits[i0:i0 + n])

    def _run(self, src, edges, control, rep):
        from . import kernels as K
        n, h, w, _ = src.shape
        ws = self.workspace(n, h, w)
        for i0, sl in self._chunks(n, self.chunk_frames(h, w)):
            self._network(src[sl], ws, i0)
        if edges is not None or control is not None:
            self._timed("finish", K.lineart_finish, ws[3], edges=edges, control=control, rep=rep)
        return ws[3]

    def logits(self, frames):
        """-> float32 [n, H, W] on the device: the network's output before the sigmoid, as a new tensor."""
        src = self._frames(frames)
        return self._run(src, None, None, 1).clone()

    def edges(self, frames, out=None):
        """frames: a list of PIL images / uint8 arrays of one size, or a uint8 tensor [n, H, W, C] (no host copy when it is on the
        device) -> uint8 device tensor [n, H, W] (the detector's map: dark background 0, lines up to 255), written into `out` when given."""
        return self._uint8_out(frames, out)
