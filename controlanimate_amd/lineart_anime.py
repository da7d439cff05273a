"""The lineart_anime annotator (every sample config of the reference lists lllyasviel/control_v11p_sd15s2_lineart_anime, whose control
frames come from controlnet_aux's LineartAnimeDetector, modules/controlresiduals_pipeline.py:59, 119-123) on the GPU, for a whole
window of frames at once.

The network is the pix2pix UnetGenerator(3, 1, num_downs=8, ngf=64, norm_layer=InstanceNorm2d(affine=False), use_dropout=False):
32 tensors and 54,405,505 parameters, channels c = [64, 128, 256, 512, 512, 512, 512, 512] at 1/2 .. 1/256 of the frame.  With
down_i = Conv2d(c[i-1], c[i], 4, stride 2, padding 1), up_i = ConvTranspose2d(., c[i-1], 4, stride 2, padding 1) and IN =
InstanceNorm2d(eps=1e-5), written out with its in-place activations (the skip tensor that is concatenated has been through the
child's LeakyReLU and then the parent's ReLU):

    d_0 = down_0(img / 127.5 - 1) + bias                                     (no norm)
    d_i = IN(down_i(LeakyReLU(0.2)(d_{i-1})))   i = 1 .. 6,     d_7 = down_7(LeakyReLU(d_6)) + bias   (no norm: a 1x1 plane at 256 x 256)
    u_7 = IN(up_7(ReLU(d_7))),   u_i = IN(up_i(cat(ReLU(d_i), ReLU(u_{i+1}))))   i = 6 .. 1
    pre-tanh = up_0(cat(ReLU(d_0), ReLU(u_1))) + bias                           (128 -> 1)

Storage convention: every activation is stored in the form its consumers read, so no MFMA operand path applies an activation.
Level i keeps L_i = LeakyReLU(d_i), contiguous, for the next convolution down, and a concatenation buffer C_i [n, h_i, w_i, 2 c_i]
whose first half is ReLU(d_i) and whose second half is ReLU(u_{i+1}); the kernel that produces d_i writes both forms in one pass, and
the transposed convolution reads one contiguous K = 2 c_i.  It runs as (the names are the keys of `timings`, the numbers the stages of
that name per pass):

    conv_in   1   ca_lanime_conv_in: uint8 frames -> d_0 at 64 channels as L_0 and the first half of C_0; the zero padding lies in the
                  normalised image (MFMA, K = 48 in 64)
    conv      7   kernels.conv4x4s2: ca_conv4x4s2, an implicit GEMM on the MFMA from an LDS halo tile, where the level has 4096 output
                  rows or more (levels 1 .. 4 of a 16-frame window of 512 x 768); below that the level is bound by its 8 MB of weights
                  and runs as ca_im2col4x4s2 (a gather of at most 64 MB) + ca_gemm with split-K; bias + ReLU in the epilogue of the
                  innermost one
    instnorm  13  ca_instnorm_act: six on the way down (two outputs: L_i and the first half of C_i), seven on the way up (one output:
                  the second half of C_{i-1}); one launch for planes of one chunk of pixels (the innermost levels), else statistics + apply
    convt     7   ca_convt4x4s2: four 2x2 phase convolutions in one launch, no zero-stuffed and no tap tensor
    conv_out  1   ca_lanime_conv_out: 128 -> 1 transposed convolution + bias on the VALU, fp32 pre-tanh values
    finish    1   ca_lanime_finish: 255 - trunc(clip(tanh * 127.5 + 127.5)) -> the uint8 map and / or the control tensor

A bias in front of a non-affine InstanceNorm cancels exactly: only three biases reach the device (down_0's, down_7's and up_0's).
No device-to-host read anywhere: the chain can be captured in a hipGraph.

The specification is tests/lineart_anime_ref.py (the fp32 torch network and the numpy detector, restated from the published code).
controlnet_aux and OpenCV are third-party packages that are absent here, and no netG.pth is available: key names and parity with
them are UNPINNED.

Scope of sizes: the reference calls the detector with detect_resolution = image_resolution = min(H, W); the detector resamples to
multiples of 256 and back.  H % 256 == 0 and W % 256 == 0 (256 x 256, 512 x 512, 512 x 768, 768 x 512, ...), for which every
resampling is the identity, is therefore the scope; anything else raises NotImplementedError.  There is no CPU fallback.
"""
from __future__ import annotations

import os

from .annotator_base import check_state_dict as _check_state_dict
from .lineart import LineartAnnotator

WEIGHTS_NAME = "netG.pth"
CHANNELS = (64, 128, 256, 512, 512, 512, 512, 512)
NUM_DOWNS = len(CHANNELS)
EPS = 1e-5
# stages per pass through the network, which is what `timings` counts: 30 stages
STAGES = {"conv_in": 1, "conv": 7, "instnorm": 13, "convt": 7, "conv_out": 1, "finish": 1}


def level_prefix(i: int) -> str:
    """The module path of level i's block: the outermost is `model`, level i = 1 .. 7 `model.model.1` + `.model.3` x (i - 1)."""
    return "model" if i == 0 else "model.model.1" + ".model.3" * (i - 1)


def conv_keys(i: int):
    """(down, up): the module paths of level i's convolution and transposed convolution."""
    p = level_prefix(i) + ".model."
    if i == 0:
        return p + "0", p + "3"
    return p + "1", p + ("3" if i == NUM_DOWNS - 1 else "5")


def lineart_anime_key_shapes() -> dict:
    """The 32 tensors of netG.pth: name -> shape (54,405,505 parameters)."""
    out = {}
    for i, c in enumerate(CHANNELS):
        down, up = conv_keys(i)
        cprev = 3 if i == 0 else CHANNELS[i - 1]
        out[down + ".weight"] = (c, cprev, 4, 4)
        out[down + ".bias"] = (c,)
        cup_in = c if i == NUM_DOWNS - 1 else 2 * c        # the innermost block has no skip below it
        cup_out = 1 if i == 0 else cprev
        out[up + ".weight"] = (cup_in, cup_out, 4, 4)      # ConvTranspose2d: [Cin, Cout, 4, 4]
        out[up + ".bias"] = (cup_out,)
    return out


def strip_module_prefix(sd) -> dict:
    """The state dict without the `module.` prefix of a DataParallel checkpoint (what the detector strips)."""
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}


def check_state_dict(sd) -> None:
    """KeyError naming a missing tensor, ValueError naming one that is unexpected or has the wrong shape."""
    _check_state_dict(sd, lineart_anime_key_shapes(), "lineart_anime", "model.model.{0,3}, and per level "
                      "model.model.1[.model.3 ...].model.{1,5} (innermost: {1,3}), each with .weight and .bias")


def pack_conv_in(w):
    """model.model.0.weight [64, 3, 4, 4] -> [64, 64] float32: column ky * 12 + kx * 3 + c, columns 48 .. 63 zero (ca_lanime_conv_in)."""
    import torch
    if tuple(w.shape) != (64, 3, 4, 4):
        raise ValueError(f"a Conv2d weight [64, 3, 4, 4] is expected, got {tuple(w.shape)}")
    return torch.nn.functional.pad(w.detach().float().permute(0, 2, 3, 1).reshape(64, 48), (0, 16)).contiguous()


def pack_conv4x4(w):
    """Conv2d weight [Cout, Cin, 4, 4] -> [Cout, 4, 4, Cin] (ca_conv4x4s2)."""
    if w.dim() != 4 or tuple(w.shape[2:]) != (4, 4):
        raise ValueError(f"a Conv2d weight [Cout, Cin, 4, 4] is expected, got {tuple(w.shape)}")
    return w.detach().permute(0, 2, 3, 1).contiguous()


def pack_convt4x4_phases(w):
    """ConvTranspose2d weight [Cin, Cout, 4, 4] -> [4, Cout, 2, 2, Cin] (ca_convt4x4s2; the layout of ca_conv_up2_phase's w_phase).
    With k = 4, stride 2 and padding 1, output pixel (2y + py, 2x + px) is a 2x2 convolution of the source: it reads source pixels
    (y + py - 1 + dy, x + px - 1 + dx), dy, dx in {0, 1}, zero outside the image, through kernel tap ky = 3 - py - 2 dy,
    kx = 3 - px - 2 dx:  out[py * 2 + px][co][dy][dx][ci] = w[ci][co][ky][kx]."""
    import torch
    if w.dim() != 4 or tuple(w.shape[2:]) != (4, 4):
        raise ValueError(f"a ConvTranspose2d weight [Cin, Cout, 4, 4] is expected, got {tuple(w.shape)}")
    cin, cout = w.shape[:2]
    out = torch.empty((4, cout, 2, 2, cin), dtype=w.dtype)
    for py in range(2):
        for px in range(2):
            for dy in range(2):
                for dx in range(2):
                    out[py * 2 + px, :, dy, dx, :] = w.detach()[:, :, 3 - py - 2 * dy, 3 - px - 2 * dx].t()
    return out.contiguous()


def cols_elems(m: int, h: int, w: int) -> int:
    """Elements of the im2col buffer that serves every chunk of 1 .. m frames of h x w pixels: kernels.conv4x4s2 picks the gather form from
    the rows of the chunk it is given, so a short last chunk can gather at a level that runs on the tile kernel at m frames.  Per level
    the largest chunk of at most m frames that still gathers counts."""
    from .kernels import CONV4X4S2_GEMM_ROWS
    need = 0
    for i in range(1, NUM_DOWNS):
        px = (h >> (i + 1)) * (w >> (i + 1))
        k = min(m, (CONV4X4S2_GEMM_ROWS - 1) // px)
        need = max(need, k * px * 16 * CHANNELS[i - 1])
    return need


class LineartAnimeAnnotator(LineartAnnotator):
    """`LineartAnimeAnnotator(weights)(image)` has the contract of `LineartAnnotator` (PIL in, PIL RGB with three equal channels out; an
    array in, an array out; `edges`, `annotate_batch(frames, out=, rep=, dtype=)`), so it plugs into
    `MultiControlNetResidualsPipeline(annotators={"lineart_anime": LineartAnimeAnnotator.from_pretrained(path)})`, whose
    `prep_control_images` then calls `annotate_batch` once per list of frames.  Nothing makes it a default: the weights are the user's
    file.  Non-uint8 input raises TypeError, frames of different sizes ValueError, sizes out of scope NotImplementedError -- all before
    the device is touched; without the library or a GPU a call raises CAHipUnavailable (there is no CPU fallback)."""

    # the largest operand of a chunk of frames (the concatenation buffer C_0 at half size: 128 channels, 64 bytes per frame pixel)
    # stays below what the kernels address
    _bytes_per_pixel = 64
    WEIGHTS_NAME = WEIGHTS_NAME

    def __init__(self, state_dict_or_path, device=None, dtype=None):
        import torch
        dtype = torch.float16 if dtype is None else dtype
        if dtype not in (torch.float16, torch.bfloat16):
            raise TypeError(f"dtype must be torch.float16 or torch.bfloat16, got {dtype}")
        self.coarse = False
        sd = self._load(state_dict_or_path) if isinstance(state_dict_or_path, (str, os.PathLike)) else state_dict_or_path
        sd = strip_module_prefix(sd)
        check_state_dict(sd)
        self.device, self.dtype = device, dtype
        keys = [conv_keys(i) for i in range(NUM_DOWNS)]
        last = NUM_DOWNS - 1
        # packed once, on the host; a bias in front of an InstanceNorm cancels: three remain
        self._host = {
            "conv_in": pack_conv_in(sd[keys[0][0] + ".weight"]).to(dtype),
            "in_b": sd[keys[0][0] + ".bias"].detach().float().contiguous(),
            "down": [pack_conv4x4(sd[keys[i][0] + ".weight"].float()).to(dtype) for i in range(1, NUM_DOWNS)],
            "inner_b": sd[keys[last][0] + ".bias"].detach().float().contiguous(),
            "up": [pack_convt4x4_phases(sd[keys[i][1] + ".weight"].float()).to(dtype) for i in range(1, NUM_DOWNS)],
            "out_w": sd[keys[0][1] + ".weight"].detach().float()[:, 0].permute(1, 2, 0).contiguous(),   # [4, 4, 128]
            "out_b": sd[keys[0][1] + ".bias"].detach().float().reshape(1).contiguous(),
        }
        self._ws = {}   # (`timings` receives events under the keys of STAGES -- tools/bench_lineart_anime.py)

    @classmethod
    def from_pretrained(cls, path, **kwargs):
        """path: a local netG.pth or a directory that holds it (no network access, ever)."""
        return cls(cls._load(path), **kwargs)

    # ---- device state ----------------------------------------------------------------------------------------------------------
    def workspace(self, n: int, h: int, w: int):
        """The buffers of a call with n frames of h x w pixels, cached per (n, h, w); contents are never assumed.  For a chunk of m
        frames: "L" [7] and "C" [7] per level 0 .. 6 (flat), "raw" (a convolution's output before its InstanceNorm), "inner"
        (ReLU(d_7 + bias)), "partials" (the InstanceNorm sums) and "pre" (float32 [n, h, w])."""
        import torch
        from . import _capi

        def make(dev):
            m = min(n, self.chunk_frames(h, w))
            lib = _capi.lib()
            px = [(h >> (i + 1)) * (w >> (i + 1)) for i in range(NUM_DOWNS)]
            floats = max(int(lib.ca_instnorm_act_partials_floats(m, h >> (i + 1), w >> (i + 1), CHANNELS[i])) for i in range(NUM_DOWNS - 1))

            def buf(elems):
                return torch.empty(elems, dtype=self.dtype, device=dev)

            cols = cols_elems(m, h, w)
            return {"cols": buf(cols) if cols else None,
                    "L": [buf(m * px[i] * CHANNELS[i]) for i in range(NUM_DOWNS - 1)],
                    "C": [buf(m * px[i] * 2 * CHANNELS[i]) for i in range(NUM_DOWNS - 1)],
                    "raw": buf(m * px[0] * CHANNELS[0]),
                    "inner": buf(m * px[-1] * CHANNELS[-1]),
                    "partials": torch.empty(floats, dtype=torch.float32, device=dev),
                    "pre": torch.empty((n, h, w), dtype=torch.float32, device=dev)}

        return self._workspace((n, h, w), make)

    # ---- input checks ----------------------------------------------------------------------------------------------------------
    def _check_size(self, h: int, w: int) -> None:
        if h < 256 or w < 256 or h % 256 or w % 256:
            raise NotImplementedError(
                f"LineartAnimeAnnotator takes frames with H % 256 == W % 256 == 0 (for which every resampling of the detector is the "
                f"identity at detect_resolution = image_resolution = min(H, W)); got {h} x {w}")

    # ---- the chain -------------------------------------------------------------------------------------------------------------
    def _network(self, src, ws, i0: int) -> None:
        """The network for the frames `src` (a chunk), pre-tanh values into ws["pre"][i0 : i0 + len(src)]."""
        from . import kernels as K
        wts = self._weights(src.device)
        n, h, w, _ = src.shape
        last = NUM_DOWNS - 1
        hs, wd = [h >> (i + 1) for i in range(NUM_DOWNS)], [w >> (i + 1) for i in range(NUM_DOWNS)]

        def view(buf, i, ch):
            return buf[: n * hs[i] * wd[i] * ch].view(n, hs[i], wd[i], ch)

        timed = self._timed
        L = [view(ws["L"][i], i, CHANNELS[i]) for i in range(last)]
        C = [view(ws["C"][i], i, 2 * CHANNELS[i]) for i in range(last)]
        timed("conv_in", K.lanime_conv_in, src, wts["conv_in"], wts["in_b"], L[0], C[0])
        for i in range(1, last):      # down: d_i -> L_i and the first half of C_i
            raw = timed("conv", K.conv4x4s2, L[i - 1], wts["down"][i - 1], out=view(ws["raw"], i, CHANNELS[i]), cols=ws["cols"])
            timed("instnorm", K.instance_norm_act, raw, [(L[i], K.IN_ACT_LEAKY, 0), (C[i], K.IN_ACT_RELU, 0)], eps=EPS, partials=ws["partials"])
        x = timed("conv", K.conv4x4s2, L[last - 1], wts["down"][last - 1], bias=wts["inner_b"], relu=True, out=view(ws["inner"], last, CHANNELS[last]),
                  cols=ws["cols"])
        for i in range(last, 0, -1):  # up: u_i -> the second half of C_{i-1}
            raw = timed("convt", K.conv_transpose4x4s2, x, wts["up"][i - 1], out=view(ws["raw"], i - 1, CHANNELS[i - 1]))
            timed("instnorm", K.instance_norm_act, raw, [(C[i - 1], K.IN_ACT_RELU, CHANNELS[i - 1])], eps=EPS, partials=ws["partials"])
            x = C[i - 1]
        timed("conv_out", K.lanime_conv_out, x, wts["out_w"], wts["out_b"], ws["pre"][i0:i0 + n])

    def _run(self, src, edges, control, rep):
        from . import kernels as K
        n, h, w, _ = src.shape
        ws = self.workspace(n, h, w)
        for i0, sl in self._chunks(n, self.chunk_frames(h, w)):
            self._network(src[sl], ws, i0)
        if edges is not None or control is not None:
            self._timed("finish", K.lanime_finish, ws["pre"], edges=edges, control=control, rep=rep)
        return ws["pre"]

    def pre_tanh(self, frames):
        """-> float32 [n, H, W] on the device: the network's output before the tanh, as a new tensor."""
        src = self._frames(frames)
        return self._run(src, None, None, 1).clone()

    logits = pre_tanh  # (the name of LineartAnnotator's surface: the values in front of the last nonlinearity)
