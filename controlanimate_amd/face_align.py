"""Face detection and alignment in front of gfpgan.FaceRestorer: the front half of facexlib's FaceRestoreHelper as GFPGANer.enhance(img,
has_aligned=False) drives it (modules/upscaler.py:53-70 of the reference) -- detect, filter, fit, warp -- for a whole window, ending in the
`[faces, 512, 512, 3]` uint8 tensor that `FaceRestorer.restore_aligned` takes and the affine matrices a paste-back needs.  The paste-back
itself (ParseNet, the mask blur, the inverse warp, the blend) is built, opt-in and UNPINNED, in face_paste.py: `FaceHelper(aligner,
paster=FacePaster(...))`; without a paster `FaceHelper.paste_faces_to_input_image` raises as before.

    network  RetinaFace(network_name='resnet50', phase='test'): torchvision's ResNet-50 v1.5 (taps behind layer2 / 3 / 4), an FPN to 256
             channels, three SSH modules, a class / box / landmark head per level; (byte - (104, 117, 123)) in, no resize
    decode   priors from min_sizes [[16, 32], [64, 128], [256, 512]] at steps [8, 16, 32], variances [0.1, 0.2]; score > conf_threshold;
             py_cpu_nms at nms_threshold; the eye-distance filter, only_keep_largest / only_center_face
    fit      the 5 landmarks onto the 512 x 512 template, then cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT (135, 133, 132))

It runs as (the names are the keys of `FaceAligner.timings`; launches per pass of a chunk of frames at the full width):

    stem     1    ca_rface_stem: the 7x7 stride-2 convolution from the byte frame on the MFMA (K = 147 gathered from an LDS tile), mean
                  subtraction, folded BatchNorm and ReLU
    body     56   ca_maxpool3x3s2; per bottleneck ca_gemm (1x1, ReLU), ca_conv3x3 (its stride, ReLU), ca_gemm (1x1, the identity as the
                  residual, ReLU: the epilogue adds the residual before the activation); the first block of a layer also ca_gemm for the
                  shortcut, behind ca_subsample2 where the stride is 2
    fpn_ssh  28   ca_gemm x 3 (output1 .. 3), ca_add_up2 + ca_conv3x3 x 2 (the top-down sums and merge2 / merge1); per level five ca_conv3x3
                  with CA_ACT_RELU (relu(cat) = cat(relu): the concatenation's ReLU sits in each branch's epilogue) and two ca_copy_cols
    heads    3    ca_gemm per level, N = 32 (4 class | 8 box | 20 landmark columns), two sources ([3X3] and [5X5_2 | 7x7_3]), fp32 output
    decode   2    ca_rface_decode (one launch per window, one block per frame), ca_face_align
    warp     1    ca_face_warp: max_faces slots per frame, an empty slot holds the border value

ca_conv3x3 takes dense operands (ca_conv_args has no row stride), so an SSH branch cannot write straight into a column range of the
256-wide concatenation: the two narrow branches are copied into one 128-wide buffer (ca_copy_cols) and the heads' GEMM reads [3X3] and that
buffer as its two sources.  No concatenation of 256 columns is ever written.

UNPINNED.  The specification is tests/retinaface_ref.py, restated from memory of facexlib's published code and of OpenCV's warpAffine:
facexlib, torchvision and OpenCV are absent here and no detection_Resnet50_Final.pth is available.  The one pinned part is the body's
arithmetic, against transformers' ResNetModel (tests/golden/retinaface_body_tiny.npz).  Two DELIBERATE DEVIATIONS: (1) the fit is the
closed-form least-squares 4-parameter similarity over all five points, float64, where facexlib calls cv2.estimateAffinePartial2D(method=
cv2.LMEDS), a seeded random search that cannot be restated; (2) exact score ties go to the lower prior index, where numpy's unstable argsort
decides in facexlib.  The reference runs the detector in fp32 (half=False); this runs fp16 / bf16 activations, so a face whose score sits at
conf_threshold can fall on either side.  The range of fp16 activations on the trained checkpoint is unmeasured; dtype=torch.bfloat16 is the escape.

Caps and their overflow bits (`overflow [n]`): OVERFLOW_CAND -- more than 1024 candidates above conf_threshold in a frame, the best by
(score, lower prior index) enter the NMS; OVERFLOW_FACES -- more faces than max_faces, the first max_faces in NMS order are taken.

Scope: frame sides that are multiples of 32 (every level's map is then exactly half of the finer one); no CPU fallback (CAHipUnavailable).
"""
from __future__ import annotations

import os
from typing import NamedTuple

import numpy as np

from . import annotator_base as _base
from .annotator_base import FrameIntake, PackedNetwork, bn_key_shapes as _bn, check_state_dict as _check_state_dict, pack_conv, pack_pointwise

WEIGHTS_NAME = "detection_Resnet50_Final.pth"
STAGES = ("stem", "body", "fpn_ssh", "heads", "decode", "warp")
LAYERS = (3, 4, 6, 3)
STEPS = (8, 16, 32)
BN_EPS = 1e-5
FACE_SIZE, HEAD_COLS, DET_COLS, MAX_CAND = 512, 32, 15, 1024
OVERFLOW_CAND, OVERFLOW_FACES = 1, 2
FLAG_CENTER, FLAG_LARGEST = 1, 2
SSH_CONVS = ("conv3X3", "conv5X5_1", "conv5X5_2", "conv7X7_2", "conv7x7_3")
HEADS = (("ClassHead", 2), ("BboxHead", 4), ("LandmarkHead", 10))


class Geometry(NamedTuple):
    stem: int            # conv1's width
    widths: tuple        # the outputs of layer1 .. layer4 (a bottleneck's inner width is a quarter)
    out_channels: int    # the FPN's and the SSH modules' width


RESNET50 = Geometry(64, (256, 512, 1024, 2048), 256)


def leaky_slope(out_channels: int) -> float:
    """facexlib's rule for the FPN and SSH modules: LeakyReLU(0.1) at out_channels <= 64, else slope 0 (a ReLU)."""
    return 0.1 if out_channels <= 64 else 0.0


def check_geometry(geo) -> None:
    if leaky_slope(geo.out_channels) != 0.0:
        raise NotImplementedError(f"out_channels={geo.out_channels}: facexlib's LeakyReLU has slope 0.1 at out_channels <= 64; only slope 0 (a ReLU) is built")
    ok = (len(geo.widths) == 4 and 8 <= geo.stem <= 64 and geo.stem % 8 == 0 and all(w >= 32 and w % 32 == 0 for w in geo.widths)
          and geo.out_channels % 32 == 0)
    if not ok:
        raise ValueError(f"geometry out of the kernels' range (stem a multiple of 8 in 8 .. 64, four layer widths and out_channels multiples of 32): {geo}")


def blocks_of(geo):
    """[(layer 1 .. 4, block, cin, inner width, cout, stride)]: the stride sits on the block's 3x3 convolution and on its shortcut."""
    out, cin = [], geo.stem
    for li, (blocks, width) in enumerate(zip(LAYERS, geo.widths), start=1):
        for b in range(blocks):
            out.append((li, b, cin, width // 4, width, 2 if (b == 0 and li > 1) else 1))
            cin = width
    return out


def ssh_widths(geo):
    """name -> (cin, cout) of an SSH module's five convolutions."""
    c = geo.out_channels
    return {"conv3X3": (c, c // 2), "conv5X5_1": (c, c // 4), "conv5X5_2": (c // 4, c // 4), "conv7X7_2": (c // 4, c // 4), "conv7x7_3": (c // 4, c // 4)}


def retinaface_key_shapes(geo=RESNET50) -> dict:
    """Every tensor of detection_Resnet50_Final.pth that the chain uses (facexlib's names, from memory): name -> shape."""
    out = {"body.conv1.weight": (geo.stem, 3, 7, 7), **_bn("body.bn1", geo.stem)}
    for li, b, cin, mid, cout, _ in blocks_of(geo):
        p = f"body.layer{li}.{b}"
        out[f"{p}.conv1.weight"] = (mid, cin, 1, 1)
        out.update(_bn(f"{p}.bn1", mid))
        out[f"{p}.conv2.weight"] = (mid, mid, 3, 3)
        out.update(_bn(f"{p}.bn2", mid))
        out[f"{p}.conv3.weight"] = (cout, mid, 1, 1)
        out.update(_bn(f"{p}.bn3", cout))
        if b == 0:
            out[f"{p}.downsample.0.weight"] = (cout, cin, 1, 1)
            out.update(_bn(f"{p}.downsample.1", cout))
    c = geo.out_channels
    for k in (1, 2, 3):
        out[f"fpn.output{k}.0.weight"] = (c, geo.widths[k], 1, 1)
        out.update(_bn(f"fpn.output{k}.1", c))
    for k in (1, 2):
        out[f"fpn.merge{k}.0.weight"] = (c, c, 3, 3)
        out.update(_bn(f"fpn.merge{k}.1", c))
    for k in (1, 2, 3):
        for name, (ci, co) in ssh_widths(geo).items():
            out[f"ssh{k}.{name}.0.weight"] = (co, ci, 3, 3)
            out.update(_bn(f"ssh{k}.{name}.1", co))
    for name, width in HEADS:
        for k in range(3):
            out[f"{name}.{k}.conv1x1.weight"], out[f"{name}.{k}.conv1x1.bias"] = (2 * width, c, 1, 1), (2 * width,)
    return out


def strip_module_prefix(sd) -> dict:
    """The state dict without the `module.` prefix of a DataParallel checkpoint (what facexlib's loader strips)."""
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}


def _ignored(k: str) -> bool:
    # torchvision's classifier rides along in some checkpoints of the body; BatchNorm's step counter is never read
    return k.endswith("num_batches_tracked") or k.startswith("body.fc.")


def check_state_dict(sd, geo=RESNET50) -> None:
    """KeyError naming a missing tensor, ValueError naming one that is unexpected or has the wrong shape."""
    _check_state_dict(sd, retinaface_key_shapes(geo), "retinaface", "body.{conv1, bn1, layer1 .. 4}, fpn.{output1 .. 3, merge1, merge2}, ssh1 .. 3 and "
                      "ClassHead / BboxHead / LandmarkHead.{0, 1, 2}.conv1x1", ignore=_ignored)


def fold_bn(sd, conv: str, bn: str):
    """(weight, bias) in fp32 of the bias-free convolution `conv` followed by the eval-mode BatchNorm `bn`."""
    return _base.fold_bn(sd, conv, bn, BN_EPS)


def pack_stem(w, dtype):
    """conv1's weight [cout, 3, 7, 7] (BatchNorm folded, fp32) -> dtype [ceil(cout / 16) * 16, 160]: column ky * 21 + kx * 3 + channel, the
    columns from 147 on and the rows from cout on zero (ca_rface_stem's A operand)."""
    import torch
    if w.dim() != 4 or tuple(w.shape[1:]) != (3, 7, 7):
        raise ValueError(f"a Conv2d weight [cout, 3, 7, 7] is expected, got {tuple(w.shape)}")
    cout = w.shape[0]
    out = torch.zeros((-(-cout // 16) * 16, 160), dtype=torch.float32)
    out[:cout, :147] = w.detach().float().permute(0, 2, 3, 1).reshape(cout, 147)
    return out.to(dtype)


def pack_network(sd, geo, dtype) -> dict:
    """The packed weights of the chain as a tree of host tensors: BatchNorm folded in fp32, rounded once to dtype where a kernel reads dtype."""
    import torch

    def lin(name, bn):
        return pack_pointwise(fold_bn(sd, name, bn), dtype)

    def conv(name, bn):
        return pack_conv(fold_bn(sd, name, bn), dtype)

    stem = fold_bn(sd, "body.conv1", "body.bn1")
    out = {"stem": (pack_stem(stem[0], dtype), stem[1].contiguous()), "blocks": [], "ssh": [], "heads": []}
    for li, b, _, _, _, _ in blocks_of(geo):
        p = f"body.layer{li}.{b}"
        blk = {"conv1": lin(p + ".conv1", p + ".bn1"), "conv2": conv(p + ".conv2", p + ".bn2"), "conv3": lin(p + ".conv3", p + ".bn3")}
        if b == 0:
            blk["down"] = lin(p + ".downsample.0", p + ".downsample.1")
        out["blocks"].append(blk)
    out["output"] = [lin(f"fpn.output{k}.0", f"fpn.output{k}.1") for k in (1, 2, 3)]
    out["merge"] = [conv(f"fpn.merge{k}.0", f"fpn.merge{k}.1") for k in (1, 2)]
    for k in (1, 2, 3):
        out["ssh"].append({name: conv(f"ssh{k}.{name}.0", f"ssh{k}.{name}.1") for name in SSH_CONVS})
        out["heads"].append(pack_pointwise((torch.cat([sd[f"{name}.{k - 1}.conv1x1.weight"] for name, _ in HEADS]),
                                            torch.cat([sd[f"{name}.{k - 1}.conv1x1.bias"] for name, _ in HEADS])), dtype))
    return out


# ---- the head tensors' layout ------------------------------------------------------------------------------------------------------------
def level_shapes(h: int, w: int):
    return [(-(-h // s), -(-w // s)) for s in STEPS]


def pack_heads(cls, box, ldm, h: int, w: int) -> list:
    """(class logits [n, P, 2], boxes [n, P, 4], landmarks [n, P, 10]) in the priors' order -> the three level tensors [n, fh, fw, 32] that
    ca_rface_decode reads (numpy in, numpy float32 out): per cell 4 class | 8 box | 20 landmark columns, the cell's two priors behind each other."""
    cls, box, ldm = (np.asarray(t, np.float32) for t in (cls, box, ldm))
    n, out, p0 = cls.shape[0], [], 0
    for fh, fw in level_shapes(h, w):
        cells = fh * fw
        sl = slice(p0, p0 + 2 * cells)
        out.append(np.ascontiguousarray(np.concatenate([cls[:, sl].reshape(n, cells, 4), box[:, sl].reshape(n, cells, 8), ldm[:, sl].reshape(n, cells, 20)], 2)
                                        .reshape(n, fh, fw, HEAD_COLS)))
        p0 += 2 * cells
    return out


def unpack_heads(levels) -> tuple:
    """The inverse of pack_heads, for torch tensors or arrays: -> (class [n, P, 2], boxes [n, P, 4], landmarks [n, P, 10]) as numpy float32."""
    cls, box, ldm = [], [], []
    for t in levels:
        a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
        n = a.shape[0]
        a = a.reshape(n, -1, HEAD_COLS)
        cls.append(a[:, :, 0:4].reshape(n, -1, 2))
        box.append(a[:, :, 4:12].reshape(n, -1, 4))
        ldm.append(a[:, :, 12:32].reshape(n, -1, 10))
    return np.concatenate(cls, 1), np.concatenate(box, 1), np.concatenate(ldm, 1)


class FaceAligner(FrameIntake, PackedNetwork):
    """`FaceAligner.from_pretrained(path).align(frames)`: detection and alignment of the faces of a window on the HIP kernels.  Non-uint8
    input raises TypeError, frames of different sizes ValueError, sizes out of scope NotImplementedError -- all before the device is
    touched; without the library or a GPU a call raises CAHipUnavailable (there is no CPU fallback)."""

    WEIGHTS_NAME = WEIGHTS_NAME
    STAGES = STAGES

    def __init__(self, state_dict_or_path, max_faces: int = 4, conf_threshold: float = 0.97, nms_threshold: float = 0.4, eye_dist_threshold: float = 5,
                 upscale_factor: float = 1, dtype=None, device=None, geometry=RESNET50):
        import torch
        dtype = torch.float16 if dtype is None else dtype
        if dtype not in (torch.float16, torch.bfloat16):
            raise TypeError(f"dtype must be torch.float16 or torch.bfloat16, got {dtype}")
        if not 1 <= int(max_faces) <= 64:
            raise ValueError(f"max_faces={max_faces} (1 .. 64)")
        if not 0 <= conf_threshold < 1 or not 0 <= nms_threshold <= 1 or eye_dist_threshold < 0 or upscale_factor <= 0:
            raise ValueError(f"conf_threshold={conf_threshold} (0 <= . < 1), nms_threshold={nms_threshold} (0 .. 1), eye_dist_threshold={eye_dist_threshold} "
                             f"(>= 0), upscale_factor={upscale_factor} (> 0)")
        check_geometry(geometry)
        sd = self._load(state_dict_or_path) if isinstance(state_dict_or_path, (str, os.PathLike)) else state_dict_or_path
        sd = strip_module_prefix(sd)
        check_state_dict(sd, geometry)
        self.device, self.dtype, self.geometry, self.max_faces = device, dtype, geometry, int(max_faces)
        self.conf_threshold, self.nms_threshold, self.eye_dist_threshold = float(conf_threshold), float(nms_threshold), float(eye_dist_threshold)
        self.upscale_factor = float(upscale_factor)
        # the largest operand of a chunk of frames, in bytes per frame pixel: the stem's output at half size, layer1's at a quarter
        self._bytes_per_pixel = int(np.ceil(max(2 * geometry.stem / 4, 2 * geometry.widths[0] / 16, 2 * geometry.widths[1] / 64)))
        self._host = pack_network(sd, geometry, dtype)
        self._ws = {}   # (`timings` receives events under the keys of STAGES -- tools/bench_facealign.py)

    @classmethod
    def from_pretrained(cls, path, max_faces: int = 4, conf_threshold: float = 0.97, nms_threshold: float = 0.4, eye_dist_threshold: float = 5,
                        upscale_factor: float = 1, dtype=None, device=None, **kwargs):
        """path: a local detection_Resnet50_Final.pth or a directory that holds it (no network access, ever)."""
        return cls(cls._load(path), max_faces=max_faces, conf_threshold=conf_threshold, nms_threshold=nms_threshold,
                   eye_dist_threshold=eye_dist_threshold, upscale_factor=upscale_factor, dtype=dtype, device=device, **kwargs)

    # ---- input checks ----------------------------------------------------------------------------------------------------------
    def _check_size(self, h: int, w: int) -> None:
        if h < 32 or w < 32 or h % 32 or w % 32:
            raise NotImplementedError(f"FaceAligner takes frames whose sides are multiples of 32 (512 x 768 and its x2 / x4 upscales; every level's map "
                                      f"is then exactly half of the finer one); got {h} x {w}")

    # ---- device state ----------------------------------------------------------------------------------------------------------
    def workspace(self, n: int, h: int, w: int) -> dict:
        """The buffers of a call with n frames of h x w pixels, cached per (n, h, w): the levels' fp32 head tensors, the decode's scratch, the
        outputs (dets, count, overflow, affine, inverse_affine, faces -- what `align` returns) and a pool of activation buffers that the
        layers of a pass take and give back in a fixed order (the first pass allocates them, every later pass reuses the same ones)."""
        import torch
        from . import kernels as K
        mf = self.max_faces

        def make(dev):
            def new(shape, dtype):
                return torch.empty(shape, dtype=dtype, device=dev)

            return {"heads": [new((n, fh, fw, HEAD_COLS), torch.float32) for fh, fw in level_shapes(h, w)],
                    "decode": new((K.rface_decode_workspace_bytes(n, h, w),), torch.uint8),
                    "dets": new((n, mf, DET_COLS), torch.float32), "count": new((n,), torch.int32), "overflow": new((n,), torch.int32),
                    "affine": new((n, mf, 2, 3), torch.float64), "inverse_affine": new((n, mf, 2, 3), torch.float64),
                    "faces": new((n * mf, FACE_SIZE, FACE_SIZE, 3), torch.uint8)}

        return self._workspace((n, h, w), make)

    # ---- the chain -------------------------------------------------------------------------------------------------------------
    def _network(self, src, ws, i0: int, bgr: bool, taps_out=None) -> None:
        """The network for the frames `src` (a chunk): the levels' head rows into ws["heads"][k][i0 : i0 + len(src)].  taps_out: a list that
        receives the stem's output and clones of the three taps (tests)."""
        from . import kernels as K
        wts = self._weights(src.device)
        geo = self.geometry
        n, h, w, _ = src.shape
        with self._pass(ws, src.device) as p:   # the same buffers in the same order on every pass
            take, give, launch, pw, c3 = p.take, p.give, p.launch, p.pointwise, p.conv3x3
            s = launch("stem", K.rface_stem, src, wts["stem"][0], wts["stem"][1], take(n, h // 2, w // 2, geo.stem), bgr)
            if taps_out is not None:
                taps_out.append(s.clone())
            x = launch("body", K.maxpool3x3s2, s, take(n, h // 4, w // 4, geo.stem))
            give(s)
            taps = []
            for (li, b, _, _, _, stride), blk in zip(blocks_of(geo), wts["blocks"]):
                t = pw("body", x, blk["conv1"], K.ACT_RELU)
                t2 = c3("body", t, blk["conv2"], stride, K.ACT_RELU)
                give(t)
                idn = x
                if b == 0:
                    if stride == 2:
                        sub = launch("body", K.subsample2, x, take(x.shape[0], x.shape[1] // 2, x.shape[2] // 2, x.shape[3]))
                        idn = pw("body", sub, blk["down"])
                        give(sub)
                    else:
                        idn = pw("body", x, blk["down"])
                y = pw("body", t2, blk["conv3"], K.ACT_RELU, residual=idn)   # the residual is added before the activation
                give(t2)
                if idn is not x:
                    give(idn)
                if not any(x is tp for tp in taps):   # a tap stays until the FPN has read it
                    give(x)
                x = y
                if li > 1 and b == LAYERS[li - 1] - 1:
                    taps.append(x)
            if taps_out is not None:
                taps_out.extend(tp.clone() for tp in taps)
            # ---- FPN
            o = [pw("fpn_ssh", tp, wb, K.ACT_RELU) for tp, wb in zip(taps, wts["output"])]
            for tp in taps:
                give(tp)
            launch("fpn_ssh", K.add_up2, o[1], o[2], o[1])
            m2 = c3("fpn_ssh", o[1], wts["merge"][1], act=K.ACT_RELU)
            give(o[1])
            launch("fpn_ssh", K.add_up2, o[0], m2, o[0])
            m1 = c3("fpn_ssh", o[0], wts["merge"][0], act=K.ACT_RELU)
            give(o[0])
            # ---- SSH and heads
            for k, (f, ssh, head) in enumerate(zip((m1, m2, o[2]), wts["ssh"], wts["heads"])):
                nn, hh, ww, c = f.shape
                m = nn * hh * ww
                b3 = c3("fpn_ssh", f, ssh["conv3X3"], act=K.ACT_RELU)
                b51 = c3("fpn_ssh", f, ssh["conv5X5_1"], act=K.ACT_RELU)
                give(f)
                cat = take(m, c // 2)                      # [5X5_2 | 7x7_3]
                b5 = c3("fpn_ssh", b51, ssh["conv5X5_2"], act=K.ACT_RELU)
                launch("fpn_ssh", K.copy_cols, b5.view(m, c // 4), cat, 0)
                give(b5)
                b72 = c3("fpn_ssh", b51, ssh["conv7X7_2"], act=K.ACT_RELU)
                give(b51)
                b7 = c3("fpn_ssh", b72, ssh["conv7x7_3"], act=K.ACT_RELU)
                give(b72)
                launch("fpn_ssh", K.copy_cols, b7.view(m, c // 4), cat, c // 4)
                give(b7)
                pw("heads", b3, head, a2=cat, out2d=ws["heads"][k][i0:i0 + nn].view(m, HEAD_COLS), out_f32=True)
                give(b3)
                give(cat)

    def _heads(self, src, ws, bgr: bool) -> list:
        n, h, w, _ = src.shape
        for i0, sl in self._chunks(n, self.chunk_frames(h, w)):
            self._network(src[sl], ws, i0, bgr)
        return ws["heads"]

    def decode(self, heads, h: int, w: int, ws=None, only_center_face: bool = False, only_keep_largest: bool = False, conf_threshold=None,
               eye_dist_threshold=None) -> dict:
        """The three levels' fp32 head tensors [n, fh, fw, 32] on the device (pack_heads' layout) -> dets, count, overflow, affine and
        inverse_affine (the workspace's tensors, or new ones without `ws`).  Tests plant head tensors here."""
        import torch
        from . import kernels as K
        n, dev = heads[0].shape[0], heads[0].device
        if ws is None:
            mf = self.max_faces
            ws = {"decode": torch.empty((K.rface_decode_workspace_bytes(n, h, w),), dtype=torch.uint8, device=dev),
                  "dets": torch.empty((n, mf, DET_COLS), dtype=torch.float32, device=dev), "count": torch.empty((n,), dtype=torch.int32, device=dev),
                  "overflow": torch.empty((n,), dtype=torch.int32, device=dev), "affine": torch.empty((n, mf, 2, 3), dtype=torch.float64, device=dev),
                  "inverse_affine": torch.empty((n, mf, 2, 3), dtype=torch.float64, device=dev)}
        flags = (FLAG_CENTER if only_center_face else 0) | (FLAG_LARGEST if only_keep_largest else 0)
        conf = self.conf_threshold if conf_threshold is None else float(conf_threshold)
        eye = self.eye_dist_threshold if eye_dist_threshold is None else float(eye_dist_threshold)
        self._timed("decode", K.rface_decode, heads, h, w, conf, self.nms_threshold, eye, flags, ws["decode"], ws["dets"], ws["count"], ws["overflow"])
        self._timed("decode", K.face_align, ws["dets"], ws["count"], self.upscale_factor, ws["affine"], ws["inverse_affine"])
        return ws

    def warp(self, src, affine, count, out=None, bgr: bool = False):
        """uint8 device frames [n, H, W, 3], float64 affine [n, max_faces, 2, 3], int32 count [n] -> uint8 [n * max_faces, 512, 512, 3]."""
        import torch
        from . import kernels as K
        if out is None:
            out = torch.empty((src.shape[0] * affine.shape[1], FACE_SIZE, FACE_SIZE, 3), dtype=torch.uint8, device=src.device)
        return self._timed("warp", K.face_warp, src, affine, count, out, bgr)

    def align(self, frames, bgr: bool = False, only_center_face: bool = False, only_keep_largest: bool = False, eye_dist_threshold=None) -> dict:
        """frames: a list of PIL images / uint8 arrays of one size, or a uint8 tensor [n, H, W, 3] (no host copy when it is on the device)
        -> a dict of DEVICE tensors: faces uint8 [n * max_faces, 512, 512, 3] (slot f * max_faces + r; a slot behind the count holds the border
        value), count int32 [n], dets float32 [n, max_faces, 15] (x1, y1, x2, y2, score, five landmarks), affine and inverse_affine float64
        [n, max_faces, 2, 3], overflow int32 [n].  Nothing is read back to the host.  The tensors belong to the workspace of (n, H, W): the
        next call on the same shapes overwrites them (and allocates nothing); clone what must outlive it.

        bgr=False is the reference's way: it hands an RGB array where facexlib expects BGR, so the detector's mean (104, 117, 123) and the
        border value (135, 133, 132) meet channels 0, 1, 2 of the array as given.  bgr=True reverses the channels on the way into the detector
        and the border value with them (what facexlib does with the BGR array it expects); the crops stay in the caller's order."""
        src = self._frames(frames)
        n, h, w, _ = src.shape
        if n == 0:
            raise ValueError("no frames")
        ws = self.workspace(n, h, w)
        self.decode(self._heads(src, ws, bool(bgr)), h, w, ws, only_center_face, only_keep_largest, eye_dist_threshold=eye_dist_threshold)
        self.warp(src, ws["affine"], ws["count"], ws["faces"], bool(bgr))
        return {k: ws[k] for k in ("faces", "count", "dets", "affine", "inverse_affine", "overflow")}

    def heads(self, frames, bgr: bool = False) -> list:
        """-> the three levels' fp32 head tensors [n, fh, fw, 32] as new tensors (tests, tools)."""
        src = self._frames(frames)
        n, h, w, _ = src.shape
        return [t.clone() for t in self._heads(src, self.workspace(n, h, w), bool(bgr))]

    def body_taps(self, frames, bgr: bool = False) -> list:
        """-> the stem's output and the outputs of layer2, layer3 and layer4 (NHWC, new tensors) for what fits one pass (tests)."""
        src = self._frames(frames)
        n, h, w, _ = src.shape
        if n > self.chunk_frames(h, w):
            raise ValueError("body_taps takes what fits one pass")
        taps = []
        self._network(src, self.workspace(n, h, w), 0, bool(bgr), taps_out=taps)
        return taps


class FaceHelper:
    """The adapter with facexlib.FaceRestoreHelper's method names that `FaceRestorer.enhance(img, has_aligned=False, face_helper=...)` drives,
    one frame at a time.  Detection, fit and warp run in `get_face_landmarks_5` (one `FaceAligner.align`); the count is read from the device
    once, there.  The paste-back runs on `paster` (a face_paste.FacePaster) when one is given; without one it raises."""

    def __init__(self, aligner: FaceAligner, bgr: bool = False, paster=None):
        self.aligner, self.bgr, self.paster = aligner, bool(bgr), paster
        self.face_size = (FACE_SIZE, FACE_SIZE)
        self.upscale_factor = aligner.upscale_factor
        self.clean_all()

    def clean_all(self) -> None:
        self.input_img = None
        self.all_landmarks_5, self.det_faces, self.affine_matrices, self.inverse_affine_matrices = [], [], [], []
        self.cropped_faces, self.restored_faces = [], []
        self._out, self._count = None, 0

    def read_image(self, img) -> None:
        """img: a PIL image or a uint8 array [H, W, 3] (facexlib also takes a path: not here)."""
        if isinstance(img, (str, os.PathLike)):
            raise NotImplementedError("read_image takes an image, not a path")
        self.input_img = np.asarray(img)

    def get_face_landmarks_5(self, only_keep_largest: bool = False, only_center_face: bool = False, resize=None, blur_ratio: float = 0.01,
                             eye_dist_threshold=None) -> int:
        if resize is not None:
            raise NotImplementedError("get_face_landmarks_5(resize=...) is not built (GFPGANer.enhance does not pass it)")
        if self.input_img is None:
            raise ValueError("read_image first")
        out = self.aligner.align([self.input_img], bgr=self.bgr, only_center_face=only_center_face, only_keep_largest=only_keep_largest,
                                 eye_dist_threshold=0.0 if eye_dist_threshold is None else eye_dist_threshold)
        self._count = int(out["count"][0])   # the one read that decides how much is copied
        self._out = {k: v[:self._count].clone() if k == "faces" else v[0, :self._count].clone() for k, v in out.items() if k not in ("count", "overflow")}
        dets = self._out["dets"].cpu().numpy()
        self.det_faces = [d[:5] for d in dets]
        self.all_landmarks_5 = [d[5:].reshape(5, 2) for d in dets]
        return self._count

    def align_warp_face(self, save_cropped_path=None, border_mode: str = "constant") -> None:
        if border_mode != "constant" or save_cropped_path is not None:
            raise NotImplementedError("align_warp_face: border_mode='constant' without a save path is what is built")
        if self._out is None:
            raise ValueError("get_face_landmarks_5 first")
        self.affine_matrices = list(self._out["affine"].cpu().numpy())
        self.cropped_faces = list(self._out["faces"].cpu().numpy())

    def add_restored_face(self, face) -> None:
        self.restored_faces.append(face)

    def get_inverse_affine(self, save_inverse_affine_path=None) -> None:
        if self._out is None:
            raise ValueError("get_face_landmarks_5 first")
        self.inverse_affine_matrices = list(self._out["inverse_affine"].cpu().numpy())

    def paste_faces_to_input_image(self, save_path=None, upsample_img=None):
        """-> the pasted uint8 array [h_up, w_up, 3] of the one frame (with a paster): the restored faces blended into `upsample_img`, or
        into the frame, at the aligner's upscale_factor."""
        if self.paster is None:
            raise NotImplementedError("paste-back (ParseNet mask, inverse warp, blend) is not built yet")
        if save_path is not None:
            raise NotImplementedError("paste_faces_to_input_image(save_path=...) is not built")
        if self._out is None or self.input_img is None:
            raise ValueError("read_image and get_face_landmarks_5 first")
        if len(self.restored_faces) != self._count:
            raise ValueError(f"{len(self.restored_faces)} restored faces for {self._count} detected ones")
        import torch
        h, w = self.input_img.shape[:2]
        bg = torch.from_numpy(np.ascontiguousarray(self.input_img if upsample_img is None else np.asarray(upsample_img)))[None]
        dev = self._out["inverse_affine"].device
        slots = max(self._count, 1)
        restored = torch.zeros((slots, FACE_SIZE, FACE_SIZE, 3), dtype=torch.uint8)
        for r, face in enumerate(self.restored_faces):
            restored[r] = torch.from_numpy(np.ascontiguousarray(face))
        inv = torch.zeros((1, slots, 2, 3), dtype=torch.float64, device=dev)
        inv[0, :self._count] = self._out["inverse_affine"]
        count = torch.tensor([self._count], dtype=torch.int32, device=dev)
        out = self.paster.paste(bg.to(dev), restored.to(dev), inv, count, self.upscale_factor, self.bgr, frame_size=(h, w))
        return out[0].cpu().numpy()
