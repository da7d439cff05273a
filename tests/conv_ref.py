"""Plain restatement of ca_conv3x3's contract, integer-valued operands on which a correct kernel has no rounding freedom, and the
rectangular cases the convolution tests share (tests/test_rect_latents_gpu.py runs them on the kernels, tests/test_conv_ref_cpu.py
checks this file against torch and shows that the comparison catches the index errors it is there for).

    y = act(post_scale * (round(alpha * (conv3x3(up2?(cat(x, x2)), w) + bias + rowbias[row // rows_per_group])) + residual))

x, x2, residual and y are NHWC, w is [Cout, 3, 3, Cin] (the layout of ca_conv_args.w), `row` is the flat output pixel index
(image * Hout + y) * Wout + x, and round() is the rounding to the activation type the tiled kernels apply before the residual joins
(the order of tools/ps_check.conv_reference; `round_to=None` leaves it out).

Why integers: with x in {-1, 0, 1}, w in {-1, 0, 1}, bias and row bias in [-3, 3] every partial sum of every accumulation order is an
integer far below 2^24, so fp32 accumulation is exact whatever the order, the split or the tile shape.  The kernel's result must then
be `exact.to(dtype)` number for number: one dropped, doubled or misplaced tap anywhere fails the comparison, and no tolerance hides an
H / W swap that a Gaussian test would report as a slightly larger rel-L2 on a mostly-right tensor.  The conditions under which
`exact.to(dtype)` is what a correct kernel returns are asserted on the operands by exact_result() -- they are conditions on the
INPUTS of a test, never on the kernel:
  * fp16 holds every integer up to 2048, so results (and, with a residual, the value before it and the sum) must stay below that;
  * bf16 holds integers up to 256 and is one round-to-nearest-even from exact above (what Elem<CA_BF16>::from_f does): a bf16 case
    takes no residual, because the value before it would be rounded twice;
  * the Winograd route keeps V = B^T d B (integers in [-4, 4]), U = G g G^T (multiples of 1/4) and the sixteen products M (multiples
    of 1/4) in the activation type: every multiple of 1/4 below 512 is an fp16 value, so max |M| < 512 makes the fp16 route exact.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F


class Case(NamedTuple):
    label: str            # the plan label the launch must report (ca_conv3x3_plan_name with a workspace offered)
    images: int
    h: int                # stored input height and width
    w: int
    c1: int
    c2: int
    cout: int
    stride: int = 1
    upsample: bool = False
    pad_asym: bool = False
    epilogue: int = 0     # 0: none; n > 0: bias, residual and a row bias whose groups are n images' worth of output rows
    wino: bool = False    # offer the Winograd weights

    @property
    def id(self) -> str:
        s = f"{self.label}-{self.images}x{self.h}x{self.w}-{self.c1}+{self.c2}to{self.cout}"
        return s + ("-s2" if self.stride == 2 else "") + ("-up" if self.upsample else "") + ("-asym" if self.pad_asym else "") + \
            (f"-epi{self.epilogue}" if self.epilogue else "") + ("-wino" if self.wino else "")

    def out_hw(self):
        hl, wl = (2 * self.h, 2 * self.w) if self.upsample else (self.h, self.w)
        pad = 1 if self.pad_asym else 2
        return (hl + pad - 3) // self.stride + 1, (wl + pad - 3) // self.stride + 1

    def rows_per_group(self) -> int:
        ho, wo = self.out_hw()
        return self.epilogue * ho * wo


# The rectangular latents of the 512x768 and 768x768 workloads (64x96, 32x48, 16x24, 8x12; 96x96 .. 12x12) and smaller rectangles
# with the same properties, one or more per kernel a convolution of those workloads reaches.  Few channels keep the operands small:
# what is under test is the row -> (image, y, x) arithmetic, the border handling and the row-bias groups, which do not depend on K.
DIRECT_CASES = [
    Case("pq256x320", 25, 30, 44, 64, 0, 640),                       # M = 33000: a ragged last tile; images cross tiles at 1320 rows
    Case("pq256x320", 22, 32, 48, 64, 64, 640, epilogue=2),
    Case("pq256x320", 22, 64, 96, 64, 0, 640, stride=2),
    Case("pq256x320", 43, 32, 48, 512, 0, 320),
    Case("pp128x320", 42, 16, 24, 128, 0, 640),
    Case("pp128x320", 21, 16, 24, 64, 64, 1280, epilogue=1),
    Case("pp128x320", 42, 32, 48, 128, 0, 640, stride=2),
    Case("pp128x320", 42, 8, 12, 128, 0, 640, upsample=True),
    Case("128x160", 43, 32, 48, 64, 0, 320, epilogue=1),
    Case("128x128", 11, 32, 48, 64, 0, 512),
    Case("128x128", 11, 64, 96, 64, 0, 512, stride=2, pad_asym=True),
    Case("128x64", 43, 32, 48, 64, 0, 64),
    Case("128x128_splitk8", 8, 8, 12, 1280, 0, 1280, epilogue=4),
    Case("128x128_splitk4", 4, 6, 10, 384, 0, 128),
    Case("128x64_r3", 3, 6, 10, 64, 0, 64),
    Case("128x64_r3", 3, 10, 6, 64, 0, 128, stride=2, pad_asym=True),
    Case("reg_128x64", 3, 6, 10, 32, 0, 32),
    Case("128x128_splitk5", 32, 8, 11, 1280, 0, 1280, wino=True),    # an odd W: the Winograd route must decline it, not mis-run it
]
WINO_CASES = [
    Case("wino_pq256x320", 32, 8, 12, 1280, 0, 1280, wino=True),
    Case("wino_pq256x320", 32, 8, 12, 1280, 1280, 1280, epilogue=16, wino=True),
    Case("wino_pq256x320", 64, 12, 12, 640, 0, 320, wino=True),
    Case("wino_pq256x320", 8, 16, 24, 640, 0, 320, wino=True),
    Case("wino_pq256x320", 32, 4, 6, 1280, 0, 1280, upsample=True, wino=True),
]
# ca_conv_up2_phase (label "up2_pq256x320"): the first is a shape ca_conv_up2_phase_supported takes, the second runs through the entry
UP2_CASES = [
    Case("up2_pq256x320", 32, 32, 48, 640, 0, 320, upsample=True),
    Case("up2_pq256x320", 3, 6, 10, 320, 0, 320, upsample=True),
]
SMALLEST = DIRECT_CASES[16]  # (3, 6, 10, 32 -> 32)
LABELS = {c.label for c in DIRECT_CASES + WINO_CASES + UP2_CASES}


def padded_input(x: torch.Tensor, x2: Optional[torch.Tensor] = None, *, upsample: bool = False, pad_asym: bool = False) -> torch.Tensor:
    """cat(x, x2) along the channels, nearest x2, zero padding (1, 1) or -- pad_asym -- (0, 1) on both axes."""
    xin = x if x2 is None else torch.cat([x, x2], dim=3)
    if upsample:
        xin = xin.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    lo = 0 if pad_asym else 1
    images, h, w, c = xin.shape
    xp = xin.new_zeros(images, h + lo + 1, w + lo + 1, c)
    xp[:, lo:lo + h, lo:lo + w] = xin
    return xp


def conv_taps(xp: torch.Tensor, w: torch.Tensor, stride: int = 1) -> torch.Tensor:
    """The nine taps on an already padded input: y[i, oy, ox] = sum_{ky, kx} xp[i, stride * oy + ky, stride * ox + kx] . w[:, ky, kx]."""
    images, hp, wp, _ = xp.shape
    ho, wo = (hp - 3) // stride + 1, (wp - 3) // stride + 1
    y = xp.new_zeros(images, ho, wo, w.shape[0])
    for ky in range(3):
        for kx in range(3):
            tap = xp[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride]
            y += tap @ w[:, ky, kx, :].t()
    return y


def row_bias_rows(rowbias: torch.Tensor, rows: int, rows_per_group: int, shift: int = 0) -> torch.Tensor:
    """[rows, Cout]: row r takes rowbias[(r + shift) // rows_per_group] (shift = 0 is the contract)."""
    idx = (torch.arange(rows, device=rowbias.device) + shift).div(rows_per_group, rounding_mode="floor").clamp_(0, rowbias.shape[0] - 1)
    return rowbias[idx]


def epilogue(y, *, bias=None, rowbias=None, rows_per_group=0, residual=None, alpha=1.0, post_scale=1.0, act=0, round_to=None, rb_shift=0):
    """y [images, Ho, Wo, Cout] -> the same with the epilogue applied, in y's dtype."""
    dt = y.dtype
    if bias is not None:
        y = y + bias.to(dt)
    if rowbias is not None:
        y = y + row_bias_rows(rowbias.to(dt), y.shape[0] * y.shape[1] * y.shape[2], rows_per_group, rb_shift).reshape(y.shape)
    y = y * alpha
    if round_to is not None:
        y = y.to(round_to).to(dt)
    if residual is not None:
        y = y + residual.to(dt).reshape(y.shape)
    y = y * post_scale
    return F.silu(y) if act == 1 else y


def conv_ref(x, w, *, x2=None, bias=None, rowbias=None, rows_per_group=0, residual=None, stride=1, upsample=False, pad_asym=False,
             alpha=1.0, post_scale=1.0, act=0, round_to=None, acc=torch.float64):
    """ca_conv3x3 on tensors of any float dtype and device, computed in `acc`; returns [images, Hout, Wout, Cout] in `acc`."""
    xp = padded_input(x.to(acc), None if x2 is None else x2.to(acc), upsample=upsample, pad_asym=pad_asym)
    y = conv_taps(xp, w.to(acc), stride)
    return epilogue(y, bias=bias, rowbias=rowbias, rows_per_group=rows_per_group, residual=residual, alpha=alpha, post_scale=post_scale,
                    act=act, round_to=round_to)


def integer_operands(case: Case, seed: int = 0) -> dict:
    """fp32 CPU tensors with integer values: x (and x2) in {-1, 0, 1} with P(non-zero) = 1/4, w in {-1, 0, 1} uniformly, and -- for a
    case with an epilogue -- bias and row bias in [-3, 3], residual in [-8, 8].  Every value is exact in fp16 and in bf16."""
    g = torch.Generator().manual_seed(1000 + seed)
    cin = case.c1 + case.c2
    ho, wo = case.out_hw()

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).float()

    def sparse(*shape):
        return (ints(0, 1, *shape) * 2 - 1) * (torch.rand(shape, generator=g) < 0.25).float()

    d = dict(x=sparse(case.images, case.h, case.w, case.c1), x2=sparse(case.images, case.h, case.w, case.c2) if case.c2 else None,
             w=ints(-1, 1, case.cout, 3, 3, cin), bias=None, rowbias=None, residual=None, rows_per_group=0)
    if case.epilogue:
        groups = -(-case.images // case.epilogue)
        d.update(bias=ints(-3, 3, case.cout), rowbias=ints(-3, 3, groups, case.cout), residual=ints(-8, 8, case.images, ho, wo, case.cout),
                 rows_per_group=case.rows_per_group())
    return d


G_WINO = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]])
BT_WINO = torch.tensor([[1.0, 0.0, -1.0, 0.0], [0.0, 1.0, 1.0, 0.0], [0.0, -1.0, 1.0, 0.0], [0.0, 1.0, 0.0, -1.0]])


def winograd_weight(w: torch.Tensor) -> torch.Tensor:
    """w [Cout, 3, 3, Cin] -> U [16, Cout, Cin] = G g G^T, position 4 xi + nu (what ca_pack_w_wino writes)."""
    g = G_WINO.to(w)
    return torch.einsum("xk,oklc,yl->xyoc", g, w, g).reshape(16, w.shape[0], w.shape[3]).contiguous()


def winograd_products(x, w, *, x2=None, upsample=False, acc=torch.float32) -> torch.Tensor:
    """M [16, tiles, Cout] of F(2x2, 3x3): V = B^T d B of every 4x4 neighbourhood (stride 2) of the padded input times U, position by position."""
    xp = padded_input(x.to(acc), None if x2 is None else x2.to(acc), upsample=upsample)
    images, hp, wp, c = xp.shape
    th, tw = (hp - 2) // 2, (wp - 2) // 2
    d = xp.unfold(1, 4, 2).unfold(2, 4, 2)                      # [images, th, tw, c, 4, 4]
    bt = BT_WINO.to(xp)
    v = torch.einsum("xi,ntscij,yj->xyntsc", bt, d, bt).reshape(16, images * th * tw, c)
    return torch.bmm(v, winograd_weight(w.to(acc)).transpose(1, 2))


def exact_before_residual(ops: dict, case: Case, acc=torch.float64) -> torch.Tensor:
    """conv + bias + row bias of integer_operands(case) (tensors on any device), after asserting that the operands are the integers
    the argument in the module docstring needs.  fp16 and bf16 comparisons of one case share it."""
    for name in ("x", "x2", "w", "bias", "rowbias", "residual"):
        t = ops[name]
        assert t is None or bool((t == t.round()).all()), f"{case.id}: {name} is not integer-valued"
    assert float(ops["x"].abs().max()) <= 1 and float(ops["w"].abs().max()) <= 1
    assert 9 * (case.c1 + case.c2) + 3 + 3 + 8 < 2 ** 24       # every partial sum, in any order, is an integer fp32 holds
    pre = conv_ref(ops["x"], ops["w"], x2=ops["x2"], bias=ops["bias"], rowbias=ops["rowbias"], rows_per_group=ops["rows_per_group"],
                   stride=case.stride, upsample=case.upsample, pad_asym=case.pad_asym, acc=acc)
    assert bool((pre == pre.round()).all())
    return pre


def exact_result(ops: dict, case: Case, dtype: torch.dtype, *, winograd: bool = False, pre: Optional[torch.Tensor] = None) -> torch.Tensor:
    """What a correct kernel returns for integer_operands(case) in `dtype`, after asserting on the OPERANDS that it has no rounding
    freedom (module docstring).  A bf16 case is compared without its residual: the launch must leave it out too."""
    assert dtype in (torch.float16, torch.bfloat16)
    if pre is None:
        pre = exact_before_residual(ops, case)
    with_res = ops["residual"] is not None and dtype == torch.float16
    final = pre + ops["residual"].to(pre.dtype) if with_res else pre
    if dtype == torch.float16:
        top = max(float(pre.abs().max()), float(final.abs().max()))
        assert top < 2048, f"{case.id}: |y| reaches {top}: not every value is an fp16 number"
    if winograd:
        assert dtype == torch.float16 and case.stride == 1 and not case.pad_asym
        m = winograd_products(ops["x"], ops["w"], x2=ops["x2"], upsample=case.upsample)
        top_m = float(m.abs().max())
        assert bool((m * 4 == (m * 4).round()).all()) and top_m < 512, f"{case.id}: max |M| = {top_m}: not every product is an fp16 number"
    return final.to(dtype)


def assert_same(out: torch.Tensor, ref: torch.Tensor, what: str) -> None:
    """out == ref number for number (NHWC, same dtype); on a mismatch: how many elements differ and the first (image, y, x, channel)."""
    assert out.shape == ref.shape and out.dtype == ref.dtype, f"{what}: {tuple(out.shape)} {out.dtype} vs {tuple(ref.shape)} {ref.dtype}"
    bad = (out != ref) | torch.isnan(out)
    n = int(bad.sum())
    if n:
        first = int(bad.flatten().to(torch.uint8).argmax())
        idx = []
        for size in reversed(out.shape):
            idx.append(first % size)
            first //= size
        i, y, x, c = reversed(idx)
        raise AssertionError(f"{what}: {n} of {out.numel()} elements differ; first at (image {i}, y {y}, x {x}, channel {c}): "
                             f"got {float(out[i, y, x, c])}, want {float(ref[i, y, x, c])}")
