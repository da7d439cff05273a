"""Operand checks of the kernel front end (kernels.py).

The library checks the integers, the alignment and the overlap it is handed; what lies behind a pointer only the Python wrapper
can know.  Every rule here raises CAHipError naming the entry (`who`) and the operand -- under `python -O` as well: none of them
is an assert.  Nothing is formatted unless a rule fails.
"""
from __future__ import annotations

from typing import Optional

import torch

from ._capi import CAHipError


def _req_cuda(who: str, names: str, *ts) -> None:
    """Every given tensor is on the device: the one place that asks.  `names`: the operands' names in the order of `ts`, one word
    each (the last word also names whatever follows it: a list of tensors)."""
    for i, t in enumerate(ts):
        if t is not None and not t.is_cuda:
            names = names.split()
            raise CAHipError(f"{who}: {names[min(i, len(names) - 1)]} is not on the device: HIP kernels need device tensors (no CPU fallback)")


def _got(t) -> str:
    return f"{str(t.dtype)[6:]} {list(t.shape)}" + ("" if t.is_contiguous() else f" with strides {list(t.stride())}")


def _need(cond, who: str, what: str, got: Optional[torch.Tensor] = None) -> None:
    """A rule that is not one tensor's dtype / shape / contiguity; `what` names the operand and says what was wanted, `got` is the
    tensor the message then describes."""
    if not cond:
        raise CAHipError(f"{who}: {what}" + ("" if got is None else "; got " + _got(got)))


_D2, _D3, _D4, _D5 = (None,) * 2, (None,) * 3, (None,) * 4, (None,) * 5  # `shape` of _t: that many dimensions of any extent


def _t(who: str, name: str, t: torch.Tensor, dtype=None, shape=None, numel=None, contiguous: bool = True, what: Optional[str] = None):
    """One tensor operand (its device: _req_cuda): `dtype` one dtype or a collection of them, `shape` a tuple in which None matches
    any extent, `numel` the element count where the shape is free, contiguous unless told otherwise.  Returns the shape.  `what`
    replaces the wanted part of the message, which names the entry, the operand, what was wanted and what was given:
    "ca_dwconv3x3: w must be float16 [9, 16], contiguous; got float16 [8, 16]"."""
    ok = dtype is None or t.dtype == dtype or (dtype.__class__ is not torch.dtype and t.dtype in dtype)
    if ok and shape is not None:
        have = t.shape
        ok = len(have) == len(shape)
        if ok:
            for w, h in zip(shape, have):
                if w is not None and w != h:
                    ok = False
                    break
    if ok and numel is not None:
        ok = t.numel() == numel
    if ok and contiguous:
        ok = t.is_contiguous()
    if not ok:
        _bad_operand(who, name, t, dtype, shape, numel, contiguous, what)
    return t.shape


def _bad_operand(who, name, t, dtype, shape, numel, contiguous, what):
    def dts(d):
        return str(d).replace("torch.", "") if d.__class__ is torch.dtype else " / ".join(str(e).replace("torch.", "") for e in d)
    if what is None:
        want = [] if dtype is None else [dts(dtype)]
        if shape is not None:
            want.append("[" + ", ".join("*" if e is None else str(e) for e in shape) + "]")
        if numel is not None:
            want.append(f"of {numel} elements")
        what = ", ".join(p for p in (" ".join(want), "contiguous" if contiguous else "") if p)
    raise CAHipError(f"{who}: {name} must be {what}; got {_got(t)}")
