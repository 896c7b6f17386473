"""FP8 Linear layers: the forward and the data gradient on the fp8 GEMM K17 (``ops.linear(fp8=True)``), on
request the weight gradient on K17W as well (``fp8="wgrad"``), or the MX block-scaled recipe on K17X (``fp8="mx"``).

:class:`Fp8Linear` is ``nn.Linear`` with another forward: same parameters, same state-dict keys, so a model
converts in place (:func:`use_fp8_linears`) and its checkpoints interchange with the bf16 model's.  Scaling is
per tensor and current (``ops.fp8_quantize``); the weight gradient stays a bf16 GEMM unless the module's
``fp8_mode`` is ``"wgrad"``, which also halves the activation the Linear saves (the e4m3 image instead of bf16).
``fp8_mode = "mx"`` swaps the recipe: one E8M0 scale per 32 elements along the reduction (``ops.mx_quantize``, one
launch and no global amax), all three operands e4m3, the scaling done by the MFMA in K17X.  ``"mx_wgrad"`` is
that with the weight gradient on K17XW from images blocked along the tokens (``ops.mx_wgrad``), which the
quantiser launches of x and dy write as well; the Linear then saves the e4m3 image of x instead of bf16 x.
Not built: delayed scaling / amax history, a cache of the quantised weight across microbatches, fp8 in the
GELU MLP and in ``linear_tee``.
"""
from __future__ import annotations

from typing import Sequence

import torch
from torch import nn

from .. import ops


class Fp8Linear(nn.Linear):
    """``nn.Linear`` whose forward is ``ops.linear(x, weight, bias, fp8=self.fp8_mode)``: K17 where
    ``ops.fp8_linear_supported`` holds (HIP bf16 tensors, feature counts multiples of 16, gradients
    enabled), the bf16 path of ``ops.linear`` otherwise.  ``fp8_mode``: ``True``, ``"wgrad"`` for the
    weight gradient on K17W too, ``"mx"`` for MX block scaling on K17X (feature counts multiples of 32), or
    ``"mx_wgrad"`` for MX with the weight gradient on K17XW too."""

    fp8_mode = True

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ops.linear(x, self.weight, self.bias, fp8=self.fp8_mode)


def use_fp8_linears(model: nn.Module, skip: Sequence[str] = ("lm_head", "decoder"), wgrad: bool = False,
                    mx=False) -> int:
    """Re-class every eligible plain ``nn.Linear`` of ``model`` to :class:`Fp8Linear` in place (the module
    objects, their parameters and hooks stay) and return how many were converted.  Eligible: in- and
    out-features multiples of 16 and a weight that is not tied to an ``nn.Embedding``; a module whose
    qualified name contains one of ``skip`` is left alone (output heads keep bf16 logits).  Tensor-parallel
    replacements are not ``nn.Linear`` and are untouched.  ``wgrad`` sets ``fp8_mode = "wgrad"`` on the
    converted modules; ``mx=True`` sets ``fp8_mode = "mx"`` and ``mx="wgrad"`` sets ``"mx_wgrad"`` (the MX weight
    gradient on K17XW); both ask for feature counts that are multiples of 32.  ``wgrad`` belongs to the
    per-tensor recipe and excludes ``mx``."""
    if mx not in (False, True, "wgrad"):
        raise ValueError(f"use_fp8_linears: mx must be a bool or 'wgrad', not {mx!r}")
    if wgrad and mx:
        raise ValueError("use_fp8_linears: wgrad is the per-tensor recipe's; the MX weight gradient is mx='wgrad'")
    mult = 32 if mx else 16
    tied = {id(m.weight) for m in model.modules() if isinstance(m, nn.Embedding)}
    n = 0
    for name, m in model.named_modules():
        if type(m) is not nn.Linear or any(s in name for s in skip) or id(m.weight) in tied:
            continue
        if m.in_features % mult or m.out_features % mult:
            continue
        m.__class__ = Fp8Linear
        if wgrad or mx:
            m.fp8_mode = "wgrad" if wgrad else ("mx_wgrad" if mx == "wgrad" else "mx")
        n += 1
    return n
