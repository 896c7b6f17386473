"""FP8 Linear layers: the forward and the data gradient on the fp8 GEMM K17 (``ops.linear(fp8=True)``).

:class:`Fp8Linear` is ``nn.Linear`` with another forward: same parameters, same state-dict keys, so a model
converts in place (:func:`use_fp8_linears`) and its checkpoints interchange with the bf16 model's.  Scaling is
per tensor and current (``ops.fp8_quantize``); the weight gradient stays a bf16 GEMM.  Not built: an fp8 weight
gradient, delayed scaling / amax history, block or MX scaling, a cache of the quantised weight across
microbatches, fp8 in the GELU MLP and in ``linear_tee``.
"""
from __future__ import annotations

from typing import Sequence

import torch
from torch import nn

from .. import ops


class Fp8Linear(nn.Linear):
    """``nn.Linear`` whose forward is ``ops.linear(x, weight, bias, fp8=True)``: K17 where
    ``ops.fp8_linear_supported`` holds (HIP bf16 tensors, feature counts multiples of 16, gradients
    enabled), the bf16 path of ``ops.linear`` otherwise."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ops.linear(x, self.weight, self.bias, fp8=True)


def use_fp8_linears(model: nn.Module, skip: Sequence[str] = ("lm_head", "decoder")) -> int:
    """Re-class every eligible plain ``nn.Linear`` of ``model`` to :class:`Fp8Linear` in place (the module
    objects, their parameters and hooks stay) and return how many were converted.  Eligible: in- and
    out-features multiples of 16 and a weight that is not tied to an ``nn.Embedding``; a module whose
    qualified name contains one of ``skip`` is left alone (output heads keep bf16 logits).  Tensor-parallel
    replacements are not ``nn.Linear`` and are untouched."""
    tied = {id(m.weight) for m in model.modules() if isinstance(m, nn.Embedding)}
    n = 0
    for name, m in model.named_modules():
        if type(m) is not nn.Linear or any(s in name for s in skip) or id(m.weight) in tied:
            continue
        if m.in_features % 16 or m.out_features % 16:
            continue
        m.__class__ = Fp8Linear
        n += 1
    return n
