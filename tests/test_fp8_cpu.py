"""The host mirrors of the FP8 Linear (no GPU): the scale recipe, ``ops.linear(fp8=True)`` on CPU tensors and
the in-place model conversion."""
import math

import pytest
import torch
from torch import nn

import madnn
from madnn import ops
from madnn.ops import reference


@pytest.mark.parametrize("fmt,fmax", [("e4m3", 448.0), ("e5m2", 57344.0)])
@pytest.mark.parametrize("amax", [0.0, 1e-40, 1e-30, 0.7, 1.0, 447.0, 448.0, 449.0, 57344.0, 3e38])
def test_fp8_scale(fmt, fmax, amax):
    s = reference.fp8_scale(torch.tensor(amax), fmt).item()
    a = torch.tensor(amax, dtype=torch.float32).item()
    assert math.frexp(s)[0] == 0.5 and 2.0 ** -126 <= s <= 2.0 ** 126   # a power of two, normal with its reciprocal
    if a == 0:
        assert s == 1.0
    else:
        assert a * s <= fmax
        assert fmax < 2 * a * s or s == 2.0 ** 126   # tight, unless the exponent clamp holds it (subnormal amax)


@pytest.mark.parametrize("has_res", [False, True])
def test_linear_fp8_on_cpu_is_the_reference(has_res):
    torch.manual_seed(1)
    x, w, b = torch.randn(5, 24).bfloat16(), torch.randn(16, 24).bfloat16(), torch.randn(16).bfloat16()
    r = torch.randn(5, 16).bfloat16() if has_res else None
    out = []
    for fn in (lambda *a: ops.linear(a[0], a[1], a[2], fp8=True, residual=r), lambda *a: reference.linear_fp8(*a, r)):
        ts = [t.clone().requires_grad_() for t in (x, w, b)]
        y = fn(*ts)
        y.float().sum().backward()
        out.append([y.detach()] + [t.grad for t in ts])
    assert all(torch.equal(p, q) for p, q in zip(*out))
    # the fp8 recipe, not the bf16 Linear
    assert not torch.equal(out[0][0], ops.linear(x, w, b, residual=r))


def test_use_fp8_linears_keeps_state_dict_keys():
    emb = nn.Embedding(32, 16)
    model = nn.ModuleDict({"emb": emb, "a": nn.Linear(16, 32), "odd": nn.Linear(16, 24), "lm_head": nn.Linear(16, 32),
                           "tied": nn.Linear(16, 32, bias=False)})
    model["tied"].weight = emb.weight
    keys = list(model.state_dict())
    assert madnn.nn.use_fp8_linears(model) == 1
    assert type(model["a"]) is madnn.nn.Fp8Linear and isinstance(model["a"], nn.Linear)
    assert all(type(model[n]) is nn.Linear for n in ("odd", "lm_head", "tied"))
    assert list(model.state_dict()) == keys
