"""The fp8 weight-gradient mode without a GPU: ``ops.linear(fp8="wgrad")`` and ``ops.fp8_wgrad`` on CPU tensors
are their plain-torch formulas, and ``use_fp8_linears(wgrad=True)`` marks exactly the modules it converts."""
import pytest
import torch
from torch import nn

import madnn
from madnn import ops
from madnn.ops import reference


def _run(fn, x, w, b, r, g):
    ts = [t.detach().clone().requires_grad_() for t in (x, w, b, r)]
    y = fn(*ts)
    y.backward(g)
    return [y.detach()] + [t.grad for t in ts]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_linear_wgrad_on_cpu_is_the_reference(dtype):
    torch.manual_seed(3)
    x, w, b = torch.randn(2, 9, 32).to(dtype), (torch.randn(48, 32) / 4).to(dtype), torch.randn(48).to(dtype)
    r, g = torch.randn(2, 9, 48).to(dtype), torch.randn(2, 9, 48).to(dtype)
    got = _run(lambda x, w, b, r: ops.linear(x, w, b, residual=r, fp8="wgrad"), x, w, b, r, g)
    want = _run(lambda x, w, b, r: reference.linear_fp8(x, w, b, r, wgrad=True), x, w, b, r, g)
    plain = _run(lambda x, w, b, r: ops.linear(x, w, b, residual=r, fp8=True), x, w, b, r, g)
    assert all(torch.equal(a, c) for a, c in zip(got, want))
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])   # y, dx: the same path
    assert not torch.equal(got[2], plain[2])                                 # dw: from the fp8 images


@pytest.mark.parametrize("into", [False, True])
def test_fp8_wgrad_on_cpu_is_the_formula(into):
    g = torch.Generator().manual_seed(5)
    sg, sx = torch.tensor([8.0]), torch.tensor([0.25])
    g8 = (torch.randn(21, 32, generator=g) * sg).to(torch.float8_e5m2)
    x8 = (torch.randn(21, 48, generator=g) * sx).to(torch.float8_e4m3fn)
    out = torch.empty(32, 48, dtype=torch.bfloat16) if into else None
    dw = ops.fp8_wgrad(g8, sg, x8, sx, out=out)
    assert (dw is out) == into
    assert torch.equal(dw, ((g8.float() / sg).t() @ (x8.float() / sx)).bfloat16())


@pytest.mark.parametrize("wgrad", [False, True])
def test_use_fp8_linears_sets_the_mode(wgrad):
    model = nn.Sequential(nn.Linear(32, 48), nn.Linear(48, 20), nn.Linear(20, 32))
    keys = list(model.state_dict())
    assert madnn.nn.use_fp8_linears(model, **({"wgrad": True} if wgrad else {})) == 1
    assert [type(m) is madnn.nn.Fp8Linear for m in model] == [True, False, False]
    assert model[0].fp8_mode == ("wgrad" if wgrad else True)
    assert not hasattr(model[1], "fp8_mode") and list(model.state_dict()) == keys
