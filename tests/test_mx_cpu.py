"""The host mirrors of the MX FP8 Linear (no GPU): the block quantiser's properties, ``ops.linear(fp8="mx")`` on CPU
tensors and the in-place model conversion."""
import pytest
import torch
from torch import nn

import madnn
from madnn import ops
from madnn.ops import reference


@pytest.mark.parametrize("fmt,fmax,emax,mant,emin", [("e4m3", 448.0, 8, 3, -6), ("e5m2", 57344.0, 15, 2, -14)])
def test_mx_quantize_properties(fmt, fmax, emax, mant, emin):
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(16, 96, generator=g) * torch.exp2(torch.randint(-12, 3, (16, 96), generator=g).float())).bfloat16()
    x[3, 32:64] = 0
    x[4, :32] *= 2.0 ** -128          # amax below 2^(emax - 127): the clamp at 0
    q, e = reference.mx_quantize(x, fmt)
    xb = x.double().view(16, 3, 32)
    amax = xb.abs().amax(-1)
    want = (torch.floor(torch.log2(amax.clamp_min(2.0 ** -140))) + 127 - emax).clamp(0, 254)
    want = torch.where(amax == 0, torch.full_like(want, 127), want)
    assert e.dtype == torch.uint8 and torch.equal(e.double(), want) and (e[4, 0] == 0) and (e[3, 1] == 127)
    scale = torch.exp2(e.double() - 127).unsqueeze(-1)
    v = xb / scale                                      # what the cast sees
    # half an fp8 ulp at v: 2^(floor(log2 |v|) - mant - 1), the subnormal step below the smallest normal 2^emin
    ulp_half = torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** emin))) - mant - 1)
    err = (q.double().view(16, 3, 32) - v).abs()
    sat = v.abs() > fmax
    assert (amax / scale.squeeze(-1) < 2.0 ** (emax + 1)).all()
    assert (err[~sat] <= ulp_half[~sat]).all() and (q.double().view(16, 3, 32)[sat].abs() == fmax).all()
    assert not q.view(torch.uint8)[3, 32:64].any()


@pytest.mark.parametrize("has_res", [False, True])
def test_linear_mx_on_cpu_is_the_reference(has_res):
    torch.manual_seed(1)
    x, w, b = torch.randn(5, 64).bfloat16(), torch.randn(32, 64).bfloat16(), torch.randn(32).bfloat16()
    r = torch.randn(5, 32).bfloat16() if has_res else None
    out = []
    for fn in (lambda *a: ops.linear(a[0], a[1], a[2], fp8="mx", residual=r), lambda *a: reference.linear_mx(*a, r)):
        ts = [t.clone().requires_grad_() for t in (x, w, b)]
        y = fn(*ts)
        (y.float() * torch.arange(32)).sum().backward()
        out.append([y.detach()] + [t.grad for t in ts])
    assert all(torch.equal(p, q) for p, q in zip(*out))
    # the MX recipe: neither the bf16 Linear nor the per-tensor one
    assert not torch.equal(out[0][0], ops.linear(x, w, b, residual=r))
    assert not torch.equal(out[0][0], ops.linear(x, w, b, residual=r, fp8=True))
    with pytest.raises(ValueError, match="bogus"):
        ops.linear(x, w, b, fp8="bogus")


def test_use_fp8_linears_mx():
    model = nn.ModuleDict({"a": nn.Linear(32, 64), "odd": nn.Linear(48, 64), "lm_head": nn.Linear(32, 64)})
    keys = list(model.state_dict())
    with pytest.raises(ValueError):
        madnn.nn.use_fp8_linears(model, wgrad=True, mx=True)
    assert madnn.nn.use_fp8_linears(model, mx=True) == 1
    assert type(model["a"]) is madnn.nn.Fp8Linear and model["a"].fp8_mode == "mx"
    assert type(model["odd"]) is nn.Linear and type(model["lm_head"]) is nn.Linear
    assert list(model.state_dict()) == keys
