"""The host mirrors of the MX weight gradient (no GPU): the column-blocked reference quantiser's properties at a
ragged row count, ``ops.linear(fp8="mx_wgrad")`` on CPU tensors and the model conversion."""
import pytest
import torch
from torch import nn

import madnn
from madnn import ops
from madnn.ops import reference


@pytest.mark.parametrize("fmt,fmax,emax,mant,emin", [("e4m3", 448.0, 8, 3, -6), ("e5m2", 57344.0, 15, 2, -14)])
def test_mx_quantize_columns_properties(fmt, fmax, emax, mant, emin):
    R, C = 70, 64                                       # two whole 32-row blocks and one of 6 rows
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(R, C, generator=g) * torch.exp2(torch.randint(-12, 3, (R, C), generator=g).float())).bfloat16()
    x[32:64, 3] = 0
    _, _, qc, ec = ops.mx_quantize(x, fmt, columns=True)
    assert qc.shape == (R, C) and ec.dtype == torch.uint8 and ec.shape == (3, C)
    xp = torch.cat([x.double(), torch.zeros(96 - R, C, dtype=torch.float64)]).view(3, 32, C)
    amax = xp.abs().amax(1)
    want = (torch.floor(torch.log2(amax.clamp_min(2.0 ** -140))) + 127 - emax).clamp(0, 254)
    want = torch.where(amax == 0, torch.full_like(want, 127), want)
    assert torch.equal(ec.double(), want) and ec[1, 3] == 127
    scale = torch.exp2(ec.double() - 127).unsqueeze(1).expand(3, 32, C).reshape(96, C)[:R]
    v = x.double() / scale                              # what the cast sees
    ulp_half = torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** emin))) - mant - 1)
    err, sat = (qc.double() - v).abs(), v.abs() > fmax
    assert (err[~sat] <= ulp_half[~sat]).all() and (qc.double()[sat].abs() == fmax).all()
    assert torch.equal(reference.mx_dequantize_columns(qc, ec, torch.float64), qc.double() * scale)
    with pytest.raises(ValueError):
        ops.mx_quantize(x, fmt, transpose=True, columns=True)


@pytest.mark.parametrize("has_res", [False, True])
def test_linear_mx_wgrad_on_cpu_is_the_reference(has_res):
    torch.manual_seed(1)
    x, w, b = torch.randn(3, 15, 64).bfloat16(), torch.randn(32, 64).bfloat16(), torch.randn(32).bfloat16()
    r = torch.randn(3, 15, 32).bfloat16() if has_res else None
    out = []
    for fn in (lambda *a: ops.linear(a[0], a[1], a[2], fp8="mx_wgrad", residual=r),
               lambda *a: reference.linear_mx(*a, r, wgrad=True),
               lambda *a: ops.linear(a[0], a[1], a[2], fp8="mx", residual=r)):
        ts = [t.clone().requires_grad_() for t in (x, w, b)]
        y = fn(*ts)
        (y.float() * torch.arange(32)).sum().backward()
        out.append([y.detach()] + [t.grad for t in ts])
    assert all(torch.equal(p, q) for p, q in zip(out[0], out[1]))
    # against "mx": the same y, dx and db, another dw
    assert all(torch.equal(out[0][i], out[2][i]) for i in (0, 1, 3)) and not torch.equal(out[0][2], out[2][2])
    # ops.mx_wgrad on CPU tensors is the same product
    g2 = torch.arange(32).float().expand(45, 32).bfloat16()
    _, _, gc, egc = ops.mx_quantize(g2, columns=True)
    _, _, xc, exc = ops.mx_quantize(x.reshape(45, 64), columns=True)
    assert torch.equal(ops.mx_wgrad(gc, egc, xc, exc), out[0][2])


def test_use_fp8_linears_mx_wgrad():
    model = nn.ModuleDict({"a": nn.Linear(32, 64), "odd": nn.Linear(48, 64), "lm_head": nn.Linear(32, 64)})
    assert madnn.nn.use_fp8_linears(model, mx="wgrad") == 1
    assert type(model["a"]) is madnn.nn.Fp8Linear and model["a"].fp8_mode == "mx_wgrad"
    assert type(model["odd"]) is nn.Linear
    with pytest.raises(ValueError):
        madnn.nn.use_fp8_linears(model, mx="bogus")
