"""FP8 Linear on the GPU: the quantiser bit for bit against torch's casts, K17 exactly on small integers and within
a derived bound on random data, ``ops.linear(fp8=True)`` against ``reference.linear_fp8`` in fp64, and the model
conversion.  Bound (all cases): |y - ref| <= 2^-7 |ref| + K 2^-23 (|a| @ |b|^T) on the dequantised operands --
twice the bf16 output rounding plus the standard fp32 accumulation bound over K terms."""
import pytest
import torch
from torch import nn

import madnn
from madnn import ops
from madnn.ops import reference

pytestmark = pytest.mark.gpu
DT = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}


def _bound(ref, a_abs, b_abs, k):
    return 2.0 ** -7 * ref.abs() + k * 2.0 ** -23 * (a_abs @ b_abs.t())


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("R,C,ld", [(16, 16, 16), (70, 48, 48), (272, 144, 144), (272, 144, 160)])
def test_quantize_bit_exact(cuda, fmt, R, C, ld):
    g = torch.Generator().manual_seed(R + ld)
    # magnitudes over 15 binades: fp8 normals, subnormals and values that round to zero
    xh = (torch.randn(R, ld, generator=g) * torch.exp2(torch.randint(-12, 3, (R, ld), generator=g).float())).bfloat16()
    x = xh.to(cuda)[:, :C]
    q, qt, scale = ops.fp8_quantize(x, fmt, transpose=R % 16 == 0)
    want_scale = reference.fp8_scale(xh[:, :C].abs().max(), fmt)
    assert scale.dtype == torch.float32 and scale.shape == (1,) and scale.item() == want_scale.item()
    want = (xh[:, :C].float() * want_scale).to(DT[fmt]).view(torch.uint8)
    assert q.dtype == DT[fmt] and torch.equal(q.view(torch.uint8).cpu(), want)
    if R % 16 == 0:
        assert qt.dtype == DT[fmt] and torch.equal(qt.view(torch.uint8).cpu(), want.t())
    else:
        assert qt is None


def test_quantize_zeros(cuda):
    q, qt, scale = ops.fp8_quantize(torch.zeros(32, 48, device=cuda, dtype=torch.bfloat16), "e4m3", transpose=True)
    assert scale.item() == 1.0
    assert not q.view(torch.uint8).any() and not qt.view(torch.uint8).any()


@pytest.mark.parametrize("fa", ["e4m3", "e5m2"])
@pytest.mark.parametrize("K", [64, 128, 208])
def test_gemm_exact_on_small_integers(cuda, fa, K):
    g = torch.Generator().manual_seed(K)
    a = torch.randint(-1, 2, (33, K), generator=g).float()
    b = torch.randint(-1, 2, (40, K), generator=g).float()
    one = torch.ones(1, device=cuda)
    y = ops.fp8_gemm(a.to(DT[fa]).to(cuda), one, b.to(DT["e4m3"]).to(cuda), one)
    assert y.dtype == torch.bfloat16 and torch.equal(y.float().cpu(), a @ b.t())


@pytest.mark.parametrize("fa", ["e4m3", "e5m2"])
@pytest.mark.parametrize("has_bias,has_res", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("M,N,K", [(1, 8, 16), (33, 40, 272), (256, 256, 128), (300, 520, 400)])
def test_gemm_within_bound(cuda, fa, has_bias, has_res, M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    sa, sb = torch.tensor([8.0]), torch.tensor([0.25])
    a8 = (torch.randn(M, K, generator=g) * sa).to(DT[fa])
    b8 = (torch.randn(N, K, generator=g) * sb).to(DT["e4m3"])
    bias = torch.randn(N, generator=g) if has_bias else None
    res = torch.randn(M, N, generator=g).bfloat16() if has_res else None
    ad, bd = a8.double() / sa.double(), b8.double() / sb.double()
    ref = ad @ bd.t() + (bias.double() if has_bias else 0) + (res.double() if has_res else 0)
    y = ops.fp8_gemm(a8.to(cuda), sa.to(cuda), b8.to(cuda), sb.to(cuda), bias.to(cuda) if has_bias else None,
                     res.to(cuda) if has_res else None)
    err, tol = (y.double().cpu() - ref).abs(), _bound(ref, ad.abs(), bd.abs(), K)
    print("max err / bound", (err / tol.clamp_min(1e-300)).max().item())
    assert y.shape == (M, N) and (err <= tol).all()


def _linear_run(x, w, b, r, g, fp8):
    ts = [t.detach().clone().requires_grad_() for t in (x, w, b, r)]
    y = ops.linear(ts[0], ts[1], ts[2], fp8=fp8, residual=ts[3])
    y.backward(g)
    return y.detach(), [t.grad for t in ts]


@pytest.mark.parametrize("bias_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N", [48, 272])
def test_linear_against_fp64_reference(cuda, N, bias_dtype):
    torch.manual_seed(N)
    x, w = torch.randn(3, 37, 80).bfloat16(), (torch.randn(N, 80) / 8).bfloat16()
    b, r, g = torch.randn(N).to(bias_dtype), torch.randn(3, 37, N).bfloat16(), torch.randn(3, 37, N).bfloat16()
    y, (dx, dw, db, dr) = _linear_run(x.to(cuda), w.to(cuda), b.to(cuda), r.to(cuda), g.to(cuda), True)
    xd = x.double().requires_grad_()
    yr = reference.linear_fp8(xd, w.double(), b.double(), r.double())
    yr.backward(g.double())
    (x8, sx), (w8, sw), (g8, sg) = (reference.fp8_quantize(t, f) for t, f in ((x, "e4m3"), (w, "e4m3"), (g, "e5m2")))
    ax, aw, ag = x8.double().abs() / sx, w8.double().abs() / sw, g8.double().abs() / sg
    tol_y = _bound(yr.detach().reshape(-1, N), ax.reshape(-1, 80), aw, 80).view_as(yr)
    tol_dx = _bound(xd.grad.reshape(-1, 80), ag.reshape(-1, N), aw.t(), N).view_as(xd)
    assert ((y.double().cpu() - yr.detach()).abs() <= tol_y).all()
    assert ((dx.double().cpu() - xd.grad).abs() <= tol_dx).all()
    # weight, bias and residual gradients: the bf16 path's kernels on the same tensors
    _, (_, dw0, db0, dr0) = _linear_run(x.to(cuda), w.to(cuda), b.to(cuda), r.to(cuda), g.to(cuda), False)
    assert torch.equal(dw, dw0) and torch.equal(db, db0) and torch.equal(dr, dr0)


def test_linear_unsupported_shape_is_the_bf16_path(cuda):
    torch.manual_seed(72)
    args = [t.to(cuda) for t in (torch.randn(3, 37, 72).bfloat16(), torch.randn(48, 72).bfloat16(), torch.randn(48),
                                 torch.randn(3, 37, 48).bfloat16(), torch.randn(3, 37, 48).bfloat16())]
    assert not ops.fp8_linear_supported(args[0], args[1])
    (y1, g1), (y0, g0) = _linear_run(*args, True), _linear_run(*args, False)
    assert torch.equal(y1, y0) and all(torch.equal(a, b) for a, b in zip(g1, g0))


def test_use_fp8_linears_on_llama(cuda, monkeypatch):
    """Loss distance: cross entropy is 2-Lipschitz in the sup norm of the logits, and the two runs (K17 / the
    torch mirror, same recipe) can differ by at most one e4m3 step, 2^-3 relative, in what feeds the head."""
    from madnn.models.common import causal_lm_loss
    from madnn.models.llama import Llama, llama_config

    torch.manual_seed(0)
    cfg = llama_config("llama3-tiny")
    model = Llama(cfg).to(cuda).bfloat16()
    assert madnn.nn.use_fp8_linears(model) == 4 * cfg.layers
    assert type(model.head.lm_head) is nn.Linear and type(model.layers[0].mlp.down) is madnn.nn.Fp8Linear
    ids = torch.randint(0, cfg.vocab_size, (2, 32), device=cuda)
    calls, real, real_linear = [], ops._LinearFp8Fn.apply, ops.linear
    monkeypatch.setattr(ops._LinearFp8Fn, "apply", lambda *a: (calls.append(1), real(*a))[1])
    loss = causal_lm_loss(model(ids), ids)
    loss.backward()
    assert len(calls) == 4 * cfg.layers and torch.isfinite(loss)
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())
    monkeypatch.setattr(ops, "linear", lambda x, w, b=None, gelu=False, force_fn=False, residual=None, fp8=None:
                        reference.linear_fp8(x, w, b, residual) if fp8 else real_linear(x, w, b, gelu, force_fn, residual))
    logits = model(ids)
    want = causal_lm_loss(logits, ids)
    assert len(calls) == 4 * cfg.layers
    assert abs(loss.item() - want.item()) <= 2 * 2.0 ** -3 * logits.detach().float().abs().max().item()
