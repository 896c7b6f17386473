"""MX FP8 Linear on the GPU: the one-pass block quantiser bit for bit against ``reference.mx_quantize``, K17X's
scale routing exactly on {-1, 0, 1} data with scales in {1/2, 1, 2}, K17X within the fp8 tests' bound on random
data, ``ops.linear(fp8="mx")`` against ``reference.linear_mx`` in fp64, and the model conversion.  Bound (all
cases): |y - ref| <= 2^-7 |ref| + K 2^-23 (|a| @ |b|^T) on the dequantised operands (tests/test_fp8_gpu.py)."""
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
@pytest.mark.parametrize("R,C,ld", [(32, 32, 32), (70, 96, 96), (96, 160, 160), (96, 160, 192)])
def test_quantize_bit_exact(cuda, fmt, R, C, ld):
    g = torch.Generator().manual_seed(R + ld)
    # magnitudes over 15 binades inside every block: fp8 normals, subnormals and values that round to zero
    xh = (torch.randn(R, ld, generator=g) * torch.exp2(torch.randint(-12, 3, (R, ld), generator=g).float())).bfloat16()
    xh[0, :32] = 0                                       # an all-zero block
    xh[1, :32] = xh[1, :32].clamp(-1, 1)
    xh[1, 5] = -7.5                                      # amax 1.875 * 2^2: amax / X exceeds FMAX, the explicit clamp
    x = xh.to(cuda)[:, :C]
    tr = R % 32 == 0
    q, e, qt, et = ops.mx_quantize(x, fmt, transpose=tr)
    want_q, want_e = reference.mx_quantize(xh[:, :C], fmt)
    assert want_e[0, 0] == 127 and want_q[1, 5].float() == -reference.FP8_FORMATS[fmt][1]
    assert q.dtype == DT[fmt] and q.shape == (R, C) and e.dtype == torch.uint8 and e.shape == (R, C // 32)
    assert torch.equal(e.cpu(), want_e) and torch.equal(q.view(torch.uint8).cpu(), want_q.view(torch.uint8))
    assert not q.view(torch.uint8)[0, :32].any()
    if tr:
        want_qt, want_et = reference.mx_quantize(xh[:, :C].t(), fmt)
        assert qt.dtype == DT[fmt] and qt.shape == (C, R) and et.shape == (C, R // 32)
        assert torch.equal(et.cpu(), want_et) and torch.equal(qt.view(torch.uint8).cpu(), want_qt.view(torch.uint8))
    else:
        assert qt is None and et is None


@pytest.mark.parametrize("fa", ["e4m3", "e5m2"])
@pytest.mark.parametrize("K", [32, 128, 160, 416])
@pytest.mark.parametrize("M,N", [(33, 40), (300, 264)])
def test_scale_routing_exact(cuda, fa, M, N, K):
    """Every product is 0 or +-2^j, j in -2..2, and |partial sums| < 4 K < 2^11: fp32 accumulation is exact in any
    order, so one wrong scale byte, row, lane half or K step changes the result."""
    g = torch.Generator().manual_seed(M + K)
    a8 = torch.randint(-1, 2, (M, K), generator=g).float().to(DT[fa])
    b8 = torch.randint(-1, 2, (N, K), generator=g).float().to(DT["e4m3"])
    ea = torch.randint(126, 129, (M, K // 32), generator=g, dtype=torch.uint8)
    eb = torch.randint(126, 129, (N, K // 32), generator=g, dtype=torch.uint8)
    ref = reference.mx_dequantize(a8, ea, torch.float64) @ reference.mx_dequantize(b8, eb, torch.float64).t()
    y = ops.mx_gemm(a8.to(cuda), ea.to(cuda), b8.to(cuda), eb.to(cuda))
    assert y.dtype == torch.bfloat16 and torch.equal(y.cpu(), ref.to(torch.bfloat16))


@pytest.mark.parametrize("fa,fb", [("e4m3", "e4m3"), ("e5m2", "e5m2")])
@pytest.mark.parametrize("has_bias,has_res", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("M,N,K,wide", [(1, 8, 32, False), (33, 40, 288, False), (33, 40, 288, True),
                                        (256, 256, 128, False), (300, 520, 416, False)])
def test_gemm_within_bound(cuda, fa, fb, has_bias, has_res, M, N, K, wide):
    g = torch.Generator().manual_seed(M + N + K)
    a8 = (torch.randn(M, K, generator=g) * 8).to(DT[fa])
    b8 = (torch.randn(N, K, generator=g) * 0.25).to(DT[fb])
    ea = torch.randint(100, 151, (M, K // 32), generator=g, dtype=torch.uint8)
    eb = torch.randint(100, 151, (N, K // 32), generator=g, dtype=torch.uint8)
    bias = torch.randn(N, generator=g) if has_bias else None
    res = torch.randn(M, N, generator=g).bfloat16() if has_res else None
    ad, bd = reference.mx_dequantize(a8, ea, torch.float64), reference.mx_dequantize(b8, eb, torch.float64)
    ref = ad @ bd.t() + (bias.double() if has_bias else 0) + (res.double() if has_res else 0)
    ea_d, eb_d = ea.to(cuda), eb.to(cuda)
    if wide:   # views of word-aligned buffers, read in place: the bytes beside the scales are 255 (2^128)
        ea_d, eb_d = (torch.full((t.shape[0], 16), 255, dtype=torch.uint8, device=cuda) for t in (ea, eb))
        ea_d[:, :K // 32], eb_d[:, :K // 32] = ea.to(cuda), eb.to(cuda)
        ea_d, eb_d = ea_d[:, :K // 32], eb_d[:, :K // 32]
    y = ops.mx_gemm(a8.to(cuda), ea_d, b8.to(cuda), eb_d, bias.to(cuda) if has_bias else None,
                    res.to(cuda) if has_res else None)
    err, tol = (y.double().cpu() - ref).abs(), _bound(ref, ad.abs(), bd.abs(), K)
    print("max err / bound", (err / tol.clamp_min(1e-300)).max().item())
    assert y.shape == (M, N) and torch.isfinite(y).all() and (err <= tol).all()


def _linear_run(x, w, b, r, g, fp8):
    ts = [t.detach().clone().requires_grad_() for t in (x, w, b, r)]
    y = ops.linear(ts[0], ts[1], ts[2], fp8=fp8, residual=ts[3])
    y.backward(g)
    return y.detach(), [t.grad for t in ts]


@pytest.mark.parametrize("bias_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N", [64, 288])
def test_linear_against_fp64_reference(cuda, N, bias_dtype):
    torch.manual_seed(N)
    x, w = torch.randn(3, 37, 96).bfloat16(), (torch.randn(N, 96) / 8).bfloat16()
    b, r, g = torch.randn(N).to(bias_dtype), torch.randn(3, 37, N).bfloat16(), torch.randn(3, 37, N).bfloat16()
    y, (dx, dw, db, dr) = _linear_run(x.to(cuda), w.to(cuda), b.to(cuda), r.to(cuda), g.to(cuda), "mx")
    xd = x.double().requires_grad_()
    yr = reference.linear_mx(xd, w.double(), b.double(), r.double())
    yr.backward(g.double())
    ax, aw, ag, awt = (reference.mx_dequantize(*reference.mx_quantize(t, "e4m3"), torch.float64).abs()
                       for t in (x, w, g, w.t()))
    tol_y = _bound(yr.detach().reshape(-1, N), ax.reshape(-1, 96), aw, 96).view_as(yr)
    tol_dx = _bound(xd.grad.reshape(-1, 96), ag.reshape(-1, N), awt, N).view_as(xd)
    assert ((y.double().cpu() - yr.detach()).abs() <= tol_y).all()
    assert ((dx.double().cpu() - xd.grad).abs() <= tol_dx).all()
    # weight, bias and residual gradients: the bf16 path's kernels on the same tensors
    _, (_, dw0, db0, dr0) = _linear_run(x.to(cuda), w.to(cuda), b.to(cuda), r.to(cuda), g.to(cuda), False)
    assert torch.equal(dw, dw0) and torch.equal(db, db0) and torch.equal(dr, dr0)


def test_linear_unsupported_shape_is_the_bf16_path(cuda):
    torch.manual_seed(80)
    args = [t.to(cuda) for t in (torch.randn(3, 37, 80).bfloat16(), torch.randn(64, 80).bfloat16(), torch.randn(64),
                                 torch.randn(3, 37, 64).bfloat16(), torch.randn(3, 37, 64).bfloat16())]
    assert not ops.mx_linear_supported(args[0], args[1])
    (y1, g1), (y0, g0) = _linear_run(*args, "mx"), _linear_run(*args, False)
    assert torch.equal(y1, y0) and all(torch.equal(a, b) for a, b in zip(g1, g0))


def test_use_fp8_linears_mx_on_llama(cuda, monkeypatch):
    """Loss distance as in test_fp8_gpu.py: cross entropy is 2-Lipschitz in the sup norm of the logits, and the two
    runs (K17X / the torch mirror, same recipe) can differ by at most one e4m3 step, 2^-3 relative, in what feeds
    the head."""
    from madnn.models.common import causal_lm_loss
    from madnn.models.llama import Llama, llama_config

    torch.manual_seed(0)
    cfg = llama_config("llama3-tiny")
    model = Llama(cfg).to(cuda).bfloat16()
    assert madnn.nn.use_fp8_linears(model, mx=True) == 4 * cfg.layers
    assert type(model.head.lm_head) is nn.Linear and model.layers[0].mlp.down.fp8_mode == "mx"
    ids = torch.randint(0, cfg.vocab_size, (2, 32), device=cuda)
    calls, real, real_linear = [], ops._LinearMxFn.apply, ops.linear
    monkeypatch.setattr(ops._LinearMxFn, "apply", lambda *a: (calls.append(1), real(*a))[1])
    loss = causal_lm_loss(model(ids), ids)
    loss.backward()
    assert len(calls) == 4 * cfg.layers and torch.isfinite(loss)
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())
    monkeypatch.setattr(ops, "linear", lambda x, w, b=None, gelu=False, force_fn=False, residual=None, fp8=None:
                        reference.linear_mx(x, w, b, residual) if fp8 else real_linear(x, w, b, gelu, force_fn, residual))
    logits = model(ids)
    want = causal_lm_loss(logits, ids)
    assert len(calls) == 4 * cfg.layers
    assert abs(loss.item() - want.item()) <= 2 * 2.0 ** -3 * logits.detach().float().abs().max().item()
