"""MX weight gradient on the GPU: the quantiser's column-blocked image bit for bit against
``reference.mx_quantize_columns``, K17XW's scale routing exactly on {-1, 0, 1} data with scales in {1/2, 1, 2}, K17XW
within the fp8 tests' bound on random data, ``ops.linear(fp8="mx_wgrad")`` against ``reference.linear_mx(wgrad=True)``
in fp64, and the model conversion.  Bound: |dW - ref| <= 2^-7 |ref| + M 2^-23 (|dq dy|^T @ |dq x|)
(tests/test_mx_gpu.py)."""
import pytest
import torch

import madnn
from madnn import ops
from madnn.ops import reference

pytestmark = pytest.mark.gpu
DT = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
dqc = reference.mx_dequantize_columns


def _bound(ref, g_abs, x_abs, m):
    return 2.0 ** -7 * ref.abs() + m * 2.0 ** -23 * (g_abs.t() @ x_abs)


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("R,C,ld", [(32, 32, 32), (70, 96, 96), (111, 64, 64), (96, 160, 192)])
def test_quantize_columns_bit_exact(cuda, fmt, R, C, ld):
    g = torch.Generator().manual_seed(R + ld)
    # the input of test_mx_gpu.py::test_quantize_bit_exact, with the zero block and the clamp case down a column too
    xh = (torch.randn(R, ld, generator=g) * torch.exp2(torch.randint(-12, 3, (R, ld), generator=g).float())).bfloat16()
    xh[0, :32] = 0
    xh[1, :32] = xh[1, :32].clamp(-1, 1)
    xh[1, 5] = -7.5
    xh[:32, 7] = 0                                       # an all-zero column block
    xh[-30:, 9] = xh[-30:, 9].clamp(-1, 1)
    xh[-1, 9] = -7.5                                     # the explicit clamp, in the (ragged) last block
    x = xh.to(cuda)[:, :C]
    q, e, qc, ec = ops.mx_quantize(x, fmt, columns=True)
    q0, e0, _, _ = ops.mx_quantize(x, fmt)
    assert torch.equal(q.view(torch.uint8), q0.view(torch.uint8)) and torch.equal(e, e0)
    want_q, want_e = reference.mx_quantize_columns(xh[:, :C], fmt)
    assert want_e[0, 7] == 127 and want_q[-1, 9].float() == -reference.FP8_FORMATS[fmt][1]
    assert qc.dtype == DT[fmt] and qc.shape == (R, C) and ec.dtype == torch.uint8 and ec.shape == ((R + 31) // 32, C)
    assert torch.equal(ec.cpu(), want_e) and torch.equal(qc.view(torch.uint8).cpu(), want_q.view(torch.uint8))


@pytest.mark.parametrize("fg", ["e4m3", "e5m2"])
@pytest.mark.parametrize("splits", [1, 3, 0])
@pytest.mark.parametrize("N,K", [(16, 48), (272, 304)])
@pytest.mark.parametrize("M", [32, 111, 192, 300])
def test_scale_routing_exact(cuda, fg, splits, N, K, M):
    """Every product is 0 or +-2^j, j in -2..2, and |partial sums| < 4 M < 2^11: fp32 accumulation is exact in any
    order and across splits, so one wrong block, lane half, row, step or split changes the result."""
    g = torch.Generator().manual_seed(M + K)
    dy8 = torch.randint(-1, 2, (M, N), generator=g).float().to(DT[fg])
    x8 = torch.randint(-1, 2, (M, K), generator=g).float().to(DT["e4m3"])
    eg = torch.randint(126, 129, ((M + 31) // 32, N), generator=g, dtype=torch.uint8)
    ex = torch.randint(126, 129, ((M + 31) // 32, K), generator=g, dtype=torch.uint8)
    ref = dqc(dy8, eg, torch.float64).t() @ dqc(x8, ex, torch.float64)
    dw = ops.mx_wgrad(dy8.to(cuda), eg.to(cuda), x8.to(cuda), ex.to(cuda), splits=splits)
    assert dw.dtype == torch.bfloat16 and torch.equal(dw.cpu(), ref.to(torch.bfloat16))


@pytest.mark.parametrize("fg,fx", [("e4m3", "e4m3"), ("e5m2", "e5m2")])
@pytest.mark.parametrize("M,N,K,views,into", [(1, 16, 16, False, False), (111, 48, 272, True, False),
                                              (111, 48, 272, False, True), (300, 520, 416, False, False)])
def test_wgrad_within_bound(cuda, fg, fx, M, N, K, views, into):
    g = torch.Generator().manual_seed(M + N + K)
    dy8 = (torch.randn(M, N, generator=g) * 8).to(DT[fg])
    x8 = (torch.randn(M, K, generator=g) * 0.25).to(DT[fx])
    eg = torch.randint(100, 151, ((M + 31) // 32, N), generator=g, dtype=torch.uint8)
    ex = torch.randint(100, 151, ((M + 31) // 32, K), generator=g, dtype=torch.uint8)
    gd, xd = dqc(dy8, eg, torch.float64), dqc(x8, ex, torch.float64)
    ref = gd.t() @ xd
    eg_d, ex_d = eg.to(cuda), ex.to(cuda)
    if views:   # rows that start at odd addresses: the copy path
        eg_d, ex_d = (torch.cat([t.new_full((t.shape[0], 1), 255), t], 1)[:, 1:] for t in (eg_d, ex_d))
        assert eg_d.data_ptr() % 4 and not eg_d.is_contiguous()
    out = torch.empty(N, K, dtype=torch.bfloat16, device=cuda) if into else None
    dw = ops.mx_wgrad(dy8.to(cuda), eg_d, x8.to(cuda), ex_d, out=out)
    assert not into or dw.data_ptr() == out.data_ptr()
    err, tol = (dw.double().cpu() - ref).abs(), _bound(ref, gd.abs(), xd.abs(), M)
    print("max err / bound", (err / tol.clamp_min(1e-300)).max().item())
    assert dw.shape == (N, K) and torch.isfinite(dw).all() and (err <= tol).all()


def _linear_run(x, w, b, r, g, fp8, saved=None):
    ts = [t.detach().clone().requires_grad_() for t in (x, w, b, r)]
    y = ops.linear(ts[0], ts[1], ts[2], fp8=fp8, residual=ts[3])
    if saved is not None:
        saved.extend(y.grad_fn.saved_tensors)
    y.backward(g)
    return y.detach(), [t.grad for t in ts]


@pytest.mark.parametrize("N", [64, 288])
def test_linear_against_fp64_reference(cuda, N):
    torch.manual_seed(N)
    x, w = torch.randn(3, 37, 96).bfloat16(), (torch.randn(N, 96) / 8).bfloat16()
    b, r, g = torch.randn(N), torch.randn(3, 37, N).bfloat16(), torch.randn(3, 37, N).bfloat16()
    dev = [t.to(cuda) for t in (x, w, b, r, g)]
    saved = []
    y, (dx, dw, db, dr) = _linear_run(*dev, "mx_wgrad", saved)
    y1, (dx1, _, _, _) = _linear_run(*dev, "mx")
    _, (_, _, db0, dr0) = _linear_run(*dev, False)
    assert torch.equal(y, y1) and torch.equal(dx, dx1) and torch.equal(db, db0) and torch.equal(dr, dr0)
    assert not any(t.dtype == torch.bfloat16 and t.numel() == x.numel() for t in saved)
    wd = w.double().requires_grad_()
    reference.linear_mx(x.double(), wd, b.double(), r.double(), wgrad=True).backward(g.double())
    ag, ax = (dqc(*reference.mx_quantize_columns(t.reshape(111, -1), "e4m3"), torch.float64).abs() for t in (g, x))
    assert ((dw.double().cpu() - wd.grad).abs() <= _bound(wd.grad, ag, ax, 111)).all()


def test_linear_unsupported_shape_is_the_bf16_path(cuda):
    torch.manual_seed(80)
    args = [t.to(cuda) for t in (torch.randn(3, 37, 80).bfloat16(), torch.randn(64, 80).bfloat16(), torch.randn(64),
                                 torch.randn(3, 37, 64).bfloat16(), torch.randn(3, 37, 64).bfloat16())]
    (y1, g1), (y0, g0) = _linear_run(*args, "mx_wgrad"), _linear_run(*args, False)
    assert torch.equal(y1, y0) and all(torch.equal(a, b) for a, b in zip(g1, g0))


def test_use_fp8_linears_mx_wgrad_on_llama(cuda, monkeypatch):
    from madnn.models.common import causal_lm_loss
    from madnn.models.llama import Llama, llama_config

    torch.manual_seed(0)
    cfg = llama_config("llama3-tiny")
    model = Llama(cfg).to(cuda).bfloat16()
    assert madnn.nn.use_fp8_linears(model, mx="wgrad") == 4 * cfg.layers
    assert model.layers[0].mlp.down.fp8_mode == "mx_wgrad"
    ids = torch.randint(0, cfg.vocab_size, (2, 32), device=cuda)
    calls, real = [], ops._LinearMxFn.apply
    monkeypatch.setattr(ops._LinearMxFn, "apply", lambda *a: (calls.append(a[4]), real(*a))[1])
    loss = causal_lm_loss(model(ids), ids)
    loss.backward()
    assert calls == [True] * (4 * cfg.layers) and torch.isfinite(loss)
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())
