"""K17W, the fp8 weight-gradient GEMM on transposed LDS reads: exact on small integers (the proof of its fragment
map and of the split over tokens), within the fp8 path's bound on random data, ``ops.linear(fp8="wgrad")`` against
``reference.linear_fp8(wgrad=True)`` in fp64, and a converted model.  Bound: |dW - ref| <= 2^-7 |ref| +
M 2^-23 (|dy|^T @ |x|) on the dequantised operands -- twice the bf16 output rounding plus the standard fp32
accumulation bound over the M tokens."""
import pytest
import torch

import madnn
from madnn import ops
from madnn.ops import reference

pytestmark = pytest.mark.gpu
DT = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}


def _bound(ref, a_abs, b_abs, k):
    return 2.0 ** -7 * ref.abs() + k * 2.0 ** -23 * (a_abs @ b_abs.t())


@pytest.mark.parametrize("fg", ["e4m3", "e5m2"])
@pytest.mark.parametrize("splits", [0, 1, 3])
@pytest.mark.parametrize("M,N,K", [(16, 16, 16), (100, 48, 272), (128, 256, 256), (333, 272, 304)])
def test_wgrad_exact_on_small_integers(cuda, M, N, K, splits, fg):
    g = torch.Generator().manual_seed(M + N + K)
    dy = torch.randint(-1, 2, (M, N), generator=g).float()
    x = torch.randint(-1, 2, (M, K), generator=g).float()
    ref = dy.t() @ x
    assert ref.abs().max() <= 256   # every sum is a bf16 integer
    one = torch.ones(1, device=cuda)
    dw = ops.fp8_wgrad(dy.to(DT[fg]).to(cuda), one, x.to(DT["e4m3"]).to(cuda), one, splits=splits)
    assert dw.dtype == torch.bfloat16 and dw.shape == (N, K) and torch.equal(dw.float().cpu(), ref)


@pytest.mark.parametrize("splits", [0, 2])
@pytest.mark.parametrize("M,N,K,into", [(1, 16, 16, False), (111, 48, 80, True), (300, 520, 400, False)])
def test_wgrad_within_bound(cuda, M, N, K, into, splits):
    g = torch.Generator().manual_seed(M + N + K)
    sg, sx = torch.tensor([8.0]), torch.tensor([0.25])
    g8 = (torch.randn(M, N, generator=g) * sg).to(DT["e5m2"])
    x8 = (torch.randn(M, K, generator=g) * sx).to(DT["e4m3"])
    gd, xd = g8.double() / sg.double(), x8.double() / sx.double()
    ref = gd.t() @ xd
    out = torch.empty(N, K, device=cuda, dtype=torch.bfloat16) if into else None
    dw = ops.fp8_wgrad(g8.to(cuda), sg.to(cuda), x8.to(cuda), sx.to(cuda), out=out, splits=splits)
    assert not into or dw.untyped_storage().data_ptr() == out.untyped_storage().data_ptr()
    err, tol = (dw.double().cpu() - ref).abs(), _bound(ref, gd.abs().t(), xd.abs().t(), M)
    print("max err / bound", (err / tol.clamp_min(1e-300)).max().item())
    assert dw.shape == (N, K) and (err <= tol).all()


def _linear_run(x, w, b, r, g, fp8):
    saved = []
    ts = [t.detach().clone().requires_grad_() for t in (x, w, b, r)]
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append((t.dtype, t.numel())), t)[1], lambda t: t):
        y = ops.linear(ts[0], ts[1], ts[2], fp8=fp8, residual=ts[3])
    y.backward(g)
    return y.detach(), [t.grad for t in ts], saved


@pytest.mark.parametrize("bias_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N", [48, 272])
def test_linear_wgrad_against_fp64_reference(cuda, N, bias_dtype):
    torch.manual_seed(N)
    x, w = torch.randn(3, 37, 80).bfloat16(), (torch.randn(N, 80) / 8).bfloat16()
    b, r, g = torch.randn(N).to(bias_dtype), torch.randn(3, 37, N).bfloat16(), torch.randn(3, 37, N).bfloat16()
    dev = [t.to(cuda) for t in (x, w, b, r, g)]
    y, (dx, dw, db, dr), saved = _linear_run(*dev, "wgrad")
    xd, wd = x.double().requires_grad_(), w.double().requires_grad_()
    yr = reference.linear_fp8(xd, wd, b.double(), r.double(), wgrad=True)
    yr.backward(g.double())
    (x8, sx), (w8, sw), (g8, sg) = (reference.fp8_quantize(t, f) for t, f in ((x, "e4m3"), (w, "e4m3"), (g, "e5m2")))
    ax, aw, ag = x8.double().abs() / sx, w8.double().abs() / sw, g8.double().abs() / sg
    tol_y = _bound(yr.detach().reshape(-1, N), ax.reshape(-1, 80), aw, 80).view_as(yr)
    tol_dx = _bound(xd.grad.reshape(-1, 80), ag.reshape(-1, N), aw.t(), N).view_as(xd)
    tol_dw = _bound(wd.grad, ag.reshape(-1, N).t(), ax.reshape(-1, 80).t(), 111)
    assert ((y.double().cpu() - yr.detach()).abs() <= tol_y).all()
    assert ((dx.double().cpu() - xd.grad).abs() <= tol_dx).all()
    assert dw.shape == w.shape and ((dw.double().cpu() - wd.grad).abs() <= tol_dw).all()
    # bias and residual gradients: the bf16 path's kernels on the same tensors
    _, (_, _, db0, dr0), _ = _linear_run(*dev, False)
    assert torch.equal(db, db0) and torch.equal(dr, dr0)
    # what the backward keeps of x: its e4m3 image with "wgrad", the bf16 tensor with fp8=True
    _, _, saved1 = _linear_run(*dev, True)
    assert (torch.float8_e4m3fn, x.numel()) in saved and (torch.bfloat16, x.numel()) not in saved
    assert (torch.bfloat16, x.numel()) in saved1 and (torch.float8_e4m3fn, x.numel()) not in saved1


def test_use_fp8_linears_wgrad_on_llama(cuda, monkeypatch):
    from madnn.models.common import causal_lm_loss
    from madnn.models.llama import Llama, llama_config

    torch.manual_seed(0)
    cfg = llama_config("llama3-tiny")
    model = Llama(cfg).to(cuda).bfloat16()
    assert madnn.nn.use_fp8_linears(model, wgrad=True) == 4 * cfg.layers
    ids = torch.randint(0, cfg.vocab_size, (2, 32), device=cuda)
    assert ops.load_kernels()
    calls, real = [], torch.ops.madnn.fp8_wgrad
    monkeypatch.setattr(torch.ops.madnn, "fp8_wgrad", lambda *a: (calls.append(1), real(*a))[1])
    loss = causal_lm_loss(model(ids), ids)
    loss.backward()
    assert len(calls) == 4 * cfg.layers and torch.isfinite(loss)
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())
