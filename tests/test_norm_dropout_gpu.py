"""Hidden (residual) dropout inside the kernels: K3 with ``dropout_p`` (mask applied while forming
x + residual, regenerated in the backward), K16 ``dropout_add``, and the GPT-2 / BERT routing that
keeps the fused paths with ``dropout > 0``.  The references are fp32 PyTorch built with the host mask
(``reference.hidden_dropout_mask``); the tolerances are those of the existing K3 tests of
``tests/test_kernels_gpu.py`` for the same mode and dtypes (test_norm_fused_residual: y / s 3e-2, input
gradients atol 8e-2 rtol 5e-2; test_norm_fwd_bwd: weight / bias gradients 5e-2 * sqrt(rows), rtol 5e-2)."""
import math

import pytest
import torch
import torch.nn.functional as F

from madnn import ops
from madnn.ops import reference as R

pytestmark = pytest.mark.gpu

SEED, OFFSET = 0xFEDCBA9876543210, (3 << 32) | 8   # 64-bit seed, offset with high bits set
RNG = (SEED, OFFSET)

# rows, H -> (TPR, NC) of norm.hip's pick_cfg
SHAPES = [(5, 64),        # 64, 1: lanes with col >= H
          (37, 768),      # 64, 2: partly filled second chunk
          (7, 1024),      # 64, 2: full row at one row per wave
          (9, 1536),      # 128, 2
          (3, 4096),      # 256, 2
          (3, 8192),      # 256, 4
          (33001, 64)]    # 64, 1: grid-stride in both the forward and the backward


def _rp(p):
    return 256.0 / R.attention_dropout_threshold(p)


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12))


def _norm_case(cuda, rows, H, rms, wdt, p, seed=0):
    torch.manual_seed(seed)
    x = (torch.randn(rows, H, device=cuda) * 2 + 0.5).bfloat16().requires_grad_(True)
    r = torch.randn(rows, H, device=cuda).bfloat16().requires_grad_(True)
    w = (torch.rand(H, device=cuda) + 0.5).to(wdt).requires_grad_(True)
    b = None if rms else (torch.randn(H, device=cuda) * 0.1).to(wdt).requires_grad_(True)
    g1, g2 = torch.randn(rows, H, device=cuda).bfloat16(), torch.randn(rows, H, device=cuda).bfloat16()
    return x, r, w, b, g1, g2


def _run_fused(x, r, w, b, g1, g2, rms, p, rng=RNG):
    for t in (x, r, w, b):
        if t is not None:
            t.grad = None
    if rms:
        y, s = ops.rms_norm(x, w, eps=1e-6, residual=r, dropout_p=p, rng=rng)
    else:
        y, s = ops.layer_norm(x, w, b, eps=1e-5, residual=r, dropout_p=p, rng=rng)
    torch.autograd.backward([y, s], [g1, g2])
    return y.detach(), s.detach(), x.grad, r.grad, w.grad, (b.grad if b is not None else None)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("rows,H", SHAPES)
def test_norm_dropout_against_fp32_reference_with_the_host_mask(cuda, rows, H, rms, wdt, p):
    keep = R.hidden_dropout_mask(rows, H, p, SEED, OFFSET).to(cuda)
    km = ops._need_native("hidden_dropout_mask").hidden_dropout_mask(rows, H, p, *ops._dropout_args(None, p, RNG)[1:])
    assert torch.equal(km.bool(), keep), "the kernel mask differs from the host mirror"

    x, r, w, b, g1, g2 = _norm_case(cuda, rows, H, rms, wdt, p)
    y, s, dx, dr, dw, db = _run_fused(x, r, w, b, g1, g2, rms, p)

    xr, rr = x.detach().float().requires_grad_(True), r.detach().float().requires_grad_(True)
    wr = w.detach().float().requires_grad_(True)
    br = None if rms else b.detach().float().requires_grad_(True)
    sr = rr + _rp(p) * keep * xr
    sr.retain_grad()
    yr = R.norm(sr, wr, br, 1e-6 if rms else 1e-5, rms)
    torch.autograd.backward([yr, sr], [g1.float(), g2.float()])

    drop = ~keep
    assert 0 < int(drop.sum()) < keep.numel()
    assert torch.equal(s[drop], r.detach()[drop]), "s != residual at a dropped position"
    assert int((dx[drop] != 0).sum()) == 0, "dx != 0 at a dropped position"
    torch.testing.assert_close(s.float(), sr.detach(), atol=3e-2, rtol=3e-2)
    torch.testing.assert_close(y.float(), yr.detach(), atol=3e-2, rtol=3e-2)
    torch.testing.assert_close(dr.float(), sr.grad, atol=8e-2, rtol=5e-2)      # dres_out: dropped and kept alike
    torch.testing.assert_close(dr.float(), rr.grad, atol=8e-2, rtol=5e-2)
    torch.testing.assert_close(dx.float(), xr.grad, atol=8e-2, rtol=5e-2)
    assert dx.data_ptr() != dr.data_ptr()
    gtol = 5e-2
    torch.testing.assert_close(dw.float(), wr.grad, atol=gtol * math.sqrt(rows), rtol=gtol)
    if not rms:
        torch.testing.assert_close(db.float(), br.grad, atol=gtol * math.sqrt(rows), rtol=gtol)


@pytest.mark.parametrize("row0", [2 ** 32 - 2, (3 << 32) + 5])
def test_kernel_mask_counts_rows_in_64_bits(cuda, row0):
    """Rows past 2**32 (reached through the test kernel's row offset): the high row word is part of the
    Philox counter on the device as in the host mirror."""
    _, seed, offset = ops._dropout_args(None, 0.3, RNG)
    km = ops._need_native("hidden_dropout_mask").hidden_dropout_mask(4, 72, 0.3, seed, offset, row0)
    assert torch.equal(km.bool().cpu(), R.hidden_dropout_mask(4, 72, 0.3, SEED, OFFSET, row0=row0))


@pytest.mark.parametrize("rows,H", [(37, 768), (3, 8192), (33001, 64)])
def test_norm_dropout_same_rng_is_bit_identical_and_offsets_differ(cuda, rows, H):
    case = _norm_case(cuda, rows, H, False, torch.float32, 0.1)
    a = [t.clone() for t in _run_fused(*case, False, 0.1)]
    b = _run_fused(*case, False, 0.1)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    c = _run_fused(*case, False, 0.1, rng=(SEED, OFFSET + 4))
    assert not torch.equal(a[1], c[1])


def test_norm_dropout_colsum_is_of_the_masked_gradient(cuda, monkeypatch):
    """A biased Linear feeding K3 with dropout: the Linear's bias gradient is the column sum of
    rp * m * dh that the norm backward hands it (no column-sum pass of its own)."""
    calls = []
    real = ops.bias_grad
    monkeypatch.setattr(ops, "bias_grad", lambda *a, **k: calls.append(1) or real(*a, **k))
    torch.manual_seed(12)
    p = 0.5
    x = torch.randn(4, 96, 256, device=cuda, dtype=torch.bfloat16, requires_grad=True)
    w = (torch.randn(512, 256, device=cuda, dtype=torch.bfloat16) * 0.06).requires_grad_()
    b = (torch.randn(512, device=cuda, dtype=torch.bfloat16) * 0.1).requires_grad_()
    lw = (torch.rand(512, device=cuda) + 0.5).requires_grad_()
    lb = (torch.randn(512, device=cuda) * 0.1).requires_grad_()
    r = torch.randn(4, 96, 512, device=cuda, dtype=torch.bfloat16, requires_grad=True)
    g1, g2 = torch.randn(4, 96, 512, device=cuda), torch.randn(4, 96, 512, device=cuda)
    y, s = ops.layer_norm(ops.linear(x, w, b), lw, lb, residual=r, dropout_p=p, rng=RNG)
    ((y.float() * g1).sum() + (s.float() * g2).sum()).backward()
    assert not calls, "the Linear ran its own bias column-sum pass"
    keep = R.hidden_dropout_mask(4 * 96, 512, p, SEED, OFFSET).to(cuda).view(4, 96, 512)
    xf, wf, bf, rf = (t.detach().float().requires_grad_() for t in (x, w, b, r))
    sr = rf + _rp(p) * keep * F.linear(xf, wf, bf)
    yr = F.layer_norm(sr, (512,), lw.detach(), lb.detach())
    ((yr * g1).sum() + (sr * g2).sum()).backward()
    print("rel: bias", _rel(b.grad, bf.grad), "weight", _rel(w.grad, wf.grad), "x", _rel(x.grad, xf.grad))
    assert _rel(b.grad, bf.grad) < 2e-2 and _rel(w.grad, wf.grad) < 2e-2 and _rel(x.grad, xf.grad) < 2e-2


def test_norm_dropout_keeps_no_mask_tensor(cuda):
    rows, H, p = 4096, 1024, 0.1
    x, r, w, b, g1, g2 = _norm_case(cuda, rows, H, False, torch.float32, p)

    def run(fn):
        for t in (x, r, w, b):
            t.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y, s = fn()
        held = torch.cuda.memory_allocated() - base     # what the forward keeps for the backward (and y, s)
        torch.autograd.backward([y, s], [g1, g2])
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, held

    fused, fused_held = run(lambda: ops.layer_norm(x, w, b, residual=r, dropout_p=p, rng=RNG))
    composed, composed_held = run(lambda: ops.layer_norm(F.dropout(x, p, True), w, b, residual=r))
    print(f"peak over forward + backward: fused {fused} B, nn.Dropout composition {composed} B; "
          f"held after the forward: fused {fused_held} B, composition {composed_held} B")
    assert fused < composed
    assert fused_held <= composed_held - rows * H   # the composition's bool mask, one byte per element


def test_norm_dropout_argument_checks_and_switch(cuda, monkeypatch):
    x, r, w, b, _, _ = _norm_case(cuda, 4, 64, False, torch.float32, 0.1)
    with pytest.raises(ValueError):
        ops.layer_norm(x, w, b, dropout_p=0.1)
    with pytest.raises(ValueError):
        ops.layer_norm(x, w, b, fork=True, dropout_p=0.1)
    with pytest.raises(ValueError):
        ops.layer_norm(x, w, b, residual=r, dropout_p=0.999)     # keeps nothing at 1/256
    assert ops.hidden_dropout_supported(x, 64, 0.1) and not ops.hidden_dropout_supported(x, 60, 0.1)
    y, _ = ops.layer_norm(x, w, b, residual=r, dropout_p=0.1)
    assert type(y.grad_fn).__name__ == "_NormDropFnBackward"
    y0, s0 = ops.layer_norm(x, w, b, residual=r)
    y1, s1 = ops.layer_norm(x, w, b, residual=r, dropout_p=0.0)
    assert torch.equal(y0, y1) and torch.equal(s0, s1) and type(y1.grad_fn).__name__ == "_NormFnBackward"
    gen = torch.cuda.default_generators[cuda.index]
    off = gen.get_offset()
    ops.layer_norm(x, w, b, residual=r, dropout_p=0.1)
    ops.dropout_add(x, r, 0.1)
    assert gen.get_offset() == off + 8                            # 4 per call
    monkeypatch.setattr(ops, "HIDDEN_DROPOUT", False)
    assert not ops.hidden_dropout_supported(x, 64, 0.1)
    y, _ = ops.layer_norm(x, w, b, residual=r, dropout_p=0.1)    # F.dropout + the existing norm
    assert type(y.grad_fn).__name__ == "_NormFnBackward"


# ---------------------------------------------------------------------------- K16
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,H", [(5, 64), (37, 768), (70001, 64), (11, 72)])   # 72: H % 16 == 8, no lane pairs
def test_dropout_add(cuda, rows, H, dt, with_res):
    p = 0.5 if rows == 37 else 0.1
    torch.manual_seed(3)
    x = torch.randn(rows, H, device=cuda).to(dt).requires_grad_(True)
    r = torch.randn(rows, H, device=cuda).to(dt).requires_grad_(True) if with_res else None
    g = torch.randn(rows, H, device=cuda).to(dt)
    keep = R.hidden_dropout_mask(rows, H, p, SEED, OFFSET).to(cuda)
    o = ops.dropout_add(x, r, p, rng=RNG)
    assert type(o.grad_fn).__name__ == "_DropoutAddFnBackward" and o.dtype == dt
    o.backward(g)
    # one fma in fp32 against mul + add; bf16: one rounding of the output (2^-9 relative)
    tol = 1e-2 if dt == torch.bfloat16 else 1e-5
    ref = _rp(p) * keep * x.detach().float() + (r.detach().float() if with_res else 0.0)
    drop = ~keep
    if with_res:
        assert torch.equal(o.detach()[drop], r.detach()[drop])
        assert torch.equal(r.grad, g)
    else:
        assert int((o.detach()[drop] != 0).sum()) == 0
    torch.testing.assert_close(o.detach().float(), ref, atol=tol, rtol=tol)
    assert int((x.grad[drop] != 0).sum()) == 0
    torch.testing.assert_close(x.grad.float(), _rp(p) * keep * g.float(), atol=tol, rtol=tol)
    assert torch.equal(ops.dropout_add(x.detach(), r.detach() if with_res else None, p, rng=RNG), o.detach())


# ------------------------------------------------------------------------- models
def _gpt2(cuda):
    from madnn.models import gpt2

    torch.manual_seed(0)
    # one head: head dim 64, so the attention (and its dropout) runs K8, not SDPA
    m = gpt2.GPT2(gpt2.gpt2_config("gpt2-tiny", n_layer=2, n_head=1, dropout=0.1))
    return m.to(cuda, torch.bfloat16), (lambda mod: list(mod.h)), (lambda mod: (mod.embed, mod.head))


def _bert(cuda):
    from madnn.models import bert

    torch.manual_seed(0)
    m = bert.BertForPreTraining(bert.bert_config("bert-tiny", layers=2, heads=1, dropout=0.1))
    return m.to(cuda, torch.bfloat16), (lambda mod: list(mod.layers)), (lambda mod: (mod.embed, mod.head))


def _graph_nodes(t):
    seen, todo, names = set(), [t.grad_fn], set()
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.add(type(f).__name__)
        todo.extend(n for n, _ in f.next_functions)
    return names


def _step(model, ids, seed, blocks=None, ends=None, ckpt=False):
    from torch.utils.checkpoint import checkpoint

    model.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    if ckpt:
        embed, head = ends(model)
        x = embed(ids)
        for blk in blocks(model):
            x = checkpoint(blk, x, use_reentrant=False)
        logits = head(x)
    else:
        logits = model(ids)
    loss = model.loss_fn(logits, ids)
    loss.backward()
    grads = [p.grad.clone() for p in model.parameters() if p.grad is not None]
    return loss.detach().clone(), grads, _graph_nodes(loss)


@pytest.mark.parametrize("make", [_gpt2, _bert])
def test_models_keep_the_fused_paths_with_hidden_dropout(cuda, monkeypatch, make):
    model, blocks, ends = make(cuda)
    ids = torch.randint(0, 512, (2, 64), device=cuda)
    model.train()
    _step(model, ids, 4)   # warm-up: per-shape GEMM choices that are timed on first use are settled
    l1, g1, nodes = _step(model, ids, 5)
    l2, g2, _ = _step(model, ids, 5)
    assert torch.equal(l1, l2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    l3, _, _ = _step(model, ids, 6)
    assert not torch.equal(l1, l3)
    assert "_GeluMLPFnBackward" in nodes and "_NormDropFnBackward" in nodes and "_DropoutAddFnBackward" in nodes
    assert "NativeDropoutBackward0" not in nodes
    # the recomputed blocks regenerate the same masks
    lc, gc, _ = _step(model, ids, 5, blocks, ends, ckpt=True)
    assert torch.equal(l1, lc)
    for a, b in zip(g1, gc):
        assert torch.equal(a, b)
    model.eval()
    with torch.no_grad():
        on = model(ids)
    monkeypatch.setattr(ops, "HIDDEN_DROPOUT", False)
    with torch.no_grad():
        assert torch.equal(model(ids), on)
    model.train()
    _, _, nodes = _step(model, ids, 5)
    assert "NativeDropoutBackward0" in nodes and "_NormDropFnBackward" not in nodes
