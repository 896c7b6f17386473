"""K8 attention over right-padded batches (``seqlens``): the VARLEN instantiations of the three
register-staged kernels against fp32 SDPA run per sequence on the slice ``[b, :L_b]`` (``dout`` sliced
the same way; the host dropout mask for p > 0, as test_attention_edges_gpu._reference).

Before every call the padded positions of q, k, v and dout are filled with NaN: nothing there may
reach a result.  Padded rows of o, dq, dk, dv must be exact zeros and the LSE finite everywhere.
Bounds are test_attention_edges_gpu._bounds (1e-2 on o, 2e-2 on the gradients, global relative error
over the valid region): the same arithmetic over fewer keys.  The lengths straddle the 128-row blocks,
the 64-row tiles and the 32-row waves."""
import functools

import pytest
import torch
import torch.nn.functional as F

from madnn import ops
from madnn.ops import reference
from test_attention_dropout_gpu import _ref as _drop_ref
from test_attention_edges_gpu import NAMES, RNG, _bounds, _ref, _rel

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _lens(device, lens):
    return torch.tensor(lens, dtype=torch.int32, device=device)


def _valid(lens, S, device):
    """bool [B, S, 1, 1] of the clamped lengths."""
    ln = torch.tensor(lens, device=device).clamp(0, S)
    return (torch.arange(S, device=device)[None, :] < ln[:, None])[:, :, None, None]


@functools.lru_cache(maxsize=None)
def _inputs(device, B, S, H, HKV, D, lens, seed=0):
    """bf16 q, k, v, dout with NaN at every padded position; never modified."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    valid = _valid(lens, S, device)
    out = []
    for heads in (H, HKV, HKV, H):
        t = torch.randn(B, S, heads, D, generator=g).to(device).bfloat16()
        out.append(torch.where(valid, t, torch.full_like(t, NAN)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _reference(device, B, S, H, HKV, D, lens, causal, p, seed=0):
    """(o, dq, dk, dv) fp32 [B, S, heads, D]: every sequence alone at its true length, zeros at the
    padded positions.  Computed once per case and shared."""
    q, k, v, do = _inputs(device, B, S, H, HKV, D, lens, seed)
    scale = D ** -0.5
    outs = [torch.zeros(t.shape, dtype=torch.float32, device=device) for t in (q, q, k, v)]
    keep = rp = None
    if p > 0.0:
        keep = reference.attention_dropout_mask(B, H, S, p, *RNG).to(device)
        rp = 256.0 / reference.attention_dropout_threshold(p)
    for b, ln in enumerate(lens):
        ln = max(0, min(ln, S))
        if ln == 0:
            continue
        qr, kr, vr = (t[b:b + 1, :ln].float().requires_grad_(True) for t in (q, k, v))
        if p > 0.0:
            orf = _drop_ref(qr, kr, vr, causal, scale, keep[b:b + 1, :, :ln, :ln], rp)
        else:
            orf = _ref(qr, kr, vr, causal, scale)
        grads = torch.autograd.grad(orf, (qr, kr, vr), do[b:b + 1, :ln].float())
        for dst, src in zip(outs, (orf.detach(), *grads)):
            dst[b:b + 1, :ln] = src
    return tuple(outs)


def _run(device, B, S, H, HKV, D, lens, causal, p, seqlens=None, seed=0):
    """(o, dq, dk, dv, lse) of the kernels; ``seqlens`` overrides the tensor handed to them."""
    q, k, v, do = _inputs(device, B, S, H, HKV, D, lens, seed)
    sl = _lens(device, lens) if seqlens is None else seqlens
    o, lse = torch.ops.madnn.attn_fwd(q, k, v, causal, D ** -0.5, p, *(RNG if p > 0.0 else (0, 0)), sl)
    dq, dk, dv = (torch.full_like(t, NAN) for t in (q, k, v))
    torch.ops.madnn.attn_bwd(do, q, k, v, o, lse, dq, dk, dv, causal, D ** -0.5, None, p,
                             *(RNG if p > 0.0 else (0, 0)), sl)
    return o, dq, dk, dv, lse


def _check(device, B, S, H, HKV, D, lens, causal, p):
    o, dq, dk, dv, lse = _run(device, B, S, H, HKV, D, lens, causal, p)
    ref = _reference(device, B, S, H, HKV, D, lens, causal, p)
    valid = _valid(lens, S, device)
    assert torch.isfinite(lse).all(), "lse"
    errs = {}
    for n, got, want in zip(NAMES, (o, dq, dk, dv), ref):
        pad = ~valid.expand_as(got)
        assert bool((got[pad] == 0).all()), (n, "padded rows are not exact zeros")
        assert torch.isfinite(got.float()).all(), n
        errs[n] = _rel(got, want)      # the padded region is zero on both sides: the valid region's error
    print((B, S, H, HKV, D, lens, causal, p), errs)
    bo, bg = _bounds(None)
    assert errs["o"] < bo, errs
    for n in NAMES[1:]:
        assert errs[n] < bg, (n, errs)
    return o, dq, dk, dv, lse


# ------------------------------------------------------------------ 1. the contract at ragged shapes
@pytest.mark.parametrize("lens", [(200, 77, 1), (129, 128, 64), (0, 65, 200)])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("D", [64, 128])
def test_varlen_matches_per_sequence_reference(cuda, D, causal, p, lens):
    _check(cuda, 3, 200, 4, 2, D, lens, causal, p)


# ------------------------------------------------------------------ 2. routing away from the ring kernels
@pytest.mark.parametrize("lens", [(256, 63), (192, 128)])
@pytest.mark.parametrize("causal", [True, False])
def test_varlen_at_a_shape_the_dense_path_sends_to_the_ring_kernels(cuda, causal, lens):
    """S % 64 == 0 at D = 64: without seqlens both LDS-DMA rings run; with seqlens the VARLEN
    register-staged kernels must (the rings know no lengths: padded rows would not be zero)."""
    _check(cuda, 2, 256, 4, 2, 64, lens, causal, 0.0)


# ------------------------------------------------------------------ 3. dense equivalence, clamping
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("D", [64, 128])
def test_full_lengths_bitwise_equal_to_no_seqlens(cuda, D, causal, p):
    """S = 200: both calls run the register-staged kernels, and L = S takes every branch as a.S does."""
    B, S, H, HKV = 1, 200, 4, 2
    q, k, v, do = _inputs(cuda, B, S, H, HKV, D, (S,), 1)
    rng = RNG if p > 0.0 else (0, 0)
    got = _run(cuda, B, S, H, HKV, D, (S,), causal, p, seed=1)
    o, lse = torch.ops.madnn.attn_fwd(q, k, v, causal, D ** -0.5, p, *rng)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    torch.ops.madnn.attn_bwd(do, q, k, v, o, lse, dq, dk, dv, causal, D ** -0.5, None, p, *rng)
    for n, a, b in zip(NAMES + ("lse",), got, (o, dq, dk, dv, lse)):
        assert torch.equal(a, b), (n, _rel(a, b))


@pytest.mark.parametrize("D", [64, 128])
def test_lengths_are_clamped_into_0_S(cuda, D):
    B, S, H, HKV = 2, 200, 4, 2
    a = _run(cuda, B, S, H, HKV, D, (S, 0), True, 0.0, seqlens=_lens(cuda, (S + 5, -3)), seed=2)
    b = _run(cuda, B, S, H, HKV, D, (S, 0), True, 0.0, seed=2)
    for n, x, y in zip(NAMES + ("lse",), a, b):
        assert torch.equal(x, y), n


def test_seqlens_argument_is_checked(cuda):
    q, k, v, _ = _inputs(cuda, 2, 200, 4, 2, 64, (200, 0), 2)
    for bad in (torch.zeros(2, dtype=torch.int64, device=cuda), torch.zeros(3, dtype=torch.int32, device=cuda),
                torch.zeros(2, dtype=torch.int32), torch.zeros(4, dtype=torch.int32, device=cuda)[::2]):
        with pytest.raises(RuntimeError):
            torch.ops.madnn.attn_fwd(q, k, v, True, 0.125, 0.0, 0, 0, bad)


# ------------------------------------------------------------------ 4. packed path, bias gradient
@pytest.mark.parametrize("B,S,H,HKV,D,lens", [(2, 200, 4, 2, 64, (200, 70)), (2, 130, 2, 2, 128, (0, 130))])
def test_packed_colsum_covers_valid_rows_only(cuda, monkeypatch, B, S, H, HKV, D, lens):
    """ops.linear with a bias into attention_qkvpacked(seqlens=...), as test_explicit_scale_packed_colsum:
    the backward kernels' column sums are the projection's bias gradient and cover valid rows only.  The
    second case has an all-padded sequence: the zero cpart rows of the workgroups that return early."""
    calls = []
    real = ops.bias_grad
    monkeypatch.setattr(ops, "bias_grad", lambda *a, **k: calls.append(1) or real(*a, **k))
    torch.manual_seed(9)
    E = 256
    x = torch.randn(B, S, E, device=cuda, dtype=torch.bfloat16, requires_grad=True)
    w = (torch.randn((H + 2 * HKV) * D, E, device=cuda) * E ** -0.5).bfloat16().requires_grad_()
    bias = (torch.randn((H + 2 * HKV) * D, device=cuda) * 0.1).bfloat16().requires_grad_()
    valid = _valid(lens, S, cuda)
    g = torch.where(valid, torch.randn(B, S, H, D, device=cuda), torch.full((), NAN, device=cuda))
    qkv = ops.linear(x, w, bias).view(B, S, H + 2 * HKV, D)
    o = ops.attention_qkvpacked(qkv, H, HKV, causal=True, seqlens=_lens(cuda, lens))
    o.backward(g.to(o.dtype))
    assert not calls, "the QKV projection ran its own bias column-sum pass"
    assert bool((o[~valid.expand_as(o)] == 0).all())
    xf, wf, bf = (t.detach().float().requires_grad_() for t in (x, w, bias))
    total = 0.0
    for b, ln in enumerate(lens):
        if ln == 0:
            continue
        qf = F.linear(xf[b:b + 1, :ln], wf, bf).view(1, ln, H + 2 * HKV, D)
        qq, kk, vv = qf.split([H, HKV, HKV], dim=2)
        orf = _ref(qq, kk, vv, True, D ** -0.5)
        total = total + (orf * g[b:b + 1, :ln].bfloat16().float()).sum()
        assert _rel(o[b:b + 1, :ln], orf) < _bounds(None)[0]
    total.backward()
    errs = {"db": _rel(bias.grad, bf.grad), "dw": _rel(w.grad, wf.grad), "dx": _rel(x.grad, xf.grad)}
    print((B, S, H, HKV, D, lens), errs)
    bg = _bounds(None)[1]
    assert torch.isfinite(x.grad.float()).all() and torch.isfinite(w.grad.float()).all()
    assert errs["db"] < bg and errs["dw"] < bg and errs["dx"] < bg, errs


# ------------------------------------------------------------------ 5. zoo BERT on the device
def test_zoo_bert_padded_batch_matches_per_sequence_fp32(cuda):
    """bert-tiny at head dim 64 (K8), bf16, training mode with dropout 0; the loss is summed over the
    valid positions only.  Parameter gradients against the fp32 eager copy run per sequence at its true
    length, within the bound the suite already applies to BERT's parameter gradients in bf16
    (test_gemmp_gpu.test_bert_layer_residual_tee_matches_eager: 5e-2 per parameter)."""
    import copy

    from madnn.models.bert import BertForPreTraining, bert_config

    torch.manual_seed(3)
    cfg = bert_config("bert-tiny", hidden=256, heads=4, intermediate=512, layers=2, max_position=256)
    ref = BertForPreTraining(cfg).to(cuda).train()
    model = copy.deepcopy(ref).bfloat16().train()
    B, S, lens = 3, 200, (200, 77, 130)
    ids = torch.randint(0, cfg.vocab_size, (B, S), device=cuda)
    tgt = torch.randint(0, cfg.vocab_size, (B, S), device=cuda)
    valid = _valid(lens, S, cuda)[:, :, 0, 0]
    calls = []
    real = ops._AttnPackedFn.apply
    ops._AttnPackedFn.apply = lambda *a: calls.append(a[-1] is not None) or real(*a)
    try:
        logits = model(ids, _lens(cuda, lens))
    finally:
        ops._AttnPackedFn.apply = real
    assert calls == [True] * cfg.layers, "the layers did not run K8 with seqlens"
    n = int(valid.sum())
    loss = F.cross_entropy(logits.float()[valid][:, :cfg.vocab_size], tgt[valid], reduction="sum") / n
    loss.backward()
    rloss = 0.0
    for b, ln in enumerate(lens):
        rl = ref(ids[b:b + 1, :ln])
        rloss = rloss + F.cross_entropy(rl[0, :, :cfg.vocab_size], tgt[b, :ln], reduction="sum") / n
    rloss.backward()
    torch.testing.assert_close(loss.detach(), rloss.detach(), atol=2e-2, rtol=2e-2)
    rp = dict(ref.named_parameters())
    worst = max((_rel(p.grad, rp[name].grad), name) for name, p in model.named_parameters())
    print("worst parameter gradient", worst)
    for name, p in model.named_parameters():
        assert torch.isfinite(p.grad.float()).all(), name
        assert _rel(p.grad, rp[name].grad) < 5e-2, (name, _rel(p.grad, rp[name].grad))
