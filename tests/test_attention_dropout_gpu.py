"""K8 attention dropout: the in-kernel Philox mask (regenerated in the backward kernels) against the
host mirror of the mask and an fp32 reference built from it; determinism, the generator default,
checkpoint recompute, and the routing of the modules that now reach K8 with dropout > 0."""
import pytest
import torch
import torch.nn.functional as F

from madnn import ops
from madnn.ops import reference

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = a.detach().float(), b.detach().float()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def _ref(q, k, v, causal, scale, keep, rp):
    """((softmax(scale QK^T [+causal]) * M) * rp) V on [B, S, heads, D] fp32 (GQA: KV heads repeated)."""
    h, hkv = q.size(2), k.size(2)
    qt, kt, vt = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
    if h != hkv:
        kt, vt = kt.repeat_interleave(h // hkv, dim=1), vt.repeat_interleave(h // hkv, dim=1)
    s = (qt @ kt.transpose(-1, -2)) * scale
    if causal:
        n = s.size(-1)
        s = s.masked_fill(~torch.ones(n, n, dtype=torch.bool, device=s.device).tril(), float("-inf"))
    p = torch.softmax(s, dim=-1)
    return (((p * keep) * rp) @ vt).transpose(1, 2)


def _mask(B, H, S, p, rng, device):
    keep = reference.attention_dropout_mask(B, H, S, p, *rng).to(device)
    return keep, 256.0 / reference.attention_dropout_threshold(p)


def _qkv(B, S, H, HKV, D, device, seed=0):
    torch.manual_seed(seed)
    q = torch.randn(B, S, H, D, device=device).bfloat16().requires_grad_(True)
    k = torch.randn(B, S, HKV, D, device=device).bfloat16().requires_grad_(True)
    v = torch.randn(B, S, HKV, D, device=device).bfloat16().requires_grad_(True)
    return q, k, v


@pytest.mark.parametrize("B,H,S", [(2, 3, 77), (1, 2, 200)])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_device_mask_equals_host_mirror(cuda, B, H, S, p):
    seed, offset = 0x9E3779B97F4A7C15, (3 << 32) | 20   # both 64-bit (seed above 2^63)
    s64 = lambda x: x - 2 ** 64 if x >= 2 ** 63 else x
    with torch.cuda.device(cuda):
        dev = torch.ops.madnn.attn_dropout_mask(B, H, S, p, s64(seed), s64(offset))
    assert dev.dtype == torch.uint8 and dev.shape == (B, H, S, S) and dev.device.type == "cuda"
    host = reference.attention_dropout_mask(B, H, S, p, seed, offset)
    assert torch.equal(dev.cpu().bool(), host)


CASES = [
    (1, 77, 3, 3, 64, False, 0.1),
    (1, 200, 4, 2, 64, True, 0.1),     # GQA: dK/dV must take the mask of the query head, not the KV head
    (1, 200, 4, 2, 64, True, 0.5),
    (2, 256, 4, 4, 64, True, 0.1),     # S % 64 == 0: the D = 64 LDS-DMA ring kernels must be bypassed
    (1, 130, 2, 2, 128, False, 0.1),
    (1, 200, 4, 2, 128, True, 0.1),
]


@pytest.mark.parametrize("B,S,H,HKV,D,causal,p", CASES)
def test_attention_dropout_fwd_bwd(cuda, B, S, H, HKV, D, causal, p):
    q, k, v = _qkv(B, S, H, HKV, D, cuda)
    rng = (1234, 8)
    o = ops.attention(q, k, v, causal=causal, dropout_p=p, rng=rng)
    assert o.shape == (B, S, H, D) and o.is_contiguous()
    do = torch.randn_like(o)
    o.backward(do)
    keep, rp = _mask(B, H, S, p, rng, cuda)
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    orf = _ref(qr, kr, vr, causal, D ** -0.5, keep, rp)
    orf.backward(do.float())
    errs = {"o": _rel(o, orf), "dq": _rel(q.grad, qr.grad), "dk": _rel(k.grad, kr.grad), "dv": _rel(v.grad, vr.grad)}
    print((B, S, H, HKV, D, causal, p), errs)
    assert errs["o"] < 1e-2, errs
    for name in ("dq", "dk", "dv"):
        assert errs[name] < 2e-2, (name, errs)
    if causal:   # row 0 sees one key: its output is rp * v[0] or exactly zero, by the mask alone
        for h in range(H):
            want = v[0, 0, h // (H // HKV)].float() * rp if bool(keep[0, h, 0, 0]) else torch.zeros(D, device=cuda)
            torch.testing.assert_close(o[0, 0, h].float(), want, atol=2e-2 * rp, rtol=1e-2)


def test_attention_dropout_is_deterministic_in_rng(cuda):
    q, k, v = _qkv(2, 200, 4, 2, 64, cuda, seed=1)
    do = torch.randn(2, 200, 4, 64, device=cuda).bfloat16()

    def run(rng):
        o = ops.attention(q, k, v, causal=True, dropout_p=0.1, rng=rng)
        return (o, *torch.autograd.grad(o, (q, k, v), do))

    a, b, c = run((5, 0)), run((5, 0)), run((5, 4))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], c[0])


@pytest.mark.parametrize("S,D", [(200, 64), (256, 64), (130, 128)])
def test_dropout_p_zero_is_todays_path(cuda, S, D):
    q, k, v = _qkv(1, S, 4, 2, D, cuda, seed=2)
    do = torch.randn(1, S, 4, D, device=cuda).bfloat16()
    o0 = ops.attention(q, k, v, causal=True)
    g0 = torch.autograd.grad(o0, (q, k, v), do)
    o1 = ops.attention(q, k, v, causal=True, dropout_p=0.0, rng=(1, 2))
    g1 = torch.autograd.grad(o1, (q, k, v), do)
    assert torch.equal(o0, o1)
    for x, y in zip(g0, g1):
        assert torch.equal(x, y)


def test_attention_dropout_rejects_keep_nothing(cuda):
    q, k, v = _qkv(1, 64, 1, 1, 64, cuda)
    with pytest.raises(ValueError):
        ops.attention(q, k, v, dropout_p=0.999)
    with pytest.raises(RuntimeError):
        torch.ops.madnn.attn_fwd(q, k, v, True, 0.125, 0.999, 0, 0)


def test_packed_dropout_inplace_grad_and_colsum(cuda, monkeypatch):
    """attention_qkvpacked(dropout_p = 0.1) on a biased ops.linear output: the in-place dQKV matches the
    reference, and the column sums the backward kernels attach (the projection's bias gradient, no
    column-sum pass of its own) are the sums of the dQKV that was written."""
    calls = []
    real = ops.bias_grad
    monkeypatch.setattr(ops, "bias_grad", lambda *a, **k: calls.append(1) or real(*a, **k))
    torch.manual_seed(9)
    B, S, E, H, HKV, D, p, rng = 2, 192, 256, 4, 2, 64, 0.1, (77, 12)
    x = torch.randn(B, S, E, device=cuda, dtype=torch.bfloat16, requires_grad=True)
    w = (torch.randn((H + 2 * HKV) * D, E, device=cuda) * E ** -0.5).bfloat16().requires_grad_()
    b = (torch.randn((H + 2 * HKV) * D, device=cuda) * 0.1).bfloat16().requires_grad_()
    g = torch.randn(B, S, H, D, device=cuda)
    qkv = ops.linear(x, w, b).view(B, S, H + 2 * HKV, D)
    got = []
    qkv.register_hook(lambda t: got.append(t.detach().clone()))
    o = ops.attention_qkvpacked(qkv, H, HKV, causal=True, dropout_p=p, rng=rng)
    (o.float() * g).sum().backward()
    assert not calls, "the QKV projection ran its own bias column-sum pass"
    dqkv = got[0]
    keep, rp = _mask(B, H, S, p, rng, cuda)
    ref = qkv.detach().float().requires_grad_(True)
    qr, kr, vr = ref.split([H, HKV, HKV], dim=2)
    orf = _ref(qr, kr, vr, True, D ** -0.5, keep, rp)
    (orf * g).sum().backward()
    assert _rel(o, orf) < 1e-2
    assert _rel(dqkv, ref.grad) < 2e-2
    colsum = dqkv.float().sum((0, 1)).reshape(-1)
    print("colsum rel", _rel(b.grad, colsum))
    assert _rel(b.grad, colsum) < 2e-2


def test_default_rng_is_torchs_device_generator(cuda):
    q, k, v = _qkv(1, 200, 2, 2, 64, cuda, seed=3)
    torch.manual_seed(42)
    a = ops.attention(q, k, v, dropout_p=0.1)
    b = ops.attention(q, k, v, dropout_p=0.1)
    torch.manual_seed(42)
    c = ops.attention(q, k, v, dropout_p=0.1)
    assert not torch.equal(a, b)
    assert torch.equal(a, c)
    torch.manual_seed(42)
    gen = torch.cuda.default_generators[cuda.index]
    d = ops.attention(q, k, v, dropout_p=0.1, rng=(gen.initial_seed(), gen.get_offset()))
    assert torch.equal(a, d)


def _self_attention(cuda, dropout):
    from madnn.models.common import SelfAttention

    torch.manual_seed(3)
    return SelfAttention(256, 4, dropout=dropout).to(cuda).bfloat16()


def test_checkpoint_recompute_regenerates_the_same_mask(cuda):
    from torch.utils.checkpoint import checkpoint

    m = _self_attention(cuda, 0.1).train()
    x = torch.randn(2, 96, 256, device=cuda).bfloat16().requires_grad_(True)
    grads = []
    for ckpt in (False, True):
        torch.manual_seed(7)
        y = checkpoint(m, x, use_reentrant=False) if ckpt else m(x)
        grads.append(torch.autograd.grad(y.float().square().mean(), x)[0])
    assert grads[0].abs().sum() > 0
    assert torch.equal(grads[0], grads[1])


def test_selfattention_routes_dropout_to_k8(cuda, monkeypatch):
    m = _self_attention(cuda, 0.1)
    x = torch.randn(2, 96, 256, device=cuda).bfloat16()
    sdpa_calls = []
    real = F.scaled_dot_product_attention

    def boom(*a, **k):
        raise AssertionError("SelfAttention took the SDPA branch")

    monkeypatch.setattr(F, "scaled_dot_product_attention", boom)
    m.train()
    y1, y2 = m(x), m(x)
    assert not torch.equal(y1, y2)                      # dropout is on, and the offset advances
    m0 = _self_attention(cuda, 0.0)
    m0.load_state_dict(m.state_dict())
    assert torch.equal(m.eval()(x), m0.eval()(x))       # eval: no dropout
    # the switch sends dropout back to SDPA
    monkeypatch.setattr(F, "scaled_dot_product_attention", lambda *a, **k: sdpa_calls.append(k) or real(*a, **k))
    monkeypatch.setattr(ops, "ATTN_DROPOUT", False)
    m.train()(x)
    assert len(sdpa_calls) == 1 and sdpa_calls[0]["dropout_p"] == 0.1


def test_hf_entry_counts_dropout_on_k8(cuda):
    from madnn.nn.swap import attention_stats, madnn_attention_forward

    class Mod:
        is_causal = True

    torch.manual_seed(0)
    q, k, v = (torch.randn(2, 4, 128, 64, device=cuda).bfloat16() for _ in range(3))   # HF layout [B, H, S, D]
    before = attention_stats()
    o, _ = madnn_attention_forward(Mod(), q, k, v, None, dropout=0.1, scaling=0.125)
    after = attention_stats()
    assert o.shape == (2, 128, 4, 64)
    assert after["k8"] == before["k8"] + 1 and after["sdpa"] == before["sdpa"]
    o0, _ = madnn_attention_forward(Mod(), q, k, v, None, dropout=0.0, scaling=0.125)
    assert not torch.equal(o, o0)


def test_hf_gpt2_with_attn_pdrop_trains_on_k8(cuda):
    pytest.importorskip("transformers")
    from madnn.models import hf
    from madnn.nn.swap import attention_stats, use_madnn_kernels

    torch.manual_seed(0)
    model = hf.gpt2_hf("gpt2-tiny", n_embd=256, n_head=4, attn_pdrop=0.1, resid_pdrop=0.0, embd_pdrop=0.0)
    model = model.to(cuda).bfloat16()
    use_madnn_kernels(model)
    model.train()
    ids = torch.randint(0, 512, (4, 64), generator=torch.Generator().manual_seed(1)).to(cuda)
    before = attention_stats()
    loss = hf.hf_loss_fn(model)(model(ids).logits, ids)
    loss.backward()
    after = attention_stats()
    assert torch.isfinite(loss)
    assert after["sdpa"] == before["sdpa"] and after["k8"] > before["k8"]
