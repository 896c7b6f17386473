"""Per-sequence lengths (``seqlens``) of a right-padded batch on the CPU tier: the eager reference and
``ops.attention`` (which runs it on CPU tensors), padding invariance of the zoo BERT, and the Hugging
Face mask function that turns a right-padded ``attention_mask`` into lengths."""
import importlib.util

import pytest
import torch
import torch.nn.functional as F

from madnn import ops
from madnn.ops import reference

B, S, H, HKV, D = 3, 10, 4, 2, 8
LENS = (10, 4, 0)
NAN = float("nan")


def _valid(lens=LENS, s=S):
    return (torch.arange(s)[None, :] < torch.tensor(lens)[:, None])[:, :, None, None]


def _inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B, S, h, D, generator=g) for h in (H, HKV, HKV, H))


def _sdpa(q, k, v, causal):
    o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), is_causal=causal,
                                       enable_gqa=True)
    return o.transpose(1, 2)


def _per_sequence(q, k, v, do, causal):
    """(o, dq, dk, dv): every sequence alone at its true length, zeros at the padded positions."""
    outs = [torch.zeros_like(t) for t in (q, q, k, v)]
    for b, ln in enumerate(LENS):
        if ln == 0:
            continue
        qr, kr, vr = (t[b:b + 1, :ln].clone().requires_grad_(True) for t in (q, k, v))
        o = _sdpa(qr, kr, vr, causal)
        for dst, src in zip(outs, (o.detach(), *torch.autograd.grad(o, (qr, kr, vr), do[b:b + 1, :ln]))):
            dst[b:b + 1, :ln] = src
    return outs


@pytest.mark.parametrize("fn", [reference.attention, ops.attention], ids=["reference", "ops"])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("poison", [False, True], ids=["clean", "nan_in_pads"])
def test_seqlens_equals_each_sequence_alone(fn, causal, poison):
    q, k, v, do = _inputs()
    want = _per_sequence(q, k, v, do, causal)
    valid = _valid()
    if poison:   # NaN at every padded position of q, k, v and of the incoming gradient changes nothing
        q, k, v, do = (torch.where(valid, t, torch.full_like(t, NAN)) for t in (q, k, v, do))
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    o = fn(q, k, v, causal=causal, seqlens=torch.tensor(LENS, dtype=torch.int32))
    got = (o.detach(), *torch.autograd.grad(o, (q, k, v), do))
    for name, a, w in zip(("o", "dq", "dk", "dv"), got, want):
        pad = ~valid.expand_as(a)
        assert bool((a[pad] == 0).all()), (name, "padded positions are not exact zeros")
        torch.testing.assert_close(a, w, atol=1e-6, rtol=1e-6, msg=lambda m: f"{name}: {m}")


@pytest.mark.parametrize("scale", [-0.125, 0.3])
def test_seqlens_on_both_branches_of_the_reference(scale):
    """The plain-ops branch (a scale that is not positive) and the SDPA branch agree with the dense
    call on each sequence's valid slice, and clamp the lengths into [0, S]."""
    q, k, v, _ = _inputs(1)
    o = reference.attention(q, k, v, causal=True, scale=scale, seqlens=torch.tensor((S + 5, 4, -3)))
    for b, ln in enumerate(LENS):
        dense = reference.attention(q[b:b + 1, :ln], k[b:b + 1, :ln], v[b:b + 1, :ln], causal=True, scale=scale)
        torch.testing.assert_close(o[b:b + 1, :ln], dense, atol=1e-6, rtol=1e-6)
        assert bool((o[b, ln:] == 0).all())


def test_seqlens_none_is_the_dense_call():
    q, k, v, _ = _inputs(2)
    assert torch.equal(ops.attention(q, k, v, causal=True, seqlens=None), ops.attention(q, k, v, causal=True))
    qkv = torch.cat([q, k, v], dim=2)
    a = ops.attention_qkvpacked(qkv, H, HKV, causal=False, seqlens=torch.tensor(LENS, dtype=torch.int32))
    b = ops.attention(q, k, v, causal=False, seqlens=torch.tensor(LENS, dtype=torch.int32))
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        ops.attention(q, k, v, seqlens=torch.tensor((1, 2)))


@pytest.mark.parametrize("dropout_path", [False, True], ids=["layer", "layer_with_hidden_dropout_config"])
def test_zoo_bert_is_invariant_to_right_padding(dropout_path):
    """fp32, eval mode: the logits of a padded batch at the valid positions are those of every
    sequence run alone at its true length (both with a dropout-free config and with one whose layers
    hold dropout modules, inactive in eval mode)."""
    from madnn.models.bert import BertForPreTraining, bert_config

    torch.manual_seed(0)
    cfg = bert_config("bert-tiny", layers=2, dropout=0.1 if dropout_path else 0.0)
    model = BertForPreTraining(cfg).eval()
    lens = (16, 5, 11)
    ids = torch.randint(0, cfg.vocab_size, (3, 16))
    padded = ids.clone()
    for b, ln in enumerate(lens):
        padded[b, ln:] = 0
    with torch.no_grad():
        out = model(padded, torch.tensor(lens, dtype=torch.int32))
        for b, ln in enumerate(lens):
            alone = model(ids[b:b + 1, :ln])[0]
            torch.testing.assert_close(out[b, :ln], alone, atol=1e-5, rtol=1e-5)
        # without the lengths the pads are attended to: the check above is not vacuous
        assert not torch.allclose(model(padded)[1, :5], model(ids[1:2, :5])[0], atol=1e-5, rtol=1e-5)


def test_self_attention_training_gradients_ignore_pads():
    """SelfAttention's eager branch (CPU) in training mode: gradients of the parameters equal those of
    the sequences run alone when the loss ignores the padded rows."""
    from madnn.models.common import SelfAttention

    torch.manual_seed(1)
    attn = SelfAttention(32, 4, kv_heads=2, causal=True)
    x = torch.randn(3, 10, 32)
    lens = (10, 4, 0)
    valid = _valid(lens, 10)[:, :, 0]
    y = attn(x, torch.tensor(lens, dtype=torch.int32))
    (y * valid).sum().backward()
    got = {n: p.grad.clone() for n, p in attn.named_parameters()}
    attn.zero_grad()
    sum(attn(x[b:b + 1, :ln]).sum() for b, ln in enumerate(lens) if ln).backward()
    for n, p in attn.named_parameters():
        torch.testing.assert_close(got[n], p.grad, atol=1e-5, rtol=1e-5, msg=lambda m: f"{n}: {m}")


# ------------------------------------------------------------------ Hugging Face mask function
needs_hf = pytest.mark.skipif(importlib.util.find_spec("transformers") is None, reason="transformers not installed")


def _mask_fn(am, causal=False):
    from transformers.masking_utils import bidirectional_mask_function, causal_mask_function

    from madnn.nn import swap

    n = am.size(1) if am is not None else 6
    mask = swap.madnn_mask(2, n, n, 0, 0, mask_function=causal_mask_function if causal else bidirectional_mask_function,
                           attention_mask=am, allow_is_causal_skip=False, allow_is_bidirectional_skip=False)
    return mask, (ops._attached(mask, swap._SEQLENS) if isinstance(mask, torch.Tensor) else None)


@needs_hf
@pytest.mark.parametrize("causal", [False, True])
def test_hf_mask_function_attaches_lengths_to_a_right_padded_mask(causal):
    from transformers.masking_utils import bidirectional_mask_function, causal_mask_function, sdpa_mask

    am = torch.tensor([[1, 1, 1, 1, 0, 0], [1, 1, 1, 1, 1, 1]], dtype=torch.bool)
    mask, rec = _mask_fn(am, causal)
    assert rec is not None
    lens, is_causal = rec
    assert lens.dtype == torch.int32 and lens.tolist() == [4, 6] and is_causal is causal
    plain = sdpa_mask(2, 6, 6, 0, 0, mask_function=causal_mask_function if causal else bidirectional_mask_function,
                      attention_mask=am, allow_is_causal_skip=False, allow_is_bidirectional_skip=False)
    assert torch.equal(mask, plain)      # the mask itself is HF's, unchanged


@needs_hf
@pytest.mark.parametrize("am", [torch.tensor([[0, 0, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1]], dtype=torch.bool),
                                torch.tensor([[1, 1, 0, 1, 0, 0], [1, 1, 1, 1, 1, 1]], dtype=torch.bool), None],
                         ids=["left_padded", "hole", "no_mask"])
def test_hf_mask_function_attaches_nothing_else(am):
    _, rec = _mask_fn(am)
    assert rec is None


@needs_hf
def test_hf_mask_function_needs_whole_sequence_self_attention():
    """q_length != kv_length (decoding with a cache) and a non-zero offset attach nothing."""
    from transformers.masking_utils import causal_mask_function

    from madnn.nn import swap

    am = torch.tensor([[1, 1, 1, 1, 0, 0], [1, 1, 1, 1, 1, 1]], dtype=torch.bool)
    for q_len, q_off in ((1, 5), (6, 1)):
        mask = swap.madnn_mask(2, q_len, 6, q_off, 0, mask_function=causal_mask_function, attention_mask=am,
                               allow_is_causal_skip=False)
        assert isinstance(mask, torch.Tensor) and ops._attached(mask, swap._SEQLENS) is None


@needs_hf
def test_hf_attention_forward_with_a_plain_mask_is_sdpa():
    """A mask that carries no lengths (here: left-padded) still returns what HF's SDPA path returns."""
    from transformers.integrations.sdpa_attention import sdpa_attention_forward

    from madnn.nn import swap

    torch.manual_seed(0)
    am = torch.tensor([[0, 0, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1]], dtype=torch.bool)
    mask, rec = _mask_fn(am)
    assert rec is None
    q, k, v = (torch.randn(2, 4, 6, 8) for _ in range(3))

    class _M(torch.nn.Module):
        is_causal = False
        num_key_value_groups = 1

    before = swap.attention_stats()
    a, _ = swap.madnn_attention_forward(_M(), q, k, v, mask, scaling=8 ** -0.5, is_causal=False)
    b, _ = sdpa_attention_forward(_M(), q, k, v, mask, scaling=8 ** -0.5, is_causal=False)
    after = swap.attention_stats()
    assert torch.equal(a, b)
    assert after["sdpa"] == before["sdpa"] + 1 and after["k8"] == before["k8"]


@needs_hf
def test_hf_bert_right_padded_cpu_attaches_lengths_and_matches_stock(monkeypatch):
    """The CPU tier of the routing through a whole model: the mask HF builds for a right-padded batch
    reaches every layer's attention call carrying the row sums, and, fp32 tensors not being K8's, each
    call still runs SDPA, so the swapped model equals the stock one (the K8 route itself is
    tests/test_hf_varlen_gpu.py)."""
    import copy

    from madnn.models import hf
    from madnn.nn import swap, use_madnn_kernels

    torch.manual_seed(0)
    m = hf.bert_hf().eval()
    ref = copy.deepcopy(m)
    use_madnn_kernels(m)
    seen = []
    real = ops._attached
    monkeypatch.setattr(ops, "_attached", lambda t, name, *a, **k: seen.append(real(t, name, *a, **k)) or seen[-1])
    ids = torch.randint(0, 512, (2, 16))
    am = torch.ones(2, 16, dtype=torch.long)
    am[0, 9:] = 0
    before = swap.attention_stats()
    with torch.no_grad():
        a = m(ids, attention_mask=am).logits
        b = ref(ids, attention_mask=am).logits
    after = swap.attention_stats()
    layers = m.config.num_hidden_layers
    assert len(seen) == layers and all(r is not None and r[0].tolist() == [9, 16] and r[1] is False for r in seen)
    assert after["sdpa"] == before["sdpa"] + layers and after["k8"] == before["k8"]
    torch.testing.assert_close(a[0, :9], b[0, :9], atol=2e-5, rtol=2e-5)
    torch.testing.assert_close(a[1], b[1], atol=2e-5, rtol=2e-5)


# ------------------------------------------------------------------ cross-attention keeps SDPA
class _Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@needs_hf
@pytest.mark.parametrize("cfg", [_Cfg(is_encoder_decoder=True), _Cfg(add_cross_attention=True, is_decoder=True)],
                         ids=["encoder_decoder", "add_cross_attention"])
def test_hf_mask_function_attaches_nothing_for_models_that_cross_attend(cfg):
    """A cross-attention mask over source and target of one padded length is built like a self-attention
    mask (same lengths, zero offsets, the bidirectional function) from the ENCODER's padding mask: for a
    config that can cross-attend nothing is attached; the same call with a plain config attaches."""
    from transformers.masking_utils import bidirectional_mask_function

    from madnn.nn import swap

    am = torch.tensor([[1, 1, 1, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1, 1, 1]], dtype=torch.bool)
    kw = dict(mask_function=bidirectional_mask_function, attention_mask=am, allow_is_bidirectional_skip=False)
    mask = swap.madnn_mask(2, 8, 8, 0, 0, config=cfg, **kw)
    assert isinstance(mask, torch.Tensor) and ops._attached(mask, swap._SEQLENS) is None
    plain = swap.madnn_mask(2, 8, 8, 0, 0, config=_Cfg(is_encoder_decoder=False), **kw)
    assert ops._attached(plain, swap._SEQLENS) is not None


@needs_hf
def test_hf_attention_forward_refuses_lengths_for_a_cross_attention_module(monkeypatch):
    """Even a mask that carries lengths runs SDPA in a cross-attention module.  K8 is made to look
    available (and to fail loudly if called): the self-attention module takes it, the cross-attention
    modules do not."""
    from madnn.nn import swap

    mask, rec = _mask_fn(torch.tensor([[1, 1, 1, 1, 0, 0], [1, 1, 1, 1, 1, 1]], dtype=torch.bool))
    assert rec is not None
    q, k, v = (torch.randn(2, 4, 6, 8) for _ in range(3))

    class _Self(torch.nn.Module):
        is_causal = False
        num_key_value_groups = 1

    class _BertCrossAttention(_Self):
        pass

    class _Flagged(_Self):
        is_cross_attention = True

    called = []

    def k8(*a, **kw):
        called.append(kw.get("seqlens"))
        raise AssertionError("K8 taken")

    monkeypatch.setattr(ops, "attention_supported", lambda *a, **k: True)
    monkeypatch.setattr(ops, "attention", k8)
    with pytest.raises(AssertionError, match="K8 taken"):
        swap.madnn_attention_forward(_Self(), q, k, v, mask, scaling=8 ** -0.5, is_causal=False)
    assert len(called) == 1 and called[0] is not None
    for mod in (_BertCrossAttention(), _Flagged()):
        before = swap.attention_stats()
        swap.madnn_attention_forward(mod, q, k, v, mask, scaling=8 ** -0.5, is_causal=False)
        after = swap.attention_stats()
        assert after["sdpa"] == before["sdpa"] + 1 and after["k8"] == before["k8"]
    assert len(called) == 1


@needs_hf
def test_hf_bart_equal_source_and_target_length_never_carries_lengths(monkeypatch):
    """A tiny BART with source and target padded to one length, the encoder mask right-padded: no
    attention call (encoder self, decoder self, cross) sees a mask with lengths, and the swapped model
    equals the stock one."""
    import copy

    from transformers import BartConfig, BartForConditionalGeneration

    from madnn.nn import swap, use_madnn_kernels

    torch.manual_seed(0)
    cfg = BartConfig(vocab_size=128, d_model=32, encoder_layers=1, decoder_layers=1, encoder_attention_heads=2,
                     decoder_attention_heads=2, encoder_ffn_dim=64, decoder_ffn_dim=64, max_position_embeddings=32,
                     pad_token_id=1, bos_token_id=0, eos_token_id=2, decoder_start_token_id=2,
                     attn_implementation="sdpa")
    m = BartForConditionalGeneration(cfg).eval()
    ref = copy.deepcopy(m)
    use_madnn_kernels(m)
    seen = []
    real = ops._attached
    monkeypatch.setattr(ops, "_attached", lambda t, name, *a, **k: seen.append(real(t, name, *a, **k)) or seen[-1])
    ids = torch.randint(3, 128, (2, 8))
    am = torch.ones(2, 8, dtype=torch.long)
    am[0, 3:] = 0
    dec = torch.randint(3, 128, (2, 8))
    with torch.no_grad():
        a = m(input_ids=ids, attention_mask=am, decoder_input_ids=dec).logits
        b = ref(input_ids=ids, attention_mask=am, decoder_input_ids=dec).logits
    assert seen and all(r is None for r in seen), seen
    torch.testing.assert_close(a, b, atol=2e-5, rtol=2e-5)
