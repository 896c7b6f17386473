"""Hugging Face BERT / GPT-2 with a right-padded ``attention_mask`` through ``use_madnn_kernels`` on the
GPU: every layer's attention runs K8 with per-sequence lengths (none falls back to SDPA), and the loss
and parameter gradients track the fp32 eager copy of the same model.  Models are built from configs."""
import copy

import pytest
import torch

pytest.importorskip("transformers")

pytestmark = pytest.mark.gpu

LAYERS = 2
B, S, LENS = 3, 96, (96, 40, 65)


def _build(kind):
    from madnn.models import hf

    torch.manual_seed(0)
    if kind == "gpt2":
        return hf.gpt2_hf("gpt2-tiny", n_embd=256, n_head=4, n_layer=LAYERS, attn_pdrop=0.0, resid_pdrop=0.0,
                          embd_pdrop=0.0)
    return hf.bert_hf(hidden_size=256, num_attention_heads=4, intermediate_size=512, num_hidden_layers=LAYERS,
                      hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)


def _batch(device, left=False):
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1, 512, (B, S), generator=g)
    pos = torch.arange(S)[None, :]
    ln = torch.tensor(LENS)[:, None]
    am = (pos >= S - ln) if left else (pos < ln)
    labels = torch.where(am, ids, torch.full_like(ids, -100))
    return ids.to(device), am.long().to(device), labels.to(device)


def _rel(a, b):
    a, b = a.detach().float(), b.detach().float()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


@pytest.mark.parametrize("kind", ["bert", "gpt2"])
def test_right_padded_batch_runs_k8_and_tracks_fp32(cuda, kind):
    """Tolerance: the 3e-2 relative bound tests/test_hf_gpu.py puts on the bf16 loss against the fp32
    eager copy, applied to the gradient of EVERY parameter on its own, |g - r| <= 3e-2 |r| + floor, so a
    wrong gradient in a bias or a LayerNorm cannot hide behind the embeddings.  The absolute floor gives
    a parameter whose gradient is nearly zero a scale: 1e-3 of what the bound allows all gradients taken
    as one vector, floor = 1e-3 * 3e-2 * |r_all| (norms are L2)."""
    from madnn.nn import use_madnn_kernels
    from madnn.nn.swap import attention_stats

    model = _build(kind)
    ref = copy.deepcopy(model).to(cuda).float().train()
    model = model.to(cuda).bfloat16().train()
    assert use_madnn_kernels(model).get("hf_attention") == 1
    ids, am, labels = _batch(cuda)
    before = attention_stats()
    loss = model(ids, attention_mask=am, labels=labels).loss
    after = attention_stats()
    assert after["k8"] == before["k8"] + LAYERS, (before, after)
    assert after["sdpa"] == before["sdpa"], (before, after)
    loss.backward()
    rloss = ref(ids, attention_mask=am, labels=labels).loss
    rloss.backward()
    print(kind, "loss", float(loss.detach()), "fp32", float(rloss.detach()))
    assert abs(float(loss) - float(rloss)) < 3e-2 * float(rloss)
    rp = dict(ref.named_parameters())
    pairs = [(name, p.grad, rp[name].grad) for name, p in model.named_parameters() if rp[name].grad is not None]
    floor = 1e-3 * 3e-2 * float(torch.cat([r.flatten() for _, _, r in pairs]).norm())
    bad = []
    for name, g, r in pairs:
        assert g is not None and torch.isfinite(g.float()).all(), name
        err, bound = float((g.float() - r).norm()), 3e-2 * float(r.norm()) + floor
        print(kind, name, "error", err, "bound", bound, "relative", _rel(g, r))
        if err > bound:
            bad.append((name, err, bound))
    assert not bad, bad


@pytest.mark.parametrize("kind", ["bert", "gpt2"])
def test_left_padded_batch_counts_sdpa_only(cuda, kind):
    from madnn.nn import use_madnn_kernels
    from madnn.nn.swap import attention_stats

    model = _build(kind).to(cuda).bfloat16().eval()
    use_madnn_kernels(model)
    ids, am, _ = _batch(cuda, left=True)
    before = attention_stats()
    with torch.no_grad():
        model(ids, attention_mask=am)
    after = attention_stats()
    assert after["sdpa"] == before["sdpa"] + LAYERS, (before, after)
    assert after["k8"] == before["k8"], (before, after)
