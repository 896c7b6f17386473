"""K8 attention over packed documents (``segments``): the SEG instantiations of the three register-staged
kernels against fp32 SDPA run on every document's slice ``[b, lo:hi]`` alone (``dout`` sliced the same way,
results scattered back), under test_attention_edges_gpu._bounds(None) -- the same arithmetic over fewer keys."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from madnn import ops
from test_attention_edges_gpu import NAMES, _bounds, _inputs, _ref, _rel

pytestmark = pytest.mark.gpu

# rows of (length, id) documents: ids unsorted, id 5 reused by two non-adjacent documents.  (72, 128): a boundary
# inside a wave (rows 64..71 | 72..95: the first computed tile of rows 72.. is fully masked for them) and a
# document across the 128-row block; (1, 63, 64, 72): a length-1 document, boundaries on a tile and a block edge
ROWS3 = (((72, 9), (128, 3)), ((1, 5), (63, 2), (64, 5), (72, 0)), ((130, 7), (70, 1)))
ROWS512 = (((64, 4), (192, 1), (256, 2)),)   # query block 256..383 starts at key tile 4; key block 0..127 ends at query 256


def _ids(rows, device):
    return torch.tensor([[i for n, i in row for _ in range(n)] for row in rows], device=device)


def _docs(rows):
    for b, row in enumerate(rows):
        lo = 0
        for n, _ in row:
            yield b, lo, lo + n
            lo += n


def _run(q, k, v, do, causal, seg):
    """(o, dq, dk, dv, lse) of the raw ops; ``seg``: bounds or None."""
    sc = q.size(-1) ** -0.5
    o, lse = torch.ops.madnn.attn_fwd(q, k, v, causal, sc, 0.0, 0, 0, None, seg)
    dq, dk, dv = (torch.full_like(t, float("nan")) for t in (q, k, v))
    torch.ops.madnn.attn_bwd(do, q, k, v, o, lse, dq, dk, dv, causal, sc, None, 0.0, 0, 0, None, seg)
    return o, dq, dk, dv, lse


@functools.lru_cache(maxsize=None)
def _reference(device, B, S, H, HKV, D, rows, causal):
    q, k, v, do = _inputs(device, B, S, H, HKV, D)
    outs = [torch.zeros(t.shape, device=device) for t in (q, q, k, v)]
    for b, lo, hi in _docs(rows):
        qr, kr, vr = (t[b:b + 1, lo:hi].float().requires_grad_(True) for t in (q, k, v))
        orf = _ref(qr, kr, vr, causal, D ** -0.5)
        for dst, src in zip(outs, (orf.detach(), *torch.autograd.grad(orf, (qr, kr, vr), do[b:b + 1, lo:hi].float()))):
            dst[b:b + 1, lo:hi] = src
    return tuple(outs)


def _check(device, B, S, H, HKV, D, rows, causal):
    ids = _ids(rows, device)
    seg = ops.segment_bounds(ids)
    assert seg.dtype == torch.int32 and torch.equal(seg.cpu(), ops.segment_bounds(ids.cpu()))
    *got, lse = _run(*_inputs(device, B, S, H, HKV, D), causal, seg)
    assert torch.isfinite(lse).all(), "lse"
    errs = {n: _rel(g, w) for n, g, w in zip(NAMES, got, _reference(device, B, S, H, HKV, D, rows, causal))}
    print((B, S, H, HKV, D, rows, causal), errs)
    bo, bg = _bounds(None)
    assert errs["o"] < bo and all(errs[n] < bg for n in NAMES[1:]), errs


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("D", [64, 128])
def test_segments_match_per_document_reference(cuda, D, causal):
    _check(cuda, 3, 200, 4, 2, D, ROWS3, causal)


@pytest.mark.parametrize("causal", [True, False])
def test_segments_leave_the_rings_and_offset_their_tile_ranges(cuda, causal):
    """S % 64 == 0 at D = 64 would send a dense call to both ring kernels."""
    _check(cuda, 1, 512, 4, 2, 64, ROWS512, causal)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("D", [64, 128])
def test_one_document_is_bitwise_the_dense_kernel(cuda, D, causal):
    inp = _inputs(cuda, 1, 200, 4, 2, D, seed=1)
    ids = torch.full((1, 200), 6, device=cuda)
    dense = _run(*inp, causal, None)
    for seg in (ops.segment_bounds(ids), None):
        if seg is None:   # through the public entry: ids, not bounds
            q, k, v = (t.clone().requires_grad_(True) for t in inp[:3])
            o = ops.attention(q, k, v, causal=causal, segments=ids)
            got = (o.detach(), *torch.autograd.grad(o, (q, k, v), inp[3]))
        else:
            got = _run(*inp, causal, seg)
        for n, a, b in zip(NAMES + ("lse",), got, dense):
            assert torch.equal(a, b), (n, _rel(a, b))


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("D", [64, 128])
def test_segment_masks_exact_by_counting_keys(cuda, D, causal):
    """The forward half of test_masks_exact_by_counting_keys: k = 0, so every visible key has p = 1 and o[q] is the
    mean of the visible v rows; dq = dS K is exactly zero."""
    q, _, v, do = _inputs(cuda, 1, 200, 4, 2, D, seed=7)
    o, dq, *_ = _run(q, torch.zeros_like(v), v, do, causal, ops.segment_bounds(_ids(ROWS3[:1], cuda)))
    vd, mean = v.double().repeat_interleave(2, dim=2), torch.empty(1, 200, 4, D, device=cuda, dtype=torch.float64)
    for _, lo, hi in _docs(ROWS3[:1]):
        n = torch.arange(1, hi - lo + 1, device=cuda, dtype=torch.float64).view(1, -1, 1, 1)
        mean[:, lo:hi] = vd[:, lo:hi].cumsum(1) / n if causal else vd[:, lo:hi].mean(1, keepdim=True)
    torch.testing.assert_close(o.double(), mean, rtol=2.0 ** -7, atol=1e-5)
    assert torch.equal(dq, torch.zeros_like(dq))


def test_segments_argument_is_checked(cuda):
    q, k, v, _ = _inputs(cuda, 2, 200, 4, 2, 64)
    good = ops.segment_bounds(torch.zeros(2, 200, dtype=torch.int32, device=cuda))
    sl = torch.full((2,), 200, dtype=torch.int32, device=cuda)
    bad = [(good.long(), None, 0.0), (good[:, :, :199].contiguous(), None, 0.0), (good.cpu(), None, 0.0),
           (good.transpose(1, 2).contiguous().transpose(1, 2), None, 0.0), (good, sl, 0.0), (good, None, 0.1)]
    for seg, lens, p in bad:
        with pytest.raises(RuntimeError):
            torch.ops.madnn.attn_fwd(q, k, v, True, 0.125, p, 1, 0, lens, seg)
    o = ops.attention(q, k, v, segments=good, dropout_p=0.1)   # the reference path: no kernel, no error
    assert o.shape == q.shape and torch.isfinite(o.float()).all()


def test_zoo_llama_packed_rows_match_per_document_fp32(cuda):
    """llama3-tiny at head dim 64, bf16, two packed rows of three documents: logits and parameter gradients against
    the fp32 eager copy run per document, under the suite's 5e-2 bound for bf16 transformers (test_gemmp_gpu)."""
    from madnn.models.llama import Llama, llama_config

    torch.manual_seed(3)
    cfg = llama_config("llama3-tiny", hidden=256, heads=4, kv_heads=2, intermediate=512, layers=2)
    ref = Llama(cfg).to(cuda).train()
    model = copy.deepcopy(ref).bfloat16().train()
    rows = (((72, 1), (100, 0), (28, 1)), ((50, 3), (50, 4), (100, 3)))
    ids, tgt = (torch.randint(0, cfg.vocab_size, (2, 200), device=cuda) for _ in range(2))
    calls, real = [], ops._AttnPackedFn.apply
    ops._AttnPackedFn.apply = lambda *a: calls.append(tuple(a[-1].shape) == (2, 2, 200)) or real(*a)
    try:
        logits = model(ids, _ids(rows, cuda))
    finally:
        ops._AttnPackedFn.apply = real
    assert calls == [True] * cfg.layers, "the layers did not run K8 with the bounds"
    F.cross_entropy(logits.float().view(-1, cfg.vocab_size), tgt.view(-1)).backward()
    for b, lo, hi in _docs(rows):
        rl = ref(ids[b:b + 1, lo:hi])
        assert _rel(logits[b:b + 1, lo:hi], rl) < 5e-2, (b, lo, hi)
        (F.cross_entropy(rl[0], tgt[b, lo:hi], reduction="sum") / tgt.numel()).backward()
    rp = dict(ref.named_parameters())
    for name, p in model.named_parameters():
        assert _rel(p.grad, rp[name].grad) < 5e-2, (name, _rel(p.grad, rp[name].grad))
