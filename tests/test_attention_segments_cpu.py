"""Packed documents (``segments``) on the CPU: ``ops.segment_bounds``' host mirror against a plain loop,
``reference.attention(segments=...)`` in fp32 against SDPA run on every document's slice alone, and the
exclusion of ``seqlens``."""
import pytest
import torch
import torch.nn.functional as F

from madnn import ops
from madnn.ops import reference

ROWS = [[5, 5, 2, 2, 5, 5, 5], [7, 0, 0, 0, 3, 3, 9], [4, 4, 4, 4, 4, 4, 4]]   # unsorted, a repeated id, a
                                                                               # length-1 document, one document


def _loop_bounds(row):
    starts = [s for s in range(len(row)) if s == 0 or row[s] != row[s - 1]] + [len(row)]
    lo = [max(x for x in starts if x <= s) for s in range(len(row))]
    return [lo, [min(x for x in starts if x > s) for s in range(len(row))]]


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_segment_bounds_cpu_matches_a_loop(dtype):
    got = ops.segment_bounds(torch.tensor(ROWS, dtype=dtype))
    assert got.dtype == torch.int32 and got.shape == (3, 2, 7)
    assert got.tolist() == [_loop_bounds(r) for r in ROWS]


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("as_bounds", [False, True])
def test_reference_attention_segments_is_per_document_sdpa(causal, as_bounds):
    torch.manual_seed(0)
    ids = torch.tensor(ROWS)
    q, k, v = torch.randn(3, 7, 4, 16), torch.randn(3, 7, 2, 16), torch.randn(3, 7, 2, 16)
    got = reference.attention(q, k, v, causal=causal, segments=ops.segment_bounds(ids) if as_bounds else ids)
    for b, row in enumerate(ROWS):
        lo, hi = _loop_bounds(row)
        for a, e in sorted(set(zip(lo, hi))):
            want = F.scaled_dot_product_attention(*(t[b:b + 1, a:e].transpose(1, 2) for t in (q, k, v)),
                                                  is_causal=causal, enable_gqa=True).transpose(1, 2)
            torch.testing.assert_close(got[b:b + 1, a:e], want, atol=1e-5, rtol=1e-5)


def test_segments_with_seqlens_raises():
    q = torch.randn(3, 7, 2, 16)
    for fn in (ops.attention, reference.attention):
        with pytest.raises(ValueError):
            fn(q, q, q, segments=torch.tensor(ROWS), seqlens=torch.tensor([7, 7, 7]))
    with pytest.raises(ValueError):
        ops.attention_qkvpacked(torch.randn(3, 7, 6, 16), 2, 2, segments=torch.tensor(ROWS), seqlens=torch.tensor([7, 7, 7]))
