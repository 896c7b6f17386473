"""``reference.attention`` (what ``ops.attention`` runs for a softmax scale K8 refuses) at scales that
are not finite and positive, against an fp64 softmax written out; no GPU."""
import pytest
import torch

from madnn import ops
from madnn.ops import reference


def _manual(q, k, v, causal, scale):
    g = q.size(2) // k.size(2)
    qt, kt, vt = (t.double().transpose(1, 2) for t in (q, k, v))
    kt, vt = kt.repeat_interleave(g, dim=1), vt.repeat_interleave(g, dim=1)
    s = (qt @ kt.transpose(-1, -2)) * scale
    if causal:
        n = s.size(-1)
        s = s.masked_fill(~torch.ones(n, n, dtype=torch.bool).tril(), float("-inf"))
    return (torch.softmax(s, dim=-1) @ vt).transpose(1, 2)


@pytest.mark.parametrize("scale", [-0.125, 0.0, 0.125])
@pytest.mark.parametrize("causal", [True, False])
def test_reference_attention_any_finite_scale(scale, causal):
    torch.manual_seed(0)
    q = torch.randn(2, 37, 4, 64, requires_grad=True)
    k = torch.randn(2, 37, 2, 64, requires_grad=True)
    v = torch.randn(2, 37, 2, 64, requires_grad=True)
    do = torch.randn(2, 37, 4, 64)
    o = ops.attention(q, k, v, causal=causal, scale=scale)
    assert o.shape == (2, 37, 4, 64) and o.is_contiguous() and o.dtype == torch.float32
    got = (o, *torch.autograd.grad(o, (q, k, v), do))
    qd, kd, vd = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    od = _manual(qd, kd, vd, causal, scale)
    want = (od, *torch.autograd.grad(od, (qd, kd, vd), do.double()))
    for a, b in zip(got, want):
        torch.testing.assert_close(a.double(), b.detach(), atol=1e-5, rtol=1e-4)


def test_reference_attention_negative_scale_packed_and_bf16():
    torch.manual_seed(1)
    qkv = torch.randn(1, 20, 4 + 2 + 2, 64).bfloat16()
    o = ops.attention_qkvpacked(qkv, 4, 2, causal=True, scale=-0.125)
    q, k, v = qkv.split([4, 2, 2], dim=2)
    assert o.dtype == torch.bfloat16
    torch.testing.assert_close(o.double(), _manual(q, k, v, True, -0.125), atol=2e-2, rtol=2.0 ** -7)
    assert torch.equal(o, reference.attention(q, k, v, causal=True, scale=-0.125))
