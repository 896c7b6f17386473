"""K8 attention at the inputs its shipped code paths reach and the other attention tests do not:
an explicit softmax scale, sequences below one tile, foreign strides, workgroup grids on the
remainder branch of the XCD remap, odd and large GQA groups, the LSE itself, and masks checked
exactly (by counting keys) instead of through a global norm.

Every kernel instantiation of launch_fwd / launch_bwd (attn.hip) is reached with a scale other than
D ** -0.5 by test_explicit_scale / test_explicit_scale_dropout (scales 1 / D and 0.3 each):

  forward ring      attn_fwd_dma_kernel<causal | full>            (2, 256, 4, 2, 64) causal / full
  forward           attn_fwd_kernel<64, causal | full>            (1, 200, 4, 2, 64) causal / full
                    attn_fwd_kernel<128, causal | full>           (1, 200, 4, 2, 128) causal / full
  forward, dropout  attn_fwd_kernel<64, causal, DROP>             (1, 200, 4, 2, 64) causal, p = 0.1
                    attn_fwd_kernel<64, full, DROP>               (1, 77, 3, 3, 64) full, p = 0.1
                    attn_fwd_kernel<128, causal, DROP>            (1, 200, 4, 2, 128) causal, p = 0.1
                    attn_fwd_kernel<128, full, DROP>              (1, 130, 2, 2, 128) full, p = 0.1
  dQ                attn_bwd_dq_kernel<64 | 128, causal | full>   all six shapes of test_explicit_scale (the
                                                                  ring shape too: dQ has no ring kernel)
  dQ, dropout       attn_bwd_dq_kernel<D, c, DROP>                the four dropout cases above
  dK/dV ring        attn_bwd_dkdv_dma_kernel<causal | full>       (2, 256, 4, 2, 64) causal / full
  dK/dV             attn_bwd_dkdv_kernel<64 | 128, causal | full> the four S = 200 cases
  dK/dV, dropout    attn_bwd_dkdv_kernel<D, c, DROP>              the four dropout cases above
  column sums       dQ / dK / dV epilogues with cpart             test_explicit_scale_packed_colsum (scale 0.3)

References are fp32 SDPA on the same bf16 values (fp64 where a bound is derived), and the host mirror
of the dropout mask for p > 0."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from madnn import ops
from madnn.ops import reference
from test_attention_dropout_gpu import _ref as _drop_ref

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634
NAMES = ("o", "dq", "dk", "dv")
RNG = (1234, 8)


def _ref(q, k, v, causal, scale):
    h, hkv = q.size(2), k.size(2)
    o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), is_causal=causal,
                                       scale=scale, enable_gqa=h != hkv)
    return o.transpose(1, 2)


def _rel(a, b):
    a, b = a.detach().float(), b.detach().float()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def _slab_rel(a, b):
    """_rel of every [S, D] slab of a [B, S, heads, D] tensor: [B, heads]."""
    a, b = a.detach().float(), b.detach().float()
    return (a - b).norm(dim=(1, 3)) / b.norm(dim=(1, 3)).clamp_min(1e-12)


def _bounds(scale):
    """(o, gradient) bounds on the global relative error: those of test_attention_fwd_bwd, and those
    of test_attention_online_softmax_rescale_branch for the sharper scores of scale = 0.3."""
    return (1.5e-2, 3e-2) if scale == 0.3 else (1e-2, 2e-2)


def _inputs(device, B, S, H, HKV, D, seed=0):
    torch.manual_seed(seed)
    q = torch.randn(B, S, H, D, device=device).bfloat16()
    k = torch.randn(B, S, HKV, D, device=device).bfloat16()
    v = torch.randn(B, S, HKV, D, device=device).bfloat16()
    do = torch.randn(B, S, H, D, device=device).bfloat16()
    return q, k, v, do


def _reference(q, k, v, do, causal, scale, p=0.0, rng=RNG, dtype=torch.float32):
    """(o, dq, dk, dv) of the reference in ``dtype`` on the values of the bf16 inputs."""
    B, S, H, _ = q.shape
    qr, kr, vr = (t.detach().to(dtype).requires_grad_(True) for t in (q, k, v))
    if p > 0.0 or dtype == torch.float64:
        if p > 0.0:
            keep = reference.attention_dropout_mask(B, H, S, p, *rng).to(q.device)
            rp = 256.0 / reference.attention_dropout_threshold(p)
        else:
            keep, rp = torch.ones((), dtype=dtype, device=q.device), 1.0
        orf = _drop_ref(qr, kr, vr, causal, scale, keep, rp)
    else:
        orf = _ref(qr, kr, vr, causal, scale)
    return (orf.detach(), *torch.autograd.grad(orf, (qr, kr, vr), do.to(dtype)))


def run_case(device, B, S, H, HKV, D, causal, scale=None, p=0.0, seed=0):
    """Forward plus all three gradients of ops.attention and of the fp32 reference (the host-mask
    reference for p > 0).  Returns (got, ref, inputs), got / ref = (o, dq, dk, dv)."""
    q, k, v, do = _inputs(device, B, S, H, HKV, D, seed)
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    o = ops.attention(q, k, v, causal=causal, scale=scale, dropout_p=p, rng=RNG if p > 0.0 else None)
    assert o.shape == (B, S, H, D) and o.is_contiguous()
    got = (o.detach(), *torch.autograd.grad(o, (q, k, v), do))
    ref = _reference(q, k, v, do, causal, D ** -0.5 if scale is None else scale, p)
    return got, ref, (q.detach(), k.detach(), v.detach(), do)


def _single_key_zero_bounds(q, k, v, do, scale, p):
    """S = 1: dq and dk are zero in exact arithmetic (one key: dS = P (dP - delta) with dP = delta), so
    an error relative to the reference is undefined.  Elementwise bounds on what the kernels may leave
    instead: dP = rp M sum_i do_i v_i and delta = sum_i do_i o_i are two fp32 sums of the same D
    products (each within D 2^-24 sum |do_i v_i| of the exact sum), and with dropout o = bf16(rp v)
    carries one more rounding (relative 2^-8 at the most).  So |dS| <= eps rp A, A = sum_i |do_i v_i|,
    eps = 2 D 2^-24 (+ 2^-8 with dropout); dq = scale dS k and dk = scale sum_h dS_h q_h over the
    group's heads, with 2^-6 of slack for P (that of the dK/dV kernel is 1 only to the rounding of the
    prescaled Q) and the bf16 roundings of dS and of the store."""
    B, _, H, D = q.shape
    g = H // k.size(2)
    rp = 256.0 / reference.attention_dropout_threshold(p) if p > 0.0 else 1.0
    eps = 2.0 * D * 2.0 ** -24 + (2.0 ** -8 if p > 0.0 else 0.0)
    vh = v.double().repeat_interleave(g, dim=2)
    ds = eps * rp * (do.double() * vh).abs().sum(-1, keepdim=True) * (1 + 2.0 ** -6)   # [B, 1, H, 1]
    dq_b = scale * ds * k.double().repeat_interleave(g, dim=2).abs()
    dk_b = scale * (ds * q.double().abs()).view(B, 1, k.size(2), g, D).sum(3)
    return dq_b, dk_b


def check_case(device, B, S, H, HKV, D, causal, scale=None, p=0.0, seed=0, fuzz=False):
    """run_case under the project's bounds (see _bounds).  ``fuzz``: at S < 8 a global norm of o is over
    too few elements to mean much at an arbitrary shape, and o is compared elementwise only, as
    test_attention_fwd_bwd does (next to the norm) at every S."""
    got, ref, (q, k, v, do) = run_case(device, B, S, H, HKV, D, causal, scale, p, seed)
    bo, bg = _bounds(scale)
    errs = {n: _rel(a, b) for n, a, b in zip(NAMES, got, ref)}
    print((B, S, H, HKV, D, causal, scale, p), errs)
    for n, a in zip(NAMES, got):
        assert torch.isfinite(a.float()).all(), n
    if S >= 8 or not fuzz:
        assert errs["o"] < bo, errs
    if S < 8 or (p == 0.0 and scale != 0.3):
        torch.testing.assert_close(got[0].float(), ref[0], atol=3e-2, rtol=3e-2)
    zero = _single_key_zero_bounds(q, k, v, do, D ** -0.5 if scale is None else scale, p) if S == 1 else None
    for i, n in enumerate(NAMES[1:], 1):
        if zero is not None and n in ("dq", "dk"):
            bound = zero[i - 1]
            over = (got[i].double().abs() - bound).max()
            assert over <= 0, (n, float(over), float(got[i].float().abs().max()), float(bound.max()))
        else:
            assert errs[n] < bg, (n, errs)
    return got, ref, (q, k, v, do)


# ------------------------------------------------------------------ 1. explicit scale
SCALE_SHAPES = [
    (2, 256, 4, 2, 64),     # both LDS-DMA rings (forward, dK/dV)
    (1, 200, 4, 2, 64),     # register-staged D = 64
    (1, 200, 4, 2, 128),
]
SCALE_DROPOUT = [
    (1, 200, 4, 2, 64, True),
    (1, 130, 2, 2, 128, False),
    (1, 77, 3, 3, 64, False),     # the two remaining DROP instantiations
    (1, 200, 4, 2, 128, True),
]


def _scale(name, D):
    return 1.0 / D if name == "1/D" else name


@pytest.mark.parametrize("scale", ["1/D", 0.3])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("B,S,H,HKV,D", SCALE_SHAPES)
def test_explicit_scale(cuda, B, S, H, HKV, D, causal, scale):
    check_case(cuda, B, S, H, HKV, D, causal, _scale(scale, D))


@pytest.mark.parametrize("scale", ["1/D", 0.3])
@pytest.mark.parametrize("B,S,H,HKV,D,causal", SCALE_DROPOUT)
def test_explicit_scale_dropout(cuda, B, S, H, HKV, D, causal, scale):
    check_case(cuda, B, S, H, HKV, D, causal, _scale(scale, D), p=0.1)


def test_explicit_scale_packed_colsum(cuda, monkeypatch):
    """attention_qkvpacked(scale = 0.3) behind a biased ops.linear: the column sums of the backward
    kernels (the projection's bias gradient) see the scale through dq and dk."""
    calls = []
    real = ops.bias_grad
    monkeypatch.setattr(ops, "bias_grad", lambda *a, **k: calls.append(1) or real(*a, **k))
    torch.manual_seed(9)
    B, E, H, HKV, D, S, scale = 2, 256, 4, 2, 64, 200, 0.3
    x = torch.randn(B, S, E, device=cuda, dtype=torch.bfloat16, requires_grad=True)
    w = (torch.randn((H + 2 * HKV) * D, E, device=cuda) * E ** -0.5).bfloat16().requires_grad_()
    b = (torch.randn((H + 2 * HKV) * D, device=cuda) * 0.1).bfloat16().requires_grad_()
    g = torch.randn(B, S, H, D, device=cuda)
    qkv = ops.linear(x, w, b).view(B, S, H + 2 * HKV, D)
    o = ops.attention_qkvpacked(qkv, H, HKV, causal=True, scale=scale)
    (o.float() * g).sum().backward()
    assert not calls, "the QKV projection ran its own bias column-sum pass"
    xf, wf, bf = (t.detach().float().requires_grad_() for t in (x, w, b))
    qf = F.linear(xf, wf, bf).view(B, S, H + 2 * HKV, D)
    q, k, v = qf.split([H, HKV, HKV], dim=2)
    orf = _ref(q, k, v, True, scale)
    (orf * g).sum().backward()
    errs = {"o": _rel(o, orf), "db": _rel(b.grad, bf.grad), "dw": _rel(w.grad, wf.grad), "dx": _rel(x.grad, xf.grad)}
    print(errs)
    bo, bg = _bounds(scale)
    assert errs["o"] < bo, errs
    assert errs["db"] < bg and errs["dw"] < bg and errs["dx"] < bg, errs


# ------------------------------------------------------------------ 2. tiny and tile-edge lengths
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129])
def test_tiny_and_tile_edge_lengths(cuda, S, D, causal):
    """S = 64 / 128 at D = 64: the DMA rings shorter than their depth (forward ntiles 1 and 2)."""
    B, H, HKV = 2, 4, 2
    got, _, (q, k, v, do) = check_case(cuda, B, S, H, HKV, D, causal)
    if S == 1:   # one key: softmax = 1, o is v of the query head's KV head
        torch.testing.assert_close(got[0].float(), v.repeat_interleave(H // HKV, dim=2).float(), rtol=2.0 ** -7, atol=0)


@pytest.mark.parametrize("B,S,H,HKV,causal", [(2, 64, 2, 2, True), (2, 64, 2, 2, False), (1, 192, 2, 2, True),
                                              (1, 128, 3, 3, True)])
def test_ring_dkdv_shorter_than_its_depth(cuda, B, S, H, HKV, causal):
    """The ring dK/dV walks G * nt tiles: with G = 1, S = 64 (and the last causal key block of S = 192)
    is the one-tile walk (its `total > 1` branch not taken), S = 128 causal one of two and one of one."""
    check_case(cuda, B, S, H, HKV, 64, causal)


# ------------------------------------------------------------------ 3. remap grids, group sizes
def _poison_then_free(device, *specs):
    ts = [torch.full(shape, float("nan"), dtype=dt, device=device) for shape, dt in specs]
    del ts


def _direct(q, k, v, do, causal, scale, outs=None, p=0.0, rng=(0, 0)):
    """torch.ops.madnn.attn_fwd / attn_bwd called directly: (o, lse, dq, dk, dv).  The gradient
    outputs (``outs``, or fresh ones) are NaN-filled before the call; for o and lse, which the binding
    allocates, NaN-filled tensors of their shapes and dtypes are freed right before it (best effort:
    the caching allocator usually hands the same blocks back)."""
    B, S, H, D = q.shape
    _poison_then_free(q.device, ((B, S, H, D), torch.bfloat16), ((B, H, S), torch.float32))
    o, lse = torch.ops.madnn.attn_fwd(q, k, v, causal, scale, p, *rng)
    dq, dk, dv = outs if outs is not None else (torch.empty_like(q), torch.empty_like(k), torch.empty_like(v))
    for t in (dq, dk, dv):
        t.fill_(float("nan"))
    torch.ops.madnn.attn_bwd(do, q, k, v, o, lse, dq, dk, dv, causal, scale, None, p, *rng)
    return o, lse, dq, dk, dv


GRID_CASES = [
    (3, 200, 6, 3, 64, True),      # 36 / 18 workgroups
    (1, 300, 7, 7, 128, False),    # 21 / 21
    (5, 64, 3, 1, 64, True),       # 15 / 5, rings, G = 3
    (3, 192, 5, 5, 64, False),     # 30 / 30, rings
    (1, 130, 8, 1, 128, True),     # G = 8
]


@pytest.mark.parametrize("B,S,H,HKV,D,causal", GRID_CASES)
def test_remap_grids_and_groups_per_head(cuda, B, S, H, HKV, D, causal):
    """Grids above 8 workgroups that are no multiple of 8 (the remainder branch of map_block), odd GQA
    groups and G = 8.  The bounds of test_attention_fwd_bwd hold for every (batch, head) slab of o,
    dq, dk and dv, so a block that landed on the wrong head cannot average out, and every output
    starts as NaN, so a block that was never computed cannot pass.  For o and lse that poison is best
    effort: the binding allocates them, and the test can only leave NaN in the blocks it expects the
    allocator to hand back."""
    q, k, v, do = _inputs(cuda, B, S, H, HKV, D, seed=3)
    scale = D ** -0.5
    o, lse, dq, dk, dv = _direct(q, k, v, do, causal, scale)
    for n, t in zip(("o", "lse", "dq", "dk", "dv"), (o, lse, dq, dk, dv)):
        assert torch.isfinite(t.float()).all(), n
    ref = _reference(q, k, v, do, causal, scale)
    worst = {n: float(_slab_rel(a, b).max()) for n, a, b in zip(NAMES, (o, dq, dk, dv), ref)}
    print((B, S, H, HKV, D, causal), worst)
    assert worst["o"] < 1e-2, worst
    for n in NAMES[1:]:
        assert worst[n] < 2e-2, (n, worst)


# ------------------------------------------------------------------ 4. foreign strides
LAYOUT_SHAPES = [
    (2, 96, 4, 2, 64),
    (2, 130, 4, 2, 128),
    (2, 128, 4, 2, 64),    # the LDS-DMA kernels, whose per-lane offsets come from the sequence stride
]


@functools.lru_cache(maxsize=None)
def _layout_base(device, B, S, H, HKV, D):
    """Inputs and the results of fresh contiguous tensors (causal, default scale); never modified."""
    q, k, v, do = _inputs(device, B, S, H, HKV, D, seed=4)
    return (q, k, v, do), _via_autograd(q, k, v, do)


def _via_autograd(q, k, v, do):
    q, k, v = (t.detach().requires_grad_(True) for t in (q, k, v))
    o = ops.attention(q, k, v, causal=True)
    return (o.detach(), *torch.autograd.grad(o, (q, k, v), do))


def _hf(t):
    """[B, S, heads, D] values stored [B, heads, S, D]: sequence stride D, head stride S * D."""
    return t.transpose(1, 2).contiguous().transpose(1, 2)


def _cache(t, pad=40, off=3):
    """A slice [:, off:off + S] of a [B, S + pad, heads, D] buffer: padded batch stride, storage
    offset off * heads * D (16-byte aligned); the rest of the buffer is NaN."""
    B, S, h, D = t.shape
    buf = torch.full((B, S + pad, h, D), float("nan"), dtype=t.dtype, device=t.device)
    buf[:, off:off + S] = t
    return buf[:, off:off + S]


LAYOUTS = {
    "hf": lambda q, k, v, do: (_hf(q), _hf(k), _hf(v), do),
    "kvcache": lambda q, k, v, do: (q, _cache(k), _cache(v), do),
    "dout_transposed": lambda q, k, v, do: (q, k, v, _hf(do)),
    # every operand in a layout of its own (q against k / v head strides, k against v batch strides)
    "mixed": lambda q, k, v, do: (_hf(q), _cache(k), _cache(v, pad=24, off=5), _hf(do)),
}


@pytest.mark.parametrize("B,S,H,HKV,D", LAYOUT_SHAPES)
def test_contiguous_baseline_of_the_layouts_meets_fp32(cuda, B, S, H, HKV, D):
    (q, k, v, do), got = _layout_base(cuda, B, S, H, HKV, D)
    ref = _reference(q, k, v, do, True, D ** -0.5)
    errs = {n: _rel(a, b) for n, a, b in zip(NAMES, got, ref)}
    assert errs["o"] < 1e-2, errs
    for n in NAMES[1:]:
        assert errs[n] < 2e-2, (n, errs)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("B,S,H,HKV,D", LAYOUT_SHAPES)
def test_foreign_strides_bitwise_equal_to_contiguous(cuda, B, S, H, HKV, D, layout):
    """A layout must not change arithmetic: o and the three gradients are bit for bit those of the
    same values in fresh contiguous tensors."""
    base, want = _layout_base(cuda, B, S, H, HKV, D)
    q, k, v, do = LAYOUTS[layout](*base)
    if layout in ("hf", "mixed"):
        assert q.stride(1) == D and q.stride(2) == S * D
    if layout in ("kvcache", "mixed"):
        assert k.stride(0) == (S + 40) * HKV * D and k.storage_offset() == 3 * HKV * D
    got = _via_autograd(q, k, v, do)
    for n, a, b in zip(NAMES, got, want):
        assert a.shape == b.shape
        assert torch.equal(a, b), (layout, n, _rel(a, b))


@pytest.mark.parametrize("B,S,H,HKV,D", LAYOUT_SHAPES)
def test_bwd_outputs_as_slices_of_a_padded_buffer(cuda, B, S, H, HKV, D):
    """attn_bwd writing dq, dk, dv into slices of one padded buffer (a guard row of sequence before
    and after, a guard head before, between and after the three): the results are bitwise those of
    contiguous outputs, and every element outside the slices keeps its sentinel."""
    (q, k, v, do), want = _layout_base(cuda, B, S, H, HKV, D)
    sentinel = -1234.0
    heads = H + 2 * HKV + 4
    buf = torch.full((B, S + 2, heads, D), sentinel, dtype=torch.bfloat16, device=cuda)
    h0, h1, h2 = 1, H + 2, H + HKV + 3
    outs = (buf[:, 1:S + 1, h0:h0 + H], buf[:, 1:S + 1, h1:h1 + HKV], buf[:, 1:S + 1, h2:h2 + HKV])
    o, _, dq, dk, dv = _direct(q, k, v, do, True, D ** -0.5, outs=outs)
    for n, a, b in zip(NAMES, (o, dq, dk, dv), want):
        assert torch.equal(a, b), (n, _rel(a, b))
    guard = buf.clone()
    for t in (guard[:, 1:S + 1, h0:h0 + H], guard[:, 1:S + 1, h1:h1 + HKV], guard[:, 1:S + 1, h2:h2 + HKV]):
        t.fill_(sentinel)
    assert torch.equal(guard, torch.full_like(guard, sentinel))


# ------------------------------------------------------------------ 5. LSE
def _lse_ref_and_bound(q, k, causal, scale):
    """fp64 LSE in log2 units [B, H, S] of the bf16 inputs, and the per-row bound on the kernels'
    deviation: the one modelled rounding is that of the prescaled Q to bf16 (relative <= 2^-8 per
    element) and the LSE is 1-Lipschitz in the max-norm of the scores, so |dLSE| <= 2^-8 max_k sum_i
    |c q_i k_i| + 1e-4 over the row's visible keys, c = scale log2(e).  The 1e-4 covers the fp32
    accumulation over D <= 128 terms (<= 2^-17 of the same sum), the hardware exp2 / log2 and the fp32
    row sum with a tenfold margin."""
    g = q.size(2) // k.size(2)
    qd = q.double().transpose(1, 2)
    kd = k.double().transpose(1, 2).repeat_interleave(g, dim=1)
    s = scale * (qd @ kd.transpose(-1, -2))
    a = scale * LOG2E * (qd.abs() @ kd.abs().transpose(-1, -2))
    if causal:
        n = s.size(-1)
        vis = torch.ones(n, n, dtype=torch.bool, device=s.device).tril()
        s = s.masked_fill(~vis, float("-inf"))
        a = a.masked_fill(~vis, 0.0)
    return torch.logsumexp(s, dim=-1) / math.log(2.0), 2.0 ** -8 * a.max(dim=-1).values + 1e-4


@pytest.mark.parametrize("scale", [None, 0.3])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("B,S,H,HKV,D", [(1, 130, 2, 2, 64), (1, 256, 2, 1, 64), (1, 130, 2, 2, 128)])
def test_lse_within_derived_bound(cuda, B, S, H, HKV, D, causal, scale):
    q, k, v, _ = _inputs(cuda, B, S, H, HKV, D, seed=5)
    scale = D ** -0.5 if scale is None else scale
    _, lse = torch.ops.madnn.attn_fwd(q, k, v, causal, scale, 0.0, 0, 0)
    assert lse.shape == (B, H, S) and lse.dtype == torch.float32
    want, bound = _lse_ref_and_bound(q, k, causal, scale)
    ratio = (lse.double() - want).abs() / bound
    print((B, S, H, HKV, D, causal, scale), "worst |dLSE| / bound", float(ratio.max()))
    assert ratio.max() <= 1.0, float(ratio.max())


@pytest.mark.parametrize("D", [64, 128])
def test_lse_is_that_of_the_undropped_softmax(cuda, D):
    """p = 0.5 against p = 0 on a ragged S (both on the register-staged forward): the same LSE bit
    for bit, while o differs."""
    q, k, v, _ = _inputs(cuda, 1, 130, 2, 2, D, seed=6)
    o0, lse0 = torch.ops.madnn.attn_fwd(q, k, v, True, 0.3, 0.0, 0, 0)
    o1, lse1 = torch.ops.madnn.attn_fwd(q, k, v, True, 0.3, 0.5, *RNG)
    assert torch.equal(lse0, lse1)
    assert not torch.equal(o0, o1)


# ------------------------------------------------------------------ 6. exact masks by counting
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [33, 65, 129])
def test_masks_exact_by_counting_keys(cuda, S, D, causal):
    """k = 0: every score is 0, p is exactly 1 and l exactly the number n of visible keys, so o[q] is
    the mean of the visible v rows rounded once to bf16 (rtol 2^-7 = one bf16 ulp; one key too many
    or too few moves a row by about |v| / n, 128 / sqrt(n) >= 11 times that).  Backward against fp64:
    dq = dS K is exactly zero; dv[k] = sum_{q sees k} do[q] / n_q and dk[k] = scale sum_q dS[q, k]
    q[q] carry only the bf16 roundings of dout, P and dS, and meet the project's gradient bound
    (2e-2) PER KEY ROW, each row's error normalised by the RMS row norm of the tensor, so a single
    wrong row is caught.  Measured on an MI355X: the worst row is at 0.0123 of the RMS row norm (dv,
    key 0, S = 129, D = 128, causal; dk 0.0119 at key 1 of the same case), 1.6 below the bound: the
    first keys of a causal sequence have by far the largest rows, and their terms P = 1 / n for small
    n carry the full bf16 rounding.  Full attention stays below 0.004."""
    B, H, HKV = 1, 4, 2
    q, _, v, do = _inputs(cuda, B, S, H, HKV, D, seed=7)
    k = torch.zeros_like(v)
    scale = D ** -0.5
    o, _, dq, dk, dv = _direct(q, k, v, do, causal, scale)
    vd = v.double().repeat_interleave(H // HKV, dim=2)
    if causal:
        n = torch.arange(1, S + 1, device=cuda, dtype=torch.float64).view(1, S, 1, 1)
        mean = vd.cumsum(1) / n
    else:
        mean = vd.mean(1, keepdim=True).expand(B, S, H, D)
    torch.testing.assert_close(o.double(), mean, rtol=2.0 ** -7, atol=1e-5)
    assert torch.equal(dq, torch.zeros_like(dq))
    _, _, rk, rv = _reference(q, k, v, do, causal, scale, dtype=torch.float64)
    for name, got, ref in (("dk", dk, rk), ("dv", dv, rv)):
        rms = ref.norm(dim=-1).square().mean().sqrt()
        row = (got.double() - ref).norm(dim=-1) / rms
        key, head = divmod(int(row.argmax()), HKV)
        print((S, D, causal), name, "worst row error / RMS row norm", float(row.max()), "key", key, "kv head", head)
        assert row.max() < 2e-2, (name, float(row.max()), key, head)


# ------------------------------------------------------------------ 7. scale <= 0 or non-finite
@pytest.mark.parametrize("scale", [-0.125, 0.0, float("inf")])
def test_kernels_refuse_a_scale_that_is_not_finite_and_positive(cuda, scale):
    q, k, v, _ = _inputs(cuda, 1, 65, 2, 2, 64)
    with pytest.raises(RuntimeError):
        torch.ops.madnn.attn_fwd(q, k, v, True, scale, 0.0, 0, 0)
    o = torch.empty_like(q)
    lse = torch.empty(1, 2, 65, device=cuda)
    with pytest.raises(RuntimeError):
        torch.ops.madnn.attn_bwd(o, q, k, v, o, lse, torch.empty_like(q), torch.empty_like(k), torch.empty_like(v),
                                 True, scale, None, 0.0, 0, 0)


@pytest.mark.parametrize("packed", [False, True])
def test_negative_scale_runs_sdpa(cuda, monkeypatch, packed):
    """ops.attention / attention_qkvpacked(scale = -0.125) on bf16 device tensors take
    reference.attention (the register-staged causal dK/dV would compute exp2(+inf) on its masked
    scores) and match the fp32 reference forward and backward under the bounds of
    test_attention_fwd_bwd."""
    calls = []
    real = reference.attention
    monkeypatch.setattr(reference, "attention", lambda *a, **k: calls.append(k["scale"]) or real(*a, **k))
    B, S, H, HKV, D, scale = 1, 65, 4, 2, 64, -0.125
    q, k, v, do = _inputs(cuda, B, S, H, HKV, D, seed=8)
    if packed:
        qkv = torch.cat([q, k, v], dim=2).requires_grad_(True)
        o = ops.attention_qkvpacked(qkv, H, HKV, causal=True, scale=scale)
        gq, gk, gv = torch.autograd.grad(o, qkv, do)[0].split([H, HKV, HKV], dim=2)
    else:
        qg, kg, vg = (t.requires_grad_(True) for t in (q, k, v))
        o = ops.attention(qg, kg, vg, causal=True, scale=scale)
        gq, gk, gv = torch.autograd.grad(o, (qg, kg, vg), do)
    assert calls == [scale]
    ref = _reference(q, k, v, do, True, scale)
    errs = {n: _rel(a, b) for n, a, b in zip(NAMES, (o, gq, gk, gv), ref)}
    print(errs)
    assert all(math.isfinite(e) for e in errs.values()), errs
    assert errs["o"] < 1e-2, errs
    for n in NAMES[1:]:
        assert errs[n] < 2e-2, (n, errs)
