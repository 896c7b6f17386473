"""The deep 1x1 forwards on K12P with the BatchNorm-statistics epilogue (``gemmp.hip: kStats``), reached through
``madnn::conv1x1_fwd`` under the native switch ``madnn_conv1x1_tune`` key 4 (``ops.K9_DEEP``), against K9 (the
switch off) and fp32 / fp64 references.

Shapes (M, Cin, Cout): one 256x256 tile; 6 tiles over more than one i tile; 260 and 264 tiles, more than the 256
CUs, so some workgroups walk two tiles and an epilogue is followed by a K tile (the ``vmcnt(S + 4)`` wait whose
S counts the statistics stores).  One 4-D NHWC and one 2-D input in each group.  The deep plain data grad
(256 -> 512), which the same switch sends to K12P's plain kernel, is checked at 2 and at 260 tiles.
"""
import pytest
import torch
import torch.nn.functional as F

from madnn import ops

pytestmark = pytest.mark.gpu

# (N, H, W or None for a 2-D [M, Cin] input, Cin, Cout)
SHAPES = [(256, None, None, 256, 256), (2, 16, 16, 512, 768), (65, 16, 16, 256, 1024),
          (256 * 33, None, None, 512, 2048)]
_IDS = ["1tile_2d", "6tiles_4d", "260tiles_4d", "264tiles_2d"]
_CACHE = {}


def _close(a, b, rel):
    torch.testing.assert_close(a, b, atol=rel * b.abs().max().item() + 1e-6, rtol=rel)


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.size(1)) if t.dim() == 4 else t


@pytest.fixture
def deep(cuda):
    """The native switch as it was, whatever a test sets."""
    old = ops.conv1x1_tune(4)
    yield cuda
    ops.conv1x1_tune(4, old)


def _under(mode, fn):
    ops.conv1x1_tune(4, mode)
    out = fn()
    torch.cuda.synchronize()
    return out


def _case(shape, dev):
    """Inputs, both arms' results and the references of one shape, computed once and left unchanged."""
    if shape not in _CACHE:
        n, h, w, cin, cout = shape
        old = ops.conv1x1_tune(4)
        torch.manual_seed(cin + cout + n)
        x = torch.randn((n, cin) if h is None else (n, cin, h, w), device=dev).bfloat16()
        if h is not None:
            x = x.contiguous(memory_format=torch.channels_last)
        wt = (torch.randn(cout, cin, 1, 1, device=dev) * cin ** -0.5).bfloat16().contiguous(
            memory_format=torch.channels_last)
        run = lambda: tuple(torch.ops.madnn.conv1x1_fwd(x, wt, True))
        on, on2, off = _under(1, run), _under(1, run), _under(0, run)
        ops.conv1x1_tune(4, old)
        ref64 = _rows(x).double() @ wt.view(cout, cin).double().t()
        _CACHE[shape] = dict(x=x, wt=wt, on=on, on2=on2, off=off, ref64=ref64, M=_rows(x).size(0))
    return _CACHE[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_output_matches_fp32(deep, shape):
    c = _case(shape, deep)
    x, wt = c["x"], c["wt"]
    y = c["on"][0]
    if x.dim() == 4:
        yr = F.conv2d(x.float(), wt.float())
        assert y.shape == yr.shape and y.is_contiguous(memory_format=torch.channels_last)
    else:
        yr = F.conv2d(x.float().t().reshape(1, x.size(1), -1, 1), wt.float()).reshape(wt.size(0), -1).t()
        assert y.shape == yr.shape and y.is_contiguous()
    _close(y.float(), yr, 2e-2)


@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_output_error_matches_k9(deep, shape):
    """Both arms round one fp32 accumulation to bf16: their relative L2 errors against fp64 are bf16's rounding
    error and agree to about three digits (the accumulation-order term is sqrt(K) * 2^-24 against 2^-9)."""
    c = _case(shape, deep)
    ref = c["ref64"]
    e_on = ((_rows(c["on"][0]).double() - ref).norm() / ref.norm()).item()
    e_off = ((_rows(c["off"][0]).double() - ref).norm() / ref.norm()).item()
    same = torch.equal(c["on"][0], c["off"][0])
    print(f"rel L2 vs fp64, shape {shape}: K12P {e_on:.6e}  K9 {e_off:.6e}  outputs bitwise equal: {same}")
    assert abs(e_on - e_off) <= 0.05 * e_off


@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_partial_rows(deep, shape):
    c = _case(shape, deep)
    cout = c["wt"].size(0)
    y, part = c["on"]
    assert part.shape == (c["M"] // 256 * 4, 2, cout) and part.dtype == torch.float32
    yf = _rows(y).double()
    tol = 1e-5 * yf.abs().sum(0).max().item()
    torch.testing.assert_close(part[:, 0].double().sum(0), yf.sum(0), atol=tol, rtol=1e-5)
    torch.testing.assert_close(part[:, 1].double().sum(0), (yf * yf).sum(0), atol=tol, rtol=1e-5)
    # row by row: row r = 4 * (tile row) + wave column holds the sums over output rows 64 r .. 64 r + 63, so a pair
    # written to another row's slot shows.  An fp32 sum of 64 terms is within 64 * 2^-24 = 3.8e-6 of its abs-sum
    # (the squares of bf16 values are exact in fp32): the project's 1e-5 of the largest abs-sum, per 64-row block
    yb = yf.view(-1, 64, cout)
    torch.testing.assert_close(part[:, 0].double(), yb.sum(1), atol=1e-5 * yb.abs().sum(1).max().item(), rtol=1e-5)
    torch.testing.assert_close(part[:, 1].double(), (yb * yb).sum(1), atol=1e-5 * (yb * yb).sum(1).max().item(),
                               rtol=1e-5)
    # fixed order, no atomics: run to run identical
    assert torch.equal(c["on2"][0], y) and torch.equal(c["on2"][1], part)
    # K9's plan writes another number of rows: the switch chose the kernel
    assert c["off"][1].size(0) != part.size(0)


# 8 partial rows, and 1024: from 1024 rows on the consumer folds them in a pass of its own first (bn.hip prereduce)
@pytest.mark.parametrize("shape", [SHAPES[1], (256, 16, 16, 256, 256)], ids=["8rows", "1024rows_prereduce"])
def test_bn_with_deep_statistics_matches_own_pass(deep, shape):
    """BatchNorm fed the K12P epilogue's rows == BatchNorm computing its statistics itself on the same y."""
    c = _case(shape, deep)
    y, part = c["on"]
    assert part.size(0) == c["M"] // 64
    cout = y.size(1)
    torch.manual_seed(2)
    w, b = torch.rand(cout, device=deep) + 0.5, torch.randn(cout, device=deep)
    outs = []
    for st in (part, None):
        rm, rv = torch.zeros(cout, device=deep), torch.ones(cout, device=deep)
        outs.append((ops.batch_norm_act(y, w, b, rm, rv, training=True, relu=True, stats=st), rm, rv))
    (o1, m1, v1), (o2, m2, v2) = outs
    torch.testing.assert_close(o1.float(), o2.float(), atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(m1, m2, atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(v1, v2, atol=1e-5, rtol=1e-4)


def test_ineligible_m_stays_on_k9(deep):
    """M = 256 * 3 + 64 is no multiple of the 256-row tile: the call runs K9 whatever the switch says."""
    torch.manual_seed(4)
    x = torch.randn(256 * 3 + 64, 256, device=deep).bfloat16()
    wt = (torch.randn(512, 256, device=deep) * 256 ** -0.5).bfloat16()
    run = lambda: tuple(torch.ops.madnn.conv1x1_fwd(x, wt, True))
    on, off = _under(1, run), _under(0, run)
    assert on[1].shape == off[1].shape
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])


def test_switch_reaches_the_launcher_and_bottleneck_matches(deep, monkeypatch):
    """``ops.K9_DEEP`` reaches the launcher through the autograd ops; a Bottleneck whose conv3 (256 -> 1024 at
    M = 256) is a deep forward gives, with the switch on and off, outputs and gradients within the tolerances of
    ``test_bf16_bottleneck_k9_matches_miopen_and_fp32``."""
    from madnn.models.resnet import Bottleneck

    torch.manual_seed(3)
    blk = Bottleneck(1024, 256)
    for m in blk.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            torch.nn.init.uniform_(m.weight, 0.5, 1.5)
    ref = Bottleneck(1024, 256)
    ref.load_state_dict(blk.state_dict())
    blk = blk.to(deep).to(memory_format=torch.channels_last)
    for p in blk.parameters():
        if p.dim() == 4:
            p.data = p.data.bfloat16().contiguous(memory_format=torch.channels_last)
    x0 = torch.randn(4, 1024, 8, 8, device=deep).bfloat16().contiguous(memory_format=torch.channels_last)
    g = torch.randn(4, 1024, 8, 8, device=deep)
    assert ops.K9_DEEP, "the deep path is the default"
    res = []
    for flag in (True, False):
        monkeypatch.setattr(ops, "K9_DEEP", flag)
        blk.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y = blk(x)
        y.float().backward(g)
        torch.cuda.synchronize()
        assert ops.conv1x1_tune(4) == (1 if flag else 0)
        res.append((y.float(), x.grad.float(), blk.conv1.weight.grad.float(), blk.conv3.weight.grad.float()))
    names = ("y", "dx", "conv1.dw", "conv3.dw")
    # between the arms: conv3's partial rows are other sums in another order, so bn3's statistics differ in fp32
    # roundings, which a 256-sample BatchNorm backward and the ReLU masks carry into the gradients; the bound is the
    # one that test has against fp32
    between = {k: ((a - b).norm() / b.norm()).item() for k, a, b in zip(names, *res)}
    print("on vs off:", {k: round(v, 5) for k, v in between.items()})
    assert all(v < 0.1 for v in between.values())
    xr = x0.float().cpu().requires_grad_(True)
    yr = ref(xr)
    yr.backward(g.cpu())
    for flag, arm in zip((True, False), res):
        errs = {}
        for k, a, b in zip(names, arm, (yr, xr.grad, ref.conv1.weight.grad, ref.conv3.weight.grad)):
            a = a.cpu().reshape(b.shape)
            errs[k] = ((a - b).norm() / b.norm()).item()
        print("switch", flag, "vs fp32:", {k: round(v, 5) for k, v in errs.items()})
        assert all(v < 0.1 for v in errs.values())  # bf16 activations vs fp32


@pytest.mark.parametrize("n,hw", [(2, 16), (260, 16)], ids=["2tiles", "260tiles"])
def test_plain_dgrad_on_k12p_matches(deep, n, hw):
    """The deep plain data grad (256 -> 512: no residual, no BN sums) runs K12P's plain kernel under the same
    switch: against fp32 with the tolerance of ``test_conv1x1_three_passes_match_fp32``, against K9 by the error
    to fp64 as the forward, and run to run bitwise."""
    torch.manual_seed(n)
    cin, cout = 256, 512
    dy = torch.randn(n, cout, hw, hw, device=deep).bfloat16().contiguous(memory_format=torch.channels_last)
    wt = (torch.randn(cout, cin, 1, 1, device=deep) * cout ** -0.5).bfloat16().contiguous(
        memory_format=torch.channels_last)
    run = lambda: torch.ops.madnn.conv1x1_dgrad(dy, wt, None, None)
    on, on2, off = _under(1, run), _under(1, run), _under(0, run)
    assert on.shape == (n, cin, hw, hw) and on.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(on, on2)
    ref = _rows(dy).double() @ wt.view(cout, cin).double()
    _close(_rows(on).float(), ref.float(), 2e-2)
    e_on = ((_rows(on).double() - ref).norm() / ref.norm()).item()
    e_off = ((_rows(off).double() - ref).norm() / ref.norm()).item()
    print(f"dgrad rel L2 vs fp64, M {n * hw * hw}: K12P {e_on:.6e}  K9 {e_off:.6e}")
    assert abs(e_on - e_off) <= 0.05 * e_off
