"""K9 ring main loop (LDS-DMA operand ring, LDS-resident weight slice) against the register-staged loop it
replaces, on the smallest shapes at which the ring can go wrong.

The ring keeps the MFMA instruction, the ascending k order, the tile-to-workgroup plan and the epilogue's
arithmetic and thread map, so outputs and partial rows are compared bitwise (``torch.equal``) between the values
of the switch; the column sums of the partial rows and the outputs are also compared with fp32 references,
with the tolerances of ``tests/test_conv_gpu.py::test_conv1x1_three_passes_match_fp32``.

K = 64 (one step: shallower than the ring), 128, 192 (the ring's depth), 256, 512 and 576 (one tile per
workgroup); I = 64 (the BI = 64 kernels), 128, 384; M = 45 (one partial tile), 130 (one row into a second tile)
and 641 with the persistent grid target at 2 (every workgroup walks >= 3 tiles, the last one partial).  The ring
takes K <= 128 at I = 128 / 384 and K = 128 .. 256 at I = 64 (forward); the shapes the launcher keeps on the
register-staged loop run it under both values of the switch.  With the ring on, the forward at K = 192 / 256 and
I = 128 / 384 runs 64-wide i tiles (so that its weight slice fits): another tile-to-workgroup plan, hence
another number and summation order of partial rows.  There the output is still bitwise the same (per element
the same MFMA chain) and the partial rows are checked against the fp32 sums instead of bitwise.
"""
import pytest
import torch
import torch.nn.functional as F

from madnn import ops

pytestmark = pytest.mark.gpu

KS = [64, 128, 192, 256, 512, 576]
IS = [64, 128, 384]
# (N, H, W, persistent grid target or None)
MS = [(1, 5, 9, None), (1, 10, 13, None), (1, 641, 1, 2)]
RING_MODES = [1]


def _rand(shape, dev, scale=1.0):
    t = (torch.randn(shape, device=dev) * scale).bfloat16()
    return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t


def _close(a, b, rel):
    torch.testing.assert_close(a, b, atol=rel * b.abs().max().item() + 1e-6, rtol=rel)


def _rows(t):
    return t.double().permute(0, 2, 3, 1).reshape(-1, t.size(1))


def _sums_close(part, s0, s1, scale0, scale1):
    torch.testing.assert_close(part[:, 0].double().sum(0), s0, atol=1e-5 * scale0, rtol=1e-5)
    torch.testing.assert_close(part[:, 1].double().sum(0), s1, atol=1e-5 * scale1, rtol=1e-5)


@pytest.fixture
def k9(cuda):
    """The native switches as they were, whatever a test sets."""
    ring, grid = ops.conv1x1_tune(3), ops.conv1x1_tune(0)
    yield cuda
    ops.conv1x1_tune(3, ring)
    ops.conv1x1_tune(0, grid)


def _under(mode, grid, fn):
    ops.conv1x1_tune(3, mode)
    old = ops.conv1x1_tune(0, grid) if grid is not None else None
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    finally:
        if old is not None:
            ops.conv1x1_tune(0, old)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and torch.equal(x, y)


@pytest.mark.parametrize("i", IS)
@pytest.mark.parametrize("k", KS)
def test_forward_ring_equals_staged(k9, k, i):
    torch.manual_seed(k + i)
    for n, h, w, grid in MS:
        x = _rand((n, k, h, w), k9)
        wt = _rand((i, k, 1, 1), k9, k ** -0.5).contiguous(memory_format=torch.channels_last)
        yr = F.conv2d(x.float(), wt.float())
        for stats in (True, False):
            run = lambda: tuple(torch.ops.madnn.conv1x1_fwd(x, wt, stats))
            staged = _under(0, grid, run)
            y, part = staged
            _close(y.float(), yr, 2e-2)
            if stats:
                yf = _rows(y)
                scale = yf.abs().sum(0).max().item()
                _sums_close(part, yf.sum(0), (yf * yf).sum(0), scale, scale)
                if grid is not None and k < 512:
                    assert part.size(0) <= 2  # the walk: >= 3 tiles per workgroup
            replanned = k in (192, 256) and i % 128 == 0
            for mode in RING_MODES:
                ring = _under(mode, grid, run)
                if replanned:
                    _same(ring[:1], staged[:1])
                    if stats:
                        _sums_close(ring[1], yf.sum(0), (yf * yf).sum(0), scale, scale)
                else:
                    _same(ring, staged)
                _same(_under(mode, grid, run), ring)  # fixed order, no atomics: run to run identical


@pytest.mark.parametrize("i", IS)
@pytest.mark.parametrize("k", KS)
def test_dgrad_ring_equals_staged(k9, k, i):
    torch.manual_seed(1000 + k + i)
    for n, h, w, grid in MS:
        dy = _rand((n, k, h, w), k9)
        wt = _rand((k, i, 1, 1), k9, k ** -0.5).contiguous(memory_format=torch.channels_last)
        res = _rand((n, i, h, w), k9)
        mask = torch.randint(0, 256, (n * h * w * i // 8,), device=k9, dtype=torch.uint8)
        bny = _rand((n, i, h, w), k9)
        # bf16-exact scale / shift: y * sc is exact in fp32, so the ReLU mask has one value however it is evaluated
        sc = (torch.rand(i, device=k9) + 0.5).bfloat16().float()
        sh = (torch.randn(i, device=k9) * 0.2).bfloat16().float()
        dxr = torch.einsum("nkhw,kc->nchw", dy.float(), wt.float().reshape(k, i))
        bits = ((mask.view(-1, 1) >> torch.arange(8, device=k9, dtype=torch.uint8)) & 1).bool().view(-1, i)
        masked = (res.float().permute(0, 2, 3, 1).reshape(-1, i) * bits).view(n, h, w, i).permute(0, 3, 1, 2)
        m = torch.ops.madnn
        forms = {
            "plain": (lambda: (m.conv1x1_dgrad(dy, wt, None, None),), dxr),
            "res": (lambda: (m.conv1x1_dgrad(dy, wt, res, None),), dxr + res.float()),
            "res_mask": (lambda: (m.conv1x1_dgrad(dy, wt, res, mask),), dxr + masked),
            "bnb": (lambda: tuple(m.conv1x1_dgrad_bnb(dy, wt, bny, sc, sh)), dxr),
        }
        for name, (run, ref) in forms.items():
            staged = _under(0, grid, run)
            _close(staged[0].float(), ref, 2e-2)
            if name == "bnb":
                g, yy = _rows(staged[0]), _rows(bny)
                gm = g * (yy * sc.double() + sh.double() > 0)
                _sums_close(staged[1], gm.sum(0), (gm * yy).sum(0), g.abs().sum(0).max().item(),
                            (g * yy).abs().sum(0).max().item())
            for mode in RING_MODES:
                ring = _under(mode, grid, run)
                _same(ring, staged)
                _same(_under(mode, grid, run), ring)


def test_switch_off_runs_the_staged_kernels(k9, monkeypatch):
    """``ops.K9_RING`` reaches the launcher through the autograd ops, and off still computes the same."""
    torch.manual_seed(7)
    x = _rand((2, 128, 9, 9), k9)
    wt = _rand((256, 128, 1, 1), k9, 128 ** -0.5).contiguous(memory_format=torch.channels_last)
    g = _rand((2, 256, 9, 9), k9)

    def step():
        xx = x.clone().requires_grad_(True)
        y, part = ops.conv1x1(xx, wt, stats=True)
        y.backward(g)
        torch.cuda.synchronize()
        return y.detach(), part, xx.grad

    assert ops.K9_RING, "the ring is the default"
    on = step()
    assert ops.conv1x1_tune(3) == 1
    monkeypatch.setattr(ops, "K9_RING", False)
    off = step()
    assert ops.conv1x1_tune(3) == 0
    _same(on, off)
    _close(off[0].float(), F.conv2d(x.float(), wt.float()), 2e-2)
    _close(off[2].float(), torch.einsum("nkhw,kc->nchw", g.float(), wt.float().reshape(256, 128)), 2e-2)
