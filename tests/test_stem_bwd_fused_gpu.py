"""The ResNet stem as one autograd node (``ops.stem_bn_relu_maxpool``): the pool forward's ``yarg``, the
pooled-domain BN backward reduction and the stem weight grad that forms ``dy = ca g + cb y + cc`` on chip.

Image shapes ``(N, H, W)`` -> stem output -> pooled, each for one way the weight-grad kernel can go wrong:
``(1, 7, 8)`` the smallest supported (4x4 -> 2x2); ``(2, 64, 64)`` plain and even; ``(3, 50, 48)`` stem height 25
and pooled height 13 odd (the last stem row has one pooled neighbour); ``(5, 18, 40)`` ``Wo = 20``, not a multiple
of the 16-pixel MFMA step (padded tile columns stay zero); ``(40, 32, 32)`` 640 rows on at most 512 workgroups (2
rows each); ``(70, 30, 32)`` 3 rows per workgroup with ``Ho = 15``: ranges cross image boundaries at odd offsets
(ring refill, no pooled row carried across images).
"""
import pytest
import torch
import torch.nn.functional as F
from torch.utils._python_dispatch import TorchDispatchMode

import madnn.models.resnet as resnet
import madnn.ops as ops
from madnn.nn.conv import FusedConv2d
from madnn.nn.norm import FusedBatchNorm2d, FusedMaxPool2d

pytestmark = pytest.mark.gpu

SHAPES = [(1, 7, 8), (2, 64, 64), (3, 50, 48), (5, 18, 40), (40, 32, 32), (70, 30, 32)]
MASKED = (3, 17, 40)   # channels whose bn1 bias (-5) masks every element: their windows must contribute nothing
FUSED_OPS = ("madnn::pool_bn_fwd_yarg", "madnn::pool_bn_bwd_coef", "madnn::stem_wgrad_bnp")
OLD_OPS = ("madnn::pool_bn_fwd", "madnn::pool_bn_bwd", "madnn::stem_wgrad")


def _rel(a, ref):
    den = ref.float().norm().item()
    num = (a.float() - ref.float()).norm().item()
    return num if den == 0.0 else num / den


def _modules(dev, seed=0):
    torch.manual_seed(seed)
    conv = FusedConv2d(3, 64, 7, stride=2, padding=3, bias=False).to(dev).bfloat16()
    bn = FusedBatchNorm2d(64).to(dev)
    with torch.no_grad():
        bn.weight.uniform_(-0.5, 1.5)   # negative scales too: max of the affine is not the affine of the max
        bn.bias.normal_(0, 0.3)
        bn.bias[list(MASKED)] = -5.0
        bn.weight[list(MASKED)] = 0.5
    return conv.train(), bn.train(), FusedMaxPool2d(3, stride=2, padding=1)


def _img(shape, dev, seed=1):
    n, h, w = shape
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(n, 3, h, w, generator=g).to(dev).bfloat16().contiguous(memory_format=torch.channels_last)


_CACHE = {}


def _case(shape, dev):
    """Per shape, computed once and left unchanged: x, the stem output y, bn1's forward vectors, both pool forwards,
    a pool output gradient dp."""
    if shape in _CACHE:
        return _CACHE[shape]
    conv, bn, pool = _modules(dev)
    x = _img(shape, dev)
    with torch.no_grad():
        y, part = torch.ops.madnn.stem_fwd(x, ops._stem_pack(conv.weight), True)
        mean, invstd, scale, shift = torch.ops.madnn.bn_coef(y, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                                             bn.num_batches_tracked, 0.1, 1e-5, part)
        out0, arg0 = torch.ops.madnn.pool_bn_fwd(y, scale, shift, 1)
        out1, arg1, yarg = torch.ops.madnn.pool_bn_fwd_yarg(y, scale, shift, 1)
        g = torch.Generator(device="cpu").manual_seed(7)
        dp = torch.randn(out0.shape, generator=g).to(dev).bfloat16().contiguous(memory_format=torch.channels_last)
    c = dict(x=x, w=conv.weight.detach(), bn_w=bn.weight.detach(), y=y, mean=mean, invstd=invstd, scale=scale,
             shift=shift, out0=out0, arg0=arg0, out1=out1, arg1=arg1, yarg=yarg, dp=dp)
    _CACHE[shape] = c
    return c


def _stem_positions(arg, n, hp, wp, p=1):
    """Decoded argmax bytes [N, Hp, Wp, 64] -> stem row / column of every pooled element."""
    q = arg.view(n, hp, wp, 64).long()
    oh = torch.arange(hp, device=arg.device).view(1, hp, 1, 1)
    ow = torch.arange(wp, device=arg.device).view(1, 1, wp, 1)
    return 2 * oh - p + q // 3, 2 * ow - p + q % 3


@pytest.mark.parametrize("shape", SHAPES)
def test_yarg_is_y_at_the_argmax(cuda, shape):
    c = _case(shape, cuda)
    assert torch.equal(c["out0"], c["out1"]) and torch.equal(c["arg0"], c["arg1"])
    y = c["y"].permute(0, 2, 3, 1)                       # NHWC view
    n, ho, wo, _ = y.shape
    hp, wp = c["out0"].shape[2:]
    ih, iw = _stem_positions(c["arg1"], n, hp, wp)
    assert int(ih.min()) >= 0 and int(ih.max()) < ho and int(iw.min()) >= 0 and int(iw.max()) < wo
    ni = torch.arange(n, device=cuda).view(n, 1, 1, 1).expand_as(ih)
    ci = torch.arange(64, device=cuda).view(1, 1, 1, 64).expand_as(ih)
    want = y[ni, ih, iw, ci]
    got = c["yarg"].permute(0, 2, 3, 1)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_wgrad_bnp_one_hot_picks_one_patch(cuda):
    """``test_stem_wgrad_asymmetric`` carried over: ca = 1, cb = cc = 0 and a one-hot dp at one pooled pixel and
    channel give dW[c] = exactly the 7x7x3 input patch at that pixel's argmax position, every other channel zero."""
    x = (torch.arange(1 * 3 * 32 * 32, device=cuda, dtype=torch.float32).reshape(1, 32, 32, 3) % 29 - 14)
    x = x.permute(0, 3, 1, 2).bfloat16().contiguous(memory_format=torch.channels_last)
    y = torch.randn(1, 64, 16, 16, device=cuda).bfloat16().contiguous(memory_format=torch.channels_last)
    scale, shift = torch.zeros(64, device=cuda), torch.ones(64, device=cuda)      # ReLU open everywhere
    coef = torch.stack([torch.ones(64), torch.zeros(64), torch.zeros(64)]).to(cuda).contiguous()
    # window position 5 = (kh 1, kw 2) everywhere: pooled (2, 3) of channel 5 -> stem pixel (2*2 - 1 + 1, 2*3 - 1 + 2)
    arg = torch.full((1 * 8 * 8 * 64,), 5, dtype=torch.uint8, device=cuda)
    dp = torch.zeros(1, 64, 8, 8, device=cuda).bfloat16().contiguous(memory_format=torch.channels_last)
    dp[0, 5, 2, 3] = 1.0
    dw = torch.ops.madnn.stem_wgrad_bnp(x, y, dp, arg, scale, shift, coef, 1)
    xp = F.pad(x.float(), (3, 3, 3, 3))
    sh, sw = 4, 7
    patch = xp[0, :, 2 * sh:2 * sh + 7, 2 * sw:2 * sw + 7]
    torch.testing.assert_close(dw[5], patch, atol=0, rtol=0)
    assert dw[torch.arange(64, device=cuda) != 5].abs().max().item() == 0
    # the same pooled pixel behind a closed ReLU contributes nothing
    dw0 = torch.ops.madnn.stem_wgrad_bnp(x, y, dp, arg, scale, -shift, coef, 1)
    assert dw0.abs().max().item() == 0


def _dy_ref(c, coef):
    """``pool_bn_bwd_kernel<1>``'s dy for coefficients of the test's own, in torch: the pool gradient gathered per
    stem pixel from the up-to-four pooled pixels in the kernel's order, the ReLU mask recomputed from y, the affine
    form rounded to bf16.  fp32 steps are written as both kernels' machine code has them: ``fma(y, scale, shift)`` for
    the mask and ``fma(cb, y, ca*g) + cc`` (hipcc's default contraction; a product of two fp32 is exact in fp64)."""
    y = c["y"].permute(0, 2, 3, 1).float()
    n, ho, wo, _ = y.shape
    hp, wp = c["out0"].shape[2:]
    dp = c["dp"].permute(0, 2, 3, 1).float()
    ih, iw = _stem_positions(c["arg1"], n, hp, wp)
    h = torch.arange(ho, device=y.device).view(1, ho, 1, 1)
    w = torch.arange(wo, device=y.device).view(1, 1, wo, 1)
    g = torch.zeros_like(y)
    for dh in (-1, 0):
        for dw in (-1, 0):
            oh, ow = (h + 1) // 2 + dh, (w + 1) // 2 + dw
            ok = (oh >= 0) & (oh < hp) & (ow >= 0) & (ow < wp)
            ohc, owc = oh.clamp(0, hp - 1).expand(1, ho, wo, 1), ow.clamp(0, wp - 1).expand(1, ho, wo, 1)
            hit = ok & (ih[:, ohc[0, :, :, 0], owc[0, :, :, 0]] == h) & (iw[:, ohc[0, :, :, 0], owc[0, :, :, 0]] == w)
            g = g + torch.where(hit, dp[:, ohc[0, :, :, 0], owc[0, :, :, 0]], torch.zeros_like(y))
    d = torch.float64
    z = (y.to(d) * c["scale"].to(d) + c["shift"].to(d)).float()
    g = torch.where(z > 0, g, torch.zeros_like(g))
    t = coef[0] * g
    o = (coef[1].to(d) * y.to(d) + t.to(d)).float() + coef[2]
    return o.bfloat16().permute(0, 3, 1, 2)              # channels_last [N, 64, Ho, Wo]


@pytest.mark.parametrize("shape", SHAPES)
def test_wgrad_bnp_random_coefficients(cuda, shape):
    """Fused weight grad against ``stem_wgrad(dy_ref, x)`` with coefficients drawn by the test.  Bound: twice the
    relative L2 distance of ``stem_wgrad(dy_ref, x)`` from the fp32 eager weight grad of the same ``dy_ref``.
    Measured relative L2 between fused and unfused on MI355X: 0.0 (bitwise equal) at all six shapes, against
    fp32-eager distances of 2.7e-8 to 2.2e-7."""
    c = _case(shape, cuda)
    g = torch.Generator(device="cpu").manual_seed(3)
    coef = torch.stack([torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1,
                        torch.randn(64, generator=g) * 0.05]).to(cuda).contiguous()
    dy = _dy_ref(c, coef).contiguous(memory_format=torch.channels_last)
    dw_ref = torch.ops.madnn.stem_wgrad(dy, c["x"])
    dw = torch.ops.madnn.stem_wgrad_bnp(c["x"], c["y"], c["dp"], c["arg1"], c["scale"], c["shift"], coef, 1)
    eager = torch.ops.aten.convolution_backward(dy.float(), c["x"].float(), c["w"].float(), None, (2, 2), (3, 3),
                                                (1, 1), False, (0, 0), 1, (False, True, False))[1]
    dist, base = _rel(dw, dw_ref), _rel(dw_ref, eager)
    print(f"stem_wgrad_bnp {shape}: rel L2 fused vs unfused {dist:.3e}, unfused vs fp32 eager {base:.3e}")
    assert dist <= 2.0 * base, (dist, base)


def _run(shape, dev, fused, monkeypatch, x_grad=False):
    """One forward + backward of the stem through the route ``ResNet.stem`` takes -> output, grads, buffers, ops."""
    monkeypatch.setattr(ops, "_STEM_BWD_FUSED", fused)
    net = _StemOnly(*_modules(dev))
    x = _img(shape, dev).requires_grad_(x_grad)
    with _Recorder() as rec:
        out = net.stem(x)
        out.backward(_case(shape, dev)["dp"])
    torch.cuda.synchronize()
    grads = dict(conv=net.conv1.weight.grad, bn_w=net.bn1.weight.grad, bn_b=net.bn1.bias.grad)
    return out.detach(), grads, (net.bn1.running_mean, net.bn1.running_var, net.bn1.num_batches_tracked), rec.names


class _StemOnly(resnet.ResNet):
    def __init__(self, conv, bn, pool):
        torch.nn.Module.__init__(self)
        self.conv1, self.bn1, self.maxpool = conv, bn, pool


class _Recorder(TorchDispatchMode):
    """The operator log of tests/test_resnet_routing_gpu.py."""

    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = func._schema.name
        if name.startswith("madnn::") and not name.endswith("_supported"):
            self.names.append(name)
        return func(*args, **(kwargs or {}))


def _eager(shape, dev):
    conv, bn, _ = _modules(dev)
    ref_bn = torch.nn.BatchNorm2d(64).to(dev)
    ref_bn.load_state_dict(bn.state_dict())
    w = conv.weight.detach().float().requires_grad_(True)
    out = F.max_pool2d(torch.relu(ref_bn(F.conv2d(_img(shape, dev).float(), w, stride=2, padding=3))), 3, 2, 1)
    out.backward(_case(shape, dev)["dp"].float())
    return dict(conv=w.grad, bn_w=ref_bn.weight.grad, bn_b=ref_bn.bias.grad)


@pytest.mark.parametrize("shape", SHAPES)
def test_node_against_unfused_and_fp32_eager(cuda, shape, monkeypatch):
    out_f, gf, buf_f, names_f = _run(shape, cuda, True, monkeypatch)
    out_u, gu, buf_u, names_u = _run(shape, cuda, False, monkeypatch)
    assert all(n in names_f for n in FUSED_OPS) and not any(n in names_f for n in OLD_OPS)
    assert all(n in names_u for n in OLD_OPS) and not any(n in names_u for n in FUSED_OPS)
    assert torch.equal(out_f, out_u)
    for a, b in zip(buf_f, buf_u):
        assert torch.equal(a, b)
    ge = _eager(shape, cuda)
    for k in ("conv", "bn_w", "bn_b"):
        ef, eu = _rel(gf[k], ge[k]), _rel(gu[k], ge[k])
        print(f"stem node {shape} {k}: rel fused {ef:.3e} unfused {eu:.3e}")
        assert ef <= 1.5 * eu + 1e-3, (k, ef, eu)
    # fully masked channels: no gradient reaches bn1's affine, so dy and their filters' gradients are zero
    m = list(MASKED)
    assert gf["bn_w"][m].abs().max().item() == 0 and gf["bn_b"][m].abs().max().item() == 0
    assert gf["conv"][m].abs().max().item() == 0


@pytest.mark.parametrize("shape", [(3, 50, 48), (70, 30, 32)])
def test_node_backward_is_bitwise_repeatable(cuda, shape, monkeypatch):
    _, g1, _, _ = _run(shape, cuda, True, monkeypatch)
    _, g2, _, _ = _run(shape, cuda, True, monkeypatch)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def test_fallbacks_take_the_old_path(cuda, monkeypatch):
    """An image that needs its gradient, and the knob switched off, both run today's two nodes."""
    shape = (2, 64, 64)
    _, g, _, names = _run(shape, cuda, True, monkeypatch, x_grad=True)
    assert all(n in names for n in OLD_OPS) and not any(n in names for n in FUSED_OPS)
    _, g0, _, names0 = _run(shape, cuda, False, monkeypatch)
    assert names0 == [n for n in names]      # the same kernels in the same order
    assert not any(n in names0 for n in FUSED_OPS)
    for k in g:
        assert torch.equal(g[k], g0[k]), k
