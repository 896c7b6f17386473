"""K9F on the layer-1 downsample bottleneck (``ops.bn2_conv3_bn3_add_bn_relu``): the fused backward kernel once
for conv3 (with bn2's sums) and once for the downsample convolution (plain data grad), behind the dual
BatchNorm reduction, against fp32 eager autograd and against the unfused path (``_BN3_CONV3_DUAL = False``: the
dual apply pass + two K9 data grads + two routed weight grads) on the same inputs.

The rules are those of ``test_bn3_conv3_fused_gpu.py``: both paths round dy3 / dyd to bf16 at the same point and
accumulate in fp32, so only summation order differs -- the fused path's relative error against fp32 may be at
most 1.5x the unfused path's, and at most 2x that of an eager emulation of the bf16 storage points (a2, y3, yd
forward; dy3, dyd, da2 backward).  Two runs of the fused path are bitwise equal.  Every test prints the
measured errors (``pytest -s``).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import madnn.ops as ops
from madnn.nn.norm import FusedBatchNorm2d

pytestmark = pytest.mark.gpu

BNS = ("bn2", "bn3", "bn_ds")
GRADS = ("y2", "xf", "w3", "w_ds") + tuple(f"{b}.{p}" for b in BNS for p in ("weight", "bias"))
# bitwise equal between the two paths: same kernels (forward, the dual reduction + its finalizes), same inputs
BITWISE = ("out",) + tuple(f"{b}.{p}" for b in BNS for p in ("running_mean", "running_var")) + (
    "bn3.weight", "bn3.bias", "bn_ds.weight", "bn_ds.bias")


def _nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def _make(shape, dev, zero_bn3=False, seed=0):
    n, c, c4, h, w = shape
    g = torch.Generator(device=dev).manual_seed(200 + seed)

    def rnd(*s):
        return torch.randn(*s, device=dev, generator=g)

    def affine(k, zero=False):
        # random affine parameters: the backward constant term cc is non-zero
        return {"weight": torch.zeros(k, device=dev) if zero else torch.rand(k, device=dev, generator=g) + 0.5,
                "bias": rnd(k) * 0.2}

    return {
        "y2": _nhwc((rnd(n, c, h, w) * 1.2 + 0.2).bfloat16()),
        "xf": _nhwc((rnd(n, c, h, w) + 0.1).bfloat16()),
        "w3": _nhwc((rnd(c4, c, 1, 1) * c ** -0.5).bfloat16()),
        "w_ds": _nhwc((rnd(c4, c, 1, 1) * c ** -0.5).bfloat16()),
        "gout": _nhwc(rnd(n, c4, h, w).bfloat16()),
        "bn2": {"weight": torch.rand(c, device=dev, generator=g) * 2 - 0.5, "bias": rnd(c) * 0.2},
        "bn3": affine(c4, zero_bn3),
        "bn_ds": affine(c4),
    }


def _bn(cls, c, state, dev):
    m = cls(c).to(dev)
    with torch.no_grad():
        m.weight.copy_(state["weight"])
        m.bias.copy_(state["bias"])
    return m


def _run(d, shape, dev, fused, monkeypatch):
    n, c, c4, h, w = shape
    monkeypatch.setattr(ops, "_BN3_CONV3_DUAL", fused)
    bns = {"bn2": _bn(FusedBatchNorm2d, c, d["bn2"], dev), "bn3": _bn(FusedBatchNorm2d, c4, d["bn3"], dev),
           "bn_ds": _bn(FusedBatchNorm2d, c4, d["bn_ds"], dev)}
    bn2, bn3, bn_ds = bns["bn2"], bns["bn3"], bns["bn_ds"]
    leaves = {k: d[k].clone().requires_grad_(True) for k in ("y2", "xf", "w3", "w_ds")}
    y2, xf, w3, w_ds = (leaves[k] for k in ("y2", "xf", "w3", "w_ds"))
    assert ops.bn2_conv3_bn3_add_bn_relu_supported(y2, bn2, w3, bn3, xf, w_ds, bn_ds) == fused
    if fused:
        out = ops.bn2_conv3_bn3_add_bn_relu(y2, bn2, w3, bn3, xf, w_ds, bn_ds)
        assert "BN2Conv3BN3Dual" in type(out.grad_fn).__name__
    else:
        assert ops.bn_relu_conv1x1_epi_supported(y2, bn2, w3) and ops.conv1x1_supported(xf, w_ds)
        yd, std = ops.conv1x1(xf, w_ds, stats=True)
        y3, st = ops.bn_relu_conv1x1(y2, bn2, w3, stats=True)
        assert ops.batch_norm_dual_supported(y3, yd, bn3, bn_ds)
        out = ops.batch_norm_add_bn_relu(y3, yd, bn3, bn_ds, st, std)
    out.backward(d["gout"])
    torch.cuda.synchronize()
    r = {"out": out.detach(), **{k: v.grad for k, v in leaves.items()}}
    for name, m in bns.items():
        r[f"{name}.weight"], r[f"{name}.bias"] = m.weight.grad, m.bias.grad
        r[f"{name}.running_mean"], r[f"{name}.running_var"] = m.running_mean.clone(), m.running_var.clone()
    return r


class _RoundBoth(torch.autograd.Function):
    """Round to bf16 forward and backward: a tensor that the kernels store in bf16 in both directions."""

    @staticmethod
    def forward(ctx, x):
        return x.bfloat16().float()

    @staticmethod
    def backward(ctx, g):
        return g.bfloat16().float()


def _reference(d, shape, dev, emulate_bf16=False):
    """fp32 eager autograd; ``emulate_bf16``: the same with the kernels' six bf16 storage points (a2, y3 and yd
    forward; dy3, dyd and da2 backward) -- its distance from the fp32 result is what bf16 storage alone costs."""
    n, c, c4, h, w = shape
    bns = {"bn2": _bn(torch.nn.BatchNorm2d, c, d["bn2"], dev), "bn3": _bn(torch.nn.BatchNorm2d, c4, d["bn3"], dev),
           "bn_ds": _bn(torch.nn.BatchNorm2d, c4, d["bn_ds"], dev)}
    leaves = {k: d[k].float().requires_grad_(True) for k in ("y2", "xf", "w3", "w_ds")}
    rnd = _RoundBoth.apply if emulate_bf16 else (lambda t: t)
    y3 = rnd(F.conv2d(rnd(torch.relu(bns["bn2"](leaves["y2"]))), leaves["w3"]))
    yd = rnd(F.conv2d(leaves["xf"], leaves["w_ds"]))
    out = torch.relu(bns["bn3"](y3) + bns["bn_ds"](yd))
    out.backward(d["gout"].float())
    r = {"out": out.detach(), **{k: v.grad for k, v in leaves.items()}}
    for name, m in bns.items():
        r[f"{name}.weight"], r[f"{name}.bias"] = m.weight.grad, m.bias.grad
    return r


def _rel(a, ref):
    den = ref.float().norm().item()
    num = (a.float() - ref.float()).norm().item()
    return num if den == 0.0 else num / den


def _check(shape, dev, monkeypatch, zero_bn3=False, seed=0):
    d = _make(shape, dev, zero_bn3, seed)
    ref, emu = _reference(d, shape, dev), _reference(d, shape, dev, emulate_bf16=True)
    unf = _run(d, shape, dev, False, monkeypatch)
    fus = _run(d, shape, dev, True, monkeypatch)
    again = _run(d, shape, dev, True, monkeypatch)
    for k in BITWISE:
        assert torch.equal(fus[k], unf[k]), f"{k}: fused and unfused paths differ"
    for k in fus:
        assert torch.equal(fus[k], again[k]), f"{k}: two runs of the fused path differ"
    for k in GRADS:
        assert torch.isfinite(fus[k].float()).all(), k
        ef, eu, fu, ee = _rel(fus[k], ref[k]), _rel(unf[k], ref[k]), _rel(fus[k], unf[k]), _rel(emu[k], ref[k])
        print(f"K9F dual {shape} zero_bn3={zero_bn3} {k}: fused-vs-fp32 {ef:.3e} unfused-vs-fp32 {eu:.3e} "
              f"fused-vs-unfused {fu:.3e} bf16-storage-emulation-vs-fp32 {ee:.3e}")
        assert ef <= 1.5 * eu, (k, ef, eu)
        # and on an absolute scale: the eager emulation rounds at the kernels' six bf16 storage points; the
        # kernels round once more on top (the stored gradient itself: dy2, dxf, dW in bf16), so twice its error
        assert ef <= 2.0 * ee, (k, ef, ee)
    return d, fus


@pytest.mark.parametrize("shape", [(1, 64, 256, 5, 7), (2, 64, 256, 9, 9)])
def test_dual_fused_matches_fp32_and_unfused(cuda, monkeypatch, shape):
    """M = 35 (less than one 128-row tile) and M = 162 (a ragged second tile)."""
    _check(shape, cuda, monkeypatch)


def test_dual_fused_many_tiles_per_workgroup(cuda, monkeypatch):
    """M = 3136 = 24.5 tiles on 3 workgroups: each walks 8-9 tiles carrying dW, and three slabs are summed."""
    tune = ctypes.CDLL(str(ops.kernels_path())).madnn_conv1x1_tune
    old = tune(0, 3)
    try:
        _check((4, 64, 256, 28, 28), cuda, monkeypatch, seed=1)
    finally:
        tune(0, old)
    assert tune(0, -1) == old


def test_dual_fused_zero_bn3_weight(cuda, monkeypatch):
    """bn3.weight = 0 (zero_init_residual): every gradient finite, dW3 and conv3's input gradient exactly 0, while
    the downsample path's gradients still follow the unfused path (_check's 1.5x rule on w_ds and xf): the two
    launches use their own coefficient sets."""
    d, fus = _check((2, 64, 256, 9, 9), cuda, monkeypatch, zero_bn3=True, seed=2)
    assert torch.count_nonzero(fus["w3"]) == 0 and torch.count_nonzero(fus["y2"]) == 0
    assert torch.count_nonzero(fus["w_ds"]) > 0 and torch.count_nonzero(fus["xf"]) > 0


def _bf16_block(dev, seed):
    from madnn.models.resnet import BN, Bottleneck, conv1x1

    torch.manual_seed(seed)
    blk = Bottleneck(64, 64, downsample=torch.nn.Sequential(conv1x1(64, 256), BN(256)))
    for m in blk.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            torch.nn.init.uniform_(m.weight, 0.5, 1.5)
            torch.nn.init.normal_(m.bias, 0, 0.2)
    blk = blk.to(dev).to(memory_format=torch.channels_last)
    for p in blk.parameters():
        if p.dim() == 4:
            p.data = _nhwc(p.data.bfloat16())
    return blk


def test_downsample_block_knob_on_vs_off(cuda, monkeypatch):
    """One Bottleneck(64, 64) with a stride-1 64 -> 256 downsample: the routed block with the knob on against
    the knob off.  Output and the bn3 / downsample-BN gradients bitwise; the others to the 1.5x rule's scale
    (summation order only: 1e-2 in norm)."""
    g = torch.Generator(device=cuda).manual_seed(5)
    x0 = _nhwc(torch.randn(3, 64, 12, 12, device=cuda, generator=g).bfloat16())
    gout = _nhwc(torch.randn(3, 256, 12, 12, device=cuda, generator=g).bfloat16())
    res = []
    for fused in (True, False):
        monkeypatch.setattr(ops, "_BN3_CONV3_DUAL", fused)
        blk = _bf16_block(cuda, 7)
        x = x0.clone().requires_grad_(True)
        y = blk(x)
        name = type(y.grad_fn).__name__
        assert ("BN2Conv3BN3Dual" in name) == fused, name
        if not fused:
            assert "BNDual" in name, name
        y.backward(gout)
        res.append({"out": y.detach(), "x": x.grad, **{k: p.grad for k, p in blk.named_parameters()}})
    for k in ("out", "bn3.weight", "bn3.bias", "downsample.1.weight", "downsample.1.bias"):
        assert torch.equal(res[0][k], res[1][k]), k
    for k in res[0]:
        e = _rel(res[0][k], res[1][k])
        print(f"K9F dual Bottleneck(64, 64, downsample) {k}: fused-vs-unfused {e:.3e}")
        assert e < 1e-2, (k, e)


def test_resnet50_two_steps_dual_knob_on_vs_off(cuda, monkeypatch):
    """Two training steps of resnet50 at batch 4, 64x64: the losses agree to 4 bf16 ulps (2^-6 relative:
    activations and the weights the second loss is computed from are bf16)."""
    import madnn
    from madnn.models import resnet50
    from madnn.optim import FusedSGD

    losses = []
    for fused in (True, False):
        monkeypatch.setattr(ops, "_BN3_CONV3_DUAL", fused)
        torch.manual_seed(0)
        model = resnet50(num_classes=100)
        opt = FusedSGD(model.parameters(), lr=0.05, momentum=0.9)
        dmodel, opt = madnn.distribute(model, opt, strategy="dp")
        x, y = madnn.data.synthetic_batch("image", 4, cuda, channels_last=True, num_classes=100, shape=(3, 64, 64))
        run = []
        for _ in range(2):
            loss = F.cross_entropy(dmodel(x).float(), y)
            loss.backward()
            opt.step()
            run.append(float(loss.detach()))
        losses.append(run)
    print(f"K9F dual resnet50 losses fused {losses[0]} unfused {losses[1]}")
    for a, b in zip(*losses):
        assert a == a and abs(a - b) <= 2.0 ** -6 * abs(b), losses
