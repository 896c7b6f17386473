"""K9F: one backward kernel for bn3's apply and conv3's data + weight gradients in ResNet identity
bottlenecks (``ops.bn2_conv3_bn3_add_relu``), against fp32 eager autograd and against the unfused path
(``MADNN_BN3_CONV3_FUSED=0``: K5 apply + K9 data grad + routed weight grad) on the same inputs.

Both paths round dy3 to bf16 at the same point and accumulate in fp32, so only summation order differs:
the fused path's relative error against fp32 may be at most 1.5x the unfused path's.  Every test prints
the measured errors (``pytest -s``).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import madnn.ops as ops
from madnn.nn.norm import FusedBatchNorm2d

pytestmark = pytest.mark.gpu

GRADS = ("y2", "w3", "bn2.weight", "bn2.bias", "bn3.weight", "bn3.bias", "idt")
# bitwise equal between the two paths: same kernels (forward, bn3's reduction + finalize), same inputs
BITWISE = ("out", "bn2.running_mean", "bn2.running_var", "bn3.running_mean", "bn3.running_var", "bn3.weight",
           "bn3.bias", "idt", "idt_raw", "idt_mask")


def _nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


class _Tap(torch.autograd.Function):
    """Identity that records the gradient tensor it receives and the ReLU bit mask attached to it, the way
    conv1's data grad receives the identity path's gradient in a Bottleneck."""

    @staticmethod
    def forward(ctx, x, box):
        ctx.box = box
        return x.clone()  # not view_as: at batch 1 a view changes the batch stride, and bn3 wants idt's strides = y3's

    @staticmethod
    def backward(ctx, g):
        mask = ops._attached(g, "_madnn_resmask", strict=True)
        ctx.box["raw"] = g.detach().clone()
        ctx.box["mask"] = None if mask is None else mask.clone()
        return (g if mask is None else ops._apply_bit_mask(g, mask)), None


def _make(shape, dev, zero_bn3=False, seed=0):
    n, c, c4, h, w = shape
    g = torch.Generator(device=dev).manual_seed(100 + seed)

    def rnd(*s):
        return torch.randn(*s, device=dev, generator=g)

    d = {
        "y2": _nhwc((rnd(n, c, h, w) * 1.2 + 0.2).bfloat16()),
        "idt": _nhwc(rnd(n, c4, h, w).bfloat16()),
        "w3": _nhwc((rnd(c4, c, 1, 1) * c ** -0.5).bfloat16()),
        "gout": _nhwc(rnd(n, c4, h, w).bfloat16()),
        # random affine parameters: bn3's backward constant term cc is non-zero
        "bn2": {"weight": torch.rand(c, device=dev, generator=g) * 2 - 0.5, "bias": rnd(c) * 0.2},
        "bn3": {"weight": torch.zeros(c4, device=dev) if zero_bn3 else torch.rand(c4, device=dev, generator=g) + 0.5,
                "bias": rnd(c4) * 0.2},
    }
    return d


def _bn(cls, c, state, dev):
    m = cls(c).to(dev)
    with torch.no_grad():
        m.weight.copy_(state["weight"])
        m.bias.copy_(state["bias"])
    return m


def _run(d, shape, dev, fused, monkeypatch):
    n, c, c4, h, w = shape
    monkeypatch.setattr(ops, "_BN3_CONV3_FUSED", fused)
    bn2, bn3 = _bn(FusedBatchNorm2d, c, d["bn2"], dev), _bn(FusedBatchNorm2d, c4, d["bn3"], dev)
    y2 = d["y2"].clone().requires_grad_(True)
    w3 = d["w3"].clone().requires_grad_(True)
    x = d["idt"].clone().requires_grad_(True)
    box = {}
    idt = _Tap.apply(x, box)
    idt._madnn_defer_mask = True
    assert idt.stride() == x.stride()
    assert ops.bn2_conv3_bn3_supported(y2, bn2, w3, bn3, idt) == fused
    if fused:
        out = ops.bn2_conv3_bn3_add_relu(y2, bn2, w3, bn3, idt)
    else:
        assert ops.bn_relu_conv1x1_epi_supported(y2, bn2, w3)
        y3, st = ops.bn_relu_conv1x1(y2, bn2, w3, stats=True)
        out = bn3(y3, residual=idt, relu=True, stats=st)
    out.backward(d["gout"])
    torch.cuda.synchronize()
    r = {"out": out.detach(), "y2": y2.grad, "w3": w3.grad, "idt": x.grad, "idt_raw": box["raw"],
         "idt_mask": box["mask"]}
    for name, m in (("bn2", bn2), ("bn3", bn3)):
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
    """fp32 eager autograd; ``emulate_bf16``: the same with the kernels' four bf16 storage points (a2 and y3
    forward, dy3 and da2 backward) -- its distance from the fp32 result is what bf16 storage alone costs."""
    n, c, c4, h, w = shape
    bn2, bn3 = _bn(torch.nn.BatchNorm2d, c, d["bn2"], dev), _bn(torch.nn.BatchNorm2d, c4, d["bn3"], dev)
    y2 = d["y2"].float().requires_grad_(True)
    w3 = d["w3"].float().requires_grad_(True)
    idt = d["idt"].float().requires_grad_(True)
    rnd = _RoundBoth.apply if emulate_bf16 else (lambda t: t)
    out = torch.relu(bn3(rnd(F.conv2d(rnd(torch.relu(bn2(y2))), w3))) + idt)
    out.backward(d["gout"].float())
    return {"out": out.detach(), "y2": y2.grad, "w3": w3.grad, "idt": idt.grad, "bn2.weight": bn2.weight.grad,
            "bn2.bias": bn2.bias.grad, "bn3.weight": bn3.weight.grad, "bn3.bias": bn3.bias.grad}


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
    assert fus["idt_mask"] is not None and unf["idt_mask"] is not None
    for k in BITWISE:
        assert torch.equal(fus[k], unf[k]), f"{k}: fused and unfused paths differ"
    for k in fus:
        assert torch.equal(fus[k], again[k]), f"{k}: two runs of the fused path differ"
    for k in GRADS:
        assert torch.isfinite(fus[k].float()).all(), k
        ef, eu, fu, ee = _rel(fus[k], ref[k]), _rel(unf[k], ref[k]), _rel(fus[k], unf[k]), _rel(emu[k], ref[k])
        print(f"K9F {shape} zero_bn3={zero_bn3} {k}: fused-vs-fp32 {ef:.3e} unfused-vs-fp32 {eu:.3e} "
              f"fused-vs-unfused {fu:.3e} bf16-storage-emulation-vs-fp32 {ee:.3e}")
        assert ef <= 1.5 * eu, (k, ef, eu)
        # and on an absolute scale: the eager emulation rounds at the kernels' four bf16 storage points; the
        # kernels round once more on top (the stored gradient itself: dy2, dW3 in bf16), so twice its error
        assert ef <= 2.0 * ee, (k, ef, ee)
    return d, fus


@pytest.mark.parametrize("shape", [(2, 64, 256, 9, 9), (1, 64, 256, 5, 7)])
def test_fused_matches_fp32_and_unfused(cuda, monkeypatch, shape):
    """M = 162 (a ragged tail in both tile sizes) and M = 35 (less than one tile)."""
    _check(shape, cuda, monkeypatch)


def test_fused_many_tiles_per_workgroup(cuda, monkeypatch):
    """M = 3136 = 24.5 tiles on 3 workgroups: each walks 8-9 tiles and carries dW3 across them."""
    tune = ctypes.CDLL(str(ops.kernels_path())).madnn_conv1x1_tune
    old = tune(0, 3)
    try:
        _check((4, 64, 256, 28, 28), cuda, monkeypatch, seed=1)
    finally:
        tune(0, old)
    assert tune(0, -1) == old


def test_fused_zero_bn3_weight(cuda, monkeypatch):
    """bn3.weight = 0 (zero_init_residual): every gradient finite, dW3 and conv3's input gradient exactly 0."""
    shape = (2, 64, 256, 9, 9)
    d, fus = _check(shape, cuda, monkeypatch, zero_bn3=True, seed=2)
    assert torch.count_nonzero(fus["w3"]) == 0 and torch.count_nonzero(fus["y2"]) == 0
    # da2 itself, from the kernel: the forward's saved tensors rebuilt with the same ops
    n, c, c4, h, w = shape
    bn2, bn3 = _bn(FusedBatchNorm2d, c, d["bn2"], cuda), _bn(FusedBatchNorm2d, c4, d["bn3"], cuda)
    a2, _, _, sc2, sh2, _ = torch.ops.madnn.bn_fwd(d["y2"], None, bn2.weight, bn2.bias, bn2.running_mean,
                                                   bn2.running_var, bn2.num_batches_tracked, True, 0.1, 1e-5, True,
                                                   None)
    y3, part = torch.ops.madnn.conv1x1_fwd(a2, d["w3"], True)
    _, mean3, inv3, sc3, sh3, mask = torch.ops.madnn.bn_fwd(y3, d["idt"], bn3.weight, bn3.bias, bn3.running_mean,
                                                            bn3.running_var, bn3.num_batches_tracked, True, 0.1,
                                                            1e-5, True, part)
    coef, _, _ = torch.ops.madnn.bn_bwd_coef(d["gout"], y3, mask, bn3.weight, mean3, inv3, sc3, sh3)
    da2, part2, dw3 = torch.ops.madnn.bn3_conv3_bwd(d["gout"], y3, mask, coef, d["w3"], a2, d["y2"], sc2, sh2, False)
    assert dw3.dtype == torch.float32
    assert torch.count_nonzero(da2) == 0 and torch.count_nonzero(dw3) == 0 and torch.count_nonzero(part2) == 0


def _bf16_block(dev, seed):
    from madnn.models.resnet import Bottleneck

    torch.manual_seed(seed)
    blk = Bottleneck(256, 64)
    for m in blk.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            torch.nn.init.uniform_(m.weight, 0.5, 1.5)
            torch.nn.init.normal_(m.bias, 0, 0.2)
    blk = blk.to(dev).to(memory_format=torch.channels_last)
    for p in blk.parameters():
        if p.dim() == 4:
            p.data = _nhwc(p.data.bfloat16())
    return blk


def test_bottleneck_block_knob_on_vs_off(cuda, monkeypatch):
    """One Bottleneck(256, 64): the routed block with the knob on against the knob off.  Output, bn3's
    gradients bitwise; the others to the 1.5x rule's scale (summation order only: 1e-2 in norm)."""
    g = torch.Generator(device=cuda).manual_seed(5)
    x0 = _nhwc(torch.randn(3, 256, 12, 12, device=cuda, generator=g).bfloat16())
    gout = _nhwc(torch.randn(3, 256, 12, 12, device=cuda, generator=g).bfloat16())
    res = []
    for fused in (True, False):
        monkeypatch.setattr(ops, "_BN3_CONV3_FUSED", fused)
        blk = _bf16_block(cuda, 7)
        x = x0.clone().requires_grad_(True)
        y = blk(x)
        assert ("BN2Conv3BN3" in type(y.grad_fn).__name__) == fused
        y.backward(gout)
        res.append({"out": y.detach(), "x": x.grad, **{k: p.grad for k, p in blk.named_parameters()}})
    for k in ("out", "bn3.weight", "bn3.bias"):
        assert torch.equal(res[0][k], res[1][k]), k
    for k in res[0]:
        e = _rel(res[0][k], res[1][k])
        print(f"K9F Bottleneck(256, 64) {k}: fused-vs-unfused {e:.3e}")
        assert e < 1e-2, (k, e)


def test_resnet50_two_steps_knob_on_vs_off(cuda, monkeypatch):
    """Two training steps of resnet50 at batch 4, 64x64: the losses agree to 4 bf16 ulps (2^-6 relative:
    activations and the weights the second loss is computed from are bf16)."""
    import madnn
    from madnn.models import resnet50
    from madnn.optim import FusedSGD

    losses = []
    for fused in (True, False):
        monkeypatch.setattr(ops, "_BN3_CONV3_FUSED", fused)
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
    print(f"K9F resnet50 losses fused {losses[0]} unfused {losses[1]}")
    for a, b in zip(*losses):
        assert a == a and abs(a - b) <= 2.0 ** -6 * abs(b), losses
