"""ResNet (v1.5, torchvision layout and parameter names) — in-repo because
torchvision is not installed.  BASELINE config 2:
"ResNet-50 auto data-parallel bf16 on 8xMI355X".

The bottleneck 1x1 convolutions (stride 1) run on madnn's K9 MFMA GEMM kernels,
which also compute the following BatchNorm's batch statistics in their epilogue; the stride-1
3x3 convolutions run on K13 (MFMA implicit GEMM over an LDS-staged input halo, statistics in the
epilogue, data grad on the flipped weight); the stride-2 3x3 on the 14x14 map runs its forward on
K13's stride-2 variant (statistics in the epilogue), the larger stride-2 3x3s on MIOpen / CK through
PyTorch-ROCm (a committed per-shape A/B: profiles/r5_conv3x3_s2_ab.json); the 7x7 stem runs on K10 (MFMA
forward with the BatchNorm statistics in its epilogue, MFMA weight gradient); the stem max-pool is madnn's
NHWC kernel (K7, byte argmax + gather backward); every
BatchNorm is madnn's fused NHWC kernel (K5) with the following ReLU and, at the
end of each block, the residual add folded in: ``relu(bn3(conv3(h)) + idt)`` is
one kernel forward and one backward.  In layer 1 (64 -> 256 channels) the backward of that tail is
K9F: bn3's apply and conv3's data and weight gradients in one kernel, and in the downsample block
the same kernel once more for the downsample BatchNorm and convolution
(``ops.bn2_conv3_bn3_add_relu`` / ``ops.bn2_conv3_bn3_add_bn_relu``).  The network runs channels_last (NHWC) in
bf16 with fp32 BatchNorm parameters — the layout MIOpen's gfx950 implicit-GEMM
convolutions prefer.
"""
from __future__ import annotations

import os
from collections import namedtuple
from typing import List, Type

import torch
from torch import nn

from ..nn.conv import FusedConv2d
from ..nn.norm import FusedBatchNorm2d as BN
from ..nn.norm import FusedGlobalAvgPool2d, FusedMaxPool2d
from ..ops import (batch_norm_add_bn_relu, bn2_conv3_bn3_add_bn_relu, bn2_conv3_bn3_add_bn_relu_supported,
                   bn2_conv3_bn3_add_relu, bn2_conv3_bn3_supported, bn_relu_conv1x1,
                   bn_relu_conv1x1_epi_supported, bn_relu_conv3x3, bn_relu_conv3x3_supported, bn_relu_maxpool,
                   bn_relu_maxpool_supported, conv1x1_route, defer_res_mask, stem_bn_relu_maxpool,
                   stem_bn_relu_maxpool_supported)

# A/B knob: sum the downsample path's input gradient inside conv1's data grad (1) or by autograd (0)
_FORK_DS = os.environ.get("MADNN_FORK_DOWNSAMPLE", "1") != "0"
# A/B knob: the downsample path's BatchNorm runs inside bn3's kernels (1) or as its own passes (0)
_DUAL_BN = os.environ.get("MADNN_DUAL_BN", "1") != "0"
# A/B knob: the stride-2 1x1 downsample convolution as a stride-1 1x1 on conv1's compact subsample
# of the block input (1) or as a stride-2 library convolution on the full input (0)
_DS_SUB = os.environ.get("MADNN_DS_SUB", "1") != "0"


# Bottleneck.forward's routes (Bottleneck._route); each is explained where forward issues it
ROUTES = (IDENTITY_K9F, IDENTITY, DUAL_SUB, DUAL_K9F, DUAL, FORK_DS, PLAIN_DS) = (
    "identity+k9f", "identity", "dual+sub", "dual+k9f", "dual", "fork-ds", "plain-ds")
_Fused = namedtuple("_Fused", "bn1_conv2 bn2_conv3 bn3 dual")


def conv3x3(cin, cout, stride=1, groups=1, dilation=1):
    # stride 1 runs on K13 (forward + BN statistics, data grad); stride 2 on MIOpen
    return FusedConv2d(cin, cout, 3, stride=stride, padding=dilation, groups=groups, bias=False, dilation=dilation)


def conv1x1(cin, cout, stride=1):
    return FusedConv2d(cin, cout, 1, stride=stride, bias=False)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = conv3x3(inplanes, planes, stride)
        self.bn1 = BN(planes)
        self.conv2 = conv3x3(planes, planes)
        self.bn2 = BN(planes)
        self.downsample = downsample

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        y, st = self.conv1(x, stats=True)
        out = self.bn1(y, relu=True, stats=st)
        y, st = self.conv2(out, stats=True)
        return self.bn2(y, residual=idt, relu=True, stats=st)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = conv1x1(inplanes, planes)
        self.bn1 = BN(planes)
        self.conv2 = conv3x3(planes, planes, stride)   # stride on the 3x3 (v1.5)
        self.bn2 = BN(planes)
        self.conv3 = conv1x1(planes, planes * 4)
        self.bn3 = BN(planes * 4)
        self.downsample = downsample

    def forward(self, x):
        fused = self._fused()
        route = self._route(x, fused)
        ds = self.downsample
        # head: conv1 on K9 (BN statistics from the GEMM epilogue) and what joins the tail from the side
        if route in (IDENTITY_K9F, IDENTITY):
            # the identity path's gradient is added inside conv1's data-grad kernel (no separate
            # residual-gradient add)
            y, st, side = self.conv1(x, stats=True, fork=True)
            if route == IDENTITY_K9F:
                # idt's only consumer is bn3 and its gradient is summed inside K9's data grad: that
                # kernel applies bn3's ReLU mask itself (ops._BNFn deferred mask)
                defer_res_mask(side)
        elif route == PLAIN_DS:
            side = ds(x)
            y, st = self.conv1(x, stats=True)
        else:
            # the downsample path's input gradient is likewise summed inside conv1's data grad.
            # DUAL_SUB: conv1 hands over the compact x[:, :, ::2, ::2] and the stride-2 downsample
            # runs as a stride-1 1x1 on it (K9, BN statistics from its epilogue); its compact
            # input gradient is added into conv1's data grad at the even pixels
            y, st, xf = self.conv1(x, stats=True, fork=2 if route == DUAL_SUB else True)
            if route == DUAL_K9F and not self._k9f_dual(y, xf):
                route = DUAL
            if route == FORK_DS:
                side = ds(xf)
            elif route == DUAL_SUB:
                side = ds[0].forward_subsampled(xf, stats=True)
            elif route == DUAL:
                side = ds[0](xf, stats=True)
        y1 = y   # DUAL_K9F was confirmed on conv1's output
        y, st = self._bn1_conv2(y, st, fused)   # K13 at stride 1: BN statistics from the epilogue
        # tail: conv3, bn3 and the residual add
        if route == IDENTITY_K9F and fused.bn2_conv3 and isinstance(y, torch.Tensor) and self.conv3._k9(y) \
                and bn2_conv3_bn3_supported(y, self.bn2, self.conv3.weight, self.bn3, side):
            # layer 1's identity blocks: one backward kernel for bn3's apply and conv3's two gradients (K9F)
            return bn2_conv3_bn3_add_relu(y, self.bn2, self.conv3.weight, self.bn3, side, stats_in=st)
        if route == DUAL_K9F:
            # layer 1's downsample block: K9F once per convolution; the downsample convolution is
            # issued inside the function, and neither dy3 nor dyd is written in the backward
            if isinstance(y, torch.Tensor) and y.requires_grad \
                    and (y.shape, y.stride(), y.dtype) == (y1.shape, y1.stride(), y1.dtype):   # conv2 kept these
                return bn2_conv3_bn3_add_bn_relu(y, self.bn2, self.conv3.weight, self.bn3, xf, ds[0].weight,
                                                 ds[1], stats_in=st)
            route, side = DUAL, ds[0](xf, stats=True)
        y, st = self._bn2_conv3(y, st, fused)
        if route in (DUAL_SUB, DUAL):
            # relu(bn3(conv3) + bn_ds(conv_ds)): the downsample BN is applied inside bn3's
            # passes (forward and backward), its normalised output never written to HBM
            return batch_norm_add_bn_relu(y, side[0], self.bn3, ds[1], st, side[1])
        return self.bn3(y, residual=side, relu=True, stats=st)   # relu(bn3 + idt): one kernel

    def _fused(self) -> "_Fused":
        """Which of the block's own modules are the fused kinds (a model surgery may have swapped some)."""
        ds = self.downsample
        return _Fused(bn1_conv2=isinstance(self.bn1, BN) and isinstance(self.conv2, FusedConv2d),
                      bn2_conv3=isinstance(self.bn2, BN) and isinstance(self.conv3, FusedConv2d),
                      bn3=isinstance(self.bn3, BN),
                      dual=(isinstance(ds, nn.Sequential) and len(ds) == 2 and isinstance(ds[0], FusedConv2d)
                            and isinstance(ds[1], BN) and isinstance(self.bn3, BN)))

    def _dual_bn(self) -> bool:
        return _DUAL_BN and self._fused().dual

    def _route(self, x, fused: "_Fused") -> str:
        """Which of ROUTES this block takes for ``x``, decided before any kernel is issued.  A K9F route is
        confirmed once the tensors its node takes exist (IDENTITY_K9F after conv2, DUAL_K9F after conv1,
        :meth:`_k9f_dual`) and continues as IDENTITY (the ReLU mask still deferred) / DUAL otherwise."""
        ds, tensor = self.downsample, isinstance(x, torch.Tensor)
        if ds is None:
            defer = (tensor and fused.bn3 and self.conv1._k9(x)
                     and conv1x1_route(x.size(1), self.conv1.weight.size(0))[1] == "k9")
            return IDENTITY_K9F if defer else IDENTITY
        if not _FORK_DS:
            return PLAIN_DS
        if not (_DUAL_BN and fused.dual):
            return FORK_DS
        if _DS_SUB and tensor and ds[0].subsampled_ok():
            return DUAL_SUB
        return DUAL_K9F if tensor and fused.bn2_conv3 and self.conv2.stride == (1, 1) else DUAL

    def _bn1_conv2(self, y, st, fused):
        """conv2(relu(bn1(y))): with conv2 on K13, bn1's backward reduction is taken in conv2's
        data-grad epilogue (ops.bn_relu_conv3x3); the stride-2 conv2s take the module path (K13's stride-2
        forward on small maps, the library otherwise)."""
        if fused.bn1_conv2 and isinstance(y, torch.Tensor) and self.conv2._k13(y) \
                and bn_relu_conv3x3_supported(y, self.bn1, self.conv2.weight):
            return bn_relu_conv3x3(y, self.bn1, self.conv2.weight, stats_in=st, stats=True, checked=True)
        out = self.bn1(y, relu=True, stats=st)
        return self.conv2(out, stats=True)

    def _bn2_conv3(self, y, st, fused):
        """conv3(relu(bn2(y))): when conv3's data grad runs on K9, bn2's backward reduction is taken
        in that kernel's epilogue."""
        if fused.bn2_conv3 and isinstance(y, torch.Tensor) and self.conv3._k9(y) \
                and bn_relu_conv1x1_epi_supported(y, self.bn2, self.conv3.weight):
            return bn_relu_conv1x1(y, self.bn2, self.conv3.weight, stats_in=st, stats=True, checked=True)
        out = self.bn2(y, relu=True, stats=st)
        return self.conv3(out, stats=True)

    def _k9f_dual(self, y1, xf) -> bool:
        """DUAL_K9F's confirmation, asked once with conv1's output: conv2 at stride 1 keeps its shape, and
        what it can change (layout, dtype, requires_grad) is compared after it."""
        ds = self.downsample
        return (isinstance(y1, torch.Tensor) and isinstance(xf, torch.Tensor) and self.conv3._k9(y1)
                and ds[0]._k9(xf) and bn2_conv3_bn3_add_bn_relu_supported(
                    y1, self.bn2, self.conv3.weight, self.bn3, xf, ds[0].weight, ds[1]))


class ResNet(nn.Module):
    def __init__(self, block: Type[nn.Module], layers: List[int], num_classes: int = 1000,
                 zero_init_residual: bool = True, width: int = 64):
        super().__init__()
        self.inplanes = width
        self.conv1 = FusedConv2d(3, width, 7, stride=2, padding=3, bias=False)   # K10 stem
        self.bn1 = BN(width)
        self.maxpool = FusedMaxPool2d(3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, width, layers[0])
        self.layer2 = self._make_layer(block, width * 2, layers[1], stride=2)
        self.layer3 = self._make_layer(block, width * 4, layers[2], stride=2)
        self.layer4 = self._make_layer(block, width * 8, layers[3], stride=2)
        self.avgpool = FusedGlobalAvgPool2d((1, 1))
        self.fc = nn.Linear(width * 8 * block.expansion, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):  # FusedBatchNorm2d included
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
        if zero_init_residual:
            for m in self.modules():
                if isinstance(m, Bottleneck):
                    nn.init.zeros_(m.bn3.weight)
                elif isinstance(m, BasicBlock):
                    nn.init.zeros_(m.bn2.weight)

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(conv1x1(self.inplanes, planes * block.expansion, stride),
                                       BN(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        layers += [block(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def _stem_fused(self, x) -> bool:
        """The whole stem as one node (its backward never writes conv1's output gradient): decided before any
        kernel is issued."""
        return (isinstance(x, torch.Tensor) and isinstance(self.conv1, FusedConv2d) and isinstance(self.bn1, BN)
                and isinstance(self.maxpool, FusedMaxPool2d) and self.conv1.stem_ok(x)
                and stem_bn_relu_maxpool_supported(x, self.conv1.weight, self.bn1, self.maxpool))

    def stem(self, x):
        if self._stem_fused(x):
            return stem_bn_relu_maxpool(x, self.conv1.weight, self.bn1, self.maxpool)
        y, st = self.conv1(x, stats=True)
        if isinstance(self.bn1, BN) and isinstance(self.maxpool, FusedMaxPool2d) \
                and bn_relu_maxpool_supported(y, self.bn1, self.maxpool):
            # BN apply + ReLU inside the max-pool's window loads; the pool gradient gathered
            # inside the BN backward: relu(bn1(y)) and its gradient never reach HBM
            return bn_relu_maxpool(y, self.bn1, self.maxpool, st)
        return self.maxpool(self.bn1(y, relu=True, stats=st))

    def head(self, x):
        return self.fc(torch.flatten(self.avgpool(x), 1))

    def forward(self, x):
        x = self.layer4(self.layer3(self.layer2(self.layer1(self.stem(x)))))
        return self.head(x)

    def pipeline_layers(self):
        """The spine the planner costs / partitions: stem, every residual block, head."""
        blocks = [b for layer in (self.layer1, self.layer2, self.layer3, self.layer4) for b in layer]
        return [_Bound(self, "stem"), *blocks, _Bound(self, "head")]


class _Bound(nn.Module):
    """One single-tensor piece of a model's forward as a layer (shares the model's modules)."""

    def __init__(self, model: nn.Module, method: str):
        super().__init__()
        self.parts = nn.ModuleDict({n: m for n, m in model.named_children()
                                    if n in {"stem": ("conv1", "bn1", "maxpool"),
                                             "head": ("avgpool", "fc")}[method]})
        object.__setattr__(self, "_model", model)
        self.method = method

    def forward(self, x):
        return getattr(self._model, self.method)(x)


def resnet18(num_classes: int = 1000, **kw) -> ResNet:
    return ResNet(BasicBlock, [2, 2, 2, 2], num_classes, **kw)


def resnet50(num_classes: int = 1000, **kw) -> ResNet:
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes, **kw)


def resnet101(num_classes: int = 1000, **kw) -> ResNet:
    return ResNet(Bottleneck, [3, 4, 23, 3], num_classes, **kw)
