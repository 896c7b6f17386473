"""Which kernels a ResNet bottleneck issues, and in which order.

One forward + backward of a bf16 NHWC block in training (batch 2) runs under a ``TorchDispatchMode`` that logs
every ``madnn::*`` op and the library convolutions / GEMMs (``aten::convolution``, ``convolution_backward``,
``mm``, ``addmm``).  The expected sequences below are literals recorded on the commit before the routing code
in ``Bottleneck.forward`` was split into "decide the route" and "issue the kernels"; a routing change has to
change them on purpose.  ``ops.WGRAD = "lt"`` and ``ops._K13_WGRAD = "miopen"`` are pinned, so nothing is timed
and no sequence depends on a tuner race.
"""
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import madnn.models.resnet as resnet
import madnn.ops as ops

pytestmark = pytest.mark.gpu

_ATEN = ("aten::convolution", "aten::convolution_backward", "aten::mm", "aten::addmm")


class _Recorder(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = func._schema.name
        # the host-side `*_supported` queries launch nothing: how often a predicate asks is not routing
        if (name.startswith("madnn::") and not name.endswith("_supported")) or name.rstrip("_") in _ATEN:
            self.names.append(name)
        return func(*args, **(kwargs or {}))


def _ds(cin, cout, stride=1):
    return torch.nn.Sequential(resnet.conv1x1(cin, cout, stride), resnet.BN(cout))


# case -> (block factory, input channels, input height = width)
BLOCKS = {
    "identity_64": (lambda: resnet.Bottleneck(256, 64), 256, 8),
    "downsample_s1_64": (lambda: resnet.Bottleneck(64, 64, downsample=_ds(64, 256)), 64, 8),
    "identity_128": (lambda: resnet.Bottleneck(512, 128), 512, 8),
    "downsample_s2_128": (lambda: resnet.Bottleneck(256, 128, stride=2, downsample=_ds(256, 512, 2)), 256, 8),
    "downsample_s2_512": (lambda: resnet.Bottleneck(1024, 512, stride=2, downsample=_ds(1024, 2048, 2)), 1024, 8),
    "identity_512": (lambda: resnet.Bottleneck(2048, 512), 2048, 4),
}

# (case, module holding the knob, knob switched off) -- None: every knob at its default
CASES = [(name, None, None) for name in BLOCKS] + [
    ("identity_64", ops, "_BN3_CONV3_FUSED"),
    ("downsample_s1_64", ops, "_BN3_CONV3_DUAL"),
    ("identity_128", ops, "_BN_DGRAD_EPI"),
    ("identity_128", ops, "DEFER_RES_MASK"),
    ("downsample_s2_128", resnet, "_DS_SUB"),
    ("downsample_s2_128", resnet, "_DUAL_BN"),
    ("downsample_s2_128", resnet, "_FORK_DS"),
]


def _id(case):
    return case[0] if case[2] is None else f"{case[0]}-{case[2]}=0"


def record(name, dev):
    """The logged op names of one forward + backward of block ``name``."""
    make, cin, hw = BLOCKS[name]
    torch.manual_seed(0)
    blk = make().to(dev).to(memory_format=torch.channels_last).train()
    for p in blk.parameters():
        if p.dim() == 4:
            p.data = p.data.bfloat16().contiguous(memory_format=torch.channels_last)
    x = torch.randn(2, cin, hw, hw, device=dev).bfloat16().contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    with _Recorder() as rec:
        y = blk(x)
        y.backward(torch.ones_like(y))
    torch.cuda.synchronize()
    assert x.grad is not None and all(p.grad is not None for p in blk.parameters())
    return rec.names


EXPECTED = {
    "identity_64": """
        madnn::conv1x1_fwd madnn::bn_fwd madnn::conv3x3_fwd madnn::bn_fwd madnn::conv1x1_fwd madnn::bn_fwd
        madnn::bn_bwd_coef madnn::bn3_conv3_bwd madnn::bn_bwd_ext madnn::conv3x3_fwd_bnb
        aten::convolution_backward madnn::bn_bwd_ext madnn::conv1x1_dgrad aten::convolution_backward
    """.split(),
    "downsample_s1_64": """
        madnn::conv1x1_fwd madnn::bn_fwd madnn::conv3x3_fwd madnn::bn_fwd madnn::conv1x1_fwd
        madnn::conv1x1_fwd madnn::bn_fwd_dual madnn::bn_bwd_dual_coef madnn::bn3_conv3_bwd
        madnn::bn3_conv3_bwd madnn::bn_bwd_ext madnn::conv3x3_fwd_bnb aten::convolution_backward
        madnn::bn_bwd_ext madnn::conv1x1_dgrad aten::convolution_backward
    """.split(),
    "identity_128": """
        aten::convolution madnn::bn_fwd madnn::conv3x3_fwd madnn::bn_fwd madnn::conv1x1_fwd madnn::bn_fwd
        madnn::bn_bwd madnn::conv1x1_dgrad_bnb aten::convolution_backward madnn::bn_bwd_ext
        madnn::conv3x3_fwd_bnb aten::convolution_backward madnn::bn_bwd_ext aten::addmm_
        aten::convolution_backward
    """.split(),
    "downsample_s2_128": """
        madnn::conv1x1_fwd madnn::conv1x1_fwd madnn::bn_fwd madnn::conv3x3_fwd_s2 madnn::bn_fwd
        madnn::conv1x1_fwd madnn::bn_fwd_dual madnn::bn_bwd_dual madnn::conv1x1_dgrad_bnb
        aten::convolution_backward madnn::bn_bwd_ext aten::convolution_backward madnn::bn_bwd
        madnn::conv1x1_dgrad aten::convolution_backward madnn::conv1x1_dgrad aten::convolution_backward
    """.split(),
    "downsample_s2_512": """
        aten::convolution madnn::conv1x1_fwd madnn::bn_fwd madnn::conv3x3_fwd_s2 madnn::bn_fwd
        madnn::conv1x1_fwd madnn::bn_fwd_dual madnn::bn_bwd_dual aten::mm aten::convolution_backward
        madnn::bn_bwd aten::convolution_backward madnn::bn_bwd aten::mm aten::convolution_backward aten::mm
        aten::convolution_backward
    """.split(),
    "identity_512": """
        aten::convolution madnn::bn_fwd madnn::conv3x3_fwd madnn::bn_fwd madnn::conv1x1_fwd madnn::bn_fwd
        madnn::bn_bwd aten::mm aten::convolution_backward madnn::bn_bwd madnn::conv3x3_fwd_bnb
        aten::convolution_backward madnn::bn_bwd_ext aten::addmm_ aten::convolution_backward
    """.split(),
    "identity_64-_BN3_CONV3_FUSED=0": """
        madnn::conv1x1_fwd madnn::bn_fwd madnn::conv3x3_fwd madnn::bn_fwd madnn::conv1x1_fwd madnn::bn_fwd
        madnn::bn_bwd madnn::conv1x1_dgrad_bnb aten::convolution_backward madnn::bn_bwd_ext
        madnn::conv3x3_fwd_bnb aten::convolution_backward madnn::bn_bwd_ext madnn::conv1x1_dgrad
        aten::convolution_backward
    """.split(),
    "downsample_s1_64-_BN3_CONV3_DUAL=0": """
        madnn::conv1x1_fwd madnn::conv1x1_fwd madnn::bn_fwd madnn::conv3x3_fwd madnn::bn_fwd
        madnn::conv1x1_fwd madnn::bn_fwd_dual madnn::bn_bwd_dual madnn::conv1x1_dgrad_bnb
        aten::convolution_backward madnn::bn_bwd_ext madnn::conv3x3_fwd_bnb aten::convolution_backward
        madnn::bn_bwd_ext madnn::conv1x1_dgrad aten::convolution_backward madnn::conv1x1_dgrad
        aten::convolution_backward
    """.split(),
    "identity_128-_BN_DGRAD_EPI=0": """
        aten::convolution madnn::bn_fwd madnn::conv3x3_fwd madnn::bn_fwd madnn::conv1x1_fwd madnn::bn_fwd
        madnn::bn_bwd madnn::conv1x1_dgrad aten::convolution_backward madnn::bn_bwd madnn::conv3x3_fwd
        aten::convolution_backward madnn::bn_bwd aten::addmm_ aten::convolution_backward
    """.split(),
    "identity_128-DEFER_RES_MASK=0": """
        aten::convolution madnn::bn_fwd madnn::conv3x3_fwd madnn::bn_fwd madnn::conv1x1_fwd madnn::bn_fwd
        madnn::bn_bwd madnn::conv1x1_dgrad_bnb aten::convolution_backward madnn::bn_bwd_ext
        madnn::conv3x3_fwd_bnb aten::convolution_backward madnn::bn_bwd_ext aten::addmm_
        aten::convolution_backward
    """.split(),
    "downsample_s2_128-_DS_SUB=0": """
        madnn::conv1x1_fwd aten::convolution madnn::bn_fwd madnn::conv3x3_fwd_s2 madnn::bn_fwd
        madnn::conv1x1_fwd madnn::bn_fwd_dual madnn::bn_bwd_dual madnn::conv1x1_dgrad_bnb
        aten::convolution_backward madnn::bn_bwd_ext aten::convolution_backward madnn::bn_bwd
        aten::convolution_backward madnn::conv1x1_dgrad aten::convolution_backward
    """.split(),
    "downsample_s2_128-_DUAL_BN=0": """
        madnn::conv1x1_fwd aten::convolution madnn::bn_fwd madnn::bn_fwd madnn::conv3x3_fwd_s2 madnn::bn_fwd
        madnn::conv1x1_fwd madnn::bn_fwd madnn::bn_bwd madnn::conv1x1_dgrad_bnb aten::convolution_backward
        madnn::bn_bwd_ext aten::convolution_backward madnn::bn_bwd madnn::bn_bwd aten::convolution_backward
        madnn::conv1x1_dgrad aten::convolution_backward
    """.split(),
    "downsample_s2_128-_FORK_DS=0": """
        aten::convolution madnn::bn_fwd madnn::conv1x1_fwd madnn::bn_fwd madnn::conv3x3_fwd_s2 madnn::bn_fwd
        madnn::conv1x1_fwd madnn::bn_fwd madnn::bn_bwd madnn::conv1x1_dgrad_bnb aten::convolution_backward
        madnn::bn_bwd_ext aten::convolution_backward madnn::bn_bwd madnn::conv1x1_dgrad
        aten::convolution_backward madnn::bn_bwd aten::convolution_backward
    """.split(),
}


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_block_op_sequence(cuda, monkeypatch, case):
    name, mod, knob = case
    monkeypatch.setattr(ops, "WGRAD", "lt")
    monkeypatch.setattr(ops, "_K13_WGRAD", "miopen")
    if knob is not None:
        monkeypatch.setattr(mod, knob, False)
    got = record(name, cuda)
    print(f"{_id(case)}: {got}")
    assert got == EXPECTED[_id(case)]
