"""Every kernel call of a ResNet bottleneck against an fp64 reference of that one op, on the tensors it received.

Each case records one forward + backward of a bf16 NHWC training-mode ``Bottleneck`` (tests/bottleneck_oracle.py)
and judges every ``madnn::*`` / library call in it under bounds derived from the op's rounding steps (about 2^-8
relative, against the 10 % in norm of the block-level tests).  Every case runs twice: the second run's outputs
equal the first's bit for bit (fixed reduction orders, no atomics), the library's convolutions excepted.  For the cases
shared with tests/test_resnet_routing_gpu.py the op sequence must be that test's, so a silent fallback cannot
make the check vacuous.  ``-s`` prints the ratio table of each case.
"""
import pytest
import torch

import madnn.models.resnet as resnet
import madnn.ops as ops
import test_resnet_routing_gpu as routing
from bottleneck_oracle import assert_bitwise, check_calls, run_block

pytestmark = pytest.mark.gpu

_ds = routing._ds
BLOCKS = dict(routing.BLOCKS)
# layer 3, which the routing test lacks
BLOCKS["identity_256"] = (lambda: resnet.Bottleneck(1024, 256), 1024, 8)
BLOCKS["downsample_s2_256"] = (lambda: resnet.Bottleneck(512, 256, stride=2, downsample=_ds(512, 1024, 2)), 512, 8)

# weight-gradient pins: the routing test's (library kernels), the project's own K9 / K13 kernels, and the K12
# split-K GEMMs a 1x1 weight gradient may be tuned to
PINS = {"lib": dict(WGRAD="lt", _K13_WGRAD="miopen", _K9_WGRAD="miopen"),
        "own": dict(WGRAD="lt", _K13_WGRAD="k13", _K9_WGRAD="k9"),
        "k12": dict(WGRAD="k12", _K13_WGRAD="miopen", _K9_WGRAD="miopen"),
        "k12w": dict(WGRAD="k12w", _K13_WGRAD="miopen", _K9_WGRAD="miopen"),
        "k12wh": dict(WGRAD="k12wh", _K13_WGRAD="miopen", _K9_WGRAD="miopen")}


def case(block, n=2, hw=None, pin="lib", off=None, grid=None, bn3_zero=False, train=True, expected=None, tag=None):
    """One case: ``block`` of BLOCKS at batch ``n`` and ``hw`` = (H, W); ``off`` = (module, knob) switched off;
    ``grid``: K9's persistent grid target; ``expected``: the routing test's id whose op sequence must be met."""
    side = BLOCKS[block][2]
    h, w = hw or (side, side)
    name = tag or "-".join([block, f"b{n}", f"{h}x{w}", pin] + ([f"{off[1]}=0"] if off else [])
                           + ([f"grid{grid}"] if grid else []) + (["bn3w0"] if bn3_zero else [])
                           + ([] if train else ["eval"]))
    return pytest.param(dict(block=block, n=n, h=h, w=w, pin=pin, off=off, grid=grid, bn3_zero=bn3_zero, train=train,
                             expected=expected), id=name)


EDGES = [(1, (5, 7)), (2, (9, 9))]   # 35 rows: less than one tile; 162 rows: ragged in both tile sizes
CASES = (
    # the routing test's 13 cases, op sequence pinned
    [case(c[0], off=None if c[2] is None else (c[1], c[2]), expected=routing._id(c)) for c in routing.CASES]
    # layer 3; 256 pixels reach the K12P deep forwards and deep data grad, and again with them off
    + [case("identity_256"), case("downsample_s2_256"), case("identity_256", n=4),
       case("identity_256", n=4, off=(ops, "K9_DEEP"))]
    # tile edges; the route is the 8x8 one (a batch-1 block once failed bn3's layout check: the identity is a view
    # of the input, and a view reports another stride for the size-1 batch dimension)
    + [case(b, n=n, hw=hw, expected=b) for b in ("identity_64", "downsample_s1_64") for n, hw in EDGES]
    # several tiles per workgroup: 3136 rows on a persistent grid of 3
    + [case(b, n=4, hw=(28, 28), grid=3, expected=b) for b in ("identity_64", "downsample_s1_64")]
    # bn3.weight = 0: exact zeros
    + [case(b, bn3_zero=True, expected=b) for b in ("identity_64", "downsample_s1_64", "identity_128")]
    # the register-staged main loop
    + [case("identity_64", off=(ops, "K9_RING"))]
    + [case("identity_64", train=False), case("downsample_s2_128", train=False)]
    # the project's own weight-gradient kernels, once per geometry
    + [case(b, pin="own") for b in BLOCKS] + [case("identity_256", n=4, pin="own")]
    + [case(b, n=n, hw=hw, pin="own") for b in ("identity_64", "downsample_s1_64") for n, hw in EDGES]
    + [case(b, n=4, hw=(28, 28), grid=3, pin="own") for b in ("identity_64", "downsample_s1_64")]
    + [case("identity_64", pin=p) for p in ("k12", "k12w", "k12wh")]
)


def _run(spec, dev):
    make, cin, _ = BLOCKS[spec["block"]]
    return run_block(make, cin, spec["n"], spec["h"], spec["w"], dev, train=spec["train"], bn3_zero=spec["bn3_zero"])


@pytest.mark.parametrize("spec", CASES)
def test_every_call_against_fp64(cuda, monkeypatch, request, spec):
    for knob, value in PINS[spec["pin"]].items():
        monkeypatch.setattr(ops, knob, value)
    if spec["off"] is not None:
        monkeypatch.setattr(spec["off"][0], spec["off"][1], False)
    old = ops.conv1x1_tune(0, spec["grid"]) if spec["grid"] else None
    try:
        calls = _run(spec, cuda)
        assert_bitwise(calls, _run(spec, cuda))
    finally:
        if old is not None:
            ops.conv1x1_tune(0, old)
    names = [c.op for c in calls]
    if spec["expected"] is not None:
        assert names == routing.EXPECTED[spec["expected"]]
    assert any(n.startswith("madnn::") for n in names)
    rep = check_calls(calls)
    print(f"\n{request.node.callspec.id}: {len(calls)} calls, worst |got - e| / bound per op\n{rep.table()}")
    for i, op, name, worst in rep.rows:
        print(f"    call {i:2d} {op:32s} {name:28s} {worst:.4f}")
    assert all(r <= 1.0 for r in rep.values())
    if spec["pin"] == "own" and spec["train"]:
        assert "madnn::conv1x1_wgrad" in names
    if spec["pin"].startswith("k12"):
        assert {"k12": "madnn::linear_wgrad", "k12w": "madnn::linear_wgrad4",
                "k12wh": "madnn::linear_wgrad4h"}[spec["pin"]] in names
    if spec["bn3_zero"]:
        # bn3's scale is zero: dy3 = ca g + cb y3 + cc vanishes, and with it conv3's data and weight gradients,
        # bn2's backward sums and bn3's dbeta-independent outputs -- exactly, not within a tolerance
        zeros = {(op, name) for _, op, name, got in rep.exact_zero if torch.count_nonzero(got) == 0}
        assert len(zeros) == len({(op, name) for _, op, name, _ in rep.exact_zero})
        fused = "madnn::bn3_conv3_bwd" in names
        want = [("madnn::bn3_conv3_bwd", "da"), ("madnn::bn3_conv3_bwd", "dw")] if fused else \
            [("madnn::bn_bwd_dual" if "madnn::bn_bwd_dual" in names else "madnn::bn_bwd", "dx")]
        for key in want:
            assert key in zeros, f"{key} is not an exact zero: {sorted(zeros)}"
