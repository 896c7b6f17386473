"""The bottleneck oracle (tests/bottleneck_oracle.py) is sound and sharp, shown without a GPU.

fp32 PyTorch stand-ins for the kernels -- fp32 math in another summation order, bf16 stores, the semantics the fp64
references were written to -- go through the same registry and bounds: as they are, every ratio is <= 1 (sound);
with one defect seeded each, some ratio exceeds 1 (sharp).
"""
import pytest
import torch

from bottleneck_oracle import REGISTRY, Call, check_calls, pack_bits, unpack_bits

# (batch, H, W): 35 rows (less than one tile), 162 rows (ragged in both tile sizes), 128 rows
SHAPES = [(1, 5, 7), (2, 9, 9), (2, 8, 8)]
C, C4 = 64, 256
DEFECTS = ["drop_rows", "omit_cc", "unrounded_g", "mask_shift", "mean_m1", "skip_res", "transpose_w"]


def _nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def _r(t):   # [M, C] fp32 rows
    return t.permute(0, 2, 3, 1).reshape(-1, t.size(1)).float()


def _like(rows, n, h, w, dtype=torch.bfloat16):   # [M, C] rows -> NHWC [N, C, H, W]
    return _nhwc(rows.view(n, h, w, -1).permute(0, 3, 1, 2).to(dtype))


def _call(op, a, o, post=None):
    return Call(op, a, post or {}, o, [])


def _group_sums(t0, t1, groups):
    """[G, 2, C] fp32 partial rows: the rows dealt round-robin to G groups (a persistent kernel's walk)."""
    return torch.stack([torch.stack([t0[g::groups].sum(0), t1[g::groups].sum(0)]) for g in range(groups)])


def _tile_sums(t0, t1, tile=256):
    return torch.stack([torch.stack([t0[i:i + tile].sum(0), t1[i:i + tile].sum(0)])
                        for i in range(0, t0.size(0), tile)])


# --------------------------------------------------------------------------------------------- stand-ins
def k_conv1x1_fwd(x, w, defect=None):
    wf = w.view(w.size(0), -1).float()
    if defect == "transpose_w":
        wf = wf.clone()
        wf[:64, :64] = wf[:64, :64].t().clone()
    y = (_r(x) @ wf.t()).bfloat16()
    yf = y.float()
    part = _group_sums(yf, yf * yf, 3)
    n, _, h, w_ = x.shape
    return _call("madnn::conv1x1_fwd", dict(x=x, w=w, stats=True), [_like(y, n, h, w_), part])


def k_bn_fwd(x, res, w, b, partial, relu=True, defect=None, momentum=0.1, eps=1e-5):
    n, c, h, w_ = x.shape
    m = n * h * w_
    rm, rv, nbt = torch.randn(c), torch.rand(c) + 0.5, torch.tensor(3)
    p = partial.double()
    s, q = p[:, 0].sum(0), p[:, 1].sum(0)
    md = m - 1 if defect == "mean_m1" else m
    mean = s / md
    var = (q / md - mean * mean).clamp_min(0)
    inv = (1.0 / (var + float(torch.tensor(eps, dtype=torch.float32))).sqrt()).float()
    scale = w * inv
    shift = b - mean.float() * w * inv
    mom = torch.tensor(momentum, dtype=torch.float32)
    rm2 = (1 - mom) * rm + mom * mean.float()
    rv2 = (1 - mom) * rv + mom * (var * m / (m - 1)).float()
    z = _r(x) * scale + shift
    if res is not None:
        rr = _r(res).clone()
        if defect == "skip_res":
            rr[m // 2] = 0
        z = z + rr
    on = z > 0
    y = torch.where(on, z, torch.zeros_like(z)) if relu else z
    mask = pack_bits(on) if (relu and res is not None) else torch.empty(0, dtype=torch.uint8)
    if defect == "mask_shift" and mask.numel():
        mask = pack_bits(torch.roll(on.reshape(-1), 1).view_as(on))
    a = dict(x=x, res=res, w=w, b=b, run_mean=rm, run_var=rv, nbt=nbt, training=True, momentum=momentum, eps=eps,
             relu=relu, partial=partial)
    return _call("madnn::bn_fwd", a, [_like(y, n, h, w_), mean.float(), inv, scale, shift, mask],
                 dict(run_mean=rm2, run_var=rv2, nbt=nbt + 1))


def k_conv1x1_dgrad_bnb(dy, w, bny, scale, shift, defect=None):
    n, _, h, w_ = dy.shape
    acc = _r(dy) @ w.view(w.size(0), -1).float()
    dx = acc.bfloat16()
    y = _r(bny)
    on = y * scale + shift > 0
    src = acc if defect == "unrounded_g" else dx.float()
    g = torch.where(on, src, torch.zeros_like(src))
    t0, t1 = g, g * y
    if defect == "drop_rows":
        t0, t1 = t0[:-3], t1[:-3]
    part = _group_sums(t0, t1, 2)
    return _call("madnn::conv1x1_dgrad_bnb", dict(dy=dy, w=w, bny=bny, scale=scale, shift=shift),
                 [_like(dx, n, h, w_), part])


def k_conv3x3_fwd_bnb(x, w, bny, scale, shift, defect=None):
    out = torch.nn.functional.conv2d(x.float(), w.float(), padding=1)
    y4 = _nhwc(out.bfloat16())
    y = _r(bny)
    on = y * scale + shift > 0
    src = _r(out) if defect == "unrounded_g" else _r(y4)
    g = torch.where(on, src, torch.zeros_like(src))
    t0, t1 = g, g * y
    if defect == "drop_rows":
        t0, t1 = t0.clone(), t1.clone()
        t0[-3:], t1[-3:] = 0, 0
    return _call("madnn::conv3x3_fwd_bnb", dict(x=x, w=w, bny=bny, scale=scale, shift=shift),
                 [y4, _tile_sums(t0, t1)])


def _bwd_coef(partial, m, w, mean, inv):
    p = partial.double()
    s, q = p[:, 0].sum(0), p[:, 1].sum(0)
    mu, is_ = mean.double(), inv.double()
    dgamma = is_ * (q - mu * s)
    a = w.double() * is_
    k2, k3 = s / m, dgamma / m
    return dgamma.float(), s.float(), a.float(), (-a * is_ * k3).float(), (a * (is_ * k3 * mu - k2)).float()


def k_bn_bwd_ext(dy, x, w, mean, inv, scale, shift, partial, defect=None):
    n, c, h, w_ = x.shape
    dw, db, ca, cb, cc = _bwd_coef(partial, n * h * w_, w, mean, inv)
    xr = _r(x)
    g = torch.where(xr * scale + shift > 0, _r(dy), torch.zeros_like(xr))
    dx = ca * g + cb * xr + (0 if defect == "omit_cc" else cc)
    a = dict(dy=dy, x=x, w=w, save_mean=mean, save_invstd=inv, scale=scale, shift=shift, partial=partial, relu=True)
    return _call("madnn::bn_bwd_ext", a, [_like(dx, n, h, w_), dw, db])


def k_bn3_conv3_bwd(dout, y3, mask, coef, w3, a2, y2, scale2, shift2, defect=None):
    n, _, h, w_ = y3.shape
    m = n * h * w_
    bits = unpack_bits(mask, m, C4)
    if defect == "mask_shift":
        bits = torch.roll(bits.reshape(-1), 1).view_as(bits)
    g = torch.where(bits, _r(dout), torch.zeros(m, C4))
    ca, cb, cc = coef
    dy3 = (ca * g + cb * _r(y3) + (0 if defect == "omit_cc" else cc)).bfloat16().float()
    wf = w3.view(C4, C).float()
    if defect == "transpose_w":
        wf = wf.clone()
        wf[64:128] = wf[64:128].t().clone()
    acc = dy3 @ wf
    da = acc.bfloat16()
    y = _r(y2)
    on = y * scale2 + shift2 > 0
    src = acc if defect == "unrounded_g" else da.float()
    gm = torch.where(on, src, torch.zeros_like(src))
    t0, t1 = gm, gm * y
    if defect == "drop_rows":
        t0, t1 = t0[:-3], t1[:-3]
    part = _group_sums(t0, t1, 2)
    dw = torch.stack([dy3[i::2].t() @ _r(a2)[i::2] for i in range(2)]).sum(0)   # two slabs, added in order
    a = dict(dout=dout, y3=y3, mask=mask, coef=coef, w3=w3, a2=a2, y2=y2, scale2=scale2, shift2=shift2, dw_bf16=False)
    return _call("madnn::bn3_conv3_bwd", a, [_like(da, n, h, w_), part, dw])


# --------------------------------------------------------------------------------------------- the chain
def chain(shape, defect=None, where=None):
    """The recorded calls of a layer-1 tail on stand-ins: conv3 forward + statistics, bn3 (+ identity, ReLU, bit
    mask), K9F backward, bn2's backward on its sums; and bn1 -> conv2's data grads (K9 and K13 BNB).  ``defect``
    is seeded into the stand-in of op ``where`` only."""
    n, h, w = shape
    torch.manual_seed(n * 100 + h * 10 + w)
    d = lambda op: defect if where == op else None   # noqa: E731
    rnd = lambda c: _nhwc((torch.randn(n, c, h, w) * 1.3 + 0.3).bfloat16())   # noqa: E731
    gamma = lambda c: torch.rand(c) * 2 - 0.5   # noqa: E731
    m = n * h * w
    calls = []
    # forward: y2 -> bn2 + relu -> a2 -> conv3 -> y3 -> bn3 + idt + relu
    y2, idt = rnd(C), rnd(C4)
    y2r = _r(y2)
    part2 = _group_sums(y2r, y2r * y2r, 2)
    bn2 = k_bn_fwd(y2, None, gamma(C), torch.randn(C) * 0.2, part2, defect=d("bn_fwd_plain"))
    a2, mean2, inv2, sc2, sh2, _ = bn2.o
    w3 = (torch.randn(C4, C, 1, 1) * C ** -0.5).bfloat16()
    conv3 = k_conv1x1_fwd(a2, w3, d("conv1x1_fwd"))
    y3, part3 = conv3.o
    w3n, b3n = gamma(C4), torch.randn(C4) * 0.2
    bn3 = k_bn_fwd(y3, idt, w3n, b3n, part3, defect=d("bn_fwd"))
    _, mean3, inv3, sc3, sh3, mask = bn3.o
    calls += [bn2, conv3, bn3]
    # backward: K9F on exact coefficients, bn2's backward on its sums
    dout = rnd(C4)
    g = torch.where(unpack_bits(mask, m, C4), _r(dout), torch.zeros(m, C4))
    rows = torch.stack([g.sum(0), (g * _r(y3)).sum(0)])[None]
    _, _, ca, cb, cc = _bwd_coef(rows, m, w3n, mean3, inv3)
    k9f = k_bn3_conv3_bwd(dout, y3, mask, torch.stack([ca, cb, cc]), w3, a2, y2, sc2, sh2, d("bn3_conv3_bwd"))
    da2, partb, _ = k9f.o
    calls += [k9f, k_bn_bwd_ext(da2, y2, bn2.a["w"], mean2, inv2, sc2, sh2, partb, d("bn_bwd_ext"))]
    # the unfused tail's data grad, and conv2's (3x3) data grad, each with the BNB sums
    calls.append(k_conv1x1_dgrad_bnb(rnd(C4), w3, y2, sc2, sh2, d("conv1x1_dgrad_bnb")))
    w2 = _nhwc((torch.randn(C, C, 3, 3) * (9 * C) ** -0.5).bfloat16())
    calls.append(k_conv3x3_fwd_bnb(rnd(C), w2, y2, sc2, sh2, d("conv3x3_fwd_bnb")))
    return calls


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sound(shape):
    rep = check_calls(chain(shape))
    print(rep.table())
    assert set(rep) == {"madnn::bn_fwd", "madnn::conv1x1_fwd", "madnn::bn3_conv3_bwd", "madnn::bn_bwd_ext",
                        "madnn::conv1x1_dgrad_bnb", "madnn::conv3x3_fwd_bnb"}
    assert all(r <= 1.0 for r in rep.values())


# (defect, the stand-in it is seeded into)
SEEDED = [("drop_rows", "conv1x1_dgrad_bnb"), ("drop_rows", "conv3x3_fwd_bnb"), ("drop_rows", "bn3_conv3_bwd"),
          ("omit_cc", "bn_bwd_ext"), ("omit_cc", "bn3_conv3_bwd"),
          ("unrounded_g", "conv1x1_dgrad_bnb"), ("unrounded_g", "conv3x3_fwd_bnb"), ("unrounded_g", "bn3_conv3_bwd"),
          ("mask_shift", "bn_fwd"), ("mask_shift", "bn3_conv3_bwd"),
          ("mean_m1", "bn_fwd"), ("mean_m1", "bn_fwd_plain"),
          ("skip_res", "bn_fwd"),
          ("transpose_w", "conv1x1_fwd"), ("transpose_w", "bn3_conv3_bwd")]


@pytest.mark.parametrize("defect,where", SEEDED, ids=lambda v: v)
def test_sharp(defect, where):
    """At 162 rows (the shape of the issue's example: three tail rows are 2 % of a sum) every seeded defect pushes
    a ratio of the op it sits in above 1."""
    assert defect in DEFECTS
    with pytest.raises(AssertionError, match=r"\|got - e\| / bound") as err:
        check_calls(chain(SHAPES[1], defect, where))
    op = {"bn_fwd_plain": "bn_fwd"}.get(where, where)
    assert f"madnn::{op} " in str(err.value)


def test_every_defect_is_seeded():
    assert {d for d, _ in SEEDED} == set(DEFECTS)


def test_unknown_op_has_no_reference():
    fake = Call("madnn::bn2_conv3_bn3_bwd_v2", {}, {}, [], [])
    with pytest.raises(AssertionError, match="no fp64 reference for madnn::bn2_conv3_bn3_bwd_v2"):
        check_calls(chain(SHAPES[0])[:1] + [fake])


def test_registry_covers_every_bottleneck_op():
    """Every op a Bottleneck route issues (the routing test's expected sequences) has a reference."""
    from test_resnet_routing_gpu import EXPECTED

    issued = {op for seq in EXPECTED.values() for op in seq}
    assert "madnn::bn_bwd_dual_coef" in issued and "aten::addmm_" in issued
    assert issued <= set(REGISTRY), sorted(issued - set(REGISTRY))


def test_batch_one_view_is_the_same_layout():
    """What the batch-1 oracle cases found: a view of a batch-1 NHWC tensor (a block's identity) reports another
    stride for the size-1 dimension, and the BatchNorm nodes took that for another layout."""
    import madnn.ops as ops

    x = torch.randn(1, 64, 5, 7).bfloat16().contiguous(memory_format=torch.channels_last)
    assert ops._same_layout(x.view_as(x), x) and ops._same_layout(torch.empty_like(x), x)
    assert not ops._same_layout(x.contiguous(), x) and not ops._same_layout(x[:, :32], x)
    two = torch.randn(2, 64, 5, 7).contiguous(memory_format=torch.channels_last)
    assert ops._same_layout(two.view_as(two), two) and not ops._same_layout(two.contiguous(), two)
