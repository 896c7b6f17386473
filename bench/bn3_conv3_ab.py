"""K9F A/B: the fused backward kernel behind bn3 + conv3 in ResNet layer-1 bottlenecks.

``kernel``: in isolation on the layer-1 shape (M = images * 56 * 56, 64 -> 256 channels), one process,
arms alternating: the fused kernel (+ its slab reduce) against the three passes it replaces (K5's bn3
backward apply, K9's BNB data grad, the routed weight grad).  bn3's reduction + finalize run in both arms
and are timed on their own, so the apply's share of ``bn_bwd`` is a difference of two timings.  Achieved
bytes/s come from the shapes: the bytes each arm has to move, over its time.

``kernel --form dual``: the downsample block's tail, ``relu(bn3(conv3(a2)) + bn_ds(conv_ds(xf)))``: the two
fused launches (conv3 with bn2's sums, conv_ds plain; each + its slab reduce) against the five passes they
replace (the dual apply, two K9 data grads, two routed weight grads).  The dual reduction + its two finalizes
run in both arms and are timed on their own.

``step``: the ResNet-50 training step of ``bench.py`` (one GPU, DP wrapper, FusedSGD) with a knob off against
on in one process, interleaved windows, medians; first the same arm against itself for the spread.
``--knob fused``: ``madnn.ops._BN3_CONV3_FUSED`` (all of K9F); ``--knob dual``: ``madnn.ops._BN3_CONV3_DUAL``
(K9F on the downsample block only, the identity blocks fused in both arms).

    python bench/bn3_conv3_ab.py kernel --images 2048 --out k9f_kernel.json
    python bench/bn3_conv3_ab.py kernel --form dual --images 2048 --out k9f_dual_kernel.json
    python bench/bn3_conv3_ab.py step --batch 2048 --windows 6 --out k9f_step.json
    python bench/bn3_conv3_ab.py step --knob dual --batch 2048 --windows 6 --out k9f_dual_step.json
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def kernel_ab(args):
    from madnn import ops

    assert ops.load_kernels()
    m = torch.ops.madnn
    dev = torch.device("cuda", 0)
    n, c, c4, hw = args.images, 64, 256, 56
    M = n * hw * hw
    g = torch.Generator(device=dev).manual_seed(0)

    def act(ch, scale=1.0, shift=0.0):
        t = torch.empty((n, ch, hw, hw), device=dev, dtype=torch.bfloat16, memory_format=torch.channels_last)
        t.normal_(0, scale, generator=g)
        return t.add_(shift) if shift else t

    y2, idt, dout = act(c, 1.2, 0.2), act(c4), act(c4)
    w3 = (torch.randn(c4, c, 1, 1, device=dev, generator=g) * c ** -0.5).bfloat16().contiguous(
        memory_format=torch.channels_last)
    f32 = dict(device=dev, dtype=torch.float32)
    bw2, bb2 = torch.rand(c, generator=g, **f32) + 0.5, torch.randn(c, generator=g, **f32) * 0.2
    bw3, bb3 = torch.rand(c4, generator=g, **f32) + 0.5, torch.randn(c4, generator=g, **f32) * 0.2
    a2, mean2, inv2, sc2, sh2, _ = m.bn_fwd(y2, None, bw2, bb2, None, None, None, True, 0.1, 1e-5, True, None)
    y3, part = m.conv1x1_fwd(a2, w3, True)
    out, mean3, inv3, sc3, sh3, mask = m.bn_fwd(y3, idt, bw3, bb3, None, None, None, True, 0.1, 1e-5, True, part)
    del out, idt, part

    def reduce_only():
        return m.bn_bwd_coef(dout, y3, mask, bw3, mean3, inv3, sc3, sh3)

    coef = reduce_only()[0]

    def fused():
        return m.bn3_conv3_bwd(dout, y3, mask, coef, w3, a2, y2, sc2, sh2, True)

    def bn_bwd_full():  # reduction + finalize + apply (dy3 written, the identity gradient deferred)
        return m.bn_bwd(dout, y3, mask, True, bw3, mean3, inv3, sc3, sh3, True, True, False)[0]

    dy3 = bn_bwd_full()

    def dgrad():
        return m.conv1x1_dgrad_bnb(dy3, w3, y2, sc2, sh2)

    def wgrad():
        return ops._conv1x1_wgrad_lib(dy3, a2, w3)

    # results first: the two arms on the same inputs
    da_f, part_f, dw_f = fused()
    da_u, part_u = dgrad()
    dw_u = wgrad()
    torch.cuda.synchronize()

    def rel(a, b):
        return ((a.float() - b.float()).norm() / b.float().norm()).item()

    check = {"da2_rel": rel(da_f, da_u), "dw3_rel": rel(dw_f.view(-1), dw_u.reshape(-1)),
             "bn2_sums_rel": rel(part_f.sum(0), part_u.sum(0))}
    del da_f, da_u, part_f, part_u, dw_f, dw_u
    arms = {"bn3_reduce_finalize": reduce_only, "fused": fused, "bn_bwd_full": bn_bwd_full, "dgrad_bnb": dgrad,
            "wgrad_routed": wgrad}
    for fn in arms.values():  # warm every shape
        fn()
    times = {k: [] for k in arms}
    for _ in range(args.rounds):  # arms alternate inside every round
        for k, fn in arms.items():
            times[k].append(timed(fn, args.reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    apply_ms = med["bn_bwd_full"] - med["bn3_reduce_finalize"]
    unfused_ms = apply_ms + med["dgrad_bnb"] + med["wgrad_routed"]
    wide, narrow, bits = M * c4 * 2, M * c * 2, M * c4 // 8
    bytes_fused = 2 * wide + bits + 3 * narrow            # dout, y3, mask, a2, y2, da2
    bytes_unfused = (2 * wide + bits + wide) + (wide + 2 * narrow) + (wide + narrow)  # apply; dgrad + BNB; wgrad
    res = {"shape": {"M": M, "C": c, "C4": c4}, "reps": args.reps, "rounds": args.rounds, "ms_median": med,
           "ms_all": times, "check_fused_vs_unfused": check,
           "fused_ms": med["fused"], "unfused_ms": unfused_ms, "bn3_apply_ms": apply_ms,
           "speedup": unfused_ms / med["fused"], "saved_ms_per_block": unfused_ms - med["fused"],
           "bytes_fused": bytes_fused, "bytes_unfused": bytes_unfused,
           "fused_TBps": bytes_fused / med["fused"] / 1e9, "unfused_TBps": bytes_unfused / unfused_ms / 1e9}
    return res


def kernel_dual_ab(args):
    from madnn import ops

    assert ops.load_kernels()
    m = torch.ops.madnn
    dev = torch.device("cuda", 0)
    n, c, c4, hw = args.images, 64, 256, 56
    M = n * hw * hw
    g = torch.Generator(device=dev).manual_seed(0)

    def act(ch, scale=1.0, shift=0.0):
        t = torch.empty((n, ch, hw, hw), device=dev, dtype=torch.bfloat16, memory_format=torch.channels_last)
        t.normal_(0, scale, generator=g)
        return t.add_(shift) if shift else t

    def weight():
        return (torch.randn(c4, c, 1, 1, device=dev, generator=g) * c ** -0.5).bfloat16().contiguous(
            memory_format=torch.channels_last)

    y2, xf, dout = act(c, 1.2, 0.2), act(c, 1.0, 0.1), act(c4)
    w3, w_ds = weight(), weight()
    f32 = dict(device=dev, dtype=torch.float32)
    bw2, bb2 = torch.rand(c, generator=g, **f32) + 0.5, torch.randn(c, generator=g, **f32) * 0.2
    bw3, bb3 = torch.rand(c4, generator=g, **f32) + 0.5, torch.randn(c4, generator=g, **f32) * 0.2
    bwd, bbd = torch.rand(c4, generator=g, **f32) + 0.5, torch.randn(c4, generator=g, **f32) * 0.2
    a2, mean2, inv2, sc2, sh2, _ = m.bn_fwd(y2, None, bw2, bb2, None, None, None, True, 0.1, 1e-5, True, None)
    y3, part = m.conv1x1_fwd(a2, w3, True)
    yd, part_d = m.conv1x1_fwd(xf, w_ds, True)
    out, mask, mean3, inv3, _, _, mean_d, inv_d, _, _ = m.bn_fwd_dual(
        y3, yd, bw3, bb3, None, None, None, 0.1, 1e-5, part, bwd, bbd, None, None, None, 0.1, 1e-5, part_d)
    del out, part, part_d

    def reduce_only():
        return m.bn_bwd_dual_coef(dout, y3, yd, mask, bw3, mean3, inv3, bwd, mean_d, inv_d)

    coef = reduce_only()[0]
    coef3, coef_d = coef[:3], coef[3:]

    def fused():
        r3 = m.bn3_conv3_bwd(dout, y3, mask, coef3, w3, a2, y2, sc2, sh2, True)
        rd = m.bn3_conv3_bwd(dout, yd, mask, coef_d, w_ds, xf, None, None, None, True)
        return r3, rd

    def bn_bwd_full():  # reduction + two finalizes + the dual apply (dy3 and dyd written)
        return m.bn_bwd_dual(dout, y3, yd, mask, bw3, mean3, inv3, bwd, mean_d, inv_d)

    dy3, dyd = bn_bwd_full()[:2]

    def dgrad3():
        return m.conv1x1_dgrad_bnb(dy3, w3, y2, sc2, sh2)

    def wgrad3():
        return ops._conv1x1_wgrad_lib(dy3, a2, w3)

    def dgrad_ds():
        return m.conv1x1_dgrad(dyd, w_ds, None, None)

    def wgrad_ds():
        return ops._conv1x1_wgrad_lib(dyd, xf, w_ds)

    # results first: the two arms on the same inputs
    (da_f, part_f, dw3_f), (dx_f, part_e, dwd_f) = fused()
    assert part_e.numel() == 0
    da_u, part_u = dgrad3()
    dw3_u, dx_u, dwd_u = wgrad3(), dgrad_ds(), wgrad_ds()
    torch.cuda.synchronize()

    def rel(a, b):
        return ((a.float() - b.float()).norm() / b.float().norm()).item()

    check = {"da2_rel": rel(da_f, da_u), "dxf_rel": rel(dx_f, dx_u), "dw3_rel": rel(dw3_f.view(-1), dw3_u.reshape(-1)),
             "dw_ds_rel": rel(dwd_f.view(-1), dwd_u.reshape(-1)), "bn2_sums_rel": rel(part_f.sum(0), part_u.sum(0))}
    del da_f, part_f, dw3_f, dx_f, part_e, dwd_f, da_u, part_u, dw3_u, dx_u, dwd_u
    arms = {"dual_reduce_finalize": reduce_only, "fused_2_launches": fused, "bn_bwd_dual_full": bn_bwd_full,
            "dgrad3_bnb": dgrad3, "wgrad3_routed": wgrad3, "dgrad_ds": dgrad_ds, "wgrad_ds_routed": wgrad_ds}
    for fn in arms.values():  # warm every shape
        fn()
    times = {k: [] for k in arms}
    for _ in range(args.rounds):  # arms alternate inside every round
        for k, fn in arms.items():
            times[k].append(timed(fn, args.reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    apply_ms = med["bn_bwd_dual_full"] - med["dual_reduce_finalize"]
    unfused_ms = apply_ms + med["dgrad3_bnb"] + med["wgrad3_routed"] + med["dgrad_ds"] + med["wgrad_ds_routed"]
    wide, narrow, bits = M * c4 * 2, M * c * 2, M * c4 // 8
    # per launch dout, y, mask; then a2, y2, da2 (conv3) and xf, dxf (conv_ds)
    bytes_fused = 2 * (2 * wide + bits) + 3 * narrow + 2 * narrow
    # apply (3 read + mask, 2 written); dgrad + BNB; wgrad; dgrad; wgrad
    bytes_unfused = (5 * wide + bits) + (wide + 2 * narrow) + (wide + narrow) + (wide + narrow) + (wide + narrow)
    return {"form": "dual", "shape": {"M": M, "C": c, "C4": c4}, "reps": args.reps, "rounds": args.rounds,
            "ms_median": med, "ms_all": times, "check_fused_vs_unfused": check,
            "fused_ms": med["fused_2_launches"], "unfused_ms": unfused_ms, "dual_apply_ms": apply_ms,
            "speedup": unfused_ms / med["fused_2_launches"], "saved_ms_per_block": unfused_ms - med["fused_2_launches"],
            "bytes_fused": bytes_fused, "bytes_unfused": bytes_unfused,
            "fused_TBps": bytes_fused / med["fused_2_launches"] / 1e9, "unfused_TBps": bytes_unfused / unfused_ms / 1e9}


def step_ab(args):
    import madnn
    from madnn import ops
    from madnn.models import resnet50
    from madnn.optim import FusedSGD

    madnn.init()
    torch.manual_seed(0)
    model = resnet50()
    opt = FusedSGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=5e-5)
    dm, opt = madnn.distribute(model, opt, strategy="dp")
    x, y = madnn.data.synthetic_batch("image", args.batch, madnn.device(), dtype=torch.bfloat16, channels_last=True)

    knob = {"fused": "_BN3_CONV3_FUSED", "dual": "_BN3_CONV3_DUAL"}[args.knob]
    assert ops._BN3_CONV3_FUSED and ops._BN3_CONV3_DUAL, "both knobs start on: the arms differ in one only"

    def window(flag, steps):
        setattr(ops, knob, flag)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(steps):
            F.cross_entropy(dm(x).float(), y).backward()
            opt.step()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / steps

    for flag in (False, True):  # warm both arms (first-use tuning, library find)
        window(flag, args.warmup)

    def ab(flag_a, flag_b):
        ta, tb = [], []
        for _ in range(args.windows):
            ta.append(window(flag_a, args.steps))
            tb.append(window(flag_b, args.steps))
        return ta, tb

    s1, s2 = ab(False, False)
    off, on = ab(False, True)
    med = statistics.median
    res = {"flag": f"madnn.ops:{knob}", "batch": args.batch, "windows": args.windows, "steps": args.steps,
           "same_arm_a_ms": med(s1), "same_arm_b_ms": med(s2), "same_arm_all": [s1, s2],
           "same_arm_spread": abs(med(s1) - med(s2)) / med(s1),
           "off_ms": med(off), "on_ms": med(on), "off_all": off, "on_all": on,
           "off_img_s": args.batch / med(off) * 1e3, "on_img_s": args.batch / med(on) * 1e3,
           "speedup": med(off) / med(on)}
    madnn.shutdown()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "step"])
    ap.add_argument("--form", choices=["identity", "dual"], default="identity", help="kernel mode: which block's tail")
    ap.add_argument("--knob", choices=["fused", "dual"], default="fused", help="step mode: which switch the arms flip")
    ap.add_argument("--out", default="")
    ap.add_argument("--images", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing elsewhere says nothing"
    if args.mode == "kernel":
        res = kernel_dual_ab(args) if args.form == "dual" else kernel_ab(args)
    else:
        res = step_ab(args)
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
