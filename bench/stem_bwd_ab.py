"""Stem backward A/B: bn1's backward sums in the pooled domain and its apply formed inside the stem weight grad.

``kernel``: in isolation on the stem shape (images x 3 x 224 x 224 -> y [images, 64, 112, 112] -> pooled 56 x 56),
one process, arms alternating, medians of ``rounds`` x ``reps`` launches.  Old backward: ``pool_bn_bwd`` (the gather
reduction, the finalize, the apply that writes dy) + ``stem_wgrad``.  New backward: ``pool_bn_bwd_coef`` (pooled
reduction + finalize) + ``stem_wgrad_bnp``.  Forward pool without and with ``yarg``.  Achieved bytes/s come from the
shapes: the bytes each arm has to move, over its time.

``step``: the ResNet-50 training step of ``bench.py`` (one GPU, DP wrapper, FusedSGD) with
``madnn.ops._STEM_BWD_FUSED`` off against on in one process, interleaved windows, medians; first the off arm against
itself, whose largest single-window deviation from its median is the yardstick for the gain.

    python bench/stem_bwd_ab.py kernel --images 2048 --out stem_bwd_kernel.json
    python bench/stem_bwd_ab.py step --batch 2048 --windows 6 --out stem_bwd_step.json
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
    n, hw, c = args.images, 224, 64
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.empty((n, 3, hw, hw), device=dev, dtype=torch.bfloat16, memory_format=torch.channels_last)
    x.normal_(0, 1, generator=g)
    w = (torch.randn(c, 3, 7, 7, device=dev, generator=g) * 147 ** -0.5).bfloat16()
    f32 = dict(device=dev, dtype=torch.float32)
    bw, bb = torch.rand(c, generator=g, **f32) + 0.5, torch.randn(c, generator=g, **f32) * 0.2
    y, part = m.stem_fwd(x, ops._stem_pack(w), True)
    mean, inv, sc, sh = m.bn_coef(y, bw, bb, None, None, None, 0.1, 1e-5, part)

    def fwd_old():
        return m.pool_bn_fwd(y, sc, sh, 1)

    def fwd_new():
        return m.pool_bn_fwd_yarg(y, sc, sh, 1)

    out, arg, yarg = fwd_new()
    dp = torch.empty_like(out).normal_(0, 1, generator=g)
    pixels = y.numel() // c

    def old_bn():  # gather reduction + finalize + apply (dy written)
        return m.pool_bn_bwd(dp, arg, y, bw, mean, inv, sc, sh, 1)

    dy = old_bn()[0]

    def old_wgrad():
        return m.stem_wgrad(dy, x)

    def new_coef():  # pooled reduction + finalize
        return m.pool_bn_bwd_coef(dp, yarg, bw, mean, inv, sc, sh, pixels)

    coef = new_coef()[0]

    def new_wgrad():
        return m.stem_wgrad_bnp(x, y, dp, arg, sc, sh, coef, 1)

    def rel(a, b):
        return ((a.float() - b.float()).norm() / b.float().norm()).item()

    _, dbw_u, dbb_u = old_bn()
    _, dbw_f, dbb_f = new_coef()
    check = {"dw_rel": rel(new_wgrad(), old_wgrad()), "bn_w_grad_rel": rel(dbw_f, dbw_u),
             "bn_b_grad_rel": rel(dbb_f, dbb_u), "out_equal": bool(torch.equal(fwd_old()[0], out)),
             "arg_equal": bool(torch.equal(fwd_old()[1], arg))}
    arms = {"fwd_pool": fwd_old, "fwd_pool_yarg": fwd_new, "old_bn_reduce_finalize_apply": old_bn,
            "old_wgrad": old_wgrad, "new_bn_reduce_finalize": new_coef, "new_wgrad_bnp": new_wgrad}
    for fn in arms.values():  # warm every shape
        fn()
    times = {k: [] for k in arms}
    for _ in range(args.rounds):  # arms alternate inside every round
        for k, fn in arms.items():
            times[k].append(timed(fn, args.reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    Y, P, A, X = y.numel() * 2, out.numel() * 2, out.numel(), x.numel() * 2
    nbytes = {"fwd_pool": Y + P + A, "fwd_pool_yarg": Y + 2 * P + A,
              "old_bn_reduce_finalize_apply": 2 * (Y + P + A) + Y, "old_wgrad": Y + X,
              "new_bn_reduce_finalize": 2 * P, "new_wgrad_bnp": Y + P + A + X}
    old_ms = med["old_bn_reduce_finalize_apply"] + med["old_wgrad"]
    new_ms = med["new_bn_reduce_finalize"] + med["new_wgrad_bnp"]
    fwd_extra = med["fwd_pool_yarg"] - med["fwd_pool"]
    return {"shape": {"images": n, "y": list(y.shape), "pooled": list(out.shape)}, "reps": args.reps,
            "rounds": args.rounds, "ms_median": med, "ms_all": times, "check_new_vs_old": check,
            "bytes": nbytes, "TBps": {k: nbytes[k] / med[k] / 1e9 for k in med},
            "old_backward_ms": old_ms, "new_backward_ms": new_ms, "forward_extra_ms": fwd_extra,
            "saved_ms": old_ms - new_ms - fwd_extra}


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
    assert ops._STEM_BWD_FUSED, "the knob starts on"

    def window(flag, steps):
        ops._STEM_BWD_FUSED = flag
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
    ctl = s1 + s2
    dev_max = max(abs(t - med(ctl)) for t in ctl)
    gain = med(off) - med(on)
    res = {"flag": "madnn.ops:_STEM_BWD_FUSED", "batch": args.batch, "windows": args.windows, "steps": args.steps,
           "control_a_ms": med(s1), "control_b_ms": med(s2), "control_all": [s1, s2],
           "control_max_window_deviation_ms": dev_max,
           "off_ms": med(off), "on_ms": med(on), "off_all": off, "on_all": on, "gain_ms": gain,
           "gain_over_control_deviation": gain / dev_max if dev_max else float("inf"),
           "off_img_s": args.batch / med(off) * 1e3, "on_img_s": args.batch / med(on) * 1e3,
           "speedup": med(off) / med(on), "peak_mem_gib": torch.cuda.max_memory_allocated() / 2 ** 30}
    madnn.shutdown()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "step"])
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
    res = kernel_ab(args) if args.mode == "kernel" else step_ab(args)
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
