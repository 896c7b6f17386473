"""A/B of the deep 1x1 convolutions on K12P (``gemmp.hip``, the forwards with the ``kStats`` BatchNorm-statistics
epilogue) against K9, on the native switch ``madnn_conv1x1_tune`` key 4 (``madnn.ops.K9_DEEP``).

``kernel``: every K9 forward shape of the ResNet-50 step and its plain data grads in isolation, one process, arms
alternating inside every round, medians of ``rounds`` x ``reps`` launches, spread = max - min over the rounds.
A forward is timed twice: the convolution alone, and the convolution plus the BatchNorm forward that consumes
its partial rows (``batch_norm_act(..., stats=part)``) -- K12P writes M / 64 partial rows where K9 writes a few
hundred, so the consumer's fold of them belongs inside the comparison.  The shapes the launcher keeps on K9
(``conv.hip: use_deep``) run the same kernel in both arms and show equal times.  Per arm: us, TB/s, TF/s and the
fraction of the bound max(bytes / 5 TB/s, FLOP / 2.5 PF/s) of the convolution alone, bytes = input + output in
bf16.

``step``: the ResNet-50 training step of ``bench.py`` with ``madnn.ops.K9_DEEP`` off against on in one process,
interleaved windows, medians; first the off arm against itself for the spread (``bench/bn3_conv3_ab.py step``).

    python bench/conv1x1_deep_ab.py kernel --images 2048 --out k12p_deep_kernel.json
    python bench/conv1x1_deep_ab.py step --batch 2048 --windows 6 --out k12p_deep_step.json
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM, MFMA = 5.0e12, 2.5e15
# (pass, H = W, Cin, Cout, calls per step)
SHAPES = [
    ("fwd", 56, 64, 256, 4), ("fwd", 56, 256, 128, 1), ("fwd", 28, 128, 512, 4), ("fwd", 28, 256, 512, 1),
    ("fwd", 14, 256, 1024, 6), ("fwd", 14, 512, 1024, 1), ("fwd", 7, 512, 2048, 3), ("fwd", 7, 1024, 2048, 1),
    ("fwd", 56, 64, 64, 1), ("fwd", 56, 256, 64, 2),
    ("dgrad", 28, 256, 512, 1), ("dgrad", 56, 64, 64, 1),
]
ARMS = {"k9": 0, "k12p": 1}


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3  # us


def kernel_ab(args):
    from madnn import ops

    assert ops.load_kernels()
    m = torch.ops.madnn
    start = ops.conv1x1_tune(4)
    assert start >= 0, "this library has no deep switch"
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    n = args.images
    rows = []
    for kind, hw, cin, cout, calls in SHAPES:
        M = n * hw * hw

        def act(ch):
            t = torch.empty((n, ch, hw, hw), device=dev, dtype=torch.bfloat16, memory_format=torch.channels_last)
            return t.normal_(0, 1, generator=g)

        w = (torch.randn(cout, cin, 1, 1, device=dev, generator=g) * cin ** -0.5).bfloat16().contiguous(
            memory_format=torch.channels_last)
        fns = {}
        if kind == "fwd":
            x = act(cin)
            gamma, beta = torch.rand(cout, device=dev, generator=g) + 0.5, torch.randn(cout, device=dev, generator=g)
            rm, rv = torch.zeros(cout, device=dev), torch.ones(cout, device=dev)

            def conv_bn():
                y, part = m.conv1x1_fwd(x, w, True)
                return ops.batch_norm_act(y, gamma, beta, rm, rv, training=True, relu=True, stats=part)

            fns["conv"] = lambda: m.conv1x1_fwd(x, w, True)
            fns["conv_bn"] = conv_bn
        else:
            dy = act(cout)
            fns["conv"] = lambda: m.conv1x1_dgrad(dy, w, None, None)
        nbytes = 2 * M * (cin + cout)
        flop = 2.0 * M * cin * cout
        bound_us = max(nbytes / HBM, flop / MFMA) * 1e6

        def run(what, mode):
            ops.conv1x1_tune(4, mode)
            return fns[what]()

        part_rows = {}
        for name, mode in ARMS.items():  # warm
            for what in fns:
                o = run(what, mode)
            if kind == "fwd":
                part_rows[name] = int(run("conv", mode)[1].size(0))
        torch.cuda.synchronize()
        del o
        times = {(what, name): [] for what in fns for name in ARMS}
        for _ in range(args.rounds):
            for what in fns:
                for name, mode in ARMS.items():
                    times[(what, name)].append(timed(lambda: run(what, mode), args.reps))
        row = {"pass": kind, "M": M, "cin": cin, "cout": cout, "calls": calls, "bytes": nbytes, "flop": flop,
               "bound_us": bound_us, "partial_rows": part_rows, "arms": {}}
        for name in ARMS:
            v = times[("conv", name)]
            us = statistics.median(v)
            arm = {"us": us, "us_all": v, "spread_us": max(v) - min(v), "TBps": nbytes / us / 1e6,
                   "TFps": flop / us / 1e6, "frac_of_bound": bound_us / us}
            if "conv_bn" in fns:
                vb = times[("conv_bn", name)]
                arm.update({"conv_bn_us": statistics.median(vb), "conv_bn_us_all": vb,
                            "conv_bn_spread_us": max(vb) - min(vb)})
            row["arms"][name] = arm
        key = "conv_bn_us" if "conv_bn" in fns else "us"
        skey = "conv_bn_spread_us" if "conv_bn" in fns else "spread_us"
        a, b = row["arms"]["k9"], row["arms"]["k12p"]
        row["k12p_gain_us"] = a[key] - b[key]
        row["k12p_wins"] = bool(a[key] - b[key] > max(a[skey], b[skey]))
        rows.append(row)
        print(kind, M, cin, cout, {k: (round(v["us"], 1), round(v.get("conv_bn_us", 0.0), 1))
                                   for k, v in row["arms"].items()},
              "bound", round(bound_us, 1), "wins", row["k12p_wins"], file=sys.stderr, flush=True)
        del fns
    ops.conv1x1_tune(4, start)
    total = {name: sum(r["calls"] * r["arms"][name].get("conv_bn_us", r["arms"][name]["us"]) for r in rows) / 1e3
             for name in ARMS}
    return {"images": n, "reps": args.reps, "rounds": args.rounds, "shapes": rows,
            "call_weighted_ms_with_bn": total}


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

    def window(flag, steps):
        ops.K9_DEEP = bool(flag)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(steps):
            F.cross_entropy(dm(x).float(), y).backward()
            opt.step()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / steps

    for flag in (False, True):
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
    both = s1 + s2
    res = {"flag": "madnn.ops:K9_DEEP", "batch": args.batch, "windows": args.windows, "steps": args.steps,
           "warmup": args.warmup, "same_arm_a_ms": med(s1), "same_arm_b_ms": med(s2), "same_arm_all": [s1, s2],
           "control_max_window_deviation_ms": max(abs(v - med(both)) for v in both),
           "off_ms": med(off), "on_ms": med(on), "off_all": off, "on_all": on, "gain_ms": med(off) - med(on),
           "off_img_s": args.batch / med(off) * 1e3, "on_img_s": args.batch / med(on) * 1e3,
           "speedup": med(off) / med(on)}
    res["gain_over_control_deviation"] = res["gain_ms"] / max(res["control_max_window_deviation_ms"], 1e-9)
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
    ap.add_argument("--warmup", type=int, default=10)
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
