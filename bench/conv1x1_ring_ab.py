"""K9 A/B: the LDS-DMA ring main loop of the 1x1 forward / data grad against the register-staged loop.

``kernel``: every K9 forward and data-grad shape of the ResNet-50 step (``conv1x1_route``) in isolation, one
process, arms alternating inside every round, medians of ``rounds`` x ``reps`` launches.  The arms are the values
of the native switch (``madnn_conv1x1_tune`` key 3): 0 register-staged, 1 ring (on the shapes the launcher gives
it; at K = 192 / 256 the forward then runs 64-wide i tiles).  A library without the switch (an older commit) runs the single arm it has.  Per shape: us, TB/s, TF/s and
the fraction of the bound max(bytes / 5 TB/s, FLOP / 2.5 PF/s), bytes = input + output in bf16 (as
``bench/resnet_convs.py``; a residual or BN input the epilogue reads is counted too).

``step``: the ResNet-50 training step of ``bench.py`` with ``madnn.ops.K9_RING`` off against on in one process,
interleaved windows, medians; first the off arm against itself for the spread (``bench/bn3_conv3_ab.py step``).

    python bench/conv1x1_ring_ab.py kernel --images 2048 --out k9_ring_kernel.json
    python bench/conv1x1_ring_ab.py step --batch 2048 --windows 6 --out k9_ring_step.json
"""
import argparse
import ctypes
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
    ("dgrad_res", 56, 256, 64, 2), ("dgrad_res", 56, 256, 128, 1), ("dgrad", 28, 256, 512, 1),
    ("dgrad", 56, 64, 64, 1), ("dgrad_bnb", 28, 128, 512, 4),
]


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
    tune = ctypes.CDLL(str(ops.kernels_path())).madnn_conv1x1_tune
    start = tune(3, -1)
    arms = {"staged": 0, "ring": 1} if start >= 0 else {"staged": None}
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
        if kind == "fwd":
            x = act(cin)
            fn = lambda: m.conv1x1_fwd(x, w, True)
            nbytes = 2 * M * (cin + cout)
        elif kind in ("dgrad", "dgrad_res"):
            dy = act(cout)
            res = act(cin) if kind == "dgrad_res" else None
            fn = lambda: m.conv1x1_dgrad(dy, w, res, None)
            nbytes = 2 * M * (cin + cout) + (2 * M * cin if res is not None else 0)
        else:
            dy, bny = act(cout), act(cin)
            sc = torch.rand(cin, device=dev, generator=g) + 0.5
            sh = torch.randn(cin, device=dev, generator=g) * 0.2
            fn = lambda: m.conv1x1_dgrad_bnb(dy, w, bny, sc, sh)
            nbytes = 2 * M * (cin + cout) + 2 * M * cin
        flop = 2.0 * M * cin * cout
        bound_us = max(nbytes / HBM, flop / MFMA) * 1e6

        def run(mode):
            if mode is not None:
                tune(3, mode)
            return fn()

        outs = {}
        for name, mode in arms.items():  # warm, and the arms' results on the same inputs
            o = run(mode)
            outs[name] = [t.clone() for t in (o if isinstance(o, tuple) else (o,))]
        torch.cuda.synchronize()
        # the output only: the forward's partial rows follow the plan, which the ring changes at K = 192 / 256
        equal = {name: torch.equal(o[0], outs["staged"][0]) for name, o in outs.items()}
        del outs
        times = {k: [] for k in arms}
        for _ in range(args.rounds):
            for name, mode in arms.items():
                times[name].append(timed(lambda: run(mode), args.reps))
        row = {"pass": kind, "M": M, "cin": cin, "cout": cout, "calls": calls, "bytes": nbytes, "flop": flop,
               "bound_us": bound_us, "output_bitwise_equal_to_staged": equal, "arms": {}}
        for name, v in times.items():
            us = statistics.median(v)
            row["arms"][name] = {"us": us, "us_all": v, "spread_us": max(v) - min(v), "TBps": nbytes / us / 1e6,
                                 "TFps": flop / us / 1e6, "frac_of_bound": bound_us / us}
        rows.append(row)
        print(kind, M, cin, cout, {k: round(a["us"], 1) for k, a in row["arms"].items()},
              "bound", round(bound_us, 1), file=sys.stderr, flush=True)
        del fn
    if start >= 0:
        tune(3, start)
    total = {name: sum(r["calls"] * r["arms"][name]["us"] for r in rows) / 1e3 for name in arms}
    return {"images": n, "reps": args.reps, "rounds": args.rounds, "shapes": rows, "call_weighted_ms": total}


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
        ops.K9_RING = bool(flag)
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
    res = {"flag": "madnn.ops:K9_RING", "batch": args.batch, "windows": args.windows, "steps": args.steps,
           "same_arm_a_ms": med(s1), "same_arm_b_ms": med(s2), "same_arm_all": [s1, s2],
           "control_max_window_deviation_ms": max(abs(v - med(both)) for v in both),
           "off_ms": med(off), "on_ms": med(on), "off_all": off, "on_all": on, "gain_ms": med(off) - med(on),
           "off_img_s": args.batch / med(off) * 1e3, "on_img_s": args.batch / med(on) * 1e3,
           "speedup": med(off) / med(on)}
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
