#!/usr/bin/env python3
"""Hidden (residual) dropout A/B in one process (interleaved rounds, same random operands), forward +
backward, bf16, at the token counts of bench.py's GPT-2 medium (batch x 1024 tokens) and BERT-large
(batch x 512 tokens) runs, hidden size 1024:

  norm:  (a) k3_drop    K3 residual LayerNorm with dropout_p (in-kernel Philox mask, regenerated in
                        the backward, two gradients out);
         (b) composed   nn.Dropout + K3 residual LayerNorm: what runs with MADNN_HIDDEN_DROPOUT=0;
         (c) k3         K3 residual LayerNorm with p = 0.
  add:   (a) k16        ops.dropout_add(x, residual, p);
         (b) composed   nn.Dropout + add.

Prints one JSON line per (shape, op, side) with the median forward and forward + backward times and
the run-to-run spread of the latter ((max - min) / median over the rounds), then one line per (shape,
op) with a/b, a/c (the price of the RNG) and whether (a) beats (b) by more than the larger of the two
spreads.

    python bench/hidden_dropout_ab.py [--p 0.1] [--batch 128] [--rounds 7] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timeit(fn, iters=10):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from madnn import ops

    assert ops.load_kernels()
    H, p = a.hidden, a.p
    rows_out = []
    for name, tokens in [("gpt2-medium", a.batch * 1024), ("bert-large", a.batch * 512)]:
        g = torch.Generator(device="cuda").manual_seed(0)
        x, r = (torch.randn(tokens, H, device="cuda", generator=g).bfloat16().requires_grad_(True) for _ in range(2))
        w = torch.ones(H, device="cuda", requires_grad=True)
        b = torch.zeros(H, device="cuda", requires_grad=True)
        gy, gs = (torch.randn(tokens, H, device="cuda", generator=g).bfloat16() for _ in range(2))
        norm_sides = {
            "k3_drop": lambda: ops.layer_norm(x, w, b, residual=r, dropout_p=p),
            "composed": lambda: ops.layer_norm(F.dropout(x, p, True), w, b, residual=r),
            "k3": lambda: ops.layer_norm(x, w, b, residual=r),
        }
        add_sides = {
            "k16": lambda: ops.dropout_add(x, r, p),
            "composed": lambda: F.dropout(x, p, True) + r,
        }

        def norm_step(fwd):
            return lambda: torch.autograd.grad(fwd(), (x, r, w, b), (gy, gs))

        def add_step(fwd):
            return lambda: torch.autograd.grad(fwd(), (x, r), gy)

        for op, sides, step, first, base in (("norm", norm_sides, norm_step, "k3_drop", "k3"),
                                             ("add", add_sides, add_step, "k16", None)):
            ts = {s: {"fwd": [], "step": []} for s in sides}
            for _ in range(a.rounds):
                for s, fwd in sides.items():
                    with torch.no_grad():
                        ts[s]["fwd"].append(timeit(fwd))
                    ts[s]["step"].append(timeit(step(fwd)))
            med = {}
            for s in sides:
                f, st = statistics.median(ts[s]["fwd"]), statistics.median(ts[s]["step"])
                med[s] = (st, (max(ts[s]["step"]) - min(ts[s]["step"])) / st)
                row = {"shape": name, "tokens": tokens, "H": H, "p": p, "op": op, "side": s,
                       "fwd_us": round(f * 1e6, 1), "fwd_bwd_us": round(st * 1e6, 1),
                       "fwd_bwd_spread": round(med[s][1], 4), "rounds": a.rounds}
                rows_out.append(row)
                print(json.dumps(row), flush=True)
            ab = med[first][0] / med["composed"][0]
            spread = max(med[first][1], med["composed"][1])
            row = {"shape": name, "op": op, "a_over_b": round(ab, 4),
                   "a_over_c": round(med[first][0] / med[base][0], 4) if base else None,
                   "spread": round(spread, 4),
                   "a_beats_b": bool(ab < 1.0 - spread)}
            rows_out.append(row)
            print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
    main()
