#!/usr/bin/env python3
"""Attention dropout A/B in one process (interleaved rounds, same random operands), forward +
backward, at the GPT-2 medium, BERT-large and Llama-3 8B attention shapes:

  (a) k8_drop   K8 with dropout p (in-kernel Philox mask, regenerated in the backward);
  (b) sdpa_drop the SDPA fallback with dropout p (transposes + F.scaled_dot_product_attention): what
                runs for this input with MADNN_ATTN_DROPOUT=0, and before K8 had dropout;
  (c) k8        K8 with p = 0.

Prints one JSON line per (shape, side) with the median forward and forward + backward times and the
run-to-run spread of the latter ((max - min) / median over the rounds), then one line per shape with
a/b, a/c (the price of the RNG) and whether (a) beats (b) by more than the larger of the two spreads.

    python bench/attn_dropout_ab.py [--p 0.1] [--batch 16] [--rounds 7] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

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
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from madnn import ops
    from madnn.ops import reference

    assert ops.load_kernels()
    rows = []
    for name, S, H, HKV, D, causal, B in [("gpt2-medium", 1024, 16, 16, 64, True, a.batch),
                                          ("bert-large", 512, 16, 16, 64, False, a.batch),
                                          ("llama3-8b", 4096, 32, 8, 128, True, 2)]:
        g = torch.Generator(device="cuda").manual_seed(0)
        q = torch.randn(B, S, H, D, device="cuda", generator=g).bfloat16().requires_grad_(True)
        k, v = (torch.randn(B, S, HKV, D, device="cuda", generator=g).bfloat16().requires_grad_(True) for _ in range(2))
        do = torch.randn(B, S, H, D, device="cuda", generator=g).bfloat16()
        sides = {
            "k8_drop": lambda: ops.attention(q, k, v, causal=causal, dropout_p=a.p),
            "sdpa_drop": lambda: reference.attention(q, k, v, causal=causal, dropout_p=a.p),
            "k8": lambda: ops.attention(q, k, v, causal=causal),
        }

        def step(fwd):
            return lambda: torch.autograd.grad(fwd(), (q, k, v), do)

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
            row = {"shape": name, "B": B, "S": S, "H": H, "Hkv": HKV, "D": D, "causal": causal, "p": a.p, "side": s,
                   "fwd_us": round(f * 1e6, 1), "fwd_bwd_us": round(st * 1e6, 1), "fwd_bwd_spread": round(med[s][1], 4),
                   "rounds": a.rounds}
            rows.append(row)
            print(json.dumps(row), flush=True)
        ab, ac = med["k8_drop"][0] / med["sdpa_drop"][0], med["k8_drop"][0] / med["k8"][0]
        spread = max(med["k8_drop"][1], med["sdpa_drop"][1])
        row = {"shape": name, "a_over_b": round(ab, 4), "a_over_c": round(ac, 4), "spread": round(spread, 4),
               "a_beats_b": bool(ab < 1.0 - spread)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
