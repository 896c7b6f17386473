#!/usr/bin/env python3
"""K8 attention over a right-padded batch, A/B at BERT-large's and GPT-2 medium's attention shapes
(D = 64) and at Llama-3 8B's (D = 128, GQA, B = 2: the VARLEN D = 128 kernels, which stage differently).

Three arms, forward + backward, interleaved round by round in ONE process per shape on the same
random operands ([B, S, heads, D], the layout the QKV projection produces):

  (a) dense     ops.attention(q, k, v)                     every position a real token
  (b) varlen    ops.attention(q, k, v, seqlens=L)          L uniform in [S/2, S], fixed seed
  (c) sdpa      transposes + F.scaled_dot_product_attention with the boolean [B, 1, S, S] mask of the
                same L (and the causal structure): what a padded batch ran before K8 took lengths.  The
                mask is built once outside the timed region (HF builds it once per model forward).
  (d) staged    (a) with the LDS-DMA ring kernels switched off (``madnn_attn_tune`` keys 7 and 8, set once
                around each timed round, outside the events): the dense call on the register-staged
                kernels, the ones (b) runs.  Not part of the bar; it separates what the skipped tiles
                save from what leaving the rings costs (at D = 128 there are no rings: (d) is (a) again).

Before timing, (b) is compared with (c) on the valid rows.  The parent process starts one child per
shape under its own time limit and stops at the first child that fails; it never touches the GPU
itself.  The result holds, per shape, the medians, all rounds of every arm, the spread (max - min
over the rounds) of (a), the ratio (b) / (a) and whether (c) - (b) exceeds that spread.

    python bench/attn_varlen_ab.py [--batch 32] [--rounds 7] [--out profiles/attn_varlen_ab.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {  # name: (S, H, Hkv, D, causal, batch or None for --batch, divisor of --iters)
    "bert-large": (512, 16, 16, 64, False, None, 1),
    "gpt2-medium": (1024, 16, 16, 64, True, None, 1),
    "llama3-8b": (4096, 32, 8, 128, True, 2, 4),
}


def child(name: str, batch: int, rounds: int, iters: int) -> dict:
    import torch
    import torch.nn.functional as F

    from madnn import ops
    from madnn.ops import reference

    assert torch.cuda.is_available() and ops.load_kernels(), "needs a GPU and the native kernels"
    S, H, HKV, D, causal, fixed_b, div = SHAPES[name]
    B = fixed_b or batch
    iters = max(iters // div, 1)
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(B, S, H, D, device="cuda", generator=g).bfloat16().requires_grad_(True)
    k, v = (torch.randn(B, S, HKV, D, device="cuda", generator=g).bfloat16().requires_grad_(True) for _ in range(2))
    do = torch.randn(B, S, H, D, device="cuda", generator=g).bfloat16()
    lens = torch.randint(S // 2, S + 1, (B,), generator=torch.Generator().manual_seed(1)).to(torch.int32)
    seqlens = lens.cuda()
    valid = reference.attention_valid(seqlens, S)
    # HF's padding mask: key valid (and not in the future); padded query rows keep their valid keys
    mask = valid[:, None, None, :].expand(B, 1, S, S)
    if causal:
        mask = mask & torch.ones(S, S, dtype=torch.bool, device="cuda").tril()
    mask = mask.contiguous()

    def dense():
        return ops.attention(q, k, v, causal=causal)

    def varlen():
        return ops.attention(q, k, v, causal=causal, seqlens=seqlens)

    def sdpa():
        o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), attn_mask=mask,
                                           enable_gqa=H != HKV)
        return o.transpose(1, 2).contiguous()

    tune = ctypes.CDLL(str(ops.kernels_path())).madnn_attn_tune

    arms = {"dense": dense, "varlen": varlen, "sdpa": sdpa, "staged": dense}

    def step(fn):
        torch.autograd.grad(fn(), (q, k, v), do)

    def rings(on: int):   # process-global: forward and backward pick their kernels at launch
        tune(7, on), tune(8, on)

    def timeit(arm):
        fn = arms[arm]
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if arm == "staged":
            rings(0)
        try:
            step(fn)
            s.record()
            for _ in range(iters):
                step(fn)
            e.record()
            e.synchronize()
        finally:
            rings(1)
        return s.elapsed_time(e) / iters * 1e3   # us

    # (b) against (c) on the valid rows (K8 writes zeros at the padded ones, SDPA values)
    vm = valid[:, :, None, None]
    ob, oc = varlen(), sdpa()
    gb = torch.autograd.grad(ob, (q, k, v), do)
    gc = torch.autograd.grad(oc, (q, k, v), torch.where(vm, do, torch.zeros_like(do)))
    rel = lambda x, y: float((x.float() - y.float()).norm() / y.float().norm())
    agree = {"o": rel(torch.where(vm, ob, torch.zeros_like(ob)), torch.where(vm, oc, torch.zeros_like(oc)))}
    agree.update({n: rel(x, torch.where(vm, y, torch.zeros_like(y))) for n, x, y in zip(("dq", "dk", "dv"), gb, gc)})
    ts = {arm: [] for arm in arms}
    for arm in arms:   # warm-up of every arm
        timeit(arm)
    for _ in range(rounds):
        for arm in arms:
            ts[arm].append(timeit(arm))
    med = {arm: statistics.median(t) for arm, t in ts.items()}
    spread = max(ts["dense"]) - min(ts["dense"])
    return {"shape": name, "B": B, "S": S, "H": H, "Hkv": HKV, "D": D, "causal": causal, "rounds": rounds,
            "iters_per_round": iters, "mean_len_over_S": round(float(lens.float().mean()) / S, 4),
            "valid_tile_fraction": round(float((lens.float() ** 2).mean()) / S ** 2, 4),
            "fwd_bwd_us": {arm: round(m, 1) for arm, m in med.items()},
            "rounds_us": {arm: [round(x, 1) for x in t] for arm, t in ts.items()},
            "dense_spread_us": round(spread, 1), "varlen_over_dense": round(med["varlen"] / med["dense"], 4),
            "varlen_over_staged": round(med["varlen"] / med["staged"], 4),
            "sdpa_over_varlen": round(med["sdpa"] / med["varlen"], 4),
            "varlen_faster_than_sdpa_by_more_than_spread": med["sdpa"] - med["varlen"] > spread,
            "varlen_vs_sdpa_rel_err_valid_rows": agree}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per shape (one child process each)")
    ap.add_argument("--out", default="profiles/attn_varlen_ab.json")
    ap.add_argument("--child", choices=sorted(SHAPES), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.batch, a.rounds, a.iters)), flush=True)
        return 0
    rows = []
    for name in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--batch", str(a.batch), "--rounds",
               str(a.rounds), "--iters", str(a.iters)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {a.timeout} s; stopping", file=sys.stderr)
            return 1
        if res.returncode != 0:   # nothing more is started on the GPU after a failure
            print(f"{name}: exit status {res.returncode}\n{res.stderr[-2000:]}", file=sys.stderr)
            return 1
        row = json.loads(res.stdout.strip().splitlines()[-1])
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"unit": "microseconds, forward + backward of one attention call", "shapes": rows}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
