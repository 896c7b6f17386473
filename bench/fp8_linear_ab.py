"""FP8 Linear A/B: the fp8 forward (quantise x, quantise w with its transposed image, K17) against the bf16
forward the same Linear runs without fp8, and the fp8 data gradient (quantise dy, K17 on the transposed weight
image) against the bf16 one, on Llama-3 8B's four Linears at 8192 tokens and GPT-2 medium's c_proj at 131072.
Both sides in one process, alternating round by round after warm-up, device events around ``reps`` calls.
Per shape one JSON line: every piece in us (median over the rounds), K17 alone in TFLOP/s (2 M N K over its
time), the quantisers in GB/s (bytes read + written over their time) and the end-to-end ratios fp8 / bf16
(< 1: fp8 is faster).  The weight gradient: K17W alone (its two fp8 images exist already in the fp8 path) against
the bf16 weight gradient the Linear runs today (``ops.wgrad_into``, its tuned choice), with K17W's split count and
the bytes of activation a Linear saves for its backward in both modes, computed from the shape.
The MX side (``fp8="mx"``): the one-pass block quantiser against the three-launch per-tensor one on x, W (with the
second image) and dy, K17X against K17 on images made beforehand, and the MX forward and data gradient end to end
against the per-tensor ones and against bf16; ``k17_spread`` is K17's own max / min over the rounds, the
run-to-run spread a K17X / K17 ratio has to be read against.
The MX weight gradient (``fp8="mx_wgrad"``): K17XW on token-blocked images made beforehand against the bf16 weight
gradient and against K17W (the same data bytes plus 1/32 for the scales; ``k17w_spread`` as above), the quantiser
launches that also write the token-blocked image against the plain MX ones, and ``mx_wgrad_over_mx``, the sum of
the pieces in which one forward + backward of the two modes differs.
``--out`` also writes the whole record as one JSON file."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [  # name, tokens, in-features, out-features
    ("llama3-8b qkv", 8192, 4096, 6144), ("llama3-8b proj", 8192, 4096, 4096),
    ("llama3-8b gate_up", 8192, 4096, 28672), ("llama3-8b down", 8192, 14336, 4096),
    ("gpt2-medium c_proj", 131072, 4096, 1024),
]


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def measure(name, M, K, N, reps, rounds):
    from madnn import ops

    k = torch.ops.madnn
    x = torch.randn(M, K, device="cuda").bfloat16()
    w = (torch.randn(N, K, device="cuda") * 0.02).bfloat16()
    dy = torch.randn(M, N, device="cuda").bfloat16()
    x8, _, sx = k.fp8_quant(x, 0, False)
    w8, w8t, sw = k.fp8_quant(w, 0, True)
    g8, _, sg = k.fp8_quant(dy, 1, False)

    mx8, mex, _, _ = k.mx_quant(x, 0, False)
    mw8, mew, mw8t, mewt = k.mx_quant(w, 0, True)
    mg8, meg, _, _ = k.mx_quant(dy, 0, False)
    _, _, mx8c, mexc = k.mx_quant_cols(x, 0)
    _, _, mg8c, megc = k.mx_quant_cols(dy, 0)

    dw8, dw16, dwx = torch.empty_like(w), torch.empty_like(w), torch.empty_like(w)

    def fp8_fwd():
        a8, _, sa = k.fp8_quant(x, 0, False)
        b8, _, sb = k.fp8_quant(w, 0, True)
        return k.fp8_gemm(a8, sa[1:], b8, sb[1:], None, None)

    def fp8_dgrad():
        a8, _, sa = k.fp8_quant(dy, 1, False)
        return k.fp8_gemm(a8, sa[1:], w8t, sw[1:], None, None)

    def mx_fwd():
        a8, ea, _, _ = k.mx_quant(x, 0, False)
        b8, eb, _, _ = k.mx_quant(w, 0, True)
        return k.mx_gemm(a8, ea, b8, eb, None, None)

    def mx_dgrad():
        a8, ea, _, _ = k.mx_quant(dy, 0, False)
        return k.mx_gemm(a8, ea, mw8t, mewt, None, None)

    cases = {
        "quant_x": lambda: k.fp8_quant(x, 0, False), "quant_w_t": lambda: k.fp8_quant(w, 0, True),
        "quant_dy": lambda: k.fp8_quant(dy, 1, False),
        "k17_fwd": lambda: k.fp8_gemm(x8, sx[1:], w8, sw[1:], None, None),
        "k17_dgrad": lambda: k.fp8_gemm(g8, sg[1:], w8t, sw[1:], None, None),
        "fp8_fwd": fp8_fwd, "bf16_fwd": lambda: torch.nn.functional.linear(x, w),
        "fp8_dgrad": fp8_dgrad, "bf16_dgrad": lambda: ops.dgrad(dy, w),
        "k17w_wgrad": lambda: k.fp8_wgrad(g8, sg[1:], x8, sx[1:], dw8, 0),
        "bf16_wgrad": lambda: ops.wgrad_into(dy, x, dw16),
        "mx_quant_x": lambda: k.mx_quant(x, 0, False), "mx_quant_w_t": lambda: k.mx_quant(w, 0, True),
        "mx_quant_dy": lambda: k.mx_quant(dy, 0, False),
        "k17x_fwd": lambda: k.mx_gemm(mx8, mex, mw8, mew, None, None),
        "k17x_dgrad": lambda: k.mx_gemm(mg8, meg, mw8t, mewt, None, None),
        "mx_fwd": mx_fwd, "mx_dgrad": mx_dgrad,
        "mx_quant_cols_x": lambda: k.mx_quant_cols(x, 0), "mx_quant_cols_dy": lambda: k.mx_quant_cols(dy, 0),
        "k17xw_wgrad": lambda: k.mx_wgrad(mg8c, megc, mx8c, mexc, dwx, 0),
    }
    for fn in cases.values():   # warm-up: code objects, library algorithm choice, dgrad's per-shape choice
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {n: [] for n in cases}
    for _ in range(rounds):     # alternate all sides inside every round
        for n, fn in cases.items():
            us[n].append(timed(fn, reps))
    med = {n: statistics.median(v) for n, v in us.items()}
    flop = 2.0 * M * N * K
    rec = {"shape": name, "M": M, "K": K, "N": N, "reps": reps, "rounds": rounds,
           "us": {n: round(v, 1) for n, v in med.items()},
           "us_min_max": {n: [round(min(v), 1), round(max(v), 1)] for n, v in us.items()},
           "k17_fwd_tflops": round(flop / med["k17_fwd"] / 1e6, 1),
           "k17_dgrad_tflops": round(flop / med["k17_dgrad"] / 1e6, 1),
           "bf16_fwd_tflops": round(flop / med["bf16_fwd"] / 1e6, 1),
           "quant_x_gbs": round(3.0 * M * K / med["quant_x"] / 1e3, 1),        # 2 B read + 1 B written per element
           "quant_w_t_gbs": round(4.0 * N * K / med["quant_w_t"] / 1e3, 1),    # + the transposed image
           "quant_dy_gbs": round(3.0 * M * N / med["quant_dy"] / 1e3, 1),
           "fwd_ratio_fp8_over_bf16": round(med["fp8_fwd"] / med["bf16_fwd"], 3),
           "dgrad_ratio_fp8_over_bf16": round(med["fp8_dgrad"] / med["bf16_dgrad"], 3),
           "k17w_wgrad_tflops": round(flop / med["k17w_wgrad"] / 1e6, 1),
           "bf16_wgrad_tflops": round(flop / med["bf16_wgrad"] / 1e6, 1),
           "bf16_wgrad_choice": ops._CHOICES["wgrad"].get(("linear", M, N, K), "lt"),
           "k17w_splits": k.fp8_wgrad_splits(M, N, K),
           "wgrad_ratio_k17w_over_bf16": round(med["k17w_wgrad"] / med["bf16_wgrad"], 3),
           "mx_quant_over_fp8_quant": {n: round(med["mx_quant_" + n] / med["quant_" + n], 3) for n in ("x", "w_t", "dy")},
           "k17x_over_k17": {n: round(med["k17x_" + n] / med["k17_" + n], 3) for n in ("fwd", "dgrad")},
           "k17_spread": {n: round(max(us["k17_" + n]) / min(us["k17_" + n]), 3) for n in ("fwd", "dgrad")},
           "k17x_fwd_tflops": round(flop / med["k17x_fwd"] / 1e6, 1),
           "mx_over_fp8": {n: round(med["mx_" + n] / med["fp8_" + n], 3) for n in ("fwd", "dgrad")},
           "mx_over_bf16": {n: round(med["mx_" + n] / med["bf16_" + n], 3) for n in ("fwd", "dgrad")},
           "k17xw_wgrad_tflops": round(flop / med["k17xw_wgrad"] / 1e6, 1),
           "wgrad_ratio_k17xw_over_bf16": round(med["k17xw_wgrad"] / med["bf16_wgrad"], 3),
           "wgrad_ratio_k17xw_over_k17w": round(med["k17xw_wgrad"] / med["k17w_wgrad"], 3),
           "k17w_spread": round(max(us["k17w_wgrad"]) / min(us["k17w_wgrad"]), 3),
           "mx_quant_cols_over_mx_quant": {n: round(med["mx_quant_cols_" + n] / med["mx_quant_" + n], 3) for n in ("x", "dy")},
           # what differs between fp8="mx_wgrad" and fp8="mx" in one forward + backward: both quantisers and the wgrad
           "mx_wgrad_over_mx": round((med["mx_quant_cols_x"] + med["mx_quant_cols_dy"] + med["k17xw_wgrad"])
                                     / (med["mx_quant_x"] + med["mx_quant_dy"] + med["bf16_wgrad"]), 3),
           # bf16 x / e4m3 x8 + its scale pair / bf16 x / token-blocked e4m3 image + a scale byte per 32 tokens and column
           "saved_activation_bytes": {"fp8": 2 * M * K, "fp8_wgrad": M * K + 8, "mx": 2 * M * K,
                                      "mx_wgrad": M * K + (M + 31) // 32 * K}}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from madnn import ops

    assert torch.cuda.is_available() and ops.load_kernels(), "needs the GPU and the kernel library"
    recs = [measure(*s, args.reps, args.rounds) for s in SHAPES]
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "records": recs}, f, indent=1)


if __name__ == "__main__":
    main()
