#!/usr/bin/env python3
"""Time half-precision min-sum against the two fp32 flooding min-sum kernels on one GPU.

BG2 Z=32 (codes/NR_2_0_32.txt), B frames of the on-device AWGN channel, alpha 0.75, --iters iterations.
Three candidates decode the same LLRs in one process, alternating inside every repetition, each decode
timed with device events after --warmup untimed rounds:
    fp16        MinSumScaledDecoder(precision="fp16")            packed binary16, two frames per lane
    fp32_table  fp32, set_variant(1)                             the table-driven kernel: same schedule as fp16
    fp32_fixed  fp32, set_variant(0)                             the compile-time-schedule kernel
once with early stop off and once with the per-frame stop.  Then the frame-error comparison: fp16 and fp32
decode the same --fer-batch frames at --fer-snr (early stop off), with the binomial 95 % interval of the
fp32 count.  Prints one JSON line.

    python tools/bench_half.py [--batch 65536] [--snr 2.0] [--iters 10] [--fer-snr -3.0]
"""
import argparse
import json
import math
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
sys.path.insert(0, PKG)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--snr", type=float, default=2.0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fer-snr", type=float, default=-3.0)
    ap.add_argument("--fer-batch", type=int, default=65536)
    ap.add_argument("--seed", type=int, default=20251015)
    a = ap.parse_args()

    import torch
    from ldpc_neural_decoder.models import MinSumScaledDecoder
    from ldpc_neural_decoder.utils import awgn_llr, expand_base_matrix, load_base_matrix

    if not torch.cuda.is_available():
        sys.exit("bench_half: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda", 0)
    H = expand_base_matrix(load_base_matrix(os.path.join(PKG, "..", "codes", "NR_2_0_32.txt")), 32)
    llr = awgn_llr(a.batch, H.shape[1], a.snr, seed=a.seed, device=dev)

    def candidates(es):
        out = {"fp16": MinSumScaledDecoder(H, a.iters, 0.75, early_stopping=es, precision="fp16")}
        for name, variant in (("fp32_table", 1), ("fp32_fixed", 0)):
            dec = MinSumScaledDecoder(H, a.iters, 0.75, early_stopping=es)
            dec.graph(dev).set_variant(variant)  # each decoder owns its graph
            out[name] = dec
        return out

    out = {"batch": a.batch, "snr_db": a.snr, "iters": a.iters, "reps": a.reps,
           "device": torch.cuda.get_device_name(0)}
    for mode, es in (("es_off", False), ("es_frame", "frame")):
        runs = candidates(es)
        times = {k: [] for k in runs}
        for rep in range(a.warmup + a.reps):
            for name, dec in runs.items():  # alternating: every repetition times each candidate once
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                dec.decode_async(llr, out_dtype=torch.uint8)
                t1.record()
                t1.synchronize()
                if rep >= a.warmup:
                    times[name].append(t0.elapsed_time(t1))
        res = {}
        for name, ts in times.items():
            ms = statistics.median(ts)
            res[name] = {"median_ms": round(ms, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                         "codewords_per_s": round(a.batch / ms * 1e3)}
        res["fp16_over_fp32_table"] = round(res["fp32_table"]["median_ms"] / res["fp16"]["median_ms"], 4)
        res["fp16_over_fp32_fixed"] = round(res["fp32_fixed"]["median_ms"] / res["fp16"]["median_ms"], 4)
        out[mode] = res

    # frame errors on the same LLRs (all-zero codeword: a frame is in error when any decision is 1)
    x = awgn_llr(a.fer_batch, H.shape[1], a.fer_snr, seed=a.seed + 1, device=dev)
    fe = {}
    for name, kw in (("fp16", {"precision": "fp16"}), ("fp32", {})):
        bits, _ = MinSumScaledDecoder(H, a.iters, 0.75, early_stopping=False, **kw).decode(x, out_dtype=torch.uint8)
        fe[name] = int(bits.any(1).sum().item())
    p = fe["fp32"] / a.fer_batch
    half = 1.96 * math.sqrt(a.fer_batch * p * (1 - p))
    out["frame_errors"] = {"snr_db": a.fer_snr, "frames": a.fer_batch, "fp16": fe["fp16"], "fp32": fe["fp32"],
                           "fp32_binomial_95": [round(fe["fp32"] - half, 1), round(fe["fp32"] + half, 1)],
                           "fp16_inside": abs(fe["fp16"] - fe["fp32"]) <= half}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
