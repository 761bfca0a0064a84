#!/usr/bin/env python3
"""Time the layered min-sum decoder against flooding min-sum on one GPU.

BG2 Z=32 (codes/NR_2_0_32.txt), B frames of the on-device AWGN channel, alpha 0.75, early stop off:
layered at each --layered iteration count and flooding at --flood iterations, alternating inside
every repetition, each decode timed with device events after --warmup untimed rounds.  Then the
mean per-frame iteration count of both under the per-frame stop.  Prints one JSON line.

    python tools/bench_layered.py [--batch 65536] [--snr 2.0] [--layered 5,7,10] [--flood 10]
"""
import argparse
import json
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
    ap.add_argument("--layered", default="5,7,10")
    ap.add_argument("--flood", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--es-iters", type=int, default=20, help="max_iterations of the per-frame-stop runs")
    ap.add_argument("--seed", type=int, default=20251015)
    a = ap.parse_args()

    import torch
    from ldpc_neural_decoder.models import LayeredMinSumDecoder, MinSumScaledDecoder
    from ldpc_neural_decoder.utils import awgn_llr, expand_base_matrix, load_base_matrix

    if not torch.cuda.is_available():
        sys.exit("bench_layered: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda", 0)
    H = expand_base_matrix(load_base_matrix(os.path.join(PKG, "..", "codes", "NR_2_0_32.txt")), 32)
    llr = awgn_llr(a.batch, H.shape[1], a.snr, seed=a.seed, device=dev)

    runs = {f"layered_{i}": LayeredMinSumDecoder(H, i, 0.75, early_stopping=False)
            for i in (int(s) for s in a.layered.split(","))}
    runs[f"flood_{a.flood}"] = MinSumScaledDecoder(H, a.flood, 0.75, early_stopping=False)
    times = {k: [] for k in runs}
    errs = {}
    for rep in range(a.warmup + a.reps):
        for name, dec in runs.items():  # alternating: every repetition times each decoder once
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            bits, _ = dec.decode_async(llr, out_dtype=torch.uint8)
            t1.record()
            t1.synchronize()
            if rep >= a.warmup:
                times[name].append(t0.elapsed_time(t1))
            elif rep == 0:
                errs[name] = int(bits.any(1).sum().item())
    out = {"batch": a.batch, "snr_db": a.snr, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    for name, ts in times.items():
        ms = statistics.median(ts)
        out[name] = {"median_ms": round(ms, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                     "codewords_per_s": round(a.batch / ms * 1e3), "frame_errors": errs[name]}
    for name, cls in (("layered", LayeredMinSumDecoder), ("flood", MinSumScaledDecoder)):
        _, _, fi = cls(H, a.es_iters, 0.75, early_stopping="frame").decode(llr, out_dtype=torch.uint8,
                                                                           return_frame_iters=True)
        out[f"{name}_frame_stop_mean_iters"] = round(float(fi.float().mean().item()), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
