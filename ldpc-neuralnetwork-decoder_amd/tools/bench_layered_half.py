#!/usr/bin/env python3
"""Time the half-precision layered min-sum decoder against the float32 layered decoders on one GPU
("Half-precision layered min-sum").

BG2 (codes/NR_2_0_32.txt) lifted to each --shapes Z:B, B frames of the on-device AWGN channel at --snr,
alpha 0.75, early stop off.  Candidates, at 1, 6 and 10 iterations, alternating inside every repetition, each
decode timed with device events after --warmup untimed rounds:
  fp16      LayeredMinSumDecoder(precision="fp16")         streaming kernels on every graph
  fp32      LayeredMinSumDecoder(any_graph=True)           streaming kernels where Z does not divide 64;
                                                           the LDS-resident kernels where it does (Z = 32)
  fp32s     the same decoder with LDPC_FLOOD_STREAM=1      only on a graph with an LDS-resident schedule: the
                                                           float32 streaming layered kernels there (the library
                                                           reads the variable at every decode, so it is set
                                                           around these decodes alone)
Per shape:
  ratio_<i>            fp16 median / fp32 median at i iterations
  fp16_max_lt_fp32_min_<i>   the fp16 decoder's slowest repetition is faster than the fp32 decoder's fastest
  per_iter_ratio       fp16 per-iteration time / fp32's, each as (t(10) - t(1)) / 9; the byte model says 0.507
  frame_errors         at --fe-snr on the same LLRs, 6 and 10 iterations: fp16, fp32, and the binomial 95 %
                       interval around the fp32 count (recorded, not barred)
Prints one JSON line.

    python tools/bench_layered_half.py [--shapes 12:65536,96:32768,384:8192,32:65536] [--snr 2.0]
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

ITERS = (1, 6, 10)
BYTE_MODEL = 0.507  # (159 * 8 + 38 * 3) / (159 * 16 + 38 * 5): DESIGN.md section 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="12:65536,96:32768,384:8192,32:65536", help="Z:B pairs")
    ap.add_argument("--snr", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fe-snr", type=float, default=-3.0)
    ap.add_argument("--seed", type=int, default=20251015)
    a = ap.parse_args()

    import torch
    from ldpc_neural_decoder.models import LayeredMinSumDecoder
    from ldpc_neural_decoder.utils import awgn_llr, expand_base_matrix, load_base_matrix

    if not torch.cuda.is_available():
        sys.exit("bench_layered_half: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda", 0)
    base = load_base_matrix(os.path.join(PKG, "..", "codes", "NR_2_0_32.txt"))
    out = {"snr_db": a.snr, "reps": a.reps, "device": torch.cuda.get_device_name(0), "byte_model": BYTE_MODEL,
           "shapes": {}}
    for shape in a.shapes.split(","):
        Z, B = (int(s) for s in shape.split(":"))
        H = expand_base_matrix(base, Z)
        llr = awgn_llr(B, H.shape[1], a.snr, seed=a.seed, device=dev)
        runs = {}
        for i in ITERS:
            runs[f"fp16_{i}"] = LayeredMinSumDecoder(H, i, 0.75, early_stopping=False, precision="fp16")
            runs[f"fp32_{i}"] = LayeredMinSumDecoder(H, i, 0.75, early_stopping=False, any_graph=True)
        if runs["fp32_1"].graph(dev).Z != 1:  # LDS-resident: the streaming float32 kernels need the switch
            for i in ITERS:
                runs[f"fp32s_{i}"] = runs[f"fp32_{i}"]
        times = {k: [] for k in runs}
        for rep in range(a.warmup + a.reps):
            for name, dec in runs.items():  # alternating: every repetition times each decoder once
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if name.startswith("fp32s"):
                    os.environ["LDPC_FLOOD_STREAM"] = "1"
                t0.record()
                bits, _ = dec.decode_async(llr, out_dtype=torch.uint8)
                t1.record()
                t1.synchronize()
                os.environ.pop("LDPC_FLOOD_STREAM", None)
                if rep >= a.warmup:
                    times[name].append(t0.elapsed_time(t1))
                del bits
        graph_z = runs["fp32_1"].graph(dev).Z
        r = {"batch": B, "graph_Z": graph_z, "fp32_path": "streaming" if graph_z == 1 else "lds_resident"}
        for name, ts in times.items():
            ms = statistics.median(ts)
            r[name] = {"median_ms": round(ms, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                       "codewords_per_s": round(B / ms * 1e3)}
        med = lambda k: r[k]["median_ms"]
        for i in ITERS:
            r[f"ratio_{i}"] = round(med(f"fp16_{i}") / med(f"fp32_{i}"), 4)
            r[f"fp16_max_lt_fp32_min_{i}"] = r[f"fp16_{i}"]["max_ms"] < r[f"fp32_{i}"]["min_ms"]
            if f"fp32s_{i}" in r:
                r[f"ratio_vs_fp32s_{i}"] = round(med(f"fp16_{i}") / med(f"fp32s_{i}"), 4)
                r[f"fp16_max_lt_fp32s_min_{i}"] = r[f"fp16_{i}"]["max_ms"] < r[f"fp32s_{i}"]["min_ms"]
        if "fp32s_10" in r:
            s_it = (med("fp32s_10") - med("fp32s_1")) / 9
            r["fp32s_ms_per_iter"] = round(s_it, 4)
            r["per_iter_ratio_vs_fp32s"] = round((med("fp16_10") - med("fp16_1")) / 9 / s_it, 4)
        h_it, f_it = (med("fp16_10") - med("fp16_1")) / 9, (med("fp32_10") - med("fp32_1")) / 9
        r["fp16_ms_per_iter"], r["fp32_ms_per_iter"] = round(h_it, 4), round(f_it, 4)
        r["per_iter_ratio"] = round(h_it / f_it, 4)
        r["per_iter_ratio_minus_byte_model"] = round(h_it / f_it - BYTE_MODEL, 4)
        # frame errors against the all-zero codeword, the two precisions on the same LLRs
        del llr
        low = awgn_llr(B, H.shape[1], a.fe_snr, seed=7, device=dev)
        fe = lambda dec: int(dec.decode(low, out_dtype=torch.uint8)[0].any(1).sum().item())
        r["frame_errors"] = {"snr_db": a.fe_snr, "frames": B}
        for i in (6, 10):  # fp32 here is whichever path the library picks: the two give the same bits
            k32, k16 = fe(runs[f"fp32_{i}"]), fe(runs[f"fp16_{i}"])
            half = 1.96 * math.sqrt(max(k32 * (1.0 - k32 / B), 0.0))
            r["frame_errors"][f"iters_{i}"] = {"fp16": k16, "fp32": k32,
                                               "fp32_ci95": [round(k32 - half, 1), round(k32 + half, 1)]}
        out["shapes"][f"Z{Z}"] = r
        del low, runs
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
