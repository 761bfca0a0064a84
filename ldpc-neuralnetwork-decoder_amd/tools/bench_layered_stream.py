#!/usr/bin/env python3
"""Time the streaming layered min-sum decoder against streaming flooding min-sum on one GPU
("Streaming layered").

BG2 (codes/NR_2_0_32.txt) lifted to each --shapes Z:B, B frames of the on-device AWGN channel at
--snr, alpha 0.75, early stop off: LayeredMinSumDecoder(any_graph=True) at 1..--iters iterations and
MinSumScaledDecoder at 1 and --iters, alternating inside every repetition, each decode timed with
device events after --warmup untimed rounds.  Per shape it also finds I*, the smallest layered count
whose frame errors at --istar-snr, seed 7, B = 256 do not exceed flooding's at --iters, and derives
  ratio_at_istar   layered(I*) / flooding(--iters)
  per_iter_ratio   layered per-iteration time / flooding's, each as (t(--iters) - t(1)) / (--iters - 1)
Prints one JSON line.

    python tools/bench_layered_stream.py [--shapes 12:65536,96:32768,384:8192] [--snr 2.0] [--iters 10]
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
    ap.add_argument("--shapes", default="12:65536,96:32768,384:8192", help="Z:B pairs")
    ap.add_argument("--snr", type=float, default=2.0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--istar-snr", type=float, default=-3.0)
    ap.add_argument("--seed", type=int, default=20251015)
    a = ap.parse_args()

    import torch
    from ldpc_neural_decoder.models import LayeredMinSumDecoder, MinSumScaledDecoder
    from ldpc_neural_decoder.utils import awgn_llr, expand_base_matrix, load_base_matrix

    if not torch.cuda.is_available():
        sys.exit("bench_layered_stream: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda", 0)
    base = load_base_matrix(os.path.join(PKG, "..", "codes", "NR_2_0_32.txt"))
    out = {"snr_db": a.snr, "reps": a.reps, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for shape in a.shapes.split(","):
        Z, B = (int(s) for s in shape.split(":"))
        H = expand_base_matrix(base, Z)
        llr = awgn_llr(B, H.shape[1], a.snr, seed=a.seed, device=dev)
        runs = {f"layered_{i}": LayeredMinSumDecoder(H, i, 0.75, early_stopping=False, any_graph=True)
                for i in range(1, a.iters + 1)}
        for i in (1, a.iters):
            runs[f"flood_{i}"] = MinSumScaledDecoder(H, i, 0.75, early_stopping=False)
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
                del bits
        r = {"batch": B, "graph_Z": runs["flood_1"].graph(dev).Z}
        for name, ts in times.items():
            ms = statistics.median(ts)
            r[name] = {"median_ms": round(ms, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                       "codewords_per_s": round(B / ms * 1e3), "frame_errors": errs[name]}
        # I*: frame errors on 256 frames at the low SNR, the GPU decoders themselves
        low = awgn_llr(256, H.shape[1], a.istar_snr, seed=7, device=dev)
        fe = lambda dec: int(dec.decode(low, out_dtype=torch.uint8)[0].any(1).sum().item())
        r["istar_frame_errors_layered"] = [fe(runs[f"layered_{i}"]) for i in range(1, a.iters + 1)]
        r["istar_frame_errors_flood"] = fe(runs[f"flood_{a.iters}"])
        ok = [i for i, e in enumerate(r["istar_frame_errors_layered"], 1) if e <= r["istar_frame_errors_flood"]]
        r["istar"] = ok[0] if ok else None
        med = lambda k: r[k]["median_ms"]
        n = a.iters
        if r["istar"]:
            r["ratio_at_istar"] = round(med(f"layered_{r['istar']}") / med(f"flood_{n}"), 4)
        lay_it, flo_it = (med(f"layered_{n}") - med("layered_1")) / (n - 1), (med(f"flood_{n}") - med("flood_1")) / (n - 1)
        r["layered_ms_per_iter"], r["flood_ms_per_iter"] = round(lay_it, 4), round(flo_it, 4)
        r["per_iter_ratio"] = round(lay_it / flo_it, 4)
        out["shapes"][f"Z{Z}"] = r
        del llr, runs
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
