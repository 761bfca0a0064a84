#!/usr/bin/env python3
"""Time LDPCNeuralDecoder's fused inference kernel against its layer path on one GPU (DESIGN.md
section 3.6).

BG2 (codes/NR_2_0_32.txt) at Z = --z, --iters iterations, depth_L = --depth, the module's initial
weights, --batches frames each of the on-device AWGN channel at --snr.  One process, one decoder, one
LLR tensor per batch size: every repetition times forward() under no_grad once with use_fused=False
(the layer chain, 4 I - 1 launches) and once with use_fused=True (one launch), alternating, each timed
with device events after --warmup untimed rounds.  Per batch size it reports median / min / max of
both, the ratio of the medians, codewords/s, whether the two outputs are bitwise equal, and
  keep_default_on   the fused path's slowest repetition is faster than the layer path's fastest
Prints one JSON line.

    python tools/bench_neural_fused.py [--batches 4096,65536] [--z 32] [--iters 10] [--depth 2] [--snr 2.0]
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
    ap.add_argument("--batches", default="4096,65536")
    ap.add_argument("--z", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--snr", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20251021)
    a = ap.parse_args()

    import torch
    from ldpc_neural_decoder.models import LDPCNeuralDecoder
    from ldpc_neural_decoder.utils import awgn_llr, create_LLR_mapping, expand_base_matrix, load_base_matrix

    if not torch.cuda.is_available():
        sys.exit("bench_neural_fused: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda", 0)
    H = expand_base_matrix(load_base_matrix(os.path.join(PKG, "..", "codes", "NR_2_0_32.txt")), a.z)
    _, cidx, vidx, _ = create_LLR_mapping(H.T)
    dec = LDPCNeuralDecoder(cidx.shape[0], num_iterations=a.iters, depth_L=a.depth).to(dev)
    out = {"Z": a.z, "E": int(cidx.shape[0]), "N": int(H.shape[1]), "iterations": a.iters, "depth_L": a.depth,
           "snr_db": a.snr, "reps": a.reps, "device": torch.cuda.get_device_name(0), "batches": {}}
    with torch.no_grad():
        for B in (int(b) for b in a.batches.split(",")):
            llr = awgn_llr(B, H.shape[1], a.snr, seed=a.seed, device=dev)
            times, soft = {"layers": [], "fused": []}, {}
            for rep in range(a.warmup + a.reps):
                for name in ("layers", "fused"):  # alternating: every repetition times each path once
                    dec.use_fused = name == "fused"
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    s, _ = dec(llr, cidx, vidx)
                    t1.record()
                    t1.synchronize()
                    if rep >= a.warmup:
                        times[name].append(t0.elapsed_time(t1))
                    elif rep == 0:
                        soft[name] = s
                    del s
            r = {"bitwise_equal": bool(torch.equal(soft["layers"].view(torch.int32), soft["fused"].view(torch.int32)))}
            for name, ts in times.items():
                ms = statistics.median(ts)
                r[name] = {"median_ms": round(ms, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                           "codewords_per_s": round(B / ms * 1e3)}
            r["speedup"] = round(r["layers"]["median_ms"] / r["fused"]["median_ms"], 3)
            r["keep_default_on"] = r["fused"]["max_ms"] < r["layers"]["min_ms"]
            out["batches"][str(B)] = r
            del llr, soft
            torch.cuda.empty_cache()
    dec.use_fused = True
    print(json.dumps(out))


if __name__ == "__main__":
    main()
