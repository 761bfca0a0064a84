#!/usr/bin/env python3
"""Per-wave, per-phase timeline of the flooding decoder (timeline build, tools/build_timeline.sh).

    LDPC_AMD_LIB=.../variants/timeline.so LDPC_TIMELINE_OUT=tl.bin python bench.py --steps 1 ...
    python tools/flood_timeline.py tl.bin [out.json]

The dump holds, for the first kTlWgs workgroups x 4 waves, s_memtime (shader clock) stamps:
[0] after the init barrier, then per iteration it: [1+4it] check phase done, [2+4it] barrier 1
passed, [3+4it] variable phase done, [4+4it] barrier 2 passed.  Reported per wave index (the
fixed kernel specialises its work per wave):
  * check / var: cycles from the previous barrier to the end of the wave's own phase work
  * wait1 / wait2: cycles the wave then waits at the barrier
  * critical: how often the wave is the last to reach the barrier (the one the others wait on)
averaged over the recorded workgroups and the iterations 1 .. max_iter - 2 (the first carries the
prologue, the last takes decisions).
The last three words of a row bracket the loop (kernel entry, exit, XCC_ID << 32 | HW_ID):
"outside_loop" reports prologue, loop, epilogue and lifetime per workgroup, the gap between a
workgroup's exit and its successor's entry on the same CU, how many workgroups were resident before
the first exit, and the iteration time by iteration index.
"""
import json
import sys

import numpy as np


LOOP_STAMPS = 2 + 4 * 16  # kTlPer without its tail (flood_dev.hpp)


def outside_loop(t, per, max_iter):
    """The three tail words of each row: entry stamp, exit stamp, XCC_ID << 32 | HW_ID.

    Per workgroup (row): prologue = entry .. post-init barrier, loop = post-init barrier .. last
    barrier, epilogue = last barrier .. exit (first wave in, last wave out).  Turnover: on each CU,
    the k-th entry that follows the CU's first exit is taken as the successor of its k-th exit
    (a freed slot is refilled in order; the recorded rows are the lowest-numbered groups, so it is
    the late entries that are missing, not the early ones)."""
    entry, exit_, where = (t[:, :, per - 3 + k] for k in range(3))
    ok = (entry > 0).all(axis=1) & (exit_ > 0).all(axis=1)
    t, entry, exit_, where = t[ok], entry[ok], exit_[ok], where[ok]
    e0, x1 = entry.min(axis=1), exit_.max(axis=1)
    init_done, last_bar = t[:, :, 0].max(axis=1), t[:, :, 4 * max_iter].max(axis=1)
    pro, loop, epi, life = init_done - e0, last_bar - init_done, x1 - last_bar, x1 - e0
    cu = ((where[:, 0] >> 32) & 0xF) << 8 | ((where[:, 0] >> 8) & 0xFF)  # XCC, then SE / SH / CU of HW_ID
    # s_memtime counters of different CUs are far apart, even inside one XCC (measured), so stamps
    # compare within a CU only: turnover, residency and span are taken per CU
    gaps, early, span = [], 0, 0
    succ = np.zeros(len(e0), dtype=bool)  # entered after an exit on its CU: the steady state
    for c in np.unique(cu):
        m = cu == c
        xs = np.sort(x1[m])
        es = np.sort(e0[m])
        succ |= m & (e0 >= xs[0])
        early += int((es < xs[0]).sum())
        span = max(span, int(xs[-1] - es[0]))
        es = es[es >= xs[0]]  # successors only: the first generation entered before any exit
        k = min(len(es), len(xs))
        gaps.extend((es[:k] - xs[:k]).tolist())
    gaps = np.array(gaps, dtype=np.float64)

    def stat(a):
        return {"mean": round(float(np.mean(a)), 1), "median": round(float(np.median(a)), 1)} if len(a) else None

    # placement: HW_ID[5:4] is the SIMD a wave ran on.  Per workgroup the SIMDs of its waves 0 .. 3,
    # counted over the recorded workgroups, and how often all four waves share the workgroup's CU
    simd = (where >> 4) & 3
    tuples, counts = np.unique(simd, axis=0, return_counts=True)
    order = np.argsort(-counts)[:8]
    wave_cu = ((where >> 32) & 0xF) << 8 | ((where >> 8) & 0xFF)
    placement = {"simd_of_waves_0_to_3": {"".join(str(int(x)) for x in tuples[i]): int(counts[i]) for i in order},
                 "one_wave_per_simd": int((np.sort(simd, axis=1) == np.arange(4)).all(axis=1).sum()),
                 "waves_on_one_cu": int((wave_cu == wave_cu[:, :1]).all(axis=1).sum())}

    return {
        "groups": int(len(e0)),
        "cus_seen": int(len(np.unique(cu))),
        "placement": placement,
        "prologue": stat(pro), "loop": stat(loop), "epilogue": stat(epi), "lifetime": stat(life),
        "dead_share": round(float(np.mean(pro + epi) / np.mean(life)), 4),
        # the same for the workgroups that entered a freed slot (the first generation loads its
        # LLRs all at once, from a cold cache)
        "successors": {"workgroups": int(succ.sum()), "prologue": stat(pro[succ]), "loop": stat(loop[succ]),
                       "epilogue": stat(epi[succ]), "lifetime": stat(life[succ]),
                       "dead_share": round(float(np.mean((pro + epi)[succ]) / np.mean(life[succ])), 4) if succ.any() else None},
        "turnover_gap": stat(gaps), "turnover_pairs": int(len(gaps)),
        "turnover_negative": int((gaps < 0).sum()),
        # residency: workgroups that entered before the first exit on their CU (the first
        # generation: resident workgroups per CU x CUs when every slot fills at once)
        "entered_before_first_exit": early,
        "span_per_cu_max": span,
        # a workgroup's iterations get faster as it ages among its CU's workgroups
        "cycles_by_iteration": [round(float((t[:, :, 4 * (i + 1)].max(axis=1) - t[:, :, 4 * i].max(axis=1)).mean()), 1)
                                for i in range(max_iter)],
    }


def main(path, out=None):
    with open(path, "rb") as f:
        hdr = np.frombuffer(f.read(16), dtype=np.int32)
        nwg, nw, per, max_iter = (int(x) for x in hdr)
        t = np.frombuffer(f.read(), dtype=np.uint64).astype(np.int64).reshape(nwg, nw, per)
    t = t[(t[:, :, 0] > 0).all(axis=1)]  # recorded workgroups only
    its = range(1, max(2, max_iter - 1))
    rows = {k: [] for k in ("check", "wait1", "var", "wait2")}
    crit1, crit2 = np.zeros(nw), np.zeros(nw)
    iter_cycles = []
    for it in its:
        b = 4 * it
        start = t[:, :, b]  # barrier 2 of the previous iteration passed (or init)
        ce, b1, ve, b2 = (t[:, :, b + k] for k in (1, 2, 3, 4))
        rows["check"].append((ce - start).mean(axis=0))
        rows["wait1"].append((b1 - ce).mean(axis=0))
        rows["var"].append((ve - b1).mean(axis=0))
        rows["wait2"].append((b2 - ve).mean(axis=0))
        crit1 += np.bincount(np.argmax(ce, axis=1), minlength=nw)
        crit2 += np.bincount(np.argmax(ve, axis=1), minlength=nw)
        iter_cycles.append((b2.max(axis=1) - start.min(axis=1)).mean())
    res = {"workgroups": int(t.shape[0]), "waves": nw, "iterations_used": list(its),
           "cycles_per_iteration": float(np.mean(iter_cycles))}
    for k, v in rows.items():
        res[k] = [round(float(x), 1) for x in np.mean(v, axis=0)]
    n = crit1.sum()
    res["critical_check"] = [round(float(x) / n, 3) for x in crit1]
    res["critical_var"] = [round(float(x) / n, 3) for x in crit2]
    if per > LOOP_STAMPS:
        res["outside_loop"] = outside_loop(t, per, max_iter)
    print(json.dumps(res, indent=1))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(*sys.argv[1:])
