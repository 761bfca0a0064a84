#!/usr/bin/env python3
"""Generate csrc/gen/fixed_codes.hpp: compile-time schedules for the codes the reference ships.

The reference decodes exactly two codes (5G LDPC CODES/NR_2_0_4.txt and NR_2_0_32.txt, copied to
codes/).  For those, libldpc_amd carries a flooding kernel whose whole schedule -- which wave
updates which block-row and column, every LDS slot offset and circulant shift -- is a set of
compile-time constants, so the iteration loop is straight-line code with immediate LDS offsets
and no descriptor decoding.  Any other graph uses the table-driven kernel.

The slot numbering and the wave schedule are the ones graph.cpp computes at runtime (same LPT
rule, same tie-breaking), so both kernels hold identical LDS images.

    python tools/gen_fixed_codes.py   (run from ldpc-neuralnetwork-decoder_amd/; Makefile does it)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CODES = [("BG2_Z4", os.path.join(ROOT, "codes", "NR_2_0_4.txt"), 4),
         ("BG2_Z32", os.path.join(ROOT, "codes", "NR_2_0_32.txt"), 32)]
W = 4
DIRECT_DC = 6  # the default of LDPC_DIRECT_DC in csrc/flood_fixed.hpp
# Register edges (RE_* arrays, reg_edges() in csrc/flood_fixed.hpp): at most this many messages
# per wave stay in VGPRs.  Above what the search finds for either code (BG2 Z=32: 11 per wave, 44;
# BG2 Z=4: 15 / 14 / 14 / 15, 58), so every eligible edge is taken; a larger cap finds no more (at
# Z=4 it only spreads the same 58 less evenly).  The kernel instances that cannot afford them all
# keep the first LDPC_SLOW_REG_EDGES of a wave's (csrc/flood_fixed.hpp FxPlan).
REG_EDGE_CAP = 16
# modelled LDS cycles a register edge saves: the check phase's per-edge term of the row costs, and
# the read and the write of var_task_cost
CHK_EDGE_LDS = 2.0
VAR_EDGE_LDS = 18.12
# The joint schedule (RE_J_* arrays, joint_schedule() below): at most this many kept messages
# (msg[] + rmsg[]) per wave -- with it the flagship instance uses 127 of its 128 VGPRs, without
# scratch (the r18 register table) -- and a column pair is formed only while the two
# columns hold at most this many messages together (the committed VT_* pairs hold at most 30: a
# task's accumulators are all live at once).
JOINT_KEPT_CAP = 24
JOINT_PAIR_MSGS = 30
JOINT_STARTS = 4
JOINT_WANDER = 25000
JOINT_THRESHOLD = 400


def load(path):
    with open(path) as f:
        return [[int(float(x)) for x in line.split()] for line in f if line.strip()]


def lpt(tasks, cost, w):
    order = sorted(range(len(tasks)), key=lambda i: -cost[i])  # stable for ties
    per = [[] for _ in range(w)]
    load_ = [0.0] * w
    for i in order:
        k = min(range(w), key=lambda j: load_[j])
        per[k].append(tasks[i])
        load_[k] += cost[i]
    return [sorted(p) for p in per]


def balance(tasks, cost, w):
    """LPT, then moves / swaps of single tasks between the heaviest wave and the others while the
    heaviest wave's load drops (the phase ends at a barrier: its time is the largest load)."""
    per = lpt(tasks, cost, w)
    c = dict(zip(tasks, cost))
    load = lambda p: sum(c[t] for t in p)
    improved = True
    while improved:
        improved = False
        per.sort(key=load, reverse=True)
        top = per[0]
        best = (load(top), None)
        for q in range(1, w):
            o = per[q]
            for t in top:  # move t from top to o
                m = max(load(top) - c[t], load(o) + c[t])
                if m < best[0] - 1e-9:
                    best = (m, ("move", t, q))
                for u in o:  # swap t and u
                    m = max(load(top) - c[t] + c[u], load(o) - c[u] + c[t])
                    if m < best[0] - 1e-9:
                        best = (m, ("swap", t, q, u))
        if best[1] is not None:
            kind = best[1][0]
            if kind == "move":
                _, t, q = best[1]
                top.remove(t)
                per[q].append(t)
            else:
                _, t, q, u = best[1]
                top.remove(t)
                per[q].remove(u)
                top.append(u)
                per[q].append(t)
            improved = True
    return [sorted(p) for p in per]


def arr(name, vals):
    vals = list(vals) or [0]
    body = ", ".join(str(v) for v in vals)
    return f"    static constexpr int {name}[{len(vals)}] = {{{body}}};\n"


def reg_edge_schedule(blocks, z, mb, dv, row_ptr, rcost, sched, cap):
    """The register-edge schedule (RE_* arrays).

    Checks are anonymous: relabelling the Z checks of block row r by an offset rho_r turns every
    shift s of the row into (s + rho_r) mod Z and leaves the code, every variable's ascending
    block-row order and every row's column order as they are.  An edge whose normalised shift is 0
    joins check lane k to variable lane k of the same frame; when its row and its column are also
    on the same wave (and the column has a slot, degree >= 2) its message can stay in one VGPR of
    that lane for the whole decode.

    Chooses rho_r and the wave of every row for the given variable schedule `sched`: most
    register edges (at most `cap` per wave), then the smallest modelled makespan of both phases
    (rcost and var_task_cost, minus the LDS terms of register edges), then the fewest distinct
    rotations (rot[] VGPRs; largest wave first, then the sum).  Restricted LPT start, then
    single-row changes and wave swaps of two rows while the key improves: deterministic.
    Returns (rho, rows per wave, register edges per wave as block indices in row order)."""
    colwave = {}
    for w, p in enumerate(sched):
        for a, b in p:
            colwave[a] = w
            if b >= 0:
                colwave[b] = w
    vbase = [sum(var_task_cost(dv[a], dv[b] if b >= 0 else 0) for a, b in p) for p in sched]
    edges = [list(range(row_ptr[r], row_ptr[r + 1])) for r in range(mb)]
    slot_edges = [[i for i in edges[r] if dv[blocks[i][1]] >= 2] for r in range(mb)]
    rhos = [sorted({0} | {(-blocks[i][2]) % z for i in slot_edges[r]}) for r in range(mb)]
    elig = {(r, rho, w): [i for i in slot_edges[r] if (blocks[i][2] + rho) % z == 0 and colwave[blocks[i][1]] == w]
            for r in range(mb) for rho in rhos[r] for w in range(W)}
    col_edges = [[i for i in range(len(blocks)) if dv[blocks[i][1]] >= 2 and colwave[blocks[i][1]] == w]
                 for w in range(W)]

    def regs(rho, wave):
        reg = [[] for _ in range(W)]
        for r in range(mb):
            reg[wave[r]] += elig[(r, rho[r], wave[r])]
        return [x[:cap] for x in reg]

    def loads(wave, reg):
        chk = [0.0] * W
        for r in range(mb):
            chk[wave[r]] += rcost[r]
        chk = [chk[w] - CHK_EDGE_LDS * len(reg[w]) for w in range(W)]
        var = [vbase[w] - 2 * VAR_EDGE_LDS * len(reg[w]) for w in range(W)]
        return chk, var

    def rotations(rho, wave, reg):
        out = []
        for w in range(W):
            inreg = set(reg[w])
            s = {(blocks[i][2] + rho[blocks[i][0]]) % z for i in col_edges[w] if i not in inreg}
            for r in range(mb):
                if wave[r] == w:
                    s |= {(-(blocks[i][2] + rho[r])) % z for i in slot_edges[r] if i not in inreg}
            out.append(len(s))
        return out

    def key2(rho, wave):
        reg = regs(rho, wave)
        chk, var = loads(wave, reg)
        return (-sum(len(x) for x in reg), round(max(chk) + max(var), 6))

    def better(rho, wave, cur):
        """full key of (rho, wave) if it beats cur, else None; rotations only counted on a tie"""
        k = key2(rho, wave)
        if k > cur[:2]:
            return None
        rot = rotations(rho, wave, regs(rho, wave))
        full = k + (max(rot), sum(rot))
        return full if full < cur else None

    # restricted LPT: heaviest row first, onto the lightest wave that gives it a register edge
    rho, wave = [0] * mb, [-1] * mb
    load, used = [0.0] * W, [0] * W
    for r in sorted(range(mb), key=lambda q: -rcost[q]):
        opts = [(load[w], -len(elig[(r, h, w)]), w, h) for w in range(W) for h in rhos[r]
                if elig[(r, h, w)] and used[w] < cap]
        if opts:
            _, n, w, h = min(opts)
        else:
            w, h, n = min(range(W), key=lambda j: load[j]), 0, 0
        rho[r], wave[r] = h, w
        load[w] += rcost[r]
        used[w] += -n
    k0 = key2(rho, wave)
    rot0 = rotations(rho, wave, regs(rho, wave))
    cur = k0 + (max(rot0), sum(rot0))
    improved = True
    while improved:
        improved = False
        for r in range(mb):
            keep = (rho[r], wave[r])
            best = None
            for w in range(W):
                for h in rhos[r]:
                    if (h, w) == keep:
                        continue
                    rho[r], wave[r] = h, w
                    k = better(rho, wave, best[0] if best else cur)
                    if k is not None:
                        best = (k, h, w)
            rho[r], wave[r] = keep
            if best:
                cur, rho[r], wave[r] = best
                improved = True
        for r in range(mb):
            for q in range(r + 1, mb):
                if wave[r] == wave[q]:
                    continue
                keep = (rho[r], wave[r], rho[q], wave[q])
                wave[r], wave[q] = wave[q], wave[r]
                # each row's own best offset on its new wave (most eligible edges, smallest first)
                rho[r] = min(rhos[r], key=lambda h: (-len(elig[(r, h, wave[r])]), h))
                rho[q] = min(rhos[q], key=lambda h: (-len(elig[(q, h, wave[q])]), h))
                k = better(rho, wave, cur)
                if k is not None:
                    cur = k
                    improved = True
                else:
                    rho[r], wave[r], rho[q], wave[q] = keep
    reg = regs(rho, wave)
    chk, var = loads(wave, reg)
    info = {"chk": chk, "var": var, "rot": rotations(rho, wave, reg)}
    return rho, [[r for r in range(mb) if wave[r] == w] for w in range(W)], reg, info


def operand_table(blocks, slot, rowwave, colwave, ridx, tidx):
    """LDS operands per wave and iteration: what the wave's LDS instructions
    send to the CU's LDS unit.  A slot edge sends 2 per phase (the read's address VGPR and the
    ds_write_addtid_b32's data VGPR), a rotated edge 1 (the swizzle's data VGPR), a register edge
    none; the check phase counts an edge on its row's wave, the variable phase on its column's."""
    chk, var = [0] * W, [0] * W
    for i, (r, c, _) in enumerate(blocks):
        if slot[i] < 0:
            continue
        n = 0 if ridx[i] >= 0 else (1 if tidx[i] >= 0 else 2)
        chk[rowwave[r]] += n
        var[colwave[c]] += n
    return chk, var


def wave_tasks(cols, dv):
    """The variable tasks of one wave's columns by the pairing rule of var_schedule: the columns
    sorted by degree, every pattern of pairing neighbours in that order (a pair holds at most
    JOINT_PAIR_MSGS messages), the least modelled cost wins (ties: the first pattern, lone columns
    first).  Returns ([(A, B or -1)] sorted, the tasks' modelled VALU load)."""
    cols = sorted(cols, key=lambda c: (-dv[c], c))
    n = len(cols)

    def pats(i):
        if i >= n:
            return [[]]
        out = [[(cols[i], -1)] + p for p in pats(i + 1)]
        if i + 1 < n and dv[cols[i]] + dv[cols[i + 1]] <= JOINT_PAIR_MSGS:
            out += [[(cols[i], cols[i + 1])] + p for p in pats(i + 2)]
        return out
    best = None
    for pat in pats(0):
        cost = sum(var_task_cost(dv[a], dv[b] if b >= 0 else 0) for a, b in pat)
        if best is None or cost < best[0] - 1e-9:
            best = (cost, pat)
    return sorted(best[1]), sum(var_task_valu(dv[a], dv[b] if b >= 0 else 0) for a, b in best[1])


def var_task_valu(DA, DB):
    """modelled VALU load of a variable task: var_task_ops's adds at var_task_cost's unit costs"""
    pk, sc, _, _, _ = var_task_ops(DA, DB)
    return 8.21 * pk + 4.85 * sc


def joint_schedule(blocks, z, mb, nb, dv, slot, rcost, old_rowwave, old_colwave, cap):
    """The joint schedule (RE_J_* arrays): block rows and slot-bearing columns are put on the waves
    together, so that what the phases' time follows -- the LDS operands of operand_table -- is what
    the search minimises, where var_schedule balances a cost fit and reg_edge_schedule then counts
    shift-0 edges only.

    Given the waves, rho_r turns the shift that most of row r's same-wave slot edges share into 0
    (ties: the smallest offset): those edges are register edges, the row's other same-wave edges
    rotated edges.  A wave keeps at most `cap` of them (msg[] + rmsg[]): past it the last rotated
    edges in row order, then the last register edges, stay slot edges.

    Key, smallest first: max over waves of the check operands + max of the variable operands; total
    operands; the spread (max - min) of the modelled VALU loads of both phases (rcost; var_task_valu
    over wave_tasks).  The modelled VALU load is a key, not a bound: with the heaviest wave of each
    phase held to the committed schedule's excess over the mean (check 0.9 %, variable 13.9 %) the
    same search ends at 108 / 410 operands (max + max / total) for BG2 Z=32 against the committed
    115 / 420, without it at 98 / 380, and the phases' time follows the operands, not that load
    (DESIGN.md 3.1, r17 and r18).
    Starts: the committed schedule, then JOINT_STARTS - 1 shuffles from a fixed linear congruential
    sequence; from each, wander() and then first-improvement passes over single moves of a row or a
    column and swaps of two rows or two columns until none improves the key.  Between the starts'
    results the number of rot[] entries of the four waves breaks a tie of the key.  Deterministic.
    Returns a dict: rho, rowwave, colwave, reg / rot (edge indices per wave in row order), tasks."""
    vcols = [c for c in range(nb) if dv[c] >= 2]
    redges = [[(i, c, s) for i, (q, c, s) in enumerate(blocks) if q == r and slot[i] >= 0] for r in range(mb)]
    rows_of = {c: sorted({r for r in range(mb) for _, cc, _ in redges[r] if cc == c}) for c in vcols}

    def row_choice(r, w, cw):
        """(rho, register edges, rotated edges) of row r on wave w, edge indices in row order"""
        same = [(i, s) for i, c, s in redges[r] if cw[c] == w]
        if not same:
            return 0, [], []
        cnt = {}
        for _, s in same:
            cnt[s] = cnt.get(s, 0) + 1
        s0 = min(cnt, key=lambda s: (-cnt[s], (-s) % z))
        return (-s0) % z, [i for i, s in same if s == s0], [i for i, s in same if s != s0]

    def row_entry(r, w, cw):
        _, reg, rot = row_choice(r, w, cw)
        var = [0] * W
        for _, c, _ in redges[r]:
            if cw[c] != w:
                var[cw[c]] += 2
        var[w] += len(rot)
        return 2 * (len(redges[r]) - len(reg) - len(rot)) + len(rot), var, len(reg), len(rot)

    tasks_memo = {}

    def var_valu(cw):
        out = []
        for w in range(W):
            k = tuple(c for c in vcols if cw[c] == w)
            if k not in tasks_memo:
                tasks_memo[k] = wave_tasks(k, dv)[1] if k else 0.0
            out.append(tasks_memo[k])
        return out

    # row costs in integer thousandths: sums kept up to date move by move stay exact
    rc = [int(round(1000 * x)) for x in rcost]

    def place(acc, r, w, tab, sign):
        """add (sign = 1) or take away (-1) row r on wave w: acc = [chk, var, nreg, nrot, cv]"""
        e = tab[r][w]
        acc[0][w] += sign * e[0]
        for q in range(W):
            acc[1][q] += sign * e[1][q]
        acc[2][w] += sign * e[2]
        acc[3][w] += sign * e[3]
        acc[4][w] += sign * rc[r]

    def sums(rw, tab):
        acc = [[0] * W for _ in range(5)]
        for r in range(mb):
            place(acc, r, rw[r], tab, 1)
        return acc

    def key_of(acc, vv):
        chk, var, nreg, nrot, cv = acc
        mc, mv, tot, sq = 0, 0, 0, 0
        for w in range(W):  # past the cap: rotated edges first, then register edges, stay slot edges
            d = nreg[w] + nrot[w] - cap
            back = min(d, nrot[w]) + 2 * max(0, d - nrot[w]) if d > 0 else 0
            c, v = chk[w] + back, var[w] + back
            mc, mv, tot, sq = max(mc, c), max(mv, v), tot + c + v, sq + c * c + v * v
        return (mc + mv, tot, round((max(cv) - min(cv)) / 1000 + max(vv) - min(vv), 6)), sq

    def key(rw, cw, tab):
        return key_of(sums(rw, tab), var_valu(cw))[0]

    def table(cw, rows=None, tab=None):
        tab = [None] * mb if tab is None else tab
        for r in (range(mb) if rows is None else rows):
            tab[r] = [row_entry(r, w, cw) for w in range(W)]
        return tab

    def descend(rw, cw):
        tab = table(cw)
        cur = key(rw, cw, tab)
        improved = True
        while improved:
            improved = False
            for r in range(mb):  # a row to another wave
                for w in range(W):
                    if w == rw[r]:
                        continue
                    keep, rw[r] = rw[r], w
                    k = key(rw, cw, tab)
                    if k < cur:
                        cur, improved = k, True
                    else:
                        rw[r] = keep
            for r in range(mb):  # two rows change places
                for q in range(r + 1, mb):
                    if rw[r] == rw[q]:
                        continue
                    rw[r], rw[q] = rw[q], rw[r]
                    k = key(rw, cw, tab)
                    if k < cur:
                        cur, improved = k, True
                    else:
                        rw[r], rw[q] = rw[q], rw[r]
            for c in vcols:  # a column to another wave
                for w in range(W):
                    if w == cw[c]:
                        continue
                    keep, cw[c] = cw[c], w
                    saved = [tab[r] for r in rows_of[c]]
                    table(cw, rows_of[c], tab)
                    k = key(rw, cw, tab)
                    if k < cur:
                        cur, improved = k, True
                    else:
                        cw[c] = keep
                        for r, e in zip(rows_of[c], saved):
                            tab[r] = e
            for x, c in enumerate(vcols):  # two columns change places
                for d in vcols[x + 1:]:
                    if cw[c] == cw[d]:
                        continue
                    touched = sorted(set(rows_of[c]) | set(rows_of[d]))
                    saved = [tab[r] for r in touched]
                    cw[c], cw[d] = cw[d], cw[c]
                    table(cw, touched, tab)
                    k = key(rw, cw, tab)
                    if k < cur:
                        cur, improved = k, True
                    else:
                        cw[c], cw[d] = cw[d], cw[c]
                        for r, e in zip(touched, saved):
                            tab[r] = e
        return cur

    def classify(rw, cw):
        rho, reg, rot = [0] * mb, [[] for _ in range(W)], [[] for _ in range(W)]
        for r in range(mb):
            rho[r], a, b = row_choice(r, rw[r], cw)
            reg[rw[r]] += a
            rot[rw[r]] += b
        for w in range(W):
            rot[w] = rot[w][:max(0, cap - min(cap, len(reg[w])))]
            reg[w] = reg[w][:cap]
        return rho, reg, rot

    def rotations(rw, cw):
        rho, reg, rot = classify(rw, cw)
        n = 0
        for w in range(W):
            kept = set(reg[w]) | set(rot[w])
            s = set()
            for i, (r, c, sh) in enumerate(blocks):
                if slot[i] < 0 or i in kept:
                    continue
                if cw[c] == w:
                    s.add((sh + rho[r]) % z)
                if rw[r] == w:
                    s.add((-(sh + rho[r])) % z)
            n += len(s)
        return n

    state = [0x9E3779B97F4A7C15]

    def rnd(n):
        state[0] = (state[0] * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        return (state[0] >> 33) % n

    def shuffled(items):
        items = list(items)
        for i in range(len(items) - 1, 0, -1):
            j = rnd(i + 1)
            items[i], items[j] = items[j], items[i]
        return items

    def wander(rw, cw):
        """Threshold accepting before the descent: JOINT_WANDER random single moves and swaps, one
        in eight on columns, each taken when the sum over waves and phases of the squared operands (a
        smooth stand-in for max + max and total together) rises by no more than a threshold that
        falls from JOINT_THRESHOLD to 0 (integers only).  Leaves the state with the best (max + max,
        total) met in rw / cw."""
        tab = table(cw)
        acc, vv = sums(rw, tab), var_valu(cw)
        k, cur = key_of(acc, vv)
        best = (k[:2], list(rw), dict(cw))

        def set_rows(rows, waves):
            for r, w in zip(rows, waves):
                place(acc, r, rw[r], tab, -1)
                rw[r] = w
                place(acc, r, w, tab, 1)

        def set_cols(cols, waves):
            touched = sorted({r for c in cols for r in rows_of[c]})
            for r in touched:
                place(acc, r, rw[r], tab, -1)
            for c, w in zip(cols, waves):
                cw[c] = w
            table(cw, touched, tab)
            for r in touched:
                place(acc, r, rw[r], tab, 1)

        for t in range(JOINT_WANDER):
            thr = JOINT_THRESHOLD * (JOINT_WANDER - t) // JOINT_WANDER
            kind = rnd(16)
            if kind < 14:  # rows: a move (kind < 7) or a swap
                r, q = rnd(mb), rnd(mb)
                keep = (rw[r], rw[q])
                new = (rnd(W), rw[q]) if kind < 7 else (rw[q], rw[r])
                if new == keep or r == q:
                    continue
                set_rows((r, q), new)
                k, sq = key_of(acc, vv)
                if sq <= cur + thr:
                    cur = sq
                else:
                    set_rows((r, q), keep)
                    continue
            else:  # columns: a move (kind 14) or a swap
                c, d = vcols[rnd(len(vcols))], vcols[rnd(len(vcols))]
                keep = (cw[c], cw[d])
                new = (rnd(W), cw[d]) if kind == 14 else (cw[d], cw[c])
                if new == keep or c == d:
                    continue
                set_cols((c, d), new)
                keepv, vv = vv, var_valu(cw)
                k, sq = key_of(acc, vv)
                if sq <= cur + thr:
                    cur = sq
                else:
                    set_cols((c, d), keep)
                    vv = keepv
                    continue
            if k[:2] < best[0]:
                best = (k[:2], list(rw), dict(cw))
        rw[:] = best[1]
        cw.update(best[2])

    best = None
    for start in range(JOINT_STARTS):
        if start == 0:
            rw, cw = list(old_rowwave), dict(old_colwave)
        else:  # columns and rows dealt round the waves in a shuffled order
            cw = {c: x % W for x, c in enumerate(shuffled(vcols))}
            rw = [0] * mb
            for x, r in enumerate(shuffled(range(mb))):
                rw[r] = x % W
        wander(rw, cw)
        k = descend(rw, cw) + (rotations(rw, cw),)
        if best is None or k < best[0]:
            best = (k, list(rw), dict(cw))
    _, rw, cw = best
    rho, reg, rot = classify(rw, cw)
    return {"rho": rho, "rowwave": rw, "colwave": cw, "reg": reg, "rot": rot, "key": best[0],
            "tasks": [wave_tasks([c for c in vcols if cw[c] == w], dv)[0] if any(cw[c] == w for c in vcols) else []
                      for w in range(W)]}


_joint_memo = {}


def gen(name, base, z, reg_edges=True, cap=None, report=None, joint_cap=None):
    mb, nb = len(base), len(base[0])
    blocks = [(r, c, base[r][c] % z) for r in range(mb) for c in range(nb) if base[r][c] >= 0]
    dv = [0] * nb
    dc = [0] * mb
    for r, c, _ in blocks:
        dv[c] += 1
        dc[r] += 1
    slot = []
    n = 0
    for r, c, _ in blocks:
        if dv[c] >= 2:
            slot.append(n)
            n += 1
        else:
            slot.append(-1)
    row_ptr = [0]
    for r in range(mb):
        row_ptr.append(row_ptr[-1] + dc[r])
    rows = list(range(mb))
    nslot = [sum(1 for i in range(row_ptr[r], row_ptr[r + 1]) if slot[i] >= 0) for r in rows]
    # per-iteration SIMD pipe cycles of one wave's share (tools/ubench costs at 4 waves / SIMD):
    # check row: the two minima (half-rate min / med3), sign parity, per slot edge compare +
    # select + sign, row constants; column: the exclusive ordered sums (full-rate adds) + its LDS
    # reads / writes issued.  Rows of degree <= DIRECT_DC take the direct form (direct_row_cost).
    rcost = [direct_row_cost(dc[r], nslot[r]) if 2 <= dc[r] <= DIRECT_DC else
             4.1 * n_min_ops(dc[r]) + 2.2 * (dc[r] // 2) + 10.4 * nslot[r] + 12 + 2.0 * dc[r] for r in rows]
    vcols = [c for c in range(nb) if dv[c] != 1]
    chk = balance(rows, rcost, W)
    vt = var_schedule(vcols, dv, W)
    bw = lpt(list(range(nb)), [1.0] * nb, W)
    col_blocks = [[i for i, b in enumerate(blocks) if b[1] == c] for c in range(nb)]
    col_ptr = [0]
    col_slot, col_shift = [], []
    for c in range(nb):
        for i in col_blocks[c]:
            col_slot.append(slot[i])
            col_shift.append(blocks[i][2])
        col_ptr.append(len(col_slot))

    def flat(lists):
        ptr = [0]
        out = []
        for l in lists:
            out += l
            ptr.append(len(out))
        return ptr, out

    cp, cl = flat(chk)
    bp, bl = flat(bw)
    s = f"struct {name} {{\n"
    s += f"    static constexpr int Z = {z}, Mb = {mb}, Nb = {nb}, N = {nb * z}, NSLOTS = {n}, W = {W};\n"
    s += f"    static constexpr int NBLOCKS = {len(blocks)};\n"
    s += arr("BLK_ROW", [b[0] for b in blocks])
    s += arr("BLK_COL", [b[1] for b in blocks])
    s += arr("BLK_SHIFT", [b[2] for b in blocks])
    s += arr("ROW_PTR", row_ptr)
    s += arr("ROW_SLOT", slot)
    s += arr("ROW_COL", [b[1] for b in blocks])
    s += arr("ROW_SHIFT", [b[2] for b in blocks])
    s += arr("COL_PTR", col_ptr)
    s += arr("COL_SLOT", col_slot)
    s += arr("COL_SHIFT", col_shift)
    s += arr("CHK_PTR", cp)
    s += arr("CHK_ROWS", cl)
    # per wave: the distinct columns of its tasks (LLRs, init, shifts), then the tasks (column A,
    # column B or -1: a pair shares v_pk_add_f32)
    vp, vl = flat([sorted({t[0] for t in p} | {t[1] for t in p if t[1] >= 0}) for p in vt])
    tp, tl = flat(vt)
    s += arr("VT_COL_PTR", vp)
    s += arr("VT_COLS", vl)
    s += arr("VT_PTR", tp)
    s += arr("VT_A", [t[0] for t in tl])
    s += arr("VT_B", [t[1] for t in tl])
    s += arr("BW_PTR", bp)
    s += arr("BW_COLS", bl)
    if reg_edges:
        # the register-edge schedule beside the one above (reg_edge_schedule): offsets, normalised
        # shifts in the order of ROW_SHIFT / COL_SHIFT, per edge the index into the wave's msg[]
        # (-1: the message lives in its LDS slot), rows per wave.  Columns stay on VT's waves.
        cap = REG_EDGE_CAP if cap is None else cap
        rho, rchk, reg, info = reg_edge_schedule(blocks, z, mb, dv, row_ptr, rcost, vt, cap)
        rshift = [(b[2] + rho[b[0]]) % z for b in blocks]
        ridx = [-1] * len(blocks)
        for w in range(W):
            for x, i in enumerate(reg[w]):
                ridx[i] = x
        rp, rl = flat(rchk)
        s += f"    static constexpr int RE_CAP = {cap};\n"
        s += arr("RE_RHO", rho)
        s += arr("RE_ROW_SHIFT", rshift)
        s += arr("RE_COL_SHIFT", [rshift[i] for c in range(nb) for i in col_blocks[c]])
        s += arr("RE_ROW_REG", ridx)
        s += arr("RE_COL_REG", [ridx[i] for c in range(nb) for i in col_blocks[c]])
        s += arr("RE_NREG", [len(x) for x in reg])
        s += arr("RE_CHK_PTR", rp)
        s += arr("RE_CHK_ROWS", rl)
        # rotated edges: a slot edge outside msg[] whose row and column are on the same wave but
        # whose normalised shift is not 0.  Producer and consumer are the same wave, so the message
        # can move between its check lane and its variable lane by one cross-lane rotation inside
        # the Z-lane segment instead of a slot store and a rotated read (flood_fixed.hpp rmsg[]).
        # Per edge the index into the wave's rmsg[] (-1: none), dense per wave in row order.
        rowwave = {r: w for w in range(W) for r in rchk[w]}
        colwave = {c: w for w in range(W) for t in vt[w] for c in t if c >= 0}
        rot = [[i for i, b in enumerate(blocks) if slot[i] >= 0 and ridx[i] < 0 and rshift[i] != 0
                and rowwave[b[0]] == w and colwave[b[1]] == w] for w in range(W)]
        tidx = [-1] * len(blocks)
        for w in range(W):
            for x, i in enumerate(rot[w]):
                tidx[i] = x
        s += arr("RE_ROW_ROT", tidx)
        s += arr("RE_COL_ROT", [tidx[i] for c in range(nb) for i in col_blocks[c]])
        s += arr("RE_NROT", [len(x) for x in rot])
        # the joint schedule (joint_schedule): the same arrays again as RE_J_*, with columns and
        # tasks of its own (RE_J_VT_*: the VT_* layout) and its LDS operands per wave.  An instance
        # of the kernel reads one family or the other (flood_fixed.hpp FxPlan).
        jcap = JOINT_KEPT_CAP if joint_cap is None else joint_cap
        if (name, jcap) not in _joint_memo:
            _joint_memo[(name, jcap)] = joint_schedule(blocks, z, mb, nb, dv, slot, rcost,
                                                       [rowwave[r] for r in range(mb)], colwave, jcap)
        j = _joint_memo[(name, jcap)]
        jshift = [(b[2] + j["rho"][b[0]]) % z for b in blocks]
        jreg, jrot = [-1] * len(blocks), [-1] * len(blocks)
        for w in range(W):
            for x, i in enumerate(j["reg"][w]):
                jreg[i] = x
            for x, i in enumerate(j["rot"][w]):
                jrot[i] = x
        jrp, jrl = flat([[r for r in range(mb) if j["rowwave"][r] == w] for w in range(W)])
        jvp, jvl = flat([sorted(c for t in p for c in t if c >= 0) for p in j["tasks"]])
        jtp, jtl = flat(j["tasks"])
        ops_old = operand_table(blocks, slot, rowwave, colwave, ridx, tidx)
        ops_new = operand_table(blocks, slot, j["rowwave"], j["colwave"], jreg, jrot)
        s += f"    static constexpr int RE_J_CAP = {jcap};\n"
        s += arr("RE_J_RHO", j["rho"])
        s += arr("RE_J_ROW_SHIFT", jshift)
        s += arr("RE_J_COL_SHIFT", [jshift[i] for c in range(nb) for i in col_blocks[c]])
        s += arr("RE_J_ROW_REG", jreg)
        s += arr("RE_J_COL_REG", [jreg[i] for c in range(nb) for i in col_blocks[c]])
        s += arr("RE_J_NREG", [len(x) for x in j["reg"]])
        s += arr("RE_J_CHK_PTR", jrp)
        s += arr("RE_J_CHK_ROWS", jrl)
        s += arr("RE_J_ROW_ROT", jrot)
        s += arr("RE_J_COL_ROT", [jrot[i] for c in range(nb) for i in col_blocks[c]])
        s += arr("RE_J_NROT", [len(x) for x in j["rot"]])
        s += arr("RE_J_VT_COL_PTR", jvp)
        s += arr("RE_J_VT_COLS", jvl)
        s += arr("RE_J_VT_PTR", jtp)
        s += arr("RE_J_VT_A", [t[0] for t in jtl])
        s += arr("RE_J_VT_B", [t[1] for t in jtl])
        s += arr("RE_J_OPS_CHK", ops_new[0])
        s += arr("RE_J_OPS_VAR", ops_new[1])
        if report is not None:
            report[name + " LDS operands"] = {"old chk": ops_old[0], "old var": ops_old[1],
                                              "old max+max, total": [max(ops_old[0]) + max(ops_old[1]), sum(ops_old[0]) + sum(ops_old[1])],
                                              "joint chk": ops_new[0], "joint var": ops_new[1],
                                              "joint max+max, total": [max(ops_new[0]) + max(ops_new[1]), sum(ops_new[0]) + sum(ops_new[1])],
                                              "joint nreg": [len(x) for x in j["reg"]], "joint nrot": [len(x) for x in j["rot"]],
                                              "joint columns": [sorted(c for c in j["colwave"] if j["colwave"][c] == w) for w in range(W)],
                                              "joint key": list(j["key"])}
        if report is not None:
            c = dict(zip(rows, rcost))
            report[name] = dict(info, rho=rho, nreg=[len(x) for x in reg], rows=rchk,
                                chk_old=[sum(c[r] for r in p) for p in chk],
                                var_old=[sum(var_task_cost(dv[a], dv[b] if b >= 0 else 0) for a, b in p) for p in vt])
    s += "};\n\n"
    return s


def n_min_ops(d):
    """half-rate min / med3 ops for the two smallest of d magnitudes (flood_dev.hpp two_smallest)"""
    if d <= 1:
        return 0
    if d == 2:
        return 2
    return 2 + 5 * ((d - 3) // 3) + 2 * ((d - 3) % 3)


def direct_row_cost(d, nout):
    """SIMD pipe cycles of a min-sum row of degree d <= DIRECT_DC with nout outputs in the direct
    form (flood_fixed.hpp direct_row), same unit costs as above: 4.1 per half-rate min / minimum3,
    2.2 per full-rate multiply / xor / bitop3, 2.0 per edge.
    d <= 4: per output a minimum over the other inputs, their sign xor, alpha * min, sign merge.
    d >= 5: per row d // 2 pair minima, the parity (one 3-input xor per two inputs) and alpha's
    sign; per output one minimum3, the product and the sign merge."""
    if d <= 4:
        row, out = 0.0, (4.1 if d >= 3 else 0.0) + (2.2 if d >= 3 else 0.0) + 2 * 2.2
    else:
        row, out = 4.1 * (d // 2) + 2.2 * (d // 2) + 2.2, 4.1 + 2 * 2.2
    return row + out * nout + 2.0 * d


def var_task_ops(DA, DB):
    """Instruction counts of a variable task (flood_fixed.hpp FixedBody::task): every output of
    column A (degree DA) and, when DB > 0, of column B (degree DB <= DA) on v_pk_add_f32 pairs.
    Per output e: acc[e] = P_e, then + c_J for J = e + 1 .. D - 1 (the reference's ascending
    exclusive sum, traditional_decoders.py:235-250); the prefix adds P_J -> P_{J+1} run to the APP
    (the column's last prefix).  Returns (pk adds, scalar adds, LDS reads, LDS writes, APPs)."""
    pk = sc = 0
    for J in range(DA):  # c_J goes to the outputs e < J and to the prefix
        if J < DB:
            pk += J + 1
        else:
            sc += J + 1
    return pk, sc, DA + DB, DA + DB, 1 + int(DB > 0)


def var_task_cost(DA, DB):
    """Modelled cycles of a variable task: the r04 least-squares fit over the phase times of the
    schedules of that time (profiles/r04_flood_timeline_*): 8.2 per v_pk_add_f32, 4.85 per
    v_add_f32, 18.1 per LDS read or write, 33.6 per task.  It only orders the schedules the search
    compares and it pins the committed one (VT_*, RE_NREG); it is NOT the kernel's cost any more.
    The fit predates own-lane stores, register edges and direct rows: measured on the kernel as it
    is the four waves' variable phases are 2 327 / 2 666 / 2 161 /
    2 612 cycles where this model says 2 525 / 2 520 / 2 518 / 2 385, a wave's time follows what its
    LDS instructions send to the LDS unit (address and data VGPRs, shared by the CU's 16 waves), and
    the scalar adds of a lone long column are nearly free."""
    pk, sc, rd, wr, apps = var_task_ops(DA, DB)
    return 8.21 * pk + 4.85 * sc + 18.12 * (rd + wr) + 33.6


def var_schedule(vcols, dv, w):
    """Variable tasks per wave.  Columns sorted by degree; every pattern of pairing neighbours in
    that order (a pair's exclusive sums share v_pk_add_f32 instructions, the smaller column's adds
    riding along for free), each balanced over the waves (LPT + move / swap refinement); the
    smallest makespan wins (ties: least total cost).  A column is always one task on one wave:
    every output reads all of the column's messages and is written in place, so a split column's
    writes would race the other reads within the phase.
    Returns [[(A, B or -1)]] per wave."""
    cols = sorted(vcols, key=lambda c: (-dv[c], c))
    n = len(cols)

    def pats(i):
        if i >= n:
            return [[]]
        out = [[(cols[i],)] + p for p in pats(i + 1)]
        if i + 1 < n:
            out += [[(cols[i], cols[i + 1])] + p for p in pats(i + 2)]
        return out
    best = None
    for pat in pats(0):
        t = [(u[0], u[1] if len(u) > 1 else -1) for u in pat]
        cost = [var_task_cost(dv[a], dv[b] if b >= 0 else 0) for a, b in t]
        per = balance(t, cost, w)
        c = dict(zip(t, cost))
        cur = (max(sum(c[x] for x in p) for p in per), sum(cost), per)
        key = (round(cur[0], 6), cur[1])
        if best is None or key < best[0]:
            best = (key, cur[2])
    return [sorted(p) for p in best[1]]


def header_text(reg_edges=True, cap=None, report=None, joint_cap=None):
    """The header's text; reg_edges=False leaves the RE_* arrays out (the schedule before them)."""
    text = ("// GENERATED by tools/gen_fixed_codes.py from codes/NR_2_0_{4,32}.txt -- do not edit.\n"
            "// Compile-time flooding schedules for the two codes the reference ships (see that script).\n"
            "#pragma once\n\nnamespace ldpc {\nnamespace fixed {\n\n")
    for name, path, z in CODES:
        text += gen(name, load(path), z, reg_edges, cap, report, joint_cap)
    text += "}  // namespace fixed\n}  // namespace ldpc\n"
    return text


def main(out):
    # LDPC_REG_EDGE_CAP: a smaller cap for A/B builds (tools/build_variant.sh on a copy of the tree)
    cap = int(os.environ["LDPC_REG_EDGE_CAP"]) if os.environ.get("LDPC_REG_EDGE_CAP") else None
    # LDPC_JOINT_CAP: another cap on the joint schedule's kept messages per wave (register budget)
    jcap = int(os.environ["LDPC_JOINT_CAP"]) if os.environ.get("LDPC_JOINT_CAP") else None
    report = {}
    text = header_text(True, cap, report, jcap)
    if os.environ.get("LDPC_GEN_REPORT"):
        for name, r in report.items():
            print(name, {k: ([round(x, 1) for x in v] if k in ("chk", "var", "chk_old", "var_old") else v)
                         for k, v in r.items()}, file=sys.stderr)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    old = open(out).read() if os.path.exists(out) else None
    if old != text:
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "..", "csrc", "gen", "fixed_codes.hpp"))
