"""Zero messages on the fixed kernel's fast check update (no GPU).

flood_fixed_kernel's min-sum check update comes in an exact form (MinSumStats: torch.sign(0) = 0)
and two fast forms that treat every sign as +-1: the two-minimum / select form and, for rows of
degree 2 .. 6, direct_row.  The kernel takes the fast forms on every row unless a non-finite value
has been seen; a zero message does not send it to the exact form.  This file is why that is right:
a numpy restatement of both fast forms, applied to every row whatever it holds, decodes whole
frames next to a numpy restatement of the reference's update, on inputs chosen so that exact zeros
and ties at the minimum are common.  With every value finite

  * every c2v, v2c and APP of the two decodes is equal up to the sign of a zero, in every iteration;
  * so the bits, the per-frame iteration counts and the error counters are identical;

and the exact restatement is itself bit-for-bit the oracle.  The count of exact-zero v2c over each
run is asserted > 0, so the inputs do exercise the case.
"""
import os

import numpy as np
import pytest

from conftest import PKG, code_path
from reg_edges_util import parse_header

ALPHA = np.float32(0.75)
SIGN = np.uint32(0x80000000)
DIRECT_DC = 6  # LDPC_DIRECT_DC of csrc/flood_fixed.hpp
ITERS = (1, 2, 3, 10)


def u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def f32(x):
    return np.ascontiguousarray(x, dtype=np.uint32).view(np.float32)


# ------------------------------------------------------------------ check rows, x: (..., d) float32
def row_exact(x):
    """traditional_decoders.py:207-232: prod of torch.sign over the others * (alpha * min of the others)"""
    d = x.shape[-1]
    sg, mag = np.sign(x).astype(np.float32), np.abs(x)
    out = np.empty_like(x)
    for e in range(d):
        rest = [q for q in range(d) if q != e]
        s = np.ones(x.shape[:-1], np.float32)
        for q in rest:
            s = s * sg[..., q]
        m = np.full(x.shape[:-1], np.inf, np.float32)
        for q in rest:
            m = np.where(mag[..., q] < m, mag[..., q], m)
        out[..., e] = s * (ALPHA * m)
    return out


def row_select(x):
    """FixedBody::row, two-minimum / select form: s1 / s2 = alpha * m1 / alpha * m2 with the row's
    sign parity, |x_e| == m1 selects s2, the edge's own sign bit is xored back out"""
    d = x.shape[-1]
    mag = np.sort(np.abs(x), axis=-1)
    m1, m2 = mag[..., 0], (mag[..., 1] if d > 1 else np.full(x.shape[:-1], np.inf, np.float32))
    par = np.bitwise_xor.reduce(u32(x), axis=-1) & SIGN
    s1, s2 = u32(ALPHA * m1) ^ par, u32(ALPHA * m2) ^ par
    out = np.empty_like(x)
    for e in range(d):
        sel = np.where(np.abs(x[..., e]) == m1, s2, s1)
        out[..., e] = f32(sel ^ (u32(x[..., e]) & SIGN))
    return out


def row_direct(x):
    """direct_row: output e from the other inputs alone.  d <= 4: alpha * min with the xor of the
    others' sign bits; d >= 5: the row's parity goes into alpha's sign, the edge's own bit comes out"""
    d = x.shape[-1]
    assert 2 <= d <= DIRECT_DC
    mag, bits = np.abs(x), u32(x)
    out = np.empty_like(x)
    par = np.bitwise_xor.reduce(bits, axis=-1)
    als = f32(u32(np.broadcast_to(ALPHA, par.shape)) ^ (par & SIGN))
    for e in range(d):
        rest = [q for q in range(d) if q != e]
        m = mag[..., rest[0]]
        for q in rest[1:]:
            m = np.minimum(m, mag[..., q])
        if d <= 4:
            sx = np.bitwise_xor.reduce(bits[..., rest], axis=-1)
            out[..., e] = f32(u32(ALPHA * m) ^ (sx & SIGN))
        else:
            out[..., e] = f32(u32(als * m) ^ (bits[..., e] & SIGN))
    return out


def row_fast(x):
    """the form the kernel takes for a row of this degree"""
    return row_direct(x) if 2 <= x.shape[-1] <= DIRECT_DC else row_select(x)


def same_up_to_zero_sign(a, b):
    return bool(np.isfinite(a).all() and np.isfinite(b).all() and np.array_equal(a, b))  # -0.0 == 0.0


@pytest.mark.parametrize("d", range(2, 11))
def test_fast_rows_equal_exact_rows_up_to_zero_sign(d):
    """Rows of degree 2 .. 10 from the grid {-2, -1, -0.0, 0, 1, 2}: every zero / tie pattern."""
    rng = np.random.default_rng(d)
    vals = np.array([-2, -1, -0.0, 0.0, 1, 2], np.float32)
    x = rng.choice(vals, size=(20000, d))
    x[:len(vals) ** min(d, 4)] = 0  # plus every combination of the first (up to) four inputs
    combos = np.stack(np.meshgrid(*[vals] * min(d, 4), indexing="ij"), -1).reshape(-1, min(d, 4))
    x[:len(combos), :min(d, 4)] = combos
    assert (x == 0).sum(-1).max() >= 2 and ((x == 0).sum(-1) == 1).any()
    ref = row_exact(x)
    forms = [row_select] + ([row_direct] if d <= DIRECT_DC else [])
    for form in forms:
        out = form(x)
        assert same_up_to_zero_sign(out, ref), form.__name__
        nz = ref != 0
        assert np.array_equal(u32(out)[nz], u32(ref)[nz]), form.__name__  # non-zero outputs: bit for bit


# ------------------------------------------------------------------ whole decodes
class Model:
    """Flooding scaled min-sum on the oracle's graph, rows / columns batched by degree."""

    def __init__(self, g):
        self.g = g
        dc, dv = np.diff(g.chk_ptr), np.diff(g.var_ptr)
        self.rows = {int(d): (g.chk_ptr[:-1][dc == d][:, None] + np.arange(d)[None, :]) for d in np.unique(dc)}
        # a variable's edges in ascending check order (traditional_decoders.py:235-250)
        self.cols = {int(d): (np.flatnonzero(dv == d), g.var_edge[g.var_ptr[:-1][dv == d][:, None] + np.arange(d)[None, :]])
                     for d in np.unique(dv)}

    def check(self, v2c, form):
        c2v = np.empty_like(v2c)
        for d, idx in self.rows.items():
            c2v[:, idx] = form(v2c[:, idx])
        return c2v

    def var(self, llr, c2v):
        """v2c_e = ((llr + c_0) + c_1) ... over e' != e in ascending check order; APP over all"""
        v2c, app = np.empty_like(c2v), np.empty_like(llr)
        for d, (vars_, idx) in self.cols.items():
            c = c2v[:, idx]
            for e in range(d):
                acc = llr[:, vars_].copy()
                for q in range(d):
                    if q != e:
                        acc = acc + c[..., q]
                v2c[:, idx[:, e]] = acc
            acc = llr[:, vars_].copy()
            for q in range(d):
                acc = acc + c[..., q]
            app[:, vars_] = acc
        return v2c, app

    def valid(self, bits):
        par = np.bitwise_xor.reduceat(bits[:, self.g.edge_var], self.g.chk_ptr[:-1], axis=1)
        return ~par.any(axis=1)

    def trace(self, llr, iters, form):
        """per iteration: (c2v, v2c, APP)"""
        v2c = llr[:, self.g.edge_var].copy()
        out = []
        for _ in range(iters):
            c2v = self.check(v2c, form)
            v2c, app = self.var(llr, c2v)
            out.append((c2v, v2c, app))
        return out

    def result(self, tr, per_frame):
        """bits, per-frame iteration counts (the oracle's modes 0 and 2)"""
        iters = len(tr)
        bits = (tr[-1][2] < 0).astype(np.uint8)
        it = np.full(bits.shape[0], iters, np.int32)
        if per_frame:
            done = np.zeros(bits.shape[0], bool)
            for t, (_, _, app) in enumerate(tr):
                b = (app < 0).astype(np.uint8)
                new = self.valid(b) & ~done
                bits[new], it[new] = b[new], t + 1
                done |= new
        return bits, it


def counters(bits, it):
    return [int(bits.sum()), int((bits.sum(1) > 0).sum()), bits.shape[0], int(it.sum())]


def frames(z, tab):
    """12 frames of LLRs k / 4, |k| <= 12 (with alpha = 0.75 sums cancel exactly and minima tie all
    the time); the last six with whole columns at zero: columns with slots only, columns that own a
    register edge, degree-1 columns, then all three kinds, a frame of zeros and one of -0.0"""
    rng = np.random.default_rng(4000 + z)
    n = tab["Nb"] * z
    x = (rng.integers(-12, 13, size=(12, n)) / 4).astype(np.float32)
    dv = np.diff(tab["COL_PTR"])
    reg = sorted({tab["BLK_COL"][e] for e, r in enumerate(tab["RE_ROW_REG"]) if r >= 0})
    slot = [c for c in range(tab["Nb"]) if dv[c] >= 2 and c not in reg]
    deg1 = [c for c in range(tab["Nb"]) if dv[c] == 1]
    assert reg and slot and deg1

    def zero(f, cols, v=0.0):
        for c in cols:
            x[f, c * z:(c + 1) * z] = v

    zero(6, slot[::2])
    zero(7, reg[::2])
    zero(8, deg1[::2])
    zero(9, slot[1::3] + reg[1::3] + deg1[1::3])
    zero(10, range(tab["Nb"]))
    zero(11, reg[::3] + deg1[::3], -0.0)
    return x


@pytest.fixture(scope="module")
def setups(oracle_mod):
    with open(os.path.join(PKG, "csrc", "gen", "fixed_codes.hpp")) as f:
        tabs = parse_header(f.read())
    out = {}
    for z in (4, 32):
        g = oracle_mod.Graph(oracle_mod.expand(oracle_mod.load_base(code_path(z)), z))
        llr = frames(z, tabs[f"BG2_Z{z}"])
        llr.setflags(write=False)
        m = Model(g)
        out[z] = (g, m, llr, m.trace(llr, max(ITERS), row_exact), m.trace(llr, max(ITERS), row_fast))
    return out


@pytest.mark.parametrize("z", (4, 32))
def test_zeros_stay_on_the_fast_path(oracle_mod, setups, z):
    g, m, llr, exact, fast = setups[z]
    zero_v2c = zero_c2v = 0
    for t, ((c0, v0, a0), (c1, v1, a1)) in enumerate(zip(exact, fast)):
        assert same_up_to_zero_sign(c0, c1), (z, t, "c2v")
        assert same_up_to_zero_sign(v0, v1), (z, t, "v2c")
        assert same_up_to_zero_sign(a0, a1), (z, t, "APP")
        zero_v2c += int((v1 == 0).sum())
        zero_c2v += int((c1 == 0).sum())
    print(f"Z={z}: {zero_v2c} exact-zero v2c and {zero_c2v} exact-zero c2v in {len(fast)} iterations of {len(llr)} frames")
    assert zero_v2c > 0 and zero_c2v > 0
    # the frames without zero LLRs make zeros of their own (k / 4 grid, alpha = 3 / 4)
    assert sum(int((v[:6] == 0).sum()) for _, v, _ in fast) > 0
    for iters in ITERS:
        for mode in (0, 2):
            b0, i0 = m.result(exact[:iters], mode == 2)
            b1, i1 = m.result(fast[:iters], mode == 2)
            ob, oa, _, oi = oracle_mod.flood_decode(g, llr, "minsum", iters, float(ALPHA), mode)
            assert np.array_equal(b0, ob) and np.array_equal(i0, oi), (z, iters, mode)  # the restatement is the oracle
            assert np.array_equal(b1, ob) and np.array_equal(i1, oi), (z, iters, mode)
            assert counters(b1, i1) == counters(ob, oi), (z, iters, mode)
            if mode == 0:
                assert np.array_equal(u32(exact[iters - 1][2]), u32(oa)), (z, iters)  # its APP too, bit for bit
                assert same_up_to_zero_sign(fast[iters - 1][2], oa), (z, iters)
