"""The fixed flood kernel's register-edge schedule (gen/fixed_codes.hpp RE_*), no GPU.

tools/gen_fixed_codes.py relabels the Z checks of every block row r by an offset rho_r, which
turns each shift s of the row into (s + rho_r) mod Z, and keeps the message of an edge in a VGPR
when its normalised shift is 0 and its row and column run on the same wave.  Checked here, for both
codes: the tables are what that rule says, the arrays from before the schedule are untouched, and
the relabelled code decodes exactly as the original one (the oracle on both parity-check matrices)."""
import hashlib
import os
import sys

import numpy as np
import pytest

from conftest import PKG, code_path

sys.path.insert(0, os.path.join(PKG, "tools"))
import gen_fixed_codes as gen  # noqa: E402
from reg_edges_util import parse_header  # noqa: E402

HEADER = os.path.join(PKG, "csrc", "gen", "fixed_codes.hpp")
# sha256 of the header as it was before the RE_* arrays were added, less the 18 lines that declared
# the unpaired schedule and the output ranges (those matching r" (VS_\w+|VT_LO|VT_HI)\["), which went
# when the kernel stopped reading them: 57 of that text's 75 lines.  Computed on the last commit that
# emitted them, whose unfiltered gen.header_text(reg_edges=False) hashed to the former constant
# f05a4b70f83e4996ad6feb15d373fd3bf7ccf78a0f17bf735c643dc6d2d107e7.
OLD_HEADER_SHA256 = "547d6bc9bfe13c879be9d87b18d1efe4e2646c1ba1ea7a66694cdb3595b47f67"
CODES = {"BG2_Z4": 4, "BG2_Z32": 32}
W = 4


@pytest.fixture(scope="module")
def header_text():
    with open(HEADER) as f:
        return f.read()


@pytest.fixture(scope="module")
def tables(header_text):
    return parse_header(header_text)


def col_order(t):
    """edge indices (row order) in the order of the COL_* arrays: by column, rows ascending"""
    nb = t["Nb"]
    return [e for c in range(nb) for e in range(t["NBLOCKS"]) if t["BLK_COL"][e] == c]


def waves(ptr, items):
    return {x: w for w in range(W) for x in items[ptr[w]:ptr[w + 1]]}


def test_header_is_the_generator_output(header_text):
    assert header_text == gen.header_text()


def test_old_arrays_are_untouched(header_text):
    old = gen.header_text(reg_edges=False)
    assert hashlib.sha256(old.encode()).hexdigest() == OLD_HEADER_SHA256
    kept = "".join(line for line in header_text.splitlines(keepends=True) if " RE_" not in line)
    assert kept == old
    assert "RE_" not in old


@pytest.mark.parametrize("code", sorted(CODES))
def test_normalised_shifts(tables, code):
    t, z = tables[code], CODES[code]
    assert t["Z"] == z and len(t["RE_RHO"]) == t["Mb"] and all(0 <= r < z for r in t["RE_RHO"])
    want = [(t["ROW_SHIFT"][e] + t["RE_RHO"][t["BLK_ROW"][e]]) % z for e in range(t["NBLOCKS"])]
    assert t["RE_ROW_SHIFT"] == want
    order = col_order(t)
    assert [t["ROW_SHIFT"][e] for e in order] == t["COL_SHIFT"]  # the order itself
    assert t["RE_COL_SHIFT"] == [want[e] for e in order]
    assert t["RE_COL_REG"] == [t["RE_ROW_REG"][e] for e in order]


@pytest.mark.parametrize("code", sorted(CODES))
def test_register_edges(tables, code):
    t = tables[code]
    dv = np.diff(t["COL_PTR"])
    row_wave = waves(t["RE_CHK_PTR"], t["RE_CHK_ROWS"])
    col_wave = waves(t["VT_COL_PTR"], t["VT_COLS"])
    assert sorted(t["RE_CHK_ROWS"]) == list(range(t["Mb"]))  # every row on exactly one wave
    assert t["RE_CAP"] == gen.REG_EDGE_CAP
    per_wave = [[] for _ in range(W)]
    for e, x in enumerate(t["RE_ROW_REG"]):
        if x < 0:
            continue
        r, c = t["BLK_ROW"][e], t["BLK_COL"][e]
        assert t["RE_ROW_SHIFT"][e] == 0
        assert dv[c] >= 2 and t["ROW_SLOT"][e] >= 0
        assert row_wave[r] == col_wave[c]
        per_wave[row_wave[r]].append(x)
    for w in range(W):
        assert sorted(per_wave[w]) == list(range(t["RE_NREG"][w]))  # msg[] indices: dense, unique
        assert t["RE_NREG"][w] <= t["RE_CAP"]
    assert sum(t["RE_NREG"]) > 0


@pytest.mark.parametrize("code", sorted(CODES))
def test_every_column_is_one_task(tables, code):
    t = tables[code]
    dv = np.diff(t["COL_PTR"])
    cols = [c for c in t["VT_A"]] + [c for c in t["VT_B"] if c >= 0]
    assert sorted(cols) == [c for c in range(t["Nb"]) if dv[c] >= 2]
    for a, b in zip(t["VT_A"], t["VT_B"]):
        assert b < 0 or dv[b] <= dv[a]  # the kernel's static_assert: A is the longer column of a pair
    task_wave = {x: w for w in range(W) for x in range(t["VT_PTR"][w], t["VT_PTR"][w + 1])}
    col_wave = waves(t["VT_COL_PTR"], t["VT_COLS"])
    for x, (a, b) in enumerate(zip(t["VT_A"], t["VT_B"])):
        assert col_wave[a] == task_wave[x] and (b < 0 or col_wave[b] == task_wave[x])


def frames(n_cols):
    """12 frames: the noisy -3 dB recipe of test_flood_layout_gpu.py, the last four with a run of
    zeros, +inf, -inf and NaN"""
    rng = np.random.default_rng(1000 + n_cols)
    llr = (rng.normal(1.0, 1.0, size=(12, n_cols)) * (2 * 10 ** (-3.0 / 10))).astype(np.float32)
    llr[8, :40] = 0.0
    llr[9, 5] = np.inf
    llr[10, 9] = -np.inf
    llr[11, 11] = np.nan
    return llr


def counters(bits, iters):
    return [int(bits.sum()), int((bits.sum(1) > 0).sum()), bits.shape[0], int(iters.sum())]


@pytest.mark.parametrize("code", sorted(CODES))
def test_relabelled_code_decodes_identically(oracle_mod, tables, code):
    t, z = tables[code], CODES[code]
    base = oracle_mod.load_base(code_path(z))
    rel = base.copy()
    for r in range(base.shape[0]):
        on = base[r] >= 0
        rel[r, on] = (base[r, on] % z + t["RE_RHO"][r]) % z
    assert any(t["RE_RHO"]) and not np.array_equal(rel, base)
    g0 = oracle_mod.Graph(oracle_mod.expand(base, z))
    g1 = oracle_mod.Graph(oracle_mod.expand(rel, z))
    llr = frames(g0.N)
    for algo in ("minsum", "bp"):
        for es in (0, 1, 2):
            b0, a0, n0, i0 = oracle_mod.flood_decode(g0, llr, algo, 10, 0.75, es)
            b1, a1, n1, i1 = oracle_mod.flood_decode(g1, llr, algo, 10, 0.75, es)
            assert np.array_equal(b0, b1), (algo, es)
            assert n0 == n1 and np.array_equal(i0, i1), (algo, es)
            assert counters(b0, i0) == counters(b1, i1), (algo, es)
            assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32)), (algo, es)
