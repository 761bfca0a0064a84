"""The fixed flood kernel's joint schedule (gen/fixed_codes.hpp RE_J_*), no GPU.

tools/gen_fixed_codes.py joint_schedule puts block rows and slot-bearing columns on the four waves
together and minimises the LDS operands per wave and iteration, the quantity a phase's time
follows: a slot edge sends 2 per phase (the read's address VGPR and the own-lane
store's data VGPR), a rotated edge (row and column on one wave, normalised shift != 0) 1 (its
swizzle), a register edge (same wave, shift 0) none; the check phase counts an edge on its row's
wave, the variable phase on its column's.  Checked here, for both codes: the arrays follow those
rules and are complete, the operand table recomputed from them is the generator's and beats the
committed schedule's (Z = 32: max + max 115, total 420), and the code relabelled with the new
rho decodes exactly as the original one on the oracle (the argument of test_reg_edges_host.py)."""
import os
import sys

import numpy as np
import pytest

from conftest import PKG, code_path

sys.path.insert(0, os.path.join(PKG, "tools"))
import gen_fixed_codes as gen  # noqa: E402
from reg_edges_util import parse_header  # noqa: E402

HEADER = os.path.join(PKG, "csrc", "gen", "fixed_codes.hpp")
CODES = {"BG2_Z4": 4, "BG2_Z32": 32}
W = 4


@pytest.fixture(scope="module")
def header_text():
    with open(HEADER) as f:
        return f.read()


@pytest.fixture(scope="module")
def tables(header_text):
    return parse_header(header_text)


@pytest.fixture(scope="module")
def report():
    """the generator's own report (LDPC_GEN_REPORT prints it) and its text"""
    rep = {}
    text = gen.header_text(report=rep)
    return text, rep


def col_order(t):
    return [e for c in range(t["Nb"]) for e in range(t["NBLOCKS"]) if t["BLK_COL"][e] == c]


def waves(ptr, items):
    out = {}
    for w in range(W):
        for x in items[ptr[w]:ptr[w + 1]]:
            assert x not in out
            out[x] = w
    return out


def operands(t, row_wave, col_wave, reg, rot):
    """the definition, restated: per slot edge 0 (register), 1 (rotated) or 2, counted on the row's
    wave in the check phase and on the column's wave in the variable phase"""
    chk, var = [0] * W, [0] * W
    for e in range(t["NBLOCKS"]):
        if t["ROW_SLOT"][e] < 0:
            continue
        n = 0 if reg[e] >= 0 else (1 if rot[e] >= 0 else 2)
        chk[row_wave[t["BLK_ROW"][e]]] += n
        var[col_wave[t["BLK_COL"][e]]] += n
    return chk, var


def test_header_is_the_generator_output(header_text, report):
    assert header_text == report[0]


def test_every_new_line_is_an_re_line(header_text):
    """the tests that pin the older arrays strip the lines holding " RE_" """
    for line in header_text.splitlines():
        assert "RE_J_" not in line or " RE_J_" in line


@pytest.mark.parametrize("code", sorted(CODES))
def test_rows_and_columns_are_on_one_wave_each(tables, code):
    t = tables[code]
    dv = np.diff(t["COL_PTR"])
    row_wave = waves(t["RE_J_CHK_PTR"], t["RE_J_CHK_ROWS"])
    col_wave = waves(t["RE_J_VT_COL_PTR"], t["RE_J_VT_COLS"])
    assert sorted(row_wave) == list(range(t["Mb"]))
    assert sorted(col_wave) == [c for c in range(t["Nb"]) if dv[c] >= 2]
    assert len(t["RE_J_CHK_PTR"]) == W + 1 and len(t["RE_J_VT_COL_PTR"]) == W + 1


@pytest.mark.parametrize("code", sorted(CODES))
def test_normalised_shifts(tables, code):
    t, z = tables[code], CODES[code]
    assert len(t["RE_J_RHO"]) == t["Mb"] and all(0 <= r < z for r in t["RE_J_RHO"])
    want = [(t["ROW_SHIFT"][e] + t["RE_J_RHO"][t["BLK_ROW"][e]]) % z for e in range(t["NBLOCKS"])]
    assert t["RE_J_ROW_SHIFT"] == want
    order = col_order(t)
    assert [t["ROW_SLOT"][e] for e in order] == t["COL_SLOT"]  # the order of the COL_* arrays
    assert t["RE_J_COL_SHIFT"] == [want[e] for e in order]


@pytest.mark.parametrize("code", sorted(CODES))
def test_register_and_rotated_edges(tables, code):
    t = tables[code]
    row_wave = waves(t["RE_J_CHK_PTR"], t["RE_J_CHK_ROWS"])
    col_wave = waves(t["RE_J_VT_COL_PTR"], t["RE_J_VT_COLS"])
    order = col_order(t)
    for kind, count, want_zero in (("REG", "NREG", True), ("ROT", "NROT", False)):
        rows, cols = t[f"RE_J_ROW_{kind}"], t[f"RE_J_COL_{kind}"]
        assert len(rows) == t["NBLOCKS"] and min(rows) >= -1
        assert cols == [rows[e] for e in order]  # row order and column order agree
        per = [[] for _ in range(W)]
        for e, x in enumerate(rows):  # ascending edge index: row order
            if x < 0:
                continue
            r, c = t["BLK_ROW"][e], t["BLK_COL"][e]
            assert t["ROW_SLOT"][e] >= 0
            assert (t["RE_J_ROW_SHIFT"][e] == 0) == want_zero, (kind, e)
            assert row_wave[r] == col_wave[c], (kind, e)
            per[row_wave[r]].append(x)
        for w in range(W):
            assert per[w] == list(range(t[f"RE_J_{count}"][w])), (kind, w)  # dense, unique, in row order
    both = [e for e in range(t["NBLOCKS"]) if t["RE_J_ROW_REG"][e] >= 0 and t["RE_J_ROW_ROT"][e] >= 0]
    assert not both


@pytest.mark.parametrize("code", sorted(CODES))
def test_rho_makes_the_rows_most_common_same_wave_shift_zero(tables, code):
    t, z = tables[code], CODES[code]
    row_wave = waves(t["RE_J_CHK_PTR"], t["RE_J_CHK_ROWS"])
    col_wave = waves(t["RE_J_VT_COL_PTR"], t["RE_J_VT_COLS"])
    for r in range(t["Mb"]):
        same = [t["RE_J_ROW_SHIFT"][e] for e in range(t["ROW_PTR"][r], t["ROW_PTR"][r + 1])
                if t["ROW_SLOT"][e] >= 0 and col_wave[t["BLK_COL"][e]] == row_wave[r]]
        if same:
            assert same.count(0) == max(same.count(s) for s in set(same)), r
        else:
            assert t["RE_J_RHO"][r] == 0


@pytest.mark.parametrize("code", sorted(CODES))
def test_kept_messages_per_wave_are_within_the_cap(tables, code):
    t = tables[code]
    assert t["RE_J_CAP"] == gen.JOINT_KEPT_CAP
    for w in range(W):
        assert t["RE_J_NREG"][w] + t["RE_J_NROT"][w] <= t["RE_J_CAP"]


@pytest.mark.parametrize("code", sorted(CODES))
def test_every_column_is_one_task(tables, code):
    t = tables[code]
    dv = np.diff(t["COL_PTR"])
    cols = list(t["RE_J_VT_A"]) + [c for c in t["RE_J_VT_B"] if c >= 0]
    assert sorted(cols) == [c for c in range(t["Nb"]) if dv[c] >= 2]
    assert len(t["RE_J_VT_A"]) == len(t["RE_J_VT_B"]) == t["RE_J_VT_PTR"][W]
    col_wave = waves(t["RE_J_VT_COL_PTR"], t["RE_J_VT_COLS"])
    task_wave = {x: w for w in range(W) for x in range(t["RE_J_VT_PTR"][w], t["RE_J_VT_PTR"][w + 1])}
    for x, (a, b) in enumerate(zip(t["RE_J_VT_A"], t["RE_J_VT_B"])):
        assert b < 0 or dv[b] <= dv[a]  # the kernel's static_assert: A is the longer column of a pair
        assert b < 0 or dv[a] + dv[b] <= gen.JOINT_PAIR_MSGS
        assert col_wave[a] == task_wave[x] and (b < 0 or col_wave[b] == task_wave[x])


@pytest.mark.parametrize("code", sorted(CODES))
def test_operand_table_is_the_generators(tables, report, code):
    t = tables[code]
    row_wave = waves(t["RE_J_CHK_PTR"], t["RE_J_CHK_ROWS"])
    col_wave = waves(t["RE_J_VT_COL_PTR"], t["RE_J_VT_COLS"])
    chk, var = operands(t, row_wave, col_wave, t["RE_J_ROW_REG"], t["RE_J_ROW_ROT"])
    rep = report[1][code + " LDS operands"]
    assert chk == rep["joint chk"] == t["RE_J_OPS_CHK"]
    assert var == rep["joint var"] == t["RE_J_OPS_VAR"]
    assert rep["joint max+max, total"] == [max(chk) + max(var), sum(chk) + sum(var)]
    # and the committed schedule's, by the same definition
    old_rows = waves(t["RE_CHK_PTR"], t["RE_CHK_ROWS"])
    old_cols = waves(t["VT_COL_PTR"], t["VT_COLS"])
    ochk, ovar = operands(t, old_rows, old_cols, t["RE_ROW_REG"], t["RE_ROW_ROT"])
    assert ochk == rep["old chk"] and ovar == rep["old var"]
    assert max(chk) + max(var) < max(ochk) + max(ovar) and sum(chk) + sum(var) < sum(ochk) + sum(ovar)


def test_operands_at_z32(tables):
    """The committed schedule: check 54 / 51 / 55 / 50, variable 46 / 57 / 47 / 60 (max + max 115,
    total 420).  The joint one, with a cap of at least 24 kept messages per wave: max + max <= 100
    and total <= 386."""
    t = tables["BG2_Z32"]
    old_rows = waves(t["RE_CHK_PTR"], t["RE_CHK_ROWS"])
    old_cols = waves(t["VT_COL_PTR"], t["VT_COLS"])
    assert operands(t, old_rows, old_cols, t["RE_ROW_REG"], t["RE_ROW_ROT"]) == ([54, 51, 55, 50], [46, 57, 47, 60])
    chk, var = t["RE_J_OPS_CHK"], t["RE_J_OPS_VAR"]
    assert t["RE_J_CAP"] >= 24
    assert max(chk) + max(var) <= 100 and sum(chk) + sum(var) <= 386
    assert max(chk) + max(var) < 115 and sum(chk) + sum(var) < 420


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
        rel[r, on] = (base[r, on] % z + t["RE_J_RHO"][r]) % z
    assert any(t["RE_J_RHO"]) and not np.array_equal(rel, base)
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
