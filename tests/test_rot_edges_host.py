"""Rotated edges of the fixed flood schedule (gen/fixed_codes.hpp RE_ROW_ROT / RE_COL_ROT / RE_NROT), no GPU.

A rotated edge is a slot edge outside msg[] whose row and column are on one wave and whose
normalised shift is not 0: the min-sum kernel moves its message between the check lane and the
variable lane with one cross-lane rotation (flood_fixed.hpp rmsg[], flood_dev.hpp seg_rotate: a
ds_swizzle_b32 whose pattern is an instruction constant) instead of an own-lane slot store and a
rotated slot read.  Here: the tables follow that rule and are complete, the per-instance cap cuts a
dense sub-set, the wave's rot[] table (FxPlan::make) still holds every rotation its remaining slot
edges read with, and the swizzle patterns give every lane what the slot round trip gave it."""
import os
import re

import numpy as np
import pytest

from conftest import PKG
from reg_edges_util import parse_header

W = 4
CODES = ("BG2_Z32", "BG2_Z4")


@pytest.fixture(scope="module")
def tables():
    with open(os.path.join(PKG, "csrc", "gen", "fixed_codes.hpp")) as f:
        return parse_header(f.read())


def waves(t):
    row_wave = {r: w for w in range(W) for r in t["RE_CHK_ROWS"][t["RE_CHK_PTR"][w]:t["RE_CHK_PTR"][w + 1]]}
    col_wave = {c: w for w in range(W) for c in t["VT_COLS"][t["VT_COL_PTR"][w]:t["VT_COL_PTR"][w + 1]]}
    return row_wave, col_wave


def qualifies(t, e, row_wave, col_wave):
    return (t["ROW_SLOT"][e] >= 0 and t["RE_ROW_REG"][e] < 0 and t["RE_ROW_SHIFT"][e] != 0
            and row_wave[t["BLK_ROW"][e]] == col_wave.get(t["BLK_COL"][e], -1))


def col_order(t):
    """block index of every entry of the COL_* arrays"""
    return [e for c in range(t["Nb"]) for e in range(t["NBLOCKS"]) if t["BLK_COL"][e] == c]


@pytest.mark.parametrize("code", CODES)
def test_listed_edges_qualify_and_the_set_is_complete(tables, code):
    t = tables[code]
    row_wave, col_wave = waves(t)
    assert len(t["RE_ROW_ROT"]) == t["NBLOCKS"]
    for e in range(t["NBLOCKS"]):
        assert (t["RE_ROW_ROT"][e] >= 0) == qualifies(t, e, row_wave, col_wave), e
        assert t["RE_ROW_ROT"][e] >= -1


@pytest.mark.parametrize("code", CODES)
def test_indices_are_dense_per_wave_in_row_order(tables, code):
    t = tables[code]
    row_wave, _ = waves(t)
    per = [[] for _ in range(W)]
    for e, x in enumerate(t["RE_ROW_ROT"]):  # ascending edge index: row order
        if x >= 0:
            per[row_wave[t["BLK_ROW"][e]]].append(x)
    for w in range(W):
        assert per[w] == list(range(t["RE_NROT"][w])), w
    assert len(t["RE_NROT"]) == W


def test_counts_at_z32(tables):
    """20 of the 115 non-register slot edges, mostly on the waves with the longest variable phase"""
    t = tables["BG2_Z32"]
    assert t["RE_NROT"] == [4, 7, 3, 6]
    assert sum(1 for e in range(t["NBLOCKS"]) if t["ROW_SLOT"][e] >= 0 and t["RE_ROW_REG"][e] < 0) == 115


@pytest.mark.parametrize("code", CODES)
def test_col_rot_is_row_rot_in_column_order(tables, code):
    t = tables[code]
    order = col_order(t)
    assert [t["ROW_SLOT"][e] for e in order] == t["COL_SLOT"]  # the order COL_* arrays use
    assert t["RE_COL_ROT"] == [t["RE_ROW_ROT"][e] for e in order]


def wave_rotations(t, w, row_wave, col_wave, skip):
    """FxPlan::make: the shifts of the wave's columns' slot edges and the inverse shifts of its rows'
    slot edges, register edges and the rotated edges in `skip` left out"""
    z = t["Z"]
    s = set()
    for e in range(t["NBLOCKS"]):
        if t["ROW_SLOT"][e] < 0 or t["RE_ROW_REG"][e] >= 0 or e in skip:
            continue
        if col_wave.get(t["BLK_COL"][e], -1) == w:
            s.add(t["RE_ROW_SHIFT"][e])
        if row_wave[t["BLK_ROW"][e]] == w:
            s.add((z - t["RE_ROW_SHIFT"][e]) % z)
    return s


@pytest.mark.parametrize("code", CODES)
def test_rot_table_without_the_rotated_edges(tables, code):
    """A rotated edge needs no rot[] entry.  Every other slot edge of a wave's rows and columns is
    still covered (by construction), the table never grows, and it fits its 64 entries."""
    t = tables[code]
    row_wave, col_wave = waves(t)
    rotated = {e for e, x in enumerate(t["RE_ROW_ROT"]) if x >= 0}
    for w in range(W):
        before = wave_rotations(t, w, row_wave, col_wave, set())
        after = wave_rotations(t, w, row_wave, col_wave, rotated)
        assert after <= before and len(before) <= 64
        for e in rotated:  # both of its rotations were entries of its wave, the slot form's addresses
            if row_wave[t["BLK_ROW"][e]] == w:
                assert {t["RE_ROW_SHIFT"][e], (t["Z"] - t["RE_ROW_SHIFT"][e]) % t["Z"]} <= before


def rot_caps():
    src = open(os.path.join(PKG, "csrc", "flood_fixed.hpp")).read()
    return {m.group(1): m.group(2) for m in re.finditer(r"#define (LDPC_\w*ROT_EDGES\w*) (\S+)", src)}


def shares(t, cap):
    """FxPlan::rot_share for every wave: the instance's cap handed out wave by wave, the wave with
    the most non-register slot edges in its columns first (ties: the lower wave)"""
    _, col_wave = waves(t)
    n = [0] * W
    for e in range(t["NBLOCKS"]):
        if t["ROW_SLOT"][e] >= 0 and t["RE_ROW_REG"][e] < 0:
            n[col_wave[t["BLK_COL"][e]]] += 1
    out = [0] * W
    left = cap
    for w in sorted(range(W), key=lambda w: (-n[w], w)):
        out[w] = max(0, min(left, t["RE_NROT"][w]))
        left -= t["RE_NROT"][w]
    return n, out


@pytest.mark.parametrize("code", CODES)
def test_per_instance_cap_cuts_a_dense_subset(tables, code):
    t = tables[code]
    caps = rot_caps()
    assert set(caps) == {"LDPC_ROT_EDGES", "LDPC_SLOW_ROT_EDGES", "LDPC_SLOW_ROT_EDGES_OFF"}
    assert caps["LDPC_SLOW_ROT_EDGES_OFF"] == "0"  # that instance has no VGPR to spare
    row_wave, _ = waves(t)
    total = sum(t["RE_NROT"])
    for cap in (0, 1, 5, 13, total, 1 << 20):
        n, sh = shares(t, cap)
        assert sum(sh) == min(cap, total)
        kept = [[] for _ in range(W)]
        for e, x in enumerate(t["RE_ROW_ROT"]):
            w = row_wave[t["BLK_ROW"][e]]
            if 0 <= x < sh[w]:  # FxPlan::row_rot
                kept[w].append(x)
        for w in range(W):
            assert kept[w] == list(range(sh[w]))
    if code == "BG2_Z32":
        n, sh = shares(t, 13)
        assert n == [25, 32, 25, 33] and sh == [0, 7, 0, 6]  # waves 3 and 1 first


def swizzle(v, pattern):
    """ds_swizzle_b32 on 64 lanes with every lane active: quad mode (bit 15; lane i takes the lane
    of its quad named by the i-th 2-bit select) and rotate mode (0xC000 | dir << 10 | amount << 5 |
    mask; with dir = 0 and mask = 0 lane i takes lane (i + amount) mod 32 of its half)."""
    i = np.arange(64)
    if pattern >= 0xE000:
        raise ValueError("FFT mode is not used")
    if pattern >= 0xC000:
        amount, left, mask = (pattern >> 5) & 31, not (pattern >> 10) & 1, pattern & 31
        assert left and mask == 0
        return v[(i & 32) | ((i + amount) & 31)]
    assert pattern & 0x8000 and pattern < 0x8100
    return v[(i & ~3) | ((pattern >> (2 * (i & 3))) & 3)]


def seg_rotate_pattern(z, s):
    """flood_dev.hpp seg_rotate<Z, S>"""
    assert z in (32, 4) and 0 <= s < z
    if z == 32:
        return 0xC000 | ((32 - s) % 32) << 5
    return 0x8000 | sum(((i - s) & 3) << (2 * i) for i in range(4))


@pytest.mark.parametrize("code", CODES)
def test_rotation_equals_slot_store_and_rotated_read(tables, code):
    """Rotating by s inside every Z-lane segment, source lane f*Z + (k - s) mod Z, gives every lane
    what an own-lane slot store followed by the read at rot[s] gives it, for every shift of the
    code and its inverse: the c2v of check (t - s) mod Z on variable lane t, the v2c of variable
    (k + s) mod Z on check lane k.  seg_rotate's swizzle pattern is that rotation."""
    t = tables[code]
    z = t["Z"]
    lanes = np.arange(64)
    f, k = lanes // z, lanes % z
    rng = np.random.default_rng(z)
    v = rng.standard_normal(64).astype(np.float32)
    base = 0x4000
    for s in sorted(set(t["RE_ROW_SHIFT"]) | {(z - x) % z for x in t["RE_ROW_SHIFT"]}):
        addr = base + 4 * (f * z) + ((4 * k + (4 * z - 4 * s)) & (4 * z - 1))  # FixedBody::init rot[]
        slot = v.copy()                          # own-lane store: position = lane
        read = slot[(addr - base) // 4]          # ds_read_b32 at rot[s]
        assert np.array_equal(read, v[f * z + (k - s) % z]), s
        moved = swizzle(v, seg_rotate_pattern(z, s))
        assert np.array_equal(moved, read), s
        # to the variable lane with s, back to the check lane with Z - s: the identity
        assert np.array_equal(swizzle(moved, seg_rotate_pattern(z, (z - s) % z)), v), s


def test_patterns_in_the_source_are_the_ones_restated_here():
    src = open(os.path.join(PKG, "csrc", "flood_dev.hpp")).read()
    body = src[src.index("float seg_rotate(float v)"):]
    body = body[:body.index("}\n")]
    assert "0xC000 | ((32 - S) % 32) << 5" in body and "0x8000 | sel" in body
    assert "((0 - S) & 3) | ((1 - S) & 3) << 2 | ((2 - S) & 3) << 4 | ((3 - S) & 3) << 6" in body
    assert "__builtin_amdgcn_ds_swizzle" in body
