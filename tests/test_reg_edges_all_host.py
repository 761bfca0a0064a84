"""Register-edge schedule with every eligible edge taken (gen/fixed_codes.hpp RE_*), no GPU.

tests/test_reg_edges_host.py checks that the RE_* tables follow the rule.  Here: the generator's cap
no longer binds, so the tables hold what the search finds (44 edges at Z = 32, 58 at Z = 4), and
the per-instance cap of csrc/flood_fixed.hpp (FxPlan<G, WV, CAP, REG>: the first CAP entries of a wave's
msg[] order stay register edges, the others fall back to their LDS slot) cuts a well-formed
sub-schedule out of them for any CAP: dense msg[] indices, the dropped edges slot edges of shift 0."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import PKG

sys.path.insert(0, os.path.join(PKG, "tools"))
import gen_fixed_codes as gen  # noqa: E402
from reg_edges_util import parse_header  # noqa: E402

W = 4
FOUND = {"BG2_Z32": [11, 11, 11, 11], "BG2_Z4": [15, 14, 14, 15]}


@pytest.fixture(scope="module")
def tables():
    with open(os.path.join(PKG, "csrc", "gen", "fixed_codes.hpp")) as f:
        return parse_header(f.read())


def slow_caps():
    src = open(os.path.join(PKG, "csrc", "flood_fixed.hpp")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (LDPC_SLOW_REG_EDGES\w*) (\d+)", src)}


@pytest.mark.parametrize("code", sorted(FOUND))
def test_every_eligible_edge_is_taken(tables, code):
    t = tables[code]
    assert t["RE_NREG"] == FOUND[code]
    assert sum(t["RE_NREG"]) == sum(1 for x in t["RE_ROW_REG"] if x >= 0) == {"BG2_Z32": 44, "BG2_Z4": 58}[code]
    assert max(t["RE_NREG"]) < t["RE_CAP"] == gen.REG_EDGE_CAP  # the cap does not bind
    # with the schedule as it stands, no further edge qualifies: shift 0, a slot, row and column on one wave
    dv = np.diff(t["COL_PTR"])
    row_wave = {r: w for w in range(W) for r in t["RE_CHK_ROWS"][t["RE_CHK_PTR"][w]:t["RE_CHK_PTR"][w + 1]]}
    col_wave = {c: w for w in range(W) for c in t["VT_COLS"][t["VT_COL_PTR"][w]:t["VT_COL_PTR"][w + 1]]}
    for e in range(t["NBLOCKS"]):
        r, c = t["BLK_ROW"][e], t["BLK_COL"][e]
        eligible = t["RE_ROW_SHIFT"][e] == 0 and dv[c] >= 2 and row_wave[r] == col_wave[c]
        assert eligible == (t["RE_ROW_REG"][e] >= 0), e


def test_a_larger_cap_finds_no_more(tables):
    wide = parse_header(gen.header_text(cap=64))
    for code in FOUND:
        assert sum(wide[code]["RE_NREG"]) == sum(tables[code]["RE_NREG"])
    assert wide["BG2_Z32"]["RE_NREG"] == FOUND["BG2_Z32"]


@pytest.mark.parametrize("code", sorted(FOUND))
def test_per_instance_cap_cuts_a_well_formed_schedule(tables, code):
    t = tables[code]
    caps = slow_caps()
    assert set(caps) == {"LDPC_SLOW_REG_EDGES", "LDPC_SLOW_REG_EDGES_OFF"}
    row_wave = {r: w for w in range(W) for r in t["RE_CHK_ROWS"][t["RE_CHK_PTR"][w]:t["RE_CHK_PTR"][w + 1]]}
    for cap in sorted(set(caps.values()) | {0, 1, 64}):
        assert 0 <= cap
        kept = [x if x < cap else -1 for x in t["RE_ROW_REG"]]  # FxPlan::row_reg
        per_wave = [[] for _ in range(W)]
        for e, x in enumerate(kept):
            if x >= 0:
                per_wave[row_wave[t["BLK_ROW"][e]]].append(x)
            elif t["RE_ROW_REG"][e] >= 0:  # dropped: read and written at its slot, own-lane
                assert t["ROW_SLOT"][e] >= 0 and t["RE_ROW_SHIFT"][e] == 0
        for w in range(W):
            assert sorted(per_wave[w]) == list(range(min(cap, t["RE_NREG"][w])))  # FxPlan::NREG
