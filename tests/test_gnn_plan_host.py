"""The message-GNN plan's tables (csrc/gnn_plan_tables.cpp), read back through ldpc_gnn_plan_tables /
ldpc_gnn_plan_tables_csr on the host: no device is touched.

Two independent checks per input:

* Equality with the builder this one replaced.  tests/golden/gnn_plan_tables.json pins the sha256 of
  the header and of every section.  The digests were recorded from the commit before the builder moved
  out of gnn.hip, not from this code: in a scratch export of that commit, ldpc_gnn_plan_create and
  ldpc_gnn_plan_create_csr were given a hook that wrote their host vectors, in the format of
  ldpc_amd.h, just before `new ldpc_gnn_plan()` (the vectors are complete before the first HIP call,
  so the calls' later failure on a machine without a device did not matter); that library was called
  through ctypes with the inputs of `group_cases()` / `csr_case()` below.
* The properties csrc/gnn.hpp states for the tables, computed here in numpy from the inputs alone.

Every case also asserts the branch of the builder it is there for."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, code_path

from ldpc_neural_decoder import _native as N
from ldpc_neural_decoder.models.message_gnn_decoder import TannerToMessageGraph
from ldpc_neural_decoder.utils import expand_base_matrix, load_base_matrix

COUNTS = ("n_gtiles", "n_gtiles_v1", "n_gtiles_v", "n_ptiles", "n_ptiles_v", "n_ptiles_v1", "n_mtiles",
          "n_mtiles_v1", "n_ctiles", "ct_aligned", "n_rw", "rw_d1")
SECTIONS = ("vgroup", "cgroup", "vg_ptr", "vg_mem", "cg_ptr", "cg_mem", "inv", "gt_meta", "gt_grp", "gt_mem",
            "pt_meta", "pt_grp", "pt_deg", "pt_mem", "mt_perm", "ct_m0", "rw_meta")
CSR_COUNTS = ("E", "nnz_v", "nnz_c")
CSR_SECTIONS = ("tab", "inv", "w", "tt", "tw")
_P = ctypes.c_void_p


# ---------------------------------------------------------------------------------------- inputs
def seeded_permutation(n, seed):
    """Fisher-Yates driven by a 32-bit LCG: the same permutation whatever numpy's generators do."""
    p, s = np.arange(n), seed
    for i in range(n - 1, 0, -1):
        s = (1664525 * s + 1013904223) & 0xFFFFFFFF
        j = (s >> 8) % (i + 1)
        p[i], p[j] = p[j], p[i]
    return p


def bg2(z):
    conv = TannerToMessageGraph(expand_base_matrix(load_base_matrix(code_path(z)), z))
    return conv.edge_var, conv.num_variables, conv.edge_chk, conv.num_checks


def runs(degrees):
    """Check labels of contiguous runs: check i owns degrees[i] consecutive messages."""
    return np.repeat(np.arange(len(degrees)), degrees)


def lone_position_graph(moved_check=None):
    """64 checks of degree 3, then 32 of degree 5.  Position 2 of every degree-3 check is the only
    message of its variable (variables 0..63); the other messages pair up in variables of degree 2.
    moved_check: that check's lone variable sits at position 1 instead."""
    cg = runs([3] * 64 + [5] * 32)
    vg = np.empty(len(cg), dtype=np.int64)
    lone = 3 * np.arange(64) + 2
    vg[lone] = np.arange(64)
    rest = np.setdiff1d(np.arange(len(cg)), lone)
    vg[rest] = 64 + np.arange(len(rest)) // 2
    if moved_check is not None:
        a, b = 3 * moved_check + 1, 3 * moved_check + 2
        vg[a], vg[b] = vg[b], vg[a]
    return vg, 64 + len(rest) // 2, cg, 96


def group_cases():
    """name -> (vgroup, n_vgroups, cgroup, n_cgroups)"""
    c = {}
    c["bg2_z4"] = bg2(4)
    c["bg2_z32"] = bg2(32)
    vg, nv, cg, nc = c["bg2_z4"]
    perm = seeded_permutation(len(vg), 2024)
    c["bg2_z4_permuted"] = (vg[perm], nv, cg[perm], nc)
    cg = runs([4, 40, 4])
    c["check_degree_40"] = (np.arange(48) // 2, 24, cg, 3)
    c["lone_position_2"] = lone_position_graph()
    c["lone_position_moved"] = lone_position_graph(moved_check=5)
    cg = runs([3, 5] * 5)
    c["alternating_degrees"] = (np.arange(40) // 2, 20, cg, 10)
    vg, nv, cg, nc = c["lone_position_2"]
    c["check_labels_reversed"] = (vg, nv, nc - 1 - cg, nc)
    # labels 0, 3 and 6 of 7 var groups and 0, 2 and 5 of 6 check groups are unused
    c["empty_groups"] = (np.array([1, 2, 4, 5, 1, 2, 4, 5, 5, 1]), 7, np.array([1, 1, 1, 3, 3, 4, 4, 4, 4, 4]), 6)
    c["e45"] = (np.arange(45) % 9, 9, runs([3] * 15), 15)
    c["e7"] = (np.array([0, 1, 2, 0, 1, 2, 3]), 4, np.array([0, 0, 0, 1, 1, 2, 2]), 3)
    return c


def csr_case():
    """E = 6.  Var side: row 1 is empty and column 3 has no nonzero; check side: row 2 is empty and
    columns 1 and 3 have none.  The values are in no order."""
    v = (np.array([0, 2, 2, 5, 6, 8, 9]), np.array([1, 4, 0, 2, 5, 2, 0, 4, 5]),
         np.array([0.5, -1.25, 2.0, 0.125, -3.0, 0.75, 1.5, -0.5, 4.0], dtype=np.float32))
    c = (np.array([0, 1, 3, 3, 4, 6, 7]), np.array([2, 0, 5, 4, 0, 2, 5]),
         np.array([3.0, -0.25, 1.0, 0.5, -2.0, 0.375, 8.0], dtype=np.float32))
    return 6, v, c


# ------------------------------------------------------------------------------- reading tables
def _split(words, counts, sections):
    n = len(counts) + len(sections)
    lengths = words[len(counts):n]
    assert n + int(lengths.sum()) == len(words)
    out = {"header": words[:n]}
    out.update(zip(counts, words[:len(counts)].tolist()))
    off = n
    for name, ln in zip(sections, lengths.tolist()):
        out[name] = words[off:off + ln]
        off += ln
    return out


def _call(fn, args):
    need = fn(*args, None, 0)
    assert need > 0, N.lib().ldpc_last_error()
    words = np.zeros(need, dtype=np.int32)
    assert fn(*args, words.ctypes.data_as(_P), need) == need
    return words


def plan_tables(vg, nv, cg, nc):
    vg, cg = np.ascontiguousarray(vg, dtype=np.int32), np.ascontiguousarray(cg, dtype=np.int32)
    words = _call(N.lib().ldpc_gnn_plan_tables, (len(vg), nv, vg.ctypes.data_as(_P), nc, cg.ctypes.data_as(_P)))
    return _split(words, COUNTS, SECTIONS)


def csr_tables(E, v, c):
    arrs = [np.ascontiguousarray(a, dtype=t) for side in (v, c) for a, t in zip(side, (np.int32, np.int32, np.float32))]
    words = _call(N.lib().ldpc_gnn_plan_tables_csr, (E, *[a.ctypes.data_as(_P) for a in arrs]))
    return _split(words, CSR_COUNTS, CSR_SECTIONS)


def digests(t, sections):
    return {k: hashlib.sha256(np.ascontiguousarray(t[k], dtype="<i4").tobytes()).hexdigest()
            for k in ("header",) + tuple(sections)}


@pytest.fixture(scope="module")
def pinned():
    with open(os.path.join(GOLDEN, "gnn_plan_tables.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def cases():
    return group_cases()


@pytest.fixture(scope="module")
def tables(cases):
    return {name: plan_tables(*args) for name, args in cases.items()}


CASE_NAMES = ("bg2_z4", "bg2_z32", "bg2_z4_permuted", "check_degree_40", "lone_position_2", "lone_position_moved",
              "alternating_degrees", "check_labels_reversed", "empty_groups", "e45", "e7")


def test_case_list_is_complete(cases, pinned):
    assert tuple(cases) == CASE_NAMES
    assert sorted(pinned) == sorted(CASE_NAMES + ("csr",))


# ----------------------------------------------------------------- equality with the old builder
@pytest.mark.parametrize("name", CASE_NAMES)
def test_tables_equal_the_previous_builder(tables, pinned, name):
    got = digests(tables[name], SECTIONS)
    assert [k for k in got if got[k] != pinned[name][k]] == []


def test_csr_tables_equal_the_previous_builder(pinned):
    E, v, c = csr_case()
    t = csr_tables(E, v, c)
    # both transposes, each on its own, besides the sections as uploaded
    nv, nc = t["nnz_v"], t["nnz_c"]
    t["vt"], t["ct"] = t["tt"][:E + 1 + nv], t["tt"][E + 1 + nv:]
    t["vt_w"], t["ct_w"] = t["tw"][:nv], t["tw"][nv:]
    got = digests(t, CSR_SECTIONS + ("vt", "ct", "vt_w", "ct_w"))
    assert [k for k in got if got[k] != pinned["csr"][k]] == []


def test_csr_transposes_match_dense():
    E, v, c = csr_case()
    t = csr_tables(E, v, c)
    assert (t["E"], t["nnz_v"], t["nnz_c"]) == (6, 9, 7)
    tt, tw = t["tt"], t["tw"].view(np.float32)
    assert len(tw) == 9 + 7 + 1 and tw[-1] == 0.0
    off_t = off_w = 0
    for ptr, col, val in (v, c):
        nnz = len(col)
        assert (np.diff(ptr) == 0).any(), "the case needs an empty row"
        dense = np.zeros((E, E), dtype=np.float32)
        dense[np.repeat(np.arange(E), np.diff(ptr)), col] = val
        assert (dense != 0).sum() == nnz and not (dense != 0).any(axis=0).all(), "... and an empty column"
        assert (np.diff(val) < 0).any() and (np.diff(val) > 0).any(), "... and unsorted values"
        tp, tm = tt[off_t:off_t + E + 1], tt[off_t + E + 1:off_t + E + 1 + nnz]
        w = tw[off_w:off_w + nnz]
        assert tp[0] == 0 and tp[-1] == nnz
        assert (np.diff(tp) == 0).any()
        for j in range(E):  # column j's nonzero rows ascending, with their weights
            rows = np.nonzero(dense[:, j])[0]
            assert tm[tp[j]:tp[j + 1]].tolist() == rows.tolist()
            assert w[tp[j]:tp[j + 1]].tolist() == dense[rows, j].tolist()
        off_t += E + 1 + nnz
        off_w += nnz
    tab = t["tab"]
    assert tab[:2 * E].tolist() == list(range(E)) * 2  # every message reads its own row
    assert (t["inv"].view(np.float32) == 1.0).all() and len(t["inv"]) == 2 * E


# ------------------------------------------------------------------------- the cases' branches
def test_bg2_branches(tables):
    z4, z32 = tables["bg2_z4"], tables["bg2_z32"]
    assert z4["ct_aligned"] == 1 and z32["ct_aligned"] == 1
    assert z32["n_rw"] > 0
    # Z = 4: four checks per degree run fill a 32-lane unit too sparsely for the row walk
    assert z4["n_rw"] == 0 and z4["rw_d1"] == 0 and len(z4["rw_meta"]) == 0


def test_permuted_messages_are_not_aligned(tables, cases):
    t = tables["bg2_z4_permuted"]
    E = len(cases["bg2_z4_permuted"][0])
    assert t["ct_aligned"] == 0 and t["n_rw"] == 0
    assert t["ct_m0"].tolist() == list(range(0, E, 32)) + [E]  # plain 32-message tiles


def test_check_of_degree_40_is_not_aligned(tables, cases):
    assert np.bincount(cases["check_degree_40"][2]).max() == 40
    t = tables["check_degree_40"]
    assert t["ct_aligned"] == 0 and t["n_rw"] == 0 and t["ct_m0"].tolist() == [0, 32, 48]


def test_row_walk_with_degree_1_masks(tables):
    t = tables["lone_position_2"]
    assert t["ct_aligned"] == 1 and t["n_rw"] == 3 and t["rw_d1"] == 1
    rw = t["rw_meta"].reshape(3, 8)
    # {first message, checks, degree, mask} {first group, 0, 0, 0}: 100 % fill, bit 2 on the degree-3 units
    assert rw.tolist() == [[0, 32, 3, 4, 0, 0, 0, 0], [96, 32, 3, 4, 32, 0, 0, 0], [192, 32, 5, 0, 64, 0, 0, 0]]


def test_row_walk_without_masks(tables):
    t = tables["lone_position_moved"]
    assert t["ct_aligned"] == 1 and t["n_rw"] == 3 and t["rw_d1"] == 0
    rw = t["rw_meta"].reshape(3, 8)
    assert (rw[:, 3] == 0).all()
    assert rw[:, :3].tolist() == [[0, 32, 3], [96, 32, 3], [192, 32, 5]]


def test_sparse_fill_has_no_row_walk(tables):
    t = tables["alternating_degrees"]  # one check per unit: 1 / 32 of the slots, below 90 %
    assert t["ct_aligned"] == 1 and t["n_rw"] == 0 and t["rw_d1"] == 0


def test_non_consecutive_check_ids_have_no_row_walk(tables):
    t = tables["check_labels_reversed"]
    assert t["ct_aligned"] == 1 and t["n_rw"] == 0 and t["rw_d1"] == 0
    assert tables["lone_position_2"]["ct_m0"].tolist() == t["ct_m0"].tolist()


def test_empty_groups_appear_nowhere(tables):
    t = tables["empty_groups"]
    assert t["ct_aligned"] == 1  # an empty check group does not break the alignment
    inv = t["inv"].view(np.float32)
    assert inv[[0, 3, 6]].tolist() == [0, 0, 0] and inv[[7 + 0, 7 + 2, 7 + 5]].tolist() == [0, 0, 0]
    assert (inv != 0).sum() == 4 + 3
    assert not np.isin(t["gt_grp"], [0, 3, 6, 7 + 0, 7 + 2, 7 + 5]).any()
    side = np.repeat(t["pt_meta"].reshape(-1, 4)[:, 0], 32)
    assert not np.isin(t["pt_grp"][side == 0], [0, 3, 6]).any()
    assert not np.isin(t["pt_grp"][side == 1], [0, 2, 5]).any()


def test_message_counts_off_the_tile_size(tables, cases):
    for name, E in (("e45", 45), ("e7", 7), ("empty_groups", 10), ("alternating_degrees", 40)):
        assert len(cases[name][0]) == E and (E % 32 != 0)
        assert tables[name]["ct_m0"][-1] == E
    assert tables["e7"]["n_ctiles"] == 1 and tables["e7"]["n_mtiles"] >= 1


# ------------------------------------------------------------- the properties gnn.hpp states
def _members(labels, n):
    return [np.nonzero(labels == g)[0] for g in range(n)]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_table_properties(tables, cases, name):
    t = tables[name]
    vg, nv, cg, nc = cases[name]
    vg, cg = np.asarray(vg), np.asarray(cg)
    E = len(vg)
    vmem, cmem = _members(vg, nv), _members(cg, nc)
    vdeg, cdeg = np.array([len(m) for m in vmem]), np.array([len(m) for m in cmem])

    # the group CSR (members ascending) and 1 / |group|
    assert t["vgroup"].tolist() == vg.tolist() and t["cgroup"].tolist() == cg.tolist()
    for ptr, mem, members, deg in ((t["vg_ptr"], t["vg_mem"], vmem, vdeg), (t["cg_ptr"], t["cg_mem"], cmem, cdeg)):
        assert ptr.tolist() == np.concatenate([[0], np.cumsum(deg)]).tolist()
        assert mem.tolist() == np.concatenate(members).tolist()
    deg = np.concatenate([vdeg, cdeg])
    want_inv = np.where(deg > 0, np.float32(1) / np.maximum(deg, 1).astype(np.float32), np.float32(0))
    assert t["inv"].view(np.float32).tolist() == want_inv.astype(np.float32).tolist()

    # group tiles: 8 groups of one degree, var side then check side (check ids offset by Gv)
    gt_meta, gt_grp = t["gt_meta"].reshape(-1, 2), t["gt_grp"].reshape(-1, 8)
    assert len(gt_meta) == t["n_gtiles"] == len(gt_grp)
    real = gt_grp[gt_grp >= 0]
    assert sorted(real.tolist()) == np.nonzero(deg > 0)[0].tolist()  # every non-empty group exactly once
    assert (gt_grp[gt_grp < 0] == -1).all()
    members = vmem + cmem
    off = 0
    for k, ((d, o), grp) in enumerate(zip(gt_meta.tolist(), gt_grp.tolist())):
        assert o == off and d >= 1
        assert all((g < nv) == (k < t["n_gtiles_v"]) for g in grp if g >= 0)
        rows = t["gt_mem"][off:off + 8 * d].reshape(d, 8)
        for q, g in enumerate(grp):
            if g >= 0:
                assert deg[g] == d and rows[:, q].tolist() == members[g].tolist()
        assert grp[0] >= 0 and all(a >= 0 or b < 0 for a, b in zip(grp, grp[1:]))  # padding trails
        off += 8 * d
    assert off == len(t["gt_mem"])
    for side in (gt_meta[:t["n_gtiles_v"], 0], gt_meta[t["n_gtiles_v"]:, 0]):
        assert (np.diff(side) >= 0).all()  # each side ascends in degree
    assert t["n_gtiles_v1"] == int((gt_meta[:t["n_gtiles_v"], 0] == 1).sum())

    # projection tiles: 32 groups of one side, ids within the side
    pt_meta = t["pt_meta"].reshape(-1, 4)
    pt_grp, pt_deg = t["pt_grp"].reshape(-1, 32), t["pt_deg"].reshape(-1, 32)
    assert len(pt_meta) == t["n_ptiles"] == len(pt_grp) == len(pt_deg)
    assert pt_meta[:, 0].tolist() == [0] * t["n_ptiles_v"] + [1] * (t["n_ptiles"] - t["n_ptiles_v"])
    assert (pt_meta[:, 3] == 0).all()
    off = 0
    for (side, dmax, o, _), grp, dg in zip(pt_meta.tolist(), pt_grp.tolist(), pt_deg.tolist()):
        mem, sdeg = (vmem, vdeg) if side == 0 else (cmem, cdeg)
        assert o == off
        rows = t["pt_mem"][off:off + 32 * (dmax + 1)].reshape(dmax + 1, 32)  # dmax + 1 rows per tile
        assert dmax == max(dg)
        for q, (g, d) in enumerate(zip(grp, dg)):
            if g < 0:
                assert g == -1 and d == 0  # padding is -1 with degree 0
            else:
                assert d == sdeg[g] and d >= 1 and rows[:d, q].tolist() == mem[g].tolist()
            assert (rows[d:, q] == 0).all()  # rows past a group's degree are 0
        off += 32 * (dmax + 1)
    assert off == len(t["pt_mem"])
    for side, sdeg in ((0, vdeg), (1, cdeg)):
        sel = pt_meta[:, 0] == side
        g, d = pt_grp[sel].ravel(), pt_deg[sel].ravel()
        assert sorted(g[g >= 0].tolist()) == np.nonzero(sdeg > 0)[0].tolist()  # exactly once
        assert (np.diff(d[g >= 0]) >= 0).all()  # the side ascends in degree
        assert (g[:int((g >= 0).sum())] >= 0).all()  # padding only at the side's end
    v1 = [bool((pt_deg[k] <= 1).all()) for k in range(t["n_ptiles_v"])]
    assert t["n_ptiles_v1"] == (v1.index(False) if False in v1 else len(v1))

    # message permutation: degree-1 var groups' messages first, each part padded to whole tiles
    mt = t["mt_perm"]
    assert len(mt) == 32 * t["n_mtiles"] and len(mt) % 32 == 0
    d1 = vdeg[vg] == 1
    head, tail = mt[:32 * t["n_mtiles_v1"]], mt[32 * t["n_mtiles_v1"]:]
    for part, want in ((head, np.nonzero(d1)[0]), (tail, np.nonzero(~d1)[0])):
        assert len(part) == (len(want) + 31) // 32 * 32
        assert part[:len(want)].tolist() == want.tolist() and (part[len(want):] == -1).all()
    assert sorted(mt[mt >= 0].tolist()) == list(range(E))

    # message tiles of the bf16 MLP
    ct = t["ct_m0"]
    assert len(ct) == t["n_ctiles"] + 1 and ct[0] == 0 and ct[-1] == E
    assert (np.diff(ct) >= 1).all() and (np.diff(ct) <= 32).all()
    runs_ok = all(len(m) == 0 or (len(m) <= 32 and m[-1] - m[0] == len(m) - 1) for m in cmem)
    assert bool(t["ct_aligned"]) == runs_ok
    if t["ct_aligned"]:
        tile = np.searchsorted(ct, np.arange(E), side="right")
        assert all(len(np.unique(tile[m])) <= 1 for m in cmem)  # no check group straddles a boundary
    else:
        assert ct.tolist() == list(range(0, E, 32)) + [E]

    # row-walk units
    assert len(t["rw_meta"]) == 8 * t["n_rw"]
    assert t["rw_d1"] in (0, 1) and (t["n_rw"] > 0 or t["rw_d1"] == 0)
    m = 0
    for m0, n, d, mask, first, *zeros in t["rw_meta"].reshape(-1, 8).tolist():
        assert m0 == m and 1 <= n <= 32 and zeros == [0, 0, 0]
        for k in range(n):
            assert cmem[first + k].tolist() == list(range(m0 + k * d, m0 + (k + 1) * d))
        for i in range(d):
            if mask >> i & 1:
                assert d1[m0 + i:m0 + n * d:d].all()
        m += n * d
    if t["n_rw"]:
        assert m == E and E >= 0.9 * 32 * t["rw_meta"].reshape(-1, 8)[:, 2].sum()
        if t["rw_d1"]:  # every degree-1 message lies in a masked position
            masked = sum(n * bin(mask).count("1") for _, n, _, mask, *_ in t["rw_meta"].reshape(-1, 8).tolist())
            assert masked == int(d1.sum())


def test_argument_errors_match_plan_create():
    lib = N.lib()
    vg = np.array([0, 1, 2], dtype=np.int32)
    assert lib.ldpc_gnn_plan_tables(3, 2, vg.ctypes.data_as(_P), 3, vg.ctypes.data_as(_P), None, 0) == N.LDPC_EINVAL
    assert lib.ldpc_last_error() == b"group label out of range"
    assert lib.ldpc_gnn_plan_tables(0, 3, vg.ctypes.data_as(_P), 3, vg.ctypes.data_as(_P), None, 0) == N.LDPC_EINVAL
    assert lib.ldpc_last_error() == b"bad GNN plan arguments"
