"""The streaming layered decoder's runs and segments (csrc/layered_runs.cpp), read back through
ldpc_layered_runs on the host: no device is touched.

Every case is held to the properties include/ldpc_amd.h states for the tables, computed here in numpy
from the edge list alone: the runs partition [0, M) in order, the checks of a run are pairwise
variable-disjoint, the first check of a run shares a variable with the run before it (maximality),
the segments tile each run grouped by exact degree, and order is a permutation of [0, M)."""
import ctypes

import numpy as np
import pytest

from conftest import code_path

from ldpc_neural_decoder import _native as N
from ldpc_neural_decoder.utils import expand_base_matrix, load_base_matrix

_P = ctypes.c_void_p


def edges_of(H):
    chk, var = np.nonzero(np.asarray(H) != 0)  # row-major: checks ascending, variables ascending
    return chk.astype(np.int32), var.astype(np.int32)


def call(M, Nv, ec, ev, words=None, capacity=0):
    ec, ev = np.ascontiguousarray(ec, dtype=np.int32), np.ascontiguousarray(ev, dtype=np.int32)
    return N.lib().ldpc_layered_runs(int(M), int(Nv), len(ec), ec.ctypes.data_as(_P), ev.ctypes.data_as(_P),
                                     None if words is None else words.ctypes.data_as(_P), capacity)


def tables(M, Nv, ec, ev):
    need = call(M, Nv, ec, ev)
    assert need >= 3, N.lib().ldpc_last_error()
    words = np.full(need, -7, dtype=np.int32)
    assert call(M, Nv, ec, ev, words, need) == need
    n_runs, n_seg = int(words[0]), int(words[1])
    assert need == 2 + (n_runs + 1) + 4 * n_seg + M
    run_ptr = words[2:3 + n_runs]
    seg = words[3 + n_runs:3 + n_runs + 4 * n_seg].reshape(n_seg, 4)
    order = words[3 + n_runs + 4 * n_seg:]
    return run_ptr, seg, order


def check_properties(M, Nv, ec, ev):
    run_ptr, seg, order = tables(M, Nv, ec, ev)
    n_runs = len(run_ptr) - 1
    deg = np.bincount(ec, minlength=M)
    vars_of = np.split(ev, np.cumsum(deg)[:-1]) if M else []
    # the runs partition [0, M) in order
    assert run_ptr[0] == 0 and run_ptr[-1] == M
    assert (np.diff(run_ptr) > 0).all()
    assert (M == 0) == (n_runs == 0)
    run_vars = []
    for r in range(n_runs):
        members = np.concatenate([vars_of[i] for i in range(run_ptr[r], run_ptr[r + 1])] + [np.zeros(0, np.int32)])
        # pairwise variable-disjoint: no variable twice in the run
        assert len(np.unique(members)) == len(members), r
        run_vars.append(set(members.tolist()))
    # maximality: the first check of run r + 1 shares a variable with run r
    for r in range(n_runs - 1):
        assert run_vars[r] & set(vars_of[run_ptr[r + 1]].tolist()), r
    # the segments tile each run, grouped by exact degree, degrees ascending inside a run
    off = 0
    for k, (r, d, o, n) in enumerate(seg.tolist()):
        assert o == off and n > 0
        off += n
        checks = order[o:o + n]
        assert (deg[checks] == d).all()
        assert (np.diff(checks) > 0).all()  # ascending inside a segment
        assert (checks >= run_ptr[r]).all() and (checks < run_ptr[r + 1]).all()
        if k:
            pr, pd = seg[k - 1][0], seg[k - 1][1]
            assert r == pr and d > pd or r == pr + 1
        else:
            assert r == 0
    assert off == M
    for r in range(n_runs):  # a run's segments hold exactly its checks
        mine = seg[seg[:, 0] == r]
        assert mine[:, 3].sum() == run_ptr[r + 1] - run_ptr[r]
    # order is a permutation of [0, M)
    assert np.array_equal(np.sort(order), np.arange(M))
    return run_ptr, seg, order


def bg2(z):
    base_z = 4 if z == 4 else 32  # Z = 12 and 96 lift the Z = 32 base file, as test_flood_gpu does
    return expand_base_matrix(load_base_matrix(code_path(base_z)), z).numpy()


@pytest.mark.parametrize("z", [4, 12, 96])
def test_bg2_runs(z):
    H = bg2(z)
    ec, ev = edges_of(H)
    run_ptr, seg, _ = check_properties(*H.shape, ec, ev)
    lengths = np.diff(run_ptr)
    assert len(lengths) == 28
    assert (lengths % z == 0).all()
    assert set((lengths // z).tolist()) == {1, 2, 3}
    # adjacent block rows that share no column merge into one run: some run holds two degrees
    assert max(np.bincount(seg[:, 0])) >= 2


def random_H(dense_row):
    """The 24 x 50 graph of test_layered_gpu, restated."""
    rng = np.random.default_rng(2024)
    H = np.zeros((24, 50), dtype=np.float32)
    for j in range(48):
        H[rng.choice(24, size=3, replace=False), j] = 1
    H[5, 48] = 1   # two appended degree-1 columns
    H[20, 49] = 1
    if dense_row:  # check 11 gets degree >= 14
        H[11, rng.choice(48, size=14, replace=False)] = 1
    return H


@pytest.mark.parametrize("dense_row", [False, True])
def test_random_graph(dense_row):
    H = random_H(dense_row)
    run_ptr, _, _ = check_properties(*H.shape, *edges_of(H))
    assert 1 < len(run_ptr) - 1 <= 24


def test_empty_check_and_mixed_degrees():
    """Checks 0 (degree 2), 1 (degree 0), 2 (degree 3) and 3 (degree 2) share no variable: one run of
    three degrees; check 4 meets variable 0 again and opens the second run; check 5 is empty and joins it."""
    H = np.zeros((6, 9), dtype=np.float32)
    H[0, [0, 1]] = 1
    H[2, [2, 3, 4]] = 1
    H[3, [5, 6]] = 1
    H[4, [0, 7]] = 1
    run_ptr, seg, order = check_properties(*H.shape, *edges_of(H))
    assert run_ptr.tolist() == [0, 4, 6]
    assert seg.tolist() == [[0, 0, 0, 1], [0, 2, 1, 2], [0, 3, 3, 1], [1, 0, 4, 1], [1, 2, 5, 1]]
    assert order.tolist() == [1, 0, 3, 2, 5, 4]


def test_empty_graph():
    run_ptr, seg, order = check_properties(0, 5, np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert run_ptr.tolist() == [0] and len(seg) == 0 and len(order) == 0
    # checks without any edge: one run, one degree-0 segment
    run_ptr, seg, order = check_properties(3, 5, np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert run_ptr.tolist() == [0, 3] and seg.tolist() == [[0, 0, 0, 3]] and order.tolist() == [0, 1, 2]


def test_size_query_and_capacity():
    H = random_H(False)
    ec, ev = edges_of(H)
    need = call(24, 50, ec, ev)  # NULL buffer: the size alone
    assert need > 2 + 24
    words = np.full(need, -7, dtype=np.int32)
    assert call(24, 50, ec, ev, words, need - 1) == need  # too small: the size again, nothing written
    assert (words == -7).all()
    assert call(24, 50, ec, ev, None, need) == need       # NULL with a capacity: still the size alone
    assert call(24, 50, ec, ev, words, need) == need
    assert words[0] >= 1 and (words != -7).all()
    big = np.full(need + 5, -7, dtype=np.int32)
    assert call(24, 50, ec, ev, big, need + 5) == need
    assert np.array_equal(big[:need], words) and (big[need:] == -7).all()


def test_errors():
    H = random_H(False)
    ec, ev = edges_of(H)
    bad = ev.copy()
    bad[7] = 50  # an edge index out of range
    assert call(24, 50, ec, bad) == N.LDPC_EINVAL
    assert b"out of range" in N.lib().ldpc_last_error()
    bad = ec.copy()
    bad[0] = -1
    assert call(24, 50, bad, ev) == N.LDPC_EINVAL
    assert call(24, 50, ec[::-1], ev[::-1]) == N.LDPC_EINVAL  # not check-major
    assert b"check-major" in N.lib().ldpc_last_error()
    assert call(24, 0, ec[:0], ev[:0]) == N.LDPC_EINVAL      # as ldpc_graph_create: N must be positive
    assert N.lib().ldpc_layered_runs(24, 50, 3, None, None, None, 0) == N.LDPC_EINVAL
