"""Fixed flood kernel: the iteration driver's loop and its peeled last iteration (GPU).

flood_drive runs the iterations before the last in a loop that takes no decisions, and the last one
behind it as straight code that stores the decisions in the caller's output type; the bail-out
instances (min-sum with a workspace) test the sticky non-finite flag at the head of both, the others
branch to the exact check update there.  What that can get wrong is checked here against the oracle, exactly:
bits (uint8 and float32 outputs), per-frame iteration counts (asked for or not), the four counters,
and which groups ldpc_flood_redo_count lists.

  iterations 1, 2, 3, 10   at 1 the loop never runs, at 2 it runs once
  stopping off / per frame, with a workspace (bail-out instances) and without (exact update inside)
  shapes (Z = 32, B = 5) and (Z = 4, B = 37): three groups, the last a tail group of 1 / 5 frames
  LLRs on the grid k / 4, |k| <= 12 (ties, exact zeros), and per input kind
    "grid"  nothing else: every group stays on the fast update
    "first" group 0 holds a NaN LLR, the tail group a +inf LLR (flag raised in init, read at the first
            head: the loop's, or the last iteration's at 1), the middle group a finite frame whose APP overflows in the
            first iteration: the flag goes up in that iteration's variable phase and is read by the
            peeled last iteration at 2 iterations, by the loop at 3 and 10, never at 1
    "second" group 0 holds a -inf LLR, the tail group a NaN, the middle group a frame whose APP
            overflows in the second iteration: read by the last iteration at 3, by the loop at 10,
            never at 1 and 2
Which iteration a frame overflows in is asserted with the oracle on the CPU (overflow_frame); the
expected redo list is derived from the oracle as in test_flood_bail_redo_gpu.py.

BP shares flood_drive (no bail-out, no redo list).  Its tanh / atanh differ from the oracle's by a
few ulp (test_flood_gpu.py), so the oracle cannot be an exact reference for it: it is held, exactly,
to the table-driven kernel, whose driver keeps the one-loop form, and to the oracle within the bar
of test_flood_gpu.py (1e-4 of all bits).
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import code_path

from ldpc_neural_decoder import _native as N
from ldpc_neural_decoder.models import BeliefPropagationDecoder, MinSumScaledDecoder
from ldpc_neural_decoder.utils import expand_base_matrix, load_base_matrix

pytestmark = pytest.mark.gpu
ALPHA = 0.75
ITERS = (1, 2, 3, 10)
SHAPES = [(32, 5), (4, 37)]
KINDS = ["grid", "first", "second"]
ES = {"off": (N.LDPC_ES_OFF, 0), "frame": (N.LDPC_ES_FRAME, 2)}
# finite frames +-mag whose APP first overflows after `first` iterations: (seed, share of minus signs, mag)
OVERFLOW = {(32, 1): (5, 0.1, 3e38), (32, 2): (5, 0.1, 2.3e37), (4, 1): (5, 0.1, 3e38), (4, 2): (7, 0.05, 2.2e37)}


@pytest.fixture(scope="module")
def codes(oracle_mod, cuda):
    out = {}
    for z in (32, 4):
        H = expand_base_matrix(load_base_matrix(code_path(z)), z)
        ms = MinSumScaledDecoder(H, 10, ALPHA, early_stopping=False)
        bp = BeliefPropagationDecoder(H, 10, early_stopping=False)
        out[z] = (ms.graph(cuda), oracle_mod.Graph(H.numpy()), bp.graph(cuda), ms, bp)
    return out


def overflow_frame(oracle_mod, og, z, first):
    seed, share, mag = OVERFLOW[z, first]
    rng = np.random.default_rng(seed)
    x = (np.where(rng.random(52 * z) < share, -1.0, 1.0) * mag).astype(np.float32)
    assert np.isfinite(x).all()
    for t in range(1, first + 1):
        _, app, _, _ = oracle_mod.flood_decode(og, x[None], "minsum", t, ALPHA, 0)
        assert np.isfinite(app).all() == (t < first), (z, first, t)
    return x


def make_input(oracle_mod, og, z, B, kind):
    fg = 64 // z
    ng = (B + fg - 1) // fg
    assert ng == 3 and 0 < B - 2 * fg < fg  # three groups, the last a tail group
    rng = np.random.default_rng(9100 + z)
    x = (rng.integers(-12, 13, size=(B, 52 * z)) / 4).astype(np.float32)
    assert (x == 0).any()
    if kind != "grid":
        first = kind == "first"
        x[1, 7 * z + 2] = np.nan if first else -np.inf        # group 0, not frame 0 (tail lanes compute on it)
        x[B - 1, 30 * z + 1] = np.inf if first else np.nan    # the tail group; column 30 has degree 1
        x[fg + 1 if fg > 1 else fg] = overflow_frame(oracle_mod, og, z, 1 if first else 2)  # the middle group
    return x


class Ref:
    """the oracle's results for one input, computed once per (iterations, stopping mode)"""

    def __init__(self, oracle_mod, og, x, z, algo="minsum"):
        self.o, self.og, self.x, self.z, self.algo = oracle_mod, og, x, z, algo
        self.dec, self.bad_after = {}, {}

    def decode(self, iters, mode):
        if (iters, mode) not in self.dec:
            bits, _, n, fi = self.o.flood_decode(self.og, self.x, self.algo, iters, ALPHA, mode)
            self.dec[iters, mode] = (bits, n, fi)
        return self.dec[iters, mode]

    def redo(self, iters, mode):
        """groups that meet a non-finite value while another check phase is still to come"""
        fg = 64 // self.z
        grp = np.arange(self.x.shape[0]) // fg
        runs = np.full(grp.max() + 1, iters)
        if mode == 2:  # a group iterates until all of its frames have stopped
            fi = self.decode(iters, 2)[2]
            runs = np.array([fi[grp == q].max() for q in range(grp.max() + 1)])
        bad = {int(q) for q in grp[~np.isfinite(self.x).all(axis=1)]}
        for t in range(1, iters):
            if t not in self.bad_after:
                _, app, _, _ = self.o.flood_decode(self.og, self.x, "minsum", t, ALPHA, 0)
                self.bad_after[t] = ~np.isfinite(app).all(axis=1)
            bad |= {int(q) for q in grp[self.bad_after[t]] if t < runs[q]}
        return sorted(bad)


def decode(g, algo, x, iters, es, cuda, out, want_iters, work):
    """-> bits as uint8, iters_out or None, batch iterations or None, counters or None, redo list or None"""
    B = x.shape[0]
    llr = torch.from_numpy(x).to(cuda)
    f32 = out == N.LDPC_OUT_F32
    bits = torch.full((B, g.N), 7, dtype=torch.float32 if f32 else torch.uint8, device=cuda)
    fi = torch.full((B,), -1, dtype=torch.int32, device=cuda) if want_iters else None
    s = N.stream_ptr(cuda)
    p = lambda t: N.ptr(t) if t is not None else None
    bi = cnt = ws = listed = None
    wsb = 0
    if work:
        bi = torch.zeros(1, dtype=torch.int32, device=cuda)
        cnt = torch.zeros(4, dtype=torch.int64, device=cuda)
        wsb = N.check(N.lib().ldpc_flood_workspace_size(g.handle, B, iters, es))
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=cuda)
    N.check(N.lib().ldpc_flood_decode(g.handle, algo, N.ptr(llr), B, iters, ALPHA, es, out, N.ptr(bits), p(fi), p(bi),
                                      p(cnt), p(ws), wsb, s))
    if work and algo == N.LDPC_ALGO_MINSUM:
        n = ctypes.c_int32(-1)
        buf = (ctypes.c_int32 * (B + 1))()
        N.check(N.lib().ldpc_flood_redo_count(g.handle, algo, B, iters, es, N.ptr(ws), s, ctypes.byref(n), buf))
        listed = sorted(buf[i] for i in range(n.value))
    torch.cuda.synchronize()
    b = bits.cpu().numpy()
    if f32:
        assert np.isin(b, (0.0, 1.0)).all()  # every element written, as exactly 0.0 or 1.0
    return (b.astype(np.uint8), None if fi is None else fi.cpu().numpy(), None if bi is None else int(bi.item()),
            None if cnt is None else cnt.cpu().numpy().tolist(), listed)


def counters(bits, it):
    return [int(bits.sum()), int((bits.sum(1) > 0).sum()), bits.shape[0], int(it.sum())]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("z,B", SHAPES)
def test_loop_and_peeled_last_iteration(cuda, oracle_mod, codes, z, B, kind):
    g, og = codes[z][0], codes[z][1]
    x = make_input(oracle_mod, og, z, B, kind)
    ref = Ref(oracle_mod, og, x, z)
    assert g.set_variant(0) == (2 if z == 32 else 1)
    for iters in ITERS:
        for name, (es, mode) in ES.items():
            rbits, rn, ri = ref.decode(iters, mode)
            want = ref.redo(iters, mode)
            if kind == "grid":
                assert want == []
            elif name == "off":  # group 0 and the tail group from init, the middle one once its flag is read
                after = 1 if kind == "first" else 2
                assert want == ([0, 1, 2] if iters > after else [0, 2]), (iters, want)
            for work in (True, False):
                for out in (N.LDPC_OUT_U8, N.LDPC_OUT_F32):
                    for want_iters in (True, False):
                        where = (z, B, kind, iters, name, work, out, want_iters)
                        bits, fi, bi, cnt, listed = decode(g, N.LDPC_ALGO_MINSUM, x, iters, es, cuda, out, want_iters, work)
                        assert np.array_equal(bits, rbits), where
                        if want_iters:
                            assert np.array_equal(fi, ri), where
                        if work:
                            assert bi == (iters if name == "off" else ri.max()), where
                            assert cnt == counters(rbits, ri), where
                            assert listed == want, where


def test_bp_shares_the_driver(cuda, oracle_mod, codes):
    z, B = 32, 5
    g_ms, og, g, _, _ = codes[z]
    x = make_input(oracle_mod, og, z, B, "grid")
    ref = Ref(oracle_mod, og, x, z, "bp")
    for iters in ITERS:
        for name, (es, mode) in ES.items():
            rbits, rn, ri = ref.decode(iters, mode)
            assert g.set_variant(1) == 0  # table-driven: one loop for every iteration
            tab = {out: decode(g, N.LDPC_ALGO_BP, x, iters, es, cuda, out, True, True) for out in (N.LDPC_OUT_U8, N.LDPC_OUT_F32)}
            assert g.set_variant(0) == 2
            for work in (True, False):
                for out in (N.LDPC_OUT_U8, N.LDPC_OUT_F32):
                    for want_iters in (True, False):
                        where = (iters, name, work, out, want_iters)
                        bits, fi, bi, cnt, _ = decode(g, N.LDPC_ALGO_BP, x, iters, es, cuda, out, want_iters, work)
                        assert np.array_equal(bits, tab[out][0]), where
                        assert (bits != rbits).mean() <= 1e-4, where
                        if want_iters:
                            assert np.array_equal(fi, tab[out][1]), where
                        if work:
                            assert bi == tab[out][2] and cnt == tab[out][3], where
                            assert cnt[:3] == counters(bits, np.zeros(B))[:3], where
                        if name == "off":
                            assert fi is None or (fi == iters).all(), where
