"""The per-variable bar for sum-product decoders (shared by test_flood_bp_gpu.py and test_flood_gpu.py).

Two legitimate float32 implementations of BP disagree in the last bits of tanh / atanh, and the
disagreement grows through the iterations of a frame.  The oracle therefore decodes every input
twice, with tanh / atanh evaluated in double and rounded once (mode 0) and with the C library's
tanhf / atanhf (mode 1), for t = 1 .. T iterations without early stop: APPs a0[t], a1[t], bits
b0[t], b1[t].  Per frame and iteration d = the largest finite |a0 - a1| of the frame (two equal
infinities count as 0).  A variable is DECIDED at t when neither APP is NaN, b0 == b1 and
min(|a0|, |a1|) >= 32 d.  A frame is CLEAN when every variable is decided at every t <= T.

The two oracle modes are each within 1 ulp per function; the kernel's functions are within a few
ulp (test_bp_math_gpu.py), so a margin of 32 times the observed disagreement of the whole frame
leaves a kernel with correct math no way to flip a decided variable, and any bit that differs on
one is a fault.  Tests assert a floor on the share of clean frames so that the rule cannot quietly
excuse a batch.
"""
import os

import numpy as np

MARGIN = 32.0
MIN_CLEAN = 0.75


def qpsk_llr(rng, B, n, snr_db, clip=None):
    """QPSK / AWGN LLRs of the all-zero codeword: mean 2 s / sqrt 2, s = 10^(snr/10)"""
    s = 10 ** (snr_db / 10)
    x = (2 * s * (1 / np.sqrt(2) + rng.normal(0, np.sqrt(1 / (2 * s)), size=(B, n)))).astype(np.float32)
    return np.clip(x, -clip, clip) if clip else x


def random_codewords(H, rng, n):
    """n random codewords (n, N) uint8 of the parity-check matrix H (M, N), so that a decoder's
    decisions are about half ones: with the all-zero codeword a NaN APP (bit 0) is the right answer.
    A check that holds a degree-1 variable gives that variable the parity of its others; the checks
    without one (the core) are solved by elimination over GF(2); everything else is drawn."""
    H = (np.asarray(H) != 0).astype(np.uint8)
    M, N = H.shape
    deg1 = H.sum(0) == 1
    dep = np.full(M, -1)  # the degree-1 variable that check i determines
    for j in np.flatnonzero(deg1):
        i = int(np.flatnonzero(H[:, j])[0])
        if dep[i] < 0:
            dep[i] = j
    core_rows = np.flatnonzero(dep < 0)
    cols = np.flatnonzero(~deg1)
    A = H[np.ix_(core_rows, cols)].copy()
    assert not H[core_rows][:, deg1].any()
    piv = []  # (row, column) of the reduced row echelon form
    r = 0
    for c in range(A.shape[1]):
        if r == A.shape[0]:
            break
        hit = np.flatnonzero(A[r:, c])
        if hit.size == 0:
            continue
        A[[r, r + hit[0]]] = A[[r + hit[0], r]]
        others = np.flatnonzero(A[:, c])
        others = others[others != r]
        A[others] ^= A[r]
        piv.append((r, c))
        r += 1
    pc = np.array([c for _, c in piv], dtype=int)
    free = np.setdiff1d(np.arange(A.shape[1]), pc)
    cw = np.zeros((n, N), np.uint8)
    cw[:, deg1] = rng.integers(0, 2, size=(n, int(deg1.sum())))  # the dependent ones are overwritten below
    sub = np.zeros((n, A.shape[1]), np.uint8)
    sub[:, free] = rng.integers(0, 2, size=(n, free.size))
    for rr, c in piv:  # reduced form: pivot variable = parity of the row's free variables
        sub[:, c] = (sub[:, free] @ A[rr, free].astype(np.int64)) % 2
    cw[:, cols] = sub
    for i in np.flatnonzero(dep >= 0):
        cw[:, dep[i]] = 0
        cw[:, dep[i]] = (cw @ H[i].astype(np.int64)) % 2
    assert not ((cw.astype(np.int64) @ H.T.astype(np.int64)) % 2).any()
    return cw


def on_codewords(x, cw):
    """LLRs of the all-zero codeword -> the same noise on the codewords cw (exact sign flips)"""
    return np.where(cw != 0, -x, x).astype(np.float32)


def classify(a0, a1, b0, b1):
    """APPs / bits (T, B, N) of the two oracle modes -> d (T, B), decided (T, B, N), clean (B,)"""
    with np.errstate(invalid="ignore"):
        diff = np.where(a0 == a1, np.float32(0), np.abs(a0 - a1))  # two equal infinities count as 0
        d = np.where(np.isfinite(diff), diff, 0).max(axis=2)
        decided = (~np.isnan(a0) & ~np.isnan(a1) & (b0 == b1) &
                   (np.minimum(np.abs(a0), np.abs(a1)) >= MARGIN * d[:, :, None]))
    return d, decided, decided.all(axis=(0, 2))


class Rule:
    """Oracle runs of one input batch in both math modes and the classification above.
    a[m], b[m]: (T, B, N) APPs / bits of mode m after t = 1 .. T iterations; d (T, B);
    decided (T, B, N); clean (B,)."""

    def __init__(self, oracle_mod, g, x, T):
        self.g, self.x, self.T = g, np.ascontiguousarray(x, dtype=np.float32), T
        self._o = oracle_mod
        B, n = self.x.shape
        self.a = np.empty((2, T, B, n), np.float32)
        self.b = np.empty((2, T, B, n), np.uint8)
        oracle_mod.set_threads(min(16, os.cpu_count() or 1))
        try:
            for m in (0, 1):
                oracle_mod.set_bp_math(m)
                for t in range(1, T + 1):
                    self.b[m, t - 1], self.a[m, t - 1], _, _ = oracle_mod.flood_decode(g, self.x, "bp", t, 0.0, 0)
        finally:
            oracle_mod.set_bp_math(0)
            oracle_mod.set_threads(1)
        self.d, self.decided, self.clean = classify(self.a[0], self.a[1], self.b[0], self.b[1])

    def stopped(self, es):
        """mode-0 oracle decode of the batch under early stop es (1 batch, 2 frame)"""
        return self._o.flood_decode(self.g, self.x, "bp", self.T, 0.0, es)

    def check_bits(self, got, t, frames=None, where=""):
        """got (len(frames), N) decisions after t iterations without stop: equal to the oracle's on
        every variable of a clean frame and on every decided variable of the others.  Returns the
        number of differing bits on non-decided variables (permitted, reported)."""
        frames = np.arange(self.x.shape[0]) if frames is None else np.asarray(frames)
        ref = self.b[0, t - 1][frames]
        must = self.decided[t - 1][frames] | self.clean[frames][:, None]
        bad = (got != ref) & must
        assert not bad.any(), (f"{where} t={t}: {int(bad.sum())} decided bits differ, frames "
                               f"{frames[bad.any(1)][:8].tolist()} (clean: {self.clean[frames][bad.any(1)][:8].tolist()})")
        return int(((got != ref) & ~must).sum())

    def check_floor(self, frames=None):
        c = self.clean if frames is None else self.clean[np.asarray(frames)]
        assert c.mean() >= MIN_CLEAN, f"only {int(c.sum())} of {c.size} frames are clean: the rule would excuse the batch"
