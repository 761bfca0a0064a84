"""The oracle's second BP rounding and the per-variable rule's own arithmetic (no GPU)."""
import numpy as np
import pytest

from conftest import code_path

from bp_rule import MARGIN, Rule, classify, on_codewords, qpsk_llr, random_codewords


@pytest.fixture
def bp_math(oracle_mod):
    """sets the oracle's BP math mode; mode 0 is back whatever the test does"""
    try:
        yield oracle_mod.set_bp_math
    finally:
        oracle_mod.set_bp_math(0)


@pytest.fixture(scope="module")
def small(oracle_mod):
    H = oracle_mod.expand(oracle_mod.load_base(code_path(4)), 4)
    rng = np.random.default_rng(8)
    x = on_codewords(qpsk_llr(rng, 8, 208, -4.0, clip=8.0), random_codewords(H, rng, 8))
    return oracle_mod.Graph(H), H, x


def test_set_bp_math_changes_bp_by_rounding_only(oracle_mod, bp_math, small):
    """Mode 1 (tanhf / atanhf) moves BP's APPs, by less than 1e-3, and leaves min-sum untouched."""
    g, _, x = small
    assert bp_math(0) == 0
    b0, a0, _, _ = oracle_mod.flood_decode(g, x, "bp", 4, 0.0, 0)
    m0 = oracle_mod.flood_decode(g, x, "minsum", 4, 0.75, 0)
    assert bp_math(1) == 1
    b1, a1, _, _ = oracle_mod.flood_decode(g, x, "bp", 4, 0.0, 0)
    m1 = oracle_mod.flood_decode(g, x, "minsum", 4, 0.75, 0)
    assert np.isfinite(a0).all() and np.isfinite(a1).all()
    diff = float(np.abs(a0 - a1).max())
    assert 0 < diff < 1e-3, diff
    assert np.array_equal(m0[0], m1[0]) and np.array_equal(m0[1], m1[1])
    assert bp_math(0) == 0
    again = oracle_mod.flood_decode(g, x, "bp", 4, 0.0, 0)
    assert np.array_equal(again[1], a0) and np.array_equal(again[0], b0)


def test_rule_restores_mode_zero(oracle_mod, small):
    g, _, x = small
    r = Rule(oracle_mod, g, x, 3)
    assert oracle_mod.set_bp_math(0) == 0  # returns the mode in use: it was put back
    assert np.array_equal(oracle_mod.flood_decode(g, x, "bp", 3, 0.0, 0)[1], r.a[0, 2])
    assert r.clean.shape == (8,) and r.decided.shape == (3, 8, 208) and r.d.shape == (3, 8)
    assert r.clean.mean() >= 0.75
    # a bit flipped on a decided variable is caught, one on a variable outside the rule is not
    got = r.b[0, 2].copy()
    assert r.check_bits(got, 3) == 0
    f, v = np.argwhere(r.decided[2])[0]
    got[f, v] ^= 1
    with pytest.raises(AssertionError, match="decided bits differ"):
        r.check_bits(got, 3)


def test_classify():
    inf, nan = np.inf, np.nan
    #             equal inf  finite  inf/finite  NaN    weak   signs differ
    a0 = np.array([[[inf,    4.0,    inf,        nan,   0.01,  -1e-4]]], np.float32)
    a1 = np.array([[[inf,    4.001,  50.0,       1.0,   0.01,   1e-4]]], np.float32)
    d, decided, clean = classify(a0, a1, (a0 < 0), (a1 < 0))
    assert d.shape == (1, 1) and abs(d[0, 0] - 0.001) < 1e-6  # inf - inf, inf - 50 and NaN do not count
    assert decided[0, 0].tolist() == [True, True, True, False, False, False]
    assert 0.01 < MARGIN * d[0, 0] < 4.0 and not clean[0]
    z = np.zeros((2, 1, 3), np.float32)  # identical runs: d = 0, an APP of exactly 0 is decided
    d, decided, clean = classify(z, z, z < 0, z < 0)
    assert not d.any() and decided.all() and clean.all()


@pytest.mark.parametrize("kind", ["bg2_z4", "hamming", "random"])
def test_random_codewords(oracle_mod, small, kind):
    if kind == "bg2_z4":
        H = small[1]
    elif kind == "hamming":
        H = np.array([[1, 1, 0, 1, 1, 0, 0], [1, 0, 1, 1, 0, 1, 0], [0, 1, 1, 1, 0, 0, 1]], np.uint8)
    else:
        rng = np.random.default_rng(5)
        H = np.zeros((30, 60), np.uint8)
        for j in range(60):
            H[rng.choice(30, size=3, replace=False), j] = 1
    cw = random_codewords(H, np.random.default_rng(1), 32)
    assert cw.shape == (32, H.shape[1]) and cw.dtype == np.uint8
    assert not ((cw.astype(np.int64) @ H.T.astype(np.int64)) % 2).any()
    assert 0.3 < cw.mean() < 0.7 and len({c.tobytes() for c in cw}) > 8
    x = np.full(cw.shape, 2.5, np.float32)
    assert np.array_equal(on_codewords(x, cw) < 0, cw.astype(bool))
