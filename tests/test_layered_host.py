"""The layered min-sum reference (tests/layered_ref.py) pinned on the CPU: a hand-worked example, an
independent scalar restatement, its gain over flooding min-sum, and its per-frame stop."""
import numpy as np
import pytest

import layered_ref as LR
from conftest import code_path


@pytest.fixture(scope="module")
def codes(oracle_mod):
    out = {}
    for z in (4, 32):
        H = oracle_mod.expand(oracle_mod.load_base(code_path(z)), z)
        out[z] = (H, LR.Code(H), oracle_mod.Graph(H))
    return out


def llr_of(oracle_mod, B, n, snr):
    return oracle_mod.awgn_llr(B, n, snr, seed=7).astype(np.float32)


def test_hand_worked_example():
    """3 x 6 H, alpha 0.5: v5 has degree 1, llr[2] = 0 (sgn 0 = 0), |llr[0]| = |llr[1]| tie the
    min of check 0.  Worked by hand, check by check:
      it 1  c0: t = [2, -2, 0, 4]        -> c = [0, 0, -1, 0]  (only k = 2 excludes the zero;
                                                                min(2, 2, 4) = 2, sign -)
            c1: t = [-2, -1, -1]         -> c = [.5, .5, .5]
            c2: t = [2, 4, -.5, llr5=3]  -> c = [-.25, -.25, 1, -.25]
      it 2  c0: t = [1.75, -1.5, .5, 3.75]   -> c = [-.25, .25, -.75, -.25]
            c1: t = [-1.75, -.75, 0]         -> c = [0, 0, .375]
            c2: t = [1.75, 3.75, -.625, 3]   -> c = [-.3125, -.3125, .875, -.3125]"""
    H = np.array([[1, 1, 1, 1, 0, 0],
                  [0, 1, 1, 0, 1, 0],
                  [1, 0, 0, 1, 1, 1]])
    llr = np.array([[2, -2, 0, 4, -1, 3]], dtype=np.float32)
    code = LR.Code(H)
    assert code.deg1.tolist() == [False] * 5 + [True]
    trace = []
    bits, iters = LR.decode(code, llr, 2, alpha=0.5, trace=trace)
    app1 = [1.75, -1.5, -0.5, 3.75, 0.5, 2.75]
    c2v1 = [0, 0, -1, 0, .5, .5, .5, -.25, -.25, 1, -.25]
    app2 = [1.4375, -1.75, -0.75, 3.4375, 0.25, 2.6875]
    c2v2 = [-.25, .25, -.75, -.25, 0, 0, .375, -.3125, -.3125, .875, -.3125]
    assert np.array_equal(trace[0][0][0], np.array(app1, np.float32))
    assert np.array_equal(trace[0][1][0], np.array(c2v1, np.float32))
    assert np.array_equal(trace[1][0][0], np.array(app2, np.float32))
    assert np.array_equal(trace[1][1][0], np.array(c2v2, np.float32))
    assert trace[0][2][0].tolist() == [0, 1, 1, 0, 0, 0]
    assert bits[0].tolist() == [0, 1, 1, 0, 0, 0] and iters.tolist() == [2]
    sb, sa = LR.decode_scalar(code, llr, 2, alpha=0.5)
    assert np.array_equal(sa[0], np.array(app2, np.float32)) and np.array_equal(sb, bits)


def test_vectorised_equals_scalar_loop(oracle_mod, codes):
    H, code, _ = codes[4]
    llr = llr_of(oracle_mod, 8, code.N, -2.0)
    llr[3, 17] = 0.0
    for iters, alpha in ((1, 0.75), (3, 0.8)):
        trace = []
        bits, _ = LR.decode(code, llr, iters, alpha, trace=trace)
        sb, sa = LR.decode_scalar(code, llr, iters, alpha)
        assert np.array_equal(bits, sb)
        assert np.array_equal(trace[-1][0], sa)


@pytest.mark.parametrize("z,B,snr", [(4, 2048, -2.0), (32, 256, -3.0)])
def test_fewer_frame_errors_than_flooding(oracle_mod, codes, z, B, snr):
    """5 iterations, alpha 0.75, all-zero codeword: the layered schedule leaves strictly fewer
    frames in error than flooding min-sum (measured 377 vs 1204 at Z = 4, 177 vs 256 at Z = 32)."""
    _, code, g = codes[z]
    llr = llr_of(oracle_mod, B, code.N, snr)
    lb, _ = LR.decode(code, llr, 5, 0.75)
    fb = oracle_mod.flood_decode(g, llr, "minsum", 5, 0.75, 0)[0]
    fe_l, fe_f = int(lb.any(1).sum()), int(fb.any(1).sum())
    print(f"Z={z} B={B} {snr} dB: layered {fe_l} flooding {fe_f} frame errors")
    assert fe_l < fe_f


def test_frame_stop_semantics(oracle_mod, codes):
    """LDPC_ES_FRAME: a frame freezes at the FIRST iteration whose decisions satisfy H x = 0, with
    that iteration's bits and count; the others run max_iter."""
    _, code, _ = codes[32]
    llr = llr_of(oracle_mod, 96, code.N, -3.0)
    trace = []
    bits, iters = LR.decode(code, llr, 10, 0.75, LR.ES_FRAME, trace=trace)
    valid = np.stack([LR.syndrome_ok(code, t[2]) for t in trace], 1)  # (B, 10)
    ever = valid.any(1)
    print("stop iterations:", np.unique(iters[ever]).tolist(), "never valid:", int((~ever).sum()))
    assert len(np.unique(iters[ever])) >= 3 and (~ever).any() and ever.any()
    for b in range(96):
        first = int(np.argmax(valid[b])) + 1 if ever[b] else 10
        assert iters[b] == first
        assert np.array_equal(bits[b], trace[first - 1][2][b])
    off, it_off = LR.decode(code, llr, 10, 0.75, LR.ES_OFF)
    assert (it_off == 10).all() and np.array_equal(off[~ever], bits[~ever])
    with pytest.raises(ValueError):
        LR.decode(code, llr[:1], 2, 0.75, LR.ES_BATCH)
