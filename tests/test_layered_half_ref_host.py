"""The half-precision layered min-sum reference (tests/layered_half_ref.py) pinned on the CPU: exact where
binary16 is exact, an independent scalar restatement, the clamp, the degree-1 check, that it is not the float32
decoder, and the Python constructor's precision switch."""
import numpy as np
import pytest

import layered_half_ref as LHR
import layered_ref as LR
from conftest import code_path


def tiny_H():
    """3 x 6 with one degree-1 check (check 1 holds variable 5 alone) and a degree-1 variable (4)."""
    return np.array([[1, 1, 1, 0, 1, 0],
                     [0, 0, 0, 0, 0, 1],
                     [0, 1, 1, 1, 0, 1]], dtype=np.float32)


@pytest.fixture(scope="module")
def z4(oracle_mod):
    H = oracle_mod.expand(oracle_mod.load_base(code_path(4)), 4)
    return H, LHR.Code(H)


def test_exact_case_equals_float32(z4):
    """LLRs k / 4 in [-4, 4], alpha 1.0, 3 iterations: every value is a multiple of 1/4 below 2048, binary16 is
    exact, so decisions and posteriors equal the float32 layered restatement's.  (alpha 0.5 does not work
    here: the layers chain the scaling and the values leave 11 bits within one iteration.)"""
    _, code = z4
    rng = np.random.default_rng(11)
    llr = (rng.integers(-16, 17, size=(16, code.N)) / 4.0).astype(np.float32)
    assert (llr == 0).any()
    trace, rtrace = [], []
    bits, iters = LHR.decode(code, llr, 3, 1.0, trace=trace)
    rb, _ = LR.decode(code, llr, 3, 1.0, trace=rtrace)
    top = max(float(np.abs(a).max()) for t in trace for a in t[:2])
    print("largest |value|:", top)
    assert top < 2048
    assert np.array_equal(bits, rb) and (iters == 3).all()
    for t, r in zip(trace, rtrace):
        assert np.array_equal(t[0].astype(np.float32), r[0])
        assert np.array_equal(t[2], r[2])


@pytest.mark.parametrize("alpha", [0.75, 0.8])
def test_vectorised_equals_scalar(oracle_mod, z4, alpha):
    _, code = z4
    llr = LHR.with_specials(oracle_mod.awgn_llr(6, code.N, -2.0, seed=7).astype(np.float32))
    for v in LHR.SPECIALS:
        assert (llr == v).any()
    for es in (LHR.ES_OFF, LHR.ES_FRAME):
        trace = []
        bits, iters = LHR.decode(code, llr, 5, alpha, es, trace=trace)
        sb, si, sa = LHR.decode_scalar(code, llr, 5, alpha, es)
        assert np.array_equal(bits, sb) and np.array_equal(iters, si)
        app = np.stack([trace[iters[b] - 1][0][b] for b in range(len(llr))])
        assert np.isfinite(app).all() and np.array_equal(app, sa)


def test_clamp_engages_and_bounds_everything(oracle_mod, z4, monkeypatch):
    _, code = z4
    llr = LHR.saturating(oracle_mod.awgn_llr(8, code.N, 0.0, seed=7))
    over = [0]
    plain = LHR._clamp

    def counting(v, clamp):
        if clamp is not None:
            over[0] += int((np.abs(v) > clamp).sum())
        return plain(v, clamp)

    monkeypatch.setattr(LHR, "_clamp", counting)
    held, free = [], []
    hb, _ = LHR.decode(code, llr, 50, 0.75, trace=held)
    engaged = over[0]
    fb, _ = LHR.decode(code, llr, 50, 0.75, trace=free, clamp=None)
    top_c2v = max(float(np.abs(t[1]).max()) for t in held)
    top_app = max(float(np.abs(t[0]).max()) for t in held)
    differ = int((hb != fb).any(axis=1).sum())
    print(f"|app - c2v| > 1024 before the clamp: {engaged}; max |c2v| {top_c2v}, max |app| {top_app}; "
          f"frames whose decisions differ without the clamp: {differ}")
    assert engaged > 0
    assert top_c2v <= 1024 and top_app <= 2048
    assert all(np.isfinite(a).all() for t in held for a in t[:2])
    assert differ >= 1


def test_clamp_engages_in_iteration_one(oracle_mod, z4, monkeypatch):
    """LLRs scaled by 256: posteriors pass C inside iteration 1, where c2v is still +0, so t = clamp(app) is
    not clamp(x) = x; a decoder without that clamp decides otherwise.  The GPU test uses this input."""
    _, code = z4
    llr = LHR.saturating(oracle_mod.awgn_llr(64, code.N, 0.0, seed=3), 256.0)
    over = [0]
    plain = LHR._clamp

    def counting(v, clamp):
        if clamp is not None:
            over[0] += int((np.abs(v) > clamp).sum())
        return plain(v, clamp)

    monkeypatch.setattr(LHR, "_clamp", counting)
    trace = []
    LHR.decode(code, llr, 1, 0.75, trace=trace)
    wrong = LHR.first_iteration_unclamped(code, llr, 0.75)
    differ = int((wrong != trace[0][2]).sum())
    print(f"|app - c2v| > 1024 in iteration 1: {over[0]}; bits that differ without that clamp: {differ}")
    assert over[0] > 0 and differ >= 1
    assert float(np.abs(trace[0][0]).max()) <= 2048 and float(np.abs(trace[0][1]).max()) <= 1024


def test_degree_one_check_sends_a_times_c():
    H = tiny_H()
    code = LHR.Code(H)
    assert (H.sum(1) == 1).tolist() == [False, True, False]
    rng = np.random.default_rng(3)
    llr = rng.normal(1.0, 2.0, size=(9, 6)).astype(np.float32)
    for alpha in (0.75, 1.0):
        trace = []
        bits, _ = LHR.decode(code, llr, 4, alpha, trace=trace)
        a = LHR.half_alpha(alpha)
        e = int(code.chk_ptr[1])
        for app, c2v, _ in trace:
            assert np.isfinite(app).all() and np.isfinite(c2v).all()
            assert (c2v[:, e] == a * np.float16(1024)).all()  # the empty sign product is +1
        sb, _, _ = LHR.decode_scalar(code, llr, 4, alpha)
        assert np.array_equal(bits, sb)


def test_fp16_is_not_fp32(oracle_mod):
    """The two restatements disagree on real inputs, so a build that ran the float32 kernels under the fp16
    switch cannot pass the exactness tests."""
    H = oracle_mod.expand(oracle_mod.load_base(code_path(32)), 12)
    code = LHR.Code(H)
    llr = oracle_mod.awgn_llr(300, code.N, -3.0, seed=7).astype(np.float32)
    hb, hi = LHR.decode(code, llr, 8, 0.75, LHR.ES_FRAME)
    fb, fi = LR.decode(code, llr, 8, 0.75, LR.ES_FRAME)
    nb, ni = int((hb != fb).any(axis=1).sum()), int((hi != fi).sum())
    print(f"frames that differ in bits {nb}, in iteration count {ni}")
    assert nb >= 1


def test_constructor_precision_switch(z4):
    import torch

    from ldpc_neural_decoder import _native as N
    from ldpc_neural_decoder.models import LayeredMinSumDecoder

    H4 = torch.from_numpy(np.asarray(z4[0], dtype=np.float32))
    assert N.LDPC_ALGO_LAYERED_MINSUM_F16 == 6
    for es in (True, "frame", False):
        assert LayeredMinSumDecoder(H4, precision="fp16", early_stopping=es)._algo == 6
        assert LayeredMinSumDecoder(H4, precision="fp16", early_stopping=es, any_graph=True)._algo == 6
    assert LayeredMinSumDecoder(H4, precision="fp16")._es_mode() == N.LDPC_ES_FRAME
    assert LayeredMinSumDecoder(H4, precision="fp16", early_stopping=False)._es_mode() == N.LDPC_ES_OFF
    with pytest.raises(ValueError):
        LayeredMinSumDecoder(H4, precision="bf16")
    assert LayeredMinSumDecoder(H4)._algo == LayeredMinSumDecoder(H4, precision="fp32")._algo == 2
    assert LayeredMinSumDecoder(H4, any_graph=True)._algo == 3
    assert LayeredMinSumDecoder(H4, any_graph=True, precision="fp32")._algo == 3
