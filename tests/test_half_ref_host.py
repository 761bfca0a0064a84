"""The half-precision min-sum reference (tests/half_ref.py) pinned on the CPU: exact where binary16 is exact,
an independent scalar restatement, the clamp, and the Python constructor's refusals."""
import numpy as np
import pytest

import half_ref as HR
from conftest import code_path


@pytest.fixture(scope="module")
def z4(oracle_mod):
    H = oracle_mod.expand(oracle_mod.load_base(code_path(4)), 4)
    return H, HR.Code(H), oracle_mod.Graph(H)


def test_exact_case_equals_float32(oracle_mod, z4):
    """LLRs k / 4 in [-4, 4], alpha 0.5, 3 iterations: every intermediate is a small dyadic number, binary16
    is exact, so decisions and posteriors equal the float32 flooding min-sum's."""
    _, code, g = z4
    rng = np.random.default_rng(11)
    llr = (rng.integers(-16, 17, size=(16, code.N)) / 4.0).astype(np.float32)
    assert (llr == 0).any()
    trace = []
    bits, iters = HR.decode(code, llr, 3, 0.5, trace=trace)
    top = max(float(np.abs(a).max()) for t in trace for a in t[:3])
    print("largest |value|:", top)
    assert top < 2048
    rb, rapp, _, _ = oracle_mod.flood_decode(g, llr, "minsum", 3, 0.5, 0)
    assert np.array_equal(bits, rb) and (iters == 3).all()
    assert np.array_equal(trace[-1][0].astype(np.float32), rapp)


@pytest.mark.parametrize("alpha", [0.75, 0.8])
def test_vectorised_equals_scalar(oracle_mod, z4, alpha):
    _, code, _ = z4
    llr = HR.with_specials(oracle_mod.awgn_llr(6, code.N, -2.0, seed=7).astype(np.float32))
    for v in HR.SPECIALS:
        assert (llr == v).any()
    for es in (HR.ES_OFF, HR.ES_FRAME):
        trace = []
        bits, iters = HR.decode(code, llr, 5, alpha, es, trace=trace)
        sb, si, sa = HR.decode_scalar(code, llr, 5, alpha, es)
        assert np.array_equal(bits, sb) and np.array_equal(iters, si)
        app = np.stack([trace[iters[b] - 1][0][b] for b in range(len(llr))])
        assert np.isfinite(app).all() and np.array_equal(app, sa)


def test_rounding_of_the_channel_values():
    x = HR.to_half(HR.SPECIALS)
    want = [0, 0, 1024, -1024, 1024, -1024, 0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -24, 2.0 ** -23, -2.0 ** -23,
            1, -1, 1 + 2.0 ** -9, -(1 + 2.0 ** -9)]
    assert x.dtype == np.float16 and x.tolist() == want
    assert np.isinf(HR.to_half(HR.SPECIALS, clamp=None)[2:6]).all()


def test_clamp_engages_and_bounds_everything(oracle_mod, z4):
    _, code, _ = z4
    llr = HR.saturating(oracle_mod.awgn_llr(8, code.N, 0.0, seed=7))
    free, held = [], []
    HR.decode(code, llr, 50, 0.75, trace=free, clamp=None)
    HR.decode(code, llr, 50, 0.75, trace=held)
    top_free = max(float(np.abs(t[1]).max()) for t in free)
    top_v2c = max(float(np.abs(t[1]).max()) for t in held)
    top_app = max(float(np.abs(t[0]).max()) for t in held)
    print(f"max |v2c| unclamped {top_free}, clamped {top_v2c}; max |app| clamped {top_app}")
    assert top_free > 1024
    assert top_v2c == 1024 and top_app <= 33792
    assert all(np.isfinite(a).all() for t in held for a in t[:3])


def test_constructor_refusals(z4):
    import torch

    from ldpc_neural_decoder import _native as N
    from ldpc_neural_decoder.models import MinSumScaledDecoder

    H4 = torch.from_numpy(np.asarray(z4[0], dtype=np.float32))
    with pytest.raises(ValueError, match=r'"frame".*False'):
        MinSumScaledDecoder(H4, precision="fp16", early_stopping=True)
    with pytest.raises(ValueError):
        MinSumScaledDecoder(H4, precision="bf16")
    assert MinSumScaledDecoder(H4, precision="fp16", early_stopping="frame")._algo == N.LDPC_ALGO_MINSUM_F16
    assert MinSumScaledDecoder(H4, precision="fp16", early_stopping=False)._algo == N.LDPC_ALGO_MINSUM_F16
    assert MinSumScaledDecoder(H4)._algo == MinSumScaledDecoder(H4, precision="fp32")._algo == N.LDPC_ALGO_MINSUM
