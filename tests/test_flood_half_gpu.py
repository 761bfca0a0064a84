"""HIP half-precision min-sum (csrc/flood_half.hip, MinSumScaledDecoder(precision="fp16")) against
tests/half_ref.py (GPU).

Bar: decisions and per-frame iteration counts equal the numpy float16 restatement EXACTLY, in both stopping
modes, for every lifting the kernel maps differently (Z = 32: 4 frames per workgroup, Z = 4: 32, Z = 1: 128),
with last workgroups that have no high halves, a few, or all of them."""
import ctypes

import numpy as np
import pytest
import torch

import half_ref as HR
from conftest import code_path, golden

from ldpc_neural_decoder import _native as N
from ldpc_neural_decoder.models import MinSumScaledDecoder
from ldpc_neural_decoder.utils import expand_base_matrix, load_base_matrix

pytestmark = pytest.mark.gpu


def H_of(z, base_z=None):
    return expand_base_matrix(load_base_matrix(code_path(base_z or z)), z)


@pytest.fixture(scope="module")
def H4():
    return H_of(4)


@pytest.fixture(scope="module")
def H32():
    return H_of(32)


@pytest.fixture(scope="module")
def code4(H4):
    return HR.Code(H4.numpy())


@pytest.fixture(scope="module")
def code32(H32):
    return HR.Code(H32.numpy())


def awgn(oracle_mod, B, n, snr):
    return oracle_mod.awgn_llr(B, n, snr, seed=7).astype(np.float32)


def mixed(oracle_mod, B, n, snrs):
    """Frame b at snrs[b % len(snrs)]: early, late and never-converging frames side by side."""
    return np.concatenate([oracle_mod.awgn_llr(1, n, snrs[b % len(snrs)], seed=7, frame_offset=b)
                           for b in range(B)]).astype(np.float32)


def run(H, llr, iters, alpha, es, cuda, out_dtype=torch.float32, **kw):
    dec = MinSumScaledDecoder(H, iters, alpha, early_stopping=es, precision="fp16")
    bits, it, fi = dec.decode(torch.from_numpy(llr).to(cuda), out_dtype=out_dtype, return_frame_iters=True, **kw)
    assert bits.dtype == out_dtype
    return bits.cpu().numpy().astype(np.uint8), it, fi.cpu().numpy()


def per_iteration(code, llr, iters, alpha):
    trace = []
    HR.decode(code, llr, iters, alpha, trace=trace)
    return [t[3] for t in trace]


@pytest.mark.parametrize("alpha", [0.75, 0.8])
@pytest.mark.parametrize("B", [45, 50])
def test_z4_exact(cuda, oracle_mod, H4, code4, B, alpha):
    """Z = 4: 32 frames per workgroup.  B = 45: the last workgroup has 13 low frames and no high half;
    B = 50: 16 low and 2 high."""
    llr = awgn(oracle_mod, B, code4.N, -2.0)
    want = per_iteration(code4, llr, 5, alpha)
    for iters in (1, 2, 5):
        bits, it, fi = run(H4, llr, iters, alpha, False, cuda)
        assert np.array_equal(bits, want[iters - 1]), iters
        assert it == iters and (fi == iters).all()


def test_z32_exact(cuda, oracle_mod, H32, code32):
    """Z = 32: 4 frames per workgroup; B = 7 leaves the second one a single high frame."""
    llr = awgn(oracle_mod, 7, code32.N, -3.5)
    want = per_iteration(code32, llr, 10, 0.75)
    for iters in (1, 10):
        bits, it, fi = run(H32, llr, iters, 0.75, False, cuda)
        assert np.array_equal(bits, want[iters - 1]), iters
        assert it == iters and (fi == iters).all()


def regular_H(seed=3, n=96, dv=3, dc=6):
    """A seeded random (3, 6)-regular H: sockets of the variables matched to sockets of the checks, drawn
    again until no edge is double."""
    rng = np.random.default_rng(seed)
    m = n * dv // dc
    while True:
        chk = rng.permutation(np.repeat(np.arange(m), dc))
        H = np.zeros((m, n), dtype=np.float32)
        np.add.at(H, (chk, np.repeat(np.arange(n), dv)), 1)
        if H.max() == 1:
            return H


def irregular_H():
    """40 x 60 with a check of degree 14 and a variable of degree 26 (past the unrolled register code of both
    phases: 12 / 24) and two degree-1 variables."""
    rng = np.random.default_rng(2025)
    H = np.zeros((40, 60), dtype=np.float32)
    for j in range(58):
        H[rng.choice(40, size=3, replace=False), j] = 1
    H[7, 58] = 1
    H[31, 59] = 1
    H[11, rng.choice(58, size=14, replace=False)] = 1
    H[rng.choice(40, size=26, replace=False), 5] = 1
    return H


@pytest.mark.parametrize("kind", ["regular", "irregular"])
def test_non_qc_graph_z1(cuda, kind):
    """Z = 1: one frame pair per lane, 128 frames per workgroup; B = 130 puts two low frames in the second."""
    H = regular_H() if kind == "regular" else irregular_H()
    code = HR.Code(H)
    if kind == "regular":
        assert H.shape == (48, 96) and (H.sum(0) == 3).all() and (H.sum(1) == 6).all()
    else:
        assert H.sum(1).max() > 12 and 24 < H.sum(0).max() <= 32 and (H.sum(0) == 1).sum() == 2
    rng = np.random.default_rng(9)
    llr = rng.normal(2.0, 1.6, size=(130, code.N)).astype(np.float32)
    Ht = torch.from_numpy(H)
    assert MinSumScaledDecoder(Ht, 3, precision="fp16", early_stopping=False).graph(cuda).Z == 1
    want = per_iteration(code, llr, 5, 0.75)
    for iters in (1, 5):
        bits, _, _ = run(Ht, llr, iters, 0.75, False, cuda)
        assert np.array_equal(bits, want[iters - 1]), iters
    rb, ri = HR.decode(code, llr, 12, 0.75, HR.ES_FRAME)
    bits, it, fi = run(Ht, llr, 12, 0.75, "frame", cuda)
    assert len(np.unique(ri)) >= 2
    assert np.array_equal(fi, ri) and np.array_equal(bits, rb) and it == int(ri.max())


@pytest.fixture(scope="module")
def frame_refs(oracle_mod, code4, code32):
    out = {}
    for z, code, B, snrs in ((4, code4, 50, [-4, -1, 0, 1, 2, 4, 6]), (32, code32, 7, [-4.5, -3, -2, -1, 0, 2, 6])):
        llr = mixed(oracle_mod, B, code.N, snrs)
        bits, iters = HR.decode(code, llr, 10, 0.75, HR.ES_FRAME)
        out[z] = (llr, bits, iters, HR.syndrome_ok(code, bits))
    return out


@pytest.mark.parametrize("out_dtype", [torch.uint8, torch.float32])
@pytest.mark.parametrize("z", [4, 32])
def test_frame_stop_exact(cuda, H4, H32, frame_refs, z, out_dtype):
    """LDPC_ES_FRAME: bits, iteration counts, `iterations` and the four counters equal numpy's; a second
    decode adds to the same counters."""
    llr, rb, ri, ok = frame_refs[z]
    assert len(np.unique(ri)) >= 3
    assert ((ri == 10) & ~ok).any()  # a frame that ends at max_iter with an invalid syndrome
    H = H4 if z == 4 else H32
    cnt = torch.zeros(4, dtype=torch.int64, device=cuda)
    want = np.array([int(rb.sum()), int(rb.any(1).sum()), len(llr), int(ri.sum())])
    for rounds in (1, 2):
        bits, it, fi = run(H, llr, 10, 0.75, "frame", cuda, out_dtype, counters=cnt)
        assert np.array_equal(bits, rb) and np.array_equal(fi, ri)
        assert it == int(ri.max())
        assert cnt.tolist() == (rounds * want).tolist()


def test_counters_without_stop(cuda, oracle_mod, H4, code4):
    llr = awgn(oracle_mod, 50, code4.N, -2.0)
    rb = per_iteration(code4, llr, 3, 0.75)[-1]
    cnt = torch.zeros(4, dtype=torch.int64, device=cuda)
    bits, it, fi = run(H4, llr, 3, 0.75, False, cuda, torch.uint8, counters=cnt)
    assert np.array_equal(bits, rb) and it == 3
    assert cnt.tolist() == [int(rb.sum()), int(rb.any(1).sum()), 50, 150]


def test_clamp(cuda, oracle_mod, H4, code4):
    """Beliefs that run into the clamp (the host test shows they pass 1024 without it): decisions along the
    way and at the end, and the per-frame stop, against the clamped reference."""
    llr = HR.saturating(awgn(oracle_mod, 8, code4.N, 0.0))
    want = per_iteration(code4, llr, 50, 0.75)
    for iters in (1, 3, 50):
        bits, _, _ = run(H4, llr, iters, 0.75, False, cuda)
        assert np.array_equal(bits, want[iters - 1]), iters
    rb, ri = HR.decode(code4, llr, 50, 0.75, HR.ES_FRAME)
    bits, it, fi = run(H4, llr, 50, 0.75, "frame", cuda)
    assert np.array_equal(bits, rb) and np.array_equal(fi, ri) and it == int(ri.max())


def test_rounding_and_specials(cuda, oracle_mod, H4, code4):
    """+-0, +-inf, values that round to infinity, to a subnormal, to zero, and rounding ties, in every frame."""
    llr = HR.with_specials(awgn(oracle_mod, 33, code4.N, 0.0))
    want = per_iteration(code4, llr, 5, 0.75)
    for iters in (1, 5):
        bits, _, _ = run(H4, llr, iters, 0.75, False, cuda)
        assert np.array_equal(bits, want[iters - 1]), iters
    rb, ri = HR.decode(code4, llr, 10, 0.75, HR.ES_FRAME)
    bits, it, fi = run(H4, llr, 10, 0.75, "frame", cuda)
    assert np.array_equal(bits, rb) and np.array_equal(fi, ri) and it == int(ri.max())


@pytest.mark.parametrize("es", [False, "frame"])
@pytest.mark.parametrize("victim", [3, 19])
def test_nan_isolation(cuda, oracle_mod, H4, code4, es, victim):
    """One NaN in frame 3 (a low half; its lanes' high half is frame 19) or in frame 19 (the reverse): every
    other frame, the partner included, decodes as the reference does."""
    clean = mixed(oracle_mod, 40, code4.N, [-2, 0, 2])
    rb, ri = HR.decode(code4, clean, 6, 0.75, HR.ES_FRAME if es else HR.ES_OFF)
    llr = clean.copy()
    llr[victim, 17] = np.nan
    bits, _, fi = run(H4, llr, 6, 0.75, es, cuda, torch.uint8)
    others = [b for b in range(40) if b != victim]
    assert np.array_equal(bits[others], rb[others]) and np.array_equal(fi[others], ri[others])
    assert set(np.unique(bits[victim]).tolist()) <= {0, 1}
    assert 1 <= fi[victim] <= 6


def raw_decode(g, llr, iters, alpha, es, cuda):
    bits = torch.empty(llr.shape, dtype=torch.uint8, device=cuda)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=cuda)
    rc = N.lib().ldpc_flood_decode(g.handle, N.LDPC_ALGO_MINSUM_F16, N.ptr(llr), llr.shape[0], iters, alpha, es,
                                   N.LDPC_OUT_U8, N.ptr(bits), None, None, None, N.ptr(ws), ws.numel(),
                                   N.stream_ptr(cuda))
    return rc, ws


def test_refusals(cuda, H4, monkeypatch):
    llr = torch.ones(4, 208, device=cuda)
    g = MinSumScaledDecoder(H4, 3, precision="fp16", early_stopping=False).graph(cuda)
    assert raw_decode(g, llr, 3, 0.75, N.LDPC_ES_BATCH, cuda)[0] == N.LDPC_EINVAL
    assert b"batch-global" in N.lib().ldpc_last_error()
    assert raw_decode(g, llr, 3, 1.5, N.LDPC_ES_OFF, cuda)[0] == N.LDPC_EINVAL
    assert raw_decode(g, llr, 3, -0.25, N.LDPC_ES_OFF, cuda)[0] == N.LDPC_EINVAL
    assert raw_decode(g, llr, 3, float("nan"), N.LDPC_ES_OFF, cuda)[0] == N.LDPC_EINVAL
    rc, ws = raw_decode(g, llr, 3, 1.0, N.LDPC_ES_OFF, cuda)
    assert rc == 0
    n = ctypes.c_int32(-1)
    assert N.lib().ldpc_flood_redo_count(g.handle, N.LDPC_ALGO_MINSUM_F16, 4, 3, N.LDPC_ES_OFF, N.ptr(ws), None,
                                         ctypes.byref(n), None) == N.LDPC_EUNSUPPORTED
    # BG2 lifted at Z = 12 does not divide 64: the flooding algorithms decode it on the streaming kernels
    H12 = H_of(12, base_z=32)
    x12 = torch.ones(3, H12.shape[1], device=cuda)
    g12 = MinSumScaledDecoder(H12, 2, precision="fp16", early_stopping=False).graph(cuda)
    assert raw_decode(g12, x12, 2, 0.75, N.LDPC_ES_OFF, cuda)[0] == N.LDPC_EUNSUPPORTED
    with pytest.raises(N.NativeError, match="LDS-resident"):
        MinSumScaledDecoder(H12, 2, precision="fp16", early_stopping=False).decode(x12)
    # a variable of degree 33
    H33 = np.zeros((34, 40), dtype=np.float32)
    H33[:33, 0] = 1
    H33[np.arange(34), np.arange(1, 35)] = 1
    H33[np.arange(34), (np.arange(34) + 3) % 39 + 1] = 1
    x33 = torch.ones(2, 40, device=cuda)
    g33 = MinSumScaledDecoder(torch.from_numpy(H33), 2, precision="fp16", early_stopping=False).graph(cuda)
    assert raw_decode(g33, x33, 2, 0.75, N.LDPC_ES_OFF, cuda)[0] == N.LDPC_EUNSUPPORTED
    assert b"degree" in N.lib().ldpc_last_error()
    monkeypatch.setenv("LDPC_FLOOD_STREAM", "1")
    assert raw_decode(g, llr, 3, 0.75, N.LDPC_ES_OFF, cuda)[0] == N.LDPC_EUNSUPPORTED
    assert b"streaming" in N.lib().ldpc_last_error()


def test_set_variant_has_no_effect(cuda, oracle_mod, H4, code4):
    llr = awgn(oracle_mod, 50, code4.N, -2.0)
    dec = MinSumScaledDecoder(H4, 4, 0.75, early_stopping=False, precision="fp16")
    x = torch.from_numpy(llr).to(cuda)
    out = []
    for variant in (0, 1):
        dec.graph(cuda).set_variant(variant)
        out.append(dec.decode(x, out_dtype=torch.uint8)[0].cpu().numpy())
    assert np.array_equal(out[0], out[1])


def test_fp32_untouched(cuda, oracle_mod, H4):
    """precision="fp32" is the default object: same decisions as before on the golden Z = 4 LLRs."""
    llrs = golden("channel_z4.npz")["llrs"]
    g = oracle_mod.Graph(H4.numpy())
    a = MinSumScaledDecoder(H4, 5, 0.75, False)
    b = MinSumScaledDecoder(H4, 5, 0.75, False, precision="fp32")
    assert a._algo == b._algo == N.LDPC_ALGO_MINSUM
    for k in range(llrs.shape[0]):
        x = torch.from_numpy(llrs[k]).to(cuda)
        ba, ia = a.decode(x)
        bb, ib = b.decode(x)
        assert torch.equal(ba, bb) and ia == ib == 5
        ref = oracle_mod.flood_decode(g, llrs[k], "minsum", 5, 0.75, 0)[0]
        assert np.array_equal(ba.cpu().numpy().astype(np.uint8), ref), k
