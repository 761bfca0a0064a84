"""HIP layered min-sum decoder (csrc/flood_layered.hip) against tests/layered_ref.py (GPU).

Bar: decisions and per-frame iteration counts equal the numpy float32 restatement EXACTLY, in every
stopping mode, for every lifting the kernel maps differently (Z = 32, 4, 1)."""
import numpy as np
import pytest
import torch

import layered_ref as LR
from conftest import code_path, golden

from ldpc_neural_decoder import _native as N
from ldpc_neural_decoder.models import LayeredMinSumDecoder, MinSumScaledDecoder
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
    return LR.Code(H4.numpy())


@pytest.fixture(scope="module")
def code32(H32):
    return LR.Code(H32.numpy())


def awgn(oracle_mod, B, n, snr):
    return oracle_mod.awgn_llr(B, n, snr, seed=7).astype(np.float32)


def run(H, llr, iters, alpha, es, cuda, out_dtype=torch.float32, variant=None, **kw):
    dec = LayeredMinSumDecoder(H, iters, alpha, early_stopping=es)
    if variant is not None:
        dec.graph(cuda).set_variant(variant)
    bits, it, fi = dec.decode(torch.from_numpy(llr).to(cuda), out_dtype=out_dtype, return_frame_iters=True, **kw)
    assert bits.dtype == out_dtype
    return bits.cpu().numpy().astype(np.uint8), it, fi.cpu().numpy()


@pytest.fixture(scope="module")
def ref32_off(oracle_mod, code32):
    """Z = 32, B = 37 (odd: a half-filled last wave), -3.5 dB: decisions after each of 10 iterations."""
    llr = awgn(oracle_mod, 37, code32.N, -3.5)
    trace = []
    LR.decode(code32, llr, 10, 0.75, trace=trace)
    return llr, [t[2] for t in trace]


@pytest.fixture(scope="module")
def ref32_frame(oracle_mod, code32):
    llr = awgn(oracle_mod, 96, code32.N, -3.0)
    bits, iters = LR.decode(code32, llr, 10, 0.75, LR.ES_FRAME)
    return llr, bits, iters


@pytest.mark.parametrize("alpha", [0.75, 0.8])
def test_z4_exact(cuda, oracle_mod, H4, code4, alpha):
    """Z = 4: 16 frames per wave, B = 50 leaves the last wave partial."""
    llr = awgn(oracle_mod, 50, code4.N, -2.0)
    trace = []
    LR.decode(code4, llr, 5, alpha, trace=trace)
    for iters in (1, 2, 5):
        bits, it, fi = run(H4, llr, iters, alpha, False, cuda)
        assert np.array_equal(bits, trace[iters - 1][2]), iters
        assert it == iters and (fi == iters).all()
    rb, ri = LR.decode(code4, llr, 10, alpha, LR.ES_FRAME)
    bits, it, fi = run(H4, llr, 10, alpha, "frame", cuda)
    never = int((~LR.syndrome_ok(code4, rb)).sum())
    print(f"alpha {alpha}: stops {np.unique(ri).tolist()}, never valid {never}")
    assert np.array_equal(fi, ri) and np.array_equal(bits, rb) and it == int(ri.max())
    b2, it2, fi2 = run(H4, llr, 10, alpha, True, cuda)  # True means the per-frame freeze too
    assert np.array_equal(b2, rb) and np.array_equal(fi2, ri) and it2 == it


@pytest.mark.parametrize("out_dtype", [torch.uint8, torch.float32])
def test_z32_es_off_exact(cuda, H32, ref32_off, out_dtype):
    llr, per_iter = ref32_off
    for iters in (1, 5, 10):
        bits, it, fi = run(H32, llr, iters, 0.75, False, cuda, out_dtype)
        assert np.array_equal(bits, per_iter[iters - 1]), iters
        assert it == iters and (fi == iters).all()


@pytest.mark.parametrize("out_dtype", [torch.uint8, torch.float32])
def test_z32_frame_stop_exact(cuda, H32, ref32_frame, out_dtype):
    llr, rb, ri = ref32_frame
    assert len(np.unique(ri)) >= 3
    bits, it, fi = run(H32, llr, 10, 0.75, "frame", cuda, out_dtype)
    assert np.array_equal(fi, ri)
    assert np.array_equal(bits, rb)
    assert it == int(ri.max())


@pytest.mark.parametrize("es", [False, "frame"])
def test_variants_bit_identical(cuda, H32, ref32_frame, es):
    """set_variant(0) (auto: a compile-time schedule where the graph has one) and set_variant(1)
    (table-driven) give the same decisions and d_iters."""
    llr = ref32_frame[0]
    b0, i0, f0 = run(H32, llr, 7, 0.75, es, cuda, variant=0)
    b1, i1, f1 = run(H32, llr, 7, 0.75, es, cuda, variant=1)
    assert np.array_equal(b0, b1) and i0 == i1 and np.array_equal(f0, f1)


def random_H(dense_row):
    rng = np.random.default_rng(2024)
    H = np.zeros((24, 50), dtype=np.float32)
    for j in range(48):
        H[rng.choice(24, size=3, replace=False), j] = 1
    H[5, 48] = 1   # two appended degree-1 columns
    H[20, 49] = 1
    if dense_row:  # check 11 gets degree >= 14: past the unrolled register code
        H[11, rng.choice(48, size=14, replace=False)] = 1
    return H


@pytest.mark.parametrize("dense_row", [False, True])
def test_non_qc_graph_z1(cuda, dense_row):
    """Z = 1: one frame per lane, every check its own layer; B = 130 = two full waves and two frames."""
    H = random_H(dense_row)
    code = LR.Code(H)
    assert code.deg1[48:].all() and (H.sum(1).max() > 12) == dense_row
    rng = np.random.default_rng(9)
    llr = rng.normal(0.8, 1.6, size=(130, 50)).astype(np.float32)
    Ht = torch.from_numpy(H)
    assert LayeredMinSumDecoder(Ht, 3).graph(cuda).Z == 1
    trace = []
    LR.decode(code, llr, 6, 0.75, trace=trace)
    for iters in (1, 6):
        bits, _, _ = run(Ht, llr, iters, 0.75, False, cuda)
        assert np.array_equal(bits, trace[iters - 1][2]), iters
    rb, ri = LR.decode(code, llr, 12, 0.75, LR.ES_FRAME)
    bits, it, fi = run(Ht, llr, 12, 0.75, True, cuda)
    assert len(np.unique(ri)) >= 2
    assert np.array_equal(fi, ri) and np.array_equal(bits, rb) and it == int(ri.max())


@pytest.mark.parametrize("es", [False, "frame"])
def test_fused_counters(cuda, H32, ref32_frame, es):
    llr = ref32_frame[0]
    cnt = torch.zeros(4, dtype=torch.int64, device=cuda)
    bits, it, fi = run(H32, llr, 10, 0.75, es, cuda, torch.uint8, counters=cnt)
    want = [int(bits.sum()), int(bits.any(1).sum()), len(llr), int(fi.sum())]
    assert cnt.tolist() == want
    if es:
        assert np.array_equal(bits, ref32_frame[1]) and it == int(fi.max())
    run(H32, llr[:37], 10, 0.75, es, cuda, torch.uint8, counters=cnt)
    b2, _, f2 = run(H32, llr[:37], 10, 0.75, es, cuda)
    want2 = [int(b2.sum()), int(b2.any(1).sum()), 37, int(f2.sum())]
    assert cnt.tolist() == [a + b for a, b in zip(want, want2)]


@pytest.mark.parametrize("es", [False, "frame"])
def test_frame_independence(cuda, H32, ref32_off, ref32_frame, es):
    """A frame's result does not depend on the batch it rides in nor on its place in it."""
    llr = ref32_off[0]
    full, _, fi = run(H32, llr, 5, 0.75, es, cuda)
    dec = LayeredMinSumDecoder(H32, 5, 0.75, early_stopping=es)
    x = torch.from_numpy(llr).to(cuda)
    for b in range(len(llr)):
        one, _, f1 = dec.decode(x[b:b + 1], return_frame_iters=True)
        assert np.array_equal(one.cpu().numpy().astype(np.uint8)[0], full[b]), b
        assert int(f1[0]) == fi[b]
    moved = np.concatenate([ref32_frame[0][:5], llr, ref32_frame[0][5:9]])  # frames 0..36 at 5..41
    big, _, fb = run(H32, moved, 5, 0.75, es, cuda)
    assert np.array_equal(big[5:42], full) and np.array_equal(fb[5:42], fi)


@pytest.mark.parametrize("es", [False, "frame"])
def test_non_finite_inputs(cuda, oracle_mod, H4, code4, es):
    """A NaN frame and a +-inf frame share a wave (Z = 4: 16 frames) with finite frames: the finite
    ones decode exactly as they do alone, the others come back as 0/1."""
    llr = awgn(oracle_mod, 16, code4.N, -2.0)
    llr[3, 11] = np.nan
    llr[7, 5] = np.inf
    llr[7, 100] = -np.inf
    finite = [b for b in range(16) if b not in (3, 7)]
    bits, _, fi = run(H4, llr, 6, 0.75, es, cuda, torch.uint8)
    alone, _, fa = run(H4, llr[finite], 6, 0.75, es, cuda, torch.uint8)
    rb, ri = LR.decode(code4, llr[finite], 6, 0.75, LR.ES_FRAME if es else LR.ES_OFF)
    assert np.array_equal(bits[finite], alone) and np.array_equal(fi[finite], fa)
    assert np.array_equal(alone, rb) and np.array_equal(fa, ri)
    assert set(np.unique(bits[[3, 7]]).tolist()) <= {0, 1}
    assert ((fi >= 1) & (fi <= 6)).all()


@pytest.mark.parametrize("es", [False, "frame"])
def test_z32_zeros_and_non_finite(cuda, oracle_mod, H32, code32, es):
    """Z = 32 (two frames per wave): zero LLRs (sgn 0 = 0) in frame 1 put its wave, frame 0
    included, on the kernels' general check update for the rows they reach and back on the short
    one afterwards; a NaN in frame 2 and infinities in frame 5 ride next to frames 3 and 4.  Finite
    frames equal the reference exactly on both variants."""
    llr = awgn(oracle_mod, 8, code32.N, -3.0)
    llr[1, :40] = 0.0
    llr[1, 700:720] = 0.0
    llr[2, 11] = np.nan
    llr[5, 5] = np.inf
    llr[5, 1000] = -np.inf
    finite = [0, 1, 3, 4, 6, 7]
    rb, ri = LR.decode(code32, llr[finite], 8, 0.75, LR.ES_FRAME if es else LR.ES_OFF)
    for variant in (0, 1):
        bits, _, fi = run(H32, llr, 8, 0.75, es, cuda, torch.uint8, variant=variant)
        assert np.array_equal(bits[finite], rb) and np.array_equal(fi[finite], ri), variant
        assert set(np.unique(bits[[2, 5]]).tolist()) <= {0, 1}


def raw_decode(g, llr, iters, es, cuda):
    bits = torch.empty(llr.shape, dtype=torch.uint8, device=cuda)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=cuda)
    return N.lib().ldpc_flood_decode(g.handle, N.LDPC_ALGO_LAYERED_MINSUM, N.ptr(llr), llr.shape[0], iters, 0.75, es,
                                     N.LDPC_OUT_U8, N.ptr(bits), None, None, None, N.ptr(ws), ws.numel(),
                                     N.stream_ptr(cuda))


def test_abi_errors(cuda, H4, monkeypatch):
    llr = torch.ones(4, 208, device=cuda)
    g = LayeredMinSumDecoder(H4, 3).graph(cuda)
    assert raw_decode(g, llr, 3, N.LDPC_ES_BATCH, cuda) == N.LDPC_EINVAL
    assert b"batch-global" in N.lib().ldpc_last_error()
    assert raw_decode(g, llr, 3, N.LDPC_ES_OFF, cuda) == 0
    with pytest.raises(UnboundLocalError):  # as the sibling classes (and the reference's loop)
        LayeredMinSumDecoder(H4, max_iterations=0).decode(llr)
    with pytest.raises(ValueError):
        LayeredMinSumDecoder(H4, 3).decode(llr[:, :207])
    # BG2 lifted at Z = 12 does not divide 64: the flooding algos decode it on the streaming kernels
    H12 = H_of(12, base_z=32)
    x12 = torch.ones(3, H12.shape[1], device=cuda)
    MinSumScaledDecoder(H12, 2, early_stopping=False).decode(x12)
    with pytest.raises(N.NativeError, match="LDS-resident"):
        LayeredMinSumDecoder(H12, 2, early_stopping=False).decode(x12)
    assert raw_decode(LayeredMinSumDecoder(H12, 2).graph(cuda), x12, 2, N.LDPC_ES_OFF, cuda) == N.LDPC_EUNSUPPORTED
    monkeypatch.setenv("LDPC_FLOOD_STREAM", "1")
    assert raw_decode(g, llr, 3, N.LDPC_ES_OFF, cuda) == N.LDPC_EUNSUPPORTED
    assert b"streaming" in N.lib().ldpc_last_error()


@pytest.mark.parametrize("es", [False, True])
def test_flooding_minsum_unchanged(cuda, H32, es):
    """The flooding decoder next door still reproduces the reference's golden decisions."""
    t = golden("trad_z32_low.npz")
    dec = MinSumScaledDecoder(H32, max_iterations=10, scaling_factor=0.75, early_stopping=es)
    for k in range(t["llrs"].shape[0]):
        bits, it = dec.decode(torch.from_numpy(t["llrs"][k]).to(cuda))
        assert np.array_equal(bits.cpu().numpy().astype(np.uint8), t[f"ms_a0.75_es{int(es)}_bits"][k]), k
        assert it == t[f"ms_a0.75_es{int(es)}_iters"][k]
