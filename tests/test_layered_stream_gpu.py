"""Streaming layered min-sum (csrc/flood_layered_stream.hip, LayeredMinSumDecoder(any_graph=True)) on the GPU.

Bar: tests/layered_ref.py's, as for the LDS-resident decoder: decisions and per-frame iteration counts
EQUAL the numpy float32 restatement, no tolerance.  The reference costs seconds per iteration above
Z = 12, so exactness against it is taken at Z = 12 (BG2 lifted from the Z = 32 base file: 12 does not
divide 64, so the graph decodes on the streaming kernels) plus two iterations at Z = 96 and a small
non-QC graph; Z = 32 and Z = 4 are held to the LDS-resident layered kernels, which test_layered_gpu
pins against the same reference.  Every reference is computed once per module."""
import numpy as np
import pytest
import torch

import layered_ref as LR
from conftest import code_path

from ldpc_neural_decoder import _native as N
from ldpc_neural_decoder.models import LayeredMinSumDecoder
from ldpc_neural_decoder.utils import awgn_llr, expand_base_matrix, load_base_matrix

pytestmark = pytest.mark.gpu


def H_of(z, base_z=32):
    return expand_base_matrix(load_base_matrix(code_path(base_z)), z)


@pytest.fixture(scope="module")
def H12():
    return H_of(12)


@pytest.fixture(scope="module")
def code12(H12):
    return LR.Code(H12.numpy())


def awgn(oracle_mod, B, n, snr):
    return oracle_mod.awgn_llr(B, n, snr, seed=7).astype(np.float32)


def run(H, llr, iters, alpha, es, cuda, out_dtype=torch.uint8, any_graph=True, **kw):
    dec = LayeredMinSumDecoder(H, iters, alpha, early_stopping=es, any_graph=any_graph)
    x = llr if torch.is_tensor(llr) else torch.from_numpy(llr)
    bits, it, fi = dec.decode(x.to(cuda), out_dtype=out_dtype, return_frame_iters=True, **kw)
    assert bits.dtype == out_dtype
    return bits.cpu().numpy().astype(np.uint8), it, fi.cpu().numpy()


# ------------------------------------------------------------------------------------ Z = 12
@pytest.fixture(scope="module")
def ref12_off(oracle_mod, code12):
    """B = 300 at -2 dB: decisions after each of 6 iterations, for both scaling factors.  A frame's
    LLRs depend on (seed, frame index) alone and the reference never mixes frames, so the first 70
    rows are the B = 70 case."""
    llr = awgn(oracle_mod, 300, code12.N, -2.0)
    per_alpha = {}
    for alpha in (0.75, 0.8):
        trace = []
        LR.decode(code12, llr, 6, alpha, trace=trace)
        per_alpha[alpha] = [t[2] for t in trace]
    return llr, per_alpha


@pytest.fixture(scope="module")
def ref12_frame(oracle_mod, code12):
    llr = awgn(oracle_mod, 300, code12.N, -3.0)
    bits, iters = LR.decode(code12, llr, 8, 0.75, LR.ES_FRAME)
    return llr, bits, iters


@pytest.mark.parametrize("out_dtype", [torch.uint8, torch.float32])
@pytest.mark.parametrize("alpha", [0.75, 0.8])
@pytest.mark.parametrize("B", [70, 300])  # one full wave and a partial one; past a 256-thread block
def test_z12_es_off_exact(cuda, H12, ref12_off, B, alpha, out_dtype):
    llr, per_alpha = ref12_off
    assert LayeredMinSumDecoder(H12, 1).graph(cuda).Z == 1  # no lifting that divides 64: streaming
    for iters in (1, 2, 6):
        bits, it, fi = run(H12, llr[:B], iters, alpha, False, cuda, out_dtype)
        assert np.array_equal(bits, per_alpha[alpha][iters - 1][:B]), iters
        assert it == iters and (fi == iters).all()


@pytest.mark.parametrize("out_dtype", [torch.uint8, torch.float32])
def test_z12_frame_stop_exact(cuda, code12, H12, ref12_frame, out_dtype):
    llr, rb, ri = ref12_frame
    never = int((~LR.syndrome_ok(code12, rb)).sum())
    print(f"stops {np.unique(ri).tolist()}, never valid {never}")
    assert len(np.unique(ri)) >= 3 and never >= 1
    for es in ("frame", True):  # True means the per-frame freeze too
        bits, it, fi = run(H12, llr, 8, 0.75, es, cuda, out_dtype)
        assert np.array_equal(fi, ri)
        assert np.array_equal(bits, rb)
        assert it == int(ri.max()) == 8


def test_z96_two_iterations(cuda, oracle_mod):
    H = H_of(96)
    code = LR.Code(H.numpy())
    llr = awgn(oracle_mod, 70, code.N, -3.0)
    trace = []
    LR.decode(code, llr, 2, 0.75, trace=trace)
    bits, it, fi = run(H, llr, 2, 0.75, False, cuda)
    assert np.array_equal(bits, trace[1][2])
    assert it == 2 and (fi == 2).all()


# ------------------------------------------------------------------------------------ non-QC
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
def test_non_qc_graph_forced_streaming(cuda, monkeypatch, dense_row):
    """A small graph has an LDS-resident schedule; LDPC_FLOOD_STREAM=1 puts it on the streaming
    kernels.  Every check is its own layer or shares one with few others: many short launches."""
    monkeypatch.setenv("LDPC_FLOOD_STREAM", "1")
    H = random_H(dense_row)
    code = LR.Code(H)
    dmax = int(H.sum(1).max())
    # the dense row (degree 16) is past the 12 that mark the LDS path's unrolled code, under the streaming 32
    assert code.deg1[48:].all() and (12 < dmax <= 32) == dense_row
    rng = np.random.default_rng(9)
    llr = rng.normal(0.8, 1.6, size=(130, 50)).astype(np.float32)
    Ht = torch.from_numpy(H)
    trace = []
    LR.decode(code, llr, 6, 0.75, trace=trace)
    for iters in (1, 6):
        bits, _, _ = run(Ht, llr, iters, 0.75, False, cuda)
        assert np.array_equal(bits, trace[iters - 1][2]), iters
    rb, ri = LR.decode(code, llr, 12, 0.75, LR.ES_FRAME)
    bits, it, fi = run(Ht, llr, 12, 0.75, "frame", cuda)
    assert len(np.unique(ri)) >= 2
    assert np.array_equal(fi, ri) and np.array_equal(bits, rb) and it == int(ri.max())
    with pytest.raises(N.NativeError, match="LDS-resident"):  # the default class still refuses here
        run(Ht, llr, 2, 0.75, False, cuda, any_graph=False)


def test_degree_above_32(cuda, monkeypatch):
    H = np.zeros((3, 40), dtype=np.float32)
    H[0, :33] = 1
    H[1, 30:36] = 1
    H[2, 34:40] = 1
    llr = np.ones((5, 40), dtype=np.float32)
    monkeypatch.setenv("LDPC_FLOOD_STREAM", "1")
    with pytest.raises(N.NativeError, match="degree above 32") as e:
        run(torch.from_numpy(H), llr, 2, 0.75, False, cuda)
    assert f"error {N.LDPC_EUNSUPPORTED}:" in str(e.value)


# ------------------------------------------------------------------- both paths, one answer
@pytest.mark.parametrize("es", [False, "frame"])
@pytest.mark.parametrize("z,B,snr", [(32, 37, -3.0), (32, 96, -3.0), (4, 50, -2.0)])
def test_same_answer_on_both_paths(cuda, oracle_mod, monkeypatch, z, B, snr, es):
    """The streaming kernels against the LDS-resident ones (pinned by test_layered_gpu): algo 2, algo 3
    where algo 2 runs, and algo 3 forced onto the streaming kernels give the same bits, per-frame
    counts and `iterations`."""
    H = H_of(z, base_z=z)
    llr = awgn(oracle_mod, B, H.shape[1], snr)
    b2, i2, f2 = run(H, llr, 7, 0.75, es, cuda, any_graph=False)
    b3, i3, f3 = run(H, llr, 7, 0.75, es, cuda)
    assert np.array_equal(b3, b2) and i3 == i2 and np.array_equal(f3, f2)
    monkeypatch.setenv("LDPC_FLOOD_STREAM", "1")
    bs, is_, fs = run(H, llr, 7, 0.75, es, cuda)
    assert np.array_equal(bs, b2) and is_ == i2 and np.array_equal(fs, f2)
    if es:
        assert len(np.unique(f2)) >= 2


# ------------------------------------------------------------------- zeros and non-finite LLRs
@pytest.mark.parametrize("es", [False, "frame"])
def test_z12_zeros(cuda, oracle_mod, H12, code12, es):
    """Zero LLRs (sgn 0 = 0) put frame 1 on the MinSumStats branch of the check rule for the rows they
    reach; every frame is finite and equals the reference exactly."""
    llr = awgn(oracle_mod, 8, code12.N, -3.0)
    llr[1, :40] = 0.0
    llr[1, 300:320] = 0.0
    rb, ri = LR.decode(code12, llr, 8, 0.75, LR.ES_FRAME if es else LR.ES_OFF)
    bits, _, fi = run(H12, llr, 8, 0.75, es, cuda)
    assert np.array_equal(bits, rb) and np.array_equal(fi, ri)


@pytest.mark.parametrize("es", [False, "frame"])
def test_z12_non_finite(cuda, oracle_mod, H12, code12, es):
    """A NaN frame and a +-inf frame ride in one wave with finite frames: those decode exactly as they
    do alone, the others come back as 0/1 with a count in [1, max]."""
    llr = awgn(oracle_mod, 16, code12.N, -2.0)
    llr[3, 11] = np.nan
    llr[7, 5] = np.inf
    llr[7, 100] = -np.inf
    finite = [b for b in range(16) if b not in (3, 7)]
    bits, _, fi = run(H12, llr, 6, 0.75, es, cuda)
    alone, _, fa = run(H12, llr[finite], 6, 0.75, es, cuda)
    assert np.array_equal(bits[finite], alone) and np.array_equal(fi[finite], fa)
    assert set(np.unique(bits[[3, 7]]).tolist()) <= {0, 1}
    assert ((fi >= 1) & (fi <= 6)).all()


# ------------------------------------------------------------------- counters, independence
@pytest.mark.parametrize("es", [False, "frame"])
def test_fused_counters(cuda, H12, ref12_frame, es):
    llr, rb, _ = ref12_frame
    cnt = torch.zeros(4, dtype=torch.int64, device=cuda)
    bits, it, fi = run(H12, llr, 8, 0.75, es, cuda, counters=cnt)
    want = [int(bits.sum()), int(bits.any(1).sum()), len(llr), int(fi.sum())]
    assert cnt.tolist() == want
    if es:
        assert np.array_equal(bits, rb) and it == int(fi.max())
    run(H12, llr[:37], 8, 0.75, es, cuda, counters=cnt)
    b2, _, f2 = run(H12, llr[:37], 8, 0.75, es, cuda)
    want2 = [int(b2.sum()), int(b2.any(1).sum()), 37, int(f2.sum())]
    assert cnt.tolist() == [a + b for a, b in zip(want, want2)]


@pytest.mark.parametrize("es", [False, "frame"])
def test_frame_independence(cuda, H12, ref12_frame, es):
    """A frame's result does not depend on the batch it rides in nor on its place in it."""
    llr = ref12_frame[0][:70]
    full, _, fi = run(H12, llr, 5, 0.75, es, cuda)
    dec = LayeredMinSumDecoder(H12, 5, 0.75, early_stopping=es, any_graph=True)
    x = torch.from_numpy(llr).to(cuda)
    for b in range(len(llr)):
        one, _, f1 = dec.decode(x[b:b + 1], out_dtype=torch.uint8, return_frame_iters=True)
        assert np.array_equal(one.cpu().numpy()[0], full[b]), b
        assert int(f1[0]) == fi[b]
    moved = np.concatenate([ref12_frame[0][100:105], llr[::-1], ref12_frame[0][200:264]])  # reversed, at 5..74
    big, _, fb = run(H12, moved, 5, 0.75, es, cuda)
    assert np.array_equal(big[5:75][::-1], full) and np.array_equal(fb[5:75][::-1], fi)


# ------------------------------------------------------------------- offsets past 2^31
def test_large_offsets(cuda):
    """Z = 96, B = 120 000: E * B = 2.27e9 message elements, so (edge, frame) offsets pass 2^31."""
    free, _ = torch.cuda.mem_get_info(cuda)
    if free < 20 * 2**30:
        pytest.skip(f"needs about 12 GB of device memory next to its inputs; {free / 2**30:.1f} GB free")
    H = H_of(96)
    B, E = 120_000, int(H.sum())
    assert E * B > 2**31 and 113_551 * E < 2**31 < 113_552 * E
    llr = awgn_llr(B, H.shape[1], -3.0, seed=7, device=cuda)
    dec = LayeredMinSumDecoder(H, 2, 0.75, early_stopping=False, any_graph=True)
    bits, _ = dec.decode(llr, out_dtype=torch.uint8)
    frames = [0, 63, 64] + list(range(113_550, 113_561)) + [B - 65, B - 1]
    idx = torch.tensor(frames, device=cuda)
    small, _ = dec.decode(llr[idx].contiguous(), out_dtype=torch.uint8)
    assert torch.equal(bits[idx], small)
    assert 0 < int(small.sum()) < small.numel()


# ------------------------------------------------------------------- errors
def raw_decode(g, llr, iters, es, cuda, algo=N.LDPC_ALGO_LAYERED_MINSUM_ANY, ws_bytes=None):
    bits = torch.empty(llr.shape, dtype=torch.uint8, device=cuda)
    need = N.check(N.lib().ldpc_flood_workspace_size(g.handle, llr.shape[0], iters, es))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=cuda)
    return N.lib().ldpc_flood_decode(g.handle, algo, N.ptr(llr), llr.shape[0], iters, 0.75, es, N.LDPC_OUT_U8,
                                     N.ptr(bits), None, None, None, N.ptr(ws), need if ws_bytes is None else ws_bytes(need),
                                     N.stream_ptr(cuda))


def test_abi_errors(cuda, H12):
    x12 = torch.ones(3, H12.shape[1], device=cuda)
    g = LayeredMinSumDecoder(H12, 2, any_graph=True).graph(cuda)
    assert raw_decode(g, x12, 2, N.LDPC_ES_BATCH, cuda) == N.LDPC_EINVAL
    assert b"batch-global" in N.lib().ldpc_last_error()
    assert raw_decode(g, x12, 2, N.LDPC_ES_OFF, cuda) == 0
    assert raw_decode(g, x12, 2, N.LDPC_ES_OFF, cuda, ws_bytes=lambda need: need - 1) == N.LDPC_EINVAL  # one byte short
    assert b"workspace too small" in N.lib().ldpc_last_error()
    assert raw_decode(g, x12, 2, N.LDPC_ES_OFF, cuda, algo=4) == N.LDPC_EINVAL
    assert b"unknown algo" in N.lib().ldpc_last_error()
    with pytest.raises(ValueError):
        LayeredMinSumDecoder(H12, 3, any_graph=True).decode(x12[:, :-1])
    with pytest.raises(N.NativeError, match="LDS-resident"):  # without any_graph: as before
        LayeredMinSumDecoder(H12, 2, early_stopping=False).decode(x12)
    assert raw_decode(g, x12, 2, N.LDPC_ES_OFF, cuda, algo=N.LDPC_ALGO_LAYERED_MINSUM) == N.LDPC_EUNSUPPORTED
