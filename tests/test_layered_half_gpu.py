"""Half-precision layered min-sum (csrc/flood_layered_stream_half.hip, LayeredMinSumDecoder(precision="fp16"))
on the GPU.

Bar: decisions and per-frame iteration counts EQUAL tests/layered_half_ref.py, the numpy float16 restatement
of the contract in include/ldpc_amd.h, no tolerance.  The kernels pack frames 2p and 2p + 1 into one lane, so
the batch sizes are chosen by where a frame falls: a lone low half, one pair, a wave (128 frames) plus one,
past a 256-thread block (512 frames) with an odd tail.  Every reference is computed once per module and
sliced."""
import ctypes

import numpy as np
import pytest
import torch

import layered_half_ref as LHR
import layered_ref as LR
from conftest import code_path

from ldpc_neural_decoder import _native as N
from ldpc_neural_decoder.models import LayeredMinSumDecoder
from ldpc_neural_decoder.utils import awgn_llr, expand_base_matrix, load_base_matrix

pytestmark = pytest.mark.gpu

ALGO = 6


def H_of(z, base_z=32):
    return expand_base_matrix(load_base_matrix(code_path(base_z)), z)


@pytest.fixture(scope="module")
def H12():
    return H_of(12)


@pytest.fixture(scope="module")
def code12(H12):
    return LHR.Code(H12.numpy())


def awgn(oracle_mod, B, n, snr):
    return oracle_mod.awgn_llr(B, n, snr, seed=7).astype(np.float32)


def run(H, llr, iters, alpha, es, cuda, out_dtype=torch.uint8, precision="fp16", **kw):
    ctor = {k: kw.pop(k) for k in ("any_graph",) if k in kw}
    dec = LayeredMinSumDecoder(H, iters, alpha, early_stopping=es, precision=precision, **ctor)
    assert dec._algo == ALGO or precision != "fp16"
    x = llr if torch.is_tensor(llr) else torch.from_numpy(llr)
    bits, it, fi = dec.decode(x.to(cuda), out_dtype=out_dtype, return_frame_iters=True, **kw)
    assert bits.dtype == out_dtype
    return bits.cpu().numpy().astype(np.uint8), it, fi.cpu().numpy()


def ref_both(code, llr, iters, alpha=0.75):
    """One reference run for both stop modes: (frozen bits, stop counts, decisions after each iteration)."""
    trace = []
    bits, it = LHR.decode(code, llr, iters, alpha, LHR.ES_FRAME, trace=trace)
    return bits, it, [t[2] for t in trace]


# ------------------------------------------------------------------------------------ Z = 12
@pytest.fixture(scope="module")
def ref12_off(oracle_mod, code12):
    """B = 600 at -2 dB: decisions after each of 6 iterations, for both scaling factors.  A frame's LLRs depend
    on (seed, frame index) alone and the reference never mixes frames, so the first B rows are the B case."""
    llr = awgn(oracle_mod, 600, code12.N, -2.0)
    per_alpha = {}
    for alpha in (0.75, 0.8):
        trace = []
        LHR.decode(code12, llr, 6, alpha, trace=trace)
        per_alpha[alpha] = [t[2] for t in trace]
    return llr, per_alpha


@pytest.fixture(scope="module")
def ref12_frame(oracle_mod, code12):
    llr = awgn(oracle_mod, 300, code12.N, -3.0)
    bits, iters = LHR.decode(code12, llr, 8, 0.75, LHR.ES_FRAME)
    return llr, bits, iters


@pytest.mark.parametrize("out_dtype", [torch.uint8, torch.float32])
@pytest.mark.parametrize("alpha", [0.75, 0.8])
@pytest.mark.parametrize("B", [1, 2, 129, 300, 515])
def test_z12_es_off_exact(cuda, H12, ref12_off, B, alpha, out_dtype):
    llr, per_alpha = ref12_off
    for iters in (1, 2, 6):
        bits, it, fi = run(H12, llr[:B], iters, alpha, False, cuda, out_dtype)
        assert np.array_equal(bits, per_alpha[alpha][iters - 1][:B]), iters
        assert it == iters and (fi == iters).all()


@pytest.mark.parametrize("out_dtype", [torch.uint8, torch.float32])
def test_z12_frame_stop_exact(cuda, code12, H12, ref12_frame, out_dtype):
    llr, rb, ri = ref12_frame
    never = int((~LHR.syndrome_ok(code12, rb)).sum())
    apart = int((ri[0::2] != ri[1::2]).sum())
    print(f"stops {np.unique(ri).tolist()}, never valid {never}, pairs that stop apart {apart}")
    assert len(np.unique(ri)) >= 3 and never >= 1 and apart >= 1
    for es in ("frame", True):  # True means the per-frame freeze too
        bits, it, fi = run(H12, llr, 8, 0.75, es, cuda, out_dtype)
        assert np.array_equal(fi, ri)
        assert np.array_equal(bits, rb)
        assert it == int(ri.max()) == 8


def test_z96_two_iterations(cuda, oracle_mod):
    H = H_of(96)
    code = LHR.Code(H.numpy())
    llr = awgn(oracle_mod, 70, code.N, -3.0)
    trace = []
    LHR.decode(code, llr, 2, 0.75, trace=trace)
    bits, it, fi = run(H, llr, 2, 0.75, False, cuda)
    assert np.array_equal(bits, trace[1][2])
    assert it == 2 and (fi == 2).all()


# ------------------------------------------------------------------- graphs with an LDS-resident schedule
@pytest.fixture(scope="module")
def refs_lds(oracle_mod):
    out = {}
    for z, B, snr in ((32, 96, -3.0), (4, 50, -2.0)):
        H = H_of(z, base_z=z)
        llr = awgn(oracle_mod, B, H.shape[1], snr)
        out[z] = (H, llr) + ref_both(LHR.Code(H.numpy()), llr, 7)
    return out


@pytest.mark.parametrize("es", [False, "frame"])
@pytest.mark.parametrize("z,B", [(32, 37), (32, 96), (4, 50)])
def test_lds_resident_graphs_stream_too(cuda, monkeypatch, refs_lds, z, B, es):
    """Z = 32 and Z = 4 have an LDS-resident schedule; algo 6 runs its streaming kernels all the same, and
    neither LDPC_FLOOD_STREAM, the kernel variant nor any_graph changes a bit."""
    H, llr, rb, ri, per_it = refs_lds[z]
    want_b, want_i = (rb[:B], ri[:B]) if es else (per_it[6][:B], np.full(B, 7))
    if es:
        print(f"Z = {z}: stops {np.unique(want_i).tolist()}")
        assert len(np.unique(want_i)) >= 2
    bits, it, fi = run(H, llr[:B], 7, 0.75, es, cuda)
    assert np.array_equal(bits, want_b) and np.array_equal(fi, want_i) and it == int(want_i.max())
    b2, i2, f2 = run(H, llr[:B], 7, 0.75, es, cuda, any_graph=True)
    assert np.array_equal(b2, bits) and i2 == it and np.array_equal(f2, fi)
    dec = LayeredMinSumDecoder(H, 7, 0.75, early_stopping=es, precision="fp16")
    x = torch.from_numpy(llr[:B]).to(cuda)
    assert dec.graph(cuda).set_variant(1) == 0
    b3, _, f3 = dec.decode(x, out_dtype=torch.uint8, return_frame_iters=True)
    assert np.array_equal(b3.cpu().numpy(), bits) and np.array_equal(f3.cpu().numpy(), fi)
    monkeypatch.setenv("LDPC_FLOOD_STREAM", "1")
    b4, i4, f4 = run(H, llr[:B], 7, 0.75, es, cuda)
    assert np.array_equal(b4, bits) and i4 == it and np.array_equal(f4, fi)


# ------------------------------------------------------------------------------------ non-QC
def random_H(dense_row):
    """The 24 x 50 graph of test_layered_stream_gpu, restated."""
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
def test_non_qc_graph(cuda, dense_row):
    """Every check is its own layer or shares one with few others: many short launches.  The dense row
    (degree 16) takes the two-pass form of the check rule."""
    H = random_H(dense_row)
    code = LHR.Code(H)
    dmax = int(H.sum(1).max())
    assert code.deg1[48:].all() and (12 < dmax <= 32) == dense_row
    rng = np.random.default_rng(9)
    llr = rng.normal(0.8, 1.6, size=(131, 50)).astype(np.float32)
    Ht = torch.from_numpy(H)
    trace = []
    LHR.decode(code, llr, 6, 0.75, trace=trace)
    for iters in (1, 6):
        bits, _, _ = run(Ht, llr, iters, 0.75, False, cuda)
        assert np.array_equal(bits, trace[iters - 1][2]), iters
    rb, ri = LHR.decode(code, llr, 12, 0.75, LHR.ES_FRAME)
    bits, it, fi = run(Ht, llr, 12, 0.75, "frame", cuda)
    print(f"stops {np.unique(ri).tolist()}")
    assert len(np.unique(ri)) >= 2
    assert np.array_equal(fi, ri) and np.array_equal(bits, rb) and it == int(ri.max())


def tiny_H():
    """The 3 x 6 graph of test_layered_half_ref_host: check 1 has degree 1 and sends +a * C."""
    return np.array([[1, 1, 1, 0, 1, 0],
                     [0, 0, 0, 0, 0, 1],
                     [0, 1, 1, 1, 0, 1]], dtype=np.float32)


@pytest.mark.parametrize("es", [False, "frame"])
def test_degree_one_check(cuda, es):
    H = tiny_H()
    rng = np.random.default_rng(3)
    llr = rng.normal(1.0, 2.0, size=(9, 6)).astype(np.float32)
    llr[4, 5] = -700.0  # against +a * C from the degree-1 check
    llr[6, 5] = -800.0
    for alpha in (0.75, 1.0):
        rb, ri = LHR.decode(LHR.Code(H), llr, 4, alpha, LHR.ES_FRAME if es else LHR.ES_OFF)
        bits, _, fi = run(torch.from_numpy(H), llr, 4, alpha, es, cuda)
        assert np.array_equal(bits, rb) and np.array_equal(fi, ri)


# ------------------------------------------------------------------- clamp, rounding, specials, zeros
def test_z4_saturating(cuda, oracle_mod):
    H = H_of(4, base_z=4)
    code = LHR.Code(H.numpy())
    llr = LHR.saturating(awgn(oracle_mod, 8, code.N, 0.0))
    for es, mode in ((False, LHR.ES_OFF), ("frame", LHR.ES_FRAME)):
        rb, ri = LHR.decode(code, llr, 50, 0.75, mode)
        bits, _, fi = run(H, llr, 50, 0.75, es, cuda)
        assert np.array_equal(bits, rb) and np.array_equal(fi, ri)


@pytest.mark.parametrize("scale", [256.0, 4096.0])
def test_z4_clamp_in_iteration_one(cuda, oracle_mod, scale):
    """LLRs scaled so far that posteriors pass C inside iteration 1, while every c2v is still +0: t = clamp(app)
    there, not x.  The input is asserted to have that property (a decoder without the iteration-1 clamp decides
    otherwise after iteration 1), then the kernel equals the restatement after 1 and 10 iterations, both modes."""
    H = H_of(4, base_z=4)
    code = LHR.Code(H.numpy())
    llr = LHR.saturating(oracle_mod.awgn_llr(64, code.N, 0.0, seed=3).astype(np.float32), scale)
    rb, ri, per_it = ref_both(code, llr, 10)
    wrong = LHR.first_iteration_unclamped(code, llr, 0.75)
    print(f"scale {scale}: bits that differ after iteration 1 without its clamp {int((wrong != per_it[0]).sum())}, "
          f"stops {np.unique(ri).tolist()}")
    assert (wrong != per_it[0]).any()
    for iters in (1, 10):
        bits, _, fi = run(H, llr, iters, 0.75, False, cuda)
        assert np.array_equal(bits, per_it[iters - 1]) and (fi == iters).all()
    bits, _, fi = run(H, llr, 10, 0.75, "frame", cuda)
    assert np.array_equal(bits, rb) and np.array_equal(fi, ri)


def test_z12_specials(cuda, oracle_mod, H12, code12):
    llr = LHR.with_specials(awgn(oracle_mod, 9, code12.N, -2.0))
    for v in LHR.SPECIALS:
        assert (llr == v).any()
    rb, ri = LHR.decode(code12, llr, 6, 0.75, LHR.ES_FRAME)
    bits, _, fi = run(H12, llr, 6, 0.75, "frame", cuda)
    assert np.array_equal(bits, rb) and np.array_equal(fi, ri)


@pytest.mark.parametrize("es", [False, "frame"])
def test_z12_zeros(cuda, oracle_mod, H12, code12, es):
    llr = awgn(oracle_mod, 8, code12.N, -3.0)
    llr[1, :40] = 0.0
    llr[1, 300:320] = -0.0
    rb, ri = LHR.decode(code12, llr, 8, 0.75, LHR.ES_FRAME if es else LHR.ES_OFF)
    bits, _, fi = run(H12, llr, 8, 0.75, es, cuda)
    assert np.array_equal(bits, rb) and np.array_equal(fi, ri)


@pytest.mark.parametrize("es", [False, "frame"])
@pytest.mark.parametrize("victims", [(2,), (3,), (2, 3)])
def test_z12_nan_isolation(cuda, oracle_mod, H12, code12, es, victims):
    """A NaN in a low half (frame 2), a high half (frame 3) or both: every finite frame, the victim's lane
    partner included, decodes exactly as it does alone.  +-inf (frame 7) is a defined input: it clamps."""
    llr = awgn(oracle_mod, 16, code12.N, -2.0)
    for b in victims:
        llr[b, 11] = np.nan
    llr[7, 5] = np.inf
    llr[7, 100] = -np.inf
    finite = [b for b in range(16) if b not in victims]
    rb, ri = LHR.decode(code12, llr[finite], 6, 0.75, LHR.ES_FRAME if es else LHR.ES_OFF)
    bits, _, fi = run(H12, llr, 6, 0.75, es, cuda)
    alone, _, fa = run(H12, llr[finite], 6, 0.75, es, cuda)
    assert np.array_equal(bits[finite], alone) and np.array_equal(fi[finite], fa)
    assert np.array_equal(alone, rb) and np.array_equal(fa, ri)  # the inf frame among them
    assert set(np.unique(bits[list(victims)]).tolist()) <= {0, 1}
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
    else:
        assert it == 8
    run(H12, llr[:37], 8, 0.75, es, cuda, counters=cnt)
    b2, _, f2 = run(H12, llr[:37], 8, 0.75, es, cuda)
    want2 = [int(b2.sum()), int(b2.any(1).sum()), 37, int(f2.sum())]
    assert cnt.tolist() == [a + b for a, b in zip(want, want2)]


@pytest.mark.parametrize("es", [False, "frame"])
def test_frame_independence(cuda, H12, ref12_frame, es):
    """A frame's result does not depend on the batch it rides in, on its place in it, nor on the half of the
    lane it falls in: reversed at an odd offset, every frame changes half and partner."""
    llr = ref12_frame[0][:70]
    full, _, fi = run(H12, llr, 5, 0.75, es, cuda)
    dec = LayeredMinSumDecoder(H12, 5, 0.75, early_stopping=es, precision="fp16")
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
    """Z = 96, B = 120 000: E * B = 2.27e9 binary16 messages, 4.5e9 bytes: (edge, frame) offsets pass 2^31
    elements and 2^32 bytes."""
    free, _ = torch.cuda.mem_get_info(cuda)
    if free < 20 * 2**30:
        pytest.skip(f"needs about 8 GB of device memory next to its inputs; {free / 2**30:.1f} GB free")
    H = H_of(96)
    B, E = 120_000, int(H.sum())
    assert E * B > 2**31 and 113_551 * E < 2**31 < 113_552 * E
    llr = awgn_llr(B, H.shape[1], -3.0, seed=7, device=cuda)
    dec = LayeredMinSumDecoder(H, 2, 0.75, early_stopping=False, precision="fp16")
    bits, _ = dec.decode(llr, out_dtype=torch.uint8)
    frames = [0, 63, 64, 127, 128] + list(range(113_550, 113_561)) + [B - 129, B - 1]
    idx = torch.tensor(frames, device=cuda)
    small, _ = dec.decode(llr[idx].contiguous(), out_dtype=torch.uint8)
    assert torch.equal(bits[idx], small)
    assert 0 < int(small.sum()) < small.numel()


# ------------------------------------------------------------------- errors
def raw_decode(g, llr, iters, es, cuda, algo=ALGO, alpha=0.75, ws_bytes=None):
    bits = torch.empty(llr.shape, dtype=torch.uint8, device=cuda)
    need = N.check(N.lib().ldpc_layered_half_workspace_size(g.handle, llr.shape[0], iters, es))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=cuda)
    return N.lib().ldpc_flood_decode(g.handle, algo, N.ptr(llr), llr.shape[0], iters, alpha, es, N.LDPC_OUT_U8,
                                     N.ptr(bits), None, None, None, N.ptr(ws), need if ws_bytes is None else ws_bytes(need),
                                     N.stream_ptr(cuda))


def test_abi_errors(cuda, H12):
    lib = N.lib()
    x12 = torch.ones(3, H12.shape[1], device=cuda)
    g = LayeredMinSumDecoder(H12, 2, precision="fp16").graph(cuda)
    assert raw_decode(g, x12, 2, N.LDPC_ES_BATCH, cuda) == N.LDPC_EINVAL
    assert b"batch-global" in lib.ldpc_last_error()
    assert raw_decode(g, x12, 2, N.LDPC_ES_OFF, cuda) == 0
    assert raw_decode(g, x12, 2, N.LDPC_ES_FRAME, cuda) == 0
    for alpha in (1.5, -0.25, float("nan")):
        assert raw_decode(g, x12, 2, N.LDPC_ES_OFF, cuda, alpha=alpha) == N.LDPC_EINVAL
        assert b"alpha" in lib.ldpc_last_error()
    assert raw_decode(g, x12, 2, N.LDPC_ES_OFF, cuda, ws_bytes=lambda need: need - 1) == N.LDPC_EINVAL  # one byte short
    assert b"workspace too small: need " in lib.ldpc_last_error()
    assert raw_decode(g, x12, 2, N.LDPC_ES_OFF, cuda, ws_bytes=lambda need: 0) == N.LDPC_EINVAL
    assert raw_decode(g, x12, 2, N.LDPC_ES_OFF, cuda, algo=4) == N.LDPC_EINVAL
    assert b"unknown algo" in lib.ldpc_last_error()
    # the workspace query: zero work, bad arguments
    assert lib.ldpc_layered_half_workspace_size(g.handle, 0, 5, 0) == 0
    assert lib.ldpc_layered_half_workspace_size(g.handle, 5, 0, 0) == 0
    assert lib.ldpc_layered_half_workspace_size(g.handle, -1, 5, 0) == N.LDPC_EINVAL
    assert lib.ldpc_layered_half_workspace_size(None, 5, 5, 0) == N.LDPC_EINVAL
    # no redo list
    n = ctypes.c_int32(-1)
    ws = torch.zeros(1024, dtype=torch.uint8, device=cuda)
    assert lib.ldpc_flood_redo_count(g.handle, ALGO, 3, 2, N.LDPC_ES_OFF, N.ptr(ws), None, ctypes.byref(n),
                                     None) == N.LDPC_EUNSUPPORTED
    with pytest.raises(ValueError):
        LayeredMinSumDecoder(H12, 3, precision="fp16").decode(x12[:, :-1])


def test_flood_workspace_answer_is_too_small_on_an_lds_graph(cuda):
    """On Z = 32 ldpc_flood_workspace_size sizes the LDS-resident decoders' scratch: not enough for algo 6."""
    H = H_of(32)
    g = LayeredMinSumDecoder(H, 2, precision="fp16").graph(cuda)
    x = torch.ones(40, H.shape[1], device=cuda)
    flood = N.check(N.lib().ldpc_flood_workspace_size(g.handle, 40, 2, N.LDPC_ES_OFF))
    need = N.check(N.lib().ldpc_layered_half_workspace_size(g.handle, 40, 2, N.LDPC_ES_OFF))
    assert 0 < flood < need
    assert raw_decode(g, x, 2, N.LDPC_ES_OFF, cuda, ws_bytes=lambda _: flood) == N.LDPC_EINVAL
    assert b"workspace too small" in N.lib().ldpc_last_error()
    assert raw_decode(g, x, 2, N.LDPC_ES_OFF, cuda) == 0


def test_degree_above_32(cuda):
    H = np.zeros((3, 40), dtype=np.float32)
    H[0, :33] = 1
    H[1, 30:36] = 1
    H[2, 34:40] = 1
    llr = np.ones((5, 40), dtype=np.float32)
    with pytest.raises(N.NativeError, match="degree above 32") as e:
        run(torch.from_numpy(H), llr, 2, 0.75, False, cuda)
    assert f"error {N.LDPC_EUNSUPPORTED}:" in str(e.value)


# ------------------------------------------------------------------- the float32 decoders are untouched
def test_fp32_untouched(cuda, oracle_mod, H12, code12):
    """After an fp16 decode on the same device: any_graph=True on Z = 12 still equals layered_ref; the default
    class still refuses Z = 12 (no LDS-resident schedule) and still equals layered_ref where it runs (Z = 4)."""
    llr = awgn(oracle_mod, 70, code12.N, -3.0)
    run(H12, llr, 8, 0.75, "frame", cuda)
    rb, ri = LR.decode(code12, llr, 8, 0.75, LR.ES_FRAME)
    bits, it, fi = run(H12, llr, 8, 0.75, "frame", cuda, precision="fp32", any_graph=True)
    assert np.array_equal(bits, rb) and np.array_equal(fi, ri) and it == int(ri.max())
    with pytest.raises(N.NativeError, match="LDS-resident"):
        LayeredMinSumDecoder(H12, 2, early_stopping=False).decode(torch.from_numpy(llr).to(cuda))
    H4 = H_of(4, base_z=4)
    llr4 = awgn(oracle_mod, 50, H4.shape[1], -2.0)
    run(H4, llr4, 7, 0.75, "frame", cuda)
    rb4, ri4 = LR.decode(LR.Code(H4.numpy()), llr4, 7, 0.75, LR.ES_FRAME)
    dec = LayeredMinSumDecoder(H4, 7, 0.75)  # default arguments
    b4, _, f4 = dec.decode(torch.from_numpy(llr4).to(cuda), out_dtype=torch.uint8, return_frame_iters=True)
    assert dec._algo == N.LDPC_ALGO_LAYERED_MINSUM
    assert np.array_equal(b4.cpu().numpy(), rb4) and np.array_equal(f4.cpu().numpy(), ri4)
