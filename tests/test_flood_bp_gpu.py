"""Sum-product (BP) decoders against the oracle under the per-variable rule of bp_rule.py (GPU).

Every BP kernel path -- the compile-time schedules, the table-driven kernel, the streaming kernels
(forced and chosen natively), Z = 1 graphs including a check row past the unrolled degrees -- in
every stopping mode: on clean frames bits (and per-frame / batch iteration counts, counters) equal
the oracle's; on the other frames bits are equal on every decided variable.  Paths that decode the
same input are bit-identical to each other.  Special inputs (zeros, +-inf, NaN, saturating LLRs)
and frame independence are exact.

Measured on an MI355X (pytest -s prints them): 0 differing bits on non-decided variables in every
case of this file; the clean shares are those asserted on the CPU side (SEEDS below).
"""
import os

import numpy as np
import pytest
import torch

from conftest import PKG, code_path

from bp_rule import Rule, on_codewords, qpsk_llr, random_codewords
from ldpc_neural_decoder import _native as N
from ldpc_neural_decoder.models import BeliefPropagationDecoder
from ldpc_neural_decoder.utils import expand_base_matrix, load_base_matrix
from reg_edges_util import parse_header

pytestmark = pytest.mark.gpu
OFF, BATCH, FRAME = N.LDPC_ES_OFF, N.LDPC_ES_BATCH, N.LDPC_ES_FRAME
# regime -> iterations.  low: -4 dB, |LLR| clipped to 8, no tanh product reaches +-1.  sat: 16
# frames each at -2 / 0 / 2 dB: messages saturate to +-inf within 3 .. 5 iterations (the regime the
# benchmark runs in) and frames stop at iterations 2 .. 9.
T_OF = {"low": 6, "sat": 10}
# seeds checked on the CPU: clean frames of 48 -- Z=4 low 47, sat 48; Z=32 low 43, sat 44 -- and
# the first 1 / 5 / 37 frames hold the floor as well
SEEDS = {(4, "low"): 401, (4, "sat"): 401, (32, "low"): 3215, (32, "sat"): 3205}


def make_batch(code, z, regime, n_frames=48):
    """channel noise on random codewords (the rule is blind to the codeword: tanh and atanh are odd)"""
    rng = np.random.default_rng(SEEDS[z, regime])
    if regime == "low":
        x = qpsk_llr(rng, n_frames, 52 * z, -4.0, clip=8.0)
    else:
        x = np.concatenate([qpsk_llr(rng, n_frames // 3, 52 * z, s) for s in (-2.0, 0.0, 2.0)])
    return on_codewords(x, code.codewords(rng, n_frames))


class Code:
    """one parity-check matrix: the library's graph, the oracle's, and cached Rules"""

    def __init__(self, H, oracle_mod, cuda):
        self.H = H
        self.dec = BeliefPropagationDecoder(H, 10, early_stopping=False)
        self.g = self.dec.graph(cuda)
        self.og = oracle_mod.Graph(H.numpy())
        self._o, self._rules, self._stops = oracle_mod, {}, {}

    def codewords(self, rng, n):
        return random_codewords(self.H.numpy(), rng, n)

    def rule(self, key, x=None, T=None):
        if key not in self._rules:
            self._rules[key] = Rule(self._o, self.og, x, T)
        return self._rules[key]

    def stop_ref(self, key, es, frames):
        """mode-0 oracle under early stop on rows `frames` of the rule's batch (cached)"""
        k = (key, es, tuple(frames))
        if k not in self._stops:
            r = self._rules[key]
            self._stops[k] = self._o.flood_decode(self.og, r.x[list(frames)], "bp", r.T, 0.0, es)
        return self._stops[k]


@pytest.fixture(scope="module")
def codes(oracle_mod, cuda):
    cache = {}

    def get(z, base_z=None):
        if (z, base_z) not in cache:
            H = expand_base_matrix(load_base_matrix(code_path(base_z or z)), z)
            cache[z, base_z] = Code(H, oracle_mod, cuda)
        return cache[z, base_z]
    return get


def run(g, x, iters, es, cuda, out=N.LDPC_OUT_U8):
    """ldpc_flood_decode, BP, every output -> (bits, per-frame iterations, batch iterations, counters)"""
    B = x.shape[0]
    llr = torch.from_numpy(np.ascontiguousarray(x)).to(cuda)
    bits = torch.empty((B, g.N), dtype=torch.uint8 if out == N.LDPC_OUT_U8 else torch.float32, device=cuda)
    fi = torch.full((B,), -1, dtype=torch.int32, device=cuda)
    bi = torch.zeros(1, dtype=torch.int32, device=cuda)
    cnt = torch.zeros(4, dtype=torch.int64, device=cuda)
    wsb = N.check(N.lib().ldpc_flood_workspace_size(g.handle, B, iters, es))
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=cuda)
    N.check(N.lib().ldpc_flood_decode(g.handle, N.LDPC_ALGO_BP, N.ptr(llr), B, iters, 0.0, es, out, N.ptr(bits),
                                      N.ptr(fi), N.ptr(bi), N.ptr(cnt), N.ptr(ws), wsb, N.stream_ptr(cuda)))
    torch.cuda.synchronize()
    b = bits.cpu().numpy()
    if out != N.LDPC_OUT_U8:
        assert np.isin(b, (0.0, 1.0)).all()
        b = b.astype(np.uint8)
    return b, fi.cpu().numpy(), int(bi.item()), cnt.cpu().numpy().tolist()


def counters(bits, it):
    return [int(bits.sum()), int((bits.sum(1) > 0).sum()), bits.shape[0], int(it.sum())]


def check_path(code, key, frames, cuda, where, modes=(OFF, FRAME, BATCH), floor=True, out=N.LDPC_OUT_U8):
    """One kernel path (whatever code.g is set to) on rows `frames` of the rule's batch, in every
    stopping mode, against the oracle.  Returns every output, for exact comparison between paths."""
    r = code.rule(key)
    frames = np.asarray(frames)
    x = r.x[frames]
    clean = r.clean[frames]
    if floor:
        r.check_floor(frames)
    res, loose = {}, 0
    if OFF in modes:
        for t in sorted({1, 2, r.T}):
            bits, fi, bi, cnt = res[OFF, t] = run(code.g, x, t, OFF, cuda, out)
            loose += r.check_bits(bits, t, frames, where)
            assert (fi == t).all() and bi == t and cnt == counters(bits, fi), (where, t)
    if FRAME in modes:
        bits, fi, bi, cnt = res[FRAME] = run(code.g, x, r.T, FRAME, cuda, out)
        rb, _, _, ri = code.stop_ref(key, 2, range(r.x.shape[0]))
        rb, ri = rb[frames], ri[frames]
        assert np.array_equal(fi[clean], ri[clean]), (where, "per-frame iteration counts on clean frames")
        assert np.array_equal(bits[clean], rb[clean]), (where, "bits of clean frames, per-frame stop")
        for k in np.flatnonzero(~clean & (fi == ri)):  # same final iteration: its decided variables
            dec = r.decided[ri[k] - 1, frames[k]]
            assert np.array_equal(bits[k][dec], rb[k][dec]), (where, "decided bits, per-frame stop", int(frames[k]))
            loose += int((bits[k] != rb[k]).sum())
        assert bi == fi.max() and cnt == counters(bits, fi), where
    if BATCH in modes and clean.any():
        sel = frames[clean]  # the batch-global stop couples the frames: clean ones only, then all is exact
        bits, fi, bi, cnt = res[BATCH] = run(code.g, r.x[sel], r.T, BATCH, cuda, out)
        rb, _, rn, ri = code.stop_ref(key, 1, sel)
        assert bi == rn and np.array_equal(fi, ri), (where, "batch stop iteration", bi, rn)
        assert np.array_equal(bits, rb), (where, "bits, batch stop")
        assert cnt == counters(rb, ri), (where, "counters, batch stop")
    print(f"{where}: {int(clean.sum())} of {clean.size} frames clean, {loose} bits differ on non-decided variables")
    return res


def assert_same(a, b, where):
    assert a.keys() == b.keys()
    for k in a:
        for u, v in zip(a[k], b[k]):
            assert np.array_equal(u, v), (where, k)


# ---------------------------------------------------------------- the reference's two codes
@pytest.mark.parametrize("regime", ["low", "sat"])
@pytest.mark.parametrize("z,B", [(32, 1), (32, 5), (32, 48), (4, 1), (4, 37), (4, 48)])
def test_fixed_and_table_driven_vs_oracle(cuda, codes, z, B, regime):
    """One group, a tail group, several groups; the compile-time schedule and the table-driven
    kernel, each against the oracle and bit-identical to each other."""
    code = codes(z)
    code.rule(regime, make_batch(code, z, regime), T_OF[regime])
    try:
        assert code.g.set_variant(1) == 0
        tab = check_path(code, regime, range(B), cuda, f"table-driven Z={z} B={B} {regime}")
        assert code.g.set_variant(0) == (2 if z == 32 else 1)
        fix = check_path(code, regime, range(B), cuda, f"fixed Z={z} B={B} {regime}")
    finally:
        code.g.set_variant(0)
    assert_same(fix, tab, (z, B, regime))


@pytest.mark.parametrize("regime", ["low", "sat"])
@pytest.mark.parametrize("B", [5, 48])
def test_forced_streaming_vs_oracle(cuda, codes, monkeypatch, B, regime):
    """The streaming kernels on the reference's Z = 32 code, float32 output: against the oracle, and
    bit-identical to the LDS-resident kernel with uint8 output."""
    code = codes(32)
    code.rule(regime, make_batch(code, 32, regime), T_OF[regime])
    lds = check_path(code, regime, range(B), cuda, f"fixed Z=32 B={B} {regime}")
    monkeypatch.setenv("LDPC_FLOOD_STREAM", "1")
    st = check_path(code, regime, range(B), cuda, f"streaming Z=32 B={B} {regime}", out=N.LDPC_OUT_F32)
    assert_same(lds, st, (B, regime))


@pytest.mark.parametrize("z,B,snr,seed", [(12, 40, 0.0, 1203), (96, 9, 2.0, 9601)])
def test_native_streaming_vs_oracle(cuda, codes, z, B, snr, seed):
    """Liftings that do not divide 64 decode on the streaming kernels by themselves (the BG2 base of
    the Z = 32 code lifted to Z, as test_lifting_sizes_beyond_lds does), 8 iterations.  Z = 96 runs
    at 2 dB: a frame of 4992 variables is rarely clean at 0 dB (3 .. 5 of 9 over three seeds, against
    36 of 40 at Z = 12), since one weak variable at one iteration is enough; seed chosen on the CPU
    (9 of 9 clean, frames stop at iterations 3 and 4)."""
    code = codes(z, 32)
    rng = np.random.default_rng(seed)
    x = on_codewords(qpsk_llr(rng, B, 52 * z, snr), code.codewords(rng, B))
    code.rule("stream", x, 8)
    check_path(code, "stream", range(B), cuda, f"streaming Z={z} B={B}")


# ---------------------------------------------------------------- Z = 1 graphs
def z1_matrix(kind):
    if kind == "hamming":
        return np.array([[1, 1, 0, 1, 1, 0, 0], [1, 0, 1, 1, 0, 1, 0], [0, 1, 1, 1, 0, 0, 1]], np.float32)
    rng = np.random.default_rng(5)  # the random code of test_generic_code_z1
    H = np.zeros((30, 60), dtype=np.float32)
    for j in range(60):
        H[rng.choice(30, size=3, replace=False), j] = 1
    if kind == "dc26":  # check 7 gets degree 26: past kMaxUnroll, the BP branch of check_task_dyn
        free = np.flatnonzero(H[7] == 0)
        H[7, free[:26 - int(H[7].sum())]] = 1
        assert H[7].sum() == 26
    return H


@pytest.mark.parametrize("kind,snr", [("hamming", 4.0), ("random", 1.0), ("dc26", 1.0)])
def test_z1_graphs_vs_oracle(cuda, oracle_mod, kind, snr):
    """Non-QC matrices (one frame per lane, B = 70: a full group and a tail group of 6)."""
    code = Code(torch.from_numpy(z1_matrix(kind)), oracle_mod, cuda)
    assert code.g.Z == 1 and code.g.max_dc == {"hamming": 4, "dc26": 26}.get(kind, code.g.max_dc)
    rng = np.random.default_rng(70)
    x = on_codewords(qpsk_llr(rng, 70, code.g.N, snr), code.codewords(rng, 70))
    code.rule("z1", x, 6)
    check_path(code, "z1", range(70), cuda, f"Z=1 {kind}")


# ---------------------------------------------------------------- special inputs
@pytest.fixture(scope="module")
def columns():
    """the column choices of test_flood_bail_redo_gpu.py: a register-edge, a degree-1, a slot column"""
    with open(os.path.join(PKG, "csrc", "gen", "fixed_codes.hpp")) as f:
        tabs = parse_header(f.read())
    out = {}
    for z in (32, 4):
        t = tabs[f"BG2_Z{z}"]
        dv = np.diff(t["COL_PTR"])
        reg = sorted({t["BLK_COL"][e] for e, r in enumerate(t["RE_ROW_REG"]) if r >= 0})
        out[z] = {"reg": reg[len(reg) // 2], "deg1": int(np.flatnonzero(dv == 1)[3]),
                  "slot": next(c for c in range(t["Nb"]) if dv[c] >= 2 and c not in reg),
                  "zeroed": [reg[::2], list(np.flatnonzero(dv == 1)[::2]), list(range(0, t["Nb"], 3))]}
    return out


NAN_F, ZERO_F, P30_F, PINF_F, NINF_F = 1, 2, 3, 4, 5  # frames of the special batch; 6, 7, 8: zeroed columns
WEAK = (NAN_F, PINF_F, NINF_F, 6, 7, 8)  # NaN APPs (inf - inf as well) or many erased variables: rarely clean


def special_batch(code, z, B, cols, where):
    rng = np.random.default_rng(900 + z)
    x = on_codewords(qpsk_llr(rng, B, 52 * z, 2.0), code.codewords(rng, B))
    c = cols[where] * z
    x[NAN_F, c + 1] = np.nan  # frame 1 of group 0
    x[ZERO_F] = 0.0
    x[P30_F] = 30.0
    x[PINF_F, c + 2] = np.inf
    x[NINF_F, c] = -np.inf
    for f, pick in zip((6, 7, 8), cols["zeroed"]):
        for q in pick:
            x[f, q * z:(q + 1) * z] = 0.0
    return x


@pytest.mark.parametrize("where", ["reg", "deg1", "slot"])
@pytest.mark.parametrize("z,B", [(32, 13), (4, 37)])
def test_special_inputs(cuda, codes, columns, monkeypatch, z, B, where):
    """Zeros, a saturating frame, +-inf and NaN through the fixed, table-driven and streaming BP
    kernels (Z = 32: seven groups, the last a tail group of one; Z = 4: three, the last of five).
    The frames in WEAK are compared on their decided variables; the floor on clean frames is asserted
    on all the others, the all-zero and the all +30 frame among them."""
    code = codes(z)
    key = ("special", where)
    x = special_batch(code, z, B, columns[z], where)
    r = code.rule(key, x, 6)
    both_nan = np.isnan(r.a[0]) & np.isnan(r.a[1])
    assert both_nan[:, NAN_F].any()
    assert r.clean[[ZERO_F, P30_F]].all()
    assert r.decided[:, [PINF_F, NINF_F, 6, 7, 8]].mean(axis=(0, 2)).min() > 0.5  # the comparison is not vacuous
    r.check_floor([f for f in range(B) if f not in WEAK])
    y = x.copy()
    y[NAN_F] = x[0]  # the same batch without the NaN frame
    others = np.arange(B) != NAN_F
    results = {}
    for path in ("table", "fixed", "stream"):
        assert code.g.set_variant(1 if path == "table" else 0) == (0 if path == "table" else (2 if z == 32 else 1))
        if path == "stream":
            monkeypatch.setenv("LDPC_FLOOD_STREAM", "1")
        try:
            res = results[path] = check_path(code, key, range(B), cuda, f"special {where} {path} Z={z}",
                                             modes=(OFF, FRAME), floor=False)
            for t in (1, 2, r.T):
                bits = res[OFF, t][0]
                assert not bits[ZERO_F].any() and not bits[P30_F].any(), (path, t)
                assert not bits[both_nan[t - 1]].any(), (path, t, "bit of a NaN APP")
                ref = r.b[0, t - 1]
                dec = r.decided[t - 1]
                for f in (PINF_F, NINF_F, 6, 7, 8, NAN_F):
                    assert np.array_equal(bits[f][dec[f]], ref[f][dec[f]]), (path, t, f)
                # GPU against GPU, exact: the NaN frame leaves the other frames of its group alone
                assert np.array_equal(bits[others], run(code.g, y, t, OFF, cuda)[0][others]), (path, t)
            fb, ff, _, _ = res[FRAME]
            yb, yf, _, _ = run(code.g, y, r.T, FRAME, cuda)
            assert np.array_equal(fb[others], yb[others]) and np.array_equal(ff[others], yf[others]), path
        finally:
            code.g.set_variant(0)
    assert_same(results["fixed"], results["table"], where)
    assert_same(results["fixed"], results["stream"], where)


# ---------------------------------------------------------------- frame independence
@pytest.mark.parametrize("path", ["fixed", "table", "stream"])
@pytest.mark.parametrize("z,B", [(32, 5), (4, 37)])
def test_frame_independence(cuda, codes, monkeypatch, z, B, path):
    """Exact, GPU against GPU: a frame decoded alone equals the same frame in position 0, in the
    middle and in the tail group of a batch; 512 frames made by tiling the 48 equal the small
    result copy by copy (stop off and per frame)."""
    code = codes(z)
    x = make_batch(code, z, "sat")
    if path == "stream":
        monkeypatch.setenv("LDPC_FLOOD_STREAM", "1")
    try:
        code.g.set_variant(1 if path == "table" else 0)
        for es in (OFF, FRAME):
            small = run(code.g, x, 10, es, cuda)
            part = run(code.g, x[:B], 10, es, cuda)
            for f in (0, B // 2, B - 1):
                alone = run(code.g, x[f:f + 1], 10, es, cuda)
                for a, s, p in zip(alone[:2], small[:2], part[:2]):
                    assert np.array_equal(a[0], s[f]) and np.array_equal(a[0], p[f]), (es, f)
            big = run(code.g, np.tile(x, (11, 1))[:512], 10, es, cuda)
            for k in range(0, 512, 48):
                n = min(48, 512 - k)
                assert np.array_equal(big[0][k:k + n], small[0][:n]), (es, k)
                assert np.array_equal(big[1][k:k + n], small[1][:n]), (es, k)
            assert big[2] == small[2]
    finally:
        code.g.set_variant(0)
