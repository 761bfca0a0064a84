"""Fixed flood kernel, min-sum: bail out and decode again instead of an exact path in the kernel (GPU).

With a workspace, the min-sum instances of flood_fixed_kernel without early stop and with the
per-frame stop hold the fast check update only.  A workgroup (one group of 64 / Z frames) that
meets a non-finite LLR or APP appends its group to a redo list and leaves; flood_redo_kernel then
decodes the listed groups from scratch with the table-driven update.  Checked here, against the
oracle and against the table-driven kernel: bits, per-frame iteration counts and the counters are
exact whichever path a group took, and ldpc_flood_redo_count shows that the path was the expected
one: none for finite inputs however many zeros they hold, exactly the groups that meet a
non-finite value otherwise.  The batch-global stop keeps its exact check update in the kernel and
is run on the same inputs.

Which groups are expected on the list is derived from the oracle: a group whose frames hold a
non-finite LLR (raised in the kernel's init), or a non-finite APP after an iteration that the group
still follows with another one (raised in the variable phase, read before the next check phase).
Lanes of a tail group that have no frame compute on frame 0's LLRs, so frame 0 stays ordinary.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import PKG, code_path

from ldpc_neural_decoder import _native as N
from ldpc_neural_decoder.models import MinSumScaledDecoder
from ldpc_neural_decoder.utils import expand_base_matrix, load_base_matrix
from reg_edges_util import parse_header

pytestmark = pytest.mark.gpu
ALPHA = 0.75
ITERS = (1, 2, 3, 10)
# (Z, B): B = 5 for both codes; at Z = 32 that is three groups of two frames, the last a tail group,
# at Z = 4 one group of 16, so Z = 4 also runs B = 37: three groups, the last a tail group
SHAPES = [(32, 5), (4, 5), (4, 37)]
ES = {"off": (N.LDPC_ES_OFF, 0), "frame": (N.LDPC_ES_FRAME, 2), "batch": (N.LDPC_ES_BATCH, 1)}


@pytest.fixture(scope="module")
def codes(oracle_mod, cuda):
    with open(os.path.join(PKG, "csrc", "gen", "fixed_codes.hpp")) as f:
        tabs = parse_header(f.read())
    out = {}
    for z in (32, 4):
        H = expand_base_matrix(load_base_matrix(code_path(z)), z)
        dec = MinSumScaledDecoder(H, 10, ALPHA, early_stopping=False)
        t = tabs[f"BG2_Z{z}"]
        dv = np.diff(t["COL_PTR"])
        reg = sorted({t["BLK_COL"][e] for e, r in enumerate(t["RE_ROW_REG"]) if r >= 0})
        cols = {"reg": reg[len(reg) // 2], "deg1": int(np.flatnonzero(dv == 1)[3]),
                "slot": next(c for c in range(t["Nb"]) if dv[c] >= 2 and c not in reg)}
        out[z] = (dec.graph(cuda), oracle_mod.Graph(H.numpy()), t, cols, dec)
    return out


def grid(z, B, seed=0):
    """LLRs k / 4, |k| <= 12: with alpha = 0.75 exact-zero messages and ties are common"""
    rng = np.random.default_rng(7000 + 10 * z + seed)
    return (rng.integers(-12, 13, size=(B, 52 * z)) / 4).astype(np.float32)


def groups_of(z, B):
    fg = 64 // z
    return fg, (B + fg - 1) // fg


def inputs(kind, z, B, t, cols):
    """-> (llr, groups that hold the special frames)"""
    fg, ng = groups_of(z, B)
    x = grid(z, B)
    mid = ng // 2                     # the middle group (the only one when ng == 1)
    f_mid = min(mid * fg + 1, B - 1)  # not frame 0 unless B == 1
    if kind == "zeros":
        dv = np.diff(t["COL_PTR"])
        reg = sorted({t["BLK_COL"][e] for e, r in enumerate(t["RE_ROW_REG"]) if r >= 0})
        for f in range(1, B):
            pick = {1: reg[::2], 2: list(np.flatnonzero(dv == 1)[::2]), 3: list(range(0, t["Nb"], 3))}.get(f % 4, [])
            for c in pick:
                x[f, c * z:(c + 1) * z] = 0.0
        if B > 4:
            x[4] = 0.0
        return x, set()
    if kind == "nan_ends":            # the first and the last group, the middle one stays
        x[1, cols["reg"] * z + 2] = np.nan
        x[B - 1, cols["slot"] * z] = -np.inf
        return x, {0, ng - 1}
    if kind.startswith(("nan", "pinf", "ninf")):
        val, where = kind.split("_")
        x[f_mid, cols[where] * z + 1] = {"nan": np.nan, "pinf": np.inf, "ninf": -np.inf}[val]
        return x, {mid}
    if kind in ("big3e38", "big3e37"):  # finite, overflows in the variable phase of a later iteration
        rng = np.random.default_rng(5)
        sign = np.where(rng.random(52 * z) < 0.1, -1.0, 1.0)
        x[f_mid] = (sign * (3e38 if kind == "big3e38" else 3e37)).astype(np.float32)
        return x, {mid}
    raise AssertionError(kind)


KINDS = ["zeros"] + [f"{v}_{w}" for v in ("nan", "pinf", "ninf") for w in ("slot", "reg", "deg1")] + \
        ["nan_ends", "big3e38", "big3e37"]


def expected_redo(oracle_mod, og, x, z, iters, mode):
    """groups that meet a non-finite value while another check phase is still to come"""
    fg, ng = groups_of(z, x.shape[0])
    grp = np.arange(x.shape[0]) // fg
    runs = np.full(ng, iters)
    if mode == 2:  # a group iterates until all of its frames have stopped
        _, _, _, fi = oracle_mod.flood_decode(og, x, "minsum", iters, ALPHA, 2)
        runs = np.array([fi[grp == q].max() for q in range(ng)])
    bad = {int(q) for q in grp[~np.isfinite(x).all(axis=1)]}
    for t in range(1, iters):
        _, app, _, _ = oracle_mod.flood_decode(og, x, "minsum", t, ALPHA, 0)
        hit = ~np.isfinite(app).all(axis=1)
        bad |= {int(q) for q in grp[hit] if t < runs[q]}
    return bad


def decode(g, x, iters, es, cuda, redo):
    B = x.shape[0]
    llr = torch.from_numpy(x).to(cuda)
    bits = torch.empty((B, g.N), dtype=torch.uint8, device=cuda)
    fi = torch.empty(B, dtype=torch.int32, device=cuda)
    bi = torch.zeros(1, dtype=torch.int32, device=cuda)
    cnt = torch.zeros(4, dtype=torch.int64, device=cuda)
    wsb = N.check(N.lib().ldpc_flood_workspace_size(g.handle, B, iters, es))
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=cuda)
    s = N.stream_ptr(cuda)
    N.check(N.lib().ldpc_flood_decode(g.handle, N.LDPC_ALGO_MINSUM, N.ptr(llr), B, iters, ALPHA, es, N.LDPC_OUT_U8,
                                      N.ptr(bits), N.ptr(fi), N.ptr(bi), N.ptr(cnt), N.ptr(ws), wsb, s))
    listed = None
    if redo:
        n = ctypes.c_int32(-1)
        buf = (ctypes.c_int32 * (B + 1))()
        N.check(N.lib().ldpc_flood_redo_count(g.handle, N.LDPC_ALGO_MINSUM, B, iters, es, N.ptr(ws), s,
                                              ctypes.byref(n), buf))
        listed = sorted(buf[i] for i in range(n.value))
    torch.cuda.synchronize()
    return bits.cpu().numpy(), fi.cpu().numpy(), int(bi.item()), cnt.cpu().numpy().tolist(), listed


def counters(bits, it):
    return [int(bits.sum()), int((bits.sum(1) > 0).sum()), bits.shape[0], int(it.sum())]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("z,B", SHAPES)
def test_bail_and_redo(cuda, oracle_mod, codes, z, B, kind):
    g, og, t, cols, _ = codes[z]
    x, special = inputs(kind, z, B, t, cols)
    fixed_id = 2 if z == 32 else 1
    for iters in ITERS:
        for name in ("off", "frame"):
            es, mode = ES[name]
            ref, _, rn, ri = oracle_mod.flood_decode(og, x, "minsum", iters, ALPHA, mode)
            assert g.set_variant(1) == 0  # table-driven
            tab = decode(g, x, iters, es, cuda, redo=False)
            assert g.set_variant(0) == fixed_id
            bits, fi, bi, cnt, listed = decode(g, x, iters, es, cuda, redo=True)
            where = (z, B, kind, iters, name)
            assert np.array_equal(bits, ref) and np.array_equal(bits, tab[0]), where
            assert np.array_equal(fi, ri) and np.array_equal(fi, tab[1]), where
            assert bi == (iters if name == "off" else ri.max()) and bi == tab[2], where
            assert cnt == counters(ref, ri) and cnt == tab[3], where
            want = expected_redo(oracle_mod, og, x, z, iters, mode)
            assert listed == sorted(want), where
            assert len(set(listed)) == len(listed), where
            if kind == "zeros":
                assert listed == [], where  # zeros, however many, stay on the fast update
            elif not kind.startswith("big"):
                assert listed == sorted(special), where  # a non-finite LLR: raised in init, any iteration count
            else:
                assert set(listed) <= special, where
                if iters == 10 and name == "off":
                    assert listed == sorted(special), where  # by then the frame has overflowed


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("z,B", SHAPES)
def test_batch_stop_keeps_its_exact_update(cuda, oracle_mod, codes, z, B, kind):
    """The batch-global stop's passes share state across workgroups and cannot leave: their exact
    check update stays in the kernel, under the smaller per-instance register-edge cap."""
    g, og, t, cols, _ = codes[z]
    x, _ = inputs(kind, z, B, t, cols)
    es, mode = ES["batch"]
    for iters in ITERS:
        ref, _, rn, ri = oracle_mod.flood_decode(og, x, "minsum", iters, ALPHA, mode)
        assert g.set_variant(1) == 0
        tab = decode(g, x, iters, es, cuda, redo=False)
        assert g.set_variant(0) == (2 if z == 32 else 1)
        bits, fi, bi, cnt, _ = decode(g, x, iters, es, cuda, redo=False)
        where = (z, B, kind, iters)
        assert np.array_equal(bits, ref) and np.array_equal(bits, tab[0]), where
        assert bi == rn and bi == tab[2], where
        assert np.array_equal(fi, ri) and np.array_equal(fi, tab[1]), where
        assert cnt == counters(ref, ri) and cnt == tab[3], where
    n = ctypes.c_int32(-1)
    ws = torch.zeros(1024, dtype=torch.uint8, device=cuda)
    rc = N.lib().ldpc_flood_redo_count(g.handle, N.LDPC_ALGO_MINSUM, B, 10, es, N.ptr(ws), None, ctypes.byref(n), None)
    assert rc == N.LDPC_EUNSUPPORTED


def test_without_a_workspace_the_exact_update_stays_in_the_kernel(cuda, oracle_mod, codes):
    """No workspace, no redo list: the instance with the exact check update inside decodes NaN frames."""
    g, og, t, cols, _ = codes[32]
    x, _ = inputs("nan_reg", 32, 5, t, cols)
    assert g.set_variant(0) == 2
    llr = torch.from_numpy(x).to(cuda)
    for iters in ITERS:
        bits = torch.empty((5, g.N), dtype=torch.uint8, device=cuda)
        N.check(N.lib().ldpc_flood_decode(g.handle, N.LDPC_ALGO_MINSUM, N.ptr(llr), 5, iters, ALPHA, N.LDPC_ES_OFF,
                                          N.LDPC_OUT_U8, N.ptr(bits), None, None, None, None, 0, N.stream_ptr(cuda)))
        torch.cuda.synchronize()
        ref, _, _, _ = oracle_mod.flood_decode(og, x, "minsum", iters, ALPHA, 0)
        assert np.array_equal(bits.cpu().numpy(), ref), iters
