"""Fixed flood kernel: messages of lane-local edges held in registers (GPU).

The fixed min-sum kernel runs on relabelled checks (normalised shifts) and keeps the message of
every register edge (gen/fixed_codes.hpp RE_ROW_REG / RE_COL_REG) in a VGPR instead of an LDS
slot (flood_fixed.hpp reg_edges(), msg[]).  The table-driven kernel and the oracle know nothing of
either, so all three must agree exactly: on noisy frames at -3 dB, on a three-level magnitude grid that
ties at the minimum in most rows, and on frames that put 0.0, +inf, -inf and NaN on variables of
columns that own a register edge, next to an ordinary frame of the same workgroup, so that the
exact (slow) check rows read and write msg[] and the sticky flag rises from a register v2c."""
import os

import numpy as np
import pytest
import torch

from conftest import PKG, code_path

from ldpc_neural_decoder.models import BeliefPropagationDecoder, MinSumScaledDecoder
from ldpc_neural_decoder.utils import expand_base_matrix, load_base_matrix
from reg_edges_util import parse_header

pytestmark = pytest.mark.gpu
ALPHA = 0.75
BATCHES = {32: (1, 2, 3, 5), 4: (1, 16, 17)}  # a lone frame, full lane vectors, tail workgroups
ITERS = (1, 2, 3, 10)
CASES = [(z, it) for z in (32, 4) for it in ITERS]
ES_MODES = {"frame": 2, True: 1}  # decoder argument -> the oracle's stopping mode


@pytest.fixture(scope="module")
def tables():
    with open(os.path.join(PKG, "csrc", "gen", "fixed_codes.hpp")) as f:
        t = parse_header(f.read())
    return {4: t["BG2_Z4"], 32: t["BG2_Z32"]}


def gauss(z, n):
    """Gaussian LLRs at -3 dB: frames fail, decisions stay sensitive."""
    rng = np.random.default_rng(100 + z)
    return (rng.normal(1.0, 1.0, size=(n, 52 * z)) * (2 * 10 ** (-3.0 / 10))).astype(np.float32)


def grid(z, n):
    """Magnitudes from {0.5, 1.0, 1.5}, random signs, no zeros: most rows of iteration 1 tie at the
    minimum and the fast path is certainly active."""
    rng = np.random.default_rng(200 + z)
    mag = rng.choice(np.array([0.5, 1.0, 1.5], np.float32), size=(n, 52 * z))
    return (mag * rng.choice(np.array([-1.0, 1.0], np.float32), size=(n, 52 * z))).astype(np.float32)


@pytest.fixture(scope="module")
def codes(oracle_mod):
    """Per lifting size: H, the oracle's graph, and max(B) frames of each kind (read-only)."""
    out = {}
    for z in (32, 4):
        H = expand_base_matrix(load_base_matrix(code_path(z)), z)
        x = {"gauss": gauss(z, max(BATCHES[z])), "grid": grid(z, max(BATCHES[z]))}
        for a in x.values():
            a.setflags(write=False)
        out[z] = (H, oracle_mod.Graph(H.numpy()), x)
    return out


def _u8(t):
    return t.cpu().numpy().astype(np.uint8)


def pair(cls, H, iters, es, cuda, z):
    args = (H, iters, ALPHA) if cls is MinSumScaledDecoder else (H, iters)
    d_fix, d_tab = cls(*args, early_stopping=es), cls(*args, early_stopping=es)
    assert d_fix.graph(cuda).set_variant(0) == (2 if z == 32 else 1)  # the compile-time schedule
    assert d_tab.graph(cuda).set_variant(1) == 0                      # table-driven
    return d_fix, d_tab


@pytest.mark.parametrize("kind", ["gauss", "grid"])
@pytest.mark.parametrize("z,iters", CASES)
def test_minsum_stop_off(cuda, oracle_mod, codes, z, iters, kind):
    H, g, x = codes[z]
    d_fix, d_tab = pair(MinSumScaledDecoder, H, iters, False, cuda, z)
    for B in BATCHES[z]:
        llr = torch.tensor(x[kind][:B]).to(cuda)
        b_fix, i_fix = d_fix.decode(llr)
        b_tab, _ = d_tab.decode(llr)
        ref, _, _, _ = oracle_mod.flood_decode(g, x[kind][:B], "minsum", iters, ALPHA, 0)
        assert i_fix == iters and torch.equal(b_fix, b_tab), (z, B, iters)
        assert np.array_equal(_u8(b_fix), ref), (z, B, iters)


@pytest.mark.parametrize("es", ["frame", True])
@pytest.mark.parametrize("kind", ["gauss", "grid"])
@pytest.mark.parametrize("z,iters", CASES)
def test_minsum_early_stop(cuda, oracle_mod, codes, z, iters, kind, es):
    H, g, x = codes[z]
    dec = MinSumScaledDecoder(H, iters, ALPHA, early_stopping=es)
    assert dec.graph(cuda).set_variant(0) == (2 if z == 32 else 1)
    for B in BATCHES[z]:
        bits, it, fi = dec.decode(torch.tensor(x[kind][:B]).to(cuda), return_frame_iters=True)
        ref, _, rn, ri = oracle_mod.flood_decode(g, x[kind][:B], "minsum", iters, ALPHA, ES_MODES[es])
        assert np.array_equal(_u8(bits), ref), (z, B, iters)
        if es == "frame":
            assert np.array_equal(fi.cpu().numpy(), ri) and it == ri.max(), (z, B, iters)
        else:
            assert it == rn, (z, B, iters)


@pytest.mark.parametrize("kind", ["gauss", "grid"])
@pytest.mark.parametrize("z,iters", CASES)
def test_bp_equals_table_driven(cuda, codes, z, iters, kind):
    H, _, x = codes[z]
    d_fix, d_tab = pair(BeliefPropagationDecoder, H, iters, False, cuda, z)
    for B in BATCHES[z]:
        llr = torch.tensor(x[kind][:B]).to(cuda)
        b1, i1 = d_fix.decode(llr)
        b2, i2 = d_tab.decode(llr)
        assert i1 == i2 and torch.equal(b1, b2), (z, B, iters)


def reg_columns(t):
    """columns that own a register edge, from the generated list"""
    return sorted({t["BLK_COL"][e] for e, x in enumerate(t["RE_ROW_REG"]) if x >= 0})


def special_batches(t, z, oracle_mod, g):
    """Batches on the tie grid whose frame 1 (frame 0 of the same workgroup stays ordinary) holds
    specials on variables of register-edge columns:
      zeros / pinf / ninf / nan   that value on one variable of every such column (zeros: on every
                  variable of them), so the first check phase already runs the exact rows on msg[]
      row   +inf and -inf on the two variables that one check of a row with a register edge joins
            through that edge and through the row's next slot edge
      late  a variable t of a register-edge column gets +inf from one check and -inf from another
            (every other variable of those two checks is infinite), so its v2c on the register edge
            is NaN after the first variable phase: the flag rises from msg[], and the second check
            phase reads a NaN from it (the oracle's APP confirms the NaN)"""
    n = max(BATCHES[z])
    cols = reg_columns(t)
    assert cols
    out = {}
    for kind, val in (("zeros", 0.0), ("pinf", np.inf), ("ninf", -np.inf), ("nan", np.nan)):
        x = grid(z, n)
        for i, c in enumerate(cols):
            if kind == "zeros":
                x[1, c * z:(c + 1) * z] = val
            else:
                x[1, c * z + (3 * i + 1) % z] = val
        out[kind] = x
    dv = np.diff(t["COL_PTR"])
    row_edges = lambda r: range(t["ROW_PTR"][r], t["ROW_PTR"][r + 1])
    var_of = lambda e, k: t["BLK_COL"][e] * z + (k + t["ROW_SHIFT"][e]) % z  # check k of e's row
    e = next(e for e, x in enumerate(t["RE_ROW_REG"]) if x >= 0)
    q = next(q for q in row_edges(t["BLK_ROW"][e]) if q != e and dv[t["BLK_COL"][q]] >= 2)
    x = grid(z, n)
    x[1, var_of(e, 1)], x[1, var_of(q, 1)] = np.inf, -np.inf
    out["row"] = x
    for e in (e for e, x in enumerate(t["RE_ROW_REG"]) if x >= 0):
        c = t["BLK_COL"][e]
        others = [q for q in range(t["NBLOCKS"]) if t["BLK_COL"][q] == c and q != e]
        if len(others) < 2:
            continue
        x = grid(z, n)
        tpos = 2 % z
        for sign, q in zip((1.0, -1.0), others[:2]):
            k = (tpos - t["ROW_SHIFT"][q]) % z
            first = True
            for p in row_edges(t["BLK_ROW"][q]):
                if p != q:
                    x[1, var_of(p, k)] = np.inf * (sign if first else 1.0)
                    first = False
        _, app, _, _ = oracle_mod.flood_decode(g, x[1:2], "minsum", 2, ALPHA, 0)
        if np.isnan(app[0, c * z + tpos]):
            out["late"] = x
            break
    assert "late" in out
    return out


@pytest.fixture(scope="module")
def specials(oracle_mod, tables, codes):
    return {z: special_batches(tables[z], z, oracle_mod, codes[z][1]) for z in (32, 4)}


@pytest.mark.parametrize("kind", ["zeros", "pinf", "ninf", "nan", "row", "late"])
@pytest.mark.parametrize("z,iters", CASES)
def test_specials_on_register_columns(cuda, oracle_mod, codes, specials, z, iters, kind):
    H, g, _ = codes[z]
    x = specials[z][kind]
    d_fix, d_tab = pair(MinSumScaledDecoder, H, iters, False, cuda, z)
    llr = torch.from_numpy(x).to(cuda)
    b_fix, _ = d_fix.decode(llr)
    b_tab, _ = d_tab.decode(llr)
    ref, _, _, _ = oracle_mod.flood_decode(g, x, "minsum", iters, ALPHA, 0)
    assert torch.equal(b_fix, b_tab)
    assert np.array_equal(_u8(b_fix), ref)


@pytest.mark.parametrize("es", ["frame", True])
@pytest.mark.parametrize("kind", ["zeros", "nan", "late"])
def test_specials_early_stop(cuda, oracle_mod, codes, specials, kind, es):
    """The early-stop instances are kernels of their own: the same frames, iteration counts too."""
    H, g, _ = codes[32]
    x = specials[32][kind]
    dec = MinSumScaledDecoder(H, 6, ALPHA, early_stopping=es)
    bits, it, fi = dec.decode(torch.from_numpy(x).to(cuda), return_frame_iters=True)
    ref, _, rn, ri = oracle_mod.flood_decode(g, x, "minsum", 6, ALPHA, ES_MODES[es])
    assert np.array_equal(_u8(bits), ref)
    if es == "frame":
        assert np.array_equal(fi.cpu().numpy(), ri) and it == ri.max()
    else:
        assert it == rn
