"""Fixed flood kernel, min-sum: the direct check update of rows of degree <= 5 (GPU).

The fixed kernel's fast check path writes every output of a short row straight from the other
inputs (flood_fixed.hpp direct_row); the table-driven kernel keeps the two-minimum / select form and
the oracle restates the reference.  All three must give the same decisions, exactly, on inputs
that keep decisions sensitive (low SNR), that tie at the minimum in most rows (a three-level
magnitude grid), and that switch a workgroup to the slow path at the start (zeros, NaN) or in a
later iteration (infinities), with ordinary frames in the same workgroup."""
import numpy as np
import pytest
import torch

from conftest import code_path

from ldpc_neural_decoder.models import MinSumScaledDecoder
from ldpc_neural_decoder.utils import expand_base_matrix, load_base_matrix

pytestmark = pytest.mark.gpu
ALPHA = 0.75
SHAPES = {32: 3, 4: 17}  # Z -> B: a tail workgroup with one frame (2 and 16 frames per workgroup)
SPECIALS = ("zeros", "pinf", "ninf", "nan")


@pytest.fixture(scope="module")
def codes():
    return {z: expand_base_matrix(load_base_matrix(code_path(z)), z) for z in SHAPES}


def gauss(z):
    """(a) Gaussian LLRs at -3 dB: frames fail, decisions stay sensitive."""
    rng = np.random.default_rng(100 + z)
    return (rng.normal(1.0, 1.0, size=(SHAPES[z], 52 * z)) * (2 * 10 ** (-3.0 / 10))).astype(np.float32)


def grid(z):
    """(b) magnitudes from {0.5, 1.0, 1.5}, random signs, no zeros: most rows of iteration 1 tie at
    the minimum and the fast path is certainly active."""
    rng = np.random.default_rng(200 + z)
    shape = (SHAPES[z], 52 * z)
    mag = rng.choice(np.array([0.5, 1.0, 1.5], np.float32), size=shape)
    return (mag * rng.choice(np.array([-1.0, 1.0], np.float32), size=shape)).astype(np.float32)


def make_special(x, frame, kind):
    if kind == "zeros":
        x[frame, :40] = 0.0
    elif kind == "pinf":
        x[frame, 5] = np.inf
    elif kind == "ninf":
        x[frame, 9] = -np.inf
    else:
        x[frame, 11] = np.nan


def special(z):
    """(c) the grid with special frames next to ordinary ones in one workgroup.  Z = 32 (frames 2j
    and 2j + 1 share a workgroup): one batch per kind with frame 1 special.  Z = 4 (16 frames per
    workgroup): frames 1, 5, 9 and 13 of one batch."""
    if z == 32:
        out = []
        for kind in SPECIALS:
            x = grid(z)
            make_special(x, 1, kind)
            out.append(x)
        return out
    x = grid(z)
    for i, kind in enumerate(SPECIALS):
        make_special(x, 1 + 4 * i, kind)
    return [x]


@pytest.fixture(scope="module")
def inputs():
    return {(kind, z): make(z) for z in SHAPES
            for kind, make in (("gauss", lambda z: [gauss(z)]), ("grid", lambda z: [grid(z)]), ("special", special))}


def decoders(H, iters, es, cuda):
    d_fix = MinSumScaledDecoder(H, iters, ALPHA, early_stopping=es)
    d_tab = MinSumScaledDecoder(H, iters, ALPHA, early_stopping=es)
    assert d_fix.graph(cuda).set_variant(0) in (1, 2)  # the compile-time schedule
    assert d_tab.graph(cuda).set_variant(1) == 0       # table-driven
    return d_fix, d_tab


@pytest.mark.parametrize("iters", [1, 2, 3, 10])
@pytest.mark.parametrize("kind", ["gauss", "grid", "special"])
@pytest.mark.parametrize("z", [32, 4])
def test_decisions_equal_table_driven_and_oracle(cuda, oracle_mod, codes, inputs, z, kind, iters):
    H = codes[z]
    g = oracle_mod.Graph(H.numpy())
    d_fix, d_tab = decoders(H, iters, False, cuda)
    for x in inputs[(kind, z)]:
        llr = torch.from_numpy(x).to(cuda)
        b_fix, i_fix = d_fix.decode(llr)
        b_tab, i_tab = d_tab.decode(llr)
        ref, _, _, _ = oracle_mod.flood_decode(g, x, "minsum", iters, ALPHA, 0)
        got = b_fix.cpu().numpy().astype(np.uint8)
        assert i_fix == iters and i_tab == iters
        assert torch.equal(b_fix, b_tab)
        assert np.array_equal(got, ref)


@pytest.mark.parametrize("kind", ["gauss", "grid"])
@pytest.mark.parametrize("es", [True, "frame"])
def test_early_stop_equal_table_driven(cuda, codes, inputs, es, kind):
    """Early-stop modes take decisions in every iteration, so the degree-1 edges' outputs go
    through the direct form too."""
    d_fix, d_tab = decoders(codes[32], 6, es, cuda)
    llr = torch.from_numpy(inputs[(kind, 32)][0]).to(cuda)
    b1, i1, f1 = d_fix.decode(llr, return_frame_iters=True)
    b2, i2, f2 = d_tab.decode(llr, return_frame_iters=True)
    assert torch.equal(b1, b2) and i1 == i2 and torch.equal(f1, f2)


@pytest.mark.parametrize("z", [32, 4])
def test_counters_on_tie_grid(cuda, codes, inputs, z):
    llr = torch.from_numpy(inputs[("grid", z)][0]).to(cuda)
    dec = MinSumScaledDecoder(codes[z], max_iterations=10, scaling_factor=ALPHA, early_stopping=False)
    cnt = torch.zeros(4, dtype=torch.int64, device=cuda)
    b8, _ = dec.decode(llr, out_dtype=torch.uint8, counters=cnt)
    bf, _ = dec.decode(llr)
    assert b8.dtype == torch.uint8 and torch.equal(b8.float(), bf)
    be = int(bf.sum().item())
    fe = int((bf.sum(1) > 0).sum().item())
    assert cnt.tolist() == [be, fe, llr.shape[0], 10 * llr.shape[0]]
