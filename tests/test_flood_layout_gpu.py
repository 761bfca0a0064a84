"""The fixed-schedule flooding kernel's alternating slot layout (GPU).

A slot of flood_fixed_kernel is variable-indexed after a variable phase (and after init) and
check-indexed after a check phase; both phases read rotated and store own-lane (flood_fixed.hpp,
"Slots").  A wrong rotation, or a store of a wave that overtakes a read of another lane of the same
wave, corrupts messages from the first iteration on, so the cases here are the smallest that show
it: both fixed codes, a lone frame / one full lane vector / tail workgroups, and 1, 2, 3 and 10
iterations (one iteration is init, one check phase and a decision-only variable phase) on noisy
frames (-3 dB) whose decisions move from iteration to iteration.  Everything is exact: min-sum
against the oracle, BP against the table-driven kernel."""
import numpy as np
import pytest
import torch

from conftest import code_path

from ldpc_neural_decoder.models import BeliefPropagationDecoder, MinSumScaledDecoder
from ldpc_neural_decoder.utils import expand_base_matrix, load_base_matrix

pytestmark = pytest.mark.gpu
BATCHES = {32: (1, 2, 3, 5), 4: (1, 16, 17)}
ITERS = (1, 2, 3, 10)
CASES = [(z, it) for z in (32, 4) for it in ITERS]


@pytest.fixture(scope="module")
def codes(oracle_mod):
    """Per lifting size: H, the oracle's graph and max(B) seeded frames at -3 dB (read-only)."""
    out = {}
    for z in (32, 4):
        H = expand_base_matrix(load_base_matrix(code_path(z)), z)
        rng = np.random.default_rng(1000 + z)
        llr = (rng.normal(1.0, 1.0, size=(max(BATCHES[z]), H.shape[1])) * (2 * 10 ** (-3.0 / 10))).astype(np.float32)
        llr.setflags(write=False)
        out[z] = (H, oracle_mod.Graph(H.numpy()), llr)
    return out


def _u8(t):
    return t.cpu().numpy().astype(np.uint8)


@pytest.mark.parametrize("z,iters", CASES)
def test_minsum_stop_off_equals_oracle(cuda, oracle_mod, codes, z, iters):
    H, g, llr = codes[z]
    dec = MinSumScaledDecoder(H, max_iterations=iters, scaling_factor=0.75, early_stopping=False)
    assert dec.graph(cuda).set_variant(0) == (2 if z == 32 else 1)  # the fixed-schedule kernel runs
    for B in BATCHES[z]:
        bits, it = dec.decode(torch.tensor(llr[:B]).to(cuda))
        ref, _, _, _ = oracle_mod.flood_decode(g, llr[:B], "minsum", iters, 0.75, 0)
        assert it == iters and np.array_equal(_u8(bits), ref), (z, B, iters)


@pytest.mark.parametrize("z,iters", CASES)
def test_minsum_frame_stop_equals_oracle(cuda, oracle_mod, codes, z, iters):
    H, g, llr = codes[z]
    dec = MinSumScaledDecoder(H, max_iterations=iters, scaling_factor=0.75, early_stopping="frame")
    for B in BATCHES[z]:
        bits, _, fi = dec.decode(torch.tensor(llr[:B]).to(cuda), return_frame_iters=True)
        ref, _, _, ri = oracle_mod.flood_decode(g, llr[:B], "minsum", iters, 0.75, 2)
        assert np.array_equal(_u8(bits), ref), (z, B, iters)
        assert np.array_equal(fi.cpu().numpy(), ri), (z, B, iters)


@pytest.mark.parametrize("z,iters", CASES)
def test_bp_equals_table_driven_kernel(cuda, codes, z, iters):
    H, _, llr = codes[z]
    d_fix = BeliefPropagationDecoder(H, max_iterations=iters, early_stopping=False)
    d_tab = BeliefPropagationDecoder(H, max_iterations=iters, early_stopping=False)
    assert d_fix.graph(cuda).set_variant(0) == (2 if z == 32 else 1)
    assert d_tab.graph(cuda).set_variant(1) == 0
    for B in BATCHES[z]:
        x = torch.tensor(llr[:B]).to(cuda)
        b1, i1 = d_fix.decode(x)
        b2, i2 = d_tab.decode(x)
        assert i1 == i2 and torch.equal(b1, b2), (z, B, iters)


def test_special_values_z32(cuda, oracle_mod, codes):
    """The frames of test_special_values (a run of zero LLRs, +inf, -inf, NaN) at Z=32: the exact
    (slow) check rows and the workgroup's sticky flag on the alternating layout."""
    H, g, _ = codes[32]
    rng = np.random.default_rng(3)
    llr = rng.normal(0.5, 1.0, size=(4, H.shape[1])).astype(np.float32)
    llr[0, :40] = 0.0
    llr[1, 5] = np.inf
    llr[2, 9] = -np.inf
    llr[3, 11] = np.nan
    dec = MinSumScaledDecoder(H, max_iterations=4, early_stopping=False)
    bits, _ = dec.decode(torch.from_numpy(llr).to(cuda))
    ref, _, _, _ = oracle_mod.flood_decode(g, llr, "minsum", 4, 0.75, 0)
    assert np.array_equal(_u8(bits), ref)
