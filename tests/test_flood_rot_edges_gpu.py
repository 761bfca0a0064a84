"""Fixed flood kernel, min-sum: rotated edges kept in registers by a cross-lane rotation (GPU).

A rotated edge (gen/fixed_codes.hpp RE_ROW_ROT / RE_COL_ROT) has its row and its column on one wave
and a normalised shift s != 0: the kernel moves its message to the lane that reads it next with
one ds_swizzle_b32 (flood_fixed.hpp rmsg[], seg_rotate) and never touches its LDS slot.  The
table-driven kernel and the oracle know nothing of that, so all three must agree exactly: decisions
in both output types, per-frame iteration counts and the fused counters, without early stop, with
the per-frame stop and with the batch stop, on batches whose last workgroup has lanes without a
frame (Z = 32: B = 5, Z = 4: B = 37).  Every batch holds noisy frames at -3 dB, tie-grid frames
(LLRs on k/4) and frames with a run of zeros, +-inf and NaN on variables of columns that own a
rotated edge, each next to ordinary frames of its workgroup: the bail-out / redo path of the
instances without the exact update, and the exact update inside the batch-stop instances, both
carry rmsg[]."""
import os

import numpy as np
import pytest
import torch

from conftest import PKG, code_path

from ldpc_neural_decoder.models import MinSumScaledDecoder
from ldpc_neural_decoder.utils import expand_base_matrix, load_base_matrix
from reg_edges_util import parse_header

pytestmark = pytest.mark.gpu
ALPHA = 0.75
BATCH = {32: 5, 4: 37}
ITERS = (1, 2, 10)
ES_MODES = {False: 0, True: 1, "frame": 2}  # decoder argument -> the oracle's stopping mode
# frame -> kind; the other frames alternate noisy / tie grid.  Z = 32: two frames per workgroup,
# the NaN frame alone in the last one; Z = 4: sixteen per workgroup, five in the last one.
SPECIAL = {32: {1: "zeros", 3: "inf", 4: "nan"}, 4: {1: "zeros", 17: "inf", 33: "nan"}}


def rot_columns(t):
    return sorted({t["BLK_COL"][e] for e, x in enumerate(t["RE_ROW_ROT"]) if x >= 0})


def make_batch(t, z):
    n = BATCH[z]
    rng = np.random.default_rng(300 + z)
    x = (rng.normal(1.0, 1.0, size=(n, 52 * z)) * (2 * 10 ** (-3.0 / 10))).astype(np.float32)
    # tie grid: LLRs on k/4, no zeros, so most rows of the first iterations tie at the minimum
    mag = rng.integers(1, 9, size=(n, 52 * z)).astype(np.float32) / 4
    tie = mag * rng.choice(np.array([-1.0, 1.0], np.float32), size=(n, 52 * z))
    x[0::2] = tie[0::2]
    cols = rot_columns(t)
    assert cols
    for fr, kind in SPECIAL[z].items():
        x[fr] = tie[fr]
        for i, c in enumerate(cols):
            k = (3 * i + 1) % z
            if kind == "zeros":  # a run over the column's first half (all of it at Z = 4)
                x[fr, c * z:c * z + max(z // 2, 4)] = 0.0
            elif kind == "inf":
                x[fr, c * z + k] = np.inf if i % 2 == 0 else -np.inf
            elif i % 3 == 0:
                x[fr, c * z + k] = np.nan
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def codes(oracle_mod):
    """Per lifting size: H, the oracle's graph and the batch (read-only)."""
    with open(os.path.join(PKG, "csrc", "gen", "fixed_codes.hpp")) as f:
        t = parse_header(f.read())
    out = {}
    for z in (32, 4):
        H = expand_base_matrix(load_base_matrix(code_path(z)), z)
        out[z] = (H, oracle_mod.Graph(H.numpy()), make_batch(t[f"BG2_Z{z}"], z))
    return out


@pytest.fixture(scope="module")
def reference(oracle_mod, codes):
    """The oracle's decode of every case, computed once."""
    return {(z, it, es): oracle_mod.flood_decode(codes[z][1], codes[z][2], "minsum", it, ALPHA, mode)
            for z in (32, 4) for it in ITERS for es, mode in ES_MODES.items()}


def test_batches_hold_what_they_claim(codes):
    for z in (32, 4):
        x = codes[z][2]
        kinds = SPECIAL[z]
        assert x.shape[0] == BATCH[z] and BATCH[z] % (64 // z) != 0  # lanes without a frame
        for fr, kind in kinds.items():
            row = x[fr]
            assert {"zeros": (row == 0).sum() >= 4, "inf": np.isposinf(row).any() and np.isneginf(row).any(),
                    "nan": np.isnan(row).any()}[kind]
        plain = [i for i in range(BATCH[z]) if i not in kinds]
        assert np.isfinite(x[plain]).all() and (x[plain] != 0).all()


def run(dec, llr, dtype, cuda):
    cnt = torch.zeros(4, dtype=torch.int64, device=cuda)
    bits, it, fi = dec.decode(llr, out_dtype=dtype, counters=cnt, return_frame_iters=True)
    assert bits.dtype == dtype
    return bits.cpu().numpy().astype(np.uint8), it, fi.cpu().numpy(), cnt.tolist()


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("es", [False, "frame", True], ids=["off", "frame", "batch"])
@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("z", [32, 4])
def test_equals_oracle_and_table_driven(cuda, codes, reference, z, iters, es, dtype):
    H, _, x = codes[z]
    B = BATCH[z]
    d_fix = MinSumScaledDecoder(H, iters, ALPHA, early_stopping=es)
    d_tab = MinSumScaledDecoder(H, iters, ALPHA, early_stopping=es)
    assert d_fix.graph(cuda).set_variant(0) == (2 if z == 32 else 1)  # the compile-time schedule
    assert d_tab.graph(cuda).set_variant(1) == 0                      # table-driven
    llr = torch.tensor(x).to(cuda)
    b_fix, i_fix, f_fix, c_fix = run(d_fix, llr, dtype, cuda)
    b_tab, i_tab, f_tab, c_tab = run(d_tab, llr, dtype, cuda)
    ref, _, rn, ri = reference[(z, iters, es)]
    assert np.array_equal(b_fix, ref) and np.array_equal(b_tab, ref)
    assert i_fix == i_tab and np.array_equal(f_fix, f_tab) and c_fix == c_tab
    assert c_fix[:3] == [int(ref.sum()), int(ref.any(1).sum()), B]
    if es == "frame":
        assert np.array_equal(f_fix, ri) and i_fix == int(ri.max()) and c_fix[3] == int(ri.sum())
    elif es:
        assert i_fix == rn and c_fix[3] == int(f_fix.sum())
    else:
        assert i_fix == iters and (f_fix == iters).all() and c_fix[3] == iters * B
