"""Fixed flood kernel, min-sum: instances that read the joint schedule (GPU).

The joint schedule (gen/fixed_codes.hpp RE_J_*, flood_fixed.hpp joint_family) puts rows and columns
on other waves than the committed one, with another rho per row, other register and rotated edges
and other column pairs.  Checks are anonymous and everything that crosses kernels is per variable,
so nothing outside the kernel may see which family an instance reads: the table-driven kernel and
the oracle know nothing of either, and all three must agree exactly -- decisions in both output
types, per-frame iteration counts and the fused counters -- without early stop, with the per-frame
stop and with the batch stop, on batches whose last workgroup has lanes without a frame (Z = 32:
B = 5, Z = 4: B = 37).  Every batch holds noisy frames at -3 dB, tie-grid frames (LLRs on k/4) and
frames with a run of zeros, +-inf and NaN on variables of columns that own an edge which is
same-wave only in the joint schedule, each next to ordinary frames of its workgroup: the bail-out /
redo path of the instances without the exact update, and the exact update inside the batch-stop
instances.  The redo list holds exactly the workgroups with a non-finite LLR."""
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
BATCH = {32: 5, 4: 37}
ITERS = (1, 2, 10)
ES_MODES = {False: 0, True: 1, "frame": 2}  # decoder argument -> the oracle's stopping mode
# frame -> kind; the other frames alternate noisy / tie grid.  Z = 32: two frames per workgroup,
# the NaN frame alone in the last one; Z = 4: sixteen per workgroup, five in the last one.
SPECIAL = {32: {1: "zeros", 3: "inf", 4: "nan"}, 4: {1: "zeros", 17: "inf", 33: "nan"}}


def new_same_wave_columns(t):
    """columns with an edge kept in a VGPR by the joint schedule and in an LDS slot by the other"""
    return sorted({t["BLK_COL"][e] for e in range(t["NBLOCKS"])
                   if (t["RE_J_ROW_REG"][e] >= 0 or t["RE_J_ROW_ROT"][e] >= 0)
                   and t["RE_ROW_REG"][e] < 0 and t["RE_ROW_ROT"][e] < 0})


def make_batch(t, z):
    n = BATCH[z]
    rng = np.random.default_rng(1800 + z)
    x = (rng.normal(1.0, 1.0, size=(n, 52 * z)) * (2 * 10 ** (-3.0 / 10))).astype(np.float32)
    # tie grid: LLRs on k/4, no zeros, so most rows of the first iterations tie at the minimum
    mag = rng.integers(1, 9, size=(n, 52 * z)).astype(np.float32) / 4
    tie = mag * rng.choice(np.array([-1.0, 1.0], np.float32), size=(n, 52 * z))
    x[0::2] = tie[0::2]
    cols = new_same_wave_columns(t)
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


@pytest.mark.parametrize("es", ["off", "frame"])
@pytest.mark.parametrize("z", [32, 4])
def test_redo_list_holds_the_workgroups_with_a_non_finite_llr(cuda, codes, reference, z, es):
    """The instances without the exact update (stopping off or per frame, with a workspace) leave
    the decode for exactly the workgroups whose frames hold +-inf or NaN -- the flag is raised in
    init, whatever the schedule -- and zeros stay on the fast update."""
    H, _, x = codes[z]
    B, iters = BATCH[z], 10
    mode = {"off": (N.LDPC_ES_OFF, False), "frame": (N.LDPC_ES_FRAME, "frame")}[es]
    g = MinSumScaledDecoder(H, iters, ALPHA, early_stopping=False).graph(cuda)
    assert g.set_variant(0) == (2 if z == 32 else 1)
    llr = torch.from_numpy(np.array(x)).to(cuda)
    bits = torch.empty((B, g.N), dtype=torch.uint8, device=cuda)
    fi = torch.empty(B, dtype=torch.int32, device=cuda)
    bi = torch.zeros(1, dtype=torch.int32, device=cuda)
    cnt = torch.zeros(4, dtype=torch.int64, device=cuda)
    wsb = N.check(N.lib().ldpc_flood_workspace_size(g.handle, B, iters, mode[0]))
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=cuda)
    s = N.stream_ptr(cuda)
    N.check(N.lib().ldpc_flood_decode(g.handle, N.LDPC_ALGO_MINSUM, N.ptr(llr), B, iters, ALPHA, mode[0], N.LDPC_OUT_U8,
                                      N.ptr(bits), N.ptr(fi), N.ptr(bi), N.ptr(cnt), N.ptr(ws), wsb, s))
    n = ctypes.c_int32(-1)
    buf = (ctypes.c_int32 * (B + 1))()
    N.check(N.lib().ldpc_flood_redo_count(g.handle, N.LDPC_ALGO_MINSUM, B, iters, mode[0], N.ptr(ws), s,
                                          ctypes.byref(n), buf))
    torch.cuda.synchronize()
    fg = 64 // z
    want = sorted({fr // fg for fr, kind in SPECIAL[z].items() if kind != "zeros"})
    assert sorted(buf[i] for i in range(n.value)) == want
    ref, _, _, ri = reference[(z, iters, mode[1])]
    assert np.array_equal(bits.cpu().numpy(), ref) and np.array_equal(fi.cpu().numpy(), ri)
