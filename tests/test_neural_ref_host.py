"""Host checks of the fused neural min-sum decoder's definition and layout (no device is touched).

tests/neural_ref.py restates ldpc_neural_forward's definition in numpy float32.  Here it is held to the
oracle's composition of the reference's layers (oracle.neural_decoder, torch on the CPU) on the
pre-sigmoid sum app, within 1e-5 abs / 1e-5 rel -- the bar tests/test_harness_gpu.py states for this
decoder; torch reduces in another order than the definition's, so equality is not expected.  The GPU
tests (tests/test_neural_fused_gpu.py) then hold the kernel to neural_ref.py bit for bit.

The LLRs are N(0, 0.5^2).  Both sides are float32 evaluations of one real function, and the recursion
is positively homogeneous in the LLRs, so either side's rounding error grows with the LLR scale while
the bar's absolute part does not.  At the harness test's scale (sigma = 3) the oracle's own float32 app
is up to 2.3e-5 from the oracle evaluated in float64 after 4 iterations on BG2 Z = 4 -- past the bar by
itself -- so no float32 restatement can be resolved against it there.  Each case therefore first asserts,
from the oracle alone, that its float32 app is within HALF the bar of its float64 app (measured: at most
0.26 of the bar at sigma = 0.5 over 8 seeds of every case); the other half is what neural_ref.py may use.

ldpc_neural_layout is the host-only query the decode entry shares: its validation, its two
LDPC_EUNSUPPORTED answers and its bounds on the reference's two codes."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import code_path

from neural_ref import groups_from_H, neural_ref

from ldpc_neural_decoder import _native as N
from ldpc_neural_decoder.utils import create_LLR_mapping, expand_base_matrix, load_base_matrix

_P = ctypes.c_void_p
EXAMPLE_H = np.array([[1, 1, 0, 0], [0, 1, 1, 1], [1, 0, 0, 1]], dtype=np.float32)
LDS_MAX = 160 * 1024


def _H(which):
    if which == "example":
        return torch.from_numpy(EXAMPLE_H)
    return expand_base_matrix(load_base_matrix(code_path(which)), which)


def _oracle_app(oracle, params, llr, cidx, vidx, var_of, depth_L):
    """oracle.neural_decoder's composition, stopped at its pre-sigmoid sum."""
    x0 = llr[:, var_of]
    v, prevs, zero = x0, [], torch.zeros_like(x0)
    for w_ch, w_res in params:
        c = oracle.check_layer(v, cidx)
        v = oracle.residual_layer(x0, oracle.variable_layer(zero, c, vidx), prevs, w_ch, w_res)
        prevs = [v] + prevs[:max(depth_L - 1, 0)]
    c = oracle.check_layer(v, cidx)
    return torch.zeros((llr.shape[0], llr.shape[1]), dtype=llr.dtype).index_add(1, var_of, c)


CASES = [("example", 3, 2)] + [(4, it, d) for it in (1, 2, 4) for d in (0, 2, 3)]


@pytest.mark.parametrize("which,iters,depth", CASES)
def test_neural_ref_matches_oracle_composition(oracle_mod, which, iters, depth):
    H = _H(which)
    _, cidx, vidx, out_idx = create_LLR_mapping(H.T)
    var_of, E = out_idx[0], cidx.shape[0]
    cptr, cmem, vptr, K = groups_from_H(H.numpy())
    assert K == cidx.shape[1] and len(cmem) == E
    assert np.array_equal(np.repeat(np.arange(H.shape[1]), np.diff(vptr)), var_of.numpy())
    g = torch.Generator().manual_seed(1234)
    params = [(torch.rand(E, generator=g) + 0.5, torch.randn(depth, generator=g) * 0.3) for _ in range(iters - 1)]
    llr = torch.randn(5, H.shape[1], generator=g) * 0.5
    llr[0, :2] = 0.0                                   # exact zeros reach the check rule
    app_ref = _oracle_app(oracle_mod, params, llr, cidx, vidx, var_of, depth)
    # the precondition (module docstring): the oracle's own float32 error uses at most half the bar
    app64 = _oracle_app(oracle_mod, [(a.double(), b.double()) for a, b in params], llr.double(), cidx, vidx,
                        var_of, depth).numpy()
    own = np.abs(app_ref.numpy() - app64) / (1e-5 + 1e-5 * np.abs(app64))
    print(f"oracle float32 vs float64: {own.max():.3f} of the bar")
    assert own.max() <= 0.5
    # the stopped composition is the oracle's own: its sigmoid is oracle.neural_decoder's soft
    soft, _ = oracle_mod.neural_decoder(params, llr, cidx, vidx, var_of, depth)
    assert torch.equal(torch.sigmoid(-app_ref + -llr), soft)
    w_ch = np.stack([p[0].numpy() for p in params]) if params else None
    w_res = np.stack([p[1].numpy() for p in params]) if params else None
    app = neural_ref(llr.numpy(), cptr, cmem, vptr, K, iters, depth, w_ch, w_res)
    assert app.dtype == np.float32 and app.shape == tuple(llr.shape)
    err = np.abs(app - app_ref.numpy()) / (1e-5 + 1e-5 * np.abs(app_ref.numpy()))
    print(f"neural_ref vs oracle float32: {err.max():.3f} of the bar")
    np.testing.assert_allclose(app, app_ref.numpy(), atol=1e-5, rtol=1e-5)


def _layout_rc(cptr, cmem, vptr, K, depth, n=None, g=None, e=None):
    cp, cm, vp = (np.ascontiguousarray(a, dtype=np.int32) for a in (cptr, cmem, vptr))
    F, T, L = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int64(-1)
    rc = N.lib().ldpc_neural_layout(len(vp) - 1 if n is None else n, len(cp) - 1 if g is None else g,
                                    len(cm) if e is None else e, cp.ctypes.data_as(_P), cm.ctypes.data_as(_P),
                                    vp.ctypes.data_as(_P), K, depth, ctypes.byref(F), ctypes.byref(T), ctypes.byref(L))
    return rc, F.value, T.value, L.value


def _chain(E, dc=4):
    """E degree-1 variables on checks of degree dc (the last one shorter): a valid description of any size."""
    cptr = np.concatenate([np.arange(0, E, dc), [E]])
    return cptr, np.arange(E), np.arange(E + 1), dc - 1


def test_layout_rejects_bad_descriptions():
    cptr, cmem, vptr, K = groups_from_H(EXAMPLE_H)
    assert _layout_rc(cptr, cmem, vptr, K, 2)[0] == 0
    dup = cmem.copy()
    dup[1] = dup[0]                                    # not a permutation
    assert _layout_rc(cptr, dup, vptr, K, 2)[0] == N.LDPC_EINVAL
    far = cmem.copy()
    far[0] = len(cmem)                                 # out of range
    assert _layout_rc(cptr, far, vptr, K, 2)[0] == N.LDPC_EINVAL
    short = vptr.copy()
    short[-1] -= 1                                     # does not reach E
    assert _layout_rc(cptr, cmem, short, K, 2)[0] == N.LDPC_EINVAL
    back = vptr.copy()
    back[1], back[2] = back[2], back[1] - 1            # not monotone
    assert _layout_rc(cptr, cmem, back, K, 2)[0] == N.LDPC_EINVAL
    late = cptr.copy()
    late[0] = 1                                        # does not start at 0
    assert _layout_rc(late, cmem, vptr, K, 2)[0] == N.LDPC_EINVAL
    assert _layout_rc(cptr, cmem, vptr, K, -1)[0] == N.LDPC_EINVAL
    assert _layout_rc(*_chain(65536), 0)[0] == N.LDPC_EINVAL     # E must stay below 65536
    assert b"65536" in N.lib().ldpc_last_error()


def test_layout_unsupported_answers():
    cptr, cmem, vptr, K = groups_from_H(EXAMPLE_H)
    assert _layout_rc(cptr, cmem, vptr, K, 8)[0] == 0
    assert _layout_rc(cptr, cmem, vptr, K, 9)[0] == N.LDPC_EUNSUPPORTED
    assert N.neural_layout(cptr, cmem, vptr, K, 9) is None
    # one frame = N + (1 + max(depth_L, 1)) E floats beside ~2 (2 E + G + N) bytes of tables: with
    # N = E = 12000 and depth_L = 2 that is 192 KB of floats alone
    big = _chain(12000)
    assert _layout_rc(*big, 2)[0] == N.LDPC_EUNSUPPORTED
    # the same E fits with fewer rows when the LLR row is short: the answer depends on depth_L
    small = _chain(4000)
    assert _layout_rc(*small, 2)[0] == 0
    assert _layout_rc(*small, 8)[0] == N.LDPC_EUNSUPPORTED


@pytest.mark.parametrize("z", [4, 32])
@pytest.mark.parametrize("depth", [0, 2, 8])
def test_layout_bounds_on_the_reference_codes(z, depth):
    H = _H(z).numpy()
    cptr, cmem, vptr, K = groups_from_H(H)
    E, G, Nv = len(cmem), len(cptr) - 1, len(vptr) - 1
    got = N.neural_layout(cptr, cmem, vptr, K, depth)
    frame = (-(-Nv // 4) * 4 + (1 + max(depth, 1)) * (-(-E // 4) * 4)) * 4
    if got is None:                                    # only a frame that cannot fit may be refused
        assert frame + 2 * (2 * E + G + Nv) > LDS_MAX
        assert (z, depth) == (32, 8)
        return
    F, T, lds = got
    assert F >= 1 and 64 <= T <= 1024 and T % 64 == 0
    assert F * frame + 2 * (2 * E + G + 1 + Nv + 1) <= lds <= LDS_MAX
    # as many frames as fit, up to the kernel's cap of 8
    assert F == 8 or lds + frame > LDS_MAX
    if (z, depth) == (32, 2):
        assert F == 1
