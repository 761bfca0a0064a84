"""tanh_half / two_atanh of the sum-product kernels (csrc/flood_dev.hpp) on their own (GPU).

ldpc_bp_math_raw runs the two device functions that every BP check update calls, element by
element, built with the decoders' own flags.  Reference: numpy.tanh(x / 2) and 2 numpy.arctanh(x)
in float64.

Relative error bar 3e-7 wherever the float64 result, rounded to float32, is a normal number other
than +-1 and +-inf: twice the 1.5e-7 that the header states for exact exp2 / log2 / rcp, the slack
being the three hardware instructions of 1 ulp each in the large-argument forms (a float32 model
with exact intrinsics has a worst case of 1.55 ulp for tanh_half).  The saturation behaviour that
the reference's arithmetic relies on is exact: |tanh| <= 1 always (a value above 1 would make the
product's atanh NaN), tanh(+-inf) = +-1, 2 atanh(+-1) = +-inf, NaN through, odd symmetry bitwise.
"""
import numpy as np
import pytest
import torch

from ldpc_neural_decoder import _native as N

pytestmark = pytest.mark.gpu
BAR = 3e-7


def all_floats(lo, hi):
    """every float32 in [lo, hi], 0 < lo < hi"""
    a, b = np.float32(lo).view(np.uint32), np.float32(hi).view(np.uint32)
    return np.arange(a, b + 1, dtype=np.uint32).view(np.float32)


def per_exponent(rng, e_lo, e_hi, n=4096):
    """n random mantissas for every binary exponent e_lo .. e_hi, both signs"""
    m = 1.0 + rng.integers(0, 1 << 23, size=(e_hi - e_lo + 1, n)) / float(1 << 23)
    x = np.ldexp(m, np.arange(e_lo, e_hi + 1)[:, None]).astype(np.float32).ravel()
    return np.concatenate([x, -x])


def device_eval(cuda, x):
    xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(cuda)
    th, at = torch.empty_like(xt), torch.empty_like(xt)
    N.check(N.lib().ldpc_bp_math_raw(N.ptr(xt), xt.numel(), N.ptr(th), N.ptr(at), N.stream_ptr(cuda)))
    torch.cuda.synchronize()
    return th.cpu().numpy(), at.cpu().numpy()


def errors(got, ref64):
    """(max relative error, max error in float32 ulp of the reference, argmax) over the entries
    whose reference rounds to a normal float32 other than +-1 / +-inf"""
    with np.errstate(over="ignore"):
        r32 = ref64.astype(np.float32)
    ok = np.isfinite(r32) & (np.abs(r32) >= np.finfo(np.float32).tiny) & (np.abs(r32) != 1.0)
    g, r = got[ok].astype(np.float64), ref64[ok]
    assert np.isfinite(g).all()
    rel = np.abs(g - r) / np.abs(r)
    ulp = np.abs(g - r) / np.spacing(np.abs(r32[ok])).astype(np.float64)
    k = int(np.argmax(rel))
    return float(rel.max()), float(ulp.max()), np.flatnonzero(ok)[k]


@pytest.fixture(scope="module")
def tanh_inputs():
    rng = np.random.default_rng(20)
    return np.concatenate([per_exponent(rng, -30, 5),   # up to |v| < 64
                           all_floats(1.2, 1.3),        # the branch switch |v / 2| = 0.625
                           all_floats(17.0, 19.0)])     # where tanh rounds to 1


@pytest.fixture(scope="module")
def atanh_inputs():
    rng = np.random.default_rng(21)
    k = np.arange(1, 25)
    edge = (1.0 - np.ldexp(1.0, -k)).astype(np.float32)
    return np.concatenate([per_exponent(rng, -30, -1),  # |x| < 1
                           all_floats(0.45, 0.55),      # the branch switch |x| = 0.5
                           edge, -edge])


def test_tanh_half_relative_error(cuda, tanh_inputs):
    x = tanh_inputs
    got, _ = device_eval(cuda, x)
    rel, ulp, k = errors(got, np.tanh(x.astype(np.float64) / 2))
    small = np.abs(x) < 1.25
    rel_s, ulp_s, _ = errors(got[small], np.tanh(x[small].astype(np.float64) / 2))
    rel_b, ulp_b, _ = errors(got[~small], np.tanh(x[~small].astype(np.float64) / 2))
    print(f"tanh_half: {x.size} inputs, max rel {rel:.3e} ({ulp:.2f} ulp) at v = {x[k]!r}; "
          f"polynomial branch {rel_s:.3e} ({ulp_s:.2f} ulp), exp branch {rel_b:.3e} ({ulp_b:.2f} ulp)")
    assert rel <= BAR, (rel, float(x[k]))


def test_two_atanh_relative_error(cuda, atanh_inputs):
    x = atanh_inputs
    _, got = device_eval(cuda, x)
    ref = 2 * np.arctanh(x.astype(np.float64))
    rel, ulp, k = errors(got, ref)
    small = np.abs(x) < 0.5
    rel_s, ulp_s, _ = errors(got[small], ref[small])
    rel_b, ulp_b, _ = errors(got[~small], ref[~small])
    print(f"two_atanh: {x.size} inputs, max rel {rel:.3e} ({ulp:.2f} ulp) at x = {x[k]!r}; "
          f"polynomial branch {rel_s:.3e} ({ulp_s:.2f} ulp), log branch {rel_b:.3e} ({ulp_b:.2f} ulp)")
    assert rel <= BAR, (rel, float(x[k]))


def test_tanh_half_exact_demands(cuda, tanh_inputs):
    f = np.float32
    big = np.concatenate([all_floats(19.0, 19.001), np.linspace(19, 400, 4001).astype(f),
                          np.array([1e3, 1e10, 3e38, np.finfo(f).max, np.inf], f)])
    tiny = np.array([0.0, np.finfo(f).tiny, 1e-45, 1e-40], f)  # zero, the smallest normal, subnormals
    x = np.concatenate([tanh_inputs, big, tiny])
    x = np.concatenate([x, -x, np.array([np.nan, -np.nan], f)])
    got, _ = device_eval(cuda, x)
    n = x.size - 2
    assert np.isnan(got[n:]).all()                                   # NaN through
    x, got = x[:n], got[:n]
    assert not np.isnan(got).any()
    assert (np.abs(got) <= 1.0).all(), float(np.abs(got).max())      # never above 1
    h = n // 2
    assert np.array_equal(got[:h].view(np.uint32) ^ np.uint32(0x80000000), got[h:].view(np.uint32))  # odd, bitwise
    zero = x == 0
    assert zero.sum() == 2 and np.array_equal(got[zero].view(np.uint32), x[zero].view(np.uint32))  # +-0 -> +-0
    sat = np.abs(x) >= 19.0
    assert sat.sum() > 8000 and np.array_equal(got[sat], np.sign(x[sat]))  # +-1 from 19 on, +-inf included
    assert np.array_equal(got[np.isinf(x)], np.sign(x[np.isinf(x)]))
    nz = x != 0
    assert np.array_equal(np.signbit(got[nz]), np.signbit(x[nz]))


def test_two_atanh_exact_demands(cuda, atanh_inputs):
    f = np.float32
    x = np.concatenate([atanh_inputs, np.array([0.0, -0.0, 1.0, -1.0, np.nan, -np.nan], f)])
    _, got = device_eval(cuda, x)
    n = atanh_inputs.size
    assert got[n] == 0 and got[n + 1] == 0
    assert got[n + 2] == np.inf and got[n + 3] == -np.inf
    assert np.isnan(got[n + 4:]).all()
    g, xx = got[:n], x[:n]
    assert np.isfinite(g).all()
    assert (xx != 0).all() and np.array_equal(np.sign(g), np.sign(xx))  # the sign of x, never 0
