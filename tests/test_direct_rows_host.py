"""The fixed flood kernel's two fast-path forms of the min-sum check update, restated in numpy and
compared bit for bit (no GPU).

select form (rows of degree > LDPC_DIRECT_DC, and the parent of the direct form):
    m1, m2 = the two smallest magnitudes; par = xor of all sign bits
    c2v_e = ((alpha * (|x_e| == m1 ? m2 : m1)) ^ par) ^ sign(x_e)
direct form (flood_fixed.hpp direct_row):
    degree <= 4:  c2v_e = (alpha * min_{e' != e} |x_e'|) ^ (xor_{e' != e} sign(x_e'))
    degree >= 5:  pair minima shared by the row, the row's parity folded into alpha's sign:
                  c2v_e = ((alpha ^ par) * min(|partner|, other pairs / odd input)) ^ sign(x_e)
Rows hold no zero and no NaN, as the kernel's sticky flag guarantees on the fast path."""
import numpy as np
import pytest

SIGN = np.uint32(0x80000000)
ALPHA = np.float32(0.75)


def u(x):
    return x.view(np.uint32)


def f(x):
    return x.view(np.float32)


def select_form(v, alpha):
    a = np.abs(v)
    s = np.sort(a, axis=1)
    m1, m2 = s[:, :1], s[:, 1:2]
    par = np.bitwise_xor.reduce(u(v), axis=1, keepdims=True) & SIGN
    s1, s2 = u(alpha * m1) ^ par, u(alpha * m2) ^ par
    sel = np.where(a == m1, s2, s1)
    return f(sel ^ (u(v) & SIGN))


def direct_form(v, alpha):
    n, dc = v.shape
    a = np.abs(v)
    out = np.empty_like(v)
    if dc <= 4:
        for e in range(dc):
            others = [q for q in range(dc) if q != e]
            m = a[:, others[0]]
            xs = u(v[:, others[0]])
            for q in others[1:]:
                m = np.minimum(m, a[:, q])
                xs = xs ^ u(v[:, q])
            out[:, e] = f(u(alpha * m) ^ (xs & SIGN))
        return out
    pr = [np.minimum(a[:, 2 * j], a[:, 2 * j + 1]) for j in range(dc // 2)]
    par = np.bitwise_xor.reduce(u(v), axis=1)
    als = f(u(np.full(n, alpha, np.float32)) ^ (par & SIGN))
    for e in range(dc):
        if dc == 5 and e == 4:
            m = np.minimum(pr[0], pr[1])
        elif dc == 5:
            m = np.minimum(np.minimum(a[:, e ^ 1], pr[1 - e // 2]), a[:, 4])
        else:
            m = np.minimum(np.minimum(a[:, e ^ 1], pr[(e // 2 + 1) % 3]), pr[(e // 2 + 2) % 3])
        out[:, e] = f(u(als * m) ^ (u(v[:, e]) & SIGN))
    return out


def rows(kind, dc, n, rng):
    if kind == "gauss":
        v = rng.normal(0.5, 2.0, size=(n, dc)).astype(np.float32)
        v[v == 0] = np.float32(1.0)
        return v
    if kind == "wide":  # magnitudes from denormal to huge, infinities included
        v = (rng.choice(np.array([-1.0, 1.0], np.float32), size=(n, dc))
             * np.exp2(rng.integers(-149, 128, size=(n, dc)).astype(np.float64)).astype(np.float32))
        v[rng.random((n, dc)) < 0.02] = np.float32(np.inf)
        return v.astype(np.float32)
    mag = rng.choice(np.array([0.5, 1.0, 1.5], np.float32), size=(n, dc))
    return (mag * rng.choice(np.array([-1.0, 1.0], np.float32), size=(n, dc))).astype(np.float32)


@pytest.mark.parametrize("alpha", [ALPHA, np.float32(0.8), np.float32(-0.75)])
@pytest.mark.parametrize("kind", ["gauss", "grid", "wide"])
@pytest.mark.parametrize("dc", [2, 3, 4, 5, 6])
def test_direct_form_is_the_select_form_bit_for_bit(dc, kind, alpha):
    rng = np.random.default_rng(dc * 31 + len(kind))
    v = rows(kind, dc, 20000, rng)
    assert not np.isnan(v).any() and (v != 0).all()
    with np.errstate(over="ignore", under="ignore"):
        a, b = select_form(v, alpha), direct_form(v, alpha)
    assert np.array_equal(u(a), u(b)), int((u(a) != u(b)).sum())


def test_select_form_is_the_reference_update():
    """The select form itself against the reference's definition, sign product times alpha times
    the minimum over the other magnitudes (traditional_decoders.py:207-232), on tie-heavy rows."""
    rng = np.random.default_rng(7)
    for dc in (2, 3, 4, 5, 6):
        v = rows("grid", dc, 5000, rng)
        ref = np.empty_like(v)
        for e in range(dc):
            o = np.delete(v, e, axis=1)
            ref[:, e] = np.prod(np.sign(o), axis=1) * (ALPHA * np.abs(o).min(axis=1))
        assert np.array_equal(u(select_form(v, ALPHA)), u(ref))
