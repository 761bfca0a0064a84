"""numpy float16 restatement of the half-precision layered scaled min-sum decoder (LDPC_ALGO_LAYERED_MINSUM_F16).

TEST INFRASTRUCTURE ONLY (a helper like half_ref.py / layered_ref.py).  The algorithm is the contract written
in include/ldpc_amd.h ("Half-precision layered min-sum"); there is no reference counterpart.
Batch-vectorised over the frames, a Python loop over the checks in ascending index.

Every value is IEEE binary16, every operation rounded to nearest-even with gradual underflow (numpy evaluates
a float16 add or multiply in float32 and rounds the result: innocuous double rounding, see half_ref.py).
C = 1024 is the clamp; clamp=None switches it off and lets the minimum start at +inf, for the tests that
show it engaged.

    x[v]     = clamp(half(llr[v]))              a magnitude that rounds to infinity becomes +-C
    app[v]   = x[v], c2v[e] = +0                at the start
    t_k      = clamp(app[j_k] - c2v[i,k])       (a degree-1 variable: t_k = x[j_k] exactly)
    c2v[i,k] = (prod_{q != k} sgn t_q) * (a * min(C, min_{q != k} |t_q|))     a = half(alpha), sgn(0) = 0
    app[j_k] = t_k + c2v[i,k]                   unclamped
for the checks in ascending index; bit[v] = (app[v] < 0) after each full iteration.

A product of signs that contains a zero may come out as -0.0 here and +0.0 in the kernel.  Neither `<`,
`abs` nor `sgn` tells the two apart, and x + (+-0) differs only when x is itself a zero, so decisions and
iteration counts cannot differ; compare app / c2v with ==, not bitwise.
"""
import numpy as np

from half_ref import F16, _clamp, half_alpha, to_half
from half_ref import SPECIALS, saturating, with_specials  # noqa: F401  (inputs the tests share)
from layered_ref import Code

ES_OFF, ES_BATCH, ES_FRAME = 0, 1, 2


def check_update(t, a, clamp=1024.0):
    """t (..., d) float16 -> c2v (..., d): half_ref.check_update with the minimum starting at C."""
    d = t.shape[-1]
    s = (t > 0).astype(F16) - (t < 0).astype(F16)  # 0 for zero and NaN
    mag = np.abs(t)
    out = np.empty_like(t)
    start = F16(np.inf) if clamp is None else F16(clamp)
    for k in range(d):
        sp = np.ones(t.shape[:-1], dtype=F16)
        mn = np.full(t.shape[:-1], start, dtype=F16)
        for q in range(d):
            if q == k:
                continue
            sp = sp * s[..., q]
            mn = np.where(mag[..., q] < mn, mag[..., q], mn)
        with np.errstate(invalid="ignore"):
            out[..., k] = sp * (a * mn)  # a * mn rounded once; the sign product is +-1 or 0: exact
    return out


def iterate(code, x, app, c2v, a, clamp):
    """One layered iteration in place on app (B, N) and c2v (B, E), both float16."""
    for i in range(code.M):
        e0, e1 = code.chk_ptr[i], code.chk_ptr[i + 1]
        if e1 == e0:
            continue
        j = code.edge_var[e0:e1]
        with np.errstate(invalid="ignore", over="ignore"):
            t = _clamp(app[:, j] - c2v[:, e0:e1], clamp)
            d1 = code.deg1[j]
            if d1.any():
                t[:, d1] = x[:, j[d1]]
            c = check_update(t, a, clamp)
            c2v[:, e0:e1] = c
            app[:, j] = t + c


def syndrome_ok(code, bits):
    return ((bits.astype(np.int64) @ code.H.T) % 2 == 0).all(axis=1)


def decode(code, llr, max_iter, alpha=0.75, early_stop=ES_OFF, trace=None, clamp=1024.0):
    """llr (B, N) float32 -> (bits uint8 (B, N), iters int32 (B,)).

    ES_OFF: every frame runs max_iter.  ES_FRAME: a frame freezes at the first iteration whose decisions
    satisfy H x = 0 (bits and count of that iteration), else runs max_iter.
    trace: optional list; gets (app.copy(), c2v.copy(), bits) after every iteration (all frames keep
    iterating there, frozen or not)."""
    if early_stop not in (ES_OFF, ES_FRAME):
        raise ValueError("layered decoding has no batch-global stop")
    if not isinstance(code, Code):
        code = Code(code)
    a = half_alpha(alpha)
    x = to_half(llr, clamp)
    B = x.shape[0]
    app = x.copy()
    c2v = np.zeros((B, code.E), dtype=F16)
    bits = np.zeros((B, code.N), dtype=np.uint8)
    iters = np.full(B, max_iter, dtype=np.int32)
    done = np.zeros(B, dtype=bool)
    for it in range(1, max_iter + 1):
        iterate(code, x, app, c2v, a, clamp)
        now = (app < 0).astype(np.uint8)
        if trace is not None:
            trace.append((app.copy(), c2v.copy(), now.copy()))
        bits[~done] = now[~done]
        if early_stop == ES_FRAME:
            newly = syndrome_ok(code, now) & ~done
            iters[newly] = it
            done |= newly
            if done.all() and trace is None:
                break
    return bits, iters


def decode_scalar(code, llr, max_iter, alpha=0.75, early_stop=ES_OFF, clamp=1024.0):
    """The same algorithm as plain scalar loops, one Python operation per rounding: an independent
    restatement for test_layered_half_ref_host.  Returns (bits, iters, app); app is the posterior of the
    iteration a frame's bits come from."""
    if not isinstance(code, Code):
        code = Code(code)
    a = half_alpha(alpha)
    llr = np.asarray(llr, dtype=np.float32)
    B = llr.shape[0]
    zero, one = F16(0), F16(1)
    C = None if clamp is None else F16(clamp)
    start = F16(np.inf) if C is None else C

    def cl(v):
        if C is None:
            return v
        return C if v > C else (-C if v < -C else v)

    bits = np.zeros((B, code.N), dtype=np.uint8)
    apps = np.zeros((B, code.N), dtype=F16)
    iters = np.full(B, max_iter, dtype=np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(B):
            x = [cl(F16(v)) for v in llr[b]]  # np.float16(np.float32) rounds to nearest-even
            app = list(x)
            c2v = [zero] * code.E
            for it in range(1, max_iter + 1):
                for i in range(code.M):
                    e0, e1 = int(code.chk_ptr[i]), int(code.chk_ptr[i + 1])
                    js = [int(v) for v in code.edge_var[e0:e1]]
                    t = [x[j] if code.deg1[j] else cl(F16(app[j] - c2v[e0 + k])) for k, j in enumerate(js)]
                    for k, j in enumerate(js):
                        sp, mn = one, start
                        for q in range(len(js)):
                            if q == k:
                                continue
                            sg = one if t[q] > 0 else (-one if t[q] < 0 else zero)
                            sp = F16(sp * sg)
                            m = F16(abs(t[q]))
                            if m < mn:
                                mn = m
                        c = F16(sp * F16(a * mn))
                        c2v[e0 + k] = c
                        app[j] = F16(t[k] + c)
                now = np.array([1 if v < 0 else 0 for v in app], dtype=np.uint8)
                bits[b] = now
                apps[b] = app
                if early_stop == ES_FRAME and syndrome_ok(code, now[None])[0]:
                    iters[b] = it
                    break
    return bits, iters, apps


def first_iteration_unclamped(code, llr, alpha=0.75):
    """Decisions after iteration 1 of a WRONG decoder that clamps the channel values but forms t = app - c2v
    without the clamp in iteration 1 (app is x only until an earlier check of the iteration has updated it).
    An input on which these differ from decode()'s shows that the iteration-1 clamp decides outcomes."""
    if not isinstance(code, Code):
        code = Code(code)
    x = to_half(llr)
    app = x.copy()
    c2v = np.zeros((x.shape[0], code.E), dtype=F16)
    iterate(code, x, app, c2v, half_alpha(alpha), None)
    return (app < 0).astype(np.uint8)
