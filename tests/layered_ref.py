"""numpy float32 restatement of the layered (row-serial) scaled min-sum decoder.

TEST INFRASTRUCTURE ONLY (a helper like golden_util.py).  The algorithm is the contract written in
include/ldpc_amd.h ("layered min-sum"); there is no reference counterpart.  Batch-vectorised over
the frames, a Python loop over the checks in ascending index.

Per frame: app[v] = llr[v], c2v[e] = +0 for every edge in check-major order.  One iteration visits
the checks in ascending index; for check i with variables j_0 < ... < j_{d-1}:
    t_k      = app[j_k] - c2v[i,k]            (a degree-1 variable: t_k = llr[j_k] exactly)
    c2v[i,k] = (prod_{q != k} sgn t_q) * (alpha * min_{q != k} |t_q|)
    app[j_k] = t_k + c2v[i,k]
with sgn(0) = sgn(NaN) = 0, the min starting at +inf and a NaN never winning it (mag < min is
false).  After each full iteration bit[v] = (app[v] < 0).

A product of signs that contains a zero may come out as -0.0 here and +0.0 in the kernel.  Neither
`<`, `abs` nor `sgn` tells the two apart, and x + (+-0) differs only when x is itself a zero, so
decisions and iteration counts cannot differ; compare app / c2v with ==, not bitwise.
"""
import numpy as np

ES_OFF, ES_BATCH, ES_FRAME = 0, 1, 2


class Code:
    """Check-major edge lists of a dense H."""

    def __init__(self, H):
        H = np.asarray(H)
        self.M, self.N = H.shape
        chk, var = np.nonzero(H != 0)  # row-major: checks ascending, variables ascending
        self.edge_var = var.astype(np.int64)
        self.chk_ptr = np.zeros(self.M + 1, dtype=np.int64)
        np.cumsum(np.bincount(chk, minlength=self.M), out=self.chk_ptr[1:])
        self.deg1 = np.bincount(var, minlength=self.N) == 1
        self.H = (H != 0).astype(np.int64)
        self.E = len(var)


def _sgn(t):
    return (t > 0).astype(np.float32) - (t < 0).astype(np.float32)  # 0 for zero and NaN


def check_update(t, alpha):
    """t (B, d) float32 -> c2v (B, d): exclusive sign product times alpha * exclusive min."""
    B, d = t.shape
    s, mag = _sgn(t), np.abs(t)
    out = np.empty_like(t)
    alpha = np.float32(alpha)
    for k in range(d):
        sp = np.ones(B, dtype=np.float32)
        mn = np.full(B, np.inf, dtype=np.float32)
        for q in range(d):
            if q == k:
                continue
            sp = sp * s[:, q]
            mn = np.where(mag[:, q] < mn, mag[:, q], mn)
        with np.errstate(invalid="ignore"):
            out[:, k] = sp * (alpha * mn)
    return out


def iterate(code, llr, app, c2v, alpha):
    """One layered iteration in place on app (B, N) and c2v (B, E)."""
    for i in range(code.M):
        e0, e1 = code.chk_ptr[i], code.chk_ptr[i + 1]
        if e1 == e0:
            continue
        j = code.edge_var[e0:e1]
        with np.errstate(invalid="ignore"):
            t = app[:, j] - c2v[:, e0:e1]
            d1 = code.deg1[j]
            if d1.any():
                t[:, d1] = llr[:, j[d1]]
            c = check_update(t, alpha)
            c2v[:, e0:e1] = c
            app[:, j] = t + c


def syndrome_ok(code, bits):
    return ((bits.astype(np.int64) @ code.H.T) % 2 == 0).all(axis=1)


def decode(code, llr, max_iter, alpha=0.75, early_stop=ES_OFF, trace=None):
    """llr (B, N) float32 -> (bits uint8 (B, N), iters int32 (B,)).

    ES_OFF: every frame runs max_iter.  ES_FRAME: a frame freezes at the first iteration whose
    decisions satisfy H x = 0 (bits and count of that iteration), else runs max_iter.
    trace: optional list; gets (app.copy(), c2v.copy(), bits) after every iteration (all frames
    keep iterating there, frozen or not)."""
    if early_stop not in (ES_OFF, ES_FRAME):
        raise ValueError("layered decoding has no batch-global stop")
    if not isinstance(code, Code):
        code = Code(code)
    llr = np.ascontiguousarray(llr, dtype=np.float32)
    B = llr.shape[0]
    app = llr.copy()
    c2v = np.zeros((B, code.E), dtype=np.float32)
    bits = np.zeros((B, code.N), dtype=np.uint8)
    iters = np.full(B, max_iter, dtype=np.int32)
    done = np.zeros(B, dtype=bool)
    for it in range(1, max_iter + 1):
        iterate(code, llr, app, c2v, alpha)
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


def decode_scalar(code, llr, max_iter, alpha=0.75):
    """The same algorithm as plain scalar float32 loops (no vectorisation), ES off: an independent
    restatement for test_layered_host.  Returns (bits, app)."""
    if not isinstance(code, Code):
        code = Code(code)
    f32 = np.float32
    llr = np.asarray(llr, dtype=np.float32)
    a = f32(alpha)
    inf = f32(np.inf)
    apps = np.empty_like(llr)
    for b in range(llr.shape[0]):
        x = [f32(v) for v in llr[b]]
        app = list(x)
        c2v = [f32(0.0)] * code.E
        for _ in range(max_iter):
            for i in range(code.M):
                e0, e1 = int(code.chk_ptr[i]), int(code.chk_ptr[i + 1])
                js = [int(v) for v in code.edge_var[e0:e1]]
                t = [x[j] if code.deg1[j] else f32(app[j] - c2v[e0 + k]) for k, j in enumerate(js)]
                for k, j in enumerate(js):
                    sp, mn = f32(1.0), inf
                    for q in range(len(js)):
                        if q == k:
                            continue
                        sg = f32(1.0) if t[q] > 0 else (f32(-1.0) if t[q] < 0 else f32(0.0))
                        sp = f32(sp * sg)
                        m = f32(abs(t[q]))
                        if m < mn:
                            mn = m
                    with np.errstate(invalid="ignore"):
                        c = f32(sp * f32(a * mn))
                        c2v[e0 + k] = c
                        app[j] = f32(t[k] + c)
        apps[b] = app
    return (apps < 0).astype(np.uint8), apps
