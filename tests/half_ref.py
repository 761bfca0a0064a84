"""numpy float16 restatement of the half-precision flooding scaled min-sum decoder (LDPC_ALGO_MINSUM_F16).

TEST INFRASTRUCTURE ONLY (a helper like layered_ref.py).  The algorithm is the contract written in
include/ldpc_amd.h ("Half-precision min-sum"); there is no reference counterpart.  Batch-vectorised over
the frames and over the nodes of one degree; a Python loop over the positions of a node.

Every value is IEEE binary16, every operation rounded to nearest-even with gradual underflow.  numpy
evaluates a float16 add or multiply in float32 and rounds the result to float16; float32 carries
24 >= 2 * 11 + 2 bits, so that double rounding is innocuous and both are correctly rounded, subnormals
included.  C = 1024 is the clamp (clamp=None switches it off, for the tests that show it engaged).

    x[v]        = clamp(half(llr[v]))                  a magnitude that rounds to infinity becomes +-C
    v2c[e]      = x[var(e)]                            at the start
    c2v[i,k]    = (prod_{q != k} sgn v2c[i,q]) * (a * min_{q != k} |v2c[i,q]|)      a = half(alpha), sgn(0) = 0
    v2c[i_k,j]  = clamp(x[j] + sum_{q != k} c2v[i_q,j])    left to right in ascending q, each add rounded
    app[j]      = x[j] + sum_q c2v[i_q,j]              unclamped; bit[j] = (app[j] < 0)

A product of signs that contains a zero may come out as -0.0 here and +0.0 in the kernel; a row with a zero
has minimum 0, so only the sign of a zero differs and `<` cannot tell: compare decisions and iteration
counts (or values with ==), never message bits.
"""
import numpy as np

ES_OFF, ES_BATCH, ES_FRAME = 0, 1, 2
F16 = np.float16


class Code:
    """Check-major edge list of a dense H, checks and variables grouped by degree."""

    def __init__(self, H):
        H = np.asarray(H)
        self.M, self.N = H.shape
        chk, var = np.nonzero(H != 0)  # row-major: checks ascending, variables ascending
        self.edge_chk = chk.astype(np.int64)
        self.edge_var = var.astype(np.int64)
        self.E = len(var)
        self.H = (H != 0).astype(np.int64)
        self.chk_ptr = np.zeros(self.M + 1, dtype=np.int64)
        np.cumsum(np.bincount(chk, minlength=self.M), out=self.chk_ptr[1:])
        # per variable: its edge ids in ascending check order (edge ids ascend with the check)
        order = np.argsort(var, kind="stable")
        self.var_ptr = np.zeros(self.N + 1, dtype=np.int64)
        np.cumsum(np.bincount(var, minlength=self.N), out=self.var_ptr[1:])
        self.var_edges = order
        # groups: degree -> (node ids, (n, degree) edge ids)
        self.chk_groups = self._groups(self.chk_ptr, np.arange(self.E))
        self.var_groups = self._groups(self.var_ptr, order)
        self.max_dv = int(np.diff(self.var_ptr).max()) if self.N else 0

    @staticmethod
    def _groups(ptr, edges):
        deg = np.diff(ptr)
        out = []
        for d in np.unique(deg):
            nodes = np.nonzero(deg == d)[0]
            idx = edges[ptr[nodes][:, None] + np.arange(d)[None, :]] if d else np.zeros((len(nodes), 0), np.int64)
            out.append((int(d), nodes, idx))
        return out


def to_half(llr, clamp=1024.0):
    """x = clamp(half(llr)): float32 -> binary16 nearest-even, +-inf (also by rounding) -> +-C, NaN stays."""
    with np.errstate(over="ignore"):
        x = np.asarray(llr, dtype=np.float32).astype(F16)
    return _clamp(x, clamp)


def _clamp(v, clamp):
    if clamp is None:
        return v
    c = F16(clamp)
    return np.where(v > c, c, np.where(v < -c, -c, v))  # a NaN passes through


def check_update(t, a):
    """t (..., d) float16 -> c2v (..., d): exclusive sign product times (a * exclusive min)."""
    d = t.shape[-1]
    s = (t > 0).astype(F16) - (t < 0).astype(F16)  # 0 for zero and NaN
    mag = np.abs(t)
    out = np.empty_like(t)
    for k in range(d):
        sp = np.ones(t.shape[:-1], dtype=F16)
        mn = np.full(t.shape[:-1], np.inf, dtype=F16)
        for q in range(d):
            if q == k:
                continue
            sp = sp * s[..., q]
            mn = np.where(mag[..., q] < mn, mag[..., q], mn)
        with np.errstate(invalid="ignore"):
            out[..., k] = sp * (a * mn)  # a * mn rounded once; the sign product is +-1 or 0: exact
    return out


def iterate(code, x, v2c, a, clamp):
    """One flooding iteration: v2c (B, E) in, -> (c2v, new v2c, app)."""
    c2v = np.empty_like(v2c)
    for d, _, idx in code.chk_groups:
        if d:
            c2v[:, idx] = check_update(v2c[:, idx], a)
    new = np.empty_like(v2c)
    app = np.empty_like(x)
    with np.errstate(invalid="ignore", over="ignore"):
        for d, nodes, idx in code.var_groups:
            c = c2v[:, idx]  # (B, n, d), ascending check order
            xs = x[:, nodes]
            s = xs.copy()
            for q in range(d):
                s = s + c[:, :, q]
            app[:, nodes] = s
            for k in range(d):
                s = xs.copy()
                for q in range(d):
                    if q != k:
                        s = s + c[:, :, q]
                new[:, idx[:, k]] = _clamp(s, clamp)
    return c2v, new, app


def syndrome_ok(code, bits):
    return ((bits.astype(np.int64) @ code.H.T) % 2 == 0).all(axis=1)


def half_alpha(alpha):
    a = F16(np.float32(alpha))
    if not (a >= 0 and a <= 1):
        raise ValueError("half(alpha) must be in [0, 1]")
    return a


def decode(code, llr, max_iter, alpha=0.75, early_stop=ES_OFF, trace=None, clamp=1024.0):
    """llr (B, N) float32 -> (bits uint8 (B, N), iters int32 (B,)).

    ES_OFF: every frame runs max_iter.  ES_FRAME: a frame freezes at the first iteration whose decisions
    satisfy H x = 0 (bits and count of that iteration), else runs max_iter.
    trace: optional list; gets (app, v2c, c2v, bits) copies after every iteration (all frames keep
    iterating there, frozen or not); v2c is what the iteration wrote."""
    if early_stop not in (ES_OFF, ES_FRAME):
        raise ValueError("half-precision min-sum has no batch-global stop")
    if not isinstance(code, Code):
        code = Code(code)
    if code.max_dv > 32:
        raise ValueError("variable degree above 32")
    a = half_alpha(alpha)
    x = to_half(llr, clamp)
    B = x.shape[0]
    v2c = x[:, code.edge_var].copy()
    bits = np.zeros((B, code.N), dtype=np.uint8)
    iters = np.full(B, max_iter, dtype=np.int32)
    done = np.zeros(B, dtype=bool)
    for it in range(1, max_iter + 1):
        c2v, v2c, app = iterate(code, x, v2c, a, clamp)
        now = (app < 0).astype(np.uint8)
        if trace is not None:
            trace.append((app.copy(), v2c.copy(), c2v.copy(), now.copy()))
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
    restatement for test_half_ref_host.  Returns (bits, iters, app); app is the posterior of the iteration a
    frame's bits come from."""
    if not isinstance(code, Code):
        code = Code(code)
    a = half_alpha(alpha)
    llr = np.asarray(llr, dtype=np.float32)
    B = llr.shape[0]
    zero, inf = F16(0), F16(np.inf)
    C = None if clamp is None else F16(clamp)

    def cl(v):
        if C is None:
            return v
        return C if v > C else (-C if v < -C else v)

    rows = [[int(e) for e in range(code.chk_ptr[i], code.chk_ptr[i + 1])] for i in range(code.M)]
    cols = [[int(e) for e in code.var_edges[code.var_ptr[j]:code.var_ptr[j + 1]]] for j in range(code.N)]
    ev = [int(v) for v in code.edge_var]
    bits = np.zeros((B, code.N), dtype=np.uint8)
    apps = np.zeros((B, code.N), dtype=F16)
    iters = np.full(B, max_iter, dtype=np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(B):
            x = [cl(F16(v)) for v in llr[b]]  # np.float16(np.float32) rounds to nearest-even
            v2c = [x[ev[e]] for e in range(code.E)]
            for it in range(1, max_iter + 1):
                c2v = [zero] * code.E
                for es in rows:
                    for e in es:
                        sp, mn = F16(1), inf
                        for q in es:
                            if q == e:
                                continue
                            t = v2c[q]
                            sg = F16(1) if t > 0 else (F16(-1) if t < 0 else zero)
                            sp = F16(sp * sg)
                            m = F16(abs(t))
                            if m < mn:
                                mn = m
                        c2v[e] = F16(sp * F16(a * mn))
                app = []
                for j, es in enumerate(cols):
                    s = x[j]
                    for q in es:
                        s = F16(s + c2v[q])
                    app.append(s)
                    for e in es:
                        s = x[j]
                        for q in es:
                            if q != e:
                                s = F16(s + c2v[q])
                        v2c[e] = cl(s)
                now = np.array([1 if v < 0 else 0 for v in app], dtype=np.uint8)
                bits[b] = now
                apps[b] = app
                if early_stop == ES_FRAME and syndrome_ok(code, now[None])[0]:
                    iters[b] = it
                    break
    return bits, iters, apps


# ---------------------------------------------------------------- inputs shared by the host and GPU tests
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, 1e6, -1e6,      # zeros, infinities, rounds to infinity
                     2.9e-8, 3e-8, -3e-8, 6e-8, 1e-7, -1e-7,     # either side of half the smallest subnormal 2^-24
                     1 + 2.0 ** -11, -(1 + 2.0 ** -11),          # ties of the float32 -> binary16 rounding:
                     1 + 3 * 2.0 ** -11, -(1 + 3 * 2.0 ** -11)],  # to even, down (1) and up (1 + 2^-9)
                    dtype=np.float32)


def with_specials(llr, seed=5):
    """A copy of llr (B, N) with every SPECIALS value at 3 random places of every frame."""
    rng = np.random.default_rng(seed)
    out = np.array(llr, dtype=np.float32)
    for b in range(out.shape[0]):
        pos = rng.choice(out.shape[1], size=3 * len(SPECIALS), replace=False)
        out[b, pos] = np.tile(SPECIALS, 3)
    return out


def saturating(llr, scale=64.0):
    """LLRs scaled up: beliefs grow past the clamp within a few iterations (0 dB: frames still take 2 to 5
    iterations to converge, so the clamped messages decide the outcome)."""
    return (np.asarray(llr, dtype=np.float32) * np.float32(scale)).astype(np.float32)
