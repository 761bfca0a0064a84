"""LDPCNeuralDecoder's forward restated in numpy float32, operation by operation, as include/ldpc_amd.h
defines ldpc_neural_forward (test infrastructure; vectorised over frames and over groups of equal
degree only -- every per-element operation and its order are the definition's).

    x0[e]  = +0 + llr[var(e)];  v_{-1} = x0
    c_l    = the check rule on v_{l-1} (check_rule below)
    S[e]   = +0 + the variable's other c_l in ascending order
    v_l[e] = x0[e] * w_ch_l[e];  + S[e];  + w_res_l[i] * v_{l-1-i}[e] for i < min(l, depth_L)
    app[j] = +0 + the variable's c_{I-1} in ascending order

Graph description (var-major edge numbering of create_LLR_mapping): cptr (G + 1) / cmem (E) list each
check's edges ascending; vptr (N + 1): variable j's edges are [vptr[j], vptr[j + 1]); K is the row
length of the check index tensor (a check with degree - 1 < K has padding: the minimum is capped at 1e10).
"""
import numpy as np

F32 = np.float32
BIG = F32(1e10)


def groups_from_H(H):
    """(cptr, cmem, vptr, K) of a dense H: edge e = the e-th nonzero of H.T in row-major order."""
    H = np.asarray(H) != 0
    var, chk = np.nonzero(H.T)                      # var-major: e ascending with (var, chk)
    E = len(var)
    order = np.argsort(chk, kind="stable")          # edges by check, ascending inside a check
    dc = np.bincount(chk, minlength=H.shape[0])
    dv = np.bincount(var, minlength=H.shape[1])
    cptr = np.concatenate([[0], np.cumsum(dc)]).astype(np.int32)
    vptr = np.concatenate([[0], np.cumsum(dv)]).astype(np.int32)
    assert cptr[-1] == E and vptr[-1] == E
    return cptr, order.astype(np.int32), vptr, int(dc.max()) - 1


def _by_degree(ptr):
    """{degree: (group ids (n,), starts (n,))} of the groups ptr describes."""
    deg = np.diff(ptr)
    return {int(d): (np.nonzero(deg == d)[0], ptr[:-1][deg == d]) for d in np.unique(deg) if d > 0}


def check_rule(v, cptr, cmem, K):
    """c[b, e] = prod sign(v + 1e-10f) * min |v|' over the other edges of e's check (|0| -> 1e10), as
    the two passes of the kernels' check rule: zero / NaN counts and the parity of negative signs give
    the sign product (a zero product keeps its sign; another NaN edge gives NaN), the two smallest |v|'
    give the minimum of the others (a NaN never wins it), capped at 1e10 when the row has padding."""
    B = v.shape[0]
    out = np.empty_like(v)
    for d, (_, starts) in _by_degree(cptr).items():
        mem = cmem[starts[:, None] + np.arange(d)[None, :]]          # (n, d) edge ids
        x = v[:, mem]                                                # (B, n, d)
        sv = x + F32(1e-10)
        zero, nan, negm = sv == 0, np.isnan(sv), sv < 0
        zeros, nans, neg = zero.sum(2), nan.sum(2), negm.sum(2) & 1
        a = np.abs(x)
        a = np.where(a == 0, BIG, a)
        m1 = np.full((B, len(starts)), np.inf, F32)
        m2 = m1.copy()
        pos = np.full(m1.shape, -1)
        for p in range(d):
            ap = a[:, :, p]
            lt1 = ap < m1
            lt2 = ~lt1 & (ap < m2)
            m2 = np.where(lt1, m1, np.where(lt2, ap, m2))
            pos = np.where(lt1, p, pos)
            m1 = np.where(lt1, ap, m1)
        for p in range(d):
            z = zeros - zero[:, :, p]
            nn = nans - nan[:, :, p]
            ng = (neg ^ negm[:, :, p]) != 0
            m = np.where(pos == p, m2, m1)
            if K > d - 1:
                m = np.minimum(m, BIG)
            sp = np.where(z > 0, np.where(ng, F32(-0.0), F32(0.0)), np.where(ng, F32(-1.0), F32(1.0)))
            out[:, mem[:, p]] = np.where(nn > 0, F32(np.nan), (sp * m).astype(F32))
    return out


def _others_sum(c, vptr):
    """S[b, e] = +0 + the other members of e's run, ascending."""
    S = np.zeros_like(c)
    for d, (_, starts) in _by_degree(vptr).items():
        x = c[:, starts[:, None] + np.arange(d)[None, :]]            # (B, n, d)
        for q in range(d):
            s = np.zeros(x.shape[:2], F32)
            for t in range(d):
                if t != q:
                    s = s + x[:, :, t]
            S[:, starts + q] = s
    return S


def _run_sum(c, vptr):
    """app[b, j] = +0 + the members of run j, ascending (an empty run: +0)."""
    app = np.zeros((c.shape[0], len(vptr) - 1), F32)
    for d, (ids, starts) in _by_degree(vptr).items():
        s = np.zeros((c.shape[0], len(ids)), F32)
        for t in range(d):
            s = s + c[:, starts + t]
        app[:, ids] = s
    return app


def neural_ref(llr, cptr, cmem, vptr, K, iterations, depth_L, w_ch=None, w_res=None):
    """app (B, N) float32.  w_ch (iterations - 1, E), w_res (iterations - 1, depth_L)."""
    llr = np.ascontiguousarray(llr, dtype=F32)
    cptr, cmem, vptr = (np.asarray(a, dtype=np.int64) for a in (cptr, cmem, vptr))
    evar = np.repeat(np.arange(len(vptr) - 1), np.diff(vptr))
    with np.errstate(all="ignore"):
        x0 = F32(0.0) + llr[:, evar]
        v, prevs = x0, []                               # prevs[i] = v_{l-1-i}
        for l in range(iterations - 1):
            c = check_rule(v, cptr, cmem, K)
            r = x0 * np.asarray(w_ch[l], dtype=F32)[None, :]
            r = r + _others_sum(c, vptr)
            for i in range(min(l, depth_L)):
                r = r + F32(w_res[l][i]) * prevs[i]
            v = r.astype(F32)
            prevs = [v] + prevs[:max(depth_L - 1, 0)]
        return _run_sum(check_rule(v, cptr, cmem, K), vptr)

