// flood_layered_stream.hip -- layered (row-serial) scaled min-sum on the streaming layout, for gfx950:
// every message and posterior in HBM, any graph (algo LDPC_ALGO_LAYERED_MINSUM_ANY where the
// LDS-resident decoder of flood_layered.hip does not run).
//
// The algorithm is the contract in include/ldpc_amd.h ("layered min-sum"), the same float32
// operations in the same order as flood_layered.hip:
//     t_k      = app[j_k] - c2v[i,k]        (a degree-1 variable: t_k = llr[j_k] exactly)
//     c2v[i,k] = prod_{q != k} sgn(t_q) * (alpha * min_{q != k} |t_q|)      (minsum_rule)
//     app[j_k] = t_k + c2v[i,k]
// for the checks in ascending index, and bit[v] = app[v] < 0 after a full iteration.
//
// Layout: the streaming decoders' workspace as it is carved (stream_ws), frame-fastest.
//     msg[E][B]   c2v.  Never zero-filled: iteration 1 (FIRST) reads none, since x - (+0) = x exactly.
//     llrT[N][B]  for a variable of degree != 1 the posterior app, updated in place (its LLR is never
//                 read again after the transpose that puts it there); for a degree-1 variable the
//                 LLR, for good: its t is the LLR and its posterior llr + c2v is only a decision
//     bitsT, done, iters, partials: as the flooding decoders use them
//
// Schedule: graph.cpp cuts the checks into runs (layered_runs.hpp): maximal stretches of
// consecutive checks with pairwise disjoint variables, each split by exact degree into segments.  One
// launch per segment, in stream order; thread = (check of the segment, frame), the frame fastest, so a
// wave is 64 consecutive frames of one check: its edge range and variables are wave-uniform (scalar
// loads) and every load and store is 256 contiguous bytes.  BG2 has 28 runs whatever the lifting.
//
// Why race-free.  Within a launch, two threads either share the check (then they differ in the
// frame) or lie in two checks of one run, which share no variable and no edge: the threads touch
// disjoint (variable, frame) and (edge, frame) pairs.  Launches on one stream run in order, so a
// segment sees every write of the segments before it; the segments of one run commute because their
// checks are disjoint too.  Hence every check reads exactly what the serial definition gives it.
//
// Decisions: a degree-1 variable's goes from its check's thread straight to bitsT (as in the
// flooding check phase); the others are app < 0 (a variable without edges: llr < 0), taken by
// layered_decide_kernel after the last iteration, and after every iteration under LDPC_ES_FRAME for
// the syndrome.  A frozen frame (done[b]) skips every later launch and keeps its bits and count.
// Compile with -ffp-contract=off: no a*b+c may fuse on this path.
#include <algorithm>

#include "flood_stream.hpp"

namespace ldpc {

// The flooding min-sum check rule on a row held in registers: out_e = prod_{f != e} sgn(v_f) *
// (alpha * min_{f != e} |v_f|), as stream_row (flood_stream.hip) evaluates it: the LDS kernels' fast path
// (two minima by v_min / v_med3, sign parity by xor) when the row has no zero and no NaN message; else
// MinSumStats (exact torch.sign semantics).  Restated here and not shared with stream_row, whose code
// object this change leaves byte for byte as it was.
template <int DC>
__device__ __forceinline__ void minsum_rule(const float (&v)[DC], float alpha, float (&out)[DC]) {
    const float ninf = opaque_sf(-INFINITY);
    float m1 = fabsf(v[0]), m2 = opaque_sf(INFINITY);
    bool special = is_zero_sign(v[0]);
#pragma unroll
    for (int e = 1; e < DC; ++e) {
        two_min_step(m1, m2, v[e], ninf);
        special |= is_zero_sign(v[e]);
    }
    if (!special) {
        const uint32_t par = sign_parity_n<DC>(v) & 0x80000000u;
        const uint32_t s1 = __float_as_uint(alpha * m1) ^ par, s2 = __float_as_uint(alpha * m2) ^ par;
#pragma unroll
        for (int e = 0; e < DC; ++e)
            out[e] = __uint_as_float((__float_as_uint(v[e]) & 0x80000000u) ^ (fabsf(v[e]) == m1 ? s2 : s1));
    } else {
        MinSumStats st;
#pragma unroll
        for (int e = 0; e < DC; ++e) st.add(e, v[e]);
#pragma unroll
        for (int e = 0; e < DC; ++e) out[e] = st.c2v(e, v[e], alpha);
    }
}

// one (check, frame) of a segment of degree DC; FIRST: iteration 1
template <int DC, bool FIRST>
__global__ __launch_bounds__(256) void layered_stream_kernel(StreamArgs S, const int32_t *__restrict__ rows) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // grid: (frames, checks)
    if (b >= S.B || stream_skip(S, b)) return;
    const int e0 = S.chk_ptr[rows[blockIdx.y]];
    float t[DC];
#pragma unroll
    for (int e = 0; e < DC; ++e) {
        t[e] = S.llrT[(int64_t)S.ev[e0 + e] * S.B + b];
        if constexpr (!FIRST)
            if (S.ext_var[e0 + e] < 0) t[e] = t[e] - S.msg[(int64_t)(e0 + e) * S.B + b];  // wave-uniform branch
    }
    float c[DC];
    minsum_rule<DC>(t, S.alpha, c);
#pragma unroll
    for (int e = 0; e < DC; ++e) {
        const int xv = S.ext_var[e0 + e];  // wave-uniform (scalar load)
        if (xv < 0) {
            S.msg[(int64_t)(e0 + e) * S.B + b] = c[e];
            S.llrT[(int64_t)S.ev[e0 + e] * S.B + b] = t[e] + c[e];
        } else {
            S.bitsT[(int64_t)xv * S.B + b] = t[e] + c[e] < 0.0f;
        }
    }
}

// decisions of the variables of degree != 1 (degree 0: llrT is the LLR): bit = app < 0, NaN -> 0
__global__ __launch_bounds__(256) void layered_decide_kernel(StreamArgs S, int j0) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // grid: (frames, variables)
    const int j = j0 + blockIdx.y;
    if (S.var_ptr[j + 1] - S.var_ptr[j] == 1) return;  // taken by its check's thread
    if (b >= S.B || stream_skip(S, b)) return;
    const int64_t jb = (int64_t)j * S.B + b;
    S.bitsT[jb] = S.llrT[jb] < 0.0f;
}

namespace {

template <bool FIRST>
void launch_layers(const ldpc_graph *g, const StreamArgs &S, hipStream_t s) {
    const unsigned gx = (unsigned)((S.B + 255) / 256);
    for (size_t q = 0; q + 3 < g->lay_seg.size(); q += 4) {  // {run, degree, offset, count}: runs ascending
        const int d = g->lay_seg[q + 1], n = g->lay_seg[q + 3];
        for (int k0 = 0; k0 < n; k0 += kGridY) {
            const dim3 grid(gx, (unsigned)std::min(kGridY, n - k0));
            const int32_t *rows = g->lay_order + g->lay_seg[q + 2] + k0;
            switch (d) {  // degree 0: nothing to update; degrees above 32 are refused on the host
#define X(k) case k: hipLaunchKernelGGL((layered_stream_kernel<k, FIRST>), grid, dim3(256), 0, s, S, rows); break;
                LDPC_STREAM_DEG_CASES(X)
#undef X
                default: break;
            }
        }
    }
}

}  // namespace

int run_layered_stream(const FloodCall &c) {
    const ldpc_graph *g = c.g;
    const int64_t B = c.B;
    const int max_iter = c.max_iter, es = c.es;
    hipStream_t s = c.s;
    const StreamWs w = stream_ws(g, B, max_iter, c.work);
    const StreamArgs S{g->chk_ptr, g->ev, g->var_ptr, g->var_edge, g->M, g->N, g->E, B, w.msg, w.llrT, w.bitsT, w.done,
                       w.iters, w.ctl, w.invalid, c.alpha, es, g->ext_var};
    LDPC_HIP(hipMemsetAsync(w.done, 0, (size_t)B, s));
    launch_stream_transpose(c.llr, B, g->N, w.llrT, s);
    const unsigned gx = (unsigned)((B + 255) / 256);
    for (int it = 0; it < max_iter; ++it) {
        if (it == 0)
            launch_layers<true>(g, S, s);
        else
            launch_layers<false>(g, S, s);
        if (es == LDPC_ES_FRAME || it == max_iter - 1) {
            for (int j0 = 0; j0 < g->N; j0 += kGridY)
                hipLaunchKernelGGL(layered_decide_kernel, dim3(gx, (unsigned)std::min(kGridY, g->N - j0)), dim3(256), 0, s,
                                   S, j0);
            if (es == LDPC_ES_FRAME) launch_stream_syndrome(S, it, s);
        }
        LDPC_CHECK_LAUNCH("layered stream iteration");
    }
    const bool want = c.counters || c.batch_iters;
    launch_stream_emit(S, max_iter, c.out_dtype, c.bits, c.iters, want ? w.partials : nullptr, s);
    LDPC_CHECK_LAUNCH("layered stream emit");
    if (!want) return LDPC_OK;
    // batch_iters: ES off was set before the launch; otherwise the largest per-frame count
    return reduce_counter_rows(w.partials, (B + 63) / 64, c.counters, es == LDPC_ES_OFF ? nullptr : c.batch_iters,
                               nullptr, s);
}

}  // namespace ldpc
