// flood_layered_stream.hip -- layered (row-serial) scaled min-sum on the streaming layout, for gfx950:
// every message and posterior in HBM, any graph (algo LDPC_ALGO_LAYERED_MINSUM_ANY where the
// LDS-resident decoder of flood_layered.hip does not run).
//
// The algorithm is the contract in include/ldpc_amd.h ("layered min-sum"), the same float32
// operations in the same order as flood_layered.hip:
//     t_k      = app[j_k] - c2v[i,k]        (a degree-1 variable: t_k = llr[j_k] exactly)
//     c2v[i,k] = prod_{q != k} sgn(t_q) * (alpha * min_{q != k} |t_q|)      (minsum_rule, flood_stream.hpp)
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
    per_segment(g, (unsigned)((S.B + 255) / 256), [&](int d, dim3 grid, const int32_t *rows) {
        switch (d) {  // degree 0: nothing to update; degrees above 32 are refused on the host
#define X(k) case k: hipLaunchKernelGGL((layered_stream_kernel<k, FIRST>), grid, dim3(256), 0, s, S, rows); break;
            LDPC_STREAM_DEG_CASES(X)
#undef X
            default: break;
        }
    });
}

}  // namespace

int run_layered_stream(const FloodCall &c) {
    const ldpc_graph *g = c.g;
    const int64_t B = c.B;
    hipStream_t s = c.s;
    const StreamWs w = stream_ws(g, B, c.max_iter, c.work);
    const StreamArgs S =
        make_stream_args(g, B, c.alpha, c.es, w.msg, w.llrT, w.bitsT, w.done, w.iters, w.ctl, w.invalid, g->ext_var);
    const unsigned gx = (unsigned)((B + 255) / 256);
    return layered_stream_drive(
        c, S, w.partials, "layered stream",
        [&]() -> int {
            launch_stream_transpose(c.llr, B, g->N, w.llrT, s);
            return LDPC_OK;
        },
        [&](bool first) { first ? launch_layers<true>(g, S, s) : launch_layers<false>(g, S, s); },
        [&] {
            for (int j0 = 0; j0 < g->N; j0 += kGridY)
                hipLaunchKernelGGL(layered_decide_kernel, dim3(gx, (unsigned)std::min(kGridY, g->N - j0)), dim3(256), 0, s,
                                   S, j0);
        });
}

}  // namespace ldpc
