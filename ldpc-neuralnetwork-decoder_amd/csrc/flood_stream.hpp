// flood_stream.hpp -- what the streaming translation units share: flood_stream.hip (flooding and hybrid
// min-sum), flood_layered_stream.hip (layered min-sum) and flood_layered_stream_half.hip (its binary16
// form, which borrows the driver and the syndrome and emit passes).  The layout is flood_stream.hip's:
// every array frame-fastest, so that a wave -- 64 consecutive frames of one node -- loads and stores 256
// contiguous bytes.  Here:
//     StreamArgs, make_stream_args   the kernels' argument block and the one place it is filled
//     stream_skip, minsum_rule       device: the stop test and the float32 min-sum rule on a register row
//     StreamWs, stream_ws            the streaming workspace carve
//     launch_stream_*                flood_stream.hip's transpose, syndrome and emit passes
//     per_segment                    one launch per layer segment (the layered twin of per_degree)
//     layered_stream_drive           the layered streaming decoders' host loop
#pragma once
#include <algorithm>
#include <string>

#include "flood_host.hpp"

namespace ldpc {

struct StreamArgs {
    const int32_t *chk_ptr, *ev, *var_ptr, *var_edge;
    int M, N;
    int64_t E, B;
    float *msg;        // [E][B] flooding: v2c / c2v in place; layered: c2v
    float *llrT;       // [N][B] flooding: the LLRs; layered: the posterior of a variable of degree != 1
    uint8_t *bitsT;    // [N][B] hard decisions of the latest iteration
    uint8_t *done;     // [B] LDPC_ES_FRAME: frame frozen
    int32_t *iters;    // [B] LDPC_ES_FRAME: iterations of a frozen frame
    int32_t *ctl;      // [0] batch stopped  [1] batch iterations
    int32_t *invalid;  // [max_iter] LDPC_ES_BATCH: frames failing H x = 0 after each iteration
    float alpha;
    int es;
    // flooding and layered decoders (null for the hybrid min-sum): per edge, its variable when that has
    // degree 1.  Such an edge's v2c is the channel LLR forever, so the check phase leaves it in
    // place and takes the variable's decision itself (APP = llr + c2v = v2c + c2v, the same
    // float add); the degree-1 variables get no variable-phase launch.
    const int32_t *ext_var;
};

__device__ __forceinline__ bool stream_skip(const StreamArgs &S, int64_t b) {
    if (S.es == LDPC_ES_BATCH) return S.ctl[0] != 0;
    if (S.es == LDPC_ES_FRAME) return S.done[b] != 0;
    return false;
}

// The only place a StreamArgs is filled; an array a decoder does not have is passed as nullptr.
inline StreamArgs make_stream_args(const ldpc_graph *g, int64_t B, float alpha, int es, float *msg, float *llrT,
                                   uint8_t *bitsT, uint8_t *done, int32_t *iters, int32_t *ctl, int32_t *invalid,
                                   const int32_t *ext_var) {
    return StreamArgs{g->chk_ptr, g->ev, g->var_ptr, g->var_edge, g->M, g->N, g->E, B, msg, llrT, bitsT, done,
                      iters, ctl, invalid, alpha, es, ext_var};
}

// The min-sum check rule on a row held in registers: out_e = prod_{f != e} sgn(v_f) * (alpha * min_{f != e}
// |v_f|).  The LDS kernels' fast path (two minima by v_min / v_med3, sign parity by xor) when the row has no
// zero and no NaN message; else MinSumStats (exact torch.sign semantics).  Used by the flooding check phase
// (stream_row) and the layered update (layered_stream_kernel).
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

#define LDPC_STREAM_DEG_CASES(X)                                                                       \
    X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) \
    X(19) X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)

// the streaming workspace (ldpc_flood_workspace_size on a streaming graph); base == nullptr only sizes it
struct StreamWs {
    float *msg, *llrT;
    uint8_t *bitsT, *done;
    int32_t *iters, *ctl, *invalid;
    uint32_t *partials;
    int64_t bytes;
};
StreamWs stream_ws(const ldpc_graph *g, int64_t B, int max_iter, void *base);

// grid.y of the per-node launches (grid = (frames, nodes)) is chunked to this many nodes
constexpr int kGridY = 65535;

// flood_stream.hip's passes that the layered decoder runs as they are: the (B, N) -> (N, B) LLR
// transpose, the per-frame syndrome of bitsT after iteration `it` (LDPC_ES_FRAME: freezes the valid
// frames), and the (N, B) -> (B, N) emission of bitsT with the iteration counts and counter rows
void launch_stream_transpose(const float *llr, int64_t B, int N, float *llrT, hipStream_t s);
void launch_stream_syndrome(const StreamArgs &S, int it, hipStream_t s);
void launch_stream_emit(const StreamArgs &S, int max_iter, int out_dtype, void *bits, int32_t *iters_out,
                        uint32_t *partials, hipStream_t s);

// One launch per layer segment, in stream order: launch(degree, grid, rows) over the {run, degree, offset,
// count} records graph.cpp builds (lay_seg: runs ascending; lay_order: the checks), grid = (gx, checks) with
// grid.y chunked to kGridY as per_degree (flood_stream.hip) does
template <class F>
void per_segment(const ldpc_graph *g, unsigned gx, F &&launch) {
    for (size_t q = 0; q + 3 < g->lay_seg.size(); q += 4) {
        const int n = g->lay_seg[q + 3];
        for (int k0 = 0; k0 < n; k0 += kGridY)
            launch(g->lay_seg[q + 1], dim3(gx, (unsigned)std::min(kGridY, n - k0)), g->lay_order + g->lay_seg[q + 2] + k0);
    }
}

// The host loop of a layered streaming decoder (`name` heads its launch-error texts).  T carries at least the
// graph, B, bitsT, done, iters and es: what the syndrome and emit passes read.  The decoder brings
//     transpose() -> int   the LLRs into its posterior array (LDPC_OK or a failure already recorded)
//     layers(first)        every segment launch of one iteration; first: iteration 1, which reads no c2v
//     decide()             bitsT of the variables of degree != 1 from the posteriors
// Decisions are taken after the last iteration, and after every iteration under LDPC_ES_FRAME for the syndrome
// that freezes the valid frames.
template <class Transpose, class Layers, class Decide>
int layered_stream_drive(const FloodCall &c, const StreamArgs &T, uint32_t *partials, const char *name,
                         Transpose &&transpose, Layers &&layers, Decide &&decide) {
    const int max_iter = c.max_iter, es = c.es;
    hipStream_t s = c.s;
    LDPC_HIP(hipMemsetAsync(T.done, 0, (size_t)T.B, s));
    if (const int rc = transpose(); rc != LDPC_OK) return rc;
    for (int it = 0; it < max_iter; ++it) {
        layers(it == 0);
        if (es == LDPC_ES_FRAME || it == max_iter - 1) {
            decide();
            if (es == LDPC_ES_FRAME) launch_stream_syndrome(T, it, s);
        }
        LDPC_CHECK_LAUNCH(std::string(name) + " iteration");
    }
    const bool want = c.counters || c.batch_iters;
    launch_stream_emit(T, max_iter, c.out_dtype, c.bits, c.iters, want ? partials : nullptr, s);
    LDPC_CHECK_LAUNCH(std::string(name) + " emit");
    if (!want) return LDPC_OK;
    // batch_iters: ES off was set before the launch; otherwise the largest per-frame count
    return reduce_counter_rows(partials, (T.B + 63) / 64, c.counters, es == LDPC_ES_OFF ? nullptr : c.batch_iters,
                               nullptr, s);
}

}  // namespace ldpc
