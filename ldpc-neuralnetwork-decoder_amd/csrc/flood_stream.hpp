// flood_stream.hpp -- what the streaming translation units share: flood_stream.hip (flooding and hybrid
// min-sum), flood_layered_stream.hip (layered min-sum) and flood_layered_stream_half.hip (its binary16
// form, which borrows the syndrome and emit passes only).  The layout is flood_stream.hip's: every
// array frame-fastest, so that a wave -- 64 consecutive frames of one node -- loads and stores 256
// contiguous bytes.
#pragma once
#include <algorithm>

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

}  // namespace ldpc
