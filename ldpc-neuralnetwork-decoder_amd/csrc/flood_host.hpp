// flood_host.hpp -- host-side interfaces between the flood*.hip translation units.
#pragma once
#include <cstddef>
#include <cstdint>

#include "flood_dev.hpp"

namespace ldpc {

constexpr int kStreamMaxDeg = 32;  // register windows of stream_check_kernel / stream_var_kernel

// flood.hip: fold per-workgroup counter rows (counters_reduce_kernel)
int reduce_counter_rows(const uint32_t *partials, int64_t nwg, uint64_t *counters, int32_t *batch_iters,
                        const int32_t *gate, hipStream_t s);

// One decode as ldpc_flood_decode has checked it: the arguments every flooding / layered / streaming
// path takes (device pointers; work may be NULL where the path needs none).
struct FloodCall {
    const ldpc_graph *g;
    const float *llr;
    int64_t B;
    int max_iter;
    float alpha;
    int es;  // the caller's early_stop: LDPC_ES_OFF / LDPC_ES_BATCH / LDPC_ES_FRAME
    int out_dtype;
    void *bits;
    int32_t *iters;
    uint64_t *counters;
    int32_t *batch_iters;
    void *work;
    hipStream_t s;
};

// flood_fixed.hpp, instantiated by flood_fixed_ms.hip (min-sum) and flood_fixed_bp.hip (BP):
// flood_fixed_kernel<code, ALGO, es> for fixed_id 1 (BG2 Z=4) or 2 (BG2 Z=32), es one of LDPC_ES_OFF /
// LDPC_ES_FRAME / LDPC_ES_BATCH / ES_P1 / ES_P2 (the pass to launch, not c.es), lds its dynamic LDS.
// redo (min-sum, LDPC_ES_OFF / LDPC_ES_FRAME only; NULL otherwise): [0] a count the caller has zeroed,
// [1 ..] room for one entry per workgroup.  With it the kernel holds the fast check update only: a
// workgroup that meets a non-finite value appends its index and writes no counter row, and the
// caller decodes the listed groups again with the table-driven kernel (flood.hip launch_flood).
template <int ALGO>
int launch_fixed(const FloodCall &c, int es, size_t lds, const Outs &O, const EsWs &W, uint32_t *redo);

// flood_layered.hip: layered min-sum (LDS-resident only; c.es is LDPC_ES_OFF or LDPC_ES_FRAME).  c.work holds
// the counter rows, one per FG frames: the head of the flooding workspace of the same arguments.
size_t layered_lds_bytes(const ldpc_graph *g, int es);
int run_layered(const FloodCall &c);

// flood_layered_stream.hip: layered min-sum on the streaming layout (any graph with check degrees up to
// kStreamMaxDeg; c.es is LDPC_ES_OFF or LDPC_ES_FRAME).  c.work is the streaming workspace (stream_ws_bytes).
int run_layered_stream(const FloodCall &c);

// flood_half.hip: half-precision min-sum (LDPC_ALGO_MINSUM_F16; LDS-resident only, c.es is LDPC_ES_OFF or
// LDPC_ES_FRAME, c.alpha already checked).  c.work holds the counter rows, one per 2 * FG frames: the head
// of the flooding workspace of the same arguments.  (half_alpha_bits, which checks c.alpha: half_pair.hpp.)
size_t half_lds_bytes(const ldpc_graph *g);
int run_half(const FloodCall &c);

// flood_layered_stream_half.hip: half-precision layered min-sum (LDPC_ALGO_LAYERED_MINSUM_F16) on streaming
// kernels of its own, any graph with node degrees up to kStreamMaxDeg; c.es is LDPC_ES_OFF or LDPC_ES_FRAME,
// c.alpha already checked.  c.work holds layered_half_ws_bytes(g, B) bytes, always.
int64_t layered_half_ws_bytes(const ldpc_graph *g, int64_t B);
int run_layered_stream_half(const FloodCall &c);

// flood_stream.hip: the streaming decoders (messages in HBM, any graph)
int64_t stream_ws_bytes(const ldpc_graph *g, int64_t B, int max_iter);
int run_stream_decode(int algo, const FloodCall &c);
int64_t custom_ws_bytes(const ldpc_graph *g, int64_t B);
int run_custom_minsum(const ldpc_graph *g, const float *llr, int64_t B, int iterations, float *probs, void *work,
                      hipStream_t s);

}  // namespace ldpc
