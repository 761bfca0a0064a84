// flood.hip -- LDS-resident flooding min-sum / sum-product decoder for gfx950.
//
// Replaces (bit-for-bit for min-sum, see DESIGN.md "Parity"):
//   MinSumScaledDecoder.decode     traditional_decoders.py:177-260
//   BeliefPropagationDecoder.decode traditional_decoders.py:42-109
//   _check_valid_codeword           traditional_decoders.py:111-134 / 262-285
//
// One workgroup = 4 waves = one "lane vector" of FG = 64/Z frames; every message of those frames
// lives in LDS for the whole decode (layout: graph.hpp).  HBM sees the LLRs once (plus L2 re-reads
// of degree-1 columns) and the decisions once.  Per iteration:
//   check phase  each wave takes whole block-rows (LPT schedule); a lane owns check r*Z+k of
//                frame f, keeps the row's messages in registers (re-reads them past degree 12),
//                writes c2v in place
//   var phase    each wave takes whole columns; a lane owns variable c*Z+t, reads its dv c2v
//                (rotated slot index), writes v2c in place as the reference's ordered sums
//   [ES]         decisions as 64-bit ballots per column in LDS, syndrome per block-row
//
// Exactness: the reference sums/multiplies in float32 in a fixed order.  The var update is
// v2c_i = (((llr + c_0) + c_1) ...) over i' != i in ascending check order; we compute it as the
// prefix P_i followed by the same tail adds, i.e. the identical operation sequence.  Min-sum's
// sign/min is order-free.  BP's exclusive product is prefix-then-tail as well; tanh/atanh are
// float32 approximations of a few ulp (tanh_half / two_atanh in flood_dev.hpp; the reference uses
// torch-CPU SLEEF float versions; neither is correctly rounded, so BP parity is "within float32
// tolerance", not bitwise).
// Compile with -ffp-contract=off: no a*b+c may fuse on this path.
// Translation units: flood_dev.hpp (device code shared by all), flood_fixed_ms.hip / flood_fixed_bp.hip
// (compile-time schedules: flood_fixed.hpp), flood_stream.hip (streaming decoders), flood_layered.hip
// (layered min-sum), flood_layered_stream.hip (layered min-sum on the streaming layout), flood_half.hip
// (half-precision min-sum, two frames per lane), flood_layered_stream_half.hip (half-precision layered
// min-sum on streaming kernels of its own), and this file (table-driven kernel, early-stop passes, host
// dispatch, the C ABI).  Shared by several: flood_stream.hpp (the streaming layout's argument block, min-sum
// row rule, workspace carve and layered host loop), half_pair.hpp (the packed-binary16 pair vocabulary of the
// two half-precision files), flood_host.hpp (their host interfaces), common.hpp (errors, the workspace Arena).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "flood_host.hpp"
#include "half_pair.hpp"

namespace ldpc {

// ---------------------------------------------------------------- batch-global early stop
__global__ void es_init_kernel(int32_t *ctl, uint64_t *staged, uint32_t *all_words) {
    const int t = threadIdx.x;
    if (t < 4) ctl[t] = 0;
    if (t < 4) staged[t] = 0;
    if (t < 64) all_words[t] = ~0u;
}

// fold the per-workgroup counter rows: counters[0..3] += column sums, *batch_iters = max(it) when
// set_iters (ES_FRAME: the largest per-frame count; the fallback: tstar + 1).  gate: run only
// when *gate != 0 (NULL: always).  One workgroup of 1024 threads.
__global__ __launch_bounds__(1024) void counters_reduce_kernel(const uint32_t *__restrict__ partials, int64_t nwg,
                                                               uint64_t *counters, int32_t *batch_iters,
                                                               const int32_t *gate) {
    if (gate && *gate == 0) return;
    uint64_t acc[4] = {0, 0, 0, 0};
    uint32_t mx = 0;
    for (int64_t r = threadIdx.x; r < nwg; r += blockDim.x) {
        const uint32_t *row = partials + r * kPartRow;
        for (int i = 0; i < 4; ++i) acc[i] += row[i];
        mx = max(mx, row[4]);
    }
    for (int off = 32; off > 0; off >>= 1) {
        for (int i = 0; i < 4; ++i) acc[i] += __shfl_xor(acc[i], off, 64);
        mx = max(mx, (uint32_t)__shfl_xor(mx, off, 64));
    }
    __shared__ uint64_t sh[16][5];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int i = 0; i < 4; ++i) sh[w][i] = acc[i];
        sh[w][4] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t t[5] = {0, 0, 0, 0, 0};
        for (int q = 0; q < (int)(blockDim.x >> 6); ++q) {
            for (int i = 0; i < 4; ++i) t[i] += sh[q][i];
            t[4] = max(t[4], sh[q][4]);
        }
        if (counters)
            for (int i = 0; i < 4; ++i) counters[i] += t[i];
        if (batch_iters) *batch_iters = (int32_t)t[4];
    }
}

__global__ void es_finalize_kernel(int32_t *ctl, int max_iter, const uint64_t *staged, uint64_t *counters,
                                   int32_t *batch_iters, int force_fallback) {
    const int T = ctl[0];
    const int fallback = force_fallback || (ctl[1] != 0 && T < max_iter);
    ctl[2] = fallback;
    if (!fallback) {
        if (counters)
            for (int i = 0; i < 4; ++i) counters[i] += staged[i];
        if (batch_iters) *batch_iters = T;
    } else if (batch_iters) {
        *batch_iters = 0;  // batch_emit_kernel takes the max
    }
}

__global__ void batch_and_kernel(const uint32_t *__restrict__ ws_valid, int64_t B, int nvw,
                                 uint32_t *__restrict__ all_words, const int32_t *__restrict__ ctl) {
    if (ctl[2] == 0) return;
    __shared__ uint32_t sh[32];
    if (threadIdx.x < 32) sh[threadIdx.x] = ~0u;
    __syncthreads();
    const int64_t frame = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (frame < B)
        for (int w = 0; w < nvw; ++w) atomicAnd(&sh[w], ws_valid[frame * nvw + w]);
    __syncthreads();
    if (threadIdx.x < nvw) atomicAnd(&all_words[threadIdx.x], sh[threadIdx.x]);
}

__global__ __launch_bounds__(512) void batch_emit_kernel(FloodTables T, const uint64_t *__restrict__ ws_words,
                                                         const uint32_t *__restrict__ all_words, int max_iter,
                                                         int nvw, int64_t B, int out_dtype, void *bits,
                                                         int32_t *iters_out, uint32_t *partials,
                                                         const int32_t *__restrict__ ctl) {
    if (ctl[2] == 0) return;
    __shared__ uint32_t red[2 * 512];
    int tstar = max_iter - 1;  // first iteration at which every frame was valid
    for (int w = 0; w < nvw; ++w) {
        const uint32_t aw = all_words[w];
        if (aw) {
            const int t = w * 32 + __builtin_ctz(aw);
            if (t < max_iter) { tstar = t; break; }
        }
    }
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const Lane L = make_lane(T, nullptr, B);
    Ctx C;
    C.T = T;
    C.out_dtype = out_dtype;
    C.bits = bits;
    int errs = 0;
    emit_from_words(C, L, ws_words + ((int64_t)blockIdx.x * max_iter + tstar) * T.Nb, ~0ull, wave, errs);
    if (iters_out && L.valid && L.k == 0) iters_out[L.frame] = tstar + 1;
    const int nf = (int)min<int64_t>((int64_t)T.FG, B - (int64_t)blockIdx.x * T.FG);
    if (partials) reduce_counters(red, L, errs, tstar + 1, nf, T.Z, partials + (int64_t)blockIdx.x * kPartRow);
}

__global__ void fill_i32_kernel(int32_t *p, int32_t v) { *p = v; }

// the sum-product decoders' two functions on their own (ldpc_bp_math_raw: unit tests)
__global__ __launch_bounds__(256) void bp_math_kernel(const float *__restrict__ x, int64_t n,
                                                      float *__restrict__ th, float *__restrict__ at) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    if (th) th[i] = tanh_half(v);
    if (at) at[i] = two_atanh(v);
}

// Second launch behind a bail-out instance of flood_fixed_kernel (flood_drive, Body::kBail): the
// groups on its redo list are decoded again from their LLRs by the table-driven update, which is
// bit-identical and exact for every value, and get their bits, iteration counts and counter rows
// here.  A fixed small grid strides over the list; with an empty list (no non-finite value in the
// batch: always, on real data) every workgroup leaves at once, so the host never has to look.
template <int ES>
__global__ __launch_bounds__(512) void flood_redo_kernel(FloodTables T, const float *__restrict__ llr, int64_t B,
                                                         int max_iter, float alpha, int out_dtype,
                                                         void *__restrict__ bits, Outs O,
                                                         const uint32_t *__restrict__ redo) {
    static_assert(ES == LDPC_ES_OFF || ES == LDPC_ES_FRAME, "flood_drive returns early in the batch-stop passes");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const uint32_t n = __builtin_amdgcn_readfirstlane(redo[0]);
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const int group = __builtin_amdgcn_readfirstlane(redo[1 + i]);
        const Lane L = make_lane(T, llr, B, group);
        Ctx C;
        init_ctx(C, T, lds, alpha, out_dtype, bits);
        GenericBody<LDPC_ALGO_MINSUM> body{__builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6)};
        flood_drive<ES>(body, C, L, B, max_iter, O, EsWs{});
        __syncthreads();  // the next group's init writes the LDS this one's epilogue reads
    }
}
constexpr unsigned kRedoGrid = 256;  // one workgroup per CU


int reduce_counter_rows(const uint32_t *partials, int64_t nwg, uint64_t *counters, int32_t *batch_iters,
                        const int32_t *gate, hipStream_t s) {
    hipLaunchKernelGGL(counters_reduce_kernel, dim3(1), dim3(1024), 0, s, partials, nwg, counters, batch_iters, gate);
    LDPC_CHECK_LAUNCH("counters_reduce_kernel");
    return LDPC_OK;
}

// ---------------------------------------------------------------- host side
namespace {
constexpr size_t kLdsMax = 160 * 1024;

size_t flood_lds_bytes(const ldpc_graph *g, int es) {
    size_t b = (size_t)g->nslots * 64 * sizeof(float) + 8;  // slots + the NaN flag
    if (es != LDPC_ES_OFF) b += (size_t)(g->Nb + 1) * sizeof(uint64_t);
    return std::max<size_t>(b, 2 * 64 * (size_t)g->ft.W * sizeof(uint32_t));
}

// Workspace: [counter rows: nwg x kPartRow uint32] [redo list: count, nwg x uint32] then, for
// LDPC_ES_BATCH, the EsWs arrays.  base == nullptr only sizes it.
struct FloodWs {
    uint32_t *partials;
    uint32_t *redo;
    EsWs es;
    uint32_t *all;
    int64_t bytes;
};

FloodWs flood_ws(const ldpc_graph *g, int64_t B, int max_iter, int early_stop, void *base) {
    FloodWs w{};
    const int64_t nwg = (B + g->FG - 1) / g->FG;
    Arena a(base);
    w.partials = a.take<uint32_t>(nwg * kPartRow * 4);
    w.redo = a.take<uint32_t>((nwg + 1) * 4);
    if (early_stop == LDPC_ES_BATCH) {
        EsWs &e = w.es;
        e.nvw = (max_iter + 31) / 32;
        e.words = a.take<uint64_t>(nwg * max_iter * g->Nb * 8);
        e.valid = a.take<uint32_t>(B * e.nvw * 4);
        w.all = a.take<uint32_t>(64 * 4);
        e.cand = a.take<uint64_t>(nwg * g->Nb * 8);
        e.twg = a.take<int32_t>(nwg * 4);
        e.ctl = a.take<int32_t>(64);
        e.staged = a.take<uint64_t>(64);
    }
    w.bytes = a.bytes;
    return w;
}

bool use_stream(const ldpc_graph *g, int es) {
    if (!g->lds_ok || flood_lds_bytes(g, es) > kLdsMax) return true;
    const char *e = std::getenv("LDPC_FLOOD_STREAM");  // force the streaming kernels (tests, A/B)
    return e && std::atoi(e) != 0;
}

// the decodes that run a bail-out instance and the redo launch behind it
bool has_redo(const ldpc_graph *g, int algo, int es) {
    return g->fixed_id != 0 && algo == LDPC_ALGO_MINSUM && (es == LDPC_ES_OFF || es == LDPC_ES_FRAME);
}

// redo (has_redo decodes, NULL without a workspace): the redo list of FloodWs
template <int ALGO, int ES>
int launch_flood(const FloodCall &c, const Outs &O, const EsWs &W, uint32_t *redo = nullptr) {
    const ldpc_graph *g = c.g;
    const size_t lds = flood_lds_bytes(g, ES);
    const int64_t nwg = (c.B + g->FG - 1) / g->FG;
    const dim3 block(64 * g->ft.W);
    if (g->fixed_id != 0) {  // compile-time schedules: their own translation units
        if (redo) LDPC_HIP(hipMemsetAsync(redo, 0, sizeof(uint32_t), c.s));
        const int rc = launch_fixed<ALGO>(c, ES, lds, O, W, redo);
        if (rc != LDPC_OK || !redo) return rc;
        if constexpr (ES == LDPC_ES_OFF || ES == LDPC_ES_FRAME) {
            auto again = flood_redo_kernel<ES>;
            LDPC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(again),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            Outs Or = O;
            Or.timeline = nullptr;
            hipLaunchKernelGGL(again, dim3((unsigned)std::min<int64_t>(nwg, kRedoGrid)), block, lds, c.s, g->ft, c.llr,
                               c.B, c.max_iter, c.alpha, c.out_dtype, c.bits, Or, (const uint32_t *)redo);
            LDPC_CHECK_LAUNCH("flood_redo_kernel");
        }
        return LDPC_OK;
    }
    auto kern = flood_kernel<ALGO, ES>;
    LDPC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)nwg), block, lds, c.s, g->ft, c.llr, c.B, c.max_iter, c.alpha,
                       c.out_dtype, c.bits, O, W);
    LDPC_CHECK_LAUNCH("flood_kernel");
    return LDPC_OK;
}

int reduce_rows(const ldpc_graph *g, int64_t B, const uint32_t *partials, uint64_t *counters, int32_t *batch_iters,
                const int32_t *gate, hipStream_t s, int frames_per_wg = 0) {
    if (!counters && !batch_iters) return LDPC_OK;
    const int fg = frames_per_wg > 0 ? frames_per_wg : g->FG;
    const int64_t nwg = (B + fg - 1) / fg;
    return reduce_counter_rows(partials, nwg, counters, batch_iters, gate, s);
}

// the refusals of ldpc_flood_decode that differ only in the decoder's name
int no_batch_stop(const char *name, const char *why = "") {
    return fail(LDPC_EINVAL, std::string(name) + " has no batch-global stop" + why + ": use LDPC_ES_OFF or LDPC_ES_FRAME");
}

int needs_lds_schedule(const char *name, const ldpc_graph *g) {
    return fail(LDPC_EUNSUPPORTED,
                std::string(name) + " needs the LDS-resident schedule, and this graph decodes on the streaming "
                "kernels (lifting Z = " + std::to_string(g->Z) + (g->lds_ok ? "" : ", schedule encoding does not fit") +
                ", or LDPC_FLOOD_STREAM is set)");
}

template <int ALGO>
int run_flood(const FloodCall &c) {
    const ldpc_graph *g = c.g;
    const int64_t B = c.B;
    const int max_iter = c.max_iter, es = c.es;
    hipStream_t s = c.s;
    const FloodWs ws = flood_ws(g, B, max_iter, es, c.work);
    const bool want = c.counters || c.batch_iters;
    const Outs O{c.iters, want ? ws.partials : nullptr};
    uint32_t *redo = has_redo(g, ALGO, es) ? ws.redo : nullptr;
    if (es == LDPC_ES_OFF) {
#ifdef LDPC_TIMELINE
        // timeline build: stamps of the first kTlWgs workgroups, dumped after the decode to
        // $LDPC_TIMELINE_OUT (header: kTlWgs, waves, stamps per wave, max_iter, then uint64 stamps)
        static uint64_t *tl = nullptr;
        const size_t tl_n = (size_t)kTlWgs * 4 * kTlPer;
        if (!tl) LDPC_HIP(hipMalloc(&tl, tl_n * 8));
        LDPC_HIP(hipMemsetAsync(tl, 0, tl_n * 8, s));
        Outs Ot = O;
        Ot.timeline = tl;
        int rc = launch_flood<ALGO, LDPC_ES_OFF>(c, Ot, EsWs{}, redo);
        if (const char *path = std::getenv("LDPC_TIMELINE_OUT")) {
            std::vector<uint64_t> h(tl_n);
            LDPC_HIP(hipStreamSynchronize(s));
            LDPC_HIP(hipMemcpy(h.data(), tl, tl_n * 8, hipMemcpyDeviceToHost));
            if (FILE *f = std::fopen(path, "wb")) {
                const int32_t hdr[4] = {kTlWgs, 4, kTlPer, max_iter};
                std::fwrite(hdr, 4, 4, f);
                std::fwrite(h.data(), 8, h.size(), f);
                std::fclose(f);
            }
        }
#else
        int rc = launch_flood<ALGO, LDPC_ES_OFF>(c, O, EsWs{}, redo);
#endif
        // ES off: every frame ran max_iter (batch_iters was set before the launch)
        return rc != LDPC_OK ? rc : reduce_rows(g, B, ws.partials, c.counters, nullptr, nullptr, s);
    }
    if (es == LDPC_ES_FRAME) {
        int rc = launch_flood<ALGO, LDPC_ES_FRAME>(c, O, EsWs{}, redo);
        return rc != LDPC_OK ? rc : reduce_rows(g, B, ws.partials, c.counters, c.batch_iters, nullptr, s);
    }
    const EsWs &W = ws.es;
    hipLaunchKernelGGL(es_init_kernel, dim3(1), dim3(64), 0, s, W.ctl, W.staged, ws.all);
    LDPC_CHECK_LAUNCH("es_init_kernel");
    LDPC_HIP(hipMemsetAsync(W.valid, 0, (size_t)B * W.nvw * 4, s));
    int rc = launch_flood<ALGO, ES_P1>(c, Outs{}, W);
    if (rc != LDPC_OK) return rc;
    // P2 always writes its counter rows: they become `staged`, applied by es_finalize_kernel
    rc = launch_flood<ALGO, ES_P2>(c, Outs{c.iters, ws.partials}, W);
    if (rc != LDPC_OK) return rc;
    rc = reduce_rows(g, B, ws.partials, W.staged, nullptr, nullptr, s);
    if (rc != LDPC_OK) return rc;
    // LDPC_FLOOD_ES_FALLBACK=1 forces the exhaustive pass (tests: both paths must agree)
    const char *ff = std::getenv("LDPC_FLOOD_ES_FALLBACK");
    hipLaunchKernelGGL(es_finalize_kernel, dim3(1), dim3(1), 0, s, W.ctl, max_iter, W.staged, c.counters,
                       c.batch_iters, (ff && std::atoi(ff) != 0) ? 1 : 0);
    LDPC_CHECK_LAUNCH("es_finalize_kernel");
    // fallback (runs only when es_finalize_kernel found a frame invalid at T)
    rc = launch_flood<ALGO, LDPC_ES_BATCH>(c, Outs{}, W);
    if (rc != LDPC_OK) return rc;
    hipLaunchKernelGGL(batch_and_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, W.valid, B, W.nvw, ws.all,
                       W.ctl);
    LDPC_CHECK_LAUNCH("batch_and_kernel");
    const int64_t nwg = (B + g->FG - 1) / g->FG;
    hipLaunchKernelGGL(batch_emit_kernel, dim3((unsigned)nwg), dim3(64 * g->ft.W), 0, s, g->ft, W.words, ws.all,
                       max_iter, W.nvw, B, c.out_dtype, c.bits, c.iters, want ? ws.partials : nullptr, W.ctl);
    LDPC_CHECK_LAUNCH("batch_emit_kernel");
    return reduce_rows(g, B, ws.partials, c.counters, c.batch_iters, W.ctl + 2, s);
}
}  // namespace

}  // namespace ldpc

using namespace ldpc;

extern "C" int64_t ldpc_flood_workspace_size(const ldpc_graph *g, int64_t B, int max_iter, int early_stop) {
    if (!g || B < 0 || max_iter < 0) return fail(LDPC_EINVAL, "bad arguments");
    if (B == 0 || max_iter == 0) return 0;
    if (use_stream(g, early_stop)) return stream_ws_bytes(g, B, max_iter);
    return flood_ws(g, B, max_iter, early_stop, nullptr).bytes;
}

extern "C" int64_t ldpc_layered_half_workspace_size(const ldpc_graph *g, int64_t B, int max_iter, int early_stop) {
    if (!g || B < 0 || max_iter < 0) return fail(LDPC_EINVAL, "bad arguments");
    if (early_stop < 0 || early_stop > 2) return fail(LDPC_EINVAL, "unknown early_stop mode");
    if (B == 0 || max_iter == 0) return 0;
    return layered_half_ws_bytes(g, B);
}

extern "C" int ldpc_flood_decode(const ldpc_graph *g, int algo, const float *d_llr, int64_t B,
                                 int max_iter, float alpha, int early_stop, int out_dtype,
                                 void *d_bits, int32_t *d_iters, int32_t *d_batch_iters,
                                 uint64_t *d_counters, void *d_work, int64_t work_bytes, void *stream) {
    if (!g) return fail(LDPC_EINVAL, "graph is NULL");
    if (algo != LDPC_ALGO_MINSUM && algo != LDPC_ALGO_BP && algo != LDPC_ALGO_LAYERED_MINSUM &&
        algo != LDPC_ALGO_LAYERED_MINSUM_ANY && algo != LDPC_ALGO_MINSUM_F16 && algo != LDPC_ALGO_LAYERED_MINSUM_F16)
        return fail(LDPC_EINVAL, "unknown algo");
    const bool layered = algo == LDPC_ALGO_LAYERED_MINSUM || algo == LDPC_ALGO_LAYERED_MINSUM_ANY;
    const bool half = algo == LDPC_ALGO_MINSUM_F16;
    const bool layered_half = algo == LDPC_ALGO_LAYERED_MINSUM_F16;
    if (early_stop < 0 || early_stop > 2) return fail(LDPC_EINVAL, "unknown early_stop mode");
    if (out_dtype != LDPC_OUT_U8 && out_dtype != LDPC_OUT_F32) return fail(LDPC_EINVAL, "unknown out_dtype");
    if (B < 0) return fail(LDPC_EINVAL, "negative batch");
    if (max_iter < 1 || max_iter > 1024) return fail(LDPC_EINVAL, "max_iter must be in [1, 1024]");
    if (early_stop == LDPC_ES_BATCH) {
        if (layered) return no_batch_stop("layered min-sum", " (LDPC_ES_BATCH mirrors the reference's flooding classes)");
        if (half) return no_batch_stop("half-precision min-sum");
        if (layered_half) return no_batch_stop("half-precision layered min-sum");
    }
    if (half || layered_half) {
        const uint32_t a = half_alpha_bits(alpha);  // 0 <= half(alpha) <= 1 (a NaN fails both)
        if (!(a <= 0x3c00u || a == 0x8000u))
            return fail(LDPC_EINVAL, "half-precision min-sum: alpha rounded to binary16 must be in [0, 1]");
    }
    if (B == 0) return LDPC_OK;
    if (!d_llr || !d_bits) return fail(LDPC_EINVAL, "llr / bits is NULL");
    if (layered_half) {
        // streaming kernels of its own on every graph: neither LDPC_FLOOD_STREAM nor the variant matters
        if (g->max_dv > kStreamMaxDeg || g->max_dc > kStreamMaxDeg)
            return fail(LDPC_EUNSUPPORTED, "half-precision layered min-sum: node degree above " + std::to_string(kStreamMaxDeg));
        const int64_t need = layered_half_ws_bytes(g, B);
        if (!d_work || work_bytes < need)
            return fail(LDPC_EINVAL, "workspace too small: need " + std::to_string(need) +
                                         " bytes (ldpc_layered_half_workspace_size)");
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (d_batch_iters && early_stop == LDPC_ES_OFF) {
            hipLaunchKernelGGL(fill_i32_kernel, dim3(1), dim3(1), 0, s, d_batch_iters, max_iter);
            LDPC_CHECK_LAUNCH("fill");
        }
        return run_layered_stream_half(FloodCall{g, d_llr, B, max_iter, alpha, early_stop, out_dtype, d_bits, d_iters,
                                                 d_counters, d_batch_iters, d_work, s});
    }
    const bool streaming = use_stream(g, early_stop);
    // LDPC_ALGO_LAYERED_MINSUM_ANY on a streaming graph: the streaming layered decoder, one launch per layer
    // segment (flood_layered_stream.hip); elsewhere it is LDPC_ALGO_LAYERED_MINSUM, refusals included (the
    // workspace query sizes the LDS-resident decoders' scratch there, not the streaming arrays)
    const bool layered_stream = algo == LDPC_ALGO_LAYERED_MINSUM_ANY && streaming;
    if (layered && !layered_stream) {
        // LDS-resident only
        if (streaming) return needs_lds_schedule("layered min-sum", g);
        if (!g->lt.prog || layered_lds_bytes(g, early_stop) > kLdsMax)
            return fail(LDPC_EUNSUPPORTED, "layered min-sum: posteriors and messages of one wave's frames need " +
                                               std::to_string(layered_lds_bytes(g, early_stop)) + " bytes of LDS, above " +
                                               std::to_string(kLdsMax));
    }
    if (half) {
        // LDS-resident only; no partial sum may overflow binary16: 33 * 1024 < 65504
        if (streaming) return needs_lds_schedule("half-precision min-sum", g);
        if (g->max_dv > 32)
            return fail(LDPC_EUNSUPPORTED, "half-precision min-sum: variable degree " + std::to_string(g->max_dv) + " above 32");
        if (half_lds_bytes(g) > kLdsMax)
            return fail(LDPC_EUNSUPPORTED, "half-precision min-sum: messages and ballots of one workgroup's frames need " +
                                               std::to_string(half_lds_bytes(g)) + " bytes of LDS, above " +
                                               std::to_string(kLdsMax));
    }
    if (streaming && (g->max_dv > kStreamMaxDeg || g->max_dc > kStreamMaxDeg))
        return fail(LDPC_EUNSUPPORTED, "streaming decoder: node degree above " + std::to_string(kStreamMaxDeg));
    // scratch is needed by the streaming decoder, the batch-global stop and any counter output
    const int64_t need = ldpc_flood_workspace_size(g, B, max_iter, early_stop);
    if (!d_work || work_bytes < need) {
        if (streaming || early_stop == LDPC_ES_BATCH || d_counters || (d_batch_iters && early_stop == LDPC_ES_FRAME))
            return fail(LDPC_EINVAL, "workspace too small: need " + std::to_string(need) + " bytes");
        d_work = nullptr;  // not required: the fixed min-sum kernels then keep their exact check update inside
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (d_batch_iters && early_stop == LDPC_ES_OFF) {
        hipLaunchKernelGGL(fill_i32_kernel, dim3(1), dim3(1), 0, s, d_batch_iters, max_iter);
        LDPC_CHECK_LAUNCH("fill");
    }
    const FloodCall c{g, d_llr, B, max_iter, alpha, early_stop, out_dtype, d_bits, d_iters, d_counters, d_batch_iters,
                      d_work, s};
    if (layered_stream) return run_layered_stream(c);
    if (layered) return run_layered(c);
    if (half) return run_half(c);
    if (streaming) return run_stream_decode(algo, c);
    return algo == LDPC_ALGO_MINSUM ? run_flood<LDPC_ALGO_MINSUM>(c) : run_flood<LDPC_ALGO_BP>(c);
}

extern "C" int ldpc_flood_redo_count(const ldpc_graph *g, int algo, int64_t B, int max_iter, int early_stop,
                                     const void *d_work, void *stream, int32_t *h_count, int32_t *h_groups) {
    if (!g || !d_work || !h_count || B <= 0 || max_iter < 1) return fail(LDPC_EINVAL, "bad arguments");
    if (use_stream(g, early_stop) || !has_redo(g, algo, early_stop))
        return fail(LDPC_EUNSUPPORTED, "this decode keeps no redo list (min-sum on a compile-time schedule, "
                                       "LDPC_ES_OFF or LDPC_ES_FRAME, only)");
    const FloodWs ws = flood_ws(g, B, max_iter, early_stop, const_cast<void *>(d_work));
    uint32_t n = 0;
    LDPC_HIP(hipMemcpyAsync(&n, ws.redo, sizeof n, hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
    LDPC_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    *h_count = (int32_t)n;
    if (h_groups && n > 0) {
        if ((int64_t)n > (B + g->FG - 1) / g->FG) return fail(LDPC_EINVAL, "d_work holds no redo list of this decode");
        LDPC_HIP(hipMemcpy(h_groups, ws.redo + 1, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return LDPC_OK;
}

extern "C" int ldpc_bp_math_raw(const float *d_x, int64_t n, float *d_tanh_half, float *d_two_atanh, void *stream) {
    if (n < 0 || n > 2147483647LL * 256) return fail(LDPC_EINVAL, "bad n");
    if (n == 0) return LDPC_OK;
    if (!d_x || (!d_tanh_half && !d_two_atanh)) return fail(LDPC_EINVAL, "x / both outputs are NULL");
    hipLaunchKernelGGL(bp_math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), d_x, n, d_tanh_half, d_two_atanh);
    LDPC_CHECK_LAUNCH("bp_math_kernel");
    return LDPC_OK;
}

extern "C" int64_t ldpc_custom_minsum_workspace_size(const ldpc_graph *g, int64_t B) {
    if (!g || B < 0) return fail(LDPC_EINVAL, "bad arguments");
    return B == 0 ? 0 : custom_ws_bytes(g, B);
}

extern "C" int ldpc_custom_minsum_decode(const ldpc_graph *g, const float *d_llr, int64_t B, int iterations,
                                         float *d_probs, void *d_work, int64_t work_bytes, void *stream) {
    if (!g) return fail(LDPC_EINVAL, "graph is NULL");
    if (B < 0) return fail(LDPC_EINVAL, "negative batch");
    if (iterations < 0 || iterations > 1024) return fail(LDPC_EINVAL, "iterations must be in [0, 1024]");
    if (B == 0) return LDPC_OK;
    if (B > 65535LL * 64) return fail(LDPC_EUNSUPPORTED, "batch above 4194240 frames in one call (chunk it)");
    if (!d_llr || !d_probs) return fail(LDPC_EINVAL, "llr / probs is NULL");
    if (g->max_dv > kStreamMaxDeg || g->max_dc > kStreamMaxDeg)
        return fail(LDPC_EUNSUPPORTED, "node degree above " + std::to_string(kStreamMaxDeg));
    const int64_t need = custom_ws_bytes(g, B);
    if (!d_work || work_bytes < need) return fail(LDPC_EINVAL, "workspace too small: need " + std::to_string(need) + " bytes");
    return run_custom_minsum(g, d_llr, B, iterations, d_probs, d_work, static_cast<hipStream_t>(stream));
}
