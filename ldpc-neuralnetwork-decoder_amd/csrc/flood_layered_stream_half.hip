// flood_layered_stream_half.hip -- LDPC_ALGO_LAYERED_MINSUM_F16: layered (row-serial) scaled min-sum on IEEE
// binary16 messages and posteriors, every one of them in HBM, any graph, two frames per lane on packed f16
// math (v_pk_add_f16 / v_pk_mul_f16 / v_pk_minimum3_f16 / v_pk_maximum3_f16), for gfx950.
//
// The algorithm is the contract written in include/ldpc_amd.h ("Half-precision layered min-sum"); the numpy
// restatement the tests hold it to is tests/layered_half_ref.py.  C = 1024:
//     t_k      = clamp(app[j_k] - c2v[i,k], +-C)      (a degree-1 variable: t_k = x[j_k] exactly)
//     c2v[i,k] = prod_{q != k} sgn(t_q) * (a * min(C, min_{q != k} |t_q|))
//     app[j_k] = t_k + c2v[i,k]                       (unclamped)
// for the checks in ascending index, and bit[v] = app[v] < 0 after a full iteration.
//
// Schedule: flood_layered_stream.hip's.  The runs and degree segments graph.cpp builds for every graph
// (lay_seg, lay_order, ext_var), one launch per segment in stream order, FIRST (iteration 1) reading no c2v.
//
// Layout: binary16, frame-fastest, with a row stride Bs = B rounded up to a multiple of 128 frames, so that
// every row starts 256-byte aligned.
//     msgH[E][Bs]  c2v.  Never zero-filled: iteration 1 reads none (c2v = +0 there, so t = clamp(app); the
//                  clamp stays, since app passes C once earlier checks of the iteration have added to x).
//     appH[N][Bs]  for a variable of degree != 1 the posterior, updated in place; for a degree-1 variable
//                  x = clamp(half(llr)), for good.  The pad frames B .. Bs - 1 are written 0 by the transpose.
//     bitsT[N][B] uint8, done[B], iters[B], partials: as the float32 streaming decoders use them, so
//                  flood_stream.hip's syndrome and emit passes run as they are on a StreamArgs carrying B.
//
// Pairing.  A thread is one (check, pair of frames): frames 2p and 2p + 1 are the low and high half of one
// dword, ONE aligned 4-byte load from the frame-fastest arrays.  A wave is 128 consecutive frames of one
// check and moves 256 contiguous bytes per message.  The two halves of a dword never meet: every operation
// on messages is a packed (per-half) f16 operation or a bitwise one, and decisions are a compare per half,
// so a NaN in one frame cannot reach its partner.
//
// Per-frame stop under pairing.  A thread runs while at least one of its two frames exists and is not
// frozen.  A frozen frame's bitsT bytes are never written again (every decision store is masked per half;
// its iters entry and done flag are the syndrome pass's, which skips a frozen frame), while its half of
// msgH / appH keeps evolving with its partner: nothing reads that half any more.  The same holds for the pad
// frame that rides with frame B - 1 when B is odd: it computes on zeros and reaches no output.
//
// Why race-free: as in flood_layered_stream.hip.  Within a launch two threads either share the check (and
// differ in the pair) or lie in two checks of one run, which share no variable and no edge, so they touch
// disjoint dwords; launches on one stream run in order.
// Compile with -ffp-contract=off (the Makefile's default): no multiply-add may fuse.
#include <algorithm>
#include <string>

#include "flood_stream.hpp"
#include "half_pair.hpp"

namespace ldpc {

namespace {

constexpr int kPairFrames = 128;  // frames of a wave: the row stride is a multiple of it

struct HalfArgs {
    const int32_t *chk_ptr, *ev, *var_ptr, *ext_var;
    int N;
    int64_t B;        // frames
    int64_t Bw;       // row stride in dwords (pairs): Bs / 2
    uint32_t *msgW;   // msgH[E][Bs] as dwords
    uint32_t *appW;   // appH[N][Bs] as dwords
    uint8_t *bitsT;   // [N][B]
    const uint8_t *done;  // [B] LDPC_ES_FRAME: frame frozen
    uint32_t a2;      // half(alpha) in both halves
    int es;
};

// which of the pair's two frames exist and still run; false: the thread has nothing to do
__device__ __forceinline__ bool pair_live(const HalfArgs &S, int64_t p, bool (&live)[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int64_t b = 2 * p + h;
        live[h] = b < S.B;
        if (live[h] && S.es == LDPC_ES_FRAME) live[h] = S.done[b] == 0;
    }
    return live[0] || live[1];
}

}  // namespace

// (B, N) float32 -> appH[N][Bs]: x = clamp(half(llr)), nearest-even (v_cvt_pk_f16_f32); pad frames 0.
// 64 x 64 LDS tiles; a thread of the store phase writes one pair of frames.
__global__ __launch_bounds__(256) void layered_half_transpose_kernel(const float *__restrict__ llr, int64_t B, int N,
                                                                     int64_t Bw, uint32_t *__restrict__ appW) {
    __shared__ float t[64][65];
    const int64_t b0 = (int64_t)blockIdx.x * 64;  // b0 + 64 <= 2 * Bw: the stride is a multiple of 128 frames
    const int v0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) t[r][tx] = (b0 + r < B && v0 + tx < N) ? llr[(b0 + r) * N + v0 + tx] : 0.0f;
    __syncthreads();
    const HConst K = make_const(0);
    const int px = threadIdx.x & 31, py = threadIdx.x >> 5;
    for (int r = py; r < 64; r += 8) {
        if (v0 + r >= N) continue;
        h2 x;
        x.x = (_Float16)t[2 * px][r];
        x.y = (_Float16)t[2 * px + 1][r];
        appW[(int64_t)(v0 + r) * Bw + (b0 >> 1) + px] = as_u(hclamp(K, x));
    }
}

// one (check, pair of frames) of a segment of degree DC; FIRST: iteration 1
template <int DC, bool FIRST>
__global__ __launch_bounds__(256) void layered_half_kernel(HalfArgs S, const int32_t *__restrict__ rows) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // grid: (pairs, checks)
    if (2 * p >= S.B) return;
    bool live[2];
    if (!pair_live(S, p, live)) return;
    const HConst K = make_const(S.a2);
    const int e0 = S.chk_ptr[rows[blockIdx.y]];
    // the row's variables and degree-1 marks: wave-uniform, read once before any store of this kernel and held
    // in SGPRs (read again behind a store through another pointer they would be one vector load per use)
    int ev[DC], xv[DC];
#pragma unroll
    for (int e = 0; e < DC; ++e) {
        ev[e] = S.ev[e0 + e];
        xv[e] = S.ext_var[e0 + e];
    }
    // Every load of the row is issued before the first use, with no branch between them.  A degree-1
    // variable's edge has no message: its load goes to the posterior's dword again (a cache hit, no new
    // bytes) and a wave-uniform select puts +0 in its place: x - (+0) = x exactly, and clamp(x) = x.
    uint32_t t[DC], m[DC];
#pragma unroll
    for (int e = 0; e < DC; ++e) {
        const uint32_t *app = S.appW + (int64_t)ev[e] * S.Bw;
        t[e] = app[p];
        if constexpr (!FIRST) m[e] = (xv[e] < 0 ? S.msgW + (int64_t)(e0 + e) * S.Bw : app)[p];
    }
    // FIRST: c2v = +0, so t = clamp(app - (+0)) = clamp(app).  The clamp stays: app is x only until an earlier
    // check of this iteration has added its c2v, and then may pass C.
#pragma unroll
    for (int e = 0; e < DC; ++e) {
        if constexpr (FIRST)
            t[e] = as_u(hclamp(K, as_h(t[e])));
        else
            t[e] = as_u(hclamp(K, as_h(t[e]) - as_h(xv[e] < 0 ? m[e] : 0u)));
    }
    // the minimum starts at C, not at +inf ("Half-precision layered min-sum", include/ldpc_amd.h): every |t| <= C,
    // so a degree-1 check sends +a * C and nothing is ever infinite.  The flooding form's is +inf (half_pair.hpp).
    uint32_t c[DC];
    half_check_rule<DC>(K, t, c, as_h(K.cpos));
#pragma unroll
    for (int e = 0; e < DC; ++e) {
        const h2 app = as_h(t[e]) + as_h(c[e]);
        if (xv[e] < 0) {
            S.msgW[(int64_t)(e0 + e) * S.Bw + p] = c[e];
            S.appW[(int64_t)ev[e] * S.Bw + p] = as_u(app);
        } else {  // degree-1 variable: app = x + c2v is a decision only
            const int64_t xb = (int64_t)xv[e] * S.B + 2 * p;
            if (live[0]) S.bitsT[xb] = app.x < (_Float16)0.0f;
            if (live[1]) S.bitsT[xb + 1] = app.y < (_Float16)0.0f;
        }
    }
}

// decisions of the variables of degree != 1 (degree 0: appH is x): bit = app < 0 per half, NaN -> 0
__global__ __launch_bounds__(256) void layered_half_decide_kernel(HalfArgs S, int j0) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // grid: (pairs, variables)
    const int j = j0 + blockIdx.y;
    if (S.var_ptr[j + 1] - S.var_ptr[j] == 1) return;  // taken by its check's thread
    if (2 * p >= S.B) return;
    bool live[2];
    if (!pair_live(S, p, live)) return;
    const h2 app = as_h(S.appW[(int64_t)j * S.Bw + p]);
    const int64_t jb = (int64_t)j * S.B + 2 * p;
    if (live[0]) S.bitsT[jb] = app.x < (_Float16)0.0f;  // a real compare: -0 is not negative
    if (live[1]) S.bitsT[jb + 1] = app.y < (_Float16)0.0f;
}

namespace {

struct HalfWs {
    uint32_t *msgW, *appW;
    uint8_t *bitsT, *done;
    int32_t *iters;
    uint32_t *partials;
    int64_t Bw, bytes;
};

// base == nullptr only sizes it
HalfWs half_ws(const ldpc_graph *g, int64_t B, void *base) {
    HalfWs w{};
    const int64_t Bs = (B + kPairFrames - 1) / kPairFrames * kPairFrames;
    w.Bw = Bs / 2;
    Arena a(base);
    w.msgW = a.take<uint32_t>(g->E * Bs * 2);
    w.appW = a.take<uint32_t>(g->N * Bs * 2);
    w.bitsT = a.take<uint8_t>(g->N * B);
    w.done = a.take<uint8_t>(B);
    w.iters = a.take<int32_t>(B * 4);
    w.partials = a.take<uint32_t>((B + 63) / 64 * kPartRow * 4);
    w.bytes = a.bytes;
    return w;
}

template <bool FIRST>
void launch_layers(const ldpc_graph *g, const HalfArgs &S, hipStream_t s) {
    per_segment(g, (unsigned)(((S.B + 1) / 2 + 255) / 256), [&](int d, dim3 grid, const int32_t *rows) {
        switch (d) {  // degree 0: nothing to update; degrees above 32 are refused on the host
#define X(k) case k: hipLaunchKernelGGL((layered_half_kernel<k, FIRST>), grid, dim3(256), 0, s, S, rows); break;
            LDPC_STREAM_DEG_CASES(X)
#undef X
            default: break;
        }
    });
}

}  // namespace

int64_t layered_half_ws_bytes(const ldpc_graph *g, int64_t B) { return half_ws(g, B, nullptr).bytes; }

int run_layered_stream_half(const FloodCall &c) {
    const ldpc_graph *g = c.g;
    const int64_t B = c.B;
    hipStream_t s = c.s;
    const HalfWs w = half_ws(g, B, c.work);
    const uint32_t a = half_alpha_bits(c.alpha);
    const HalfArgs S{g->chk_ptr, g->ev, g->var_ptr, g->ext_var, g->N, B, w.Bw, w.msgW, w.appW, w.bitsT, w.done,
                     a | (a << 16), c.es};
    // the float32 streaming decoders' passes read only the graph, B, bitsT, done, iters and es of this
    const StreamArgs T = make_stream_args(g, B, c.alpha, c.es, nullptr, nullptr, w.bitsT, w.done, w.iters, nullptr,
                                          nullptr, g->ext_var);
    const unsigned gx = (unsigned)(((B + 1) / 2 + 255) / 256);
    return layered_stream_drive(
        c, T, w.partials, "half layered stream",
        [&]() -> int {
            const dim3 tgrid((unsigned)(2 * w.Bw / 64), (unsigned)((g->N + 63) / 64));
            hipLaunchKernelGGL(layered_half_transpose_kernel, tgrid, dim3(256), 0, s, c.llr, B, g->N, w.Bw, w.appW);
            LDPC_CHECK_LAUNCH("half layered stream transpose");
            return LDPC_OK;
        },
        [&](bool first) { first ? launch_layers<true>(g, S, s) : launch_layers<false>(g, S, s); },
        [&] {
            for (int j0 = 0; j0 < g->N; j0 += kGridY)
                hipLaunchKernelGGL(layered_half_decide_kernel, dim3(gx, (unsigned)std::min(kGridY, g->N - j0)),
                                   dim3(256), 0, s, S, j0);
        });
}

}  // namespace ldpc
