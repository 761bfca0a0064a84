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

namespace ldpc {

namespace {

typedef _Float16 h2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ h2 as_h(uint32_t u) { return __builtin_bit_cast(h2, u); }
__device__ __forceinline__ uint32_t as_u(h2 h) { return __builtin_bit_cast(uint32_t, h); }
// IEEE minimum / maximum: one v_pk_minimum3_f16 / v_pk_maximum3_f16, no canonicalising v_pk_max
__device__ __forceinline__ h2 hmin(h2 a, h2 b) { return __builtin_elementwise_minimum(a, b); }
__device__ __forceinline__ h2 hmax(h2 a, h2 b) { return __builtin_elementwise_maximum(a, b); }

constexpr uint32_t kSign2 = 0x80008000u, kAbs2 = 0x7fff7fffu;
constexpr uint32_t kClampPos2 = 0x64006400u, kClampNeg2 = 0xe400e400u;  // +-1024
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

// uniform constants in VGPRs (a VALU op with an SGPR source issues at half rate)
struct HConst {
    uint32_t a2, cpos, cneg, sign, absm;
};
__device__ __forceinline__ HConst make_const(uint32_t a2) {
    return HConst{opaque_vu(a2), opaque_vu(kClampPos2), opaque_vu(kClampNeg2), opaque_vu(kSign2), opaque_vu(kAbs2)};
}
__device__ __forceinline__ h2 hclamp(const HConst &K, h2 v) { return hmin(hmax(v, as_h(K.cneg)), as_h(K.cpos)); }

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

// out = sign | magnitude: prod >= +0 (a >= 0, min >= 0), so its sign bits are free for the parity
__device__ __forceinline__ uint32_t signed_c2v(const HConst &K, uint32_t par, uint32_t v, h2 excl_min) {
    const uint32_t prod = as_u(as_h(K.a2) * excl_min);  // rounded once
    return ((par ^ v) & K.sign) | prod;
}

// The check rule on a row of packed halves held in registers.  The minimum starts at C: every |t| <= C, so
// that changes nothing for DC >= 2 and makes a degree-1 check send +a * C.  sgn(0) = 0 needs no code: if
// another message of the row is zero the exclusive minimum is 0 and the result is a zero whatever its sign,
// and if only t_k itself is zero its sign bit cancels in the XOR.
template <int DC>
__device__ __forceinline__ void hcheck_rule(const HConst &K, const uint32_t (&v)[DC], uint32_t (&out)[DC]) {
    uint32_t par = v[0];
#pragma unroll
    for (int e = 1; e < DC; ++e) par ^= v[e];
    if constexpr (DC == 1) {
        out[0] = signed_c2v(K, par, v[0], as_h(K.cpos));  // the empty minimum
    } else if constexpr (DC <= 12) {
        // exclusive minimum of the magnitudes: prefix and suffix minima
        h2 pre[DC], suf[DC];
        pre[0] = as_h(v[0] & K.absm);
#pragma unroll
        for (int e = 1; e < DC; ++e) pre[e] = hmin(pre[e - 1], as_h(v[e] & K.absm));
        suf[DC - 1] = as_h(v[DC - 1] & K.absm);
#pragma unroll
        for (int e = DC - 2; e >= 0; --e) suf[e] = hmin(suf[e + 1], as_h(v[e] & K.absm));
#pragma unroll
        for (int e = 0; e < DC; ++e) {
            h2 m;
            if (e == 0)
                m = suf[1];
            else if (e == DC - 1)
                m = pre[DC - 2];
            else
                m = hmin(pre[e - 1], suf[e + 1]);
            out[e] = signed_c2v(K, par, v[e], m);
        }
    } else {
        // the row's two smallest magnitudes in a first pass, the exclusive minimum chosen per half in a second
        // (the excluded minimum is m2 exactly when |v| == m1: a tie at m1 puts m1 in m2 as well)
        h2 m1 = as_h(K.cpos), m2 = as_h(K.cpos);
#pragma unroll
        for (int e = 0; e < DC; ++e) {
            const h2 a = as_h(v[e] & K.absm);
            m2 = hmin(m2, hmax(m1, a));
            m1 = hmin(m1, a);
        }
#pragma unroll
        for (int e = 0; e < DC; ++e) {
            const h2 a = as_h(v[e] & K.absm);
            h2 m;
            m.x = a.x == m1.x ? m2.x : m1.x;
            m.y = a.y == m1.y ? m2.y : m1.y;
            out[e] = signed_c2v(K, par, v[e], m);
        }
    }
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
    uint32_t c[DC];
    hcheck_rule<DC>(K, t, c);
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
    char *p = static_cast<char *>(base);
    size_t off = 0;
    auto take = [&](size_t n) { char *q = p ? p + off : nullptr; off += align256(n); return q; };
    w.msgW = reinterpret_cast<uint32_t *>(take((size_t)g->E * Bs * 2));
    w.appW = reinterpret_cast<uint32_t *>(take((size_t)g->N * Bs * 2));
    w.bitsT = reinterpret_cast<uint8_t *>(take((size_t)g->N * B));
    w.done = reinterpret_cast<uint8_t *>(take((size_t)B));
    w.iters = reinterpret_cast<int32_t *>(take((size_t)B * 4));
    w.partials = reinterpret_cast<uint32_t *>(take((size_t)((B + 63) / 64) * kPartRow * 4));
    w.bytes = (int64_t)off;
    return w;
}

template <bool FIRST>
void launch_layers(const ldpc_graph *g, const HalfArgs &S, hipStream_t s) {
    const unsigned gx = (unsigned)(((S.B + 1) / 2 + 255) / 256);
    for (size_t q = 0; q + 3 < g->lay_seg.size(); q += 4) {  // {run, degree, offset, count}: runs ascending
        const int d = g->lay_seg[q + 1], n = g->lay_seg[q + 3];
        for (int k0 = 0; k0 < n; k0 += kGridY) {
            const dim3 grid(gx, (unsigned)std::min(kGridY, n - k0));
            const int32_t *rows = g->lay_order + g->lay_seg[q + 2] + k0;
            switch (d) {  // degree 0: nothing to update; degrees above 32 are refused on the host
#define X(k) case k: hipLaunchKernelGGL((layered_half_kernel<k, FIRST>), grid, dim3(256), 0, s, S, rows); break;
                LDPC_STREAM_DEG_CASES(X)
#undef X
                default: break;
            }
        }
    }
}

}  // namespace

int64_t layered_half_ws_bytes(const ldpc_graph *g, int64_t B) { return half_ws(g, B, nullptr).bytes; }

int run_layered_stream_half(const FloodCall &c) {
    const ldpc_graph *g = c.g;
    const int64_t B = c.B;
    const int max_iter = c.max_iter, es = c.es;
    hipStream_t s = c.s;
    const HalfWs w = half_ws(g, B, c.work);
    const uint32_t a = half_alpha_bits(c.alpha);
    const HalfArgs S{g->chk_ptr, g->ev, g->var_ptr, g->ext_var, g->N, B, w.Bw, w.msgW, w.appW, w.bitsT, w.done,
                     a | (a << 16), es};
    // the float32 streaming decoders' passes read only the graph, B, bitsT, done, iters and es of this
    StreamArgs T{};
    T.chk_ptr = g->chk_ptr; T.ev = g->ev; T.var_ptr = g->var_ptr; T.var_edge = g->var_edge;
    T.M = g->M; T.N = g->N; T.E = g->E; T.B = B;
    T.bitsT = w.bitsT; T.done = w.done; T.iters = w.iters;
    T.alpha = c.alpha; T.es = es; T.ext_var = g->ext_var;
    LDPC_HIP(hipMemsetAsync(w.done, 0, (size_t)B, s));
    const dim3 tgrid((unsigned)(2 * w.Bw / 64), (unsigned)((g->N + 63) / 64));
    hipLaunchKernelGGL(layered_half_transpose_kernel, tgrid, dim3(256), 0, s, c.llr, B, g->N, w.Bw, w.appW);
    LDPC_CHECK_LAUNCH("half layered stream transpose");
    const unsigned gx = (unsigned)(((B + 1) / 2 + 255) / 256);
    for (int it = 0; it < max_iter; ++it) {
        if (it == 0)
            launch_layers<true>(g, S, s);
        else
            launch_layers<false>(g, S, s);
        if (es == LDPC_ES_FRAME || it == max_iter - 1) {
            for (int j0 = 0; j0 < g->N; j0 += kGridY)
                hipLaunchKernelGGL(layered_half_decide_kernel, dim3(gx, (unsigned)std::min(kGridY, g->N - j0)),
                                   dim3(256), 0, s, S, j0);
            if (es == LDPC_ES_FRAME) launch_stream_syndrome(T, it, s);
        }
        LDPC_CHECK_LAUNCH("half layered stream iteration");
    }
    const bool want = c.counters || c.batch_iters;
    launch_stream_emit(T, max_iter, c.out_dtype, c.bits, c.iters, want ? w.partials : nullptr, s);
    LDPC_CHECK_LAUNCH("half layered stream emit");
    if (!want) return LDPC_OK;
    // batch_iters: ES off was set before the launch; otherwise the largest per-frame count
    return reduce_counter_rows(w.partials, (B + 63) / 64, c.counters, es == LDPC_ES_OFF ? nullptr : c.batch_iters,
                               nullptr, s);
}

}  // namespace ldpc
