// flood_layered.hip -- LDS-resident layered (row-serial) scaled min-sum decoder for gfx950.
//
// No reference counterpart: the algorithm is the contract in include/ldpc_amd.h ("layered
// min-sum").  Per frame app[v] = llr[v], c2v[e] = +0; one iteration visits the checks in ascending
// index, and for check i with variables j_0 < ... < j_{d-1}
//     t_k      = app[j_k] - c2v[i,k]        (a degree-1 variable: t_k = llr[j_k] exactly)
//     c2v[i,k] = prod_{q != k} sgn(t_q) * (alpha * min_{q != k} |t_q|)      (MinSumStats)
//     app[j_k] = t_k + c2v[i,k]
// and bit[v] = app[v] < 0 after a full iteration.
//
// Schedule.  The graph is lifted with weight-1 circulants (graph.cpp try_lift: one shift per block,
// exactly Z edges), so the Z checks of a block row touch disjoint variables: updating them at once
// is bit-identical to the serial definition.  A block row is a layer; at Z = 1 every check is one.
// Layers are sequential, so ONE WAVE owns its FG = 64/Z frames for the whole decode and walks all
// block rows in order (lane = f*Z + k as in the flooding kernels: no idle lanes).  A workgroup is
// one wave: no workgroup barrier anywhere, and one counter row per FG frames as the flooding path.
//
// Two kernels: layered_kernel (table-driven, any LDS-resident graph: the correctness baseline) and
// layered_fixed_kernel (compile-time schedule for BG2 Z=32, c2v compressed in registers; below).
//
// LDS of a wave in the table-driven kernel (LayeredTables, graph.hpp):
//   posteriors  one slot of 64 floats per column of degree != 1, column-indexed; the check lane k
//               reads and writes position f*Z + (k + s) mod Z (a permutation inside a frame's Z
//               lanes: conflict-free)
//   c2v         one slot per block of those columns, check-indexed: own-lane reads and writes
//   [ES_FRAME]  Nb decision ballots
// Degree-1 columns own nothing: their t is the channel LLR and their posterior llr + c2v is
// needed for the decision only.
//
// Why race-free.  Inside a layer a lane touches only its own positions: the row's blocks lie in
// distinct columns and a block maps the Z check lanes of a frame onto Z distinct positions.
// Between layers a lane reads what another lane of the SAME wave wrote; a wave's DS instructions
// execute in issue order, and layer_sync() keeps the compiler from moving LDS accesses across the
// layer boundary.  No other wave ever touches these bytes.
// Compile with -ffp-contract=off: no a*b+c may fuse on this path.
#include <string>
#include "flood_host.hpp"
#include "gen/fixed_codes.hpp"

namespace ldpc {
namespace {

// compiler-only ordering point between layers (emits no instruction)
__device__ __forceinline__ void layer_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct LayCtx {
    Ctx C;
    char *app;  // posterior slots
    char *cv;   // c2v slots
};

// byte offset inside a posterior slot of variable (k + s) mod Z of frame f
__device__ __forceinline__ int post_off(const Lane &L, int s4) { return L.fz4 + ((L.k4 + s4) & L.zmask4); }

// One layer, DC compile-time: the row's inputs stay in registers.
template <int DC>
__device__ __forceinline__ void layer_task(const LayCtx &Y, const Lane &L, const int32_t *prog, int slot0,
                                           int &errs) {
    float t[DC];
    int32_t w[DC];
    int ao[DC];
    const int so = slot0 + L.lane4;
    int q = 0;
#pragma unroll
    for (int e = 0; e < DC; ++e) {
        w[e] = tab(prog, e);
        const int lo = w[e] & kLowMask, s4 = (w[e] >> kShiftBit) & 0xFF;
        if (w[e] < 0) {
            ao[e] = 0;
            t[e] = L.llr_at(L.col_off(lo, s4));
        } else {
            ao[e] = lo + post_off(L, s4);
            t[e] = lds_rd(Y.app, ao[e]) - lds_rd(Y.cv, so + q);
            q += 256;
        }
    }
    MinSumStats st;
#pragma unroll
    for (int e = 0; e < DC; ++e) st.add(e, t[e]);
    q = 0;
#pragma unroll
    for (int e = 0; e < DC; ++e) {
        const float c = st.c2v(e, t[e], Y.C.alpha);
        const float a = t[e] + c;
        if (w[e] >= 0) {
            lds_wr(Y.cv, so + q, c);
            lds_wr(Y.app, ao[e], a);
            q += 256;
        } else if (Y.C.direct_bits || Y.C.ballots) {
            ext_decision(Y.C, L, w[e] & kLowMask, (w[e] >> kShiftBit) & 0xFF, a, errs);
        }
    }
}

// Any degree: the inputs are formed twice instead of kept (an edge's posterior and c2v are
// overwritten only at its own turn of the second pass, after they were read for it).
__device__ __forceinline__ void layer_task_dyn(const LayCtx &Y, const Lane &L, const int32_t *prog, int dc,
                                               int slot0, int &errs) {
    const int so = slot0 + L.lane4;
    auto input = [&](int32_t w, int q) -> float {
        const int lo = w & kLowMask, s4 = (w >> kShiftBit) & 0xFF;
        return w < 0 ? L.llr_at(L.col_off(lo, s4)) : lds_rd(Y.app, lo + post_off(L, s4)) - lds_rd(Y.cv, so + q);
    };
    MinSumStats st;
    int q = 0;
    for (int e = 0; e < dc; ++e) {
        const int32_t w = tab(prog, e);
        st.add(e, input(w, q));
        if (w >= 0) q += 256;
    }
    q = 0;
    for (int e = 0; e < dc; ++e) {
        const int32_t w = tab(prog, e);
        const int lo = w & kLowMask, s4 = (w >> kShiftBit) & 0xFF;
        const float x = input(w, q);
        const float c = st.c2v(e, x, Y.C.alpha);
        const float a = x + c;
        if (w >= 0) {
            lds_wr(Y.cv, so + q, c);
            lds_wr(Y.app, lo + post_off(L, s4), a);
            q += 256;
        } else if (Y.C.direct_bits || Y.C.ballots) {
            ext_decision(Y.C, L, lo, s4, a, errs);
        }
    }
}

// syndrome of every block row from the ballots: 1 if any check of this lane fails
__device__ __forceinline__ int parity_all(const Ctx &C, const Lane &L) {
    const int W1 = C.T.W + 1;
    const int p1 = tab(C.T.prog_ptr, 2 * W1 + C.T.W);
    int inv = 0;
    for (int pc = tab(C.T.prog_ptr, 2 * W1); pc < p1;) {
        const int dc = tab(C.T.par_prog, pc);
        int p = 0;
        for (int e = 0; e < dc; ++e) {
            const int32_t w = tab(C.T.par_prog, pc + 1 + e);
            const int col = w & kLowMask, s = w >> kShiftBit;
            p ^= (int)((C.words[col] >> (L.f * L.Z() + ((L.k + s) & (L.Z() - 1)))) & 1ull);
        }
        inv |= p;
        pc += 1 + dc;
    }
    return inv;
}

// decisions of the frames in `mask` from the ballots
__device__ __forceinline__ void emit_all(const Ctx &C, const Lane &L, uint64_t mask, int &errs) {
    if (!(L.valid && ((mask >> L.f) & 1ull))) return;
    for (int col = 0; col < C.T.Nb; ++col) {
        const int bit = (int)((C.words[col] >> L.lane) & 1ull);
        put_bit(C.bits, C.out_dtype, L.frame * C.T.N + (int64_t)col * L.Z() + L.k, bit);
        errs += bit;
    }
}

}  // namespace

// The decode of one wave's FG frames, shared by the table-driven and the compile-time schedule.
// Body supplies: init (posteriors <- llr, c2v <- +0), layers (one full iteration), core_decisions
// (decisions of the posterior columns from LDS) and parity (1 if any check of this lane fails).
// ES is LDPC_ES_OFF or LDPC_ES_FRAME.
template <int ES, class Body>
__device__ __forceinline__ void layered_drive(Body &body, LayCtx &Y, const Lane &L, int64_t B, int max_iter,
                                              const Outs &O) {
    Ctx &C = Y.C;
    const FloodTables &T = C.T;
    body.init(Y, L);
    layer_sync();

    const int nf = (int)min<int64_t>((int64_t)T.FG, B - (int64_t)blockIdx.x * T.FG);
    const uint64_t exist = nf >= 64 ? ~0ull : ((1ull << nf) - 1ull);
    int errs = 0, my_iters = max_iter;
    uint64_t done = 0;
    for (int it = 0; it < max_iter; ++it) {
        const bool last = it == max_iter - 1;
        C.direct_bits = ES == LDPC_ES_OFF && last;
        C.ballots = ES == LDPC_ES_FRAME;
        body.layers(Y, L, errs);
        if (C.direct_bits || C.ballots) body.core_decisions(Y, L, errs);
        if constexpr (ES == LDPC_ES_FRAME) {
            layer_sync();  // lane 0's ballots, read by every lane
            const uint64_t inv = __ballot(body.parity(Y, L));
            const uint64_t newly = frame_valid_mask(inv, T.Z, T.FG) & exist & ~done;
            if (newly) {
                emit_all(C, L, newly, errs);
                if ((newly >> L.f) & 1ull) {
                    my_iters = it + 1;
                    if (O.iters_out && L.valid && L.k == 0) O.iters_out[L.frame] = it + 1;
                }
                done |= newly;
            }
            if (done == exist) break;
            layer_sync();
        }
    }
    if constexpr (ES == LDPC_ES_FRAME) {
        const uint64_t rest = exist & ~done;  // never valid: the last iteration's decisions
        if (rest) {
            emit_all(C, L, rest, errs);
            if (O.iters_out && L.valid && L.k == 0 && ((rest >> L.f) & 1ull)) O.iters_out[L.frame] = max_iter;
        }
    } else {
        if (O.iters_out && L.valid && L.k == 0) O.iters_out[L.frame] = max_iter;
    }
    if (O.partials) {
        // row = {bit errors, frame errors, frames, iteration sum, max iterations} of this wave's frames
        uint32_t be = (uint32_t)errs;
        for (int off = 1; off < T.Z; off <<= 1) be += __shfl_xor(be, off, 64);  // per frame
        const bool lead = L.valid && L.k == 0;
        be = lead ? be : 0;
        uint32_t fe = lead && be > 0, fr = lead, itn = lead ? (uint32_t)my_iters : 0, itmax = itn;
        for (int off = 32; off > 0; off >>= 1) {
            be += __shfl_xor(be, off, 64);
            fe += __shfl_xor(fe, off, 64);
            fr += __shfl_xor(fr, off, 64);
            itn += __shfl_xor(itn, off, 64);
            itmax = max(itmax, (uint32_t)__shfl_xor(itmax, off, 64));
        }
        if (L.lane == 0) {
            uint32_t *row = O.partials + (int64_t)blockIdx.x * kPartRow;
            row[0] = be;
            row[1] = fe;
            row[2] = fr;
            row[3] = itn;
            row[4] = itmax;
        }
    }
}

__device__ __forceinline__ void init_lay_ctx(LayCtx &Y, const FloodTables &T, char *lds, int ncols, int nslots,
                                             float alpha, int out_dtype, void *bits) {
    Ctx &C = Y.C;
    C.T = T;
    C.lds = lds;
    C.flag = nullptr;
    C.alpha = alpha;
    C.out_dtype = out_dtype;
    C.bits = bits;
    C.direct_bits = false;
    C.ballots = false;
    Y.app = lds;
    Y.cv = lds + (size_t)ncols * 256;
    C.words = reinterpret_cast<uint64_t *>(Y.cv + (size_t)nslots * 256);
}

// ---------------------------------------------------------------- table-driven schedule
struct TableBody {
    LayeredTables LT;
    __device__ __forceinline__ void init(const LayCtx &Y, const Lane &L) {
        for (int ci = 0; ci < LT.ncols; ++ci)
            lds_wr(Y.app, ci * 256 + L.lane4, L.llr_at(tab(LT.cols, ci) * L.z4 + L.k4));
        for (int sl = 0; sl < Y.C.T.nslots; ++sl) lds_wr(Y.cv, sl * 256 + L.lane4, 0.0f);
    }
    __device__ __forceinline__ void layers(const LayCtx &Y, const Lane &L, int &errs) {
        int pc = 0;
        for (int r = 0; r < Y.C.T.Mb; ++r) {
            const int dc = tab(LT.prog, pc), slot0 = tab(LT.prog, pc + 1);
            const int32_t *prog = LT.prog + pc + 2;
            switch (dc) {
                case 0: break;
#define X(n) case n: layer_task<n>(Y, L, prog, slot0, errs); break;
                LDPC_DC_CASES(X)
#undef X
                default: layer_task_dyn(Y, L, prog, dc, slot0, errs); break;
            }
            pc += 2 + dc;
            layer_sync();
        }
    }
    __device__ __forceinline__ void core_decisions(const LayCtx &Y, const Lane &L, int &errs) {
        for (int ci = 0; ci < LT.ncols; ++ci)
            var_decision(Y.C, L, tab(LT.cols, ci), lds_rd(Y.app, ci * 256 + L.lane4), errs);
    }
    __device__ __forceinline__ int parity(const LayCtx &Y, const Lane &L) { return parity_all(Y.C, L); }
};

// One workgroup = one wave = FG frames.
template <int ES>
__global__ __launch_bounds__(64) void layered_kernel(FloodTables T, LayeredTables LT, const float *__restrict__ llr,
                                                     int64_t B, int max_iter, float alpha, int out_dtype,
                                                     void *__restrict__ bits, Outs O) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const Lane L = make_lane(T, llr, B);
    LayCtx Y;
    init_lay_ctx(Y, T, lds, LT.ncols, T.nslots, alpha, out_dtype, bits);
    TableBody body{LT};
    layered_drive<ES>(body, Y, L, B, max_iter, O);
}

// ---------------------------------------------------------------- compile-time schedule
// The same decode for a graph known at compile time (gen/fixed_codes.hpp), every layer unrolled:
// shifts, columns and degrees are constants, and the per-lane state that the table-driven kernel
// keeps in LDS or re-reads from HBM lives in registers for the whole decode:
//   ext[]   the channel LLRs of the degree-1 columns' edges (their t forever)
//   am1[], am2[], pk[]   the c2v of a block row, compressed: alpha * (the two smallest |t|), and a
//           word in one of two formats (bit 31; the same on every lane of the wave):
//           0  the row had no zero and no NaN in any lane: the c2v's sign bits (bits 0..11) and
//              which edges take alpha * m2 (12..23); c2v = that magnitude with the sign bit xored
//           1  the sign bits of t (0..11), its zero/NaN bits (12..23) and the first index attaining
//              the minimum (24..30; 0x7F: none) -- what MinSumStats yields; the old c2v is
//              re-derived with MinSumStats::c2v's own operations
//           either way it is the float that was added to the posterior: alpha * m is kept as computed.
// LDS holds the posteriors alone (NCORE slots = 3.5 KB per wave at BG2), so the registers, not
// LDS, bound the occupancy.  As compiled the kernel takes more than 256 registers, i.e. one wave
// per SIMD, which runs the layers' dependent chain alone.
// Bit-identical to the table-driven kernel (tests/test_layered_gpu.py).
template <class G>
struct LayFixedBody {
    static constexpr int ncore() {
        int n = 0;
        while (n < G::Nb && G::COL_PTR[n + 1] - G::COL_PTR[n] != 1) ++n;
        return n;
    }
    static constexpr bool layout_ok() {  // posterior columns first, then degree-1 columns only
        for (int c = ncore(); c < G::Nb; ++c)
            if (G::COL_PTR[c + 1] - G::COL_PTR[c] != 1) return false;
        for (int r = 0; r < G::Mb; ++r)
            if (G::ROW_PTR[r + 1] - G::ROW_PTR[r] > 12) return false;
        for (int i = 0; i < G::NBLOCKS; ++i)
            if ((G::ROW_SLOT[i] < 0) != (G::ROW_COL[i] >= ncore())) return false;
        return true;
    }
    static constexpr int NCORE = ncore(), NEXT = G::Nb - NCORE;
    static_assert(layout_ok(), "compile-time layered schedule: unexpected graph shape");

    float ext[NEXT];
    float am1[G::Mb], am2[G::Mb];
    uint32_t pk[G::Mb];

    __device__ __forceinline__ void init(const LayCtx &Y, const Lane &L) {
        sfor<NCORE>([&](auto c) {
            constexpr int col = decltype(c)::value;
            lds_wr(Y.app, col * 256 + L.lane4, L.llr_at(col * L.z4 + L.k4));
        });
        sfor<G::NBLOCKS>([&](auto i) {
            constexpr int b = decltype(i)::value;
            if constexpr (G::ROW_SLOT[b] < 0) ext[G::ROW_COL[b] - NCORE] = L.llr_at(L.col_off(G::ROW_COL[b], 4 * G::ROW_SHIFT[b]));
        });
        sfor<G::Mb>([&](auto r) {
            am1[decltype(r)::value] = 0.0f;  // c2v = +1 * 0 = +0 on every edge
            am2[decltype(r)::value] = 0.0f;
            pk[decltype(r)::value] = 0;
        });
    }

    template <int R>
    __device__ __forceinline__ void layer(const LayCtx &Y, const Lane &L, int &errs) {
        constexpr int E0 = G::ROW_PTR[R], DC = G::ROW_PTR[R + 1] - E0;
        float t[DC];
        int ao[DC];
        const float o1 = am1[R], o2 = am2[R];
        const uint32_t op = pk[R];
        // a row's word has the same format on every lane (both branches below are wave-uniform)
        const bool ogen = (__builtin_amdgcn_readfirstlane(op) >> 31) != 0;
        const int oi1 = (int)((op >> 24) & 0x7Fu), onz = __popc((op >> 12) & 0xFFFu), oneg = __popc(op & 0xFFFu) & 1;
        sfor<DC>([&](auto q) {
            constexpr int e = decltype(q)::value, col = G::ROW_COL[E0 + e], s4 = 4 * G::ROW_SHIFT[E0 + e];
            if constexpr (G::ROW_SLOT[E0 + e] < 0) {
                ao[e] = 0;
                t[e] = ext[col - NCORE];
            } else {
                ao[e] = col * 256 + post_off(L, s4);
                t[e] = lds_rd(Y.app, ao[e]);
            }
        });
        if (!ogen) {  // old c2v = +-(alpha * m): the kept sign bit on the kept magnitude word
            sfor<DC>([&](auto q) {
                constexpr int e = decltype(q)::value;
                if constexpr (G::ROW_SLOT[E0 + e] >= 0) {
                    const float m = ((op >> (12 + e)) & 1u) ? o2 : o1;
                    t[e] = t[e] - __uint_as_float(__float_as_uint(m) ^ ((op << (31 - e)) & 0x80000000u));
                }
            });
        } else {  // MinSumStats::c2v on the kept statistics of the previous visit
            sfor<DC>([&](auto q) {
                constexpr int e = decltype(q)::value;
                if constexpr (G::ROW_SLOT[E0 + e] >= 0) {
                    const float m = (e == oi1) ? o2 : o1;
                    const int zex = onz - (int)((op >> (12 + e)) & 1u);
                    const float sg = zex > 0 ? 0.0f : ((oneg ^ (int)((op >> e) & 1u)) ? -1.0f : 1.0f);
                    t[e] = t[e] - sg * m;
                }
            });
        }
        bool special = false;
        sfor<DC>([&](auto q) { special |= is_zero_sign(t[decltype(q)::value]); });
        auto put = [&](auto q, float a) {
            constexpr int e = decltype(q)::value, col = G::ROW_COL[E0 + e], s4 = 4 * G::ROW_SHIFT[E0 + e];
            if constexpr (G::ROW_SLOT[E0 + e] >= 0) {
                lds_wr(Y.app, ao[e], a);
            } else {
                if (Y.C.direct_bits || Y.C.ballots) ext_decision(Y.C, L, col, s4, a, errs);
            }
        };
        uint32_t np = 0;
        if (!__any(special)) {
            // no zero, no NaN in any lane's row (every row, in practice): sgn is +-1, so the output
            // sign is (xor of all sign bits) ^ own sign bit, the excluded minimum is m2 exactly when
            // |t| == m1 (a tie puts m1 in m2 too), and +-1 * x is x with the sign bit xored:
            // every float below is the one MinSumStats::c2v gives (flood_dev.hpp, MinSumFast)
            uint32_t par = 0;
            sfor<DC>([&](auto q) { par ^= __float_as_uint(t[decltype(q)::value]); });
            float m1 = INFINITY, m2 = INFINITY;
            two_smallest<DC>(t, m1, m2, opaque_sf(-INFINITY));
            const float n1 = Y.C.alpha * m1, n2 = Y.C.alpha * m2;
            sfor<DC>([&](auto q) {
                constexpr int e = decltype(q)::value;
                const bool ismin = fabsf(t[e]) == m1;
                const uint32_t sbit = (__float_as_uint(t[e]) ^ par) & 0x80000000u;
                const float c = __uint_as_float(__float_as_uint(ismin ? n2 : n1) ^ sbit);
                np |= (sbit >> (31 - e)) | (ismin ? 1u << (12 + e) : 0u);
                put(q, t[e] + c);
            });
            am1[R] = n1;
            am2[R] = n2;
            pk[R] = np;  // bit 31 clear: the sign / minimum-position format
        } else {
            MinSumStats st;
            sfor<DC>([&](auto q) {
                constexpr int e = decltype(q)::value;
                st.add(e, t[e]);
                np |= (t[e] < 0.0f ? 1u : 0u) << e;
                np |= (is_zero_sign(t[e]) ? 1u : 0u) << (12 + e);
            });
            const float n1 = Y.C.alpha * st.m1, n2 = Y.C.alpha * st.m2;
            sfor<DC>([&](auto q) {
                constexpr int e = decltype(q)::value;
                const float m = (e == st.i1) ? n2 : n1;
                const int zex = st.nz - (int)is_zero_sign(t[e]);
                const float sg = zex > 0 ? 0.0f : ((st.neg ^ (t[e] < 0.0f)) ? -1.0f : 1.0f);
                put(q, t[e] + sg * m);
            });
            am1[R] = n1;
            am2[R] = n2;
            pk[R] = np | ((uint32_t)(st.i1 & 0x7F) << 24) | 0x80000000u;  // bit 31: the MinSumStats format
        }
    }

    __device__ __forceinline__ void layers(const LayCtx &Y, const Lane &L, int &errs) {
        sfor<G::Mb>([&](auto r) {
            this->template layer<decltype(r)::value>(Y, L, errs);
            layer_sync();
        });
    }
    __device__ __forceinline__ void core_decisions(const LayCtx &Y, const Lane &L, int &errs) {
        sfor<NCORE>([&](auto c) {
            constexpr int col = decltype(c)::value;
            var_decision(Y.C, L, col, lds_rd(Y.app, col * 256 + L.lane4), errs);
        });
    }
    __device__ __forceinline__ int parity(const LayCtx &Y, const Lane &L) {
        int inv = 0;
        sfor<G::Mb>([&](auto r) {
            constexpr int E0 = G::ROW_PTR[decltype(r)::value], DC = G::ROW_PTR[decltype(r)::value + 1] - E0;
            int p = 0;
            sfor<DC>([&](auto q) {
                constexpr int b = E0 + decltype(q)::value;
                p ^= (int)((Y.C.words[G::ROW_COL[b]] >> (L.f * G::Z + ((L.k + G::ROW_SHIFT[b]) & (G::Z - 1)))) & 1ull);
            });
            inv |= p;
        });
        return inv;
    }
};

template <class G, int ES>
__global__ __launch_bounds__(64)
void layered_fixed_kernel(FloodTables T, const float *__restrict__ llr, int64_t B, int max_iter, float alpha,
                          int out_dtype, void *__restrict__ bits, Outs O) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const Lane L = make_lane(T, llr, B);
    LayCtx Y;
    init_lay_ctx(Y, T, lds, LayFixedBody<G>::NCORE, 0, alpha, out_dtype, bits);
    LayFixedBody<G> body;
    layered_drive<ES>(body, Y, L, B, max_iter, O);
}

size_t layered_lds_bytes(const ldpc_graph *g, int es) {
    size_t b = ((size_t)g->lt.ncols + (size_t)g->nslots) * 64 * sizeof(float);
    if (es != LDPC_ES_OFF) b += (size_t)g->Nb * sizeof(uint64_t);
    return b;
}

int run_layered(const FloodCall &c) {
    const ldpc_graph *g = c.g;
    const int es = c.es;
    const int64_t nwg = (c.B + g->FG - 1) / g->FG;
    const bool want = c.counters || (c.batch_iters && es == LDPC_ES_FRAME);
    const Outs O{c.iters, want ? static_cast<uint32_t *>(c.work) : nullptr, nullptr};
    if (g->fixed_id == 2) {  // compile-time schedule: BG2 Z=32
        using FB = LayFixedBody<fixed::BG2_Z32>;
        const size_t lds = (size_t)FB::NCORE * 256 + (es != LDPC_ES_OFF ? (size_t)g->Nb * sizeof(uint64_t) : 0);
        auto kern = es == LDPC_ES_OFF ? layered_fixed_kernel<fixed::BG2_Z32, LDPC_ES_OFF>
                                      : layered_fixed_kernel<fixed::BG2_Z32, LDPC_ES_FRAME>;
        hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(64), lds, c.s, g->ft, c.llr, c.B, c.max_iter, c.alpha,
                           c.out_dtype, c.bits, O);
        LDPC_CHECK_LAUNCH("layered_fixed_kernel");
    } else {
        const size_t lds = layered_lds_bytes(g, es);
        auto kern = es == LDPC_ES_OFF ? layered_kernel<LDPC_ES_OFF> : layered_kernel<LDPC_ES_FRAME>;
        LDPC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
        hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(64), lds, c.s, g->ft, g->lt, c.llr, c.B, c.max_iter, c.alpha,
                           c.out_dtype, c.bits, O);
        LDPC_CHECK_LAUNCH("layered_kernel");
    }
    if (!want) return LDPC_OK;
    // ES off: every frame ran max_iter (batch_iters was set before the launch)
    return reduce_counter_rows(O.partials, nwg, c.counters, es == LDPC_ES_FRAME ? c.batch_iters : nullptr, nullptr, c.s);
}

}  // namespace ldpc
