// flood_half.hip -- LDPC_ALGO_MINSUM_F16: flooding scaled min-sum on IEEE binary16 messages, two frames per
// lane on packed f16 math (v_pk_add_f16 / v_pk_mul_f16 / v_pk_minimum3_f16 / v_pk_maximum3_f16).
//
// The algorithm is the contract written in include/ldpc_amd.h ("Half-precision min-sum"); the numpy
// restatement the tests hold it to is tests/half_ref.py.  Schedule and layout are the table-driven fp32
// kernel's (flood_dev.hpp, graph.hpp), driven by the same FloodTables, with one change: a message slot is
// still 64 dwords indexed by check row, rotations are still per-lane byte offsets, but each dword holds
// the binary16 messages of TWO frames, so every LDS instruction and every packed VALU instruction of an
// iteration serves twice the frames.
//
// Pairing.  A workgroup (4 waves) decodes 2 * FG frames (FG = 64 / Z).  Lane l = f * Z + k of workgroup g
// holds, in every dword it touches,
//     low  half (bits 15:0)   frame g * 2 * FG + f
//     high half (bits 31:16)  frame g * 2 * FG + FG + f
// so a last workgroup that is not full loses its high halves first.  A frame slot beyond B reads the LLR
// row of frame 0 and writes nothing.  The two halves of a dword never meet: every operation on messages
// is a packed (per-half) f16 operation or a bitwise one, so a NaN in one frame cannot reach its partner.
//
// Check update.  c2v_k = (prod_{q != k} sgn v_q) * (a * min_{q != k} |v_q|).  The exclusive minimum is
// min(prefix_{k-1}, suffix_{k+1}) of the magnitudes (3 packed mins per edge, no compare), a * min is one
// v_pk_mul_f16, and the sign is the XOR of all packed sign bits with the edge's own XORed back out.
// sgn(0) = 0 needs no code: if another message of the row is zero the exclusive minimum is 0 and the
// result is a zero whatever its sign (the sign of a zero is not part of the contract), and if only v_k
// itself is zero its sign bit cancels in the XOR.  The clamp keeps every operand finite, so the
// NaN-propagating minimum / maximum (no canonicalising v_pk_max x, x per operand) are exact here.
//
// Variable update.  v2c_k = clamp(x + sum_{q != k} c2v_q) in ascending q, each add rounded: the prefix
// P_k followed by the tail adds, as the fp32 kernel does; the posterior P_dv is not clamped.  x =
// clamp(half(llr)) is converted from the float32 LLRs where it is used (v_cvt_pk_f16_f32, nearest-even).
// Decisions are a real compare per half (app < 0; -0 is not negative), kept as two ballot words per
// column when the per-frame stop needs them.
//
// LDS: nslots * 256 bytes of slots, 8 bytes unused (the fp32 layout's flag), 2 * (Nb + 1) ballot words
// (low frames, then high frames; the last word of each is the invalid-lane word of the syndrome).
// Counter rows are in the kPartRow format, one per workgroup: reduce_counter_rows folds them unchanged.
// Compile with -ffp-contract=off (the Makefile's default): no multiply-add may fuse.
#include <algorithm>
#include <string>

#include "flood_host.hpp"
#include "half_pair.hpp"

namespace ldpc {

namespace {

struct HLane {
    int lane;        // 0..63 = f * Z + k
    int f, k;        // frame within a half, row (or column position) within a block
    int lane4;       // 4 * lane
    int fz4, k4, zmask4, z4;  // as Lane (flood_dev.hpp)
    bool valid[2];   // the lane's low / high frame exists
    int64_t frame[2];
    const char *row[2];  // LLR rows of the two frames (frame 0 for a slot without a frame)
    __device__ __forceinline__ int vrot(int s4) const { return fz4 + ((k4 - s4) & zmask4); }
    __device__ __forceinline__ int col_off(int col, int s4) const { return col * z4 + ((k4 + s4) & zmask4); }
    __device__ __forceinline__ int Z() const { return z4 >> 2; }
};

struct HCtx {
    FloodTables T;
    char *lds;
    uint64_t *words;   // [2][Nb + 1] decision ballots + invalid-lane word, low frames then high frames
    HConst K;
    int out_dtype;
    void *bits;
    bool direct_bits;  // LDPC_ES_OFF, final iteration: decisions straight to HBM
    bool ballots;      // LDPC_ES_FRAME: decisions as ballots
};

__device__ __forceinline__ uint32_t ldu(const char *lds, int off) { return *reinterpret_cast<const uint32_t *>(lds + off); }
__device__ __forceinline__ void stu(char *lds, int off, uint32_t v) { *reinterpret_cast<uint32_t *>(lds + off) = v; }

// x = clamp(half(llr)) of the lane's two frames at a byte offset inside an LLR row.  A magnitude that
// rounds to infinity clamps to +-C; a NaN stays one (its frame's outputs are unspecified).
__device__ __forceinline__ h2 x_at(const HCtx &C, const HLane &L, int byte_off) {
    const float lo = *reinterpret_cast<const float *>(L.row[0] + byte_off);
    const float hi = *reinterpret_cast<const float *>(L.row[1] + byte_off);
    h2 x;
    x.x = (_Float16)lo;
    x.y = (_Float16)hi;
    return hclamp(C.K, x);
}

// decisions of one column: bit = (app < 0) per half, to HBM and / or the ballots.  rot: the column's
// variable (k + rot) mod Z sits on this lane (check phase, degree-1 columns); 0 in the variable phase.
__device__ __forceinline__ void decide(const HCtx &C, const HLane &L, int col, int rot4, h2 app, int (&errs)[2]) {
    const int bit[2] = {app.x < (_Float16)0.0f, app.y < (_Float16)0.0f};  // NaN < 0 is false
    if (C.direct_bits) {
        const int64_t idx = (col * L.z4 + ((L.k4 + rot4) & L.zmask4)) / 4;
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (L.valid[h]) {
                put_bit(C.bits, C.out_dtype, L.frame[h] * C.T.N + idx, bit[h]);
                errs[h] += bit[h];
            }
    }
    if (C.ballots) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint64_t w = seg_rotl(__ballot(bit[h]), rot4 >> 2, C.T.Z, C.T.rep1);
            if (L.lane == 0) C.words[h * (C.T.Nb + 1) + col] = w;
        }
    }
}

// ---------------------------------------------------------------- check node update
template <int DC>
__device__ __forceinline__ void hcheck_task(const HCtx &C, const HLane &L, const int32_t *prog, int (&errs)[2]) {
    uint32_t v[DC];
    int32_t w[DC];
#pragma unroll
    for (int e = 0; e < DC; ++e) {
        w[e] = tab(prog, e);
        const int lo = w[e] & kLowMask, s4 = (w[e] >> kShiftBit) & 0xFF;
        v[e] = w[e] < 0 ? as_u(x_at(C, L, L.col_off(lo, s4))) : ldu(C.lds, lo + L.lane4);
    }
    // the empty minimum is +inf here: the contract's min over no message ("Half-precision min-sum",
    // include/ldpc_amd.h), as in the float32 rule.  The layered form's is C (half_pair.hpp).
    uint32_t out[DC];
    half_check_rule<DC>(C.K, v, out, as_h(kInf2));
#pragma unroll
    for (int e = 0; e < DC; ++e) {
        const int lo = w[e] & kLowMask;
        if (w[e] >= 0)
            stu(C.lds, lo + L.lane4, out[e]);
        else if (C.direct_bits || C.ballots)  // degree-1 variable: app = x + c2v
            decide(C, L, lo, (w[e] >> kShiftBit) & 0xFF, as_h(v[e]) + as_h(out[e]), errs);
    }
}

// Any degree: the two-pass form (half_two_min_step / half_excl_select), the row read from LDS twice.
__device__ __forceinline__ void hcheck_task_dyn(const HCtx &C, const HLane &L, const int32_t *prog, int dc,
                                                int (&errs)[2]) {
    auto rd = [&](int e) -> uint32_t {
        const int32_t w = tab(prog, e);
        const int lo = w & kLowMask;
        return w < 0 ? as_u(x_at(C, L, L.col_off(lo, (w >> kShiftBit) & 0xFF))) : ldu(C.lds, lo + L.lane4);
    };
    h2 m1 = as_h(kInf2), m2 = as_h(kInf2);  // the empty minimum, as in hcheck_task
    uint32_t par = 0;
    for (int e = 0; e < dc; ++e) {
        const uint32_t x = rd(e);
        par ^= x;
        half_two_min_step(m1, m2, as_h(x & C.K.absm));
    }
    for (int e = 0; e < dc; ++e) {
        const uint32_t x = rd(e);
        const uint32_t o = signed_c2v(C.K, par, x, half_excl_select(as_h(x & C.K.absm), m1, m2));
        const int32_t w = tab(prog, e);
        const int lo = w & kLowMask;
        if (w >= 0)
            stu(C.lds, lo + L.lane4, o);
        else if (C.direct_bits || C.ballots)
            decide(C, L, lo, (w >> kShiftBit) & 0xFF, as_h(x) + as_h(o), errs);
    }
}

// ---------------------------------------------------------------- variable node update
template <int DV>
__device__ __forceinline__ void hvar_task(const HCtx &C, const HLane &L, const int32_t *prog, int col, bool write,
                                          int (&errs)[2]) {
    h2 P = x_at(C, L, col * L.z4 + L.k4);
    if constexpr (DV > 0) {
        h2 acc[DV];
        int off[DV];
#pragma unroll
        for (int j = 0; j < DV; ++j) {
            const int32_t w = tab(prog, j);
            off[j] = (w & kLowMask) + L.vrot((w >> kShiftBit) & 0xFF);
            const h2 c = as_h(ldu(C.lds, off[j]));
#pragma unroll
            for (int e = 0; e < j; ++e) acc[e] = acc[e] + c;
            acc[j] = P;
            P = P + c;
        }
        if (write) {
#pragma unroll
            for (int e = 0; e < DV; ++e) stu(C.lds, off[e], as_u(hclamp(C.K, acc[e])));
        }
    }
    if (C.direct_bits || C.ballots) decide(C, L, col, 0, P, errs);
}

__device__ __forceinline__ void hvar_task_dyn(const HCtx &C, const HLane &L, const int32_t *prog, int dv, int col,
                                              bool write, int (&errs)[2]) {
    auto off = [&](int e) {
        const int32_t w = tab(prog, e);
        return (w & kLowMask) + L.vrot((w >> kShiftBit) & 0xFF);
    };
    h2 P = x_at(C, L, col * L.z4 + L.k4);
    for (int e = 0; e < dv; ++e) {
        const int o = off(e);
        const h2 cp = as_h(ldu(C.lds, o));
        h2 acc = P;
        for (int q = e + 1; q < dv; ++q) acc = acc + as_h(ldu(C.lds, off(q)));
        P = P + cp;
        if (write) stu(C.lds, o, as_u(hclamp(C.K, acc)));  // slot e is not read again
    }
    if (C.direct_bits || C.ballots) decide(C, L, col, 0, P, errs);
}

__device__ __forceinline__ void hcheck_phase(const HCtx &C, const HLane &L, int wave, int (&errs)[2]) {
    const int p1 = tab(C.T.prog_ptr, wave + 1);
    for (int pc = tab(C.T.prog_ptr, wave); pc < p1;) {
        const int dc = tab(C.T.chk_prog, pc);
        const int32_t *prog = C.T.chk_prog + pc + 1;
        switch (dc) {
            case 0: break;
#define X(n) case n: hcheck_task<n>(C, L, prog, errs); break;
            LDPC_DC_CASES(X)
#undef X
            default: hcheck_task_dyn(C, L, prog, dc, errs); break;
        }
        pc += 1 + dc;
    }
}

__device__ __forceinline__ void hvar_phase(const HCtx &C, const HLane &L, int wave, bool write, int (&errs)[2]) {
    const int W1 = C.T.W + 1;
    const int p1 = tab(C.T.prog_ptr, W1 + wave + 1);
    for (int pc = tab(C.T.prog_ptr, W1 + wave); pc < p1;) {
        const int h = tab(C.T.var_prog, pc);
        const int dv = h & 0xFF, col = h >> 8;
        const int32_t *prog = C.T.var_prog + pc + 1;
        switch (dv) {
            case 0: hvar_task<0>(C, L, prog, col, write, errs); break;
#define X(n) case n: hvar_task<n>(C, L, prog, col, write, errs); break;
            LDPC_DV_CASES(X)
#undef X
            default: hvar_task_dyn(C, L, prog, dv, col, write, errs); break;
        }
        pc += 1 + dv;
    }
}

// v2c <- x on every slot
__device__ __forceinline__ void hinit_phase(const HCtx &C, const HLane &L, int wave) {
    const int W1 = C.T.W + 1;
    const int p1 = tab(C.T.prog_ptr, W1 + wave + 1);
    for (int pc = tab(C.T.prog_ptr, W1 + wave); pc < p1;) {
        const int h = tab(C.T.var_prog, pc);
        const int dv = h & 0xFF, col = h >> 8;
        const uint32_t x = as_u(x_at(C, L, col * L.z4 + L.k4));
        for (int e = 0; e < dv; ++e) {
            const int32_t w = tab(C.T.var_prog, pc + 1 + e);
            stu(C.lds, (w & kLowMask) + L.vrot((w >> kShiftBit) & 0xFF), x);
        }
        pc += 1 + dv;
    }
}

// syndrome of this wave's rows from the ballots of one half: 1 if any of its checks fails for this lane
__device__ __forceinline__ int hparity_phase(const HCtx &C, const HLane &L, int wave, const uint64_t *words) {
    const int W1 = C.T.W + 1;
    const int p1 = tab(C.T.prog_ptr, 2 * W1 + wave + 1);
    int inv = 0;
    for (int pc = tab(C.T.prog_ptr, 2 * W1 + wave); pc < p1;) {
        const int dc = tab(C.T.par_prog, pc);
        int p = 0;
        for (int e = 0; e < dc; ++e) {
            const int32_t w = tab(C.T.par_prog, pc + 1 + e);
            const int col = w & kLowMask, s = w >> kShiftBit;
            p ^= (int)((words[col] >> (L.f * L.Z() + ((L.k + s) & (L.Z() - 1)))) & 1ull);
        }
        inv |= p;
        pc += 1 + dc;
    }
    return inv;
}

// emit the decisions of the frames in mask[h] from the ballots (columns spread over the waves)
__device__ __forceinline__ void hemit(const HCtx &C, const HLane &L, const uint64_t (&mask)[2], int wave,
                                      int (&errs)[2]) {
    const int W1 = C.T.W + 1;
    const int i0 = tab(C.T.prog_ptr, 3 * W1 + wave), i1 = tab(C.T.prog_ptr, 3 * W1 + wave + 1);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (!(L.valid[h] && ((mask[h] >> L.f) & 1ull))) continue;
        const uint64_t *words = C.words + h * (C.T.Nb + 1);
        for (int i = i0; i < i1; ++i) {
            const int col = tab(C.T.bw_task, i);
            const int bit = (int)((words[col] >> L.lane) & 1ull);
            put_bit(C.bits, C.out_dtype, L.frame[h] * C.T.N + (int64_t)col * L.Z() + L.k, bit);
            errs[h] += bit;
        }
    }
}

// this workgroup's counter row {bit errors, frame errors, frames, iteration sum, max iterations}
__device__ __forceinline__ void hreduce_counters(void *lds, const int (&errs)[2], const int (&my_iters)[2],
                                                 const int (&nf)[2], int Z, uint32_t *row) {
    uint32_t *u = reinterpret_cast<uint32_t *>(lds);
    const int nt = blockDim.x;
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        u[(2 * h) * nt + threadIdx.x] = (uint32_t)errs[h];
        u[(2 * h + 1) * nt + threadIdx.x] = (uint32_t)my_iters[h];
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int f = threadIdx.x;
        uint32_t be = 0, fe = 0, fr = 0, it = 0, itmax = 0;
        for (int h = 0; h < 2; ++h) {
            if (f >= nf[h]) continue;
            uint32_t b = 0;
            for (int w = 0; w < nt / 64; ++w)
                for (int k = 0; k < Z; ++k) b += u[(2 * h) * nt + w * 64 + f * Z + k];
            const uint32_t i = u[(2 * h + 1) * nt + f * Z];
            be += b;
            fe += b > 0;
            fr += 1;
            it += i;
            itmax = max(itmax, i);
        }
        for (int off = 32; off > 0; off >>= 1) {
            be += __shfl_xor(be, off, 64);
            fe += __shfl_xor(fe, off, 64);
            fr += __shfl_xor(fr, off, 64);
            it += __shfl_xor(it, off, 64);
            itmax = max(itmax, (uint32_t)__shfl_xor(itmax, off, 64));
        }
        if (f == 0) {
            row[0] = be;
            row[1] = fe;
            row[2] = fr;
            row[3] = it;
            row[4] = itmax;
        }
    }
}

__device__ __forceinline__ HLane make_hlane(const FloodTables &T, const float *llr, int64_t B) {
    HLane L;
    L.lane = threadIdx.x & 63;
    const int lz = __builtin_ctz((unsigned)T.Z);  // Z is a power of two
    L.f = L.lane >> lz;
    L.k = L.lane & (T.Z - 1);
    L.lane4 = 4 * L.lane;
    L.fz4 = 4 * (L.f << lz);
    L.k4 = 4 * L.k;
    L.z4 = 4 * T.Z;
    L.zmask4 = 4 * T.Z - 1;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        L.frame[h] = (int64_t)blockIdx.x * 2 * T.FG + h * T.FG + L.f;
        L.valid[h] = L.frame[h] < B;
        L.row[h] = reinterpret_cast<const char *>(llr + (L.valid[h] ? L.frame[h] : 0) * (int64_t)T.N);
    }
    return L;
}

}  // namespace

// ES: LDPC_ES_OFF or LDPC_ES_FRAME.  Every branch around a barrier depends on workgroup-uniform values.
template <int ES>
__global__ __launch_bounds__(256) void flood_half_kernel(FloodTables T, const float *__restrict__ llr, int64_t B,
                                                         int max_iter, uint32_t alpha2, int out_dtype,
                                                         void *__restrict__ bits, int32_t *__restrict__ iters_out,
                                                         uint32_t *__restrict__ partials) {
    static_assert(ES == LDPC_ES_OFF || ES == LDPC_ES_FRAME, "no batch-global stop");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const HLane L = make_hlane(T, llr, B);
    HCtx C;
    C.T = T;
    C.lds = lds;
    C.words = reinterpret_cast<uint64_t *>(lds + (size_t)T.nslots * 256 + 8);
    C.K = make_const(alpha2);
    C.out_dtype = out_dtype;
    C.bits = bits;
    C.direct_bits = false;
    C.ballots = false;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int FG = T.FG, Nb = T.Nb, Z = T.Z;
    const int64_t left = B - (int64_t)blockIdx.x * 2 * FG;  // >= 1
    const int nf[2] = {(int)min<int64_t>(FG, left), (int)max<int64_t>(0, min<int64_t>(FG, left - FG))};
    uint64_t exist[2];
    for (int h = 0; h < 2; ++h) exist[h] = nf[h] >= 64 ? ~0ull : ((1ull << nf[h]) - 1ull);
    int errs[2] = {0, 0};
    int my_iters[2] = {max_iter, max_iter};
    uint64_t done[2] = {0, 0};

    hinit_phase(C, L, wave);
    __syncthreads();
    for (int it = 0; it < max_iter; ++it) {
        const bool last = it == max_iter - 1;
        C.direct_bits = ES == LDPC_ES_OFF && last;
        C.ballots = ES == LDPC_ES_FRAME;
        hcheck_phase(C, L, wave, errs);
        __syncthreads();
        if (C.ballots && tid == 0) {
            C.words[Nb] = 0;
            C.words[Nb + 1 + Nb] = 0;
        }
        hvar_phase(C, L, wave, !last, errs);
        __syncthreads();
        if constexpr (ES == LDPC_ES_FRAME) {
            // syndrome H x = 0 per frame, from the ballots
            for (int h = 0; h < 2; ++h) {
                const uint64_t m = __ballot(hparity_phase(C, L, wave, C.words + h * (Nb + 1)));
                if (L.lane == 0 && m)
                    atomicOr((unsigned long long *)&C.words[h * (Nb + 1) + Nb], (unsigned long long)m);
            }
            __syncthreads();
            uint64_t newly[2];
            for (int h = 0; h < 2; ++h)
                newly[h] = frame_valid_mask(C.words[h * (Nb + 1) + Nb], Z, FG) & exist[h] & ~done[h];
            if (newly[0] | newly[1]) {
                hemit(C, L, newly, wave, errs);
                for (int h = 0; h < 2; ++h) {
                    if (!((newly[h] >> L.f) & 1ull)) continue;
                    my_iters[h] = it + 1;
                    if (iters_out && L.valid[h] && L.k == 0) iters_out[L.frame[h]] = it + 1;
                }
                done[0] |= newly[0];
                done[1] |= newly[1];
            }
            const bool stop = done[0] == exist[0] && done[1] == exist[1];
            __syncthreads();
            if (stop) break;
        }
    }
    if constexpr (ES == LDPC_ES_FRAME) {
        const uint64_t rest[2] = {exist[0] & ~done[0], exist[1] & ~done[1]};
        if (rest[0] | rest[1]) {
            hemit(C, L, rest, wave, errs);
            for (int h = 0; h < 2; ++h)
                if (iters_out && L.valid[h] && L.k == 0 && ((rest[h] >> L.f) & 1ull)) iters_out[L.frame[h]] = max_iter;
        }
    } else {
        for (int h = 0; h < 2; ++h)
            if (iters_out && L.valid[h] && L.k == 0) iters_out[L.frame[h]] = max_iter;
    }
    if (partials) hreduce_counters(lds, errs, my_iters, nf, Z, partials + (int64_t)blockIdx.x * kPartRow);
}

// ---------------------------------------------------------------- host side
size_t half_lds_bytes(const ldpc_graph *g) {
    const size_t b = (size_t)g->nslots * 256 + 8 + 2 * (size_t)(g->Nb + 1) * sizeof(uint64_t);
    return std::max<size_t>(b, 4 * 64 * (size_t)g->ft.W * sizeof(uint32_t));  // hreduce_counters
}

template <int ES>
static int launch_half(const FloodCall &c, uint32_t *partials) {
    const ldpc_graph *g = c.g;
    const size_t lds = half_lds_bytes(g);
    const int64_t nwg = (c.B + 2 * g->FG - 1) / (2 * g->FG);
    const uint32_t a = half_alpha_bits(c.alpha);
    auto kern = flood_half_kernel<ES>;
    LDPC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(64 * g->ft.W), lds, c.s, g->ft, c.llr, c.B, c.max_iter,
                       a | (a << 16), c.out_dtype, c.bits, c.iters, partials);
    LDPC_CHECK_LAUNCH("flood_half_kernel");
    return LDPC_OK;
}

int run_half(const FloodCall &c) {
    const ldpc_graph *g = c.g;
    if (64 * g->ft.W > 256) return fail(LDPC_EUNSUPPORTED, "half-precision min-sum: more than 4 waves per workgroup");
    // counter rows: the head of the flooding workspace (one row per 2 * FG frames: half of its rows)
    const bool want = c.counters || c.batch_iters;
    uint32_t *partials = want ? static_cast<uint32_t *>(c.work) : nullptr;
    const int64_t nwg = (c.B + 2 * g->FG - 1) / (2 * g->FG);
    if (c.es == LDPC_ES_OFF) {
        // every frame ran max_iter (batch_iters was set before the launch)
        const int rc = launch_half<LDPC_ES_OFF>(c, c.counters ? partials : nullptr);
        if (rc != LDPC_OK || !c.counters) return rc;
        return reduce_counter_rows(partials, nwg, c.counters, nullptr, nullptr, c.s);
    }
    const int rc = launch_half<LDPC_ES_FRAME>(c, partials);
    if (rc != LDPC_OK || !want) return rc;
    return reduce_counter_rows(partials, nwg, c.counters, c.batch_iters, nullptr, c.s);
}

}  // namespace ldpc
