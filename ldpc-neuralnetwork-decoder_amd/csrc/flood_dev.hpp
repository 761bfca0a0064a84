// flood_dev.hpp -- device side of the flooding decoders, shared by the flood*.hip translation units:
// lanes and LDS helpers, the min-sum and sum-product math, the iteration driver (flood_drive) and the
// table-driven kernel.  The algorithm notes are at the top of flood.hip; the compile-time-schedule
// kernel is flood_fixed.hpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>

#include <utility>

#include "common.hpp"
#include "graph.hpp"

namespace ldpc {

// Shared by the flood translation units (flood*.hip): counter rows, internal early-stop modes
// (see flood_drive) and the workspace views the kernels take.
constexpr int kPartRow = 8;  // uint32 per workgroup row
constexpr int ES_P1 = 3, ES_P2 = 4;

struct EsWs {
    uint64_t *words;   // ES_BATCH: [nwg][max_iter][Nb] ballots
    uint32_t *valid;   // ES_BATCH: [B][nvw] validity bit per iteration
    int nvw;
    uint64_t *cand;    // ES_P1: [nwg][Nb] ballots at t_wg
    int32_t *twg;      // ES_P1: [nwg] t_wg
    int32_t *ctl;      // [0] T = max t_wg  [1] bad  [2] fallback needed
    uint64_t *staged;  // [4] counters of the P2 result (applied by es_finalize_kernel)
};

struct Outs {
    int32_t *iters_out;
    uint32_t *partials;  // [nwg][kPartRow] counter rows (NULL: no counters wanted)
    uint64_t *timeline;  // LDPC_TIMELINE builds only (tools/flood_timeline.py): NULL otherwise
};

// Timeline build (-DLDPC_TIMELINE, tools/build_timeline.sh): lane 0 of every wave of the first
// kTlWgs workgroups stores s_memtime at each phase boundary of the iteration loop -- after the
// init barrier, then per iteration: check phase done, barrier 1 passed, variable phase done,
// barrier 2 passed -- so the waves each barrier waits on can be read off.
// The last three words of a wave's row (flood_fixed_kernel only) bracket the loop: the stamp at
// kernel entry (before make_lane), the stamp after the epilogue, and where the wave ran
// (XCC_ID << 32 | HW_ID), so that prologue, epilogue and the gap between a workgroup's exit and
// its successor's entry on the same CU can be read off.  The waves of one CU read the same
// s_memtime counter; the counters of different CUs are far apart, even inside one XCC (measured:
// ~2e8 units between the entry stamps of one generation), so stamps compare within a CU only.
constexpr int kTlWgs = 2048, kTlMaxIter = 16, kTlTail = 3, kTlPer = 2 + 4 * kTlMaxIter + kTlTail;
constexpr int kTlEntry = kTlPer - 3, kTlExit = kTlPer - 2, kTlWhere = kTlPer - 1;

namespace {

// Graph programs are read-only for the kernel's lifetime and indexed by wave-uniform values:
// reading them through the constant address space makes every word a scalar (SMEM) load.
typedef const __attribute__((address_space(4))) int32_t const_i32;
__device__ __forceinline__ int32_t tab(const int32_t *p, int i) { return ((const_i32 *)p)[i]; }

// compile-time loop: f(ic<0>{}), ..., f(ic<N-1>{})
template <int I>
using ic = std::integral_constant<int, I>;
template <class F, int... I>
__device__ __forceinline__ void sfor_impl(F &&f, std::integer_sequence<int, I...>) {
    (f(ic<I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void sfor(F &&f) {
    sfor_impl(f, std::make_integer_sequence<int, N>{});
}

struct Lane {
    int lane;      // 0..63 = f * Z + k
    int f, k;      // frame within the lane vector, row (or column position) within a block
    int lane4;     // 4 * lane: byte offset of this lane's entry in a slot
    int fz4;       // 4 * f * Z
    int k4;        // 4 * k
    int zmask4;    // 4 * Z - 1 (Z is a power of two)
    int z4;        // 4 * Z
    bool valid;    // the lane's frame exists
    int group;     // the workgroup's lane vector: frames group * FG ..  (the block index, except in a redo)
    int64_t frame;
    const char *llr_row;  // this lane's frame row (frame 0 for lanes without a frame)
    // byte offset inside a slot of the message on a block with byte shift s4, seen from the
    // variable at position k: row (k - s) mod Z of frame f
    __device__ __forceinline__ int vrot(int s4) const { return fz4 + ((k4 - s4) & zmask4); }
    // byte offset of variable (col, (k + s) mod Z) in an LLR row
    __device__ __forceinline__ int col_off(int col, int s4) const { return col * z4 + ((k4 + s4) & zmask4); }
    __device__ __forceinline__ int Z() const { return z4 >> 2; }
    __device__ __forceinline__ float llr_at(int byte_off) const {
        return *reinterpret_cast<const float *>(llr_row + byte_off);
    }
};

#ifdef LDPC_TIMELINE
// one asm statement with its own lgkmcnt(0) and scheduling fences around it: the builtin form
// leaves the wait's place to the compiler, which then drains LDS reads all over the loop
__device__ __forceinline__ uint64_t tl_now() {
    uint64_t t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
// entry / exit stamps and the place (XCC, SE, SH, CU, SIMD, wave slot) of this wave's decode
__device__ __forceinline__ void tl_bracket(uint64_t *timeline, int wave, uint64_t t_in) {
    const uint64_t t_out = tl_now();
    uint32_t hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)\n\ts_getreg_b32 %1, hwreg(HW_REG_XCC_ID)" : "=s"(hw), "=s"(xcc));
    if (timeline && blockIdx.x < (unsigned)kTlWgs && (threadIdx.x & 63) == 0) {
        uint64_t *tl = timeline + ((int64_t)blockIdx.x * 4 + wave) * kTlPer;
        tl[kTlEntry] = t_in;
        tl[kTlExit] = t_out;
        tl[kTlWhere] = ((uint64_t)xcc << 32) | hw;
    }
}
#endif

__device__ __forceinline__ float lds_rd(const char *lds, int off) { return *reinterpret_cast<const float *>(lds + off); }
// read at an absolute LDS byte address (the low half of a generic pointer into LDS) plus a
// compile-time offset: the offset lands in the instruction's immediate field and the address VGPR
// is used as it is (through a generic pointer, every use of a kept address costs a v_add of the
// LDS base, which the compiler rematerialises instead of keeping)
typedef const __attribute__((address_space(3))) float lds_cf32;
template <int OFF>
__device__ __forceinline__ float lds_rd_abs(uint32_t addr) {
    static_assert(OFF >= 0 && OFF < 65536, "ds offset is 16 bits");
    return *(lds_cf32 *)(uintptr_t)(addr + OFF);
}

// Lane t of every Z-lane segment takes v of lane (t - S) mod Z of its segment: ds_swizzle_b32, whose
// pattern sits in the offset field -- rotate mode over the 32 lanes of a half wave (0xC000 |
// amount << 5: lane i takes lane (i + amount) mod 32), quad mode over 4 (0x8000 | four 2-bit source
// selects).  An LDS instruction that touches no LDS memory and has no address operand: only the
// data VGPR crosses to the LDS unit, half of what ds_write_addtid_b32 + ds_read_b32 (or a
// ds_bpermute_b32) send.  The compiler counts it in lgkmcnt.  Every lane must be active: a masked
// source lane gives 0.
template <int Z, int S>
__device__ __forceinline__ float seg_rotate(float v) {
    static_assert(Z == 32 || Z == 4, "rotate mode turns 32 lanes, quad mode 4");
    static_assert(S >= 0 && S < Z, "a shift inside the segment");
    constexpr int sel = ((0 - S) & 3) | ((1 - S) & 3) << 2 | ((2 - S) & 3) << 4 | ((3 - S) & 3) << 6;
    constexpr int pattern = Z == 32 ? (0xC000 | ((32 - S) % 32) << 5) : (0x8000 | sel);
    return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), pattern));
}

// ds_write_addtid_b32: LDS[M0 + OFF + 4 * lane] = v.  No address VGPR, and half the LDS cycles of a
// ds_write_b32 (MI355X_MICROARCH.md, LDS table: 2 vs 4 per wave-instruction).  M0 must hold the
// LDS base (addtid_begin) and the compiler must not see these stores: callers drain them with
// addtid_end() (s_waitcnt lgkmcnt(0)) before any barrier or LDS read of the same bytes.
__device__ __forceinline__ void addtid_begin(const char *lds) {
    const uint32_t base = (uint32_t)(uintptr_t)lds;
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" : : "s"(base) : "memory");
}
template <int OFF>
__device__ __forceinline__ void lds_wr_tid(float v) {
    static_assert(OFF >= 0 && OFF < 65536, "addtid offset is 16 bits");
    asm volatile("ds_write_addtid_b32 %0 offset:%1" : : "v"(v), "i"(OFF) : "memory");
}
__device__ __forceinline__ void addtid_end() { asm volatile("s_waitcnt lgkmcnt(0)" : : : "memory"); }
__device__ __forceinline__ void lds_wr(char *lds, int off, float v) { *reinterpret_cast<float *>(lds + off) = v; }

__device__ __forceinline__ void put_bit(void *bits, int out_dtype, int64_t idx, int bit) {
    if (out_dtype == LDPC_OUT_F32)
        static_cast<float *>(bits)[idx] = bit ? 1.0f : 0.0f;
    else
        static_cast<uint8_t *>(bits)[idx] = (uint8_t)bit;
}

__device__ __forceinline__ bool is_zero_sign(float x) { return !(x > 0.0f || x < 0.0f); }
typedef float f32x2 __attribute__((ext_vector_type(2)));

// Min-sum statistics of one check row (traditional_decoders.py:207-232):
//   c2v_e = prod_{e'!=e} sign(v) * (alpha * min_{e'!=e} |v|)
// with torch.sign(0) = torch.sign(NaN) = 0 and NaN never winning the min (mag < min_mag fails).
struct MinSumStats {
    int nz = 0;         // number of zero/NaN signs in the row
    bool neg = false;   // parity of negative signs
    float m1 = INFINITY, m2 = INFINITY;
    int i1 = -1;        // first index attaining m1
    __device__ __forceinline__ void add(int e, float x) {
        const float a = fabsf(x);
        nz += is_zero_sign(x);
        neg ^= (x < 0.0f);
        const bool lt1 = a < m1, lt2 = a < m2;  // NaN: both false
        m2 = lt1 ? m1 : (lt2 ? a : m2);
        i1 = lt1 ? e : i1;
        m1 = lt1 ? a : m1;
    }
    __device__ __forceinline__ float c2v(int e, float x, float alpha) const {
        const float m = (e == i1) ? m2 : m1;
        const int zex = nz - (int)is_zero_sign(x);
        const float s = zex > 0 ? 0.0f : ((neg ^ (x < 0.0f)) ? -1.0f : 1.0f);
        return s * (alpha * m);
    }
};

// Fast path of the same update for a row with no zero and no NaN message (every row, in practice;
// a wave takes it when none of its 64 rows has one).  Then torch.sign is +-1, so
//   * the sign parity is the XOR of the sign bits, and the output sign is parity ^ signbit(x);
//   * the two smallest magnitudes are a min/max network (v_min/v_max are exact, NaN-free here);
//   * the excluded minimum is m2 exactly when |x| == m1: a tie at m1 puts m1 in m2 as well, so
//     no first-index bookkeeping is needed.
// Every output is bit-identical to MinSumStats::c2v: +-(alpha * m) with the same alpha * m.
// xor of the messages' bit patterns (its sign bit = the row's sign parity): v_bitop3_b32 with the
// three-input xor table (0x96) takes two messages per instruction (the compiler keeps a chain of
// two-input xors here)
template <int DC, int CAP>
__device__ __forceinline__ uint32_t sign_parity_n(const float (&v)[CAP]) {
    static_assert(DC <= CAP, "row longer than its buffer");
    uint32_t p = __float_as_uint(v[0]);
#pragma unroll
    for (int e = 1; e + 1 < DC; e += 2)
        asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(p) : "v"(p), "v"(v[e]), "v"(v[e + 1]));
    if constexpr (DC % 2 == 0) p ^= __float_as_uint(v[DC - 1]);
    return p;
}

// m2 = median(m1, |x|, m2) then m1 = min(m1, |x|): the two smallest magnitudes of a row with no
// NaN (v_min / v_med3 with |x| as a source modifier; fminf would add a NaN-quieting v_max)
// -inf in a VGPR the compiler cannot see through: med3(m, |x|, -inf) = min(m, |x|) for non-NaN
// operands, and an opaque third operand keeps the compiler from turning it back into a
// canonicalising fminf
// (an SGPR: one scalar operand per v_med3 is within the constant-bus limit)
__device__ __forceinline__ float opaque_sf(float v) {
    asm volatile("" : "+s"(v));
    return v;
}
// a uniform constant held in a VGPR: a VALU op with an SGPR source issues at half rate
__device__ __forceinline__ uint32_t opaque_vu(uint32_t v) {
    asm volatile("" : "+v"(v));
    return v;
}
__device__ __forceinline__ float opaque_vf(float v) {
    asm volatile("" : "+v"(v));
    return v;
}
__device__ __forceinline__ void two_min_step(float &m1, float &m2, float x, float ninf) {
    // builtins, not inline asm: a VALU reading a VGPR written by inline asm gets a conservative
    // s_nop from the hazard recognizer (one per edge in the check phase)
    m2 = __builtin_amdgcn_fmed3f(m1, fabsf(x), m2);
    m1 = __builtin_amdgcn_fmed3f(m1, fabsf(x), ninf);
}

// The two smallest magnitudes of a row with no NaN, three messages per step: the smallest and the
// middle of a triple are one v_minimum3 and one v_med3 (|x| as source modifiers), and a sorted
// pair (m1 <= m2) absorbs a sorted pair (t1 <= t2) as m1' = min(m1, t1),
// m2' = min(max(m1, t1), m2, t2) -- 5 ops per further triple, 2 per leftover message, against 2 per
// message for the running med3 / min chain (BG2: 217 instead of 310 of these half-rate ops per
// base-graph iteration).  Every op returns one of its inputs: the pair (m1, m2) is bit-identical.
// minimum / maximum (IEEE, NaN-propagating) need no canonicalising v_max, unlike fminf.
__device__ __forceinline__ float vmin(float a, float b) { return __builtin_elementwise_minimum(a, b); }
__device__ __forceinline__ float vmax(float a, float b) { return __builtin_elementwise_maximum(a, b); }
template <int DC, int CAP>
__device__ __forceinline__ void two_smallest(const float (&v)[CAP], float &m1, float &m2, float ninf) {
    static_assert(DC <= CAP, "row longer than its buffer");
    if constexpr (DC == 1) {
        m1 = fabsf(v[0]);
    } else if constexpr (DC == 2) {
        m1 = vmin(fabsf(v[0]), fabsf(v[1]));
        m2 = vmax(fabsf(v[0]), fabsf(v[1]));
    } else {
        m1 = vmin(vmin(fabsf(v[0]), fabsf(v[1])), fabsf(v[2]));
        m2 = __builtin_amdgcn_fmed3f(fabsf(v[0]), fabsf(v[1]), fabsf(v[2]));
        constexpr int NT = (DC - 3) / 3;  // further whole triples
        sfor<NT>([&](auto q) {
            constexpr int B0 = 3 + 3 * decltype(q)::value;
            const float a = fabsf(v[B0]), b = fabsf(v[B0 + 1]), c = fabsf(v[B0 + 2]);
            const float t1 = vmin(vmin(a, b), c), t2 = __builtin_amdgcn_fmed3f(a, b, c);
            m2 = vmin(vmin(vmax(m1, t1), m2), t2);
            m1 = vmin(m1, t1);
        });
        sfor<DC - 3 - 3 * NT>([&](auto q) { two_min_step(m1, m2, v[3 + 3 * NT + decltype(q)::value], ninf); });
    }
}

// lane mask of |x| == m (v_cmp_eq_f32 into an SGPR pair) and a select by it; volatile so that the
// issue order written by the caller is kept
__device__ __forceinline__ uint64_t cmp_eq_abs(float x, float m) {
    uint64_t k;
    asm volatile("v_cmp_eq_f32_e64 %0, |%1|, %2" : "=s"(k) : "v"(x), "v"(m));
    return k;
}
__device__ __forceinline__ uint32_t cndmask(uint32_t if0, uint32_t if1, uint64_t k) {
    uint32_t r;
    asm volatile("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(if0), "v"(if1), "s"(k));
    return r;
}

struct MinSumFast {
    float m1 = INFINITY, m2 = INFINITY;
    uint32_t par = 0;
    bool special = false;  // a zero or NaN message: the row needs MinSumStats
    __device__ __forceinline__ void add(float x) {
        const float a = fabsf(x);
        special |= is_zero_sign(x);
        // m2 = min(m2, max(m1, a)) = median(m1, a, m2) since m1 <= m2: one v_med3_f32 with |x|
        // as a source modifier.  m1 = min(m1, |x|) as one v_min_f32 in asm: fminf (and a med3
        // with -inf, which the compiler turns back into it) adds a NaN-quieting v_max per edge,
        // and this path never sees a NaN (special -> MinSumStats).
        m2 = __builtin_amdgcn_fmed3f(m1, a, m2);
        asm("v_min_f32 %0, %1, |%2|" : "=v"(m1) : "v"(m1), "v"(x));
    }
    // s1 / s2 = |alpha m1| / |alpha m2| with the row's sign parity in the sign bit (sel_words);
    // the message's own sign bit is xored back out: out = (x & SIGN) ^ sel (one v_bitop3)
    __device__ __forceinline__ float c2v(float x, uint32_t s1, uint32_t s2) const {
        const uint32_t sel = fabsf(x) == m1 ? s2 : s1;
        return __uint_as_float((__float_as_uint(x) & 0x80000000u) ^ sel);
    }
    __device__ __forceinline__ void sel_words(float alpha, uint32_t &s1, uint32_t &s2) const {
        const uint32_t ps = par & 0x80000000u;
        s1 = __float_as_uint(fabsf(alpha * m1)) | ps;
        s2 = __float_as_uint(fabsf(alpha * m2)) | ps;
    }
};

// float32 tanh / atanh, branch-free, a few ulp (the reference calls torch-CPU's float32 SLEEF
// versions, 1 ulp; neither is correctly rounded).  Small arguments: the odd minimax polynomials of
// the Cephes float library (tanh |y| < 0.625, atanh |p| < 0.5; 1.1 and 1.4 ulp in float
// arithmetic); larger ones: the exp / log forms on the hardware v_exp_f32 / v_log_f32 / v_rcp_f32.
// Measured against double on the device (tests/test_bp_math_gpu.py, every float32 around the branch
// switches and 4096 per binary exponent): tanh_half <= 1.75e-7 relative (1.63 ulp, the same with
// exact exp2 / rcp), two_atanh <= 2.01e-7 (2.58 ulp; 1.63e-7 / 1.92 ulp with exact rcp / log2); the
// tests' bar is 3e-7.  Saturation as in the reference: |tanh| <= 1 always, +-1 for |y| >~ 9, -0 at
// -0, and 2 atanh(+-1) = +-inf; NaN goes through both.  ~16 + ~18 VALU per edge against ~130 for
// the ROCm libm calls (and 4x that for double).
__device__ __forceinline__ float tanh_half(float v) {
    const float y = v * 0.5f;  // exact, = v / 2
    const float a = fabsf(y), z = y * y;
    float p = fmaf(-5.70498872745e-3f, z, 2.06390887954e-2f);
    p = fmaf(p, z, -5.37397155531e-2f);
    p = fmaf(p, z, 1.33314422036e-1f);
    p = fmaf(p, z, -3.33332819422e-1f);
    // both branches on |y|, the sign put back last: fmaf(p * z, y, y) is (+0) + (-0) = +0 at y = -0,
    // and tanh(-0) is -0 (for y != 0 this is the same bits: rounding to nearest is symmetric)
    const float small = fmaf(p * z, a, a);
    const float e = __builtin_amdgcn_exp2f(a * 2.88539008177792681f);  // exp(2a)
    const float big = fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);
    return copysignf(a < 0.625f ? small : big, y);
}
__device__ __forceinline__ float two_atanh(float x) {
    const float z = x * x;
    float p = fmaf(1.81740078349e-1f, z, 8.24370301058e-2f);
    p = fmaf(p, z, 1.46691431730e-1f);
    p = fmaf(p, z, 1.99782164500e-1f);
    p = fmaf(p, z, 3.33337300303e-1f);
    const float small = 2.0f * fmaf(p * z, x, x);
    // log((1 + x) / (1 - x)); 1 - x is exact for x >= 0.5, (1 + x) * rcp(0) = +inf at x = 1
    const float r = (1.0f + x) * __builtin_amdgcn_rcpf(1.0f - x);
    const float big = __builtin_amdgcn_logf(r) * 0.693147180559945309f;
    return fabsf(x) < 0.5f ? small : big;
}

struct Ctx {
    FloodTables T;
    char *lds;
    uint64_t *words;  // ES: Nb decision ballots + 1 invalid-lane word (in LDS)
    uint32_t *flag;   // LDS: sticky "a v2c may be NaN" flag of the fixed kernel's fast check path
    uint32_t *redo;   // bail-out instances (Body::kBail): [0] count, [1 ..] groups to decode again
    float alpha;
    int out_dtype;
    void *bits;
    bool direct_bits;  // mode 0, final iteration: write decisions straight to HBM (flood_kernel; the
                       // fixed kernel's bodies take it as a template parameter, DIRECT)
    bool ballots;      // ES: record decisions as ballots
};

// rotate each z-bit segment of w left by s (0 <= s < z; z a power of two dividing 64), given
// rep1 = the word with a 1 at the bottom of every segment (scalar ops: w and rep1 are uniform)
__device__ __forceinline__ uint64_t seg_rotl(uint64_t w, int s, int z, uint64_t rep1) {
    if (s == 0) return w;
    if (z >= 64) return (w << s) | (w >> (64 - s));
    const uint64_t low = ((1ull << (z - s)) - 1ull) * rep1;  // the low z - s bits of every segment
    return ((w & low) << s) | ((w & ~low) >> (z - s));
}

// the decisions of column col as a ballot word: bit f*Z + t is variable t of frame f
__device__ __forceinline__ void var_ballot(const Ctx &C, const Lane &L, int col, int bit) {
    const uint64_t w = __ballot(bit);
    if (L.lane == 0) C.words[col] = w;
}
// the same from the lanes of check row k, where lane f*Z + k holds variable (k + s) mod Z: rotate
// every Z-bit segment of the ballot left by s (uniform, scalar) so that bit f*Z + t is variable t
__device__ __forceinline__ void ext_ballot(const Ctx &C, const Lane &L, int col, int s4, int bit) {
    const uint64_t w = seg_rotl(__ballot(bit), s4 >> 2, C.T.Z, C.T.rep1);
    if (L.lane == 0) C.words[col] = w;
}

// decision of variable (col, (k + s) mod Z) computed on the lane of check row k (the table-driven
// kernel's form; the fixed kernel stores through FixedBody's DecOut)
__device__ __forceinline__ void ext_decision(const Ctx &C, const Lane &L, int col, int s4, float app,
                                             int &errs) {
    const int bit = app < 0.0f;  // NaN < 0 is false -> 0 (traditional_decoders.py:252)
    if (C.direct_bits && L.valid) {
        // the empty asm keeps the (final-iteration only) 64-bit output address from being
        // hoisted out of the iteration loop, where it would hold registers for nothing
        int64_t fr = L.frame;
        int k4 = L.k4;
        asm volatile("" : "+v"(fr), "+v"(k4));
        put_bit(C.bits, C.out_dtype, fr * C.T.N + (col * L.z4 + ((k4 + s4) & L.zmask4)) / 4, bit);
        errs += bit;
    }
    if (C.ballots) ext_ballot(C, L, col, s4, bit);
}

__device__ __forceinline__ void var_decision(const Ctx &C, const Lane &L, int col, float app, int &errs) {
    const int bit = app < 0.0f;
    if (C.direct_bits && L.valid) {
        int64_t fr = L.frame;
        int k = L.k;
        asm volatile("" : "+v"(fr), "+v"(k));
        put_bit(C.bits, C.out_dtype, fr * C.T.N + (int64_t)col * L.Z() + k, bit);
        errs += bit;
    }
    if (C.ballots) var_ballot(C, L, col, bit);
}

// ---------------------------------------------------------------- check node update
// prog points at the row's first edge word (uniform); DC compile-time.
template <int ALGO, int DC>
__device__ __forceinline__ void check_task(const Ctx &C, const Lane &L, const int32_t *prog, int &errs) {
    float v[DC];
    int32_t w[DC];
#pragma unroll
    for (int e = 0; e < DC; ++e) {
        w[e] = tab(prog, e);
        const int lo = w[e] & kLowMask, s4 = (w[e] >> kShiftBit) & 0xFF;
        v[e] = w[e] < 0 ? L.llr_at(L.col_off(lo, s4)) : lds_rd(C.lds, lo + L.lane4);
    }
    auto emit = [&](int e, float o) {
        const int lo = w[e] & kLowMask;
        if (w[e] >= 0)
            lds_wr(C.lds, lo + L.lane4, o);
        else if (C.direct_bits || C.ballots)  // degree-1 variable: APP = llr.clone() + c2v
            ext_decision(C, L, lo, (w[e] >> kShiftBit) & 0xFF, v[e] + o, errs);
    };
    if constexpr (ALGO == LDPC_ALGO_MINSUM) {
        MinSumFast fs;
#pragma unroll
        for (int e = 0; e < DC; ++e) fs.add(v[e]);
        fs.par = sign_parity_n<DC>(v);
        if (!__any(fs.special)) {  // wave-uniform
            uint32_t s1, s2;
            fs.sel_words(C.alpha, s1, s2);
#pragma unroll
            for (int e = 0; e < DC; ++e) emit(e, fs.c2v(v[e], s1, s2));
        } else {
            MinSumStats st;
#pragma unroll
            for (int e = 0; e < DC; ++e) st.add(e, v[e]);
#pragma unroll
            for (int e = 0; e < DC; ++e) emit(e, st.c2v(e, v[e], C.alpha));
        }
    } else {
        // sum-product (traditional_decoders.py:72-81): c2v_e = 2 atanh(prod_{e'!=e} tanh(v/2)),
        // product from 1.0 in ascending e'.  acc[e] = P_e * t_{e+1} * ... built column by column.
        float acc[DC];
        float P = 1.0f;
#pragma unroll
        for (int j = 0; j < DC; ++j) {
            const float t = tanh_half(v[j]);
#pragma unroll
            for (int e = 0; e < j; ++e) acc[e] = acc[e] * t;
            acc[j] = P;
            P = P * t;
        }
#pragma unroll
        for (int e = 0; e < DC; ++e) emit(e, two_atanh(acc[e]));
    }
}

// Any degree: messages re-read instead of kept in registers (O(dc^2) reads; used past the
// unrolled range).  In-place is safe in ascending e: slot e is overwritten after P_{e+1} used it.
template <int ALGO>
__device__ __forceinline__ void check_task_dyn(const Ctx &C, const Lane &L, const int32_t *prog, int dc,
                                               int &errs) {
    auto rd = [&](int e) -> float {
        const int32_t w = tab(prog, e);
        const int lo = w & kLowMask;
        return w < 0 ? L.llr_at(L.col_off(lo, (w >> kShiftBit) & 0xFF)) : lds_rd(C.lds, lo + L.lane4);
    };
    auto wr = [&](int e, float in, float out) {
        const int32_t w = tab(prog, e);
        const int lo = w & kLowMask;
        if (w >= 0)
            lds_wr(C.lds, lo + L.lane4, out);
        else if (C.direct_bits || C.ballots)
            ext_decision(C, L, lo, (w >> kShiftBit) & 0xFF, in + out, errs);
    };
    if constexpr (ALGO == LDPC_ALGO_MINSUM) {
        MinSumStats st;
        for (int e = 0; e < dc; ++e) st.add(e, rd(e));
        for (int e = 0; e < dc; ++e) {
            const float x = rd(e);
            wr(e, x, st.c2v(e, x, C.alpha));
        }
    } else {
        float P = 1.0f;
        for (int e = 0; e < dc; ++e) {
            const float x = rd(e);
            float rr = P;
            for (int q = e + 1; q < dc; ++q) rr = rr * tanh_half(rd(q));
            const float t = tanh_half(x);
            wr(e, x, two_atanh(rr));
            P = P * t;
        }
    }
}

// ---------------------------------------------------------------- variable node update
// Variable update (traditional_decoders.py:235-250): v2c_e = llr + sum_{e'!=e} c_e' added in
// ascending check order, i.e. acc[e] = P_e (prefix) followed by c_{e+1}, c_{e+2}, ...;
// the APP is P_DV = llr + c_0 + ... + c_{DV-1}.
template <int DV>
__device__ __forceinline__ void var_task(const Ctx &C, const Lane &L, const int32_t *prog, int col, bool write,
                                         int &errs) {
    float P = L.llr_at(col * L.z4 + L.k4);
    if constexpr (DV > 0) {
        float acc[DV];
        int off[DV];
#pragma unroll
        for (int j = 0; j < DV; ++j) {
            const int32_t w = tab(prog, j);
            off[j] = (w & kLowMask) + L.vrot((w >> kShiftBit) & 0xFF);
            const float c = lds_rd(C.lds, off[j]);
#pragma unroll
            for (int e = 0; e < j; ++e) acc[e] = acc[e] + c;
            acc[j] = P;
            P = P + c;
        }
        if (write) {
#pragma unroll
            for (int e = 0; e < DV; ++e) lds_wr(C.lds, off[e], acc[e]);
        }
    }
    if (C.direct_bits || C.ballots) var_decision(C, L, col, P, errs);
}

__device__ __forceinline__ void var_task_dyn(const Ctx &C, const Lane &L, const int32_t *prog, int dv, int col,
                                             bool write, int &errs) {
    auto off = [&](int e) {
        const int32_t w = tab(prog, e);
        return (w & kLowMask) + L.vrot((w >> kShiftBit) & 0xFF);
    };
    float P = L.llr_at(col * L.z4 + L.k4);
    for (int e = 0; e < dv; ++e) {
        const int o = off(e);
        const float cp = lds_rd(C.lds, o);
        float acc = P;
        for (int q = e + 1; q < dv; ++q) acc = acc + lds_rd(C.lds, off(q));
        P = P + cp;
        if (write) lds_wr(C.lds, o, acc);
    }
    if (C.direct_bits || C.ballots) var_decision(C, L, col, P, errs);
}

// degrees with unrolled register code; larger ones take the *_dyn paths
#define LDPC_DC_CASES(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12)
#define LDPC_DV_CASES(X) \
    X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) \
    X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24)

// run this wave's check program
template <int ALGO>
__device__ __forceinline__ void check_phase(const Ctx &C, const Lane &L, int wave, int &errs) {
    const int p1 = tab(C.T.prog_ptr, wave + 1);
    for (int pc = tab(C.T.prog_ptr, wave); pc < p1;) {
        const int dc = tab(C.T.chk_prog, pc);
        const int32_t *prog = C.T.chk_prog + pc + 1;
        switch (dc) {
            case 0: break;
#define X(n) case n: check_task<ALGO, n>(C, L, prog, errs); break;
            LDPC_DC_CASES(X)
#undef X
            default: check_task_dyn<ALGO>(C, L, prog, dc, errs); break;
        }
        pc += 1 + dc;
    }
}

__device__ __forceinline__ void var_phase(const Ctx &C, const Lane &L, int wave, bool write, int &errs) {
    const int W1 = C.T.W + 1;
    const int p1 = tab(C.T.prog_ptr, W1 + wave + 1);
    for (int pc = tab(C.T.prog_ptr, W1 + wave); pc < p1;) {
        const int h = tab(C.T.var_prog, pc);
        const int dv = h & 0xFF, col = h >> 8;
        const int32_t *prog = C.T.var_prog + pc + 1;
        switch (dv) {
            case 0: var_task<0>(C, L, prog, col, write, errs); break;
#define X(n) case n: var_task<n>(C, L, prog, col, write, errs); break;
            LDPC_DV_CASES(X)
#undef X
            default: var_task_dyn(C, L, prog, dv, col, write, errs); break;
        }
        pc += 1 + dv;
    }
}

// v2c <- llr on every slot (traditional_decoders.py:199-202)
__device__ __forceinline__ void init_phase(const Ctx &C, const Lane &L, int wave) {
    const int W1 = C.T.W + 1;
    const int p1 = tab(C.T.prog_ptr, W1 + wave + 1);
    for (int pc = tab(C.T.prog_ptr, W1 + wave); pc < p1;) {
        const int h = tab(C.T.var_prog, pc);
        const int dv = h & 0xFF, col = h >> 8;
        const float x = L.llr_at(col * L.z4 + L.k4);
        for (int e = 0; e < dv; ++e) {
            const int32_t w = tab(C.T.var_prog, pc + 1 + e);
            lds_wr(C.lds, (w & kLowMask) + L.vrot((w >> kShiftBit) & 0xFF), x);
        }
        pc += 1 + dv;
    }
}

// syndrome of this wave's rows from the ballots: 1 if any of its checks fails for this lane
__device__ __forceinline__ int parity_phase(const Ctx &C, const Lane &L, int wave) {
    const int W1 = C.T.W + 1;
    const int p1 = tab(C.T.prog_ptr, 2 * W1 + wave + 1);
    int inv = 0;
    for (int pc = tab(C.T.prog_ptr, 2 * W1 + wave); pc < p1;) {
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

__device__ __forceinline__ uint64_t frame_valid_mask(uint64_t invalid_lanes, int Z, int FG) {
    const uint64_t seg = Z >= 64 ? ~0ull : ((1ull << Z) - 1ull);
    uint64_t m = 0;
    for (int f = 0; f < FG; ++f)
        if (((invalid_lanes >> (f * Z)) & seg) == 0) m |= 1ull << f;
    return m;
}

// emit the decisions of frames in `mask` from the ballots (columns spread over the waves)
__device__ __forceinline__ void emit_from_words(const Ctx &C, const Lane &L, const uint64_t *words, uint64_t mask,
                                                int wave, int &errs) {
    if (!(L.valid && ((mask >> L.f) & 1ull))) return;
    const int W1 = C.T.W + 1;
    for (int i = tab(C.T.prog_ptr, 3 * W1 + wave); i < tab(C.T.prog_ptr, 3 * W1 + wave + 1); ++i) {
        const int col = tab(C.T.bw_task, i);
        const int bit = (int)((words[col] >> L.lane) & 1ull);
        put_bit(C.bits, C.out_dtype, L.frame * C.T.N + (int64_t)col * L.Z() + L.k, bit);
        errs += bit;
    }
}

// per-workgroup totals of the error counters, written to this workgroup's row of the partials
// array (no global atomics: 32 768 workgroups adding into the same 4 words serialise at L2):
//   row = {bit errors, frame errors, frames, iteration sum, max iterations}
// counters_reduce_kernel folds the rows into the caller's counters afterwards.
__device__ __forceinline__ void reduce_counters(void *lds, const Lane &L, int errs, int my_iters, int nf,
                                                int Z, uint32_t *row) {
    uint32_t *u = reinterpret_cast<uint32_t *>(lds);
    const int nt = blockDim.x;
    __syncthreads();
    u[threadIdx.x] = (uint32_t)errs;
    u[nt + threadIdx.x] = (uint32_t)my_iters;
    __syncthreads();
    if (threadIdx.x < 64) {
        const int f = threadIdx.x;
        uint32_t be = 0, fe = 0, fr = 0, it = 0, itmax = 0;
        if (f < nf) {
            for (int w = 0; w < nt / 64; ++w)
                for (int k = 0; k < Z; ++k) be += u[w * 64 + f * Z + k];
            fe = be > 0;
            fr = 1;
            it = u[nt + f * Z];
            itmax = it;
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

__device__ __forceinline__ Lane make_lane(const FloodTables &T, const float *llr, int64_t B, int group) {
    Lane L;
    L.group = group;
    L.lane = threadIdx.x & 63;
    const int lz = __builtin_ctz((unsigned)T.Z);  // Z is a power of two
    L.f = L.lane >> lz;
    L.k = L.lane & (T.Z - 1);
    L.lane4 = 4 * L.lane;
    L.fz4 = 4 * (L.f << lz);
    L.k4 = 4 * L.k;
    L.z4 = 4 * T.Z;
    L.zmask4 = 4 * T.Z - 1;
    L.frame = (int64_t)group * T.FG + L.f;
    L.valid = L.frame < B;
    L.llr_row = reinterpret_cast<const char *>(llr ? llr + (L.valid ? L.frame : 0) * (int64_t)T.N : nullptr);
    return L;
}
__device__ __forceinline__ Lane make_lane(const FloodTables &T, const float *llr, int64_t B) {
    return make_lane(T, llr, B, (int)blockIdx.x);
}

// ---------------------------------------------------------------- early stop: internal modes
// Public early_stop values are LDPC_ES_OFF / LDPC_ES_BATCH / LDPC_ES_FRAME.  The reference's
// batch-global rule (stop at the first iteration at which EVERY frame satisfies H x = 0 and return
// that iteration's decisions, traditional_decoders.py:104-107) runs as up to three passes, so that
// a batch that converges after t iterations costs about t iterations, not max_iter:
//   ES_P1     each workgroup iterates until all of ITS frames are valid at the same iteration
//             t_wg (or max_iter), keeps that iteration's decision ballots; T = max over t_wg.
//             No iteration before T can be valid for the whole batch.
//   ES_P2     workgroups with t_wg == T emit their kept ballots; the others decode T iterations
//             again and emit; a frame that is not valid at T (with T < max_iter) raises `bad`.
//   ES_BATCH  (runs only when bad) the exhaustive search: decode max_iter iterations keeping every
//             iteration's ballots and validity bits; batch_and / batch_emit take the first
//             iteration at which every frame is valid.
// es_finalize_kernel between P2 and the fallback decides, on the device, which result stands.

// The iteration loop shared by both kernels.  Body supplies the four per-wave phases:
//   init(C, L)             v2c <- llr on every slot
//   check(C, L, errs)      c2v of this wave's check rows, in place
//   var(C, L, write, errs) v2c (write) and APP of this wave's columns; decisions when asked
//   parity(C, L) -> int    1 if any of this wave's checks fails for this lane (needs ballots)
// Every branch below depends on workgroup-uniform values only, so all waves meet the same
// barriers even when Body is specialised per wave.
template <int ES, class Body>
__device__ __forceinline__ void flood_drive(Body &body, Ctx &C, const Lane &L, int64_t B, int max_iter,
                                            const Outs &O, const EsWs &W) {
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int FG = C.T.FG, Nb = C.T.Nb, Z = C.T.Z;
    const int nf = (int)min<int64_t>((int64_t)FG, B - (int64_t)L.group * FG);
    const uint64_t exist = nf >= 64 ? ~0ull : ((1ull << nf) - 1ull);
    int errs = 0;
    if constexpr (ES == LDPC_ES_BATCH) {
        if (__builtin_amdgcn_readfirstlane(W.ctl[2]) == 0) return;  // the fast passes stood
    }
    if constexpr (ES == ES_P2) {
        const int T = __builtin_amdgcn_readfirstlane(W.ctl[0]);
        if (__builtin_amdgcn_readfirstlane(W.twg[L.group]) == T) {
            emit_from_words(C, L, W.cand + (int64_t)L.group * Nb, exist, wave, errs);
            if (O.iters_out && L.valid && L.k == 0) O.iters_out[L.frame] = T;
            reduce_counters(C.lds, L, errs, T, nf, Z, O.partials + (int64_t)L.group * kPartRow);
            return;
        }
        max_iter = T;
    }
    if (tid == 0) *C.flag = 0;
    __syncthreads();
    body.init(C, L);
    __syncthreads();
#ifdef LDPC_TIMELINE
    uint64_t *tl = (O.timeline && blockIdx.x < (unsigned)kTlWgs && L.lane == 0)
                       ? O.timeline + ((int64_t)blockIdx.x * 4 + wave) * kTlPer : nullptr;
    auto mark = [&](int k) {
        const uint64_t t = tl_now();
        if (tl && k < kTlPer - kTlTail) tl[k] = t;
    };
#else
    auto mark = [](int) {};
#endif
    mark(0);

    int my_iters = max_iter;
    uint64_t done = 0;
    constexpr bool kEvery = ES == LDPC_ES_BATCH || ES == LDPC_ES_FRAME || ES == ES_P1;  // ballots every iteration
    // One iteration.  ES_OFF and ES_P2 take decisions in the last iteration only: where the body
    // asks for it (Body::kPeel) their loop runs the iterations before it (WHEN 0: no decision code,
    // no store to global memory, ballots and direct_bits constant) and the last one follows the
    // loop as straight code (WHEN 1: decisions stored directly, DIRECT, and no v2c written).
    // Otherwise one loop holds both forms (WHEN 2: `last` is a run-time value); the modes that
    // take decisions, as ballots, in every iteration always do.  The barriers of an iteration are
    // the same in every form.
    // -> kGoOn, kStop (early stop: leave the loop) or kLeft (bail-out: the workgroup has left the decode)
    constexpr int kGoOn = 0, kStop = 1, kLeft = 2;
    constexpr bool kPeel = !kEvery && Body::kPeel;
    auto iteration = [&](auto when, int it) __attribute__((always_inline)) -> int {
        constexpr int WHEN = decltype(when)::value;
        static_assert(kPeel ? WHEN < 2 : WHEN == 2, "the last iteration is peeled or it is not");
        const bool last = WHEN == 2 ? it == max_iter - 1 : WHEN == 1;
        constexpr bool DIRECT = WHEN == 1;
        C.direct_bits = !kEvery && last;
        C.ballots = kEvery || (ES == ES_P2 && last);
        if constexpr (Body::kBail) {
            // Bail-out instances hold the fast check update only.  The sticky flag (a non-finite
            // LLR or APP: a message may be NaN) is read here by every wave after a barrier and
            // written only between the next two, so the branch is workgroup-uniform: the group is
            // appended to the redo list and decoded again, from its LLRs, by flood_redo_kernel.
            // Whatever this workgroup has emitted so far is rewritten there; no counter row yet.
            if (__builtin_expect(__builtin_amdgcn_readfirstlane(*C.flag) != 0, 0)) {
                if (tid == 0) C.redo[1 + atomicAdd(C.redo, 1u)] = (uint32_t)L.group;
                return kLeft;
            }
        }
        // decisions are taken only in the iterations that need them (DEC = true), so the other
        // iterations carry no decision code at all
        if constexpr (WHEN == 0) {
            body.template check<false, false>(C, L, errs);
        } else if constexpr (WHEN == 1 || kEvery) {
            body.template check<true, DIRECT>(C, L, errs);
        } else {
            if (last)
                body.template check<true, false>(C, L, errs);
            else
                body.template check<false, false>(C, L, errs);
        }
        mark(1 + 4 * it);
        __syncthreads();
        mark(2 + 4 * it);
        if (C.ballots && tid == 0) C.words[Nb] = 0;
        if constexpr (WHEN == 0) {
            body.template var<false, true, false>(C, L, errs);
        } else if constexpr (WHEN == 1) {
            body.template var<true, false, DIRECT>(C, L, errs);
        } else {
            if (last)
                body.template var<true, false, false>(C, L, errs);
            else if (kEvery)
                body.template var<true, true, false>(C, L, errs);
            else
                body.template var<false, true, false>(C, L, errs);
        }
        mark(3 + 4 * it);
        __syncthreads();
        mark(4 + 4 * it);
        bool stop = false;
        if (C.ballots) {
            // syndrome H x = 0 per frame (traditional_decoders.py:111-134), from the ballots
            const uint64_t m = __ballot(body.parity(C, L));
            if (L.lane == 0 && m) atomicOr((unsigned long long *)&C.words[Nb], (unsigned long long)m);
            __syncthreads();
            const uint64_t vmask = frame_valid_mask(C.words[Nb], Z, FG) & exist;
            if constexpr (ES == LDPC_ES_BATCH) {
                if (L.valid && L.k == 0 && ((vmask >> L.f) & 1ull))
                    W.valid[L.frame * W.nvw + (it >> 5)] |= 1u << (it & 31);
                uint64_t *dst = W.words + ((int64_t)L.group * max_iter + it) * Nb;
                for (int c = tid; c < Nb; c += blockDim.x) dst[c] = C.words[c];
            } else if constexpr (ES == LDPC_ES_FRAME) {
                const uint64_t newly = vmask & ~done;
                if (newly) {
                    emit_from_words(C, L, C.words, newly, wave, errs);
                    if ((newly >> L.f) & 1ull) my_iters = it + 1;
                    if (O.iters_out && L.valid && L.k == 0 && ((newly >> L.f) & 1ull)) O.iters_out[L.frame] = it + 1;
                    done |= newly;
                }
                stop = done == exist;
            } else if constexpr (ES == ES_P1) {
                stop = vmask == exist || last;
                if (stop) {
                    uint64_t *dst = W.cand + (int64_t)L.group * Nb;
                    for (int c = tid; c < Nb; c += blockDim.x) dst[c] = C.words[c];
                    if (tid == 0) {
                        W.twg[L.group] = it + 1;
                        atomicMax(&W.ctl[0], it + 1);
                    }
                }
            } else if constexpr (ES == ES_P2) {
                if (vmask != exist && tid == 0) atomicOr(&W.ctl[1], 1);
            }
            __syncthreads();
        }
        return stop ? kStop : kGoOn;
    };
    if constexpr (!kPeel) {
        for (int it = 0; it < max_iter; ++it) {
            const int r = iteration(ic<2>{}, it);
            if (r == kLeft) return;
            if (r == kStop) break;
        }
    } else {
        for (int it = 0; it < max_iter - 1; ++it)
            if (iteration(ic<0>{}, it) == kLeft) return;
        if (max_iter > 0 && iteration(ic<1>{}, max_iter - 1) == kLeft) return;
    }
    if constexpr (ES == LDPC_ES_FRAME) {
        const uint64_t rest = exist & ~done;
        if (rest) {
            emit_from_words(C, L, C.words, rest, wave, errs);
            if (O.iters_out && L.valid && L.k == 0 && ((rest >> L.f) & 1ull)) O.iters_out[L.frame] = max_iter;
        }
    }
    if constexpr (ES == LDPC_ES_OFF || ES == ES_P2) {
        if (O.iters_out && L.valid && L.k == 0) O.iters_out[L.frame] = max_iter;
    }
    if constexpr (ES == LDPC_ES_OFF || ES == LDPC_ES_FRAME) {
        if (O.partials) reduce_counters(C.lds, L, errs, my_iters, nf, Z, O.partials + (int64_t)L.group * kPartRow);
    }
    if constexpr (ES == ES_P2) reduce_counters(C.lds, L, errs, max_iter, nf, Z, O.partials + (int64_t)L.group * kPartRow);
}

template <int ALGO>
struct GenericBody {
    static constexpr bool kBail = false;  // its check update handles every value
    static constexpr bool kPeel = false;  // one loop: decisions are a run-time matter here (C.direct_bits)
    int wave;
    __device__ __forceinline__ void init(Ctx &C, const Lane &L) { init_phase(C, L, wave); }
    // DEC, DIRECT: this body reads C.direct_bits / C.ballots at run time instead
    template <bool DEC, bool DIRECT>
    __device__ __forceinline__ void check(const Ctx &C, const Lane &L, int &errs) { check_phase<ALGO>(C, L, wave, errs); }
    template <bool DEC, bool WRITE, bool DIRECT>
    __device__ __forceinline__ void var(const Ctx &C, const Lane &L, int &errs) {
        var_phase(C, L, wave, WRITE, errs);
    }
    __device__ __forceinline__ int parity(const Ctx &C, const Lane &L) { return parity_phase(C, L, wave); }
};

__device__ __forceinline__ void init_ctx(Ctx &C, const FloodTables &T, char *lds, float alpha, int out_dtype,
                                         void *bits) {
    C.T = T;
    C.lds = lds;
    C.flag = reinterpret_cast<uint32_t *>(lds + (size_t)T.nslots * 256);
    C.words = reinterpret_cast<uint64_t *>(lds + (size_t)T.nslots * 256 + 8);
    C.alpha = alpha;
    C.out_dtype = out_dtype;
    C.bits = bits;
    C.direct_bits = false;
    C.ballots = false;
    C.redo = nullptr;
}

}  // namespace

template <int ALGO, int ES>
__global__ __launch_bounds__(512) void flood_kernel(FloodTables T, const float *__restrict__ llr, int64_t B,
                                                    int max_iter, float alpha, int out_dtype,
                                                    void *__restrict__ bits, Outs O, EsWs W) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const Lane L = make_lane(T, llr, B);
    Ctx C;
    init_ctx(C, T, lds, alpha, out_dtype, bits);
    GenericBody<ALGO> body{__builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6)};
    flood_drive<ES>(body, C, L, B, max_iter, O, W);
}

}  // namespace ldpc
