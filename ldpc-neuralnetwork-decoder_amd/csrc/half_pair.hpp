// half_pair.hpp -- the packed-binary16 pair vocabulary of the half-precision decoders: flood_half.hip
// (flooding, LDS-resident) and flood_layered_stream_half.hip (layered, streaming).  A dword holds the binary16
// values of two frames; every operation here is a packed (per-half) f16 operation or a bitwise one, so the two
// halves never meet.
//
// The one value the two decoders do not share is the empty or initial minimum of the check rule, a parameter
// of everything below that needs one.  Their contracts in include/ldpc_amd.h differ there on purpose:
//     flooding ("Half-precision min-sum"):         +infinity (kInf2): a degree-1 check sends a * inf
//     layered  ("Half-precision layered min-sum"): C = 1024 (HConst::cpos): min(C, .), a degree-1 check sends a * C
#pragma once
#include <cstdint>

#include "flood_dev.hpp"

namespace ldpc {

typedef _Float16 h2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ h2 as_h(uint32_t u) { return __builtin_bit_cast(h2, u); }
__device__ __forceinline__ uint32_t as_u(h2 h) { return __builtin_bit_cast(uint32_t, h); }
// IEEE minimum / maximum: one v_pk_minimum3_f16 / v_pk_maximum3_f16, no canonicalising v_pk_max
__device__ __forceinline__ h2 hmin(h2 a, h2 b) { return __builtin_elementwise_minimum(a, b); }
__device__ __forceinline__ h2 hmax(h2 a, h2 b) { return __builtin_elementwise_maximum(a, b); }

constexpr uint32_t kSign2 = 0x80008000u, kAbs2 = 0x7fff7fffu, kInf2 = 0x7c007c00u;
constexpr uint32_t kClampPos2 = 0x64006400u, kClampNeg2 = 0xe400e400u;  // +-C = +-1024

// uniform constants in VGPRs (a VALU op with an SGPR source issues at half rate); a2: half(alpha) in both halves
struct HConst {
    uint32_t a2, cpos, cneg, sign, absm;
};
__device__ __forceinline__ HConst make_const(uint32_t a2) {
    return HConst{opaque_vu(a2), opaque_vu(kClampPos2), opaque_vu(kClampNeg2), opaque_vu(kSign2), opaque_vu(kAbs2)};
}
__device__ __forceinline__ h2 hclamp(const HConst &K, h2 v) { return hmin(hmax(v, as_h(K.cneg)), as_h(K.cpos)); }

// out = sign | magnitude: prod >= +0 (a >= 0, min >= 0), so its sign bits are free for the parity
__device__ __forceinline__ uint32_t signed_c2v(const HConst &K, uint32_t par, uint32_t v, h2 excl_min) {
    const uint32_t prod = as_u(as_h(K.a2) * excl_min);  // rounded once
    return ((par ^ v) & K.sign) | prod;
}

// The two-pass form of the exclusive minimum, for rows too long for prefix / suffix registers: a first pass
// keeps the row's two smallest magnitudes (m1 <= m2, both starting at the empty minimum), a second chooses per
// half (the excluded minimum is m2 exactly when |v| == m1: a tie at m1 puts m1 in m2 as well).
__device__ __forceinline__ void half_two_min_step(h2 &m1, h2 &m2, h2 a) {
    m2 = hmin(m2, hmax(m1, a));
    m1 = hmin(m1, a);
}
__device__ __forceinline__ h2 half_excl_select(h2 a, h2 m1, h2 m2) {
    h2 m;
    m.x = a.x == m1.x ? m2.x : m1.x;
    m.y = a.y == m1.y ? m2.y : m1.y;
    return m;
}

// The check rule on a row of packed halves held in registers: out_k = (prod_{q != k} sgn v_q) *
// (a * min(empty_min, min_{q != k} |v_q|)), where empty_min (see the head of this file) is no smaller than any
// |v_q|: it changes nothing for DC >= 2 and is what a degree-1 check scales.  sgn(0) = 0 needs no code: if
// another message of the row is zero the exclusive minimum is 0 and the result is a zero whatever its sign, and
// if only v_k itself is zero its sign bit cancels in the XOR.
template <int DC>
__device__ __forceinline__ void half_check_rule(const HConst &K, const uint32_t (&v)[DC], uint32_t (&out)[DC],
                                                h2 empty_min) {
    uint32_t par = v[0];
#pragma unroll
    for (int e = 1; e < DC; ++e) par ^= v[e];
    if constexpr (DC == 1) {
        out[0] = signed_c2v(K, par, v[0], empty_min);
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
        h2 m1 = empty_min, m2 = empty_min;
#pragma unroll
        for (int e = 0; e < DC; ++e) half_two_min_step(m1, m2, as_h(v[e] & K.absm));
#pragma unroll
        for (int e = 0; e < DC; ++e) out[e] = signed_c2v(K, par, v[e], half_excl_select(as_h(v[e] & K.absm), m1, m2));
    }
}

// binary16 bits of half(alpha), round-to-nearest-even
inline uint32_t half_alpha_bits(float alpha) {
    const _Float16 a = (_Float16)alpha;
    uint16_t u;
    __builtin_memcpy(&u, &a, sizeof u);
    return u;
}

}  // namespace ldpc
