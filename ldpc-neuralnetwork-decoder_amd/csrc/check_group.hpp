// check_group.hpp -- CheckLayer's rule on one check of a frame row held in LDS, shared by the layer
// kernels (layers.hip) and the fused neural min-sum kernel (neural_ms.hip) so that the two cannot
// drift apart.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace ldpc {

// CheckLayer when its index is a set of checks (every edge's row = the other edges of its check,
// as create_LLR_mapping builds it; detected once in Python): per (check, frame) one pass collects
// the sign-zero / NaN counts, the parity of negative signs and the two smallest |v|' (|0| -> 1e10),
// a second pass writes each edge's output, in place over its staged input.  Every output equals
// gather_lds_kernel's: the sign product is exact (its value and the sign of a zero product follow
// from the counts and the parity), the min of the others is min1, or min2 for the edge holding
// min1, NaN if another edge is NaN, capped at 1e10 when the row has padding (K > degree - 1).
// O(degree) per check instead of O(degree^2).
// One check of a staged frame row r, members gmem[p0 .. p1): the two passes above, in place.  The
// member indices come from global memory (int32) or from LDS (uint16).
template <typename Idx>
__device__ __forceinline__ void check_group_minsum(float *r, const Idx *gmem, int p0, int p1, int K) {
    int zeros = 0, nans = 0, neg = 0, pos = -1;
    float m1 = INFINITY, m2 = INFINITY;
    for (int p = p0; p < p1; ++p) {
        const float v = r[gmem[p]];
        const float sv = v + 1e-10f;
        zeros += sv == 0.0f;
        nans += sv != sv;
        neg ^= sv < 0.0f;
        float a = fabsf(v);
        if (a == 0.0f) a = 1e10f;
        if (a < m1) { m2 = m1; m1 = a; pos = p; }
        else if (a < m2) m2 = a;
    }
    const bool pad = K > p1 - p0 - 1;
    for (int p = p0; p < p1; ++p) {
        const int j = gmem[p];
        const float v = r[j];
        const float sv = v + 1e-10f;
        const int z = zeros - (sv == 0.0f), nn = nans - (sv != sv), ng = neg ^ (sv < 0.0f);
        float m = p == pos ? m2 : m1;
        if (pad) m = fminf(m, 1e10f);
        const float sp = z > 0 ? (ng ? -0.0f : 0.0f) : (ng ? -1.0f : 1.0f);
        r[j] = nn > 0 ? __builtin_nanf("") : sp * m;
    }
}

}  // namespace ldpc
