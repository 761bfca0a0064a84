// neural_layout.cpp -- see neural_layout.hpp.  Plain C++, no HIP include.
#include "neural_layout.hpp"

#include <algorithm>

namespace ldpc {

namespace {
inline int pad_to(int n, int m) { return (n + m - 1) / m * m; }
}  // namespace

const char *neural_validate(int N, int G, int64_t E, const int32_t *cptr, const int32_t *cmem, const int32_t *vptr,
                            int K) {
    if (N <= 0 || G <= 0 || E <= 0 || K <= 0) return "bad neural-plan dimensions";
    if (E >= 65536) return "neural plan: E must be below 65536 (16-bit index tables)";
    if (!cptr || !cmem || !vptr) return "neural plan: NULL table";
    if (cptr[0] != 0 || cptr[G] != E) return "neural plan: cptr does not tile [0, E)";
    for (int g = 0; g < G; ++g)
        if (cptr[g + 1] < cptr[g]) return "neural plan: cptr is not monotone";
    if (vptr[0] != 0 || vptr[N] != E) return "neural plan: vptr does not tile [0, E)";
    for (int j = 0; j < N; ++j)
        if (vptr[j + 1] < vptr[j]) return "neural plan: vptr is not monotone";
    std::vector<uint8_t> seen((size_t)E, 0);
    for (int64_t p = 0; p < E; ++p) {
        const int32_t e = cmem[p];
        if (e < 0 || e >= E || seen[(size_t)e]) return "neural plan: cmem is not a permutation of 0 .. E - 1";
        seen[(size_t)e] = 1;
    }
    return nullptr;
}

void neural_table_layout(int N, int G, int E, int K, NeuralLayout &L) {
    L.N = N; L.G = G; L.E = E; L.K = K;
    L.small = N < 65536 && G < 65536;
    if (!L.small) return;  // neural_layout refuses it; nothing below may overflow
    L.Np = pad_to(N, 4);
    L.Ep = pad_to(E, 4);
    L.o_cptr = pad_to(E, 8);
    L.o_evar = L.o_cptr + pad_to(G + 1, 8);
    L.o_vptr = L.o_evar + pad_to(E, 8);
    L.table_words = L.o_vptr + pad_to(N + 1, 8);
}

const char *neural_layout(int depth_L, NeuralLayout &L) {
    if (depth_L > kNeuralMaxDepth) return "neural min-sum: depth_L > 8";
    if (!L.small) return "neural min-sum: more than 65535 variables or checks";
    L.ring = std::max(depth_L, 1);
    const size_t tables = (size_t)L.table_words * 2;
    const size_t frame = ((size_t)L.Np + (size_t)(1 + L.ring) * L.Ep) * 4;
    if (tables + frame > kNeuralLdsMax) return "neural min-sum: one frame's messages do not fit LDS";
    L.frame_floats = (int)(frame / 4);
    L.frames = (int)std::min<size_t>((kNeuralLdsMax - tables) / frame, (size_t)kNeuralMaxFrames);
    L.lds_bytes = tables + (size_t)L.frames * frame;
    const int64_t items = (int64_t)L.frames * L.E;
    L.threads = (int)std::min<int64_t>(kNeuralMaxThreads, (items + 63) / 64 * 64);
    return nullptr;
}

std::vector<uint16_t> neural_tables(const NeuralLayout &L, const int32_t *cptr, const int32_t *cmem,
                                    const int32_t *vptr) {
    std::vector<uint16_t> t((size_t)L.table_words, 0);
    // checks by descending degree (the rule does not depend on their order): a wave walks its checks
    // in lockstep, so it takes its longest check's time -- equal degrees share a wave, and the long
    // checks come first, where no thread has a second one
    std::vector<int32_t> order((size_t)L.G);
    for (int g = 0; g < L.G; ++g) order[(size_t)g] = g;
    std::stable_sort(order.begin(), order.end(),
                     [&](int32_t a, int32_t b) { return cptr[a + 1] - cptr[a] > cptr[b + 1] - cptr[b]; });
    int p = 0;
    for (int g = 0; g < L.G; ++g) {
        t[(size_t)L.o_cptr + g] = (uint16_t)p;
        for (int q = cptr[order[(size_t)g]]; q < cptr[order[(size_t)g] + 1]; ++q) t[(size_t)p++] = (uint16_t)cmem[q];
    }
    t[(size_t)L.o_cptr + L.G] = (uint16_t)p;
    for (int j = 0; j < L.N; ++j)
        for (int e = vptr[j]; e < vptr[j + 1]; ++e) t[(size_t)L.o_evar + e] = (uint16_t)j;
    for (int j = 0; j <= L.N; ++j) t[(size_t)L.o_vptr + j] = (uint16_t)vptr[j];
    return t;
}

}  // namespace ldpc
