// neural_layout.hpp -- host side of the fused neural min-sum kernel (neural_ms.hip): validation of the
// graph description, the 16-bit index tables the kernel stages in LDS, and the workgroup's shape.
// Plain C++, no HIP include: ldpc_neural_layout answers without touching a device, and the plan and
// the launch use the same functions, so the three cannot disagree.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ldpc {

constexpr size_t kNeuralLdsMax = 160 * 1024;  // one CU's LDS
constexpr int kNeuralMaxDepth = 8;            // ResidualLayer's bound on depth_L
constexpr int kNeuralMaxFrames = 8;           // frames per workgroup (see neural_layout)
constexpr int kNeuralMaxThreads = 1024;

// Offsets of the kernel's LDS image.  Floats first, per frame [llr Np | c Ep | ring R x Ep], then the
// 16-bit tables [cmem | cptr | evar | vptr], each padded to 8 words; the plan's device blob has the
// tables in the same order and padding, so staging is one copy.
struct NeuralLayout {
    int N = 0, G = 0, E = 0, K = 0;
    bool small = false;      // N and G below 65536 (else no layout: LDPC_EUNSUPPORTED)
    int Np = 0, Ep = 0;      // row lengths padded to 4 floats
    int ring = 1;            // max(depth_L, 1) rows of v per frame
    int frame_floats = 0;    // Np + (1 + ring) * Ep
    int o_cptr = 0, o_evar = 0, o_vptr = 0, table_words = 0;  // 16-bit word offsets inside the tables
    int frames = 0, threads = 0;
    size_t lds_bytes = 0;
};

// Validates (N, G, E, cptr, cmem, vptr, K): cptr (G + 1) and vptr (N + 1) monotone from 0 to E, cmem a
// permutation of 0 .. E - 1, E < 65536.  Returns nullptr or the message (LDPC_EINVAL).
const char *neural_validate(int N, int G, int64_t E, const int32_t *cptr, const int32_t *cmem, const int32_t *vptr,
                            int K);

// The table part of the layout (no depth_L needed) for a validated description.
void neural_table_layout(int N, int G, int E, int K, NeuralLayout &L);

// Completes L for depth_L: frames = as many as fit 160 KB beside the tables, at most kNeuralMaxFrames;
// threads = one per (frame, edge), a multiple of 64 up to kNeuralMaxThreads.  Returns nullptr, or the
// message when depth_L > 8 or one frame does not fit (LDPC_EUNSUPPORTED).
const char *neural_layout(int depth_L, NeuralLayout &L);

// The tables as the kernel reads them (L.table_words 16-bit words; padding is zero).  The checks are
// listed by descending degree, not in the caller's order: the check rule does not depend on it.
std::vector<uint16_t> neural_tables(const NeuralLayout &L, const int32_t *cptr, const int32_t *cmem,
                                    const int32_t *vptr);

}  // namespace ldpc
