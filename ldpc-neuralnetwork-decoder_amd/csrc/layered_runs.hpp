// layered_runs.hpp -- the layers of the streaming layered decoder (flood_layered_stream.hip) as host
// vectors.  layered_runs.cpp fills them with no HIP call (so tests and a sanitizer build reach them
// without a device); graph.cpp uploads `order` beside the CSR tables and keeps the segments for the
// launch loop.
//
// A run is a maximal stretch of consecutive checks, in ascending index, whose variable sets are
// pairwise disjoint: check i joins the current run unless one of its variables is already in it, and
// then opens the next.  The checks of a run touch disjoint posteriors and messages, so updating them
// in one launch equals the serial (check by check) definition bit for bit.  Inside a run the checks
// are grouped by exact degree, one segment = one launch of the kernel compiled for that degree; a
// check without edges sits in a degree-0 segment that launches nothing.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ldpc {

struct LayeredRuns {
    std::vector<int32_t> run_ptr;  // [n_runs + 1] check indices: run r = checks run_ptr[r] .. run_ptr[r + 1] - 1
    std::vector<int32_t> seg;      // [n_seg][4] {run, degree, offset into order, count}: runs ascending, degrees
                                   // ascending inside a run; the segments tile order
    std::vector<int32_t> order;    // [M] check indices, ascending inside a segment
    int n_runs() const { return (int)run_ptr.size() - 1; }
    int n_seg() const { return (int)(seg.size() / 4); }
};

// The runs of a check-major edge list (the arguments of ldpc_graph_create).  Returns null, or the
// message of the argument error (LDPC_EINVAL) that ldpc_graph_create gives for the same input.
const char *layered_runs(int M, int N, int64_t E, const int32_t *edge_chk, const int32_t *edge_var, LayeredRuns &t);

// The tables as 32-bit words (ldpc_amd.h, ldpc_layered_runs): n_runs, n_seg, run_ptr, seg, order.
// Returns the words needed; out is filled when cap holds them.
int64_t layered_runs_words(const LayeredRuns &t, int32_t *out, int64_t cap);

}  // namespace ldpc
