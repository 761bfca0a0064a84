// layered_runs.cpp -- builds the streaming layered decoder's runs and per-degree segments
// (layered_runs.hpp) on the host: plain C++, no HIP include.  O(E + M log M).
#include "layered_runs.hpp"

#include <algorithm>

namespace ldpc {

const char *layered_runs(int M, int N, int64_t E, const int32_t *edge_chk, const int32_t *edge_var, LayeredRuns &t) {
    if (M < 0 || N <= 0 || E < 0 || (E > 0 && (!edge_chk || !edge_var))) return "bad graph dimensions";
    for (int64_t e = 0; e < E; ++e) {
        if (edge_chk[e] < 0 || edge_chk[e] >= M || edge_var[e] < 0 || edge_var[e] >= N) return "edge index out of range";
        if (e && (edge_chk[e] < edge_chk[e - 1] || (edge_chk[e] == edge_chk[e - 1] && edge_var[e] <= edge_var[e - 1])))
            return "edge list must be check-major, strictly ascending, no duplicates";
    }
    t.run_ptr.assign(1, 0);
    t.seg.clear();
    t.order.assign((size_t)M, 0);
    if (M == 0) return nullptr;

    std::vector<int32_t> deg((size_t)M, 0);
    std::vector<int32_t> seen((size_t)N, -1);  // the last run that holds the variable
    int run = 0;
    int64_t e = 0;
    for (int i = 0; i < M; ++i) {
        const int64_t e0 = e;
        bool clash = false;
        for (; e < E && edge_chk[e] == i; ++e) clash |= seen[edge_var[e]] == run;
        deg[i] = (int32_t)(e - e0);
        if (clash) {  // check i opens the next run
            t.run_ptr.push_back(i);
            ++run;
        }
        for (int64_t q = e0; q < e; ++q) seen[edge_var[q]] = run;
    }
    t.run_ptr.push_back(M);

    for (int r = 0; r <= run; ++r) {
        const int i0 = t.run_ptr[r], i1 = t.run_ptr[r + 1];
        int32_t *o = t.order.data() + i0;
        for (int i = i0; i < i1; ++i) o[i - i0] = i;
        std::stable_sort(o, o + (i1 - i0), [&](int32_t a, int32_t b) { return deg[a] < deg[b]; });
        for (int k = i0; k < i1; ++k) {
            const int32_t d = deg[t.order[k]];
            if (k == i0 || t.seg[t.seg.size() - 3] != d) t.seg.insert(t.seg.end(), {r, d, k, 0});
            ++t.seg.back();
        }
    }
    return nullptr;
}

int64_t layered_runs_words(const LayeredRuns &t, int32_t *out, int64_t cap) {
    const int64_t need = 2 + (int64_t)t.run_ptr.size() + (int64_t)t.seg.size() + (int64_t)t.order.size();
    if (!out || cap < need) return need;
    *out++ = t.n_runs();
    *out++ = t.n_seg();
    out = std::copy(t.run_ptr.begin(), t.run_ptr.end(), out);
    out = std::copy(t.seg.begin(), t.seg.end(), out);
    std::copy(t.order.begin(), t.order.end(), out);
    return need;
}

}  // namespace ldpc
