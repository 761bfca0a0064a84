// Stand-alone run of the streaming layered decoder's run builder (csrc/layered_runs.cpp) for sanitizers:
// it needs no GPU, no HIP and no Python.  Not run by pytest.
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/layered_runs_check
//       tools/layered_runs_check.cpp ldpc-neuralnetwork-decoder_amd/csrc/layered_runs.cpp       (one line)
//   /tmp/layered_runs_check codes/NR_2_0_32.txt
//
// Cases: BG2 (the base file given) lifted to Z = 12; a graph whose last check has no edge; an empty
// graph.  Every case is built from heap copies of exactly the edge list's size, serialised into a heap
// buffer of exactly the size asked for (and refused one word short), checked against the properties
// the tables promise, and built once more with one edge out of range (the builder must refuse it).
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "../ldpc-neuralnetwork-decoder_amd/csrc/layered_runs.hpp"

using namespace ldpc;

static int check(const char *name, int M, int N, const std::vector<int32_t> &ec, const std::vector<int32_t> &ev,
                 int want_runs) {
    const int64_t E = (int64_t)ec.size();
    LayeredRuns t;
    if (const char *msg = layered_runs(M, N, E, ec.data(), ev.data(), t)) return std::printf("%s: %s\n", name, msg), 1;
    const int64_t need = layered_runs_words(t, nullptr, 0);
    std::vector<int32_t> out((size_t)need), small((size_t)need - 1, -7);
    if (layered_runs_words(t, out.data(), need) != need) return std::printf("%s: size changed\n", name), 1;
    if (layered_runs_words(t, small.data(), need - 1) != need || std::count(small.begin(), small.end(), -7) != need - 1)
        return std::printf("%s: a short buffer was written\n", name), 1;
    if (out[0] != t.n_runs() || out[1] != t.n_seg() || need != 2 + (t.n_runs() + 1) + 4 * (int64_t)t.n_seg() + M)
        return std::printf("%s: bad header\n", name), 1;
    if (want_runs >= 0 && t.n_runs() != want_runs) return std::printf("%s: %d runs, not %d\n", name, t.n_runs(), want_runs), 1;
    // checks of a run are variable-disjoint, and the next run's first check meets the run before it
    std::vector<std::vector<int32_t>> vars((size_t)M);
    for (int64_t e = 0; e < E; ++e) vars[ec[e]].push_back(ev[e]);
    std::set<int32_t> prev;
    for (int r = 0; r < t.n_runs(); ++r) {
        std::set<int32_t> cur;
        for (int i = t.run_ptr[r]; i < t.run_ptr[r + 1]; ++i)
            for (int32_t v : vars[i])
                if (!cur.insert(v).second) return std::printf("%s: run %d holds variable %d twice\n", name, r, v), 1;
        if (r) {
            bool meets = false;
            for (int32_t v : vars[t.run_ptr[r]]) meets |= prev.count(v) != 0;
            if (!meets) return std::printf("%s: run %d could have joined run %d\n", name, r, r - 1), 1;
        }
        prev.swap(cur);
    }
    // the segments tile order, by exact degree
    int64_t off = 0;
    std::vector<int> hit((size_t)M, 0);
    for (int q = 0; q < t.n_seg(); ++q) {
        const int32_t *s = &t.seg[4 * (size_t)q];
        if (s[2] != off) return std::printf("%s: segment %d does not follow its predecessor\n", name, q), 1;
        for (int k = 0; k < s[3]; ++k) {
            const int32_t i = t.order[(size_t)(off + k)];
            if (i < t.run_ptr[s[0]] || i >= t.run_ptr[s[0] + 1] || (int)vars[i].size() != s[1])
                return std::printf("%s: segment %d holds check %d\n", name, q, i), 1;
            ++hit[i];
        }
        off += s[3];
    }
    if (off != M || std::count(hit.begin(), hit.end(), 1) != M) return std::printf("%s: order is no permutation\n", name), 1;
    if (E > 0) {
        std::vector<int32_t> bad(ev);
        bad[(size_t)E / 2] = N;
        if (!layered_runs(M, N, E, ec.data(), bad.data(), t)) return std::printf("%s: bad edge accepted\n", name), 1;
    }
    std::printf("%s: M %d, E %lld, %d runs, %d segments, %lld words\n", name, M, (long long)E, t.n_runs(), t.n_seg(),
                (long long)need);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) return std::fprintf(stderr, "usage: %s codes/NR_2_0_32.txt\n", argv[0]), 2;
    std::ifstream f(argv[1]);
    std::vector<std::vector<int>> base;
    for (std::string line; std::getline(f, line);) {
        std::istringstream ss(line);
        std::vector<int> row;
        for (double x; ss >> x;) row.push_back((int)x);
        if (!row.empty()) base.push_back(row);
    }
    if (base.empty()) return std::fprintf(stderr, "%s: no base matrix\n", argv[1]), 2;
    const int Z = 12, mb = (int)base.size(), nb = (int)base[0].size();
    std::vector<int32_t> ec, ev;
    for (int r = 0; r < mb; ++r)
        for (int k = 0; k < Z; ++k)
            for (int c = 0; c < nb; ++c) {
                if (base[r][c] < 0) continue;
                ec.push_back(r * Z + k);
                ev.push_back(c * Z + (k + base[r][c] % Z) % Z);
            }
    int rc = check("BG2 at Z = 12", mb * Z, nb * Z, ec, ev, 28);
    // checks 0 and 1 share variable 1; check 2, the last, has no edge and joins the second run
    rc |= check("last check of degree 0", 3, 4, {0, 0, 1, 1}, {0, 1, 1, 2}, 2);
    rc |= check("empty graph", 0, 1, {}, {}, 0);
    std::printf(rc ? "FAILED\n" : "ok\n");
    return rc;
}
