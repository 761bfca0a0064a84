// Stand-alone run of the GNN plan's host table builder (csrc/gnn_plan_tables.cpp) for sanitizers: it
// needs no GPU, no HIP and no Python.  Not run by pytest.
//
//   python3 tools/gnn_plan_cases.py /tmp/gnn_plan_cases.bin        # the inputs of tests/test_gnn_plan_host.py
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/gnn_plan_tables_check
//       tools/gnn_plan_tables_check.cpp ldpc-neuralnetwork-decoder_amd/csrc/gnn_plan_tables.cpp       (one line)
//   /tmp/gnn_plan_tables_check /tmp/gnn_plan_cases.bin
//
// The file is a sequence of int32 records: {0, E, n_vgroups, n_cgroups, vgroup[E], cgroup[E]} or
// {1, E, nnz_v, nnz_c, v_ptr[E+1], v_col, v_val (float bits), c_ptr[E+1], c_col, c_val}.  Every case
// is built and serialised into a heap buffer of exactly the size asked for, then once more with one
// label out of range (the builder must refuse it).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../ldpc-neuralnetwork-decoder_amd/csrc/gnn_plan_tables.hpp"

using namespace ldpc;

int main(int argc, char **argv) {
    if (argc != 2) return std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]), 2;
    std::ifstream f(argv[1], std::ios::binary);
    const std::vector<char> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<int32_t> in(bytes.size() / 4);
    std::memcpy(in.data(), bytes.data(), in.size() * 4);
    int cases = 0;
    int64_t total = 0;
    for (size_t i = 0; i + 4 <= in.size(); ++cases) {
        const int32_t kind = in[i], E = in[i + 1], a = in[i + 2], b = in[i + 3];
        const int32_t *d = in.data() + i + 4;
        int64_t need = 0;
        std::vector<int32_t> out;
        if (kind == 0) {
            std::vector<int32_t> vg(d, d + E), cg(d + E, d + 2 * E);  // exact-size copies: an overread is caught
            GnnPlanTables t;
            if (const char *msg = gnn_plan_tables(E, a, vg.data(), b, cg.data(), t)) return std::printf("case %d: %s\n", cases, msg), 1;
            need = gnn_plan_tables_words(t, nullptr, 0);
            out.resize(need);
            if (gnn_plan_tables_words(t, out.data(), need) != need) return 1;
            vg[E / 2] = a;
            if (!gnn_plan_tables(E, a, vg.data(), b, cg.data(), t)) return std::printf("case %d: bad label accepted\n", cases), 1;
            i += 4 + 2 * (size_t)E;
        } else {
            const float *fl = reinterpret_cast<const float *>(d);
            std::vector<int32_t> vp(d, d + E + 1), vc(d + E + 1, d + E + 1 + a);
            std::vector<float> vv(fl + E + 1 + a, fl + E + 1 + 2 * a);
            const size_t o = E + 1 + 2 * (size_t)a;
            std::vector<int32_t> cp(d + o, d + o + E + 1), cc(d + o + E + 1, d + o + E + 1 + b);
            std::vector<float> cv(fl + o + E + 1 + b, fl + o + E + 1 + 2 * b);
            GnnCsrTables t;
            if (const char *msg = gnn_csr_tables(E, vp.data(), vc.data(), vv.data(), cp.data(), cc.data(), cv.data(), t))
                return std::printf("case %d: %s\n", cases, msg), 1;
            need = gnn_csr_tables_words(t, nullptr, 0);
            out.resize(need);
            if (gnn_csr_tables_words(t, out.data(), need) != need) return 1;
            if (a) {
                vc[0] = E;
                if (!gnn_csr_tables(E, vp.data(), vc.data(), vv.data(), cp.data(), cc.data(), cv.data(), t))
                    return std::printf("case %d: bad column accepted\n", cases), 1;
            }
            i += 4 + 2 * ((size_t)E + 1) + 2 * (size_t)a + 2 * (size_t)b;
        }
        total += need;
    }
    std::printf("%d cases, %lld words: ok\n", cases, (long long)total);
    return 0;
}
