// gnn_plan_tables.cpp -- builds the message-GNN plan's tables (gnn.hpp) on the host: plain C++, no
// HIP header and no HIP call, one function per table family.
#include "gnn_plan_tables.hpp"

#include <algorithm>
#include <cstring>
#include <initializer_list>

namespace ldpc {
namespace {

using Ints = std::vector<int32_t>;

int degree(const Ints &ptr, int g) { return ptr[g + 1] - ptr[g]; }

// the var-group degree of message m
int var_degree(const GnnPlanTables &t, int64_t m) { return degree(t.vg_ptr, t.vgroup[m]); }

// One side's group CSR, members in ascending message order; false: a label out of range
bool group_csr(const Ints &group, int ngroups, Ints &ptr, Ints &mem) {
    ptr.assign(ngroups + 1, 0);
    mem.resize(group.size());
    for (int32_t g : group) {
        if (g < 0 || g >= ngroups) return false;
        ptr[g + 1]++;
    }
    for (int g = 0; g < ngroups; ++g) ptr[g + 1] += ptr[g];
    Ints fill(ptr.begin(), ptr.end() - 1);
    for (size_t m = 0; m < group.size(); ++m) mem[fill[group[m]]++] = (int32_t)m;
    return true;
}

// 1 / |group|, 0 for a group with no messages
void append_inverse_sizes(const Ints &ptr, std::vector<float> &inv) {
    for (size_t g = 0; g + 1 < ptr.size(); ++g) {
        const int d = degree(ptr, (int)g);
        inv.push_back(d ? 1.0f / (float)d : 0.0f);
    }
}

// The groups of one side that have messages (an empty group is never read), ascending in degree
Ints degree_order(const Ints &ptr) {
    Ints order;
    for (int g = 0; g + 1 < (int)ptr.size(); ++g)
        if (degree(ptr, g) > 0) order.push_back(g);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return degree(ptr, a) < degree(ptr, b); });
    return order;
}

// bf16 path: one side's group tiles of 8 groups of one degree
void add_group_tiles(GnnPlanTables &t, const Ints &ptr, const Ints &mem, int gbase) {
    const Ints order = degree_order(ptr);
    for (size_t i = 0; i < order.size();) {
        const int d = degree(ptr, order[i]);
        size_t n = 0;
        while (n < 8 && i + n < order.size() && degree(ptr, order[i + n]) == d) ++n;
        t.gt_meta.push_back(d);
        t.gt_meta.push_back((int32_t)t.gt_mem.size());
        for (int k = 0; k < d; ++k)
            for (size_t q = 0; q < 8; ++q) t.gt_mem.push_back(mem[ptr[order[i + (q < n ? q : 0)]] + k]);
        for (size_t q = 0; q < 8; ++q) t.gt_grp.push_back(q < n ? gbase + order[i + q] : -1);
        i += n;
    }
}

void build_group_tiles(GnnPlanTables &t) {
    add_group_tiles(t, t.vg_ptr, t.vg_mem, 0);
    t.n_gtiles_v = t.n_gtiles();
    // the var tiles are sorted by degree: the degree-1 ones lead
    while (t.n_gtiles_v1 < t.n_gtiles_v && t.gt_meta[2 * t.n_gtiles_v1] == 1) ++t.n_gtiles_v1;
    add_group_tiles(t, t.cg_ptr, t.cg_mem, t.Gv);
}

// bf16 MLP tiles (ct_m0): whole check groups when each is a contiguous message run of at most 32
// (greedy, in message order), else plain 32-message tiles
void build_check_tiles(GnnPlanTables &t) {
    t.ct_aligned = true;
    for (int g = 0; g < t.Gc && t.ct_aligned; ++g) {
        const int d = degree(t.cg_ptr, g);
        t.ct_aligned = d <= 32 && (d == 0 || t.cg_mem[t.cg_ptr[g + 1] - 1] - t.cg_mem[t.cg_ptr[g]] == d - 1);
    }
    t.ct_m0.assign(1, 0);
    if (t.ct_aligned) {
        for (int64_t m = 0; m < t.E;) {
            const int d = degree(t.cg_ptr, t.cgroup[m]);  // the group's run starts at m (contiguous, ascending)
            if (m + d - t.ct_m0.back() > 32) t.ct_m0.push_back((int32_t)m);
            m += d;
        }
    } else {
        for (int64_t m = 32; m < t.E; m += 32) t.ct_m0.push_back((int32_t)m);
    }
    t.ct_m0.push_back((int32_t)t.E);
}

// fp32 row walk (rw_meta): units of up to 32 consecutive check groups of one degree, kept when the
// plan is aligned, lane k of every unit holds check group first + k and the units fill >= 90 % of
// their 32 d slots
void build_row_walk(GnnPlanTables &t) {
    if (!t.ct_aligned) return;
    int64_t slots = 0, d1_msgs = 0, d1_in_tiles = 0;
    bool contig = true;
    for (int64_t m = 0; m < t.E; ++m) d1_msgs += var_degree(t, m) == 1;
    for (int64_t m = 0; m < t.E;) {
        const int d = degree(t.cg_ptr, t.cgroup[m]);
        const int64_t m0 = m;
        const int first = t.cgroup[m];
        int n = 0;
        for (; n < 32 && m < t.E && degree(t.cg_ptr, t.cgroup[m]) == d; ++n, m += d)
            contig = contig && t.cgroup[m] == first + n;
        int32_t mask = 0;  // bit i: message i of every check of the unit is its var group's only one
        for (int i = 0; i < d; ++i) {
            bool all = true;
            for (int k = 0; k < n && all; ++k) all = var_degree(t, m0 + (int64_t)k * d + i) == 1;
            if (!all) continue;
            mask |= (int32_t)(1u << i);
            d1_in_tiles += n;
        }
        t.rw_meta.insert(t.rw_meta.end(), {(int32_t)m0, n, d, mask, first, 0, 0, 0});
        slots += 32LL * d;
    }
    const bool d1 = d1_in_tiles == d1_msgs;  // every degree-1 message lies in a masked position
    if (!d1)
        for (size_t c = 0; c < t.rw_meta.size(); c += 8) t.rw_meta[c + 3] = 0;
    if ((double)t.E < 0.9 * (double)slots || !contig) t.rw_meta.clear();
    t.rw_d1 = d1 && t.n_rw() > 0;
}

// fp32 path: one side's projection tiles of 32 groups
void add_proj_tiles(GnnPlanTables &t, const Ints &ptr, const Ints &mem, int side) {
    const Ints order = degree_order(ptr);
    for (size_t i = 0; i < order.size(); i += 32) {
        const size_t n = std::min<size_t>(32, order.size() - i);
        const int dmax = degree(ptr, order[i + n - 1]);  // ascending degrees: the last group's
        t.pt_meta.insert(t.pt_meta.end(), {side, dmax, (int32_t)t.pt_mem.size(), 0});
        for (int k = 0; k <= dmax; ++k)  // one padding row: the kernel reads members in pairs
            for (size_t q = 0; q < 32; ++q) {
                const int g = q < n ? order[i + q] : -1;
                t.pt_mem.push_back(g >= 0 && k < degree(ptr, g) ? mem[ptr[g] + k] : 0);
            }
        for (size_t q = 0; q < 32; ++q) {
            t.pt_grp.push_back(q < n ? order[i + q] : -1);
            t.pt_deg.push_back(q < n ? degree(ptr, order[i + q]) : 0);
        }
    }
}

void build_proj_tiles(GnnPlanTables &t) {
    add_proj_tiles(t, t.vg_ptr, t.vg_mem, 0);
    t.n_ptiles_v = t.n_ptiles();
    // leading var tiles of degree-1 groups only (padding has degree 0)
    while (t.n_ptiles_v1 < t.n_ptiles_v &&
           std::all_of(t.pt_deg.begin() + 32 * t.n_ptiles_v1, t.pt_deg.begin() + 32 * (t.n_ptiles_v1 + 1),
                       [](int32_t d) { return d <= 1; }))
        ++t.n_ptiles_v1;
    add_proj_tiles(t, t.cg_ptr, t.cg_mem, 1);
}

// bf16 projected MLP: degree-1 var groups' messages first, each part padded to whole tiles
void build_message_perm(GnnPlanTables &t) {
    for (int pass = 0; pass < 2; ++pass) {
        for (int64_t m = 0; m < t.E; ++m)
            if ((var_degree(t, m) == 1) == (pass == 0)) t.mt_perm.push_back((int32_t)m);
        while (t.mt_perm.size() % 32) t.mt_perm.push_back(-1);
        if (pass == 0) t.n_mtiles_v1 = t.n_mtiles();
    }
}

// A's transpose appended to tt (ptr[E+1] mem[nnz]) and tw (w[nnz]): a counting sort of the nonzeros
// by column, rows ascending within a column
void append_transpose(int64_t E, const int32_t *ptr, const int32_t *col, const float *val, int64_t nnz, Ints &tt,
                      std::vector<float> &tw) {
    const size_t p0 = tt.size(), w0 = tw.size();
    tt.resize(p0 + E + 1 + nnz, 0);
    tw.resize(w0 + nnz);
    int32_t *tp = tt.data() + p0, *mem = tp + E + 1;
    for (int64_t i = 0; i < nnz; ++i) tp[col[i] + 1]++;
    for (int64_t j = 0; j < E; ++j) tp[j + 1] += tp[j];
    Ints cur(tp, tp + E);
    for (int64_t m = 0; m < E; ++m)
        for (int32_t i = ptr[m]; i < ptr[m + 1]; ++i) {
            const int32_t k = cur[col[i]]++;
            mem[k] = (int32_t)m;
            tw[w0 + k] = val[i];
        }
}

struct Section {
    const void *data;
    size_t words;
};
template <typename T>
Section section(const std::vector<T> &v) {
    static_assert(sizeof(T) == 4, "the tables are 32-bit words");
    return {v.data(), v.size()};
}

// counts | every section's length | the sections
int64_t write_words(std::initializer_list<int32_t> counts, std::initializer_list<Section> sections, int32_t *out,
                    int64_t cap) {
    int64_t need = (int64_t)(counts.size() + sections.size());
    for (const Section &s : sections) need += (int64_t)s.words;
    if (!out || cap < need) return need;
    out = std::copy(counts.begin(), counts.end(), out);
    for (const Section &s : sections) *out++ = (int32_t)s.words;
    for (const Section &s : sections) {
        if (s.words) std::memcpy(out, s.data, s.words * 4);
        out += s.words;
    }
    return need;
}

}  // namespace

const char *gnn_plan_tables(int64_t E, int n_vgroups, const int32_t *vgroup, int n_cgroups, const int32_t *cgroup,
                            GnnPlanTables &t) {
    if (E <= 0 || n_vgroups <= 0 || n_cgroups <= 0 || !vgroup || !cgroup) return "bad GNN plan arguments";
    t = GnnPlanTables();
    t.E = E;
    t.Gv = n_vgroups;
    t.Gc = n_cgroups;
    t.vgroup.assign(vgroup, vgroup + E);
    t.cgroup.assign(cgroup, cgroup + E);
    if (!group_csr(t.vgroup, t.Gv, t.vg_ptr, t.vg_mem) || !group_csr(t.cgroup, t.Gc, t.cg_ptr, t.cg_mem))
        return "group label out of range";
    append_inverse_sizes(t.vg_ptr, t.inv);
    append_inverse_sizes(t.cg_ptr, t.inv);
    build_group_tiles(t);
    build_check_tiles(t);
    build_row_walk(t);
    build_proj_tiles(t);
    build_message_perm(t);
    return nullptr;
}

const char *gnn_csr_tables(int64_t E, const int32_t *v_ptr, const int32_t *v_col, const float *v_val,
                           const int32_t *c_ptr, const int32_t *c_col, const float *c_val, GnnCsrTables &t) {
    if (E <= 0 || E > (1 << 30) || !v_ptr || !c_ptr) return "bad GNN CSR plan arguments";
    const int64_t nv = v_ptr[E], nc = c_ptr[E];
    if (v_ptr[0] != 0 || c_ptr[0] != 0 || nv < 0 || nc < 0 || (nv && (!v_col || !v_val)) || (nc && (!c_col || !c_val)))
        return "bad CSR arrays";
    for (int64_t m = 0; m < E; ++m)
        if (v_ptr[m + 1] < v_ptr[m] || c_ptr[m + 1] < c_ptr[m]) return "CSR row pointers must ascend";
    for (int64_t i = 0; i < nv; ++i)
        if (v_col[i] < 0 || v_col[i] >= E) return "CSR column out of range";
    for (int64_t i = 0; i < nc; ++i)
        if (c_col[i] < 0 || c_col[i] >= E) return "CSR column out of range";
    t = GnnCsrTables();
    t.E = E;
    t.nv = nv;
    t.nc = nc;
    t.tab.reserve(2 * E + 2 * (E + 1) + nv + nc);
    for (int side = 0; side < 2; ++side)  // vgroup, cgroup: every message reads its own row
        for (int64_t m = 0; m < E; ++m) t.tab.push_back((int32_t)m);
    t.tab.insert(t.tab.end(), v_ptr, v_ptr + E + 1);
    t.tab.insert(t.tab.end(), v_col, v_col + nv);
    t.tab.insert(t.tab.end(), c_ptr, c_ptr + E + 1);
    t.tab.insert(t.tab.end(), c_col, c_col + nc);
    t.inv.assign(2 * E, 1.0f);
    t.w.insert(t.w.end(), v_val, v_val + nv);
    t.w.insert(t.w.end(), c_val, c_val + nc);
    t.w.push_back(0.0f);
    append_transpose(E, v_ptr, v_col, v_val, nv, t.tt, t.tw);
    append_transpose(E, c_ptr, c_col, c_val, nc, t.tt, t.tw);
    t.tw.push_back(0.0f);
    return nullptr;
}

int64_t gnn_plan_tables_words(const GnnPlanTables &t, int32_t *out, int64_t cap) {
    return write_words({t.n_gtiles(), t.n_gtiles_v1, t.n_gtiles_v, t.n_ptiles(), t.n_ptiles_v, t.n_ptiles_v1, t.n_mtiles(),
                        t.n_mtiles_v1, t.n_ctiles(), (int32_t)t.ct_aligned, t.n_rw(), (int32_t)t.rw_d1},
                       {section(t.vgroup), section(t.cgroup), section(t.vg_ptr), section(t.vg_mem), section(t.cg_ptr),
                        section(t.cg_mem), section(t.inv), section(t.gt_meta), section(t.gt_grp), section(t.gt_mem),
                        section(t.pt_meta), section(t.pt_grp), section(t.pt_deg), section(t.pt_mem), section(t.mt_perm),
                        section(t.ct_m0), section(t.rw_meta)},
                       out, cap);
}

int64_t gnn_csr_tables_words(const GnnCsrTables &t, int32_t *out, int64_t cap) {
    return write_words({(int32_t)t.E, (int32_t)t.nv, (int32_t)t.nc},
                       {section(t.tab), section(t.inv), section(t.w), section(t.tt), section(t.tw)}, out, cap);
}

}  // namespace ldpc
