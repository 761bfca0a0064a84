// gnn_plan_tables.hpp -- the message-GNN plan's tables as host vectors.  gnn_plan_tables.cpp fills
// them with no HIP call (so tests and a sanitizer build reach them without a device); gnn_plan.cpp
// uploads them, one device allocation per family.  gnn.hpp documents every table's content.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ldpc {

// Group plan (ldpc_gnn_plan_create).  Each line of vectors is one device allocation, in this order.
struct GnnPlanTables {
    int64_t E = 0;
    int Gv = 0, Gc = 0;
    std::vector<int32_t> vgroup, cgroup, vg_ptr, vg_mem, cg_ptr, cg_mem;  // d_tab
    std::vector<float> inv;                                               // d_inv: inv_v[Gv] inv_c[Gc]
    std::vector<int32_t> gt_meta, gt_grp, gt_mem;                         // d_gt
    std::vector<int32_t> pt_meta, pt_grp, pt_deg, pt_mem, mt_perm;        // d_pt
    std::vector<int32_t> ct_m0;                                           // d_ct
    std::vector<int32_t> rw_meta;                                         // d_rw (empty: no row walk)
    int n_gtiles_v1 = 0, n_gtiles_v = 0;
    int n_ptiles_v = 0, n_ptiles_v1 = 0;
    int n_mtiles_v1 = 0;
    bool ct_aligned = false, rw_d1 = false;
    int n_gtiles() const { return (int)(gt_meta.size() / 2); }
    int n_ptiles() const { return (int)(pt_meta.size() / 4); }
    int n_mtiles() const { return (int)(mt_perm.size() / 32); }
    int n_ctiles() const { return (int)ct_m0.size() - 1; }
    int n_rw() const { return (int)(rw_meta.size() / 8); }
};

// CSR plan (ldpc_gnn_plan_create_csr).  One device allocation per vector.
struct GnnCsrTables {
    int64_t E = 0, nv = 0, nc = 0;  // messages, nonzeros of the var side and of the check side
    std::vector<int32_t> tab;       // vgroup[E] cgroup[E] (own row) vg_ptr[E+1] vg_mem[nv] cg_ptr[E+1] cg_mem[nc]
    std::vector<float> inv;         // 1 for every row: inv_v[E] inv_c[E]
    std::vector<float> w;           // vg_w[nv] cg_w[nc] 0
    std::vector<int32_t> tt;        // the transposes: vt_ptr[E+1] vt_mem[nv] ct_ptr[E+1] ct_mem[nc]
    std::vector<float> tw;          // vt_w[nv] ct_w[nc] 0
};

// Both return null, or the message of the argument error (LDPC_EINVAL) that stopped them.
const char *gnn_plan_tables(int64_t E, int n_vgroups, const int32_t *vgroup, int n_cgroups, const int32_t *cgroup,
                            GnnPlanTables &t);
const char *gnn_csr_tables(int64_t E, const int32_t *v_ptr, const int32_t *v_col, const float *v_val,
                           const int32_t *c_ptr, const int32_t *c_col, const float *c_val, GnnCsrTables &t);

// The tables as 32-bit words (ldpc_amd.h, ldpc_gnn_plan_tables / _csr): the words needed; out is
// filled when cap holds them.
int64_t gnn_plan_tables_words(const GnnPlanTables &t, int32_t *out, int64_t cap);
int64_t gnn_csr_tables_words(const GnnCsrTables &t, int32_t *out, int64_t cap);

}  // namespace ldpc
