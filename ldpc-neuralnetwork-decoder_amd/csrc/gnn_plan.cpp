// gnn_plan.cpp -- the message-GNN plan's C entry points: the tables of gnn_plan_tables.cpp uploaded
// to the current device and viewed through ldpc_gnn_plan's pointers (gnn.hpp).  No kernels here.
#include <initializer_list>
#include <vector>

#include "common.hpp"
#include "gnn.hpp"
#include "gnn_plan_tables.hpp"

using namespace ldpc;

namespace {

// One device allocation holding the parts back to back (nothing to hold: *dst stays null).  Returns
// null or the error message; the plan's destroy frees what was allocated.
template <typename T>
const char *upload(T **dst, std::initializer_list<const std::vector<T> *> parts) {
    size_t n = 0;
    for (const auto *v : parts) n += v->size();
    if (!n) return nullptr;
    if (hipMalloc(dst, n * sizeof(T)) != hipSuccess) return "GNN plan allocation failed";
    T *d = *dst;
    for (const auto *v : parts) {
        if (!v->empty() && hipMemcpy(d, v->data(), v->size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
            return "GNN plan upload failed";
        d += v->size();
    }
    return nullptr;
}

int upload_failed(ldpc_gnn_plan *p, const char *msg) {
    ldpc_gnn_plan_destroy(p);
    return fail(LDPC_EHIP, msg);
}

}  // namespace

extern "C" int ldpc_gnn_plan_create(int64_t E, int n_vgroups, const int32_t *h_vgroup, int n_cgroups,
                                    const int32_t *h_cgroup, ldpc_gnn_plan **out) {
    if (!out) return fail(LDPC_EINVAL, "out is NULL");
    *out = nullptr;
    GnnPlanTables t;
    if (const char *msg = gnn_plan_tables(E, n_vgroups, h_vgroup, n_cgroups, h_cgroup, t)) return fail(LDPC_EINVAL, msg);
    auto *p = new ldpc_gnn_plan();
    p->E = E;
    p->Gv = n_vgroups;
    p->Gc = n_cgroups;
    if (hipGetDevice(&p->device) != hipSuccess) return upload_failed(p, "GNN plan allocation failed");
    const char *msg = upload(&p->d_tab, {&t.vgroup, &t.cgroup, &t.vg_ptr, &t.vg_mem, &t.cg_ptr, &t.cg_mem});
    if (!msg) msg = upload(&p->d_inv, {&t.inv});
    if (!msg) msg = upload(&p->d_gt, {&t.gt_meta, &t.gt_grp, &t.gt_mem});
    if (!msg) msg = upload(&p->d_pt, {&t.pt_meta, &t.pt_grp, &t.pt_deg, &t.pt_mem, &t.mt_perm});
    if (!msg) msg = upload(&p->d_ct, {&t.ct_m0});
    if (!msg) msg = upload(&p->d_rw, {&t.rw_meta});
    if (msg) return upload_failed(p, msg);
    p->vgroup = p->d_tab;
    p->cgroup = p->vgroup + E;
    p->vg_ptr = p->cgroup + E;
    p->vg_mem = p->vg_ptr + n_vgroups + 1;
    p->cg_ptr = p->vg_mem + E;
    p->cg_mem = p->cg_ptr + n_cgroups + 1;
    p->inv_v = p->d_inv;
    p->inv_c = p->d_inv + n_vgroups;
    p->n_gtiles = t.n_gtiles();
    p->n_gtiles_v1 = t.n_gtiles_v1;
    p->n_gtiles_v = t.n_gtiles_v;
    p->gt_meta = reinterpret_cast<const int2 *>(p->d_gt);
    p->gt_grp = p->d_gt + t.gt_meta.size();
    p->gt_mem = p->gt_grp + t.gt_grp.size();
    p->n_ptiles = t.n_ptiles();
    p->n_ptiles_v = t.n_ptiles_v;
    p->n_ptiles_v1 = t.n_ptiles_v1;
    p->pt_meta = reinterpret_cast<const int4 *>(p->d_pt);
    p->pt_grp = p->d_pt + t.pt_meta.size();
    p->pt_deg = p->pt_grp + t.pt_grp.size();
    p->pt_mem = p->pt_deg + t.pt_deg.size();
    p->mt_perm = p->pt_mem + t.pt_mem.size();
    p->n_mtiles = t.n_mtiles();
    p->n_mtiles_v1 = t.n_mtiles_v1;
    p->n_ctiles = t.n_ctiles();
    p->ct_aligned = t.ct_aligned;
    p->ct_m0 = p->d_ct;
    p->n_rw = t.n_rw();
    p->rw_d1 = t.rw_d1;
    p->rw_meta = reinterpret_cast<const int4 *>(p->d_rw);
    *out = p;
    return LDPC_OK;
}

// General adjacencies (message_gnn_decoder.py:93-118: any (E x E) matrix after the reference's
// zero-pad / crop) as two CSR matrices: row m lists the messages j with A[m, j] != 0, ascending, and
// their values.  Every message reads aggregation row m of each side, so the MLP kernels run
// unchanged on rows that are bmm(A, c) instead of group means.
extern "C" int ldpc_gnn_plan_create_csr(int64_t E, const int32_t *h_v_ptr, const int32_t *h_v_col, const float *h_v_val,
                                        const int32_t *h_c_ptr, const int32_t *h_c_col, const float *h_c_val,
                                        ldpc_gnn_plan **out) {
    if (!out) return fail(LDPC_EINVAL, "out is NULL");
    *out = nullptr;
    GnnCsrTables t;
    if (const char *msg = gnn_csr_tables(E, h_v_ptr, h_v_col, h_v_val, h_c_ptr, h_c_col, h_c_val, t))
        return fail(LDPC_EINVAL, msg);
    auto *p = new ldpc_gnn_plan();
    p->E = E;
    p->Gv = (int)E;
    p->Gc = (int)E;
    p->weighted = true;
    if (hipGetDevice(&p->device) != hipSuccess) return upload_failed(p, "GNN plan allocation failed");
    const char *msg = upload(&p->d_tab, {&t.tab});
    if (!msg) msg = upload(&p->d_inv, {&t.inv});
    if (!msg) msg = upload(&p->d_w, {&t.w});
    if (!msg) msg = upload(&p->d_tt, {&t.tt});
    if (!msg) msg = upload(&p->d_tw, {&t.tw});
    if (msg) return upload_failed(p, msg);
    p->vgroup = p->d_tab;
    p->cgroup = p->vgroup + E;
    p->vg_ptr = p->cgroup + E;
    p->vg_mem = p->vg_ptr + E + 1;
    p->cg_ptr = p->vg_mem + t.nv;
    p->cg_mem = p->cg_ptr + E + 1;
    p->inv_v = p->d_inv;
    p->inv_c = p->d_inv + E;
    p->vg_w = p->d_w;
    p->cg_w = p->d_w + t.nv;
    p->vt_ptr = p->d_tt;
    p->vt_mem = p->vt_ptr + E + 1;
    p->ct_ptr = p->vt_mem + t.nv;
    p->ct_mem = p->ct_ptr + E + 1;
    p->vt_w = p->d_tw;
    p->ct_w = p->d_tw + t.nv;
    *out = p;
    return LDPC_OK;
}

extern "C" int ldpc_gnn_plan_destroy(ldpc_gnn_plan *p) {
    if (!p) return LDPC_OK;
    for (void *d : {(void *)p->d_tab, (void *)p->d_inv, (void *)p->d_w, (void *)p->d_tt, (void *)p->d_tw, (void *)p->d_gt,
                    (void *)p->d_pt, (void *)p->d_ct, (void *)p->d_rw})
        if (d) (void)hipFree(d);
    delete p;
    return LDPC_OK;
}

extern "C" int64_t ldpc_gnn_plan_tables(int64_t E, int n_vgroups, const int32_t *h_vgroup, int n_cgroups,
                                        const int32_t *h_cgroup, int32_t *h_words, int64_t capacity) {
    GnnPlanTables t;
    if (const char *msg = gnn_plan_tables(E, n_vgroups, h_vgroup, n_cgroups, h_cgroup, t)) return fail(LDPC_EINVAL, msg);
    return gnn_plan_tables_words(t, h_words, capacity);
}

extern "C" int64_t ldpc_gnn_plan_tables_csr(int64_t E, const int32_t *h_v_ptr, const int32_t *h_v_col,
                                            const float *h_v_val, const int32_t *h_c_ptr, const int32_t *h_c_col,
                                            const float *h_c_val, int32_t *h_words, int64_t capacity) {
    GnnCsrTables t;
    if (const char *msg = gnn_csr_tables(E, h_v_ptr, h_v_col, h_v_val, h_c_ptr, h_c_col, h_c_val, t))
        return fail(LDPC_EINVAL, msg);
    return gnn_csr_tables_words(t, h_words, capacity);
}
