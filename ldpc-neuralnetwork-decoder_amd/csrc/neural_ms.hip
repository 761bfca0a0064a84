// neural_ms.hip -- LDPCNeuralDecoder's inference forward (models/decoder.py) as one kernel.
//
// The layer chain (layers.hip) runs 4 I - 1 launches and carries every (B, E) message row through
// HBM between them.  Inference saves no activations, and one frame's whole state -- the LLR row, one
// check-message row and the ring of max(depth_L, 1) variable-message rows -- fits a CU's LDS beside
// the 16-bit index tables, so here a workgroup owns F frames and runs every iteration on them in LDS:
// HBM sees the LLRs in, the weights (shared by all frames: L2) and the output.
//
// The arithmetic is the layer kernels' operation sequence, float32, nothing fused (the library is
// built with -ffp-contract=off), so the output equals the layer path's bit for bit:
//   x0[e]  = +0.0f + llr[var(e)]                       gather_sum_kernel on the x0 index
//   c_l    = check_group_minsum on v_{l-1}             (check_group.hpp, shared with layers.hip)
//   S[e]   = +0.0f + the variable's other c_l, ascending (prefix, then tail)   var_group_sum_kernel
//   v_l[e] = x0[e] * w_ch_l[e]; + S[e]; + w_res_l[i] * v_{l-1-i}[e], i < min(l, depth_L)   residual_kernel
//   app[j] = +0.0f + the variable's c_{I-1}, ascending                           gather_sum_kernel
//   soft   = 1 / (1 + expf(-((-app) + (-llr))))                                  output_layer_kernel
// One thread per (frame, edge) in the variable update: with the rows in LDS its at most degree - 1
// adds are a chain of 22 on BG2's degree-23 columns, where the per-run walk of var_group_sum_kernel
// is ~260 long.  v_l[e] goes to ring slot l mod R, the slot of v_{l-R}[e], which only this thread
// reads (as its last residual term): no cross-thread hazard on the ring.  The check rule works in
// place, so v_l is copied into the c row behind a barrier (other threads still read c for their S).
#include <cstdint>

#include "check_group.hpp"
#include "common.hpp"
#include "neural_layout.hpp"

struct ldpc_neural_plan {
    ldpc::NeuralLayout L;  // the table part (frames / threads / LDS depend on depth_L: neural_layout)
    uint16_t *d_tab = nullptr;
    int device = 0;
};

namespace ldpc {
namespace {

struct NeuralArgs {
    const uint16_t *tab;
    const float *w_ch, *w_res, *llr;
    float *app, *soft;
    int64_t B;
    int N, G, E, K, Np, Ep, R, FS, o_cptr, o_evar, o_vptr, table_words, F, I, D;
};

// work item w of nb x n -> (frame, index); one frame per workgroup needs no division
__device__ __forceinline__ void split(int w, int n, int nb, int &f, int &i) {
    f = nb == 1 ? 0 : w / n;
    i = w - f * n;
}

// S + c[t0] + c[t0 + 1] + ... + c[t1 - 1], added in this order, leaving out t == skip.  Four loads are
// issued before the first add (one LDS round trip per four members instead of one each); a load past
// t1 stays inside the frame's rows (c is followed by the ring) and its value is not used.
__device__ __forceinline__ float add_run(float S, const float *c, int t0, int t1, int skip) {
    for (int t = t0; t < t1; t += 4) {
        float x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = c[t + k];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (t + k < t1 && t + k != skip) S += x[k];
    }
    return S;
}

__global__ __launch_bounds__(kNeuralMaxThreads) void neural_ms_kernel(NeuralArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];  // [F][llr Np | c Ep | ring R x Ep] | u16 tables
    uint16_t *tab = reinterpret_cast<uint16_t *>(smem + (size_t)a.F * a.FS);
    const uint16_t *cm = tab, *cp = tab + a.o_cptr, *ev = tab + a.o_evar, *vp = tab + a.o_vptr;
    const int64_t b0 = (int64_t)blockIdx.x * a.F;
    const int nb = (int)min<int64_t>(a.F, a.B - b0);
    const int tid = threadIdx.x, nt = blockDim.x;
    const int N = a.N, E = a.E, Np = a.Np, Ep = a.Ep, R = a.R, FS = a.FS;

    {  // the tables: the plan's blob has the LDS image's order and padding (a multiple of 8 words)
        const uint4 *s = reinterpret_cast<const uint4 *>(a.tab);
        uint4 *d = reinterpret_cast<uint4 *>(tab);
        for (int i = tid; i < a.table_words / 8; i += nt) d[i] = s[i];
    }
    const float *src = a.llr + b0 * N;  // the workgroup's LLR rows are one contiguous span
    for (int w = tid; w < nb * N; w += nt) {
        int f, j;
        split(w, N, nb, f, j);
        smem[f * FS + j] = src[w];
    }
    __syncthreads();
    for (int w = tid; w < nb * E; w += nt) {
        int f, e;
        split(w, E, nb, f, e);
        float *fr = smem + f * FS;
        fr[Np + e] = 0.0f + fr[ev[e]];
    }
    __syncthreads();

    for (int l = 0;; ++l) {
        // rounds alternate direction: a thread's second check is one of the other end of the list, so
        // BG2's long first rows (one serial walk per check) do not meet a second check in their wave
        for (int w0 = 0, back = 0; w0 < nb * a.G; w0 += nt, back ^= 1) {
            const int w = w0 + (back ? nt - 1 - tid : tid);
            if (w >= nb * a.G) continue;
            int f, g;
            split(w, a.G, nb, f, g);
            check_group_minsum(smem + f * FS + Np, cm, cp[g], cp[g + 1], a.K);
        }
        __syncthreads();
        if (l == a.I - 1) break;
        const float *wch = a.w_ch + (size_t)l * E, *wres = a.w_res + (size_t)l * a.D;
        const int np = min(l, a.D), newest = l % R;
        for (int w = tid; w < nb * E; w += nt) {
            int f, e;
            split(w, E, nb, f, e);
            float *fr = smem + f * FS, *ring = fr + Np + Ep;
            const float *c = fr + Np;
            const float wc = wch[e];  // L2: issued before the LDS walk, used after it
            const int j = ev[e], s0 = vp[j], s1 = vp[j + 1];
            const float x0 = 0.0f + fr[j];
            const float S = add_run(0.0f, c, s0, s1, e);
            float r = x0 * wc;
            r = r + S;
            int slot = newest;  // v_{l-1-i} sits in slot (l - 1 - i) mod R
            for (int i = 0; i < np; ++i) {
                slot = slot == 0 ? R - 1 : slot - 1;
                r = r + wres[i] * ring[slot * Ep + e];
            }
            ring[newest * Ep + e] = r;
        }
        __syncthreads();  // every S has been read: c may take v_l
        for (int w = tid; w < nb * E; w += 4 * nt) {  // four loads in flight, then their stores
            float x[4];
            int at[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int f, e;
                split(min(w + k * nt, nb * E - 1), E, nb, f, e);
                at[k] = f * FS + Np + e;
                x[k] = smem[at[k] + Ep + newest * Ep];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (w + k * nt < nb * E) smem[at[k]] = x[k];
        }
        __syncthreads();
    }

    for (int w = tid; w < nb * N; w += nt) {
        int f, j;
        split(w, N, nb, f, j);
        const float *fr = smem + f * FS, *c = fr + Np;
        const float s = add_run(0.0f, c, vp[j], vp[j + 1], -1);
        const int64_t o = b0 * N + w;
        if (a.app) a.app[o] = s;
        if (a.soft) a.soft[o] = 1.0f / (1.0f + expf(-((-s) + (-fr[j]))));
    }
}

int describe(int N, int G, int64_t E, const int32_t *cptr, const int32_t *cmem, const int32_t *vptr, int K,
             NeuralLayout &L) {
    if (const char *msg = neural_validate(N, G, E, cptr, cmem, vptr, K)) return fail(LDPC_EINVAL, msg);
    neural_table_layout(N, G, (int)E, K, L);
    return LDPC_OK;
}

}  // namespace
}  // namespace ldpc

using namespace ldpc;

extern "C" int ldpc_neural_layout(int N, int G, int64_t E, const int32_t *h_cptr, const int32_t *h_cmem,
                                  const int32_t *h_vptr, int K, int depth_L, int *frames, int *threads,
                                  int64_t *lds_bytes) {
    NeuralLayout L;
    if (int rc = describe(N, G, E, h_cptr, h_cmem, h_vptr, K, L)) return rc;
    if (depth_L < 0) return fail(LDPC_EINVAL, "depth_L is negative");
    if (const char *msg = neural_layout(depth_L, L)) return fail(LDPC_EUNSUPPORTED, msg);
    if (frames) *frames = L.frames;
    if (threads) *threads = L.threads;
    if (lds_bytes) *lds_bytes = (int64_t)L.lds_bytes;
    return LDPC_OK;
}

extern "C" int ldpc_neural_plan_create(int N, int G, int64_t E, const int32_t *h_cptr, const int32_t *h_cmem,
                                       const int32_t *h_vptr, int K, ldpc_neural_plan **out) {
    if (!out) return fail(LDPC_EINVAL, "out is NULL");
    *out = nullptr;
    NeuralLayout L;
    if (int rc = describe(N, G, E, h_cptr, h_cmem, h_vptr, K, L)) return rc;
    NeuralLayout probe = L;  // a graph no depth_L can run gets no plan
    if (const char *msg = neural_layout(0, probe)) return fail(LDPC_EUNSUPPORTED, msg);
    const std::vector<uint16_t> t = neural_tables(L, h_cptr, h_cmem, h_vptr);
    auto *p = new ldpc_neural_plan();
    p->L = L;
    hipError_t e = hipGetDevice(&p->device);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&p->d_tab), t.size() * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMemcpy(p->d_tab, t.data(), t.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        if (p->d_tab) (void)hipFree(p->d_tab);
        delete p;
        return fail(LDPC_EHIP, std::string("neural plan upload: ") + hipGetErrorString(e));
    }
    *out = p;
    return LDPC_OK;
}

extern "C" int ldpc_neural_plan_destroy(ldpc_neural_plan *p) {
    if (!p) return LDPC_OK;
    if (p->d_tab) (void)hipFree(p->d_tab);
    delete p;
    return LDPC_OK;
}

extern "C" int ldpc_neural_forward(const ldpc_neural_plan *p, int iterations, int depth_L, const float *d_w_ch,
                                   const float *d_w_res, const float *d_llr, int64_t B, float *d_app, float *d_soft,
                                   void *stream) {
    if (!p) return fail(LDPC_EINVAL, "plan is NULL");
    if (iterations < 1 || depth_L < 0 || B < 0) return fail(LDPC_EINVAL, "bad neural-forward arguments");
    NeuralLayout L = p->L;
    if (const char *msg = neural_layout(depth_L, L)) return fail(LDPC_EUNSUPPORTED, msg);
    if (!d_app && !d_soft) return fail(LDPC_EINVAL, "neither d_app nor d_soft is given");
    if (!B) return LDPC_OK;
    if (!d_llr) return fail(LDPC_EINVAL, "d_llr is NULL");
    if (iterations > 1 && (!d_w_ch || (depth_L > 0 && !d_w_res))) return fail(LDPC_EINVAL, "NULL weights");
    const int64_t nwg = (B + L.frames - 1) / L.frames;
    if (nwg > 0x7fffffff) return fail(LDPC_EUNSUPPORTED, "batch too large for one launch");
    NeuralArgs a{};
    a.tab = p->d_tab;
    a.w_ch = d_w_ch; a.w_res = d_w_res; a.llr = d_llr; a.app = d_app; a.soft = d_soft;
    a.B = B;
    a.N = L.N; a.G = L.G; a.E = L.E; a.K = L.K; a.Np = L.Np; a.Ep = L.Ep; a.R = L.ring; a.FS = L.frame_floats;
    a.o_cptr = L.o_cptr; a.o_evar = L.o_evar; a.o_vptr = L.o_vptr; a.table_words = L.table_words;
    a.F = L.frames; a.I = iterations; a.D = depth_L;
    if (L.lds_bytes > 64 * 1024)
        LDPC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(neural_ms_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds_bytes));
    hipLaunchKernelGGL(neural_ms_kernel, dim3((unsigned)nwg), dim3((unsigned)L.threads), L.lds_bytes,
                       static_cast<hipStream_t>(stream), a);
    LDPC_CHECK_LAUNCH("neural_ms_kernel");
    return LDPC_OK;
}
