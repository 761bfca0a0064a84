// flood_fixed.hpp -- flood_fixed_kernel and its launcher: included by flood_fixed_ms.hip and
// flood_fixed_bp.hip only (flood_dev.hpp holds what every flood*.hip unit shares).
//
// flood_fixed_kernel: the same algorithm for a graph whose schedule is known at compile time
// (gen/fixed_codes.hpp: the reference's two codes), specialised per wave.  Every slot offset,
// shift, degree and task list is a constant, and the loop-invariant per-lane data lives in
// registers for the whole decode:
//   ext[]   the channel LLRs of the wave's degree-1 edges (their v2c forever)
//   cllr[]  the channel LLRs of the wave's columns
//   rot[]   the rotated LDS address base + 4 (f*Z + (k - s) mod Z) of every rotation s the wave
//           reads with
//   msg[]   the messages of the wave's register edges (reg_edges() further down): edges whose
//           check lane and variable lane are the same lane of this wave, so the message never
//           leaves its VGPR -- no slot traffic, no rotation
//   rmsg[]  the messages of the wave's rotated edges (further down): the wave's own edges with a
//           shift, moved between their two lanes by one ds_swizzle_b32 -- no slot traffic either
// so the iteration touches no global memory and computes no addresses: every message is a
// ds_read at rot[s] + slot*256 (immediate offsets) and a ds_write_addtid at slot*256.  Both
// phases are software-pipelined: the next row's / column's LDS reads are issued before the
// current one is computed (slots are disjoint between rows and between columns, so the reads
// never depend on the writes in flight).  Bit-identical to flood_kernel.
//
// Slots.  Unlike flood_kernel's (always check-indexed) slots, a slot's layout here alternates with
// the phase, so that every store is the own-lane ds_write_addtid_b32 (no address VGPR, half the
// LDS cycles of a ds_write_b32 at a rotated address):
//   after a check phase     check-indexed: position k holds the c2v of check row k
//   after a variable phase  variable-indexed: position t holds the v2c of variable t (init too)
// and both phases read rotated: the variable lane t reads position (t - s) mod Z, the check lane k
// position (k + s) mod Z, which is the same rotation for the shift Z - s.  rot[] holds one entry
// per distinct rotation of the wave's columns and rows (FxPlan::make).
// Ordering.  All of this is about LDS slots: a register edge's message is a VGPR that one lane
// writes and the same lane reads, ordered by the program like any other value (its slot number
// stays allocated and unused).  Across waves nothing differs from in-place slots: in each phase a slot belongs to
// one wave (its row's in the check phase, its column's in the variable phase) and the two barriers
// separate the phases.  Inside the owning wave a lane now stores to a position that another lane
// of the same wave reads, so every read of a slot must be issued before the first store to it.
// A wave's DS instructions execute in issue order, and the compiler keeps the order because the
// asm stores carry a "memory" clobber.  In the check phase a two-minimum row's outputs depend on
// every input of the row, so data dependence gives the order as well; a directly computed row's
// output e (LDPC_DIRECT_DC) does not depend on input e, and there the order rests on load_row
// reading the whole row before row's first store.  In the variable phase output e
// does not depend on input e either: there the order rests on load_task reading the whole column
// before task's first store, which is why a column's outputs are always one task (a task's stores
// turn its slots variable-indexed: a second task over the column would read the wrong layout).
// Reads issued ahead for the next row / task touch other slots.
// The compiler does not count the asm stores in its lgkmcnt waits; LDS returns in order, so it can
// only wait longer than needed, never shorter.
#pragma once
#include "flood_host.hpp"
#include "gen/fixed_codes.hpp"

namespace ldpc {
namespace {

// Register edges (gen/fixed_codes.hpp RE_*, tools/gen_fixed_codes.py reg_edge_schedule): the checks
// of every block row are relabelled by an offset rho_r, so that the kernel sees the shifts
// (s + rho_r) mod Z -- the same code, the same operation order -- and an edge whose normalised shift
// is 0, with its row and its column on one wave, keeps its message in a VGPR (msg[]) of that lane
// instead of an LDS slot.  Without them a kernel reads the schedule as it is (CHK_*, *_SHIFT).
// The BP instances run without: their check phase is bound by the tanh / atanh VALU work, not by
// LDS, and with msg[] bp-z32 measured 1.7 % slower (profiles/r10; the tests pass
// either way).
constexpr bool reg_edges(int algo) { return algo == LDPC_ALGO_MINSUM; }

// Instances that keep the exact slow check update in the kernel (rows<DEC, true>: the batch-stop
// passes, and every min-sum instance when the caller gives no workspace for a redo list) hold both
// forms' registers at once, so they keep at most this many of a wave's register edges: the
// largest values at which none of them spills VGPRs -- one for the instances with
// early stop (3 workgroups per CU, 168 VGPRs: every edge fits), one for those without (4 per CU,
// 128 VGPRs).
#ifndef LDPC_SLOW_REG_EDGES
#define LDPC_SLOW_REG_EDGES 16
#endif
#ifndef LDPC_SLOW_REG_EDGES_OFF
#define LDPC_SLOW_REG_EDGES_OFF 6
#endif
constexpr int kAllRegEdges = 1 << 20;
template <int ES, bool BAIL>
constexpr int reg_edge_cap() {
    return BAIL ? kAllRegEdges : (ES == LDPC_ES_OFF ? LDPC_SLOW_REG_EDGES_OFF : LDPC_SLOW_REG_EDGES);
}

// Rotated edges (RE_ROW_ROT / RE_COL_ROT / RE_NROT): a slot edge outside msg[] whose row and column
// are on one wave, with a normalised shift s != 0.  The wave produces and consumes the message
// itself, so it moves between the check lane and the variable lane by one cross-lane rotation
// inside the Z-lane segment (seg_rotate, at the producer) into rmsg[], instead of a slot store and
// a rotated read: per edge and phase one LDS instruction that sends one VGPR to the LDS unit, not
// two that send a data and an address VGPR.  That traffic, not the instruction count, is what the
// phases' time follows (the same edges through ds_bpermute_b32, data + address,
// gained nothing).  The slot stays allocated and unused, as a register edge's does.
// An instance keeps at most this many over its four waves, handed out wave by wave, the wave with
// the most slot edges in its columns first (the longest variable phase).  The exact-update
// instance without early stop is at its 128 VGPRs already: none.
#ifndef LDPC_ROT_EDGES
#define LDPC_ROT_EDGES (1 << 20)
#endif
#ifndef LDPC_SLOW_ROT_EDGES
#define LDPC_SLOW_ROT_EDGES (1 << 20)
#endif
#ifndef LDPC_SLOW_ROT_EDGES_OFF
#define LDPC_SLOW_ROT_EDGES_OFF 0
#endif
template <int ES, bool BAIL>
constexpr int rot_edge_cap() {
    return BAIL ? LDPC_ROT_EDGES : (ES == LDPC_ES_OFF ? LDPC_SLOW_ROT_EDGES_OFF : LDPC_SLOW_ROT_EDGES);
}

// The joint schedule (gen/fixed_codes.hpp RE_J_*, tools/gen_fixed_codes.py joint_schedule): rows and
// columns placed on the waves together so that the LDS operands of the heaviest wave of each phase
// -- what an iteration's time follows -- are fewest: more edges have both
// ends on one wave and fewer cross waves.  Checks are anonymous and everything that crosses kernels
// (ballot words, candidates, decisions, the redo list) is per variable, so every instance picks its
// family on its own: an instance reads the joint one where it fits its register budget without
// scratch (the r18 register table), the others and BP keep the schedule they had.
// LDPC_JOINT_MASK: bit 0 the BAIL instance without early stop (the flagship), bit 1 BAIL with the
// per-frame stop, bit 2 the exact-update instance without early stop, bit 3 the other exact-update
// instances (per-frame and batch stop, P1, P2); A/B builds set other masks.
#ifndef LDPC_JOINT_MASK
#define LDPC_JOINT_MASK 11
#endif
template <class G, int ALGO, int ES, bool BAIL>
constexpr bool joint_family() {
    if (!reg_edges(ALGO)) return false;
    const int bit = BAIL ? (ES == LDPC_ES_OFF ? 0 : 1) : (ES == LDPC_ES_OFF ? 2 : 3);
    return (LDPC_JOINT_MASK >> bit) & 1;
}

// per-wave compile-time plan; CAP: the first CAP register edges of the wave's msg[] order are kept,
// an edge past it is the shift-0 slot edge it still is (its slot stays allocated).  RCAP: the
// instance's rotated edges (above); an edge past the wave's share is the slot edge it still is.
// REG: reg_edges().  JOINT: the instance reads the joint schedule (RE_J_*, joint_family() below):
// rows, shifts, register and rotated edges, columns and tasks all come from that family.
template <class G, int WV, int CAP, int RCAP, bool REG, bool JOINT>
struct FxPlan {
    static_assert(REG || !JOINT, "the joint schedule is a register-edge schedule");
    // the family's arrays: the joint schedule's, the register-edge schedule's or the plain one's
    static constexpr int chk_ptr(int w) { return JOINT ? G::RE_J_CHK_PTR[w] : (REG ? G::RE_CHK_PTR[w] : G::CHK_PTR[w]); }
    static constexpr int chk_rows(int x) { return JOINT ? G::RE_J_CHK_ROWS[x] : (REG ? G::RE_CHK_ROWS[x] : G::CHK_ROWS[x]); }
    static constexpr int nreg(int w) { return JOINT ? G::RE_J_NREG[w] : G::RE_NREG[w]; }
    static constexpr int nrot(int w) { return JOINT ? G::RE_J_NROT[w] : G::RE_NROT[w]; }
    static constexpr int row_reg_all(int e) { return JOINT ? G::RE_J_ROW_REG[e] : G::RE_ROW_REG[e]; }
    static constexpr int col_reg_all(int j) { return JOINT ? G::RE_J_COL_REG[j] : G::RE_COL_REG[j]; }
    static constexpr int row_rot_all(int e) { return JOINT ? G::RE_J_ROW_ROT[e] : G::RE_ROW_ROT[e]; }
    static constexpr int col_rot_all(int j) { return JOINT ? G::RE_J_COL_ROT[j] : G::RE_COL_ROT[j]; }
    static constexpr int vt_col_ptr(int w) { return JOINT ? G::RE_J_VT_COL_PTR[w] : G::VT_COL_PTR[w]; }
    static constexpr int vt_cols(int x) { return JOINT ? G::RE_J_VT_COLS[x] : G::VT_COLS[x]; }
    static constexpr int vt_ptr(int w) { return JOINT ? G::RE_J_VT_PTR[w] : G::VT_PTR[w]; }
    static constexpr int vt_a(int x) { return JOINT ? G::RE_J_VT_A[x] : G::VT_A[x]; }
    static constexpr int vt_b(int x) { return JOINT ? G::RE_J_VT_B[x] : G::VT_B[x]; }
    // the wave's rows
    static constexpr int R0 = chk_ptr(WV);
    static constexpr int NR = chk_ptr(WV + 1) - R0;
    static constexpr int NREG = !REG ? 0 : (nreg(WV) < CAP ? nreg(WV) : CAP);
    static constexpr int chk_row(int i) { return chk_rows(R0 + i); }
    // by edge index in row order (ROW_*) / in column order (COL_*): the (normalised) shift, and the
    // edge's index into msg[] (-1: the message lives in its LDS slot)
    static constexpr int row_shift(int e) { return JOINT ? G::RE_J_ROW_SHIFT[e] : (REG ? G::RE_ROW_SHIFT[e] : G::ROW_SHIFT[e]); }
    static constexpr int col_shift(int j) { return JOINT ? G::RE_J_COL_SHIFT[j] : (REG ? G::RE_COL_SHIFT[j] : G::COL_SHIFT[j]); }
    static constexpr int row_reg(int e) { return REG && row_reg_all(e) < CAP ? row_reg_all(e) : -1; }
    static constexpr int col_reg(int j) { return REG && col_reg_all(j) < CAP ? col_reg_all(j) : -1; }
    // the wave's share of the instance's RCAP rotated edges: what the waves with more slot edges
    // in their columns (ties: the lower wave) leave of it
    static constexpr int col_slot_edges(int w) {
        int n = 0;
        for (int i = vt_col_ptr(w); i < vt_col_ptr(w + 1); ++i)
            for (int j = G::COL_PTR[vt_cols(i)]; j < G::COL_PTR[vt_cols(i) + 1]; ++j)
                if (G::COL_SLOT[j] >= 0 && col_reg_all(j) < 0) ++n;
        return n;
    }
    static constexpr int rot_share() {
        if (!REG) return 0;
        int left = RCAP;
        for (int w = 0; w < G::W; ++w) {
            const int a = col_slot_edges(w), b = col_slot_edges(WV);
            if (a > b || (a == b && w < WV)) left -= nrot(w);
        }
        return left < 0 ? 0 : (left < nrot(WV) ? left : nrot(WV));
    }
    static constexpr int NROT = rot_share();
    // the edge's index into rmsg[] (-1: not a rotated edge of this instance)
    static constexpr int row_rot(int e) { return REG && row_rot_all(e) < NROT ? row_rot_all(e) : -1; }
    static constexpr int col_rot(int j) { return REG && col_rot_all(j) < NROT ? col_rot_all(j) : -1; }
    // the wave's columns (LLRs in registers, init, shifts) and its variable tasks
    static constexpr int C0 = vt_col_ptr(WV), NC = vt_col_ptr(WV + 1) - C0;
    static constexpr int T0 = vt_ptr(WV), NT = vt_ptr(WV + 1) - T0;
    static constexpr int col(int i) { return vt_cols(C0 + i); }
    static constexpr int col_index(int col) {
        for (int i = 0; i < NC; ++i)
            if (vt_cols(C0 + i) == col) return i;
        return -1;
    }
    struct Tab {
        int nsh = 0, next = 0, maxdc = 1, maxdv = 1;
        int shv[64] = {};        // distinct rotations the wave reads with (see make)
        int shidx[64] = {};      // shift -> index into shv (or -1)
        int ext_before[64] = {}; // ext edges in the wave's rows before row i
    };
    // the rotation a check lane reads a variable-indexed slot with: row k of a block with shift s
    // meets variable (k + s) mod Z, which is the variable side's rotation for shift Z - s
    static constexpr int inv_shift(int s) { return (G::Z - s) % G::Z; }
    // One rotation table per wave: the shifts of its columns (variable phase, lane t reads
    // position (t - s) mod Z) and the inverse shifts of its rows' slot edges (check phase).
    // A rotated edge needs neither entry: its rotations are instruction constants (seg_rotate).
    static constexpr Tab make() {
        Tab t{};
        for (int i = 0; i < 64; ++i) t.shidx[i] = -1;
        auto use = [&t](int s) {
            if (t.shidx[s] < 0) {
                t.shidx[s] = t.nsh;
                t.shv[t.nsh++] = s;
            }
        };
        for (int i = 0; i < NC; ++i) {
            const int c = vt_cols(C0 + i);
            const int dv = G::COL_PTR[c + 1] - G::COL_PTR[c];
            if (dv > t.maxdv) t.maxdv = dv;
            for (int j = G::COL_PTR[c]; j < G::COL_PTR[c + 1]; ++j)
                if (col_reg(j) < 0 && col_rot(j) < 0) use(col_shift(j));
        }
        for (int i = 0; i < NR; ++i) {
            const int R = chk_row(i);
            t.ext_before[i] = t.next;
            const int dc = G::ROW_PTR[R + 1] - G::ROW_PTR[R];
            if (dc > t.maxdc) t.maxdc = dc;
            for (int e = G::ROW_PTR[R]; e < G::ROW_PTR[R + 1]; ++e) {
                if (G::ROW_SLOT[e] < 0)
                    ++t.next;
                else if (row_reg(e) < 0 && row_rot(e) < 0)
                    use(inv_shift(row_shift(e)));
            }
        }
        return t;
    }
    static constexpr Tab T = make();
    // index into ext[] of edge e of the wave's row i (an edge without a slot)
    static constexpr int ext_index(int i, int e) {
        const int R = chk_row(i);
        int x = T.ext_before[i];
        for (int q = 0; q < e; ++q)
            if (G::ROW_SLOT[G::ROW_PTR[R] + q] < 0) ++x;
        return x;
    }
};

// the next column's reads are issued before the current column's adds when the two columns hold
// at most this many messages together (register budget: 4 workgroups per CU = 128 VGPRs)
constexpr int kVarPipe = 24;

// Min-sum check rows of degree 2 .. LDPC_DIRECT_DC compute every output directly from the other
// inputs on the fast path (direct_row); longer rows keep the two-minimum / select form.
// 0 restores the select form for every row (A/B builds).
#ifndef LDPC_DIRECT_DC
#define LDPC_DIRECT_DC 6
#endif
constexpr int kDirectDc = LDPC_DIRECT_DC;
static_assert(kDirectDc >= 0 && kDirectDc <= 6, "direct_row is written out for degrees 2 .. 6");

__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }

// Output E of a min-sum row of degree DC with no NaN message, without the two minima (a zero
// message gives the reference's outputs up to the sign of a zero, see FixedBody::row):
//   c2v_E = (xor of the other inputs' sign bits) ^ (alpha * min of the other inputs' magnitudes)
// The excluded minimum |x_E| == m1 ? m2 : m1 of the select form is this minimum as a float (a tie
// at m1 puts m1 in m2), the product is the same single multiply, and the sign is the same xor: bit
// for bit the select form, with no compare into an SGPR pair and no v_cndmask.
//   DC <= 4  v_min / v_minimum3 and v_xor / v_bitop3 over the 1 .. 3 other inputs, alpha * min,
//            then product ^ (xor & sign mask) as one v_bitop3 (0x78)
//   DC >= 5  pair minima pr[] = min(|x_2j|, |x_2j+1|) shared by the row, one v_minimum3 over the
//            pair partner and the other pairs (or the odd input) per output; the row's parity goes
//            into alpha's sign once (als: (-alpha) * m = -(alpha * m) exactly), so an output is
//            minimum3, multiply and product ^ (x_E & sign mask)
template <int DC, int E, int CAP>
__device__ __forceinline__ float direct_row(const float (&v)[CAP], const float (&pr)[3], float als, float alv, uint32_t sgn) {
    static_assert(DC >= 2 && DC <= 6 && E < DC && DC <= CAP, "direct form: degrees 2 .. 6");
    constexpr int A = E == 0 ? 1 : 0, B = E <= 1 ? 2 : 1, Cc = E <= 2 ? 3 : 2;  // the first other inputs
    auto bits = [&](int e) { return __float_as_uint(v[e]); };
    if constexpr (DC == 2) {
        return __uint_as_float(__builtin_amdgcn_bitop3_b32(__float_as_uint(alv * fabsf(v[A])), bits(A), sgn, 0x78));
    } else if constexpr (DC == 3) {
        const float m = vmin(fabsf(v[A]), fabsf(v[B]));
        return __uint_as_float(__builtin_amdgcn_bitop3_b32(__float_as_uint(alv * m), bits(A) ^ bits(B), sgn, 0x78));
    } else if constexpr (DC == 4) {
        const float m = vmin(vmin(fabsf(v[A]), fabsf(v[B])), fabsf(v[Cc]));
        return __uint_as_float(__builtin_amdgcn_bitop3_b32(__float_as_uint(alv * m), xor3(bits(A), bits(B), bits(Cc)), sgn, 0x78));
    } else {
        constexpr int PE = E / 2;  // E's pair; DC == 5: input 4 has none
        float m;
        if constexpr (DC == 5 && E == 4)
            m = vmin(pr[0], pr[1]);
        else if constexpr (DC == 5)
            m = vmin(vmin(fabsf(v[E ^ 1]), pr[1 - PE]), fabsf(v[4]));
        else
            m = vmin(vmin(fabsf(v[E ^ 1]), pr[(PE + 1) % 3]), pr[(PE + 2) % 3]);
        return __uint_as_float(__builtin_amdgcn_bitop3_b32(__float_as_uint(als * m), bits(E), sgn, 0x78));
    }
}

// Where a lane's decisions go in a phase that stores them directly (DIRECT: the last iteration
// without early stop and of ES_P2), formed once at the head of the phase: the group's first output
// element as a uniform pointer (an SGPR pair) and the lane's byte offsets from it, so that a column
// decision is compare, select and a store at an immediate offset (COL * Z elements), and the
// decision of a degree-1 variable met through a shift adds its rotated position to the frame's row.
// OUT: LDPC_OUT_U8 / LDPC_OUT_F32, chosen by one uniform branch around the phase (FixedBody::check,
// var), or kOutAny: the type is looked up at every store (the exact check update's phases, which
// never run on real data and are not worth a copy per type).  Lanes without a frame store nothing;
// their error count is never summed (reduce_counters).
constexpr int kOutAny = 2;
template <class G, int OUT>
struct DecOut {
    static_assert(OUT == LDPC_OUT_U8 || OUT == LDPC_OUT_F32 || OUT == kOutAny, "one form per output type");
    // a frame's row starts at a multiple of a block, so a position inside a block can be or-ed in
    static_assert(G::N % G::Z == 0 && (G::Z & (G::Z - 1)) == 0, "rotated(): row | position");
    char *base;    // uniform: variable 0 of the group's first frame
    uint32_t row;  // byte offset of the lane's frame row from base
    uint32_t own;  // row + the lane's position k in a block
    uint32_t kb;   // size() * k
    uint32_t any;  // kOutAny: the element size
    bool valid;
    __device__ __forceinline__ uint32_t size() const {
        if constexpr (OUT == kOutAny)
            return any;
        else
            return OUT == LDPC_OUT_F32 ? 4u : 1u;
    }
    __device__ __forceinline__ DecOut(const Ctx &C, const Lane &L) {
        any = C.out_dtype == LDPC_OUT_F32 ? 4u : 1u;
        base = static_cast<char *>(C.bits) + (int64_t)L.group * (64 / G::Z) * G::N * size();
        row = (uint32_t)L.f * (G::N * size());
        kb = (uint32_t)L.k * size();
        own = row + kb;
        valid = L.valid;
    }
    __device__ __forceinline__ void put(uint32_t off, int bit, int &errs) const {
        if (valid) {
            if (size() == 4u)
                *reinterpret_cast<float *>(base + off) = (float)bit;
            else
                *reinterpret_cast<uint8_t *>(base + off) = (uint8_t)bit;
        }
        errs += bit;
    }
    // variable (COL, k)
    template <int COL>
    __device__ __forceinline__ void col(int bit, int &errs) const { put(own + COL * G::Z * size(), bit, errs); }
    // variable (COL, (k + S) mod Z), decided on the lane of check row k
    template <int COL, int S>
    __device__ __forceinline__ void rotated(int bit, int &errs) const {
        put((row | ((kb + S * size()) & (G::Z * size() - 1))) + COL * G::Z * size(), bit, errs);
    }
};
struct NoOut {  // decisions are not stored directly in this phase
    __device__ __forceinline__ NoOut(const Ctx &, const Lane &) {}
};
template <class G, int OUT>
using DecOutFor = std::conditional_t<OUT < 0, NoOut, DecOut<G, OUT>>;

// BAIL: the min-sum instance holds the fast check update only and leaves the decode when the sticky
// flag is up (flood_drive, Body::kBail); otherwise check() branches to the exact form in the kernel.
template <class G, int ALGO, int WV, bool BAIL, int CAP, int RCAP, bool REG, bool JOINT>
struct FixedBody {
    static_assert(!BAIL || ALGO == LDPC_ALGO_MINSUM, "only min-sum has a fast and an exact check update");
    static constexpr bool kBail = BAIL;
    static constexpr bool kPeel = true;  // decisions of the last iteration only are straight code behind the loop
    using P = FxPlan<G, WV, CAP, RCAP, REG, JOINT>;
    static constexpr int ZM4 = 4 * G::Z - 1;
    static constexpr int NEXT = P::T.next > 0 ? P::T.next : 1;
    static constexpr int NCOL = P::NC > 0 ? P::NC : 1;
    static constexpr int NSH = P::T.nsh > 0 ? P::T.nsh : 1;
    static constexpr int MAXDC = P::T.maxdc, MAXDV = P::T.maxdv;
    static constexpr int NRG = P::NREG > 0 ? P::NREG : 1;
    static constexpr int NRT = P::NROT > 0 ? P::NROT : 1;
    float ext[NEXT];
    // one float past the wave's columns, never written: the compiler widens a pair task's load of
    // cllr[IA] to two floats, and where that reached into rot[] and overlapped the next pair's load
    // the arrays stayed in scratch memory.  Only the joint schedule's column lists meet that, so only
    // its instances carry the float: the others' code stays what it was
    float cllr[NCOL + (JOINT ? 1 : 0)];
    uint32_t rot[NSH];  // absolute LDS byte addresses (lds_rd_abs)
    float msg[NRG];     // the messages of the wave's register edges: v2c after init / var, c2v after check
    float rmsg[NRT];    // the messages of the wave's rotated edges, on the lane that reads them next:
                        // v2c on the check lane after init / var, c2v on the variable lane after check


    // a rotated edge's message (normalised shift S) moved to the lane that reads it next: variable
    // lane t takes the c2v of check (t - S) mod Z, check lane k the v2c of variable (k + S) mod Z --
    // the rotations the slot reads would have used
    template <int S>
    __device__ __forceinline__ float to_var_lane(float c2v) const { return seg_rotate<G::Z, S>(c2v); }
    template <int S>
    __device__ __forceinline__ float to_chk_lane(float v2c) const { return seg_rotate<G::Z, P::inv_shift(S)>(v2c); }

    __device__ __forceinline__ void init(Ctx &C, const Lane &L) {
        bool nan = false;
        sfor<P::NR>([&](auto i) {
            constexpr int I = decltype(i)::value, R = P::chk_row(I);
            constexpr int P0 = G::ROW_PTR[R], DC = G::ROW_PTR[R + 1] - P0;
            sfor<DC>([&](auto e) {
                constexpr int E = decltype(e)::value;
                if constexpr (G::ROW_SLOT[P0 + E] < 0) {
                    constexpr int X = P::ext_index(I, E), COL = G::ROW_COL[P0 + E], S4 = 4 * P::row_shift(P0 + E);
                    ext[X] = L.llr_at(COL * 4 * G::Z + ((L.k4 + S4) & ZM4));
                    nan |= !(fabsf(ext[X]) < INFINITY);  // NaN or infinite: the sticky flag (see check())
                }
            });
        });
        sfor<P::T.nsh>([&](auto j) {
            constexpr int J = decltype(j)::value, SH = P::T.shv[J];
            const uint32_t base = (uint32_t)(uintptr_t)C.lds;
            if constexpr (SH == 0)
                rot[J] = opaque_vu(base + L.lane4);
            else
                rot[J] = opaque_vu(base + L.fz4 + ((L.k4 + (4 * G::Z - 4 * SH)) & ZM4));
        });
        // the first v2c of an edge is its column's LLR: variable-indexed, so stored own-lane (a
        // register edge's variable lane is its check lane: the LLR goes into msg[], no store; a
        // rotated edge's goes to its check lane)
        addtid_begin(C.lds);
        sfor<P::NC>([&](auto i) {
            constexpr int I = decltype(i)::value, COL = P::col(I);
            constexpr int P0 = G::COL_PTR[COL], DV = G::COL_PTR[COL + 1] - P0;
            cllr[I] = L.llr_at(COL * 4 * G::Z + L.k4);
            nan |= !(fabsf(cllr[I]) < INFINITY);
            sfor<DV>([&](auto jj) {
                constexpr int J = P0 + decltype(jj)::value;
                if constexpr (P::col_reg(J) >= 0)
                    msg[P::col_reg(J)] = cllr[I];
                else if constexpr (P::col_rot(J) >= 0)
                    rmsg[P::col_rot(J)] = to_chk_lane<P::col_shift(J)>(cllr[I]);
                else
                    lds_wr_tid<G::COL_SLOT[J] * 256>(cllr[I]);
            });
        });
        addtid_end();
        if (__any(nan) && L.lane == 0) *C.flag = 1;
    }

    // ---- check phase
    template <int I>
    __device__ __forceinline__ void load_row(const Ctx &C, const Lane &L, float (&v)[MAXDC]) const {
        constexpr int R = P::chk_row(I), P0 = G::ROW_PTR[R], DC = G::ROW_PTR[R + 1] - P0;
        sfor<DC>([&](auto e) {
            constexpr int E = decltype(e)::value, SL = G::ROW_SLOT[P0 + E];
            if constexpr (P::row_reg(P0 + E) >= 0)  // register edge: variable k's v2c is in this lane
                v[E] = msg[P::row_reg(P0 + E)];
            else if constexpr (P::row_rot(P0 + E) >= 0)  // rotated edge: var / init moved the v2c here
                v[E] = rmsg[P::row_rot(P0 + E)];
            else if constexpr (SL >= 0) {  // variable-indexed slot: row k's edge is at position (k + s) mod Z
                static_assert(P::T.shidx[P::inv_shift(P::row_shift(P0 + E))] >= 0, "rot[] holds the rotation");
                v[E] = lds_rd_abs<SL * 256>(rot[P::T.shidx[P::inv_shift(P::row_shift(P0 + E))]]);
            } else {
                v[E] = ext[P::ext_index(I, E)];
            }
        });
    }

    template <int I, bool DEC, bool SLOW, int OUT>
    __device__ __forceinline__ void row(const Ctx &C, const Lane &L, const DecOutFor<G, OUT> &D, const float (&v)[MAXDC], int &errs, float ninf, float pinf, uint32_t sgn, float alv) {
        constexpr int R = P::chk_row(I), P0 = G::ROW_PTR[R], DC = G::ROW_PTR[R + 1] - P0;
        // an output is needed for a slot edge always, for a degree-1 edge only to take its decision
        auto needed = [](int e) constexpr { return DEC || G::ROW_SLOT[P0 + e] >= 0; };
        auto emit = [&](auto e, float o) {
            constexpr int E = decltype(e)::value, SL = G::ROW_SLOT[P0 + E];
            if constexpr (P::row_reg(P0 + E) >= 0) {
                msg[P::row_reg(P0 + E)] = o;  // register edge: the c2v stays in this lane
            } else if constexpr (P::row_rot(P0 + E) >= 0) {
                rmsg[P::row_rot(P0 + E)] = to_var_lane<P::row_shift(P0 + E)>(o);  // rotated edge: to its variable lane
            } else if constexpr (SL >= 0) {
                lds_wr_tid<SL * 256>(o);  // ds_write_addtid_b32: the slot entry of a row is slot[lane]
            } else if constexpr (DEC) {
                // degree-1 variable: APP = llr + c2v; NaN < 0 is false -> 0 (traditional_decoders.py:252)
                constexpr int COL = G::ROW_COL[P0 + E], S = P::row_shift(P0 + E);
                const int bit = v[E] + o < 0.0f;
                if constexpr (OUT >= 0) D.template rotated<COL, S>(bit, errs);
                if (C.ballots) ext_ballot(C, L, COL, 4 * S, bit);
            }
        };
        if constexpr (ALGO == LDPC_ALGO_MINSUM && !SLOW && DC >= 2 && DC <= kDirectDc) {
            // short row on the fast path (no NaN: the sticky flag, see below): every
            // output straight from the other inputs, see direct_row
            float pr[3] = {};
            float als = alv;
            if constexpr (DC >= 5) {
                sfor<DC / 2>([&](auto j) {
                    constexpr int J = decltype(j)::value;
                    pr[J] = vmin(fabsf(v[2 * J]), fabsf(v[2 * J + 1]));
                });
                uint32_t par = xor3(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]));
                if constexpr (DC == 5)
                    par = xor3(par, __float_as_uint(v[3]), __float_as_uint(v[4]));
                else
                    par = xor3(par, __float_as_uint(v[3]), __float_as_uint(v[4])) ^ __float_as_uint(v[5]);
                als = __uint_as_float(__builtin_amdgcn_bitop3_b32(__float_as_uint(alv), par, sgn, 0x78));
            }
            sfor<DC>([&](auto e) {
                constexpr int E = decltype(e)::value;
                if constexpr (needed(E)) emit(e, direct_row<DC, E>(v, pr, als, alv, sgn));
            });
        } else if constexpr (ALGO == LDPC_ALGO_MINSUM) {
            // the two smallest magnitudes (v_med3 / v_min with |x| source modifiers)
            // m2 starts as an opaque +inf: a constant one lets the compiler rewrite the first
            // v_med3 as a canonicalising fmaxf
            float m1 = fabsf(v[0]), m2 = pinf;
            two_smallest<DC>(v, m1, m2, ninf);
            // Fast path: no possible NaN in the workgroup (the sticky flag, see var()).  On a row
            // without a zero torch.sign is +-1 on every message, so
            //   c2v_e = (par ^ sign(x_e)) * (alpha * (|x_e| == m1 ? m2 : m1))
            // bit for bit (a tie at m1 puts m1 in m2 too).  A row with a zero message x_z has
            // m1 = 0: every other output is +-(alpha * 0) where the reference has sign 0 times
            // alpha * 0, and output z is the others' parity and minimum as in the reference (its
            // own sign bit is xored out, |x_z| == m1 selects m2).  The values differ in the sign of
            // a zero at most, which no later sum, minimum, decision or syndrome can see
            // (tests/test_minsum_zeros_host.py).  Otherwise MinSumStats (exact NaN semantics).
            // The workgroup's sticky flag (init / var) covers non-finite inputs: one branch per
            // phase instead of one per row, and the hot loop holds the fast code only
            if (!SLOW) {
                // the sign mask and alpha as VGPR operands: an SGPR (or SGPR-held constant) source
                // halves a VALU op's issue rate (tools/ubench), so the per-edge v_bitop3 below and
                // the per-row products run at the full rate
                const uint32_t par = sign_parity_n<DC>(v) & sgn;
                const uint32_t s1 = __float_as_uint(alv * m1) ^ par, s2 = __float_as_uint(alv * m2) ^ par;
                // |x_e| == m1 ? s2 : s1, with each compare issued three instructions ahead of its
                // select (a VALU-written lane mask read by a VALU needs 2 wait states on gfx950;
                // left to the compiler, every edge paid an s_nop 1)
                uint64_t mk[DC];
                uint32_t sel[DC];
                sfor<DC + 3>([&](auto q) {
                    constexpr int Q = decltype(q)::value;
                    if constexpr (Q < DC && needed(Q)) mk[Q] = cmp_eq_abs(v[Q], m1);
                    if constexpr (Q >= 3 && needed(Q - 3)) sel[Q - 3] = cndmask(s1, s2, mk[Q - 3]);
                });
                sfor<DC>([&](auto e) {
                    constexpr int E = decltype(e)::value;
                    if constexpr (needed(E))
                        emit(e, __uint_as_float(__builtin_amdgcn_bitop3_b32(sel[E], __float_as_uint(v[E]), sgn, 0x78)));
                });
            } else {
                MinSumStats st;
                sfor<DC>([&](auto e) { st.add(decltype(e)::value, v[decltype(e)::value]); });
                sfor<DC>([&](auto e) { emit(e, st.c2v(decltype(e)::value, v[decltype(e)::value], C.alpha)); });
            }
        } else {
            // sum-product (traditional_decoders.py:72-81): exclusive product from 1.0 ascending
            float acc[DC];
            float Pp = 1.0f;
            sfor<DC>([&](auto jj) {
                constexpr int J = decltype(jj)::value;
                const float t = tanh_half(v[J]);
                sfor<J>([&](auto e) { acc[decltype(e)::value] = acc[decltype(e)::value] * t; });
                acc[J] = Pp;
                Pp = Pp * t;
            });
            sfor<DC>([&](auto e) { emit(e, two_atanh(acc[decltype(e)::value])); });
        }
    }

    // DIRECT: decisions are stored directly, in the output type picked here for the whole phase
    template <bool DEC, bool DIRECT>
    __device__ __forceinline__ void check(const Ctx &C, const Lane &L, int &errs) {
        static_assert(DEC || !DIRECT, "stores need decisions");
        if constexpr (ALGO == LDPC_ALGO_MINSUM && !BAIL) {  // BAIL: flood_drive has tested the flag
            if (__builtin_amdgcn_readfirstlane(*C.flag) != 0) {
                rows<DEC, true, (DIRECT ? kOutAny : -1)>(C, L, errs);
                return;
            }
        }
        if constexpr (!DIRECT)
            rows<DEC, false, -1>(C, L, errs);
        else if (C.out_dtype == LDPC_OUT_F32)
            rows<DEC, false, LDPC_OUT_F32>(C, L, errs);
        else
            rows<DEC, false, LDPC_OUT_U8>(C, L, errs);
    }

    template <bool DEC, bool SLOW, int OUT>
    __device__ __forceinline__ void rows(const Ctx &C, const Lane &L, int &errs) {
        float va[MAXDC], vb[MAXDC];
        const DecOutFor<G, OUT> D(C, L);
        addtid_begin(C.lds);
        const float ninf = opaque_sf(-INFINITY), pinf = opaque_sf(INFINITY);
        const uint32_t sgn = opaque_vu(0x80000000u);
        const float alv = opaque_vf(C.alpha);
        load_row<0>(C, L, va);
        sfor<P::NR>([&](auto i) {
            constexpr int I = decltype(i)::value;
            if constexpr (I % 2 == 0) {
                if constexpr (I + 1 < P::NR) load_row<I + 1>(C, L, vb);
                row<I, DEC, SLOW, OUT>(C, L, D, va, errs, ninf, pinf, sgn, alv);
            } else {
                if constexpr (I + 1 < P::NR) load_row<I + 1>(C, L, va);
                row<I, DEC, SLOW, OUT>(C, L, D, vb, errs, ninf, pinf, sgn, alv);
            }
        });
        addtid_end();
    }

    // ---- variable phase: tasks (column A, column B or none, every output of both), see
    // tools/gen_fixed_codes.py var_schedule.  Per output e of a column of degree D:
    //   v2c_e = P_e + c_{e+1} + ... + c_{D-1},  P_0 = llr, P_{J+1} = P_J + c_J
    // in this order (traditional_decoders.py:235-250: the sum over i' != i from llr in ascending
    // check order); the APP is P_D.  A pair runs both columns' chains in the two halves of
    // v_pk_add_f32 (two independent IEEE fp32 adds: each half is the scalar sequence, bit for bit)
    // while both have messages (J < DB); column A's remaining steps are scalar v_add_f32.
    template <int TK>
    struct Task {
        static constexpr int X = P::T0 + TK;
        static constexpr int CA = P::vt_a(X), CB = P::vt_b(X);
        static constexpr int PA = G::COL_PTR[CA], DA = G::COL_PTR[CA + 1] - PA;
        static constexpr int PB = CB >= 0 ? G::COL_PTR[CB] : 0, DB = CB >= 0 ? G::COL_PTR[CB + 1] - PB : 0;
        static_assert(DB <= DA, "pair tasks: A is the longer column");
        static constexpr int IA = P::col_index(CA), IB = CB >= 0 ? P::col_index(CB) : 0;
        static constexpr int NMSG = DA + DB;
        static_assert(IA >= 0 && IB >= 0, "a task's columns are columns of its wave");
    };
    struct TaskIn {
        f32x2 cp[MAXDV];  // J < DB: {c_A[J], c_B[J]}
        float cs[MAXDV];  // DB <= J < DA: c_A[J]
    };

    // the c2v of the edge at index X of COL_*: from msg[] (register edge: check k's output is in
    // this lane), from rmsg[] (rotated edge: check moved it here) or from its check-indexed slot,
    // read rotated
    template <int X>
    __device__ __forceinline__ float c2v_in() const {
        if constexpr (P::col_reg(X) >= 0)
            return msg[P::col_reg(X)];
        else if constexpr (P::col_rot(X) >= 0)
            return rmsg[P::col_rot(X)];
        else {
            static_assert(P::T.shidx[P::col_shift(X)] >= 0, "rot[] holds the rotation");
            return lds_rd_abs<G::COL_SLOT[X] * 256>(rot[P::T.shidx[P::col_shift(X)]]);
        }
    }
    // the v2c of that edge: into msg[], to its check lane's rmsg[], or own-lane into its slot, which turns variable-indexed
    // (ds_write_addtid_b32; every read of the slot was issued by load_task, before this store)
    template <int X>
    __device__ __forceinline__ void v2c_out(float o) {
        if constexpr (P::col_reg(X) >= 0)
            msg[P::col_reg(X)] = o;
        else if constexpr (P::col_rot(X) >= 0)
            rmsg[P::col_rot(X)] = to_chk_lane<P::col_shift(X)>(o);
        else
            lds_wr_tid<G::COL_SLOT[X] * 256>(o);
    }

    template <int TK>
    __device__ __forceinline__ void load_task(const Ctx &C, TaskIn &in) const {
        using K = Task<TK>;
        sfor<K::DA>([&](auto jj) {
            constexpr int J = decltype(jj)::value;
            if constexpr (J < K::DB) {
                in.cp[J].x = c2v_in<K::PA + J>();
                in.cp[J].y = c2v_in<K::PB + J>();
            } else {
                in.cs[J] = c2v_in<K::PA + J>();
            }
        });
    }

    template <int TK, bool DEC, bool WRITE, int OUT>
    __device__ __forceinline__ void task(const Ctx &C, const Lane &L, const DecOutFor<G, OUT> &D, const TaskIn &in, int &errs, bool &bad) {
        using K = Task<TK>;
        constexpr int DA = K::DA, DB = K::DB;
        f32x2 P2;
        float PA = cllr[K::IA];
        if constexpr (DB > 0) {
            P2.x = cllr[K::IA];
            P2.y = cllr[K::IB];
        }
        f32x2 acc2[DB > 0 ? DB : 1];
        float accA[DA];
        sfor<DA>([&](auto jj) {
            constexpr int J = decltype(jj)::value;  // outputs [0, J) take c_J
            if constexpr (J < DB) {
                sfor<J>([&](auto e) {
                    constexpr int E = decltype(e)::value;
                    acc2[E] = acc2[E] + in.cp[J];
                });
                acc2[J] = P2;
                P2 = P2 + in.cp[J];
                if constexpr (J == DB - 1) PA = P2.x;
            } else {
                sfor<J>([&](auto e) {
                    constexpr int E = decltype(e)::value;
                    if constexpr (E < DB)
                        acc2[E].x = acc2[E].x + in.cs[J];
                    else
                        accA[E] = accA[E] + in.cs[J];
                });
                accA[J] = PA;
                PA = PA + in.cs[J];
            }
        });
        if constexpr (WRITE) {
            sfor<DA>([&](auto e) {
                constexpr int E = decltype(e)::value;
                // the v2c of variable t goes to position t of its slot, or stays in msg[] (v2c_out)
                if constexpr (E < DB) {
                    v2c_out<K::PA + E>(acc2[E].x);
                    v2c_out<K::PB + E>(acc2[E].y);
                } else {
                    v2c_out<K::PA + E>(accA[E]);
                }
            });
        }
        // a NaN v2c implies a NaN or infinite APP of its column (every summand of a v2c is a
        // summand of the APP; +-inf is absorbing), so this flag bounds the fast check path.  A zero
        // v2c needs no flag: the fast forms give the reference's values up to the sign of a zero
        // (DESIGN.md 3.1 "Exactness of the fast path", tests/test_minsum_zeros_host.py)
        auto decide = [&](auto col, float app) {
            constexpr int COL = decltype(col)::value;
            const int bit = app < 0.0f;  // NaN < 0 is false -> 0 (traditional_decoders.py:252)
            if constexpr (OUT >= 0) D.template col<COL>(bit, errs);
            if (C.ballots) var_ballot(C, L, COL, bit);
        };
        if constexpr (ALGO == LDPC_ALGO_MINSUM) bad |= !(fabsf(PA) < INFINITY);
        if constexpr (DEC) decide(ic<K::CA>{}, PA);
        if constexpr (DB > 0) {
            if constexpr (ALGO == LDPC_ALGO_MINSUM) bad |= !(fabsf(P2.y) < INFINITY);
            if constexpr (DEC) decide(ic<K::CB>{}, P2.y);
        }
    }

    template <bool DEC, bool WRITE, bool DIRECT>
    __device__ __forceinline__ void var(const Ctx &C, const Lane &L, int &errs) {
        static_assert(DEC || !DIRECT, "stores need decisions");
        if constexpr (!DIRECT)
            var_as<DEC, WRITE, -1>(C, L, errs);
        else if (C.out_dtype == LDPC_OUT_F32)
            var_as<DEC, WRITE, LDPC_OUT_F32>(C, L, errs);
        else
            var_as<DEC, WRITE, LDPC_OUT_U8>(C, L, errs);
    }
    template <bool DEC, bool WRITE, int OUT>
    __device__ __forceinline__ void var_as(const Ctx &C, const Lane &L, int &errs) {
        bool bad = false;
        if constexpr (P::NT > 0) {
            const DecOutFor<G, OUT> D(C, L);
            // software pipelining: the next task's reads are issued before the current task's adds
            // when the two hold at most kVarPipe messages together (slots are disjoint between
            // tasks, so the reads never depend on the writes in flight).  A task's own reads are
            // all issued (load_task) before its first store: the stores land on positions that
            // other lanes of this wave read (header comment, "Slots").
            TaskIn ta, tb;
            if constexpr (WRITE) addtid_begin(C.lds);
            load_task<0>(C, ta);
            sfor<P::NT>([&](auto i) {
                constexpr int I = decltype(i)::value;
                constexpr bool more = I + 1 < P::NT;
                constexpr bool ahead = more && Task<I>::NMSG + Task<(more ? I + 1 : I)>::NMSG <= kVarPipe;
                if constexpr (I % 2 == 0) {
                    if constexpr (ahead) load_task<I + 1>(C, tb);
                    task<I, DEC, WRITE, OUT>(C, L, D, ta, errs, bad);
                    if constexpr (more && !ahead) load_task<(more ? I + 1 : I)>(C, tb);
                } else {
                    if constexpr (ahead) load_task<I + 1>(C, ta);
                    task<I, DEC, WRITE, OUT>(C, L, D, tb, errs, bad);
                    if constexpr (more && !ahead) load_task<(more ? I + 1 : I)>(C, ta);
                }
            });
            if constexpr (WRITE) addtid_end();
        }
        if constexpr (ALGO == LDPC_ALGO_MINSUM) {
            if (__any(bad) && L.lane == 0) *C.flag = 1;
        }
    }

    __device__ __forceinline__ int parity(const Ctx &C, const Lane &L) const {
        int inv = 0;
        // opaque copies: the per-edge bit positions are recomputed here (early-stop iterations
        // only) instead of being hoisted out of the loop into ~50 live registers
        int f = L.f, k = L.k;
        asm volatile("" : "+v"(f), "+v"(k));
        sfor<P::NR>([&](auto i) {
            constexpr int R = P::chk_row(decltype(i)::value);
            constexpr int P0 = G::ROW_PTR[R], DC = G::ROW_PTR[R + 1] - P0;
            int p = 0;  // parity of check r*Z + k of frame f: xor of its variables' decisions
            sfor<DC>([&](auto e) {
                constexpr int E = decltype(e)::value;
                constexpr int COL = G::ROW_COL[P0 + E], S = P::row_shift(P0 + E);
                p ^= (int)(C.words[COL] >> (f * G::Z + ((k + S) & (G::Z - 1))));
            });
            inv |= p;
        });
        return inv & 1;
    }
};

template <class G, class F>
__device__ __forceinline__ void fx_by_wave(int wave, F &&f) {
    static_assert(G::W == 4, "fixed schedules are generated for 4 waves");
    switch (wave) {
        case 0: f(ic<0>{}); break;
        case 1: f(ic<1>{}); break;
        case 2: f(ic<2>{}); break;
        default: f(ic<3>{}); break;
    }
}

}  // namespace

// 4 workgroups per CU without early stop (LDS: 159 slots x 256 B + 8 B each); the early-stop
// modes also keep Nb + 1 ballot words in LDS, which leaves room for 3, so they may use 168 VGPRs
// BAIL (min-sum, stopping off or per frame, redo != NULL): see FixedBody
template <class G, int ALGO, int ES, bool BAIL = false>
__global__ __launch_bounds__(256, ES == LDPC_ES_OFF ? 4 : 3) void flood_fixed_kernel(FloodTables T, const float *__restrict__ llr,
                                                          int64_t B, int max_iter, float alpha, int out_dtype,
                                                          void *__restrict__ bits, Outs O, EsWs W, uint32_t *redo) {
    static_assert(!BAIL || ES == LDPC_ES_OFF || ES == LDPC_ES_FRAME, "the batch-stop passes share state across workgroups");
    extern __shared__ __attribute__((aligned(16))) char lds[];
#ifdef LDPC_TIMELINE
    const uint64_t t_in = tl_now();
#endif
    // the code's dimensions are compile-time constants here: they need no SGPRs (the early-stop
    // instances spilled VGPRs to scratch with the kernel-argument copies)
    FloodTables Tc = T;
    Tc.Z = G::Z, Tc.FG = 64 / G::Z, Tc.Mb = G::Mb, Tc.Nb = G::Nb, Tc.N = G::N, Tc.nslots = G::NSLOTS, Tc.W = G::W;
    static_assert(G::Z < 64 && 64 % G::Z == 0, "rep1 below: a 1 at the bottom of every Z-bit segment");
    Tc.rep1 = ~0ull / ((1ull << G::Z) - 1ull);
    const Lane L = make_lane(Tc, llr, B);
    Ctx C;
    init_ctx(C, Tc, lds, alpha, out_dtype, bits);
    if constexpr (BAIL) C.redo = redo;
    fx_by_wave<G>(__builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), [&](auto wv) {
        FixedBody<G, ALGO, decltype(wv)::value, BAIL, reg_edge_cap<ES, BAIL>(), rot_edge_cap<ES, BAIL>(), reg_edges(ALGO), joint_family<G, ALGO, ES, BAIL>()> body;
        flood_drive<ES>(body, C, L, B, max_iter, O, W);
#ifdef LDPC_TIMELINE
        if constexpr (ES == LDPC_ES_OFF) tl_bracket(O.timeline, decltype(wv)::value, t_in);
#endif
    });
}

// The launcher declared in flood_host.hpp; flood_fixed_ms.hip and flood_fixed_bp.hip instantiate it
// for their ALGO.
template <int ALGO>
int launch_fixed(const FloodCall &c, int es, size_t lds, const Outs &O, const EsWs &W, uint32_t *redo) {
    auto pick = [&](auto code) -> const void * {
        using G = decltype(code);
        // with a redo list: the instances without the exact check update (they leave the decode
        // instead, launch_flood launches flood_redo_kernel behind them)
        if constexpr (ALGO == LDPC_ALGO_MINSUM) {
            if (redo && es == LDPC_ES_OFF) return reinterpret_cast<const void *>(flood_fixed_kernel<G, ALGO, LDPC_ES_OFF, true>);
            if (redo && es == LDPC_ES_FRAME) return reinterpret_cast<const void *>(flood_fixed_kernel<G, ALGO, LDPC_ES_FRAME, true>);
        }
        if (redo) return nullptr;
        switch (es) {
            case LDPC_ES_OFF: return reinterpret_cast<const void *>(flood_fixed_kernel<G, ALGO, LDPC_ES_OFF>);
            case LDPC_ES_FRAME: return reinterpret_cast<const void *>(flood_fixed_kernel<G, ALGO, LDPC_ES_FRAME>);
            case LDPC_ES_BATCH: return reinterpret_cast<const void *>(flood_fixed_kernel<G, ALGO, LDPC_ES_BATCH>);
            case ES_P1: return reinterpret_cast<const void *>(flood_fixed_kernel<G, ALGO, ES_P1>);
            case ES_P2: return reinterpret_cast<const void *>(flood_fixed_kernel<G, ALGO, ES_P2>);
            default: return nullptr;
        }
    };
    const int id = c.g->fixed_id;
    const void *kern = id == 1 ? pick(fixed::BG2_Z4{}) : (id == 2 ? pick(fixed::BG2_Z32{}) : nullptr);
    if (!kern) return fail(LDPC_EINVAL, "no fixed kernel for this code / stopping mode");
    LDPC_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    FloodCall a = c;
    FloodTables t = c.g->ft;
    Outs o = O;
    EsWs w = W;
    void *args[] = {&t, &a.llr, &a.B, &a.max_iter, &a.alpha, &a.out_dtype, &a.bits, &o, &w, &redo};
    const int64_t nwg = (c.B + c.g->FG - 1) / c.g->FG;
    LDPC_HIP(hipLaunchKernel(kern, dim3((unsigned)nwg), dim3(64 * c.g->ft.W), args, lds, c.s));
    return LDPC_OK;
}

}  // namespace ldpc
