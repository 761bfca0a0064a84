/*
 * ldpc_amd.h -- C ABI of the MI355X-native LDPC decoding library (libldpc_amd.so).
 *
 * The reference (BananaFalls/LDPC-NeuralNetwork-Decoder) is pure Python/PyTorch and has no
 * FFI of its own; its hot-path interface is the set of Python calls listed next to each entry
 * point below.  The Python package ldpc_neural_decoder (this repo) keeps those Python
 * signatures and binds these symbols with ctypes.
 *
 * Conventions
 *   - Every pointer named d_* is DEVICE memory owned by the caller (e.g. torch tensors on a HIP
 *     device, passed as data_ptr()).  Host pointers are named h_*.
 *   - Work is enqueued on `stream` (a hipStream_t, passed as void*; NULL = the legacy default
 *     stream) and is asynchronous unless stated otherwise.  No entry point allocates device
 *     memory on the decode path: scratch is caller-provided (query its size first).
 *   - Return value: 0 on success, a negative LDPC_E* code on error; the message of the last
 *     error on the calling thread is available from ldpc_last_error().
 *   - Layouts follow the reference: LLRs are float32 (B, N) row-major (utils/channel.py:90-154),
 *     hard decisions are (B, N) row-major, 0/1, either uint8 or float32
 *     (traditional_decoders.py:101,252 returns float32).
 */
#ifndef LDPC_AMD_H
#define LDPC_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    LDPC_OK = 0,
    LDPC_EINVAL = -1,       /* bad argument */
    LDPC_EHIP = -2,         /* HIP runtime error */
    LDPC_EUNSUPPORTED = -3, /* shape/degree outside what the kernels support */
    LDPC_ENOMEM = -4
};

enum {
    LDPC_ALGO_MINSUM = 0,
    LDPC_ALGO_BP = 1,
    LDPC_ALGO_LAYERED_MINSUM = 2,
    LDPC_ALGO_LAYERED_MINSUM_ANY = 3,
    LDPC_ALGO_MINSUM_F16 = 5, /* 4 is not assigned: it stays an unknown value (LDPC_EINVAL) */
    LDPC_ALGO_LAYERED_MINSUM_F16 = 6
};
enum { LDPC_ES_OFF = 0, LDPC_ES_BATCH = 1, LDPC_ES_FRAME = 2 };
enum { LDPC_OUT_U8 = 0, LDPC_OUT_F32 = 1 };

typedef struct ldpc_graph ldpc_graph; /* opaque: a Tanner graph resident on one device */

/* Last error message of the calling thread ("" if none). */
const char *ldpc_last_error(void);
/* Library version string. */
const char *ldpc_version(void);

/* ------------------------------------------------------------------ graph (setup, host-sync)
 * Replaces: the per-decoder Python setup loops
 *   traditional_decoders.py:26-40 / 161-175  (_precompute_indices over a dense H)
 *   message_gnn_decoder.py:382-488           (TannerToMessageGraph edge list + groups)
 * The edge list is check-major (checks ascending, vars ascending inside a check), i.e. the
 * order of TannerToMessageGraph.messages (message_gnn_decoder.py:397-406).  The library
 * detects quasi-cyclic structure (largest lifting Z <= 64 that H is block-circulant for) and
 * builds the per-wave schedules; a non-QC H is handled as Z = 1.
 * Tables are uploaded to the current HIP device; the call synchronizes. */
int ldpc_graph_create(int M, int N, int64_t E, const int32_t *h_edge_chk,
                      const int32_t *h_edge_var, ldpc_graph **out);
/* Base-graph form: replaces load_base_matrix + expand_base_matrix (ldpc_utils.py:97-147),
 * h_base is (mb, nb) int32 with -1 for a zero block; shifts are taken modulo z. */
int ldpc_graph_create_qc(const int32_t *h_base, int mb, int nb, int z, ldpc_graph **out);
int ldpc_graph_destroy(ldpc_graph *g);
/* M, N, E, detected lifting Z, max check degree, max variable degree. */
int ldpc_graph_info(const ldpc_graph *g, int *M, int *N, int64_t *E, int *Z, int *max_dc,
                    int *max_dv);
/* Kernel variant for this graph: 0 = auto (a compile-time schedule when the graph is one of the
 * reference's shipped codes, else table-driven), 1 = always table-driven.  Returns the variant
 * in use (0 table-driven, 1 BG2 Z=4, 2 BG2 Z=32) or a negative error. */
int ldpc_graph_set_variant(ldpc_graph *g, int variant);
/* Check-major edge list of the graph (E entries each) -- the reference's message order. */
int ldpc_graph_edges(const ldpc_graph *g, int32_t *h_edge_chk, int32_t *h_edge_var);

/* ------------------------------------------------------------------ flooding BP / min-sum
 * Replaces: MinSumScaledDecoder.decode  (traditional_decoders.py:177-260, alpha = scaling_factor)
 *           BeliefPropagationDecoder.decode (traditional_decoders.py:42-109, alpha ignored)
 * early_stop: LDPC_ES_OFF, LDPC_ES_BATCH (the reference's rule: stop at the first iteration at
 *   which ALL B frames satisfy H x = 0, traditional_decoders.py:104-107), LDPC_ES_FRAME
 *   (per-frame freeze at the first valid iteration; no reference counterpart).
 * d_llr     (B, N) float32
 * d_bits    (B, N) uint8 or float32 (out_dtype), 0/1, bit = (APP < 0)
 * d_iters   optional (B,) int32: iterations each frame ran (all equal unless LDPC_ES_FRAME)
 * d_batch_iters optional int32 scalar: the reference's returned `iterations`
 * d_counters optional uint64[4] += {bit errors vs the all-zero codeword, frame errors,
 *   frames, sum of per-frame iterations} -- the all-zero transmit of every reference harness
 *   (comparative_evaluation.py:133); counting is fused into the decoder's epilogue.
 * d_work / work_bytes: scratch of ldpc_flood_workspace_size(...) bytes, required for
 *   LDPC_ES_BATCH and whenever d_counters (or d_batch_iters with LDPC_ES_FRAME) is given: the
 *   counters are reduced through per-workgroup rows, not same-address atomics.  Give it always
 *   where speed matters: with it, min-sum on the reference's two codes (LDPC_ES_OFF / LDPC_ES_FRAME)
 *   runs a kernel that holds the fast check update only; a group of frames that meets a NaN or an
 *   infinity leaves that kernel, is listed in the workspace and is decoded again by the exact
 *   table-driven kernel in a second launch on the same stream (same results, no host round trip).
 * LDPC_ES_BATCH runs as passes on the stream (first all-valid iteration per workgroup, then the
 *   batch's candidate T, then -- only if some frame is invalid at T -- the exhaustive search);
 *   it never synchronises with the host.
 *
 * Layered min-sum (algo LDPC_ALGO_LAYERED_MINSUM; no reference counterpart, this text is its
 * definition).  Row-serial scaled min-sum on the Tanner graph, all arithmetic float32 without fused
 * multiply-add.  Per frame: app[v] = llr[v]; c2v[e] = +0 for every edge (check-major order).  One
 * iteration visits the checks in ascending index; for check i with variables j_0 < ... < j_{d-1}:
 *   1. t_k = app[j_k] - c2v[i,k]; for a variable of degree 1, t_k = llr[j_k] exactly (the flooding
 *      decoders' rule that a degree-1 variable's v2c is the channel LLR forever);
 *   2. c2v[i,k] = (prod_{q != k} sgn(t_q)) * (alpha * min_{q != k} |t_q|): the flooding min-sum
 *      check rule, sgn(0) = sgn(NaN) = 0, the min starts at +inf and a NaN never wins it, the
 *      product of signs is formed first and multiplied by alpha * min;
 *   3. app[j_k] = t_k + c2v[i,k] (a degree-1 variable: llr + c2v, used for the decision only).
 * After each full iteration bit[v] = (app[v] < 0).  The result depends on the graph alone, not on
 * the lifting the library detects (the Z checks of a block row touch disjoint variables, so the
 * kernel updates them at once).
 * early_stop: LDPC_ES_OFF (every frame runs max_iter) or LDPC_ES_FRAME (a frame freezes at the
 *   first iteration whose decisions satisfy H x = 0, with that iteration's bits and count, else
 *   runs max_iter; d_batch_iters = the largest per-frame count).  LDPC_ES_BATCH exists to mirror
 *   the reference's flooding classes: with this algo it is LDPC_EINVAL.
 * LDS-resident only: a graph that the flooding algos decode on the streaming kernels (lifting not
 *   a divisor of 64, LDS need above a CU's, or LDPC_FLOOD_STREAM set) is LDPC_EUNSUPPORTED.
 * d_work: ldpc_flood_workspace_size of the same arguments suffices, when required as above.
 * Non-finite LLRs: the call returns and every output is 0 or 1; the outputs of a frame holding a
 *   NaN or an infinity are otherwise unspecified, the other frames of the batch are unaffected.
 *
 * Layered min-sum on any graph (algo LDPC_ALGO_LAYERED_MINSUM_ANY).  The same algorithm, word for word:
 * the "Layered min-sum" text above is its definition, and d_bits, d_iters, d_batch_iters and d_counters
 * mean the same.  LDPC_ES_BATCH is LDPC_EINVAL here too.  What differs is where it runs:
 *   - on a graph that the flooding algos decode LDS-resident (and LDPC_FLOOD_STREAM unset) it is
 *     LDPC_ALGO_LAYERED_MINSUM itself: the same kernels, the same d_work rule, and the same
 *     LDPC_EUNSUPPORTED if the layered schedule (posteriors and messages of a wave's frames) does not fit
 *     a CU's LDS while the flooding one does;
 *   - on a graph that the flooding algos decode on the streaming kernels (lifting not a divisor of 64,
 *     LDS need above a CU's, or LDPC_FLOOD_STREAM set) it runs streaming kernels of its own: posteriors
 *     and messages in d_work, the checks cut into runs (ldpc_layered_runs below) and one launch per run
 *     and check degree, per iteration.  Same results as the LDS-resident kernels, bit for bit.  A
 *     check or variable degree above 32 is LDPC_EUNSUPPORTED, as for the streaming flooding decoders.
 * d_work: ldpc_flood_workspace_size of the same arguments suffices; on the streaming path it is
 *   required (LDPC_EINVAL without it), as for the streaming flooding decoders.
 * Non-finite LLRs: the call returns and every output is 0 or 1; the outputs of a frame holding a
 *   NaN or an infinity are otherwise unspecified, the other frames of the batch are unaffected.
 *
 * Half-precision min-sum (algo LDPC_ALGO_MINSUM_F16 = 5; no reference counterpart, this text is its
 * definition).  Flooding scaled min-sum on the Tanner graph.  Every value is IEEE binary16.  Every
 * operation is rounded to nearest-even with gradual underflow.  No multiply-add is fused.  C = 1024 is
 * the clamp.
 *   Channel.   x[v] = clamp(half(llr[v]), -C, +C).  half() is the float32 -> binary16 conversion,
 *              round-to-nearest-even.  A magnitude that rounds to infinity becomes +-C.  An infinite
 *              LLR is therefore a defined input.
 *   Scaling.   a = half(alpha).  Require 0 <= a <= 1, else LDPC_EINVAL.
 *   Init.      v2c[e] = x[var(e)].
 *   Check i with variables j_0 < ... < j_{d-1}:
 *              c2v[i,k] = (prod_{q != k} sgn v2c[i,q]) * (a * min_{q != k} |v2c[i,q]|).
 *              sgn(0) = 0.  The product of signs is formed first.  a * min is rounded once to binary16.
 *   Variable j with checks i_0 < ... < i_{dv-1}:
 *              v2c[i_k, j] = clamp(x[j] + sum_{q != k} c2v[i_q, j], -C, +C).  The sum is taken left to
 *              right in ascending q, starting from x[j].  Each add is rounded.  A degree-1 variable's
 *              v2c is x[j] forever.
 *   Posterior. app[j] = x[j] + sum_q c2v[i_q, j], in the same order, unclamped.  bit[j] = (app[j] < 0).
 * With a <= 1 and variable degree <= 32, no partial sum exceeds 33 * 1024 = 33 792 < 65 504.  Nothing
 * ever overflows, so there is no bail-out and no redo path (ldpc_flood_redo_count: LDPC_EUNSUPPORTED).
 *   - A variable degree above 32 is LDPC_EUNSUPPORTED.
 *   - The sign of a zero is not part of the contract.  A row containing a zero has minimum 0, so
 *     c2v = +-0, and `<` cannot tell the two zeros apart.  Decisions and iteration counts are defined,
 *     message bits are not.
 *   - NaN LLR.  That frame's outputs are 0 or 1 and otherwise unspecified.  Every other frame is
 *     unaffected, the frame sharing its lanes included (the kernel packs two frames per lane).
 *   - Early stop.  LDPC_ES_OFF and LDPC_ES_FRAME behave as for LDPC_ALGO_MINSUM: a frame freezes at the
 *     first iteration whose decisions satisfy H x = 0, with that iteration's bits and count.
 *     LDPC_ES_BATCH is LDPC_EINVAL, as for the layered algorithm.
 *   - Graphs.  LDS-resident only.  A graph the flooding algorithms send to the streaming kernels is
 *     LDPC_EUNSUPPORTED.  That covers a lifting that does not divide 64, an LDS need above a CU's
 *     (here nslots * 256 + 8 + 2 * (Nb + 1) * 8 bytes), and LDPC_FLOOD_STREAM set.
 *   - Outputs.  d_llr stays float32 (B, N).  d_bits, d_iters, d_batch_iters and d_counters mean what
 *     they mean for LDPC_ALGO_MINSUM.
 *   - Workspace.  ldpc_flood_workspace_size of the same arguments suffices.  It is required under the
 *     same conditions as for LDPC_ALGO_MINSUM.
 *   - ldpc_graph_set_variant has no effect on it: there is no compile-time schedule.
 *
 * Half-precision layered min-sum (algo LDPC_ALGO_LAYERED_MINSUM_F16 = 6; no reference counterpart, this
 * text is its definition).  Row-serial scaled min-sum on the Tanner graph.  Every value is IEEE binary16.
 * Every operation is rounded to nearest-even with gradual underflow.  No multiply-add is fused.  C = 1024
 * is the clamp.
 *   Channel.   x[v] = clamp(half(llr[v]), -C, +C), as for LDPC_ALGO_MINSUM_F16: a magnitude that rounds to
 *              infinity becomes +-C, so an infinite LLR is a defined input.
 *   Scaling.   a = half(alpha).  Require 0 <= a <= 1, else LDPC_EINVAL.
 *   Init.      app[v] = x[v].  c2v[e] = +0 for every edge (check-major order).
 *   One iteration visits the checks in ascending index.  For check i with variables j_0 < ... < j_{d-1}:
 *     1. t_k = clamp(app[j_k] - c2v[i,k], -C, +C).  For a variable of degree 1, t_k = x[j_k] exactly.
 *     2. c2v[i,k] = (prod_{q != k} sgn t_q) * (a * min_{q != k} |t_q|).  sgn(0) = 0.  The product of signs
 *        is formed first.  a * min is rounded once to binary16.  The minimum starts at C, not at +inf:
 *        for d >= 2 that changes nothing, since every |t| <= C; a check of degree 1 therefore sends +a * C,
 *        and nothing is ever infinite.
 *     3. app[j_k] = t_k + c2v[i,k], unclamped.  For a degree-1 variable it is x + c2v, used for the
 *        decision only.
 *   Decision.  After each full iteration bit[v] = (app[v] < 0).
 * |c2v| <= C and |t| <= C, so |app| <= 2 048 and |app - c2v| <= 3 072 < 65 504.  Nothing overflows, so
 * there is no bail-out and no redo path (ldpc_flood_redo_count: LDPC_EUNSUPPORTED).
 *   - The sign of a zero is not part of the contract.  `<`, abs and sgn cannot tell the two zeros apart,
 *     and x + (+-0) differs only when x is itself a zero.  Decisions and iteration counts are defined,
 *     message bits are not.
 *   - NaN LLR.  That frame's outputs are 0 or 1 and otherwise unspecified.  Every other frame is
 *     unaffected, the frame sharing its lanes included (the kernel packs two frames per lane).
 *   - Early stop.  LDPC_ES_OFF and LDPC_ES_FRAME behave as for the other layered algorithms.
 *     LDPC_ES_BATCH is LDPC_EINVAL.
 *   - Graphs.  Every graph runs on streaming kernels of this algorithm's own, whatever lifting the library
 *     detects.  LDPC_FLOOD_STREAM and ldpc_graph_set_variant have no effect.  A check or variable degree
 *     above 32 is LDPC_EUNSUPPORTED.
 *   - Outputs.  d_llr stays float32 (B, N).  d_bits, d_iters, d_batch_iters and d_counters mean what
 *     they mean for the other layered algorithms.
 *   - Workspace.  d_work of at least ldpc_layered_half_workspace_size(...) bytes is required, always:
 *     posteriors and messages live there.  A missing or short one is LDPC_EINVAL.
 *     ldpc_flood_workspace_size has no algo argument and sizes something else on an LDS-resident graph.
 *     The query returns 0 for B = 0 or max_iter = 0, and LDPC_EINVAL for bad arguments. */
int64_t ldpc_layered_half_workspace_size(const ldpc_graph *g, int64_t B, int max_iter, int early_stop);
int64_t ldpc_flood_workspace_size(const ldpc_graph *g, int64_t B, int max_iter, int early_stop);
int ldpc_flood_decode(const ldpc_graph *g, int algo, const float *d_llr, int64_t B, int max_iter,
                      float alpha, int early_stop, int out_dtype, void *d_bits, int32_t *d_iters,
                      int32_t *d_batch_iters, uint64_t *d_counters, void *d_work,
                      int64_t work_bytes, void *stream);
/* The layers of the streaming layered decoder, as host words (for unit tests; no device is touched).  The
 * arguments of ldpc_graph_create, then a buffer of `capacity` 32-bit words.  Returns the words needed (or a
 * negative error, as ldpc_graph_create would) and fills h_words when capacity holds them (h_words may be
 * NULL to ask for the size).  A run is a maximal stretch of consecutive checks, in ascending index, whose
 * variable sets are pairwise disjoint, built greedily: check i joins the current run unless one of its
 * variables is already in it, and then opens the next.  Layout:
 *   n_runs, n_seg
 *   run_ptr[n_runs + 1]  check indices: run r is the checks run_ptr[r] .. run_ptr[r + 1] - 1
 *   seg[n_seg][4]        {run, degree, offset into order, count}: runs ascending, degrees ascending inside
 *                        a run (a check without edges: a degree-0 segment, which launches nothing)
 *   order[M]             check indices, ascending inside a segment */
int64_t ldpc_layered_runs(int M, int N, int64_t E, const int32_t *h_edge_chk, const int32_t *h_edge_var,
                          int32_t *h_words, int64_t capacity);
/* How many frame groups (64 / Z frames each: group i holds frames i * 64 / Z ..) the last
 * ldpc_flood_decode with these arguments and this d_work decoded a second time (see d_work above),
 * and, when h_groups is given (room for ceil(B / (64 / Z)) entries), which, in no particular order.
 * Synchronises the stream.  LDPC_EUNSUPPORTED for a decode that keeps no such list. */
int ldpc_flood_redo_count(const ldpc_graph *g, int algo, int64_t B, int max_iter, int early_stop,
                          const void *d_work, void *stream, int32_t *h_count, int32_t *h_groups);
/* The sum-product decoders' own float32 functions, element by element (for unit tests):
 * d_tanh_half[i] = tanh(d_x[i] / 2) and d_two_atanh[i] = 2 atanh(d_x[i]) exactly as the check
 * update evaluates them.  Either output may be NULL. */
int ldpc_bp_math_raw(const float *d_x, int64_t n, float *d_tanh_half, float *d_two_atanh,
                     void *stream);

/* ------------------------------------------------------------------ hybrid min-sum
 * Replaces: CustomMinSumMessageGNNDecoder.forward (models/message_gnn_decoder.py:1167-1251) with
 * CustomVariableMessageGNNLayer.variable_layer_update (:611-670) and
 * CustomCheckMessageGNNLayer.check_layer_update (:976-1044).  The reference cannot run these
 * (SURVEY.md section 0); the semantics this build defines from them (total-minus-own variable update,
 * damping 0.5 with the incoming c2v from the second iteration on, unscaled min-sum check update,
 * probs = sigmoid(llr + sum of c2v)) are spelled out in csrc/flood.hip and DESIGN.md.
 * d_llr (B, N) float32 -> d_probs (B, N) float32.  No early stop (the reference has none).
 * d_work: ldpc_custom_minsum_workspace_size(g, B) bytes.  B <= 4194240 per call. */
int64_t ldpc_custom_minsum_workspace_size(const ldpc_graph *g, int64_t B);
int ldpc_custom_minsum_decode(const ldpc_graph *g, const float *d_llr, int64_t B, int iterations,
                              float *d_probs, void *d_work, int64_t work_bytes, void *stream);

/* ------------------------------------------------------------------ channel
 * Replaces: qpsk_modulate -> awgn_channel -> qpsk_demodulate (utils/channel.py:4-154) fused:
 *   s = 1/sqrt2 - b*sqrt2 (I = even bits, Q = odd bits), n ~ N(0, (1/snr)/2) per component,
 *   llr = 2*(s+n) / (1/snr), all in float32 as the reference rounds them.
 * Noise comes from Philox-4x32-10 keyed by `seed`, counter = (frame_offset + b, symbol), so a
 * frame's LLRs depend only on (seed, its global frame index, snr): ranks of a sharded sweep
 * draw disjoint streams by passing disjoint frame_offset.
 * d_bits optional (B, N) uint8 transmitted bits (NULL = the all-zero codeword).
 * bpsk != 0 selects AWGNChannel.transmit instead (utils/channel.py:193-232). */
int ldpc_awgn_llr(uint64_t seed, uint64_t frame_offset, float snr_db, const uint8_t *d_bits,
                  int64_t B, int N, int bpsk, float *d_llr, void *stream);
/* Raw Philox-4x32-10 stream (for known-answer tests): out[4*i + j] = word j of block
 * (counter = {i lo, i hi, ctr2, ctr3}, key = seed). */
int ldpc_philox_raw(uint64_t seed, uint32_t ctr2, uint32_t ctr3, int64_t n_blocks,
                    uint32_t *d_out, void *stream);

/* ------------------------------------------------------------------ BER / FER
 * Replaces: compute_ber_fer (utils/channel.py:156-190) as integer counts:
 * d_counters uint64[3] += {bit errors, frame errors, frames}.  d_ref NULL = all-zero codeword.
 * bits_dtype: LDPC_OUT_U8 / LDPC_OUT_F32 (a decision is "1" iff the value != 0). */
int ldpc_count_errors(const void *d_bits, int bits_dtype, const uint8_t *d_ref, int64_t B, int N,
                      uint64_t *d_counters, void *stream);

/* ------------------------------------------------------------------ message-centred GNN
 * Replaces: MessageGNNDecoder.forward (message_gnn_decoder.py:190-317) with its
 *           MessageGNNLayer.forward (:51-129) and decode_messages (:131-152).
 * The reference aggregates with dense normalized adjacencies D^-1/2 (A+I) D^-1/2 over the
 * messages that share a variable / a check (:410-469); those are group means.  A plan holds
 * the two groupings (message -> variable group, message -> check group) and the kernels
 * compute segment means, O(E*H) instead of the reference's O(E^2*H) bmm.
 *
 * Weights: one contiguous float32 blob (H = hidden, T = message types, L = layers):
 *   w_in[H], b_in[H]                                  input_embedding (Linear(1,H))
 *   per layer l: emb[T*H]                             message_type_embeddings
 *                w1v[H*2H] b1v[H] w2v[H*H] b2v[H]     var_to_check_update.{0,2}
 *                w1c[H*2H] b1c[H] w2c[H*H] b2c[H]     check_to_var_update.{0,2}
 *                wo[H] bo[1]                          output_projection
 * (nn.Linear weights as stored: (out, in) row-major; ldpc_gnn_weights_size gives the count.)
 * d_msg_type (E,) int32 already padded/truncated/clamped to [0,T) (the Python layer does
 *   :68-81).  d_msg_var (E,) int32 message -> variable for the LLR gather and the output sum
 *   (the reference's message_to_var_mapping, or its column-0 quirk: :218-229 / :285-295).
 * precision: 0 = float32 features and fp32-accurate products (H = 64: scaled two-term f16 splits on
 *   the f16 MFMA, each weight matrix group under one power-of-two scale; H = 96..256: the same splits
 *   per weight slice; other widths: fp32 fma chains); 1 = bf16 MLP operands, fp32 accumulate.
 * d_probs (B, N) float32 = sigmoid(llr + sum of each variable's projected messages).
 * d_work: at least ldpc_gnn_workspace_size(plan, H, N, B, precision) bytes. */
typedef struct ldpc_gnn_plan ldpc_gnn_plan;
/* flags of ldpc_gnn_forward_ex (and, FP32_PRODUCTS, of the training and hybrid _ex entries) */
#define LDPC_GNN_EARLY_STOP 1 /* cfg5 per-frame early termination (bf16 path; see below) */
#define LDPC_GNN_FP32_PRODUCTS 2 /* fp32 path, H = 64: every product on the fp32 MFMA (see below) */
#define LDPC_GNN_CHECK_RANGE 4   /* training forward: decide FP32_PRODUCTS from the weights, on the device */
int ldpc_gnn_plan_create(int64_t E, int n_vgroups, const int32_t *h_vgroup, int n_cgroups,
                         const int32_t *h_cgroup, ldpc_gnn_plan **out);
/* General adjacencies: the reference runs a dense bmm with whatever (E x E) matrices it is given
 * (message_gnn_decoder.py:106-118), after zero-padding / cropping them to E (:93-104).  A CSR plan
 * takes each side as a CSR matrix (row m: the columns j with A[m][j] != 0, ascending, and the
 * values; h_*_ptr has E + 1 entries): every message then aggregates sum_j A[m][j] c[j] over its
 * own row.  fp32 forward only (precision 0); the bf16 path and training need a group plan. */
int ldpc_gnn_plan_create_csr(int64_t E, const int32_t *h_v_ptr, const int32_t *h_v_col, const float *h_v_val,
                             const int32_t *h_c_ptr, const int32_t *h_c_col, const float *h_c_val,
                             ldpc_gnn_plan **out);
int ldpc_gnn_plan_destroy(ldpc_gnn_plan *p);
/* The tables a plan uploads, as host words (for unit tests; no device is touched).  The arguments of
 * ldpc_gnn_plan_create / _create_csr, then a buffer of `capacity` 32-bit words.  Returns the words
 * needed (or a negative error, as the create call would) and fills h_words when capacity holds them
 * (h_words may be NULL to ask for the size).  Layout: the counts, one length per section, then the
 * sections in the order the plan uploads them; float tables are stored as their bits.
 * ldpc_gnn_plan_tables: 12 counts n_gtiles, n_gtiles_v1, n_gtiles_v, n_ptiles, n_ptiles_v,
 *   n_ptiles_v1, n_mtiles, n_mtiles_v1, n_ctiles, ct_aligned, n_rw, rw_d1; 17 sections vgroup,
 *   cgroup, vg_ptr, vg_mem, cg_ptr, cg_mem, inv (inv_v | inv_c), gt_meta, gt_grp, gt_mem, pt_meta,
 *   pt_grp, pt_deg, pt_mem, mt_perm, ct_m0, rw_meta (csrc/gnn.hpp documents each).
 * ldpc_gnn_plan_tables_csr: 3 counts E, nnz of the var side, nnz of the check side; 5 sections
 *   tab (vgroup cgroup vg_ptr vg_mem cg_ptr cg_mem), inv, w (vg_w cg_w 0), tt (vt_ptr vt_mem ct_ptr
 *   ct_mem: the transposes), tw (vt_w ct_w 0). */
int64_t ldpc_gnn_plan_tables(int64_t E, int n_vgroups, const int32_t *h_vgroup, int n_cgroups,
                             const int32_t *h_cgroup, int32_t *h_words, int64_t capacity);
int64_t ldpc_gnn_plan_tables_csr(int64_t E, const int32_t *h_v_ptr, const int32_t *h_v_col, const float *h_v_val,
                                 const int32_t *h_c_ptr, const int32_t *h_c_col, const float *h_c_val,
                                 int32_t *h_words, int64_t capacity);
/* Hybrid GNN (CustomVariableMessageGNNDecoder.forward, models/message_gnn_decoder.py:798-879 with
 * CustomVariableMessageGNNLayer.forward :672-755).  The reference cannot run it;
 * the semantics this build defines (check-side MLP + the layer's own output head, min-sum variable
 * update on those LLRs with damping 0.5, the decoder's Linear(1, H) back to features, mean-normalised
 * output) are spelled out in csrc/gnn.hip and DESIGN.md.  hidden must be 64; group plans only.
 * Weights: the ldpc_gnn_forward blob.  d_probs (B, N). */
int64_t ldpc_gnn_custom_var_workspace_size(const ldpc_gnn_plan *p, int hidden, int N, int64_t B, int layers);
int ldpc_gnn_custom_var_forward(const ldpc_gnn_plan *p, int hidden, int types, int layers,
                                const float *d_weights, const int32_t *d_msg_type,
                                const int32_t *d_msg_var, const float *d_llr, int N, int64_t B,
                                float *d_probs, void *d_work, int64_t work_bytes, void *stream);
/* ldpc_gnn_custom_var_forward_ex: ... plus flags.  LDPC_GNN_FP32_PRODUCTS (hidden 64): the check side's
 * products on the fp32 MFMA instead of as f16 splits, for weights beyond the splits' range (see
 * ldpc_gnn_forward_ex); other widths run fp32 fma chains either way. */
int ldpc_gnn_custom_var_forward_ex(const ldpc_gnn_plan *p, int hidden, int types, int layers,
                                   const float *d_weights, const int32_t *d_msg_type,
                                   const int32_t *d_msg_var, const float *d_llr, int N, int64_t B, int flags,
                                   float *d_probs, void *d_work, int64_t work_bytes, void *stream);
int64_t ldpc_gnn_weights_size(int hidden, int types, int layers);
/* Whether a weight blob is beyond the f16 splits' range: *d_exceeded (device int32) = 1 when, in some
 * layer, a nonzero row of a weight group has its largest |w| below `range` (2^-17) times the group's
 * largest, else 0.  The groups are those that share one power-of-two scale: hidden 64, the projection's
 * W1v / W1c right halves, and the MLP's left halves, W2v, W2c and W1v_left + W1v_right; hidden 96..256,
 * each side's W1 right half, both left halves together, and W2v | W2c row by row.  Other widths have no
 * splits (always 0).  One launch, no synchronisation.  (The training forward asks the same question
 * itself under LDPC_GNN_CHECK_RANGE.) */
int ldpc_gnn_split_range_exceeded(int hidden, int types, int layers, const float *d_weights, float range,
                                  int32_t *d_exceeded, void *stream);
int64_t ldpc_gnn_workspace_size(const ldpc_gnn_plan *p, int hidden, int N, int64_t B, int layers,
                                int precision);
int ldpc_gnn_forward(const ldpc_gnn_plan *p, int hidden, int types, int layers,
                     const float *d_weights, const int32_t *d_msg_type, const int32_t *d_msg_var,
                     const float *d_llr, int N, int64_t B, int precision, float *d_probs,
                     void *d_work, int64_t work_bytes, void *stream);

/* ldpc_gnn_forward_ex: ldpc_gnn_forward plus flags and a per-frame layer count d_iters (B,) int32
 * (optional).  LDPC_GNN_EARLY_STOP (precision 1 only; a feature with no reference counterpart,
 * BASELINE cfg5): after every layer but the last, each frame still decoding takes the hard
 * decision [llr + sum of the LAST layer's output_projection over its messages > 0] on its current
 * features; a frame whose decision satisfies every parity check stops there, gets its probs from
 * that decision's soft values and d_iters = layers used; the others run on.
 * LDPC_GNN_FP32_PRODUCTS (precision 0): the products of W1_right g and of the MLP run on the fp32 MFMA
 * (H = 64) or as three-term bf16 splits (H = 96..256) instead of as scaled two-term f16 splits.  The
 * splits hold 22 bits of every weight whose row's largest |w| is at least 2^-17 of its matrix group's; a
 * caller whose weights span more (MessageGNNDecoder checks this per weight version) sets the flag to
 * keep fp32 accuracy. */
int ldpc_gnn_forward_ex(const ldpc_gnn_plan *p, int hidden, int types, int layers,
                        const float *d_weights, const int32_t *d_msg_type, const int32_t *d_msg_var,
                        const float *d_llr, int N, int64_t B, int precision, int flags, float *d_probs,
                        int32_t *d_iters, void *d_work, int64_t work_bytes, void *stream);

/* ---- training (fp32, hidden_dim <= 1024, any plan) ---------------------------------------------
 * Replaces torch autograd through MessageGNNDecoder.forward + F.binary_cross_entropy
 * (message_gnn_decoder.py:190-317, :314), as driven by trainer.py:70-102 (zero_grad, forward,
 * loss.backward(), SGD step).
 * ldpc_gnn_forward_train: the fp32 forward (same arguments as ldpc_gnn_forward, precision 0) that
 *   also writes every layer's output features to d_saved (L, B, E, H) float32.
 * ldpc_gnn_backward: given d_grad_probs = dLoss/dprobs (B, N), writes dLoss/dweights into
 *   d_grad_weights, laid out exactly like the weight blob (zeroed first).  The output_projection of
 *   every layer but the last gets zeros (the reference's forward never uses it: its grad is None).
 * Both take a workspace of ldpc_gnn_train_workspace_size(...) bytes. */
int64_t ldpc_gnn_train_workspace_size(const ldpc_gnn_plan *p, int hidden, int N, int64_t B, int layers);
int ldpc_gnn_forward_train(const ldpc_gnn_plan *p, int hidden, int types, int layers,
                           const float *d_weights, const int32_t *d_msg_type, const int32_t *d_msg_var,
                           const float *d_llr, int N, int64_t B, float *d_probs, float *d_saved,
                           void *d_work, int64_t work_bytes, void *stream);
int ldpc_gnn_backward(const ldpc_gnn_plan *p, int hidden, int types, int layers, const float *d_weights,
                      const int32_t *d_msg_type, const int32_t *d_msg_var, const float *d_llr, int N,
                      int64_t B, const float *d_probs, const float *d_grad_probs, const float *d_saved,
                      float *d_grad_weights, void *d_work, int64_t work_bytes, void *stream);
/* Deep supervision (training extension, no reference counterpart; it is what makes the cfg5
 * per-frame early termination fire: the syndrome check decodes every layer's output through the
 * last layer's output_projection, so a model trained on the last layer's loss alone never yields a
 * codeword before the end).
 * ldpc_gnn_layer_probs: probs of every layer l < L - 1 through the LAST layer's output_projection,
 *   p_l[b][v] = sigmoid(llr + sum_{m -> v} (wo_L . x_{l+1}[b][m] + bo_L)) from d_saved, into
 *   d_layer_probs (L - 1, B, N); the output stage's own variable sums (ascending messages).
 *   Workspace: ldpc_gnn_train_workspace_size(...) bytes suffice.
 * ldpc_gnn_backward_ds: ldpc_gnn_backward plus dLoss/d(layer probs) (L - 1, B, N): each layer's
 *   head gradient is added to the feature gradient that arrives from above and to dwo_L / dbo_L.
 *   Both layer pointers null = ldpc_gnn_backward. */
int ldpc_gnn_layer_probs(const ldpc_gnn_plan *p, int hidden, int types, int layers, const float *d_weights,
                         const int32_t *d_msg_var, const float *d_llr, int N, int64_t B, const float *d_saved,
                         float *d_layer_probs, void *d_work, int64_t work_bytes, void *stream);
int ldpc_gnn_backward_ds(const ldpc_gnn_plan *p, int hidden, int types, int layers, const float *d_weights,
                         const int32_t *d_msg_type, const int32_t *d_msg_var, const float *d_llr, int N,
                         int64_t B, const float *d_probs, const float *d_grad_probs, const float *d_saved,
                         const float *d_layer_probs, const float *d_grad_layer_probs, float *d_grad_weights,
                         void *d_work, int64_t work_bytes, void *stream);
/* Saved projections (round 5): the forward keeps every layer's projected group rows W1_s,right g_s +
 * b1_s and group means g_s (the fp32 path's gnn_group_proj_kernel outputs) in d_proj, so that the
 * backward does not recompute them.  hidden_dim 64 with a group plan; elsewhere the area is 0 floats
 * and the _ex functions behave as the ones above.
 * ldpc_gnn_train_proj_floats: float32 elements of d_proj = L * B * (Gv + Gc) * 2 * H, laid out per
 *   layer as [Pv (B, Gv, H) | Pc (B, Gc, H) | gv (B, Gv, H) | gc (B, Gc, H)].
 * ldpc_gnn_forward_train_ex / ldpc_gnn_backward_ds_ex: ldpc_gnn_forward_train / ldpc_gnn_backward_ds
 *   with d_proj (null = recompute in the backward).  The backward only reads d_proj. */
int64_t ldpc_gnn_train_proj_floats(const ldpc_gnn_plan *p, int hidden, int64_t B, int layers);
int ldpc_gnn_forward_train_ex(const ldpc_gnn_plan *p, int hidden, int types, int layers,
                              const float *d_weights, const int32_t *d_msg_type, const int32_t *d_msg_var,
                              const float *d_llr, int N, int64_t B, float *d_probs, float *d_saved, float *d_proj,
                              void *d_work, int64_t work_bytes, void *stream);
int ldpc_gnn_backward_ds_ex(const ldpc_gnn_plan *p, int hidden, int types, int layers, const float *d_weights,
                            const int32_t *d_msg_type, const int32_t *d_msg_var, const float *d_llr, int N,
                            int64_t B, const float *d_probs, const float *d_grad_probs, const float *d_saved,
                            const float *d_proj, const float *d_layer_probs, const float *d_grad_layer_probs,
                            float *d_grad_weights, void *d_work, int64_t work_bytes, void *stream);
/* ldpc_gnn_forward_train_ex2 / ldpc_gnn_backward_ds_ex2: the _ex functions plus flags.
 *   LDPC_GNN_FP32_PRODUCTS (hidden 64, group plans): the training forward's products of W1_right g and of
 *   the MLP on the fp32 MFMA instead of as f16 splits, as ldpc_gnn_forward_ex does for inference, and
 *   the projections the backward recomputes (d_proj null) likewise; the backward's own MLP products are
 *   three-term bf16 splits or fp32 MFMAs, which hold fp32's range.  Other widths train on fp32 fma chains
 *   and ignore the flag.
 *   LDPC_GNN_CHECK_RANGE (forward): the forward itself decides FP32_PRODUCTS, by the rule of
 *   ldpc_gnn_split_range_exceeded with range 2^-17, for a trainer whose weights are new at every step.  It
 *   queues the check and its preparation, synchronises the stream once, and launches the layers; a stream
 *   under capture cannot take this flag.
 *   *flags_used (host, optional) receives the flags the forward ran with (FP32_PRODUCTS or 0): pass them
 *   to ldpc_gnn_backward_ds_ex2. */
int ldpc_gnn_forward_train_ex2(const ldpc_gnn_plan *p, int hidden, int types, int layers,
                               const float *d_weights, const int32_t *d_msg_type, const int32_t *d_msg_var,
                               const float *d_llr, int N, int64_t B, float *d_probs, float *d_saved, float *d_proj,
                               int flags, int *flags_used, void *d_work, int64_t work_bytes, void *stream);
int ldpc_gnn_backward_ds_ex2(const ldpc_gnn_plan *p, int hidden, int types, int layers, const float *d_weights,
                             const int32_t *d_msg_type, const int32_t *d_msg_var, const float *d_llr, int N,
                             int64_t B, const float *d_probs, const float *d_grad_probs, const float *d_saved,
                             const float *d_proj, const float *d_layer_probs, const float *d_grad_layer_probs,
                             float *d_grad_weights, int flags, void *d_work, int64_t work_bytes, void *stream);

/* ---- index-gather neural-BP layers (models/layers.py) ------------------
 * d_idx is the reference's (n_out, K) index tensor transposed to (K, n_out) int32, -1 = padding
 * (a zero value): d_idx[k * n_out + i]; inputs (B, n_in) fp32.
 * ldpc_gather_minsum   CheckLayer.forward (layers.py:14-66): out = prod sign(v + 1e-10) * min |v|
 *                      (|0| -> 1e10); d_argmin (B, n_out) int32 (optional) keeps torch.min's index.
 * ldpc_gather_sum      VariableLayer.forward (layers.py:78-125): out = llr + sum of gathered msgs
 *                      (d_llr NULL: out = the sum alone).  A row ends at its first -1: put the
 *                      padding last (for a sum, padding anywhere adds an exact +0.0).
 * ldpc_residual        ResidualLayer.forward (layers.py:143-168), h_prev = host array of `depth`
 *                      device pointers (depth <= 8).
 * ldpc_output_layer    OutputLayer.forward (layers.py:180-208): soft = sigmoid(final + llr); with
 *                      d_gt, max over n of the elementwise BCE (+ its argmax for the backward).
 * The *_backward entry points write torch autograd's input gradients of the same functions. */
int ldpc_gather_minsum(const float *d_in, int64_t B, int n_in, const int32_t *d_idx, int n_out, int K,
                       float *d_out, int32_t *d_argmin, void *stream);
/* ldpc_check_groups_minsum: the same CheckLayer outputs (no argmin) when the index is a set of
 * checks -- every edge's row holds exactly the other edges of its check (n_in == n_out == n), as
 * create_LLR_mapping builds it.  d_gptr (G + 1) / d_gmem (n) list each check's edges; K is the
 * index's row length (padding K > degree - 1 contributes the 1e10 of a zero entry). */
int ldpc_check_groups_minsum(const float *d_in, int64_t B, int n, const int32_t *d_gptr, const int32_t *d_gmem,
                             int G, int K, float *d_out, void *stream);
int ldpc_gather_minsum_backward(const float *d_grad_out, const float *d_in, int64_t B, int n_in,
                                const int32_t *d_idx, int n_out, int K, const int32_t *d_argmin,
                                float *d_grad_in, void *stream);
int ldpc_gather_sum(const float *d_llr, const float *d_msgs, int64_t B, int n_in, const int32_t *d_idx,
                    int n_out, int K, float *d_out, void *stream);
/* ldpc_var_groups_sum: the same VariableLayer outputs (layers.py:78-125) when the index is a set of
 * contiguous variable groups -- every edge's row holds exactly the other edges of its variable in
 * ascending order, and each variable's edges are a run [gptr[g], gptr[g + 1]) tiling [0, n)
 * (n_in == n_out == n), as create_LLR_mapping builds it.  Sums in the row's order, bit-identical
 * to ldpc_gather_sum.  d_out must not alias d_msgs or d_llr.  LDPC_EUNSUPPORTED when a row does
 * not fit LDS. */
int ldpc_var_groups_sum(const float *d_llr, const float *d_msgs, int64_t B, int n, const int32_t *d_gptr, int G,
                        float *d_out, void *stream);
int ldpc_gather_sum_backward(const float *d_grad_out, int64_t B, int n_in, const int32_t *d_idx, int n_out,
                             int K, float *d_grad_msgs, void *stream);
int ldpc_residual(const float *d_llr, const float *d_w_ch, const float *d_cm, const float *d_w_res,
                  const float *const *h_prev, int depth, int64_t B, int n, float *d_out, void *stream);
int ldpc_residual_backward(const float *d_grad, const float *d_llr, const float *d_w_ch,
                           const float *d_w_res, const float *const *h_prev, int depth, int64_t B, int n,
                           float *d_grad_llr, float *d_grad_w_ch, float *d_grad_w_res,
                           float *const *h_grad_prev, void *stream);
int ldpc_output_layer(const float *d_final, const float *d_llr, const float *d_gt, int64_t B, int n,
                      float *d_soft, float *d_max_loss, int32_t *d_argmax, void *stream);
int ldpc_output_layer_backward(const float *d_soft, const float *d_gt, const float *d_grad_soft,
                               const float *d_grad_loss, const int32_t *d_argmax, int64_t B, int n,
                               float *d_grad_z, void *stream);

/* ---- hybrid layers' per-message updates on index rows (message_gnn_decoder.py:611-670, :976-1044)
 * d_rows (R, W) int64 row-major: row m = [node, incoming message ids..., -1 padding]; ids index the
 * E_in columns of d_x / d_c2v (validated by the caller).  Outputs (B, R) fp32.
 * ldpc_index_rows_minsum  CustomCheckMessageGNNLayer.check_layer_update (:976-1044): the min-sum
 *                         update of the row's other entries, leaving out its last valid entry
 *                         (torch.sign / torch.min semantics; 0 without two valid entries).
 * ldpc_index_rows_varsum  CustomVariableMessageGNNLayer.variable_layer_update (:611-670):
 *                         (llr[b, node] + sum of the valid entries, ascending) - the last one;
 *                         llr[b, node] without valid entries; damp != 0 (iteration > 0):
 *                         0.5 * out + 0.5 * c2v[b, m] (needs R == E_in).  d_llr (B, N_var). */
int ldpc_index_rows_minsum(const float *d_x, int64_t B, int64_t E_in, const int64_t *d_rows, int64_t R, int W,
                           float *d_out, void *stream);
int ldpc_index_rows_varsum(const float *d_llr, int64_t B, int64_t N_var, const float *d_c2v, int64_t E_in,
                           const int64_t *d_rows, int64_t R, int W, int damp, float *d_out, void *stream);

/* ---- neural min-sum decoder, fused inference (LDPCNeuralDecoder.forward, models/decoder.py) ----
 * One kernel runs every iteration of a frame with its messages in LDS; HBM sees the LLRs, the weights
 * and the output.  The result is DEFINED as the operation sequence of LDPCNeuralDecoder.forward as the
 * layer kernels above evaluate it -- float32 throughout, no multiply-add fused, every sum in the stated
 * order -- so it equals the layer path's output bit for bit:
 *   x0[e]  = +0.0f + llr[var(e)]   (ldpc_gather_sum's sequence on a one-entry row: -0.0 becomes +0.0)
 *   v_{-1} = x0
 *   for l = 0 .. I - 1:
 *     c_l[e] = ldpc_check_groups_minsum's rule on v_{l-1}: prod sign(v + 1e-10f) * min |v|' over the
 *              other edges of e's check, |0| -> 1e10, the minimum capped at 1e10 when the check has
 *              padding (K > degree - 1), NaN if another edge is NaN, the sign of a zero product kept
 *              (the same device function, csrc/check_group.hpp, serves both paths)
 *     for l < I - 1:
 *       S[e]   = ldpc_var_groups_sum's sequence: start at +0.0f, add the c_l of the variable's other
 *                edges in ascending order, skipping e
 *       r      = x0[e] * w_ch_l[e];  r = r + S[e];
 *       r      = r + w_res_l[i] * v_{l-1-i}[e]   for i = 0 .. min(l, depth_L) - 1, in this order
 *       v_l[e] = r
 *   app[j] = +0.0f + the c_{I-1} of variable j's edges, ascending
 *   soft   = 1.0f / (1.0f + expf(-((-app) + (-llr))))      ldpc_output_layer on (-app, -llr)
 * Non-finite inputs propagate exactly as through the layers; frames are independent.
 *
 * Graph description: the var-major edge numbering of create_LLR_mapping in the group form of the layer
 * kernels.  h_cptr (G + 1) / h_cmem (E): each check's edges, ascending inside a check; h_vptr (N + 1):
 * variable j's edges are the run [vptr[j], vptr[j + 1]); K: the row length of the check index tensor.
 * ldpc_neural_plan_create validates on the host (cmem a permutation of 0 .. E - 1, cptr and vptr
 * monotone and tiling [0, E), E < 65536: else LDPC_EINVAL; LDPC_EUNSUPPORTED when no depth_L could
 * run, see below), uploads the 16-bit tables to the current device once, and synchronises.
 * ldpc_neural_layout touches no device: the same validation, then the kernel's frames per workgroup
 * (as many as fit beside the tables, at most 8), threads per workgroup and LDS bytes for depth_L (any
 * output may be NULL).  LDPC_EUNSUPPORTED when depth_L > 8, when N or G exceeds 65535, or when one
 * frame (the LLR row, one c row and max(depth_L, 1) v rows) does not fit 160 KB beside the tables.
 * ldpc_neural_forward decides through the same function, so the two cannot disagree.
 * ldpc_neural_forward: asynchronous on `stream`, no workspace, no allocation.  d_w_ch (I - 1, E) and
 * d_w_res (I - 1, depth_L) float32 row-major (iterations == 1: no variable layer, both may be NULL;
 * depth_L == 0: d_w_res may be NULL); d_llr (B, N) rows contiguous, any 4-byte-aligned base; at least
 * one of d_app (B, N) and d_soft (B, N) must be given.  iterations >= 1; B == 0 launches nothing. */
typedef struct ldpc_neural_plan ldpc_neural_plan;
int ldpc_neural_plan_create(int N, int G, int64_t E, const int32_t *h_cptr, const int32_t *h_cmem,
                            const int32_t *h_vptr, int K, ldpc_neural_plan **out);
int ldpc_neural_plan_destroy(ldpc_neural_plan *p);
int ldpc_neural_layout(int N, int G, int64_t E, const int32_t *h_cptr, const int32_t *h_cmem,
                       const int32_t *h_vptr, int K, int depth_L, int *frames, int *threads,
                       int64_t *lds_bytes);
int ldpc_neural_forward(const ldpc_neural_plan *p, int iterations, int depth_L, const float *d_w_ch,
                        const float *d_w_res, const float *d_llr, int64_t B, float *d_app, float *d_soft,
                        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_AMD_H */
