/*
 * nann_hip.h -- C ABI of libnann_hip.so: the MI355X (gfx950) implementation of
 * NANN's HNSW-with-model-scoring retrieval hot path.
 *
 * Every entry point replaces one piece of the reference's TensorFlow custom-op
 * path (citations relative to /root/reference/,
 * UO/ = tensorflow/tensorflow/core/user_ops/).  extern "C", POD arguments,
 * int status returns, no exceptions/STL/torch types across the boundary.
 * The op-kernel shims in nann_amd/tf_ops/ (REGISTER_OP / REGISTER_KERNEL_BUILDER
 * with the reference's op names) and the Python mirror in nann_amd/ops.py are
 * thin callers of this file.  INTEGRATION.md shows the binding a reference
 * maintainer would add.
 *
 * Memory convention: unless a parameter is marked [host], data pointers are
 * DEVICE pointers (HBM) valid on the library's current HIP device, and the
 * call is enqueued on `stream` (a hipStream_t passed as void*; NULL = the
 * default stream).  Calls that return a data-dependent count synchronise the
 * stream before returning (exactly where the reference must know the size to
 * allocate_output: GroupGather_kernel.cc:147-148, bitmap_ops.cc:245).
 * All entry points are thread-safe and re-entrant on shared immutable handles.
 */
#ifndef NANN_HIP_H_
#define NANN_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NANN_ABI_VERSION 6

/* status codes; 1..8 share the oracle's numbering (oracle/nann_oracle.h) and
 * map to the TF errors the reference raises at the cited lines */
enum nann_status {
  NANN_OK = 0,
  NANN_ERR_INVALID_RAGGED_PARAMS = 1,  /* InvalidArgument, GroupGather_kernel.cc:62-64 */
  NANN_ERR_INVALID_RAGGED_INDICES = 2, /* InvalidArgument, GroupGather_kernel.cc:65-67 */
  NANN_ERR_INVALID_RAGGED_INPUT = 3,   /* InvalidArgument, bitmap_ops.cc:182-184 */
  NANN_ERR_TOPK_K_GT_N = 4,            /* InvalidArgument, topk_op.cc:67-71 */
  NANN_ERR_INDEX_OUT_OF_RANGE = 5,     /* InvalidArgument, gather_op.cc:170-175; also the
                                          bounds checks the reference omits (UB there) */
  NANN_ERR_EMPTY_SCORE_BATCH = 6,      /* blaze_xla_predictor.cc:259-263 */
  NANN_ERR_BAD_ARGUMENT = 7,
  NANN_ERR_TOPK_SCALAR_INPUT = 8,      /* topk_op.cc:63-65 after Squeeze of one candidate */
  NANN_ERR_HIP = 100,                  /* a HIP runtime call failed (nann_last_error) */
  NANN_ERR_NO_DEVICE = 101,
  NANN_ERR_UNSUPPORTED = 102,
  NANN_ERR_CAPACITY = 103,             /* caller-provided output too small; count returned */
  NANN_ERR_IO = 104,                   /* HugeConst: file/npy header problems */
  NANN_ERR_DTYPE_MISMATCH = 105,       /* HugeConst: huge_const_op.cc:117-147 */
  NANN_ERR_SHAPE_MISMATCH = 106        /* HugeConst: huge_const_op.cc:111-115 */
};

enum nann_dtype { NANN_F16 = 0, NANN_BF16 = 1, NANN_F32 = 2, NANN_I32 = 3, NANN_I64 = 4,
                  NANN_F64 = 5 };
enum nann_scorer_kind { NANN_SCORER_L2 = 0, NANN_SCORER_MLP = 1, NANN_SCORER_IP = 2 };

typedef void* nann_stream_t; /* hipStream_t */

int nann_abi_version(void);
/* [host] NUL-terminated description of the calling thread's last failure */
const char* nann_last_error(void);
/* number of visible HIP devices (0 when there is no GPU; never fails) */
int nann_device_count(void);

/* ---- device memory plumbing for hosts without torch (the TF shims) -------- */
int nann_malloc(void** dev_ptr, int64_t nbytes);
int nann_free(void* dev_ptr);
/* kind: 0 host->device, 1 device->host, 2 device->device; async on stream */
int nann_memcpy(void* dst, const void* src, int64_t nbytes, int kind, nann_stream_t stream);
int nann_stream_synchronize(nann_stream_t stream);
/* a stream of the host's own (non-blocking with respect to the null stream) and page-locked staging memory: what a
 * multi-lane C++ host needs to overlap one batch's copies with another's search (csrc/host/nann_serve.cpp) */
int nann_stream_create(nann_stream_t* out);
int nann_stream_destroy(nann_stream_t stream);
int nann_host_malloc(void** host_ptr, int64_t nbytes);
int nann_host_free(void* host_ptr);

/* ---- a6: HugeConst (UO/huge_const_op/huge_const_op.cc:58-226) --------------
 * Loads a .npy (format 1.0/2.0, C order) into HBM once; the GPU kernel of the
 * reference op does the same one-time H2D copy (:187-218).  expect_dtype /
 * expect_shape mirror the op's dtype/shape attrs and are validated against
 * the header (:108-147); expect_shape may be NULL to accept the file's shape.
 * allow_cast != 0 reproduces the Python wrapper huge_constant()
 * (NANN_impls/nann/model/model_util.py:107-121), which casts the array to the
 * requested dtype (f32->f16, i64->i32, ...) -- here at load time, without
 * rewriting the file as the wrapper does.  *nbytes = bytes resident in HBM.
 * path [host]; expect_shape [host]. */
int nann_huge_const_load(const char* path, int expect_dtype, const int64_t* expect_shape,
                         int expect_rank, int allow_cast, void** dev_ptr, int64_t* nbytes);

/* ---- a1: GroupGather<int32>, unique=false (UO/beam_search_op/
 *          GroupGather_kernel.cc:55-173) -------------------------------------
 * Step 1 (count): validates both ragged inputs (codes 1/2/3 in *ragged_code
 * [host]), writes ret_row_splits (device, n_indices_splits entries, or [0] on
 * the void-input path), returns the number of values in *n_ret [host] and the
 * number of row_splits written in *n_ret_splits [host].
 * Step 2 (fill): writes ret_values (device, n_ret entries).  scratch_offsets
 * (device, int64[n_indices_values + 1]) carries the per-row output offsets
 * from step 1 to step 2. */
int nann_group_gather_count(const int64_t* params_row_splits, int64_t n_params_splits,
                            int64_t n_params_values, const int64_t* indices_values,
                            int64_t n_indices_values, const int64_t* indices_row_splits,
                            int64_t n_indices_splits, int64_t* ret_row_splits,
                            int64_t* scratch_offsets, int64_t* n_ret, int64_t* n_ret_splits,
                            int32_t* ragged_code, nann_stream_t stream);
int nann_group_gather_fill(const int32_t* params_values, const int64_t* params_row_splits,
                           const int64_t* indices_values, int64_t n_indices_values,
                           const int64_t* scratch_offsets, int32_t* ret_values,
                           nann_stream_t stream);

/* GroupGather unique=true (UO/beam_search_op/GroupGather_kernel.cc:91-131): per group the SET of the gathered
 * values -- the reference inserts the rows into a std::unordered_set per group and writes it in the set's iteration
 * order, i.e. any order of a group's distinct values is its answer; this library emits first-occurrence order.
 * Input = the unique=false result (values int32[n_values], row_splits int64[n_splits], both device: count + fill
 * above, whose validation and void-input path are the shared head of Compute).  out_values (device) must hold
 * n_values entries, out_row_splits n_splits; scratch: nann_group_gather_unique_scratch_bytes().  *n_out [host]. */
int nann_group_gather_unique_scratch_bytes(int64_t n_values, int64_t n_splits, int64_t* nbytes);
int nann_group_gather_unique(const int32_t* values, int64_t n_values, const int64_t* row_splits, int64_t n_splits,
                             void* scratch, int32_t* out_values, int64_t* out_row_splits, int64_t* n_out,
                             nann_stream_t stream);

/* ---- a2: BitmapRefDifference<int32> (UO/bitmap_op/bitmap_ops.cc:175-257) ---
 * Serial-scan semantics: first occurrence of every id whose bit is clear is
 * kept, in input order, and its bit is set; ONE bitmap shared by all groups.
 * idx_flag (device, int32[n_flag_words]) is mutated in place (Ref input).
 * c_values (device) must hold n_values entries; c_row_splits n_splits entries.
 * *n_out / *n_out_splits [host].  ids outside [0, 32*n_flag_words) ->
 * NANN_ERR_INDEX_OUT_OF_RANGE with the bitmap untouched (UB in the reference). */
int nann_bitmap_ref_difference(const int32_t* idx_next_values, int64_t n_values,
                               const int64_t* idx_next_row_splits, int64_t n_splits,
                               int32_t* idx_flag, int64_t n_flag_words, int32_t* c_values,
                               int64_t* c_row_splits, int64_t* n_out, int64_t* n_out_splits,
                               int32_t* ragged_code, nann_stream_t stream);

/* ---- a8: BloomFilterDifference<int32> (UO/bitmap_op/bitmap_ops.cc:264-425) ----------------
 * The approximate sibling of BitmapRefDifference (registered by the reference, not wired into the
 * serving graph): per node, in input order, four positions of a 32 * bucket_size-bit filter from
 * tensorflow::Fingerprint64 (FarmHash) of the node's decimal string; kept iff one of them was clear;
 * all four set.  idx_flag (device, int32[n_flag_words >= bucket_size]) mutated in place.  Buffers,
 * counts and errors as nann_bitmap_ref_difference. */
int nann_bloom_filter_difference(const int32_t* idx_next_values, int64_t n_values,
                                 const int64_t* idx_next_row_splits, int64_t n_splits, int32_t* idx_flag,
                                 int64_t n_flag_words, int64_t bucket, int64_t bucket_size, int32_t* c_values,
                                 int64_t* c_row_splits, int64_t* n_out, int64_t* n_out_splits,
                                 int32_t* ragged_code, nann_stream_t stream);

/* ---- a3: GatherV2 axis 0 (core/kernels/gather_functor.h:38-116) ------------
 * out[i,:] = params[indices[i],:]; row_bytes must be a multiple of 4.
 * A bad index returns NANN_ERR_INDEX_OUT_OF_RANGE and its position in *bad_i
 * [host] (gather_op.cc:170-175). */
int nann_gather_rows(const void* params, int64_t n_rows, int64_t row_bytes,
                     const int32_t* indices, int64_t n_indices, void* out, int64_t* bad_i,
                     nann_stream_t stream);

/* ---- a5: TopKV2 sorted=true (core/kernels/topk_op.cc:40-205) ---------------
 * values f32[n_rows, n_cols] -> out_values f32[n_rows,k], out_indices
 * i32[n_rows,k]; descending, ties -> lower index.  n_cols < k ->
 * NANN_ERR_TOPK_K_GT_N (checked on the host, nothing launched).  k <= 1024: radix select;
 * larger k (the reference's tests go to k = n = 5000): whole-row sort in LDS, n_cols <= 16384. */
int nann_topk(const float* values, int64_t n_rows, int64_t n_cols, int32_t k,
              float* out_values, int32_t* out_indices, nann_stream_t stream);

/* ---- a4: the scorer behind the BlazeXlaOp contract (UO/blaze_op/
 *          blaze_xla_kernel.cc:24-33, blaze_xla_predictor.cc:360-459) --------
 * A scorer holds what the frozen scoring GraphDef holds in the reference.
 * L2: s = -||q - x||^2.  MLP: x=[q;e] -> h1 -> PReLU -> h2 -> PReLU -> 1
 * (weights f32; [host] pointers, copied to HBM at creation).
 * IP (NANN_SCORER_IP): s = sum_k q_k x_k, the inner product; larger is better, nothing is negated.  It takes no weights: h1, h2,
 * precision and the weight pointers are ignored; every d and row dtype of L2.  Canonical order (the order every entry point
 * sums in, so that one (q, row) has the same score bits whichever call produced them): for d = 8 L, chunk l runs
 * acc = fmaf(q_k, x_k, acc) from +0 over its 8 elements in order, 16-bit rows widened to f32 exactly; the L partials are added
 * in the xor butterfly with strides 1, 2, 4, ...; score = sum.  (L2's tree with the other term and without the final 0 - sum.)
 * Accepted wherever an L2 scorer is -- nann_score, nann_search_opt and its deprecated forwards, nann_search_filtered,
 * nann_search_all(_filtered), nann_search_candidates, and as an `ip` model directory by the *_model calls -- with the L2
 * contract of each call otherwise unchanged (TopKV2 order, the -0 / +0 tie, status codes, batch independence; no table:
 * nann_scorer_prepare / release / table_bytes as for L2).  NOT supported: nann_search_eval, nann_search_eval_ex and
 * nann_search_eval_model return NANN_ERR_UNSUPPORTED for an IP scorer or model and launch nothing.
 * The index is the caller's, and it should be linked by the metric it is searched with: nann_hnsw_build_device_metric and
 * nann_hnsw_append_device_metric (the Python builders: metric="ip") link rows by dist(a, b) = -<a, b>.  The builders' other
 * entry points link by L2 distance, and a graph built that way is a poor neighbourhood structure for inner-product search
 * where the rows' norms carry information (rows of large norm attract queries from far away in L2 terms; measured on such a
 * corpus, DESIGN.md 4.6: recall@50 0.25 on the L2-linked graph, 0.87 on the IP-linked one).  Recall under IP is the caller's
 * to measure, against nann_search_all with the same scorer.
 * Cosine similarity is not a kind of its own: normalise the rows (and the queries) and use either metric -- on unit vectors
 * -||q - x||^2 = 2 <q, x> - 2 ranks as <q, x> does. */
typedef struct nann_scorer nann_scorer;
typedef struct nann_index nann_index;
typedef struct {
  int32_t kind;      /* nann_scorer_kind */
  int32_t d;         /* embedding dim: 64, 128, 256 or 512 */
  int32_t emb_dtype; /* NANN_F16 / NANN_BF16 / NANN_F32 of item rows */
  int32_t h1, h2;    /* MLP only; multiples of 32 */
  const float* w1;     /* [2d, h1] row-major */
  const float* b1;     /* [h1] */
  const float* alpha1; /* [h1] PReLU slope (model_util.py:9-11) */
  const float* w2;     /* [h1, h2] */
  const float* b2;     /* [h2] */
  const float* alpha2; /* [h2] */
  const float* w3;     /* [h2]; last layer has no bias (model.py:218-219) */
  int32_t precision;   /* MLP only: nann_mlp_precision */
} nann_scorer_desc;
/* How the MLP's contractions run on the matrix cores.
 *   SPLIT_F16  every f32 operand as two f16 values (22 significant bits), products on
 *              v_mfma_f32_32x32x16_f16 with f32 accumulation; scores within 1e-5 relative of the
 *              fp32 chain (north_star's bound; ~3e-7 measured), ids equal up to near-ties.
 *              Preconditions: 16-bit item rows; |w| <= 511 for the item half of W1 and for W2
 *              (checked at creation: NANN_ERR_UNSUPPORTED); hidden activations |h1| <= 511
 *              (f16 range after the x2^7 operand scale).  A larger activation SATURATES (the
 *              hi plane is cut with round-toward-zero, which never produces inf): the score is
 *              finite and wrong, so a model with such activations must use EXACT_F32.  The
 *              reference's models are batch-normalised / PReLU nets with O(1) activations.
 *   EXACT_F32  v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, scores BIT-identical to the oracle's
 *              fp32 chain (and therefore identical top-k ids); 1/16 of the 16-bit MFMA rate.
 *   In nann_search BOTH forms run with the ITEM HALF OF LAYER 1 PRE-PROJECTED: P_i = W1e^T e_i is the same vector
 *   whoever scores item i (the canonical order of layer 1 is a1 = u + P with P a chain of its own, oracle/
 *   nann_oracle.c), so it is computed for every item once per (scorer, index) pair -- a resident f32 [n_items, 256]
 *   table owned by the scorer, 1 GB per million items, ~10 ms per million to build: at the pair's first search, or
 *   ahead of traffic by nann_scorer_prepare (below) -- and the traversal gathers that row instead of running layer 1,
 *   with all of layer 2 resident in LDS (csrc/nann_mlp5.h).  Without room for the table (or with pre-projection
 *   switched off) the kernels that read the embedding rows run instead: same results for EXACT_F32, same tolerance for
 *   SPLIT_F16.  nann_score (stand-alone rows, no index) runs all three layers on the matrix cores.
 *   DEFAULT    (0, what a zero-initialised descriptor asks for) SPLIT_F16 when the weights meet its
 *              precondition, else EXACT_F32: 1e-5 is the contract, bit-exactness is opt-in.
 *   CERTIFIED  ids, scores, out_index and counters BIT-identical to EXACT_F32 (and so to the oracle) for every weight
 *              set EXACT_F32 accepts: no |w| or activation precondition.  In the pipeline of phases (nann_search_plan
 *              .phased) a round is scored by an f16 filter -- one v_mfma_f32_32x32x16_f16 per fragment, an approximate
 *              score and a rigorous bound on its distance to the exact one -- and only the rows whose bound interval
 *              reaches the round's k-th largest lower bound are rescored exactly (csrc/nann_mlp6.h); a row the filter
 *              cannot bound (f16 overflow, non-finite values) is always rescored.  Everywhere else CERTIFIED runs the
 *              EXACT_F32 kernels: the planner's non-phased plans, the bitmap rerun of handed-back queries,
 *              preprojection = 0, nann_score, nann_search_eval*; mlp_form = FUSED is taken as PHASED.  Rows rescored
 *              per round: nann_search_refined.  MLP scorers only (nann_attn_scorer_create rejects it). */
enum nann_mlp_precision { NANN_MLP_PRECISION_DEFAULT = 0, NANN_MLP_SPLIT_F16 = 1, NANN_MLP_EXACT_F32 = 2,
                          NANN_MLP_CERTIFIED = 3 };
int nann_scorer_create(const nann_scorer_desc* desc /*[host]*/, nann_scorer** out);
void nann_scorer_destroy(nann_scorer* s);

/* Lifecycle of the pre-projected tables (MLP scorers; attention models, both precisions since round 4: nann_model_* below).
 *   nann_scorer_prepare      builds the table of (scorer, index) on `stream` NOW (or finds it), waits for it, and PINS
 *                            it: a pinned table is never evicted.  A serving host calls this at start-up, so that no
 *                            request pays the build (a hipMalloc + ~10-20 ms per million items + one stream wait).
 *                            NANN_ERR_CAPACITY when HBM has no room for it (searches of the pair still work: they read
 *                            the embedding rows).  Counts: n prepare calls need n releases.
 *   nann_scorer_release      drops one pin; at zero the table is retired at once.
 *   nann_scorer_table_bytes  *table_bytes = HBM bytes the table of this pair takes (ix may be NULL: 0), *resident_bytes
 *                            = bytes the scorer holds right now, all indices (either may be NULL).  This memory is NOT
 *                            part of nann_search_workspace_bytes.
 * Without prepare, the first nann_search of a pair builds the table inside the call (one stream wait) and the scorer
 * keeps the unpinned tables of the two indices it searched last (least recently used goes).  Eviction, release and
 * nann_index_destroy only RETIRE a table: it is freed by a later call once every launch that reads it has completed
 * (an event per stream behind each search), so no call synchronises the device and a concurrent search on another
 * thread never loses its table.  Thread-safe.
 * nann_search_options.preprojection = 0 runs a call without tables; nann_set_preprojection(0) makes that the process
 * default (NANN_PREPROJECT=0 in the environment: the same). */
int nann_scorer_prepare(const nann_scorer* scorer, const nann_index* ix, nann_stream_t stream);
int nann_scorer_release(const nann_scorer* scorer, const nann_index* ix);
int nann_scorer_table_bytes(const nann_scorer* scorer, const nann_index* ix, int64_t* table_bytes,
                            int64_t* resident_bytes);
int nann_set_preprojection(int32_t enabled);

/* comm_seq f16[n_queries, seq_len, d] -> q f32[n_queries, d]: mean over
 * non-pad (not all-zero) rows; the user side of forward()
 * (build_opt_graph.py:76-79, 91-107). */
int nann_user_seq_mean(const void* comm_seq_f16, int64_t n_queries, int32_t seq_len, int32_t d,
                       float* q, nann_stream_t stream);

/* ---- user interests: cluster a behaviour sequence into query vectors -------------------------------------------------
 * comm_seq f16[n_users, seq_len, d] -> q f32[n_users, n_vec, d], the layout nann_search_multi takes for q, and weights
 * f32[n_users, n_vec], the layout nann_fusion takes for per-user weights: the user side of the multi-vector calls, as
 * nann_user_seq_mean is the user side of nann_search.  A history that mixes two tastes has its mean in the empty space
 * between them; here it gets one vector per taste.  The reference has no such call; the contract below is this library's own
 * and is held bit for bit against a numpy model (tests/interests_model.py).
 *
 * Per user.  Every step is a single f32 operation, with no FMA contraction, in the order given.
 *   pad rows      a row whose d halves are all +-0 is pad, as in nann_user_seq_mean: it belongs to no interest, assign = -1.
 *                 m = the number of non-pad rows.
 *   dist(r, c)    for k ascending from acc = +0.0f: t = (float)x[r][k] - c[k]; acc = acc + t * t.  This one chain is the
 *                 whole definition: no tree, no lanes.
 *   first seed    mean = what nann_user_seq_mean returns for this user, bit for bit.  Seed 0 is the non-pad row with the
 *                 greatest dist(r, mean), ties to the lowest r.
 *   more seeds    seed j is the non-pad row with the greatest min over the seeds so far of dist(r, seed), ties to the lowest
 *                 r; if that greatest value is 0, seeding stops.  A seed's centroid is its row converted to f32, so n_seed <=
 *                 min(n_vec, distinct non-pad rows).  Farthest-point seeding is deterministic and needs no RNG state; its
 *                 weakness is that an outlier becomes a seed.
 *   n_vec == 1    there is nothing to separate: the one centroid is the mean itself and no seed row is chosen.
 *   Lloyd rounds  n_iter of them.  In each, every non-pad row goes to the centroid with the least dist, ties to the lowest
 *                 cluster number; then every cluster with members gets, per column, acc from +0.0f over its member rows in
 *                 ascending r and one divide by (float)count; a cluster without members keeps its centroid.  (A round that
 *                 moves no row may end the rounds: the result is the same.)
 *   final pass    one more assignment against the final centroids; clusters it leaves empty are dropped.
 *   order         the rest in descending member count, ties to the lower cluster number.  n_interests[u] = how many remain;
 *                 weights[u][c] = (float)count_c / (float)m; assign[u][r] = the output slot of row r.  Slots c >=
 *                 n_interests[u] hold a copy of slot 0's vector with weight 0.0f -- "a user with fewer interests repeats one
 *                 of them", as nann_search_multi puts it.  A user with m == 0 gets all-zero q, zero weights, n_interests = 0
 *                 and assign = -1 everywhere.
 * Consequences: with n_vec == 1, q is nann_user_seq_mean's output bit for bit for every n_iter, with weight 1; with n_iter ==
 * 0 and n_vec >= 2, q holds the seed rows themselves; a user's answer does not depend on its batch.  NaN / inf in comm_seq
 * are outside the contract.  Asynchronous on `stream`, no host read-back.  weights, n_interests and assign are optional
 * (NULL: not written).  Any d >= 1 and any alignment of comm_seq_f16 work: d % 8 != 0 or a base off the 16-byte grid takes
 * 2-byte loads instead of 16-byte ones, the same bits.
 * Nothing is launched and nothing is written by a refused call: n_users < 0, seq_len < 1, d < 1, n_vec < 1 or n_iter < 0 ->
 * NANN_ERR_BAD_ARGUMENT; n_vec > NANN_INTERESTS_MAX_VEC, n_iter > NANN_INTERESTS_MAX_ITER, n_users > 2^31 - 1, or a shape
 * beyond the kernel's LDS budget -> NANN_ERR_UNSUPPORTED; n_users == 0 -> NANN_OK; a null comm_seq_f16 or q with work to do ->
 * NANN_ERR_BAD_ARGUMENT.  (Where several apply: the sizes first, their NANN_ERR_BAD_ARGUMENT before their
 * NANN_ERR_UNSUPPORTED, then the early NANN_OK, then the null pointers.)  The LDS budget: one workgroup holds a user's whole
 * history and its centroids in 64 KB -- 256 + 4 seq_len ((ceil(d / 2) | 1) + n_vec + 2) + 4 d (n_vec + 1) bytes; 200 x 128 x 8,
 * 50 x 256 x 16 and 600 x 16 x 4 (seq_len x d x n_vec) all fit. */
#define NANN_INTERESTS_MAX_VEC 16
#define NANN_INTERESTS_MAX_ITER 32
int nann_user_seq_interests(const void* comm_seq_f16, int64_t n_users, int32_t seq_len, int32_t d,
                            int32_t n_vec, int32_t n_iter,
                            float* q /*[n_users, n_vec, d]*/, float* weights /*[n_users, n_vec] or NULL*/,
                            int32_t* n_interests /*[n_users] or NULL*/, int32_t* assign /*[n_users, seq_len] or NULL*/,
                            nann_stream_t stream);

/* Score n rows against ONE query vector q f32[d] (rows are scored
 * independently, f32 logits -- the contract PadToStatic/SliceToDynamic rely
 * on).  indices == NULL: rows = item_emb[n, d] as BlazeXlaOp receives them
 * (already gathered).  indices != NULL: fused GatherV2 + score over
 * table[n_table_rows, d] (out-of-range -> NANN_ERR_INDEX_OUT_OF_RANGE,
 * *bad_i [host]).  n == 0 -> NANN_ERR_EMPTY_SCORE_BATCH. */
int nann_score(const nann_scorer* scorer, const float* q, const void* table,
               int64_t n_table_rows, const int32_t* indices, int64_t n, float* out_scores,
               int64_t* bad_i, nann_stream_t stream);

/* ---- a4 (b): the scoring model a BlazeXlaOp node names ----------------------------------
 * The reference's op takes the path of a frozen TensorFlow GraphDef in its `graph_def` attr and runs it in a
 * nested session (blaze_xla_kernel.cc:156-180, blaze_xla_predictor.cc:360-459).  nann_model_load takes the
 * same attr value:
 *   a FILE       the frozen GraphDef itself as convert_meta.py:361-398 writes it (`frozen_graph.pb`:
 *                Model.forward(training=False), model.py:189-233, frozen + fold_constants'ed or merely frozen),
 *                text or binary: read as text first, then as binary, the reference's order (blaze_xla_kernel.cc:
 *                169-175; csrc/host/nann_graphdef_text.h, nann_graphdef.h).
 *                No TensorFlow here and nothing of the graph is executed: the weights are pulled out of the
 *                Const nodes by the names the reference's Python gives their consumers (csrc/host/
 *                nann_graphdef.h), batch norm folded to scale / shift, and handed to the hand-written kernels
 *                (nann_attn_desc).  A graph that is not that model -> NANN_ERR_UNSUPPORTED naming what is
 *                missing; a file that parses as neither -> NANN_ERR_IO.  An optional `<file>.precision` beside it
 *                holds "split" | "exact" (| "certified": MLP only).
 *   a DIRECTORY  of .npy weight files, for scorers that have no frozen graph in the reference (BASELINE's L2
 *                and MLP) and for hosts that hold the model as arrays:
 *                  scorer.txt   one word: l2 | ip | mlp | attention  (l2, ip: no further file)
 *                  mlp          w1 [2d,256]  b1  alpha1  w2 [256,128]  b2  alpha2  w3 [128]     (nann_scorer_desc)
 *                  attention    wq1 bq1 aq wq2 bq2 wk1 bk1 ak wk2 bk2  w0..w3  b0..b2  bn_scale0..2  bn_shift0..2
 *                               alpha0..2                                                    (nann_attn_desc)
 *                  precision.txt (optional, mlp / attention): "split" (default: split-f16 operands on the 16-bit
 *                               MFMA) | "exact" (f32-input MFMA) | "certified" (mlp only: NANN_MLP_CERTIFIED)
 *                Every tensor is checked against the element count (d, seq_len) imply: NANN_ERR_SHAPE_MISMATCH.
 * nann_model_forward is forward() of build_opt_graph.py:91-107 for ONE user: user_seq f16
 * [seq_len, d] (l2 / ip / mlp: its non-pad mean is the query vector; attention: [seq_len, 64]),
 * item_emb [n, d] rows as BlazeXlaOp receives them (already gathered) -> f32 logits[n].
 * All pointers device; workspace = nann_model_workspace_bytes() bytes; asynchronous on stream. */
typedef struct nann_model nann_model;
enum nann_model_kind { NANN_MODEL_L2 = 0, NANN_MODEL_MLP = 1, NANN_MODEL_ATTENTION = 2, NANN_MODEL_IP = 3 };
int nann_model_load(const char* dir /*[host]*/, int32_t d, int32_t emb_dtype, int32_t seq_len, nann_model** out);
void nann_model_destroy(nann_model* m);
int nann_model_kind(const nann_model* m);
/* the l2 / ip / mlp model as the scorer nann_search takes (borrowed; NULL for attention) */
const nann_scorer* nann_model_scorer(const nann_model* m);
int nann_model_workspace_bytes(const nann_model* m, int64_t* nbytes);
int nann_model_forward(const nann_model* m, const void* user_seq_f16, const void* item_emb, int64_t n,
                       float* logits, void* workspace, nann_stream_t stream);

/* BlazeXlaOp's `blaze_option_path` attr as BlazeXlaOp::ParseAttr reads it (UO/blaze_op/blaze_xla_kernel.cc:156-167): first
 * as the PATH of a text-format BlazeKernelOptions file (core/protobuf/config.proto:805-841; NANN_impls/nann/delivery/
 * opt_default.conf is the one build_opt_graph.py:104 passes), then the attr STRING ITSELF as text format; neither ->
 * NANN_ERR_IO "parse proto from ... failed" (the reference: errors::Internal).  A top-level field the message does not
 * have fails the parse, as protobuf's TextFormat does.  What the MI355X op acts on: wait_ms (admission deadline,
 * blaze_xla_kernel.cc:221-258) and run_mode (SKIP, :183-205); the rest is reported for the host's log.  attr [host]. */
typedef struct {
  int32_t struct_bytes;
  int32_t wait_ms;
  int32_t run_mode;               /* 0 DEFAULT, 1 BENCHMARK, 2 SKIP */
  int32_t xla_compilation;
  int32_t auto_mixed_precision;
  int32_t disable_output_padding;
  int32_t n_warmup_batchsize;     /* entries of warmup_batchsize (no warm-up here: rows are scored as they come) */
  int32_t max_warmup_batchsize;
  int32_t from_file;              /* 1: the attr named a readable file; 0: the attr string was the message */
} nann_blaze_options;
int nann_blaze_options_parse(const char* attr, nann_blaze_options* out);

/* ---- a6 + a7: resident index and the fused traversal -----------------------
 * The index is what the serving graph's HugeConst nodes hold
 * (build_opt_graph.py:83-90, 70): item_embs [N,d], item_ids i64[N], per level
 * CSR (values i32, row_splits i64[N+1]) for levels 0 and 1, enter_points
 * i32[E] (ascending, unique). */
typedef struct {
  int64_t n_items;
  int32_t d;
  int32_t emb_dtype;
  const void* item_embs;
  const int64_t* item_ids;
  const int32_t* nb_values[2];
  const int64_t* nb_row_splits[2];
  int64_t nb_nnz[2];
  const int32_t* enter_points;
  int64_t n_enter;
  int32_t on_device; /* 0: [host] pointers, copied to HBM once (HugeConst's one-time
                        H2D); 1: device pointers, borrowed for the handle's lifetime */
} nann_index_desc;
int nann_index_create(const nann_index_desc* desc /*[host]*/, nann_index** out);
void nann_index_destroy(nann_index* ix);
/* [host] out: n_items, d, n_enter, max row length at level 0 / 1, bitmap words */
int nann_index_info(const nann_index* ix, int64_t out[6]);
/* nann_index_create note: the probe below makes the call SYNCHRONISE the device (a hipMalloc, one small launch on the NULL
 * stream, two blocking copies, a hipFree): create indices at start-up, not next to traffic.  NANN_INDEX_PROBE=0 in the
 * environment skips it (the planner falls back to its estimate from the mean degree).  A probe that fails never fails the
 * creation and leaves nann_last_error as it found it.
 * The probe nann_index_create runs on every index of >= 4096 items (round 5): 64 of its own rows as queries, ef = min(64,
 * #enter points), L2 scorer, one small launch -- how many NEW nodes a level-0 round finds per frontier row on THIS graph,
 * which is what sizes a query's visited set (16K-slot hash set, two workgroups per CU; 32K slots, one; bitmap).  The planner
 * uses the measurement in place of rounds 1-4's guess from the mean degree: 1.15 x the 90th percentile of the probe's queries
 * (a query in the tail beyond it is rerun on the bitmap kernel like any query whose set would overflow).  out[5] = {valid
 * queries of the probe (0: none, the planner falls back to the guess), ef, mean, 90th percentile, max}. */
int nann_index_probe_info(const nann_index* ix, float out[5]);

#define NANN_NUM_ROUNDS 5
/* Where a query's visited set lives (the reference: a TemporaryVariable bitmap of N/32 words,
 * build_opt_graph.py:115-118).  AUTO picks per call: shards below 2^27 items -> an exact hash
 * set of visited ids in LDS -- LDS_HASH (16K slots, 64 KB: two queries per CU with the L2 scorer,
 * one with the matrix-core scorers) or, L2 scorer only, for beams whose visited set is expected to
 * outgrow it and for batches of at most one query per CU, LDS_HASH32 (32K slots, one query per CU);
 * a query whose set could overflow is rerun on a bitmap kernel inside the same call.  Otherwise
 * (matrix-core scorers with wide beams, larger shards) LDS_BITMAP when ceil(N/32) words fit the CU's
 * LDS next to the phase buffers, else HBM_BITMAP.  Results are identical in every mode (tested);
 * the knob exists for tests and tuning.  Per call: nann_search_options.traversal_mode; nann_set_traversal_mode stores the
 * process default of that field.  Thread-safe. */
enum nann_traversal_mode { NANN_TRAVERSAL_AUTO = 0, NANN_TRAVERSAL_LDS_BITMAP = 1,
                           NANN_TRAVERSAL_HBM_BITMAP = 2, NANN_TRAVERSAL_LDS_HASH = 3,
                           NANN_TRAVERSAL_LDS_HASH32 = 4 };
int nann_set_traversal_mode(int32_t mode);
/* Workgroup slots the persistent traversal grid leaves free on the device (default 0: it takes every CU, two
 * workgroups each for the L2 plan).  A host that runs other kernels NEXT TO a search -- the exchange of batch i on its
 * own stream while batch i + 1 is searched (8(e), nann_sharded_topk) -- reserves a few: without them those kernels
 * only start when the first traversal workgroups exit (measured, profiles/r4_overlap_*.json).  Per call:
 * nann_search_options.slot_reserve; this setter stores the process default of that field. */
int nann_set_search_reserve(int32_t workgroups);

/* Workspace bytes nann_search needs for (index, level_topn, n_queries), any scorer. */
int nann_search_workspace_bytes(const nann_index* ix, const int32_t level_topn[6] /*[host]*/,
                                int64_t n_queries, int64_t* nbytes);

/* ONE search operation, ONE entry point per query form (ABI v6):
 *     nann_search_opt        queries as vectors   q f32[n_queries, d]                 (l2 / mlp scorers)
 *     nann_search_model_opt  queries as comm_seq  f16[n_queries, seq_len, E]          (any model a BlazeXlaOp node names)
 * Both take per-launch maxima `level_topn_max`, an optional per-query `level_topn` table, per-call options and return the
 * planner's choice.  The five older spellings below (nann_search, nann_search_v, nann_search_ex, nann_search_model,
 * nann_search_model_v: rounds 1-5) are DEPRECATED THIN WRAPPERS -- each is one `return` of the canonical call with NULLs in
 * the places it does not have (tests/test_abi.py asserts that) -- kept so that hosts built against v5 keep linking; new
 * hosts (csrc/host/nann_serve.cpp, tf_ops/nann_tf_ops.cc, nann_amd/retrieval.py) call the canonical pair only.
 *
 * The whole schedule of build_model() (NANN_impls/nann/delivery/
 * build_opt_graph.py:109-149) for n_queries independent
 * queries, persistent workgroups that pull queries from a device-wide queue, visited set in LDS
 * (nann_traversal_mode).
 *   q            f32[n_queries, d]      (nann_user_seq_mean of comm_seq)
 *   level_topn   [host] i32[6]          (the `level_topn` feed)
 *   workspace    device, nann_search_workspace_bytes(...) bytes
 *   out_item_ids i64[n_queries, level_topn[5]]   ('top_k' fetch)
 *   out_scores   f32[n_queries, level_topn[5]]   (not a reference output;
 *                                                 for the 1e-5 check) or NULL
 *   out_index    i32[n_queries, level_topn[5]]   internal indices or NULL
 *   status       i32[n_queries]: per-query nann_status -- a query the
 *                reference would fail (k > n, empty score batch, ...) gets
 *                its code here and zeroed outputs
 *   counters     i32[n_queries, 3, NANN_NUM_ROUNDS] (F_r, G_r, S_r per round:
 *                rows walked, neighbours gathered, rows scored) or NULL
 * Asynchronous on `stream`. */
/* deprecated: thin wrapper of nann_search_opt */
int nann_search(const nann_index* ix, const nann_scorer* scorer, const float* q,
                int64_t n_queries, const int32_t level_topn[6], void* workspace,
                int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores,
                int32_t* out_index, int32_t* status, int32_t* counters, nann_stream_t stream);

/* The same with level_topn PER QUERY, as the reference feeds it per request (build_opt_graph.py:75,151-159: `level_topn`
 * is a placeholder of the serving signature, so two requests of one batch may ask for different beams).
 *   level_topn_max [host] i32[6]  per-launch maxima: they size the workspace (nann_search_workspace_bytes) and the
 *                                 plan, and level_topn_max[5] is the ROW STRIDE of out_item_ids / out_scores / out_index
 *   level_topn     device i32[n_queries, 6] (NULL: every query takes level_topn_max -- nann_search's fast path)
 * Query i returns its level_topn[i][5] results at the head of row i, zeros behind.  An entry outside
 * [0, level_topn_max[j]] fails THAT query with NANN_ERR_BAD_ARGUMENT in status[i]; k > n and the other failures of
 * the reference are per query as before.  Each query's result is bit-identical to a uniform launch with its values. */
/* deprecated: thin wrapper of nann_search_opt */
int nann_search_v(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries,
                  const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace,
                  int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                  int32_t* status, int32_t* counters, nann_stream_t stream);

/* Same as nann_search, plus per-query time attribution for tuning: phase_ticks
 * i64[n_queries, NANN_NUM_PHASES] receives shader-clock ticks spent in
 * {bitmap zeroing, mark walks, CSR expand+walk, gather+score, top-k, other} followed by
 * sub-phases {top-k: load, search, collect, sort; expand: pass 1, pipeline loop, filter; hash-set
 * expand per piece: lookup + prefetch, id load wait, insert, barrier, check, rank + store}; NULL
 * disables the instrumentation (nann_search passes NULL). */
#define NANN_NUM_PHASES 19
/* deprecated: thin wrapper of nann_search_opt */
int nann_search_ex(const nann_index* ix, const nann_scorer* scorer, const float* q,
                   int64_t n_queries, const int32_t level_topn[6], void* workspace,
                   int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores,
                   int32_t* out_index, int32_t* status, int32_t* counters, int64_t* phase_ticks,
                   nann_stream_t stream);

/* ---- options of a search call (round 5; ABI v5) -----------------------------------------------------------------
 * Every knob of the planner travels WITH THE CALL, so threads that share an index / scorer handle do not share a plan
 * (rounds 1-4 had three process-global setters beside an ABI that promises re-entrancy).  A field left at -1 takes the
 * process default: what the matching nann_set_* call stored, else the built-in value (AUTO, 0, 1, AUTO).
 *   traversal_mode  enum nann_traversal_mode: where a query's visited set lives
 *   slot_reserve    workgroup slots the persistent grids leave free for kernels of other streams (the exchange of a
 *                   sharded search that overlaps the next batch); the MLP's pipeline of phases honours it too
 *   preprojection   1: MLP / attention scorers read their per-(scorer, index) tables; 0: the kernels that read the
 *                   embedding rows (a host with no HBM to spare)
 *   mlp_form        enum nann_mlp_form: the fused kernel or the pipeline of phases for an MLP traversal on its table;
 *                   AUTO = the planner's measured rule (exact f32: phased; split-f16: phased up to 160 queries and for
 *                   wide beams)
 * nann_search_plan ([host], optional) receives what the planner chose; the number of queries the hash-set kernel handed
 * back to the bitmap kernel is read from the workspace afterwards (nann_search_reruns: synchronises `stream`). */
enum nann_mlp_form { NANN_MLP_FORM_AUTO = 0, NANN_MLP_FORM_FUSED = 1, NANN_MLP_FORM_PHASED = 2 };
typedef struct {
  int32_t struct_bytes;   /* sizeof(nann_search_options) of the caller's header (nann_search_options_init sets it) */
  int32_t traversal_mode;
  int32_t slot_reserve;
  int32_t preprojection;
  int32_t mlp_form;
} nann_search_options;
typedef struct {
  int32_t visited_set;           /* enum nann_traversal_mode of the main launch (of the traversal stages when phased) */
  int32_t fallback_visited_set;  /* ... of the rerun of handed-back queries */
  int32_t threads;               /* per workgroup */
  int32_t workgroups;            /* resident workgroups (= queries in flight) */
  int32_t phased;                /* 1: the MLP's pipeline of phases */
  int32_t table;                 /* 1: a pre-projected table is read */
  float est_visited;             /* the planner's estimate of a level's visited ids (hash-set capacity: 16K / 32K slots) */
  float worst_visited;           /* the bound from the index's maximum degrees */
  int32_t lean;                  /* 1: the main launch is the lean instantiation of the L2 / inner-product hash-set kernel, its
                                  * phase timers off at compile time (a plain call: uniform level_topn, no phase_ticks, at most
                                  * 2^20 items; NANN_LEAN_KERNEL=0 switches it off); results are the general kernel's bit for bit */
} nann_search_plan;
void nann_search_options_init(nann_search_options* o);
/* nann_search_v + phase_ticks (uniform level_topn only) + options + plan.  level_topn == NULL: level_topn_max for all. */
int nann_search_opt(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries,
                    const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace, int64_t workspace_bytes,
                    int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* status, int32_t* counters,
                    int64_t* phase_ticks, const nann_search_options* options, nann_search_plan* plan, nann_stream_t stream);
/* queries of the LAST search on `workspace` that were rerun on the bitmap kernel (phased MLP: of its last chunk) */
int nann_search_reruns(const void* workspace, int64_t* n_rerun, nann_stream_t stream);
/* rows the LAST search on `workspace` rescored exactly, per round, summed over its queries (NANN_MLP_CERTIFIED in the
 * pipeline of phases; counters' S_r counts every scored row, rescored or not).  0 for rounds no filter ran: other
 * precisions and scorers, and the plans on which CERTIFIED runs the exact kernels.  Synchronises `stream`. */
int nann_search_refined(const void* workspace, int64_t out[NANN_NUM_ROUNDS], nann_stream_t stream);

/* ---- exhaustive search: test_all (NANN_impls/main.py:194-237) for a batch of queries ------------------------------
 * Every item of the index scored for every query, then TopKV2 sorted=true per query (NANN_impls/nann/util.py:9-11 is the
 * recall the reference computes against it): descending, ties -> lower internal row number, -0 and +0 tie.  The ground
 * truth of every recall figure, as ONE call instead of a nann_score + nann_topk loop over the queries: a row is fetched
 * once for a tile of queries, the selection runs on every CU (csrc/nann_scan.h).
 *   q            f32[n_queries, d]
 *   out_item_ids i64[n_queries, k] = item_ids[out_index]
 *   out_scores   f32[n_queries, k] or NULL;  out_index i32[n_queries, k] (internal row numbers) or NULL
 *   workspace    device, 256-byte aligned (else NANN_ERR_BAD_ARGUMENT), nann_search_all_workspace_bytes(...) bytes; smaller ->
 *                NANN_ERR_CAPACITY.  Bounded: queries are processed in chunks inside the call -- the scores of a chunk take at
 *                most max(512 MiB, one query's 4 B x n_items) at a time, never n_queries x n_items
 *   options      NULL = defaults; only `preprojection` is read (-1: the process default)
 * L2 scorer: every d and row dtype nann_score accepts, scores bit-identical to the oracle (DESIGN.md 2's order).  MLP scorer:
 * scored from the pre-projected table of the (scorer, index) pair, found or built as in nann_search_opt -- EXACT_F32 and
 * CERTIFIED (which runs the exact arithmetic here) bit-identical to the oracle, SPLIT_F16 within 1e-5 max(1, |s|); without a
 * table NANN_ERR_CAPACITY (no room in HBM) or NANN_ERR_UNSUPPORTED (preprojection resolves to 0).
 * k < 0 or n_queries < 0 -> NANN_ERR_BAD_ARGUMENT; k > n_items -> NANN_ERR_TOPK_K_GT_N, nothing launched (as nann_topk); k == 0 or
 * n_queries == 0 -> NANN_OK, nothing written; k > 1024 -> NANN_ERR_UNSUPPORTED.  A query's answer does not depend on the batch
 * it is in.  Asynchronous on `stream`, no host read-back, re-entrant on shared handles. */
int nann_search_all_workspace_bytes(const nann_index* ix, const nann_scorer* scorer, int64_t n_queries, int32_t k,
                                    int64_t* nbytes);
int nann_search_all(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries, int32_t k,
                    int64_t* out_item_ids, float* out_scores, int32_t* out_index, void* workspace, int64_t workspace_bytes,
                    const nann_search_options* options, nann_stream_t stream);

/* The serving signature in one call (build_opt_graph.py:151-159): comm_seq f16[n_queries, seq_len, E]
 * + level_topn -> top_k, scored by whatever model the BlazeXlaOp nodes of the graph name.  l2 / mlp:
 * nann_user_seq_mean + nann_search.  attention: the per-user projection once per request
 * (nann_attn_prepare), then the fused traversal with the attention + DNN scorer on the matrix cores
 * (scores within 1e-5 of the oracle restatement: device expf / MFMA order; ids tie-aware).
 * workspace: nann_search_model_workspace_bytes(); other arguments as nann_search. */
int nann_search_model_workspace_bytes(const nann_index* ix, const nann_model* m, const int32_t level_topn[6],
                                      int64_t n_queries, int64_t* nbytes);
/* deprecated: thin wrapper of nann_search_model_opt */
int nann_search_model(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_queries,
                      const int32_t level_topn[6], void* workspace, int64_t workspace_bytes,
                      int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* status,
                      int32_t* counters, nann_stream_t stream);

/* per-query level_topn (nann_search_v) and the table lifecycle (nann_scorer_prepare ...) for a model */
/* deprecated: thin wrapper of nann_search_model_opt */
int nann_search_model_v(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_queries,
                        const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace,
                        int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                        int32_t* status, int32_t* counters, nann_stream_t stream);
/* ... with per-call options and the planner's choice (see nann_search_opt) */
int nann_search_model_opt(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_queries,
                          const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace,
                          int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                          int32_t* status, int32_t* counters, const nann_search_options* options, nann_search_plan* plan,
                          nann_stream_t stream);
int nann_model_prepare(const nann_model* m, const nann_index* ix, nann_stream_t stream);
int nann_model_release(const nann_model* m, const nann_index* ix);
int nann_model_table_bytes(const nann_model* m, const nann_index* ix, int64_t* table_bytes, int64_t* resident_bytes);

/* ---- exhaustive search under a model: test_all (NANN_impls/main.py:194-237) with the serving signature's input ------
 * nann_search_all for whatever model the node names, the reference's own attention + DNN model included: every item of the
 * index scored for every user, then TopKV2 sorted=true per user (NANN_impls/nann/util.py:9-11): descending, ties -> lower
 * internal row number, -0 and +0 tie.
 *   comm_seq_f16 f16[n_users, seq_len, E], as nann_search_model_opt takes it
 *   out_item_ids i64[n_users, k] = item_ids[out_index]
 *   out_scores   f32[n_users, k] or NULL;  out_index i32[n_users, k] (internal row numbers) or NULL
 *   workspace    device, 256-byte aligned (else NANN_ERR_BAD_ARGUMENT), nann_search_all_model_workspace_bytes(...) bytes; smaller
 *                -> NANN_ERR_CAPACITY.  Bounded: users are processed in chunks of at most 128 inside the call -- the scores of a
 *                chunk take at most max(512 MiB, one user's 4 B x n_items) at a time, never n_users x n_items; the attention
 *                model adds the chunk's per-user side (nann_attn_prepare: 80 KB per user)
 *   options      NULL = defaults; only `preprojection` is read (-1: the process default)
 * l2 / mlp model: nann_user_seq_mean into the workspace, then nann_search_all with the model's own scorer (same bits).
 * attention model: nann_attn_prepare per chunk of users, then every row scored from the pre-projected table of the (model,
 * index) pair (csrc/nann_scan_attn_inst.hip), found or built as in nann_search_model_opt and released with the call's event --
 * both precisions scan from the table: scores within 1e-5 max(1, |s|) of the oracle, and for the split-f16 precision
 * bit-identical to what the hash-set traversal computes for the same (user, row); without a table NANN_ERR_CAPACITY (no room
 * in HBM) or NANN_ERR_UNSUPPORTED (preprojection resolves to 0).  Model and index disagree on d / dtype -> NANN_ERR_BAD_ARGUMENT.
 * k < 0 or n_users < 0 -> NANN_ERR_BAD_ARGUMENT; k > n_items -> NANN_ERR_TOPK_K_GT_N, nothing launched (as nann_topk); k == 0 or
 * n_users == 0 -> NANN_OK, nothing written; k > 1024 -> NANN_ERR_UNSUPPORTED.  A user's answer does not depend on the batch
 * it is in.  Asynchronous on `stream`, no host read-back, re-entrant on shared handles. */
int nann_search_all_model_workspace_bytes(const nann_index* ix, const nann_model* m, int64_t n_users, int32_t k, int64_t* nbytes);
int nann_search_all_model(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_users, int32_t k,
                          int64_t* out_item_ids, float* out_scores, int32_t* out_index, void* workspace, int64_t workspace_bytes,
                          const nann_search_options* options, nann_stream_t stream);

/* ---- filtered retrieval: a deny bitmap for every query and an exclusion list per query ------------------------------
 * What a recommender removes before it answers: rows blocked for everybody (out of stock, withdrawn) and, per user, the
 * rows that user has seen.  The reference has no such feature -- its serving graph returns the top_k of the traversal as it
 * is -- so nothing here restates a line of it; the semantics below are this library's own.
 * A filter is a plain struct, passed per call and BORROWED for the call: no handle, no process state.  NULL, or all three
 * pointers NULL, denies nothing.  Malformed contents never fault: a listed row outside [0, n_items) denies nothing, every
 * [splits[i], splits[i + 1]) is clamped to [0, n_excl] and an inverted range is empty.  struct_bytes: 0 or
 * sizeof(nann_filter); n_excl < 0, or splits without rows while n_excl > 0 -> NANN_ERR_BAD_ARGUMENT. */
typedef struct {
  int32_t struct_bytes;
  const uint32_t* deny_bits;        /* device, ceil(n_items / 32) words, or NULL: row r is denied for EVERY query when
                                       bit (r & 31) of word (r >> 5) is set (idx_flag's convention); bits at or beyond
                                       n_items in the last word are ignored */
  const int64_t* excl_row_splits;   /* device i64[n_queries + 1], or NULL: query i excludes excl_rows[splits[i] .. splits[i+1]) */
  const int32_t* excl_rows;         /* device i32[n_excl]: INTERNAL row numbers; any order, duplicates allowed */
  int64_t n_excl;
} nann_filter;

/* Exhaustive search over the ALLOWED rows: nann_search_all / nann_search_all_model -- same arguments, checks and error codes --
 * plus the filter and n_out (device i32[n_queries], or NULL).  Query i returns the top k of its allowed rows in TopKV2 order
 * (descending, ties -> lower row), n_out[i] valid entries at the head of its row and zeros behind.  When every allowed row
 * scores above -inf, n_out[i] = min(k, allowed rows of query i); an allowed row whose own score is -inf may be displaced by a
 * denied one (denied rows are taken out by writing -inf over their scores between scoring and selection); NaN scores stay
 * outside the contract, as for nann_topk.  The workspace adds 16 B x k per query of a chunk to the unfiltered one.
 * Asynchronous, no host read-back, and a query's answer does not depend on its batch. */
int nann_search_all_filtered_workspace_bytes(const nann_index* ix, const nann_scorer* scorer, int64_t n_queries, int32_t k,
                                             int64_t* nbytes);
int nann_search_all_filtered(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries, int32_t k,
                             int64_t* out_item_ids, float* out_scores, int32_t* out_index, void* workspace,
                             int64_t workspace_bytes, const nann_search_options* options, const nann_filter* filter,
                             int32_t* n_out, nann_stream_t stream);
int nann_search_all_model_filtered_workspace_bytes(const nann_index* ix, const nann_model* m, int64_t n_users, int32_t k,
                                                   int64_t* nbytes);
int nann_search_all_model_filtered(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_users,
                                   int32_t k, int64_t* out_item_ids, float* out_scores, int32_t* out_index, void* workspace,
                                   int64_t workspace_bytes, const nann_search_options* options, const nann_filter* filter,
                                   int32_t* n_out, nann_stream_t stream);

/* ---- range search: every row scoring at or above a per-query cut ------------------------------------------------------
 * "Which rows score at least t for this query?" -- every item whose logit clears a serving cut, every near-duplicate within
 * an L2 radius (L2 scores are -dist^2, so a radius is a cut), the size of a recall set before k is chosen.  The reference has
 * no such call -- its test_all job keeps a top k -- so nothing here restates a line of it; the semantics below are this
 * library's own.  The scoring of nann_search_all / nann_search_all_model, chunk by chunk, with a second
 * selection stage over each chunk's scores (csrc/nann_range.h) in the place of the top k.  There is no k: NANN_ERR_TOPK_K_GT_N
 * and the k <= 1024 limit do not apply.
 *   q / comm_seq_f16  f32[n_queries, d] / f16[n_users, seq_len, E], as nann_search_all / nann_search_all_model take them
 *   thresholds        device f32[n_queries]: the cut of every query
 *   capacity          entries of out_item_ids / out_scores / out_index
 *   out_row_splits    device i64[n_queries + 1]
 *   out_item_ids      device i64[capacity] = item_ids[out_index]; NULL only with capacity == 0
 *   out_scores        device f32[capacity] or NULL;  out_index device i32[capacity] (internal row numbers) or NULL
 *   workspace         device, 256-byte aligned (else NANN_ERR_BAD_ARGUMENT), nann_search_all_range[_model]_workspace_bytes(...)
 *                     bytes; smaller -> NANN_ERR_CAPACITY.  The unfiltered workspace of nann_search_all without its k-wide lists,
 *                     plus 4 B per (query of a chunk, block of 2048 rows)
 *   options           NULL = defaults; only `preprojection` is read, as in nann_search_all
 *   filter            NULL: none.  Else as in nann_search_all_filtered, a malformed one included
 * Match rule: row r matches query i iff score(i, r) >= thresholds[i] and score(i, r) != -inf, compared as IEEE does: -0 >= +0
 * holds, a NaN score or a NaN threshold matches nothing.  -inf is how a denied row is marked, so a row scoring -inf is never
 * returned, whatever the threshold: denied and excluded rows are absent also at a threshold of -inf.
 * Results: out_row_splits holds the TRUE counts, whatever the capacity -- out_row_splits[0] = 0, out_row_splits[i + 1] -
 * out_row_splits[i] rows match query i, out_row_splits[n_queries] is the total.  Query i's entries are the positions
 * [out_row_splits[i], out_row_splits[i + 1]) of the outputs, in ASCENDING ROW ORDER.  Capacity guard: a position at or beyond
 * capacity is dropped, never written -- what is written is the head [0, min(total, capacity)) of the uncapped result, and
 * positions [min(total, capacity), capacity) are left untouched.  capacity == 0 with the three entry outputs NULL is a valid
 * count-only call; the caller sees truncation by out_row_splits[n_queries] > capacity and calls again.
 * Scores: each returned score is bit-identical to what nann_search_all / nann_search_all_model return for the same (query,
 * row) under the same handle and options -- L2, inner product, EXACT_F32 and CERTIFIED MLP bit-identical to the oracle,
 * SPLIT_F16 MLP and the attention model within 1e-5 max(1, |s|) of it.
 * Batch independence: a query's segment -- rows, order, score bits -- does not depend on the batch it is in.
 * Errors, each in front of the first launch, so that a failing call launches nothing and writes nothing: a null handle,
 * n_queries < 0, capacity < 0, handle and index disagree on d / dtype, a bad struct_bytes of options or filter, a workspace off
 * the 256-byte grid -> NANN_ERR_BAD_ARGUMENT; with work to do (n_queries > 0) a null q / thresholds / out_row_splits, or
 * capacity > 0 with a null out_item_ids -> NANN_ERR_BAD_ARGUMENT; workspace too small -> NANN_ERR_CAPACITY; n_queries >
 * 2^31 - 1 -> NANN_ERR_UNSUPPORTED; no pre-projected table: as in nann_search_all.  n_queries == 0 -> NANN_OK, nothing
 * written.  Asynchronous on `stream`, no host read-back, re-entrant on shared handles. */
int nann_search_all_range_workspace_bytes(const nann_index* ix, const nann_scorer* scorer, int64_t n_queries, int64_t* nbytes);
int nann_search_all_range(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries,
                          const float* thresholds, int64_t capacity, int64_t* out_row_splits, int64_t* out_item_ids,
                          float* out_scores, int32_t* out_index, void* workspace, int64_t workspace_bytes,
                          const nann_search_options* options, const nann_filter* filter, nann_stream_t stream);
int nann_search_all_range_model_workspace_bytes(const nann_index* ix, const nann_model* m, int64_t n_users, int64_t* nbytes);
int nann_search_all_range_model(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_users,
                                const float* thresholds, int64_t capacity, int64_t* out_row_splits, int64_t* out_item_ids,
                                float* out_scores, int32_t* out_index, void* workspace, int64_t workspace_bytes,
                                const nann_search_options* options, const nann_filter* filter, nann_stream_t stream);

/* The traversal, filtered at its final selection: nann_search_opt / nann_search_model_opt -- same arguments, checks and error
 * codes -- plus the filter, k and n_out (device i32[n_queries], or NULL).  level_topn_max[5] is the FETCH WIDTH F: the inner
 * search runs unchanged at F into a staging area of the workspace (16 B x F per query, counted by the _workspace_bytes
 * functions), and query i's answer is the first k allowed entries of what the unfiltered call returns for it at its own
 * level_topn[i][5], order kept: outputs are [n_queries, k], n_out[i] entries at the head of row i and zeros behind.  Denied
 * rows still guide the walk -- a graph search needs them to stay connected -- but are not returned.  F as wide as the pool,
 * min(level_topn[1] + ... + level_topn[4], 1024), ranks the whole pool; F obeys the limits of level_topn[5] (at most 1024; a
 * query whose level_topn[5] exceeds its pool fails as it does unfiltered).  k outside [0, F] -> NANN_ERR_BAD_ARGUMENT.  A
 * query with status[i] != 0 gets n_out[i] = 0 and zeros.  counters, status, plan, nann_search_reruns and nann_search_refined
 * report what the inner search reported. */
int nann_search_filtered_workspace_bytes(const nann_index* ix, const int32_t level_topn[6] /*[host]*/, int64_t n_queries,
                                         int64_t* nbytes);
int nann_search_filtered(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries,
                         const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace, int64_t workspace_bytes,
                         int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* status, int32_t* counters,
                         int64_t* phase_ticks, const nann_search_options* options, nann_search_plan* plan,
                         const nann_filter* filter, int32_t k, int32_t* n_out, nann_stream_t stream);
int nann_search_model_filtered_workspace_bytes(const nann_index* ix, const nann_model* m, const int32_t level_topn[6],
                                               int64_t n_queries, int64_t* nbytes);
int nann_search_model_filtered(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_queries,
                               const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace,
                               int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                               int32_t* status, int32_t* counters, const nann_search_options* options, nann_search_plan* plan,
                               const nann_filter* filter, int32_t k, int32_t* n_out, nann_stream_t stream);

/* ---- candidate-list search: exact top-k over per-query candidate rows ------------------------------------------------
 * "Here are the rows I may, or want to, return for this user: score them and give me the best k" -- re-ranking a merged
 * recall set, an allow-list (a category, a campaign, a seller's stock), the small-allowed-set end of filtered retrieval.  The
 * reference has no such call -- its serving graph scores what its own traversal reaches -- so nothing here restates a line of
 * it; the semantics below are this library's own.  The cost is proportional to the lists, not to the index.
 * The lists are a plain struct, passed per call and BORROWED for the call: */
typedef struct {
  int32_t struct_bytes;        /* 0 or sizeof(nann_candidates) */
  const int64_t* row_splits;   /* device i64[n_queries + 1]: query i's list is rows[row_splits[i] .. row_splits[i+1]) */
  const int32_t* rows;         /* device i32[n_cand]: INTERNAL row numbers; any order; duplicates allowed */
  int64_t n_cand;              /* [host] length of rows: sizes the workspace */
} nann_candidates;
/*   q            f32[n_queries, d]
 *   out_item_ids i64[n_queries, k] = item_ids[out_index];  status i32[n_queries] -- both required
 *   out_scores   f32[n_queries, k], out_index i32[n_queries, k] (internal row numbers), out_pos i32[n_queries, k] (the entry's
 *                0-based position within query i's list: what a re-ranking host maps back with), n_out i32[n_queries] -- each
 *                may be NULL
 *   workspace    device, 256-byte aligned (else NANN_ERR_BAD_ARGUMENT), nann_search_candidates_workspace_bytes(...) bytes; smaller
 *                -> NANN_ERR_CAPACITY.  4 B per candidate, 24 B per query, and 1 KB per query under the MLP scorer
 *   options      NULL = defaults; only `preprojection` is read (-1: the process default), as in nann_search_all
 * Results: query i returns the min(k, len_i) best-scoring entries of its own list in TopKV2 order -- scores descending, ties ->
 * the lower position in the list, -0 and +0 tie; NaN scores stay outside the contract, as for nann_topk.  n_out[i] entries at the
 * head of row i of every output and zeros behind.  A row listed twice is scored twice and can be returned twice: there is no
 * dedup, and k may exceed n_items (no NANN_ERR_TOPK_K_GT_N here).  An empty list is no error: n_out = 0, status = 0.  A caller
 * who passes each list in ascending row order without duplicates gets "the top k of the allowed rows" of
 * nann_search_all_filtered.
 * Failures are per query, never per call and never a fault.  Query i is WELL-FORMED iff 0 <= row_splits[i] <= row_splits[i+1] <=
 * n_cand and row_splits[i] >= row_splits[j] for every j < i; any other query gets status[i] = NANN_ERR_INVALID_RAGGED_INPUT,
 * n_out[i] = 0 and a zeroed row.  (The rule makes the ranges of well-formed queries pairwise disjoint -- an earlier well-formed
 * query's end is an earlier split, hence <= this query's begin -- so the score buffer, addressed by list position, has one
 * writer per element whatever the caller passes.)  A well-formed query that lists a row outside [0, n_items) gets status[i] =
 * NANN_ERR_INDEX_OUT_OF_RANGE, n_out[i] = 0 and zeros.  No other query's answer changes in either case.
 * L2 scorer: every d (64, 128, 256, 512) and row dtype nann_score accepts, scores bit-identical to the oracle on the gathered
 * rows and so to nann_score with `indices`.  MLP scorer: scored from the pre-projected table of the (scorer, index) pair, found or
 * built as in nann_search_all and released behind the call's event -- EXACT_F32 and CERTIFIED (which runs the exact arithmetic
 * here) bit-identical to the oracle, SPLIT_F16 within 1e-5 max(1, |s|); without a table NANN_ERR_CAPACITY (no room in HBM) or
 * NANN_ERR_UNSUPPORTED (preprojection resolves to 0).  The attention model is not served by this call: it has a handle type of
 * its own, and nann_search_candidates_model below takes it.
 * Nothing is launched for: null ix, scorer or cand, a struct_bytes mismatch, n_queries < 0, n_cand < 0, k < 0, rows == NULL with
 * n_cand > 0, row_splits == NULL with n_queries > 0, scorer and index disagreeing on d / dtype -> NANN_ERR_BAD_ARGUMENT; k > 1024
 * or n_cand > 2^31 - 1 -> NANN_ERR_UNSUPPORTED; n_queries == 0 or k == 0 -> NANN_OK, nothing written.  A query's answer does not
 * depend on the batch it is in.  Asynchronous on `stream`, no host read-back (the lists' lengths are device data), re-entrant
 * on shared handles. */
int nann_search_candidates_workspace_bytes(const nann_index* ix, const nann_scorer* scorer, int64_t n_queries, int64_t n_cand,
                                           int32_t k, int64_t* nbytes);
int nann_search_candidates(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries, int32_t k,
                           const nann_candidates* cand, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                           int32_t* out_pos, int32_t* n_out, int32_t* status, void* workspace, int64_t workspace_bytes,
                           const nann_search_options* options, nann_stream_t stream);

/* ---- candidate-list search under a model: nann_search_candidates for whatever model the node names ---------------------
 * nann_search_candidates with the serving signature's input, as nann_search_all_model is to nann_search_all: comm_seq_f16 is
 * f16[n_users, seq_len, E] (what nann_search_model_opt and nann_search_all_model take), `cand` the same nann_candidates with
 * one list per user, the outputs and the workspace rule the same.  Lists, ordering (TopKV2, ties -> the lower position in
 * the list, -0 and +0 tie), counts (n_out[i] = min(k, len_i) entries at the head of row i, zeros behind), duplicates (no
 * dedup; k may exceed n_items), empty lists (no error) and the per-user failures -- the WELL-FORMED rule on row_splits with
 * status 3, a row outside [0, n_items) with status 5, a zeroed row for the failed user and no other user's answer changed --
 * are word for word the contract of nann_search_candidates above.
 * l2 / mlp model: nann_user_seq_mean into the head of the workspace, then nann_search_candidates with the model's own scorer
 * (nann_model_scorer) -- the same bits.  Workspace: 4 d bytes per user, rounded up to 256, plus that call's.
 * attention model (NANN_impls/nann/model/model.py:189-233, the model the reference ships): both precisions score from the
 * pre-projected table of the (model, index) pair, found or built as in nann_search_all_model and released behind the call's
 * event; without a table NANN_ERR_CAPACITY (no room in HBM) or NANN_ERR_UNSUPPORTED (preprojection resolves to 0).  Scores
 * are within 1e-5 max(1, |s|) of the oracle and, in both precisions, bit-identical to what nann_search_all_model returns for
 * the same (user, row) -- the same block functions on the same table row; for split-f16 those are the traversal's bits too.
 * Workspace, each part rounded up to 256 bytes: scores f32[n_cand], 16 B per user (the plan), 8 B x (n_users + 1), and the
 * per-user side of ONE CHUNK: min(n_users, 128) x 80 KB (kt 64 KB + upad 16 KB per user).  The per-user side is bounded: the
 * users are processed in chunks of at most 128, a chunk's nann_attn_prepare and scoring launch enqueued one after the other
 * on `stream`, so the workspace never exceeds 4 n_cand + 24 n_users + 10 MB (+ rounding) however many users a call brings.
 * Nothing is launched for: null ix, m or cand, a struct_bytes mismatch, n_users < 0, n_cand < 0, k < 0, rows == NULL with
 * n_cand > 0, row_splits == NULL with n_users > 0, model and index disagreeing on d / dtype, null comm_seq_f16 / out_item_ids /
 * status when there is work, a workspace off the 256-byte grid -> NANN_ERR_BAD_ARGUMENT; k > 1024, n_cand > 2^31 - 1 or
 * n_users > 2^31 - 1 -> NANN_ERR_UNSUPPORTED; a workspace smaller than ..._workspace_bytes() -> NANN_ERR_CAPACITY; n_users == 0
 * or k == 0 -> NANN_OK, nothing written.  A user's answer does not depend on the batch it is in.  Asynchronous on `stream`, no
 * host read-back, re-entrant on shared handles. */
int nann_search_candidates_model_workspace_bytes(const nann_index* ix, const nann_model* m, int64_t n_users, int64_t n_cand,
                                                 int32_t k, int64_t* nbytes);
int nann_search_candidates_model(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_users, int32_t k,
                                 const nann_candidates* cand, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                                 int32_t* out_pos, int32_t* n_out, int32_t* status, void* workspace, int64_t workspace_bytes,
                                 const nann_search_options* options, nann_stream_t stream);

/* ---- multi-vector queries: union top-k over a user's interest vectors --------------------------------------------------
 * A user tower that emits several interest vectors per user (MIND, ComiRec) wants the k best rows by the best score ANY of the
 * user's vectors gives a row.  The reference has no such call; the semantics below are this library's own.
 *
 * nann_union_topk is the step on its own, for result lists from anywhere -- several traversals, a filtered search plus a
 * candidate search, ...: a user brings n_lists lists of k_in (score, row) entries.
 *   scores       f32[n_users, n_lists, k_in];  rows i32, the same shape (internal row numbers)
 *   n_valid      i32[n_users, n_lists], or NULL = k_in everywhere: only the first clamp(n_valid[u][l], 0, k_in) entries of list
 *                l count (a filtered call's n_out, a candidate call's n_out)
 *   n_items      rows outside [0, n_items) are dropped;  item_ids device i64[n_items], or NULL
 *   out_index    i32[n_users, k], required;  out_scores f32, out_item_ids i64 (= item_ids[out_index], needs item_ids), out_list
 *                i32 (the list l the entry came from: "which interest retrieved this"), each [n_users, k], n_out i32[n_users]
 *                -- each may be NULL
 *   workspace    device, 256-byte aligned, nann_union_topk_workspace_bytes(...) bytes: 8 B per entry
 * Entry p = l * k_in + j of a user is VALID iff j < clamp(n_valid[u][l], 0, k_in) and its row lies in [0, n_items); anything
 * else is dropped, malformed input never faults.  Among the valid entries that share a row the REPRESENTATIVE is the one with
 * the largest score (-0 and +0 tie), ties -> the lowest p; every other entry of the row is deleted.  The answer is TopKV2 over
 * the representatives taken in ascending p: score descending, ties -> the lower p.  n_out[u] = min(k, distinct valid rows)
 * entries at the head of row u of every output, zeros behind.  NaN scores stay outside the contract, as for nann_topk; -inf is
 * a score like any other.  Limits: n_lists * k_in <= NANN_UNION_MAX_IN, k <= 1024.
 * Nothing is launched for: a negative n_users, n_lists, k_in, n_items or k, k > n_lists * k_in, out_item_ids without item_ids,
 * null scores / rows / out_index when there is work, a workspace off the 256-byte grid -> NANN_ERR_BAD_ARGUMENT; k > 1024,
 * n_lists * k_in > NANN_UNION_MAX_IN, n_items or n_users > 2^31 - 1 -> NANN_ERR_UNSUPPORTED; a workspace smaller than
 * nann_union_topk_workspace_bytes() -> NANN_ERR_CAPACITY; n_users == 0 or k == 0 -> NANN_OK, nothing written.  (Where
 * several apply: the sizes and k first, their NANN_ERR_BAD_ARGUMENT before their NANN_ERR_UNSUPPORTED, then the early
 * NANN_OK, then the null pointers, out_item_ids without item_ids, the workspace's size, its alignment.)  nann_union_topk_workspace_bytes leaves
 * *nbytes untouched when it fails.  A user's answer does not depend on the batch it is in.  Asynchronous on `stream`, no host
 * read-back. */
#define NANN_UNION_MAX_IN 8192
int nann_union_topk_workspace_bytes(int64_t n_users, int32_t n_lists, int32_t k_in, int64_t* nbytes);
int nann_union_topk(const float* scores, const int32_t* rows, const int32_t* n_valid, int64_t n_users, int32_t n_lists,
                    int32_t k_in, int64_t n_items, const int64_t* item_ids, int32_t k, int32_t* out_index, float* out_scores,
                    int64_t* out_item_ids, int32_t* out_list, int32_t* n_out, void* workspace, int64_t workspace_bytes,
                    nann_stream_t stream);

/* The traversal form: q is f32[n_users, n_vec, d], n_vec interest vectors per user.  The inner search is nann_search_opt,
 * unchanged, over the n_users * n_vec vectors as queries at the fetch width F = level_topn_max[5], into a staging area of the
 * workspace (16 B x F per vector, counted by nann_search_multi_workspace_bytes); level_topn, optional, is device
 * i32[n_users * n_vec, 6], per VECTOR.  Then the union above with list l of user u = what vector (u, l) returned: its own
 * level_topn[..][5] entries, or none when status[u][l] != 0.
 *   status       i32[n_users, n_vec], required: what the inner search reports per vector.  A failed vector contributes nothing;
 *                the user still gets the union of the vectors that succeeded
 *   out_item_ids i64[n_users, k], required;  out_scores f32, out_index i32, out_vec i32 (the vector an entry came from), each
 *                [n_users, k], n_out i32[n_users] -- each may be NULL
 *   counters     i32[n_users * n_vec, 3, NANN_NUM_ROUNDS] or NULL, options, plan: the inner search's
 *   workspace    device, 256-byte aligned (else NANN_ERR_BAD_ARGUMENT); smaller than ..._workspace_bytes -> NANN_ERR_CAPACITY
 * Every scorer nann_search_opt accepts is accepted: L2, the inner product, the MLP in every precision; a returned score has the
 * bits nann_search_opt returns for that (vector, row).  n_vec < 1, k outside [0, n_vec * F] -> NANN_ERR_BAD_ARGUMENT; n_vec * F >
 * NANN_UNION_MAX_IN or k > 1024 -> NANN_ERR_UNSUPPORTED; these, the null pointers and the workspace are looked at before
 * anything is launched.  n_users == 0 or k == 0 -> NANN_OK behind those shape checks, nothing launched and nothing written,
 * status included, as in nann_union_topk.  A user with fewer than n_vec interests repeats one of them: duplicates collapse, the answer is that of
 * the distinct vectors.  Filters compose from the parts: nann_search_filtered over the n_users * n_vec vectors, then
 * nann_union_topk with n_valid = its n_out.  There is no _model form: a comm_seq is ONE user sequence, which a model turns into
 * one query (l2 / mlp: its mean) or scores as a whole (attention); several interest vectors come from the caller's user tower, or from that sequence through
 * nann_user_seq_interests. */
int nann_search_multi_workspace_bytes(const nann_index* ix, const int32_t level_topn[6] /*[host]*/, int64_t n_users,
                                      int32_t n_vec, int64_t* nbytes);
int nann_search_multi(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_users, int32_t n_vec,
                      const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace, int64_t workspace_bytes,
                      int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* out_vec, int32_t* n_out,
                      int32_t* status, int32_t* counters, const nann_search_options* options, nann_search_plan* plan, int32_t k,
                      nann_stream_t stream);

/* The exhaustive form, the ground truth of multi-vector recall: nann_search_all over the n_users * n_vec vectors at k, then the
 * union of each user's n_vec lists.  The union of per-vector top-k lists is EXACT: let b(r) = max_m s(q_m, r) be a row's best
 * score and r a row whose b(r) is among the k largest; with m the vector that attains b(r), any row r' ahead of r in vector
 * m's order has s(q_m, r') >= b(r), hence b(r') >= b(r), and fewer than k rows can be ahead of r under the total order -- so r
 * stands in vector m's top k with its best score, and the returned score values are the k largest of max_m s(q_m, r).  (Among
 * rows that tie at the k-th value, which ones are returned follows the union's position rule.)
 * Checks: nann_search_all's -- k > n_items -> NANN_ERR_TOPK_K_GT_N, k > 1024 -> NANN_ERR_UNSUPPORTED, ... -- and n_vec < 1 ->
 * NANN_ERR_BAD_ARGUMENT, n_vec * k > NANN_UNION_MAX_IN -> NANN_ERR_UNSUPPORTED; n_users == 0 or k == 0 -> NANN_OK, nothing
 * written.  out_item_ids i64[n_users, k] is required; out_scores, out_index, out_vec, n_out (always min(k, n_items) = k) may be
 * NULL.  No _model form, as above. */
int nann_search_all_multi_workspace_bytes(const nann_index* ix, const nann_scorer* scorer, int64_t n_users, int32_t n_vec,
                                          int32_t k, int64_t* nbytes);
int nann_search_all_multi(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_users, int32_t n_vec,
                          int32_t k, int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* out_vec,
                          int32_t* n_out, void* workspace, int64_t workspace_bytes, const nann_search_options* options,
                          nann_stream_t stream);

/* ---- group caps: at most m rows per group in every top-k ----------------------------------------------------------------
 * "At most 2 items of one seller", "at most 3 of one category", "one per brand" among the k rows a query returns.  The
 * reference has no such call; the semantics below are this library's own.
 *
 * A GROUPING is group_of_row, device i32[n_items]: the group id of every internal row.  An id >= 0 can be any value and there
 * can be any number of distinct ids; a negative id means UNGROUPED: the row is never capped and never counts against anything.
 * A CAP m >= 1 applies to every query, or caps, device i32[n_queries], gives one cap per query; caps[i] <= 0: query i is
 * uncapped.
 *
 * The input per query is a RANKED list of k_in (row, score) entries.  Entry j is VALID iff j < clamp(n_valid[i], 0, k_in), its
 * row lies in [0, n_items) and it is not denied by the nann_filter where one is given; anything else is dropped, malformed
 * input never faults.  Walking the valid entries in ascending j, an entry is KEPT iff its group g is negative, or fewer than m
 * valid entries before it have group g -- equivalently, its rank among the valid entries of its group is < m.  Denied and
 * invalid entries use no quota ("filter first, then cap").  A row that appears twice counts twice: there is no dedup, that is
 * nann_union_topk's job.  The answer is the first k kept entries with their order unchanged: n_out[i] entries at the head of
 * row i of every output, zeros behind.  Scores are carried through, never recomputed and never compared: NaN and -inf are
 * scores like any other here.
 *
 * PREFIX PROPERTY: for any F' >= F, the capped list over the first F entries is a prefix of the capped list over the first
 * F'.  Proof: whether entry j is valid and kept depends only on entries 0 .. j, so both walks decide every j < F alike; the
 * walk over F' only appends entries j >= F behind them.  Two consequences: a query with n_out == k has the exact answer over
 * the full ranking; a query with n_out < k was cut short by F, unless the list held every valid row -- the host sees this from
 * n_out and widens F.  A query's answer does not depend on the batch it is in. */
typedef struct {
  int32_t struct_bytes;          /* 0 or sizeof(nann_groups) */
  const int32_t* group_of_row;   /* device i32[n_items]; < 0 = ungrouped */
  int32_t cap;                   /* >= 1 when caps is NULL */
  const int32_t* caps;           /* device i32[n_queries] or NULL; caps[i] <= 0: query i uncapped */
} nann_groups;

/* The step on its own, for ranked lists from anywhere: a union's output, a candidate search's, another shard's.
 *   scores       f32[n_queries, k_in], or NULL (out_scores then holds zeros);  rows i32[n_queries, k_in] (internal row numbers)
 *   n_valid      i32[n_queries], or NULL = k_in everywhere (a filtered / union / candidate call's n_out)
 *   n_items      rows outside [0, n_items) are dropped;  item_ids device i64[n_items], or NULL
 *   groups       required;  filter optional (its exclusion lists are by the query number of THIS call)
 *   out_index    i32[n_queries, k], required;  out_scores f32, out_item_ids i64 (= item_ids[out_index], needs item_ids),
 *                out_group i32 (the group id of each returned row), out_pos i32 (the position j in the input list), each
 *                [n_queries, k], n_out i32[n_queries] -- each may be NULL
 * No workspace.  Limits: k_in <= 1024, 0 <= k <= k_in.
 * Nothing is launched and nothing written for: a negative n_queries, k_in, n_items or k, k > k_in, a null groups, a bad
 * groups->struct_bytes, a null group_of_row, cap < 1 with caps == NULL, a malformed filter, out_item_ids without item_ids, null
 * rows / out_index when there is work -> NANN_ERR_BAD_ARGUMENT; k_in > 1024, n_items or n_queries > 2^31 - 1 ->
 * NANN_ERR_UNSUPPORTED; n_queries == 0 or k == 0 -> NANN_OK, nothing written.  (Where several apply: the sizes and k first,
 * their NANN_ERR_BAD_ARGUMENT before their NANN_ERR_UNSUPPORTED, then the groups, then the early NANN_OK, then the null
 * pointers, out_item_ids without item_ids, the filter.)  None of these checks touches the device.  Asynchronous on `stream`,
 * no host read-back. */
int nann_group_cap_topk(const float* scores, const int32_t* rows, const int32_t* n_valid, int64_t n_queries, int32_t k_in,
                        int64_t n_items, const int64_t* item_ids, const nann_groups* groups, const nann_filter* filter, int32_t k,
                        int32_t* out_index, float* out_scores, int64_t* out_item_ids, int32_t* out_group, int32_t* out_pos,
                        int32_t* n_out, nann_stream_t stream);

/* The traversal forms: the arguments of nann_search_filtered / nann_search_model_filtered plus the groups and out_group
 * (i32[n_queries, k] or NULL); the filter may be NULL.  The inner search is nann_search_opt / nann_search_model_opt,
 * unchanged, at the fetch width F = level_topn_max[5] into the staging area a filtered call has -- the workspace is that of
 * the filtered call -- and the cap runs over what it returned: a query's own level_topn[5] entries, none when status[i] != 0.
 * status, counters, plan, nann_search_reruns and nann_search_refined are the inner search's.  A failed query gets n_out = 0
 * and zeros.  k outside [0, F], a null groups / group_of_row, a bad struct_bytes, cap < 1 with caps == NULL ->
 * NANN_ERR_BAD_ARGUMENT, in front of the first launch; a short workspace -> NANN_ERR_CAPACITY.  n_queries == 0 -> NANN_OK.  By
 * the prefix property a query with n_out == k has the capped answer over the traversal's whole ranking. */
int nann_search_grouped_workspace_bytes(const nann_index* ix, const int32_t level_topn[6] /*[host]*/, int64_t n_queries,
                                        int64_t* nbytes);
int nann_search_grouped(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries,
                        const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace, int64_t workspace_bytes,
                        int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* status, int32_t* counters,
                        int64_t* phase_ticks, const nann_search_options* options, nann_search_plan* plan,
                        const nann_filter* filter, const nann_groups* groups, int32_t k, int32_t* out_group, int32_t* n_out,
                        nann_stream_t stream);
int nann_search_model_grouped_workspace_bytes(const nann_index* ix, const nann_model* m, const int32_t level_topn[6],
                                              int64_t n_queries, int64_t* nbytes);
int nann_search_model_grouped(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_queries,
                              const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace,
                              int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                              int32_t* status, int32_t* counters, const nann_search_options* options, nann_search_plan* plan,
                              const nann_filter* filter, const nann_groups* groups, int32_t k, int32_t* out_group,
                              int32_t* n_out, nann_stream_t stream);

/* The exhaustive forms: the arguments of nann_search_all_filtered / nann_search_all_model_filtered plus the fetch width and the
 * groups; the filter may be NULL.  F = fetch, 0 <= k <= fetch (else NANN_ERR_BAD_ARGUMENT).  The inner call is the existing
 * filtered exhaustive search at k = F, with nann_search_all's checks applied to F: fetch > 1024 -> NANN_ERR_UNSUPPORTED, fetch >
 * n_items -> NANN_ERR_TOPK_K_GT_N.  It writes into a staging list in the workspace (16 B x F per query, plus its n_out), and
 * the cap runs over that list's n_out entries.  By the prefix property this is the ground truth of the traversal form
 * wherever n_out == k; with fetch = n_items it is the capped answer over the whole ranking of the allowed rows.  A workspace
 * smaller than ..._workspace_bytes -> NANN_ERR_CAPACITY, off the 256-byte grid -> NANN_ERR_BAD_ARGUMENT; n_queries == 0 or k == 0
 * -> NANN_OK, nothing written. */
int nann_search_all_grouped_workspace_bytes(const nann_index* ix, const nann_scorer* scorer, int64_t n_queries, int32_t fetch,
                                            int64_t* nbytes);
int nann_search_all_grouped(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries, int32_t fetch,
                            int32_t k, int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* out_group,
                            void* workspace, int64_t workspace_bytes, const nann_search_options* options,
                            const nann_filter* filter, const nann_groups* groups, int32_t* n_out, nann_stream_t stream);
int nann_search_all_model_grouped_workspace_bytes(const nann_index* ix, const nann_model* m, int64_t n_users, int32_t fetch,
                                                  int64_t* nbytes);
int nann_search_all_model_grouped(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_users,
                                  int32_t fetch, int32_t k, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                                  int32_t* out_group, void* workspace, int64_t workspace_bytes,
                                  const nann_search_options* options, const nann_filter* filter, const nann_groups* groups,
                                  int32_t* n_out, nann_stream_t stream);

/* ---- diversified results: MMR re-ranking of a fetched top-F ---------------------------------------------------------------
 * "Do not return 200 near-copies of the best hit": group caps give diversity by label, this gives it by embedding.  MMR
 * (maximal marginal relevance, Carbonell & Goldstein) picks k of F fetched entries one at a time, each time the entry whose
 * score, weighted by lambda, least resembles what was picked before it.  The reference has no such call; the semantics below
 * are this library's own.
 *
 * The input per query i is a list of k_in (row, score) entries.  Entry j is VALID iff j < clamp(n_valid[i], 0, k_in), its row
 * lies in [0, n_items), its score is finite and -- in the search forms -- the nann_filter does not deny the row; anything else
 * is dropped, malformed input never faults.  A row that appears twice gives two candidates: there is no dedup, that is
 * nann_union_topk's job.
 *
 * PARAMETERS: lambda in [0, 1] for every query (NaN or out of range: NANN_ERR_BAD_ARGUMENT), or lambdas, device
 * f32[n_queries], one per query, a value x read as !(x >= 0) ? 0 : (x > 1 ? 1 : x).  sim: NANN_SCORER_L2 or NANN_SCORER_IP
 * (NANN_SCORER_MLP: NANN_ERR_UNSUPPORTED; any other value: NANN_ERR_BAD_ARGUMENT).  Let a be the query's lambda and
 * b = 1.0f - a.
 *
 * SIMILARITY: sim(j, t) is the canonical score of the chosen metric (L2: -||q - x||^2, IP: <q, x>) with row rows[t] widened
 * exactly to f32 as the query and row rows[j] as the item: the lane sums and the xor butterfly of nann_score, so it is bit for
 * bit what nann_score returns for that pair.
 *
 * SELECTION, all arithmetic f32 and uncontracted: r_j = a * s_j, computed once.  Step 0 picks the valid j with the greatest
 * r_j.  After pick t the penalty updates: p_j = sim(j, t) after the first pick, afterwards p_j = (sim(j, t) > p_j) ?
 * sim(j, t) : p_j.  Step n >= 1 picks, among the valid unpicked j, the greatest v_j = r_j - (b * p_j).  "Greatest" is by the
 * key of TopKV2's order here: x + 0.0f, then the monotone u32 map of the bits; ties go to the lower j.  Selection stops after
 * n_out = min(k, #valid) picks.  Every output is filled in pick order, zeros behind.
 *
 * CONSEQUENCES: with lambda == 1 the answer is the valid entries in (score descending, position ascending) order -- on a
 * ranked list, the input's prefix.  A query's answer does not depend on the batch it is in.  The answer is MMR over the F
 * entries given, not over the whole table, and there is NO PREFIX PROPERTY: the picks over the first F entries need not begin
 * the picks over the first F' > F, and n_out == k says nothing about a wider fetch. */
typedef struct {
  int32_t struct_bytes;   /* 0 or sizeof(nann_diversity) */
  float lambda;           /* in [0, 1]: 1 = relevance only, 0 = the first entry, then the farthest rows */
  const float* lambdas;   /* device f32[n_queries] or NULL; clamped per query as above */
  int32_t sim;            /* NANN_SCORER_L2 | NANN_SCORER_IP */
} nann_diversity;

/* The step on its own, for lists from anywhere.  From ix it reads the table, d, the row dtype, n_items and item_ids.
 *   scores       f32[n_queries, k_in];  rows i32[n_queries, k_in] (internal row numbers)
 *   n_valid      i32[n_queries], or NULL = k_in everywhere (a filtered / union / candidate call's n_out)
 *   out_index    i32[n_queries, k], required;  out_scores f32 (the ORIGINAL s_j, carried through), out_mmr f32 (r_j at step
 *                0, v_j after), out_pos i32 (the picked j), out_item_ids i64 (= item_ids[out_index]), each [n_queries, k],
 *                n_out i32[n_queries] -- each may be NULL
 * No workspace.  Limits: k_in <= 1024, 0 <= k <= k_in.
 * Nothing is launched and nothing written for: a negative n_queries, k_in or k, k > k_in, a null diversity, a bad
 * diversity->struct_bytes, a sim that is no scorer kind, a lambda outside [0, 1] or NaN, null ix / scores / rows / out_index
 * when there is work -> NANN_ERR_BAD_ARGUMENT; k_in > 1024, n_queries > 2^31 - 1, sim == NANN_SCORER_MLP, an index whose d is
 * not 64 / 128 / 256 / 512 -> NANN_ERR_UNSUPPORTED; n_queries == 0 or k == 0 -> NANN_OK, nothing written.  (Where several
 * apply: the sizes and k first, their NANN_ERR_BAD_ARGUMENT before their NANN_ERR_UNSUPPORTED, then the diversity -- null,
 * struct_bytes, sim, lambda --, then the early NANN_OK, then the null pointers, and last the index, which nothing before it
 * reads.)  None of these checks touches the device.  Asynchronous on `stream`, no host read-back. */
int nann_mmr_topk(const nann_index* ix, const float* scores, const int32_t* rows, const int32_t* n_valid, int64_t n_queries,
                  int32_t k_in, const nann_diversity* diversity, int32_t k, int32_t* out_index, float* out_scores,
                  float* out_mmr, int32_t* out_pos, int64_t* out_item_ids, int32_t* n_out, nann_stream_t stream);

/* The traversal forms: the arguments of nann_search_filtered / nann_search_model_filtered plus the diversity and out_mmr /
 * out_pos (f32 / i32 [n_queries, k] or NULL); the filter may be NULL.  The inner search is nann_search_opt /
 * nann_search_model_opt, unchanged, at the fetch width F = level_topn_max[5] into the staging area a filtered call has -- the
 * workspace is that of the filtered call -- and MMR runs over what it returned: a query's own level_topn[5] entries without
 * the rows the filter denies, none when status[i] != 0.  out_pos is the position in that fetched list.  status, counters,
 * plan, nann_search_reruns and nann_search_refined are the inner search's.  A failed query gets n_out = 0 and zeros.  k
 * outside [0, F], a null diversity, a bad struct_bytes, sim or lambda -> as above, in front of the first launch; a short
 * workspace -> NANN_ERR_CAPACITY.  n_queries == 0 -> NANN_OK.  The similarity is over the index's rows whatever scored them:
 * under an MLP scorer or an attention model choose the metric the embeddings were trained for. */
int nann_search_diverse_workspace_bytes(const nann_index* ix, const int32_t level_topn[6] /*[host]*/, int64_t n_queries,
                                        int64_t* nbytes);
int nann_search_diverse(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries,
                        const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace, int64_t workspace_bytes,
                        int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* status, int32_t* counters,
                        int64_t* phase_ticks, const nann_search_options* options, nann_search_plan* plan,
                        const nann_filter* filter, const nann_diversity* diversity, int32_t k, float* out_mmr, int32_t* out_pos,
                        int32_t* n_out, nann_stream_t stream);
int nann_search_model_diverse_workspace_bytes(const nann_index* ix, const nann_model* m, const int32_t level_topn[6],
                                              int64_t n_queries, int64_t* nbytes);
int nann_search_model_diverse(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_queries,
                              const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace,
                              int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                              int32_t* status, int32_t* counters, const nann_search_options* options, nann_search_plan* plan,
                              const nann_filter* filter, const nann_diversity* diversity, int32_t k, float* out_mmr,
                              int32_t* out_pos, int32_t* n_out, nann_stream_t stream);

/* The exhaustive forms: the arguments of nann_search_all_filtered / nann_search_all_model_filtered plus the fetch width and the
 * diversity; the filter may be NULL.  F = fetch, 0 <= k <= fetch (else NANN_ERR_BAD_ARGUMENT).  The inner call is the existing
 * filtered exhaustive search at k = F, with nann_search_all's checks applied to F as in nann_search_all_grouped: fetch > 1024
 * -> NANN_ERR_UNSUPPORTED, fetch > n_items -> NANN_ERR_TOPK_K_GT_N.  It writes into a staging list in the workspace (16 B x F
 * per query, plus its n_out), and MMR runs over that list's n_out entries: the exact top F of the allowed rows, re-ranked.  A
 * workspace smaller than ..._workspace_bytes -> NANN_ERR_CAPACITY, off the 256-byte grid -> NANN_ERR_BAD_ARGUMENT;
 * n_queries == 0 or k == 0 -> NANN_OK, nothing written. */
int nann_search_all_diverse_workspace_bytes(const nann_index* ix, const nann_scorer* scorer, int64_t n_queries, int32_t fetch,
                                            int64_t* nbytes);
int nann_search_all_diverse(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries, int32_t fetch,
                            int32_t k, int64_t* out_item_ids, float* out_scores, int32_t* out_index, float* out_mmr,
                            int32_t* out_pos, void* workspace, int64_t workspace_bytes, const nann_search_options* options,
                            const nann_filter* filter, const nann_diversity* diversity, int32_t* n_out, nann_stream_t stream);
int nann_search_all_model_diverse_workspace_bytes(const nann_index* ix, const nann_model* m, int64_t n_users, int32_t fetch,
                                                  int64_t* nbytes);
int nann_search_all_model_diverse(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_users,
                                  int32_t fetch, int32_t k, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                                  float* out_mmr, int32_t* out_pos, void* workspace, int64_t workspace_bytes,
                                  const nann_search_options* options, const nann_filter* filter,
                                  const nann_diversity* diversity, int32_t* n_out, nann_stream_t stream);

/* ---- attribute predicates: per-query label, range and tag conditions -------------------------------------------------------
 * "Only rows of category 7 or 12 for this user", "price between this user's bounds", "in stock in this user's region, and not
 * adult": a condition on ROW ATTRIBUTES that differs from query to query.  The deny bitmap of a nann_filter is one for the whole
 * batch, and an exclusion list would have to name every row that fails.  The reference has no such feature; the semantics below
 * are this library's own.
 *
 * A nann_predicates is a plain struct, passed per call and BORROWED for the call, as nann_filter and nann_groups are.  Row
 * attributes, each a device array of n_items entries or NULL: label_of_row (i32), value_of_row (f32), tags_of_row (u64: a set of
 * up to 64 tags).  Per-query conditions, each by the query number of the call:
 *   labels  query i allows the labels labels[label_splits[i] .. label_splits[i + 1]): any order, duplicates allowed, any number.
 *           The range is clamped to [0, n_labels]; an empty or inverted range means NO label test for that query
 *   value   the row passes iff value_lo[i] <= value_of_row[r] <= value_hi[i], compared as IEEE does: a NaN row value or a NaN
 *           bound passes nothing; a NULL side is unbounded; lo > hi is how a caller says "match nothing"
 *   tags    with t = tags_of_row[r] the row passes iff (t & all) == all, any == 0 || (t & any) != 0, and (t & none) == 0; a
 *           NULL array reads as zeros
 * A row PASSES query i iff every test that is present passes: the tests are ANDed with each other and with the nann_filter
 * where one is given.  NULL, or a struct without any per-query condition, passes every row.
 * Argument errors, all NANN_ERR_BAD_ARGUMENT: struct_bytes other than 0 or sizeof(nann_predicates); a per-query condition
 * without its attribute column (label_splits without label_of_row, value_lo / value_hi without value_of_row, tags_all /
 * tags_any / tags_none without tags_of_row); n_labels < 0; label_splits without labels while n_labels > 0.  All checks run in
 * front of the first launch and none touches the device; the four search calls below look at the struct before any other
 * argument, so a malformed one is refused whatever the handles and also for an empty batch.  Malformed device contents never fault. */
typedef struct {
  int32_t struct_bytes;             /* 0 or sizeof(nann_predicates) */
  const int32_t* label_of_row;      /* device i32[n_items], or NULL */
  const float* value_of_row;        /* device f32[n_items], or NULL */
  const uint64_t* tags_of_row;      /* device u64[n_items], or NULL */
  const int64_t* label_splits;      /* device i64[n_queries + 1], or NULL */
  const int32_t* labels;            /* device i32[n_labels] */
  int64_t n_labels;
  const float* value_lo;            /* device f32[n_queries] each, or NULL */
  const float* value_hi;
  const uint64_t* tags_all;         /* device u64[n_queries] each, or NULL */
  const uint64_t* tags_any;
  const uint64_t* tags_none;
} nann_predicates;

/* The step on its own, for ranked lists from anywhere: the arguments of nann_group_cap_topk without the groups.  Entry j of
 * query i is VALID iff j < clamp(n_valid[i], 0, k_in) and its row lies in [0, n_items); the answer is the first k valid entries
 * that pass the predicates and the filter, order kept: n_out[i] of them at the head of row i of every output, zeros behind.
 * Scores are carried through, never compared; a row that stands twice is judged twice.  Usage: a union's output filtered by
 * predicate and handed on to nann_group_cap_topk through n_valid = this call's n_out.
 *   out_index i32[n_queries, k] is required; out_scores f32, out_item_ids i64 (needs item_ids), out_pos i32 (the position j in
 *   the input list), n_out i32[n_queries] may be NULL.  No workspace.  Limits: k_in <= 1024, 0 <= k <= k_in.
 * Checks as nann_group_cap_topk's, with the predicates in the place of the groups (NULL: none), in front of the first launch. */
int nann_predicate_topk(const float* scores, const int32_t* rows, const int32_t* n_valid, int64_t n_queries, int32_t k_in,
                        int64_t n_items, const int64_t* item_ids, const nann_predicates* predicates, const nann_filter* filter,
                        int32_t k, int32_t* out_index, float* out_scores, int64_t* out_item_ids, int32_t* out_pos, int32_t* n_out,
                        nann_stream_t stream);

/* The SELECTIVITY: out_counts[i] (device i64[n_queries]) = rows of [0, n_items) that pass query i's predicates and the filter.
 * It tells a caller whether a traversal at fetch width F can fill k -- about F x count / n_items of the fetched rows pass -- or
 * the exhaustive form is the one to call.  A row an exclusion list names twice counts once.  Negative sizes, a malformed
 * struct, a null out_counts while n_queries > 0 -> NANN_ERR_BAD_ARGUMENT; n_items > 2^31 - 1 -> NANN_ERR_UNSUPPORTED.
 * Asynchronous on `stream`, no host read-back. */
int nann_predicate_count(int64_t n_items, const nann_predicates* predicates, const nann_filter* filter, int64_t n_queries,
                         int64_t* out_counts, nann_stream_t stream);

/* The traversal forms: nann_search_filtered / nann_search_model_filtered plus the predicates, with the same fetch-width
 * contract: the inner search is nann_search_opt / nann_search_model_opt, unchanged, at F = level_topn_max[5]; the answer is the
 * first k passing entries of what the unchanged traversal returns at F, order kept.  The workspace is that of the filtered
 * call.  n_out[i] < k means the list was cut short: widen F, or take the exhaustive form.  A failed query (status[i] != 0)
 * gets n_out = 0 and zeros.  Rows that fail still guide the walk. */
int nann_search_where_workspace_bytes(const nann_index* ix, const int32_t level_topn[6] /*[host]*/, int64_t n_queries,
                                      int64_t* nbytes);
int nann_search_where(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries,
                      const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace, int64_t workspace_bytes,
                      int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* status, int32_t* counters,
                      int64_t* phase_ticks, const nann_search_options* options, nann_search_plan* plan,
                      const nann_filter* filter, const nann_predicates* predicates, int32_t k, int32_t* n_out,
                      nann_stream_t stream);
int nann_search_model_where_workspace_bytes(const nann_index* ix, const nann_model* m, const int32_t level_topn[6],
                                            int64_t n_queries, int64_t* nbytes);
int nann_search_model_where(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_queries,
                            const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace,
                            int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                            int32_t* status, int32_t* counters, const nann_search_options* options, nann_search_plan* plan,
                            const nann_filter* filter, const nann_predicates* predicates, int32_t k, int32_t* n_out,
                            nann_stream_t stream);

/* The exhaustive forms: nann_search_all_filtered / nann_search_all_model_filtered plus the predicates -- the same arguments,
 * checks, error codes and workspace.  The top k over the PASSING rows is exact, in TopKV2 order (descending, ties -> lower row):
 * n_out[i] = min(k, passing rows of query i) wherever the passing rows score above -inf -- the -inf caveat of the filtered call:
 * failing rows are taken out by writing -inf over their scores between scoring and selection.  Scores are bit-identical to
 * nann_search_all for the same (query, row), and a query's answer does not depend on its batch. */
int nann_search_all_where_workspace_bytes(const nann_index* ix, const nann_scorer* scorer, int64_t n_queries, int32_t k,
                                          int64_t* nbytes);
int nann_search_all_where(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries, int32_t k,
                          int64_t* out_item_ids, float* out_scores, int32_t* out_index, void* workspace,
                          int64_t workspace_bytes, const nann_search_options* options, const nann_filter* filter,
                          const nann_predicates* predicates, int32_t* n_out, nann_stream_t stream);
int nann_search_all_model_where_workspace_bytes(const nann_index* ix, const nann_model* m, int64_t n_users, int32_t k,
                                                int64_t* nbytes);
int nann_search_all_model_where(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_users,
                                int32_t k, int64_t* out_item_ids, float* out_scores, int32_t* out_index, void* workspace,
                                int64_t workspace_bytes, const nann_search_options* options, const nann_filter* filter,
                                const nann_predicates* predicates, int32_t* n_out, nann_stream_t stream);

/* ---- fused result lists: reciprocal rank fusion and weighted score fusion ----------------------------------------------------
 * nann_union_topk keeps each row's BEST score: "any of my interests likes this row".  Hybrid retrieval -- a list from the L2
 * traversal, one from the attention model, a lexical one from outside, each on its own scale -- and consensus over interest
 * vectors want a score ACCUMULATED over the lists that contain a row instead.  The reference has no such call; the semantics
 * below are this library's own.
 *
 * nann_fuse_topk is the step on its own: a user brings n_lists lists of k_in (score, row) entries, as for nann_union_topk, whose
 * arguments these are, plus the fusion and with out_lists in the place of out_list.
 *   scores       f32[n_users, n_lists, k_in];  rows i32, the same shape (internal row numbers)
 *   n_valid      i32[n_users, n_lists], or NULL = k_in everywhere
 *   n_items      rows outside [0, n_items) are dropped;  item_ids device i64[n_items], or NULL
 *   fusion       required: the mode, the RRF constant and the weights -- device f32[n_lists] for a per-call weight
 *                (weights_per_user == 0, w = weights[l]) or f32[n_users, n_lists] for a per-user weight (w = weights[u *
 *                n_lists + l]); NULL means 1.0f.  Weights are used as given: negative and zero weights included, no host read-back
 *   out_index    i32[n_users, k], required;  out_scores f32 (the fused score), out_item_ids i64 (= item_ids[out_index], needs
 *                item_ids), out_lists u64 (bit l is set iff list l contains the row: "which retrievers found this"; this is
 *                why n_lists <= NANN_FUSE_MAX_LISTS = 64), each [n_users, k], n_out i32[n_users] -- each may be NULL
 *   workspace    device, 256-byte aligned, nann_fuse_topk_workspace_bytes(...) bytes: 24 B per entry
 * VALIDITY.  Entry p = l * k_in + j of a user is VALID iff j < clamp(n_valid[u][l], 0, k_in) and its row lies in [0, n_items);
 * no n_valid means k_in; in the search forms a list whose status word is non-zero counts as 0 entries.  Anything else is
 * dropped; malformed input never faults.
 * OCCURRENCES AND RANK.  Within one list a row COUNTS ONCE, at its lowest valid j; later entries of the same row in that list
 * are ignored.  The rank of a counting entry is its position j, whether or not the entries before it are valid.
 * THE TERM of list l for a row it contains, with s the counting entry's score and w the list's weight.  Every step is a single
 * f32 operation; there is no FMA contraction:
 *   NANN_FUSE_SUM        w * s
 *   NANN_FUSE_SUM_FLOOR  w * (s - lo_l)
 *   NANN_FUSE_MINMAX     w * ((s - lo_l) / (hi_l - lo_l)); where hi_l == lo_l the quotient is read as 1.0f
 *   NANN_FUSE_RRF        w / (rrf_c + (float)(j + 1)): one add, one IEEE division
 * lo_l and hi_l are the least and greatest valid score of list l for this user (every valid entry, counting or not), compared
 * as TopKV2 compares scores, with -0 read as +0.  In NANN_FUSE_SUM_FLOOR every list is shifted so that its floor is 0, and a
 * list that does not hold a row then rightly adds nothing: this is what makes a sum of L2 scores usable -- they are negative,
 * and a missing list must not look better than a present one.  The score returned in that mode is the margin over the floors,
 * not a sum of the scores.
 * THE FUSED SCORE starts from +0.0f and takes the terms of the lists that contain the row in ascending l, one f32 add each; a
 * list that does not contain the row adds nothing.  The order of the additions is fixed, so the result is reproducible bit for bit.
 * THE ANSWER is TopKV2 over the distinct valid rows, taken in ascending order of each row's lowest valid p: fused score
 * descending (-0 and +0 tie), ties -> the lower first p.  n_out[u] = min(k, distinct valid rows) entries at the head of row u
 * of every output, zeros behind.  A user's answer does not depend on the batch it is in.
 * OUTSIDE THE CONTRACT: NaN scores or weights; +-inf scores under NANN_FUSE_SUM_FLOOR and NANN_FUSE_MINMAX; a sum that meets
 * +inf and -inf.  Under NANN_FUSE_SUM and NANN_FUSE_RRF -inf is a score like any other.
 * Limits: n_lists <= NANN_FUSE_MAX_LISTS, n_lists * k_in <= NANN_UNION_MAX_IN, k <= 1024.
 * Nothing is launched and nothing is written by a refused call.  The refusals are nann_union_topk's, in its order (the sizes
 * and k, their NANN_ERR_BAD_ARGUMENT before their NANN_ERR_UNSUPPORTED); then n_lists > 64 -> NANN_ERR_UNSUPPORTED; then the
 * fusion -> NANN_ERR_BAD_ARGUMENT: NULL, a struct_bytes that is neither 0 nor sizeof(nann_fusion), an unknown mode, under
 * NANN_FUSE_RRF an rrf_c that is not a finite value >= 0, weights_per_user outside {0, 1}; then the early NANN_OK for n_users
 * == 0 or k == 0; then the null pointers, out_item_ids without item_ids, the workspace's size (NANN_ERR_CAPACITY), its
 * alignment.  nann_fuse_topk_workspace_bytes leaves *nbytes untouched when it fails.  Asynchronous on `stream`, no host
 * read-back. */
#define NANN_FUSE_MAX_LISTS 64
enum { NANN_FUSE_SUM = 0, NANN_FUSE_SUM_FLOOR = 1, NANN_FUSE_MINMAX = 2, NANN_FUSE_RRF = 3 };
typedef struct nann_fusion {            /* borrowed for the call, like nann_filter */
  int32_t struct_bytes;                 /* 0 or sizeof(nann_fusion) */
  int32_t mode;                         /* NANN_FUSE_SUM | _SUM_FLOOR | _MINMAX | _RRF */
  float   rrf_c;                        /* RRF only; !(rrf_c >= 0) or inf -> NANN_ERR_BAD_ARGUMENT */
  int32_t weights_per_user;             /* 0: weights f32[n_lists]; 1: f32[n_users, n_lists] */
  const float* weights;                 /* device, or NULL = 1.0f */
} nann_fusion;
int nann_fuse_topk_workspace_bytes(int64_t n_users, int32_t n_lists, int32_t k_in, int64_t* nbytes);
int nann_fuse_topk(const float* scores, const int32_t* rows, const int32_t* n_valid, int64_t n_users, int32_t n_lists,
                   int32_t k_in, int64_t n_items, const int64_t* item_ids, int32_t k, const nann_fusion* fusion,
                   int32_t* out_index, float* out_scores, int64_t* out_item_ids, uint64_t* out_lists, int32_t* n_out,
                   void* workspace, int64_t workspace_bytes, nann_stream_t stream);

/* The traversal form: nann_search_multi with the fuse in the place of the union and out_lists (u64[n_users, k], bit m = vector
 * m's list holds the row) in the place of out_vec.  The inner search is nann_search_opt, unchanged, over the n_users * n_vec
 * vectors at the fetch width F = level_topn_max[5]; list l of user u is what vector (u, l) returned, its own level_topn[..][5]
 * entries.  status is per vector, i32[n_users, n_vec]: a failed vector contributes nothing.  Every scorer nann_search_opt
 * takes is accepted.  n_vec < 1, k outside [0, n_vec * F], a malformed fusion -> NANN_ERR_BAD_ARGUMENT; n_vec > 64, n_vec * F
 * > NANN_UNION_MAX_IN or k > 1024 -> NANN_ERR_UNSUPPORTED; these, the null pointers and the workspace are looked at before
 * anything is launched; n_users == 0 or k == 0 -> NANN_OK behind them, nothing launched and nothing written.
 * Unlike the union, fusion over truncated lists has no exactness property: a row beyond depth F (here) or `fetch` (below) in a
 * list loses that list's term, so the depth is the caller's trade-off between cost and how far down a list agreement is still
 * seen.  A weighted NANN_FUSE_SUM of inner-product scores of several vectors equals ONE query with the weighted sum of the
 * vectors; the multi forms are for NANN_FUSE_RRF, NANN_FUSE_MINMAX and the MLP scorer.  There are no _model forms, for the
 * reason the union section gives: a comm_seq is one user sequence. */
int nann_search_multi_fused_workspace_bytes(const nann_index* ix, const int32_t level_topn[6] /*[host]*/, int64_t n_users,
                                            int32_t n_vec, int64_t* nbytes);
int nann_search_multi_fused(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_users, int32_t n_vec,
                            const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace,
                            int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                            uint64_t* out_lists, int32_t* n_out, int32_t* status, int32_t* counters,
                            const nann_search_options* options, nann_search_plan* plan, int32_t k, const nann_fusion* fusion,
                            nann_stream_t stream);

/* The exhaustive form: nann_search_all over the n_users * n_vec vectors at k = fetch, the per-vector depth, then the fuse of each
 * user's n_vec lists at k.  k outside [0, n_vec * fetch] -> NANN_ERR_BAD_ARGUMENT; the other checks are nann_search_all's, held
 * against fetch (fetch > n_items -> NANN_ERR_TOPK_K_GT_N, fetch > 1024 -> NANN_ERR_UNSUPPORTED, ...), and n_vec < 1 or a
 * malformed fusion -> NANN_ERR_BAD_ARGUMENT, n_vec > 64 or n_vec * fetch > NANN_UNION_MAX_IN -> NANN_ERR_UNSUPPORTED; n_users
 * == 0 or k == 0 -> NANN_OK, nothing written.  out_item_ids i64[n_users, k] is required; out_scores, out_index, out_lists,
 * n_out may be NULL.  `fetch` is the caller's trade-off, as above. */
int nann_search_all_multi_fused_workspace_bytes(const nann_index* ix, const nann_scorer* scorer, int64_t n_users, int32_t n_vec,
                                                int32_t fetch, int64_t* nbytes);
int nann_search_all_multi_fused(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_users, int32_t n_vec,
                                int32_t fetch, int32_t k, const nann_fusion* fusion, int64_t* out_item_ids, float* out_scores,
                                int32_t* out_index, uint64_t* out_lists, int32_t* n_out, void* workspace,
                                int64_t workspace_bytes, const nann_search_options* options, nann_stream_t stream);

/* ---- scalar-quantised exhaustive search: an int8 code table, a wide approximate fetch on the integer matrix cores, an exact
 * re-rank.  Added to ABI version 6: new symbols only.
 * The code of a vector x (a row widened exactly from its 16 bits, or a query's f32 vector), every step ONE IEEE f32 operation,
 * round to nearest:  amax = max_j |x_j|;  scale = amax / 127.0f;  code_j = clamp(rintf(x_j / scale), -127, 127), and scale = 0
 * with every code 0 where amax == 0;  norm = sum_j code_j^2 (i32).  Non-finite inputs are outside the contract.
 * The approximate score of a query (cq, sq, nq) against a row (cx, sx, nx), with the exact integer D = sum_j cq_j cx_j:
 *   NANN_SCORER_IP   s = (sq * sx) * (float)D
 *   NANN_SCORER_L2   a = (sq * sq) * (float)nq,  b = (sx * sx) * (float)nx,  c = ((2 * sq) * sx) * (float)D,  s = c - (a + b)
 * every product, sum and difference one f32 operation; the conversions are exact (|D|, norms <= 127^2 * 512 < 2^24).
 *
 * A nann_sq8 holds codes i8[n_items, d], scales f32[n_items] and norms i32[n_items] of an index's rows in device memory.  It
 * BORROWS the index: the index must outlive it, and a table made before the index's rows were refreshed in place is STALE --
 * re-create it.  The index's rows are f16 or bf16 and d is 64, 128, 256 or 512; an f32-row index -> NANN_ERR_UNSUPPORTED.
 * nann_sq8_create encodes asynchronously on `stream`; nann_sq8_destroy(NULL) is a no-op.
 * nann_sq8_info: out = {n_items, d, device bytes held, 0}.  nann_sq8_view: the three device arrays, borrowed (any may be NULL).
 * nann_sq8_encode: the codes of n f32 vectors of d elements (device arrays in and out), what the search does to its queries. */
typedef struct nann_sq8 nann_sq8;
int nann_sq8_create(const nann_index* ix, nann_stream_t stream, nann_sq8** out);
void nann_sq8_destroy(nann_sq8* t);
int nann_sq8_info(const nann_sq8* t, int64_t out[4] /*[host]*/);
int nann_sq8_view(const nann_sq8* t, const int8_t** codes, const float** scales, const int32_t** norms);
int nann_sq8_encode(const float* x, int64_t n, int32_t d, int8_t* codes, float* scales, int32_t* norms, nann_stream_t stream);

/* The search.  Fetch stage: the `fetch` best rows of every query by APPROXIMATE score, TopKV2 order (ties -> lower row), into
 * out_fetch_index i32[n_queries, fetch] / out_fetch_scores f32[n_queries, fetch] (either may be NULL).  Result: the k best of
 * those rows by EXACT score -- the bits nann_score gives for that (query, row) -- ties -> lower row number, into out_item_ids
 * i64[n_queries, k] (required), out_scores, out_index (may be NULL).  The scorer is NANN_SCORER_L2 or NANN_SCORER_IP; an MLP
 * scorer -> NANN_ERR_UNSUPPORTED.  The checks are nann_search_all's, held against fetch (fetch > n_items -> NANN_ERR_TOPK_K_GT_N,
 * fetch > 1024 -> NANN_ERR_UNSUPPORTED, negative sizes -> NANN_ERR_BAD_ARGUMENT), and k outside [0, fetch] or a table that was
 * not made from `ix` -> NANN_ERR_BAD_ARGUMENT; k == 0 or n_queries == 0 -> NANN_OK, nothing written.  The workspace rule is
 * nann_search_all's (256-byte aligned; smaller than nann_search_all_sq8_workspace_bytes gives -> NANN_ERR_CAPACITY) and its
 * size is bounded by a chunk of queries, not by n_queries.  A query's answer does not depend on its batch.  Asynchronous on
 * `stream`, no host read-back, re-entrant.  The result is the exact top k iff every row of it was fetched: `fetch` is the
 * caller's trade-off between recall and the width of the selection. */
int nann_search_all_sq8_workspace_bytes(const nann_index* ix, const nann_sq8* t, const nann_scorer* scorer, int64_t n_queries,
                                        int32_t fetch, int32_t k, int64_t* nbytes);
int nann_search_all_sq8(const nann_index* ix, const nann_sq8* t, const nann_scorer* scorer, const float* q, int64_t n_queries,
                        int32_t fetch, int32_t k, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                        int32_t* out_fetch_index, float* out_fetch_scores, void* workspace, int64_t workspace_bytes,
                        const nann_search_options* options, nann_stream_t stream);

/* ---- certified scalar-quantised search: nann_search_all's exact bits at the int8 scan's cost.  Added to ABI
 * version 6: new symbols only.
 * A nann_sq8_bounds holds two device arrays over the rows of a code table, each f32[n_items]:
 *   err[i]  >= |x_i - scale_i codes_i|_2 (the real-valued quantisation error of row i)     xhat[i] >= scale_i sqrt(norm_i)
 * both upper bounds by construction (an explicit inflation covers every rounding of their f32 evaluation).  It BORROWS the index
 * and the table, which must outlive it, and goes STALE with the table.  nann_sq8_bounds_create computes asynchronously on
 * `stream`; a table that was not made from `ix` -> NANN_ERR_BAD_ARGUMENT.  nann_sq8_bounds_destroy(NULL) is a no-op.
 * nann_sq8_bounds_view: the two device arrays, borrowed (either may be NULL).
 *
 * nann_search_all_sq8_exact, per query and without a host read-back:
 *   (a) nann_search_all_sq8's fetch stage and exact re-rank at `fetch`; tau = the exact score of the k-th entry, a lower bound of
 *       the true k-th best score;
 *   (b) a pass over the approximate scores of EVERY row keeps the rows whose exact f32 score a rigorous bound cannot put below
 *       tau -- the survivors, ties at tau among them; out_n_survivors[q] = their number, whatever `cap`;
 *   (c) out_certified[q] = 1 iff tau and the query's terms are finite and n_survivors[q] <= cap.  A certified query's outputs are
 *       the exact top k of its survivors: nann_search_all's result BIT FOR BIT -- item ids, scores, index, TopKV2 order with ties
 *       to the lower row.  An uncertified query's outputs are exactly what nann_search_all_sq8 returns at the same fetch.
 * out_item_ids i64[n_queries, k], out_certified i32[n_queries] and out_n_survivors i32[n_queries] are required; out_scores and
 * out_index may be NULL.  Nothing is written beyond a query's k outputs and its two words.
 * The checks are nann_search_all_sq8's (k <= fetch <= min(1024, n_items), an MLP scorer -> NANN_ERR_UNSUPPORTED, ...), and: a NULL
 * bounds object, bounds made from another index or table, or cap < fetch -> NANN_ERR_BAD_ARGUMENT; cap beyond the longest list a
 * candidate-list search takes per query, (2^31 - 1) / (queries per chunk, at most 128) -> NANN_ERR_UNSUPPORTED.  A cap above
 * n_items counts as n_items.  n_queries == 0 or k == 0 -> NANN_OK, nothing written.  Workspace: 256-byte aligned, smaller than
 * nann_search_all_sq8_exact_workspace_bytes gives -> NANN_ERR_CAPACITY; bounded by a chunk of queries (it holds chunk * cap row
 * numbers).  A query's answer does not depend on its batch.  Asynchronous on `stream`, re-entrant.
 * nann_search_all_sq8_exact_layout (tests, tools): out = {queries per chunk, cap as counted, offset of the LAST chunk's final
 * row_splits i64[chunk + 1], of its final lists i32, of its query terms, bytes per query term {tau, eq, qhat, w f32; ok,
 * certified i32; 8 bytes unused}, offset of stage (a)'s scores f32[chunk, k], workspace bytes}. */
typedef struct nann_sq8_bounds nann_sq8_bounds;
int nann_sq8_bounds_create(const nann_index* ix, const nann_sq8* t, nann_stream_t stream, nann_sq8_bounds** out);
void nann_sq8_bounds_destroy(nann_sq8_bounds* b);
int nann_sq8_bounds_view(const nann_sq8_bounds* b, const float** err, const float** xhat);
int nann_search_all_sq8_exact_workspace_bytes(const nann_index* ix, const nann_sq8* t, const nann_sq8_bounds* b,
                                              const nann_scorer* scorer, int64_t n_queries, int32_t fetch, int64_t cap, int32_t k,
                                              int64_t* nbytes);
int nann_search_all_sq8_exact_layout(const nann_index* ix, const nann_sq8* t, const nann_sq8_bounds* b, const nann_scorer* scorer,
                                     int64_t n_queries, int32_t fetch, int64_t cap, int32_t k, int64_t out[8] /*[host]*/);
int nann_search_all_sq8_exact(const nann_index* ix, const nann_sq8* t, const nann_sq8_bounds* b, const nann_scorer* scorer,
                              const float* q, int64_t n_queries, int32_t fetch, int64_t cap, int32_t k, int64_t* out_item_ids,
                              float* out_scores, int32_t* out_index, int32_t* out_certified, int32_t* out_n_survivors,
                              void* workspace, int64_t workspace_bytes, const nann_search_options* options, nann_stream_t stream);

/* ---- certified scalar-quantised RANGE search: nann_search_all_range's exact result from the int8 scan.  Added
 * to ABI version 6: new symbols only.
 * The caller's threshold is the cut, so there is no fetch stage and no top-k.  Per query, without a host read-back:
 *   (a) the int8 scan, and a pass over the approximate scores of EVERY row that keeps the rows whose exact f32 score the bound of
 *       nann_search_all_sq8_exact cannot put below tau = thresholds[q] -- the survivors, rows scoring exactly tau among them;
 *       out_n_survivors[q] = their number, the true count whatever `cap`;
 *   (b) out_certified[q] = 1 iff the threshold and the query's terms are finite and n_survivors[q] <= min(cap, n_items).  A
 *       non-finite threshold (NaN, +inf, -inf) is never certified.
 *       NANN_SCORER_L2 with a finite threshold above +0: out_certified[q] = 1, out_n_survivors[q] = 0 and an empty segment,
 *       whatever the pass counted -- the scorer stores 0.0f - (a sum of squares), so no score exceeds +0 and a NaN score matches
 *       nothing.  A threshold of +0 or -0 takes the normal path;
 *   (c) a certified query's segment is exactly what nann_search_all_range with filter = NULL returns for it: the rows with
 *       score >= threshold and score != -inf, in ascending row order, the scores nann_score's bits, with item ids and index.  An
 *       uncertified query's segment is EMPTY (its count in out_row_splits is 0): the caller sees out_certified[q] == 0 and runs
 *       that query through nann_search_all_range.
 * q, thresholds, capacity and the ragged outputs are nann_search_all_range's, word for word: out_row_splits i64[n_queries + 1]
 * holds the true totals whatever the capacity, a position at or beyond `capacity` is never written, the positions in
 * [min(total, capacity), capacity) are left untouched, capacity == 0 with NULL entry outputs is a count-only call, and a query's
 * segment does not depend on its batch.  out_certified i32[n_queries] and out_n_survivors i32[n_queries] are required.
 * There is NO filter argument: a denied row is marked by a score of -inf, while the survivor pass keeps every row whose
 * approximate score is not finite; combining the two needs an argument of its own.
 * Checks, all in front of the first launch: nann_search_all_range's own; an MLP scorer or an index with f32 rows ->
 * NANN_ERR_UNSUPPORTED; a NULL table or bounds, a table or bounds made from another index or table, cap < 1, or a NULL
 * out_certified / out_n_survivors while n_queries > 0 -> NANN_ERR_BAD_ARGUMENT; cap beyond the longest list a candidate-list search
 * takes per query, (2^31 - 1) / (queries per chunk, at most 128) -> NANN_ERR_UNSUPPORTED; a workspace smaller than
 * nann_search_all_range_sq8_exact_workspace_bytes gives -> NANN_ERR_CAPACITY (256-byte aligned; it holds an f32 and an i32 per
 * (query of a chunk, cap position) and is bounded by a chunk of queries); n_queries == 0 -> NANN_OK, nothing written.  A cap above
 * n_items counts as n_items.  Asynchronous on `stream`, re-entrant. */
int nann_search_all_range_sq8_exact_workspace_bytes(const nann_index* ix, const nann_sq8* t, const nann_sq8_bounds* b,
                                                    const nann_scorer* scorer, int64_t n_queries, int64_t cap, int64_t* nbytes);
int nann_search_all_range_sq8_exact(const nann_index* ix, const nann_sq8* t, const nann_sq8_bounds* b, const nann_scorer* scorer,
                                    const float* q, int64_t n_queries, const float* thresholds, int64_t cap, int64_t capacity,
                                    int64_t* out_row_splits, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                                    int32_t* out_certified, int32_t* out_n_survivors, void* workspace, int64_t workspace_bytes,
                                    const nann_search_options* options, nann_stream_t stream);

/* ---- wide exhaustive search: the exact top k for k up to NANN_WIDE_MAX_K rows per query.  Added to ABI
 * version 6: new symbols only; nann_search_all and every call built on it keep their limit of 1024.
 * nann_search_all_wide / nann_search_all_model_wide take nann_search_all[_model]_where's arguments, checks and check order, with
 * k <= NANN_WIDE_MAX_K in the place of k <= 1024: k < 0 -> NANN_ERR_BAD_ARGUMENT, k > n_items -> NANN_ERR_TOPK_K_GT_N,
 * k > NANN_WIDE_MAX_K -> NANN_ERR_UNSUPPORTED, a NULL q or out_item_ids -> NANN_ERR_BAD_ARGUMENT, a workspace smaller than
 * nann_search_all[_model]_wide_workspace_bytes gives -> NANN_ERR_CAPACITY, one that is not 256-byte aligned ->
 * NANN_ERR_BAD_ARGUMENT; n_queries == 0 or k == 0 -> NANN_OK, nothing written.  Every check stands in front of the first launch,
 * the mean of an l2 / mlp model included.  `filter` and `predicates` may be NULL; out_scores, out_index and n_out may be NULL.
 * Every scorer is served: L2, inner product, the MLP in every precision, l2 / mlp / attention models.
 *   Query i returns the top k of its rows whose score is not -inf, in TopKV2 order: score descending, ties to the lower row, -0
 *   and +0 tie.  n_out[i] = min(k, such rows); the entries behind it are zeros.  A row scoring -inf -- a denied row's mark, or
 *   what the scorer gave -- is never returned: nann_search_all_range's rule.  Scores are nann_search_all's bits for the same
 *   (query, row).  NaN scores are outside the contract.
 * Asynchronous on `stream`, re-entrant, no read-back; a query's answer does not depend on its batch.  The workspace is bounded
 * by a chunk of queries: the scores of the chunk, three histograms and two block counters per query, and a staging list of k
 * (key, row) pairs per query.
 * nann_select_wide is the selection alone over a caller's matrix values f32[n_rows, n_cols] (device, 16-byte aligned): per row,
 * out_values f32[n_rows, k] (may be NULL), out_indices i32[n_rows, k] (column numbers), n_out i32[n_rows] (may be NULL), the same
 * rule.  Any n_cols up to 2^31 - 1 and any n_rows; 0 <= k <= min(n_cols, NANN_WIDE_MAX_K) as above. */
#define NANN_WIDE_MAX_K 16384
int nann_search_all_wide_workspace_bytes(const nann_index* ix, const nann_scorer* scorer, int64_t n_queries, int32_t k,
                                         int64_t* nbytes);
int nann_search_all_wide(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries, int32_t k,
                         int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* n_out, void* workspace,
                         int64_t workspace_bytes, const nann_search_options* options, const nann_filter* filter,
                         const nann_predicates* predicates, nann_stream_t stream);
int nann_search_all_model_wide_workspace_bytes(const nann_index* ix, const nann_model* m, int64_t n_users, int32_t k,
                                               int64_t* nbytes);
int nann_search_all_model_wide(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_users, int32_t k,
                               int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* n_out, void* workspace,
                               int64_t workspace_bytes, const nann_search_options* options, const nann_filter* filter,
                               const nann_predicates* predicates, nann_stream_t stream);
int nann_select_wide_workspace_bytes(int64_t n_rows, int64_t n_cols, int32_t k, int64_t* nbytes);
int nann_select_wide(const float* values, int64_t n_rows, int64_t n_cols, int32_t k, float* out_values, int32_t* out_indices,
                     int32_t* n_out, void* workspace, int64_t workspace_bytes, nann_stream_t stream);

/* ---- 8(f3): the evaluation graph's traversal, one kernel per batch of users ---------------
 * Model.retrieval + search_level (NANN_impls/nann/model.py:299-362), the traversal behind
 * main.py --job-type test: start level scored whole, then levels 1 and 0 with
 * num_scoring_per_level[level] rounds each; neighbours taken as an ascending SET minus visited
 * (tf.unique + tf.sets.difference), top_k = min(k, n), next frontier = new nodes scoring at least
 * the worst kept result, an exhausted frontier is not an error.  Arrays are indexed by level
 * (config.py:50-58); num_scoring_per_level[2] must be 1, top_k_per_level and topk_eval in [1, 2048].
 * Outputs [n_queries, topk_eval] (out_scores / out_index may be NULL); n_out[q] = valid rows of
 * query q (the rest is zero); status[q] as nann_search (NANN_ERR_CAPACITY: more than 2048 new nodes
 * tie at the threshold of a round that is not its level's last).  Bit-identical to oracle_search_eval for the l2 and exact mlp
 * scorers.  workspace: nann_search_eval_workspace_bytes(ix, model or NULL, n_queries).
 * nann_search_eval_model: comm_seq f16[n_queries, seq_len, E] in, as nann_search_model. */
int nann_search_eval_workspace_bytes(const nann_index* ix, const nann_model* m, int64_t n_queries,
                                     int64_t* nbytes);
/* The plan a nann_search_eval* call with these arguments runs, from the host alone (nothing is launched): exactly one of
 * scorer / m is given.  form: 0 = `seen` in each slot's HBM (every MLP and attention call; L2 on indices of more than 8
 * windows or with a neighbour row of 65 536 entries or more, and under NANN_EVAL_SEEN=hbm), 1 = the L2 form with `seen`
 * in LDS, one window (up to 1 015 808 items), 2 = the same sweeping the id space in n_windows windows.  slots = workgroups
 * launched, threads = their size, use_dirty = form 0 keeps the second-level bitmap of `seen` (else it scans `seen` whole).
 * Refuses what the call refuses by its scorer (NANN_SCORER_IP, NANN_MODEL_IP, an unknown kind, a handle that disagrees with
 * the index); what a call refuses by its other arguments or at its launch (an MLP of d = 512) is the call's to report.
 * Added without a change of nann_abi_version(). */
typedef struct nann_eval_plan {
  int32_t struct_bytes; /* out: sizeof(nann_eval_plan) of the library */
  int32_t form;
  int32_t n_windows;
  int32_t slots;
  int32_t threads;
  int32_t use_dirty;
} nann_eval_plan;
int nann_search_eval_plan(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, int64_t n_queries,
                          nann_eval_plan* out);
int nann_search_eval(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries,
                     const int32_t num_scoring_per_level[3], const int32_t top_k_per_level[3],
                     int32_t topk_eval, void* workspace, int64_t workspace_bytes, int64_t* out_item_ids,
                     float* out_scores, int32_t* out_index, int32_t* n_out, int32_t* status,
                     nann_stream_t stream);
/* nann_search_eval + counters i32[n_queries, 3] (device, or NULL): rows walked F, neighbours gathered G, rows scored S (the
 * enter points included), summed over a user's rounds -- what SURVEY.md 8(d)'s byte formula is evaluated on (bench.py's
 * roofline of the f3 line); a user whose request failed keeps zeros. */
int nann_search_eval_ex(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries,
                        const int32_t num_scoring_per_level[3], const int32_t top_k_per_level[3], int32_t topk_eval,
                        void* workspace, int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores,
                        int32_t* out_index, int32_t* n_out, int32_t* status, int32_t* counters, nann_stream_t stream);
int nann_search_eval_model(const nann_index* ix, const nann_model* m, const void* comm_seq_f16,
                           int64_t n_queries, const int32_t num_scoring_per_level[3],
                           const int32_t top_k_per_level[3], int32_t topk_eval, void* workspace,
                           int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores,
                           int32_t* out_index, int32_t* n_out, int32_t* status, nann_stream_t stream);

/* ---- 8(e): merge of per-shard top-k lists ----------------------------------
 * scores f32[n_queries, n_shards, k_in], ids i64[n_queries, n_shards, k_in]
 * (shard-major as all-gathered); concat in shard order, then TopKV2 order
 * (score desc, ties -> lower shard then lower local rank).
 * nann_merge_topk: device pointers; nann_merge_topk_host: [host] pointers. */
int nann_merge_topk(const float* scores, const int64_t* ids, int64_t n_queries, int32_t n_shards,
                    int32_t k_in, int32_t k_out, float* out_scores, int64_t* out_ids,
                    nann_stream_t stream);
int nann_merge_topk_host(const float* scores, const int64_t* ids, int64_t n_queries,
                         int32_t n_shards, int32_t k_in, int32_t k_out, float* out_scores,
                         int64_t* out_ids);

/* ---- 8(e): the exchange step owned by the C++ host (one process per GPU) -----------------
 * Rank g searches every query on shard g (nann_search), then nann_sharded_topk packs its
 * [scores | item ids] lists into one record, exchanges the records with ONE ncclAllGather
 * (RCCL over xGMI, k_in x 12 B per query per shard) and merges them on the device with
 * nann_merge_topk's order.  The reference has no collective on this path (replicas only,
 * blaze-benchmark/benchmark/core/model.cc:192-235); BASELINE configs 4-5 define this one.
 * RCCL is bound at run time (an RCCL already loaded in the process is shared, else
 * /opt/rocm/lib/librccl.so.1); without it these calls return NANN_ERR_UNSUPPORTED.
 *   nann_comm_get_unique_id  one rank draws the 128-byte id (ncclGetUniqueId) and the host
 *                            hands it to the others by its own means (file, socket, MPI ...)
 *   nann_comm_create         collective over all ranks (ncclCommInitRank) on the calling
 *                            thread's current HIP device; world == 1 needs no id and no RCCL;
 *                            world > 1 with id == NULL makes a LOOPBACK communicator for
 *                            single-process tests (every shard returns this rank's record)
 *   status (may be NULL)     a query with status != 0 on this shard contributes scores -inf /
 *                            ids 0: it is never selected while another shard holds real
 *                            candidates, and surfaces as (-inf, 0) entries otherwise
 *   workspace                device, nann_sharded_topk_workspace_bytes(...) bytes
 * Asynchronous on `stream`; every rank must make the same sequence of calls. */
typedef struct nann_comm nann_comm;
#define NANN_COMM_ID_BYTES 128
int nann_comm_get_unique_id(void* id /*[host] NANN_COMM_ID_BYTES*/);
int nann_comm_create(int32_t world, int32_t rank, const void* id /*[host]*/, nann_comm** out);
void nann_comm_destroy(nann_comm* c);
/* *world = shards of this communicator; *rccl_ranks = ncclCommCount of the RCCL communicator behind it (0: none -- a
 * loopback, or a one-shard communicator created without an id): what a multi-GPU bench line states so that "N ranks
 * exchanged over RCCL" is a measured fact. */
int nann_comm_ranks(const nann_comm* c, int32_t* world, int32_t* rccl_ranks);
/* enabled: HIP events around the three parts of every later nann_sharded_topk call on its stream;
 * nann_comm_last_breakdown -> ms[3] = {pack, all-gather, merge} of the LAST call (waits for it).  Loopback communicators
 * only (one-GPU measurements of the overlap and the slot reserve, tools/overlap_bench.py): loopback_wait_us > 0 puts a
 * kernel of 16 waiting workgroups in front of the stand-in copies -- an exchange that holds its slots and its stream as long
 * as 8 GPUs' all-gather over xGMI would (~1.5 ms at configs[3]) --, loopback_repeat >= 1 issues the copies that many times. */
int nann_comm_set_timing(nann_comm* c, int32_t enabled, int32_t loopback_repeat, int32_t loopback_wait_us);
int nann_comm_last_breakdown(nann_comm* c, float ms[3]);
/* A dead rank must not hang the node (round 6).  nann_sharded_topk only ENQUEUES; a host that then waits on the stream waits
 * for ever when a peer never joins the all-gather.  Instead:
 *   nann_comm_wait   bounded wait for the LAST exchange enqueued on this communicator: polls its completion event next to
 *                    ncclCommGetAsyncError.  Done -> NANN_OK.  RCCL reports an asynchronous error, or timeout_ms (>= 0; < 0: no
 *                    deadline) elapse -> the communicator is ABORTED (ncclCommAbort: RCCL's kernels see the flag and leave, so
 *                    the stream drains) and NANN_ERR_HIP is returned with the reason in nann_last_error.
 *   nann_comm_abort  the same abort on the host's own decision (a watchdog, a failed health check of a peer).
 * An aborted communicator fails every later call with NANN_ERR_HIP; the host destroys it and creates a new one with the ranks
 * that are left.  nann_sharded_topk itself refuses to enqueue on a communicator whose RCCL state already reports an error. */
int nann_comm_wait(nann_comm* c, int32_t timeout_ms);
int nann_comm_abort(nann_comm* c);
int nann_sharded_topk_workspace_bytes(int32_t world, int64_t n_queries, int32_t k_in, int64_t* nbytes);
int nann_sharded_topk(nann_comm* c, const float* scores, const int64_t* ids, const int32_t* status,
                      int64_t n_queries, int32_t k_in, int32_t k_out, void* workspace,
                      int64_t workspace_bytes, float* out_scores, int64_t* out_ids, nann_stream_t stream);
/* The merge step of nann_sharded_topk on its own, for a host whose transport is not RCCL (MPI, sockets, a gather of its own):
 * recv (device) holds `world` records, record s at recv + s * record_bytes, each laid out as nann_sharded_topk packs it --
 * scores f32[n_queries, k_in], then at byte n_queries * k_in * 4 the ids i64[n_queries, k_in]; a query that failed on the
 * shard carries (-inf, 0).  record_bytes: a multiple of 4, at least nann_sharded_topk_workspace_bytes(1, ...) / 2 (the record
 * padded to 256 bytes, which is the stride nann_sharded_topk gathers with), else NANN_ERR_CAPACITY.  Same kernel, same order
 * and same limits as nann_sharded_topk (k_out in [0, 1024], k_out <= world * k_in <= 16384); n_queries == 0 or k_out == 0 does
 * nothing.  Asynchronous on `stream`.  Held, like nann_sharded_topk, nann_merge_topk and nann_topk with k > 1024, to the plain
 * model of tests/merge_model.py on the cases of tests/merge_cases.py, records of shards that differ among them
 * (tests/test_merge_gpu.py; tests/test_merge_model_cpu.py shows on the host that those cases tell a wrong merge from a right one). */
int nann_merge_records(const void* recv, int64_t record_bytes, int32_t world, int64_t n_queries, int32_t k_in, int32_t k_out,
                       float* out_scores, int64_t* out_ids, nann_stream_t stream);

/* ---- 8(f1): HNSW index construction on the device -------------------------------------------------
 * What the reference does on the host with faiss.IndexHNSWFlat(d, M).add(embeddings)
 * (NANN_impls/nann/delivery/build_hnsw_index.py:33-35): the HNSW insertion algorithm (Malkov & Yashunin alg. 1-4
 * with Faiss' conventions: L2, M links above level 0 and 2M at level 0, efConstruction = 40, selection heuristic
 * without keepPrunedConnections), batched -- nodes go in by descending level in batches of at most a quarter of
 * the graph built so far (<= 16384), every node of a batch searches the graph of the earlier batches with one
 * wavefront, back-links are applied per target in a deterministic order (csrc/nann_hnsw_build.hip).  Index
 * contents are not a parity target against Faiss (its own are thread-schedule dependent); layout, invariants and recall are.
 * They are a pure function of (rows, levels, M, ef_construction, keep_pruned, metric), pinned entry for entry to the model
 * of tests/hnsw_build_model.py for the cases of its tests.  Everything is ordered by the key (distance with -0 taken as +0,
 * then id), ascending: the beam of a search, the candidates of a selection, a full row and its new link, a repair's pool.
 *   nann_hnsw_draw_levels   [host] levels[i] = number of levels of node i (Faiss convention, P(levels > l) = M^-l),
 *                           same draw as the CPU builder's; *n_up_rows = sum(levels - 1) = rows of adj_up
 *   nann_hnsw_build_device  item_embs device [n, d] f16 | bf16 (d in 64 | 128 | 256), levels [host];
 *                           outputs (device, caller-allocated): adj0 i32[n, 2M] (-1 = empty slot), up_row i32[n]
 *                           (first row of node i in adj_up, -1 if it has one level), adj_up i32[n_up_rows, M]
 *                           (level l >= 1 of node i: row up_row[i] + l - 1).  Synchronous (returns when built).
 * nann_amd/index_build.py exports these as build_hnsw_index.py:41-66 does (enter points = levels > start_level,
 * per-level CSR over all items with the -1 slots dropped). */
int nann_hnsw_draw_levels(int64_t n_items, int32_t M, uint64_t seed, int32_t* levels /*[host]*/, int64_t* n_up_rows);
int nann_hnsw_build_device(const void* item_embs, int64_t n_items, int32_t d, int32_t emb_dtype, int32_t M,
                           int32_t ef_construction, const int32_t* levels /*[host]*/, int32_t* adj0, int32_t* up_row,
                           int32_t* adj_up, nann_stream_t stream);
/* The same with alg. 4's keepPrunedConnections switch (keep_pruned != 0: a row's free slots are filled with the nearest
 * candidates the heuristic discarded -- Faiss and hence the reference leave it off): rows fill up to their cap, mean level-0
 * degree ~55 of 64 instead of ~17.  The dense-graph family SURVEY.md 8's gather bound (L0 gathered <= ef * 64) is about;
 * bench.py --graph hnsw_dense and the planner tests run on it. */
int nann_hnsw_build_device_ex(const void* item_embs, int64_t n_items, int32_t d, int32_t emb_dtype, int32_t M,
                              int32_t ef_construction, int32_t keep_pruned, const int32_t* levels /*[host]*/, int32_t* adj0,
                              int32_t* up_row, int32_t* adj_up, nann_stream_t stream);
/* Append: n_new rows go into a graph that nann_hnsw_build_device(_ex) or an earlier append built -- what a second
 * faiss.IndexHNSWFlat.add on a built index does -- at the cost of the new rows, not of the corpus.
 *   item_embs  device [n_old + n_new, d]; its first n_old rows are the rows the graph was built on (not checked)
 *   levels     [host] n_old + n_new: the old nodes' levels as the build had them, then nann_hnsw_draw_levels(n_new, M, seed)
 *              with a seed of the caller's choosing
 *   adj0, up_row, adj_up   the builder's arrays (device, the caller's), sized for n_old + n_new nodes and sum(levels - 1)
 *              upper rows over ALL nodes, the old graph in their heads as the build left it.  Their tails are ignored on
 *              entry and overwritten: -1 slots, up_row continuing the prefix rule.
 *   d, emb_dtype, M, ef_construction, keep_pruned   the limits and the status codes of the build.
 * The old graph is INPUT, and malformed input never faults: one pass over the old rows, before anything is written or
 * searched, holds them to the rules the insertion relies on -- up_row[i] is what `levels` implies (-1 for one level, else the
 * running sum of levels - 1); every entry lies in [-1, n_old); no entry follows a -1 (rows are dense prefixes, their length
 * is the fill count the build keeps private and the append recomputes); an entry of a level-l row names a node with more
 * than l levels (so no row is looked up that does not exist).  A graph that breaks one is refused with
 * NANN_ERR_BAD_ARGUMENT, every array untouched, nann_last_error naming the first broken rule and the lowest node that
 * breaks it.
 * Insertion is the build's (the same kernels): new nodes by descending level, then ascending id; the entry point is the
 * lowest id among the nodes with the most levels; a new node with MORE levels than the entry point goes in alone, is linked
 * on the levels the graph has (its rows above stay empty) and is the entry point from then on.  A batch is at most
 * min(16384, inserted / 4, ceil(n_new / 64)) nodes: batch mates do not see each other, and appended rows, unlike a build's
 * random order, may all be neighbours (a new category) -- in one batch they get no links to one another and requests near
 * them fail; in 64 batches recall there is that of a build in random order (measured; 8 and 32 fall short).
 * Deterministic: the same inputs give the same arrays.
 * OLD ROWS CHANGE: back-links append new ids to an old row while it has room and re-select a full row with the heuristic, so
 * the old part of a row can only shrink.  A caller that keeps serving the old graph while appending appends to a COPY.
 * Synchronous.  NANN_OK (n_new == 0: after the checks, nothing written); NANN_ERR_BAD_ARGUMENT (a null pointer, n_old < 1,
 * n_new < 0, levels[i] < 1, a malformed graph); NANN_ERR_UNSUPPORTED (more than 2^31 - 1 nodes in total, d, dtype, M or
 * ef_construction outside the build's limits); NANN_ERR_HIP. */
int nann_hnsw_append_device(const void* item_embs, int64_t n_old, int64_t n_new, int32_t d, int32_t emb_dtype,
                            int32_t M, int32_t ef_construction, int32_t keep_pruned,
                            const int32_t* levels /*[host] n_old + n_new*/,
                            int32_t* adj0, int32_t* up_row, int32_t* adj_up, nann_stream_t stream);
/* Build and append with a metric: the arguments of nann_hnsw_build_device_ex / nann_hnsw_append_device and `metric`, a
 * nann_scorer_kind, the kind of scorer the index will be searched with.  NANN_SCORER_L2: the calls above (which are these with
 * L2).  NANN_SCORER_IP: rows are linked by dist(a, b) = -<a, b>, smaller is nearer (Faiss' IndexHNSWFlat(d, M,
 * METRIC_INNER_PRODUCT)); greedy descent, the ef_construction beam, the selection heuristic (keep c iff dist(c, s) >=
 * dist(c, base) for every kept s) with its keep_pruned switch and the back-links' re-selection run on that distance unchanged.
 * Per lane acc = fmaf(a_k, b_k, acc) from +0 over its 8 elements, the partials added in the xor butterfly, dist = 0 - sum:
 * deterministic, not a promise of the scorer's bits.  NANN_SCORER_MLP: NANN_ERR_UNSUPPORTED; any other value:
 * NANN_ERR_BAD_ARGUMENT; both before anything is launched or written.  Every other limit, status code, the validation pass of
 * an append, the batch rule and the determinism promise are those of the calls above.  Appending with another metric than the
 * graph was built with is the caller's error and is not checked (neither are the old rows).  The export calls below do not
 * depend on the metric.  Under IP with the default heuristic rows are sparse (mean level-0 degree 2-3 on the test corpus of
 * DESIGN.md 4.6 against 3-4 for L2 on the same rows: a kept neighbour of large norm dominates most later candidates);
 * keep_pruned is the switch for denser rows. */
int nann_hnsw_build_device_metric(const void* item_embs, int64_t n_items, int32_t d, int32_t emb_dtype, int32_t M,
                                  int32_t ef_construction, int32_t keep_pruned, int32_t metric,
                                  const int32_t* levels /*[host]*/, int32_t* adj0, int32_t* up_row, int32_t* adj_up,
                                  nann_stream_t stream);
int nann_hnsw_append_device_metric(const void* item_embs, int64_t n_old, int64_t n_new, int32_t d, int32_t emb_dtype,
                                   int32_t M, int32_t ef_construction, int32_t keep_pruned, int32_t metric,
                                   const int32_t* levels /*[host] n_old + n_new*/,
                                   int32_t* adj0, int32_t* up_row, int32_t* adj_up, nann_stream_t stream);
/* Export on the device: the builder's arrays -> what nann_index_desc takes (on_device = 1), by the rule of
 * build_hnsw_index.py:41-66 with start_level = 2 (the levels serving walks; any other value: NANN_ERR_UNSUPPORTED).  Two steps,
 * as nann_group_gather_count / _fill, because the sizes depend on the data.  adj0, up_row, adj_up (device) and levels [host]
 * as the build or an append left them, n nodes; all outputs are the caller's.
 *   count  row_splits0, row_splits1: device i64[n + 1], the CSR offsets of level 0 and 1 (a node absent on level 1 has an empty
 *          row); nnz [host] i64[2] = their last entries; *n_enter [host] = nodes with levels > 2.  Synchronises.
 *   fill   values0 i32[nnz[0]], values1 i32[nnz[1]] (device): every non-negative slot of a row in slot order, the -1 slots
 *          dropped wherever they stand; enter_points i32[n_enter] (device): the nodes with levels > 2, ascending.
 *          row_splits0/1 and nnz [host] i64[2] are count's.  Synchronises.
 * NANN_ERR_BAD_ARGUMENT: a null pointer, n < 1, levels[i] < 1, an up_row entry of a node with more than one level outside
 * adj_up, nnz < 0 or a null values array with nnz > 0, row_splits (fill) that are not this graph's -- a row is written only where
 * its span has the row's own length and lies inside values[0, nnz), rs[0] is 0 and rs[n] is nnz, so nothing is written
 * outside the arrays.  NANN_ERR_UNSUPPORTED:
 * n > 2^31 - 1, M outside [2, 32], start_level != 2.  NANN_ERR_HIP. */
int nann_hnsw_export_count(const int32_t* adj0, const int32_t* up_row, const int32_t* adj_up,
                           const int32_t* levels /*[host] n*/, int64_t n, int32_t M, int32_t start_level,
                           int64_t* row_splits0, int64_t* row_splits1, int64_t* nnz /*[host] 2*/,
                           int64_t* n_enter /*[host]*/, nann_stream_t stream);
int nann_hnsw_export_fill(const int32_t* adj0, const int32_t* up_row, const int32_t* adj_up,
                          const int32_t* levels /*[host] n*/, int64_t n, int32_t M, int32_t start_level,
                          const int64_t* row_splits0, const int64_t* row_splits1, const int64_t* nnz /*[host] 2*/,
                          int32_t* values0, int32_t* values1, int32_t* enter_points, nann_stream_t stream);
/* Remove: rows leave a graph that a build or an append made; the result is a SMALLER, RENUMBERED graph over the survivors whose
 * rows have been reconnected across the holes -- at the cost of the rows that lost a neighbour, not of a rebuild.  (A withdrawn
 * row is hidden at once by a deny bit, nann_filter; it still costs its embedding, its place in every pre-projected table and a
 * gather and a score in every traversal that meets it, and the unfiltered calls do not know the bitmap.  This call is what
 * follows when the denied share has grown.)  The semantics are this library's own: the reference and Faiss' IndexHNSWFlat have
 * no removal.
 *   remove_bits  device u32[ceil(n / 32)], the deny bitmap's convention: row r is removed iff bit (r & 31) of word (r >> 5) is
 *                set; bits at or beyond n are ignored.  A nann_filter's deny_bits goes in as it is.
 *   the old graph (adj0, up_row, adj_up: device; levels: host; n nodes) and item_embs [n, d] are const and stay untouched, so an
 *                index that still serves from them is safe; the outputs are NEW arrays, the caller's.
 * Renumbering: the survivor with old id i gets new id = number of survivors below i (order kept); it keeps its levels;
 * out_up_row follows the prefix rule over the survivors' levels.  The result is therefore valid input of
 * nann_hnsw_append_device(_metric), of nann_hnsw_export_count / _fill and of this call again.
 * A row none of whose entries is removed is copied, renumbered, slot for slot.  A row with at least one removed entry is
 * REPAIRED (the delete consolidation of FreshDiskANN, alg. 4, with this builder's selection heuristic in the place of
 * RobustPrune): the candidate pool of node p on level l is the SET (p itself left out) of the surviving entries of p's row and,
 * for every removed entry r of the row, the surviving entries of r's row on level l -- one hop: removed entries of r's row are
 * not followed.  The pool is cut to its 64 nearest members by the build's (distance to p, id) key in `metric` (L2, or -<a, b>),
 * the heuristic runs over them in ascending order with the level's cap (2M on level 0, M above) and honours keep_pruned, and the
 * row is written as a dense prefix in that order with -1 behind.
 * WHAT IT DOES NOT DO: no back-links are added (no other row learns of a repaired row's new entries); a node may come out with
 * an empty row or without in-links, which is counted in stats and not healed here (nann_hnsw_orphan_bits followed by
 * nann_hnsw_update_device, below, re-inserts such nodes); and nothing guards the entry layer -- after a
 * removal the serving enter points are the survivors with levels > 2, and when fewer remain than the first top-k asks for,
 * requests fail k > n exactly as on any small index.  That is the caller's to watch (new_levels says how many are left).
 *   nann_hnsw_remove_count  step 1, because the sizes depend on the data (as nann_hnsw_export_count).  kept_rows device i32[n]:
 *                its head holds the n_keep surviving old ids ascending -- the `indices` nann_gather_rows takes to compact
 *                item_embs and item_ids; new_levels [host] i32[n]: its head holds the survivors' levels; *n_keep, *n_up_rows
 *                [host] (sum(levels - 1) over the survivors).  Tails are left as they were.  The graph is not read.  Synchronises.
 *   nann_hnsw_remove_device step 2.  out_adj0 i32[n_keep, 2M], out_up_row i32[n_keep], out_adj_up i32[max(n_up_rows, 1), M]
 *                (device).  stats [host] i64[4] or NULL: {rows repaired (all levels), level-0 rows that were non-empty and came
 *                out empty, rows whose distinct pool exceeded 64, survivors}.  Synchronous.
 * The old graph is INPUT, and malformed input never faults: the validation pass of the append runs first over all n nodes (the
 * same four rules, the same words in nann_last_error, the lowest offending node); the old -> new map comes from the call's own
 * scan of remove_bits, no caller array is trusted; an n_keep that is not the bitmap's survivor count is refused.  All of these
 * give NANN_ERR_BAD_ARGUMENT with every output array untouched.  Argument checks come before any device call:
 * NANN_ERR_BAD_ARGUMENT (a null pointer -- out_adj_up included, adj_up when a node has more than one level --, n < 1,
 * levels[i] < 1, n_keep < 1: a graph keeps at least one node, n_keep > n, a metric that is no scorer kind);
 * NANN_ERR_UNSUPPORTED (n > 2^31 - 1, d, dtype or M outside the build's limits, NANN_SCORER_MLP); NANN_ERR_HIP.
 * Removing nothing is not an error: the outputs equal the inputs bit for bit, kept_rows = 0 .. n - 1, stats[0] = 0.
 * Deterministic: a row's result depends on the inputs only, and the counters are totals. */
int nann_hnsw_remove_count(const uint32_t* remove_bits, const int32_t* levels /*[host] n*/, int64_t n,
                           int32_t* kept_rows, int32_t* new_levels /*[host]*/, int64_t* n_keep, int64_t* n_up_rows,
                           nann_stream_t stream);
int nann_hnsw_remove_device(const void* item_embs, int64_t n, int32_t d, int32_t emb_dtype, int32_t M,
                            int32_t keep_pruned, int32_t metric, const int32_t* levels /*[host] n*/,
                            const int32_t* adj0, const int32_t* up_row, const int32_t* adj_up,
                            const uint32_t* remove_bits, int64_t n_keep,
                            int32_t* out_adj0, int32_t* out_up_row, int32_t* out_adj_up, int64_t* stats,
                            nann_stream_t stream);
/* Update: rows of a graph are refreshed IN PLACE -- an item whose embedding has changed, or a node a removal left without
 * links.  Row numbers and levels do not change, so everything that speaks in internal rows (a nann_filter's deny_bits and
 * excl_rows, nann_candidates.rows, out_index, the caller's item_ids order) stays valid; remove + nann_gather_rows + append
 * would move the row to the tail and renumber every survivor.  Overwriting the embedding alone leaves the row's links, and the
 * links to it, where its OLD embedding put them.
 *   item_embs    device [n, d]: already holds the NEW embeddings of the marked rows.  The old ones are not needed: no distance
 *                the call computes involves a marked row before that row is re-inserted.
 *   update_bits  device u32[ceil(n / 32)], the deny bitmap's convention (row r is marked iff bit (r & 31) of word (r >> 5) is
 *                set); bits at or beyond n are ignored.
 *   the old graph (adj0, up_row, adj_up: device; levels: host; n nodes) is const and stays untouched; the outputs are NEW
 *                arrays of the same shapes, the caller's: out_adj0 i32[n, 2M], out_up_row i32[n] (the prefix rule, equal to
 *                up_row), out_adj_up i32[max(sum(levels - 1), 1), M] (without upper rows it is not written).  The result is
 *                valid input of nann_hnsw_append_device(_metric), of the export calls, of nann_hnsw_remove_* and of this call again.
 * Two phases, on the path build, append and remove share.
 * DETACH is the repair of nann_hnsw_remove_device without the renumbering: a marked node's rows come out empty on every level;
 * a staying row with no marked entry is copied slot for slot; a staying row with a marked entry is re-selected from its pool --
 * the staying entries of the row and, one hop out, the staying entries of each marked entry's old row on that level, the node
 * itself left out --, cut to its 64 nearest members by the (distance, id) key, with the level's cap and keep_pruned.  After it
 * no row names a marked node.  The fill counts of the new arrays come from a device pass over them.
 * RE-INSERT is the append's insertion: the marked nodes by descending level, then ascending id, onto the staying ones; the
 * entry point is the lowest id among the STAYING nodes with the most levels; a batch is at most min(16384, (staying + inserted
 * so far) / 4, ceil(n_marked / 64)) nodes; a marked node with more levels than the entry point goes in alone, is linked on the
 * levels the graph has (its rows above stay empty) and is the entry point from then on; back-links as in the build.
 *   stats [host] i64[4] or NULL: {rows repaired by the detach phase (all levels), level-0 rows of staying nodes that were
 *                non-empty and came out of the detach phase empty, rows whose distinct pool exceeded 64, rows updated}.
 * The old graph is INPUT, and malformed input never faults: the validation pass of the append runs first over all n nodes (the
 * same four rules, the same words in nann_last_error, the lowest offending node); a malformed graph gives
 * NANN_ERR_BAD_ARGUMENT with every output (stats included) untouched.  Argument checks come before any device call:
 * NANN_ERR_BAD_ARGUMENT (a null pointer -- out_adj_up included, adj_up when a node has more than one level --, n < 1,
 * levels[i] < 1, a metric that is no scorer kind); NANN_ERR_UNSUPPORTED (n > 2^31 - 1, d, dtype, M or ef_construction outside
 * the build's limits, NANN_SCORER_MLP).  Every row marked, so that nothing stays, is NANN_ERR_BAD_ARGUMENT with the outputs
 * untouched: that is a build.  Nothing marked is not an error: the outputs equal the inputs bit for bit, stats all zero.
 * Synchronous.  Deterministic: the same inputs give the same arrays.  Outputs that alias inputs are the caller's error.
 * WHAT IT DOES NOT DO: it does not heal the in-links of STAYING nodes (mark them: nann_hnsw_orphan_bits), and it does not
 * promise that a re-inserted node keeps an in-link -- a full row may re-select it away.  It does promise that every re-inserted
 * node's own level-0 row is non-empty when at least one node stays.
 *   nann_hnsw_orphan_bits  which rows to heal: out_bits device u32[ceil(n / 32)], bit r set iff level-0 row r is empty or no
 *                level-0 row names r; entries outside [0, n) are skipped as if their slots were empty, so a malformed adj0 never
 *                faults; bits at or beyond n in the last word are zero.  *n_orphans [host] = the bits set.  Synchronous; the
 *                output is a set, hence deterministic.  NANN_ERR_BAD_ARGUMENT (a null pointer, n < 1); NANN_ERR_UNSUPPORTED
 *                (n > 2^31 - 1, M outside [2, 32]).  The heal after a removal: nann_hnsw_orphan_bits on the removal's output,
 *                then nann_hnsw_update_device with those bits and the embeddings as they are. */
int nann_hnsw_update_device(const void* item_embs, int64_t n, int32_t d, int32_t emb_dtype, int32_t M,
                            int32_t ef_construction, int32_t keep_pruned, int32_t metric,
                            const int32_t* levels /*[host] n*/,
                            const int32_t* adj0, const int32_t* up_row, const int32_t* adj_up,
                            const uint32_t* update_bits /*device, the deny bitmap's convention*/,
                            int32_t* out_adj0, int32_t* out_up_row, int32_t* out_adj_up,
                            int64_t* stats /*[host] i64[4] or NULL*/, nann_stream_t stream);
int nann_hnsw_orphan_bits(const int32_t* adj0, int64_t n, int32_t M, uint32_t* out_bits /*device, ceil(n/32) words*/,
                          int64_t* n_orphans /*[host]*/, nann_stream_t stream);

/* ---- 8(f2): the reference's own scorer model behind the BlazeXlaOp contract -------------
 * NANN_impls/nann/model/model.py:189-233 + model_util.py:70-97: softmax attention of the candidate
 * over the user's behaviour sequence u f16[L, 64] (comm_seq, build_opt_graph.py:76-79), then a DNN
 * 128-64-32-1 with batch norm (folded to scale/shift) and PReLU, last layer bias-free.  f32 logits,
 * rows scored independently.  This build: E = 64, L <= 64, d in {64, 128}, rows f16 or bf16.
 * All descriptor pointers are [host] f32; the scorer owns device copies. */
typedef struct nann_attn_scorer nann_attn_scorer;
typedef struct {
  int32_t d;         /* item embedding dim */
  int32_t emb_dtype; /* NANN_F16 | NANN_BF16 */
  int32_t seq_len;   /* L */
  const float *wq1, *bq1, *aq; /* [d,128] [128] [128] */
  const float *wq2, *bq2;      /* [128,256] [256] */
  const float *wk1, *bk1, *ak; /* [64,128] [128] [128] */
  const float *wk2, *bk2;      /* [128,256] [256] */
  const float* w[4];           /* [64+d,128] [128,64] [64,32] [32] */
  const float* b[3];
  const float* bn_scale[3];
  const float* bn_shift[3];
  const float* alpha[3];
  int32_t precision;  /* enum nann_mlp_precision: NANN_MLP_SPLIT_F16 (every f32 operand as hi + lo f16 on the
                       * 16-bit MFMA, 3x fewer matrix cycles; logits within ~1e-6 of the exact form; the default),
                       * NANN_MLP_EXACT_F32 (f32-input MFMA); NANN_MLP_CERTIFIED is rejected (MLP scorers only).
                       * Both forms hold 1e-5 max(1, |s|) against the f32 chain at every seq_len in [1, 64] and with a
                       * peaked softmax as with a flat one: attention logits spanning 15-21 per row, |att| up to ~25
                       * (wq2 and wk2 x 32), measured <= 6.3e-7 split, <= 5.7e-7 exact (tests/test_attn_shapes_gpu.py).
                       * Range of the split form: a user's projected keys are carried as f16 hi + lo of k x 2^7
                       * (k_attn_prepare_split, round-to-nearest conversions), so every component of every key needs
                       * |k| < 511.875 (|k| x 2^7 < 65520, where the conversion to f16 stays finite).  A position with
                       * a key component at or beyond that gets hi = +-inf, lo = -+inf and a NaN attention logit, and
                       * the softmax DROPS it: fmaxf skips the NaN in the row maximum and the exponential clamps its
                       * argument from below, so the position gets weight 0 and the others are renormalised.  That
                       * user's logits are FINITE AND WRONG -- the model's logits for the sequence without that
                       * position -- with no status and no NaN to test for; they are NaN only when every one of the
                       * user's L positions overflows.  Other users are not touched.  A caller that cannot bound its
                       * keys must check them itself or use the exact form, which has no such limit.
                       * (tests/attn_reference.py split_softmax restates those lines; test_attn_shapes_gpu.py runs it.) */
} nann_attn_desc;
int nann_attn_scorer_create(const nann_attn_desc* desc /*[host]*/, nann_attn_scorer** out);
void nann_attn_scorer_destroy(nann_attn_scorer* s);
/* Per-user part, once per request: user_seq f16[n_users, L, 64] -> kt f32[n_users, 256, 64]
 * (the projected keys, transposed, zero beyond L) and upad f32[n_users, 64, 64] (the sequence,
 * zero-padded); both caller-owned device buffers. */
int nann_attn_prepare(const nann_attn_scorer* s, const void* user_seq_f16, int64_t n_users, float* kt,
                      float* upad, nann_stream_t stream);
/* Logits of n candidate rows for ONE user (kt / upad of that user); table / indices / errors as
 * nann_score. */
int nann_attn_score(const nann_attn_scorer* s, const float* kt, const float* upad, const void* table,
                    int64_t n_table_rows, const int32_t* indices, int64_t n, float* out_scores,
                    int64_t* bad_i, nann_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NANN_HIP_H_ */
