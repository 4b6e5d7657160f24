// nann_cand.h -- candidate-list search (nann_search_candidates): every query of a batch brings a list of rows of its own,
// the rows are scored and the list's top k returned in TopKV2 order, ties by position in the list.  The reference has no such
// call; nothing here restates a line of it.
//
// The host knows n_queries, n_cand and k; the lists' lengths are device data and are never read back.  Three steps:
//   1. k_cand_plan (one workgroup): per query (begin, len, status) from row_splits, and the exclusive prefix sum of the
//      queries' block counts, ceil(len / C) -- item_off i64[n_queries + 1], the last entry the number of work items.  Query i is
//      WELL-FORMED iff 0 <= splits[i] <= splits[i + 1] <= n_cand and splits[i] >= splits[j] for every j < i, i.e. splits[i] equals
//      the running maximum of splits[0 .. i].  An earlier well-formed query's end is an earlier split, hence <= this query's
//      begin: the ranges of well-formed queries are pairwise disjoint whatever the caller passes, and a score buffer addressed by
//      list position has one writer per element.  An ill-formed query gets status 3, length 0 and no work item.
//   2. k_cand_score_l2 / k_cand_score_ip / k_cand_score_mlp (persistent grids): work item w = block w - item_off[i] of the query i with
//      item_off[i] <= w < item_off[i + 1], found by bisection (no list of items is written: the plan stays one pass over the
//      queries however long a list is).  L2: the block's <= kCandRows row numbers are staged into LDS and checked -- a row outside
//      [0, n_items) becomes row 0 and flags its query with an atomic OR on the plan's status word -- then wg_score_l2_part
//      (nann_device.h, the traversal's scorer) runs on the LDS list.  MLP: W2 resident in LDS, u per query from k_cand_mlp_u, the
//      block functions of nann_mlp5.h with ids = rows + begin; they clamp a row beyond the table to row 0 themselves, so the
//      check only flags.
//   3. k_cand_topk (one workgroup per query): wg_topk over scores[begin, +len) with ids = rows + begin -- positions, rows,
//      scores and item ids in one pass, its tie rule (lower position) is the contract's; zeros behind min(k, len) entries, and a
//      whole row of zeros for a query with a status.
//
// Under a model (nann_search_candidates_model): an l2 / mlp model is the call above on the mean of the user's sequence.  The
// attention model keeps steps 1 and 3 and scores with k_cand_score_attn (nann_cand_attn_inst.hip), k_scan_attn crossed with
// k_cand_score_mlp: the users are taken in chunks of at most kCandAttnChunk, whose kt / upad (nann_attn_prepare) share one
// buffer of the workspace; per chunk the persistent grid walks the work items of the chunk's users only,
// [item_off[c0], item_off[c0 + n_q)), and an item is one call of the resident attention block scorers of nann_attn_proj.h /
// nann_attn_kernels.h on the model's pre-projected table with ids = rows + begin and the keys of user qi - c0.
#pragma once
#include <cstddef>

#include "nann_scan.h"
#include "nann_search.h"

namespace nann {

constexpr int kCandRows = 1024;     // C: candidates of an L2 work item (unmeasured)
constexpr int kCandMlpRows = 4096;  // candidates of an MLP work item: what k_scan_mlp gives the block scorers per call (kScanMlpRows)
// R: candidates of a work item under the attention model (unmeasured).  A multiple of 256: eight wavefronts take 32
// candidates each.  An item loads its user's keys (72 KB in the split form, from L2 / Infinity Cache: a chunk's keys are
// 10 MB) against 1.5 KB of table per scored row, so 256 rows put 19 % on top of the table's bytes; what this call is for,
// re-ranking a few hundred rows for tens of users, has a few dozen items at any R and its time is the time of ONE item --
// one 32-candidate block per wavefront at 256, two at 512.  The smallest legal value serves that case; the long lists of a
// large batch have items enough for every CU at any R and pay the 19 %.
constexpr int kCandAttnRows = 256;
constexpr int kCandAttnChunk = 128;  // most users whose kt / upad are resident at a time (kScanMaxChunk of the exhaustive scan)

struct CandQuery {  // the plan of one query
  int32_t begin, len;  // its list: rows[begin, +len); len = 0 for an ill-formed query
  int32_t status;      // 0, NANN_ERR_INVALID_RAGGED_INPUT (k_cand_plan) or NANN_ERR_INDEX_OUT_OF_RANGE (the scoring kernels)
  int32_t pad;
};

struct CandArgs {
  const void* emb;          // L2, inner product: the index's rows
  const float* proj;        // MLP: the pre-projected table of (scorer, index)
  const int64_t* item_ids;
  long long n_items;
  int d, dt;
  int kind, exact;          // nann_scorer_kind; MLP: the exact f32 form (also the certified precision) or split-f16
  MlpParams mlp;
  int cus;                  // compute units of the device: sizes the persistent grids
  const int64_t* row_splits;
  const int32_t* rows;
  long long n_cand;
};
// workspace layout of a call: [scores f32[n_cand] | plan CandQuery[n_queries] | item_off i64[n_queries + 1] | u f32[n_queries, 256] (MLP)]
struct CandLayout {
  size_t off_scores, off_plan, off_items, off_u, total;
};
CandLayout cand_layout(int kind, long long n_queries, long long n_cand);
// the longest list a query of a call of n_queries may bring when every query brings one as long: list positions are 32-bit
// (CandQuery, and the n_cand a call takes)
inline long long cand_max_list(long long n_queries) { return 0x7fffffffll / (n_queries > 0 ? n_queries : 1); }
int launch_cand(const CandArgs& a, const CandLayout& L, const float* q, long long n_queries, int k, unsigned char* ws,
                int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* out_pos, int32_t* n_out, int32_t* status,
                hipStream_t st);
// steps 1 and 2 of launch_cand without its top-k: the plan, and the exact score of every list position in L's score buffer, in
// position order (the range form of the certified int8 search selects from them by a cut, nann_sq8.h)
int launch_cand_scores(const CandArgs& a, const CandLayout& L, const float* q, long long n_queries, unsigned char* ws, hipStream_t st);
// steps 1 and 3 on their own (nann_cand_inst.hip): launch_cand's, and the attention form's around its chunks
int launch_cand_plan(const int64_t* row_splits, long long n_queries, long long n_cand, int rows_per_item, CandQuery* plan,
                     long long* item_off, hipStream_t st);
int launch_cand_topk(const CandQuery* plan, const int32_t* rows, const float* scores, long long n_queries, int k,
                     const int64_t* item_ids, int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* out_pos,
                     int32_t* n_out, int32_t* status, hipStream_t st);

// ---- the attention model (nann_cand_attn_inst.hip) ------------------------------------------------------------------
struct CandAttnArgs {
  AttnParams attn;
  int exact;                // the f32 form or split-f16
  const float* proj;        // the pre-projected table of (model, index)
  const int64_t* item_ids;
  long long n_items;
  int cus;
  const int64_t* row_splits;
  const int32_t* rows;
  long long n_cand;
};
// workspace layout of a call: [scores f32[n_cand] | plan CandQuery[n_users] | item_off i64[n_users + 1] | kt + upad of one chunk]
struct CandAttnLayout {
  int chunk;  // users per pass = min(n_users, kCandAttnChunk)
  size_t off_scores, off_plan, off_items, off_user, total;
};
CandAttnLayout cand_attn_layout(long long n_users, long long n_cand);
int launch_cand_attn(const CandAttnArgs& a, const CandAttnLayout& L, const void* comm_seq_f16, long long n_users, int k,
                     unsigned char* ws, int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* out_pos,
                     int32_t* n_out, int32_t* status, hipStream_t st);

// work item w of a scoring kernel: the query it belongs to (item_off[qi] <= w < item_off[qi + 1]), where its block starts in
// `rows` / `scores` and how many candidates it holds.  Uniform over the workgroup.
struct CandItem {
  long long qi;
  int begin, count;
};
__device__ __forceinline__ CandItem cand_item(const CandQuery* __restrict__ plan, const long long* __restrict__ item_off,
                                              long long n_queries, long long w, int rows_per_item) {
  long long lo = 0, hi = n_queries;  // item_off[lo] <= w < item_off[hi]
  while (hi - lo > 1) {
    const long long mid = lo + (hi - lo) / 2;
    if (item_off[mid] <= w) lo = mid; else hi = mid;
  }
  const CandQuery p = plan[lo];
  const int at = (int)(w - item_off[lo]) * rows_per_item;
  return CandItem{lo, p.begin + at, min(rows_per_item, p.len - at)};
}

}  // namespace nann

#ifdef NANN_CAND_IMPL  // the kernels: nann_cand_inst.hip only (nann_flat.hip takes the declarations above)
namespace nann {

constexpr int kCandNT = 256;  // threads of k_cand_plan and k_cand_score_l2

// inclusive scan of v over the workgroup's threads (MAX: running maximum, else running sum); *total = over all of them.
// wsum: LDS, one entry per wavefront.
template <bool MAX, int NT>
__device__ __forceinline__ long long cand_wg_scan(long long v, long long* wsum, long long* total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long t = __shfl_up(v, o);
    if (lane >= o) v = MAX ? max(v, t) : v + t;
  }
  __syncthreads();  // (the scan before this one has read wsum)
  if (lane == 63) wsum[wave] = v;
  __syncthreads();
  long long all = wsum[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) {
    if (w == wave) v = MAX ? max(v, all) : v + all;
    all = MAX ? max(all, wsum[w]) : all + wsum[w];
  }
  *total = all;
  return v;
}

// One workgroup, tiles of kCandNT queries: a running maximum over the splits decides well-formedness, a running sum over the
// block counts places every query's work items.  Writes every word the later kernels read or accumulate into.
__global__ __launch_bounds__(kCandNT) void k_cand_plan(const int64_t* __restrict__ splits, long long n_queries, long long n_cand,
                                                        int rows_per_item, CandQuery* __restrict__ plan,
                                                        long long* __restrict__ item_off) {
  __shared__ long long wsum[kCandNT / 64];
  long long seen = (long long)0x8000000000000000ull;  // max of splits[0 .. t0): nothing yet
  long long items = 0;                                // work items of the queries before t0
  for (long long t0 = 0; t0 < n_queries; t0 += kCandNT) {
    const long long i = t0 + threadIdx.x;
    const bool valid = i < n_queries;
    const long long b = valid ? splits[i] : (long long)0x8000000000000000ull;
    const long long e = valid ? splits[i + 1] : 0;
    long long tile_max, tile_items;
    const long long run = max(seen, cand_wg_scan<true, kCandNT>(b, wsum, &tile_max));  // max of splits[0 .. i]
    const bool ok = b >= 0 && b <= e && e <= n_cand && b >= run;
    const long long len = ok ? e - b : 0;
    const long long nb = (len + rows_per_item - 1) / rows_per_item;
    const long long upto = items + cand_wg_scan<false, kCandNT>(nb, wsum, &tile_items);
    if (valid) {
      plan[i] = CandQuery{(int32_t)(ok ? b : 0), (int32_t)len, ok ? 0 : NANN_ERR_INVALID_RAGGED_INPUT, 0};
      item_off[i] = upto - nb;
    }
    seen = max(seen, tile_max);
    items += tile_items;
  }
  if (threadIdx.x == 0) item_off[n_queries] = items;
}

// what the scoring kernels take (by value)
struct CandScoreArgs {
  const void* emb;
  const float* proj;
  long long n_items;
  int d;
  const int32_t* rows;
  const float* q;             // L2, inner product: f32[n_queries, d]
  const float* u;             // MLP: f32[n_queries, 256]
  float* scores;              // f32[n_cand], by list position
  CandQuery* plan;
  const long long* item_off;
  long long n_queries;
};

// L2: a persistent grid over the work items; their number is device data (item_off[n_queries]).
template <int LPR, int DT>
__global__ __launch_bounds__(kCandNT) void k_cand_score_l2(CandScoreArgs a) {
  __shared__ int32_t ids[kCandRows];
  __shared__ float qv[kMaxD];
  const int tid = threadIdx.x;
  const long long n_work = a.item_off[a.n_queries];
  for (long long w = blockIdx.x; w < n_work; w += gridDim.x) {
    const CandItem it = cand_item(a.plan, a.item_off, a.n_queries, w, kCandRows);
    __syncthreads();  // (every wavefront has left the item before: its list and query may go)
    bool bad = false;
    for (int j = tid; j < it.count; j += kCandNT) {
      int32_t r = a.rows[it.begin + j];
      if ((uint32_t)r >= (uint32_t)a.n_items) {  // (n_items < 2^31: a negative row is out of range too)
        bad = true;
        r = 0;
      }
      ids[j] = r;
    }
    for (int e = tid; e < a.d; e += kCandNT) qv[e] = a.q[(size_t)it.qi * a.d + e];
    if (bad) atomicOr(&a.plan[it.qi].status, NANN_ERR_INDEX_OUT_OF_RANGE);
    __syncthreads();
    if (a.n_items <= 0) continue;  // (no row 0 to stand in: every candidate of an empty index has flagged its query)
    wg_score_l2_part<LPR, DT, kCandNT / 64>(a.emb, a.d, ids, 0, it.count, qv, a.scores + it.begin, tid >> 6, (unsigned long long)a.n_items * (unsigned)(a.d * 2) <= 0xffffffffull && a.n_items <= (1u << 24));
  }
}

// The inner product: the same items, the shared scorer with the other term.  (A kernel of its own and not a shared body: a body
// behind a common device function cost k_cand_score_l2 a scalar register, and the L2 kernels stay as they were to the register.)
template <int LPR, int DT>
__global__ __launch_bounds__(kCandNT) void k_cand_score_ip(CandScoreArgs a) {
  __shared__ int32_t ids[kCandRows];
  __shared__ float qv[kMaxD];
  const int tid = threadIdx.x;
  const long long n_work = a.item_off[a.n_queries];
  for (long long w = blockIdx.x; w < n_work; w += gridDim.x) {
    const CandItem it = cand_item(a.plan, a.item_off, a.n_queries, w, kCandRows);
    __syncthreads();  // (every wavefront has left the item before: its list and query may go)
    bool bad = false;
    for (int j = tid; j < it.count; j += kCandNT) {
      int32_t r = a.rows[it.begin + j];
      if ((uint32_t)r >= (uint32_t)a.n_items) {  // (n_items < 2^31: a negative row is out of range too)
        bad = true;
        r = 0;
      }
      ids[j] = r;
    }
    for (int e = tid; e < a.d; e += kCandNT) qv[e] = a.q[(size_t)it.qi * a.d + e];
    if (bad) atomicOr(&a.plan[it.qi].status, NANN_ERR_INDEX_OUT_OF_RANGE);
    __syncthreads();
    if (a.n_items <= 0) continue;  // (no row 0 to stand in: every candidate of an empty index has flagged its query)
    wg_score_l2_part<LPR, DT, kCandNT / 64, MT_IP>(a.emb, a.d, ids, 0, it.count, qv, a.scores + it.begin, tid >> 6, (unsigned long long)a.n_items * (unsigned)(a.d * 2) <= 0xffffffffull && a.n_items <= (1u << 24));
  }
}

// u[q][j] = b1[j] + sum_k q[k] W1[k][j]: the query's part of layer 1, once per query (k_scan_mlp_u's body)
__global__ __launch_bounds__(256) void k_cand_mlp_u(MlpParams P, const float* __restrict__ q, float* __restrict__ u) {
  __shared__ float qv[256];
  for (int k = threadIdx.x; k < P.d; k += 256) qv[k] = q[(size_t)blockIdx.x * P.d + k];
  __syncthreads();
  const float v = wg_mlp_query_u<256>(P, qv);
  if ((int)threadIdx.x < P.h1) u[(size_t)blockIdx.x * 256 + threadIdx.x] = v;
}

// The MLP on the pre-projected table, after k_scan_mlp: W2 resident in LDS for the whole launch (one workgroup per CU), an item
// is one call of wg_score_mlp_xres / wg_score_mlp_res with the block's stretch of `rows` as the row list.
template <bool EXACT>
__global__ __launch_bounds__(512) void k_cand_score_mlp(MlpParams P, CandScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NT = 512;
  uint4* W2 = reinterpret_cast<uint4*>(smem);
  Mlp2Vectors* V = reinterpret_cast<Mlp2Vectors*>(smem + kMlpResW2Bytes);
  const int tid = threadIdx.x;
  const uint4* src = EXACT ? reinterpret_cast<const uint4*>(P.p2x) : P.p2;
  for (int i = tid; i < kMlpResW2Vec; i += NT) W2[i] = src[i];
  if (EXACT) wg_mlp_xres_vectors<NT>(P, 0.0f, V); else wg_mlp_res_vectors<NT>(P, 0.0f, V);
  const long long n_work = a.item_off[a.n_queries];
  for (long long w = blockIdx.x; w < n_work; w += gridDim.x) {
    const CandItem it = cand_item(a.plan, a.item_off, a.n_queries, w, kCandMlpRows);
    const int32_t* ids = a.rows + it.begin;
    bool bad = false;
    for (int j = tid; j < it.count; j += NT) bad |= (uint32_t)ids[j] >= (uint32_t)a.n_items;
    if (bad) atomicOr(&a.plan[it.qi].status, NANN_ERR_INDEX_OUT_OF_RANGE);
    __syncthreads();  // (every wavefront has left the item before: its u may go)
    if (tid < 256) V->u[tid] = EXACT ? a.u[(size_t)it.qi * 256 + tid] : a.u[(size_t)it.qi * 256 + tid] * kSplit2Scale;
    __syncthreads();
    if (a.n_items <= 0) continue;  // (no row 0 for the clamp to land on)
    float* out = a.scores + it.begin;
    if (EXACT) wg_score_mlp_xres<NT>(a.proj, (uint32_t)a.n_items, ids, it.count, reinterpret_cast<const float4*>(W2), V, out);
    else wg_score_mlp_res<NT>(a.proj, (uint32_t)a.n_items, ids, it.count, W2, V, out);
  }
}

// one workgroup per query: TopKV2 over the list's scores, ties to the lower position; positions, rows, scores and item ids
// ride along.  A query with a status gets zeros.
__global__ __launch_bounds__(kNT) void k_cand_topk(const CandQuery* __restrict__ plan, const int32_t* __restrict__ rows,
                                                   const float* __restrict__ scores, int k, const int64_t* __restrict__ item_ids,
                                                   int64_t* __restrict__ out_item_ids, float* __restrict__ out_scores,
                                                   int32_t* __restrict__ out_index, int32_t* __restrict__ out_pos,
                                                   int32_t* __restrict__ n_out, int32_t* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) unsigned char scratch[sizeof(TopkScratch)];
  const size_t qi = blockIdx.x;
  const CandQuery p = plan[qi];
  const int kk = p.status != 0 ? 0 : min(k, p.len);
  if (kk > 0)
    wg_topk(rows + p.begin, scores + p.begin, nullptr, p.len, kk, out_pos ? out_pos + qi * k : nullptr,
            out_index ? out_index + qi * k : nullptr, out_scores ? out_scores + qi * k : nullptr, item_ids, out_item_ids + qi * k,
            scratch);
  for (int i = kk + (int)threadIdx.x; i < k; i += kNT) {
    const size_t at = qi * (size_t)k + i;
    out_item_ids[at] = 0;
    if (out_scores) out_scores[at] = 0.0f;
    if (out_index) out_index[at] = 0;
    if (out_pos) out_pos[at] = 0;
  }
  if (threadIdx.x == 0) {
    if (n_out) n_out[qi] = kk;
    status[qi] = p.status;
  }
}

}  // namespace nann
#endif
