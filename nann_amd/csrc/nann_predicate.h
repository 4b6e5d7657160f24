// nann_predicate.h -- attribute predicates: per-query label, range and tag conditions on row attributes (nann_predicates,
// include/nann_hip.h).  The reference has no such feature; nothing here restates a line of it.
//
// Row r PASSES query g iff every test that is present passes:
//   label  present iff the query's clamped range [b, e) of `labels` is not empty: label_of_row[r] is one of labels[b .. e);
//   value  present iff value_lo or value_hi is given: lo[g] <= value_of_row[r] <= hi[g], compared as IEEE does (a missing side
//          is -inf / +inf, which no comparison with a non-NaN value fails; a NaN value or bound passes nothing);
//   tags   present iff one of tags_all / tags_any / tags_none is given: (t & all) == all, any == 0 || (t & any) != 0,
//          (t & none) == 0 for t = tags_of_row[r] (a missing word is 0).
// Like the filter (nann_filter.h) the predicate is applied by kernels of its own next to the search kernels, which do not change:
//   * k_pred_scatter  exhaustive search: -inf over the failing positions of a chunk's scores f32[n_q, n_items], behind
//                     launch_filter_scatter and in front of the selection.  Unlike the deny scatter it has to look at every
//                     (query, row) pair: a workgroup takes a TILE of kPredTileRows rows and a GROUP of kPredQueries queries, a
//                     thread keeps the attributes of its four rows in registers and walks the group; the group's scalar
//                     conditions lie in LDS, its label sets in one LDS hash table per query, built by the workgroup in ROUNDS of
//                     kPredRound labels per query -- a list of any length takes ceil(len / kPredRound) rounds, the match is ORed
//                     over them.  It stores only where a row fails; a group without any test ends behind the check.
//   * k_pred_compact  k_filter_compact's job -- a ranked list of at most 1024 (row, score) pairs -> the passing pairs in order,
//                     zeros behind, their count -- plus the predicate.  The label test is the exclusion test mirrored: the
//                     entries' labels go into the LDS table, the query's label list streams through it, whatever its length.
//   * k_pred_count    rows of the index that pass each query and the filter, i64 per query: the tile walk of k_pred_scatter with
//                     a count in the place of the stores.
// The empty mark of a label table is INT32_MIN; a label of that value is carried by a flag per query instead.
//
// Malformed contents never fault: a label range is clamped to [0, n_labels] as filter_list_range clamps, rows of a list outside
// [0, n_items) are dropped, and the per-query arrays are read at the call's query number only.
#pragma once
#include <cstdint>

#include "nann_filter.h"

namespace nann {

// a nann_predicates as the kernels take it (all pointers device; any of them may be null)
struct PredArgs {
  const int32_t* label_of_row;             // i32[n_items]
  const float* value_of_row;               // f32[n_items]
  const unsigned long long* tags_of_row;   // u64[n_items]
  const int64_t* label_splits;             // i64[n_queries + 1] into labels, by the GLOBAL query number of the call
  const int32_t* labels;                   // i32[n_labels]
  long long n_labels;
  const float* value_lo;                   // f32[n_queries] each
  const float* value_hi;
  const unsigned long long* tags_all;      // u64[n_queries] each
  const unsigned long long* tags_any;
  const unsigned long long* tags_none;
};
__host__ __device__ inline bool pred_has_labels(const PredArgs& p) {
  return p.label_of_row && p.label_splits && p.labels && p.n_labels > 0;
}
__host__ __device__ inline bool pred_has_value(const PredArgs& p) { return p.value_of_row && (p.value_lo || p.value_hi); }
__host__ __device__ inline bool pred_has_tags(const PredArgs& p) {
  return p.tags_of_row && (p.tags_all || p.tags_any || p.tags_none);
}
__host__ __device__ inline bool pred_any(const PredArgs& p) { return pred_has_labels(p) || pred_has_value(p) || pred_has_tags(p); }

constexpr int kPredTileRows = 1024;  // rows per workgroup of k_pred_scatter / k_pred_count: four per thread

// the launch arguments of k_pred_compact
struct PredCompactArgs {
  FilterArgs f;                 // validity: f.n_items bounds the rows; deny bitmap and exclusion lists, any of them null
  PredArgs p;
  const int32_t* in_rows;       // i32[n_q, in_stride]
  const float* in_scores;       // f32, the same shape, or null (scores then read as 0)
  int in_stride;                // <= kMaxK
  int n_in;                     // entries of every query when n_valid is null
  const int32_t* n_valid;       // query i counts n_valid[i * nv_stride] entries
  int nv_stride;                //   (1: i32[n_q]; 6, from &level_topn[0][5]: a traversal's per-query level_topn)
  const int32_t* status;        // i32[n_q] or null: a query with a non-zero word counts none
  long long q0;                 // row i of the lists is query q0 + i of the call
  int k;
  const int64_t* item_ids;      // i64[n_items]; may be null when out_item_ids is
  int32_t* out_index;           // [n_q, k] each, any of them may be null
  float* out_scores;
  int64_t* out_item_ids;
  int32_t* out_pos;
  int32_t* n_out;               // i32[n_q] or null
};

// -inf over the failing rows of scores f32[n_q, n_items]; row i of the buffer is query q0 + i of the call
int launch_pred_scatter(const PredArgs& p, float* scores, long long n_items, long long q0, int n_q, hipStream_t st);
// the caller has held the shape to the kernel's limits IN FRONT OF ITS FIRST LAUNCH: 0 <= k, 0 <= in_stride <= 1024 (the checks
// in the launcher only restate that: behind a search they come too late to keep the call from writing)
int launch_pred_compact(const PredCompactArgs& a, long long n_q, hipStream_t st);
// counts[i] = rows of [0, f.n_items) that pass query i and the filter, i < n_queries
int launch_pred_count(const FilterArgs& f, const PredArgs& p, long long n_queries, long long* counts, hipStream_t st);

}  // namespace nann

#ifdef NANN_PREDICATE_IMPL  // the kernels: nann_filter_inst.hip only, behind NANN_FILTER_IMPL
namespace nann {

constexpr int kPredQueries = 16;                           // queries of a group: what a thread of the tile kernels walks
constexpr int kPredRowsPerThread = kPredTileRows / kFilterNT;
constexpr int kPredLabelSlots = 256;                       // hash slots of one query's label table in the tile kernels
constexpr int kPredRound = kPredLabelSlots / 2;            // labels a table takes per round: never more than half full
constexpr int32_t kPredEmpty = INT32_MIN;                  // the empty mark of a label table
static_assert(kPredRowsPerThread * kFilterNT == kPredTileRows && kPredRowsPerThread * kPredQueries == 64,
              "a thread's (query, row) verdicts are the bits of one 64-bit word");
static_assert(kFilterNT == kPredQueries * 16, "16 threads build one query's table");

// the label list of global query g, clamped as filter_list_range clamps: [*b, *e) within [0, n_labels], empty when inverted
__device__ __forceinline__ void pred_label_range(const PredArgs& p, long long g, long long* b, long long* e) {
  const long long lo = p.label_splits[g], hi = p.label_splits[g + 1];
  *b = min(max(lo, 0ll), p.n_labels);
  *e = max(*b, min(max(hi, 0ll), p.n_labels));
}
__device__ __forceinline__ bool pred_value_ok(float v, float lo, float hi) { return lo <= v && v <= hi; }
__device__ __forceinline__ bool pred_tags_ok(unsigned long long t, unsigned long long all, unsigned long long any,
                                             unsigned long long none) {
  return (t & all) == all && (any == 0ull || (t & any) != 0ull) && (t & none) == 0ull;
}

// open addressing with linear probing over `mask + 1` slots, of which the callers fill at most half: every probe ends.
// pred_tab_insert: the slot of `key` (!= empty), taken or shared with an equal key
__device__ __forceinline__ int pred_tab_insert(int32_t* tab, int h, int mask, int32_t key, int32_t empty) {
  for (;;) {
    const int32_t prev = atomicCAS(&tab[h], empty, key);
    if (prev == empty || prev == key) return h;
    h = (h + 1) & mask;
  }
}
// the slot that holds `key`, or -1
__device__ __forceinline__ int pred_tab_find(const int32_t* tab, int h, int mask, int32_t key, int32_t empty) {
  for (;;) {
    const int32_t at = tab[h];
    if (at == key) return h;
    if (at == empty) return -1;
    h = (h + 1) & mask;
  }
}
__device__ __forceinline__ int pred_hash8(int32_t l) { return (int)(((uint32_t)l * 2654435761u) >> 24); }

// ---- the tile walk of k_pred_scatter and k_pred_count ----------------------------------------------------------------------
struct PredTileLds {
  int32_t tab[kPredQueries][kPredLabelSlots];  // 16 KB: one label table per query of the group
  unsigned long long all[kPredQueries], any[kPredQueries], none[kPredQueries];
  long long lb[kPredQueries], le[kPredQueries];
  float lo[kPredQueries], hi[kPredQueries];
  int flags[kPredQueries];    // bit 0: label test, bit 1: value test, bit 2: tags test
  int has_min[kPredQueries];  // the query's list names the label kPredEmpty
};

// Thread tid owns rows tile0 + j * 256 + tid, j < 4, and the queries g0 .. g0 + n_g - 1 (n_g <= 16) of the call.  -> bit
// (q * 4 + j) set where row j FAILS query g0 + q; bits of rows at or beyond n_items mean nothing.  Uniform control flow: every
// thread of the workgroup calls it and reaches its barriers.
__device__ __forceinline__ unsigned long long pred_tile_fail(const PredArgs& p, long long n_items, long long g0, int n_g,
                                                             long long tile0, PredTileLds& s) {
  const int tid = threadIdx.x;
  if (tid < kPredQueries) {
    int fl = 0;
    long long b = 0, e = 0;
    float lo = -__builtin_inff(), hi = __builtin_inff();
    unsigned long long ta = 0ull, ty = 0ull, tn = 0ull;
    if (tid < n_g) {
      const long long g = g0 + tid;
      if (pred_has_labels(p)) {
        pred_label_range(p, g, &b, &e);
        if (e > b) fl |= 1;
      }
      if (pred_has_value(p)) {
        fl |= 2;
        if (p.value_lo) lo = p.value_lo[g];
        if (p.value_hi) hi = p.value_hi[g];
      }
      if (pred_has_tags(p)) {
        fl |= 4;
        if (p.tags_all) ta = p.tags_all[g];
        if (p.tags_any) ty = p.tags_any[g];
        if (p.tags_none) tn = p.tags_none[g];
      }
    }
    s.flags[tid] = fl;
    s.has_min[tid] = 0;
    s.lb[tid] = b;
    s.le[tid] = e;
    s.lo[tid] = lo;
    s.hi[tid] = hi;
    s.all[tid] = ta;
    s.any[tid] = ty;
    s.none[tid] = tn;
  }
  __syncthreads();
  int tests = 0;
  long long longest = 0;
#pragma unroll
  for (int q = 0; q < kPredQueries; ++q) {
    tests |= s.flags[q];
    if (s.flags[q] & 1) longest = max(longest, s.le[q] - s.lb[q]);
  }
  if (tests == 0) return 0ull;  // (uniform) no query of the group has a condition
  int32_t lab[kPredRowsPerThread];
  float val[kPredRowsPerThread];
  unsigned long long tag[kPredRowsPerThread];
#pragma unroll
  for (int j = 0; j < kPredRowsPerThread; ++j) {
    const long long r = tile0 + j * kFilterNT + tid;
    const bool in = r < n_items;
    lab[j] = (tests & 1) && in ? p.label_of_row[r] : 0;
    val[j] = (tests & 2) && in ? p.value_of_row[r] : 0.0f;
    tag[j] = (tests & 4) && in ? p.tags_of_row[r] : 0ull;
  }
  unsigned long long fail = 0ull;
  for (int q = 0; q < kPredQueries; ++q) {
    const int fl = s.flags[q];
    if (fl & 2) {
      const float lo = s.lo[q], hi = s.hi[q];
#pragma unroll
      for (int j = 0; j < kPredRowsPerThread; ++j)
        if (!pred_value_ok(val[j], lo, hi)) fail |= 1ull << (q * kPredRowsPerThread + j);
    }
    if (fl & 4) {
      const unsigned long long ta = s.all[q], ty = s.any[q], tn = s.none[q];
#pragma unroll
      for (int j = 0; j < kPredRowsPerThread; ++j)
        if (!pred_tags_ok(tag[j], ta, ty, tn)) fail |= 1ull << (q * kPredRowsPerThread + j);
    }
  }
  if (tests & 1) {
    unsigned long long match = 0ull;
    const long long rounds = (longest + kPredRound - 1) / kPredRound;
    for (long long rd = 0; rd < rounds; ++rd) {
      for (int i = tid; i < kPredQueries * kPredLabelSlots; i += kFilterNT) (&s.tab[0][0])[i] = kPredEmpty;
      __syncthreads();
      {
        const int q = tid >> 4;  // 16 threads fill the table of one query
        if (s.flags[q] & 1) {
          const long long base = s.lb[q] + rd * kPredRound, end = s.le[q];
          for (int i = tid & 15; i < kPredRound; i += 16) {
            if (base + i >= end) break;
            const int32_t l = p.labels[base + i];
            if (l == kPredEmpty) s.has_min[q] = 1;
            else pred_tab_insert(s.tab[q], pred_hash8(l), kPredLabelSlots - 1, l, kPredEmpty);
          }
        }
      }
      __syncthreads();
      for (int q = 0; q < kPredQueries; ++q) {
        if (!(s.flags[q] & 1) || s.lb[q] + rd * kPredRound >= s.le[q]) continue;  // (uniform) no test, or the list has ended
#pragma unroll
        for (int j = 0; j < kPredRowsPerThread; ++j)
          if (lab[j] != kPredEmpty && pred_tab_find(s.tab[q], pred_hash8(lab[j]), kPredLabelSlots - 1, lab[j], kPredEmpty) >= 0)
            match |= 1ull << (q * kPredRowsPerThread + j);
      }
      __syncthreads();  // (the tables are read for the last time: the next round clears them)
    }
    for (int q = 0; q < kPredQueries; ++q) {
      if (!(s.flags[q] & 1)) continue;
      const bool has_min = s.has_min[q] != 0;
#pragma unroll
      for (int j = 0; j < kPredRowsPerThread; ++j) {
        const unsigned long long bit = 1ull << (q * kPredRowsPerThread + j);
        if (!((match & bit) || (has_min && lab[j] == kPredEmpty))) fail |= bit;
      }
    }
  }
  return fail;
}

// grid: (tiles of kPredTileRows rows, groups of kPredQueries score rows)
__global__ __launch_bounds__(kFilterNT) void k_pred_scatter(PredArgs p, long long n_items, long long q0, int n_q,
                                                            float* __restrict__ scores) {
  __shared__ PredTileLds s;
  const int qb = (int)blockIdx.y * kPredQueries, n_g = min(kPredQueries, n_q - qb);
  const long long tile0 = (long long)blockIdx.x * kPredTileRows;
  const unsigned long long fail = pred_tile_fail(p, n_items, q0 + qb, n_g, tile0, s);
  if (fail == 0ull) return;
  for (int q = 0; q < n_g; ++q) {
    if (((fail >> (q * kPredRowsPerThread)) & 0xfull) == 0ull) continue;
    float* row = scores + (size_t)(qb + q) * n_items;
#pragma unroll
    for (int j = 0; j < kPredRowsPerThread; ++j) {
      const long long r = tile0 + j * kFilterNT + threadIdx.x;
      if (((fail >> (q * kPredRowsPerThread + j)) & 1ull) && r < n_items) row[r] = filter_neg_inf();
    }
  }
}

// grid: (tiles, groups of kPredQueries queries from q0 on); counts is zeroed in front of the launch.  The exclusion lists of
// the group stream through every tile's workgroup, which keeps one bit per (query, row of the tile): a row listed twice
// counts once.
__global__ __launch_bounds__(kFilterNT) void k_pred_count(FilterArgs f, PredArgs p, long long q0, long long n_queries,
                                                          unsigned long long* __restrict__ counts) {
  __shared__ PredTileLds s;
  __shared__ uint32_t excl[kPredQueries][kPredTileRows / 32];
  __shared__ int cnt[kPredQueries];
  const int tid = threadIdx.x, lane = tid & 63;
  const long long g0 = q0 + (long long)blockIdx.y * kPredQueries;
  const int n_g = (int)min((long long)kPredQueries, n_queries - g0);
  const long long tile0 = (long long)blockIdx.x * kPredTileRows;
  const unsigned long long fail = pred_tile_fail(p, f.n_items, g0, n_g, tile0, s);
  const bool lists = filter_has_lists(f);
  if (tid < kPredQueries) cnt[tid] = 0;
  if (lists)
    for (int i = tid; i < kPredQueries * (kPredTileRows / 32); i += kFilterNT) (&excl[0][0])[i] = 0u;
  __syncthreads();
  if (lists) {
    for (int q = 0; q < n_g; ++q) {
      long long b, e;
      filter_list_range(f, g0 + q, &b, &e);
      for (long long i = b + tid; i < e; i += kFilterNT) {
        const long long r = (long long)f.rows[i] - tile0;
        if (r >= 0 && r < kPredTileRows) atomicOr(&excl[q][r >> 5], 1u << (int)(r & 31));
      }
    }
    __syncthreads();
  }
  bool live[kPredRowsPerThread];
#pragma unroll
  for (int j = 0; j < kPredRowsPerThread; ++j) {
    const long long r = tile0 + j * kFilterNT + tid;
    live[j] = r < f.n_items;
    if (live[j] && f.deny_bits) live[j] = ((f.deny_bits[r >> 5] >> (int)(r & 31)) & 1u) == 0u;
  }
  for (int q = 0; q < n_g; ++q) {
    int c = 0;
#pragma unroll
    for (int j = 0; j < kPredRowsPerThread; ++j) {
      bool ok = live[j] && !((fail >> (q * kPredRowsPerThread + j)) & 1ull);
      if (ok && lists) ok = ((excl[q][(j * kFilterNT + tid) >> 5] >> (tid & 31)) & 1u) == 0u;
      c += __popcll(__ballot(ok));
    }
    if (lane == 0 && c) atomicAdd(&cnt[q], c);
  }
  __syncthreads();
  if (tid < n_g && cnt[tid]) atomicAdd(&counts[g0 + tid], (unsigned long long)cnt[tid]);
}

// One workgroup per query, the walk of k_filter_compact: validity, the deny bitmap, the exclusion list through the row table;
// then the predicate -- the labels of the entries still standing go into the same table, the query's label list streams through
// it -- and the ballot + prefix compaction, order kept.
__global__ __launch_bounds__(kFilterNT) void k_pred_compact(PredCompactArgs a) {
  constexpr int W = kFilterNT / 64;
  __shared__ int32_t tab[kFilterSlots];
  __shared__ int32_t hit[kFilterSlots];
  __shared__ int cnt[kFilterPasses * W];
  __shared__ int has_min;
  const size_t qi = blockIdx.x;
  const long long g = a.q0 + (long long)qi;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int n = a.n_valid ? a.n_valid[qi * (size_t)a.nv_stride] : a.n_in;
  if (a.status && a.status[qi] != 0) n = 0;
  n = max(0, min(n, min(a.in_stride, kMaxK)));
  long long lb = 0, le = 0, pb = 0, pe = 0;
  if (filter_has_lists(a.f)) filter_list_range(a.f, g, &lb, &le);
  if (pred_has_labels(a.p)) pred_label_range(a.p, g, &pb, &pe);
  const bool lists = le > lb && n > 0;   // (uniform over the workgroup)
  const bool labels = pe > pb && n > 0;  // (uniform)
  if (lists) {
    for (int i = tid; i < kFilterSlots; i += kFilterNT) { tab[i] = -1; hit[i] = 0; }
    __syncthreads();
  }
  int32_t row[kFilterPasses];
  float score[kFilterPasses];
  int slot[kFilterPasses];
  bool ok[kFilterPasses];
#pragma unroll
  for (int j = 0; j < kFilterPasses; ++j) {
    const int e = j * kFilterNT + tid;
    row[j] = e < n ? a.in_rows[qi * (size_t)a.in_stride + e] : -1;
    score[j] = e < n && a.in_scores ? a.in_scores[qi * (size_t)a.in_stride + e] : 0.0f;
    ok[j] = row[j] >= 0 && (long long)row[j] < a.f.n_items;
    if (ok[j] && a.f.deny_bits) ok[j] = ((a.f.deny_bits[row[j] >> 5] >> (row[j] & 31)) & 1u) == 0u;
    slot[j] = -1;
    if (lists && ok[j]) slot[j] = pred_tab_insert(tab, filter_hash(row[j]), kFilterSlots - 1, row[j], -1);  // (a repeated row shares its slot)
  }
  if (lists) {
    __syncthreads();
    for (long long i = lb + tid; i < le; i += kFilterNT) {
      const int32_t r = a.f.rows[i];
      if (r < 0 || (long long)r >= a.f.n_items) continue;
      const int h = pred_tab_find(tab, filter_hash(r), kFilterSlots - 1, r, -1);  // (ends: at most kMaxK of the slots are taken)
      if (h >= 0) hit[h] = 1;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kFilterPasses; ++j)
      if (slot[j] >= 0 && hit[slot[j]]) ok[j] = false;
  }
  // ---- the predicate: value and tags by a gather per entry, labels through the table
  if (pred_has_value(a.p)) {
    const float lo = a.p.value_lo ? a.p.value_lo[g] : -__builtin_inff(), hi = a.p.value_hi ? a.p.value_hi[g] : __builtin_inff();
#pragma unroll
    for (int j = 0; j < kFilterPasses; ++j)
      if (ok[j]) ok[j] = pred_value_ok(a.p.value_of_row[row[j]], lo, hi);
  }
  if (pred_has_tags(a.p)) {
    const unsigned long long ta = a.p.tags_all ? a.p.tags_all[g] : 0ull, ty = a.p.tags_any ? a.p.tags_any[g] : 0ull,
                             tn = a.p.tags_none ? a.p.tags_none[g] : 0ull;
#pragma unroll
    for (int j = 0; j < kFilterPasses; ++j)
      if (ok[j]) ok[j] = pred_tags_ok(a.p.tags_of_row[row[j]], ta, ty, tn);
  }
  if (labels) {
    __syncthreads();  // (the row table and its flags are read for the last time: the labels take their place)
    for (int i = tid; i < kFilterSlots; i += kFilterNT) { tab[i] = kPredEmpty; hit[i] = 0; }
    if (tid == 0) has_min = 0;
    __syncthreads();
    int32_t lab[kFilterPasses];
#pragma unroll
    for (int j = 0; j < kFilterPasses; ++j) {
      lab[j] = ok[j] ? a.p.label_of_row[row[j]] : kPredEmpty;
      slot[j] = -1;
      if (ok[j] && lab[j] != kPredEmpty) slot[j] = pred_tab_insert(tab, filter_hash(lab[j]), kFilterSlots - 1, lab[j], kPredEmpty);
    }
    __syncthreads();
    for (long long i = pb + tid; i < pe; i += kFilterNT) {
      const int32_t l = a.p.labels[i];
      if (l == kPredEmpty) { has_min = 1; continue; }
      const int h = pred_tab_find(tab, filter_hash(l), kFilterSlots - 1, l, kPredEmpty);
      if (h >= 0) hit[h] = 1;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kFilterPasses; ++j)
      if (ok[j]) ok[j] = slot[j] >= 0 ? hit[slot[j]] != 0 : has_min != 0;
  }
  // ---- the passing entries, compacted in list order
  int rank[kFilterPasses];
#pragma unroll
  for (int j = 0; j < kFilterPasses; ++j) {
    const unsigned long long m = __ballot(ok[j]);
    rank[j] = (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
    if (lane == 0) cnt[j * W + wave] = __popcll(m);
  }
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int j = 0; j < kFilterPasses; ++j) {
    int base = 0;
#pragma unroll
    for (int i = 0; i < kFilterPasses * W; ++i) {
      const int c = cnt[i];
      if (i < j * W + wave) base += c;
      if (j == 0) total += c;
    }
    const int pos = base + rank[j];
    if (ok[j] && pos < a.k) {
      const size_t at = qi * (size_t)a.k + pos;
      if (a.out_index) a.out_index[at] = row[j];
      if (a.out_scores) a.out_scores[at] = score[j];
      if (a.out_item_ids) a.out_item_ids[at] = a.item_ids[row[j]];
      if (a.out_pos) a.out_pos[at] = j * kFilterNT + tid;
    }
  }
  total = min(total, a.k);
  for (int i = total + tid; i < a.k; i += kFilterNT) {
    const size_t at = qi * (size_t)a.k + i;
    if (a.out_index) a.out_index[at] = 0;
    if (a.out_scores) a.out_scores[at] = 0.0f;
    if (a.out_item_ids) a.out_item_ids[at] = 0;
    if (a.out_pos) a.out_pos[at] = 0;
  }
  if (a.n_out && tid == 0) a.n_out[qi] = total;
}

}  // namespace nann
#endif
