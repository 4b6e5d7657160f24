// nann_filter.h -- filtered retrieval: a deny bitmap for every query of a call and an exclusion list per query (nann_filter,
// include/nann_hip.h).  The reference has no such feature; nothing here restates a line of it.
//
// The filter is applied AFTER the fact, by kernels of its own next to the search kernels, which do not change:
//   * exhaustive search (nann_scan.h): the scores of a chunk lie in f32[chunk, n_items] between scoring and selection.
//     k_filter_scatter_bits / k_filter_scatter_lists write -inf over the denied positions -- they load nothing from that
//     buffer and their cost grows with what is denied, not with the corpus -- and the selection runs as it is;
//   * traversal (nann_search.h): asked for a fetch width F = level_topn[5] as wide as its pool, the last stage returns the whole
//     pool ranked; the first k allowed entries of that list are the answer.  Denied rows still guide the walk.
// k_filter_compact produces the final rows of both: a ranked list of at most 1024 (row, score) pairs -> the allowed pairs in
// order, item_ids[row], zeros behind them and their count.  The exhaustive forms run it on the merge's k-wide list, which
// removes the denied rows that surface when a query has fewer than k allowed rows.
//
// Malformed filters never fault: a listed row outside [0, n_items) denies nothing, a list's range is clamped to [0, n_excl]
// and an inverted one is empty, bitmap bits at or beyond n_items are ignored.
#pragma once
#include <cstdint>

#include "nann_search.h"

namespace nann {

// a nann_filter as the kernels take it (all pointers device; any of them may be null)
struct FilterArgs {
  const uint32_t* deny_bits;  // ceil(n_items / 32) words: row r is denied when bit (r & 31) of word (r >> 5) is set
  const int64_t* splits;      // i64[n_queries + 1] into rows, by the GLOBAL query number of the call
  const int32_t* rows;        // i32[n_excl] internal row numbers
  long long n_excl;
  long long n_items;
};
__host__ __device__ inline bool filter_has_lists(const FilterArgs& f) { return f.splits && f.rows && f.n_excl > 0; }

// -inf over the denied rows of scores f32[n_q, n_items]; row i of the buffer is query q0 + i of the call
int launch_filter_scatter(const FilterArgs& f, float* scores, long long q0, int n_q, hipStream_t st);
// Query i (of n_q; q0 + i of the call) has the ranked list in_rows / in_scores [i * in_stride, +n_i): n_i = tq[6 i + 5] where
// tq is given, else n_in; 0 where status[i] != 0.  Its first k allowed pairs go to row i of the outputs ([n_q, k]; out_scores,
// out_index and n_out may be null).
int launch_filter_compact(const FilterArgs& f, const int32_t* in_rows, const float* in_scores, int in_stride, int n_in,
                          const int32_t* tq, const int32_t* status, long long q0, long long n_q, int k, const int64_t* item_ids,
                          int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* n_out, hipStream_t st);

}  // namespace nann

#ifdef NANN_FILTER_IMPL  // the kernels: nann_filter_inst.hip only
namespace nann {

constexpr int kFilterNT = 256;                       // threads of every kernel here
constexpr int kFilterPasses = kMaxK / kFilterNT;     // list entries per thread of k_filter_compact
constexpr int kFilterSlots = 2048;                   // hash slots of k_filter_compact: twice the longest list
constexpr int kFilterScatterQueries = 16;            // score rows a thread of k_filter_scatter_bits writes
static_assert(kFilterPasses * kFilterNT == kMaxK && kFilterSlots >= 2 * kMaxK, "the table is never more than half full");

__device__ __forceinline__ float filter_neg_inf() { return __uint_as_float(0xff800000u); }

// One thread owns a 32-row word of the bitmap (grid.x) and up to kFilterScatterQueries score rows (grid.y).
__global__ __launch_bounds__(kFilterNT) void k_filter_scatter_bits(const uint32_t* __restrict__ bits, long long n_items, int n_q,
                                                                   float* __restrict__ scores) {
  const long long w = (long long)blockIdx.x * kFilterNT + threadIdx.x;
  const long long r0 = w * 32;
  if (r0 >= n_items) return;
  uint32_t m = bits[w];
  if (n_items - r0 < 32) m &= (1u << (int)(n_items - r0)) - 1u;  // (bits at or beyond n_items: ignored)
  if (m == 0u) return;
  const int qb = (int)blockIdx.y * kFilterScatterQueries, qe = min(n_q, qb + kFilterScatterQueries);
  for (int qi = qb; qi < qe; ++qi) {
    float* row = scores + (size_t)qi * n_items + r0;
    for (uint32_t mm = m; mm; mm &= mm - 1u) row[__ffs((int)mm) - 1] = filter_neg_inf();
  }
}

// the exclusion list of global query g, clamped: [*b, *e) within [0, n_excl], empty when inverted
__device__ __forceinline__ void filter_list_range(const FilterArgs& f, long long g, long long* b, long long* e) {
  const long long lo = f.splits[g], hi = f.splits[g + 1];
  *b = min(max(lo, 0ll), f.n_excl);
  *e = max(*b, min(max(hi, 0ll), f.n_excl));
}

// one workgroup per query of the chunk: -inf at every in-range listed row of its score row
__global__ __launch_bounds__(kFilterNT) void k_filter_scatter_lists(FilterArgs f, long long q0, float* __restrict__ scores) {
  long long b, e;
  filter_list_range(f, q0 + blockIdx.x, &b, &e);
  float* row = scores + (size_t)blockIdx.x * f.n_items;
  for (long long i = b + threadIdx.x; i < e; i += kFilterNT) {
    const int32_t r = f.rows[i];
    if (r >= 0 && (long long)r < f.n_items) row[r] = filter_neg_inf();
  }
}

__device__ __forceinline__ int filter_hash(int32_t r) { return (int)(((uint32_t)r * 2654435761u) >> 21); }  // 11 bits

// One workgroup per query.  Entry e of the list belongs to thread e % 256 in pass e / 256, so that a wavefront of a pass
// holds 64 consecutive entries: a ballot per (pass, wavefront) and an exclusive prefix over the 16 counts give every allowed
// entry its place, order kept.  Exclusion list, whatever its order and length: the list's rows (distinct: a TopKV2 output
// over distinct nodes; a repeated row would share its slot) go into an LDS hash table with linear probing, the query's
// exclusion list streams through it and flags the slots it finds.
__global__ __launch_bounds__(kFilterNT) void k_filter_compact(FilterArgs f, const int32_t* __restrict__ in_rows,
                                                              const float* __restrict__ in_scores, int in_stride, int n_in,
                                                              const int32_t* __restrict__ tq, const int32_t* __restrict__ status,
                                                              long long q0, int k, const int64_t* __restrict__ item_ids,
                                                              int64_t* __restrict__ out_item_ids, float* __restrict__ out_scores,
                                                              int32_t* __restrict__ out_index, int32_t* __restrict__ n_out) {
  constexpr int W = kFilterNT / 64;
  __shared__ int32_t tab[kFilterSlots];
  __shared__ int32_t hit[kFilterSlots];
  __shared__ int cnt[kFilterPasses * W];
  const size_t qi = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int n = tq ? tq[qi * 6 + 5] : n_in;
  if (status && status[qi] != 0) n = 0;
  n = max(0, min(n, min(in_stride, kMaxK)));
  long long lb = 0, le = 0;
  if (filter_has_lists(f)) filter_list_range(f, q0 + (long long)qi, &lb, &le);
  const bool lists = le > lb && n > 0;  // (uniform over the workgroup)
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
    row[j] = e < n ? in_rows[qi * in_stride + e] : -1;
    score[j] = e < n ? in_scores[qi * in_stride + e] : 0.0f;
    ok[j] = row[j] >= 0 && (long long)row[j] < f.n_items;
    if (ok[j] && f.deny_bits) ok[j] = ((f.deny_bits[row[j] >> 5] >> (row[j] & 31)) & 1u) == 0u;  // one gathered word per entry
    slot[j] = -1;
    if (lists && ok[j]) {
      int h = filter_hash(row[j]);
      for (;;) {
        const int32_t prev = atomicCAS(&tab[h], -1, row[j]);
        if (prev == -1 || prev == row[j]) break;
        h = (h + 1) & (kFilterSlots - 1);
      }
      slot[j] = h;
    }
  }
  if (lists) {
    __syncthreads();
    for (long long i = lb + tid; i < le; i += kFilterNT) {
      const int32_t r = f.rows[i];
      if (r < 0 || (long long)r >= f.n_items) continue;
      int h = filter_hash(r);
      for (;;) {  // (ends: at most kMaxK of the kFilterSlots slots are taken)
        const int32_t key = tab[h];
        if (key == r) hit[h] = 1;
        if (key == r || key == -1) break;
        h = (h + 1) & (kFilterSlots - 1);
      }
    }
    __syncthreads();
  }
  int rank[kFilterPasses];
#pragma unroll
  for (int j = 0; j < kFilterPasses; ++j) {
    if (slot[j] >= 0 && hit[slot[j]]) ok[j] = false;
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
    if (ok[j] && pos < k) {
      const size_t at = qi * (size_t)k + pos;
      out_item_ids[at] = item_ids[row[j]];
      if (out_scores) out_scores[at] = score[j];
      if (out_index) out_index[at] = row[j];
    }
  }
  total = min(total, k);
  for (int i = total + tid; i < k; i += kFilterNT) {
    const size_t at = qi * (size_t)k + i;
    out_item_ids[at] = 0;
    if (out_scores) out_scores[at] = 0.0f;
    if (out_index) out_index[at] = 0;
  }
  if (n_out && tid == 0) n_out[qi] = total;
}

}  // namespace nann
#endif
