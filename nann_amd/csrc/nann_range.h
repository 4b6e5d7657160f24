// nann_range.h -- threshold ("range") selection of the exhaustive search (nann_search_all_range): every row of a query whose
// score is at or above the query's cut, in ascending row order, into ragged outputs.  The reference has no such call; nothing
// here restates a line of it.
//
// The second selection stage over scores f32[chunk, n_items] (nann_scan.h), in the place of the slab top-k and the merge:
// it runs behind scoring and behind launch_filter_scatter, which has written -inf over the denied scores.
//   match          s >= thr[query] and s != -inf, IEEE: -0 >= +0 holds, a NaN score or a NaN cut matches nothing, and -inf --
//                  a denied row's mark -- is never returned, whatever the cut
//   k_range_count  grid (block of kRangeBlockRows positions, query): the matches of the block, i32 into the workspace
//   k_range_scan   one workgroup per query: the block counts become their exclusive prefix, in place, in a loop over any
//                  number of blocks; the query's total goes behind the counts
//   k_range_splits one workgroup: out_row_splits[c0 + i + 1] = out_row_splits[c0 + i] + total_i.  The first chunk writes
//                  out_row_splits[0] = 0, a later one reads the last split of the chunk before it (stream order)
//   k_range_fill   the grid of k_range_count: the matches again, each to out_row_splits[query] + (block prefix) + (rank in
//                  block) -- a position no atomic decides -- and EVERY store guarded by pos < capacity
// A block is a run of kRangeBlockRows POSITIONS of the score buffer that begins on a 16-byte boundary: a query's scores begin
// wherever query * n_items falls, so its first block starts up to three positions in front of its row 0 and every load is an
// aligned, coalesced 16 bytes per lane; positions outside the query's row never match.  Within a block the order is (pass,
// wavefront, lane, element) = ascending position = ascending row: four ballots per pass and mbcnt give a lane its rank.
#pragma once
#include <cstddef>
#include <cstdint>

#include "nann_search.h"

namespace nann {

constexpr int kRangeNT = 256;                                    // threads of every kernel here
constexpr int kRangePasses = 2;                                  // 16-byte loads per thread of a block
constexpr int kRangeBlockRows = kRangeNT * 4 * kRangePasses;     // positions of a block: 2048

// the range form of a launch_scan (ScanArgs::range): the outputs are ragged, the k of the call is not read
struct ScanRange {
  const float* thr;     // device f32[n_queries]: the cut of every query of the call
  long long capacity;   // entries of the outputs; a position at or beyond it is dropped
  int64_t* row_splits;  // device i64[n_queries + 1]: the true counts, whatever the capacity
  int32_t* counts;      // workspace i32[chunk, n_blocks]: block counts, then their exclusive prefixes; i32[chunk] totals behind
  int n_blocks;         // range_n_blocks(n_items)
};
// blocks of a query: its n_items positions and the up to three in front of them
inline int range_n_blocks(long long n_items) { return (int)((n_items + 3 + kRangeBlockRows - 1) / kRangeBlockRows); }
inline size_t range_counts_bytes(int chunk, long long n_items) {
  return ((size_t)chunk * ((size_t)range_n_blocks(n_items) + 1) * 4 + 255) & ~(size_t)255;
}
// count, scan, splits, fill for the n_q queries c0 .. c0 + n_q - 1 of the call, whose scores lie in scores f32[n_q, n_items];
// the buffer is readable up to the next 16-byte boundary behind its last score (nann_scan_inst.hip)
int launch_range(const ScanRange& r, const float* scores, long long n_items, long long c0, int n_q, const int64_t* item_ids,
                 int64_t* out_item_ids, float* out_scores, int32_t* out_index, hipStream_t st);

}  // namespace nann

#ifdef NANN_SCAN_IMPL  // the kernels: nann_scan_inst.hip only
namespace nann {

// What a thread holds of block blockIdx.x of query blockIdx.y: pass p is the 16 bytes at position at[p] of the score buffer,
// bit j of m[p] says that element j of them is a row of the query and matches.
struct RangeBlock {
  f32x4v s[kRangePasses];
  size_t at[kRangePasses];
  unsigned m[kRangePasses];
  size_t begin;  // position of the query's row 0
};
__device__ __forceinline__ void range_load(const float* __restrict__ scores, long long n_items, float thr, RangeBlock* b) {
  const size_t begin = (size_t)blockIdx.y * (size_t)n_items, end = begin + (size_t)n_items;
  const size_t g0 = (begin >> 2) + (size_t)blockIdx.x * (kRangeBlockRows / 4);
  b->begin = begin;
#pragma unroll
  for (int p = 0; p < kRangePasses; ++p) {
    const size_t at = (g0 + (size_t)p * kRangeNT + threadIdx.x) * 4;
    b->at[p] = at;
    b->m[p] = 0u;
    b->s[p] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    if (at < end) {  // (the 16 bytes begin inside the row or up to three positions in front of it, and end within 16 B of its end)
      b->s[p] = *reinterpret_cast<const f32x4v*>(scores + at);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float s = b->s[p][j];
        const bool in = at + j >= begin && at + j < end;
        if (in && s >= thr && s != -__builtin_inff()) b->m[p] |= 1u << j;
      }
    }
  }
}

__device__ __forceinline__ int range_lanes_below(unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
}

// counts[query][block] = matches of the block
__global__ __launch_bounds__(kRangeNT) void k_range_count(const float* __restrict__ scores, long long n_items,
                                                          const float* __restrict__ thr, long long c0,
                                                          int32_t* __restrict__ counts) {
  __shared__ int wave_cnt[kRangeNT / 64];
  RangeBlock b;
  range_load(scores, n_items, thr[c0 + blockIdx.y], &b);
  int c = 0;
#pragma unroll
  for (int p = 0; p < kRangePasses; ++p)
#pragma unroll
    for (int j = 0; j < 4; ++j) c += __popcll(__ballot((b.m[p] >> j) & 1u));
  if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < kRangeNT / 64; ++w) t += wave_cnt[w];
    counts[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
  }
}

// One workgroup per query: counts[query][0 .. n_blocks) -> their exclusive prefix, kRangeNT blocks per step of a loop that
// carries the sum so far; totals[query] = the sum of all.  (A query holds fewer than 2^31 rows: the sums fit 32 bits.)
__global__ __launch_bounds__(kRangeNT) void k_range_scan(int32_t* __restrict__ counts, int n_blocks, int32_t* __restrict__ totals) {
  __shared__ int part[kRangeNT];
  int32_t* row = counts + (size_t)blockIdx.x * n_blocks;
  const int tid = threadIdx.x;
  int carry = 0;
  for (int i0 = 0; i0 < n_blocks; i0 += kRangeNT) {
    const int i = i0 + tid;
    const int c = i < n_blocks ? row[i] : 0;
    part[tid] = c;
    __syncthreads();
    for (int step = 1; step < kRangeNT; step <<= 1) {  // inclusive scan of the step's counts
      const int v = tid >= step ? part[tid - step] : 0;
      __syncthreads();
      part[tid] += v;
      __syncthreads();
    }
    if (i < n_blocks) row[i] = carry + part[tid] - c;
    carry += part[kRangeNT - 1];
    __syncthreads();  // (part is written again by the next step)
  }
  if (tid == 0) totals[blockIdx.x] = carry;
}

// One workgroup: the splits of the chunk's queries, continued from the chunk before
__global__ __launch_bounds__(kRangeNT) void k_range_splits(const int32_t* __restrict__ totals, int n_q, long long c0,
                                                           int64_t* __restrict__ row_splits) {
  __shared__ int t[kRangeNT];
  const int tid = threadIdx.x;
  const long long base = c0 == 0 ? 0ll : (long long)row_splits[c0];
  if (c0 == 0 && tid == 0) row_splits[0] = 0;
  t[tid] = tid < n_q ? totals[tid] : 0;  // (n_q <= kScanMaxChunk <= kRangeNT: launch_range asserts it)
  __syncthreads();
  long long sum = base;
  for (int j = 0; j <= tid; ++j) sum += t[j];
  if (tid < n_q) row_splits[c0 + tid + 1] = sum;
}

// The matches of a block to their places.  prefix = counts behind k_range_scan.
__global__ __launch_bounds__(kRangeNT) void k_range_fill(const float* __restrict__ scores, long long n_items,
                                                         const float* __restrict__ thr, long long c0,
                                                         const int32_t* __restrict__ prefix, const int64_t* __restrict__ row_splits,
                                                         long long capacity, const int64_t* __restrict__ item_ids,
                                                         int64_t* __restrict__ out_item_ids, float* __restrict__ out_scores,
                                                         int32_t* __restrict__ out_index) {
  constexpr int W = kRangeNT / 64;
  __shared__ int cnt[kRangePasses * W];
  RangeBlock b;
  range_load(scores, n_items, thr[c0 + blockIdx.y], &b);
  const int wave = threadIdx.x >> 6;
  int rank[kRangePasses];  // matches of the pass's wavefront in the lanes below this one
#pragma unroll
  for (int p = 0; p < kRangePasses; ++p) {
    int below = 0, all = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned long long m = __ballot((b.m[p] >> j) & 1u);
      below += range_lanes_below(m);
      all += __popcll(m);
    }
    rank[p] = below;
    if ((threadIdx.x & 63) == 0) cnt[p * W + wave] = all;
  }
  __syncthreads();
  const long long q_base = (long long)row_splits[c0 + blockIdx.y] + prefix[(size_t)blockIdx.y * gridDim.x + blockIdx.x];
#pragma unroll
  for (int p = 0; p < kRangePasses; ++p) {
    int base = 0;
#pragma unroll
    for (int i = 0; i < kRangePasses * W; ++i)
      if (i < p * W + wave) base += cnt[i];
    long long pos = q_base + base + rank[p];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!((b.m[p] >> j) & 1u)) continue;
      if (pos >= 0 && pos < capacity) {  // the guard of every store below: a position at or beyond capacity is dropped
        const long long r = (long long)(b.at[p] + j - b.begin);
        out_item_ids[pos] = item_ids[r];
        if (out_scores) out_scores[pos] = b.s[p][j];
        if (out_index) out_index[pos] = (int32_t)r;
      }
      ++pos;
    }
  }
}

}  // namespace nann
#endif
