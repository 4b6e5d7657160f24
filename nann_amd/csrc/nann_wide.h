// nann_wide.h -- the wide selection of the exhaustive search (nann_search_all_wide, nann_search_all_model_wide) and on its own
// (nann_select_wide): the exact top k of every query for k up to kWideMaxK = 16384, TopKV2 order, at a cost that does not grow
// with k as the slab top-k's does.  The reference has no such call; nothing here restates a line of it.
//
// The third selection stage over scores f32[chunk, n_items] (nann_scan.h), in the place of the slab top-k and the merge: it runs
// behind scoring, launch_filter_scatter and launch_pred_scatter, which have written -inf over the denied scores.  A row whose
// score is -inf is never returned (the range search's rule): n_out = min(k, rows that are not -inf).
//   1. the cut      a most-significant-digit radix select on score_key (nann_device.h: -0 and +0 tie), digits of 11, 11 and 10
//                   bits.  k_wide_hist<PASS>, grid (block of positions, query): an LDS histogram of the digit over the rows whose
//                   higher digits equal the prefix found so far, its non-zero bins flushed with integer atomic adds (sums of
//                   integers: any order gives the same bits).  k_wide_pick<PASS>, one workgroup per query: the bin that holds the
//                   rank, the rank that remains inside it, the rows above it.  Behind pass 2: T = the key of the k-th largest
//                   valid score, n_gt = rows with key > T, m = k - n_gt = the quota of rows with key == T.  A query with at most
//                   k valid rows takes them all (T = 0, m = k) and skips passes 1 and 2.
//   2. the gather   k_wide_count / k_range_scan / k_wide_fill: nann_range.h's count, scan and fill with two counters per block.
//                   A row is taken iff key > T, or key == T and fewer than m rows of key T precede it in row order; its place is
//                   (gt before it) + min(eq before it, m) -- no atomic decides a position, and EVERY store is guarded by
//                   pos < k.  Into the staging list u64[chunk, k]: (key << 32) | ~row.
//   3. the sort     k_wide_sort, one workgroup per query: a bitonic network over the composites in LDS, descending -- key
//                   descending, row ascending; the composites are distinct -- then item ids, the ORIGINAL score bits re-read from
//                   the buffer (a key has lost the sign of a zero), row numbers, zeros behind n_out.
// Blocks are nann_range.h's: runs of kRangeBlockRows positions that begin on a 16-byte boundary, so that a query's first block
// starts up to three positions in front of its row 0; positions outside the query's row never count.  `limit` is the number of
// floats readable from the base of the buffer: the 16 bytes that would cross it are read one float at a time (nann_select_wide
// reads a caller's matrix, which ends where it ends).
// NaN scores are outside the contract; every kernel sees the same key for the same bits, so the counts agree, and nothing is
// stored outside the outputs.
#pragma once
#include <cstddef>
#include <cstdint>

#include "nann_range.h"
#include "nann_search.h"

namespace nann {

constexpr int kWideMaxK = 16384;      // capacity of k_wide_sort: 16384 x 8 B = 128 KB of LDS (NANN_WIDE_MAX_K)
constexpr int kWideBins = 2048;       // bins of a pass's histogram (pass 2 uses 1024 of them)
constexpr int kWidePasses = 3;
constexpr int kWideStateInts = 8;     // per query: [T / prefix, rank, n_gt, n_valid, m, done, -, -]
constexpr int kWideSortNT = 1024;
constexpr int kWideMaxChunk = 128;    // most queries of one launch_wide (grid y)

// the wide form of a launch_scan (ScanArgs::wide)
struct ScanWide {
  int k;
  uint32_t* hist;             // workspace u32[kWidePasses, chunk, kWideBins]
  int32_t* state;             // workspace i32[chunk, kWideStateInts]
  int32_t* counts;            // workspace i32[2, chunk, n_blocks] (gt, eq): block counts, then their prefixes; i32[2, chunk] totals behind
  int n_blocks;               // range_n_blocks(n_items)
  unsigned long long* stage;  // workspace u64[chunk, k]
  int32_t* n_out;             // device i32[n_queries] or null
};
inline size_t wide_up256(size_t v) { return (v + 255) & ~(size_t)255; }
inline size_t wide_hist_bytes(int chunk) { return wide_up256((size_t)kWidePasses * chunk * kWideBins * 4); }
inline size_t wide_state_bytes(int chunk) { return wide_up256((size_t)chunk * kWideStateInts * 4); }
inline size_t wide_counts_bytes(int chunk, long long n_items) {
  return wide_up256((size_t)2 * chunk * ((size_t)range_n_blocks(n_items) + 1) * 4);
}
inline size_t wide_stage_bytes(int chunk, int k) { return wide_up256((size_t)chunk * (size_t)k * 8); }
inline size_t wide_bytes(int chunk, long long n_items, int k) {
  return wide_hist_bytes(chunk) + wide_state_bytes(chunk) + wide_counts_bytes(chunk, n_items) + wide_stage_bytes(chunk, k);
}
// the areas of a workspace of wide_bytes(chunk, n_items, k) at `at`
inline ScanWide wide_carve(unsigned char* at, int chunk, long long n_items, int k, int32_t* n_out) {
  ScanWide w = {};
  w.k = k;
  w.hist = reinterpret_cast<uint32_t*>(at);
  at += wide_hist_bytes(chunk);
  w.state = reinterpret_cast<int32_t*>(at);
  at += wide_state_bytes(chunk);
  w.counts = reinterpret_cast<int32_t*>(at);
  at += wide_counts_bytes(chunk, n_items);
  w.stage = reinterpret_cast<unsigned long long*>(at);
  w.n_out = n_out;
  w.n_blocks = range_n_blocks(n_items);
  return w;
}
// The three stages for n_q <= kWideMaxChunk queries whose scores are rows q0 .. q0 + n_q - 1 of scores f32[.., n_items]; `limit`
// floats are readable from `scores`.  The out_* pointers and n_out are those of the first of these queries; out_item_ids is
// written only where it is given (item_ids null: the row number), out_scores and out_index likewise.
int launch_wide(const ScanWide& w, const float* scores, size_t limit, long long n_items, long long q0, int n_q,
                const int64_t* item_ids, int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* n_out, hipStream_t st);

}  // namespace nann

#ifdef NANN_SCAN_IMPL  // the kernels: nann_scan_inst.hip only
namespace nann {

__host__ __device__ constexpr int wide_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }
__host__ __device__ constexpr int wide_bits(int pass) { return pass == 2 ? 10 : 11; }
enum { kWsT = 0, kWsRank = 1, kWsGt = 2, kWsValid = 3, kWsM = 4, kWsDone = 5 };

// What a thread holds of block blockIdx.x of query q0 + blockIdx.y: pass p is the 16 bytes at position at[p] of the score
// buffer, bit j of v[p] says that element j of them is a row of the query and not -inf.
struct WideBlock {
  f32x4v s[kRangePasses];
  size_t at[kRangePasses];
  unsigned v[kRangePasses];
  size_t begin;  // position of the query's row 0
};
__device__ __forceinline__ void wide_load(const float* __restrict__ scores, size_t limit, long long n_items, long long q0, WideBlock* b) {
  const size_t begin = (size_t)(q0 + blockIdx.y) * (size_t)n_items, end = begin + (size_t)n_items;
  const size_t g0 = (begin >> 2) + (size_t)blockIdx.x * (kRangeBlockRows / 4);
  b->begin = begin;
#pragma unroll
  for (int p = 0; p < kRangePasses; ++p) {
    const size_t at = (g0 + (size_t)p * kRangeNT + threadIdx.x) * 4;
    b->at[p] = at;
    b->v[p] = 0u;
    f32x4v s = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    if (at < end) {  // (the 16 bytes begin inside the row or up to three positions in front of it)
      if (at + 4 <= limit) {
        s = *reinterpret_cast<const f32x4v*>(scores + at);
      } else {  // the last 16 bytes of the buffer, in part: what lies inside it
        const float s0 = at + 0 < limit ? scores[at + 0] : 0.0f, s1 = at + 1 < limit ? scores[at + 1] : 0.0f;
        const float s2 = at + 2 < limit ? scores[at + 2] : 0.0f;
        s = f32x4v{s0, s1, s2, 0.0f};
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = at + j >= begin && at + j < end;
        if (in && s[j] != -__builtin_inff()) b->v[p] |= 1u << j;
      }
    }
    b->s[p] = s;
  }
}

// hist[query][digit PASS of the key] += 1 over the valid rows of the block whose higher digits are the prefix's
template <int PASS>
__global__ __launch_bounds__(kRangeNT) void k_wide_hist(const float* __restrict__ scores, size_t limit, long long n_items, long long q0,
                                                        const int32_t* __restrict__ state, uint32_t* __restrict__ hist) {
  constexpr int SH = wide_shift(PASS), NB = 1 << wide_bits(PASS);
  __shared__ uint32_t h[NB];
  const int32_t* st = state + (size_t)blockIdx.y * kWideStateInts;
  uint32_t prefix = 0u;
  if constexpr (PASS > 0) {
    if (st[kWsDone]) return;  // (the whole workgroup: the cut is known)
    prefix = (uint32_t)st[kWsT];
  }
  for (int i = threadIdx.x; i < NB; i += kRangeNT) h[i] = 0u;
  __syncthreads();
  WideBlock b;
  wide_load(scores, limit, n_items, q0, &b);
#pragma unroll
  for (int p = 0; p < kRangePasses; ++p)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!((b.v[p] >> j) & 1u)) continue;
      const uint32_t key = score_key(b.s[p][j]);
      if constexpr (PASS > 0) {
        if ((key >> (SH + wide_bits(PASS))) != (prefix >> (SH + wide_bits(PASS)))) continue;
      }
      atomicAdd(&h[(key >> SH) & (uint32_t)(NB - 1)], 1u);
    }
  __syncthreads();
  uint32_t* out = hist + (size_t)blockIdx.y * kWideBins;
  for (int i = threadIdx.x; i < NB; i += kRangeNT) {
    const uint32_t c = h[i];
    if (c) atomicAdd(&out[i], c);
  }
}

// One workgroup per query, behind k_wide_hist<PASS>: the bin, from the top, in which the rank falls.
template <int PASS>
__global__ __launch_bounds__(kRangeNT) void k_wide_pick(const uint32_t* __restrict__ hist, int32_t* __restrict__ state, int k) {
  constexpr int SH = wide_shift(PASS), NB = 1 << wide_bits(PASS), PER = NB / kRangeNT;
  __shared__ int part[kRangeNT];
  int32_t* st = state + (size_t)blockIdx.x * kWideStateInts;
  const int tid = threadIdx.x;
  int rank = k, gt = 0;
  uint32_t prefix = 0u;
  if constexpr (PASS > 0) {
    if (st[kWsDone]) return;
    prefix = (uint32_t)st[kWsT];
    rank = st[kWsRank];
    gt = st[kWsGt];
  }
  const uint32_t* h = hist + (size_t)blockIdx.x * kWideBins;
  const int hi = NB - 1 - tid * PER;  // this thread's bins: hi, hi - 1, .. hi - PER + 1
  int c[PER], sum = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    c[i] = (int)h[hi - i];
    sum += c[i];
  }
  part[tid] = sum;
  __syncthreads();  // (every thread has read the state: it may be written below)
  for (int step = 1; step < kRangeNT; step <<= 1) {  // inclusive scan, from the top bins down
    const int v = tid >= step ? part[tid - step] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  const int incl = part[tid], excl = incl - sum, total = part[kRangeNT - 1];
  if constexpr (PASS == 0) {
    if (total <= k) {  // at most k valid rows: all of them, and no further pass
      if (tid == 0) {
        st[kWsT] = 0;
        st[kWsRank] = 0;
        st[kWsGt] = 0;
        st[kWsValid] = total;
        st[kWsM] = k;
        st[kWsDone] = 1;
      }
      return;
    }
  }
  if (excl < rank && rank <= incl) {  // one thread: the counts are not negative and rank >= 1
    int above = excl, bin = hi, found = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      if (!found) {
        if (above + c[i] >= rank) {
          found = 1;
          bin = hi - i;
        } else {
          above += c[i];
        }
      }
    }
    st[kWsT] = (int32_t)(prefix | ((uint32_t)bin << SH));
    st[kWsRank] = rank - above;
    st[kWsGt] = gt + above;
    if constexpr (PASS == 0) {
      st[kWsValid] = total;
      st[kWsDone] = 0;
    }
    if constexpr (PASS == kWidePasses - 1) st[kWsM] = k - (gt + above);
  }
}

// bit j of g / e: element j of the pass is a valid row with key > T / key == T
__device__ __forceinline__ void wide_classify(const WideBlock& b, uint32_t T, unsigned (&g)[kRangePasses], unsigned (&e)[kRangePasses]) {
#pragma unroll
  for (int p = 0; p < kRangePasses; ++p) {
    g[p] = e[p] = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool valid = (b.v[p] >> j) & 1u;
      const uint32_t key = score_key(b.s[p][j]);
      g[p] |= (valid && key > T ? 1u : 0u) << j;
      e[p] |= (valid && key == T ? 1u : 0u) << j;
    }
  }
}

// counts[0][query][block] = rows of the block above the cut, counts[1][query][block] = rows at the cut
__global__ __launch_bounds__(kRangeNT) void k_wide_count(const float* __restrict__ scores, size_t limit, long long n_items, long long q0,
                                                         const int32_t* __restrict__ state, int32_t* __restrict__ counts) {
  __shared__ int wave_g[kRangeNT / 64], wave_e[kRangeNT / 64];
  WideBlock b;
  wide_load(scores, limit, n_items, q0, &b);
  unsigned g[kRangePasses], e[kRangePasses];
  wide_classify(b, (uint32_t)state[(size_t)blockIdx.y * kWideStateInts + kWsT], g, e);
  int cg = 0, ce = 0;
#pragma unroll
  for (int p = 0; p < kRangePasses; ++p)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      cg += __popcll(__ballot((g[p] >> j) & 1u));
      ce += __popcll(__ballot((e[p] >> j) & 1u));
    }
  if ((threadIdx.x & 63) == 0) {
    wave_g[threadIdx.x >> 6] = cg;
    wave_e[threadIdx.x >> 6] = ce;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int tg = 0, te = 0;
#pragma unroll
    for (int w = 0; w < kRangeNT / 64; ++w) {
      tg += wave_g[w];
      te += wave_e[w];
    }
    counts[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = tg;
    counts[((size_t)gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = te;
  }
}

// The taken rows of a block to their places in the staging list.  prefix = counts behind k_range_scan.
__global__ __launch_bounds__(kRangeNT) void k_wide_fill(const float* __restrict__ scores, size_t limit, long long n_items, long long q0,
                                                        const int32_t* __restrict__ state, const int32_t* __restrict__ prefix, int k,
                                                        unsigned long long* __restrict__ stage) {
  constexpr int W = kRangeNT / 64;
  __shared__ int cnt_g[kRangePasses * W], cnt_e[kRangePasses * W];
  WideBlock b;
  wide_load(scores, limit, n_items, q0, &b);
  const int32_t* st = state + (size_t)blockIdx.y * kWideStateInts;
  const uint32_t T = (uint32_t)st[kWsT];
  const int m = st[kWsM];
  unsigned g[kRangePasses], e[kRangePasses];
  wide_classify(b, T, g, e);
  const int wave = threadIdx.x >> 6;
  int rank_g[kRangePasses], rank_e[kRangePasses];  // rows of the pass's wavefront in the lanes below this one
#pragma unroll
  for (int p = 0; p < kRangePasses; ++p) {
    int bg = 0, ag = 0, be = 0, ae = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned long long mg = __ballot((g[p] >> j) & 1u), me = __ballot((e[p] >> j) & 1u);
      bg += range_lanes_below(mg);
      ag += __popcll(mg);
      be += range_lanes_below(me);
      ae += __popcll(me);
    }
    rank_g[p] = bg;
    rank_e[p] = be;
    if ((threadIdx.x & 63) == 0) {
      cnt_g[p * W + wave] = ag;
      cnt_e[p * W + wave] = ae;
    }
  }
  __syncthreads();
  const int blk_g = prefix[(size_t)blockIdx.y * gridDim.x + blockIdx.x];
  const int blk_e = prefix[((size_t)gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x];
  unsigned long long* out = stage + (size_t)blockIdx.y * (size_t)k;
#pragma unroll
  for (int p = 0; p < kRangePasses; ++p) {
    int base_g = 0, base_e = 0;
#pragma unroll
    for (int i = 0; i < kRangePasses * W; ++i)
      if (i < p * W + wave) {
        base_g += cnt_g[i];
        base_e += cnt_e[i];
      }
    int ng = blk_g + base_g + rank_g[p], ne = blk_e + base_e + rank_e[p];  // rows above / at the cut in front of the next element
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool is_g = (g[p] >> j) & 1u, is_e = (e[p] >> j) & 1u;
      if (is_g || (is_e && ne < m)) {
        const int pos = ng + (ne < m ? ne : m);
        if (pos >= 0 && pos < k) {  // the guard of every store below
          const uint32_t row = (uint32_t)(b.at[p] + j - b.begin);
          out[pos] = ((unsigned long long)score_key(b.s[p][j]) << 32) | (unsigned long long)(~row);
        }
      }
      ng += is_g ? 1 : 0;
      ne += is_e ? 1 : 0;
    }
  }
}

// One workgroup per query: the n_out = min(k, n_valid) composites of its staging list, sorted descending in P >= k (a power of
// two) slots of dynamic LDS, then the outputs; zeros behind n_out.
__global__ __launch_bounds__(kWideSortNT) void k_wide_sort(const unsigned long long* __restrict__ stage, const int32_t* __restrict__ state,
                                                           int k, int P, const float* __restrict__ scores, long long n_items, long long q0,
                                                           const int64_t* __restrict__ item_ids, int64_t* __restrict__ out_item_ids,
                                                           float* __restrict__ out_scores, int32_t* __restrict__ out_index,
                                                           int32_t* __restrict__ n_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char wide_smem[];
  unsigned long long* c = reinterpret_cast<unsigned long long*>(wide_smem);
  const size_t qi = blockIdx.x;
  const int tid = threadIdx.x;
  int n = state[qi * kWideStateInts + kWsValid];
  n = n < 0 ? 0 : n < k ? n : k;
  const unsigned long long* in = stage + qi * (size_t)k;
  for (int i = tid; i < P; i += kWideSortNT) c[i] = i < n ? in[i] : 0ull;  // (a composite is never 0: ~row has its top bit set)
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (P >> 1); t += kWideSortNT) {
        const int i = 2 * t - (t & (stride - 1)), j = i + stride;
        const bool desc = (i & size) == 0;
        const unsigned long long a = c[i], b = c[j];
        if ((a < b) == desc) {
          c[i] = b;
          c[j] = a;
        }
      }
      __syncthreads();
    }
  const float* srow = scores + (size_t)(q0 + (long long)qi) * (size_t)n_items;
  for (int i = tid; i < k; i += kWideSortNT) {
    const size_t at = qi * (size_t)k + i;
    long long row = 0;
    float s = 0.0f;
    if (i < n) {
      row = (long long)(uint32_t)(~(uint32_t)c[i]);
      if (row >= n_items) row = 0;  // (cannot be: a staged row is a row of the query)
      s = srow[row];
    }
    if (out_item_ids) out_item_ids[at] = i < n ? (item_ids ? item_ids[row] : (int64_t)row) : 0;
    if (out_scores) out_scores[at] = s;
    if (out_index) out_index[at] = (int32_t)row;
  }
  if (n_out && tid == 0) n_out[qi] = n;
}

}  // namespace nann
#endif
