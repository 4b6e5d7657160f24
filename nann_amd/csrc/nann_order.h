// Locality order of a search batch ("Query order and XCD queues").
//
// k_search's slots pull queries from a shared queue; the hardware deals workgroups round-robin over the XCDs, so in input
// order the queries in flight on one XCD come from all over the corpus and their rows do not share that XCD's L2.  Before
// the main launch of an L2 hash-set plan the batch is ordered by neighbourhood instead:
//   k_order_key:  key[q] = the nearest of P pivot rows (a sample of the index's enter points, chosen at index creation)
//   k_order_perm: a stable counting sort of the query indices by key -> perm[n]; perm is cut into kOrderSegs contiguous
//                 segments of near-equal size, one per XCD, each with its own head counter (k_search's pull loop)
// The key only decides order, never results: any key is correct, this one just has to be cheap and group neighbours.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include "../../include/nann_hip.h"

namespace nann {

constexpr int kOrderSegs = 8;          // XCDs of an MI355X: one segment of the ordered batch each
constexpr int kOrderHeadStride = 32;   // head words 128 bytes apart (one cache line each)
constexpr int kOrderMaxPivots = 128;
constexpr int kOrderPivotLds = 64 * 1024;  // pivots * d * 4 bytes staged per key workgroup
constexpr int kOrderKeyQueries = 16;   // queries per key workgroup (4 waves x 4)
static_assert(kOrderKeyQueries % 4 == 0, "a key workgroup is 4 waves");
constexpr int kOrderSortThreads = 1024;
// k_order_perm's fast path: a batch of at most this many queries is sorted from registers with one scan over a
// [key][run of 64 queries] count table (u16, 32 KB of LDS at 128 runs); larger batches go tile by tile
constexpr int kOrderFastQueries = 8192;
constexpr int kOrderFastRuns = kOrderFastQueries / 64;
static_assert(kOrderFastQueries % kOrderSortThreads == 0 && kOrderFastQueries < 65536, "u16 prefixes, whole tiles");
static_assert(kOrderMaxPivots * kOrderFastRuns == 16 * kOrderSortThreads, "the scan gives each thread 16 table entries");
static_assert(kOrderMaxPivots == 128, "a key is seven bits (order_same_key)");
// k_order_perm also zeroes the 256-byte header of the search workspace (WsHeader, nann_search.h) for the launch behind it
constexpr int kOrderHeaderWords = 64;

__host__ __device__ inline int order_seg_begin(int n, int s) { return (int)((long long)n * s / kOrderSegs); }

// pivots the key kernel can stage for row width d (the workspace and the index agree on this)
inline int order_pivots(int64_t n_enter, int d) {
  return (int)std::min<int64_t>(n_enter, std::min(kOrderMaxPivots, kOrderPivotLds / (4 * d)));
}

// workspace of the order: kOrderSegs heads, then perm[n], key[n] (bytes, a multiple of 256)
inline unsigned long long order_ws_bytes(int64_t n) {
  return ((unsigned long long)kOrderSegs * kOrderHeadStride * 4 + (unsigned long long)n * 8 + 255) / 256 * 256;
}

// the XCD this wave runs on (bits 3:0 of HW_REG_XCC_ID)
__device__ inline unsigned int xcc_id() {
#if defined(__HIP_DEVICE_COMPILE__)
  unsigned int x;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(x));
  return x;
#else
  return 0;
#endif
}

}  // namespace nann
