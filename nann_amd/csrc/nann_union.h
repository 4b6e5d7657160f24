// nann_union.h -- union top-k (nann_union_topk, and the last step of nann_search_multi / nann_search_all_multi): a user brings
// n_lists result lists of k_in (score, row) entries -- one per interest vector, or per search of any kind -- and gets the k best
// DISTINCT rows by the best score any list gives a row.  The reference has no such step; nothing here restates a line of it
// (DESIGN.md 4.14).
//
// The contract, per user u:
//   * entry p = l * k_in + j of the user's n_in = n_lists * k_in entries is VALID iff j < clamp(n_valid[u][l], 0, k_in) (no
//     n_valid: k_in; a list whose status word is non-zero: 0) and its row lies in [0, n_items).  Anything else is dropped:
//     malformed input never faults;
//   * among the valid entries of one row the REPRESENTATIVE has the largest score_key (nann_device.h: wg_topk's monotone key, so
//     -0 and +0 tie), ties to the lowest p; every other entry of the row is deleted;
//   * the answer is TopKV2 over the representatives in ascending p: score descending, ties to the lower p.  n_out[u] =
//     min(k, distinct valid rows) entries at the head of row u of every output, zeros behind.  NaN scores are outside the
//     contract; -inf is a score like any other.
//
// k_union_topk, one workgroup of kNT threads per user, entry p owned by thread p % kNT in pass p / kNT:
//   1. every valid entry is inserted into an LDS open-addressing table (linear probing, S = the power of two >= 2 n_in, at
//      least 64 slots: never more than half full) whose slots hold the position of the row's LEADER, the entry whose
//      atomicCAS took the slot; an occupied slot is compared through rows[leader].  With its leader known the entry raises
//      best[leader] to (score_key << 32 | ~p) with an atomicMax: the largest key wins, then the lowest p.  `best` is
//      u64[n_users, n_in] in the WORKSPACE the call's ABI brings, zeroed by the workgroup itself -- a packed value is never 0,
//      ~p has high bits set.  (In LDS it would be another 64 KB at n_in = 8192, 142.7 KB in all: it would fit, and occupancy
//      would not change -- see below.  That form has not been built or measured.);
//   2. an entry is its row's representative iff the low word of best[leader] is ~p.  A ballot per (pass, wavefront) and an
//      exclusive prefix over the kUnionPasses * kNW counts (one wavefront scans them) give every representative its place in
//      ascending p, as k_filter_compact does: (score, p) pairs compacted into the LDS the table has left;
//   3. wg_topk over the compacted scores with ids = positions: its tie rule (lower index of an ascending-p list) is the contract's;
//   4. the k positions back into rows, scores, item_ids[row] and the list p / k_in the representative came from.
// A user's slice of `best` is touched by its own workgroup only: the atomics on it are relaxed at WORKGROUP scope and
// __syncthreads(), a release / acquire pair at that scope around the barrier, orders zeroing, raising and reading.  (Agent
// scope -- __threadfence() -- would have each of the two fences write the XCD's L2 back, which nothing here needs.)
//
// LDS, dynamic: sizeof(TopkScratch) 10 448 B + 4 KB (the selected positions) + 528 B (the counts) + 4 S bytes -- 15.0 KB at
// n_in <= 32, 22.7 KB at the 4 x 200 of a four-interest top-200, 78.7 KB at the limit of 8192.  Workgroups per CU: ONE at every
// size, and the registers set that, not the LDS: the kernel takes 74 VGPRs (wg_topk's share: k_cand_topk takes 72), allocated
// as 80, which is 6 wavefronts per SIMD, and a workgroup of 1024 threads is 4 per SIMD -- a second one would need 64 VGPRs or
// fewer.  Held to that (__launch_bounds__(kNT, 8)) hipcc spills 6 VGPRs to a 12-byte scratch frame inside the selection, so the
// kernel runs as every other wg_topk kernel of 1024 threads here does.
#pragma once
#include <cstddef>
#include <cstdint>

#include "nann_search.h"

namespace nann {

static_assert(NANN_UNION_MAX_IN == 8192, "include/nann_hip.h: most entries of a user, n_lists * k_in");

struct UnionArgs {
  const float* scores;       // f32[n_users, n_lists, k_in]
  const int32_t* rows;       // i32, the same shape
  const int32_t* n_valid;    // list i = u * n_lists + l counts n_valid[i * nv_stride] entries; null: k_in
  int nv_stride;             //   (1: i32[n_users, n_lists]; 6, from &level_topn[0][5]: a traversal's per-query level_topn)
  const int32_t* status;     // i32[n_users, n_lists] or null: a list with a non-zero word counts none
  int n_lists, k_in, k;
  long long n_items;
  const int64_t* item_ids;   // i64[n_items]; may be null when out_item_ids is
  unsigned long long* best;  // the workspace: u64[n_users, n_lists * k_in]
  int32_t* out_index;        // [n_users, k] each, any of them may be null
  float* out_scores;
  int64_t* out_item_ids;
  int32_t* out_list;
  int32_t* n_out;            // i32[n_users] or null
};
size_t union_ws_bytes(long long n_users, long long n_in);
// the caller has held the shape to the kernel's limits (union_check, nann_flat.hip): 0 <= k <= min(n_lists * k_in, 1024),
// n_lists * k_in <= NANN_UNION_MAX_IN, n_users <= 2^31 - 1, `best` of union_ws_bytes(n_users, n_lists * k_in) bytes
int launch_union_topk(const UnionArgs& a, long long n_users, hipStream_t st);

}  // namespace nann

#ifdef NANN_UNION_IMPL  // the kernel: nann_cand_inst.hip only
namespace nann {

constexpr int kUnionPasses = NANN_UNION_MAX_IN / kNT;  // entries per thread
constexpr int kUnionCounts = kUnionPasses * kNW;       // (pass, wavefront) pairs
constexpr size_t kUnionSelOff = (sizeof(TopkScratch) + 15) & ~(size_t)15;
constexpr size_t kUnionCntOff = kUnionSelOff + (size_t)kMaxK * 4;
constexpr size_t kUnionTabOff = kUnionCntOff + ((((size_t)kUnionCounts + 1) * 4 + 15) & ~(size_t)15);
static_assert(kUnionPasses * kNT == NANN_UNION_MAX_IN && kUnionCounts == 2 * 64, "one wavefront scans two counts per lane");

// log2 of the table's slots: the power of two >= 2 n_in, at least 64
inline int union_slots_log2(int n_in) {
  int b = 6;
  while ((1 << b) < 2 * n_in) ++b;
  return b;
}
inline size_t union_lds_bytes(int n_in) { return kUnionTabOff + ((size_t)4 << union_slots_log2(n_in)); }

__global__ __launch_bounds__(kNT) void k_union_topk(UnionArgs a, int slots_log2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int32_t* sel = reinterpret_cast<int32_t*>(smem + kUnionSelOff);  // the k selected positions, ranked
  int* cnt = reinterpret_cast<int*>(smem + kUnionCntOff);          // representatives per (pass, wavefront), then their prefix
  int32_t* tab = reinterpret_cast<int32_t*>(smem + kUnionTabOff);  // the table; later the compacted (score, position) pairs
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t u = blockIdx.x;
  const int n_in = a.n_lists * a.k_in, slots = 1 << slots_log2;
  const float* sc = a.scores + u * (size_t)n_in;
  const int32_t* rw = a.rows + u * (size_t)n_in;
  unsigned long long* best = a.best + u * (size_t)n_in;
  for (int i = tid; i < slots; i += kNT) tab[i] = -1;
  for (int i = tid; i < n_in; i += kNT) best[i] = 0ull;
  __syncthreads();
  // ---- 1. leaders, and the best entry of every leader's row
  int lead[kUnionPasses];
  float score[kUnionPasses];
#pragma unroll
  for (int j = 0; j < kUnionPasses; ++j) {
    const int p = j * kNT + tid;
    lead[j] = -1;
    score[j] = 0.0f;
    if (p >= n_in) continue;
    const int l = p / a.k_in;
    const size_t li = u * (size_t)a.n_lists + l;
    int nv = a.n_valid ? a.n_valid[li * (size_t)a.nv_stride] : a.k_in;
    if (a.status && a.status[li] != 0) nv = 0;
    nv = max(0, min(nv, a.k_in));
    const int32_t r = rw[p];
    if (p - l * a.k_in >= nv || r < 0 || (long long)r >= a.n_items) continue;
    score[j] = sc[p];
    int h = (int)(((uint32_t)r * 2654435761u) >> (32 - slots_log2));
    for (;;) {  // (ends: at most n_in of the >= 2 n_in slots are taken)
      const int32_t prev = atomicCAS(&tab[h], -1, p);
      if (prev == -1) { lead[j] = p; break; }
      if (rw[prev] == r) { lead[j] = prev; break; }
      h = (h + 1) & (slots - 1);
    }
    const unsigned long long mine = ((unsigned long long)score_key(score[j]) << 32) | (uint32_t)~(uint32_t)p;
    (void)__hip_atomic_fetch_max(&best[lead[j]], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  // ---- 2. the representatives, compacted in ascending position
  bool rep[kUnionPasses];
  int rank[kUnionPasses];
#pragma unroll
  for (int j = 0; j < kUnionPasses; ++j) {
    const int p = j * kNT + tid;
    rep[j] = false;
    if (lead[j] >= 0) {
      const unsigned long long b = __hip_atomic_load(&best[lead[j]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      rep[j] = (uint32_t)b == ~(uint32_t)p;
    }
    const unsigned long long m = __ballot(rep[j]);
    rank[j] = (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
    if (lane == 0) cnt[j * kNW + wave] = __popcll(m);
  }
  __syncthreads();
  if (wave == 0) {  // cnt[i] <- the representatives before pair i, cnt[kUnionCounts] <- all of them
    const int c0 = cnt[2 * lane], c1 = cnt[2 * lane + 1];
    int incl = c0 + c1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    cnt[2 * lane] = incl - c0 - c1;
    cnt[2 * lane + 1] = incl - c1;
    if (lane == 63) cnt[kUnionCounts] = incl;
  }
  __syncthreads();
  float* cscore = reinterpret_cast<float*>(tab);  // (every probe of the table lies two barriers back)
  int32_t* cpos = tab + n_in;
#pragma unroll
  for (int j = 0; j < kUnionPasses; ++j) {
    if (!rep[j]) continue;
    const int c = cnt[j * kNW + wave] + rank[j];
    cscore[c] = score[j];
    cpos[c] = j * kNT + tid;
  }
  const int m = cnt[kUnionCounts];  // distinct valid rows
  const int kk = min(a.k, m);
  __syncthreads();
  // ---- 3. TopKV2 over the representatives; 4. what the caller asked for of each
  if (kk > 0) wg_topk(cpos, cscore, nullptr, m, kk, nullptr, sel, nullptr, nullptr, nullptr, smem);
  for (int i = tid; i < a.k; i += kNT) {
    const size_t at = u * (size_t)a.k + i;
    const int p = i < kk ? sel[i] : -1;
    const int32_t r = p >= 0 ? rw[p] : 0;
    if (a.out_index) a.out_index[at] = r;
    if (a.out_scores) a.out_scores[at] = p >= 0 ? sc[p] : 0.0f;
    if (a.out_item_ids) a.out_item_ids[at] = p >= 0 ? a.item_ids[r] : 0;
    if (a.out_list) a.out_list[at] = p >= 0 ? p / a.k_in : 0;
  }
  if (a.n_out && tid == 0) a.n_out[u] = kk;
}

}  // namespace nann
#endif
