// nann_fuse.h -- fused top-k (nann_fuse_topk, and the last step of nann_search_multi_fused / nann_search_all_multi_fused): a
// user brings n_lists result lists of k_in (score, row) entries -- one per interest vector, or per search of any kind, on any
// scale -- and gets the k best DISTINCT rows by a score ACCUMULATED over the lists that contain a row: reciprocal rank fusion
// or a weighted sum of raw, floor-shifted or min-max-normalised scores.  The reference has no such step; nothing here restates
// a line of it.
//
// The contract, per user u:
//   * entry p = l * k_in + j of the user's n_in = n_lists * k_in entries is VALID iff j < clamp(n_valid[u][l], 0, k_in) (no
//     n_valid: k_in; a list whose status word is non-zero: 0) and its row lies in [0, n_items).  Anything else is dropped:
//     malformed input never faults;
//   * within one list a row COUNTS ONCE, at its lowest valid j; its rank is that j, whether or not the entries before it are
//     valid.  lo_l / hi_l are the least / greatest valid score of list l, compared through score_key (-0 read as +0);
//   * the term of list l for a row it contains, every step a single f32 operation (the build's -ffp-contract=off stays):
//       NANN_FUSE_SUM        w * s
//       NANN_FUSE_SUM_FLOOR  w * (s - lo_l)
//       NANN_FUSE_MINMAX     w * ((s - lo_l) / (hi_l - lo_l)), the quotient read as 1.0f where hi_l == lo_l
//       NANN_FUSE_RRF        w / (rrf_c + (float)(j + 1))
//     with w = weights[l] or weights[u * n_lists + l], 1.0f without weights;
//   * the fused score starts from +0.0f and takes the terms of the lists that contain the row in ascending l, one f32 add
//     each.  The ORDER of the additions is part of the contract, which is why nothing here adds floats atomically;
//   * the answer is TopKV2 over the distinct valid rows in ascending order of each row's lowest valid p: fused score descending
//     through score_key, ties to the lower first p.  n_out[u] = min(k, distinct valid rows) entries at the head of row u of
//     every output, zeros behind; out_lists: bit l set iff list l contains the row.
//
// k_fuse_topk, one workgroup of kNT threads per user, entry p owned by thread p % kNT in pass p / kNT:
//   1. every valid entry is inserted into the LDS open-addressing table of k_union_topk (linear probing, S = the power of two
//      >= 2 n_in, at least 64 slots: never more than half full; a slot holds the position of the row's LEADER, the entry
//      whose atomicCAS took it, and is compared through rows[leader]).  With its leader known the entry lowers first[leader]
//      to p (atomicMin), and, in modes 1 and 2, lowers lo[l] / raises hi[l] (u32[64] each in LDS) with its score_key;
//   2. one round per list, in ascending l: the valid entries of list l raise stamp[l & 1][leader] to (l + 1) << 13 | (8191 - j)
//      with an atomicMax -- a later list beats an earlier one, then the lowest j wins -- and, behind ONE barrier, the entry that
//      finds its own value there is the slot's only writer of the round: acc[leader] += term, mask[leader] |= 1 << l with plain
//      loads and stores.  Two stamp arrays take turns so that a round's atomics cannot overtake the reads of the round before
//      (the array of round l is written again in round l + 2, a barrier later); the next round's reader of acc stands behind
//      that round's barrier.  n_in atomics in all, n_lists barriers;
//   3. an entry represents its row iff first[leader] == p.  The union's ballot per (pass, wavefront) and prefix over the counts
//      give every representative its place in ascending p: (acc[leader], leader) pairs compacted into the LDS the table has left;
//   4. wg_topk over the compacted fused scores with out_pos: its tie rule (lower index of an ascending-first-p list) is the
//      contract's; then rows[leader], the fused score, item_ids[row] and mask[leader] of the k places.
// mask u64, acc f32, first i32 and stamp u32[2], 24 B per entry, lie in the WORKSPACE the call's ABI brings (beside a 64 KB
// table they would not all fit in a CU's 160 KB of LDS at n_in = 8192), initialised by the workgroup itself.  A user's slice is
// touched by its own workgroup only: the atomics on it are relaxed at WORKGROUP scope, and __syncthreads(), a release /
// acquire pair at that scope around the barrier, orders them and the plain accesses, as in k_union_topk.
//
// LDS, dynamic: sizeof(TopkScratch) 10 448 B + 4 KB (the selected places) + 528 B (the counts) + 512 B (lo, hi) + 4 S bytes --
// 15.5 KB at n_in <= 32, 23.2 KB at the 4 x 200 of a four-interest top-200, 79.2 KB at the limit of 8192.  The compiler's
// resource report: 83 VGPRs, 83 SGPRs, no scratch (ScratchSize 0, no spills), 5 wavefronts per SIMD allowed -- a workgroup of
// 1024 threads is 4 per SIMD, so ONE workgroup per CU at every size, as for k_union_topk.
#pragma once
#include <cstddef>
#include <cstdint>

#include "nann_search.h"
#include "nann_union.h"

namespace nann {

static_assert(NANN_FUSE_MAX_LISTS == 64, "include/nann_hip.h: out_lists is one u64 per entry");

struct FuseArgs {
  const float* scores;       // f32[n_users, n_lists, k_in]
  const int32_t* rows;       // i32, the same shape
  const int32_t* n_valid;    // list i = u * n_lists + l counts n_valid[i * nv_stride] entries; null: k_in
  int nv_stride;             //   (1: i32[n_users, n_lists]; 6, from &level_topn[0][5]: a traversal's per-query level_topn)
  const int32_t* status;     // i32[n_users, n_lists] or null: a list with a non-zero word counts none
  int n_lists, k_in, k;
  long long n_items;
  const int64_t* item_ids;   // i64[n_items]; may be null when out_item_ids is
  int mode;                  // NANN_FUSE_SUM .. NANN_FUSE_RRF
  float rrf_c;
  const float* weights;      // f32[n_lists], f32[n_users, n_lists] (weights_per_user) or null = 1.0f
  int weights_per_user;
  unsigned char* ws;         // the workspace: fuse_ws_bytes(n_users, n_lists * k_in) bytes, 24 per entry
  int32_t* out_index;        // [n_users, k] each, any of them may be null
  float* out_scores;
  int64_t* out_item_ids;
  unsigned long long* out_lists;
  int32_t* n_out;            // i32[n_users] or null
};
size_t fuse_ws_bytes(long long n_users, long long n_in);
// the caller has held the shape to the kernel's limits (fuse_check, nann_flat.hip): 0 <= k <= min(n_lists * k_in, 1024),
// n_lists <= NANN_FUSE_MAX_LISTS, n_lists * k_in <= NANN_UNION_MAX_IN, n_users <= 2^31 - 1, a known mode
int launch_fuse_topk(const FuseArgs& a, long long n_users, hipStream_t st);

}  // namespace nann

#ifdef NANN_FUSE_IMPL  // the kernel: nann_cand_inst.hip only, behind the union's (its table sizes and pass counts are shared)
#ifndef NANN_UNION_IMPL
#error "nann_fuse.h: the kernel shares k_union_topk's constants; define NANN_UNION_IMPL as well"
#endif
namespace nann {

constexpr size_t kFuseSelOff = (sizeof(TopkScratch) + 15) & ~(size_t)15;
constexpr size_t kFuseCntOff = kFuseSelOff + (size_t)kMaxK * 4;
constexpr size_t kFuseLoOff = kFuseCntOff + ((((size_t)kUnionCounts + 1) * 4 + 15) & ~(size_t)15);
constexpr size_t kFuseTabOff = kFuseLoOff + 2 * (size_t)NANN_FUSE_MAX_LISTS * 4;
constexpr size_t kFuseEntryBytes = 24;  // mask u64, acc f32, first i32, stamp u32[2]
static_assert(NANN_UNION_MAX_IN <= (1 << 13), "a stamp keeps 8191 - j in 13 bits");

inline size_t fuse_lds_bytes(int n_in) { return kFuseTabOff + ((size_t)4 << union_slots_log2(n_in)); }

// the f32 a score_key came from, a zero as +0
__device__ __forceinline__ float fuse_key_score(uint32_t key) {
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

__global__ __launch_bounds__(kNT) void k_fuse_topk(FuseArgs a, int slots_log2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int32_t* sel = reinterpret_cast<int32_t*>(smem + kFuseSelOff);    // the k selected places of the compacted list, ranked
  int* cnt = reinterpret_cast<int*>(smem + kFuseCntOff);            // representatives per (pass, wavefront), then their prefix
  uint32_t* lo = reinterpret_cast<uint32_t*>(smem + kFuseLoOff);    // per list: the least / greatest valid score_key
  uint32_t* hi = lo + NANN_FUSE_MAX_LISTS;
  int32_t* tab = reinterpret_cast<int32_t*>(smem + kFuseTabOff);    // the table; later the compacted (fused score, leader) pairs
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t u = blockIdx.x;
  const int n_in = a.n_lists * a.k_in, slots = 1 << slots_log2;
  const float* sc = a.scores + u * (size_t)n_in;
  const int32_t* rw = a.rows + u * (size_t)n_in;
  unsigned char* slice = a.ws + u * (size_t)n_in * kFuseEntryBytes;
  unsigned long long* mask = reinterpret_cast<unsigned long long*>(slice);
  float* acc = reinterpret_cast<float*>(slice + (size_t)n_in * 8);
  int32_t* first = reinterpret_cast<int32_t*>(slice + (size_t)n_in * 12);
  uint32_t* stamp = reinterpret_cast<uint32_t*>(slice + (size_t)n_in * 16);  // [2][n_in]
  for (int i = tid; i < slots; i += kNT) tab[i] = -1;
  for (int i = tid; i < n_in; i += kNT) {
    mask[i] = 0ull;
    acc[i] = 0.0f;
    first[i] = 0x7fffffff;
    stamp[i] = 0u;
    stamp[n_in + i] = 0u;
  }
  if (tid < NANN_FUSE_MAX_LISTS) {
    lo[tid] = 0xffffffffu;
    hi[tid] = 0u;
  }
  __syncthreads();
  // ---- 1. leaders, every row's first position, every list's floor and ceiling
  int lead[kUnionPasses];  // the leader's position; -1: not a valid entry
  int lj[kUnionPasses];    // l << 16 | j
  float term[kUnionPasses];
#pragma unroll
  for (int e = 0; e < kUnionPasses; ++e) {
    const int p = e * kNT + tid;
    lead[e] = -1;
    lj[e] = 0;
    term[e] = 0.0f;
    if (p >= n_in) continue;
    const int l = p / a.k_in, j = p - l * a.k_in;
    const size_t li = u * (size_t)a.n_lists + l;
    int nv = a.n_valid ? a.n_valid[li * (size_t)a.nv_stride] : a.k_in;
    if (a.status && a.status[li] != 0) nv = 0;
    nv = max(0, min(nv, a.k_in));
    const int32_t r = rw[p];
    if (j >= nv || r < 0 || (long long)r >= a.n_items) continue;
    lj[e] = l << 16 | j;
    term[e] = sc[p];  // (the score until the floors are known)
    int h = (int)(((uint32_t)r * 2654435761u) >> (32 - slots_log2));
    for (;;) {  // (ends: at most n_in of the >= 2 n_in slots are taken)
      const int32_t prev = atomicCAS(&tab[h], -1, p);
      if (prev == -1) { lead[e] = p; break; }
      if (rw[prev] == r) { lead[e] = prev; break; }
      h = (h + 1) & (slots - 1);
    }
    (void)__hip_atomic_fetch_min(&first[lead[e]], p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (a.mode == NANN_FUSE_SUM_FLOOR || a.mode == NANN_FUSE_MINMAX) {
      const uint32_t key = score_key(term[e]);
      atomicMin(&lo[l], key);
      atomicMax(&hi[l], key);
    }
  }
  __syncthreads();
  // ---- the term an entry would add, every step one f32 operation
#pragma unroll
  for (int e = 0; e < kUnionPasses; ++e) {
    if (lead[e] < 0) continue;
    const int l = lj[e] >> 16, j = lj[e] & 0xffff;
    const float w = a.weights ? a.weights[(a.weights_per_user ? u * (size_t)a.n_lists : 0) + l] : 1.0f;
    const float s = term[e];
    if (a.mode == NANN_FUSE_SUM) {
      term[e] = w * s;
    } else if (a.mode == NANN_FUSE_RRF) {
      const float den = a.rrf_c + (float)(j + 1);
      term[e] = w / den;
    } else {
      const float lo_l = fuse_key_score(lo[l]), hi_l = fuse_key_score(hi[l]);
      const float above = s - lo_l;
      if (a.mode == NANN_FUSE_SUM_FLOOR) {
        term[e] = w * above;
      } else {
        const float span = hi_l - lo_l;
        const float quot = hi_l == lo_l ? 1.0f : above / span;
        term[e] = w * quot;
      }
    }
  }
  // ---- 2. one round per list: the lowest valid j of a row in list l adds the list's term
  for (int l = 0; l < a.n_lists; ++l) {
    uint32_t* st = stamp + (size_t)(l & 1) * n_in;
#pragma unroll
    for (int e = 0; e < kUnionPasses; ++e) {
      if (lead[e] < 0 || (lj[e] >> 16) != l) continue;
      const uint32_t mine = (uint32_t)(l + 1) << 13 | (uint32_t)(8191 - (lj[e] & 0xffff));
      (void)__hip_atomic_fetch_max(&st[lead[e]], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kUnionPasses; ++e) {
      if (lead[e] < 0 || (lj[e] >> 16) != l) continue;
      const uint32_t mine = (uint32_t)(l + 1) << 13 | (uint32_t)(8191 - (lj[e] & 0xffff));
      if (__hip_atomic_load(&st[lead[e]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != mine) continue;
      acc[lead[e]] = acc[lead[e]] + term[e];
      mask[lead[e]] |= 1ull << l;
    }
  }
  __syncthreads();
  // ---- 3. the representatives (a row's first position), compacted in ascending position
  bool rep[kUnionPasses];
  int rank[kUnionPasses];
#pragma unroll
  for (int e = 0; e < kUnionPasses; ++e) {
    const int p = e * kNT + tid;
    rep[e] = false;
    if (lead[e] >= 0) rep[e] = __hip_atomic_load(&first[lead[e]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == p;
    const unsigned long long m = __ballot(rep[e]);
    rank[e] = (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
    if (lane == 0) cnt[e * kNW + wave] = __popcll(m);
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
  float* cscore = reinterpret_cast<float*>(tab);  // (every probe of the table lies behind the rounds' barriers)
  int32_t* clead = tab + n_in;
#pragma unroll
  for (int e = 0; e < kUnionPasses; ++e) {
    if (!rep[e]) continue;
    const int c = cnt[e * kNW + wave] + rank[e];
    cscore[c] = acc[lead[e]];
    clead[c] = lead[e];
  }
  const int m = cnt[kUnionCounts];  // distinct valid rows
  const int kk = min(a.k, m);
  __syncthreads();
  // ---- 4. TopKV2 over the fused scores; what the caller asked for of each place
  if (kk > 0) wg_topk(nullptr, cscore, nullptr, m, kk, sel, nullptr, nullptr, nullptr, nullptr, smem);
  for (int i = tid; i < a.k; i += kNT) {
    const size_t at = u * (size_t)a.k + i;
    const int c = i < kk ? sel[i] : -1;
    const int ld = c >= 0 ? clead[c] : -1;
    const int32_t r = ld >= 0 ? rw[ld] : 0;
    if (a.out_index) a.out_index[at] = r;
    if (a.out_scores) a.out_scores[at] = ld >= 0 ? cscore[c] : 0.0f;
    if (a.out_item_ids) a.out_item_ids[at] = ld >= 0 ? a.item_ids[r] : 0;
    if (a.out_lists) a.out_lists[at] = ld >= 0 ? mask[ld] : 0ull;
  }
  if (a.n_out && tid == 0) a.n_out[u] = kk;
}

}  // namespace nann
#endif
