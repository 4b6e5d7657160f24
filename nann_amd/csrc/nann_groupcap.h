// nann_groupcap.h -- group caps (nann_group_cap_topk, and the last step of nann_search_grouped / nann_search_all_grouped and
// their _model forms): at most m rows of one group -- a seller, a category, a brand -- among the k rows a query returns.  The
// reference has no such step; nothing here restates a line of it.
//
// The contract, per query i, over a RANKED list of k_in (row, score) entries:
//   * entry j is VALID iff j < clamp(n_valid[i], 0, k_in) (no n_valid: k_in; a query whose status word is non-zero: 0), its row
//     lies in [0, n_items) and the filter, where one is given, does not deny the row.  Anything else is dropped and uses no
//     quota: malformed input never faults;
//   * the group of a valid entry is g = group_of_row[row]; g < 0 is UNGROUPED: never capped, counted against nothing;
//   * walking the valid entries in ascending j, an entry is KEPT iff g < 0, or the query is uncapped (caps[i] <= 0), or fewer
//     than m valid entries before it have group g -- its rank among the valid entries of its group is < m.  A row that stands
//     twice counts twice;
//   * the answer is the first k kept entries, order unchanged: n_out[i] of them at the head of row i of every output, zeros
//     behind.  Scores are carried through, never compared: NaN and -inf are scores like any other.
// PREFIX PROPERTY: for F' >= F the capped list over the first F entries is a prefix of the capped list over the first F'.
// Proof: whether entry j is valid and kept depends on entries 0 .. j alone, so both walks decide every j < F alike; the walk
// over F' only appends entries j >= F behind them.  Hence n_out == k means the exact answer over the full ranking, and
// n_out < k means the list was cut short by F (unless it held every valid row).
//
// k_group_cap, one workgroup of 256 threads per query, entry e owned by thread e % 256 in pass e / 256 as in k_filter_compact,
// so that wavefront w of pass j holds CHUNK c = 4 j + w: the 64 consecutive entries 64 c .. 64 c + 63.
//   0. validity: n_valid, the row's range, the deny bitmap, and the exclusion list through k_filter_compact's row table (the
//      standalone call has no workspace for a second list, so the filter is applied here; the table's LDS is reused below);
//   1. every valid grouped entry of a capped query inserts its group id into an LDS open-addressing table (atomicCAS, linear
//      probing; at most 1024 keys in 2048 slots: never more than half full, the probing ends) and keeps its SLOT;
//   2. rank within the group, in list order, in two parts.  Within a chunk: the wavefront loops over the distinct slots its
//      lanes hold -- the slot of the lowest lane still open, a ballot of the lanes that share it, mbcnt for a lane's place among
//      them; every round closes at least that lowest lane, so the loop ends after at most 64 rounds by construction -- and
//      the first lane of a slot stores the chunk's population of it as one BYTE (<= 64) at per[slot][chunk].  Across chunks:
//      behind one barrier an entry reads the 16 bytes of its slot with one 128-bit load and adds those of the chunks before
//      its own.  No wavefront waits for another one outside __syncthreads();
//   3. compaction as in k_filter_compact: a ballot per (pass, wavefront), an exclusive prefix over the 16 counts, mbcnt --
//      stable, no atomics on the outputs; positions >= k are dropped, the tail is zeroed, n_out written.
// LDS: 8 KB (keys; step 3 keeps its 16 counts there) + 32 KB (the bytes; their first 8 KB hold the row table's flags during
// step 0) = 40 KB exactly, four workgroups to a CU's 160 KB.
#pragma once
#include <cstdint>

#include "nann_filter.h"

namespace nann {

struct GroupCapArgs {
  FilterArgs f;                 // validity: f.n_items bounds the rows; deny bitmap and exclusion lists, any of them null
  const int32_t* in_rows;       // i32[n_queries, k_in]
  const float* in_scores;       // f32, the same shape, or null (scores then read as 0)
  int k_in;                     // <= kMaxK
  const int32_t* n_valid;       // query i counts n_valid[i * nv_stride] entries; null: k_in
  int nv_stride;                //   (1: i32[n_queries]; 6, from &level_topn[0][5]: a traversal's per-query level_topn)
  const int32_t* status;        // i32[n_queries] or null: a query with a non-zero word counts none
  const int32_t* group_of_row;  // i32[n_items]; < 0: ungrouped
  int cap;                      // the cap of every query when caps is null
  const int32_t* caps;          // i32[n_queries] or null; <= 0: the query is uncapped
  int k;
  const int64_t* item_ids;      // i64[n_items]; may be null when out_item_ids is
  int32_t* out_index;           // [n_queries, k] each, any of them may be null
  float* out_scores;
  int64_t* out_item_ids;
  int32_t* out_group;
  int32_t* out_pos;
  int32_t* n_out;               // i32[n_queries] or null
};
// the caller has held the shape to the kernel's limits: 0 <= k, 0 <= k_in <= 1024, n_queries <= 2^31 - 1
int launch_group_cap(const GroupCapArgs& a, long long n_queries, hipStream_t st);

}  // namespace nann

#ifdef NANN_GROUPCAP_IMPL  // the kernel: nann_filter_inst.hip only
namespace nann {

constexpr int kGroupCapChunks = kFilterPasses * (kFilterNT / 64);  // 64-entry chunks of the longest list
static_assert(kGroupCapChunks == 16, "a slot's per-chunk populations are the 16 bytes of one 128-bit load");

__device__ __forceinline__ int groupcap_hash(int32_t g) { return (int)(((uint32_t)g * 2654435761u) >> 21); }  // 11 bits
__device__ __forceinline__ int groupcap_bytes(uint32_t w) {
  return (int)((w & 0xffu) + ((w >> 8) & 0xffu) + ((w >> 16) & 0xffu) + (w >> 24));
}

__global__ __launch_bounds__(kFilterNT) void k_group_cap(GroupCapArgs a) {
  constexpr int W = kFilterNT / 64;
  __shared__ int32_t tab[kFilterSlots];                                       // keys: rows in step 0, group ids from step 1
  __shared__ __attribute__((aligned(16))) uint32_t per[kFilterSlots * 4];     // [slot][chunk] bytes; step 0: the flags
  int* cnt = reinterpret_cast<int*>(tab);  // the 16 counts of step 3: every probe of the table lies a barrier back by then
  const size_t qi = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int n = a.n_valid ? a.n_valid[qi * (size_t)a.nv_stride] : a.k_in;
  if (a.status && a.status[qi] != 0) n = 0;
  n = max(0, min(n, min(a.k_in, kMaxK)));
  const int cap = a.caps ? a.caps[qi] : a.cap;
  const bool capped = cap > 0 && n > 0;  // (uniform over the workgroup, as `lists` is)
  long long lb = 0, le = 0;
  if (filter_has_lists(a.f)) filter_list_range(a.f, (long long)qi, &lb, &le);
  const bool lists = le > lb && n > 0;
  int32_t* hit = reinterpret_cast<int32_t*>(per);
  if (lists) {
    for (int i = tid; i < kFilterSlots; i += kFilterNT) { tab[i] = -1; hit[i] = 0; }
    __syncthreads();
  }
  // ---- 0. the valid entries
  int32_t row[kFilterPasses], grp[kFilterPasses];
  float score[kFilterPasses];
  int slot[kFilterPasses];
  bool ok[kFilterPasses];
#pragma unroll
  for (int j = 0; j < kFilterPasses; ++j) {
    const int e = j * kFilterNT + tid;
    row[j] = e < n ? a.in_rows[qi * (size_t)a.k_in + e] : -1;
    score[j] = e < n && a.in_scores ? a.in_scores[qi * (size_t)a.k_in + e] : 0.0f;
    ok[j] = row[j] >= 0 && (long long)row[j] < a.f.n_items;
    if (ok[j] && a.f.deny_bits) ok[j] = ((a.f.deny_bits[row[j] >> 5] >> (row[j] & 31)) & 1u) == 0u;
    slot[j] = -1;
    if (lists && ok[j]) {
      int h = filter_hash(row[j]);
      for (;;) {  // (ends: at most kMaxK of the kFilterSlots slots are taken; a repeated row shares its slot)
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
      const int32_t r = a.f.rows[i];
      if (r < 0 || (long long)r >= a.f.n_items) continue;
      int h = filter_hash(r);
      for (;;) {
        const int32_t key = tab[h];
        if (key == r) hit[h] = 1;
        if (key == r || key == -1) break;
        h = (h + 1) & (kFilterSlots - 1);
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kFilterPasses; ++j)
      if (slot[j] >= 0 && hit[slot[j]]) ok[j] = false;
    __syncthreads();  // (the table and the flags are read for the last time: step 1 takes their place)
  }
#pragma unroll
  for (int j = 0; j < kFilterPasses; ++j) grp[j] = ok[j] ? a.group_of_row[row[j]] : -1;
  bool keep[kFilterPasses];
#pragma unroll
  for (int j = 0; j < kFilterPasses; ++j) keep[j] = ok[j];
  if (capped) {
    // ---- 1. the slot of every group
    for (int i = tid; i < kFilterSlots; i += kFilterNT) tab[i] = -1;
    for (int i = tid; i < kFilterSlots * 4; i += kFilterNT) per[i] = 0u;
    __syncthreads();
    uint8_t* per8 = reinterpret_cast<uint8_t*>(per);
    int in_chunk[kFilterPasses];
#pragma unroll
    for (int j = 0; j < kFilterPasses; ++j) {
      slot[j] = -1;
      in_chunk[j] = 0;
      if (grp[j] >= 0) {
        int h = groupcap_hash(grp[j]);
        for (;;) {  // (ends: at most kMaxK of the kFilterSlots slots are taken)
          const int32_t prev = atomicCAS(&tab[h], -1, grp[j]);
          if (prev == -1 || prev == grp[j]) break;
          h = (h + 1) & (kFilterSlots - 1);
        }
        slot[j] = h;
      }
      // ---- 2a. the place of a lane among the lanes of its chunk that share its slot, and the chunk's population of the slot
      unsigned long long open = __ballot(slot[j] >= 0);
      while (open) {  // (uniform; every round closes at least the lowest open lane: at most 64 rounds)
        const int first = __ffsll((long long)open) - 1;
        const int s = __builtin_amdgcn_readlane(slot[j], first);  // (`first` is uniform: a lane read, no trip through LDS)
        const bool mine = slot[j] == s;
        const unsigned long long m = __ballot(mine);
        if (mine) {
          in_chunk[j] = (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
          if (in_chunk[j] == 0) per8[s * kGroupCapChunks + j * W + wave] = (uint8_t)__popcll(m);
        }
        open &= ~m;
      }
    }
    __syncthreads();
    // ---- 2b. the entries of the group in the chunks before
#pragma unroll
    for (int j = 0; j < kFilterPasses; ++j) {
      if (slot[j] < 0) continue;
      const uint4 v = *reinterpret_cast<const uint4*>(&per[slot[j] * 4]);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};  // word i: chunks 4 i .. 4 i + 3 = pass i, wavefronts 0 .. 3
      int before = groupcap_bytes(w[j] & ((1u << (8 * wave)) - 1u));
#pragma unroll
      for (int i = 0; i < j; ++i) before += groupcap_bytes(w[i]);
      keep[j] = before + in_chunk[j] < cap;
    }
  }
  // ---- 3. the kept entries, compacted in list order
  int rank[kFilterPasses];
#pragma unroll
  for (int j = 0; j < kFilterPasses; ++j) {
    const unsigned long long m = __ballot(keep[j]);
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
    if (keep[j] && pos < a.k) {
      const size_t at = qi * (size_t)a.k + pos;
      if (a.out_index) a.out_index[at] = row[j];
      if (a.out_scores) a.out_scores[at] = score[j];
      if (a.out_item_ids) a.out_item_ids[at] = a.item_ids[row[j]];
      if (a.out_group) a.out_group[at] = grp[j];
      if (a.out_pos) a.out_pos[at] = j * kFilterNT + tid;
    }
  }
  total = min(total, a.k);
  for (int i = total + tid; i < a.k; i += kFilterNT) {
    const size_t at = qi * (size_t)a.k + i;
    if (a.out_index) a.out_index[at] = 0;
    if (a.out_scores) a.out_scores[at] = 0.0f;
    if (a.out_item_ids) a.out_item_ids[at] = 0;
    if (a.out_group) a.out_group[at] = 0;
    if (a.out_pos) a.out_pos[at] = 0;
  }
  if (a.n_out && tid == 0) a.n_out[qi] = total;
}

}  // namespace nann
#endif
