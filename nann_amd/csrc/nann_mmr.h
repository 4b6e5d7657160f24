// nann_mmr.h -- diversified results (nann_mmr_topk, and the last step of nann_search_diverse / nann_search_all_diverse and their
// _model forms): MMR (maximal marginal relevance, Carbonell & Goldstein) re-ranking of a fetched list of F (row, score) entries
// into k picks that trade a row's score against its similarity to the rows picked before it.  The reference has no such step;
// nothing here restates a line of it.
//
// The contract, per query i, over k_in (row, score) entries:
//   * entry j is VALID iff j < clamp(n_valid[i], 0, k_in) (no n_valid: k_in; a query whose status word is non-zero: 0), its row
//     lies in [0, n_items), its score is finite and the filter, where one is given, does not deny the row.  Anything else is
//     dropped: malformed input never faults.  A row that stands twice gives two candidates;
//   * a = the query's lambda (lambdas[i] read as !(x >= 0) ? 0 : (x > 1 ? 1 : x), else lambda), b = 1.0f - a;
//   * sim(j, t): the canonical score of the metric (MT_L2 / MT_IP, nann_device.h) with row rows[t] widened exactly to f32 as
//     the query and row rows[j] as the item -- the lane sums and the xor butterfly of nann_score, hence its bits;
//   * r_j = a * s_j once; step 0 picks the valid j with the greatest r_j; after pick t, p_j = sim(j, t) behind the first pick
//     and p_j = (sim(j, t) > p_j) ? sim(j, t) : p_j behind the later ones; step n >= 1 picks, among the valid unpicked j, the
//     greatest v_j = r_j - (b * p_j).  f32, no contraction.  Greatest by wg_topk's key -- score_key(x): x + 0.0f, then the
//     monotone u32 map -- ties to the lower j;
//   * min(k, #valid) picks, in pick order at the head of row i of every output, zeros behind.
//
// k_mmr, one workgroup of 1024 threads per query; k_in <= 1024, so thread j OWNS entry j: its row, score, r, p, v and the picked
// flag are registers.  LDS holds what crosses threads: the row list, the current similarities, the picked row as f32[d], one
// word per wavefront for the argmax -- and, on the LDS path, the candidate rows themselves.
//   setup  validity (n_valid, the row's range, the score, the deny bitmap, the exclusion list through a row table as in
//          k_filter_compact; the table's LDS becomes the row list and the similarities afterwards); on the LDS path the valid
//          prefix's rows are copied from the table into LDS once, 16 bytes per thread and trip;
//   a step 1. argmax: per wavefront the greatest key by DPP (wave_max) and the lowest lane that holds it (ballot, ffs), packed
//             with the valid bit into one u64 (valid, key, 1023 - j); one word per wavefront into LDS, one pass of every thread
//             over the 16 words -- the pick is uniform without a broadcast;
//          2. the owner of the pick writes the outputs;
//          3. the F similarities, by one of two paths of identical bits (they share the lane sums and the tree):
//             LDS path    when k_in * (row_bytes + kMmrRowPad) fits beside the state in the CU's LDS (mmr_rows_in_lds): a row's
//                         LPR lanes read their 16-byte chunks from LDS (ds_read_b128), four rows per lane in flight, l2_lane_* /
//                         ip_lane_* (f32 rows: l2_finish / ip_finish's terms), row_butterfly.  The query is the pick's row
//                         where it lies in LDS, each lane widening its own 8 elements: no query vector and no barrier for it.
//                         The row stride is padded by 16 B so that the lanes of different rows of one load do not meet in a bank;
//             table path  otherwise: the pick's row is widened into the LDS query vector, a barrier, then
//                         wg_score_l2<LPR, DT, 1024, METRIC> straight from the table with the row list in LDS;
//          4. p and v of every entry from its similarity.
// Two barriers per step on the LDS path, three on the table path.  Nothing here waits on another wavefront outside
// __syncthreads().  The kernel has no static LDS: the launch's dynamic size is all it takes, up to the CU's 160 KB.
#pragma once
#include <cstdint>

#include "nann_filter.h"

namespace nann {

constexpr int kMmrNT = 1024;            // threads of k_mmr = the longest list (kMaxK): one entry per thread
constexpr int kMmrLdsBytes = 163840;    // a CU's LDS (160 KB), all of which one workgroup may take
constexpr int kMmrStateBytes = 18560;   // the state in front of the candidate rows: 16 KB + f32[512] + u64[16]
constexpr int kMmrRowPad = 16;          // bytes added to a candidate row's stride in LDS
static_assert(kMmrNT == kMaxK, "one entry per thread");

// the LDS path: do k_in rows of row_bytes each fit beside the state?  (NANN_MMR_TABLE_ONLY: a build variant for the A/B of the
// two paths, tools/diverse_rate.py)
__host__ __device__ inline bool mmr_rows_in_lds(int k_in, int row_bytes) {
#ifdef NANN_MMR_TABLE_ONLY
  (void)k_in;
  (void)row_bytes;
  return false;
#else
  return (long long)k_in * (row_bytes + kMmrRowPad) <= (long long)(kMmrLdsBytes - kMmrStateBytes);
#endif
}

struct MmrArgs {
  FilterArgs f;                 // validity: f.n_items bounds the rows; deny bitmap and exclusion lists, any of them null
  const void* emb;              // the index's rows
  int d, dt;                    // 64 | 128 | 256 | 512; NANN_F16 | NANN_BF16 | NANN_F32
  int metric;                   // MT_L2 | MT_IP
  const int32_t* in_rows;       // i32[n_queries, k_in]
  const float* in_scores;       // f32, the same shape
  int k_in;                     // <= kMaxK
  const int32_t* n_valid;       // query i counts n_valid[i * nv_stride] entries; null: k_in
  int nv_stride;                //   (1: i32[n_queries]; 6, from &level_topn[0][5]: a traversal's per-query level_topn)
  const int32_t* status;        // i32[n_queries] or null: a query with a non-zero word counts none
  float lambda;                 // in [0, 1]: the lambda of every query when lambdas is null
  const float* lambdas;         // f32[n_queries] or null
  int k;
  const int64_t* item_ids;      // i64[n_items]; may be null when out_item_ids is
  int32_t* out_index;           // [n_queries, k] each, any of them may be null
  float* out_scores;
  float* out_mmr;
  int32_t* out_pos;
  int64_t* out_item_ids;
  int32_t* n_out;               // i32[n_queries] or null
  int lds_rows;                 // launch_mmr's: 1 = the LDS path
};
// the caller has held the shape to the kernel's limits: 0 <= k, 0 <= k_in <= 1024, n_queries <= 2^31 - 1, d and dt as above
int launch_mmr(const MmrArgs& a, long long n_queries, hipStream_t st);

}  // namespace nann

#ifdef NANN_MMR_IMPL  // the kernel: nann_cand_inst.hip only
namespace nann {

constexpr int kMmrSlots = 2048;  // slots of the setup's row table: twice the longest list, never more than half full
static_assert(kMmrSlots >= 2 * kMaxK && kMmrSlots * 8 == 16384 && kMmrStateBytes == 16384 + kMaxD * 4 + (kMmrNT / 64) * 8,
              "the state: the row table and its flags (later: rows and similarities), the query vector, the wavefronts' words");
static_assert(kMmrStateBytes % 16 == 0 && kMmrRowPad % 16 == 0, "candidate rows are read 16 bytes at a time");

__device__ __forceinline__ int mmr_hash(int32_t r) { return (int)(((uint32_t)r * 2654435761u) >> 21); }  // 11 bits

// element e of a row, widened exactly
template <int DT>
__device__ __forceinline__ float mmr_widen(const void* row, int e) {
  if constexpr (DT == DT_F32) return static_cast<const float*>(row)[e];
  else if constexpr (DT == DT_F16) return half_bits_to_float(static_cast<const uint16_t*>(row)[e]);
  else return bf16_bits_to_float(static_cast<const uint16_t*>(row)[e]);
}

// sim[i] for 0 <= i < n from the candidate rows in LDS (row i at cand + i * stride): the lane layout, the lane sums and the
// tree of wg_score_l2_part.  All 16 wavefronts; every lane of a wavefront runs every trip (a position past n reads row n - 1
// and drops the result), so the butterfly never meets an idle lane.
// The query is the picked row, read where it lies: lane `sub` of a row's group widens its own 8 elements of it.
template <int LPR, int DT, int METRIC>
__device__ __forceinline__ void mmr_score_lds(const unsigned char* cand, int stride, int n, const unsigned char* qrow, float* sim) {
  constexpr int GPW = 64 / LPR, RPI = (kMmrNT / 64) * GPW;
  constexpr int U = 4;                               // rows per lane in flight: the loads of a trip stand in front of its sums
  constexpr int kChunk = DT == DT_F32 ? 32 : 16;     // bytes of a lane's 8 elements
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub = lane % LPR, grp = lane / LPR;
  auto load = [&](const unsigned char* row) -> RowChunk<DT> {
    RowChunk<DT> c;
    c.a = *reinterpret_cast<const uint4*>(row + sub * kChunk);
    if constexpr (DT == DT_F32) c.b = *reinterpret_cast<const uint4*>(row + sub * kChunk + 16);
    else c.b = make_uint4(0, 0, 0, 0);
    return c;
  };
  float q[8];
  chunk_to_float<DT>(load(qrow), q);
  for (int base = wave * GPW + grp; base - grp < n; base += RPI * U) {
    RowChunk<DT> c[U];
#pragma unroll
    for (int u = 0; u < U; ++u) c[u] = load(cand + (size_t)min(base + u * RPI, n - 1) * stride);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = base + u * RPI;
      float s;
      if constexpr (DT == DT_F32) {
        float x[8];
        chunk_to_float<DT>(c[u], x);
        if constexpr (METRIC == MT_IP) s = ip_finish<LPR>(q, x); else s = l2_finish<LPR>(q, x);
      } else {
        if constexpr (METRIC == MT_IP) s = row_butterfly<LPR>(DT == DT_F16 ? ip_lane_f16(q, c[u].a) : ip_lane_bf16(q, c[u].a));
        else s = 0.0f - row_butterfly<LPR>(DT == DT_F16 ? l2_lane_f16(q, c[u].a) : l2_lane_bf16(q, c[u].a));
      }
      if (sub == 0 && i < n) sim[i] = s;
    }
  }
}

template <int LPR, int DT, int METRIC>
__global__ __launch_bounds__(kMmrNT) void k_mmr(MmrArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mmr_smem[];
  int32_t* tab = reinterpret_cast<int32_t*>(mmr_smem);                        // setup: the row table ...
  int32_t* hit = reinterpret_cast<int32_t*>(mmr_smem + kMmrSlots * 4);        //   ... and its flags
  int32_t* ids = reinterpret_cast<int32_t*>(mmr_smem);                        // the steps: the row of every entry (invalid: 0)
  float* sim = reinterpret_cast<float*>(mmr_smem + kMaxK * 4);                //   ... and its similarity to the last pick
  float* qv = reinterpret_cast<float*>(mmr_smem + kMmrSlots * 8);             // the last pick's row, f32[d]
  unsigned long long* red = reinterpret_cast<unsigned long long*>(mmr_smem + kMmrSlots * 8 + kMaxD * 4);  // one per wavefront
  unsigned char* cand = mmr_smem + kMmrStateBytes;                            // the LDS path: the candidate rows
  constexpr int kRowBytes = LPR * 8 * (DT == DT_F32 ? 4 : 2);
  constexpr int kStride = kRowBytes + kMmrRowPad;
  const size_t qi = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int n = a.n_valid ? a.n_valid[qi * (size_t)a.nv_stride] : a.k_in;
  if (a.status && a.status[qi] != 0) n = 0;
  n = max(0, min(n, min(a.k_in, kMaxK)));
  float lam = a.lambda;
  if (a.lambdas) {
    const float x = a.lambdas[qi];
    lam = !(x >= 0.0f) ? 0.0f : (x > 1.0f ? 1.0f : x);
  }
  const float b = __fsub_rn(1.0f, lam);
  long long lb = 0, le = 0;
  if (filter_has_lists(a.f)) {  // (the list of query qi, clamped to [0, n_excl]; an inverted one is empty)
    const long long lo = a.f.splits[qi], hi = a.f.splits[qi + 1];
    lb = min(max(lo, 0ll), a.f.n_excl);
    le = max(lb, min(max(hi, 0ll), a.f.n_excl));
  }
  const bool lists = le > lb && n > 0;  // (uniform over the workgroup)
  if (lists) {
    for (int i = tid; i < kMmrSlots; i += kMmrNT) { tab[i] = -1; hit[i] = 0; }
    __syncthreads();
  }
  // ---- setup: the valid entries
  const int32_t row = tid < n ? a.in_rows[qi * (size_t)a.k_in + tid] : -1;
  const float score = tid < n ? a.in_scores[qi * (size_t)a.k_in + tid] : 0.0f;
  bool ok = row >= 0 && (long long)row < a.f.n_items && (__float_as_uint(score) & 0x7f800000u) != 0x7f800000u;
  if (ok && a.f.deny_bits) ok = ((a.f.deny_bits[row >> 5] >> (row & 31)) & 1u) == 0u;
  if (lists) {
    int slot = -1;
    if (ok) {
      int h = mmr_hash(row);
      for (;;) {  // (ends: at most kMaxK of the kMmrSlots slots are taken; a repeated row shares its slot)
        const int32_t prev = atomicCAS(&tab[h], -1, row);
        if (prev == -1 || prev == row) break;
        h = (h + 1) & (kMmrSlots - 1);
      }
      slot = h;
    }
    __syncthreads();
    for (long long i = lb + tid; i < le; i += kMmrNT) {
      const int32_t r = a.f.rows[i];
      if (r < 0 || (long long)r >= a.f.n_items) continue;
      int h = mmr_hash(r);
      for (;;) {  // (ends: an empty slot is met, the table is never more than half full)
        const int32_t key = tab[h];
        if (key == r) hit[h] = 1;
        if (key == r || key == -1) break;
        h = (h + 1) & (kMmrSlots - 1);
      }
    }
    __syncthreads();
    if (slot >= 0 && hit[slot]) ok = false;
    __syncthreads();  // (the table and the flags are read for the last time: the row list takes their place)
  }
  ids[tid] = ok ? row : 0;
  // the number of valid entries: a ballot per wavefront, the 16 counts through the query vector's LDS (free until the first
  // pick is widened into it, behind step 0's barrier); no static LDS, so that the launch's dynamic size is all the kernel takes
  int* cnt = reinterpret_cast<int*>(qv);
  const unsigned long long okm = __ballot(ok);
  if (lane == 0) cnt[wave] = __popcll(okm);
  __syncthreads();  // (also: the row list is whole)
  int n_ok = 0;
#pragma unroll
  for (int w = 0; w < kMmrNT / 64; ++w) n_ok += cnt[w];
  const int n_pick = min(a.k, n_ok);
  if (n_pick > 0 && a.lds_rows) {
    constexpr int CPR = kRowBytes / 16;  // 16-byte chunks of a row
    for (int c = tid; c < n * CPR; c += kMmrNT) {
      const int j = c / CPR, s = c % CPR;
      *reinterpret_cast<uint4*>(cand + (size_t)j * kStride + s * 16) =
          *reinterpret_cast<const uint4*>(static_cast<const unsigned char*>(a.emb) + (size_t)ids[j] * kRowBytes + s * 16);
    }
    // (the first reader of these rows stands behind the barrier of step 0's argmax)
  }
  // ---- the steps
  const float r = __fmul_rn(lam, score);
  float p = 0.0f, v = r;
  bool avail = ok;
  for (int step = 0; step < n_pick; ++step) {
    // 1. the greatest key among the valid unpicked entries, ties to the lower j
    //    (a wavefront: the greatest key by DPP, then the lowest lane that holds it -- an idle lane counts as key 0, which no
    //     valid key is below, so the ballot is empty only where the wavefront has no valid unpicked entry)
    const uint32_t kv = avail ? score_key(v) : 0u;
    const uint32_t wmax = wave_max(kv);
    const unsigned long long holders = __ballot(avail && kv == wmax);
    if (lane == 0)
      red[wave] = holders ? ((1ull << 42) | ((unsigned long long)wmax << 10) |
                             (unsigned long long)(1023 - (wave * 64 + __ffsll((long long)holders) - 1))) : 0ull;
    __syncthreads();
    unsigned long long best = red[0];
#pragma unroll
    for (int w = 1; w < kMmrNT / 64; ++w) {
      const unsigned long long other = red[w];
      best = other > best ? other : best;
    }
    const int t = 1023 - (int)(best & 1023ull);  // (n_pick <= #valid: a valid unpicked entry exists, best != 0)
    // 2. the pick
    if (tid == t) {
      const size_t at = qi * (size_t)a.k + step;
      if (a.out_index) a.out_index[at] = row;
      if (a.out_scores) a.out_scores[at] = score;
      if (a.out_mmr) a.out_mmr[at] = v;
      if (a.out_pos) a.out_pos[at] = tid;
      if (a.out_item_ids) a.out_item_ids[at] = a.item_ids[row];
      avail = false;
    }
    if (step + 1 == n_pick) break;
    // 3. the similarities of entries 0 .. n - 1 to the pick
    if (a.lds_rows) {  // (uniform) the pick's row is read where it lies, by the lanes that need it: no query vector, no barrier
      mmr_score_lds<LPR, DT, METRIC>(cand, kStride, n, cand + (size_t)t * kStride, sim);
    } else {
      if (tid < LPR * 8) qv[tid] = mmr_widen<DT>(static_cast<const unsigned char*>(a.emb) + (size_t)ids[t] * kRowBytes, tid);
      __syncthreads();
      wg_score_l2<LPR, DT, kMmrNT, METRIC>(a.emb, LPR * 8, ids, n, qv, sim);
    }
    __syncthreads();
    // 4. the penalty and the value
    const float sj = tid < n ? sim[tid] : 0.0f;
    p = step == 0 ? sj : (sj > p ? sj : p);
    v = __fsub_rn(r, __fmul_rn(b, p));
  }
  // ---- zeros behind the picks
  for (int i = n_pick + tid; i < a.k; i += kMmrNT) {
    const size_t at = qi * (size_t)a.k + i;
    if (a.out_index) a.out_index[at] = 0;
    if (a.out_scores) a.out_scores[at] = 0.0f;
    if (a.out_mmr) a.out_mmr[at] = 0.0f;
    if (a.out_pos) a.out_pos[at] = 0;
    if (a.out_item_ids) a.out_item_ids[at] = 0;
  }
  if (a.n_out && tid == 0) a.n_out[qi] = n_pick;
}

}  // namespace nann
#endif
