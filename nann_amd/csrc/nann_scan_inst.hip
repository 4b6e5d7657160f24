// nann_scan_inst.hip -- the kernels of the exhaustive search (nann_scan.h): the L2 and inner-product scans for every (d, row dtype), the MLP scan
// in both precisions, the slab top-k and the merge, the range selection (nann_range.h) and the wide selection (nann_wide.h); workspace layout and the launch
// sequence of a call.
#define NANN_SCAN_IMPL
#include "nann_scan.h"

#include <algorithm>

namespace nann {

namespace {
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
constexpr size_t kScanScoreBytes = (size_t)512 << 20;  // most bytes of a chunk's score buffer -- or one query's scores (4 B x n_items) where that is more
}  // namespace

ScanLayout scan_layout(long long n_items, int d, int kind, long long n_queries, int k) {
  ScanLayout L = {};
  const int tq = kScanTileQueries;
  long long chunk = std::min<long long>(kScanMaxChunk, (long long)(kScanScoreBytes / ((size_t)n_items * 4)));
  chunk = std::max<long long>(1, std::min(chunk, n_queries));
  const bool flat = kind == NANN_SCORER_L2 || kind == NANN_SCORER_IP;  // the vector scans: tiles of queries, a transposed copy
  if (flat && chunk > tq) chunk -= chunk % tq;  // whole tiles of queries
  L.chunk = (int)chunk;
  L.n_slabs = scan_n_slabs(n_items);
  const size_t cand = (size_t)L.chunk * L.n_slabs * k * 4;
  const size_t qbytes = flat ? (size_t)((L.chunk + tq - 1) / tq) * tq * d * 4
                        : kind == kScanAttn ? (size_t)L.chunk * kScanAttnUserBytes : (size_t)L.chunk * 256 * 4;
  L.off_scores = 0;
  L.off_cand_scores = up256((size_t)L.chunk * (size_t)n_items * 4);
  L.off_cand_rows = L.off_cand_scores + up256(cand);
  L.off_q = L.off_cand_rows + up256(cand);
  L.total = L.off_q + up256(qbytes);
  return L;
}

template <int LPR, int DT, int METRIC>
static int launch_scan_l2_as(const ScanArgs& a, const float* qT, int n_q, float* scores, hipStream_t st) {
  constexpr int TQ = kScanTileQueries;
  const int tiles = (n_q + TQ - 1) / TQ;
  const long long blocks = (a.n_items + kScanRows - 1) / kScanRows * tiles;
  if (blocks > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, "nann_search_all: index too large for one launch");
  if constexpr (METRIC == MT_IP)
    hipLaunchKernelGGL((k_scan_ip<LPR, DT, TQ>), dim3((unsigned)blocks), dim3(kScanRows), 0, st, a.emb, a.n_items, qT, n_q, tiles, scores);
  else
    hipLaunchKernelGGL((k_scan_l2<LPR, DT, TQ>), dim3((unsigned)blocks), dim3(kScanRows), 0, st, a.emb, a.n_items, qT, n_q, tiles, scores);
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

template <int LPR, int METRIC>
static int launch_scan_l2_dt(const ScanArgs& a, const float* qT, int n_q, float* scores, hipStream_t st) {
  if (a.dt == NANN_F16) return launch_scan_l2_as<LPR, DT_F16, METRIC>(a, qT, n_q, scores, st);
  if (a.dt == NANN_BF16) return launch_scan_l2_as<LPR, DT_BF16, METRIC>(a, qT, n_q, scores, st);
  return launch_scan_l2_as<LPR, DT_F32, METRIC>(a, qT, n_q, scores, st);
}

template <int METRIC>
static int launch_scan_flat(const ScanArgs& a, const float* qT, int n_q, float* scores, hipStream_t st) {
  switch (a.d / 8) {
    case 8: return launch_scan_l2_dt<8, METRIC>(a, qT, n_q, scores, st);
    case 16: return launch_scan_l2_dt<16, METRIC>(a, qT, n_q, scores, st);
    case 32: return launch_scan_l2_dt<32, METRIC>(a, qT, n_q, scores, st);
    case 64: return launch_scan_l2_dt<64, METRIC>(a, qT, n_q, scores, st);
    default: return fail(NANN_ERR_UNSUPPORTED, "nann_search_all: d must be 64, 128, 256 or 512");
  }
}

template <bool EXACT>
static int launch_scan_mlp_as(const ScanArgs& a, const float* u, int n_q, float* scores, hipStream_t st) {
  auto kern = k_scan_mlp<EXACT>;
  NANN_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kMlpResBytes));
  const long long n_work = (a.n_items + kScanMlpRows - 1) / kScanMlpRows * n_q;
  const unsigned grid = (unsigned)std::min<long long>(n_work, std::max(1, a.mlp_workgroups));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), (size_t)kMlpResBytes, st, a.mlp, a.proj, a.n_items, u, n_q, scores);
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

int launch_range(const ScanRange& r, const float* scores, long long n_items, long long c0, int n_q, const int64_t* item_ids,
                 int64_t* out_item_ids, float* out_scores, int32_t* out_index, hipStream_t st) {
  static_assert(kScanMaxChunk <= kRangeNT, "k_range_splits: one thread per query of a chunk");
  int32_t* totals = r.counts + (size_t)n_q * r.n_blocks;
  const dim3 grid((unsigned)r.n_blocks, (unsigned)n_q);
  hipLaunchKernelGGL(k_range_count, grid, dim3(kRangeNT), 0, st, scores, n_items, r.thr, c0, r.counts);
  NANN_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_range_scan, dim3((unsigned)n_q), dim3(kRangeNT), 0, st, r.counts, r.n_blocks, totals);
  NANN_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_range_splits, dim3(1), dim3(kRangeNT), 0, st, totals, n_q, c0, r.row_splits);
  NANN_HIP_TRY(hipGetLastError());
  if (r.capacity <= 0) return NANN_OK;  // a count-only call: nothing to fill
  hipLaunchKernelGGL(k_range_fill, grid, dim3(kRangeNT), 0, st, scores, n_items, r.thr, c0, r.counts, r.row_splits, r.capacity,
                     item_ids, out_item_ids, out_scores, out_index);
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

int launch_wide(const ScanWide& w, const float* scores, size_t limit, long long n_items, long long q0, int n_q,
                const int64_t* item_ids, int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* n_out, hipStream_t st) {
  static_assert(kScanMaxChunk <= kWideMaxChunk, "launch_wide: a chunk of the scan is one grid");
  if (n_q < 1 || n_q > kWideMaxChunk || w.k < 1 || w.k > kWideMaxK) return fail(NANN_ERR_BAD_ARGUMENT, "launch_wide: shape");
  const dim3 grid((unsigned)w.n_blocks, (unsigned)n_q), nt(kRangeNT);
  const size_t hq = (size_t)n_q * kWideBins;  // a pass's histograms
  NANN_HIP_TRY(hipMemsetAsync(w.hist, 0, (size_t)kWidePasses * hq * 4, st));
  hipLaunchKernelGGL(k_wide_hist<0>, grid, nt, 0, st, scores, limit, n_items, q0, w.state, w.hist);
  hipLaunchKernelGGL(k_wide_pick<0>, dim3((unsigned)n_q), nt, 0, st, w.hist, w.state, w.k);
  hipLaunchKernelGGL(k_wide_hist<1>, grid, nt, 0, st, scores, limit, n_items, q0, w.state, w.hist + hq);
  hipLaunchKernelGGL(k_wide_pick<1>, dim3((unsigned)n_q), nt, 0, st, w.hist + hq, w.state, w.k);
  hipLaunchKernelGGL(k_wide_hist<2>, grid, nt, 0, st, scores, limit, n_items, q0, w.state, w.hist + 2 * hq);
  hipLaunchKernelGGL(k_wide_pick<2>, dim3((unsigned)n_q), nt, 0, st, w.hist + 2 * hq, w.state, w.k);
  NANN_HIP_TRY(hipGetLastError());
  int32_t* totals = w.counts + (size_t)2 * n_q * w.n_blocks;
  hipLaunchKernelGGL(k_wide_count, grid, nt, 0, st, scores, limit, n_items, q0, w.state, w.counts);
  hipLaunchKernelGGL(k_range_scan, dim3((unsigned)(2 * n_q)), nt, 0, st, w.counts, w.n_blocks, totals);
  hipLaunchKernelGGL(k_wide_fill, grid, nt, 0, st, scores, limit, n_items, q0, w.state, w.counts, w.k, w.stage);
  NANN_HIP_TRY(hipGetLastError());
  int P = 1;
  while (P < w.k) P <<= 1;
  const size_t lds = (size_t)P * 8;
  NANN_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_wide_sort), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_wide_sort, dim3((unsigned)n_q), dim3(kWideSortNT), lds, st, w.stage, w.state, w.k, P, scores, n_items, q0, item_ids,
                     out_item_ids, out_scores, out_index, n_out);
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

int launch_scan(const ScanArgs& a, const ScanLayout& L, const float* q, long long n_queries, int k, unsigned char* ws,
                int64_t* out_item_ids, float* out_scores, int32_t* out_index, hipStream_t st) {
  float* scores = reinterpret_cast<float*>(ws + L.off_scores);
  float* cand_scores = reinterpret_cast<float*>(ws + L.off_cand_scores);
  int32_t* cand_rows = reinterpret_cast<int32_t*>(ws + L.off_cand_rows);
  float* qbuf = reinterpret_cast<float*>(ws + L.off_q);
  for (long long c0 = 0; c0 < n_queries; c0 += L.chunk) {
    const int n_q = (int)std::min<long long>(L.chunk, n_queries - c0);
    const float* qc = q + (size_t)c0 * a.d;
    int rc;
    if (a.kind == kScanAttn) {  // the chunk's users: kt [n_q][256][64] then upad [n_q][64][64], as the traversal takes them
      const uint16_t* seq = reinterpret_cast<const uint16_t*>(q) + (size_t)c0 * a.attn.L * kAttnE;
      float* kt = qbuf;
      float* upad = qbuf + (size_t)n_q * 256 * kAttnLP;
      rc = a.exact ? launch_attn_prepare(st, a.attn, seq, n_q, kt, upad) : launch_attn_prepare_split(st, a.attn, seq, n_q, kt, upad);
      if (rc) return rc;
      rc = launch_scan_attn(a, kt, upad, n_q, scores, st);
    } else if (a.kind == NANN_SCORER_L2 || a.kind == NANN_SCORER_IP) {
      const int tq = kScanTileQueries;
      const long long total = (long long)((n_q + tq - 1) / tq) * tq * a.d;
      hipLaunchKernelGGL(k_scan_transpose_q, dim3((unsigned)std::min<long long>((total + 255) / 256, 1024)), dim3(256), 0, st, qc, n_q, a.d, tq, qbuf);
      NANN_HIP_TRY(hipGetLastError());
      rc = a.kind == NANN_SCORER_IP ? launch_scan_flat<MT_IP>(a, qbuf, n_q, scores, st) : launch_scan_flat<MT_L2>(a, qbuf, n_q, scores, st);
    } else if (a.kind == NANN_SCORER_MLP) {
      hipLaunchKernelGGL(k_scan_mlp_u, dim3((unsigned)n_q), dim3(256), 0, st, a.mlp, qc, qbuf);
      NANN_HIP_TRY(hipGetLastError());
      rc = a.exact ? launch_scan_mlp_as<true>(a, qbuf, n_q, scores, st) : launch_scan_mlp_as<false>(a, qbuf, n_q, scores, st);
    } else {
      return fail(NANN_ERR_BAD_ARGUMENT, "nann_search_all: unknown scorer kind");
    }
    if (rc) return rc;
    if (a.filter) {  // the denied rows of this chunk leave the selection: exclusion lists go by the call's query number c0 + i
      rc = launch_filter_scatter(a.filter->f, scores, c0, n_q, st);
      if (rc) return rc;
      if (a.filter->pred) rc = launch_pred_scatter(*a.filter->pred, scores, a.n_items, c0, n_q, st);  // ... and the rows that fail its predicates
      if (rc) return rc;
    }
    if (a.range) {  // every row at or above the cut, not the best k: the ragged outputs are addressed by the call's row_splits
      rc = launch_range(*a.range, scores, a.n_items, c0, n_q, a.item_ids, out_item_ids, out_scores, out_index, st);
      if (rc) return rc;
      continue;
    }
    if (a.wide) {  // the top k for k up to kWideMaxK: cut, gather, sort; the buffer is readable to the next 256-byte boundary
      const size_t limit = ((size_t)n_q * (size_t)a.n_items + 3) & ~(size_t)3;
      rc = launch_wide(*a.wide, scores, limit, a.n_items, 0, n_q, a.item_ids, out_item_ids + (size_t)c0 * k,
                       out_scores ? out_scores + (size_t)c0 * k : nullptr, out_index ? out_index + (size_t)c0 * k : nullptr,
                       a.wide->n_out ? a.wide->n_out + c0 : nullptr, st);
      if (rc) return rc;
      continue;
    }
    hipLaunchKernelGGL(k_scan_slab_topk, dim3((unsigned)((long long)n_q * L.n_slabs)), dim3(kNT), 0, st, scores, a.n_items, L.n_slabs, k,
                       cand_scores, cand_rows);
    NANN_HIP_TRY(hipGetLastError());
    if (a.filter) {
      // the merge's lists go to the staging area; the final rows are their allowed entries (a query with fewer than k allowed
      // rows has denied ones, at -inf, in its list)
      int64_t* s_ids = reinterpret_cast<int64_t*>(a.filter->stage);
      float* s_scores = reinterpret_cast<float*>(s_ids + (size_t)L.chunk * k);
      int32_t* s_rows = reinterpret_cast<int32_t*>(s_scores + (size_t)L.chunk * k);
      hipLaunchKernelGGL(k_scan_merge, dim3((unsigned)n_q), dim3(kNT), 0, st, cand_scores, cand_rows, L.n_slabs * k, k, a.item_ids,
                         s_ids, s_scores, s_rows);
      NANN_HIP_TRY(hipGetLastError());
      // (the shape both compactions hold their launch to, 0 <= k <= kMaxK, is flat_check's: it stood before the first chunk was scored)
      if (a.filter->pred) {  // (a query with fewer than k passing rows has failing ones, at -inf, in its list as well)
        PredCompactArgs pc = {};
        pc.f = a.filter->f;
        pc.p = *a.filter->pred;
        pc.in_rows = s_rows;
        pc.in_scores = s_scores;
        pc.in_stride = pc.n_in = k;
        pc.q0 = c0;
        pc.k = k;
        pc.item_ids = a.item_ids;
        pc.out_item_ids = out_item_ids + (size_t)c0 * k;
        pc.out_scores = out_scores ? out_scores + (size_t)c0 * k : nullptr;
        pc.out_index = out_index ? out_index + (size_t)c0 * k : nullptr;
        pc.n_out = a.filter->n_out ? a.filter->n_out + c0 : nullptr;
        rc = launch_pred_compact(pc, n_q, st);
        if (rc) return rc;
        continue;
      }
      rc = launch_filter_compact(a.filter->f, s_rows, s_scores, k, k, nullptr, nullptr, c0, n_q, k, a.item_ids,
                                 out_item_ids + (size_t)c0 * k, out_scores ? out_scores + (size_t)c0 * k : nullptr,
                                 out_index ? out_index + (size_t)c0 * k : nullptr, a.filter->n_out ? a.filter->n_out + c0 : nullptr, st);
      if (rc) return rc;
      continue;
    }
    hipLaunchKernelGGL(k_scan_merge, dim3((unsigned)n_q), dim3(kNT), 0, st, cand_scores, cand_rows, L.n_slabs * k, k, a.item_ids,
                       out_item_ids + (size_t)c0 * k, out_scores ? out_scores + (size_t)c0 * k : nullptr,
                       out_index ? out_index + (size_t)c0 * k : nullptr);
    NANN_HIP_TRY(hipGetLastError());
  }
  return NANN_OK;
}

}  // namespace nann
