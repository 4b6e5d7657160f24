// nann_lists_inst.hip -- the kernels of the shared-list search (nann_lists.h): the partition build, the plan of a chunk, the tiles'
// transposed queries, the L2 and inner-product list scans for every (d, row dtype), the pad and the finish; workspace layout and
// the launch sequence of a call; the int8 form's scan over the code table for every (d, metric), its fetch and finish kernels, its
// workspace layout and launch sequence.  Rides in nann_scan.o behind nann_scan_inst.hip and nann_sq8_inst.hip: the scans are
// ScanL2's (nann_scan.h), the int8 form's epilogue and encoder are nann_sq8.h's.
#ifndef NANN_SCAN_IMPL
#define NANN_SCAN_IMPL
#endif
#ifndef NANN_SQ8_IMPL
#define NANN_SQ8_IMPL
#endif
#define NANN_LISTS_IMPL
#include "nann_lists.h"
#include "nann_cand.h"

#include <algorithm>

namespace nann {

ListsLayout lists_layout(long long max_len, int d, long long n_queries, int n_probe, int k) {
  ListsLayout L = {};
  L.S = std::max<long long>({1, (long long)k, (long long)n_probe * max_len});
  long long chunk = std::min<long long>(kListsMaxChunk, (long long)(((size_t)512 << 20) / ((size_t)L.S * 4)));
  chunk = std::max<long long>(1, std::min(chunk, n_queries));
  if (chunk > kScanTileQueries) chunk -= chunk % kScanTileQueries;  // whole tiles of queries
  L.chunk = (int)chunk;
  L.n_slabs = scan_n_slabs(L.S);
  L.max_tiles = L.chunk * std::max(1, n_probe);
  const size_t cand = (size_t)L.chunk * L.n_slabs * k * 4;
  L.off_scores = 0;
  L.off_cand_scores = lists_up256((size_t)L.chunk * (size_t)L.S * 4);
  L.off_cand_rows = L.off_cand_scores + lists_up256(cand);
  L.off_pos = L.off_cand_rows + lists_up256(cand);
  L.off_head = L.off_pos + lists_up256((size_t)L.chunk * k * 4);
  L.off_queries = L.off_head + lists_up256(sizeof(ListsHead));
  L.off_blk = L.off_queries + lists_up256((size_t)L.chunk * sizeof(ListsQuery));
  L.off_tiles = L.off_blk + lists_up256((size_t)(L.max_tiles + 1) * 8);
  L.off_qt = L.off_tiles + lists_up256((size_t)L.max_tiles * sizeof(ListsTile));
  L.total = L.off_qt + lists_up256((size_t)L.max_tiles * d * kScanTileQueries * 4);
  return L;
}

// ---- the partition build ----------------------------------------------------------------------------------------------------
// row groups of a build: one wavefront each, at least 4096 rows each, and at most 32 MB of counts
size_t lists_build_groups(long long n_items, int n_lists) {
  const long long by_rows = (n_items + 4095) / 4096, by_bytes = ((long long)32 << 20) / ((long long)std::max(1, n_lists) * 4);
  return (size_t)std::max<long long>(1, std::min<long long>({(long long)kListsGroupsMax, by_rows, by_bytes}));
}

int launch_lists_count(const int32_t* list_of_row, long long n_items, int n_lists, int groups, int32_t* counts, long long* info, hipStream_t st) {
  hipLaunchKernelGGL(k_lists_count, dim3((unsigned)groups), dim3(64), 0, st, list_of_row, n_items, n_lists, groups, counts, info);
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

int launch_lists_splits(int n_lists, int groups, int32_t* counts, int64_t* list_splits, long long* info, hipStream_t st) {
  if (n_lists > 0) hipLaunchKernelGGL(k_lists_group_prefix, dim3((unsigned)((n_lists + 255) / 256)), dim3(256), 0, st, n_lists, groups, counts, list_splits);
  hipLaunchKernelGGL(k_lists_splits, dim3(1), dim3(256), 0, st, n_lists, list_splits, info);
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

int launch_lists_fill(const int32_t* list_of_row, long long n_items, int n_lists, int groups, int32_t* counts,
                      const int64_t* list_splits, int32_t* list_rows, hipStream_t st) {
  hipLaunchKernelGGL(k_lists_fill, dim3((unsigned)groups), dim3(64), 0, st, list_of_row, n_items, n_lists, groups, counts, list_splits, list_rows);
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

// ---- the search -----------------------------------------------------------------------------------------------------------------
// what a list scan takes, one kernel argument each (nann_lists.h: NANN_LISTS_SCAN_PARAMS)
struct ListsScanArgs {
  const void* emb;
  const int32_t* list_rows;
  const ListsHead* head;
  const long long* blk;
  const ListsTile* tiles;
  const float* qT;
  float* scores;  // f32[chunk, stride]
  long long stride;
};

template <int LPR, int METRIC>
static void launch_lists_scan_dt(int dt, const ListsScanArgs& s, unsigned grid, hipStream_t st) {
  auto run = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kScanRows), 0, st, s.emb, s.list_rows, s.head, s.blk, s.tiles, s.qT, s.scores, s.stride);
  };
  if constexpr (METRIC == MT_IP) {
    if (dt == NANN_F16) run(k_lists_scan_ip<LPR, DT_F16>);
    else if (dt == NANN_BF16) run(k_lists_scan_ip<LPR, DT_BF16>);
    else run(k_lists_scan_ip<LPR, DT_F32>);
  } else {
    if (dt == NANN_F16) run(k_lists_scan_l2<LPR, DT_F16>);
    else if (dt == NANN_BF16) run(k_lists_scan_l2<LPR, DT_BF16>);
    else run(k_lists_scan_l2<LPR, DT_F32>);
  }
}

template <int METRIC>
static int launch_lists_scan(int d, int dt, const ListsScanArgs& s, unsigned grid, hipStream_t st) {
  switch (d / 8) {
    case 8: launch_lists_scan_dt<8, METRIC>(dt, s, grid, st); break;
    case 16: launch_lists_scan_dt<16, METRIC>(dt, s, grid, st); break;
    case 32: launch_lists_scan_dt<32, METRIC>(dt, s, grid, st); break;
    case 64: launch_lists_scan_dt<64, METRIC>(dt, s, grid, st); break;
    default: return fail(NANN_ERR_UNSUPPORTED, "nann_search_lists: d must be 64, 128, 256 or 512");
  }
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

int launch_lists(const ListsArgs& a, const ListsLayout& L, const float* q, long long n_queries, int k, unsigned char* ws,
                 int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* out_pos, int32_t* n_out, int32_t* status,
                 hipStream_t st) {
  if (a.kind != NANN_SCORER_L2 && a.kind != NANN_SCORER_IP) return fail(NANN_ERR_UNSUPPORTED, "nann_search_lists: L2 and inner-product scorers only");
  float* scores = reinterpret_cast<float*>(ws + L.off_scores);
  float* cand_scores = reinterpret_cast<float*>(ws + L.off_cand_scores);
  int32_t* cand_rows = reinterpret_cast<int32_t*>(ws + L.off_cand_rows);
  ListsHead* head = reinterpret_cast<ListsHead*>(ws + L.off_head);
  ListsQuery* queries = reinterpret_cast<ListsQuery*>(ws + L.off_queries);
  long long* blk = reinterpret_cast<long long*>(ws + L.off_blk);
  ListsTile* tiles = reinterpret_cast<ListsTile*>(ws + L.off_tiles);
  float* qT = reinterpret_cast<float*>(ws + L.off_qt);
  const unsigned resident = (unsigned)std::max(1, a.cus) * 8;
  int n_sort = 2;
  while (n_sort < L.chunk * std::max(1, a.n_probe)) n_sort <<= 1;
  NANN_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_lists_plan), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lists_plan_lds(1 << kListsPairBits)));
  for (long long c0 = 0; c0 < n_queries; c0 += L.chunk) {
    const int n_q = (int)std::min<long long>(L.chunk, n_queries - c0);
    const int32_t* probes = a.probes + (size_t)c0 * a.n_probe;
    ListsPlanArgs p = {};
    p.probes = probes;
    p.n_q = n_q;
    p.n_probe = a.n_probe;
    p.n_lists = a.n_lists;
    p.n_sort = n_sort;
    p.list_splits = a.list_splits;
    p.head = head;
    p.queries = queries;
    p.blk = blk;
    p.tiles = tiles;
    hipLaunchKernelGGL(k_lists_plan, dim3(1), dim3(kListsPlanNT), lists_plan_lds(n_sort), st, p);
    NANN_HIP_TRY(hipGetLastError());
    if (a.n_probe > 0 && a.max_len > 0) {
      const unsigned most_tiles = (unsigned)(n_q * a.n_probe);
      hipLaunchKernelGGL(k_lists_tile_q, dim3(std::min(most_tiles, resident)), dim3(256), 0, st, head, tiles, q + (size_t)c0 * a.d, a.d, qT);
      NANN_HIP_TRY(hipGetLastError());
      ListsScanArgs s = {};
      s.emb = a.emb;
      s.list_rows = a.list_rows;
      s.head = head;
      s.blk = blk;
      s.tiles = tiles;
      s.qT = qT;
      s.scores = scores;
      s.stride = L.S;
      // (at most the work items the chunk can name: every pair a tile of its own)
      const long long most_work = (long long)most_tiles * ((a.max_len + kScanRows - 1) / kScanRows);
      const unsigned grid = (unsigned)std::min<long long>(most_work, resident);
      const int rc = a.kind == NANN_SCORER_IP ? launch_lists_scan<MT_IP>(a.d, a.dt, s, grid, st) : launch_lists_scan<MT_L2>(a.d, a.dt, s, grid, st);
      if (rc) return rc;
    }
    hipLaunchKernelGGL(k_lists_pad, dim3((unsigned)std::min<long long>((L.S + 1023) / 1024, 256), (unsigned)n_q), dim3(256), 0, st, queries, L.S, scores);
    NANN_HIP_TRY(hipGetLastError());
    const int rc = launch_scan_slab_topk(scores, L.S, n_q, k, cand_scores, cand_rows, st);
    if (rc) return rc;
    ListsFinishArgs f = {};
    f.cand_scores = cand_scores;
    f.cand_rows = cand_rows;
    f.n_in = L.n_slabs * k;
    f.k = k;
    f.queries = queries;
    f.probes = probes;
    f.n_probe = a.n_probe;
    f.n_lists = a.n_lists;
    f.list_splits = a.list_splits;
    f.list_rows = a.list_rows;
    f.item_ids = a.item_ids;
    f.pos = reinterpret_cast<int32_t*>(ws + L.off_pos);
    f.out_item_ids = out_item_ids + (size_t)c0 * k;
    f.out_scores = out_scores ? out_scores + (size_t)c0 * k : nullptr;
    f.out_index = out_index ? out_index + (size_t)c0 * k : nullptr;
    f.out_pos = out_pos ? out_pos + (size_t)c0 * k : nullptr;
    f.n_out = n_out ? n_out + c0 : nullptr;
    f.status = status + c0;
    hipLaunchKernelGGL(k_lists_finish, dim3((unsigned)n_q), dim3(kNT), 0, st, f);
    NANN_HIP_TRY(hipGetLastError());
  }
  return NANN_OK;
}

// ---- the int8 form ------------------------------------------------------------------------------------------------------------
ListsSq8Layout lists_sq8_layout(long long max_len, int d, int kind, long long n_queries, int n_probe, int fetch, int k) {
  ListsSq8Layout X = {};
  X.L = lists_layout(max_len, 0, n_queries, n_probe, fetch);  // (d = 0: no qT)
  const size_t c = (size_t)X.L.chunk, cf = c * (size_t)fetch;
  X.off_qcodes = X.L.total;
  X.off_qscales = X.off_qcodes + lists_up256(c * d);
  X.off_qnorms = X.off_qscales + lists_up256(c * 4);
  X.off_fscores = X.off_qnorms + lists_up256(c * 4);
  X.off_spos = X.off_fscores + lists_up256(cf * 4);
  X.off_rows = X.off_spos + lists_up256(cf * 4);
  X.off_splits = X.off_rows + lists_up256(cf * 4);
  X.off_sel = X.off_splits + lists_up256((c + 1) * 8);
  X.off_cand = X.off_sel + lists_up256(c * (size_t)k * 4);
  X.total = X.off_cand + lists_up256(cand_layout(kind, X.L.chunk, (long long)cf).total);
  return X;
}

// what the int8 list scan takes, one kernel argument each
struct ListsScanSq8Args {
  const int8_t* codes;
  const float* scales;
  const int32_t* norms;
  long long n_items;
  const int32_t* list_rows;
  const ListsHead* head;
  const long long* blk;
  const ListsTile* tiles;
  const int8_t* qcodes;
  const float* qscales;
  const int32_t* qnorms;
  float* scores;  // f32[chunk, stride]
  long long stride;
};

template <int METRIC>
static int launch_lists_scan_sq8(int d, const ListsScanSq8Args& s, unsigned grid, hipStream_t st) {
  auto run = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kScanRows), 0, st, s.codes, s.scales, s.norms, s.n_items, s.list_rows, s.head, s.blk,
                       s.tiles, s.qcodes, s.qscales, s.qnorms, s.scores, s.stride);
  };
  switch (d / 64) {
    case 1: run(k_lists_scan_sq8<1, METRIC>); break;
    case 2: run(k_lists_scan_sq8<2, METRIC>); break;
    case 4: run(k_lists_scan_sq8<4, METRIC>); break;
    case 8: run(k_lists_scan_sq8<8, METRIC>); break;
    default: return fail(NANN_ERR_UNSUPPORTED, "nann_search_lists_sq8: d must be 64, 128, 256 or 512");
  }
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

int launch_lists_sq8(const ListsArgs& a, const Sq8Args& t, const ListsSq8Layout& X, const float* q, long long n_queries, int fetch,
                     int k, unsigned char* ws, int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* out_pos,
                     int32_t* n_out, int32_t* status, int32_t* out_fetch_pos, float* out_fetch_scores, hipStream_t st) {
  const ListsLayout& L = X.L;
  if (a.kind != NANN_SCORER_L2 && a.kind != NANN_SCORER_IP) return fail(NANN_ERR_UNSUPPORTED, "nann_search_lists_sq8: L2 and inner-product scorers only");
  if (fetch < 1 || fetch > kMaxK || k < 1 || k > fetch || (a.d != 64 && a.d != 128 && a.d != 256 && a.d != 512) || t.d != a.d)
    return fail(NANN_ERR_BAD_ARGUMENT, "nann_search_lists_sq8: call shape");
  float* scores = reinterpret_cast<float*>(ws + L.off_scores);
  float* cand_scores = reinterpret_cast<float*>(ws + L.off_cand_scores);
  int32_t* cand_rows = reinterpret_cast<int32_t*>(ws + L.off_cand_rows);
  ListsHead* head = reinterpret_cast<ListsHead*>(ws + L.off_head);
  ListsQuery* queries = reinterpret_cast<ListsQuery*>(ws + L.off_queries);
  long long* blk = reinterpret_cast<long long*>(ws + L.off_blk);
  ListsTile* tiles = reinterpret_cast<ListsTile*>(ws + L.off_tiles);
  int8_t* qcodes = reinterpret_cast<int8_t*>(ws + X.off_qcodes);
  float* qscales = reinterpret_cast<float*>(ws + X.off_qscales);
  int32_t* qnorms = reinterpret_cast<int32_t*>(ws + X.off_qnorms);
  const unsigned resident = (unsigned)std::max(1, a.cus) * 8;
  const bool rows_to_score = a.n_probe > 0 && a.max_len > 0;  // (else every query of the call is empty)
  int n_sort = 2;
  while (n_sort < L.chunk * std::max(1, a.n_probe)) n_sort <<= 1;
  NANN_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_lists_plan), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lists_plan_lds(1 << kListsPairBits)));
  CandArgs ca = {};
  ca.emb = a.emb;
  ca.item_ids = a.item_ids;
  ca.n_items = a.n_items;
  ca.d = a.d;
  ca.dt = a.dt;
  ca.kind = a.kind;
  ca.cus = a.cus;
  ca.row_splits = reinterpret_cast<const int64_t*>(ws + X.off_splits);
  ca.rows = reinterpret_cast<const int32_t*>(ws + X.off_rows);
  for (long long c0 = 0; c0 < n_queries; c0 += L.chunk) {
    const int n_q = (int)std::min<long long>(L.chunk, n_queries - c0);
    const int32_t* probes = a.probes + (size_t)c0 * a.n_probe;
    const float* qc = q + (size_t)c0 * a.d;
    ListsPlanArgs p = {};
    p.probes = probes;
    p.n_q = n_q;
    p.n_probe = a.n_probe;
    p.n_lists = a.n_lists;
    p.n_sort = n_sort;
    p.list_splits = a.list_splits;
    p.head = head;
    p.queries = queries;
    p.blk = blk;
    p.tiles = tiles;
    hipLaunchKernelGGL(k_lists_plan, dim3(1), dim3(kListsPlanNT), lists_plan_lds(n_sort), st, p);
    NANN_HIP_TRY(hipGetLastError());
    if (rows_to_score) {
      int rc = launch_sq8_encode(qc, NANN_F32, n_q, a.d, qcodes, qscales, qnorms, st);
      if (rc) return rc;
      ListsScanSq8Args s = {t.codes, t.scales, t.norms, a.n_items, a.list_rows, head, blk, tiles, qcodes, qscales, qnorms, scores, L.S};
      // (at most the work items the chunk can name: every pair a tile of its own)
      const long long most_work = (long long)n_q * a.n_probe * ((a.max_len + kScanRows - 1) / kScanRows);
      const unsigned grid = (unsigned)std::min<long long>(most_work, resident);
      rc = a.kind == NANN_SCORER_IP ? launch_lists_scan_sq8<MT_IP>(a.d, s, grid, st) : launch_lists_scan_sq8<MT_L2>(a.d, s, grid, st);
      if (rc) return rc;
    }
    hipLaunchKernelGGL(k_lists_pad, dim3((unsigned)std::min<long long>((L.S + 1023) / 1024, 256), (unsigned)n_q), dim3(256), 0, st, queries, L.S, scores);
    NANN_HIP_TRY(hipGetLastError());
    int rc = launch_scan_slab_topk(scores, L.S, n_q, fetch, cand_scores, cand_rows, st);
    if (rc) return rc;
    ListsFetchSq8Args f = {};
    f.cand_scores = cand_scores;
    f.cand_rows = cand_rows;
    f.n_in = L.n_slabs * fetch;
    f.fetch = fetch;
    f.queries = queries;
    f.probes = probes;
    f.n_probe = a.n_probe;
    f.n_lists = a.n_lists;
    f.list_splits = a.list_splits;
    f.list_rows = a.list_rows;
    f.n_items = a.n_items;
    f.fpos = reinterpret_cast<int32_t*>(ws + L.off_pos);
    f.fscores = reinterpret_cast<float*>(ws + X.off_fscores);
    f.spos = reinterpret_cast<int32_t*>(ws + X.off_spos);
    f.rows = reinterpret_cast<int32_t*>(ws + X.off_rows);
    f.splits = reinterpret_cast<long long*>(ws + X.off_splits);
    f.out_fetch_pos = out_fetch_pos ? out_fetch_pos + (size_t)c0 * fetch : nullptr;
    f.out_fetch_scores = out_fetch_scores ? out_fetch_scores + (size_t)c0 * fetch : nullptr;
    hipLaunchKernelGGL(k_lists_fetch_sq8, dim3((unsigned)n_q), dim3(kNT), 0, st, f);
    NANN_HIP_TRY(hipGetLastError());
    if (rows_to_score) {  // the exact score of every fetched position, in ascending position order
      ca.n_cand = (long long)n_q * fetch;
      rc = launch_cand_scores(ca, cand_layout(a.kind, n_q, ca.n_cand), qc, n_q, ws + X.off_cand, st);
      if (rc) return rc;
    }
    ListsFinishSq8Args g = {};
    g.exact = reinterpret_cast<const float*>(ws + X.off_cand);  // (CandLayout: the scores first)
    g.spos = f.spos;
    g.rows = f.rows;
    g.fetch = fetch;
    g.k = k;
    g.queries = queries;
    g.item_ids = a.item_ids;
    g.sel = reinterpret_cast<int32_t*>(ws + X.off_sel);
    g.out_item_ids = out_item_ids + (size_t)c0 * k;
    g.out_scores = out_scores ? out_scores + (size_t)c0 * k : nullptr;
    g.out_index = out_index ? out_index + (size_t)c0 * k : nullptr;
    g.out_pos = out_pos ? out_pos + (size_t)c0 * k : nullptr;
    g.n_out = n_out ? n_out + c0 : nullptr;
    g.status = status + c0;
    hipLaunchKernelGGL(k_lists_finish_sq8, dim3((unsigned)n_q), dim3(kNT), 0, st, g);
    NANN_HIP_TRY(hipGetLastError());
  }
  return NANN_OK;
}

}  // namespace nann
