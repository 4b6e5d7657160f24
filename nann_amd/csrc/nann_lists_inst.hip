// nann_lists_inst.hip -- the kernels of the shared-list search (nann_lists.h): the partition build, the plan of a chunk, the tiles'
// transposed queries, the L2 and inner-product list scans for every (d, row dtype), the pad and the finish; workspace layout and
// the launch sequence of a call.  Rides in nann_scan.o behind nann_scan_inst.hip: the scans are ScanL2's (nann_scan.h).
#define NANN_SCAN_IMPL
#define NANN_LISTS_IMPL
#include "nann_lists.h"

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

}  // namespace nann
