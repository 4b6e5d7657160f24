// nann_filter_inst.hip -- the kernels of filtered retrieval (nann_filter.h) and their launchers.  Also the group cap
// (nann_groupcap.h), a per-query pass over a ranked list of the shape of k_filter_compact, and its launch; and the attribute
// predicates (nann_predicate.h): their scatter, compaction and count.
#define NANN_FILTER_IMPL
#define NANN_GROUPCAP_IMPL
#define NANN_PREDICATE_IMPL
#include "nann_filter.h"
#include "nann_groupcap.h"
#include "nann_predicate.h"

#include <algorithm>

namespace nann {

int launch_filter_scatter(const FilterArgs& f, float* scores, long long q0, int n_q, hipStream_t st) {
  if (n_q <= 0 || f.n_items <= 0) return NANN_OK;
  if (f.deny_bits) {
    const long long words = (f.n_items + 31) / 32;
    const dim3 grid((unsigned)((words + kFilterNT - 1) / kFilterNT), (unsigned)((n_q + kFilterScatterQueries - 1) / kFilterScatterQueries));
    hipLaunchKernelGGL(k_filter_scatter_bits, grid, dim3(kFilterNT), 0, st, f.deny_bits, f.n_items, n_q, scores);
    NANN_HIP_TRY(hipGetLastError());
  }
  if (filter_has_lists(f)) {
    hipLaunchKernelGGL(k_filter_scatter_lists, dim3((unsigned)n_q), dim3(kFilterNT), 0, st, f, q0, scores);
    NANN_HIP_TRY(hipGetLastError());
  }
  return NANN_OK;
}

int launch_filter_compact(const FilterArgs& f, const int32_t* in_rows, const float* in_scores, int in_stride, int n_in,
                          const int32_t* tq, const int32_t* status, long long q0, long long n_q, int k, const int64_t* item_ids,
                          int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* n_out, hipStream_t st) {
  if (n_q <= 0) return NANN_OK;
  if (n_q > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, "too many queries in one call");
  if (k < 0 || in_stride < 0 || in_stride > kMaxK) return fail(NANN_ERR_BAD_ARGUMENT, "filter: a ranked list holds at most 1024 entries");
  hipLaunchKernelGGL(k_filter_compact, dim3((unsigned)n_q), dim3(kFilterNT), 0, st, f, in_rows, in_scores, in_stride, n_in, tq, status,
                     q0, k, item_ids, out_item_ids, out_scores, out_index, n_out);
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

int launch_group_cap(const GroupCapArgs& a, long long n_queries, hipStream_t st) {
  if (n_queries <= 0) return NANN_OK;
  if (n_queries > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, "too many queries in one call");
  if (a.k < 0 || a.k_in < 0 || a.k_in > kMaxK) return fail(NANN_ERR_BAD_ARGUMENT, "group cap: a ranked list holds at most 1024 entries");
  hipLaunchKernelGGL(k_group_cap, dim3((unsigned)n_queries), dim3(kFilterNT), 0, st, a);
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

int launch_pred_scatter(const PredArgs& p, float* scores, long long n_items, long long q0, int n_q, hipStream_t st) {
  if (n_q <= 0 || n_items <= 0 || !pred_any(p)) return NANN_OK;
  const dim3 grid((unsigned)((n_items + kPredTileRows - 1) / kPredTileRows), (unsigned)((n_q + kPredQueries - 1) / kPredQueries));
  hipLaunchKernelGGL(k_pred_scatter, grid, dim3(kFilterNT), 0, st, p, n_items, q0, n_q, scores);
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

int launch_pred_compact(const PredCompactArgs& a, long long n_q, hipStream_t st) {
  if (n_q <= 0) return NANN_OK;
  if (n_q > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, "too many queries in one call");
  if (a.k < 0 || a.in_stride < 0 || a.in_stride > kMaxK) return fail(NANN_ERR_BAD_ARGUMENT, "predicates: a ranked list holds at most 1024 entries");
  hipLaunchKernelGGL(k_pred_compact, dim3((unsigned)n_q), dim3(kFilterNT), 0, st, a);
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

int launch_pred_count(const FilterArgs& f, const PredArgs& p, long long n_queries, long long* counts, hipStream_t st) {
  if (n_queries <= 0) return NANN_OK;
  NANN_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)n_queries * sizeof(long long), st));
  if (f.n_items <= 0) return NANN_OK;
  const unsigned tiles = (unsigned)((f.n_items + kPredTileRows - 1) / kPredTileRows);
  const long long per_launch = 65535ll * kPredQueries;  // (grid.y holds 65535 groups)
  for (long long q0 = 0; q0 < n_queries; q0 += per_launch) {
    const long long n = std::min(per_launch, n_queries - q0);
    hipLaunchKernelGGL(k_pred_count, dim3(tiles, (unsigned)((n + kPredQueries - 1) / kPredQueries)), dim3(kFilterNT), 0, st, f, p, q0,
                       n_queries, reinterpret_cast<unsigned long long*>(counts));
    NANN_HIP_TRY(hipGetLastError());
  }
  return NANN_OK;
}

}  // namespace nann
