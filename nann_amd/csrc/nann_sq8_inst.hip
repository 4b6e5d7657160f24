// nann_sq8_inst.hip -- the kernels of the scalar-quantised exhaustive search (nann_sq8.h): the encoder for every input dtype, the
// int8 MFMA scan for every (d, metric), the row sort; workspace layout and the launch sequence of a chunk's fetch stage; the
// certified form's row-error kernel, query terms and survivor pass (count, k_range_scan, lists, fill); the certified range form's
// lists kernel and ragged selection (count, k_range_scan, k_range_splits, fill).  Rides in
// nann_scan.o behind nann_scan_inst.hip: the slab top-k and the merge it launches are that file's kernels.
#ifndef NANN_SCAN_IMPL
#define NANN_SCAN_IMPL
#endif
#define NANN_SQ8_IMPL
#include "nann_sq8.h"
#include "nann_cand.h"

#include <algorithm>

namespace nann {

namespace {
inline size_t sq8_up256(size_t v) { return (v + 255) & ~(size_t)255; }
}  // namespace

Sq8Layout sq8_layout(const ScanLayout& L, int d, int fetch, size_t cand_bytes) {
  Sq8Layout S = {};
  const size_t c = (size_t)L.chunk, cf = c * (size_t)fetch;
  S.off_qcodes = sq8_up256(L.total);
  S.off_qscales = S.off_qcodes + sq8_up256(c * d);
  S.off_qnorms = S.off_qscales + sq8_up256(c * 4);
  S.off_ids = S.off_qnorms + sq8_up256(c * 4);
  S.off_fscores = S.off_ids + sq8_up256(cf * 8);
  S.off_frows = S.off_fscores + sq8_up256(cf * 4);
  S.off_sorted = S.off_frows + sq8_up256(cf * 4);
  S.off_splits = S.off_sorted + sq8_up256(cf * 4);
  S.off_status = S.off_splits + sq8_up256((c + 1) * 8);
  S.off_cand = S.off_status + sq8_up256(c * 4);
  S.total = S.off_cand + sq8_up256(cand_bytes);
  return S;
}

int launch_sq8_encode(const void* x, int dt, long long n, int d, int8_t* codes, float* scales, int32_t* norms, hipStream_t st) {
  if (n <= 0) return NANN_OK;
  if (!(d == 64 || d == 128 || d == 256 || d == 512)) return fail(NANN_ERR_UNSUPPORTED, "nann_sq8: d must be 64, 128, 256 or 512");
  const unsigned grid = (unsigned)std::min<long long>((n + kSq8NT / 64 - 1) / (kSq8NT / 64), 1 << 16);
  if (dt == NANN_F16) hipLaunchKernelGGL(k_sq8_encode<DT_F16>, dim3(grid), dim3(kSq8NT), 0, st, x, n, d, codes, scales, norms);
  else if (dt == NANN_BF16) hipLaunchKernelGGL(k_sq8_encode<DT_BF16>, dim3(grid), dim3(kSq8NT), 0, st, x, n, d, codes, scales, norms);
  else if (dt == NANN_F32) hipLaunchKernelGGL(k_sq8_encode<DT_F32>, dim3(grid), dim3(kSq8NT), 0, st, x, n, d, codes, scales, norms);
  else return fail(NANN_ERR_BAD_ARGUMENT, "nann_sq8: unknown dtype");
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

template <int NS, int METRIC>
static int launch_scan_sq8_as(const Sq8Args& a, const int8_t* qcodes, const float* qscales, const int32_t* qnorms, int n_q,
                              float* scores, hipStream_t st) {
  auto kern = k_scan_sq8<NS, METRIC>;
  constexpr int lds = sq8_scan_lds(NS * 32);
  static_assert(lds <= 80 * 1024, "two workgroups per CU");
  if (lds > 64 * 1024)  // (only d = 512 is beyond the default limit)
    NANN_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  const long long blocks = (a.n_items + kSq8RowsPerWg - 1) / kSq8RowsPerWg;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kSq8NT), (size_t)lds, st, a.codes, a.scales, a.norms, a.n_items, qcodes,
                     qscales, qnorms, n_q, scores);
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

template <int METRIC>
static int launch_scan_sq8(const Sq8Args& a, const int8_t* qcodes, const float* qscales, const int32_t* qnorms, int n_q,
                           float* scores, hipStream_t st) {
  switch (a.d / 32) {
    case 2: return launch_scan_sq8_as<2, METRIC>(a, qcodes, qscales, qnorms, n_q, scores, st);
    case 4: return launch_scan_sq8_as<4, METRIC>(a, qcodes, qscales, qnorms, n_q, scores, st);
    case 8: return launch_scan_sq8_as<8, METRIC>(a, qcodes, qscales, qnorms, n_q, scores, st);
    case 16: return launch_scan_sq8_as<16, METRIC>(a, qcodes, qscales, qnorms, n_q, scores, st);
    default: return fail(NANN_ERR_UNSUPPORTED, "nann_search_all_sq8: d must be 64, 128, 256 or 512");
  }
}

int launch_sq8_scan(const Sq8Args& a, const float* q, int n_q, int8_t* qcodes, float* qscales, int32_t* qnorms, float* scores,
                    hipStream_t st) {
  const int rc = launch_sq8_encode(q, NANN_F32, n_q, a.d, qcodes, qscales, qnorms, st);
  if (rc) return rc;
  return a.metric == MT_IP ? launch_scan_sq8<MT_IP>(a, qcodes, qscales, qnorms, n_q, scores, st)
                           : launch_scan_sq8<MT_L2>(a, qcodes, qscales, qnorms, n_q, scores, st);
}

int launch_sq8_fetch(const Sq8Args& a, const ScanLayout& L, const Sq8Layout& S, const float* q, int n_q, int fetch,
                     unsigned char* ws, int32_t* out_fetch_index, float* out_fetch_scores, hipStream_t st) {
  if (n_q < 1 || n_q > kScanMaxChunk || fetch < 1 || fetch > kMaxK) return fail(NANN_ERR_BAD_ARGUMENT, "nann_search_all_sq8: chunk shape");
  float* scores = reinterpret_cast<float*>(ws + L.off_scores);
  float* cand_scores = reinterpret_cast<float*>(ws + L.off_cand_scores);
  int32_t* cand_rows = reinterpret_cast<int32_t*>(ws + L.off_cand_rows);
  const int rc = launch_sq8_scan(a, q, n_q, reinterpret_cast<int8_t*>(ws + S.off_qcodes), reinterpret_cast<float*>(ws + S.off_qscales),
                                 reinterpret_cast<int32_t*>(ws + S.off_qnorms), scores, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_scan_slab_topk, dim3((unsigned)((long long)n_q * L.n_slabs)), dim3(kNT), 0, st, scores, a.n_items, L.n_slabs,
                     fetch, cand_scores, cand_rows);
  NANN_HIP_TRY(hipGetLastError());
  int64_t* f_ids = reinterpret_cast<int64_t*>(ws + S.off_ids);
  float* f_scores = reinterpret_cast<float*>(ws + S.off_fscores);
  int32_t* f_rows = reinterpret_cast<int32_t*>(ws + S.off_frows);
  hipLaunchKernelGGL(k_scan_merge, dim3((unsigned)n_q), dim3(kNT), 0, st, cand_scores, cand_rows, L.n_slabs * fetch, fetch, a.item_ids,
                     f_ids, f_scores, f_rows);
  NANN_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_sq8_sort_rows, dim3((unsigned)n_q), dim3(kSq8NT), 0, st, f_rows, f_scores, fetch,
                     reinterpret_cast<int32_t*>(ws + S.off_sorted), reinterpret_cast<long long*>(ws + S.off_splits), out_fetch_index,
                     out_fetch_scores);
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

// ---- the certified form ---------------------------------------------------------------------------------------------------
Sq8ExactLayout sq8_exact_layout(const ScanLayout& L, int kind, int d, int fetch, long long cap, int k, long long n_items) {
  Sq8ExactLayout X = {};
  const size_t c = (size_t)L.chunk;
  X.cap = std::min(cap, n_items);
  X.n_blocks = range_n_blocks(n_items);
  // one CandLayout serves both candidate-list searches of a chunk: the fetch lists (chunk * fetch positions), then the final
  // lists (at most chunk * cap, fetch <= cap)
  X.S = sq8_layout(L, d, fetch, cand_layout(kind, L.chunk, (long long)L.chunk * X.cap).total);
  X.off_qerr = X.S.total;
  X.off_qxhat = X.off_qerr + sq8_up256(c * 4);
  X.off_a_ids = X.off_qxhat + sq8_up256(c * 4);
  X.off_a_scores = X.off_a_ids + sq8_up256(c * (size_t)k * 8);
  X.off_terms = X.off_a_scores + sq8_up256(c * (size_t)k * 4);
  X.off_counts = X.off_terms + sq8_up256(c * sizeof(Sq8QTerms));
  X.off_xsplits = X.off_counts + range_counts_bytes(L.chunk, n_items);
  X.off_rows = X.off_xsplits + sq8_up256((c + 1) * 8);
  X.total = X.off_rows + sq8_up256(c * (size_t)X.cap * 4);
  return X;
}

int launch_sq8_row_err(const void* x, int dt, long long n, int d, const int8_t* codes, const float* scales, const int32_t* norms,
                       float* err, float* xhat, hipStream_t st) {
  if (n <= 0) return NANN_OK;
  if (!(d == 64 || d == 128 || d == 256 || d == 512)) return fail(NANN_ERR_UNSUPPORTED, "nann_sq8_bounds: d must be 64, 128, 256 or 512");
  const unsigned grid = (unsigned)std::min<long long>((n + kSq8NT / 64 - 1) / (kSq8NT / 64), 1 << 16);
  if (dt == NANN_F16) hipLaunchKernelGGL(k_sq8_row_err<DT_F16>, dim3(grid), dim3(kSq8NT), 0, st, x, n, d, codes, scales, norms, err, xhat);
  else if (dt == NANN_BF16) hipLaunchKernelGGL(k_sq8_row_err<DT_BF16>, dim3(grid), dim3(kSq8NT), 0, st, x, n, d, codes, scales, norms, err, xhat);
  else if (dt == NANN_F32) hipLaunchKernelGGL(k_sq8_row_err<DT_F32>, dim3(grid), dim3(kSq8NT), 0, st, x, n, d, codes, scales, norms, err, xhat);
  else return fail(NANN_ERR_BAD_ARGUMENT, "nann_sq8_bounds: unknown dtype");
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

template <int METRIC>
static int launch_sq8_survivors_as(const Sq8Args& a, const ScanLayout& L, const Sq8ExactLayout& X, const float* q, const float* err,
                                   const float* xhat, int n_q, int fetch, int k, unsigned char* ws, int32_t* out_certified,
                                   int32_t* out_n_survivors, hipStream_t st) {
  const float* scores = reinterpret_cast<const float*>(ws + L.off_scores);
  float* qerr = reinterpret_cast<float*>(ws + X.off_qerr);
  float* qxhat = reinterpret_cast<float*>(ws + X.off_qxhat);
  Sq8QTerms* terms = reinterpret_cast<Sq8QTerms*>(ws + X.off_terms);
  int32_t* counts = reinterpret_cast<int32_t*>(ws + X.off_counts);
  int32_t* totals = counts + (size_t)n_q * X.n_blocks;
  long long* xsplits = reinterpret_cast<long long*>(ws + X.off_xsplits);
  int32_t* rows = reinterpret_cast<int32_t*>(ws + X.off_rows);
  const float g = sq8_gamma(a.d);
  // the queries' own error terms, from the codes launch_sq8_fetch has left in the workspace
  int rc = launch_sq8_row_err(q, NANN_F32, n_q, a.d, reinterpret_cast<const int8_t*>(ws + X.S.off_qcodes),
                              reinterpret_cast<const float*>(ws + X.S.off_qscales), reinterpret_cast<const int32_t*>(ws + X.S.off_qnorms),
                              qerr, qxhat, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_sq8_exact_terms<METRIC>, dim3((unsigned)((n_q + kSq8NT - 1) / kSq8NT)), dim3(kSq8NT), 0, st,
                     reinterpret_cast<const float*>(ws + X.off_a_scores), k, qerr, qxhat, n_q, g, terms);
  NANN_HIP_TRY(hipGetLastError());
  const dim3 grid((unsigned)X.n_blocks, (unsigned)n_q);
  hipLaunchKernelGGL(k_sq8_surv_count<METRIC>, grid, dim3(kRangeNT), 0, st, scores, a.n_items, err, xhat, terms, g, counts);
  NANN_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_range_scan, dim3((unsigned)n_q), dim3(kRangeNT), 0, st, counts, X.n_blocks, totals);
  NANN_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_sq8_exact_lists, dim3(1), dim3(kSq8NT), 0, st, totals, terms, n_q, fetch, X.cap,
                     reinterpret_cast<const int32_t*>(ws + X.S.off_sorted), xsplits, rows, out_certified, out_n_survivors);
  NANN_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_sq8_surv_fill<METRIC>, grid, dim3(kRangeNT), 0, st, scores, a.n_items, err, xhat, terms, g, counts, totals,
                     xsplits, X.cap, rows);
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

int launch_sq8_survivors(const Sq8Args& a, const ScanLayout& L, const Sq8ExactLayout& X, const float* q, const float* err,
                         const float* xhat, int n_q, int fetch, int k, unsigned char* ws, int32_t* out_certified,
                         int32_t* out_n_survivors, hipStream_t st) {
  static_assert(kScanMaxChunk <= kSq8NT && kScanMaxChunk <= kRangeNT, "one workgroup walks a chunk's queries");
  if (n_q < 1 || n_q > kScanMaxChunk || k < 1 || k > fetch || X.cap < fetch)
    return fail(NANN_ERR_BAD_ARGUMENT, "nann_search_all_sq8_exact: chunk shape");
  return a.metric == MT_IP
             ? launch_sq8_survivors_as<MT_IP>(a, L, X, q, err, xhat, n_q, fetch, k, ws, out_certified, out_n_survivors, st)
             : launch_sq8_survivors_as<MT_L2>(a, L, X, q, err, xhat, n_q, fetch, k, ws, out_certified, out_n_survivors, st);
}

// ---- the certified range form ---------------------------------------------------------------------------------------------
Sq8RangeLayout sq8_range_layout(const ScanLayout& L, int kind, int d, long long cap, long long n_items) {
  Sq8RangeLayout R = {};
  const size_t c = (size_t)L.chunk;
  R.cap = std::min(cap, n_items);
  R.n_blocks = range_n_blocks(n_items);
  R.n_lblocks = range_n_blocks(R.cap);
  R.off_qcodes = sq8_up256(L.total);
  R.off_qscales = R.off_qcodes + sq8_up256(c * d);
  R.off_qnorms = R.off_qscales + sq8_up256(c * 4);
  R.off_qerr = R.off_qnorms + sq8_up256(c * 4);
  R.off_qxhat = R.off_qerr + sq8_up256(c * 4);
  R.off_terms = R.off_qxhat + sq8_up256(c * 4);
  R.off_counts = R.off_terms + sq8_up256(c * sizeof(Sq8QTerms));
  R.off_xsplits = R.off_counts + range_counts_bytes(L.chunk, n_items);
  R.off_rows = R.off_xsplits + sq8_up256((c + 1) * 8);
  R.off_cand = R.off_rows + sq8_up256(c * (size_t)R.cap * 4);
  R.off_rcounts = R.off_cand + sq8_up256(cand_layout(kind, L.chunk, (long long)L.chunk * R.cap).total);
  R.total = R.off_rcounts + range_counts_bytes(L.chunk, R.cap);
  return R;
}

template <int METRIC>
static int launch_sq8_range_survivors_as(const Sq8Args& a, const ScanLayout& L, const Sq8RangeLayout& R, const float* q, const float* thr,
                                         const float* err, const float* xhat, int n_q, unsigned char* ws, int32_t* out_certified,
                                         int32_t* out_n_survivors, hipStream_t st) {
  float* scores = reinterpret_cast<float*>(ws + L.off_scores);
  int8_t* qcodes = reinterpret_cast<int8_t*>(ws + R.off_qcodes);
  float* qscales = reinterpret_cast<float*>(ws + R.off_qscales);
  int32_t* qnorms = reinterpret_cast<int32_t*>(ws + R.off_qnorms);
  float* qerr = reinterpret_cast<float*>(ws + R.off_qerr);
  float* qxhat = reinterpret_cast<float*>(ws + R.off_qxhat);
  Sq8QTerms* terms = reinterpret_cast<Sq8QTerms*>(ws + R.off_terms);
  int32_t* counts = reinterpret_cast<int32_t*>(ws + R.off_counts);
  int32_t* totals = counts + (size_t)n_q * R.n_blocks;
  long long* xsplits = reinterpret_cast<long long*>(ws + R.off_xsplits);
  int32_t* rows = reinterpret_cast<int32_t*>(ws + R.off_rows);
  const float g = sq8_gamma(a.d);
  int rc = launch_sq8_scan(a, q, n_q, qcodes, qscales, qnorms, scores, st);
  if (rc) return rc;
  rc = launch_sq8_row_err(q, NANN_F32, n_q, a.d, qcodes, qscales, qnorms, qerr, qxhat, st);
  if (rc) return rc;
  // tau = the query's threshold: k_sq8_exact_terms reads a_scores[qi * k + k - 1], the chunk's slice of the thresholds at k = 1
  hipLaunchKernelGGL(k_sq8_exact_terms<METRIC>, dim3((unsigned)((n_q + kSq8NT - 1) / kSq8NT)), dim3(kSq8NT), 0, st, thr, 1, qerr, qxhat,
                     n_q, g, terms);
  NANN_HIP_TRY(hipGetLastError());
  const dim3 grid((unsigned)R.n_blocks, (unsigned)n_q);
  hipLaunchKernelGGL(k_sq8_surv_count<METRIC>, grid, dim3(kRangeNT), 0, st, scores, a.n_items, err, xhat, terms, g, counts);
  NANN_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_range_scan, dim3((unsigned)n_q), dim3(kRangeNT), 0, st, counts, R.n_blocks, totals);
  NANN_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_sq8_range_lists, dim3(1), dim3(kSq8NT), 0, st, totals, terms, n_q, METRIC, R.cap, xsplits, out_certified,
                     out_n_survivors);
  NANN_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_sq8_surv_fill<METRIC>, grid, dim3(kRangeNT), 0, st, scores, a.n_items, err, xhat, terms, g, counts, totals,
                     xsplits, R.cap, rows);
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

int launch_sq8_range_survivors(const Sq8Args& a, const ScanLayout& L, const Sq8RangeLayout& R, const float* q, const float* thr,
                               const float* err, const float* xhat, int n_q, unsigned char* ws, int32_t* out_certified,
                               int32_t* out_n_survivors, hipStream_t st) {
  if (n_q < 1 || n_q > kScanMaxChunk || R.cap < 1) return fail(NANN_ERR_BAD_ARGUMENT, "nann_search_all_range_sq8_exact: chunk shape");
  return a.metric == MT_IP
             ? launch_sq8_range_survivors_as<MT_IP>(a, L, R, q, thr, err, xhat, n_q, ws, out_certified, out_n_survivors, st)
             : launch_sq8_range_survivors_as<MT_L2>(a, L, R, q, thr, err, xhat, n_q, ws, out_certified, out_n_survivors, st);
}

int launch_sq8_range_select(const Sq8Args& a, const Sq8RangeLayout& R, size_t off_scores, const float* thr, long long c0, int n_q,
                            long long capacity, unsigned char* ws, int64_t* row_splits, int64_t* out_item_ids, float* out_scores,
                            int32_t* out_index, hipStream_t st) {
  if (n_q < 1 || n_q > kScanMaxChunk) return fail(NANN_ERR_BAD_ARGUMENT, "nann_search_all_range_sq8_exact: chunk shape");
  const float* scores = reinterpret_cast<const float*>(ws + off_scores);
  const long long* xsplits = reinterpret_cast<const long long*>(ws + R.off_xsplits);
  const int32_t* rows = reinterpret_cast<const int32_t*>(ws + R.off_rows);
  int32_t* counts = reinterpret_cast<int32_t*>(ws + R.off_rcounts);
  int32_t* totals = counts + (size_t)n_q * R.n_lblocks;
  const dim3 grid((unsigned)R.n_lblocks, (unsigned)n_q);
  hipLaunchKernelGGL(k_sq8_range_count, grid, dim3(kRangeNT), 0, st, scores, xsplits, thr, c0, counts);
  NANN_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_range_scan, dim3((unsigned)n_q), dim3(kRangeNT), 0, st, counts, R.n_lblocks, totals);
  NANN_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_range_splits, dim3(1), dim3(kRangeNT), 0, st, totals, n_q, c0, row_splits);
  NANN_HIP_TRY(hipGetLastError());
  if (capacity > 0) {  // (a count-only call: the entry outputs may be null)
    hipLaunchKernelGGL(k_sq8_range_fill, grid, dim3(kRangeNT), 0, st, scores, xsplits, rows, thr, c0, counts, row_splits, capacity,
                       a.item_ids, a.n_items, out_item_ids, out_scores, out_index);
    NANN_HIP_TRY(hipGetLastError());
  }
  return NANN_OK;
}

}  // namespace nann
