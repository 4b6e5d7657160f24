// nann_cand_inst.hip -- the kernels of the candidate-list search (nann_cand.h): the plan, the L2 and inner-product scorers for every (d, row
// dtype), the MLP scorer in both precisions and the per-query top-k; workspace layout and the launch sequence of a call.  Also
// the union top-k (nann_union.h), a per-user selection over wg_topk like k_cand_topk, and its launch; and the MMR re-ranking
// (nann_mmr.h), a per-query selection over the L2 / inner-product scorer for the (d, row dtype) set of k_cand_score_l2, and its launch.
// And the fused top-k (nann_fuse.h), the union's sibling with an accumulator per row, and its launch.  And the user side of the
// multi-vector calls (nann_interests.h): the kernel that clusters a behaviour sequence into interest vectors, with its entry point.
#define NANN_CAND_IMPL
#define NANN_UNION_IMPL
#define NANN_MMR_IMPL
#define NANN_FUSE_IMPL
#define NANN_INTERESTS_IMPL
#include "nann_cand.h"
#include "nann_union.h"
#include "nann_mmr.h"
#include "nann_fuse.h"
#include "nann_interests.h"

#include <algorithm>

namespace nann {

namespace {
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
}  // namespace

CandLayout cand_layout(int kind, long long n_queries, long long n_cand) {
  CandLayout L = {};
  L.off_scores = 0;
  L.off_plan = up256((size_t)n_cand * 4);
  L.off_items = L.off_plan + up256((size_t)n_queries * sizeof(CandQuery));
  L.off_u = L.off_items + up256((size_t)(n_queries + 1) * 8);
  L.total = L.off_u + (kind == NANN_SCORER_MLP ? up256((size_t)n_queries * 256 * 4) : 0);
  return L;
}

// the persistent grid of a scoring kernel: at most the work items the lengths can add up to, n_cand / C whole blocks and one
// ragged block per query
static unsigned cand_grid(long long n_queries, long long n_cand, int rows_per_item, int resident) {
  const long long most = n_cand / rows_per_item + std::min(n_queries, n_cand);
  return (unsigned)std::max<long long>(1, std::min<long long>(most, resident));
}

template <int LPR>
static void launch_cand_l2(const CandArgs& a, const CandScoreArgs& s, unsigned grid, hipStream_t st) {
  if (a.dt == NANN_F16) hipLaunchKernelGGL((k_cand_score_l2<LPR, DT_F16>), dim3(grid), dim3(kCandNT), 0, st, s);
  else if (a.dt == NANN_BF16) hipLaunchKernelGGL((k_cand_score_l2<LPR, DT_BF16>), dim3(grid), dim3(kCandNT), 0, st, s);
  else hipLaunchKernelGGL((k_cand_score_l2<LPR, DT_F32>), dim3(grid), dim3(kCandNT), 0, st, s);
}

template <int LPR>
static void launch_cand_ip(const CandArgs& a, const CandScoreArgs& s, unsigned grid, hipStream_t st) {
  if (a.dt == NANN_F16) hipLaunchKernelGGL((k_cand_score_ip<LPR, DT_F16>), dim3(grid), dim3(kCandNT), 0, st, s);
  else if (a.dt == NANN_BF16) hipLaunchKernelGGL((k_cand_score_ip<LPR, DT_BF16>), dim3(grid), dim3(kCandNT), 0, st, s);
  else hipLaunchKernelGGL((k_cand_score_ip<LPR, DT_F32>), dim3(grid), dim3(kCandNT), 0, st, s);
}

template <bool EXACT>
static int launch_cand_mlp(const CandArgs& a, const CandScoreArgs& s, unsigned grid, hipStream_t st) {
  auto kern = k_cand_score_mlp<EXACT>;
  NANN_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kMlpResBytes));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), (size_t)kMlpResBytes, st, a.mlp, s);
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

int launch_cand_plan(const int64_t* row_splits, long long n_queries, long long n_cand, int rows_per_item, CandQuery* plan,
                     long long* item_off, hipStream_t st) {
  hipLaunchKernelGGL(k_cand_plan, dim3(1), dim3(kCandNT), 0, st, row_splits, n_queries, n_cand, rows_per_item, plan, item_off);
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

int launch_cand_topk(const CandQuery* plan, const int32_t* rows, const float* scores, long long n_queries, int k,
                     const int64_t* item_ids, int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* out_pos,
                     int32_t* n_out, int32_t* status, hipStream_t st) {
  hipLaunchKernelGGL(k_cand_topk, dim3((unsigned)n_queries), dim3(kNT), 0, st, plan, rows, scores, k, item_ids, out_item_ids,
                     out_scores, out_index, out_pos, n_out, status);
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

int launch_cand_scores(const CandArgs& a, const CandLayout& L, const float* q, long long n_queries, unsigned char* ws, hipStream_t st) {
  if (a.kind != NANN_SCORER_L2 && a.kind != NANN_SCORER_MLP && a.kind != NANN_SCORER_IP)
    return fail(NANN_ERR_BAD_ARGUMENT, "nann_search_candidates: unknown scorer kind");
  const bool mlp = a.kind == NANN_SCORER_MLP, ip = a.kind == NANN_SCORER_IP;
  const int rows_per_item = mlp ? kCandMlpRows : kCandRows;
  CandScoreArgs s = {};
  s.emb = a.emb;
  s.proj = a.proj;
  s.n_items = a.n_items;
  s.d = a.d;
  s.rows = a.rows;
  s.q = q;
  s.u = reinterpret_cast<const float*>(ws + L.off_u);
  s.scores = reinterpret_cast<float*>(ws + L.off_scores);
  s.plan = reinterpret_cast<CandQuery*>(ws + L.off_plan);
  s.item_off = reinterpret_cast<const long long*>(ws + L.off_items);
  s.n_queries = n_queries;
  int rc = launch_cand_plan(a.row_splits, n_queries, a.n_cand, rows_per_item, s.plan, reinterpret_cast<long long*>(ws + L.off_items), st);
  if (rc) return rc;
  if (a.n_cand > 0 && mlp) {
    hipLaunchKernelGGL(k_cand_mlp_u, dim3((unsigned)n_queries), dim3(256), 0, st, a.mlp, q, reinterpret_cast<float*>(ws + L.off_u));
    NANN_HIP_TRY(hipGetLastError());
    const unsigned grid = cand_grid(n_queries, a.n_cand, rows_per_item, std::max(1, a.cus));
    rc = a.exact ? launch_cand_mlp<true>(a, s, grid, st) : launch_cand_mlp<false>(a, s, grid, st);
    if (rc) return rc;
  } else if (a.n_cand > 0) {
    const unsigned grid = cand_grid(n_queries, a.n_cand, rows_per_item, std::max(1, a.cus) * 8);
    switch (a.d / 8) {
      case 8: ip ? launch_cand_ip<8>(a, s, grid, st) : launch_cand_l2<8>(a, s, grid, st); break;
      case 16: ip ? launch_cand_ip<16>(a, s, grid, st) : launch_cand_l2<16>(a, s, grid, st); break;
      case 32: ip ? launch_cand_ip<32>(a, s, grid, st) : launch_cand_l2<32>(a, s, grid, st); break;
      case 64: ip ? launch_cand_ip<64>(a, s, grid, st) : launch_cand_l2<64>(a, s, grid, st); break;
      default: return fail(NANN_ERR_UNSUPPORTED, "nann_search_candidates: d must be 64, 128, 256 or 512");
    }
    NANN_HIP_TRY(hipGetLastError());
  }
  return NANN_OK;
}

int launch_cand(const CandArgs& a, const CandLayout& L, const float* q, long long n_queries, int k, unsigned char* ws,
                int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* out_pos, int32_t* n_out, int32_t* status,
                hipStream_t st) {
  const int rc = launch_cand_scores(a, L, q, n_queries, ws, st);
  if (rc) return rc;
  return launch_cand_topk(reinterpret_cast<const CandQuery*>(ws + L.off_plan), a.rows, reinterpret_cast<const float*>(ws + L.off_scores),
                          n_queries, k, a.item_ids, out_item_ids, out_scores, out_index, out_pos, n_out, status, st);
}

// ---- the union top-k (nann_union.h) -----------------------------------------------------------------------------------
size_t union_ws_bytes(long long n_users, long long n_in) { return up256((size_t)n_users * (size_t)n_in * 8); }

int launch_union_topk(const UnionArgs& a, long long n_users, hipStream_t st) {
  const int n_in = a.n_lists * a.k_in;
  if (n_users <= 0) return NANN_OK;
  const size_t lds = union_lds_bytes(n_in);
  if (lds > 64 * 1024)  // (only the sizes beyond the default limit need the opt-in: n_in > 4096)
    NANN_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_union_topk), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)union_lds_bytes(NANN_UNION_MAX_IN)));
  hipLaunchKernelGGL(k_union_topk, dim3((unsigned)n_users), dim3(kNT), lds, st, a, union_slots_log2(n_in));
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

// ---- the fused top-k (nann_fuse.h) --------------------------------------------------------------------------------------
size_t fuse_ws_bytes(long long n_users, long long n_in) { return up256((size_t)n_users * (size_t)n_in * kFuseEntryBytes); }

int launch_fuse_topk(const FuseArgs& a, long long n_users, hipStream_t st) {
  const int n_in = a.n_lists * a.k_in;
  if (n_users <= 0) return NANN_OK;
  const size_t lds = fuse_lds_bytes(n_in);
  if (lds > 64 * 1024)  // (only the sizes beyond the default limit need the opt-in: n_in > 4096)
    NANN_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_fuse_topk), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)fuse_lds_bytes(NANN_UNION_MAX_IN)));
  hipLaunchKernelGGL(k_fuse_topk, dim3((unsigned)n_users), dim3(kNT), lds, st, a, union_slots_log2(n_in));
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

// ---- the MMR re-ranking (nann_mmr.h) ----------------------------------------------------------------------------------
template <int LPR, int DT>
static int launch_mmr_as(const MmrArgs& a, unsigned grid, size_t lds, hipStream_t st) {
  auto run = [&](auto kern) -> int {
    if (lds > 48 * 1024)
      NANN_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kMmrNT), lds, st, a);
    NANN_HIP_TRY(hipGetLastError());
    return NANN_OK;
  };
  return a.metric == MT_IP ? run(k_mmr<LPR, DT, MT_IP>) : run(k_mmr<LPR, DT, MT_L2>);
}

template <int LPR>
static int launch_mmr_dt(const MmrArgs& a, unsigned grid, size_t lds, hipStream_t st) {
  if (a.dt == NANN_F16) return launch_mmr_as<LPR, DT_F16>(a, grid, lds, st);
  if (a.dt == NANN_BF16) return launch_mmr_as<LPR, DT_BF16>(a, grid, lds, st);
  if (a.dt == NANN_F32) return launch_mmr_as<LPR, DT_F32>(a, grid, lds, st);
  return fail(NANN_ERR_UNSUPPORTED, "mmr: rows must be f16, bf16 or f32");
}

int launch_mmr(const MmrArgs& a0, long long n_queries, hipStream_t st) {
  if (n_queries <= 0 || a0.k == 0) return NANN_OK;
  if (n_queries > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, "too many queries in one call");
  if (a0.k < 0 || a0.k_in < 0 || a0.k_in > kMaxK) return fail(NANN_ERR_BAD_ARGUMENT, "mmr: a list holds at most 1024 entries");
  if (a0.metric != MT_L2 && a0.metric != MT_IP) return fail(NANN_ERR_BAD_ARGUMENT, "mmr: the similarity is L2 or the inner product");
  MmrArgs a = a0;
  const int row_bytes = a.d * (a.dt == NANN_F32 ? 4 : 2);
  a.lds_rows = mmr_rows_in_lds(a.k_in, row_bytes) ? 1 : 0;
  const size_t lds = (size_t)kMmrStateBytes + (a.lds_rows ? (size_t)a.k_in * (size_t)(row_bytes + kMmrRowPad) : 0);
  const unsigned grid = (unsigned)n_queries;
  switch (a.d) {
    case 64: return launch_mmr_dt<8>(a, grid, lds, st);
    case 128: return launch_mmr_dt<16>(a, grid, lds, st);
    case 256: return launch_mmr_dt<32>(a, grid, lds, st);
    case 512: return launch_mmr_dt<64>(a, grid, lds, st);
    default: return fail(NANN_ERR_UNSUPPORTED, "mmr: d must be 64, 128, 256 or 512");
  }
}

}  // namespace nann
