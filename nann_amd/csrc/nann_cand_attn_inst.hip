// nann_cand_attn_inst.hip -- the candidate-list search under the attention model (nann_search_candidates_model, nann_cand.h):
// k_cand_score_attn scores every user's own list of rows from the model's pre-projected table T (nann_attn_proj.h: 384
// floats = 1.5 KB per row); the plan before it and the per-user top-k behind it are the candidate-list search's own.
//
// Shape, k_scan_attn (nann_scan_attn_inst.hip) crossed with k_cand_score_mlp (nann_cand.h): one 512-thread workgroup per CU,
// persistent, the LDS of the scan (kScanAttnSplitLds / kScanAttnExactLds, nann_scan.h).  The work items of a launch are those
// of ONE CHUNK of users -- [item_off[c0], item_off[c0 + n_q)), device data -- because only a chunk's kt / upad exist at a time;
// an item resolves to (user qi, block of <= kCandAttnRows list positions) by cand_item's bisection and scores with the keys of
// user qi - c0.
//
// Split-f16 form: what every user shares is placed once per launch (kAttnResShared), an item loads its user's key and
// sequence fragments (72 KB, kAttnResUser) and runs the traversal's per-block body with ids = rows + begin.  f32 form: an item
// is one call of wg_score_attn<128, DT_F16, NT, true, true>.  Both are the calls k_scan_attn makes with a row list in the place
// of the identity: per (user, row) the score has the bits of nann_search_all_model's.  Both clamp a row outside the table to
// row 0 themselves, so the range check here only flags the user.
#include <algorithm>

#include "nann_cand.h"

namespace nann {

namespace {
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
}  // namespace

static_assert(kCandAttnRows % 256 == 0, "eight wavefronts take 32 candidates each");
static_assert(kCandAttnChunk <= 128, "the per-user side of the workspace is bounded by 128 users");

CandAttnLayout cand_attn_layout(long long n_users, long long n_cand) {
  CandAttnLayout L = {};
  L.chunk = (int)std::max<long long>(1, std::min<long long>(n_users, kCandAttnChunk));
  L.off_scores = 0;
  L.off_plan = up256((size_t)n_cand * 4);
  L.off_items = L.off_plan + up256((size_t)n_users * sizeof(CandQuery));
  L.off_user = L.off_items + up256((size_t)(n_users + 1) * 8);
  L.total = L.off_user + up256((size_t)L.chunk * kScanAttnUserBytes);
  return L;
}

// what the scoring kernel takes (by value)
struct CandAttnScoreArgs {
  const float* proj;
  long long n_items;
  const int32_t* rows;
  float* scores;              // f32[n_cand], by list position
  CandQuery* plan;
  const long long* item_off;
  long long n_users;
  const float* kt;            // the chunk's users: [n_q][256][kAttnLP]
  const float* upad;          // [n_q][kAttnLP][kAttnE]
  long long c0;               // first user of the chunk
  int n_q;
};

template <bool EXACT>
__global__ __launch_bounds__(512) void k_cand_score_attn(AttnParams P, CandAttnScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NT = 512;
  uint4* keys = reinterpret_cast<uint4*>(smem);
  float* rest = reinterpret_cast<float*>(smem + 65536);
  const int tid = threadIdx.x;
  if constexpr (!EXACT)  // the launch prologue: what every user shares
    wg_score_attn_res<NT, kAttnResShared>(P, nullptr, nullptr, a.proj, 0, nullptr, 0, keys, rest, nullptr);
  const long long w_end = a.item_off[a.c0 + a.n_q];
  for (long long w = a.item_off[a.c0] + blockIdx.x; w < w_end; w += gridDim.x) {
    const CandItem it = cand_item(a.plan, a.item_off, a.n_users, w, kCandAttnRows);  // (uniform: so is every barrier below)
    const int32_t* ids = a.rows + it.begin;
    bool bad = false;
    for (int j = tid; j < it.count; j += NT) bad |= (uint32_t)ids[j] >= (uint32_t)a.n_items;
    if (bad) atomicOr(&a.plan[it.qi].status, NANN_ERR_INDEX_OUT_OF_RANGE);
    if (a.n_items <= 0) continue;  // (no row 0 for the clamp to land on)
    const size_t u = (size_t)(it.qi - a.c0);  // the user's place in the chunk's kt / upad
    const float* ktu = a.kt + u * 256 * kAttnLP;
    const float* upu = a.upad + u * kAttnLP * kAttnE;
    float* out = a.scores + it.begin;
    // (both forms open with a barrier -- every wavefront has left the item before -- and close with one)
    if constexpr (EXACT)
      wg_score_attn<128, DT_F16, NT, true, true>(P, ktu, upu, a.proj, a.n_items, ids, it.count, rest, out, reinterpret_cast<float*>(keys));
    else
      wg_score_attn_res<NT, kAttnResUser>(P, reinterpret_cast<const uint4*>(ktu), reinterpret_cast<const uint4*>(upu), a.proj,
                                          a.n_items, ids, it.count, keys, rest, out);
  }
}

template <bool EXACT>
static int launch_cand_score_attn(const AttnParams& P, const CandAttnScoreArgs& s, unsigned grid, hipStream_t st) {
  auto kern = k_cand_score_attn<EXACT>;
  constexpr int lds = EXACT ? kScanAttnExactLds : kScanAttnSplitLds;
  NANN_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), (size_t)lds, st, P, s);
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

int launch_cand_attn(const CandAttnArgs& a, const CandAttnLayout& L, const void* comm_seq_f16, long long n_users, int k,
                     unsigned char* ws, int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* out_pos,
                     int32_t* n_out, int32_t* status, hipStream_t st) {
  CandAttnScoreArgs s = {};
  s.proj = a.proj;
  s.n_items = a.n_items;
  s.rows = a.rows;
  s.scores = reinterpret_cast<float*>(ws + L.off_scores);
  s.plan = reinterpret_cast<CandQuery*>(ws + L.off_plan);
  s.item_off = reinterpret_cast<const long long*>(ws + L.off_items);
  s.n_users = n_users;
  int rc = launch_cand_plan(a.row_splits, n_users, a.n_cand, kCandAttnRows, s.plan, reinterpret_cast<long long*>(ws + L.off_items), st);
  if (rc) return rc;
  // one buffer of kt / upad serves every chunk: stream order puts a chunk's prepare behind the scoring of the chunk before
  for (long long c0 = 0; a.n_cand > 0 && c0 < n_users; c0 += L.chunk) {
    const int n_q = (int)std::min<long long>(L.chunk, n_users - c0);
    const uint16_t* seq = static_cast<const uint16_t*>(comm_seq_f16) + (size_t)c0 * a.attn.L * kAttnE;
    float* kt = reinterpret_cast<float*>(ws + L.off_user);
    float* upad = kt + (size_t)n_q * 256 * kAttnLP;
    rc = a.exact ? launch_attn_prepare(st, a.attn, seq, n_q, kt, upad) : launch_attn_prepare_split(st, a.attn, seq, n_q, kt, upad);
    if (rc) return rc;
    s.kt = kt;
    s.upad = upad;
    s.c0 = c0;
    s.n_q = n_q;
    // at most the work items the chunk's lengths can add up to: n_cand / R whole blocks and one ragged block per user
    const long long most = a.n_cand / kCandAttnRows + std::min<long long>(n_q, a.n_cand);
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>(most, std::max(1, a.cus)));
    rc = a.exact ? launch_cand_score_attn<true>(a.attn, s, grid, st) : launch_cand_score_attn<false>(a.attn, s, grid, st);
    if (rc) return rc;
  }
  return launch_cand_topk(s.plan, a.rows, s.scores, n_users, k, a.item_ids, out_item_ids, out_scores, out_index, out_pos, n_out,
                          status, st);
}

}  // namespace nann
