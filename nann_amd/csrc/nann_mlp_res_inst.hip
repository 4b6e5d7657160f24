// nann_mlp_res_inst.hip -- the traversal with the MLP scorer's layer 2 resident in LDS (nann_mlp5.h): split-f16 and
// exact f32, on the 16K-slot hash-set plan and on the HBM-bitmap plan (wide beams, large shards, and the rerun of
// queries the set handed back).  An object of its own so that the four kernels compile next to the others.
#include <cstddef>

#include "nann_search.h"

namespace nann {

int launch_search_mlp_res(int exact, int vis, int slots, size_t lds_bytes, const SearchArgs& a, hipStream_t st) {
  // the scorers never read the embedding table: one instance per (precision, plan) serves every d and row dtype
  if (vis == VIS_LDS_HASH) {
    if (exact) return launch_search_as<16, DT_F16, VIS_LDS_HASH, kScorerMlpXRes, 512>(slots, lds_bytes, a, st);
    return launch_search_as<16, DT_F16, VIS_LDS_HASH, kScorerMlpRes, 512>(slots, lds_bytes, a, st);
  }
  if (vis != VIS_HBM_BITMAP) return fail(NANN_ERR_UNSUPPORTED, "MLP traversal with resident layer 2: hash-set or HBM-bitmap plan");
  if (exact) return launch_search_as<16, DT_F16, VIS_HBM_BITMAP, kScorerMlpXRes, 512>(slots, lds_bytes, a, st);
  return launch_search_as<16, DT_F16, VIS_HBM_BITMAP, kScorerMlpRes, 512>(slots, lds_bytes, a, st);
}

int launch_search_mlp_phase(int vis, int slots, size_t lds_bytes, const SearchArgs& a, hipStream_t st) {
  // the traversal stages read no embedding row and score nothing: one instance per set size (16K slots: two 512-thread
  // workgroups per CU; 32K slots, wide beams: one of 1024)
  if (vis == VIS_LDS_HASH32) return launch_search_as<16, DT_F16, VIS_LDS_HASH32, kScorerMlpPhase, kNT>(slots, lds_bytes, a, st);
  return launch_search_as<16, DT_F16, VIS_LDS_HASH, kScorerMlpPhase, 512>(slots, lds_bytes, a, st);
}

// The arguments of a round's scoring launches (the certified fields: launch_mlp_phase_certified); off = the slot layout.
static PhaseScoreArgs phase_score_args(const SearchArgs& a, int round, unsigned long long (&off)[9]) {
  slot_layout(a.max_cand, a.max_raw, a.pool_cap, 0u, off);  // (offsets do not depend on the last region's size)
  PhaseScoreArgs p = {};
  p.ws = a.ws; p.slot_bytes = a.slot_bytes;
  p.off_cand_ids = off[0]; p.off_cand_scores = off[1]; p.off_state = off[8];
  p.enter = a.enter; p.proj = a.proj; p.n_items = a.n_items; p.n_queries = a.n_queries;
  p.round = round; p.mlp = a.mlp;
  return p;
}

template <class Kernel>
static int launch_phase_score(Kernel kern, const PhaseScoreArgs& p, int workgroups, hipStream_t st) {
  NANN_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPhaseScoreLds));
  hipLaunchKernelGGL(kern, dim3((unsigned)workgroups), dim3(512), kPhaseScoreLds, st, p);
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

int launch_mlp_phase_score(int exact, const SearchArgs& a, int round, int workgroups, hipStream_t st) {
  if (a.n_queries > kPhaseChunk) return fail(NANN_ERR_BAD_ARGUMENT, "phased MLP traversal: chunks of at most 1024 queries");
  unsigned long long off[9];
  const PhaseScoreArgs p = phase_score_args(a, round, off);
  return exact ? launch_phase_score(k_mlp_phase_score<true>, p, workgroups, st)
               : launch_phase_score(k_mlp_phase_score<false>, p, workgroups, st);
}

int launch_mlp_phase_certified(const SearchArgs& a, int round, int workgroups, hipStream_t st) {
  if (a.n_queries > kPhaseChunk) return fail(NANN_ERR_BAD_ARGUMENT, "phased MLP traversal: chunks of at most 1024 queries");
  unsigned long long off[9];
  PhaseScoreArgs p = phase_score_args(a, round, off);
  p.off_raw = off[2]; p.max_raw = a.max_raw; p.t_r = a.t[round]; p.tq = a.tq;
  p.refined = reinterpret_cast<unsigned long long*>(a.ws + offsetof(WsHeader, refined));
  const int rc = launch_phase_score(k_mlp_phase_score<false, 2>, p, workgroups, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_mlp_phase_certify<kCertNT>, dim3((unsigned)a.n_queries), dim3(kCertNT), 0, st, p);
  NANN_HIP_TRY(hipGetLastError());
  return launch_phase_score(k_mlp_phase_score<true, 1>, p, workgroups, st);
}

}  // namespace nann
