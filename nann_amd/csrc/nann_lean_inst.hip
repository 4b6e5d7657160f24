// nann_lean_inst.hip -- the lean instantiations of the fused traversal (k_search_lean, nann_search.h) for ONE flat scorer and
// ONE row dtype (-DNANN_LEAN_SC=0 L2 | 12 inner product, -DNANN_LEAN_DT=0 f16 | 1 bf16 | 2 f32,
// -DNANN_LEAN_NAME=l2_f16|...|ip_f32): the two hash-set plans only.  A unit may include the file several times; the six ride in
// the light objects (nann_amd/build.py), not in the ones that bound a build from scratch.
#include "nann_search.h"

#if !defined(NANN_LEAN_SC) || !defined(NANN_LEAN_DT) || !defined(NANN_LEAN_NAME)
#error "compile with -DNANN_LEAN_SC=<0|12> -DNANN_LEAN_DT=<0|1|2> -DNANN_LEAN_NAME=<l2|ip>_<f16|bf16|f32>"
#endif
#define NANN_LEAN_CAT2(a, b) a##b
#define NANN_LEAN_CAT(a, b) NANN_LEAN_CAT2(a, b)

namespace nann {

#define NANN_LAUNCH_LEAN NANN_LEAN_CAT(launch_lean_as_, NANN_LEAN_NAME)
template <int LPR>
static int NANN_LAUNCH_LEAN(int vis, int nt, int slots, size_t lds_bytes, const SearchArgs& a, hipStream_t st) {
  if (vis == VIS_LDS_HASH && nt == 512)  // two queries per CU
    return launch_search_lean_as<LPR, NANN_LEAN_DT, VIS_LDS_HASH, NANN_LEAN_SC, 512>(slots, lds_bytes, a, st);
  if (vis == VIS_LDS_HASH32 && nt == kNT)  // wide beams: one query per CU, 32K-slot set
    return launch_search_lean_as<LPR, NANN_LEAN_DT, VIS_LDS_HASH32, NANN_LEAN_SC, kNT>(slots, lds_bytes, a, st);
  return fail(NANN_ERR_UNSUPPORTED, "lean traversal: no kernel for this plan");
}

int NANN_LEAN_CAT(launch_search_lean_, NANN_LEAN_NAME)(int lpr, int vis, int nt, int slots, size_t lds_bytes,
                                                       const SearchArgs& a, hipStream_t st) {
  if (!lean_eligible(vis, a)) return fail(NANN_ERR_UNSUPPORTED, "lean traversal: this launch needs the general kernel");
  switch (lpr) {
    case 8: return NANN_LAUNCH_LEAN<8>(vis, nt, slots, lds_bytes, a, st);
    case 16: return NANN_LAUNCH_LEAN<16>(vis, nt, slots, lds_bytes, a, st);
    case 32: return NANN_LAUNCH_LEAN<32>(vis, nt, slots, lds_bytes, a, st);
    default: return NANN_LAUNCH_LEAN<64>(vis, nt, slots, lds_bytes, a, st);
  }
}

#undef NANN_LAUNCH_LEAN

}  // namespace nann
