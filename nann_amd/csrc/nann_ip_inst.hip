// nann_ip_inst.hip -- inner-product (NANN_SCORER_IP) instantiations of the fused traversal for ONE row dtype
// (-DNANN_IP_DT=0 f16 | 1 bf16 | 2 f32, -DNANN_IP_NAME=f16|bf16|f32): the four plans of nann_l2_inst.hip with kScorerIp.  The
// three dtypes ride in three light objects (nann_amd/build.py), not in the nann_l2_* objects that bound a build from scratch.
#include "nann_search.h"

#if !defined(NANN_IP_DT) || !defined(NANN_IP_NAME)
#error "compile with -DNANN_IP_DT=<0|1|2> -DNANN_IP_NAME=<f16|bf16|f32>"
#endif
#define NANN_IP_CAT2(a, b) a##b
#define NANN_IP_CAT(a, b) NANN_IP_CAT2(a, b)

namespace nann {

#define NANN_LAUNCH_IP NANN_IP_CAT(launch_ip_as_, NANN_IP_NAME)
template <int LPR>
static int NANN_LAUNCH_IP(int vis, int nt, int slots, size_t lds_bytes, const SearchArgs& a, hipStream_t st) {
  if (vis == VIS_LDS_HASH && nt == 512)  // two queries per CU
    return launch_search_as<LPR, NANN_IP_DT, VIS_LDS_HASH, kScorerIp, 512>(slots, lds_bytes, a, st);
  if (vis == VIS_LDS_HASH32 && nt == kNT)  // wide beams: one query per CU, 32K-slot set
    return launch_search_as<LPR, NANN_IP_DT, VIS_LDS_HASH32, kScorerIp, kNT>(slots, lds_bytes, a, st);
  if ((vis == VIS_LDS_BITMAP || vis == VIS_HBM_BITMAP) && nt == kNT)
    return launch_search_bitmap<LPR, NANN_IP_DT, kScorerIp, kNT>(vis, slots, lds_bytes, a, st);
  return fail(NANN_ERR_UNSUPPORTED, "inner-product traversal: no kernel for this plan");
}

int NANN_IP_CAT(launch_search_ip_, NANN_IP_NAME)(int lpr, int vis, int nt, int slots, size_t lds_bytes,
                                                 const SearchArgs& a, hipStream_t st) {
  switch (lpr) {
    case 8: return NANN_LAUNCH_IP<8>(vis, nt, slots, lds_bytes, a, st);
    case 16: return NANN_LAUNCH_IP<16>(vis, nt, slots, lds_bytes, a, st);
    case 32: return NANN_LAUNCH_IP<32>(vis, nt, slots, lds_bytes, a, st);
    default: return NANN_LAUNCH_IP<64>(vis, nt, slots, lds_bytes, a, st);
  }
}

#undef NANN_LAUNCH_IP

}  // namespace nann
