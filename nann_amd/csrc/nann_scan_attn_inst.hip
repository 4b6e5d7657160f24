// nann_scan_attn_inst.hip -- the exhaustive search under the attention model (nann_search_all_model): k_scan_attn scores
// every row of the model's pre-projected table T (nann_attn_proj.h: 384 floats = 1.5 KB per row) for a chunk of users;
// the slab top-k and the merge of nann_scan.h follow unchanged.
//
// Shape, as k_scan_mlp: one 512-thread workgroup per CU, persistent; work items = (block of kScanAttnRows rows, user), THE
// USER FASTEST.  T is 1.5 GB per million rows, six times the 256 MiB Infinity Cache: a pass over it per user would come
// from HBM.  With the user fastest the workgroups that run together score the same block (6 MB at 4096 rows) for different
// users, and the block is fetched from HBM once per chunk of users.
//
// Split-f16 form.  LDS = [keys 64 KB | W2 32 KB | vectors 6 KB | sequence 8 KB, W1a 32 KB, W3 8 KB] = 150 KB of the CU's
// 160: one workgroup per CU, two wavefronts per SIMD.  What every user shares (W2, W1a, W3, the vectors: 78 KB) is placed
// once per launch (wg_score_attn_res<.., kAttnResShared>); an item loads its user's key and sequence fragments only
// (72 KB, kAttnResUser) and then runs the traversal's own per-block body -- per (user, row) the scan's score has the bits
// of the hash-set traversal's.  There is no room for a second key buffer: an item's key load is exposed behind one barrier,
// 72 KB from L2 against ~4096 x 220 / 32 MFMAs of arithmetic.
//
// f32 form (precision "exact"): an item is one call of wg_score_attn<128, DT_F16, NT, true, true> as the traversal makes it
// -- it reloads its 152 KB per item; the parity form, the slower one by design.
#include <algorithm>

#include "nann_scan.h"

namespace nann {

constexpr int kScanAttnRows = 4096;  // rows of a work item (the LDS sizes: kScanAttnSplitLds / kScanAttnExactLds, nann_scan.h)

template <bool EXACT>
__global__ __launch_bounds__(512) void k_scan_attn(AttnParams P, const float* __restrict__ proj, long long n_items,
                                                   const float* __restrict__ kt, const float* __restrict__ upad, int n_q,
                                                   float* __restrict__ scores) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NT = 512;
  uint4* keys = reinterpret_cast<uint4*>(smem);
  float* rest = reinterpret_cast<float*>(smem + 65536);
  if constexpr (!EXACT)  // the launch prologue: what every user shares
    wg_score_attn_res<NT, kAttnResShared>(P, nullptr, nullptr, proj, 0, nullptr, 0, keys, rest, nullptr);
  const long long n_blocks = (n_items + kScanAttnRows - 1) / kScanAttnRows;
  const long long n_work = n_blocks * n_q;
  for (long long w = blockIdx.x; w < n_work; w += gridDim.x) {
    const int qi = (int)(w % n_q);
    const long long r0 = (w / n_q) * kScanAttnRows;
    const long long n = min((long long)kScanAttnRows, n_items - r0);
    const float* T = proj + (size_t)r0 * kAttnProjWidth;
    const float* ktu = kt + (size_t)qi * 256 * kAttnLP;
    const float* upu = upad + (size_t)qi * kAttnLP * kAttnE;
    float* out = scores + (size_t)qi * n_items + r0;
    // (both forms open with a barrier -- every wavefront has left the item before -- and close with one)
    if constexpr (EXACT)
      wg_score_attn<128, DT_F16, NT, true, true>(P, ktu, upu, T, n, nullptr, n, rest, out, reinterpret_cast<float*>(keys));
    else
      wg_score_attn_res<NT, kAttnResUser>(P, reinterpret_cast<const uint4*>(ktu), reinterpret_cast<const uint4*>(upu), T, n,
                                          nullptr, n, keys, rest, out);
  }
}

template <bool EXACT>
static int launch_scan_attn_as(const ScanArgs& a, const float* kt, const float* upad, int n_q, float* scores, hipStream_t st) {
  auto kern = k_scan_attn<EXACT>;
  constexpr int lds = EXACT ? kScanAttnExactLds : kScanAttnSplitLds;
  NANN_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  const long long n_work = (a.n_items + kScanAttnRows - 1) / kScanAttnRows * n_q;
  const unsigned grid = (unsigned)std::min<long long>(n_work, std::max(1, a.mlp_workgroups));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), (size_t)lds, st, a.attn, a.proj, a.n_items, kt, upad, n_q, scores);
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

int launch_scan_attn(const ScanArgs& a, const float* kt, const float* upad, int n_q, float* scores, hipStream_t st) {
  return a.exact ? launch_scan_attn_as<true>(a, kt, upad, n_q, scores, st) : launch_scan_attn_as<false>(a, kt, upad, n_q, scores, st);
}

}  // namespace nann
