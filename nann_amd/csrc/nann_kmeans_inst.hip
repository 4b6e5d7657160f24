// nann_kmeans_inst.hip -- the kernels of the coarse quantiser (nann_kmeans.h): the prepare and assign kernels for every
// (d, row dtype), the update and the inertia; workspace layouts and the launch sequences of nann_kmeans_assign and
// nann_kmeans_train.  The CSR of a round is built by the partition build's launchers (nann_lists.h).
#define NANN_KMEANS_IMPL
#include "nann_kmeans.h"
#include "nann_lists.h"

#include <algorithm>

namespace nann {

KmeansLayout kmeans_layout(int d, int dt, int n_lists) {
  KmeansLayout L = {};
  L.n_tiles = (n_lists + kKmeansTile - 1) / kKmeansTile;
  L.off_ops = 0;
  L.off_c2 = kmeans_up256((size_t)L.n_tiles * (d / 16) * kmeans_terms(dt) * 1024);
  L.total = L.off_c2 + kmeans_up256((size_t)L.n_tiles * kKmeansTile * 4);
  return L;
}

static int kmeans_inertia_blocks(long long n) {
  return (int)std::max<long long>(1, std::min<long long>(kKmeansInertiaBlocks, (n + 4095) / 4096));
}

KmeansTrainLayout kmeans_train_layout(long long n_items, int d, int dt, int n_lists) {
  KmeansTrainLayout L = {};
  L.A = kmeans_layout(d, dt, n_lists);
  L.groups = (int)lists_build_groups(n_items, n_lists);
  L.max_segs = n_items / kKmeansSeg + n_lists;  // a list of len rows: ceil(len / seg) <= len / seg + 1 segments
  L.off_dist = L.A.total;
  L.off_splits = L.off_dist + kmeans_up256((size_t)n_items * 4);
  L.off_rows = L.off_splits + kmeans_up256(((size_t)n_lists + 1) * 8);
  L.off_counts = L.off_rows + kmeans_up256((size_t)n_items * 4);
  L.off_info = L.off_counts + kmeans_up256((size_t)L.groups * n_lists * 4);  // (the two are cleared as one range)
  L.off_seg = L.off_info + kmeans_up256(32);
  L.off_partial = L.off_seg + kmeans_up256(((size_t)n_lists + 1) * 8);
  L.off_inertia = L.off_partial + kmeans_up256((size_t)L.max_segs * d * 4);
  L.total = L.off_inertia + kmeans_up256((size_t)kKmeansInertiaBlocks * 8);
  return L;
}

template <int D, int RT>
static void launch_kmeans_assign_d(int dt, const void* emb, long long row_begin, long long n_rows, const uint4* ops, const float* c2,
                                   int n_tiles, int32_t* out_list, float* out_dist, hipStream_t st) {
  const unsigned grid = (unsigned)((n_rows + 128 * RT - 1) / (128 * RT));
  auto run = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kKmeansNT), 0, st, emb, row_begin, n_rows, ops, c2, n_tiles, out_list, out_dist);
  };
  if (dt == NANN_F16) run(k_kmeans_assign<D, DT_F16, RT>);
  else run(k_kmeans_assign<D, DT_BF16, RT>);
}

int launch_kmeans_assign(const KmeansArgs& a, const KmeansLayout& L, const float* centroids, long long row_begin, long long n_rows,
                         int32_t* out_list, float* out_dist, unsigned char* ws, hipStream_t st) {
  if (n_rows <= 0) return NANN_OK;  // (dtype and d: the caller's flat_kmeans_check has held them to the instances below)
  uint4* ops = reinterpret_cast<uint4*>(ws + L.off_ops);
  float* c2 = reinterpret_cast<float*>(ws + L.off_c2);
  if (a.dt == NANN_F16)
    hipLaunchKernelGGL(k_kmeans_prepare<DT_F16>, dim3((unsigned)L.n_tiles), dim3(kKmeansNT), 0, st, centroids, a.n_lists, a.d, ops, c2);
  else
    hipLaunchKernelGGL(k_kmeans_prepare<DT_BF16>, dim3((unsigned)L.n_tiles), dim3(kKmeansNT), 0, st, centroids, a.n_lists, a.d, ops, c2);
  NANN_HIP_TRY(hipGetLastError());
  switch (a.d) {
    case 64: launch_kmeans_assign_d<64, 2>(a.dt, a.emb, row_begin, n_rows, ops, c2, L.n_tiles, out_list, out_dist, st); break;
    case 128: launch_kmeans_assign_d<128, 2>(a.dt, a.emb, row_begin, n_rows, ops, c2, L.n_tiles, out_list, out_dist, st); break;
    case 256: launch_kmeans_assign_d<256, 2>(a.dt, a.emb, row_begin, n_rows, ops, c2, L.n_tiles, out_list, out_dist, st); break;
    default: launch_kmeans_assign_d<512, 1>(a.dt, a.emb, row_begin, n_rows, ops, c2, L.n_tiles, out_list, out_dist, st); break;
  }
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

// the CSR of out_list: list_splits always, list_rows where `fill`
static int kmeans_csr(const KmeansArgs& a, const KmeansTrainLayout& L, const int32_t* out_list, bool fill, unsigned char* ws, hipStream_t st) {
  int32_t* counts = reinterpret_cast<int32_t*>(ws + L.off_counts);
  long long* info = reinterpret_cast<long long*>(ws + L.off_info);
  int64_t* list_splits = reinterpret_cast<int64_t*>(ws + L.off_splits);
  const long long n_clear = (long long)((L.off_seg - L.off_counts) / 4);
  hipLaunchKernelGGL(k_kmeans_clear, dim3((unsigned)std::min<long long>((n_clear + kKmeansNT - 1) / kKmeansNT, 2048)), dim3(kKmeansNT), 0, st, counts, n_clear);
  NANN_HIP_TRY(hipGetLastError());
  int rc = launch_lists_count(out_list, a.n_items, a.n_lists, L.groups, counts, info, st);
  if (rc) return rc;
  rc = launch_lists_splits(a.n_lists, L.groups, counts, list_splits, info, st);
  if (rc || !fill) return rc;
  return launch_lists_fill(out_list, a.n_items, a.n_lists, L.groups, counts, list_splits, reinterpret_cast<int32_t*>(ws + L.off_rows), st);
}

int launch_kmeans_train(const KmeansArgs& a, const KmeansTrainLayout& L, float* centroids, int n_iter, int32_t* out_list,
                        int32_t* out_counts, double* out_inertia, unsigned char* ws, hipStream_t st) {
  float* dist = reinterpret_cast<float*>(ws + L.off_dist);
  int64_t* list_splits = reinterpret_cast<int64_t*>(ws + L.off_splits);
  const int32_t* list_rows = reinterpret_cast<const int32_t*>(ws + L.off_rows);
  int64_t* seg_splits = reinterpret_cast<int64_t*>(ws + L.off_seg);
  float* partial = reinterpret_cast<float*>(ws + L.off_partial);
  double* block_sums = reinterpret_cast<double*>(ws + L.off_inertia);
  const int n_blocks = kmeans_inertia_blocks(a.n_items);
  const long long per = (a.n_items + n_blocks - 1) / n_blocks;
  // the segments of a round are counted on the device (at most max_segs): a grid of a few workgroups per CU strides over them
  const unsigned seg_grid = (unsigned)std::min<long long>(L.max_segs, kKmeansSegGrid);
  for (int it = 0; it <= n_iter; ++it) {
    int rc = launch_kmeans_assign(a, L.A, centroids, 0, a.n_items, out_list, dist, ws, st);
    if (rc) return rc;
    if (out_inertia) {
      hipLaunchKernelGGL(k_kmeans_inertia_blocks, dim3((unsigned)n_blocks), dim3(kKmeansNT), 0, st, dist, a.n_items, per, block_sums);
      hipLaunchKernelGGL(k_kmeans_inertia_sum, dim3(1), dim3(1), 0, st, block_sums, n_blocks, out_inertia + it);
      NANN_HIP_TRY(hipGetLastError());
    }
    rc = kmeans_csr(a, L, out_list, it < n_iter, ws, st);
    if (rc) return rc;
    if (it == n_iter) break;
    hipLaunchKernelGGL(k_kmeans_seg_splits, dim3(1), dim3(kKmeansNT), 0, st, list_splits, a.n_lists, seg_splits);
    if (a.dt == NANN_F16)
      hipLaunchKernelGGL(k_kmeans_partial<DT_F16>, dim3(seg_grid), dim3(kKmeansNT), 0, st, a.emb, a.d, list_splits, list_rows, seg_splits, a.n_lists, partial);
    else
      hipLaunchKernelGGL(k_kmeans_partial<DT_BF16>, dim3(seg_grid), dim3(kKmeansNT), 0, st, a.emb, a.d, list_splits, list_rows, seg_splits, a.n_lists, partial);
    hipLaunchKernelGGL(k_kmeans_mean, dim3((unsigned)a.n_lists), dim3(kKmeansNT), 0, st, centroids, a.d, list_splits, seg_splits, partial);
    NANN_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_kmeans_counts, dim3((unsigned)((a.n_lists + kKmeansNT - 1) / kKmeansNT)), dim3(kKmeansNT), 0, st, list_splits, a.n_lists, out_counts);
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}

}  // namespace nann
