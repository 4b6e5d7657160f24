// The kernels of the batch order (nann_order.h): compiled into the core object only (nann_hip.hip).
#pragma once
#include "nann_order.h"

namespace nann {

__device__ inline float order_row_elem(const void* emb, int dt, size_t i) {
  if (dt == NANN_F32) return reinterpret_cast<const float*>(emb)[i];
  const uint16_t h = reinterpret_cast<const uint16_t*>(emb)[i];
  if (dt == NANN_F16) return __half2float(__ushort_as_half(h));
  return __uint_as_float((uint32_t)h << 16);
}

// key[q] = argmin_p |q - piv_p|^2 = argmin_p (|piv_p|^2 - 2 q . piv_p); ties -> the lower pivot.  The pivots come as f32
// [d][P] with their norms behind, padded to kOrderMaxPivots (pivT, built at index creation): staged with 16-byte copies that all issue at once, lane p
// of a wave reads column p (no bank conflicts).  A wave takes 4 queries (from LDS, broadcast) x pivots lane, lane + 64.
__global__ __launch_bounds__(256) void k_order_key(const float* pivT, int d, int P, const float* q, int n, int32_t* key) {
  extern __shared__ float4 order_lds4[];
  float* piv = reinterpret_cast<float*>(order_lds4);  // [d][P], then pn[kOrderMaxPivots]
  float* qs = piv + (size_t)d * P + kOrderMaxPivots;   // [kOrderKeyQueries][d]
  const int q0 = blockIdx.x * kOrderKeyQueries, nq = min(kOrderKeyQueries, n - q0);
  const int pv4 = (d * P + kOrderMaxPivots) / 4, qv4 = nq * d / 4;  // (d is a multiple of 64)
  for (int i = threadIdx.x; i < pv4; i += 256) order_lds4[i] = reinterpret_cast<const float4*>(pivT)[i];
  for (int i = threadIdx.x; i < qv4; i += 256)
    reinterpret_cast<float4*>(qs)[i] = reinterpret_cast<const float4*>(q + (size_t)q0 * d)[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pa = lane, pb = lane + 64;
  float acc[4][2] = {};
  const float* qw = qs + (size_t)wave * 4 * d;
  for (int k = 0; k < d; ++k) {
    const float va = piv[k * P + min(pa, P - 1)], vb = piv[k * P + min(pb, P - 1)];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float x = qw[j * d + k];
      acc[j][0] = fmaf(x, va, acc[j][0]);
      acc[j][1] = fmaf(x, vb, acc[j][1]);
    }
  }
  const float* pn = piv + (size_t)d * P;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int qi = wave * 4 + j;
    float best = pa < P ? fmaf(-2.0f, acc[j][0], pn[min(pa, P - 1)]) : INFINITY;
    int arg = pa < P ? pa : 0x7fffffff;
    if (pb < P) {
      const float s = fmaf(-2.0f, acc[j][1], pn[pb]);
      if (s < best) { best = s; arg = pb; }
    }
    for (int m = 32; m >= 1; m >>= 1) {
      const float ob = __shfl_xor(best, m);
      const int oa = __shfl_xor(arg, m);
      if (ob < best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    if (lane == 0 && qi < nq) key[q0 + qi] = arg < P ? arg : 0;  // (NaN queries: pivot 0)
  }
}

// one workgroup: histogram of keys, exclusive prefix, then a stable scatter tile by tile (rank inside a wave by
// shuffles, wave offsets inside a tile by a per-key scan over the waves).  Also zeroes the segment heads.
__global__ __launch_bounds__(kOrderSortThreads) void k_order_perm(const int32_t* key, int n, int P, int32_t* perm,
                                                                 unsigned int* heads) {
  constexpr int W = kOrderSortThreads / 64;
  __shared__ int base[kOrderMaxPivots];
  __shared__ int wofs[W][kOrderMaxPivots];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid < kOrderSegs * kOrderHeadStride) heads[tid] = 0u;
  for (int p = tid; p < P; p += blockDim.x) base[p] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += blockDim.x) atomicAdd(&base[key[i]], 1);
  __syncthreads();
  int pre = 0;  // exclusive prefix of the histogram: thread p sums the counts below p
  if (tid < P)
    for (int p = 0; p < tid; ++p) pre += base[p];
  __syncthreads();
  if (tid < P) base[tid] = pre;
  __syncthreads();
  for (int t0 = 0; t0 < n; t0 += kOrderSortThreads) {
    for (int i = tid; i < W * kOrderMaxPivots; i += blockDim.x) (&wofs[0][0])[i] = 0;
    __syncthreads();
    const int i = t0 + tid;
    const int k = i < n ? key[i] : -1;
    int rank = 0;
    bool last = true;
#pragma unroll
    for (int j = 0; j < 64; ++j) {
      const int kj = __builtin_amdgcn_readlane(k, j);
      if (kj == k) { if (j < lane) ++rank; else if (j > lane) last = false; }
    }
    if (k >= 0 && last) wofs[w][k] = rank + 1;  // this wave's count of key k
    __syncthreads();
    for (int p = tid; p < P; p += blockDim.x) {
      int run = base[p];
      for (int v = 0; v < W; ++v) { const int c = wofs[v][p]; wofs[v][p] = run; run += c; }
      base[p] = run;
    }
    __syncthreads();
    if (k >= 0) perm[wofs[w][k] + rank] = i;
    __syncthreads();
  }
}

}  // namespace nann
