// The kernels of the batch order (nann_order.h): compiled into the core object only (nann_traverse.hip).
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
// of a wave reads column p (no bank conflicts).  A wave takes kOrderKeyQueries / 4 queries (from LDS, broadcast) x pivots
// lane, lane + 64.
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
  constexpr int QW = kOrderKeyQueries / 4;  // queries per wave
  float acc[QW][2] = {};
  const float* qw = qs + (size_t)wave * QW * d;
  for (int k = 0; k < d; ++k) {
    const float va = piv[k * P + min(pa, P - 1)], vb = piv[k * P + min(pb, P - 1)];
#pragma unroll
    for (int j = 0; j < QW; ++j) {
      const float x = qw[j * d + k];
      acc[j][0] = fmaf(x, va, acc[j][0]);
      acc[j][1] = fmaf(x, vb, acc[j][1]);
    }
  }
  const float* pn = piv + (size_t)d * P;
#pragma unroll
  for (int j = 0; j < QW; ++j) {
    const int qi = wave * QW + j;
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

// The lanes of this wavefront that hold this lane's key, as a mask (k < 0: not a query, in no lane's mask): one ballot per
// key bit, each ANDed in as it is or complemented.  A lane's rank among them is the popcount of the mask below it, and
// the highest lane of a mask knows the wavefront's count of the key: its rank + 1.
__device__ inline unsigned long long order_same_key(int k) {
  unsigned long long m = __ballot(k >= 0);
#pragma unroll
  for (int b = 0; b < 7; ++b) {
    const unsigned long long s = __ballot((k >> b) & 1);
    m &= ((k >> b) & 1) ? s : ~s;
  }
  return m;
}

__device__ inline int order_rank(unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
}

__device__ inline int order_wave_scan(int v, int lane) {  // inclusive
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const int o = __shfl_up(v, s);
    if (lane >= s) v += o;
  }
  return v;
}

// One workgroup: a stable counting sort of the query indices by key.  Also zeroes the segment heads and the header of
// the search workspace (the launch behind it starts from both).
// n <= kOrderFastQueries: every thread keeps its keys (positions t * 1024 + tid) in registers; a wavefront is a run of 64
// consecutive queries and writes its count of every key it holds into cnt[key][run]; one exclusive scan of that table
// in key-major, run-minor order -- 16 entries per thread, a wave scan, 16 wave totals -- turns every entry into the
// first position of its (key, run); perm[cnt[key][run] + rank] = i.  Four barriers, no atomics.
// Larger n: histogram of keys, exclusive prefix (wavefront 0, two keys per lane), then the same ranks tile by tile with
// a per-key scan over the tile's 16 wavefronts.
__global__ __launch_bounds__(kOrderSortThreads) void k_order_perm(const int32_t* key, int n, int P, int32_t* perm,
                                                                 unsigned int* heads, unsigned int* header) {
  constexpr int W = kOrderSortThreads / 64;
  __shared__ __attribute__((aligned(16))) uint16_t cnt[kOrderMaxPivots * kOrderFastRuns];
  __shared__ int wtot[W];
  __shared__ int base[kOrderMaxPivots];
  __shared__ int wofs[W][kOrderMaxPivots];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (tid < kOrderSegs * kOrderHeadStride) heads[tid] = 0u;
  if (tid < kOrderHeaderWords) header[tid] = 0u;
  if (n <= kOrderFastQueries) {
    constexpr int T = kOrderFastQueries / kOrderSortThreads;
    int k[T], rank[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int i = t * kOrderSortThreads + tid;
      k[t] = i < n ? key[i] : -1;
    }
    uint4* cnt4 = reinterpret_cast<uint4*>(cnt);
    cnt4[tid] = make_uint4(0u, 0u, 0u, 0u);
    cnt4[tid + kOrderSortThreads] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < T; ++t) {
      rank[t] = 0;
      if ((t * W + w) * 64 < n) {  // (one run per wavefront and tile: uniform)
        const unsigned long long m = order_same_key(k[t]);
        rank[t] = order_rank(m);
        if (k[t] >= 0 && (m >> lane) == 1ull) cnt[k[t] * kOrderFastRuns + t * W + w] = (uint16_t)(rank[t] + 1);
      }
    }
    __syncthreads();
    const uint4 lo = cnt4[2 * tid], hi = cnt4[2 * tid + 1];  // entries 16 tid .. 16 tid + 15, two to a word
    const uint32_t v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    int sum = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) sum += (int)(v[j] & 0xffffu) + (int)(v[j] >> 16);
    const int incl = order_wave_scan(sum, lane);
    if (lane == 63) wtot[w] = incl;
    __syncthreads();
    uint32_t run = (uint32_t)(incl - sum);
    for (int x = 0; x < w; ++x) run += (uint32_t)wtot[x];
    uint32_t o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // (a prefix is at most n: it fits 16 bits)
      const uint32_t c0 = v[j] & 0xffffu, c1 = v[j] >> 16;
      o[j] = run | ((run + c0) << 16);
      run += c0 + c1;
    }
    cnt4[2 * tid] = make_uint4(o[0], o[1], o[2], o[3]);
    cnt4[2 * tid + 1] = make_uint4(o[4], o[5], o[6], o[7]);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < T; ++t)
      if (k[t] >= 0) perm[(int)cnt[k[t] * kOrderFastRuns + t * W + w] + rank[t]] = t * kOrderSortThreads + tid;
    return;
  }
  for (int p = tid; p < kOrderMaxPivots; p += blockDim.x) base[p] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += blockDim.x) atomicAdd(&base[key[i]], 1);
  __syncthreads();
  if (w == 0) {  // exclusive prefix of the histogram (the keys from P up count nothing)
    const int c0 = base[2 * lane], c1 = base[2 * lane + 1];
    const int pre = order_wave_scan(c0 + c1, lane) - (c0 + c1);
    base[2 * lane] = pre;
    base[2 * lane + 1] = pre + c0;
  }
  __syncthreads();
  for (int t0 = 0; t0 < n; t0 += kOrderSortThreads) {
    for (int i = tid; i < W * kOrderMaxPivots; i += blockDim.x) (&wofs[0][0])[i] = 0;
    __syncthreads();
    const int i = t0 + tid;
    const int k = i < n ? key[i] : -1;
    const unsigned long long m = order_same_key(k);
    const int rank = order_rank(m);
    if (k >= 0 && (m >> lane) == 1ull) wofs[w][k] = rank + 1;  // this wave's count of key k
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
