// nann_interests.h -- nann_user_seq_interests: one behaviour sequence comm_seq f16[L, d] -> up to n_vec interest vectors, their
// weights and the slot of every history row, in the layout nann_search_multi takes for q and nann_fusion for per-user weights.
// The reference has no such step (its user side is the mean, build_opt_graph.py:76-79); the contract is the header's, held bit
// for bit against tests/interests_model.py.
//
// k_user_seq_interests, one workgroup of kInterestsNT threads per user, everything after the first pass out of LDS:
//   0. the history is staged once: 16-byte global loads where d % 8 == 0 and the base is 16-byte aligned (as
//      k_user_seq_mean_lds), 2-byte loads otherwise; a piece with a non-zero half (+-0 are zero) marks its row as live.  A row
//      takes PD = (ceil(d / 2) | 1) dwords of LDS: an ODD dword pitch, so that the lanes of a wavefront that hold different rows
//      and the same k -- the distance passes -- hit 64 different banks (at a pitch of 2 d bytes, d = 128, they would hit one);
//   1. m = live rows; the mean in k_user_seq_mean's order (per column one chain over the rows ascending from +0, one divide);
//   2. seeds: farthest point.  One thread per row runs the k-ascending chain against the newest centroid and keeps the row's
//      running minimum; the argmax over rows is a u64 max of (distance bits << 32 | ~r) -- distances are >= +0, so their bits
//      order as the values do, and ~r sends ties to the lowest r -- reduced with DPP / permute shuffles inside a wavefront and
//      through LDS across the four;
//   3. Lloyd rounds: one thread per (cluster, row) pair, pair p = c * L + r, runs the chain into dist[c][r] (a wavefront shares
//      c: the centroid reads are broadcasts); one thread per row takes the argmin in ascending c (strict <: ties to the lowest
//      c), counts its cluster and raises `changed` when the row moved; one thread per (cluster, column) sums the member rows in
//      ascending r and divides once.  A round that moves no row ends the rounds: its update would rebuild the centroids it
//      started from, so every later round and the final pass repeat it;
//   4. one thread sorts the at most 16 live clusters (insertion sort: count descending, stable, so ties keep the lower cluster
//      number in front); everyone writes q, weights, n_interests and assign.
// LDS, dynamic: L * PD * 4 (the history) + (n_vec + 1) * d * 4 (centroids, mean) + L * n_vec * 4 (dist) + 2 * L * 4 (running
// minimum, assign) + 256 B of state: 16.6 KB at the serving shape 50 x 128 x 4, 63.3 KB at 200 x 128 x 8.  The budget is 64 KB
// (kInterestsMaxLds), two workgroups per CU at the worst; a shape beyond it is NANN_ERR_UNSUPPORTED.
#pragma once
#include <cstddef>
#include <cstdint>

#include "nann_search.h"

namespace nann {

static_assert(NANN_INTERESTS_MAX_VEC == 16 && NANN_INTERESTS_MAX_ITER == 32, "include/nann_hip.h: the limits of the call");

constexpr int kInterestsNT = 256;
constexpr size_t kInterestsMaxLds = 64 * 1024;
constexpr size_t kInterestsStateBytes = 256;

struct InterestsArgs {
  const void* seq;      // f16[n_users, seq_len, d]
  int seq_len, d, n_vec, n_iter;
  int wide;             // 1: d % 8 == 0 and a 16-byte aligned base -> 16-byte loads
  float* q;             // f32[n_users, n_vec, d]
  float* weights;       // f32[n_users, n_vec] or null
  int32_t* n_interests; // i32[n_users] or null
  int32_t* assign;      // i32[n_users, seq_len] or null
};

// dwords of LDS a history row takes: odd, see above
__host__ __device__ inline int interests_pitch(int d) { return ((d + 1) / 2) | 1; }
inline size_t interests_lds_bytes(long long seq_len, long long d, long long n_vec) {
  return kInterestsStateBytes + (size_t)seq_len * (size_t)interests_pitch((int)d) * 4 + (size_t)(n_vec + 1) * (size_t)d * 4 +
         (size_t)seq_len * (size_t)n_vec * 4 + (size_t)seq_len * 8;
}

}  // namespace nann

#ifdef NANN_INTERESTS_IMPL  // the kernel and the entry point: nann_cand_inst.hip only
namespace nann {

struct InterestsState {
  unsigned long long red[kInterestsNT / 64];  // a wavefront's best (value, row)
  int cnt[NANN_INTERESTS_MAX_VEC];            // members per cluster
  int order[NANN_INTERESTS_MAX_VEC];          // slot -> cluster
  int slot[NANN_INTERESTS_MAX_VEC];           // cluster -> slot, -1: dropped
  int m, changed, n_out;
};
static_assert(sizeof(InterestsState) <= kInterestsStateBytes, "the state block of k_user_seq_interests");

// dist(r, c): k ascending from +0, t = x[k] - c[k], acc = acc + t * t -- one chain, no FMA (-ffp-contract=off)
__device__ __forceinline__ float interests_dist(const uint32_t* row, const float* c, int d) {
  float acc = 0.0f;
  const int pairs = d >> 1;
  for (int i = 0; i < pairs; ++i) {
    const uint32_t w = row[i];
    float t = half_bits_to_float(w & 0xffffu) - c[2 * i];
    acc = acc + t * t;
    t = half_bits_to_float(w >> 16) - c[2 * i + 1];
    acc = acc + t * t;
  }
  if (d & 1) {
    const float t = half_bits_to_float(row[pairs] & 0xffffu) - c[d - 1];
    acc = acc + t * t;
  }
  return acc;
}

__device__ __forceinline__ float interests_elem(const uint32_t* rows, int pd, int r, int k) {
  const uint32_t w = rows[r * pd + (k >> 1)];
  return half_bits_to_float((k & 1) ? (w >> 16) : (w & 0xffffu));
}

// the greatest key of the workgroup, for every thread
__device__ __forceinline__ unsigned long long interests_wg_max(unsigned long long key, InterestsState* S) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o);
    key = other > key ? other : key;
  }
  __syncthreads();  // (the previous reduction's reads of red[])
  if ((threadIdx.x & 63) == 0) S->red[threadIdx.x >> 6] = key;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kInterestsNT / 64; ++w) key = S->red[w] > key ? S->red[w] : key;
  return key;
}

__global__ __launch_bounds__(kInterestsNT) void k_user_seq_interests(InterestsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char interests_smem[];
  const int tid = threadIdx.x;
  const int L = a.seq_len, d = a.d, n_vec = a.n_vec, pd = interests_pitch(d);
  const size_t u = blockIdx.x;
  InterestsState* S = reinterpret_cast<InterestsState*>(interests_smem);
  uint32_t* rows = reinterpret_cast<uint32_t*>(interests_smem + kInterestsStateBytes);  // [L][pd]
  float* cent = reinterpret_cast<float*>(rows + (size_t)L * pd);                        // [n_vec][d]
  float* mean = cent + (size_t)n_vec * d;                                               // [d]
  float* dist = mean + d;                                                               // [n_vec][L]
  float* mind = dist + (size_t)n_vec * L;                                               // [L]
  int* asg = reinterpret_cast<int*>(mind + L);  // [L]: -1 pad, kFree live and not yet assigned, else the row's cluster
  constexpr int kFree = NANN_INTERESTS_MAX_VEC;

  // ---- 0. the history into LDS, live rows flagged on the way
  for (int r = tid; r < L; r += kInterestsNT) asg[r] = -1;
  if (tid == 0) S->m = 0;
  if (d & 1)  // (the narrow path fills a row half by half: an odd d would leave the upper half of its last dword unwritten)
    for (int r = tid; r < L; r += kInterestsNT) rows[r * pd + (d >> 1)] = 0u;
  __syncthreads();
  if (a.wide) {
    const int ppr = d >> 3, n_pieces = L * ppr;
    const uint4* src = static_cast<const uint4*>(a.seq) + u * (size_t)n_pieces;
    for (int i = tid; i < n_pieces; i += kInterestsNT) {
      const uint4 v = src[i];
      const int r = i / ppr, c = i - r * ppr;
      uint32_t* dst = rows + r * pd + 4 * c;
      dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
      if ((v.x | v.y | v.z | v.w) & 0x7fff7fffu) asg[r] = kFree;  // (every writer stores the same value)
    }
  } else {
    const uint16_t* src = static_cast<const uint16_t*>(a.seq) + u * (size_t)L * d;
    uint16_t* rows16 = reinterpret_cast<uint16_t*>(rows);
    const int n = L * d;
    for (int i = tid; i < n; i += kInterestsNT) {
      const uint16_t h = src[i];
      const int r = i / d, k = i - r * d;
      rows16[(size_t)r * pd * 2 + k] = h;
      if (h & 0x7fffu) asg[r] = kFree;
    }
  }
  __syncthreads();
  // ---- 1. m and the mean
  for (int r = tid; r < L; r += kInterestsNT)
    if (asg[r] >= 0) atomicAdd(&S->m, 1);
  __syncthreads();
  const int m = S->m;
  float* q = a.q + u * (size_t)n_vec * d;
  if (m == 0) {  // (the whole workgroup: m is the same for every thread)
    for (int i = tid; i < n_vec * d; i += kInterestsNT) q[i] = 0.0f;
    if (a.weights) for (int i = tid; i < n_vec; i += kInterestsNT) a.weights[u * n_vec + i] = 0.0f;
    if (a.assign) for (int r = tid; r < L; r += kInterestsNT) a.assign[u * L + r] = -1;
    if (a.n_interests && tid == 0) a.n_interests[u] = 0;
    return;
  }
  for (int k = tid; k < d; k += kInterestsNT) {
    float acc = 0.0f;
    for (int r = 0; r < L; ++r) acc = acc + interests_elem(rows, pd, r, k);  // (a pad row adds +-0: nothing)
    mean[k] = acc / (float)m;
  }
  __syncthreads();
  // ---- 2. the seeds
  int n_c = 1;
  if (n_vec == 1) {
    for (int k = tid; k < d; k += kInterestsNT) cent[k] = mean[k];
  } else {
    for (int j = 0; j < n_vec; ++j) {  // pass 0 against the mean, pass j against seed j - 1
      const float* c = j == 0 ? mean : cent + (size_t)(j - 1) * d;
      unsigned long long key = 0ull;  // (below every live row's key: ~r has high bits set)
      for (int r = tid; r < L; r += kInterestsNT) {
        if (asg[r] < 0) continue;
        float v = interests_dist(rows + r * pd, c, d);
        if (j >= 2) v = fminf(mind[r], v);
        if (j >= 1) mind[r] = v;
        const unsigned long long mine = ((unsigned long long)__float_as_uint(v) << 32) | (uint32_t)~(uint32_t)r;
        key = mine > key ? mine : key;
      }
      key = interests_wg_max(key, S);
      if (j >= 1 && (uint32_t)(key >> 32) == 0u) break;  // every row lies on a seed (the same key in every thread)
      const int r = (int)~(uint32_t)key;
      for (int k = tid; k < d; k += kInterestsNT) cent[(size_t)j * d + k] = interests_elem(rows, pd, r, k);
      n_c = j + 1;
      __syncthreads();
    }
  }
  __syncthreads();
  // ---- 3. Lloyd rounds; pass n_iter is the final assignment
  for (int it = 0;; ++it) {
    if (tid < NANN_INTERESTS_MAX_VEC) S->cnt[tid] = 0;
    if (tid == 0) S->changed = 0;
    const int n_pairs = n_c * L;
    for (int p = tid; p < n_pairs; p += kInterestsNT) {
      const int c = p / L, r = p - c * L;
      if (asg[r] >= 0) dist[p] = interests_dist(rows + r * pd, cent + (size_t)c * d, d);
    }
    __syncthreads();
    for (int r = tid; r < L; r += kInterestsNT) {
      const int was = asg[r];
      if (was < 0) continue;
      int at = 0;
      float best = dist[r];
      for (int c = 1; c < n_c; ++c) {
        const float v = dist[c * L + r];
        if (v < best) { best = v; at = c; }
      }
      asg[r] = at;
      atomicAdd(&S->cnt[at], 1);
      if (at != was) S->changed = 1;
    }
    __syncthreads();
    if (it == a.n_iter || !S->changed) break;  // (LDS: the same for every thread)
    const int n_cols = n_c * d;
    for (int i = tid; i < n_cols; i += kInterestsNT) {
      const int c = i / d, k = i - c * d;
      const int count = S->cnt[c];
      if (count == 0) continue;  // a cluster without members keeps its centroid
      float acc = 0.0f;
      for (int r = 0; r < L; ++r)
        if (asg[r] == c) acc = acc + interests_elem(rows, pd, r, k);
      cent[i] = acc / (float)count;
    }
    __syncthreads();  // (also: every read of changed and cnt lies in front of the next round's reset)
  }
  // ---- 4. order, padding, outputs
  if (tid == 0) {
    int n = 0;
    for (int c = 0; c < n_c; ++c) {
      S->slot[c] = -1;
      if (S->cnt[c] == 0) continue;
      int at = n++;
      while (at > 0 && S->cnt[S->order[at - 1]] < S->cnt[c]) { S->order[at] = S->order[at - 1]; --at; }
      S->order[at] = c;
    }
    for (int s = 0; s < n; ++s) S->slot[S->order[s]] = s;
    S->n_out = n;
  }
  __syncthreads();
  const int n_out = S->n_out;
  for (int i = tid; i < n_vec * d; i += kInterestsNT) {
    const int s = i / d, k = i - s * d;
    q[i] = cent[(size_t)S->order[s < n_out ? s : 0] * d + k];
  }
  if (a.weights)
    for (int s = tid; s < n_vec; s += kInterestsNT)
      a.weights[u * n_vec + s] = s < n_out ? (float)S->cnt[S->order[s]] / (float)m : 0.0f;
  if (a.assign)
    for (int r = tid; r < L; r += kInterestsNT) a.assign[u * L + r] = asg[r] < 0 ? -1 : S->slot[asg[r]];
  if (a.n_interests && tid == 0) a.n_interests[u] = n_out;
}

}  // namespace nann

extern "C" int nann_user_seq_interests(const void* comm_seq_f16, int64_t n_users, int32_t seq_len, int32_t d, int32_t n_vec,
                                       int32_t n_iter, float* q, float* weights, int32_t* n_interests, int32_t* assign,
                                       nann_stream_t stream) {
  using namespace nann;
  const char* who = "nann_user_seq_interests";
  if (n_users < 0 || seq_len < 1 || d < 1 || n_vec < 1 || n_iter < 0)
    return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": bad shape (n_users < 0, seq_len < 1, d < 1, n_vec < 1 or n_iter < 0)");
  if (n_vec > NANN_INTERESTS_MAX_VEC) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": n_vec exceeds NANN_INTERESTS_MAX_VEC");
  if (n_iter > NANN_INTERESTS_MAX_ITER) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": n_iter exceeds NANN_INTERESTS_MAX_ITER");
  if (n_users > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": too many users in one call");
  // (seq_len and d first: within 64 KB of halves each, so the sum below cannot overflow)
  if (seq_len > 32768 || d > 32768 || interests_lds_bytes(seq_len, d, n_vec) > kInterestsMaxLds)
    return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": seq_len x d x n_vec beyond the kernel's LDS budget of 64 KB");
  if (n_users == 0) return NANN_OK;
  if (!comm_seq_f16 || !q) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  InterestsArgs a = {};
  a.seq = comm_seq_f16;
  a.seq_len = seq_len;
  a.d = d;
  a.n_vec = n_vec;
  a.n_iter = n_iter;
  a.wide = d % 8 == 0 && (reinterpret_cast<uintptr_t>(comm_seq_f16) & 15) == 0;
  a.q = q;
  a.weights = weights;
  a.n_interests = n_interests;
  a.assign = assign;
  const size_t lds = interests_lds_bytes(seq_len, d, n_vec);
  if (lds > 48 * 1024)
    NANN_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_user_seq_interests), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)kInterestsMaxLds));
  hipLaunchKernelGGL(k_user_seq_interests, dim3((unsigned)n_users), dim3(kInterestsNT), lds, reinterpret_cast<hipStream_t>(stream),
                     a);
  NANN_HIP_TRY(hipGetLastError());
  return NANN_OK;
}
#endif
