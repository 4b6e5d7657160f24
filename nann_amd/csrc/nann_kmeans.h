// nann_kmeans.h -- the coarse quantiser on the device (nann_kmeans_assign, nann_kmeans_train): the nearest of
// n_lists f32 centroids by L2 for every row of an index of f16 / bf16 rows, on the matrix cores, and deterministic Lloyd rounds
// around it.  The reference has no such call; nothing here restates a line of it.
//
// Assignment.  argmin_c |x - c|^2 = argmin_c (|c|^2 - 2 <x, c>): an n_rows x n_lists matrix product whose result is needed only
// as a running (min, argmin) per row -- it dies in registers.
//   1. k_kmeans_prepare: the centroids are means and carry full f32 mantissas; one 16-bit value would throw half of them away.
//      They are split as the MLP scorers split their weights: c = hi + lo in f16 for f16 rows (hi = f16(c), lo = f16(c - hi)),
//      c = hi + mid + lo in bf16 for bf16 rows.  The row operand is exact, so <x, c> is the sum of two (three) MFMA products
//      into one f32 accumulator.  The terms are stored AS B FRAGMENTS of v_mfma_f32_32x32x16_{f16,bf16}: per tile of 32
//      centroids and k-step of 16 elements one block of 64 x 16 bytes a term -- lane l holds elements 16 ks + 8 (l >> 5) + [0, 8)
//      of centroid 32 t + (l & 31) --, so that the assign kernel's LDS fill and its LDS reads are straight 16-byte copies at
//      consecutive addresses.  |c|^2 in f32, elements in ascending order; behind n_lists the operands are zero and |c|^2 is
//      +inf, which masks the tail of the last tile without a branch in the sweep.
//   2. k_kmeans_assign<D, DT, RT>: a workgroup of 4 wavefronts owns 128 RT rows, a wavefront RT tiles of 32.  The wavefront
//      loads its rows' A fragments once, straight from the table (lane l: 16 bytes of row l & 31 at element 16 ks + 8 (l >> 5)),
//      and keeps them in registers for the whole sweep: RT D / 4 VGPRs.  The centroid operands stream through LDS in stages of
//      32 centroids x min(D, 128) elements, double-buffered: the loads of stage s + 1 are in flight in registers while stage s
//      feeds the MFMAs, one barrier a stage.  Every B fragment read from LDS serves RT MFMAs.  The C/D layout puts the centroid
//      on the lane (l & 31) and the row in the register (row 8 (j >> 2) + 4 (l >> 5) + (j & 3) in register j), so the
//      epilogue of a tile is, per register, one multiply-subtract and one strict `<` into the lane's own running (best,
//      argbest): a lane meets its centroids in ascending order, so its ties stay with the lower number.  After the sweep one
//      butterfly over the 32 lanes of a half (smaller value, then smaller number) ends in out_list / out_dist; |x|^2 comes from
//      the A fragments in registers.  Rows behind n_rows read the last row again and are never stored.
//
//      stage bytes (one buffer)      D = 64    D >= 128        registers of a wavefront      D = 64  128  256  512
//        f16  (2 terms)               8 KB      16 KB            A fragments (RT D / 4)          32   64  128  128
//        bf16 (3 terms)              12 KB      24 KB            accumulators (16 RT)            32   32   32   16
//      two buffers: at most 48 KB of a CU's 160 KB,              best, argbest (32 RT)           64   64   64   32
//      three workgroups a CU by LDS                              (RT = 2; 1 at D = 512)
//
// Update (a Lloyd round; deterministic, no float atomics).  The device CSR builder of nann_partition_create gives every list in
// ascending row order.  A list is cut into segments of kKmeansSeg rows counted from ITS OWN start; k_kmeans_partial sums a
// segment's rows in f32 -- 256 / (d / 8) row slots, a slot's rows in ascending order, then the slots in slot order --,
// k_kmeans_mean adds a list's segment sums in segment order and divides by the count in one f32 operation; a list of no rows
// keeps its centroid.  The order of every addition is a function of the list alone: neither the grid nor the other lists nor
// timing enter.  A list that holds most of the table is as many units of work as it has segments; the workgroups stride over them.
//
// Inertia: f64; a block's threads take its rows strided, a fixed tree joins them, the block sums are added in block order.
#pragma once
#include <cstddef>

#include "nann_search.h"

namespace nann {

constexpr int kKmeansMaxLists = 65536;      // most centroids of a call
constexpr int kKmeansTile = 32;             // centroids of one MFMA tile
constexpr int kKmeansNT = 256;              // threads of every kernel here
constexpr int kKmeansSeg = 1024;            // rows of a segment of the update
constexpr int kKmeansInertiaBlocks = 1024;  // most blocks of the inertia sum
constexpr int kKmeansSegGrid = 2048;        // most workgroups of the segment sums (they stride over the segments)

struct KmeansArgs {
  const void* emb;
  long long n_items;
  int d, dt;  // dt: NANN_F16 / NANN_BF16
  int n_lists;
};
inline size_t kmeans_up256(size_t v) { return (v + 255) & ~(size_t)255; }
inline int kmeans_terms(int dt) { return dt == NANN_F16 ? 2 : 3; }
// workspace of an assignment: [operands: n_tiles x (d / 16) k-steps x terms blocks of 1 KB | |c|^2 f32[32 n_tiles]]
struct KmeansLayout {
  int n_tiles;
  size_t off_ops, off_c2, total;
};
KmeansLayout kmeans_layout(int d, int dt, int n_lists);
int launch_kmeans_assign(const KmeansArgs& a, const KmeansLayout& L, const float* centroids, long long row_begin, long long n_rows,
                         int32_t* out_list, float* out_dist, unsigned char* ws, hipStream_t st);

// workspace of a training call: [the assignment's | dist f32[n] | list_splits i64[n_lists + 1] | list_rows i32[n] | the CSR
// build's counts i32[groups, n_lists] and info i64[4] | seg_splits i64[n_lists + 1] | segment sums f32[n_segs, d] | block sums f64]
struct KmeansTrainLayout {
  KmeansLayout A;
  int groups;
  long long max_segs;
  size_t off_dist, off_splits, off_rows, off_counts, off_info, off_seg, off_partial, off_inertia, total;
};
KmeansTrainLayout kmeans_train_layout(long long n_items, int d, int dt, int n_lists);
int launch_kmeans_train(const KmeansArgs& a, const KmeansTrainLayout& L, float* centroids, int n_iter, int32_t* out_list,
                        int32_t* out_counts, double* out_inertia, unsigned char* ws, hipStream_t st);

}  // namespace nann

#ifdef NANN_KMEANS_IMPL  // the kernels: nann_kmeans_inst.hip only (nann_flat.hip takes the declarations above)
namespace nann {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---- prepare ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t kmeans_bf16_rne(float f) {  // finite f
  const uint32_t u = __float_as_uint(f);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
// the 16-bit terms of c, the leading one first: T = 2 halves or T = 3 bf16
template <int DT>
__device__ __forceinline__ void kmeans_split(float c, uint32_t* t) {
  if constexpr (DT == DT_F16) {
    const __half hi = __float2half_rn(c);
    t[0] = __half_as_ushort(hi);
    t[1] = __half_as_ushort(__float2half_rn(c - __half2float(hi)));
  } else {
    t[0] = kmeans_bf16_rne(c);
    const float r1 = c - bf16_bits_to_float(t[0]);
    t[1] = kmeans_bf16_rne(r1);
    t[2] = kmeans_bf16_rne(r1 - bf16_bits_to_float(t[1]));
  }
}

// one workgroup per tile of 32 centroids
template <int DT>
__global__ __launch_bounds__(kKmeansNT) void k_kmeans_prepare(const float* __restrict__ cent, int n_lists, int d, uint4* __restrict__ ops,
                                                              float* __restrict__ c2) {
  constexpr int T = DT == DT_F16 ? 2 : 3;
  const int t = blockIdx.x, tid = threadIdx.x;
  if (tid < kKmeansTile) {
    const int c = t * kKmeansTile + tid;
    float s = __builtin_inff();
    if (c < n_lists) {
      s = 0.0f;
      for (int e = 0; e < d; ++e) {
        const float v = cent[(size_t)c * d + e];
        s += v * v;
      }
    }
    c2[c] = s;
  }
  const int n_ks = d / 16;
  for (int i = tid; i < n_ks * 64; i += kKmeansNT) {
    const int ks = i >> 6, lane = i & 63, c = t * kKmeansTile + (lane & 31);
    uint32_t h[8][T];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float v = c < n_lists ? cent[(size_t)c * d + ks * 16 + 8 * (lane >> 5) + e] : 0.0f;
      kmeans_split<DT>(v, h[e]);
    }
#pragma unroll
    for (int term = 0; term < T; ++term)
      ops[(((size_t)t * n_ks + ks) * T + term) * 64 + lane] =
          make_uint4(h[0][term] | h[1][term] << 16, h[2][term] | h[3][term] << 16, h[4][term] | h[5][term] << 16, h[6][term] | h[7][term] << 16);
  }
}

// ---- assign -----------------------------------------------------------------------------------------------------------------
template <int DT>
__device__ __forceinline__ f32x16 kmeans_mfma(const uint4& a, const uint4& b, const f32x16& c) {
  if constexpr (DT == DT_F16)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// element e of the 8 a uint4 holds
template <int DT>
__device__ __forceinline__ float kmeans_elem(const uint4& v, int e) {
  const uint32_t w = e < 2 ? v.x : e < 4 ? v.y : e < 6 ? v.z : v.w, bits = (w >> (16 * (e & 1))) & 0xffffu;
  return DT == DT_F16 ? half_bits_to_float(bits) : bf16_bits_to_float(bits);
}

// grid: ceil(n_rows / (128 RT)) workgroups; n_rows >= 1, n_tiles >= 1
template <int D, int DT, int RT>
__global__ __launch_bounds__(kKmeansNT) void k_kmeans_assign(const void* __restrict__ emb, long long row_begin, long long n_rows,
                                                             const uint4* __restrict__ ops, const float* __restrict__ c2, int n_tiles,
                                                             int32_t* __restrict__ out_list, float* __restrict__ out_dist) {
  constexpr int T = DT == DT_F16 ? 2 : 3;
  constexpr int KC = D < 128 ? D : 128;    // elements of a stage
  constexpr int KS = KC / 16;              // its k-steps
  constexpr int SPT = D / KC;              // stages of a centroid tile
  constexpr int STAGE = KS * T * 64;       // uint4 of a stage
  constexpr int FILL = STAGE / kKmeansNT;  // of them a thread copies
  static_assert(STAGE % kKmeansNT == 0, "a stage is a whole number of copies per thread");
  __shared__ uint4 lds[2][STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
  const long long r0 = ((long long)blockIdx.x * 4 + wave) * (32 * RT);

  // the wavefront's rows, once
  uint4 a[RT][D / 16];
  float x2[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const long long row = row_begin + min(r0 + rt * 32 + col, n_rows - 1);
    const uint4* src = reinterpret_cast<const uint4*>(static_cast<const unsigned char*>(emb) + (size_t)row * D * 2) + half;
    float s = 0.0f;
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks) {
      a[rt][ks] = src[2 * ks];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float v = kmeans_elem<DT>(a[rt][ks], e);
        s += v * v;
      }
    }
    const float o = __shfl_xor(s, 32);
    x2[rt] = half ? o + s : s + o;  // (the lower half's elements first)
  }

  f32x16 acc[RT];
  float best[RT][16];
  int32_t arg[RT][16];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      acc[rt][j] = 0.0f;
      best[rt][j] = __builtin_inff();
      arg[rt][j] = 0;
    }
  }

  const int n_stages = n_tiles * SPT;
#pragma unroll
  for (int i = 0; i < FILL; ++i) lds[0][tid + kKmeansNT * i] = ops[tid + kKmeansNT * i];
  __syncthreads();
  for (int t = 0; t < n_tiles; ++t) {
    const float c2v = c2[t * kKmeansTile + col];
#pragma unroll
    for (int kc = 0; kc < SPT; ++kc) {
      const int s = t * SPT + kc;
      const uint4* next = ops + (size_t)min(s + 1, n_stages - 1) * STAGE;  // (behind the last stage: itself again, never read)
      uint4 pre[FILL];
#pragma unroll
      for (int i = 0; i < FILL; ++i) pre[i] = next[tid + kKmeansNT * i];
      const uint4* B = lds[s & 1];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
        for (int term = 0; term < T; ++term) {
          const uint4 b = B[(ks * T + term) * 64 + lane];
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) acc[rt] = kmeans_mfma<DT>(a[rt][kc * KS + ks], b, acc[rt]);
        }
      }
#pragma unroll
      for (int i = 0; i < FILL; ++i) lds[(s + 1) & 1][tid + kKmeansNT * i] = pre[i];
      __syncthreads();
    }
    const int32_t c = t * kKmeansTile + col;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float v = c2v - 2.0f * acc[rt][j];
        if (v < best[rt][j]) {
          best[rt][j] = v;
          arg[rt][j] = c;
        }
        acc[rt][j] = 0.0f;
      }
    }
  }

  // a row's best over the 32 lanes of its half; lane j of a half ends up with register j's row
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    float mv = 0.0f;
    int32_t ma = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      float v = best[rt][j];
      int32_t c = arg[rt][j];
#pragma unroll
      for (int o = 1; o < 32; o <<= 1) {
        const float ov = __shfl_xor(v, o);
        const int32_t oc = __shfl_xor(c, o);
        if (ov < v || (ov == v && oc < c)) {
          v = ov;
          c = oc;
        }
      }
      if (col == j) {
        mv = v;
        ma = c;
      }
    }
    const int m = 8 * ((col & 15) >> 2) + 4 * half + (col & 3);  // the row of register col within the tile
    const float xv = __shfl(x2[rt], m);
    const long long row = r0 + rt * 32 + m;
    if (col < 16 && row < n_rows) {
      out_list[row] = ma;
      if (out_dist) out_dist[row] = mv + xv;
    }
  }
}

// ---- update -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kKmeansNT) void k_kmeans_clear(int32_t* __restrict__ p, long long n) {
  for (long long i = (long long)blockIdx.x * kKmeansNT + threadIdx.x; i < n; i += (long long)gridDim.x * kKmeansNT) p[i] = 0;
}

// one workgroup: seg_splits[l] = segments of the lists before l; a thread takes a run of lists
__global__ __launch_bounds__(kKmeansNT) void k_kmeans_seg_splits(const int64_t* __restrict__ list_splits, int n_lists,
                                                                 int64_t* __restrict__ seg_splits) {
  __shared__ long long run[kKmeansNT];
  const int tid = threadIdx.x, per = (n_lists + kKmeansNT - 1) / kKmeansNT;
  const int l0 = min(tid * per, n_lists), l1 = min(l0 + per, n_lists);
  long long mine = 0;
  for (int l = l0; l < l1; ++l) mine += (list_splits[l + 1] - list_splits[l] + kKmeansSeg - 1) / kKmeansSeg;
  run[tid] = mine;
  __syncthreads();
  long long at = 0;
  for (int i = 0; i < tid; ++i) at += run[i];
  for (int l = l0; l < l1; ++l) {
    seg_splits[l] = at;
    at += (list_splits[l + 1] - list_splits[l] + kKmeansSeg - 1) / kKmeansSeg;
  }
  if (tid == kKmeansNT - 1) seg_splits[n_lists] = at;
}

// the f32 sum of every segment, the workgroups striding over them (the result does not depend on which workgroup takes a segment).
// Thread (slot, c) owns elements 8 c + [0, 8) of the rows slot, slot + RS, .. of the segment; the slots are joined in slot order.
template <int DT>
__global__ __launch_bounds__(kKmeansNT) void k_kmeans_partial(const void* __restrict__ emb, int d, const int64_t* __restrict__ list_splits,
                                                              const int32_t* __restrict__ list_rows, const int64_t* __restrict__ seg_splits,
                                                              int n_lists, float* __restrict__ partial) {
  __shared__ float sums[kKmeansNT * 8];
  const int tpr = d / 8, rs = kKmeansNT / tpr, slot = threadIdx.x / tpr, c = threadIdx.x % tpr;
  const long long n_segs = seg_splits[n_lists];
  for (long long g = blockIdx.x; g < n_segs; g += gridDim.x) {
    int lo = 0, hi = n_lists - 1;  // the last list with seg_splits[l] <= g (lists of no rows share their successor's value)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (seg_splits[mid] <= g) lo = mid;
      else hi = mid - 1;
    }
    const long long p0 = list_splits[lo] + (g - seg_splits[lo]) * kKmeansSeg, p1 = min(p0 + kKmeansSeg, (long long)list_splits[lo + 1]);
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (long long p = p0 + slot; p < p1; p += rs) {
      const uint4 v = reinterpret_cast<const uint4*>(static_cast<const unsigned char*>(emb) + (size_t)list_rows[p] * d * 2)[c];
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += kmeans_elem<DT>(v, e);
    }
    __syncthreads();  // (the segment before this one has been read out of sums)
#pragma unroll
    for (int e = 0; e < 8; ++e) sums[slot * d + 8 * c + e] = acc[e];
    __syncthreads();
    for (int e = threadIdx.x; e < d; e += kKmeansNT) {
      float s = 0.0f;
      for (int i = 0; i < rs; ++i) s += sums[i * d + e];
      partial[(size_t)g * d + e] = s;
    }
  }
}

// workgroup l: centroid l = (its segment sums, in segment order) / count; untouched where the list is empty
__global__ __launch_bounds__(kKmeansNT) void k_kmeans_mean(float* __restrict__ cent, int d, const int64_t* __restrict__ list_splits,
                                                           const int64_t* __restrict__ seg_splits, const float* __restrict__ partial) {
  const int l = blockIdx.x;
  const long long count = list_splits[l + 1] - list_splits[l];
  if (count == 0) return;
  const float n = (float)count;
  for (int e = threadIdx.x; e < d; e += kKmeansNT) {
    float s = 0.0f;
    for (long long g = seg_splits[l]; g < seg_splits[l + 1]; ++g) s += partial[(size_t)g * d + e];
    cent[(size_t)l * d + e] = s / n;
  }
}

__global__ __launch_bounds__(kKmeansNT) void k_kmeans_counts(const int64_t* __restrict__ list_splits, int n_lists, int32_t* __restrict__ out_counts) {
  const int l = blockIdx.x * kKmeansNT + threadIdx.x;
  if (l < n_lists) out_counts[l] = (int32_t)(list_splits[l + 1] - list_splits[l]);
}

// ---- inertia ----------------------------------------------------------------------------------------------------------------
// block b: rows [b per, (b + 1) per)
__global__ __launch_bounds__(kKmeansNT) void k_kmeans_inertia_blocks(const float* __restrict__ dist, long long n, long long per,
                                                                     double* __restrict__ block_sums) {
  __shared__ double sh[kKmeansNT];
  const long long i0 = (long long)blockIdx.x * per, i1 = min(i0 + per, n);
  double s = 0.0;
  for (long long i = i0 + threadIdx.x; i < i1; i += kKmeansNT) s += (double)dist[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = kKmeansNT / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) block_sums[blockIdx.x] = sh[0];
}
__global__ void k_kmeans_inertia_sum(const double* __restrict__ block_sums, int n_blocks, double* __restrict__ out) {
  double s = 0.0;
  for (int b = 0; b < n_blocks; ++b) s += block_sums[b];
  *out = s;
}

}  // namespace nann
#endif  // NANN_KMEANS_IMPL
