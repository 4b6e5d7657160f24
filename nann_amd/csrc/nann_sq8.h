// nann_sq8.h -- scalar-quantised exhaustive search (nann_search_all_sq8): an int8 code table of an index's rows, scanned on the
// integer matrix cores for a wide approximate fetch, then an exact re-rank of the fetched rows.
//
// The code of a vector x (a row, widened exactly from its 16 bits, or a query's f32 vector); every step is ONE IEEE f32
// operation, round to nearest, nothing contracted:
//   amax = max_j |x_j|     scale = amax / 127     code_j = clamp(rint(x_j / scale), -127, 127)     norm = sum_j code_j^2 (i32)
// (amax == 0: scale = 0 and every code 0).  The approximate score of a query (cq, sq, nq) against a row (cx, sx, nx), with the
// exact integer D = sum_j cq_j cx_j:
//   inner product   s = (sq * sx) * (float)D
//   L2              a = (sq * sq) * (float)nq,  b = (sx * sx) * (float)nx,  c = ((2 * sq) * sx) * (float)D,  s = c - (a + b)
// |D| and the norms are at most 127^2 * 512 < 2^24: the conversions are exact, and the whole score is a function of integers and
// four roundings that a numpy model restates bit for bit (tests/sq8_model.py).
//
// Per chunk of queries (the ScanLayout chunk of nann_scan.h, at most 128):
//   1. k_sq8_encode: the chunk's queries -> codes, scales, norms;
//   2. k_scan_sq8: scores f32[chunk, n_items], the buffer k_scan_slab_topk and k_scan_merge take as they are -- their selection
//      and its tie rule (score descending, lower row first) give the fetch lists;
//   3. k_sq8_sort_rows: each query's fetched rows in ascending row order, the row_splits of the chunk's lists, and the fetch
//      lists to the caller's arrays.  The candidate-list search (nann_cand.h) then scores the sorted lists exactly; its tie rule,
//      lower position, is then "lower row number": the final list is in TopKV2 order.
//
// k_scan_sq8: v_mfma_i32_32x32x32_i8 with the QUERIES as A and the table ROWS as B.  The C/D layout puts the table row on the
// lane (col = lane & 31) and the query in the register (row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)), so one store of one
// query covers 32 consecutive rows per half-wave: 128-byte runs.  A wave keeps the B fragments of its 32 rows in registers (d / 8
// VGPRs) and sweeps the chunk's query tiles past them; the chunk's query codes lie in LDS, rows d + 16 bytes apart (an odd number
// of 16-byte units: ds_read_b128 without bank conflicts).  Operand element j of lane (r, h = lane >> 5) in k-step s is byte
// 32 s + 16 h + j of query / row r -- the SAME bytes on both sides, which is all an integer dot product needs: whatever k the
// hardware gives position (h, j), it gives it in A and in B alike.  tests/test_sq8_gpu.py pins this with one-hot queries.
#pragma once
#include <cstddef>

#include "nann_scan.h"
#include "nann_search.h"

namespace nann {

// the table as the kernels take it (device pointers)
struct Sq8Args {
  const int8_t* codes;     // i8[n_items, d]
  const float* scales;     // f32[n_items]
  const int32_t* norms;    // i32[n_items]
  const int64_t* item_ids;
  long long n_items;
  int d;
  int metric;              // MT_L2 or MT_IP
};

// workspace of a call: [the ScanLayout at k = fetch | what follows], every part a multiple of 256 bytes.  Sized by the chunk.
struct Sq8Layout {
  size_t off_qcodes, off_qscales, off_qnorms;          // the chunk's encoded queries
  size_t off_ids, off_fscores, off_frows;              // the merge's fetch lists: item ids i64, scores f32, rows i32 [chunk, fetch]
  size_t off_sorted, off_splits, off_status;           // rows ascending i32[chunk, fetch], row_splits i64[chunk + 1], status i32[chunk]
  size_t off_cand;                                     // the candidate-list search's workspace (CandLayout)
  size_t total;
};
Sq8Layout sq8_layout(const ScanLayout& L, int d, int fetch, size_t cand_bytes);

// codes, scales, norms of n vectors of d elements (dt: NANN_F16 / NANN_BF16 / NANN_F32)
int launch_sq8_encode(const void* x, int dt, long long n, int d, int8_t* codes, float* scales, int32_t* norms, hipStream_t st);
// the fetch stage of one chunk of n_q queries: steps 1-3 above.  out_fetch_*: this chunk's slice of the caller's arrays, or null.
int launch_sq8_fetch(const Sq8Args& a, const ScanLayout& L, const Sq8Layout& S, const float* q, int n_q, int fetch,
                     unsigned char* ws, int32_t* out_fetch_index, float* out_fetch_scores, hipStream_t st);

}  // namespace nann

#ifdef NANN_SQ8_IMPL  // the kernels: nann_sq8_inst.hip only (nann_flat.hip takes the declarations above)
namespace nann {

typedef int i32x4v __attribute__((ext_vector_type(4)));
typedef int i32x16v __attribute__((ext_vector_type(16)));

constexpr int kSq8NT = 256;           // threads of k_sq8_encode and k_scan_sq8: four wavefronts
constexpr int kSq8RowsPerWg = 1024;   // table rows of a workgroup of k_scan_sq8: eight tiles of 32 per wavefront
constexpr int kSq8QPad = 16;          // bytes behind a query's codes in LDS
// dynamic LDS of k_scan_sq8: the chunk's query codes, then per query its scale term and its norm term
__host__ __device__ constexpr int sq8_scan_lds(int d) { return kScanMaxChunk * (d + kSq8QPad) + kScanMaxChunk * 8; }

template <int DT>
__device__ __forceinline__ float sq8_load(const void* x, size_t i) {
  if constexpr (DT == DT_F32) return static_cast<const float*>(x)[i];
  else if constexpr (DT == DT_F16) return half_bits_to_float(static_cast<const uint16_t*>(x)[i]);
  else return bf16_bits_to_float(static_cast<const uint16_t*>(x)[i]);
}

// one wavefront per vector; lane l holds elements l, l + 64, ...  (max and the integer sum do not depend on the order)
template <int DT>
__global__ __launch_bounds__(kSq8NT) void k_sq8_encode(const void* __restrict__ x, long long n, int d, int8_t* __restrict__ codes,
                                                       float* __restrict__ scales, int32_t* __restrict__ norms) {
  const int lane = threadIdx.x & 63;
  const int per = d >> 6;  // d / 64 <= 8
  for (long long v = (long long)blockIdx.x * (kSq8NT / 64) + (threadIdx.x >> 6); v < n; v += (long long)gridDim.x * (kSq8NT / 64)) {
    float e[kMaxD / 64];
    float amax = 0.0f;
#pragma unroll
    for (int i = 0; i < kMaxD / 64; ++i) {
      e[i] = i < per ? sq8_load<DT>(x, (size_t)v * d + i * 64 + lane) : 0.0f;
      amax = fmaxf(amax, fabsf(e[i]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    const float scale = __fdiv_rn(amax, 127.0f);
    int norm = 0;
#pragma unroll
    for (int i = 0; i < kMaxD / 64; ++i) {
      if (i < per) {
        float c = amax == 0.0f ? 0.0f : rintf(__fdiv_rn(e[i], scale));
        c = fminf(fmaxf(c, -127.0f), 127.0f);
        const int ci = (int)c;
        norm += ci * ci;
        codes[(size_t)v * d + i * 64 + lane] = (int8_t)ci;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) norm += __shfl_xor(norm, o);
    if (lane == 0) {
      scales[v] = scale;
      norms[v] = norm;
    }
  }
}

// grid: blocks of kSq8RowsPerWg rows.  scores f32[n_q, n_items], n_q <= kScanMaxChunk.
// LDS: qc[kScanMaxChunk][D + 16] the query codes (zeros behind n_q), qs[kScanMaxChunk] = sq (inner product) or 2 sq (L2),
// qa[kScanMaxChunk] = (sq sq) (float)nq.
template <int NS, int METRIC>  // NS = d / 32 k-steps
__global__ __launch_bounds__(kSq8NT) void k_scan_sq8(const int8_t* __restrict__ codes, const float* __restrict__ scales,
                                                     const int32_t* __restrict__ norms, long long n_items,
                                                     const int8_t* __restrict__ qcodes, const float* __restrict__ qscales,
                                                     const int32_t* __restrict__ qnorms, int n_q, float* __restrict__ scores) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int D = NS * 32, QS = D + kSq8QPad;
  float* qs = reinterpret_cast<float*>(smem + kScanMaxChunk * QS);
  float* qa = qs + kScanMaxChunk;
  const int tid = threadIdx.x;
  // the chunk's queries: 16-byte pieces, zeros for the queries behind n_q (their products are never stored)
  for (int i = tid; i < kScanMaxChunk * (D / 16); i += kSq8NT) {
    const int qi = i / (D / 16), p = i % (D / 16);
    i32x4v v = {0, 0, 0, 0};
    if (qi < n_q) v = *reinterpret_cast<const i32x4v*>(qcodes + (size_t)qi * D + p * 16);
    *reinterpret_cast<i32x4v*>(smem + qi * QS + p * 16) = v;
  }
  for (int qi = tid; qi < kScanMaxChunk; qi += kSq8NT) {
    const float sq = qi < n_q ? qscales[qi] : 0.0f;
    const int nq = qi < n_q ? qnorms[qi] : 0;
    qs[qi] = METRIC == MT_IP ? sq : __fmul_rn(2.0f, sq);
    qa[qi] = __fmul_rn(__fmul_rn(sq, sq), (float)nq);
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int n_qt = (n_q + 31) >> 5;
  const long long wg_row0 = (long long)blockIdx.x * kSq8RowsPerWg;
  for (int it = 0; it < kSq8RowsPerWg / (32 * (kSq8NT / 64)); ++it) {
    const long long row0 = wg_row0 + (long long)(it * (kSq8NT / 64) + wave) * 32;
    if (row0 >= n_items) break;  // (uniform over the wavefront)
    const long long row = row0 + r;
    const long long row_ld = row < n_items ? row : n_items - 1;  // (a row behind the table: the last one again, never stored)
    i32x4v b[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) b[s] = *reinterpret_cast<const i32x4v*>(codes + (size_t)row_ld * D + s * 32 + h * 16);
    const float sx = scales[row_ld];
    const float bx = __fmul_rn(__fmul_rn(sx, sx), (float)norms[row_ld]);
    for (int t = 0; t < n_qt; ++t) {
      i32x16v acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      const unsigned char* qrow = smem + (t * 32 + r) * QS + h * 16;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const i32x4v a = *reinterpret_cast<const i32x4v*>(qrow + s * 32);
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b[s], acc, 0, 0, 0);
      }
      if (row < n_items) {
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          const int qi = t * 32 + (g & 3) + 8 * (g >> 2) + 4 * h;
          if (qi < n_q) {
            const float dot = (float)acc[g];
            float sc;
            if constexpr (METRIC == MT_IP) {
              sc = __fmul_rn(__fmul_rn(qs[qi], sx), dot);
            } else {
              const float c = __fmul_rn(__fmul_rn(qs[qi], sx), dot);
              sc = __fsub_rn(c, __fadd_rn(qa[qi], bx));
            }
            scores[(size_t)qi * n_items + row] = sc;
          }
        }
      }
    }
  }
}

// one workgroup per query: the fetched rows (all distinct) in ascending order by a bitonic sort in LDS; thread 0 of every
// workgroup writes its query's two row_splits (neighbours write the same value to the shared one); the fetch lists as the merge
// left them go to the caller's arrays.
__global__ __launch_bounds__(kSq8NT) void k_sq8_sort_rows(const int32_t* __restrict__ rows, const float* __restrict__ fscores, int fetch,
                                                          int32_t* __restrict__ sorted, long long* __restrict__ splits,
                                                          int32_t* __restrict__ out_fetch_index, float* __restrict__ out_fetch_scores) {
  __shared__ int32_t v[kMaxK];
  const size_t qi = blockIdx.x;
  const int tid = threadIdx.x;
  int n2 = 1;
  while (n2 < fetch) n2 <<= 1;
  for (int i = tid; i < n2; i += kSq8NT) {
    const int32_t rw = i < fetch ? rows[qi * fetch + i] : 0x7fffffff;
    v[i] = rw;
    if (i < fetch) {
      if (out_fetch_index) out_fetch_index[qi * fetch + i] = rw;
      if (out_fetch_scores) out_fetch_scores[qi * fetch + i] = fscores[qi * fetch + i];
    }
  }
  __syncthreads();
  for (int size = 2; size <= n2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < (n2 >> 1); i += kSq8NT) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const bool up = (lo & size) == 0;
        const int32_t x = v[lo], y = v[hi];
        if ((x > y) == up) {
          v[lo] = y;
          v[hi] = x;
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < fetch; i += kSq8NT) sorted[qi * fetch + i] = v[i];
  if (tid == 0) {
    splits[qi] = (long long)qi * fetch;
    splits[qi + 1] = (long long)(qi + 1) * fetch;
  }
}

}  // namespace nann
#endif
