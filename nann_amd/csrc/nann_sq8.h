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
// steps 1 and 2 of one chunk of n_q queries: the queries' codes, scales and norms, and the approximate score of every row into
// scores f32[n_q, n_items] (the ScanLayout's buffer)
int launch_sq8_scan(const Sq8Args& a, const float* q, int n_q, int8_t* qcodes, float* qscales, int32_t* qnorms, float* scores,
                    hipStream_t st);
// the fetch stage of one chunk of n_q queries: steps 1-3 above.  out_fetch_*: this chunk's slice of the caller's arrays, or null.
int launch_sq8_fetch(const Sq8Args& a, const ScanLayout& L, const Sq8Layout& S, const float* q, int n_q, int fetch,
                     unsigned char* ws, int32_t* out_fetch_index, float* out_fetch_scores, hipStream_t st);


// ---- the certified form (nann_search_all_sq8_exact): the fetch stage and its exact re-rank give a cut tau_q,
// a survivor pass over the chunk's score buffer keeps every row whose exact score the bound cannot put below tau_q, and the
// candidate-list search over the survivors returns nann_search_all's bits.
//
// Per row (k_sq8_row_err, nann_sq8_bounds; the same kernel gives a chunk's queries theirs), every step ONE f32 operation:
//   lane l of the row's wavefront, elements j = l, l + 64, ... in that order:  p = scale * (float)code_j;  r = x_j - p;
//   acc = acc + r * r (from +0);  then acc = acc + shfl_xor(acc, o) for o = 32, 16, 8, 4, 2, 1;  e0 = sqrt(acc)
//   xhat = (scale * sqrt((float)norm)) * kSq8Infl + kSq8Abs
//   err  = (e0 + 2^-23 * xhat) * kSq8Infl + kSq8Abs
// sqrt is sqrtf, which the build rounds correctly (hipcc's default; __fsqrt_rn is the hardware's approximate root here).
// The inflations make the stored values upper bounds of the real |x - scale code| and scale sqrt(norm) (lemma 1).
constexpr float kSq8Infl = 1.0f + 0x1p-18f;   // covers up to 32 roundings of a sum of non-negative terms
constexpr float kSq8Infl2 = 1.0f + 0x1p-20f;  // covers up to 8
constexpr float kSq8Abs = 0x1p-60f;           // covers what underflows in a row's squares and products
constexpr float kSq8Tiny = 0x1p-100f;         // covers what underflows in a score, approximate or exact

// the terms of one query of a chunk (k_sq8_exact_terms), read by the survivor predicate
struct Sq8QTerms {
  float tau;    // the exact score of the k-th entry of the re-ranked fetch list: a lower bound of the true k-th best score (the range form: the threshold)
  float eq;     // >= |q - sq cq|
  float qhat;   // >= sq sqrt(nq)
  float w;      // L2: >= sqrt((-tau + tiny) / (1 - G)) + eq, the radius a row's code must lie beyond.  IP: >= qhat + eq
  int32_t ok;   // tau, eq and qhat are finite (L2: and tau <= 0)
  int32_t certified;  // ok and at most cap survivors (k_sq8_exact_lists, behind the count); the range form: the query has a list to fill
  int32_t pad[2];
};
// G: the relative error of the exact scorer's f32 accumulation over d terms and one subtraction each, (d + 4) 2^-24 >=
// gamma_(d + 2) (exact in f32)
inline float sq8_gamma(int d) { return (float)(d + 4) * 0x1p-24f; }

// workspace of a certified call: [Sq8Layout, its CandLayout sized for chunk * cap positions | what follows]
struct Sq8ExactLayout {
  Sq8Layout S;
  int n_blocks;                         // range_n_blocks(n_items)
  long long cap;                        // min(cap, n_items): most survivors of a certified query
  size_t off_qerr, off_qxhat;           // f32[chunk] each: the chunk's queries through k_sq8_row_err
  size_t off_a_ids, off_a_scores;       // stage (a): i64[chunk, k], f32[chunk, k]
  size_t off_terms;                     // Sq8QTerms[chunk]
  size_t off_counts;                    // i32[chunk, n_blocks] block counts, then prefixes; i32[chunk] totals behind
  size_t off_xsplits;                   // i64[chunk + 1]: the compact row_splits of the final lists
  size_t off_rows;                      // i32[chunk * cap]: the final lists, survivors or the sorted fetch list
  size_t total;
};
Sq8ExactLayout sq8_exact_layout(const ScanLayout& L, int kind, int d, int fetch, long long cap, int k, long long n_items);

// err, xhat f32[n] of n vectors and their codes (dt: NANN_F16 / NANN_BF16 / NANN_F32)
int launch_sq8_row_err(const void* x, int dt, long long n, int d, const int8_t* codes, const float* scales, const int32_t* norms,
                       float* err, float* xhat, hipStream_t st);
// behind a chunk's launch_sq8_fetch and its launch_cand at k into off_a_*: the query terms, the survivor count, the block
// prefixes, certified / n_survivors of the chunk (out_*: this chunk's slice), the compact row_splits and the final lists
int launch_sq8_survivors(const Sq8Args& a, const ScanLayout& L, const Sq8ExactLayout& X, const float* q, const float* err,
                         const float* xhat, int n_q, int fetch, int k, unsigned char* ws, int32_t* out_certified,
                         int32_t* out_n_survivors, hipStream_t st);


// ---- the certified range form (nann_search_all_range_sq8_exact): the caller's threshold IS the cut, so there is
// no fetch stage and no top-k.  Per chunk: the int8 scan; the query terms at tau = thresholds[q] (k_sq8_exact_terms at k = 1); the
// survivor pass (k_sq8_surv_count, k_range_scan, k_sq8_surv_fill, unchanged) with k_sq8_range_lists in the place of
// k_sq8_exact_lists; the candidate-list search's plan and scorer over the survivor lists (launch_cand_scores, no top-k), which
// leaves the exact scores in list-position order = row order; and the ragged selection over them:
//   k_sq8_range_count  grid (block of kRangeBlockRows positions of the list buffer, query): the matches of the block by
//                      k_range_count's rule, s >= t and s != -inf; a block beyond the query's list writes 0 and leaves unloaded
//   k_range_scan, k_range_splits (nann_range.h, with the chunk's c0): the block prefixes and the call-wide row_splits
//   k_sq8_range_fill   the same grid: every match to row_splits[query] + (block prefix) + (rank in block), ballots and
//                      range_lanes_below, no atomic, EVERY store behind pos < capacity
// A block is a run of positions of the list buffer that begins on a 16-byte boundary, as in nann_range.h: a query's list begins
// wherever the lists in front of it end.
// L2 and a finite threshold above +0 (k_sq8_range_lists): the scorer stores 0 - (a sum of squares), no score exceeds +0 and a NaN
// matches nothing, so the query is certified with no survivor and an empty list, whatever the survivor count says.
// workspace of a call: [the ScanLayout at k = 0 | what follows], every part a multiple of 256 bytes.  Sized by the chunk.
struct Sq8RangeLayout {
  int n_blocks;                                   // range_n_blocks(n_items): blocks of a query in the survivor pass
  int n_lblocks;                                  // range_n_blocks(cap): blocks of a query's list in the selection
  long long cap;                                  // min(cap, n_items): most survivors of a certified query
  size_t off_qcodes, off_qscales, off_qnorms;     // the chunk's encoded queries
  size_t off_qerr, off_qxhat;                     // f32[chunk] each: the chunk's queries through k_sq8_row_err
  size_t off_terms;                               // Sq8QTerms[chunk]
  size_t off_counts;                              // i32[chunk, n_blocks] survivor counts, then prefixes; i32[chunk] totals behind
  size_t off_xsplits;                             // i64[chunk + 1]: the compact row_splits of the survivor lists
  size_t off_rows;                                // i32[chunk * cap]: the survivor lists
  size_t off_cand;                                // CandLayout for chunk * cap positions: the exact scores f32[chunk * cap] first
  size_t off_rcounts;                             // i32[chunk, n_lblocks] match counts, then prefixes; i32[chunk] totals behind
  size_t total;
};
Sq8RangeLayout sq8_range_layout(const ScanLayout& L, int kind, int d, long long cap, long long n_items);
// One chunk, up to the survivor lists: scan, query terms at thr (this chunk's slice of the thresholds), survivor pass, lists.
int launch_sq8_range_survivors(const Sq8Args& a, const ScanLayout& L, const Sq8RangeLayout& R, const float* q, const float* thr,
                               const float* err, const float* xhat, int n_q, unsigned char* ws, int32_t* out_certified,
                               int32_t* out_n_survivors, hipStream_t st);
// One chunk, behind launch_cand_scores over the survivor lists: the ragged selection.  thr, row_splits: the call's arrays (c0
// picks the chunk's part).  Entry outputs may be null when capacity == 0.
int launch_sq8_range_select(const Sq8Args& a, const Sq8RangeLayout& R, size_t off_scores, const float* thr, long long c0, int n_q,
                            long long capacity, unsigned char* ws, int64_t* row_splits, int64_t* out_item_ids, float* out_scores,
                            int32_t* out_index, hipStream_t st);

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

// ---- the certified form ---------------------------------------------------------------------------------------------------
// one wavefront per vector, shaped like k_sq8_encode; the order of every step is the one stated at the head of this file
template <int DT>
__global__ __launch_bounds__(kSq8NT) void k_sq8_row_err(const void* __restrict__ x, long long n, int d, const int8_t* __restrict__ codes,
                                                        const float* __restrict__ scales, const int32_t* __restrict__ norms,
                                                        float* __restrict__ err, float* __restrict__ xhat) {
  const int lane = threadIdx.x & 63;
  const int per = d >> 6;  // d / 64 <= 8
  for (long long v = (long long)blockIdx.x * (kSq8NT / 64) + (threadIdx.x >> 6); v < n; v += (long long)gridDim.x * (kSq8NT / 64)) {
    const float scale = scales[v];
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < kMaxD / 64; ++i) {
      if (i < per) {
        const size_t at = (size_t)v * d + i * 64 + lane;
        const float p = __fmul_rn(scale, (float)codes[at]);
        const float r = __fsub_rn(sq8_load<DT>(x, at), p);
        acc = __fadd_rn(acc, __fmul_rn(r, r));
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, o));
    if (lane == 0) {
      const float e0 = sqrtf(acc);
      const float xh = __fadd_rn(__fmul_rn(__fmul_rn(scale, sqrtf((float)norms[v])), kSq8Infl), kSq8Abs);
      xhat[v] = xh;
      err[v] = __fadd_rn(__fmul_rn(__fadd_rn(e0, __fmul_rn(0x1p-23f, xh)), kSq8Infl), kSq8Abs);
    }
  }
}

// one thread per query of the chunk: tau from stage (a)'s scores f32[n_q, k], the query's error terms, the radius / norm term
template <int METRIC>
__global__ __launch_bounds__(kSq8NT) void k_sq8_exact_terms(const float* __restrict__ a_scores, int k, const float* __restrict__ qerr,
                                                            const float* __restrict__ qxhat, int n_q, float g,
                                                            Sq8QTerms* __restrict__ terms) {
  const int qi = blockIdx.x * kSq8NT + threadIdx.x;
  if (qi >= n_q) return;
  Sq8QTerms t = {};
  t.tau = a_scores[(size_t)qi * k + (k - 1)];
  t.eq = qerr[qi];
  t.qhat = qxhat[qi];
  const float big = 3.402823466e+38f;
  bool ok = fabsf(t.tau) <= big && fabsf(t.eq) <= big && fabsf(t.qhat) <= big;  // (a NaN fails every comparison)
  if constexpr (METRIC == MT_L2) {
    ok = ok && t.tau <= 0.0f;
    const float t2 = __fmul_rn(__fadd_rn(-t.tau, kSq8Tiny), __fadd_rn(1.0f, __fmul_rn(2.0f, g)));
    const float rho = __fmul_rn(sqrtf(t2), kSq8Infl2);
    t.w = __fmul_rn(__fadd_rn(rho, t.eq), kSq8Infl2);
  } else {
    t.w = __fmul_rn(__fadd_rn(t.qhat, t.eq), kSq8Infl2);
  }
  t.ok = ok ? 1 : 0;
  terms[qi] = t;
}

// The survivor predicate: false only where the exact f32 score of the row is provably below tau.  a: the
// approximate score; err, xhat: the row's terms.  Every comparison is written so that a NaN keeps the row; a row ties tau survives.
template <int METRIC>
__device__ __forceinline__ bool sq8_survives(float a, float err, float xhat, const Sq8QTerms& t, float g) {
  if (!(fabsf(a) <= 3.402823466e+38f)) return true;  // (an overflowed or NaN score bounds nothing)
  if constexpr (METRIC == MT_L2) {
    const float w = __fadd_rn(t.qhat, xhat);
    const float dl = __fadd_rn(__fmul_rn(__fmul_rn(w, w), 0x1p-20f), kSq8Tiny);  // >= |a - (-|qhat_vec - xhat_vec|^2)|
    const float lo = __fsub_rn(-a, dl);                                            // a lower bound of |qhat_vec - xhat_vec|^2
    const float s = __fadd_rn(t.w, err);
    const float hi = __fmul_rn(__fmul_rn(s, s), kSq8Infl);
    return !(lo > hi);
  } else {
    const float cross = __fadd_rn(__fadd_rn(__fmul_rn(t.eq, xhat), __fmul_rn(err, t.qhat)), __fmul_rn(t.eq, err));
    const float gt = __fmul_rn(g, __fmul_rn(t.w, __fadd_rn(xhat, err)));
    const float p = __fadd_rn(__fadd_rn(__fadd_rn(cross, gt), __fmul_rn(0x1p-22f, fabsf(a))), kSq8Tiny);
    const float ub = __fadd_rn(a, __fmul_rn(p, kSq8Infl));
    return !(ub < t.tau);
  }
}

// What a thread holds of block blockIdx.x of query blockIdx.y, after range_load (nann_range.h): the same 16-byte aligned walk
// over the score buffer; bit j of m[p] says that element j of pass p is a row of the query and survives.
struct Sq8SurvBlock {
  size_t at[kRangePasses];
  unsigned m[kRangePasses];
  size_t begin;
};
template <int METRIC>
__device__ __forceinline__ void sq8_surv_load(const float* __restrict__ scores, long long n_items, const float* __restrict__ err,
                                              const float* __restrict__ xhat, const Sq8QTerms t, float g, Sq8SurvBlock* b) {
  const size_t begin = (size_t)blockIdx.y * (size_t)n_items, end = begin + (size_t)n_items;
  const size_t g0 = (begin >> 2) + (size_t)blockIdx.x * (kRangeBlockRows / 4);
  b->begin = begin;
#pragma unroll
  for (int p = 0; p < kRangePasses; ++p) {
    const size_t at = (g0 + (size_t)p * kRangeNT + threadIdx.x) * 4;
    b->at[p] = at;
    b->m[p] = 0u;
    if (at < end) {  // (the 16 bytes begin inside the row or up to three positions in front of it, and end within 16 B of its end)
      const f32x4v s = *reinterpret_cast<const f32x4v*>(scores + at);
      if (at >= begin && at + 3 < end) {
        // all four positions are rows of the query: their terms are 16 contiguous bytes of each array, at a 4-byte alignment
        // that depends on the query (begin mod 4) -- one load each where the target takes unaligned vector loads
        const size_t row = at - begin;
        f32x4v e, xh;
        __builtin_memcpy(&e, err + row, 16);
        __builtin_memcpy(&xh, xhat + row, 16);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (sq8_survives<METRIC>(s[j], e[j], xh[j], t, g)) b->m[p] |= 1u << j;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (at + j >= begin && at + j < end) {
            const size_t row = at + j - begin;  // < n_items: the loads below are inside the two arrays
            if (sq8_survives<METRIC>(s[j], err[row], xhat[row], t, g)) b->m[p] |= 1u << j;
          }
        }
      }
    }
  }
}

// counts[query][block] = survivors of the block (k_range_count's shape)
template <int METRIC>
__global__ __launch_bounds__(kRangeNT) void k_sq8_surv_count(const float* __restrict__ scores, long long n_items,
                                                             const float* __restrict__ err, const float* __restrict__ xhat,
                                                             const Sq8QTerms* __restrict__ terms, float g,
                                                             int32_t* __restrict__ counts) {
  __shared__ int wave_cnt[kRangeNT / 64];
  Sq8SurvBlock b;
  sq8_surv_load<METRIC>(scores, n_items, err, xhat, terms[blockIdx.y], g, &b);
  int c = 0;
#pragma unroll
  for (int p = 0; p < kRangePasses; ++p)
#pragma unroll
    for (int j = 0; j < 4; ++j) c += __popcll(__ballot((b.m[p] >> j) & 1u));
  if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < kRangeNT / 64; ++w) t += wave_cnt[w];
    counts[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
  }
}

// One workgroup per chunk, behind k_range_scan: certified and n_survivors of every query, the compact row_splits of the final
// lists -- a certified query's survivors, else its fetch list -- and the sorted fetch lists of the uncertified queries copied
// into their places.  n_q <= kScanMaxChunk <= kSq8NT.
__global__ __launch_bounds__(kSq8NT) void k_sq8_exact_lists(const int32_t* __restrict__ totals, Sq8QTerms* __restrict__ terms,
                                                            int n_q, int fetch, long long cap, const int32_t* __restrict__ sorted,
                                                            long long* __restrict__ xsplits, int32_t* __restrict__ rows,
                                                            int32_t* __restrict__ out_certified,
                                                            int32_t* __restrict__ out_n_survivors) {
  __shared__ long long len[kSq8NT];
  __shared__ long long begin[kSq8NT + 1];
  __shared__ int cert[kSq8NT];
  const int tid = threadIdx.x;
  int total = 0, c = 1;
  if (tid < n_q) {
    total = totals[tid];
    c = terms[tid].ok != 0 && (long long)total <= cap ? 1 : 0;
    terms[tid].certified = c;
    out_certified[tid] = c;
    out_n_survivors[tid] = total;
  }
  cert[tid] = c;
  len[tid] = tid < n_q ? (c ? (long long)total : (long long)fetch) : 0;
  __syncthreads();
  long long sum = 0;
  for (int j = 0; j < tid; ++j) sum += len[j];
  begin[tid] = sum;
  if (tid < n_q) xsplits[tid] = sum;
  if (tid == n_q - 1) xsplits[n_q] = sum + len[tid];
  __syncthreads();
  for (int qi = 0; qi < n_q; ++qi) {
    if (cert[qi]) continue;
    for (int i = tid; i < fetch; i += kSq8NT) rows[begin[qi] + i] = sorted[(size_t)qi * fetch + i];  // (fetch <= cap: inside the list's room)
  }
}

// The survivors of a block to their places in the query's list, ascending row order, no atomics (k_range_fill's shape).
// prefix = counts behind k_range_scan, totals = the queries' sums behind them.  An uncertified query's list is its fetch list:
// nothing is written for it.
template <int METRIC>
__global__ __launch_bounds__(kRangeNT) void k_sq8_surv_fill(const float* __restrict__ scores, long long n_items,
                                                            const float* __restrict__ err, const float* __restrict__ xhat,
                                                            const Sq8QTerms* __restrict__ terms, float g,
                                                            const int32_t* __restrict__ prefix, const int32_t* __restrict__ totals,
                                                            const long long* __restrict__ xsplits, long long cap,
                                                            int32_t* __restrict__ rows) {
  constexpr int W = kRangeNT / 64;
  __shared__ int cnt[kRangePasses * W];
  // (uniform over the workgroup) nothing to place: an uncertified query, or a block without a survivor -- most blocks of a
  // large corpus -- leaves before it reads a score
  const size_t pb = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  const int block_end = blockIdx.x + 1 < gridDim.x ? prefix[pb + 1] : totals[blockIdx.y];
  if (terms[blockIdx.y].certified == 0 || block_end == prefix[pb]) return;
  Sq8SurvBlock b;
  sq8_surv_load<METRIC>(scores, n_items, err, xhat, terms[blockIdx.y], g, &b);
  const int wave = threadIdx.x >> 6;
  int rank[kRangePasses];  // survivors of the pass's wavefront in the lanes below this one
#pragma unroll
  for (int p = 0; p < kRangePasses; ++p) {
    int below = 0, all = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned long long m = __ballot((b.m[p] >> j) & 1u);
      below += range_lanes_below(m);
      all += __popcll(m);
    }
    rank[p] = below;
    if ((threadIdx.x & 63) == 0) cnt[p * W + wave] = all;
  }
  __syncthreads();
  const long long q_begin = xsplits[blockIdx.y];
  const long long room = min(cap, xsplits[blockIdx.y + 1] - q_begin);  // the list's length: the survivor count iff certified
  const bool certified = terms[blockIdx.y].certified != 0;
  const long long in_q = prefix[pb];
#pragma unroll
  for (int p = 0; p < kRangePasses; ++p) {
    int base = 0;
#pragma unroll
    for (int i = 0; i < kRangePasses * W; ++i)
      if (i < p * W + wave) base += cnt[i];
    long long pos = in_q + base + rank[p];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!((b.m[p] >> j) & 1u)) continue;
      if (certified && pos >= 0 && pos < room) rows[q_begin + pos] = (int32_t)(b.at[p] + j - b.begin);  // the guard of the store
      ++pos;
    }
  }
}

// ---- the certified range form ---------------------------------------------------------------------------------------------
// One workgroup per chunk, behind k_range_scan, in the place of k_sq8_exact_lists: certified and n_survivors of every query and
// the compact row_splits of the survivor lists, where an uncertified query has length 0.  terms[].tau is the query's threshold
// (k_sq8_exact_terms at k = 1).  L2 and a finite threshold above +0: certified, no survivor, an empty list (the head of this
// part).  terms[].certified, which k_sq8_surv_fill reads, says that the query has a list to fill.  n_q <= kScanMaxChunk <= kSq8NT.
__global__ __launch_bounds__(kSq8NT) void k_sq8_range_lists(const int32_t* __restrict__ totals, Sq8QTerms* __restrict__ terms, int n_q,
                                                            int metric, long long cap, long long* __restrict__ xsplits,
                                                            int32_t* __restrict__ out_certified,
                                                            int32_t* __restrict__ out_n_survivors) {
  __shared__ long long len[kSq8NT];
  const int tid = threadIdx.x;
  long long l = 0;
  if (tid < n_q) {
    const Sq8QTerms t = terms[tid];
    const float big = 3.402823466e+38f;
    const bool finite = fabsf(t.tau) <= big && fabsf(t.eq) <= big && fabsf(t.qhat) <= big;  // (a NaN fails every comparison)
    const bool above = metric == MT_L2 && finite && t.tau > 0.0f;
    const int total = above ? 0 : totals[tid];
    const int c = above || (t.ok != 0 && (long long)total <= cap) ? 1 : 0;
    l = c ? (long long)total : 0;
    terms[tid].certified = l > 0 ? 1 : 0;
    out_certified[tid] = c;
    out_n_survivors[tid] = total;
  }
  len[tid] = l;
  __syncthreads();
  long long sum = 0;
  for (int j = 0; j < tid; ++j) sum += len[j];
  if (tid < n_q) xsplits[tid] = sum;
  if (tid == n_q - 1) xsplits[n_q] = sum + l;
}

// range_load (nann_range.h) over a query's LIST: block blockIdx.x of the positions [begin, end) of the list buffer, the same
// 16-byte aligned walk -- the first block begins up to three positions in front of the list -- and the same match rule.
__device__ __forceinline__ size_t sq8_list_block(size_t begin) { return ((begin >> 2) + (size_t)blockIdx.x * (kRangeBlockRows / 4)) * 4; }
__device__ __forceinline__ void sq8_list_load(const float* __restrict__ scores, size_t begin, size_t end, float thr, RangeBlock* b) {
  const size_t g0 = sq8_list_block(begin) >> 2;
  b->begin = begin;
#pragma unroll
  for (int p = 0; p < kRangePasses; ++p) {
    const size_t at = (g0 + (size_t)p * kRangeNT + threadIdx.x) * 4;
    b->at[p] = at;
    b->m[p] = 0u;
    b->s[p] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    if (at < end) {  // (the 16 bytes begin inside the list or up to three positions in front of it, and end within 16 B of its end)
      b->s[p] = *reinterpret_cast<const f32x4v*>(scores + at);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float s = b->s[p][j];
        const bool in = at + j >= begin && at + j < end;
        if (in && s >= thr && s != -__builtin_inff()) b->m[p] |= 1u << j;
      }
    }
  }
}

// counts[query][block] = matches of the block of the query's list; scores: the exact scores by list position
__global__ __launch_bounds__(kRangeNT) void k_sq8_range_count(const float* __restrict__ scores, const long long* __restrict__ xsplits,
                                                              const float* __restrict__ thr, long long c0,
                                                              int32_t* __restrict__ counts) {
  __shared__ int wave_cnt[kRangeNT / 64];
  const size_t begin = (size_t)xsplits[blockIdx.y], end = (size_t)xsplits[blockIdx.y + 1];
  const size_t cb = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  if (sq8_list_block(begin) >= end) {  // (uniform over the workgroup) a block beyond the list: nothing is loaded
    if (threadIdx.x == 0) counts[cb] = 0;
    return;
  }
  RangeBlock b;
  sq8_list_load(scores, begin, end, thr[c0 + blockIdx.y], &b);
  int c = 0;
#pragma unroll
  for (int p = 0; p < kRangePasses; ++p)
#pragma unroll
    for (int j = 0; j < 4; ++j) c += __popcll(__ballot((b.m[p] >> j) & 1u));
  if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < kRangeNT / 64; ++w) t += wave_cnt[w];
    counts[cb] = t;
  }
}

// The matches of a block to their places (k_range_fill's shape).  prefix = counts behind k_range_scan; rows: the survivor lists,
// by the same positions as scores.
__global__ __launch_bounds__(kRangeNT) void k_sq8_range_fill(const float* __restrict__ scores, const long long* __restrict__ xsplits,
                                                             const int32_t* __restrict__ rows, const float* __restrict__ thr,
                                                             long long c0, const int32_t* __restrict__ prefix,
                                                             const int64_t* __restrict__ row_splits, long long capacity,
                                                             const int64_t* __restrict__ item_ids, long long n_items,
                                                             int64_t* __restrict__ out_item_ids, float* __restrict__ out_scores,
                                                             int32_t* __restrict__ out_index) {
  constexpr int W = kRangeNT / 64;
  __shared__ int cnt[kRangePasses * W];
  const size_t begin = (size_t)xsplits[blockIdx.y], end = (size_t)xsplits[blockIdx.y + 1];
  if (sq8_list_block(begin) >= end) return;  // (uniform over the workgroup)
  RangeBlock b;
  sq8_list_load(scores, begin, end, thr[c0 + blockIdx.y], &b);
  const int wave = threadIdx.x >> 6;
  int rank[kRangePasses];  // matches of the pass's wavefront in the lanes below this one
#pragma unroll
  for (int p = 0; p < kRangePasses; ++p) {
    int below = 0, all = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned long long m = __ballot((b.m[p] >> j) & 1u);
      below += range_lanes_below(m);
      all += __popcll(m);
    }
    rank[p] = below;
    if ((threadIdx.x & 63) == 0) cnt[p * W + wave] = all;
  }
  __syncthreads();
  const long long q_base = (long long)row_splits[c0 + blockIdx.y] + prefix[(size_t)blockIdx.y * gridDim.x + blockIdx.x];
#pragma unroll
  for (int p = 0; p < kRangePasses; ++p) {
    int base = 0;
#pragma unroll
    for (int i = 0; i < kRangePasses * W; ++i)
      if (i < p * W + wave) base += cnt[i];
    long long pos = q_base + base + rank[p];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!((b.m[p] >> j) & 1u)) continue;
      if (pos >= 0 && pos < capacity) {  // the guard of every store below: a position at or beyond capacity is dropped
        const int32_t r = rows[b.at[p] + j];  // (a matching position lies inside the list: a survivor's row number)
        if ((uint32_t)r < (uint32_t)n_items) {  // (always: k_sq8_surv_fill has written every position of the list)
          out_item_ids[pos] = item_ids[r];
          if (out_scores) out_scores[pos] = b.s[p][j];
          if (out_index) out_index[pos] = r;
        }
      }
      ++pos;
    }
  }
}

}  // namespace nann
#endif
