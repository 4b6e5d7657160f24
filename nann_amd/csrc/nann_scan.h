// nann_scan.h -- exhaustive search on the device (nann_search_all): every row of the index scored for a BATCH of queries,
// TopKV2 top-k per query.  The reference's test_all job (NANN_impls/main.py:194-237) one user at a time; here a row is
// fetched once for a TILE of queries.
//
// Three steps per chunk of queries (the chunk bounds the workspace: no buffer of n_queries x n_items elements exists):
//   1. scores f32[chunk, n_items]: k_scan_l2 or k_scan_ip (vector arithmetic, below), k_scan_mlp (the block functions of nann_mlp5.h on
//      the pre-projected table, identity row list) or, for the attention model (nann_search_all_model), k_scan_attn (the
//      resident block scorers of nann_attn_proj.h / nann_attn_kernels.h on the model's table; nann_scan_attn_inst.hip);
//   2. k_scan_slab_topk: the row range is cut into balanced slabs of 8192..16384 rows (wg_topk keeps that many keys in
//      registers; a corpus of at most 16384 rows is one slab); one workgroup per (query, slab) keeps the slab's top k as
//      (score, row number), TopKV2 order;
//   3. k_scan_merge: one workgroup per query, TopKV2 over the slabs' lists laid end to end in slab order.
// Why materialise + slab top-k + merge and not a fused threshold filter: wg_topk breaks ties by POSITION, and in both steps
// position order is row order -- a slab is a contiguous range of rows, a slab's list is sorted (score desc, row asc), and the
// lists are concatenated in slab order, so among equal scores a lower position is always a lower row.  A filter that appends
// through an atomic counter loses that and needs 64-bit keys and a compaction of its own; the price of this form is one
// write and one read of 4 B per (query, row), which the measured table in DESIGN.md 4.7 puts next to the scoring time.
//
// k_scan_l2, the canonical order of DESIGN.md 2 without a cross-lane instruction: ONE THREAD OWNS ONE ROW.  A chunk of 8
// elements accumulates acc = fma(t, t, acc), t = q_k - x_k, in element order from +0; the d / 8 partials are added in the
// xor-butterfly tree (strides 1, 2, 4, ...), which over chunk numbers is the balanced binary tree ((p0 + p1) + (p2 + p3)) +
// ... -- the tree fixes which partials are added, not which lane adds them, and f32 addition commutes -- so a thread walks
// the chunks in order and folds finished subtrees like a binary counter: log2(d / 8) + 1 live sums per query.  The queries
// of a tile are wave-uniform: they are read through the scalar cache from a transposed copy (element-major, so that the two
// queries of a packed f32 operation are neighbours) and never occupy a vector register; a row's 8 elements are converted to
// f32 once per chunk and serve the whole tile (q - f32(x) has the bits of the v_fma_mix_f32 form: the widening is exact).
// Rows reach their threads through LDS: a workgroup stages 256 rows x 128 bytes per panel with coalesced 16-byte loads.
#pragma once
#include <cstddef>

#include "nann_filter.h"
#include "nann_predicate.h"
#include "nann_range.h"
#include "nann_search.h"
#include "nann_wide.h"

namespace nann {

// a filtered call (nann_search_all_filtered): the filter, where the merge's k-wide lists of a chunk are staged -- item ids
// i64[chunk, k], scores f32[chunk, k], rows i32[chunk, k] -- and the counts of the final rows
struct ScanFilter {
  FilterArgs f;
  unsigned char* stage;
  int32_t* n_out;  // i32[n_queries] or null
  const PredArgs* pred;  // null: none.  Else the attribute predicates of the call (nann_predicate.h): k_pred_scatter behind the
                         // filter's scatters, and k_pred_compact in the place of k_filter_compact
};
inline size_t scan_filter_stage_bytes(int chunk, int k) { return ((size_t)chunk * k * 16 + 255) & ~(size_t)255; }

// ---- launchers (nann_scan_inst.hip) -----------------------------------------------------------------------------------
struct ScanArgs {
  const void* emb;          // L2, inner product: the index's rows
  const float* proj;        // MLP: the pre-projected table of (scorer, index)
  const int64_t* item_ids;
  long long n_items;
  int d, dt;
  int kind, exact;          // nann_scorer_kind or kScanAttn; MLP / attention: the exact f32 form (also the MLP's certified precision) or split-f16
  MlpParams mlp;
  int mlp_workgroups;       // resident workgroups of k_scan_mlp / k_scan_attn (one per CU)
  AttnParams attn;          // kScanAttn: the model; `proj` is its table, and launch_scan's `q` the users' sequences
                            // f16[n_queries, attn.L, kAttnE], from which each chunk's kt / upad are prepared into the workspace
  const ScanFilter* filter; // null: the unfiltered call.  Else -inf over the denied scores of every chunk before the slab top-k
                            // (nann_filter.h), and k_filter_compact behind the merge writes the outputs
  const ScanRange* range;   // null: the top k.  Else the range form (nann_range.h): every row at or above the query's cut, in the
                            // place of the slab top-k and the merge; of a filter only `f` is read, and the call's k not at all
  const ScanWide* wide;     // null: the slab top-k and the merge.  Else the wide form (nann_wide.h): cut, gather and sort in their
                            // place, for k up to kWideMaxK; of a filter only `f` and `pred` are read (their scatters), and the
                            // layout is the one of k = 0
};
constexpr int kScanAttn = 100;  // ScanArgs::kind of the attention model (no nann_scorer_kind: it has a handle type of its own)
constexpr size_t kScanAttnUserBytes = (size_t)(256 * kAttnLP + kAttnLP * kAttnE) * 4;  // kt 64 KB + upad 16 KB (nann_attn_prepare)
// dynamic LDS of a 512-thread workgroup that runs the resident attention block scorers (k_scan_attn, k_cand_score_attn)
constexpr int kScanAttnSplitLds = 65536 + kAttnSplitScratch;      // keys + [W2 | vectors | resident fragments]
constexpr int kScanAttnExactLds = 65536 + kAttnXResFloats * 4;    // keys f32 [256][64] + [upad | W1a | W2 | W3]
static_assert(kScanAttnSplitLds <= 160 * 1024 && kScanAttnExactLds <= 160 * 1024, "one workgroup per CU");
// workspace layout of a call: [scores chunk x n_items | cand scores | cand rows | qT, u or kt + upad]; chunk = queries scored per pass
struct ScanLayout {
  int chunk, n_slabs;
  size_t off_scores, off_cand_scores, off_cand_rows, off_q, total;
};
ScanLayout scan_layout(long long n_items, int d, int kind, long long n_queries, int k);
int launch_scan(const ScanArgs& a, const ScanLayout& L, const float* q, long long n_queries, int k, unsigned char* ws,
                int64_t* out_item_ids, float* out_scores, int32_t* out_index, hipStream_t st);
// scores f32[n_q, n_items] of the attention model for the users whose kt / upad lie one after the other (nann_scan_attn_inst.hip)
int launch_scan_attn(const ScanArgs& a, const float* kt, const float* upad, int n_q, float* scores, hipStream_t st);

}  // namespace nann

#ifdef NANN_SCAN_IMPL  // the kernels: nann_scan_inst.hip only (nann_flat.hip takes the declarations above)
namespace nann {

constexpr int kScanRows = 256;          // rows per workgroup of k_scan_l2 = its threads
constexpr int kScanPanelBytes = 128;    // bytes of a row staged per panel
constexpr int kScanRowStride = kScanPanelBytes + 16;  // LDS row stride: 9 x 16 bytes, odd -> ds_read_b128 without bank conflicts
constexpr int kScanSlabRows = 16384;    // most rows of a slab (kTopkEPT * kNT: wg_topk's keys stay in registers)
constexpr int kScanMlpRows = 4096;      // rows of a work item of k_scan_mlp
constexpr int kScanMaxChunk = 128;      // most queries scored per chunk

// queries per tile of k_scan_l2: (log2(d / 8) + 1) * 16 accumulators and 16 differences stay in registers
constexpr int kScanTileQueries = 16;
// wavefronts per SIMD k_scan_l2 is compiled for: 128 registers up to d = 128, 168 beyond (four 36 KB workgroups fit a CU's LDS)
__host__ __device__ constexpr int scan_waves(int lpr) { return lpr <= 16 ? 4 : 3; }

// slab s of n_slabs covers rows [slab_begin(s), slab_begin(s + 1)): balanced, so that every slab of a corpus cut in two or more
// holds at least kScanSlabRows / 2 >= kMaxK rows (a slab's list is then always k long)
__host__ __device__ inline long long scan_slab_begin(long long n_items, int n_slabs, int s) {
  return n_items * (long long)s / n_slabs;
}
inline int scan_n_slabs(long long n_items) { return (int)((n_items + kScanSlabRows - 1) / kScanSlabRows); }

// qT[tile][e][i] = q[tile * TQ + i][e] (queries behind n_q: the last one again; their scores are not stored)
__global__ __launch_bounds__(256) void k_scan_transpose_q(const float* __restrict__ q, int n_q, int d, int tq,
                                                          float* __restrict__ qT) {
  const long long total = (long long)((n_q + tq - 1) / tq) * d * tq;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int in_tile = (int)(i % tq);
    const int e = (int)((i / tq) % d);
    const long long tile = i / ((long long)tq * d);
    const long long qi = min(tile * tq + in_tile, (long long)n_q - 1);
    qT[i] = q[qi * d + e];
  }
}

// METRIC = MT_IP (k_scan_ip): the chunk accumulates acc = fma(q_k, x_k, acc) instead, in the same order and the same tree.
template <int LPR, int DT, int TQ, int METRIC = MT_L2>
struct ScanL2 {
  static constexpr int NP = TQ / 2;                         // packed pairs of queries
  static constexpr int PJ = DT == DT_F32 ? 4 : 8;           // chunks of 8 elements per 128-byte panel
  static constexpr int D = LPR * 8;
  static constexpr int kRowBytes = D * (DT == DT_F32 ? 4 : 2);
  static_assert(LPR % PJ == 0, "whole panels");

  const unsigned char* table;
  long long n_items, row0;
  const f32x2* qt;  // this tile's queries: [D][NP] pairs
  unsigned char* lds;

  // rows row0 .. row0 + 255, bytes [panel * 128, +128) of each, into LDS: 8 coalesced 16-byte loads per thread, held in
  // eight NAMED registers across the barrier (an indexed array of HIP's uint4 was left in private memory by hipcc: every
  // staged byte went through scratch; the build refuses a k_scan_l2 with a scratch frame, build.py)
  __device__ __forceinline__ u32x4v stage_load(int panel, int i) const {
    const int g = i * kScanRows + (int)threadIdx.x, r = g >> 3, p = g & 7;
    const long long row = min(row0 + r, n_items - 1);
    return *reinterpret_cast<const u32x4v*>(table + (size_t)row * kRowBytes + panel * kScanPanelBytes + p * 16);
  }
  __device__ __forceinline__ void stage_store(int i, u32x4v v) const {
    const int g = i * kScanRows + (int)threadIdx.x, r = g >> 3, p = g & 7;
    *reinterpret_cast<u32x4v*>(lds + r * kScanRowStride + p * 16) = v;
  }
  __device__ __forceinline__ void stage(int panel) const {
    const u32x4v v0 = stage_load(panel, 0), v1 = stage_load(panel, 1), v2 = stage_load(panel, 2), v3 = stage_load(panel, 3);
    const u32x4v v4 = stage_load(panel, 4), v5 = stage_load(panel, 5), v6 = stage_load(panel, 6), v7 = stage_load(panel, 7);
    __syncthreads();  // (the panel before this one has been consumed)
    stage_store(0, v0); stage_store(1, v1); stage_store(2, v2); stage_store(3, v3);
    stage_store(4, v4); stage_store(5, v5); stage_store(6, v6); stage_store(7, v7);
    __syncthreads();
  }

  // element e of the tile's queries, through the scalar cache (wave-uniform address)
  __device__ __forceinline__ void load_q(int e, f32x2 (&qv)[NP]) const {
#pragma unroll
    for (int p = 0; p < NP; ++p) qv[p] = qt[e * NP + p];
  }

  __device__ __forceinline__ float load_x(const unsigned char* at, int k) const {
    if constexpr (DT == DT_F32) return *reinterpret_cast<const float*>(at + 4 * k);
    else if constexpr (DT == DT_F16) return half_bits_to_float(*reinterpret_cast<const uint16_t*>(at + 2 * k));
    else return bf16_bits_to_float(*reinterpret_cast<const uint16_t*>(at + 2 * k));
  }

  // chunk J of this thread's row against every query of the tile: out[p] = the pair's partial sums.  The loop over the
  // chunk's elements is ROLLED on purpose: unrolled, every scalar load of the body was hoisted to the head of the kernel
  // (thousands of spilled scalar registers) and d = 512 overflowed the instruction cache.  Per element: the subtractions
  // consume the queries (scalar registers) and the row element, THEN the next element's queries and row element are
  // requested, THEN the fmas run with those loads in flight -- scalar loads return out of order, so a wait for them is always
  // a wait for all of them, and the only place for it is the head of the next element.  qn holds element 8 J of the queries on
  // entry and element 8 (J + 1) on return.
  template <int J>
  __device__ __forceinline__ void partial(f32x2 (&out)[NP], f32x2 (&qn)[NP]) const {
    if constexpr (J % PJ == 0) stage(J / PJ);
    constexpr int kElem = DT == DT_F32 ? 4 : 2;
    const unsigned char* at = lds + threadIdx.x * kScanRowStride + (J % PJ) * 8 * kElem;
#pragma unroll
    for (int p = 0; p < NP; ++p) out[p] = f32x2{0.0f, 0.0f};
    float x = load_x(at, 0);
#pragma unroll 1
    for (int k = 0; k < 8; ++k) {
      const f32x2 xk = f32x2{x, x};
      f32x2 t[NP];  // L2: the differences.  Inner product: the queries themselves, moved aside (scalar registers) while the next ones load
#pragma unroll
      for (int p = 0; p < NP; ++p) t[p] = METRIC == MT_IP ? qn[p] : qn[p] - xk;
      __builtin_amdgcn_sched_barrier(0);
      const int e = J * 8 + k + 1;
      load_q(e < D ? e : 0, qn);
      x = load_x(at, k + 1);  // (k = 7: the next chunk's first element or the row's padding; not used)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int p = 0; p < NP; ++p) out[p] = __builtin_elementwise_fma(t[p], METRIC == MT_IP ? xk : t[p], out[p]);
    }
  }

  // the butterfly's subtree over chunks [J0, J0 + N)
  template <int N, int J0>
  __device__ __forceinline__ void tree(f32x2 (&out)[NP], f32x2 (&qn)[NP]) const {
    if constexpr (N == 1) {
      partial<J0>(out, qn);
    } else {
      tree<N / 2, J0>(out, qn);
      f32x2 other[NP];
      tree<N / 2, J0 + N / 2>(other, qn);
      // (the empty asm pins a sum where it is formed: left alone, the compiler sinks every addition of the tree into the
      //  guarded stores at the kernel's end and keeps all d / 8 partials of every query alive until then -- in scratch)
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        out[p] = out[p] + other[p];
        asm volatile("" : "+v"(out[p]));
      }
    }
  }
};

// grid: (tiles of TQ queries) x (blocks of 256 rows), the tile index fastest -- the workgroups that run together share rows.
// scores f32[n_q, n_items].
template <int LPR, int DT, int TQ, int METRIC>
__device__ __forceinline__ void scan_rows(unsigned char* rows, const void* __restrict__ table, long long n_items,
                                          const float* __restrict__ qT, int n_q, int n_tiles, float* __restrict__ scores) {
  typedef ScanL2<LPR, DT, TQ, METRIC> S;
  const int tile = (int)(blockIdx.x % (unsigned)n_tiles);
  S s;
  s.table = static_cast<const unsigned char*>(table);
  s.n_items = n_items;
  s.row0 = (long long)(blockIdx.x / (unsigned)n_tiles) * kScanRows;
  s.qt = reinterpret_cast<const f32x2*>(qT + (size_t)tile * S::D * TQ);
  s.lds = rows;
  f32x2 sum[S::NP], qn[S::NP];
  s.load_q(0, qn);
  s.template tree<LPR, 0>(sum, qn);
  const long long row = s.row0 + threadIdx.x;
  if (row >= n_items) return;
#pragma unroll
  for (int p = 0; p < S::NP; ++p) {
    const int qi = tile * TQ + 2 * p;
    if (qi < n_q) scores[(size_t)qi * n_items + row] = METRIC == MT_IP ? sum[p].x : 0.0f - sum[p].x;
    if (qi + 1 < n_q) scores[(size_t)(qi + 1) * n_items + row] = METRIC == MT_IP ? sum[p].y : 0.0f - sum[p].y;
  }
}

template <int LPR, int DT, int TQ>
__global__ __launch_bounds__(kScanRows) __attribute__((amdgpu_waves_per_eu(scan_waves(LPR), scan_waves(LPR)))) void k_scan_l2(const void* __restrict__ table, long long n_items,
                                                       const float* __restrict__ qT, int n_q, int n_tiles,
                                                       float* __restrict__ scores) {
  __shared__ __attribute__((aligned(16))) unsigned char rows[kScanRows * kScanRowStride];
  scan_rows<LPR, DT, TQ, MT_L2>(rows, table, n_items, qT, n_q, n_tiles, scores);
}

// the inner-product scan: scores[q][row] = <q, row>, everything else as k_scan_l2
template <int LPR, int DT, int TQ>
__global__ __launch_bounds__(kScanRows) __attribute__((amdgpu_waves_per_eu(scan_waves(LPR), scan_waves(LPR)))) void k_scan_ip(const void* __restrict__ table, long long n_items,
                                                       const float* __restrict__ qT, int n_q, int n_tiles,
                                                       float* __restrict__ scores) {
  __shared__ __attribute__((aligned(16))) unsigned char rows[kScanRows * kScanRowStride];
  scan_rows<LPR, DT, TQ, MT_IP>(rows, table, n_items, qT, n_q, n_tiles, scores);
}

// u[q][j] = b1[j] + sum_k q[k] W1[k][j]: the query's part of layer 1, once per query (what stage 0 of the pipeline of phases
// keeps in PhaseState.u)
__global__ __launch_bounds__(256) void k_scan_mlp_u(MlpParams P, const float* __restrict__ q, float* __restrict__ u) {
  __shared__ float qv[256];
  for (int k = threadIdx.x; k < P.d; k += 256) qv[k] = q[(size_t)blockIdx.x * P.d + k];
  __syncthreads();
  const float v = wg_mlp_query_u<256>(P, qv);
  if ((int)threadIdx.x < P.h1) u[(size_t)blockIdx.x * 256 + threadIdx.x] = v;
}

// The MLP on the pre-projected table over every row: W2 resident in LDS for the whole launch (one workgroup per CU), work
// items = (block of kScanMlpRows rows, query), the query fastest, so that the workgroups that run together read the same
// block of the table; an item is one call of wg_score_mlp_xres / wg_score_mlp_res with the identity row list.
template <bool EXACT>
__global__ __launch_bounds__(512) void k_scan_mlp(MlpParams P, const float* __restrict__ proj, long long n_items,
                                                  const float* __restrict__ u, int n_q, float* __restrict__ scores) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NT = 512;
  uint4* W2 = reinterpret_cast<uint4*>(smem);
  Mlp2Vectors* V = reinterpret_cast<Mlp2Vectors*>(smem + kMlpResW2Bytes);
  const int tid = threadIdx.x;
  const uint4* src = EXACT ? reinterpret_cast<const uint4*>(P.p2x) : P.p2;
  for (int i = tid; i < kMlpResW2Vec; i += NT) W2[i] = src[i];
  if (EXACT) wg_mlp_xres_vectors<NT>(P, 0.0f, V); else wg_mlp_res_vectors<NT>(P, 0.0f, V);
  const long long n_blocks = (n_items + kScanMlpRows - 1) / kScanMlpRows;
  const long long n_work = n_blocks * n_q;
  for (long long w = blockIdx.x; w < n_work; w += gridDim.x) {
    const int qi = (int)(w % n_q);
    const long long r0 = (w / n_q) * kScanMlpRows;
    const int n = (int)min((long long)kScanMlpRows, n_items - r0);
    __syncthreads();  // (every wavefront has left the item before: its u may go)
    if (tid < 256) V->u[tid] = EXACT ? u[(size_t)qi * 256 + tid] : u[(size_t)qi * 256 + tid] * kSplit2Scale;
    __syncthreads();
    float* out = scores + (size_t)qi * n_items + r0;
    if (EXACT) wg_score_mlp_xres<NT>(proj + (size_t)r0 * kMlpProjWidth, (uint32_t)n, nullptr, n, reinterpret_cast<const float4*>(W2), V, out);
    else wg_score_mlp_res<NT>(proj + (size_t)r0 * kMlpProjWidth, (uint32_t)n, nullptr, n, W2, V, out);
  }
}

// one workgroup per (slab, query): TopKV2 over the slab's scores, positions turned into row numbers.  cand_* [n_q][n_slabs][k]
// (a slab's list is always k long: a lone slab holds n_items >= k rows, one of several at least kScanSlabRows / 2 >= kMaxK).
__global__ __launch_bounds__(kNT) void k_scan_slab_topk(const float* __restrict__ scores, long long n_items, int n_slabs, int k,
                                                        float* __restrict__ cand_scores, int32_t* __restrict__ cand_rows) {
  __shared__ __attribute__((aligned(16))) unsigned char scratch[sizeof(TopkScratch)];
  const int s = (int)(blockIdx.x % (unsigned)n_slabs);
  const long long qi = blockIdx.x / (unsigned)n_slabs;
  const long long b = scan_slab_begin(n_items, n_slabs, s), e = scan_slab_begin(n_items, n_slabs, s + 1);
  const size_t at = ((size_t)qi * n_slabs + s) * k;
  wg_topk(nullptr, scores + (size_t)qi * n_items + b, nullptr, (int)(e - b), k, cand_rows + at, nullptr, cand_scores + at,
          nullptr, nullptr, scratch);
  __syncthreads();
  for (int i = threadIdx.x; i < k; i += kNT) cand_rows[at + i] += (int32_t)b;
}

// one workgroup per query: TopKV2 over the slabs' lists in slab order; row numbers and item ids ride along
__global__ __launch_bounds__(kNT) void k_scan_merge(const float* __restrict__ cand_scores, const int32_t* __restrict__ cand_rows,
                                                    int n_in, int k, const int64_t* __restrict__ item_ids,
                                                    int64_t* __restrict__ out_item_ids, float* __restrict__ out_scores,
                                                    int32_t* __restrict__ out_index) {
  __shared__ __attribute__((aligned(16))) unsigned char scratch[sizeof(TopkScratch)];
  const size_t qi = blockIdx.x;
  wg_topk(cand_rows + qi * n_in, cand_scores + qi * n_in, nullptr, n_in, k, nullptr, out_index ? out_index + qi * k : nullptr,
          out_scores ? out_scores + qi * k : nullptr, item_ids, out_item_ids + qi * k, scratch);
}

}  // namespace nann
#endif
