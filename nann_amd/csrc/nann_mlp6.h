// nann_mlp6.h -- the MLP traversal as a PIPELINE OF PHASES (round 4): scoring in a kernel of its own.
//
// The fused traversal with the MLP scorer (nann_mlp5.h inside k_search) keeps the matrix pipe 0.41 busy: 0.54 inside the
// scoring calls, and 18 % of a query -- expand, top-k -- with the pipe idle, because the scorer's 256 registers and
// 137 KB of LDS allow ONE workgroup per CU, so nothing runs beside a query's latency-bound phases.  Both halves do better
// apart:
//   * the traversal stages (top-k of the last round, marks, expand of the next: search_one between two scoring calls) are
//     the L2 kernel's code at its occupancy -- two 512-thread workgroups per CU, 64 KB set + 11 KB scratch each -- so
//     one query's dependent HBM / LDS trips hide behind another's;
//   * the scoring of ALL queries' candidate lists of a round is one launch of k_mlp_phase_score: W2 loaded into LDS once
//     per workgroup for the whole launch (no per-call reload, no set to park), the 32-row blocks of every query laid end
//     to end and cut into 2048 equal runs, one per wavefront -- no ragged last blocks per call, no barrier anywhere.
// Per 1024-query chunk: 6 traversal launches and 5 scoring launches (each works out the blocks of every query -> their
// prefix sums for itself); state between launches lives in the query's slot (PhaseState, the candidate arrays the
// fused kernel uses anyway, the set parked in the slot's bitmap region around rounds 2 and 3).  Results are what the
// fused kernel computes: the same building blocks run on the same lists (exact precision: bit-identical to the oracle).
#pragma once
#include "nann_mlp5.h"

namespace nann {

constexpr int kPhaseChunk = 1024;     // queries per pipeline pass (one prefix workgroup, bounded workspace)
constexpr int kPhasePending = -100;   // PhaseState.status while a query waits for its scores
constexpr int kPhaseSkip = -101;      // search_one's return for a query an earlier stage finished (never stored)
constexpr int kPhaseScoreWaves = 2048;  // 256 workgroups x 8 wavefronts: runs of the scoring launch

// what a query carries from one launch to the next (in its slot)
struct PhaseState {
  int status;     // kPhasePending | final nann_status
  int r;          // the round whose scoring call is pending
  int sc_n;       // rows of that call
  int base_off;   // they are cand_ids[base_off ..] (r == 0: the index's enter points), scores to cand_scores[base_off ..]
  int nP;         // pool size so far
  int vis_count;  // ids in the parked set
  int ctr[3 * NANN_NUM_ROUNDS];
  int ref_n;      // certified form: rows of the pending round the refine launch rescores exactly (k_mlp_phase_certify)
  int ref_list;   //   1: they are listed (raw region of the slot), 0: all sc_n rows
  int pad[9];
  float u[256];   // b1 + W1q^T q: the query's part of layer 1, computed once (stage 0)
};
static_assert(sizeof(PhaseState) == 128 + 1024, "PhaseState layout");

struct PhaseScoreArgs {
  unsigned char* ws;            // the search workspace: [header | slots]
  unsigned long long slot_bytes;
  unsigned long long off_cand_ids, off_cand_scores, off_state;  // within a slot
  const int32_t* enter;
  const float* proj;            // the pre-projected table
  uint32_t n_items;
  int n_queries;
  int round;
  MlpParams mlp;
  // certified form only (k_mlp_phase_certify and the filter / refine instances of k_mlp_phase_score)
  unsigned long long off_raw;   // the slot's raw region: the filter's bounds, then the certify step's survivor list
  int max_raw;                  // its capacity in 4-byte entries
  int t_r;                      // level_topn[round] of the launch (tq: per query)
  const int32_t* tq;
  unsigned long long* refined;  // WsHeader::refined[NANN_NUM_ROUNDS]
};

// ---------------------------------------------------------------------------------------------------------------
// The certified form (NANN_MLP_CERTIFIED): a round is scored by THREE launches, and its selection then runs as usual.
//   filter   (k_mlp_phase_score CERT = 2) every row: an approximate score s~ and a bound B >= |s~ - s|, s = the exact
//            form's score of the row (bit for bit the oracle's); s~ to cand_scores, B to the slot's raw region
//   certify  (k_mlp_phase_certify) per query: L = the k-th largest lower bound s~ - B of the round's selection input
//            (k = level_topn[round]; round 1's carried beam entries are exact: lo = hi = their score); a row survives
//            unless s~ + B < L; non-survivors get -inf in cand_scores, survivors are listed in the raw region
//   refine   (k_mlp_phase_score CERT = 1) the exact form's arithmetic over the listed rows, scores to their places
// Why the selection is the exact form's: at least k entries have lo >= L, so at least k survivors score >= L -- strictly
// above every non-survivor's exact score (<= its hi < L) and above -inf.  TopKV2 therefore takes the same entries in the
// same order (ties break on position, which nothing moves), and every selected score is an exact one.  One pass per
// selection suffices because whatever a later round reads (beam, pool) was selected, hence exact.
//
// The filter is the exact form's front end on the split form's operands: h1 = PReLU(u + P) computed with the same f32
// operations on operands x 2^7 (powers of two: 2^7 h1 exactly), converted to f16 with ROUND TO NEAREST (v_fma_mix: an
// overflow is inf, never a clamped 65504), times the f16 hi plane of W2 x 2^7 (pack_split_weights) in ONE
// v_mfma_f32_32x32x16_f16 per fragment -- no lo planes: a third of the split form's matrix work -- then layer 2's PReLU and
// the output layer in f32.  The bound, with u = 2^-24, u16 = 2^-11, gamma_n = n u / (1 - n u), gamma'_n the same with 2u
// (the matrix core's order and rounding of its f32 sums are not specified: 2u per add), T_m = b2_m + sum_j W2_jm h_j
// (real arithmetic on the exact form's f32 h_j), A_m = |b2_m| + sum_j w_jm |h_j|, M_m = max(1, |alpha2_m|):
//   operands   |f16(2^7 h_j) - 2^7 h_j| <= u16 |2^7 h_j| + eta (eta = 2^-13 covers an f16 result or input flushed to zero
//              and the f32 subnormal rounding of the x 2^7 operands); the W2 plane's error e_jm is known on the host
//              exactly (a subnormal f16 counted as possibly flushed); w_jm = |W2_jm| + max(0, e_jm - u16 |W2_jm|) / u16
//              widens an entry only where e_jm is not within u16 relative (f16 subnormals)
//   layer 2    exact form: a 257-term fmaf chain, |E_m - T_m| <= gamma_257 A_m; filter: products of f16 are exact in f32,
//              |F_m - T_m| <= [u16 (2 + u16) + gamma'_257 (1 + u16)^2] sum_j w_jm |h_j| + gamma'_257 |b2_m| + zeta Omega_m,
//              zeta = eta 2^-7 (1 + gamma'_257)(1 + u16), Omega_m = sum_j w_jm.  So D_m = |F_m - E_m| <= a1 A_m + zeta Omega_m,
//              a1 = u16 (2 + u16) + gamma'_257 (1 + u16)^2 + gamma_257
//   output     exact form: y = fl(alpha2 x) or x, a <= 129-term chain: u M_m |E_m| + gamma_129 (1 + u) M_m |E_m|;
//              filter: y = x + fl(alpha2 - 1) min(x, 0) (<= 3u (1 + u) M_m |x|), the same chain length; PReLU is
//              M_m-Lipschitz.  With |E_m| <= (1 + gamma_257) A_m and |F_m| <= |E_m| + D_m:
//   |s~ - s| <= K1 sum_j |h_j| c_j + K0,  c_j = sum_m w_jm |w3_m| M_m,
//     K1 = a1 + [3u(1 + u) + gamma_129 (1 + 3u(1 + u))](1 + gamma_257 + a1) + [u + gamma_129 (1 + u)](1 + gamma_257)
//     K0 = K1 sum_m |w3_m| M_m |b2_m| + 2 zeta sum_j c_j
// (about 1.03e-3 per unit of sum_j |h_j| c_j).  The host (certified_bound, nann_scorers.hip) evaluates it in double and stores
// K1 2^-7 (the kernel sums |2^7 h_j|), K0 and c_j rounded up, with 1e-3 of margin for the f32 evaluation of B; the kernel
// then widens B by 2^-20 (|s~| + B) so that s~ -/+ B stay bounds after their own rounding.  Overflow anywhere -- h1 beyond
// f16, W2 beyond f16 (|w| > 511), b2 or alpha2 large enough that an f32 value of the exact form overflows (the filter's
// are x 2^14 larger) -- leaves a non-finite s~ or B, and such a row gets B = +inf: it is always refined.  No precondition
// on the weights.
//
// Vectors of the filter: u x 2^7 per wavefront (as split), c_j in the vectors' u slot, alpha1 (the exact form's PReLU),
// b2 x 2^14, alpha2 - 1, w3.
template <int NT>
__device__ __forceinline__ void mlp_filter_vectors(const MlpParams& P, Mlp2Vectors* V) {
  const int tid = local_tid();
  static_assert(NT >= 256, "one hidden unit per thread");
  if (tid < 256) {
    V->u[tid] = P.cb[tid];
    V->beta1[tid] = P.alpha1[tid];
  }
  if (tid < 128) {
    V->b2[tid] = P.b2[tid] * (kSplit2Scale * kSplit2Scale);
    V->beta2[tid] = P.alpha2[tid] - 1.0f;
    V->w3[tid] = P.w3[tid];
  }
}

// One launch scores the pending candidate lists of every query of the chunk.  256 workgroups x 8 wavefronts; wavefront
// gw takes blocks [gw T / 2048, (gw + 1) T / 2048) of the T blocks laid end to end.  EXACT: f32 MFMA on the table
// (wg_score_mlp_xres's arithmetic), else split-f16 (wg_score_mlp_res's).
// CERT (the certified form, NANN_MLP_CERTIFIED; see the filter's comment below): 1 = EXACT over the rows the certify step
// kept (PhaseState.ref_n, listed in the raw region when ref_list), scores scattered to their places; 2 = the f16 filter.
template <bool EXACT, int CERT = 0>
__global__ __launch_bounds__(512, 2) void k_mlp_phase_score(PhaseScoreArgs a) {
  static_assert(CERT == 0 || (CERT == 1) == EXACT, "refine: exact f32; filter: f16");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int H1T = 8, H2T = 4, NT = 512;
  // LDS: [W2 128 KB | beta1 b2 beta2 w3 (Mlp2Vectors without u) | per-wavefront u: 8 x 1 KB | block prefix]
  uint4* W2 = reinterpret_cast<uint4*>(smem);
  Mlp2Vectors* V = reinterpret_cast<Mlp2Vectors*>(smem + kMlpResW2Bytes);
  float* u_all = reinterpret_cast<float*>(smem + kMlpResBytes);
  int* prefix = reinterpret_cast<int*>(smem + kMlpResBytes + 8 * 1024);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cand = lane & 31, g = lane >> 5;
  // the 32-row blocks every pending query contributes to this round, as exclusive prefix sums in query order: every
  // workgroup works them out for itself from the queries' PhaseState (two queries per thread; round 4's first form had
  // a launch of its own for this -- 5 of a chunk's 17 launches, 24 us of a 32-query call's 308)
  static_assert(kPhaseChunk == 2 * NT, "two queries per thread");
  uint32_t* wave_tot = reinterpret_cast<uint32_t*>(prefix + kPhaseChunk + 4);
  uint32_t nb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int q = 2 * tid + h;
    nb[h] = 0;
    if (q < a.n_queries) {
      const PhaseState* st = reinterpret_cast<const PhaseState*>(a.ws + 256 + (unsigned long long)q * a.slot_bytes + a.off_state);
      if (st->status == kPhasePending && st->r == a.round) nb[h] = (uint32_t)((CERT == 1 ? st->ref_n : st->sc_n) + 31) >> 5;
    }
  }
  const uint32_t inc = wave_scan_add(nb[0] + nb[1]);
  if (lane == 63) wave_tot[wave] = inc;
  {  // once per launch: the weights and the vectors that do not depend on the query
    const uint4* src = EXACT ? reinterpret_cast<const uint4*>(a.mlp.p2x) : a.mlp.p2;
    for (int i = tid; i < kMlpResW2Vec; i += NT) W2[i] = src[i];
    if (EXACT) wg_mlp_xres_vectors<NT>(a.mlp, 0.0f, V);
    else if (CERT == 2) mlp_filter_vectors<NT>(a.mlp, V);
    else wg_mlp_res_vectors<NT>(a.mlp, 0.0f, V);
  }
  __syncthreads();
  int total = 0;
  {
    uint32_t base = 0, tot = 0;
    for (int w = 0; w < NT / 64; ++w) {
      const uint32_t t = wave_tot[w];
      if (w < wave) base += t;
      tot += t;
    }
    total = (int)tot;
    const uint32_t excl = base + inc - (nb[0] + nb[1]);
    prefix[2 * tid] = (int)excl;
    prefix[2 * tid + 1] = (int)(excl + nb[0]);
    if (tid == 0) prefix[kPhaseChunk] = total;  // (queries behind n_queries contribute nothing: prefix[n_queries ..] = total)
  }
  __syncthreads();
  if (total == 0) return;
  const int gw = (int)blockIdx.x * (NT / 64) + wave;
  const int nw = (int)gridDim.x * (NT / 64);
  const int b_lo = (int)((long long)total * gw / nw), b_hi = (int)((long long)total * (gw + 1) / nw);
  if (b_lo >= b_hi) return;
  float* u_w = u_all + wave * 256;  // this wavefront's copy of the current query's u

  // the query of block b (prefix[q] <= b < prefix[q + 1]); uniform over the wavefront
  auto query_of = [&](int b) {
    int lo = 0, hi = a.n_queries - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (prefix[mid] <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
  };
  // a query's u into the wavefront's LDS copy (the split form keeps it x 2^7 like the table; exact powers of two)
  auto load_u_of = [&](const PhaseState* st) {
    float4 v = reinterpret_cast<const float4*>(st->u)[lane];
    if constexpr (!EXACT) { v.x *= kSplit2Scale; v.y *= kSplit2Scale; v.z *= kSplit2Scale; v.w *= kSplit2Scale; }
    reinterpret_cast<float4*>(u_w)[lane] = v;
  };
  struct Cur {  // the query the wavefront is in
    int q, first, n;
    const int32_t* ids;
    float* out;
    const int32_t* list;  // CERT == 1: row i of the launch is row list[i] of the round (nullptr: row i)
    float* bnd;           // CERT == 2: where the bounds go (nullptr: the round's rows do not fit the raw region)
  };
  auto enter_query = [&](int q, Cur& c, bool load_u) {
    unsigned char* slot = a.ws + 256 + (unsigned long long)q * a.slot_bytes;
    const PhaseState* st = reinterpret_cast<const PhaseState*>(slot + a.off_state);
    c.q = q;
    c.first = prefix[q];
    c.n = CERT == 1 ? st->ref_n : st->sc_n;
    const int off = st->base_off;
    c.ids = a.round == 0 ? a.enter : reinterpret_cast<const int32_t*>(slot + a.off_cand_ids) + off;
    c.out = reinterpret_cast<float*>(slot + a.off_cand_scores) + off;
    c.list = (CERT == 1 && st->ref_list) ? reinterpret_cast<const int32_t*>(slot + a.off_raw) : nullptr;
    c.bnd = (CERT == 2 && st->sc_n <= a.max_raw) ? reinterpret_cast<float*>(slot + a.off_raw) : nullptr;
    if (load_u) load_u_of(st);
  };
  auto row_ptr = [&](const Cur& c, int b) -> const float* {
    int i = min((b - c.first) * 32 + cand, c.n - 1);
    if (CERT == 1 && c.list != nullptr) i = c.list[i];
    const uint32_t rid = (uint32_t)c.ids[i];
    return a.proj + (size_t)(rid < a.n_items ? rid : 0u) * kMlpProjWidth + 4 * g;
  };
  auto load_tile = [&](const float* row, int t, float4 (&p)[4]) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) p[rr] = *reinterpret_cast<const float4*>(row + 32 * t + 8 * rr);
  };
  // LDS bases (byte addresses), opaque: every read is `base + immediate` (nann_mlp5.h)
  uint32_t w_lo = lds_offset_of(W2) + (uint32_t)lane * 16u;
  uint32_t w_hi = w_lo + 65536u;
  uint32_t v_at = lds_offset_of(V) + (uint32_t)g * 16u;
  uint32_t u_at = lds_offset_of(u_w) + (uint32_t)g * 16u;
  asm volatile("" : "+v"(w_lo), "+v"(w_hi), "+v"(v_at), "+v"(u_at));
  auto vec4 = [&](int float_index) -> f32x4v { return *reinterpret_cast<lds_f4_ptr>(v_at + 4 * float_index); };
  auto uvec4 = [&](int float_index) -> f32x4v { return *reinterpret_cast<lds_f4_ptr>(u_at + 4 * float_index); };
  constexpr int kBeta1 = 256, kB2 = 512, kBeta2 = 640, kW3 = 768;  // Mlp2Vectors, in floats

  if constexpr (CERT == 2) {
    // ---- the certified form's filter (comment above mlp_filter_vectors): one f16 product per fragment, tile by tile
    Cur cur, nxt;
    enter_query(query_of(b_lo), cur, true);
    const float* row = row_ptr(cur, b_lo);
    float4 x[2][4];
    load_tile(row, 0, x[0]);
    load_tile(row, 1, x[1]);
    constexpr int kC = 0;  // c_j, in the place of the fused kernel's per-workgroup u (this launch keeps one u per wavefront)
    for (int b = b_lo; b < b_hi; ++b) {
      nxt = cur;
      bool change = false;
      if (b + 1 < b_hi && b + 1 >= prefix[cur.q + 1]) {
        int q2 = cur.q + 1;
        while (prefix[q2 + 1] <= b + 1) ++q2;  // (queries without blocks)
        enter_query(q2, nxt, false);
        change = true;
      }
      const float* next = (b + 1 < b_hi) ? row_ptr(nxt, b + 1) : row;
      const int i = (b - cur.first) * 32 + cand;
      f32x16 acc[H2T];
#pragma unroll
      for (int mt = 0; mt < H2T; ++mt)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const f32x4v v = vec4(kB2 + 32 * mt + 8 * rr);
          acc[mt][4 * rr] = v.x; acc[mt][4 * rr + 1] = v.y; acc[mt][4 * rr + 2] = v.z; acc[mt][4 * rr + 3] = v.w;
        }
      float bsum = 0.0f;  // sum of |2^7 h1_j| c_j over this lane's half of the hidden units
      auto tile = [&](int t, float4 (&xt)[4]) {
        uint32_t hb[4][2];  // [rr][pair]: f16 (round to nearest even) of 2^7 h1, two units per register
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const f32x4v u = uvec4(32 * t + 8 * rr), al = vec4(kBeta1 + 32 * t + 8 * rr), c = vec4(kC + 32 * t + 8 * rr);
          float h[4];
          h[0] = prelu(xt[rr].x + u.x, al.x);  // the exact form's h1 x 2^7: same operations on operands x 2^7
          h[1] = prelu(xt[rr].y + u.y, al.y);
          h[2] = prelu(xt[rr].z + u.z, al.z);
          h[3] = prelu(xt[rr].w + u.w, al.w);
#pragma unroll
          for (int e = 0; e < 4; ++e) bsum = __builtin_fmaf(__builtin_fabsf(h[e]), c[e], bsum);
#pragma unroll
          for (int p = 0; p < 2; ++p) {
            uint32_t v;
            asm("v_fma_mixlo_f16 %0, %1, 1.0, 0" : "=v"(v) : "v"(h[2 * p]));
            asm("v_fma_mixhi_f16 %0, %1, 1.0, 0" : "+v"(v) : "v"(h[2 * p + 1]));
            hb[rr][p] = v;
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        load_tile(t + 2 >= H1T ? next : row, (t + 2) & (H1T - 1), xt);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 2; ++q) {  // step q: units 16 q + 4 g + {0..3} and 16 q + 8 + 4 g + {0..3} (pack_split_weights' k order)
          const f16x8 bh = as_f16x8(uint4{hb[2 * q][0], hb[2 * q][1], hb[2 * q + 1][0], hb[2 * q + 1][1]});
#pragma unroll
          for (int mt = 0; mt < H2T; ++mt) {
            const u32x4v w = *reinterpret_cast<lds_u4_ptr>((t < 4 ? w_lo : w_hi) + (t & 3) * 16384 + (q * 2 * H2T + 2 * mt) * 1024);
            acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, w), bh, acc[mt], 0, 0, 0);
          }
        }
      };
#pragma unroll 1
      for (int t = 0; t < H1T; t += 2) { tile(t, x[0]); tile(t + 1, x[1]); }
      if (change) load_u_of(reinterpret_cast<const PhaseState*>(a.ws + 256 + (unsigned long long)nxt.q * a.slot_bytes + a.off_state));
      // layer 2's PReLU as x + (alpha2 - 1) min(x, 0): a NaN stays a NaN (prelu() would make it 0) -- the bound relies on it
      float part = 0.0f;
#pragma unroll
      for (int mt = 0; mt < H2T; ++mt)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const f32x4v be = vec4(kBeta2 + 32 * mt + 8 * rr), w3 = vec4(kW3 + 32 * mt + 8 * rr);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float xa = acc[mt][4 * rr + e];
            part = __builtin_fmaf(__builtin_fmaf(__builtin_fminf(xa, 0.0f), be[e], xa), w3[e], part);
          }
        }
      const float s = (part + __shfl_xor(part, 32)) * (1.0f / (kSplit2Scale * kSplit2Scale));
      float bnd = __builtin_fmaf(bsum + __shfl_xor(bsum, 32), a.mlp.k1s, a.mlp.k0);
      // widened by 2^-20 (|s| + B): s - B and s + B are then bounds after their own f32 rounding
      bnd = __builtin_fmaf(__builtin_fabsf(s), 0x1p-20f, bnd * (1.0f + 0x1p-20f));
      if (!(__builtin_isfinite(s) && __builtin_isfinite(bnd))) bnd = __builtin_inff();
      if (g == 0 && i < cur.n) {
        cur.out[i] = s;
        if (cur.bnd != nullptr) cur.bnd[i] = bnd;
      }
      row = next;
      cur = nxt;
    }
    return;
  }
  if constexpr (!EXACT) {
    // ---- split-f16: one software pipeline over the wavefront's blocks (wave_mlp_split_pipeline, nann_mlp5.h)
    auto read_u_of = [&](int q) -> float4 {
      const PhaseState* st = reinterpret_cast<const PhaseState*>(a.ws + 256 + (unsigned long long)q * a.slot_bytes + a.off_state);
      float4 v = reinterpret_cast<const float4*>(st->u)[lane];
      v.x *= kSplit2Scale; v.y *= kSplit2Scale; v.z *= kSplit2Scale; v.w *= kSplit2Scale;
      return v;
    };
    Cur cur, nxt;
    enter_query(query_of(b_lo), cur, true);
    int i_cur = 0;
    SplitPipeLds L;
    L.w_lo = w_lo; L.w_hi = w_hi; L.v_at = v_at; L.u_at = u_at;
    L.u_wr = lds_offset_of(u_w) + (uint32_t)lane * 16u;
    wave_mlp_split_pipeline(
        L, row_ptr(cur, b_lo), b_hi - b_lo,
        [&](int k, const float* row, const float*& next, bool& change, float4& u_next) {  // the block behind block b_lo + k
          const int b = b_lo + k;
          nxt = cur;
          if (b + 1 < b_hi && b + 1 >= prefix[cur.q + 1]) {
            int q2 = cur.q + 1;
            while (prefix[q2 + 1] <= b + 1) ++q2;  // (queries without blocks)
            enter_query(q2, nxt, false);
            change = true;
            u_next = read_u_of(nxt.q);
          }
          next = (b + 1 < b_hi) ? row_ptr(nxt, b + 1) : row;
          i_cur = (b - cur.first) * 32 + cand;
        },
        [&](int, float score) {
          if (g == 0 && i_cur < cur.n) cur.out[i_cur] = score;
          cur = nxt;
        });
    return;
  }
  // ---- exact f32 (wg_score_mlp_xres's arithmetic, nann_mlp5.h): tile by tile, two tiles per trip of a rolled loop
  Cur cur, nxt;
  enter_query(query_of(b_lo), cur, true);
  const float* row = row_ptr(cur, b_lo);
  float4 x[2][4];
  load_tile(row, 0, x[0]);
  load_tile(row, 1, x[1]);
  for (int b = b_lo; b < b_hi; ++b) {
    // the next block: of this query or of the next one that has blocks (its rows are gathered from tile 6 on; its u
    // replaces this one's behind the last tile)
    nxt = cur;
    bool change = false;
    if (b + 1 < b_hi && b + 1 >= prefix[cur.q + 1]) {
      int q2 = cur.q + 1;
      while (prefix[q2 + 1] <= b + 1) ++q2;  // (queries without blocks)
      enter_query(q2, nxt, false);
      change = true;
    }
    const float* next = (b + 1 < b_hi) ? row_ptr(nxt, b + 1) : row;
    const int i = (b - cur.first) * 32 + cand;
    f32x16 acc[H2T];
#pragma unroll
    for (int mt = 0; mt < H2T; ++mt)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const f32x4v v = vec4(kB2 + 32 * mt + 8 * rr);
        acc[mt][4 * rr] = v.x; acc[mt][4 * rr + 1] = v.y; acc[mt][4 * rr + 2] = v.z; acc[mt][4 * rr + 3] = v.w;
      }
    auto tile = [&](int t, float4 (&xt)[4]) {
      f32x4v ub[8];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) { ub[rr] = uvec4(32 * t + 8 * rr); ub[4 + rr] = vec4(kBeta1 + 32 * t + 8 * rr); }
      float h[16];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const f32x4v u = ub[rr], al = ub[4 + rr];
        constexpr float kInv = 1.0f / kSplit2Scale;  // the table holds 2^7 P: exact both ways
        h[4 * rr + 0] = prelu(u.x + xt[rr].x * kInv, al.x);
        h[4 * rr + 1] = prelu(u.y + xt[rr].y * kInv, al.y);
        h[4 * rr + 2] = prelu(u.z + xt[rr].z * kInv, al.z);
        h[4 * rr + 3] = prelu(u.w + xt[rr].w * kInv, al.w);
      }
      __builtin_amdgcn_sched_barrier(0);
      load_tile(t + 2 >= H1T ? next : row, (t + 2) & (H1T - 1), xt);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f32x4v f[H2T];
#pragma unroll
        for (int mt = 0; mt < H2T; ++mt)  // p2x[t][mt][j][lane]: four chain steps per 16 bytes
          f[mt] = *reinterpret_cast<lds_f4_ptr>((t < 4 ? w_lo : w_hi) + (t & 3) * 16384 + (mt * 4 + j) * 1024);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int mt = 0; mt < H2T; ++mt)
            acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(f[mt][e], h[4 * j + e], acc[mt], 0, 0, 0);
      }
    };
#pragma unroll 1
    for (int t = 0; t < H1T; t += 2) { tile(t, x[0]); tile(t + 1, x[1]); }
    // the next block's query takes over the wavefront's u (every lane has read this block's)
    if (change) load_u_of(reinterpret_cast<const PhaseState*>(a.ws + 256 + (unsigned long long)nxt.q * a.slot_bytes + a.off_state));
    // PReLU of layer 2 and the bias-free output layer (wg_score_mlp_xres's epilogue: ORDER_O)
    float part = 0.0f;
#pragma unroll
    for (int mt = 0; mt < H2T; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * g;
        part = __fmaf_rn(prelu(acc[mt][r], V->beta2[m]), V->w3[m], part);
      }
    const float other = __shfl_xor(part, 32);
    const float p0 = g == 0 ? part : other, p1 = g == 0 ? other : part;
    if (g == 0 && i < cur.n) cur.out[(CERT == 1 && cur.list != nullptr) ? cur.list[i] : i] = p0 + p1;
    row = next;
    cur = nxt;
  }
}

// The certify step of the certified form (comment above mlp_filter_vectors): one 256-thread workgroup per query of the chunk.
// L by a most-significant-digit-first radix select (4 x 8 bits) over order-preserving keys of the lower bounds, the keys
// cached in LDS when the selection input has at most kCertKeys entries; then one pass that marks and compacts.  A round
// whose rows do not fit the raw region, whose k reaches its input size, or whose L is -inf refines every row.
constexpr int kCertNT = 256;
constexpr int kCertKeys = 8192;
__device__ __forceinline__ uint32_t cert_key(float f) {  // monotone: f < g <=> key(f) < key(g) (no NaN reaches it)
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float cert_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
template <int NT>
__global__ __launch_bounds__(NT) void k_mlp_phase_certify(PhaseScoreArgs a) {
  static_assert(NT == kCertNT, "one thread per digit of the radix select");
  __shared__ uint32_t keys[kCertKeys];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t wtot[kCertNT / 64];
  __shared__ uint32_t pick[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = blockIdx.x;
  unsigned char* slot = a.ws + 256 + (unsigned long long)q * a.slot_bytes;
  PhaseState* st = reinterpret_cast<PhaseState*>(slot + a.off_state);
  if (st->status != kPhasePending || st->r != a.round) return;
  const int n = st->sc_n, off = st->base_off, ntot = off + n;
  const int k = a.tq ? a.tq[(size_t)q * 6 + a.round] : a.t_r;
  float* sc = reinterpret_cast<float*>(slot + a.off_cand_scores);
  const float* bnd = reinterpret_cast<const float*>(slot + a.off_raw);
  int32_t* list = reinterpret_cast<int32_t*>(slot + a.off_raw);
  // inclusive prefix sum over the workgroup (every thread; ends behind a barrier)
  auto block_scan = [&](uint32_t v, uint32_t& total) -> uint32_t {
    const uint32_t inc = wave_scan_add(v);
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kCertNT / 64; ++w) {
      const uint32_t t = wtot[w];
      if (w < wave) base += t;
      total += t;
    }
    __syncthreads();
    return base + inc;
  };
  auto lo_key = [&](int i) -> uint32_t {
    const float s = sc[i];
    float lo;
    if (i < off) lo = s == s ? s : -__builtin_inff();  // carried, exact
    else {
      const float b = bnd[i - off];
      lo = b < __builtin_inff() ? s - b : -__builtin_inff();
    }
    return cert_key(lo);
  };
  bool all = n > a.max_raw || k <= 0 || k >= ntot;
  float L = -__builtin_inff();
  if (!all) {
    const bool cached = ntot <= kCertKeys;
    if (cached)
      for (int i = tid; i < ntot; i += kCertNT) keys[i] = lo_key(i);
    uint32_t prefix = 0, mask = 0, remaining = (uint32_t)k;
    for (int shift = 24; shift >= 0; shift -= 8) {
      hist[tid] = 0;
      __syncthreads();
      for (int i = tid; i < ntot; i += kCertNT) {
        const uint32_t key = cached ? keys[i] : lo_key(i);
        if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      // thread tid counts digit 255 - tid: the inclusive scan is the number of keys at or above that digit
      const uint32_t v = hist[255 - tid];
      uint32_t total;
      const uint32_t at_or_above = block_scan(v, total);
      if (v != 0 && at_or_above >= remaining && at_or_above - v < remaining) {
        pick[0] = 255u - (uint32_t)tid;
        pick[1] = remaining - (at_or_above - v);
      }
      __syncthreads();
      prefix |= pick[0] << shift;
      mask |= 255u << shift;
      remaining = pick[1];
      __syncthreads();
    }
    L = cert_unkey(prefix);
    all = !(L > -__builtin_inff());
  }
  if (all) {
    if (tid == 0) {
      st->ref_n = n;
      st->ref_list = 0;
      atomicAdd(&a.refined[a.round], (unsigned long long)n);
    }
    return;
  }
  // mark and compact: a chunk's bounds are all read before the scan's barrier, and a survivor's list position never
  // exceeds its row, so the list overwrites only bounds that were read
  uint32_t kept = 0;
  for (int c = off; c < ntot; c += kCertNT) {
    const int i = c + tid;
    bool surv = false;
    if (i < ntot) {
      const float b = bnd[i - off];
      const float hi = b < __builtin_inff() ? sc[i] + b : __builtin_inff();
      surv = !(hi < L);
    }
    uint32_t total;
    const uint32_t pos = block_scan(surv ? 1u : 0u, total) - (surv ? 1u : 0u);
    if (i < ntot) {
      if (surv) list[kept + pos] = i - off;
      else sc[i] = -__builtin_inff();
    }
    kept += total;
  }
  if (tid == 0) {
    st->ref_n = (int)kept;
    st->ref_list = 1;
    atomicAdd(&a.refined[a.round], (unsigned long long)kept);
  }
}

constexpr size_t kPhaseScoreLds = (size_t)kMlpResBytes + 8 * 1024 + (size_t)(kPhaseChunk + 4) * 4 + 64;  // + the scan's wavefront totals

}  // namespace nann
