// nann_hnsw_build.hip -- HNSW index construction ON THE DEVICE (SURVEY.md 8 f1 follow-up).
//
// The reference builds its index with faiss.IndexHNSWFlat(d, 32).add(embeddings) on the host
// (NANN_impls/nann/delivery/build_hnsw_index.py:33-35); nann_amd/csrc/host/hnsw_build.cpp restates that algorithm
// (Malkov & Yashunin alg. 1-4 with Faiss' conventions) multi-threaded on the CPU: 16 s for 1M x 128-d on 16 cores,
// minutes for a 4M x 256-d shard -- all outside the GPU, and the longest part of every test / bench set-up.
// Same algorithm here, BATCHED: nodes go in by descending level (as Faiss adds them), in batches that grow with the
// graph (a batch never exceeds a quarter of what is already inserted, <= 16384); the nodes of a batch
//   1. descend greedily through the levels above their own (ef = 1),
//   2. on each of their levels run the ef_construction beam search on the graph of the EARLIER batches (batch
//      mates do not see each other: with random insertion order a node's true neighbours are in its own batch with
//      probability batch / inserted), pick their links with the selection heuristic (alg. 4, no
//      keepPrunedConnections) and write their own adjacency rows,
//   3. hand (dst, src) pairs to the back-link pass: pairs sorted by dst (radix sort, stable, so the result does
//      not depend on atomics or scheduling), one wavefront per dst appends the new links while there is room
//      and re-selects with the heuristic when the row is full -- one incoming link at a time, as Faiss' add_link.
// Every step is one kernel over the whole batch, one WAVEFRONT per node: the beam (up to 64 sorted (distance, id)
// candidates) lives in the lanes of the wavefront -- lane i holds the i-th best --, is merged with a node's new
// neighbours by a bitonic network on shuffles, the visited set is a per-wavefront hash table in LDS, row distances
// are computed d/8 lanes per row from 16-byte loads.  A search is a chain of dependent HBM round trips (~50 hops of
// ~2 us), so a wavefront is slow and the chip is filled by the batch: thousands of searches in flight.
//
// Output = the arrays the exporter needs, on the device: levels (Faiss convention: number of levels of the node),
// adj0 [N, 2M] (-1 = empty slot), and for nodes with more than one level their rows in adj_up [rows, M]
// (row of node i on level l >= 1: up_row[i] + l - 1).  nann_amd/index_build.py turns them into
// neighbors_level_{l}_{values,row_splits}.npy / enter_points.npy exactly as build_hnsw_index.py:41-66 does.
// Index CONTENTS are not a parity target against Faiss (its own insertion order is thread-schedule dependent);
// the structural invariants and recall are (tests/test_index_build.py, -m gpu).  They ARE pinned, entry for entry, to the plain
// model of tests/hnsw_build_model.py for the cases of its tests (tests/test_index_build_exact_gpu.py).
//
// APPEND (nann_hnsw_append_device): the same batch loop started from a graph that exists -- the old rows are checked
// once (k_hb_check: the rules the kernels rely on, and the rows' fill counts), then the new nodes go in as a build's
// would.  EXPORT (nann_hnsw_export_count / _fill): the arrays -> the per-level CSR and enter points nann_index_create
// takes, on the device (tests/test_index_append_gpu.py).
//
// HOST SIDE, what the calls share: build, append and update the scratch of a run and the batch loop (HbScratch, hb_insert); every
// call the walk over `levels` (hb_levels: first upper rows, their total, the refusals) and the owner of its device memory
// (HbOwned, filled by dev_alloc, freed on every return); append, remove and update the check of the graph they are given
// (hb_check_enqueue, hb_check_result); search, back-link and repair the map (d, dtype, metric) -> <LPR, DT, MT> (hb_dispatch).
//
// REMOVE (nann_hnsw_remove_count / nann_hnsw_remove_device): the arrays and a bitmap of rows to drop -> NEW arrays over the
// survivors, renumbered in order; a row that lost an entry is re-selected (wave_select) from its survivors and the surviving
// entries of its removed entries' rows, one hop (k_hb_repair; tests/test_index_remove_gpu.py).
//
// UPDATE (nann_hnsw_update_device): rows whose embedding changed, or that a removal left without links, are refreshed IN PLACE --
// detach (k_hb_repair with the identity map: nobody is renumbered, the marked nodes' rows come out empty), the fill counts of
// the new arrays from a device pass (k_hb_check over them), then hb_insert as the append calls it.  nann_hnsw_orphan_bits
// (k_hb_orphan_mark / _bits) names the rows a heal would mark.  tests/test_index_update_gpu.py; DESIGN.md 4.6.
//
// METRIC (nann_hnsw_build_device_metric / nann_hnsw_append_device_metric): the same kernels with dist(a, b) = -<a, b>, for an
// index that is searched with the inner-product scorer.  Algorithms 1-4 run on that distance unchanged; the beam's keys take
// an order-preserving map of its bits (hb_key).  tests/test_index_build_ip_gpu.py.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <random>
#include <string>
#include <type_traits>
#include <vector>

#include "nann_host.h"

using namespace nann;

namespace {

constexpr int kHbWaves = 4;          // wavefronts (= nodes) per workgroup
constexpr int kHbVisSlots = 4096;    // visited-set slots per wavefront (16 KB): ef_construction x degree ids at most, kept < 3/4 full
constexpr uint32_t kHbEmpty = 0xffffffffu;
constexpr int kHbMaxCand = 64;       // beam slots = lanes
constexpr unsigned long long kKeyInf = 0xffffffffffffffffull;

struct HbGraph {
  const void* emb;      // [N, d] f16 / bf16 rows
  int32_t* adj0;        // [N, cap0]
  int32_t* cnt0;        // [N]
  const int32_t* up_row;  // [N] first upper row or -1
  int32_t* adj_up;      // [rows, M]
  int32_t* cnt_up;      // [rows]
  int n_items, d, M;
  int keep_pruned;      // alg. 4's keepPrunedConnections: fill a row's free slots with the nearest candidates the heuristic discarded
};

__device__ __forceinline__ int32_t* hb_row(const HbGraph& g, int node, int level, int* cap, int32_t** cnt) {
  if (level == 0) { *cap = 2 * g.M; *cnt = g.cnt0 + node; return g.adj0 + (size_t)node * 2 * g.M; }
  const size_t r = (size_t)g.up_row[node] + (size_t)(level - 1);
  *cap = g.M; *cnt = g.cnt_up + r;
  return g.adj_up + r * g.M;
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
  return ((unsigned long long)hi << 32) | lo;
}

// ascending bitonic sort of one 64-bit key per lane over the wavefront.  USER (here and on wave_select): a tag with no meaning
// in the code.  The build's kernels use instance 0, k_hb_repair instance 1: a further user of ONE always-inlined instance changes
// the order in which hipcc emits a few instructions of the kernels that already inline it (Remove), and the
// build's kernels are to compile to what they did.
template <int USER = 0>
__device__ __forceinline__ unsigned long long wave_sort64(unsigned long long key, int lane) {
#pragma unroll
  for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const unsigned long long other = shfl_xor_u64(key, stride);
      const bool up = (lane & size) == 0;          // ascending block
      const bool lower = (lane & stride) == 0;     // this lane keeps the smaller one in an ascending block
      const bool take_min = up == lower;
      key = take_min ? (key < other ? key : other) : (key > other ? key : other);
    }
  }
  return key;
}

// merge: `sorted` ascending over the lanes, `fresh` arbitrary -> the 64 smallest of the 128, ascending
__device__ __forceinline__ unsigned long long wave_merge64(unsigned long long sorted, unsigned long long fresh, int lane) {
  fresh = wave_sort64(fresh, lane);
  const unsigned long long rev = shfl_xor_u64(fresh, 63);  // descending
  unsigned long long key = sorted < rev ? sorted : rev;     // bitonic: the 64 smallest
#pragma unroll
  for (int stride = 32; stride > 0; stride >>= 1) {
    const unsigned long long other = shfl_xor_u64(key, stride);
    const bool lower = (lane & stride) == 0;
    key = lower ? (key < other ? key : other) : (key > other ? key : other);
  }
  return key;
}

// 8 consecutive elements of row `r` (sub-chunk `sub`) as f32; DT: 0 f16, 1 bf16
template <int DT>
__device__ __forceinline__ void hb_load8(const void* emb, size_t r, int d, int sub, float x[8]) {
  const uint4 v = *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(emb) + r * d + sub * 8);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (DT == 0) { x[2 * i] = half_bits_to_float(w[i] & 0xffffu); x[2 * i + 1] = half_bits_to_float(w[i] >> 16); }
    else { x[2 * i] = bf16_bits_to_float(w[i] & 0xffffu); x[2 * i + 1] = bf16_bits_to_float(w[i] >> 16); }
  }
}

// a lane's partial (8 squared differences, or 8 products) summed over the LPR lanes of a row group: every lane of the group
// returns the total
template <int LPR>
__device__ __forceinline__ float hb_group_sum(float acc) {
#pragma unroll
  for (int s = 1; s < LPR; s <<= 1) acc += __shfl_xor(acc, s);
  return acc;
}

// The metric rows are linked by (a template parameter of every kernel below): kHbL2 = squared L2, kHbIp = -<a, b> (Faiss'
// convention for METRIC_INNER_PRODUCT: smaller is nearer).  The L2 instances are the code they were before the parameter.
constexpr int kHbL2 = 0, kHbIp = 1;

// distance key.  L2: squared distances are >= 0, so their f32 bit patterns order like the values.  IP: distances take both
// signs, so the pattern goes through the order-preserving map of a radix sort -- all bits flipped when the sign bit is set,
// else the sign bit set; -0 is made +0 first.  Either way kKeyInf (a NaN pattern no distance has) sorts last.
template <int MT>
__device__ __forceinline__ unsigned long long hb_key(float dist, int id) {
  uint32_t u = __float_as_uint(dist + 0.0f);
  if constexpr (MT == kHbIp) u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (uint32_t)id;
}

// the distance a key's upper half holds
template <int MT>
__device__ __forceinline__ float hb_key_dist(uint32_t u) {
  if constexpr (MT == kHbIp) u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  return __uint_as_float(u);
}

// a group's sum -> the distance: L2 the sum of squares itself, IP 0 - <a, b>
template <int MT>
__device__ __forceinline__ float hb_dist_of_sum(float sum) {
  if constexpr (MT == kHbIp) return 0.0f - sum;
  return sum;
}

constexpr int kHbMaxEf = 40;  // ef_construction this build stages rows for (Faiss' default)
template <int D>
struct HbWaveLds {
  static constexpr int kStage = kHbMaxEf * D * 2;  // bytes of row staging for the selection among the beam
  static constexpr int kRegion = kStage > kHbVisSlots * 4 ? kStage : kHbVisSlots * 4;
  union {
    uint32_t vis[kHbVisSlots];           // visited ids (search) ...
    unsigned char stage[kRegion];        // ... reused as row staging by the selection once the search is over
  };
  int32_t list[kHbMaxCand];   // ids of a node's unvisited neighbours (compacted)
  float dist[kHbMaxCand];
};

// the selection heuristic (alg. 4 / Faiss shrink_neighbor_list) over candidates sorted ascending by distance to the
// base: keep c iff it is closer to the base than to every candidate kept so far (dist(c, s) >= dist(c, base) for every kept
// s, in the kernel's metric); at most `cap`.  cand_key: lane i = i-th nearest (kKeyInf beyond n).  Rows are staged into
// `rows` (LDS, n x d halves).  Returns the keep mask (bit i = candidate i kept; wave-uniform).
template <int LPR, int DT, int MT, int USER = 0>
__device__ __forceinline__ uint64_t wave_select(const HbGraph& g, unsigned long long cand_key, int n, int cap,
                                                uint16_t* rows, int lane) {
  constexpr int GPW = 64 / LPR;
  const int d = g.d, sub = lane % LPR, grp = lane / LPR;
  // stage the candidates' rows: group `grp` copies rows grp, grp + GPW, ...
  for (int i0 = 0; i0 < n; i0 += GPW) {
    const int i = i0 + grp;
    const int id = (int)(uint32_t)__shfl((int)(uint32_t)cand_key, min(i, n - 1));
    if (i < n)
      *reinterpret_cast<uint4*>(rows + (size_t)i * d + sub * 8) =
          *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(g.emb) + (size_t)id * d + sub * 8);
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  uint64_t kept = 0;
  int n_kept = 0;
  for (int c = 0; c < n && n_kept < cap; ++c) {
    const float dc = hb_key_dist<MT>((uint32_t)__shfl((int)(uint32_t)(cand_key >> 32), c));  // distance of c to the base
    bool dominated = false;
    if (n_kept > 0) {
      // distances of c to the kept candidates, GPW pairs per step
      float xc[8];
      {
        const uint4 v = *reinterpret_cast<const uint4*>(rows + (size_t)c * d + sub * 8);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (DT == 0) { xc[2 * i] = half_bits_to_float(w[i] & 0xffffu); xc[2 * i + 1] = half_bits_to_float(w[i] >> 16); }
          else { xc[2 * i] = bf16_bits_to_float(w[i] & 0xffffu); xc[2 * i + 1] = bf16_bits_to_float(w[i] >> 16); }
        }
      }
      uint64_t todo = kept;
      while (todo && !dominated) {  // uniform
        // the grp-th set bit of `todo`
        uint64_t t = todo;
        for (int k = 0; k < grp && t; ++k) t &= t - 1;
        const int s = t ? __ffsll((unsigned long long)t) - 1 : -1;
        float acc = 0.0f;
        if (s >= 0) {
          const uint4 v = *reinterpret_cast<const uint4*>(rows + (size_t)s * d + sub * 8);
          const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float a, b;
            if (DT == 0) { a = half_bits_to_float(w[i] & 0xffffu); b = half_bits_to_float(w[i] >> 16); }
            else { a = bf16_bits_to_float(w[i] & 0xffffu); b = bf16_bits_to_float(w[i] >> 16); }
            if constexpr (MT == kHbIp) {
              acc = __fmaf_rn(xc[2 * i], a, acc);
              acc = __fmaf_rn(xc[2 * i + 1], b, acc);
            } else {
              const float t0 = xc[2 * i] - a, t1 = xc[2 * i + 1] - b;
              acc = __fmaf_rn(t0, t0, acc);
              acc = __fmaf_rn(t1, t1, acc);
            }
          }
        }
        acc = hb_dist_of_sum<MT>(hb_group_sum<LPR>(acc));
        dominated = __ballot(s >= 0 && acc < dc) != 0ull;
        for (int k = 0; k < GPW && todo; ++k) todo &= todo - 1;  // the GPW bits just processed
      }
    }
    if (!dominated) { kept |= 1ull << c; ++n_kept; }
  }
  if (g.keep_pruned && n_kept < cap) {
    // keepPrunedConnections (Malkov & Yashunin alg. 4, lines 15-17): the discarded candidates, nearest first, until the row
    // is full.  Faiss leaves this off (so do the reference's graphs and this builder's default); with it rows fill up to the
    // cap -- the dense-graph case of SURVEY.md 8's gather bound (L0 gathered <= ef * 64).
    const int n_all = min(n, 64);
    uint64_t rest = ~kept & (n_all >= 64 ? ~0ull : ((1ull << n_all) - 1ull));
    while (rest && n_kept < cap) {
      const int c = __ffsll((unsigned long long)rest) - 1;
      kept |= 1ull << c;
      rest &= rest - 1;
      ++n_kept;
    }
  }
  return kept;
}

struct HbBatch {
  const int32_t* nodes;   // [n] node ids of the batch
  int n;
  int level;              // the level searched
  int ef;                 // beam width (1 on the levels above the batch's own)
  int link;               // 1: select + write the node's row + emit back-link pairs
  int32_t* entry;         // [n] in: entry node of this level; out: nearest node found (entry of the next level down)
  uint32_t* pair_dst;     // [n * pair_cap] back-link targets (kHbEmpty = none)
  uint32_t* pair_src;     // [n * pair_cap]
  int pair_cap;
};

template <int LPR, int DT, int MT>
__global__ __launch_bounds__(kHbWaves * 64) void k_hb_search(HbGraph g, HbBatch b) {
  __shared__ __attribute__((aligned(16))) HbWaveLds<LPR * 8> lds_all[kHbWaves];
  constexpr int GPW = 64 / LPR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bi = blockIdx.x * kHbWaves + wave;
  if (bi >= b.n) return;
  HbWaveLds<LPR * 8>& L = lds_all[wave];
  const int u = b.nodes[bi];
  const int sub = lane % LPR, grp = lane / LPR;
  float q[8];
  hb_load8<DT>(g.emb, (size_t)u, g.d, sub, q);
  for (int i = lane; i < kHbVisSlots; i += 64) L.vis[i] = kHbEmpty;
  auto row_dist = [&](int id) -> float {  // all lanes of a group pass the same id
    float x[8];
    hb_load8<DT>(g.emb, (size_t)id, g.d, sub, x);
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if constexpr (MT == kHbIp) acc = __fmaf_rn(q[k], x[k], acc);
      else { const float t = q[k] - x[k]; acc = __fmaf_rn(t, t, acc); }
    }
    return hb_dist_of_sum<MT>(hb_group_sum<LPR>(acc));
  };
  auto visit = [&](int id) -> bool {  // true if the id was not in the set (and is now)
    uint32_t h = ((uint32_t)id * 2654435761u) >> 20;  // 12 bits
    for (int probe = 0; probe < kHbVisSlots; ++probe) {
      const uint32_t c = atomicCAS(&L.vis[h], kHbEmpty, (uint32_t)id);
      if (c == kHbEmpty) return true;
      if (c == (uint32_t)id) return false;
      h = (h + 1) & (kHbVisSlots - 1);
    }
    return false;
  };
  __builtin_amdgcn_wave_barrier();
  const int ep = b.entry[bi];
  const float d_ep = row_dist(ep);
  if (lane == 0) visit(ep);
  int n_vis = 1;
  // the beam: lane i = i-th best (distance, id); low bit of `expanded` per lane
  unsigned long long beam = lane == 0 ? hb_key<MT>(d_ep, ep) : kKeyInf;
  bool expanded = false;
  const int ef = b.ef;
  for (;;) {
    const uint64_t open = __ballot(!expanded && beam != kKeyInf && lane < ef);
    if (!open) break;
    const int p = __ffsll((unsigned long long)open) - 1;
    if (lane == p) expanded = true;
    const int cur = (int)(uint32_t)__shfl((int)(uint32_t)beam, p);
    int cap;
    int32_t* cnt;
    const int32_t* row = hb_row(g, cur, b.level, &cap, &cnt);
    const int n_nb = min(*cnt, cap);
    // unvisited neighbours, compacted into L.list
    int nb = lane < n_nb ? row[lane] : -1;
    bool fresh = false;
    if (nb >= 0 && n_vis < (kHbVisSlots * 3) / 4) fresh = visit(nb);
    const uint64_t fm = __ballot(fresh);
    const int n_new = popc64(fm);
    if (fresh) L.list[popc64(fm & lanemask_lt(lane))] = nb;
    n_vis += n_new;
    __builtin_amdgcn_wave_barrier();
    // distances, GPW rows per step
    for (int i0 = 0; i0 < n_new; i0 += GPW) {
      const int i = i0 + grp;
      const int id = L.list[min(i, n_new - 1)];
      const float dv = row_dist(id);
      if (i < n_new && sub == 0) L.dist[i] = dv;
    }
    __builtin_amdgcn_wave_barrier();
    unsigned long long fresh_key = kKeyInf;
    if (lane < n_new) fresh_key = hb_key<MT>(L.dist[lane], L.list[lane]);
    // merge; a lane's `expanded` flag travels with its key BELOW the id: the id half becomes (id << 1) | flag (ids are < 2^31).
    // Ids are unique in the beam, so the flag never decides an order: the beam is sorted by (distance, id) alone, and it stays
    // sorted -- what wave_merge64 asks of its first argument -- when lane p's flag has just been set.  (In bit 31, above the id,
    // the flag put lane p behind the unexpanded lanes of the SAME distance without moving it: an unsorted input on exact ties.)
    auto tag = [](unsigned long long k, bool e) -> unsigned long long {
      return k == kKeyInf ? k : ((k & 0xffffffff00000000ull) | ((k & 0x7fffffffull) << 1) | (e ? 1ull : 0ull));
    };
    const unsigned long long merged = wave_merge64(tag(beam, expanded), tag(fresh_key, false), lane);
    expanded = merged != kKeyInf && (merged & 1ull) != 0ull;
    beam = merged == kKeyInf ? merged : ((merged & 0xffffffff00000000ull) | ((merged & 0xffffffffull) >> 1));
    if (lane >= ef) { beam = kKeyInf; expanded = false; }  // the beam holds ef candidates
    __builtin_amdgcn_wave_barrier();
  }
  // nearest node found: the next level's entry
  const int nearest = (int)(uint32_t)__shfl((int)(uint32_t)beam, 0);
  if (lane == 0) b.entry[bi] = nearest;
  if (!b.link) return;
  // ---- link: heuristic selection among the beam, own row, back-link pairs
  const int n_cand = popc64(__ballot(beam != kKeyInf));
  int cap;
  int32_t* cnt;
  int32_t* my_row = hb_row(g, u, b.level, &cap, &cnt);
  uint16_t* rows = reinterpret_cast<uint16_t*>(L.stage);  // the search is over: its table becomes row staging
  const uint64_t kept = wave_select<LPR, DT, MT>(g, beam, n_cand, cap, rows, lane);
  const int n_kept = popc64(kept);
  const bool mine = (kept >> lane) & 1ull;
  const int pos = popc64(kept & lanemask_lt(lane));
  const int id = (int)(uint32_t)beam;
  if (mine) {
    my_row[pos] = id;
    b.pair_dst[(size_t)bi * b.pair_cap + pos] = (uint32_t)id;
    b.pair_src[(size_t)bi * b.pair_cap + pos] = (uint32_t)u;
  }
  for (int i = n_kept + lane; i < b.pair_cap; i += 64) b.pair_dst[(size_t)bi * b.pair_cap + i] = kHbEmpty;
  if (lane == 0) *cnt = n_kept;
}

// run starts of the sorted pair list -> (dst, first, count) records
__global__ void k_hb_runs(const uint32_t* dst, int n_pairs, int32_t* run_first, int32_t* run_len, int* n_runs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pairs) return;
  const uint32_t k = dst[i];
  if (k == kHbEmpty) return;
  if (i > 0 && dst[i - 1] == k) return;
  int len = 1;
  while (i + len < n_pairs && dst[i + len] == k) ++len;
  const int r = atomicAdd(n_runs, 1);
  run_first[r] = i;
  run_len[r] = len;
}

// back-links of one batch: one wavefront per target node; its incoming sources in pair order (deterministic: the
// pair buffer is filled by batch position and the sort is stable).  Room left: append.  Full: re-select among the
// row + the new link (Faiss add_link), one incoming link at a time.  The row lives in the lanes (lane i = link i)
// and is written back once.
template <int LPR, int DT, int MT>
__global__ __launch_bounds__(kHbWaves * 64) void k_hb_backlink(HbGraph g, int level, const uint32_t* pair_dst,
                                                               const uint32_t* pair_src, const int32_t* run_first,
                                                               const int32_t* run_len, const int* n_runs) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int GPW = 64 / LPR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ri = blockIdx.x * kHbWaves + wave;
  if (ri >= *n_runs) return;
  const int sub = lane % LPR, grp = lane / LPR;
  const size_t row_bytes = (size_t)kHbMaxCand * g.d * 2;
  unsigned char* mine_lds = smem + (size_t)wave * (row_bytes + 1024);
  uint16_t* rows = reinterpret_cast<uint16_t*>(mine_lds);
  float* dist = reinterpret_cast<float*>(mine_lds + row_bytes);       // [64]
  int32_t* ids = reinterpret_cast<int32_t*>(mine_lds + row_bytes + 512);  // [64]
  const int first = run_first[ri], len = run_len[ri];
  const int v = (int)pair_dst[first];
  int cap;
  int32_t* cnt;
  int32_t* row = hb_row(g, v, level, &cap, &cnt);
  int c = min(*cnt, cap);
  int link = lane < c ? row[lane] : -1;  // the row, one link per lane
  float qv[8];
  hb_load8<DT>(g.emb, (size_t)v, g.d, sub, qv);
  for (int j = 0; j < len; ++j) {
    const int s = (int)pair_src[first + j];
    if (c < cap) {
      if (lane == c) link = s;
      ++c;
      continue;
    }
    // full: candidates = the cap links + s (at cap = 64 the 65 do not fit the lanes: the farthest of them is
    // dropped before the walk -- it could only have been kept if fewer than cap nearer ones survive).  Distances to v:
    ids[lane] = lane < cap ? link : -1;
    __builtin_amdgcn_wave_barrier();
    for (int i0 = 0; i0 <= cap; i0 += GPW) {
      const int i = i0 + grp;
      const int id = i < cap ? ids[min(i, cap - 1)] : s;
      float x[8];
      hb_load8<DT>(g.emb, (size_t)id, g.d, sub, x);
      float acc = 0.0f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if constexpr (MT == kHbIp) acc = __fmaf_rn(qv[k], x[k], acc);
        else { const float t = qv[k] - x[k]; acc = __fmaf_rn(t, t, acc); }
      }
      acc = hb_dist_of_sum<MT>(hb_group_sum<LPR>(acc));
      if (i < cap && sub == 0) dist[i] = acc;
      if (i == cap && sub == 0) dist[63] = cap == 64 ? dist[63] : acc;  // (placeholder slot; the extra's distance is re-derived below)
    }
    __builtin_amdgcn_wave_barrier();
    float d_extra;
    {  // distance of the new link, computed by group 0 and broadcast
      float x[8];
      hb_load8<DT>(g.emb, (size_t)s, g.d, sub, x);
      float acc = 0.0f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if constexpr (MT == kHbIp) acc = __fmaf_rn(qv[k], x[k], acc);
        else { const float t = qv[k] - x[k]; acc = __fmaf_rn(t, t, acc); }
      }
      d_extra = hb_dist_of_sum<MT>(hb_group_sum<LPR>(acc));
    }
    unsigned long long key = lane < cap ? hb_key<MT>(dist[lane], link) : kKeyInf;
    key = wave_sort64(key, lane);
    const unsigned long long extra = hb_key<MT>(d_extra, s);
    const int before = popc64(__ballot(key < extra));  // the extra candidate's place in the ascending order
    const int src_lane = lane <= before ? lane : lane - 1;
    const unsigned long long from = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(key >> 32), src_lane) << 32) |
                                    (uint32_t)__shfl((int)(uint32_t)key, src_lane);
    unsigned long long cand = lane == before ? extra : from;
    const int n_cand = min(cap + 1, 64);
    if (lane >= n_cand) cand = kKeyInf;
    const uint64_t kept = wave_select<LPR, DT, MT>(g, cand, n_cand, cap, rows, lane);
    const int n_kept = popc64(kept);
    __builtin_amdgcn_wave_barrier();
    if ((kept >> lane) & 1ull) ids[popc64(kept & lanemask_lt(lane))] = (int)(uint32_t)cand;
    __builtin_amdgcn_wave_barrier();
    link = lane < n_kept ? ids[lane] : -1;
    c = n_kept;
    __builtin_amdgcn_wave_barrier();
  }
  if (lane < cap) row[lane] = lane < c ? link : -1;
  if (lane == 0) *cnt = c;
}

// the device allocations of one call: freed when it returns, by whichever return
struct HbOwned {
  std::vector<void*> ptrs;
  HbOwned() = default;
  HbOwned(const HbOwned&) = delete;
  HbOwned& operator=(const HbOwned&) = delete;
  ~HbOwned() { for (void* p : ptrs) (void)hipFree(p); }
};

template <typename T>
int dev_alloc(T** p, size_t n, HbOwned* owned) {
  void* q = nullptr;
  HIP_TRY(hipMalloc(&q, std::max<size_t>(n * sizeof(T), 16)));
  owned->ptrs.push_back(q);
  *p = static_cast<T*>(q);
  return NANN_OK;
}

template <int LPR, int DT, int MT>
int run_batch_level(const HbGraph& g, const HbBatch& b, hipStream_t st) {
  const unsigned blocks = (unsigned)((b.n + kHbWaves - 1) / kHbWaves);
  hipLaunchKernelGGL((k_hb_search<LPR, DT, MT>), dim3(blocks), dim3(kHbWaves * 64), 0, st, g, b);
  HIP_TRY(hipGetLastError());
  return NANN_OK;
}

template <int LPR, int DT, int MT>
int run_backlink(const HbGraph& g, int level, const uint32_t* dst, const uint32_t* src, const int32_t* rf, const int32_t* rl,
                 const int* n_runs, int max_runs, hipStream_t st) {
  const size_t per_wave = (size_t)kHbMaxCand * g.d * 2 + 1024;
  const size_t lds = per_wave * kHbWaves;
  auto kern = k_hb_backlink<LPR, DT, MT>;
  if (lds > 48 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const unsigned blocks = (unsigned)((max_runs + kHbWaves - 1) / kHbWaves);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(kHbWaves * 64), lds, st, g, level, dst, src, rf, rl, n_runs);
  HIP_TRY(hipGetLastError());
  return NANN_OK;
}

// ---- append: the old graph is INPUT -------------------------------------------------------------------------
// k_hb_check reads every row of the old graph once, one wavefront per node, BEFORE anything is written or searched:
// it holds the arrays to the four rules the insertion kernels rely on and recomputes the rows' fill counts (the
// length of the dense prefix) into the call's scratch.  Rows are addressed through `up_expect` (what the host
// derived from `levels`), never through a value read from the arrays, so the pass itself cannot leave them.
// bad[r] = lowest node that breaks rule r (kHbNone: none).
enum { kHbBadUpRow = 0, kHbBadRange, kHbBadHole, kHbBadLevel, kHbRules };
constexpr int32_t kHbNone = 0x7fffffff;

__global__ __launch_bounds__(kHbWaves * 64) void k_hb_check(const int32_t* adj0, const int32_t* up_row, const int32_t* adj_up,
                                                            const int32_t* levels, const int32_t* up_expect, int n_old, int M,
                                                            int32_t* cnt0, int32_t* cnt_up, int32_t* bad) {
  const int lane = threadIdx.x & 63;
  const size_t at = (size_t)blockIdx.x * kHbWaves + (threadIdx.x >> 6);
  if (at >= (size_t)n_old) return;
  const int node = (int)at;
  const int lv = levels[node], ur = up_expect[node];
  if (lane == 0 && up_row[node] != ur) atomicMin(&bad[kHbBadUpRow], node);
  for (int l = 0; l < lv; ++l) {
    const int cap = l == 0 ? 2 * M : M;
    const int32_t* row = l == 0 ? adj0 + (size_t)node * 2 * M : adj_up + ((size_t)ur + (size_t)(l - 1)) * M;
    const int e = lane < cap ? row[lane] : -1;
    const bool in_range = e >= -1 && e < n_old;
    const uint64_t used = __ballot(e != -1);
    const int c = popc64(used);
    const bool hole = used != (c >= 64 ? ~0ull : (1ull << c) - 1ull);
    const bool low = in_range && e >= 0 && levels[e] <= l;  // a link to a node that has no row on this level
    const bool any_out = __ballot(!in_range) != 0ull, any_low = __ballot(low) != 0ull;
    if (lane == 0) {
      if (any_out) atomicMin(&bad[kHbBadRange], node);
      if (hole) atomicMin(&bad[kHbBadHole], node);
      if (any_low) atomicMin(&bad[kHbBadLevel], node);
      if (l == 0) cnt0[node] = c; else cnt_up[(size_t)ur + (size_t)(l - 1)] = c;
    }
  }
}

// ---- export: the builder's arrays -> the per-level CSR of build_hnsw_index.py:41-66 (start_level = 2) --------
// One wavefront per node and level: the row's slots one per lane, ballot of the non-negative ones, popcount = the
// row's length (count), prefix popcount = a kept slot's place (fill) -- the compaction of nann_filter.h.  A node
// absent on level 1 has an empty row.  up_row is data: a value outside [0, n_up) raises *bad instead of being used.
__device__ __forceinline__ int hb_export_slot(const int32_t* adj0, const int32_t* up_row, const int32_t* adj_up,
                                              const int32_t* levels, int64_t n_up, int M, int node, int level, int lane, int* bad) {
  if (level == 0) return lane < 2 * M ? adj0[(size_t)node * 2 * M + lane] : -1;
  if (levels[node] < 2) return -1;
  const int64_t r = up_row[node];
  if (r < 0 || r >= n_up) {
    if (lane == 0) *bad = 1;
    return -1;
  }
  return lane < M ? adj_up[(size_t)r * M + lane] : -1;
}

__global__ __launch_bounds__(kHbWaves * 64) void k_hb_export_count(const int32_t* adj0, const int32_t* up_row, const int32_t* adj_up,
                                                                   const int32_t* levels, int n, int64_t n_up, int M,
                                                                   int64_t* len0, int64_t* len1, int* bad) {
  const int lane = threadIdx.x & 63;
  const size_t at = (size_t)blockIdx.x * kHbWaves + (threadIdx.x >> 6);
  if (at >= (size_t)n) return;
  const int node = (int)at;
#pragma unroll
  for (int level = 0; level < 2; ++level) {
    const int e = hb_export_slot(adj0, up_row, adj_up, levels, n_up, M, node, level, lane, bad);
    const int c = popc64(__ballot(e >= 0));
    if (lane == 0) (level == 0 ? len0 : len1)[node] = c;
  }
}

__global__ __launch_bounds__(kHbWaves * 64) void k_hb_export_fill(const int32_t* adj0, const int32_t* up_row, const int32_t* adj_up,
                                                                  const int32_t* levels, int n, int64_t n_up, int M,
                                                                  const int64_t* rs0, const int64_t* rs1, int64_t nnz0, int64_t nnz1,
                                                                  int32_t* v0, int32_t* v1, int* bad) {
  const int lane = threadIdx.x & 63;
  const size_t at = (size_t)blockIdx.x * kHbWaves + (threadIdx.x >> 6);
  if (at >= (size_t)n) return;
  const int node = (int)at;
#pragma unroll
  for (int level = 0; level < 2; ++level) {
    const int e = hb_export_slot(adj0, up_row, adj_up, levels, n_up, M, node, level, lane, bad);
    const uint64_t keep = __ballot(e >= 0);
    const int64_t* rs = level == 0 ? rs0 : rs1;
    const int64_t first = rs[node], len = rs[node + 1] - first, nnz = level == 0 ? nnz0 : nnz1;
    // row_splits of another graph: a row is written only where its span is its own length and lies inside values[0, nnz)
    if (len != popc64(keep) || first < 0 || first > nnz - len || (node == 0 && first != 0) || (node == n - 1 && first + len != nnz)) {
      if (lane == 0) *bad = 1;
      continue;
    }
    if (e >= 0) (level == 0 ? v0 : v1)[first + popc64(keep & lanemask_lt(lane))] = e;
  }
}

// ---- remove: a smaller, renumbered graph whose surviving rows are reconnected across the holes ----------------
// The removal bitmap is the deny bitmap of nann_filter: row r is removed iff bit (r & 31) of word (r >> 5) is set.  Entries of
// a checked graph lie in [0, n), so no word at or beyond ceil(n / 32) is ever read.
__device__ __forceinline__ bool hb_removed(const uint32_t* bits, int r) { return (bits[(uint32_t)r >> 5] >> (r & 31)) & 1u; }

// keep flags (for the scan that gives the old -> new map) ...
__global__ void k_hb_keep_flags(const uint32_t* bits, int n, int32_t* flag) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (size_t)n) flag[i] = hb_removed(bits, (int)i) ? 0 : 1;
}

// ... and the compaction of the surviving ids through that map: kept_rows[map[i]] = i
__global__ void k_hb_kept_rows(const uint32_t* bits, const int32_t* map, int n, int32_t* kept_rows) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (size_t)n && !hb_removed(bits, (int)i)) kept_rows[map[i]] = (int32_t)i;
}

// `sorted` ascending over the lanes and free of duplicates, `fresh` arbitrary -> the 64 smallest DISTINCT keys of the 128,
// ascending (kKeyInf behind); returns how many distinct keys the 128 held.  wave_merge64 with both halves of the bitonic merge
// kept: a key that is in both inputs (the same id reached twice has the same key) would otherwise take two of the 64 places
// and push a pool member out before the duplicate is seen.  Equal keys are adjacent in the sorted 128; the first of each run
// is compacted through `buf` (LDS, 64 keys).
__device__ __forceinline__ unsigned long long wave_merge64_unique(unsigned long long sorted, unsigned long long fresh, int lane,
                                                                  unsigned long long* buf, int* n_distinct) {
  fresh = wave_sort64<1>(fresh, lane);
  const unsigned long long rev = shfl_xor_u64(fresh, 63);  // descending
  unsigned long long lo = sorted < rev ? sorted : rev, hi = sorted < rev ? rev : sorted;  // two bitonic halves, lo <= hi
#pragma unroll
  for (int stride = 32; stride > 0; stride >>= 1) {
    const unsigned long long olo = shfl_xor_u64(lo, stride), ohi = shfl_xor_u64(hi, stride);
    const bool lower = (lane & stride) == 0;
    lo = lower ? (lo < olo ? lo : olo) : (lo > olo ? lo : olo);
    hi = lower ? (hi < ohi ? hi : ohi) : (hi > ohi ? hi : ohi);
  }
  auto from_lane = [](unsigned long long v, int src) -> unsigned long long {
    return ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(v >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)v, src);
  };
  const int below = (lane + 63) & 63;  // the lane before this one; lane 0 of `hi` follows lane 63 of `lo`
  const unsigned long long plo = from_lane(lo, below), phi = from_lane(hi, below);
  const bool keep_lo = lo != kKeyInf && (lane == 0 || lo != plo);
  const bool keep_hi = hi != kKeyInf && hi != (lane == 0 ? plo : phi);
  const uint64_t mlo = __ballot(keep_lo), mhi = __ballot(keep_hi);
  const int nlo = popc64(mlo);
  buf[lane] = kKeyInf;
  __builtin_amdgcn_wave_barrier();
  if (keep_lo) buf[popc64(mlo & lanemask_lt(lane))] = lo;
  const int at = nlo + popc64(mhi & lanemask_lt(lane));
  if (keep_hi && at < kHbMaxCand) buf[at] = hi;
  __builtin_amdgcn_wave_barrier();
  const unsigned long long out = buf[lane];
  __builtin_amdgcn_wave_barrier();
  *n_distinct = nlo + popc64(mhi);
  return out;
}

struct HbRepair {
  const void* emb;            // [n, d] the old rows
  const int32_t* adj0;        // the old graph, checked by k_hb_check
  const int32_t* up_expect;   // [n] first upper row of a node by the prefix rule (what the check held up_row to)
  const int32_t* adj_up;
  const int32_t* up_owner;    // [up_rows] the node an upper row belongs to
  const uint32_t* bits;       // the removal bitmap
  const int32_t* map;         // [n] old -> new id of a survivor (exclusive scan of the keep flags)
  const int32_t* out_up_row;  // [n_keep] the survivors' first upper rows, already written
  int32_t* out_adj0;
  int32_t* out_adj_up;
  unsigned long long* stats;  // {rows repaired, level-0 rows that came out empty, rows whose distinct pool exceeded 64}
  int n, d, M, keep_pruned;
  long long n_work;           // n level-0 rows, then the upper rows
};

// One wavefront per (old node, level).  A removed node's rows are dropped.  A surviving row none of whose entries is removed is
// copied through the map, slot for slot.  A row with a removed entry is repaired (FreshDiskANN alg. 4 with this builder's
// heuristic): the pool is the SET of the row's surviving entries and of the surviving entries of every removed entry's row on
// the same level (one hop; p itself left out), held as the beam of up to 64 nearest (distance to p, id) keys; wave_select
// picks the new row from it in ascending order.  Every row read belongs to a node of a checked graph on a level it has.
template <int LPR, int DT, int MT>
__global__ __launch_bounds__(kHbWaves * 64) void k_hb_repair(HbRepair r) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int GPW = 64 / LPR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long w = (long long)blockIdx.x * kHbWaves + wave;
  if (w >= r.n_work) return;
  int node, level;
  if (w < r.n) { node = (int)w; level = 0; }
  else { const long long u = w - r.n; node = r.up_owner[u]; level = (int)(u - r.up_expect[node]) + 1; }
  if (hb_removed(r.bits, node)) return;
  const int cap = level == 0 ? 2 * r.M : r.M;
  auto old_row = [&](int v) -> const int32_t* {
    return level == 0 ? r.adj0 + (size_t)v * 2 * r.M : r.adj_up + ((size_t)r.up_expect[v] + (size_t)(level - 1)) * r.M;
  };
  const int me = r.map[node];
  int32_t* dst = level == 0 ? r.out_adj0 + (size_t)me * 2 * r.M : r.out_adj_up + ((size_t)r.out_up_row[me] + (size_t)(level - 1)) * r.M;
  const int e = lane < cap ? old_row(node)[lane] : -1;
  const bool gone = e >= 0 && hb_removed(r.bits, e);
  const uint64_t holes = __ballot(gone);
  if (!holes) {
    if (lane < cap) dst[lane] = e >= 0 ? r.map[e] : -1;
    return;
  }
  const int sub = lane % LPR, grp = lane / LPR;
  const size_t row_bytes = (size_t)kHbMaxCand * r.d * 2;
  unsigned char* mine_lds = smem + (size_t)wave * (row_bytes + 1024);
  uint16_t* rows = reinterpret_cast<uint16_t*>(mine_lds);                   // wave_select's staging
  float* dist = reinterpret_cast<float*>(mine_lds + row_bytes);             // [64]
  int32_t* ids = reinterpret_cast<int32_t*>(mine_lds + row_bytes + 256);    // [64]
  unsigned long long* buf = reinterpret_cast<unsigned long long*>(mine_lds + row_bytes + 512);  // [64]
  float q[8];
  hb_load8<DT>(r.emb, (size_t)node, r.d, sub, q);
  unsigned long long beam = kKeyInf;
  bool over = false;
  // the surviving entries among one row's slots (one per lane) join the beam
  auto pool_add = [&](int id, bool member) {
    const uint64_t fm = __ballot(member);
    if (!fm) return;
    const int n_new = popc64(fm);
    if (member) ids[popc64(fm & lanemask_lt(lane))] = id;
    __builtin_amdgcn_wave_barrier();
    for (int i0 = 0; i0 < n_new; i0 += GPW) {  // distances to p, GPW rows per step
      const int i = i0 + grp;
      float x[8];
      hb_load8<DT>(r.emb, (size_t)ids[min(i, n_new - 1)], r.d, sub, x);
      float acc = 0.0f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if constexpr (MT == kHbIp) acc = __fmaf_rn(q[k], x[k], acc);
        else { const float t = q[k] - x[k]; acc = __fmaf_rn(t, t, acc); }
      }
      acc = hb_dist_of_sum<MT>(hb_group_sum<LPR>(acc));
      if (i < n_new && sub == 0) dist[i] = acc;
    }
    __builtin_amdgcn_wave_barrier();
    const unsigned long long fresh = lane < n_new ? hb_key<MT>(dist[lane], ids[lane]) : kKeyInf;
    __builtin_amdgcn_wave_barrier();
    int n_distinct;
    beam = wave_merge64_unique(beam, fresh, lane, buf, &n_distinct);
    over = over || n_distinct > kHbMaxCand;
  };
  pool_add(e, e >= 0 && !gone && e != node);
  for (uint64_t todo = holes; todo; todo &= todo - 1) {  // uniform
    const int v = __shfl(e, __ffsll((unsigned long long)todo) - 1);
    const int f = lane < cap ? old_row(v)[lane] : -1;
    pool_add(f, f >= 0 && f != node && !hb_removed(r.bits, f));
  }
  const int n_cand = popc64(__ballot(beam != kKeyInf));
  HbGraph g;
  g.emb = r.emb; g.adj0 = nullptr; g.cnt0 = nullptr; g.up_row = nullptr; g.adj_up = nullptr; g.cnt_up = nullptr;
  g.n_items = r.n; g.d = r.d; g.M = r.M; g.keep_pruned = r.keep_pruned;
  const uint64_t kept = wave_select<LPR, DT, MT, 1>(g, beam, n_cand, cap, rows, lane);
  const int n_kept = popc64(kept);
  if ((kept >> lane) & 1ull) dst[popc64(kept & lanemask_lt(lane))] = r.map[(int)(uint32_t)beam];
  if (lane >= n_kept && lane < cap) dst[lane] = -1;
  if (lane == 0) {
    atomicAdd(&r.stats[0], 1ull);
    if (level == 0 && n_kept == 0) atomicAdd(&r.stats[1], 1ull);
    if (over) atomicAdd(&r.stats[2], 1ull);
  }
}

// ---- orphans: the level-0 rows that a removal (or anything else) left empty or unnamed ----------------------------------------
// One wavefront per row, a slot per lane.  An entry outside [0, n) is skipped as if the slot were empty, so nothing is read or
// written beyond the bitmaps.  named: bit e set iff some row holds e; empty_bits: bit r set iff row r holds no entry.  Both are
// sets, so the order of the atomics does not show.
__global__ __launch_bounds__(kHbWaves * 64) void k_hb_orphan_mark(const int32_t* adj0, int n, int M, uint32_t* named, uint32_t* empty_bits) {
  const int lane = threadIdx.x & 63;
  const size_t at = (size_t)blockIdx.x * kHbWaves + (threadIdx.x >> 6);
  if (at >= (size_t)n) return;
  const int e = lane < 2 * M ? adj0[at * 2 * M + lane] : -1;
  const bool valid = e >= 0 && e < n;
  if (valid) atomicOr(&named[(uint32_t)e >> 5], 1u << (e & 31));
  if (__ballot(valid) == 0ull && lane == 0) atomicOr(&empty_bits[at >> 5], 1u << (at & 31));
}

// bits (in: the empty rows) |= the unnamed rows, bits at or beyond n cleared; *count += the rows set
__global__ void k_hb_orphan_bits(const uint32_t* named, int n, uint32_t* bits, unsigned long long* count) {
  const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t words = ((size_t)n + 31) / 32;
  if (w >= words) return;
  const uint32_t mask = (w == words - 1 && (n & 31)) ? (1u << (n & 31)) - 1u : 0xffffffffu;
  const uint32_t v = (bits[w] | ~named[w]) & mask;
  bits[w] = v;
  if (v) atomicAdd(count, (unsigned long long)__popc(v));
}

template <int LPR, int DT, int MT>
int run_repair(const HbRepair& r, hipStream_t st) {
  const size_t lds = ((size_t)kHbMaxCand * r.d * 2 + 1024) * kHbWaves;  // k_hb_backlink's budget
  auto kern = k_hb_repair<LPR, DT, MT>;
  if (lds > 48 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const unsigned blocks = (unsigned)((r.n_work + kHbWaves - 1) / kHbWaves);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(kHbWaves * 64), lds, st, r);
  HIP_TRY(hipGetLastError());
  return NANN_OK;
}

// ---- the host side (the header's HOST SIDE paragraph): first what build and append share, the scratch of a run -----------
struct HbScratch {
  int32_t *order = nullptr, *cnt0 = nullptr, *cnt_up = nullptr, *entry = nullptr, *run_first = nullptr, *run_len = nullptr;
  uint32_t *pair_dst = nullptr, *pair_src = nullptr, *pair_dst2 = nullptr, *pair_src2 = nullptr;
  int* n_runs = nullptr;
  void* sort = nullptr;
  size_t sort_bytes = 0;
  int max_batch = 16384, pair_cap = 0;
  // n_order: nodes this run inserts (+ the entry point of a build); n_nodes / up_rows: the whole graph's
  int alloc(size_t n_order, size_t n_nodes, int64_t up_rows, int M, HbOwned* own, hipStream_t st) {
    pair_cap = 2 * M;
    const size_t pairs = (size_t)max_batch * pair_cap;
    int rc;
    if ((rc = dev_alloc(&order, n_order, own)) || (rc = dev_alloc(&cnt0, n_nodes, own)) ||
        (rc = dev_alloc(&cnt_up, (size_t)std::max<int64_t>(up_rows, 1), own)) || (rc = dev_alloc(&entry, (size_t)max_batch, own)) ||
        (rc = dev_alloc(&pair_dst, pairs, own)) || (rc = dev_alloc(&pair_src, pairs, own)) || (rc = dev_alloc(&pair_dst2, pairs, own)) ||
        (rc = dev_alloc(&pair_src2, pairs, own)) || (rc = dev_alloc(&run_first, pairs, own)) || (rc = dev_alloc(&run_len, pairs, own)) ||
        (rc = dev_alloc(&n_runs, 1, own)))
      return rc;
    hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, pair_dst, pair_dst2, pair_src, pair_src2, max_batch * pair_cap, 0, 32, st);
    unsigned char* p;
    if ((rc = dev_alloc(&p, sort_bytes, own))) return rc;
    sort = p;
    return NANN_OK;
  }
};

int hb_hip_rc(hipError_t e, const char* what) {
  return e == hipSuccess ? NANN_OK : fail(NANN_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// The one walk over `levels`: *up_rows = the number of upper rows (the sum of levels - 1) and, where asked for, up_first[i] =
// node i's first upper row by the prefix rule (-1: one level).  Refused: a level < 1; with up_first (int32 rows) a total beyond
// 2^31 - 1, at the node that crosses it, before a caller sizes anything by it; with adj_up (the address of the caller's
// pointer) upper rows and no adj_up.
int hb_levels(const char* who, const int32_t* levels, int n, const int32_t* const* adj_up, std::vector<int32_t>* up_first,
              int64_t* up_rows) {
  if (up_first) up_first->resize((size_t)n);
  int64_t up = 0;
  for (int i = 0; i < n; ++i) {
    if (levels[i] < 1) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": levels must be >= 1");
    if (up_first) (*up_first)[(size_t)i] = levels[i] > 1 ? (int32_t)up : -1;
    up += levels[i] - 1;
    if (up_first && up > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": more than 2^31 - 1 upper rows");
  }
  if (adj_up && up > 0 && !*adj_up) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": adj_up is null");
  *up_rows = up;
  return NANN_OK;
}

// The check of a graph that is input (append, remove), before anything is written.  hb_check_enqueue puts on the stream: levels
// and the first upper rows the host derived go up, k_hb_check runs over the n nodes (fill counts -> cnt0 / cnt_up), the flags
// come back into c->h_bad.  The caller synchronises, once, with whatever else it has on the stream; hb_check_result then turns
// the flags into the refusal.
struct HbCheck {
  int32_t *levels = nullptr, *up_expect = nullptr, *bad = nullptr;  // on the device
  int32_t h_bad[kHbRules] = {kHbNone, kHbNone, kHbNone, kHbNone};
};

int hb_check_enqueue(const int32_t* adj0, const int32_t* up_row, const int32_t* adj_up, const int32_t* levels,
                     const std::vector<int32_t>& h_up, int n, int M, int32_t* cnt0, int32_t* cnt_up, HbCheck* c, HbOwned* own,
                     hipStream_t st) {
  int rc;
  if ((rc = dev_alloc(&c->levels, (size_t)n, own)) || (rc = dev_alloc(&c->up_expect, (size_t)n, own)) ||
      (rc = dev_alloc(&c->bad, (size_t)kHbRules, own)) ||
      (rc = hb_hip_rc(hipMemcpyAsync(c->levels, levels, (size_t)n * 4, hipMemcpyHostToDevice, st), "levels")) ||
      (rc = hb_hip_rc(hipMemcpyAsync(c->up_expect, h_up.data(), (size_t)n * 4, hipMemcpyHostToDevice, st), "up_row")) ||
      (rc = hb_hip_rc(hipMemcpyAsync(c->bad, c->h_bad, sizeof(c->h_bad), hipMemcpyHostToDevice, st), "flag")))
    return rc;
  hipLaunchKernelGGL(k_hb_check, dim3((unsigned)((n + kHbWaves - 1) / kHbWaves)), dim3(kHbWaves * 64), 0, st, adj0, up_row, adj_up,
                     c->levels, c->up_expect, n, M, cnt0, cnt_up, c->bad);
  if ((rc = hb_hip_rc(hipGetLastError(), "k_hb_check"))) return rc;
  return hb_hip_rc(hipMemcpyAsync(c->h_bad, c->bad, sizeof(c->h_bad), hipMemcpyDeviceToHost, st), "flag");
}

int hb_check_result(const char* who, const HbCheck& c) {
  static const char* const kRule[kHbRules] = {
      "up_row differs from what levels implies (-1 for one level, else the running sum of levels - 1)",
      "a row entry lies outside [-1, n_old)", "a row entry follows a -1 (rows are dense prefixes)",
      "a row entry names a node that has no row on that level"};
  for (int r = 0; r < kHbRules; ++r)
    if (c.h_bad[r] != kHbNone)
      return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": malformed graph, node " + std::to_string(c.h_bad[r]) + ": " + kRule[r]);
  return NANN_OK;
}

// (d, emb_dtype, metric), all checked by then -> the kernels' <LPR, DT, MT>: f(lpr, dt, mt) gets them as integral constants
template <int V>
using HbInt = std::integral_constant<int, V>;

template <typename F>
int hb_dispatch(int d, int emb_dtype, int metric, F&& f) {
  auto with_lpr = [&](auto lpr) -> int {
    auto with_dt = [&](auto dt) -> int { return metric == NANN_SCORER_IP ? f(lpr, dt, HbInt<kHbIp>{}) : f(lpr, dt, HbInt<kHbL2>{}); };
    return emb_dtype == NANN_F16 ? with_dt(HbInt<0>{}) : with_dt(HbInt<1>{});
  };
  return d == 64 ? with_lpr(HbInt<8>{}) : d == 128 ? with_lpr(HbInt<16>{}) : with_lpr(HbInt<32>{});
}

// The batch loop.  order[pos0 .. n_order) (also on the device, s.order) go into the graph `g`, which holds `base` nodes
// that are not in `order` (append: the old graph) and order[0 .. pos0) (build: the entry point); `entry` has `T` levels,
// the most of any node in it.  Same level count inside a batch; a batch is at most a quarter of what is already in the
// graph, <= 16384, <= batch_cap.  A node with MORE levels than the entry point (append only: a build inserts in descending
// order) is a batch of its own, searched and linked on the levels the graph has, T - 1 .. 0; its rows above stay empty,
// and it is the entry point from then on -- so no row is ever looked up on a level its node does not have.
int hb_insert(const char* who, const HbGraph& g, int emb_dtype, int metric, const int32_t* levels, const std::vector<int32_t>& order, int pos0, int64_t base,
              int entry, int T, int batch_cap, int ef, HbScratch& s, hipStream_t st) {
  const int n_order = (int)order.size(), d = g.d, pair_cap = s.pair_cap;
  std::vector<int32_t> h_entry((size_t)s.max_batch, entry);
  int rc;
  int pos = pos0;
  while (pos < n_order) {
    const int lv = levels[order[(size_t)pos]];  // number of levels of the batch's nodes
    int end = pos;
    const int64_t quarter = std::max<int64_t>(1, (base + pos) / 4);
    const int limit = lv > T ? 1 : (int)std::min<int64_t>(std::min(s.max_batch, batch_cap), quarter);
    while (end < n_order && end - pos < limit && levels[order[(size_t)end]] == lv) ++end;
    const int n = end - pos;
    if ((rc = hb_hip_rc(hipMemcpyAsync(s.entry, h_entry.data(), (size_t)n * 4, hipMemcpyHostToDevice, st), "entry"))) return rc;
    for (int level = T - 1; level >= 0; --level) {
      HbBatch b;
      b.nodes = s.order + pos; b.n = n; b.level = level;
      b.link = level <= lv - 1;
      b.ef = b.link ? ef : 1;
      b.entry = s.entry; b.pair_dst = s.pair_dst; b.pair_src = s.pair_src; b.pair_cap = pair_cap;
      if ((rc = hb_dispatch(d, emb_dtype, metric, [&](auto lpr, auto dt, auto mt) { return run_batch_level<lpr(), dt(), mt()>(g, b, st); })))
        return rc;
      if (!b.link) continue;
      const int n_pairs = n * pair_cap;
      if (hipcub::DeviceRadixSort::SortPairs(s.sort, s.sort_bytes, s.pair_dst, s.pair_dst2, s.pair_src, s.pair_src2, n_pairs, 0, 32, st) != hipSuccess)
        return fail(NANN_ERR_HIP, std::string(who) + ": radix sort failed");
      if ((rc = hb_hip_rc(hipMemsetAsync(s.n_runs, 0, 4, st), "n_runs"))) return rc;
      hipLaunchKernelGGL(k_hb_runs, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, st, s.pair_dst2, n_pairs, s.run_first, s.run_len, s.n_runs);
      if ((rc = hb_dispatch(d, emb_dtype, metric, [&](auto lpr, auto dt, auto mt) {
             return run_backlink<lpr(), dt(), mt()>(g, level, s.pair_dst2, s.pair_src2, s.run_first, s.run_len, s.n_runs, n_pairs, st);
           })))
        return rc;
    }
    if (lv > T) {
      if ((rc = hb_hip_rc(hipStreamSynchronize(st), "entry"))) return rc;  // the enqueued copies of h_entry have been read
      T = lv;
      std::fill(h_entry.begin(), h_entry.end(), order[(size_t)pos]);
    }
    pos = end;
  }
  return hb_hip_rc(hipStreamSynchronize(st), who);
}

// The nodes [n0, n) go in (a build: n0 = 0): their order goes up, and the tails of the arrays, theirs, become empty rows with the
// prefix rule continued -- up_row from h_up, upper rows [up0, up_rows).
int hb_new_rows(const HbScratch& s, const std::vector<int32_t>& order, const std::vector<int32_t>& h_up, int n0, int n, int64_t up0,
                int64_t up_rows, int M, int32_t* adj0, int32_t* up_row, int32_t* adj_up, hipStream_t st) {
  const size_t n_new = (size_t)(n - n0), up_new = (size_t)(up_rows - up0);
  int rc;
  if ((rc = hb_hip_rc(hipMemcpyAsync(s.order, order.data(), order.size() * 4, hipMemcpyHostToDevice, st), "order")) ||
      (rc = hb_hip_rc(hipMemcpyAsync(up_row + n0, h_up.data() + n0, n_new * 4, hipMemcpyHostToDevice, st), "up_row")) ||
      (rc = hb_hip_rc(hipMemsetAsync(adj0 + (size_t)n0 * 2 * M, 0xff, n_new * 2 * M * 4, st), "adj0")) ||
      (rc = hb_hip_rc(hipMemsetAsync(s.cnt0 + n0, 0, n_new * 4, st), "cnt0")))
    return rc;
  if (up_new > 0 && ((rc = hb_hip_rc(hipMemsetAsync(adj_up + (size_t)up0 * M, 0xff, up_new * M * 4, st), "adj_up")) ||
                     (rc = hb_hip_rc(hipMemsetAsync(s.cnt_up + up0, 0, up_new * 4, st), "cnt_up"))))
    return rc;
  return NANN_OK;
}

// the limits build, append and remove share, checked before anything is launched or written: the metric (a nann_scorer_kind),
// then the shape
int hb_check_args(const char* who, int32_t metric, int64_t n_total, int32_t d, int32_t emb_dtype, int32_t M, int ef) {
  const std::string w(who);
  if (metric == NANN_SCORER_MLP) return fail(NANN_ERR_UNSUPPORTED, w + ": rows are linked by L2 or inner product, not by a model");
  if (metric != NANN_SCORER_L2 && metric != NANN_SCORER_IP)
    return fail(NANN_ERR_BAD_ARGUMENT, w + ": metric must be NANN_SCORER_L2 or NANN_SCORER_IP");
  if (n_total > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, w + ": more than 2^31 - 1 items");
  if (!(d == 64 || d == 128 || d == 256)) return fail(NANN_ERR_UNSUPPORTED, w + ": d must be 64, 128 or 256");
  if (emb_dtype != NANN_F16 && emb_dtype != NANN_BF16) return fail(NANN_ERR_UNSUPPORTED, w + ": f16 or bf16 rows");
  if (M < 2 || 2 * M > kHbMaxCand) return fail(NANN_ERR_UNSUPPORTED, w + ": 2 <= M <= 32");
  if (ef > kHbMaxEf) return fail(NANN_ERR_UNSUPPORTED, w + ": ef_construction <= 40 in this build");
  return NANN_OK;
}

constexpr int kHbAppendDiv = 64;  // an append goes in in at least this many batches (8 and 32 measured short)

// the arguments the two export calls share
int hb_export_args(const char* who, const void* adj0, const void* up_row, const int32_t* levels, int64_t n, int32_t M,
                   int32_t start_level) {
  const std::string w(who);
  if (!adj0 || !up_row || !levels || n < 1) return fail(NANN_ERR_BAD_ARGUMENT, w + ": null argument or n < 1");
  if (n > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, w + ": more than 2^31 - 1 items");
  if (M < 2 || 2 * M > kHbMaxCand) return fail(NANN_ERR_UNSUPPORTED, w + ": 2 <= M <= 32");
  if (start_level != 2) return fail(NANN_ERR_UNSUPPORTED, w + ": start_level must be 2 (the levels serving walks)");
  return NANN_OK;
}

// the old -> new map of a removal on the stream: keep flags, their exclusive scan into `map`; the bitmap also comes to the
// host (h_bits, ceil(n / 32) words), where the survivors' levels are walked.  The caller synchronises.
int hb_remove_map(const char* who, const uint32_t* remove_bits, int N, int32_t** map, std::vector<uint32_t>* h_bits, HbOwned* own,
                  hipStream_t st) {
  int32_t* flag;
  int rc;
  if ((rc = dev_alloc(&flag, (size_t)N, own)) || (rc = dev_alloc(map, (size_t)N, own))) return rc;
  size_t scan_bytes = 0;
  hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, flag, *map, N, st);
  unsigned char* d_scan;
  if ((rc = dev_alloc(&d_scan, scan_bytes, own))) return rc;
  hipLaunchKernelGGL(k_hb_keep_flags, dim3((unsigned)(((size_t)N + 255) / 256)), dim3(256), 0, st, remove_bits, N, flag);
  if ((rc = hb_hip_rc(hipGetLastError(), "k_hb_keep_flags"))) return rc;
  if (hipcub::DeviceScan::ExclusiveSum(d_scan, scan_bytes, flag, *map, N, st) != hipSuccess)
    return fail(NANN_ERR_HIP, std::string(who) + ": scan failed");
  h_bits->resize(((size_t)N + 31) / 32);
  return hb_hip_rc(hipMemcpyAsync(h_bits->data(), remove_bits, h_bits->size() * 4, hipMemcpyDeviceToHost, st), "remove_bits");
}

inline bool hb_bit(const std::vector<uint32_t>& bits, int i) { return (bits[(size_t)i >> 5] >> (i & 31)) & 1u; }

}  // namespace

extern "C" {

int nann_hnsw_draw_levels(int64_t n_items, int32_t M, uint64_t seed, int32_t* levels, int64_t* n_up_rows) {
  if (n_items <= 0 || M < 2 || !levels) return fail(NANN_ERR_BAD_ARGUMENT, "nann_hnsw_draw_levels: bad argument");
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  const double mult = 1.0 / std::log((double)M);
  int64_t up = 0;
  for (int64_t i = 0; i < n_items; ++i) {
    double u = uni(rng);
    if (u < 1e-300) u = 1e-300;
    const int lv = (int)std::floor(-std::log(u) * mult) + 1;  // Faiss convention: number of levels
    levels[i] = lv;
    up += lv - 1;
  }
  if (n_up_rows) *n_up_rows = up;
  return NANN_OK;
}

int nann_hnsw_build_device(const void* item_embs, int64_t n_items, int32_t d, int32_t emb_dtype, int32_t M,
                           int32_t ef_construction, const int32_t* levels, int32_t* adj0, int32_t* up_row,
                           int32_t* adj_up, nann_stream_t stream) {
  return nann_hnsw_build_device_metric(item_embs, n_items, d, emb_dtype, M, ef_construction, 0, NANN_SCORER_L2, levels, adj0, up_row, adj_up, stream);
}

int nann_hnsw_build_device_ex(const void* item_embs, int64_t n_items, int32_t d, int32_t emb_dtype, int32_t M,
                              int32_t ef_construction, int32_t keep_pruned, const int32_t* levels, int32_t* adj0,
                              int32_t* up_row, int32_t* adj_up, nann_stream_t stream) {
  return nann_hnsw_build_device_metric(item_embs, n_items, d, emb_dtype, M, ef_construction, keep_pruned, NANN_SCORER_L2, levels, adj0, up_row, adj_up, stream);
}

int nann_hnsw_build_device_metric(const void* item_embs, int64_t n_items, int32_t d, int32_t emb_dtype, int32_t M,
                                  int32_t ef_construction, int32_t keep_pruned, int32_t metric, const int32_t* levels,
                                  int32_t* adj0, int32_t* up_row, int32_t* adj_up, nann_stream_t stream) {
  const char* who = "nann_hnsw_build_device";
  if (!item_embs || !levels || !adj0 || !up_row || n_items <= 0) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  const int ef = ef_construction > 0 ? ef_construction : 40;
  int rc = hb_check_args(who, metric, n_items, d, emb_dtype, M, ef);
  if (rc) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int N = (int)n_items;
  std::vector<int32_t> h_up;
  int64_t up_rows = 0;
  if ((rc = hb_levels(who, levels, N, &adj_up, &h_up, &up_rows))) return rc;
  // ---- insertion order: top level first, ascending id inside a level (Faiss adds the highest levels first)
  std::vector<int32_t> order((size_t)N);
  for (int i = 0; i < N; ++i) order[(size_t)i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return levels[a] > levels[b]; });

  HbOwned own;
  HbScratch s;
  if ((rc = s.alloc((size_t)N, (size_t)N, up_rows, M, &own, st)) ||
      (rc = hb_new_rows(s, order, h_up, 0, N, 0, up_rows, M, adj0, up_row, adj_up, st)))
    return rc;
  HbGraph g;
  g.emb = item_embs; g.adj0 = adj0; g.cnt0 = s.cnt0; g.up_row = up_row; g.adj_up = adj_up; g.cnt_up = s.cnt_up;
  g.n_items = N; g.d = d; g.M = M; g.keep_pruned = keep_pruned ? 1 : 0;
  // order[0] is the entry point: inserted with no links
  return hb_insert(who, g, emb_dtype, metric, levels, order, 1, 0, order[0], levels[order[0]], 0x7fffffff, ef, s, st);
}

int nann_hnsw_append_device(const void* item_embs, int64_t n_old, int64_t n_new, int32_t d, int32_t emb_dtype, int32_t M,
                            int32_t ef_construction, int32_t keep_pruned, const int32_t* levels, int32_t* adj0,
                            int32_t* up_row, int32_t* adj_up, nann_stream_t stream) {
  return nann_hnsw_append_device_metric(item_embs, n_old, n_new, d, emb_dtype, M, ef_construction, keep_pruned, NANN_SCORER_L2, levels, adj0, up_row, adj_up, stream);
}

int nann_hnsw_append_device_metric(const void* item_embs, int64_t n_old, int64_t n_new, int32_t d, int32_t emb_dtype, int32_t M,
                                   int32_t ef_construction, int32_t keep_pruned, int32_t metric, const int32_t* levels,
                                   int32_t* adj0, int32_t* up_row, int32_t* adj_up, nann_stream_t stream) {
  const char* who = "nann_hnsw_append_device";
  if (!item_embs || !levels || !adj0 || !up_row || n_old < 1 || n_new < 0)
    return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument, n_old < 1 or n_new < 0");
  const int ef = ef_construction > 0 ? ef_construction : 40;
  int rc = hb_check_args(who, metric, n_old > 0x7fffffffll - n_new ? 0x80000000ll : n_old + n_new, d, emb_dtype, M, ef);
  if (rc) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int N0 = (int)n_old, N1 = (int)n_new, N = N0 + N1;
  std::vector<int32_t> h_up;
  int64_t up_rows = 0, up_rows_old = 0;
  if ((rc = hb_levels(who, levels, N, &adj_up, &h_up, &up_rows))) return rc;
  // ---- the old graph's entry point and upper rows, the new nodes' order
  int entry = 0;
  for (int i = 0; i < N0; ++i) {
    if (levels[i] > levels[entry]) entry = i;  // the lowest id among the nodes with the most levels
    up_rows_old += levels[i] - 1;
  }
  std::vector<int32_t> order((size_t)N1);
  for (int i = 0; i < N1; ++i) order[(size_t)i] = N0 + i;
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return levels[a] > levels[b]; });

  HbOwned own;
  HbScratch s;
  HbCheck check;
  // ---- the old graph is checked before anything is written: one pass, one flag back
  if ((rc = s.alloc((size_t)std::max(N1, 1), (size_t)N, up_rows, M, &own, st)) ||
      (rc = hb_check_enqueue(adj0, up_row, adj_up, levels, h_up, N0, M, s.cnt0, s.cnt_up, &check, &own, st)) ||
      (rc = hb_hip_rc(hipStreamSynchronize(st), "k_hb_check")) || (rc = hb_check_result(who, check)))
    return rc;
  if (N1 == 0) return NANN_OK;
  if ((rc = hb_new_rows(s, order, h_up, N0, N, up_rows_old, up_rows, M, adj0, up_row, adj_up, st))) return rc;
  HbGraph g;
  g.emb = item_embs; g.adj0 = adj0; g.cnt0 = s.cnt0; g.up_row = up_row; g.adj_up = adj_up; g.cnt_up = s.cnt_up;
  g.n_items = N; g.d = d; g.M = M; g.keep_pruned = keep_pruned ? 1 : 0;
  const int batch_cap = std::max(1, (N1 + kHbAppendDiv - 1) / kHbAppendDiv);
  return hb_insert(who, g, emb_dtype, metric, levels, order, 0, n_old, entry, levels[entry], batch_cap, ef, s, st);
}

int nann_hnsw_export_count(const int32_t* adj0, const int32_t* up_row, const int32_t* adj_up, const int32_t* levels, int64_t n,
                           int32_t M, int32_t start_level, int64_t* row_splits0, int64_t* row_splits1, int64_t* nnz,
                           int64_t* n_enter, nann_stream_t stream) {
  const char* who = "nann_hnsw_export_count";
  int rc = hb_export_args(who, adj0, up_row, levels, n, M, start_level);
  if (rc) return rc;
  if (!row_splits0 || !row_splits1 || !nnz || !n_enter) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null output");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int N = (int)n;
  int64_t n_up = 0, enter = 0;
  if ((rc = hb_levels(who, levels, N, &adj_up, nullptr, &n_up))) return rc;
  for (int i = 0; i < N; ++i) enter += levels[i] > start_level;
  HbOwned own;
  int32_t* d_levels;
  int64_t* d_len;
  int* d_bad;
  if ((rc = dev_alloc(&d_levels, (size_t)N, &own)) || (rc = dev_alloc(&d_len, (size_t)N * 2, &own)) || (rc = dev_alloc(&d_bad, 1, &own)))
    return rc;
  size_t scan_bytes = 0;
  hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, d_len, row_splits0 + 1, N, st);
  unsigned char* d_scan;
  if ((rc = dev_alloc(&d_scan, scan_bytes, &own)) ||
      (rc = hb_hip_rc(hipMemcpyAsync(d_levels, levels, (size_t)N * 4, hipMemcpyHostToDevice, st), "levels")) ||
      (rc = hb_hip_rc(hipMemsetAsync(d_bad, 0, 4, st), "flag")) ||
      (rc = hb_hip_rc(hipMemsetAsync(row_splits0, 0, 8, st), "row_splits")) ||
      (rc = hb_hip_rc(hipMemsetAsync(row_splits1, 0, 8, st), "row_splits")))
    return rc;
  hipLaunchKernelGGL(k_hb_export_count, dim3((unsigned)((N + kHbWaves - 1) / kHbWaves)), dim3(kHbWaves * 64), 0, st, adj0, up_row,
                     adj_up, d_levels, N, n_up, M, d_len, d_len + N, d_bad);
  if ((rc = hb_hip_rc(hipGetLastError(), "k_hb_export_count"))) return rc;
  if (hipcub::DeviceScan::InclusiveSum(d_scan, scan_bytes, d_len, row_splits0 + 1, N, st) != hipSuccess ||
      hipcub::DeviceScan::InclusiveSum(d_scan, scan_bytes, d_len + N, row_splits1 + 1, N, st) != hipSuccess)
    return fail(NANN_ERR_HIP, std::string(who) + ": scan failed");
  int h_bad = 0;
  if ((rc = hb_hip_rc(hipMemcpyAsync(&nnz[0], row_splits0 + N, 8, hipMemcpyDeviceToHost, st), "nnz")) ||
      (rc = hb_hip_rc(hipMemcpyAsync(&nnz[1], row_splits1 + N, 8, hipMemcpyDeviceToHost, st), "nnz")) ||
      (rc = hb_hip_rc(hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, st), "flag")) ||
      (rc = hb_hip_rc(hipStreamSynchronize(st), who)))
    return rc;
  if (h_bad) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": an up_row entry lies outside adj_up");
  *n_enter = enter;
  return NANN_OK;
}

int nann_hnsw_export_fill(const int32_t* adj0, const int32_t* up_row, const int32_t* adj_up, const int32_t* levels, int64_t n,
                          int32_t M, int32_t start_level, const int64_t* row_splits0, const int64_t* row_splits1,
                          const int64_t* nnz, int32_t* values0, int32_t* values1, int32_t* enter_points, nann_stream_t stream) {
  const char* who = "nann_hnsw_export_fill";
  int rc = hb_export_args(who, adj0, up_row, levels, n, M, start_level);
  if (rc) return rc;
  if (!row_splits0 || !row_splits1 || !nnz) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null row_splits or nnz");
  if (nnz[0] < 0 || nnz[1] < 0 || (nnz[0] > 0 && !values0) || (nnz[1] > 0 && !values1))
    return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": nnz < 0 or values is null");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int N = (int)n;
  int64_t n_up = 0;
  if ((rc = hb_levels(who, levels, N, nullptr, nullptr, &n_up))) return rc;
  std::vector<int32_t> enter;
  for (int i = 0; i < N; ++i)
    if (levels[i] > start_level) enter.push_back(i);
  if ((n_up > 0 && !adj_up) || (!enter.empty() && !enter_points))
    return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": adj_up or enter_points is null");
  HbOwned own;
  int32_t* d_levels;
  int* d_bad;
  if ((rc = dev_alloc(&d_levels, (size_t)N, &own)) || (rc = dev_alloc(&d_bad, 1, &own)) ||
      (rc = hb_hip_rc(hipMemcpyAsync(d_levels, levels, (size_t)N * 4, hipMemcpyHostToDevice, st), "levels")) ||
      (rc = hb_hip_rc(hipMemsetAsync(d_bad, 0, 4, st), "flag")))
    return rc;
  if (!enter.empty() &&
      (rc = hb_hip_rc(hipMemcpyAsync(enter_points, enter.data(), enter.size() * 4, hipMemcpyHostToDevice, st), "enter_points")))
    return rc;
  hipLaunchKernelGGL(k_hb_export_fill, dim3((unsigned)((N + kHbWaves - 1) / kHbWaves)), dim3(kHbWaves * 64), 0, st, adj0, up_row,
                     adj_up, d_levels, N, n_up, M, row_splits0, row_splits1, nnz[0], nnz[1], values0, values1, d_bad);
  int h_bad = 0;
  if ((rc = hb_hip_rc(hipGetLastError(), "k_hb_export_fill")) ||
      (rc = hb_hip_rc(hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, st), "flag")) ||
      (rc = hb_hip_rc(hipStreamSynchronize(st), who)))
    return rc;
  if (h_bad) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": row_splits are not this graph's (call nann_hnsw_export_count first)");
  return NANN_OK;
}

int nann_hnsw_remove_count(const uint32_t* remove_bits, const int32_t* levels, int64_t n, int32_t* kept_rows,
                           int32_t* new_levels, int64_t* n_keep, int64_t* n_up_rows, nann_stream_t stream) {
  const char* who = "nann_hnsw_remove_count";
  if (!remove_bits || !levels || !kept_rows || !new_levels || !n_keep || !n_up_rows || n < 1)
    return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument or n < 1");
  if (n > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": more than 2^31 - 1 items");
  const int N = (int)n;
  int64_t up_old = 0;  // not asked for: the survivors' is
  int rc = hb_levels(who, levels, N, nullptr, nullptr, &up_old);
  if (rc) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  HbOwned own;
  int32_t* map;
  std::vector<uint32_t> h_bits;
  if ((rc = hb_remove_map(who, remove_bits, N, &map, &h_bits, &own, st))) return rc;
  hipLaunchKernelGGL(k_hb_kept_rows, dim3((unsigned)(((size_t)N + 255) / 256)), dim3(256), 0, st, remove_bits, map, N, kept_rows);
  if ((rc = hb_hip_rc(hipGetLastError(), "k_hb_kept_rows")) || (rc = hb_hip_rc(hipStreamSynchronize(st), who))) return rc;
  int64_t keep = 0, up = 0;
  for (int i = 0; i < N; ++i) {
    if (hb_bit(h_bits, i)) continue;
    new_levels[keep++] = levels[i];
    up += levels[i] - 1;
  }
  *n_keep = keep;
  *n_up_rows = up;
  return NANN_OK;
}

int nann_hnsw_remove_device(const void* item_embs, int64_t n, int32_t d, int32_t emb_dtype, int32_t M, int32_t keep_pruned,
                            int32_t metric, const int32_t* levels, const int32_t* adj0, const int32_t* up_row,
                            const int32_t* adj_up, const uint32_t* remove_bits, int64_t n_keep, int32_t* out_adj0,
                            int32_t* out_up_row, int32_t* out_adj_up, int64_t* stats, nann_stream_t stream) {
  const char* who = "nann_hnsw_remove_device";
  if (!item_embs || !levels || !adj0 || !up_row || !remove_bits || !out_adj0 || !out_up_row || !out_adj_up || n < 1)
    return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument or n < 1");
  if (n_keep < 1 || n_keep > n)
    return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": n_keep must lie in [1, n] (a graph keeps at least one node)");
  int rc = hb_check_args(who, metric, n, d, emb_dtype, M, 0);
  if (rc) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int N = (int)n;
  std::vector<int32_t> h_up, h_owner;
  int64_t up_rows = 0;
  if ((rc = hb_levels(who, levels, N, &adj_up, &h_up, &up_rows))) return rc;
  // ---- the owner of every upper row: grown only now that their number is known to be in range
  h_owner.reserve((size_t)up_rows);
  for (int i = 0; i < N; ++i) h_owner.insert(h_owner.end(), (size_t)(levels[i] - 1), i);

  HbOwned own;
  HbCheck check;
  // ---- the old graph is checked, and the bitmap scanned, before anything is written
  int32_t *d_owner, *cnt0, *cnt_up, *map;
  unsigned long long* d_stats;
  if ((rc = dev_alloc(&d_owner, (size_t)std::max<int64_t>(up_rows, 1), &own)) || (rc = dev_alloc(&cnt0, (size_t)N, &own)) ||
      (rc = dev_alloc(&cnt_up, (size_t)std::max<int64_t>(up_rows, 1), &own)) || (rc = dev_alloc(&d_stats, 3, &own)) ||
      (rc = hb_hip_rc(hipMemsetAsync(d_stats, 0, 3 * sizeof(unsigned long long), st), "stats")))
    return rc;
  if (up_rows > 0 && (rc = hb_hip_rc(hipMemcpyAsync(d_owner, h_owner.data(), (size_t)up_rows * 4, hipMemcpyHostToDevice, st), "owner")))
    return rc;
  std::vector<uint32_t> h_bits;
  if ((rc = hb_check_enqueue(adj0, up_row, adj_up, levels, h_up, N, M, cnt0, cnt_up, &check, &own, st)) ||
      (rc = hb_remove_map(who, remove_bits, N, &map, &h_bits, &own, st)) ||
      (rc = hb_hip_rc(hipStreamSynchronize(st), "k_hb_check")) || (rc = hb_check_result(who, check)))
    return rc;
  // ---- the survivors: their count against n_keep, their first upper rows by the prefix rule
  std::vector<int32_t> h_new_up;
  h_new_up.reserve((size_t)n_keep);
  int64_t keep = 0, new_up_rows = 0;
  for (int i = 0; i < N; ++i) {
    if (hb_bit(h_bits, i)) continue;
    if (++keep <= n_keep) h_new_up.push_back(levels[i] > 1 ? (int32_t)new_up_rows : -1);
    new_up_rows += levels[i] - 1;
  }
  if (keep != n_keep)
    return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": n_keep is " + std::to_string(n_keep) + ", the bitmap leaves " +
                                           std::to_string(keep) + " rows (call nann_hnsw_remove_count first)");
  if ((rc = hb_hip_rc(hipMemcpyAsync(out_up_row, h_new_up.data(), (size_t)n_keep * 4, hipMemcpyHostToDevice, st), "out_up_row")))
    return rc;
  HbRepair r;
  r.emb = item_embs; r.adj0 = adj0; r.up_expect = check.up_expect; r.adj_up = adj_up; r.up_owner = d_owner; r.bits = remove_bits; r.map = map;
  r.out_up_row = out_up_row; r.out_adj0 = out_adj0; r.out_adj_up = out_adj_up; r.stats = d_stats;
  r.n = N; r.d = d; r.M = M; r.keep_pruned = keep_pruned ? 1 : 0; r.n_work = (long long)N + up_rows;
  unsigned long long h_stats[3] = {0, 0, 0};
  if ((rc = hb_dispatch(d, emb_dtype, metric, [&](auto lpr, auto dt, auto mt) { return run_repair<lpr(), dt(), mt()>(r, st); })) ||
      (rc = hb_hip_rc(hipMemcpyAsync(h_stats, d_stats, sizeof(h_stats), hipMemcpyDeviceToHost, st), "stats")) ||
      (rc = hb_hip_rc(hipStreamSynchronize(st), who)))
    return rc;
  if (stats) {
    for (int i = 0; i < 3; ++i) stats[i] = (int64_t)h_stats[i];
    stats[3] = n_keep;
  }
  return NANN_OK;
}

int nann_hnsw_update_device(const void* item_embs, int64_t n, int32_t d, int32_t emb_dtype, int32_t M, int32_t ef_construction,
                            int32_t keep_pruned, int32_t metric, const int32_t* levels, const int32_t* adj0, const int32_t* up_row,
                            const int32_t* adj_up, const uint32_t* update_bits, int32_t* out_adj0, int32_t* out_up_row,
                            int32_t* out_adj_up, int64_t* stats, nann_stream_t stream) {
  const char* who = "nann_hnsw_update_device";
  if (!item_embs || !levels || !adj0 || !up_row || !update_bits || !out_adj0 || !out_up_row || !out_adj_up || n < 1)
    return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument or n < 1");
  const int ef = ef_construction > 0 ? ef_construction : 40;
  int rc = hb_check_args(who, metric, n, d, emb_dtype, M, ef);
  if (rc) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int N = (int)n;
  std::vector<int32_t> h_up, h_owner;
  int64_t up_rows = 0;
  if ((rc = hb_levels(who, levels, N, &adj_up, &h_up, &up_rows))) return rc;
  h_owner.reserve((size_t)up_rows);
  for (int i = 0; i < N; ++i) h_owner.insert(h_owner.end(), (size_t)(levels[i] - 1), i);

  HbOwned own;
  HbScratch s;
  HbCheck check;
  // ---- the old graph is checked, and the bitmap brought to the host, before anything is written
  int32_t *d_owner, *ident, *bad2;
  unsigned long long* d_stats;
  const size_t words = ((size_t)N + 31) / 32;
  std::vector<uint32_t> h_bits(words);
  if ((rc = s.alloc((size_t)N, (size_t)N, up_rows, M, &own, st)) || (rc = dev_alloc(&d_owner, (size_t)std::max<int64_t>(up_rows, 1), &own)) ||
      (rc = dev_alloc(&ident, (size_t)N, &own)) || (rc = dev_alloc(&bad2, (size_t)kHbRules, &own)) || (rc = dev_alloc(&d_stats, 3, &own)) ||
      (rc = hb_hip_rc(hipMemsetAsync(d_stats, 0, 3 * sizeof(unsigned long long), st), "stats")) ||
      (rc = hb_hip_rc(hipMemcpyAsync(h_bits.data(), update_bits, words * 4, hipMemcpyDeviceToHost, st), "update_bits")) ||
      (rc = hb_check_enqueue(adj0, up_row, adj_up, levels, h_up, N, M, s.cnt0, s.cnt_up, &check, &own, st)) ||
      (rc = hb_hip_rc(hipStreamSynchronize(st), "k_hb_check")) || (rc = hb_check_result(who, check)))
    return rc;
  // ---- the marked nodes in the order they go back in, and the entry point among those that stay
  std::vector<int32_t> order;
  int entry = -1;
  for (int i = 0; i < N; ++i) {
    if (hb_bit(h_bits, i)) order.push_back(i);
    else if (entry < 0 || levels[i] > levels[entry]) entry = i;  // the lowest id among the staying nodes with the most levels
  }
  const int n_marked = (int)order.size();
  if (n_marked == N)
    return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": every row is marked, nothing stays to link to (that is a build)");
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return levels[a] > levels[b]; });
  // ---- detach: the removal's repair under the identity map; the marked nodes' rows stay the empty rows written here
  std::vector<int32_t> h_ident((size_t)N);
  for (int i = 0; i < N; ++i) h_ident[(size_t)i] = i;
  if ((rc = hb_hip_rc(hipMemcpyAsync(ident, h_ident.data(), (size_t)N * 4, hipMemcpyHostToDevice, st), "map")) ||
      (rc = hb_hip_rc(hipMemcpyAsync(out_up_row, h_up.data(), (size_t)N * 4, hipMemcpyHostToDevice, st), "out_up_row")) ||
      (rc = hb_hip_rc(hipMemsetAsync(out_adj0, 0xff, (size_t)N * 2 * M * 4, st), "out_adj0")))
    return rc;
  if (up_rows > 0 && ((rc = hb_hip_rc(hipMemcpyAsync(d_owner, h_owner.data(), (size_t)up_rows * 4, hipMemcpyHostToDevice, st), "owner")) ||
                      (rc = hb_hip_rc(hipMemsetAsync(out_adj_up, 0xff, (size_t)up_rows * M * 4, st), "out_adj_up"))))
    return rc;
  HbRepair r;
  r.emb = item_embs; r.adj0 = adj0; r.up_expect = check.up_expect; r.adj_up = adj_up; r.up_owner = d_owner; r.bits = update_bits; r.map = ident;
  r.out_up_row = out_up_row; r.out_adj0 = out_adj0; r.out_adj_up = out_adj_up; r.stats = d_stats;
  r.n = N; r.d = d; r.M = M; r.keep_pruned = keep_pruned ? 1 : 0; r.n_work = (long long)N + up_rows;
  unsigned long long h_stats[3] = {0, 0, 0};
  if ((rc = hb_dispatch(d, emb_dtype, metric, [&](auto lpr, auto dt, auto mt) { return run_repair<lpr(), dt(), mt()>(r, st); })) ||
      (rc = hb_hip_rc(hipMemcpyAsync(h_stats, d_stats, sizeof(h_stats), hipMemcpyDeviceToHost, st), "stats")))
    return rc;
  if (n_marked > 0) {
    // ---- the fill counts of the new arrays: the check's pass over them (its flags go nowhere: these rows are the call's own)
    hipLaunchKernelGGL(k_hb_check, dim3((unsigned)((N + kHbWaves - 1) / kHbWaves)), dim3(kHbWaves * 64), 0, st, out_adj0, out_up_row,
                       out_adj_up, check.levels, check.up_expect, N, M, s.cnt0, s.cnt_up, bad2);
    if ((rc = hb_hip_rc(hipGetLastError(), "k_hb_check")) ||
        (rc = hb_hip_rc(hipMemcpyAsync(s.order, order.data(), order.size() * 4, hipMemcpyHostToDevice, st), "order")))
      return rc;
    // ---- re-insert, as an append of the marked nodes onto the staying ones
    HbGraph g;
    g.emb = item_embs; g.adj0 = out_adj0; g.cnt0 = s.cnt0; g.up_row = out_up_row; g.adj_up = out_adj_up; g.cnt_up = s.cnt_up;
    g.n_items = N; g.d = d; g.M = M; g.keep_pruned = keep_pruned ? 1 : 0;
    const int batch_cap = std::max(1, (n_marked + kHbAppendDiv - 1) / kHbAppendDiv);
    if ((rc = hb_insert(who, g, emb_dtype, metric, levels, order, 0, (int64_t)(N - n_marked), entry, levels[entry], batch_cap, ef, s, st)))
      return rc;
  } else if ((rc = hb_hip_rc(hipStreamSynchronize(st), who))) {
    return rc;
  }
  if (stats) {
    for (int i = 0; i < 3; ++i) stats[i] = (int64_t)h_stats[i];
    stats[3] = n_marked;
  }
  return NANN_OK;
}

int nann_hnsw_orphan_bits(const int32_t* adj0, int64_t n, int32_t M, uint32_t* out_bits, int64_t* n_orphans, nann_stream_t stream) {
  const char* who = "nann_hnsw_orphan_bits";
  if (!adj0 || !out_bits || !n_orphans || n < 1) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument or n < 1");
  if (n > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": more than 2^31 - 1 items");
  if (M < 2 || 2 * M > kHbMaxCand) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": 2 <= M <= 32");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int N = (int)n;
  const size_t words = ((size_t)N + 31) / 32;
  HbOwned own;
  uint32_t* named;
  unsigned long long* d_count;
  unsigned long long h_count = 0;
  int rc;
  if ((rc = dev_alloc(&named, words, &own)) || (rc = dev_alloc(&d_count, 1, &own)) ||
      (rc = hb_hip_rc(hipMemsetAsync(named, 0, words * 4, st), "named")) ||
      (rc = hb_hip_rc(hipMemsetAsync(out_bits, 0, words * 4, st), "out_bits")) ||
      (rc = hb_hip_rc(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), st), "count")))
    return rc;
  hipLaunchKernelGGL(k_hb_orphan_mark, dim3((unsigned)((N + kHbWaves - 1) / kHbWaves)), dim3(kHbWaves * 64), 0, st, adj0, N, M, named, out_bits);
  if ((rc = hb_hip_rc(hipGetLastError(), "k_hb_orphan_mark"))) return rc;
  hipLaunchKernelGGL(k_hb_orphan_bits, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, named, N, out_bits, d_count);
  if ((rc = hb_hip_rc(hipGetLastError(), "k_hb_orphan_bits")) ||
      (rc = hb_hip_rc(hipMemcpyAsync(&h_count, d_count, sizeof(h_count), hipMemcpyDeviceToHost, st), "count")) ||
      (rc = hb_hip_rc(hipStreamSynchronize(st), who)))
    return rc;
  *n_orphans = (int64_t)h_count;
  return NANN_OK;
}

}  // extern "C"
