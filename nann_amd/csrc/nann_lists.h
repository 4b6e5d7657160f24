// nann_lists.h -- shared-list search (nann_search_lists): every query of a batch names up to NANN_LISTS_MAX_PROBE of the row
// lists of a nann_partition (the cells of a coarse partition, a category, a seller's stock), and gets the exact top k of their
// concatenation -- slot order, each list in its stored order -- with the bits, the order and the counts nann_search_candidates
// gives on that concatenation.  The reference has no such call; nothing here restates a line of it.
//
// What the candidate-list search cannot do: a list probed by many queries is fetched ONCE PER TILE of 16 probing queries, the
// way k_scan_l2 fetches a row of the table once per tile (nann_scan.h) -- one thread owns a row, the tile's queries arrive
// through the scalar cache, a row is converted once and serves all 16.
//
// Per chunk of queries (S = the longest concatenation a query can name, n_probe x the longest list and at least k; the chunk is
// min(128, 512 MiB / 4 S) queries in whole tiles of 16):
//   1. k_lists_plan (one workgroup): validates the slots, gives every (query, slot) pair its offset in the query's concatenation
//      (the prefix of the list lengths in slot order; its end is len_q), sorts the pairs by list (a bitonic sort in LDS of the
//      keys list << 13 | pair number: unique, so the order is fixed and stable), cuts every list's run of pairs into tiles of 16
//      and writes per tile the list, the 16 (query, offset) destinations and the exclusive prefix of ceil(len / 256) row blocks;
//      the numbers of tiles and of work items go to device memory.
//   2. k_lists_tile_q: qT[tile][e][i] of every tile, k_scan_transpose_q's layout (a short tile repeats its last query).
//   3. k_lists_scan_l2 / k_lists_scan_ip (persistent grid): work item w = row block w - blk[t] of tile t, found by bisection;
//      the block's 256 row numbers go from list_rows to LDS, ScanL2 stages those rows panel by panel and runs its tree against
//      the tile's qT -- the bits of k_scan_l2 by construction --, and each thread stores its row's scores to
//      scores[query][offset + row in list] for the tile's real queries.
//   4. k_lists_pad: -inf over [len_q, S) of every query's row of the score buffer (all of a failed query's).
//   5. k_scan_slab_topk (nann_scan.h) over scores f32[chunk][S]: position order is concatenation order.
//   6. k_lists_finish (one workgroup per query): the merge of the slabs' lists (k_scan_merge's wg_topk call, to positions: the
//      merge kernel itself maps its rows through item_ids, and a position is no row), then position -> (slot, row in list) by
//      bisection over the query's slot offsets, item ids, zeros behind n_out = min(k, len_q).
//
// The partition (nann_partition_create) is built on the device from list_of_row: the rows are cut into groups, a count per
// (group, list), a running sum over the groups of a list, a prefix over the lists, and a fill in which one wavefront walks a
// group's rows in order -- ballots find a row's peers of the same list among the 64, the first of them advances the group's
// cursor of that list.  Integer counts commute and a cursor has one writer: the layout does not depend on timing, every list
// comes out in ascending row order.
//
// ---- the int8 form (nann_search_lists_sq8): the same plan over the code table of the index (nann_sq8.h), an
// approximate fetch of the `fetch` best positions of a query's concatenation and their exact re-rank.  Per chunk:
//   1. k_lists_plan, unchanged; the chunk's queries through the table's encoder (launch_sq8_encode).  No qT.
//   2. k_lists_scan_sq8 (persistent grid, the same work items): v_mfma_i32_16x16x64_i8 with the tile's 16 QUERIES as A and 16
//      gathered code ROWS as B.  Operand element j of lane (r = lane & 15, h = lane >> 4) in k-step s is byte 64 s + 16 h + j of
//      query / row r -- the same bytes on both sides, all an integer dot product needs.  The tile's query fragments are loaded
//      once per item and stay in registers (d / 16 VGPRs); a code row is never staged: four lanes cover 64 contiguous bytes of
//      it with one 16-byte load each.  Each wavefront takes 64 rows of the block as 4 groups of 16.  The C/D layout puts the row
//      on the lane (col = lane & 15) and the query in the register (4 (lane >> 4) + reg): one store of one query covers 16
//      consecutive positions.  The epilogue is k_scan_sq8's: sq8_score (nann_sq8.h), the same bits.
//   3. k_lists_pad, k_scan_slab_topk at width fetch.
//   4. k_lists_fetch_sq8 (one workgroup per query): the merge of the slabs' lists at min(fetch, len_q) -- the fetch lists, to
//      the caller's arrays --, the fetched positions in ascending order (sq8_sort_i32, the sort of k_sq8_sort_rows) and their
//      rows, as candidate lists of `fetch` entries a query (behind the fetched ones: row 0, never selected).
//   5. the candidate-list search's plan and scorer over those lists (launch_cand_scores, nann_cand.h): nann_score's bits.
//   6. k_lists_finish_sq8 (one workgroup per query): wg_topk over the min(fetch, len_q) exact scores -- list position order is
//      concatenation order, so ties fall to the lower position --, then the outputs as k_lists_finish writes them.
#pragma once
#include <cstddef>

#include "nann_scan.h"
#include "nann_search.h"
#include "nann_sq8.h"

namespace nann {

constexpr int kListsMaxProbe = 64;       // NANN_LISTS_MAX_PROBE
constexpr int kListsMaxChunk = 128;      // most queries per chunk (kScanMaxChunk)
constexpr int kListsPairBits = 13;       // a chunk holds at most 128 x 64 = 2^13 (query, slot) pairs
constexpr int kListsPlanNT = 1024;       // threads of k_lists_plan
constexpr int kListsGroupsMax = 1024;    // most row groups of a partition build
static_assert(kListsMaxChunk * kListsMaxProbe == 1 << kListsPairBits, "a pair number fits the key");

struct ListsTile {  // one tile of the plan: up to 16 queries that probe the same list
  long long begin;  // the list: list_rows[begin, +len)
  int32_t len, nq;  // nq: the tile's real queries
  int32_t q[16];    // the query within the chunk (behind nq: the last one again)
  int32_t off[16];  // where the list starts in that query's concatenation
};
struct ListsQuery {  // one query of the chunk
  int32_t len, status;  // len_q (0 for a failed query); 0 or NANN_ERR_INDEX_OUT_OF_RANGE
};
struct ListsHead {
  long long n_work;  // row blocks over all tiles
  int32_t n_tiles, pad;
};

struct ListsArgs {
  const void* emb;
  const int64_t* item_ids;
  long long n_items;
  int d, dt, kind;
  int cus;
  const int64_t* list_splits;  // the partition
  const int32_t* list_rows;
  int n_lists;
  long long max_len;
  const int32_t* probes;       // i32[n_queries, n_probe]
  int n_probe;
};
// workspace of a call: [scores f32[chunk, S] | cand scores | cand rows | pos i32[chunk, k] | head | queries | blk i64[T + 1] |
// tiles[T] | qT f32[T, d, 16]], T = chunk x n_probe tiles at most
struct ListsLayout {
  int chunk, n_slabs, max_tiles;
  long long S;
  size_t off_scores, off_cand_scores, off_cand_rows, off_pos, off_head, off_queries, off_blk, off_tiles, off_qt, total;
};
inline size_t lists_up256(size_t v) { return (v + 255) & ~(size_t)255; }
ListsLayout lists_layout(long long max_len, int d, long long n_queries, int n_probe, int k);
int launch_lists(const ListsArgs& a, const ListsLayout& L, const float* q, long long n_queries, int k, unsigned char* ws,
                 int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* out_pos, int32_t* n_out, int32_t* status,
                 hipStream_t st);

// the int8 form.  workspace of a call: [the ListsLayout at k = fetch and without qT: scores f32[chunk, S], the slabs' lists, the
// fetch positions i32[chunk, fetch] (off_pos), the plan | what follows], every part a multiple of 256 bytes
struct ListsSq8Layout {
  ListsLayout L;
  size_t off_qcodes, off_qscales, off_qnorms;  // the chunk's encoded queries
  size_t off_fscores;                          // the fetch lists' scores f32[chunk, fetch]
  size_t off_spos, off_rows, off_splits;       // positions ascending and their rows i32[chunk, fetch], row_splits i64[chunk + 1]
  size_t off_sel;                              // the finish's selection i32[chunk, k]: places in a query's sorted list
  size_t off_cand;                             // the candidate-list search's workspace (CandLayout) for chunk * fetch positions
  size_t total;
};
ListsSq8Layout lists_sq8_layout(long long max_len, int d, int kind, long long n_queries, int n_probe, int fetch, int k);
// t: the code table of the index a names.  out_fetch_pos / out_fetch_scores [n_queries, fetch]: may be null.
int launch_lists_sq8(const ListsArgs& a, const Sq8Args& t, const ListsSq8Layout& X, const float* q, long long n_queries, int fetch,
                     int k, unsigned char* ws, int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* out_pos,
                     int32_t* n_out, int32_t* status, int32_t* out_fetch_pos, float* out_fetch_scores, hipStream_t st);

// the partition build.  info i64[4] (device): n_listed_rows, max_len, rows with a value >= n_lists, unused
size_t lists_build_groups(long long n_items, int n_lists);
int launch_lists_count(const int32_t* list_of_row, long long n_items, int n_lists, int groups, int32_t* counts, long long* info, hipStream_t st);
int launch_lists_splits(int n_lists, int groups, int32_t* counts, int64_t* list_splits, long long* info, hipStream_t st);
int launch_lists_fill(const int32_t* list_of_row, long long n_items, int n_lists, int groups, int32_t* counts,
                      const int64_t* list_splits, int32_t* list_rows, hipStream_t st);

}  // namespace nann

#ifdef NANN_LISTS_IMPL  // the kernels: nann_lists_inst.hip only (nann_flat.hip takes the declarations above)
namespace nann {

// inclusive scan of v over the workgroup's threads (MAX: running maximum, else running sum); *total = over all of them.
// wsum: LDS, one entry per wavefront.
template <bool MAX, int NT>
__device__ __forceinline__ long long lists_wg_scan(long long v, long long* wsum, long long* total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long t = __shfl_up(v, o);
    if (lane >= o) v = MAX ? max(v, t) : v + t;
  }
  __syncthreads();  // (the scan before this one has read wsum)
  if (lane == 63) wsum[wave] = v;
  __syncthreads();
  long long all = wsum[0];
  for (int w = 1; w < NT / 64; ++w) {
    if (w == wave) v = MAX ? max(v, all) : v + all;
    all = MAX ? max(all, wsum[w]) : all + wsum[w];
  }
  *total = all;
  return v;
}

// ---- the partition build ----------------------------------------------------------------------------------------------------
// group g holds rows [g * per, (g + 1) * per), per a multiple of 64; one wavefront per group
__host__ __device__ inline long long lists_group_rows(long long n_items, int groups) {
  return ((n_items + groups - 1) / groups + 63) / 64 * 64;
}

// counts[g][l] = rows of group g in list l (integer atomics: the sums do not depend on their order)
__global__ __launch_bounds__(64) void k_lists_count(const int32_t* __restrict__ list_of_row, long long n_items, int n_lists,
                                                    int groups, int32_t* __restrict__ counts, long long* __restrict__ info) {
  const long long per = lists_group_rows(n_items, groups);
  const long long r0 = (long long)blockIdx.x * per, r1 = min(r0 + per, n_items);
  int bad = 0;
  for (long long r = r0 + threadIdx.x; r < r1; r += 64) {
    const int32_t l = list_of_row[r];
    if (l >= n_lists) ++bad;
    else if (l >= 0) atomicAdd(&counts[(size_t)blockIdx.x * n_lists + l], 1);
  }
  if (bad) atomicAdd(reinterpret_cast<unsigned long long*>(&info[2]), (unsigned long long)bad);
}

// one thread per list: counts[g][l] becomes the rows of list l in the groups before g; len[l] (in the place of splits[l + 1])
__global__ __launch_bounds__(256) void k_lists_group_prefix(int n_lists, int groups, int32_t* __restrict__ counts,
                                                           int64_t* __restrict__ list_splits) {
  const long long l = (long long)blockIdx.x * 256 + threadIdx.x;
  if (l >= n_lists) return;
  int32_t run = 0;
  for (int g = 0; g < groups; ++g) {
    const int32_t c = counts[(size_t)g * n_lists + l];
    counts[(size_t)g * n_lists + l] = run;
    run += c;
  }
  list_splits[l + 1] = run;
}

// one workgroup: list_splits[l + 1] from the lengths stored there, in place; the listed rows and the longest list
__global__ __launch_bounds__(256) void k_lists_splits(int n_lists, int64_t* __restrict__ list_splits, long long* __restrict__ info) {
  __shared__ long long wsum[4];
  long long before = 0, longest = 0;
  for (long long t0 = 0; t0 < n_lists; t0 += 256) {
    const long long l = t0 + threadIdx.x;
    const long long len = l < n_lists ? list_splits[l + 1] : 0;
    long long total, tile_max;
    const long long upto = before + lists_wg_scan<false, 256>(len, wsum, &total);
    (void)lists_wg_scan<true, 256>(len, wsum, &tile_max);
    if (l < n_lists) list_splits[l + 1] = upto;
    before += total;
    longest = max(longest, tile_max);
  }
  if (threadIdx.x == 0) {
    list_splits[0] = 0;
    info[0] = before;
    info[1] = longest;
  }
}

// one wavefront per group, its rows in order, 64 at a time: a row's peers are the rows of the 64 in the same list (one ballot per
// bit of the list number); the first peer advances the group's cursor of that list -- counts[g][l], which k_lists_group_prefix
// left at the list's rows in earlier groups -- and hands the old value to the others.  The cursor row belongs to this wavefront
// alone.
__global__ __launch_bounds__(64) void k_lists_fill(const int32_t* __restrict__ list_of_row, long long n_items, int n_lists,
                                                   int groups, int32_t* __restrict__ counts, const int64_t* __restrict__ list_splits,
                                                   int32_t* __restrict__ list_rows) {
  const long long per = lists_group_rows(n_items, groups);
  const long long r0 = (long long)blockIdx.x * per, r1 = min(r0 + per, n_items);
  const int lane = threadIdx.x;
  const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  int32_t* cursor = counts + (size_t)blockIdx.x * n_lists;
  for (long long b = r0; b < r1; b += 64) {
    const long long r = b + lane;
    const int32_t l = r < r1 ? list_of_row[r] : -1;
    const bool listed = l >= 0 && l < n_lists;
    unsigned long long peers = __ballot(listed);
#pragma unroll 1
    for (int bit = 0; bit < 31; ++bit) {
      const unsigned long long m = __ballot((l >> bit) & 1);
      peers &= ((l >> bit) & 1) ? m : ~m;
    }
    int32_t base = 0;
    if (listed && (peers & lt) == 0) base = atomicAdd(&cursor[l], __popcll(peers));
    base = __shfl(base, listed ? __ffsll((long long)peers) - 1 : lane);
    if (listed) list_rows[list_splits[l] + base + __popcll(peers & lt)] = (int32_t)r;
  }
}

// ---- the plan of a chunk ------------------------------------------------------------------------------------------------------
struct ListsPlanArgs {
  const int32_t* probes;  // the chunk's: i32[n_q, n_probe]
  int n_q, n_probe, n_lists;
  int n_sort;             // the power of two at or above n_q * n_probe
  const int64_t* list_splits;
  ListsHead* head;
  ListsQuery* queries;
  long long* blk;
  ListsTile* tiles;
};
// dynamic LDS of k_lists_plan: keys u64[n_sort] | pair offsets i32[n_sort] | pair lengths i32[n_sort]
inline size_t lists_plan_lds(int n_sort) { return (size_t)n_sort * 16; }

constexpr unsigned long long kListsNoPair = ~0ull;

__global__ __launch_bounds__(kListsPlanNT) void k_lists_plan(ListsPlanArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ long long wsum[kListsPlanNT / 64];
  __shared__ long long carry[kListsPlanNT];
  __shared__ int bad[kListsMaxChunk];
  constexpr int NT = kListsPlanNT;
  unsigned long long* key = reinterpret_cast<unsigned long long*>(smem);
  int32_t* poff = reinterpret_cast<int32_t*>(smem + (size_t)a.n_sort * 8);
  int32_t* plen = poff + a.n_sort;
  const int tid = threadIdx.x, n_pairs = a.n_q * a.n_probe;

  // 1. the slots: a pair's list length (0 for an unused slot), a query's bad flag
  if (tid < kListsMaxChunk) bad[tid] = 0;
  __syncthreads();
  for (int i = tid; i < a.n_sort; i += NT) {
    int32_t len = 0;
    if (i < n_pairs) {
      const int32_t l = a.probes[i];
      if (l >= a.n_lists) atomicOr(&bad[i / a.n_probe], 1);
      else if (l >= 0) len = (int32_t)(a.list_splits[l + 1] - a.list_splits[l]);
    }
    plen[i] = len;
  }
  __syncthreads();
  // 2. a pair's offset in its query's concatenation: the prefix of the lengths in slot order; its end is len_q
  if (tid < a.n_q) {
    int32_t at = 0;
    for (int s = 0; s < a.n_probe; ++s) {
      poff[tid * a.n_probe + s] = at;
      at += plen[tid * a.n_probe + s];
    }
    a.queries[tid] = ListsQuery{bad[tid] ? 0 : at, bad[tid] ? NANN_ERR_INDEX_OUT_OF_RANGE : 0};
  }
  // 3. the pairs with rows to score, sorted by list; within a list by pair number = (query, slot)
  for (int i = tid; i < a.n_sort; i += NT) {
    const bool work = i < n_pairs && plen[i] > 0 && !bad[i / a.n_probe];
    key[i] = work ? ((unsigned long long)(uint32_t)a.probes[i] << kListsPairBits) | (unsigned)i : kListsNoPair;
  }
  __syncthreads();
  for (int k = 2; k <= a.n_sort; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < a.n_sort; i += NT) {
        const int o = i ^ j;
        if (o > i) {
          const unsigned long long x = key[i], y = key[o];
          if ((x > y) == ((i & k) == 0)) {
            key[i] = y;
            key[o] = x;
          }
        }
      }
      __syncthreads();
    }
  }
  // 4. tiles.  A thread owns E consecutive places of the sorted order.  A run = the pairs of one list; place i is the r-th of
  //    its run, r = i - (the run's first place); a tile starts where r % 16 == 0.
  const int E = a.n_sort >= NT ? a.n_sort / NT : 1;
  const int i0 = tid * E, i1 = i0 < a.n_sort ? i0 + E : i0;
  auto list_at = [&](int i) { return (long long)(key[i] >> kListsPairBits); };
  auto is_head = [&](int i) { return key[i] != kListsNoPair && (i == 0 || list_at(i - 1) != list_at(i)); };
  long long last_head = -1, unused;
  for (int i = i0; i < i1; ++i)
    if (is_head(i)) last_head = i;
  carry[tid] = lists_wg_scan<true, NT>(last_head, wsum, &unused);
  __syncthreads();
  const long long start_in = tid > 0 ? carry[tid - 1] : -1;  // the first place of the run that reaches into this thread's places
  long long n_t = 0, n_b = 0;  // tiles that start in this thread's places, and their row blocks
  {
    long long start = start_in;
    for (int i = i0; i < i1; ++i) {
      if (key[i] == kListsNoPair) break;
      if (is_head(i)) start = i;
      if (((i - start) & 15) == 0) {
        ++n_t;
        n_b += ((long long)plen[key[i] & ((1u << kListsPairBits) - 1)] + kScanRows - 1) / kScanRows;
      }
    }
  }
  long long tiles_all, blocks_all;
  long long t_at = lists_wg_scan<false, NT>(n_t, wsum, &tiles_all) - n_t;  // tiles before this thread's
  long long b_at = lists_wg_scan<false, NT>(n_b, wsum, &blocks_all) - n_b;
  {
    long long start = start_in;
    for (int i = i0; i < i1; ++i) {
      if (key[i] == kListsNoPair) break;
      const int pair = (int)(key[i] & ((1u << kListsPairBits) - 1));
      if (is_head(i)) start = i;
      const int r = (int)(i - start) & 15;
      if (r == 0) {
        const long long l = list_at(i);
        ListsTile* t = a.tiles + t_at;
        t->begin = a.list_splits[l];
        t->len = plen[pair];
        a.blk[t_at] = b_at;
        b_at += ((long long)plen[pair] + kScanRows - 1) / kScanRows;
        ++t_at;
      }
      ListsTile* t = a.tiles + (t_at - 1);
      t->q[r] = pair / a.n_probe;
      t->off[r] = poff[pair];
      const bool last = r == 15 || i + 1 >= a.n_sort || key[i + 1] == kListsNoPair || list_at(i + 1) != list_at(i);
      if (last) {
        t->nq = r + 1;
        for (int j = r + 1; j < 16; ++j) {
          t->q[j] = pair / a.n_probe;
          t->off[j] = 0;
        }
      }
    }
  }
  if (tid == 0) {
    a.blk[tiles_all] = blocks_all;
    *a.head = ListsHead{blocks_all, (int32_t)tiles_all, 0};
  }
}

// qT[tile][e][i] = q[tiles[tile].q[i]][e]: k_scan_transpose_q's layout per tile.  A persistent grid over the tiles.
__global__ __launch_bounds__(256) void k_lists_tile_q(const ListsHead* __restrict__ head, const ListsTile* __restrict__ tiles,
                                                      const float* __restrict__ q, int d, float* __restrict__ qT) {
  const int n_tiles = head->n_tiles;
  for (int t = blockIdx.x; t < n_tiles; t += gridDim.x)
    for (int i = threadIdx.x; i < d * 16; i += 256) qT[(size_t)t * d * 16 + i] = q[(size_t)tiles[t].q[i & 15] * d + (i >> 4)];
}

// the block's rows of the table: row numbers staged in LDS by the work item (behind the list's end: its last row again)
struct ListsRowsGathered {
  const int32_t* ids;
  __device__ __forceinline__ long long at(int r, long long, long long) const { return ids[r]; }
};

// Every pointer is a __restrict__ kernel argument of its own, as k_scan_l2's are: the tile's queries and destinations go through
// the scalar cache only where the compiler can see that the kernel's stores do not reach them (behind a struct of pointers
// they were vector loads, 32 more registers, and every d spilled).
#define NANN_LISTS_SCAN_PARAMS                                                                                                  \
  const void *__restrict__ emb, const int32_t *__restrict__ list_rows, const ListsHead *__restrict__ head,                        \
      const long long *__restrict__ blk, const ListsTile *__restrict__ tiles, const float *__restrict__ qT,                     \
      float *__restrict__ scores, long long stride /* S */
#define NANN_LISTS_SCAN_ARGS emb, list_rows, head, blk, tiles, qT, scores, stride

template <int LPR, int DT, int METRIC>
__device__ __forceinline__ void lists_scan(unsigned char* rows, int32_t* ids, NANN_LISTS_SCAN_PARAMS) {
  constexpr int TQ = kScanTileQueries;
  typedef ScanL2<LPR, DT, TQ, METRIC, ListsRowsGathered> S;
  const long long n_work = head->n_work;
  const int n_tiles = head->n_tiles;
  for (long long w = blockIdx.x; w < n_work; w += gridDim.x) {
    int lo = 0, hi = n_tiles;  // blk[lo] <= w < blk[hi]
    while (hi - lo > 1) {
      const int mid = lo + (hi - lo) / 2;
      if (blk[mid] <= w) lo = mid; else hi = mid;
    }
    const ListsTile* __restrict__ t = tiles + lo;
    const int len = t->len, nq = t->nq;
    const int row = (int)(w - blk[lo]) * kScanRows + (int)threadIdx.x;  // this thread's row of the list
    __syncthreads();  // (every wavefront has left the item before: its row numbers and its last panel may go)
    ids[threadIdx.x] = list_rows[t->begin + min(row, len - 1)];
    __syncthreads();
    S s;
    s.table = static_cast<const unsigned char*>(emb);
    s.n_items = 0;
    s.row0 = 0;
    s.qt = reinterpret_cast<const f32x2*>(qT + (size_t)lo * S::D * TQ);
    s.lds = rows;
    s.rows.ids = ids;
    f32x2 sum[S::NP], qn[S::NP];
    s.load_q(0, qn);
    s.template tree<LPR, 0>(sum, qn);
    if (row >= len) continue;
#pragma unroll
    for (int p = 0; p < S::NP; ++p) {
      if (2 * p < nq) scores[(size_t)t->q[2 * p] * stride + t->off[2 * p] + row] = METRIC == MT_IP ? sum[p].x : 0.0f - sum[p].x;
      if (2 * p + 1 < nq) scores[(size_t)t->q[2 * p + 1] * stride + t->off[2 * p + 1] + row] = METRIC == MT_IP ? sum[p].y : 0.0f - sum[p].y;
    }
  }
}

template <int LPR, int DT>
__global__ __launch_bounds__(kScanRows) __attribute__((amdgpu_waves_per_eu(scan_waves(LPR), scan_waves(LPR)))) void k_lists_scan_l2(NANN_LISTS_SCAN_PARAMS) {
  __shared__ __attribute__((aligned(16))) unsigned char rows[kScanRows * kScanRowStride];
  __shared__ int32_t ids[kScanRows];
  lists_scan<LPR, DT, MT_L2>(rows, ids, NANN_LISTS_SCAN_ARGS);
}

template <int LPR, int DT>
__global__ __launch_bounds__(kScanRows) __attribute__((amdgpu_waves_per_eu(scan_waves(LPR), scan_waves(LPR)))) void k_lists_scan_ip(NANN_LISTS_SCAN_PARAMS) {
  __shared__ __attribute__((aligned(16))) unsigned char rows[kScanRows * kScanRowStride];
  __shared__ int32_t ids[kScanRows];
  lists_scan<LPR, DT, MT_IP>(rows, ids, NANN_LISTS_SCAN_ARGS);
}

// -inf behind every query's concatenation: grid (blocks of 1024 positions, queries)
__global__ __launch_bounds__(256) void k_lists_pad(const ListsQuery* __restrict__ queries, long long S, float* __restrict__ scores) {
  const long long from = queries[blockIdx.y].len;
  for (long long i = from + (long long)blockIdx.x * 256 + threadIdx.x; i < S; i += (long long)gridDim.x * 256)
    scores[(size_t)blockIdx.y * S + i] = -__builtin_inff();
}

struct ListsFinishArgs {
  const float* cand_scores;   // [n_q][n_in]: the slabs' lists, end to end
  const int32_t* cand_rows;   // positions in the concatenation
  int n_in, k;
  const ListsQuery* queries;
  const int32_t* probes;      // the chunk's
  int n_probe, n_lists;
  const int64_t* list_splits;
  const int32_t* list_rows;
  const int64_t* item_ids;
  int32_t* pos;               // workspace i32[n_q, k]
  int64_t* out_item_ids;      // the chunk's rows of the outputs
  float* out_scores;
  int32_t* out_index;
  int32_t* out_pos;
  int32_t* n_out;
  int32_t* status;
};

// The slots' offsets of query qi again, by the first wavefront: an exclusive prefix of the lengths over the lanes.  sbegin, soff:
// LDS, kListsMaxProbe entries each; a barrier publishes them.
__device__ __forceinline__ void lists_slot_offsets(const int32_t* __restrict__ probes, size_t qi, int n_probe, int n_lists,
                                                   const int64_t* __restrict__ list_splits, long long* sbegin, int32_t* soff) {
  const int tid = threadIdx.x;
  if (tid < 64) {
    const int32_t l = tid < n_probe ? probes[qi * n_probe + tid] : -1;
    const bool named = l >= 0 && l < n_lists;
    const long long b = named ? list_splits[l] : 0;
    int32_t len = named ? (int32_t)(list_splits[l + 1] - b) : 0, at = len;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int32_t t = __shfl_up(at, o);
      if (tid >= o) at += t;
    }
    sbegin[tid] = b;
    soff[tid] = at - len;
  }
}

// position of a query's concatenation -> row of the table
__device__ __forceinline__ int32_t lists_row_at(int32_t pos, int32_t len_q, int n_probe, const long long* sbegin, const int32_t* soff,
                                                const int32_t* __restrict__ list_rows) {
  int lo = 0, hi = n_probe;  // soff[lo] <= pos < soff[hi]: the last slot that starts at or before pos holds it
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (soff[mid] <= pos) lo = mid; else hi = mid;
  }
  // (pos < len_q unless a NaN score outranked the padding -- outside the contract, as for nann_topk, but never out of bounds)
  return pos < len_q ? list_rows[sbegin[lo] + (pos - soff[lo])] : 0;
}

__global__ __launch_bounds__(kNT) void k_lists_finish(ListsFinishArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char scratch[sizeof(TopkScratch)];
  __shared__ long long sbegin[kListsMaxProbe];
  __shared__ int32_t soff[kListsMaxProbe];
  const size_t qi = blockIdx.x;
  const int tid = threadIdx.x;
  const ListsQuery Q = a.queries[qi];
  const int kk = Q.status != 0 ? 0 : min(a.k, Q.len);
  lists_slot_offsets(a.probes, qi, a.n_probe, a.n_lists, a.list_splits, sbegin, soff);
  __syncthreads();
  if (kk > 0) {
    wg_topk(a.cand_rows + qi * a.n_in, a.cand_scores + qi * a.n_in, nullptr, a.n_in, kk, nullptr, a.pos + qi * a.k,
            a.out_scores ? a.out_scores + qi * a.k : nullptr, nullptr, nullptr, scratch);
    __syncthreads();
  }
  for (int i = tid; i < a.k; i += kNT) {
    const size_t at = qi * (size_t)a.k + i;
    int32_t pos = 0, row = 0;
    int64_t id = 0;
    if (i < kk) {
      pos = a.pos[at];
      row = lists_row_at(pos, Q.len, a.n_probe, sbegin, soff, a.list_rows);
      id = a.item_ids[row];
    } else if (a.out_scores) {
      a.out_scores[at] = 0.0f;
    }
    a.out_item_ids[at] = id;
    if (a.out_index) a.out_index[at] = row;
    if (a.out_pos) a.out_pos[at] = pos;
  }
  if (tid == 0) {
    if (a.n_out) a.n_out[qi] = kk;
    a.status[qi] = Q.status;
  }
}

// ---- the int8 form ------------------------------------------------------------------------------------------------------------
// Work item w as in lists_scan.  LDS: the block's 256 row numbers (behind the list's end: its last row again; a number outside the
// table becomes row 0) and, per query of the tile, its scale term, its norm term (sq8_scan_front's qs and qa) and where its
// run of the score buffer starts.  Wavefront v takes rows [64 v, +64) of the block as 4 groups of 16; per k-step the four
// groups' 16-byte loads are issued, then the four MFMAs.  No row of the table passes through LDS.
template <int NS, int METRIC>  // NS = d / 64 k-steps
__global__ __launch_bounds__(kScanRows) void k_lists_scan_sq8(const int8_t* __restrict__ codes, const float* __restrict__ scales,
                                                              const int32_t* __restrict__ norms, long long n_items,
                                                              const int32_t* __restrict__ list_rows, const ListsHead* __restrict__ head,
                                                              const long long* __restrict__ blk, const ListsTile* __restrict__ tiles,
                                                              const int8_t* __restrict__ qcodes, const float* __restrict__ qscales,
                                                              const int32_t* __restrict__ qnorms, float* __restrict__ scores,
                                                              long long stride /* S */) {
  constexpr int D = NS * 64, TQ = kScanTileQueries, G = 4;  // G groups of 16 rows per wavefront
  static_assert(TQ == 16 && kScanRows == 4 * 16 * G, "a tile is the A operand; four wavefronts of 64 rows");
  __shared__ int32_t ids[kScanRows];
  __shared__ float qs[TQ], qa[TQ];
  __shared__ long long dst[TQ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, h = lane >> 4;
  const long long n_work = head->n_work;
  const int n_tiles = head->n_tiles;
  for (long long w = blockIdx.x; w < n_work; w += gridDim.x) {
    int lo = 0, hi = n_tiles;  // blk[lo] <= w < blk[hi]
    while (hi - lo > 1) {
      const int mid = lo + (hi - lo) / 2;
      if (blk[mid] <= w) lo = mid; else hi = mid;
    }
    const ListsTile* __restrict__ t = tiles + lo;
    const int len = t->len, nq = t->nq;
    const int row0 = (int)(w - blk[lo]) * kScanRows;  // the block's first row of the list
    __syncthreads();  // (every wavefront has left the item before: its row numbers and query terms may go)
    {
      const int32_t id = list_rows[t->begin + min(row0 + tid, len - 1)];
      ids[tid] = id >= 0 && id < n_items ? id : 0;
    }
    if (tid < TQ) {
      const int qi = t->q[tid];
      const float sq = qscales[qi];
      qs[tid] = METRIC == MT_IP ? sq : __fmul_rn(2.0f, sq);
      qa[tid] = __fmul_rn(__fmul_rn(sq, sq), (float)qnorms[qi]);
      dst[tid] = (long long)qi * stride + t->off[tid];
    }
    __syncthreads();
    const int wrow0 = row0 + wave * (16 * G);
    if (wrow0 >= len) continue;  // (uniform over the wavefront; the barriers stand at the head of an item)
    // A: query r of the tile, bytes [64 s + 16 h, +16) of k-step s -- once per item, in registers to its end
    i32x4v a[NS];
    {
      const int8_t* qrow = qcodes + (size_t)t->q[r] * D + h * 16;
#pragma unroll
      for (int s = 0; s < NS; ++s) a[s] = *reinterpret_cast<const i32x4v*>(qrow + s * 64);
    }
    // B: row r of group g, the same bytes
    const int8_t* xrow[G];
#pragma unroll
    for (int g = 0; g < G; ++g) xrow[g] = codes + (size_t)ids[wave * (16 * G) + 16 * g + r] * D + h * 16;
    i32x4v acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = i32x4v{0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      i32x4v b[G];
#pragma unroll
      for (int g = 0; g < G; ++g) b[g] = *reinterpret_cast<const i32x4v*>(xrow[g] + s * 64);
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[s], b[g], acc[g], 0, 0, 0);
    }
    // C/D: register i of lane (r, h) is query 4 h + i against row r of the group
    float my_qs[4], my_qa[4];
    long long my_dst[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      my_qs[i] = qs[4 * h + i];
      my_qa[i] = qa[4 * h + i];
      my_dst[i] = dst[4 * h + i];
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int row = wrow0 + 16 * g + r;  // this lane's row of the list
      if (row >= len) continue;
      const int32_t id = ids[wave * (16 * G) + 16 * g + r];
      const float sx = scales[id];
      const float bx = __fmul_rn(__fmul_rn(sx, sx), (float)norms[id]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (4 * h + i < nq) scores[my_dst[i] + row] = sq8_score<METRIC>(my_qs[i], my_qa[i], sx, bx, acc[g][i]);
    }
  }
}

struct ListsFetchSq8Args {
  const float* cand_scores;   // [n_q][n_in]: the slabs' lists at width fetch, end to end
  const int32_t* cand_rows;   // positions in the concatenation
  int n_in, fetch;
  const ListsQuery* queries;
  const int32_t* probes;      // the chunk's
  int n_probe, n_lists;
  const int64_t* list_splits;
  const int32_t* list_rows;
  long long n_items;
  int32_t* fpos;              // workspace [n_q, fetch]: the fetch lists, TopKV2 order
  float* fscores;
  int32_t* spos;              // workspace [n_q, fetch]: the fetched positions ascending (behind them: 0),
  int32_t* rows;              // and their rows (behind them: row 0): the candidate lists,
  long long* splits;          // and their row_splits i64[n_q + 1]
  int32_t* out_fetch_pos;     // the chunk's rows of the caller's arrays, or null
  float* out_fetch_scores;
};

__global__ __launch_bounds__(kNT) void k_lists_fetch_sq8(ListsFetchSq8Args a) {
  __shared__ __attribute__((aligned(16))) unsigned char scratch[sizeof(TopkScratch)];
  __shared__ long long sbegin[kListsMaxProbe];
  __shared__ int32_t soff[kListsMaxProbe];
  __shared__ int32_t v[kMaxK];
  const size_t qi = blockIdx.x, base = qi * (size_t)a.fetch;
  const int tid = threadIdx.x;
  const ListsQuery Q = a.queries[qi];
  const int ff = Q.status != 0 ? 0 : min(a.fetch, Q.len);
  lists_slot_offsets(a.probes, qi, a.n_probe, a.n_lists, a.list_splits, sbegin, soff);
  __syncthreads();
  if (ff > 0) {
    wg_topk(a.cand_rows + qi * a.n_in, a.cand_scores + qi * a.n_in, nullptr, a.n_in, ff, nullptr, a.fpos + base, a.fscores + base,
            nullptr, nullptr, scratch);
    __syncthreads();
  }
  int n2 = 1;
  while (n2 < a.fetch) n2 <<= 1;
  for (int i = tid; i < n2; i += kNT) {
    const int32_t pos = i < ff ? a.fpos[base + i] : 0x7fffffff;
    v[i] = pos;
    if (i < a.fetch) {
      if (a.out_fetch_pos) a.out_fetch_pos[base + i] = i < ff ? pos : 0;
      if (a.out_fetch_scores) a.out_fetch_scores[base + i] = i < ff ? a.fscores[base + i] : -__builtin_inff();
    }
  }
  sq8_sort_i32<kNT>(v, n2);
  for (int i = tid; i < a.fetch; i += kNT) {
    int32_t pos = 0, row = 0;
    if (i < ff) {
      pos = v[i];
      row = lists_row_at(pos, Q.len, a.n_probe, sbegin, soff, a.list_rows);
      if (row < 0 || row >= a.n_items) row = 0;
    }
    a.spos[base + i] = pos;
    a.rows[base + i] = row;
  }
  if (tid == 0) {  // (neighbours write the same value to the split they share)
    a.splits[qi] = (long long)base;
    a.splits[qi + 1] = (long long)(base + a.fetch);
  }
}

struct ListsFinishSq8Args {
  const float* exact;         // the candidate-list scorer's buffer: query qi's list at [qi * fetch, +fetch), position order
  const int32_t* spos;        // [n_q, fetch]
  const int32_t* rows;
  int fetch, k;
  const ListsQuery* queries;
  const int64_t* item_ids;
  int32_t* sel;               // workspace i32[n_q, k]
  int64_t* out_item_ids;      // the chunk's rows of the outputs
  float* out_scores;
  int32_t* out_index;
  int32_t* out_pos;
  int32_t* n_out;
  int32_t* status;
};

__global__ __launch_bounds__(kNT) void k_lists_finish_sq8(ListsFinishSq8Args a) {
  __shared__ __attribute__((aligned(16))) unsigned char scratch[sizeof(TopkScratch)];
  const size_t qi = blockIdx.x, base = qi * (size_t)a.fetch;
  const int tid = threadIdx.x;
  const ListsQuery Q = a.queries[qi];
  const int ff = Q.status != 0 ? 0 : min(a.fetch, Q.len), kk = min(a.k, ff);
  if (kk > 0) {  // (a place in the sorted list is a rank among the fetched positions: ties -> the lower position)
    wg_topk(nullptr, a.exact + base, nullptr, ff, kk, a.sel + qi * a.k, nullptr, a.out_scores ? a.out_scores + qi * a.k : nullptr,
            nullptr, nullptr, scratch);
    __syncthreads();
  }
  for (int i = tid; i < a.k; i += kNT) {
    const size_t at = qi * (size_t)a.k + i;
    int32_t pos = 0, row = 0;
    int64_t id = 0;
    if (i < kk) {
      const int32_t j = a.sel[at];
      pos = a.spos[base + j];
      row = a.rows[base + j];
      id = a.item_ids[row];
    } else if (a.out_scores) {
      a.out_scores[at] = 0.0f;
    }
    a.out_item_ids[at] = id;
    if (a.out_index) a.out_index[at] = row;
    if (a.out_pos) a.out_pos[at] = pos;
  }
  if (tid == 0) {
    if (a.n_out) a.n_out[qi] = kk;
    a.status[qi] = Q.status;
  }
}

}  // namespace nann
#endif
