// nann_ops.hip -- the drop-in ops of the reference's graph, kernels and entry points: HugeConst (nann_huge_const_load),
// GroupGather (count / fill, and unique = true), BitmapRefDifference, BloomFilterDifference, GatherV2 (nann_gather_rows) and
// TopKV2 (nann_topk).  A source of nann_core.o; what it shares with the other host sources is in nann_host.h.
// The ABI is documented in include/nann_hip.h; the workgroup building blocks in nann_device.h.  Reference citations are
// relative to /root/reference/.
#include "nann_host.h"
#include "host/nann_npy.h"

#include <algorithm>
#include <cmath>
#include <fstream>
#include <string>
#include <vector>

using namespace nann;

// ===========================================================================
// kernels: per-op drop-ins
// ===========================================================================

// ragged validation (GroupGather_kernel.cc:9-16, bitmap_ops.cc:12-19)
__device__ __forceinline__ int validate_ragged(long long n_values, const int64_t* rs, long long n_splits) {
  if (n_splits == 0) return 1;
  if (rs[0] != 0) return 2;
  if (rs[n_splits - 1] != n_values) return 3;
  return 0;
}

// GroupGather count pass (:137-145) for all groups at once: per frontier row j
// the output offset (exclusive scan of row lengths), then ret_row_splits.
__global__ __launch_bounds__(kNT) void k_group_gather_count(
    const int64_t* params_row_splits, long long n_params_splits, long long n_params_values,
    const int64_t* indices_values, long long n_iv, const int64_t* indices_row_splits,
    long long n_irs, int64_t* ret_row_splits, int64_t* offsets, OpResult* res) {
  __shared__ long long s_wave[kNW];
  __shared__ long long s_running;
  __shared__ int s_bad;
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
  if (tid == 0) {
    res->n_out = 0; res->n_out_splits = 0; res->bad_i = -1; res->code = 0; res->err = 0;
    s_running = 0; s_bad = 0;
  }
  __syncthreads();
  int code = validate_ragged(n_params_values, params_row_splits, n_params_splits);
  if (code) {
    if (tid == 0) { res->code = code; res->err = NANN_ERR_INVALID_RAGGED_PARAMS; }
    return;
  }
  // indices ragged: its values are indices_values
  code = validate_ragged(n_iv, indices_row_splits, n_irs);
  if (code) {
    if (tid == 0) { res->code = code; res->err = NANN_ERR_INVALID_RAGGED_INDICES; }
    return;
  }
  if (n_params_splits == 1 || n_irs == 1) {  // void inputs -> ([], [0])  :69-77
    if (tid == 0) { ret_row_splits[0] = 0; res->n_out = 0; res->n_out_splits = 1; }
    return;
  }
  const long long n_rows = n_params_splits - 1;
  for (long long j0 = 0; j0 < n_iv; j0 += kNT) {
    const long long j = j0 + tid;
    long long len = 0;
    if (j < n_iv) {
      const long long idx = indices_values[j];
      if (idx < 0 || idx >= n_rows) s_bad = 1;
      else len = params_row_splits[idx + 1] - params_row_splits[idx];
    }
    long long inc = len;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long t = __shfl_up(inc, d);
      if (lane >= d) inc += t;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    long long wb = 0, tot = 0;
    for (int w = 0; w < kNW; ++w) { const long long t = s_wave[w]; if (w < wave) wb += t; tot += t; }
    const long long run = s_running;
    if (j < n_iv) offsets[j] = run + wb + inc - len;
    __syncthreads();
    if (tid == 0) s_running = run + tot;
    __syncthreads();
  }
  if (s_bad) {
    if (tid == 0) res->err = NANN_ERR_INDEX_OUT_OF_RANGE;
    return;
  }
  if (tid == 0) offsets[n_iv] = s_running;
  __syncthreads();
  for (long long i = tid; i < n_irs; i += kNT) ret_row_splits[i] = offsets[indices_row_splits[i]];
  if (tid == 0) { res->n_out = s_running; res->n_out_splits = n_irs; }
}

// GroupGather fill pass (:152-168): one wavefront per gathered row.
__global__ __launch_bounds__(256) void k_group_gather_fill(const int32_t* __restrict__ params_values,
                                                           const int64_t* __restrict__ params_row_splits,
                                                           const int64_t* __restrict__ indices_values,
                                                           long long n_iv,
                                                           const int64_t* __restrict__ offsets,
                                                           int32_t* __restrict__ ret_values) {
  const int lane = lane_id();
  const long long wave_global = (long long)blockIdx.x * (blockDim.x >> 6) + wave_id();
  const long long n_waves = (long long)gridDim.x * (blockDim.x >> 6);
  for (long long j = wave_global; j < n_iv; j += n_waves) {
    const long long g = indices_values[j];
    const long long s = params_row_splits[g], e = params_row_splits[g + 1], o = offsets[j];
    for (long long c = lane; c < e - s; c += 64) ret_values[o + c] = params_values[s + c];
  }
}

// GroupGather unique=true (GroupGather_kernel.cc:91-131): per group the SET of the gathered values.  The reference
// writes a group in its unordered_set's iteration order -- any order of the distinct values is its answer --; here:
// first-occurrence order of the unique=false list, which is the input (values / row_splits = that op's outputs).
// One open-addressing table for all groups, keyed by (group, value): a 64-bit entry is (value << 32 | position) with the
// position global, so the group of an entry is grp[position] and "the smallest position of a key" is one atomicMin
// on the entry (equal high halves).  Position p is kept iff its key's entry still says p.
constexpr unsigned long long kGguEmpty = ~0ull;
__device__ __forceinline__ uint32_t ggu_hash(uint32_t v, uint32_t g) {
  uint32_t h = v * 0x9E3779B1u ^ (g * 0x85EBCA77u);
  h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 13;
  return h;
}
__global__ __launch_bounds__(256) void k_ggu_groups(const int64_t* row_splits, long long n_groups, uint32_t* grp) {
  for (long long g = blockIdx.x; g < n_groups; g += gridDim.x)
    for (long long p = row_splits[g] + threadIdx.x; p < row_splits[g + 1]; p += blockDim.x) grp[p] = (uint32_t)g;
}
__global__ __launch_bounds__(256) void k_ggu_insert(const int32_t* values, long long n, const uint32_t* grp,
                                                    unsigned long long* table, uint32_t mask) {
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
    const uint32_t v = (uint32_t)values[p], g = grp[p];
    const unsigned long long mine = ((unsigned long long)v << 32) | (unsigned long long)(uint32_t)p;
    uint32_t h = ggu_hash(v, g) & mask;
    for (;;) {
      unsigned long long e = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (e == kGguEmpty) {
        e = atomicCAS(&table[h], kGguEmpty, mine);
        if (e == kGguEmpty) break;  // claimed
      }
      if ((uint32_t)(e >> 32) == v && grp[(uint32_t)e] == g) { atomicMin(&table[h], mine); break; }
      h = (h + 1) & mask;
    }
  }
}
__device__ __forceinline__ bool ggu_is_first(const int32_t* values, const uint32_t* grp, const unsigned long long* table,
                                             uint32_t mask, long long p) {
  const uint32_t v = (uint32_t)values[p], g = grp[p];
  uint32_t h = ggu_hash(v, g) & mask;
  for (;;) {
    const unsigned long long e = table[h];
    if ((uint32_t)(e >> 32) == v && e != kGguEmpty && grp[(uint32_t)e] == g) return (uint32_t)e == (uint32_t)p;
    h = (h + 1) & mask;
  }
}
// per group: distinct values -> counts[g]
__global__ __launch_bounds__(256) void k_ggu_count(const int32_t* values, const int64_t* row_splits, long long n_groups,
                                                   const uint32_t* grp, const unsigned long long* table, uint32_t mask,
                                                   long long* counts) {
  __shared__ unsigned int s_n;
  for (long long g = blockIdx.x; g < n_groups; g += gridDim.x) {
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    unsigned int mine = 0;
    for (long long p = row_splits[g] + threadIdx.x; p < row_splits[g + 1]; p += blockDim.x)
      mine += ggu_is_first(values, grp, table, mask, p) ? 1u : 0u;
    if (mine) atomicAdd(&s_n, mine);
    __syncthreads();
    if (threadIdx.x == 0) counts[g] = s_n;
    __syncthreads();
  }
}
__global__ __launch_bounds__(kNT) void k_ggu_scan(const long long* counts, long long n_groups, int64_t* out_row_splits,
                                                  OpResult* res) {
  __shared__ long long s_wave[kNW];
  __shared__ long long s_running;
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
  if (tid == 0) { s_running = 0; out_row_splits[0] = 0; }
  __syncthreads();
  for (long long g0 = 0; g0 < n_groups; g0 += kNT) {
    const long long g = g0 + tid;
    const long long c = g < n_groups ? counts[g] : 0;
    long long inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long t = __shfl_up(inc, d);
      if (lane >= d) inc += t;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    long long wb = 0, tot = 0;
    for (int w = 0; w < kNW; ++w) { const long long t = s_wave[w]; if (w < wave) wb += t; tot += t; }
    const long long run = s_running;
    if (g < n_groups) out_row_splits[g + 1] = run + wb + inc;
    __syncthreads();
    if (tid == 0) s_running = run + tot;
    __syncthreads();
  }
  if (tid == 0) { res->n_out = s_running; res->n_out_splits = n_groups + 1; res->bad_i = -1; res->code = 0; res->err = 0; }
}
// per group: the kept positions in position order
__global__ __launch_bounds__(256) void k_ggu_emit(const int32_t* values, const int64_t* row_splits, long long n_groups,
                                                  const uint32_t* grp, const unsigned long long* table, uint32_t mask,
                                                  const int64_t* out_row_splits, int32_t* out_values) {
  __shared__ uint32_t s_wave[4];
  __shared__ long long s_base;
  const int lane = lane_id(), wave = wave_id();
  for (long long g = blockIdx.x; g < n_groups; g += gridDim.x) {
    if (threadIdx.x == 0) s_base = out_row_splits[g];
    __syncthreads();
    const long long b = row_splits[g], e = row_splits[g + 1];
    for (long long p0 = b; p0 < e; p0 += 256) {
      const long long p = p0 + threadIdx.x;
      const bool keep = p < e && ggu_is_first(values, grp, table, mask, p);
      const unsigned long long m = __ballot(keep);
      if (lane == 0) s_wave[wave] = (uint32_t)__popcll(m);
      __syncthreads();
      uint32_t wb = 0, tot = 0;
      for (int w = 0; w < 4; ++w) { const uint32_t t = s_wave[w]; if (w < wave) wb += t; tot += t; }
      const long long base = s_base;
      if (keep) out_values[base + wb + __popcll(m & ((1ull << lane) - 1ull))] = values[p];
      __syncthreads();
      if (threadIdx.x == 0) s_base = base + tot;
      __syncthreads();
    }
  }
}

// BitmapRefDifference (bitmap_ops.cc:175-257): one workgroup; the bitmap is
// staged into LDS when it fits, walked by one wavefront, and written back.
template <bool kLds>
__global__ __launch_bounds__(kNT) void k_bitmap_ref_difference(
    const int32_t* values, long long n_values, const int64_t* row_splits, long long n_splits,
    uint32_t* flags, long long n_words, int32_t* c_values, int64_t* c_row_splits, OpResult* res) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int& s_bad = *reinterpret_cast<int*>(smem);  // first 16 bytes: flags; bitmap follows
  const int tid = threadIdx.x;
  if (tid == 0) {
    res->n_out = 0; res->n_out_splits = 0; res->bad_i = -1; res->code = 0; res->err = 0;
    s_bad = 0;
  }
  __syncthreads();
  const int code = validate_ragged(n_values, row_splits, n_splits);
  if (code) {
    if (tid == 0) { res->code = code; res->err = NANN_ERR_INVALID_RAGGED_INPUT; }
    return;
  }
  if (n_splits == 1) {  // void input :187-196; bitmap forwarded untouched
    if (tid == 0) { c_row_splits[0] = 0; res->n_out = 0; res->n_out_splits = 1; }
    return;
  }
  // bounds pre-check so that an error leaves the bitmap untouched
  const unsigned long long limit = (unsigned long long)n_words * 32ull;
  for (long long j = tid; j < n_values; j += kNT) {
    const int32_t v = values[j];
    if (v < 0 || (unsigned long long)v >= limit) s_bad = 1;
  }
  __syncthreads();
  if (s_bad) {
    if (tid == 0) res->err = NANN_ERR_INDEX_OUT_OF_RANGE;
    return;
  }
  uint32_t* bm = kLds ? reinterpret_cast<uint32_t*>(smem + 16) : flags;
  if (kLds) {
    for (long long w = tid; w < n_words; w += kNT) bm[w] = flags[w];
  }
  __syncthreads();
  if (wave_id() == 0) {
    int err = 0;
    long long base = 0;
    const long long groups = n_splits - 1;
    const uint32_t n_items = limit < 0x7fffffffull ? (uint32_t)limit : 0x7fffffffu;
    if (lane_id() == 0) c_row_splits[0] = 0;
    for (long long g = 0; g < groups; ++g) {  // ONE bitmap for all groups
      const long long s = row_splits[g], e = row_splits[g + 1];
      base = wave_walk_span<kLds>(values + s, (int)(e - s), bm, n_items, c_values, (int)base, &err);
      if (lane_id() == 0) c_row_splits[g + 1] = base;
    }
    if (lane_id() == 0) { res->n_out = base; res->n_out_splits = n_splits; }
  }
  __syncthreads();
  if (kLds) {
    for (long long w = tid; w < n_words; w += kNT) flags[w] = bm[w];
  }
}

// ---- BloomFilterDifference (bitmap_ops.cc:264-425) ------------------------------------------------
// tensorflow::Fingerprint64 = FarmHash farmhashna::Hash64, restated for the <= 11-byte decimal strings
// of int32 ids (oracle/nann_oracle.c carries the longer branches and the pinning note).
__device__ __forceinline__ uint64_t fh_rot(uint64_t v, int s) { return (v >> s) | (v << (64 - s)); }
__device__ __forceinline__ uint64_t fh_len16(uint64_t u, uint64_t v, uint64_t mul) {
  uint64_t a = (u ^ v) * mul; a ^= (a >> 47);
  uint64_t b = (v ^ a) * mul; b ^= (b >> 47);
  return b * mul;
}
__device__ __forceinline__ uint64_t fingerprint64_short(const unsigned char* s, int len) {  // len in [1, 16]
  constexpr uint64_t K0 = 0xc3a5c85c97cb3127ULL, K2 = 0x9ae16a3b2f90404fULL;
  auto fetch = [&](int at, int bytes) { uint64_t v = 0; for (int i = 0; i < bytes; ++i) v |= (uint64_t)s[at + i] << (8 * i); return v; };
  const uint64_t n = (uint64_t)len;
  if (len >= 8) {
    const uint64_t mul = K2 + n * 2, a = fetch(0, 8) + K2, b = fetch(len - 8, 8);
    return fh_len16(fh_rot(b, 37) * mul + a, (fh_rot(a, 25) + b) * mul, mul);
  }
  if (len >= 4) {
    const uint64_t mul = K2 + n * 2;
    return fh_len16(n + (fetch(0, 4) << 3), fetch(len - 4, 4), mul);
  }
  const uint32_t y = (uint32_t)s[0] + ((uint32_t)s[len >> 1] << 8), z = (uint32_t)n + ((uint32_t)s[len - 1] << 2);
  uint64_t v = (y * K2) ^ (z * K0);
  v ^= v >> 47;
  return v * K2;
}

struct BloomParams { long long bucket, bucket_size; unsigned long long prime[4]; };

__device__ __forceinline__ void bloom_positions(int32_t node, const BloomParams& B, uint32_t pos[4]) {
  unsigned char buf[12];  // std::to_string(node), bitmap_ops.cc:346
  int len = 0;
  uint32_t mag = node < 0 ? 0u - (uint32_t)node : (uint32_t)node;
  unsigned char rev[10];
  int nd = 0;
  do { rev[nd++] = (unsigned char)('0' + mag % 10u); mag /= 10u; } while (mag);
  if (node < 0) buf[len++] = '-';
  while (nd) buf[len++] = rev[--nd];
  uint64_t raw = fingerprint64_short(buf, len);
  if (B.bucket > 0) raw = raw % (uint64_t)B.bucket;
  const uint64_t mult[4] = {1, 3, 5, 7};
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    const uint64_t tmp = ((raw * mult[l]) % B.prime[l] + B.prime[l]) % B.prime[l];
    pos[l] = (uint32_t)(tmp % (uint64_t)(B.bucket_size * 32));
  }
}

// One workgroup; the filter is staged in LDS when it fits.  Positions are hashed by all lanes of
// wavefront 0, 64 nodes per step; the test-and-set of a step runs in node order on one lane (the four
// positions of a node and of its neighbours may coincide, and which node "misses" decides what is kept).
template <bool kLds>
__global__ __launch_bounds__(kNT) void k_bloom_filter_difference(
    const int32_t* values, long long n_values, const int64_t* row_splits, long long n_splits, uint32_t* flags,
    long long n_words, BloomParams B, int32_t* c_values, int64_t* c_row_splits, OpResult* res) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = lane_id();
  if (tid == 0) { res->n_out = 0; res->n_out_splits = 0; res->bad_i = -1; res->code = 0; res->err = 0; }
  __syncthreads();
  const int code = validate_ragged(n_values, row_splits, n_splits);
  if (code) {
    if (tid == 0) { res->code = code; res->err = NANN_ERR_INVALID_RAGGED_INPUT; }
    return;
  }
  if (n_splits == 1) {  // void input :315-325; filter forwarded untouched
    if (tid == 0) { c_row_splits[0] = 0; res->n_out = 0; res->n_out_splits = 1; }
    return;
  }
  uint32_t* bm = kLds ? reinterpret_cast<uint32_t*>(smem) : flags;
  if (kLds) for (long long w = tid; w < n_words; w += kNT) bm[w] = flags[w];
  __syncthreads();
  if (wave_id() == 0) {
    long long out = 0;
    if (lane == 0) c_row_splits[0] = 0;
    for (long long g = 0; g + 1 < n_splits; ++g) {
      const long long s = row_splits[g], e = row_splits[g + 1];
      for (long long j0 = s; j0 < e; j0 += 64) {
        const int cnt = (int)((e - j0) < 64 ? (e - j0) : 64);
        uint32_t pos[4] = {0, 0, 0, 0};
        int32_t node = 0;
        if (lane < cnt) { node = values[j0 + lane]; bloom_positions(node, B, pos); }
        uint64_t keepmask = 0;
        for (int i = 0; i < cnt; ++i) {  // node order
          uint32_t p[4];
#pragma unroll
          for (int l = 0; l < 4; ++l) p[l] = (uint32_t)__builtin_amdgcn_readlane((int)pos[l], i);
          int miss = 0;
          if (lane == 0) {
#pragma unroll
            for (int l = 0; l < 4; ++l) {
              const uint32_t bit = 1u << (p[l] & 31), w = bm[p[l] >> 5];
              if (!(w & bit)) { ++miss; bm[p[l] >> 5] = w | bit; }
            }
          }
          miss = __builtin_amdgcn_readfirstlane(miss);
          if (miss > 0) keepmask |= 1ull << i;
        }
        if ((keepmask >> lane) & 1ull) c_values[out + popc64(keepmask & lanemask_lt(lane))] = node;
        out += popc64(keepmask);
      }
      if (lane == 0) c_row_splits[g + 1] = out;
    }
    if (lane == 0) { res->n_out = out; res->n_out_splits = n_splits; }
  }
  __syncthreads();
  if (kLds) for (long long w = tid; w < n_words; w += kNT) flags[w] = bm[w];
}

// GatherV2 axis 0 (gather_functor.h:96-103): word-wise coalesced row copy.
template <typename W>
__global__ __launch_bounds__(256) void k_gather_rows(const W* __restrict__ params, long long n_rows,
                                                     long long row_words,
                                                     const int32_t* __restrict__ indices,
                                                     long long n_idx, W* __restrict__ out,
                                                     OpResult* res) {
  const long long total = n_idx * row_words;
  for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < total;
       w += (long long)gridDim.x * blockDim.x) {
    const long long i = w / row_words, c = w - i * row_words;
    const long long r = indices[i];
    if (r < 0 || r >= n_rows) {  // FastBoundsCheck, gather_functor.h:85-89
      atomicMin(reinterpret_cast<unsigned long long*>(&res->bad_i), (unsigned long long)i);
      continue;
    }
    out[w] = params[r * row_words + c];
  }
}

__global__ void k_init_result(OpResult* res) {
  res->n_out = 0; res->n_out_splits = 0; res->bad_i = 0x7fffffffffffffffll; res->code = 0; res->err = 0;
}

// TopKV2 (topk_op.cc:104-205): one workgroup per row.
__global__ __launch_bounds__(kNT) void k_topk(const float* values, long long n_cols, int k,
                                              float* out_values, int32_t* out_indices) {
  __shared__ __attribute__((aligned(16))) unsigned char scratch[sizeof(TopkScratch)];
  const long long row = blockIdx.x;
  wg_topk(nullptr, values + row * n_cols, nullptr, (int)n_cols, k, out_indices + row * k, nullptr,
          out_values + row * k, nullptr, nullptr, scratch);
}

// TopKV2 with k beyond the radix-select kernel's 1024 (topk_op.cc:154-173 sorts the whole row
// when k == n; the reference's own tests go to k = n = 5000): one workgroup per row, the row's
// (key, ~position) pairs bitonic-sorted in LDS (n <= 16384 -> 128 KB), first k written out.
__global__ __launch_bounds__(kNT) void k_topk_sort(const float* values, long long n_cols, int k, int n_pow2,
                                                   float* out_values, int32_t* out_indices) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned long long* e = reinterpret_cast<unsigned long long*>(smem);
  const long long row = blockIdx.x;
  const float* v = values + row * n_cols;
  for (int i = threadIdx.x; i < n_pow2; i += kNT)  // pads sort behind every real pair (key 0 is below any score key)
    e[i] = i < n_cols ? (((unsigned long long)score_key(v[i]) << 32) | (uint32_t)(~(uint32_t)i)) : 0ull;
  __syncthreads();
  for (int size = 2; size <= n_pow2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < (n_pow2 >> 1); t += kNT) {
        const int lo = ((t / stride) * stride << 1) + (t % stride), hi = lo + stride;
        const bool desc = ((lo & size) == 0);  // descending overall
        const unsigned long long a = e[lo], b = e[hi];
        if ((a < b) == desc) { e[lo] = b; e[hi] = a; }
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < k; i += kNT) {
    const int pos = (int)(~(uint32_t)(e[i] & 0xffffffffull));
    out_indices[row * k + i] = pos;
    out_values[row * k + i] = v[pos];
  }
}

// ===========================================================================
// C ABI
// ===========================================================================
// ---- HugeConst -------------------------------------------------------------
// The .npy decoder is a host header of its own (host/nann_npy.h: every length checked, fuzzed under ASan in the CPU suite);
// here: the file into memory, the decoder, the payload into HBM.
int nann::read_whole_file(const char* path, std::vector<unsigned char>* out) {
  std::ifstream f(path, std::ifstream::binary | std::ifstream::ate);
  if (!f) return fail(NANN_ERR_IO, std::string("Fail to open file: ") + path);  // huge_const_op.cc:96-98
  const std::streamoff size = f.tellg();
  if (size < 0) return fail(NANN_ERR_IO, std::string("Fail to open file: ") + path);
  out->resize((size_t)size);
  f.seekg(0);
  if (size > 0) f.read(reinterpret_cast<char*>(out->data()), size);
  if (!f || f.gcount() != size) return fail(NANN_ERR_IO, std::string("short read of ") + path);
  return NANN_OK;
}

extern "C" {

int nann_huge_const_load(const char* path, int expect_dtype, const int64_t* expect_shape,
                         int expect_rank, int allow_cast, void** dev_ptr, int64_t* nbytes) {
  if (!path || !dev_ptr) return fail(NANN_ERR_BAD_ARGUMENT, "nann_huge_const_load: null argument");
  std::vector<unsigned char> image;
  int rc = read_whole_file(path, &image);
  if (rc) return rc;
  const unsigned char* payload = nullptr;
  size_t bytes = 0;
  std::vector<char> conv;
  std::string err;
  rc = nann_npy::decode(image.data(), image.size(), expect_dtype, expect_shape, expect_rank, allow_cast != 0, &payload, &bytes, &conv,
                        nullptr, &err);
  if (rc) return fail(rc, err);
  const int64_t total = (int64_t)bytes;
  void* d = nullptr;
  HIP_TRY(hipMalloc(&d, (size_t)std::max<int64_t>(total, 1)));
  if (total) {
    const hipError_t e = hipMemcpy(d, payload, (size_t)total, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(d);  // do not leak the allocation on a failed copy
      return fail(NANN_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
    }
  }
  *dev_ptr = d;
  if (nbytes) *nbytes = total;
  return NANN_OK;
}

// ---- GroupGather -----------------------------------------------------------
int nann_group_gather_count(const int64_t* params_row_splits, int64_t n_params_splits,
                            int64_t n_params_values, const int64_t* indices_values,
                            int64_t n_indices_values, const int64_t* indices_row_splits,
                            int64_t n_indices_splits, int64_t* ret_row_splits,
                            int64_t* scratch_offsets, int64_t* n_ret, int64_t* n_ret_splits,
                            int32_t* ragged_code, nann_stream_t stream) {
  if (!n_ret || !n_ret_splits) return fail(NANN_ERR_BAD_ARGUMENT, "nann_group_gather_count: null out");
  ResultBuf* rb;
  int rc = get_result_buf(&rb);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_group_gather_count, dim3(1), dim3(kNT), 0, st, params_row_splits,
                     (long long)n_params_splits, (long long)n_params_values, indices_values,
                     (long long)n_indices_values, indices_row_splits, (long long)n_indices_splits,
                     ret_row_splits, scratch_offsets, rb->dev);
  HIP_TRY(hipGetLastError());
  rc = fetch_result(rb, st);
  if (rc) return rc;
  if (ragged_code) *ragged_code = rb->host->code;
  *n_ret = rb->host->n_out;
  *n_ret_splits = rb->host->n_out_splits;
  if (rb->host->err) return fail(rb->host->err, "GroupGather: invalid input, code " +
                                                    std::to_string(rb->host->code));
  return NANN_OK;
}

int nann_group_gather_fill(const int32_t* params_values, const int64_t* params_row_splits,
                           const int64_t* indices_values, int64_t n_indices_values,
                           const int64_t* scratch_offsets, int32_t* ret_values,
                           nann_stream_t stream) {
  if (n_indices_values <= 0) return NANN_OK;
  const int waves_per_block = 4;
  const long long blocks = std::min<long long>((n_indices_values + waves_per_block - 1) / waves_per_block, 4096);
  hipLaunchKernelGGL(k_group_gather_fill, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                     params_values, params_row_splits, indices_values, (long long)n_indices_values,
                     scratch_offsets, ret_values);
  HIP_TRY(hipGetLastError());
  return NANN_OK;
}

// ---- GroupGather unique=true: the set of every group of a unique=false result, first-occurrence order ---------
static uint64_t ggu_table_slots(int64_t n_values) {
  uint64_t t = 64;
  while (t < 2 * (uint64_t)n_values) t <<= 1;
  return t;
}
int nann_group_gather_unique_scratch_bytes(int64_t n_values, int64_t n_splits, int64_t* nbytes) {
  if (!nbytes || n_values < 0 || n_splits < 0) return fail(NANN_ERR_BAD_ARGUMENT, "nann_group_gather_unique_scratch_bytes: bad argument");
  if (n_values > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, "GroupGather unique: more than 2^31 values");
  *nbytes = (int64_t)(ggu_table_slots(n_values) * 8 + (((uint64_t)n_values * 4 + 255) & ~255ull) + (uint64_t)(n_splits + 1) * 8);
  return NANN_OK;
}
int nann_group_gather_unique(const int32_t* values, int64_t n_values, const int64_t* row_splits, int64_t n_splits,
                             void* scratch, int32_t* out_values, int64_t* out_row_splits, int64_t* n_out,
                             nann_stream_t stream) {
  if (!n_out) return fail(NANN_ERR_BAD_ARGUMENT, "nann_group_gather_unique: null out");
  if (n_splits < 1) return fail(NANN_ERR_BAD_ARGUMENT, "nann_group_gather_unique: row_splits of the unique=false result expected");
  if (n_values > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, "GroupGather unique: more than 2^31 values");
  hipStream_t st = as_stream(stream);
  const long long n_groups = n_splits - 1;
  if (n_values == 0 || n_groups == 0) {  // every group empty: row_splits of zeros
    HIP_TRY(hipMemsetAsync(out_row_splits, 0, (size_t)n_splits * 8, st));
    *n_out = 0;
    return NANN_OK;
  }
  if (!scratch) return fail(NANN_ERR_BAD_ARGUMENT, "nann_group_gather_unique: null scratch");
  ResultBuf* rb;
  int rc = get_result_buf(&rb);
  if (rc) return rc;
  const uint64_t slots = ggu_table_slots(n_values);
  unsigned long long* table = static_cast<unsigned long long*>(scratch);
  uint32_t* grp = reinterpret_cast<uint32_t*>(table + slots);
  long long* counts = reinterpret_cast<long long*>(reinterpret_cast<unsigned char*>(grp) + (((uint64_t)n_values * 4 + 255) & ~255ull));
  const uint32_t mask = (uint32_t)(slots - 1);
  HIP_TRY(hipMemsetAsync(table, 0xff, slots * 8, st));
  const unsigned gblocks = (unsigned)std::min<long long>(n_groups, 4096);
  const unsigned pblocks = (unsigned)std::min<long long>((n_values + 255) / 256, 4096);
  hipLaunchKernelGGL(k_ggu_groups, dim3(gblocks), dim3(256), 0, st, row_splits, n_groups, grp);
  hipLaunchKernelGGL(k_ggu_insert, dim3(pblocks), dim3(256), 0, st, values, (long long)n_values, grp, table, mask);
  hipLaunchKernelGGL(k_ggu_count, dim3(gblocks), dim3(256), 0, st, values, row_splits, n_groups, grp, table, mask, counts);
  hipLaunchKernelGGL(k_ggu_scan, dim3(1), dim3(kNT), 0, st, counts, n_groups, out_row_splits, rb->dev);
  hipLaunchKernelGGL(k_ggu_emit, dim3(gblocks), dim3(256), 0, st, values, row_splits, n_groups, grp, table, mask,
                     out_row_splits, out_values);
  HIP_TRY(hipGetLastError());
  rc = fetch_result(rb, st);
  if (rc) return rc;
  *n_out = rb->host->n_out;
  return NANN_OK;
}

// ---- BitmapRefDifference -----------------------------------------------------
int nann_bitmap_ref_difference(const int32_t* values, int64_t n_values, const int64_t* row_splits,
                               int64_t n_splits, int32_t* idx_flag, int64_t n_flag_words,
                               int32_t* c_values, int64_t* c_row_splits, int64_t* n_out,
                               int64_t* n_out_splits, int32_t* ragged_code, nann_stream_t stream) {
  if (!n_out || !n_out_splits) return fail(NANN_ERR_BAD_ARGUMENT, "nann_bitmap_ref_difference: null out");
  if (n_values > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, "more than 2^31 candidates");
  DeviceInfo di;
  int rc = device_info(&di);
  if (rc) return rc;
  ResultBuf* rb;
  rc = get_result_buf(&rb);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  const size_t lds_need = align_up((size_t)n_flag_words * 4, 16) + 16;
  const bool lds = lds_need <= di.lds_max;
  uint32_t* flags = reinterpret_cast<uint32_t*>(idx_flag);
  if (lds) {
    auto kern = k_bitmap_ref_difference<true>;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_need));
    hipLaunchKernelGGL(kern, dim3(1), dim3(kNT), lds_need, st, values, (long long)n_values, row_splits,
                       (long long)n_splits, flags, (long long)n_flag_words, c_values, c_row_splits,
                       rb->dev);
  } else {
    hipLaunchKernelGGL(k_bitmap_ref_difference<false>, dim3(1), dim3(kNT), 16, st, values,
                       (long long)n_values, row_splits, (long long)n_splits, flags,
                       (long long)n_flag_words, c_values, c_row_splits, rb->dev);
  }
  HIP_TRY(hipGetLastError());
  rc = fetch_result(rb, st);
  if (rc) return rc;
  if (ragged_code) *ragged_code = rb->host->code;
  *n_out = rb->host->n_out;
  *n_out_splits = rb->host->n_out_splits;
  if (rb->host->err) return fail(rb->host->err, "BitmapRefDifference: invalid input");
  return NANN_OK;
}

// ---- BloomFilterDifference ---------------------------------------------------------
static long long bloom_prime_below(long long num) {  // bitmap_ops.cc:384-403
  for (long long n = num; n > 1; --n) {
    bool prime = true;
    for (long long i = (long long)(std::sqrt((double)n) + 1e-6); i > 1; --i)
      if (n % i == 0) { prime = false; break; }
    if (prime) return n;
  }
  return 1;
}

int nann_bloom_filter_difference(const int32_t* values, int64_t n_values, const int64_t* row_splits,
                                 int64_t n_splits, int32_t* idx_flag, int64_t n_flag_words, int64_t bucket,
                                 int64_t bucket_size, int32_t* c_values, int64_t* c_row_splits, int64_t* n_out,
                                 int64_t* n_out_splits, int32_t* ragged_code, nann_stream_t stream) {
  if (!n_out || !n_out_splits) return fail(NANN_ERR_BAD_ARGUMENT, "nann_bloom_filter_difference: null out");
  if (bucket < 0 || bucket_size < 1 || n_flag_words < bucket_size)
    return fail(NANN_ERR_BAD_ARGUMENT, "BloomFilterDifference: bucket >= 0, bucket_size >= 1, idx_flag >= bucket_size words");
  if (bucket_size > (1ll << 26)) return fail(NANN_ERR_UNSUPPORTED, "BloomFilterDifference: filter beyond 2^31 bits");
  DeviceInfo di;
  int rc = device_info(&di);
  if (rc) return rc;
  ResultBuf* rb;
  rc = get_result_buf(&rb);
  if (rc) return rc;
  BloomParams B;
  B.bucket = bucket; B.bucket_size = bucket_size;
  const int modp[4] = {29, 47, 67, 83};  // multi_hash_mod_param, bitmap_ops.cc:297
  for (int l = 0; l < 4; ++l) B.prime[l] = (unsigned long long)bloom_prime_below((long long)modp[l] * bucket_size * 32);
  hipStream_t st = as_stream(stream);
  const size_t lds_need = align_up((size_t)n_flag_words * 4, 16);
  uint32_t* flags = reinterpret_cast<uint32_t*>(idx_flag);
  if (lds_need <= di.lds_max) {
    auto kern = k_bloom_filter_difference<true>;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)std::max<size_t>(lds_need, 16)));
    hipLaunchKernelGGL(kern, dim3(1), dim3(kNT), std::max<size_t>(lds_need, 16), st, values, (long long)n_values,
                       row_splits, (long long)n_splits, flags, (long long)n_flag_words, B, c_values, c_row_splits, rb->dev);
  } else {
    hipLaunchKernelGGL(k_bloom_filter_difference<false>, dim3(1), dim3(kNT), 16, st, values, (long long)n_values,
                       row_splits, (long long)n_splits, flags, (long long)n_flag_words, B, c_values, c_row_splits, rb->dev);
  }
  HIP_TRY(hipGetLastError());
  rc = fetch_result(rb, st);
  if (rc) return rc;
  if (ragged_code) *ragged_code = rb->host->code;
  *n_out = rb->host->n_out;
  *n_out_splits = rb->host->n_out_splits;
  if (rb->host->err) return fail(rb->host->err, "BloomFilterDifference: invalid input");
  return NANN_OK;
}

// ---- GatherV2 ------------------------------------------------------------------
int nann_gather_rows(const void* params, int64_t n_rows, int64_t row_bytes, const int32_t* indices,
                     int64_t n_indices, void* out, int64_t* bad_i, nann_stream_t stream) {
  if (row_bytes <= 0 || row_bytes % 4) return fail(NANN_ERR_BAD_ARGUMENT, "row_bytes must be a multiple of 4");
  if (bad_i) *bad_i = -1;
  if (n_indices <= 0) return NANN_OK;
  ResultBuf* rb;
  int rc = get_result_buf(&rb);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_init_result, dim3(1), dim3(1), 0, st, rb->dev);
  const bool vec = row_bytes % 16 == 0 && (reinterpret_cast<uintptr_t>(params) % 16 == 0) &&
                   (reinterpret_cast<uintptr_t>(out) % 16 == 0);
  const long long words = vec ? row_bytes / 16 : row_bytes / 4;
  const long long total = n_indices * words;
  const unsigned blocks = (unsigned)std::min<long long>((total + 255) / 256, 8192);
  if (vec)
    hipLaunchKernelGGL(k_gather_rows<uint4>, dim3(blocks), dim3(256), 0, st,
                       static_cast<const uint4*>(params), (long long)n_rows, words, indices,
                       (long long)n_indices, static_cast<uint4*>(out), rb->dev);
  else
    hipLaunchKernelGGL(k_gather_rows<uint32_t>, dim3(blocks), dim3(256), 0, st,
                       static_cast<const uint32_t*>(params), (long long)n_rows, words, indices,
                       (long long)n_indices, static_cast<uint32_t*>(out), rb->dev);
  HIP_TRY(hipGetLastError());
  rc = fetch_result(rb, st);
  if (rc) return rc;
  if (rb->host->bad_i != 0x7fffffffffffffffll) {
    if (bad_i) *bad_i = rb->host->bad_i;
    return fail(NANN_ERR_INDEX_OUT_OF_RANGE, "indices[" + std::to_string(rb->host->bad_i) +
                                                 "] is not in [0, " + std::to_string(n_rows) + ")");
  }
  return NANN_OK;
}

// ---- TopKV2 ----------------------------------------------------------------------
int nann_topk(const float* values, int64_t n_rows, int64_t n_cols, int32_t k, float* out_values,
              int32_t* out_indices, nann_stream_t stream) {
  if (k < 0) return fail(NANN_ERR_BAD_ARGUMENT, "Need k >= 0, got " + std::to_string(k));  // :60-61
  if (n_cols < k)
    return fail(NANN_ERR_TOPK_K_GT_N, "input must have at least k columns. Had " +
                                          std::to_string(n_cols) + ", needed " + std::to_string(k));
  if (n_cols > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, "n_cols too large");
  if (k == 0 || n_rows == 0) return NANN_OK;  // :84-85
  if (k > kMaxK) {  // whole-row sort in LDS
    if (n_cols > 16384) return fail(NANN_ERR_UNSUPPORTED, "k > 1024 needs n_cols <= 16384");
    int p2 = 2;
    while (p2 < n_cols) p2 <<= 1;
    auto kern = k_topk_sort;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                p2 * 8));
    hipLaunchKernelGGL(kern, dim3((unsigned)n_rows), dim3(kNT), (size_t)p2 * 8, as_stream(stream), values,
                       (long long)n_cols, (int)k, p2, out_values, out_indices);
    HIP_TRY(hipGetLastError());
    return NANN_OK;
  }
  hipLaunchKernelGGL(k_topk, dim3((unsigned)n_rows), dim3(kNT), 0, as_stream(stream), values,
                     (long long)n_cols, (int)k, out_values, out_indices);
  HIP_TRY(hipGetLastError());
  return NANN_OK;
}

}  // extern "C"
