// nann_hip.hip -- kernels + C ABI of libnann_hip.so (gfx950 only).
// The ABI is documented in include/nann_hip.h; the workgroup building blocks
// in nann_device.h.  Reference citations are relative to /root/reference/.
#include "nann_eval.h"
#include "nann_attn.h"
#include "nann_order_kernels.h"
#include "nann_scan.h"
#include "nann_cand.h"
#include "host/nann_graphdef_text.h"
#include "host/nann_blaze_options.h"
#include "host/nann_npy.h"
#include "host/nann_projcache.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include <sys/stat.h>

using namespace nann;

// ===========================================================================
// host-side helpers
// ===========================================================================
namespace nann {
thread_local std::string g_err;
int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
}  // namespace nann

namespace {

#define HIP_TRY(expr)                                                                    \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess)                                                                \
      return fail(NANN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));      \
  } while (0)

struct DeviceInfo {
  bool ok = false;
  int cus = 0;
  size_t lds_max = 0;
};

// per-device facts, queried once
int device_info(DeviceInfo* out) {
  static std::mutex mu;
  static DeviceInfo cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return fail(NANN_ERR_NO_DEVICE, "no HIP device");
  if (dev < 0 || dev >= 64) return fail(NANN_ERR_NO_DEVICE, "device ordinal out of range");
  std::lock_guard<std::mutex> lk(mu);
  if (!cache[dev].ok) {
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, dev));
    cache[dev].cus = p.multiProcessorCount;
    cache[dev].lds_max = p.maxSharedMemoryPerMultiProcessor ? p.maxSharedMemoryPerMultiProcessor
                                                            : p.sharedMemPerBlock;
    if (cache[dev].lds_max < p.sharedMemPerBlock) cache[dev].lds_max = p.sharedMemPerBlock;
    cache[dev].ok = true;
  }
  *out = cache[dev];
  return NANN_OK;
}

struct ResultBuf {
  OpResult* dev = nullptr;
  OpResult* host = nullptr;
  int device = -1;
};

int get_result_buf(ResultBuf** out) {
  thread_local ResultBuf rb;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (!rb.dev || rb.device != dev) {
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&rb.dev), sizeof(OpResult)));
    if (!rb.host) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&rb.host), sizeof(OpResult)));
    rb.device = dev;
  }
  *out = &rb;
  return NANN_OK;
}

int fetch_result(ResultBuf* rb, hipStream_t st) {
  HIP_TRY(hipMemcpyAsync(rb->host, rb->dev, sizeof(OpResult), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return NANN_OK;
}

inline hipStream_t as_stream(nann_stream_t s) { return reinterpret_cast<hipStream_t>(s); }
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

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

// merge of per-shard top-k lists: TopKV2 over the shard-major
// concatenation, ids carried along.
__global__ __launch_bounds__(kNT) void k_merge_topk(const float* scores, const int64_t* ids,
                                                    int n_in, int k_out, float* out_scores,
                                                    int64_t* out_ids) {
  __shared__ __attribute__((aligned(16))) unsigned char scratch[sizeof(TopkScratch)];
  const long long qi = blockIdx.x;
  wg_topk(nullptr, scores + qi * n_in, nullptr, n_in, k_out, nullptr, nullptr, out_scores + qi * k_out,
          ids + qi * n_in, out_ids + qi * k_out, scratch);
}

// comm_seq f16[B, L, d] -> q f32[B, d]; one workgroup per query, one thread per
// dimension.  Same order as oracle_user_seq_mean.
__global__ void k_user_seq_mean(const uint16_t* seq, int seq_len, int d, float* q) {
  // generic form (any d, any seq_len): one thread per row for the count, one per column for the sums
  __shared__ int s_count;
  const long long b = blockIdx.x;
  const uint16_t* s = seq + b * seq_len * d;
  if (threadIdx.x == 0) s_count = 0;
  __syncthreads();
  for (int r = threadIdx.x; r < seq_len; r += blockDim.x) {
    int nz = 0;
    for (int k = 0; k < d; ++k) nz |= (s[(long long)r * d + k] & 0x7fffu) != 0;
    if (nz) atomicAdd(&s_count, 1);
  }
  __syncthreads();
  const int count = s_count;
  for (int k = threadIdx.x; k < d; k += blockDim.x) {
    float acc = 0.0f;
    for (int r = 0; r < seq_len; ++r) acc = acc + half_bits_to_float(s[(long long)r * d + k]);
    q[b * d + k] = count ? acc / (float)count : 0.0f;
  }
}

// The shape the serving path feeds (d a multiple of 8, one history <= 48 KB: 50 x 128 f16 = 12.8 KB).  Round 5: the
// generic kernel above read 52 MB at 0.66 TB/s (each of <= 50 threads scanning a whole row with 2-byte strided loads,
// then 2-byte loads again for the sums: 80 us per 4096 queries, 4.3 % of the headline step).  Here a 256-thread
// workgroup copies its query's history into LDS with 16-byte loads, all of them in flight at once (seq_len d / 8
// pieces, row-major = fully coalesced) and flags the non-zero pieces on the way.  The sums then run out of LDS in the
// oracle's order -- per column one chain over the rows ascending from +0, one divide (oracle_user_seq_mean) -- so the
// result is bitwise the generic kernel's.
constexpr int kSeqMeanThreads = 256;
constexpr int kSeqMeanMaxBytes = 48 * 1024;
__global__ __launch_bounds__(kSeqMeanThreads) void k_user_seq_mean_lds(const uint4* seq, int seq_len, int d, float* q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char seq_smem[];
  __shared__ int s_count;
  uint4* rows = reinterpret_cast<uint4*>(seq_smem);
  const int tid = threadIdx.x;
  const int ppr = d >> 3;                 // 16-byte pieces per row
  const int n_pieces = seq_len * ppr;
  const uint4* src = seq + (long long)blockIdx.x * n_pieces;
  if (tid == 0) s_count = 0;
  constexpr int kMaxPer = (kSeqMeanMaxBytes / 16 + kSeqMeanThreads - 1) / kSeqMeanThreads;  // 12
  uint4 v[kMaxPer];
#pragma unroll
  for (int j = 0; j < kMaxPer; ++j) {
    const int i = tid + j * kSeqMeanThreads;
    v[j] = (i < n_pieces) ? src[i] : uint4{0u, 0u, 0u, 0u};
  }
  __syncthreads();  // (s_count = 0 above)
  // piece i belongs to row i / ppr; the pieces of a row can straddle wavefronts and trips, so "this piece has a non-zero
  // element" goes through one flag byte per piece and thread r ORs row r's flags behind the barrier
  unsigned char* nzf = seq_smem + (size_t)n_pieces * 16;  // one byte per piece
#pragma unroll
  for (int j = 0; j < kMaxPer; ++j) {
    const int i = tid + j * kSeqMeanThreads;
    if (i < n_pieces) {
      rows[i] = v[j];
      // +-0 halves are zero: both sign bits of a word are cleared before the test
      nzf[i] = ((v[j].x | v[j].y | v[j].z | v[j].w) & 0x7fff7fffu) ? 1 : 0;
    }
  }
  __syncthreads();
  for (int r = tid; r < seq_len; r += kSeqMeanThreads) {
    int nz = 0;
    for (int k = 0; k < ppr; ++k) nz |= nzf[r * ppr + k];
    if (nz) atomicAdd(&s_count, 1);
  }
  __syncthreads();
  const int count = s_count;
  const uint16_t* h = reinterpret_cast<const uint16_t*>(seq_smem);
  for (int k = tid; k < d; k += kSeqMeanThreads) {
    float acc = 0.0f;
    for (int r = 0; r < seq_len; ++r) acc = acc + half_bits_to_float(h[r * d + k]);
    q[(long long)blockIdx.x * d + k] = count ? acc / (float)count : 0.0f;
  }
}

// stand-alone scorer (the BlazeXlaOp contract): rows scored independently.
template <int LPR, int DT>
__global__ __launch_bounds__(256) void k_score_l2(const void* table, long long n_table_rows, int d,
                                                  const int32_t* indices, long long n,
                                                  const float* qv, float* scores, OpResult* res) {
  constexpr int GPW = 64 / LPR;
  const int lane = lane_id();
  const int sub = lane % LPR, grp = lane / LPR;
  float q[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) q[k] = qv[sub * 8 + k];
  const long long wave_global = (long long)blockIdx.x * (blockDim.x >> 6) + wave_id();
  const long long n_waves = (long long)gridDim.x * (blockDim.x >> 6);
  for (long long i0 = wave_global * GPW; i0 < n; i0 += n_waves * GPW) {
    const long long i = i0 + grp;
    long long row = -1;
    if (i < n) {
      row = indices ? (long long)indices[i] : i;
      if (row < 0 || row >= n_table_rows) {
        if (sub == 0) atomicMin(reinterpret_cast<unsigned long long*>(&res->bad_i), (unsigned long long)i);
        row = -1;
      }
    }
    float x[8];
    if (row >= 0) {
      const RowChunk<DT> ch = load_chunk<DT>(table, (size_t)row, d, sub);
      chunk_to_float<DT>(ch, x);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) x[k] = 0.0f;
    }
    const float s = l2_finish<LPR>(q, x);
    if (sub == 0 && i < n) scores[i] = s;
  }
}

// The inner product <q, row> (NANN_SCORER_IP): k_score_l2 with ip_finish.  (A kernel of its own and not a shared body: routed
// through a common device function, k_score_l2<64, *> came out of the register allocator two VGPRs wider than before.)
template <int LPR, int DT>
__global__ __launch_bounds__(256) void k_score_ip(const void* table, long long n_table_rows, int d,
                                                  const int32_t* indices, long long n,
                                                  const float* qv, float* scores, OpResult* res) {
  constexpr int GPW = 64 / LPR;
  const int lane = lane_id();
  const int sub = lane % LPR, grp = lane / LPR;
  float q[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) q[k] = qv[sub * 8 + k];
  const long long wave_global = (long long)blockIdx.x * (blockDim.x >> 6) + wave_id();
  const long long n_waves = (long long)gridDim.x * (blockDim.x >> 6);
  for (long long i0 = wave_global * GPW; i0 < n; i0 += n_waves * GPW) {
    const long long i = i0 + grp;
    long long row = -1;
    if (i < n) {
      row = indices ? (long long)indices[i] : i;
      if (row < 0 || row >= n_table_rows) {
        if (sub == 0) atomicMin(reinterpret_cast<unsigned long long*>(&res->bad_i), (unsigned long long)i);
        row = -1;
      }
    }
    float x[8];
    if (row >= 0) {
      const RowChunk<DT> ch = load_chunk<DT>(table, (size_t)row, d, sub);
      chunk_to_float<DT>(ch, x);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) x[k] = 0.0f;
    }
    const float s = ip_finish<LPR>(q, x);
    if (sub == 0 && i < n) scores[i] = s;
  }
}

// ===========================================================================
// C ABI
// ===========================================================================
// The item-only part of a split-f16 scorer, pre-projected for the indices the scorer has searched (nann_mlp3.h: the item
// half of the MLP's layer 1, f32 [n_items, 256]; nann_attn_proj.h: q_ and the e rows of DNN layer 1, f32 [n_items, 384]):
// built at the first nann_search of the (scorer, index) pair, at most two kept per scorer (the older one goes).
// Lifecycle (round 4): host/nann_projcache.h -- ref-counted tables, LRU among the unpinned ones, retirement instead of
// freeing (an event per stream behind every launch that reads a table), pinning by nann_*_prepare.
struct HipProjBackend {
  typedef hipStream_t Stream;
  typedef hipEvent_t Event;
  static bool malloc(void** p, size_t bytes) {
    if (hipMalloc(p, bytes) == hipSuccess) return true;
    (void)hipGetLastError();  // not sticky: the search goes on without a table
    return false;
  }
  static void free(void* p) { (void)hipFree(p); }
  static bool mem_info(size_t* free_b) {
    size_t total = 0;
    if (hipMemGetInfo(free_b, &total) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
  }
  static bool event_create(Event* e) {
    if (hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
  }
  static void event_destroy(Event e) { (void)hipEventDestroy(e); }
  static void event_record(Event e, Stream s) { (void)hipEventRecord(e, s); }
  static bool event_done(Event e) { return hipEventQuery(e) != hipErrorNotReady; }
  static void event_wait(Event e) { (void)hipEventSynchronize(e); }
};
typedef nann::ProjCacheT<HipProjBackend> ProjCache;
typedef nann::ProjTableT<HipProjBackend> ProjTable;
// ---- options of a search call -------------------------------------------------------------------------------------
// Every knob of the planner is a field of nann_search_options (include/nann_hip.h, round 5); a field left at -1 takes the
// PROCESS DEFAULT: what nann_set_traversal_mode / nann_set_search_reserve / nann_set_preprojection last stored, else the
// environment read ONCE below (A/B tooling: NANN_PREPROJECT=0, NANN_SEARCH_SLOT_RESERVE=n, NANN_MLP_FORM=fused|phased,
// NANN_PHASE_SMALL32=0, NANN_QUERY_ORDER=0, NANN_LEAN_KERNEL=0), else the built-in value.  plan_search and the launchers only ever see the resolved struct.
struct SearchOpt {
  int mode;        // nann_traversal_mode
  int reserve;     // workgroup slots the persistent grids leave free
  int preproject;  // 1: the MLP / attention scorers read their pre-projected tables
  int mlp_form;    // nann_mlp_form
  int small32;     // 1: at most one query per CU -> one 1024-thread workgroup per CU for the traversal (stages)
  int order;       // 1: L2 hash-set plans run a batch larger than their slots in locality order (nann_order.h)
  int lean;        // 1: a plain L2 / inner-product call on a hash-set plan launches k_search_lean (nann_search.h)
};
static std::atomic<int> g_traversal_mode{-1}, g_slot_reserve{-1}, g_preproject{-1};
static const SearchOpt& env_defaults() {
  static const SearchOpt d = [] {
    SearchOpt o{NANN_TRAVERSAL_AUTO, 0, 1, NANN_MLP_FORM_AUTO, 1, 1, 1};
    if (const char* e = std::getenv("NANN_PREPROJECT")) o.preproject = !(e[0] == '0' && e[1] == 0);
    if (const char* e = std::getenv("NANN_SEARCH_SLOT_RESERVE")) o.reserve = std::max(0, std::atoi(e));
    if (const char* e = std::getenv("NANN_MLP_FORM")) o.mlp_form = std::string(e) == "fused" ? NANN_MLP_FORM_FUSED : std::string(e) == "phased" ? NANN_MLP_FORM_PHASED : NANN_MLP_FORM_AUTO;
    if (const char* e = std::getenv("NANN_PHASE_SMALL32")) o.small32 = !(e[0] == '0');
    if (const char* e = std::getenv("NANN_QUERY_ORDER")) o.order = !(e[0] == '0');
    if (const char* e = std::getenv("NANN_LEAN_KERNEL")) o.lean = !(e[0] == '0');
    return o;
  }();
  return d;
}
static SearchOpt resolve_options(const nann_search_options* u) {
  SearchOpt o = env_defaults();
  const int gm = g_traversal_mode.load(std::memory_order_relaxed), gr = g_slot_reserve.load(std::memory_order_relaxed),
            gp = g_preproject.load(std::memory_order_relaxed);
  if (gm >= 0) o.mode = gm;
  if (gr >= 0) o.reserve = gr;
  if (gp >= 0) o.preproject = gp;
  if (u) {
    // struct_bytes: a caller built against an older header passes a shorter struct; fields behind it keep their defaults
    const size_t nb = u->struct_bytes > 0 ? (size_t)u->struct_bytes : sizeof(*u);
    auto has = [&](const int32_t* f) { return (size_t)(reinterpret_cast<const char*>(f) - reinterpret_cast<const char*>(u)) + 4 <= nb; };
    if (has(&u->traversal_mode) && u->traversal_mode >= 0) o.mode = u->traversal_mode;
    if (has(&u->slot_reserve) && u->slot_reserve >= 0) o.reserve = u->slot_reserve;
    if (has(&u->preprojection) && u->preprojection >= 0) o.preproject = u->preprojection != 0;
    if (has(&u->mlp_form) && u->mlp_form >= 0) o.mlp_form = u->mlp_form;
  }
  return o;
}
static int check_options(const nann_search_options* u) {
  if (!u) return NANN_OK;
  if (u->struct_bytes < 0 || (u->struct_bytes > 0 && u->struct_bytes < 8)) return fail(NANN_ERR_BAD_ARGUMENT, "nann_search_options: struct_bytes");
  const SearchOpt o = resolve_options(u);
  if (o.mode < NANN_TRAVERSAL_AUTO || o.mode > NANN_TRAVERSAL_LDS_HASH32) return fail(NANN_ERR_BAD_ARGUMENT, "nann_search_options: unknown traversal_mode");
  if (o.mlp_form < NANN_MLP_FORM_AUTO || o.mlp_form > NANN_MLP_FORM_PHASED) return fail(NANN_ERR_BAD_ARGUMENT, "nann_search_options: unknown mlp_form");
  return NANN_OK;
}

struct nann_scorer {
  nann_scorer_desc desc;
  float* dev_weights = nullptr;  // MLP weights block in HBM
  uint4* dev_packed = nullptr;   // split-f16 planes in MFMA A-fragment order
  float4* dev_packed_x = nullptr;  // W2 as f32 A fragments (exact form, layer 2 resident in LDS)
  float* dev_cert = nullptr;       // certified form: the filter's c_j (certified_bound)
  MlpParams mlp = {};
  mutable ProjCache proj;
};

struct nann_attn_scorer {
  AttnParams P = {};
  int emb_dtype = 0;
  int precision = NANN_MLP_EXACT_F32;  // NANN_MLP_SPLIT_F16: the split-f16 kernels (nann_attn_split.h, nann_attn_proj.h)
  float* dev_weights = nullptr;
  uint4* dev_packed = nullptr;         // split form: A fragments + pre-scaled vectors
  mutable ProjCache proj;
};

struct nann_index {
  nann_index_desc desc;  // device pointers
  uint64_t uid = 0;      // process-unique (a scorer keys its per-index tables by it; a pointer could be reused)
  bool owns = false;
  std::vector<void*> owned;
  int64_t max_deg[2] = {0, 0};
  uint32_t bm_words = 0;  // ceil(N/32) padded to a multiple of 4
  // the probe launch of nann_index_create (round 5): new level-0 nodes per frontier row, measured on THIS graph
  bool probe_valid = false;
  int probe_ef = 0, probe_queries = 0;
  float probe_new_per_row_mean = 0.0f, probe_new_per_row_q90 = 0.0f, probe_new_per_row_max = 0.0f;
  // the pivots of the batch order (nann_order.h): f32 [d][n_pivots] rows, then their squared norms (kOrderMaxPivots
  // floats); n_pivots < 2: no order
  float* pivots = nullptr;
  int n_pivots = 0;
};
// the probe and the batch order of nann_index_create (nann_traverse.hip, behind this file in the unit, defines them)
static void probe_index(nann_index* ix);
static void choose_pivots(nann_index* ix, const std::vector<int32_t>& enter);
static int launch_order(const nann_index* ix, const float* q, int n, int32_t* key, int32_t* perm, unsigned int* heads,
                        unsigned int* header, hipStream_t st);

extern "C" {

int nann_abi_version(void) { return NANN_ABI_VERSION; }
const char* nann_last_error(void) { return nann::g_err.c_str(); }

int nann_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int nann_malloc(void** dev_ptr, int64_t nbytes) {
  if (!dev_ptr || nbytes < 0) return fail(NANN_ERR_BAD_ARGUMENT, "nann_malloc: bad argument");
  HIP_TRY(hipMalloc(dev_ptr, (size_t)std::max<int64_t>(nbytes, 1)));
  return NANN_OK;
}

int nann_free(void* dev_ptr) {
  if (dev_ptr) HIP_TRY(hipFree(dev_ptr));
  return NANN_OK;
}

int nann_memcpy(void* dst, const void* src, int64_t nbytes, int kind, nann_stream_t stream) {
  static const hipMemcpyKind kinds[3] = {hipMemcpyHostToDevice, hipMemcpyDeviceToHost,
                                         hipMemcpyDeviceToDevice};
  if (kind < 0 || kind > 2 || nbytes < 0) return fail(NANN_ERR_BAD_ARGUMENT, "nann_memcpy: bad argument");
  if (nbytes == 0) return NANN_OK;
  HIP_TRY(hipMemcpyAsync(dst, src, (size_t)nbytes, kinds[kind], as_stream(stream)));
  return NANN_OK;
}

int nann_stream_synchronize(nann_stream_t stream) {
  HIP_TRY(hipStreamSynchronize(as_stream(stream)));
  return NANN_OK;
}

int nann_stream_create(nann_stream_t* out) {
  if (!out) return fail(NANN_ERR_BAD_ARGUMENT, "nann_stream_create: null argument");
  hipStream_t s = nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  *out = reinterpret_cast<nann_stream_t>(s);
  return NANN_OK;
}

int nann_stream_destroy(nann_stream_t stream) {
  if (!stream) return NANN_OK;
  HIP_TRY(hipStreamDestroy(as_stream(stream)));
  return NANN_OK;
}

int nann_host_malloc(void** host_ptr, int64_t nbytes) {
  if (!host_ptr || nbytes < 0) return fail(NANN_ERR_BAD_ARGUMENT, "nann_host_malloc: bad argument");
  HIP_TRY(hipHostMalloc(host_ptr, (size_t)std::max<int64_t>(nbytes, 1), hipHostMallocDefault));
  return NANN_OK;
}

int nann_host_free(void* host_ptr) {
  if (!host_ptr) return NANN_OK;
  HIP_TRY(hipHostFree(host_ptr));
  return NANN_OK;
}

// ---- HugeConst -------------------------------------------------------------
// The .npy decoder is a host header of its own (host/nann_npy.h: every length checked, fuzzed under ASan in the CPU suite);
// here: the file into memory, the decoder, the payload into HBM.
static uint16_t f32_to_f16_rne(float f) { return nann_npy::f32_to_f16_rne(f); }

static int read_whole_file(const char* path, std::vector<unsigned char>* out) {
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

// .npy -> host bytes in `expect_dtype` (the scorer-model loader; HugeConst below copies straight from the file image)
static int read_npy_host(const char* path, int expect_dtype, const int64_t* expect_shape, int expect_rank,
                         int allow_cast, std::vector<char>* out, std::vector<int64_t>* out_shape) {
  std::vector<unsigned char> image;
  int rc = read_whole_file(path, &image);
  if (rc) return rc;
  const unsigned char* payload = nullptr;
  size_t bytes = 0;
  std::vector<char> conv;
  std::string err;
  rc = nann_npy::decode(image.data(), image.size(), expect_dtype, expect_shape, expect_rank, allow_cast != 0, &payload, &bytes, &conv,
                        out_shape, &err);
  if (rc) return fail(rc, err);
  if (!conv.empty() || bytes == 0) { conv.resize(bytes); out->swap(conv); }
  else out->assign(reinterpret_cast<const char*>(payload), reinterpret_cast<const char*>(payload) + bytes);
  return NANN_OK;
}

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

// ---- scorer ------------------------------------------------------------------------
static float f16_bits_to_f32(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
  uint32_t exp = (h >> 10) & 0x1fu, man = h & 0x3ffu, out;
  if (exp == 0) {
    if (man == 0) { out = sign; }
    else {  // subnormal: normalise
      int e = -1;
      do { ++e; man <<= 1; } while (!(man & 0x400u));
      out = sign | ((uint32_t)(127 - 15 - e) << 23) | ((man & 0x3ffu) << 13);
    }
  } else if (exp == 31) {
    out = sign | 0x7f800000u | (man << 13);
  } else {
    out = sign | ((exp - 15 + 127) << 23) | (man << 13);
  }
  float f;
  std::memcpy(&f, &out, 4);
  return f;
}

// 2^7 v = hi + lo with hi = f16(2^7 v), lo = f16(2^7 v - hi)   (nann_mlp.h, split-f16 form: the scaling
// keeps lo a normal f16 for every weight above ~1e-3 in magnitude)
static void split_f16(float v, uint16_t* hi, uint16_t* lo) {
  const float sv = v * 128.0f;
  *hi = f32_to_f16_rne(sv);
  *lo = f32_to_f16_rne(sv - f16_bits_to_f32(*hi));
}

// A fragments of v_mfma_f32_32x32x16_f16 for the item half of W1 and for W2, hi and lo planes:
//   p1[t][kc][plane][lane][i] = W1[d + 16 kc + 8 g + i][32 t + j]                       (j = lane & 31, g = lane >> 5)
//   p2[t][q][m][plane][lane][i] = W2[32 t + (r & 3) + 8 (r >> 2) + 4 g][32 m + j], r = 8 q + i
// (layer 2's k order is the C/D register order of the finished layer-1 tile: nann_mlp.h)
static void pack_split_weights(const float* w1, const float* w2, int d, int h1, int h2, std::vector<uint16_t>* out,
                               size_t* p2_off) {
  const int T = h1 / 32, KC = d / 16, M = h2 / 32;
  const size_t n1 = (size_t)T * KC * 2 * 64 * 8, n2 = (size_t)T * 2 * M * 2 * 64 * 8;
  out->assign(n1 + n2, 0);
  *p2_off = n1;
  for (int t = 0; t < T; ++t)
    for (int kc = 0; kc < KC; ++kc)
      for (int lane = 0; lane < 64; ++lane)
        for (int i = 0; i < 8; ++i) {
          const int j = lane & 31, g = lane >> 5;
          const float v = w1[(size_t)(d + 16 * kc + 8 * g + i) * h1 + 32 * t + j];
          const size_t base = ((size_t)(t * KC + kc) * 2) * 64 * 8;
          split_f16(v, &(*out)[base + (size_t)lane * 8 + i], &(*out)[base + 64 * 8 + (size_t)lane * 8 + i]);
        }
  for (int t = 0; t < T; ++t)
    for (int q = 0; q < 2; ++q)
      for (int m = 0; m < M; ++m)
        for (int lane = 0; lane < 64; ++lane)
          for (int i = 0; i < 8; ++i) {
            const int j = lane & 31, g = lane >> 5, r = 8 * q + i;
            const int k = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * g;
            const float v = w2[(size_t)k * h2 + 32 * m + j];
            const size_t base = n1 + ((size_t)((t * 2 + q) * M + m) * 2) * 64 * 8;
            split_f16(v, &(*out)[base + (size_t)lane * 8 + i], &(*out)[base + 64 * 8 + (size_t)lane * 8 + i]);
          }
}

// The certified form's bound constants (derivation above mlp_filter_vectors, nann_mlp6.h): c_j = sum_m w_jm |w3_m| M_m with
// w_jm = |W2_jm| widened where the f16 plane's error is not within u16 relative, K1 2^-7 and K0; all rounded up to f32.
static void certified_bound(const float* w2, const float* b2, const float* alpha2, const float* w3, int h1, int h2,
                            std::vector<float>* c, float* k1s, float* k0) {
  const double u = std::ldexp(1.0, -24), u16 = std::ldexp(1.0, -11), eta = std::ldexp(1.0, -13);
  auto gam = [&](double n, double unit) { return n * unit / (1.0 - n * unit); };
  const double g257 = gam(h1 + 1, u), gp257 = gam(h1 + 1, 2 * u), g129 = gam(h2 + 1, u);
  const double a1 = u16 * (2 + u16) + gp257 * (1 + u16) * (1 + u16) + g257;
  const double K1 = a1 + (3 * u * (1 + u) + g129 * (1 + 3 * u * (1 + u))) * (1 + g257 + a1) + (u + g129 * (1 + u)) * (1 + g257);
  const double zeta = eta / 128.0 * (1 + gp257) * (1 + u16);
  std::vector<double> wm(h2);
  double sb = 0.0;
  for (int m = 0; m < h2; ++m) {
    wm[m] = std::fabs((double)w3[m]) * std::max(1.0, std::fabs((double)alpha2[m]));
    sb += wm[m] * std::fabs((double)b2[m]);
  }
  auto up = [](double v) {  // the f32 at or above v
    float f = (float)v;
    if ((double)f < v) f = std::nextafter(f, std::numeric_limits<float>::infinity());
    return f;
  };
  c->assign(h1, 0.0f);
  double sc = 0.0;
  for (int j = 0; j < h1; ++j) {
    double cj = 0.0;
    for (int m = 0; m < h2; ++m) {
      const double w = w2[(size_t)j * h2 + m], sw = w * 128.0;
      const double hv = (double)f16_bits_to_f32(f32_to_f16_rne((float)sw));
      double e = std::fabs(hv - sw);
      if (hv != 0.0 && std::fabs(hv) < std::ldexp(1.0, -14)) e = std::max(e, std::fabs(sw));  // subnormal: maybe flushed
      e /= 128.0;
      const double wide = std::fabs(w) + std::max(0.0, e - u16 * std::fabs(w)) / u16;
      cj += wide * wm[m];
    }
    (*c)[j] = up(cj);
    sc += cj;
  }
  constexpr double kMargin = 1.001;  // the kernel's f32 evaluation of B (two chains of 128 fmaf, an add, an fmaf)
  *k1s = up(K1 * kMargin / 128.0);
  *k0 = up((K1 * sb + 2 * zeta * sc) * kMargin + std::ldexp(1.0, -120));
}

int nann_scorer_create(const nann_scorer_desc* desc, nann_scorer** out) {
  if (!desc || !out) return fail(NANN_ERR_BAD_ARGUMENT, "nann_scorer_create: null argument");
  const int d = desc->d;
  if (!(d == 64 || d == 128 || d == 256 || d == 512))
    return fail(NANN_ERR_UNSUPPORTED, "embedding dim must be 64, 128, 256 or 512");
  if (desc->emb_dtype != NANN_F16 && desc->emb_dtype != NANN_BF16 && desc->emb_dtype != NANN_F32)
    return fail(NANN_ERR_UNSUPPORTED, "embedding dtype must be f16, bf16 or f32");
  if (desc->kind != NANN_SCORER_L2 && desc->kind != NANN_SCORER_MLP && desc->kind != NANN_SCORER_IP)
    return fail(NANN_ERR_BAD_ARGUMENT, "unknown scorer kind");
  nann_scorer* s = new nann_scorer();
  s->desc = *desc;
  if (desc->kind == NANN_SCORER_MLP) {
    if (desc->h1 != 256 || desc->h2 != 128 || d > 256) {
      delete s;
      return fail(NANN_ERR_UNSUPPORTED, "MLP scorer: this build has the 2d-256-128-1 shape, d <= 256");
    }
    if (desc->emb_dtype == NANN_F32) {
      delete s;
      return fail(NANN_ERR_UNSUPPORTED, "MLP scorer: item rows must be f16 or bf16");
    }
    if (!desc->w1 || !desc->b1 || !desc->alpha1 || !desc->w2 || !desc->b2 || !desc->alpha2 || !desc->w3) {
      delete s;
      return fail(NANN_ERR_BAD_ARGUMENT, "MLP scorer: null weight pointer");
    }
    const size_t h1 = 256, h2 = 128;
    const size_t n_w1 = 2 * (size_t)d * h1, n_w2 = h1 * h2;
    const size_t total = n_w1 + h1 + h1 + n_w2 + h2 + h2 + h2;
    std::vector<float> host(total);
    size_t o = 0;
    auto put = [&](const float* src, size_t cnt) { std::memcpy(host.data() + o, src, cnt * 4); o += cnt; return o - cnt; };
    const size_t o_w1 = put(desc->w1, n_w1), o_b1 = put(desc->b1, h1), o_a1 = put(desc->alpha1, h1);
    const size_t o_w2 = put(desc->w2, n_w2), o_b2 = put(desc->b2, h2), o_a2 = put(desc->alpha2, h2);
    const size_t o_w3 = put(desc->w3, h2);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->dev_weights), total * 4);
    if (e == hipSuccess) e = hipMemcpy(s->dev_weights, host.data(), total * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      nann_scorer_destroy(s);
      return fail(NANN_ERR_HIP, std::string("scorer weights: ") + hipGetErrorString(e));
    }
    const float* w = s->dev_weights;
    s->mlp.w1 = w + o_w1; s->mlp.b1 = w + o_b1; s->mlp.alpha1 = w + o_a1;
    s->mlp.w2 = w + o_w2; s->mlp.b2 = w + o_b2; s->mlp.alpha2 = w + o_a2; s->mlp.w3 = w + o_w3;
    s->mlp.d = d; s->mlp.h1 = 256; s->mlp.h2 = 128;
    if (desc->precision != NANN_MLP_PRECISION_DEFAULT && desc->precision != NANN_MLP_EXACT_F32 &&
        desc->precision != NANN_MLP_SPLIT_F16 && desc->precision != NANN_MLP_CERTIFIED) {
      nann_scorer_destroy(s);
      return fail(NANN_ERR_BAD_ARGUMENT, "MLP scorer: unknown precision");
    }
    if (desc->precision == NANN_MLP_CERTIFIED) {  // no precondition: rows the filter cannot bound are refined
      std::vector<float> c;
      certified_bound(desc->w2, desc->b2, desc->alpha2, desc->w3, 256, 128, &c, &s->mlp.k1s, &s->mlp.k0);
      e = hipMalloc(reinterpret_cast<void**>(&s->dev_cert), c.size() * 4);
      if (e == hipSuccess) e = hipMemcpy(s->dev_cert, c.data(), c.size() * 4, hipMemcpyHostToDevice);
      if (e != hipSuccess) {
        nann_scorer_destroy(s);
        return fail(NANN_ERR_HIP, std::string("scorer weights: ") + hipGetErrorString(e));
      }
      s->mlp.cb = s->dev_cert;
    } else if (desc->precision != NANN_MLP_EXACT_F32) {  // the pre-scaled weights must stay inside f16's range
      float wmax = 0.0f;
      for (size_t i2 = (size_t)d * h1; i2 < n_w1; ++i2) wmax = std::max(wmax, std::fabs(desc->w1[i2]));
      for (size_t i2 = 0; i2 < n_w2; ++i2) wmax = std::max(wmax, std::fabs(desc->w2[i2]));
      const bool fits = wmax <= 511.0f;
      if (!fits && desc->precision == NANN_MLP_SPLIT_F16) {
        nann_scorer_destroy(s);
        return fail(NANN_ERR_UNSUPPORTED, "MLP scorer: split-f16 precision needs |w| <= 511; use NANN_MLP_EXACT_F32");
      }
      s->desc.precision = fits ? NANN_MLP_SPLIT_F16 : NANN_MLP_EXACT_F32;  // DEFAULT resolved
    }
    {  // the split-f16 planes are small (256 KB): always built, used when precision says so
      std::vector<uint16_t> packed;
      size_t p2_off = 0;
      pack_split_weights(desc->w1, desc->w2, d, 256, 128, &packed, &p2_off);
      e = hipMalloc(reinterpret_cast<void**>(&s->dev_packed), packed.size() * 2);
      if (e == hipSuccess) e = hipMemcpy(s->dev_packed, packed.data(), packed.size() * 2, hipMemcpyHostToDevice);
      if (e != hipSuccess) {
        nann_scorer_destroy(s);
        return fail(NANN_ERR_HIP, std::string("scorer weights: ") + hipGetErrorString(e));
      }
      s->mlp.p1 = s->dev_packed;
      s->mlp.p2 = s->dev_packed + p2_off / 8;
    }
    {  // W2 as f32 A fragments of the exact form's resident layer 2 (nann_mlp5.h): p2x[t][mt][j][lane][i] =
       // W2[32 t + i + 8 j + 4 (lane >> 5)][32 mt + (lane & 31)] -- step r = 4 j + i of tile t in ORDER_H
      std::vector<float> px((size_t)256 * 128);
      for (int t = 0; t < 8; ++t)
        for (int mt = 0; mt < 4; ++mt)
          for (int j = 0; j < 4; ++j)
            for (int lane = 0; lane < 64; ++lane)
              for (int i = 0; i < 4; ++i)
                px[((((size_t)t * 4 + mt) * 4 + j) * 64 + lane) * 4 + i] =
                    desc->w2[(size_t)(32 * t + i + 8 * j + 4 * (lane >> 5)) * 128 + 32 * mt + (lane & 31)];
      e = hipMalloc(reinterpret_cast<void**>(&s->dev_packed_x), px.size() * 4);
      if (e == hipSuccess) e = hipMemcpy(s->dev_packed_x, px.data(), px.size() * 4, hipMemcpyHostToDevice);
      if (e != hipSuccess) {
        nann_scorer_destroy(s);
        return fail(NANN_ERR_HIP, std::string("scorer weights: ") + hipGetErrorString(e));
      }
      s->mlp.p2x = s->dev_packed_x;
    }
    // the host pointers of the descriptor are not kept
    s->desc.w1 = s->desc.b1 = s->desc.alpha1 = s->desc.w2 = s->desc.b2 = s->desc.alpha2 = s->desc.w3 = nullptr;
  }
  *out = s;
  return NANN_OK;
}

void nann_scorer_destroy(nann_scorer* s) {
  if (!s) return;
  if (s->dev_weights) (void)hipFree(s->dev_weights);
  if (s->dev_packed) (void)hipFree(s->dev_packed);
  if (s->dev_packed_x) (void)hipFree(s->dev_packed_x);
  if (s->dev_cert) (void)hipFree(s->dev_cert);
  delete s;
}

int nann_user_seq_mean(const void* comm_seq_f16, int64_t n_queries, int32_t seq_len, int32_t d,
                       float* q, nann_stream_t stream) {
  if (n_queries <= 0) return NANN_OK;
  if (seq_len <= 0 || d <= 0) return fail(NANN_ERR_BAD_ARGUMENT, "nann_user_seq_mean: bad shape");
  const long long bytes = (long long)seq_len * d * 2;
  if (d % 8 == 0 && bytes <= kSeqMeanMaxBytes && (reinterpret_cast<uintptr_t>(comm_seq_f16) & 15) == 0) {
    const size_t lds = (size_t)bytes + (size_t)seq_len * (d / 8);  // the history + one flag byte per 16-byte piece
    hipLaunchKernelGGL(k_user_seq_mean_lds, dim3((unsigned)n_queries), dim3(kSeqMeanThreads), lds, as_stream(stream),
                       static_cast<const uint4*>(comm_seq_f16), (int)seq_len, (int)d, q);
  } else {
    hipLaunchKernelGGL(k_user_seq_mean, dim3((unsigned)n_queries), dim3(std::min(256, (d + 63) / 64 * 64)),
                       0, as_stream(stream), static_cast<const uint16_t*>(comm_seq_f16), (int)seq_len,
                       (int)d, q);
  }
  HIP_TRY(hipGetLastError());
  return NANN_OK;
}

}  // extern "C"

template <int LPR>
static void launch_score_ip(int dt, unsigned blocks, hipStream_t st, const void* table, long long nt, int d,
                            const int32_t* idx, long long n, const float* q, float* out, OpResult* res) {
  if (dt == NANN_F16)
    hipLaunchKernelGGL((k_score_ip<LPR, DT_F16>), dim3(blocks), dim3(256), 0, st, table, nt, d, idx, n, q, out, res);
  else if (dt == NANN_BF16)
    hipLaunchKernelGGL((k_score_ip<LPR, DT_BF16>), dim3(blocks), dim3(256), 0, st, table, nt, d, idx, n, q, out, res);
  else
    hipLaunchKernelGGL((k_score_ip<LPR, DT_F32>), dim3(blocks), dim3(256), 0, st, table, nt, d, idx, n, q, out, res);
}

template <int LPR>
static void launch_score(int dt, unsigned blocks, hipStream_t st, const void* table, long long nt, int d,
                         const int32_t* idx, long long n, const float* q, float* out, OpResult* res) {
  if (dt == NANN_F16)
    hipLaunchKernelGGL((k_score_l2<LPR, DT_F16>), dim3(blocks), dim3(256), 0, st, table, nt, d, idx, n, q, out, res);
  else if (dt == NANN_BF16)
    hipLaunchKernelGGL((k_score_l2<LPR, DT_BF16>), dim3(blocks), dim3(256), 0, st, table, nt, d, idx, n, q, out, res);
  else
    hipLaunchKernelGGL((k_score_l2<LPR, DT_F32>), dim3(blocks), dim3(256), 0, st, table, nt, d, idx, n, q, out, res);
}

extern "C" {

int nann_score(const nann_scorer* scorer, const float* q, const void* table, int64_t n_table_rows,
               const int32_t* indices, int64_t n, float* out_scores, int64_t* bad_i,
               nann_stream_t stream) {
  if (!scorer) return fail(NANN_ERR_BAD_ARGUMENT, "nann_score: null scorer");
  if (bad_i) *bad_i = -1;
  if (n <= 0)  // blaze_xla_predictor.cc:259-263
    return fail(NANN_ERR_EMPTY_SCORE_BATCH, "Error when getting input address or size");
  ResultBuf* rb;
  int rc = get_result_buf(&rb);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_init_result, dim3(1), dim3(1), 0, st, rb->dev);
  const int d = scorer->desc.d, lpr = d / 8, dt = scorer->desc.emb_dtype;
  if (scorer->desc.kind == NANN_SCORER_MLP) {
    const unsigned blocks = (unsigned)std::min<long long>((n + 255) / 256, 512);  // (each takes a contiguous run of passes)
    const MlpParams& P = scorer->mlp;
    const int split = scorer->desc.precision == NANN_MLP_SPLIT_F16;
    if (d == 64) rc = launch_score_mlp_d64(dt, split, blocks, st, P, table, n_table_rows, indices, n, q, out_scores, rb->dev);
    else if (d == 128) rc = launch_score_mlp_d128(dt, split, blocks, st, P, table, n_table_rows, indices, n, q, out_scores, rb->dev);
    else rc = launch_score_mlp_d256(dt, split, blocks, st, P, table, n_table_rows, indices, n, q, out_scores, rb->dev);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    rc = fetch_result(rb, st);
    if (rc) return rc;
    if (rb->host->bad_i != 0x7fffffffffffffffll) {
      if (bad_i) *bad_i = rb->host->bad_i;
      return fail(NANN_ERR_INDEX_OUT_OF_RANGE, "indices[" + std::to_string(rb->host->bad_i) +
                                                   "] is not in [0, " + std::to_string(n_table_rows) + ")");
    }
    return NANN_OK;
  }
  const long long rows_per_block = 4 * (64 / lpr);
  const unsigned blocks = (unsigned)std::min<long long>((n + rows_per_block - 1) / rows_per_block, 8192);
  if (scorer->desc.kind == NANN_SCORER_IP) {
    switch (lpr) {
      case 8: launch_score_ip<8>(dt, blocks, st, table, n_table_rows, d, indices, n, q, out_scores, rb->dev); break;
      case 16: launch_score_ip<16>(dt, blocks, st, table, n_table_rows, d, indices, n, q, out_scores, rb->dev); break;
      case 32: launch_score_ip<32>(dt, blocks, st, table, n_table_rows, d, indices, n, q, out_scores, rb->dev); break;
      default: launch_score_ip<64>(dt, blocks, st, table, n_table_rows, d, indices, n, q, out_scores, rb->dev); break;
    }
  } else if (scorer->desc.kind == NANN_SCORER_L2) {
    switch (lpr) {
      case 8: launch_score<8>(dt, blocks, st, table, n_table_rows, d, indices, n, q, out_scores, rb->dev); break;
      case 16: launch_score<16>(dt, blocks, st, table, n_table_rows, d, indices, n, q, out_scores, rb->dev); break;
      case 32: launch_score<32>(dt, blocks, st, table, n_table_rows, d, indices, n, q, out_scores, rb->dev); break;
      default: launch_score<64>(dt, blocks, st, table, n_table_rows, d, indices, n, q, out_scores, rb->dev); break;
    }
  } else {
    return fail(NANN_ERR_BAD_ARGUMENT, "nann_score: unknown scorer kind");
  }
  HIP_TRY(hipGetLastError());
  rc = fetch_result(rb, st);
  if (rc) return rc;
  if (rb->host->bad_i != 0x7fffffffffffffffll) {
    if (bad_i) *bad_i = rb->host->bad_i;
    return fail(NANN_ERR_INDEX_OUT_OF_RANGE, "indices[" + std::to_string(rb->host->bad_i) +
                                                 "] is not in [0, " + std::to_string(n_table_rows) + ")");
  }
  return NANN_OK;
}

// ---- 8(f2): the reference scorer model -------------------------------------------------
}  // extern "C"

// A fragments of v_mfma_f32_32x32x16_f16 for W [K][n_out] (row-major), hi and lo planes of W * 2^7:
//   out[m][kc][plane][lane][i] = W[krow(kc, lane >> 5, i)][32 m + (lane & 31)]
// natural k order (the operand is a table row): krow = 16 kc + 8 g + i
// cd order (the operand is a finished 32-unit tile in C/D register order, two chunks per tile):
//   krow = 32 (kc >> 1) + (i & 3) + 16 (kc & 1) + 8 (i >> 2) + 4 g                      (nann_attn_split.h)
static bool pack_attn_frags(const float* W, int n_out, int n_chunks, bool cd_order, std::vector<uint16_t>* out) {
  const int M = n_out / 32;
  const size_t base0 = out->size();
  out->resize(base0 + (size_t)M * n_chunks * 2 * 64 * 8);
  bool ok = true;
  for (int m = 0; m < M; ++m)
    for (int kc = 0; kc < n_chunks; ++kc)
      for (int lane = 0; lane < 64; ++lane)
        for (int i = 0; i < 8; ++i) {
          const int g = lane >> 5;
          const int k = cd_order ? 32 * (kc >> 1) + (i & 3) + 16 * (kc & 1) + 8 * (i >> 2) + 4 * g : 16 * kc + 8 * g + i;
          const float v = W[(size_t)k * n_out + 32 * m + (lane & 31)];
          if (!(std::fabs(v) <= 511.0f)) ok = false;  // v * 2^7 must stay inside f16
          const size_t base = base0 + ((size_t)(m * n_chunks + kc) * 2) * 64 * 8;
          split_f16(v, &(*out)[base + (size_t)lane * 8 + i], &(*out)[base + 64 * 8 + (size_t)lane * 8 + i]);
        }
  return ok;
}

extern "C" {

int nann_attn_scorer_create(const nann_attn_desc* desc, nann_attn_scorer** out) {
  if (!desc || !out) return fail(NANN_ERR_BAD_ARGUMENT, "nann_attn_scorer_create: null argument");
  const int d = desc->d, L = desc->seq_len;
  if (d != 64 && d != 128) return fail(NANN_ERR_UNSUPPORTED, "attention scorer: d must be 64 or 128");
  if (L <= 0 || L > kAttnLP) return fail(NANN_ERR_UNSUPPORTED, "attention scorer: seq_len must be in [1, 64]");
  // (before any allocation; NANN_MLP_CERTIFIED is an MLP form: the attention model has no filter)
  if (desc->precision != NANN_MLP_PRECISION_DEFAULT && desc->precision != NANN_MLP_EXACT_F32 &&
      desc->precision != NANN_MLP_SPLIT_F16)
    return fail(NANN_ERR_BAD_ARGUMENT, desc->precision == NANN_MLP_CERTIFIED ? "attention scorer: the certified precision is an MLP form"
                                                                           : "attention scorer: unknown precision");
  if (desc->emb_dtype != NANN_F16 && desc->emb_dtype != NANN_BF16)
    return fail(NANN_ERR_UNSUPPORTED, "attention scorer: item rows must be f16 or bf16");
  const float* src[] = {desc->wq1, desc->bq1, desc->aq, desc->wq2, desc->bq2, desc->wk1, desc->bk1, desc->ak,
                        desc->wk2, desc->bk2,
                        desc->w[0], desc->b[0], desc->bn_scale[0], desc->bn_shift[0], desc->alpha[0],
                        desc->w[1], desc->b[1], desc->bn_scale[1], desc->bn_shift[1], desc->alpha[1],
                        desc->w[2], desc->b[2], desc->bn_scale[2], desc->bn_shift[2], desc->alpha[2],
                        desc->w[3]};
  const size_t cnt[] = {(size_t)d * 128, 128, 128, 128 * 256, 256, 64 * 128, 128, 128, 128 * 256, 256,
                        (size_t)(64 + d) * 128, 128, 128, 128, 128,
                        128 * 64, 64, 64, 64, 64,
                        64 * 32, 32, 32, 32, 32,
                        32};
  constexpr int NV = sizeof(cnt) / sizeof(cnt[0]);
  size_t off[NV], total = 0;
  for (int i = 0; i < NV; ++i) {
    if (!src[i]) return fail(NANN_ERR_BAD_ARGUMENT, "attention scorer: null weight pointer");
    off[i] = total;
    total += (cnt[i] + 3) & ~(size_t)3;  // keep every vector 16-byte aligned (float4 staging)
  }
  std::vector<float> host(total, 0.0f);
  for (int i = 0; i < NV; ++i) std::memcpy(host.data() + off[i], src[i], cnt[i] * 4);
  nann_attn_scorer* s = new nann_attn_scorer();
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->dev_weights), total * 4);
  if (e == hipSuccess) e = hipMemcpy(s->dev_weights, host.data(), total * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    nann_attn_scorer_destroy(s);
    return fail(NANN_ERR_HIP, std::string("attention scorer weights: ") + hipGetErrorString(e));
  }
  const float* w = s->dev_weights;
  AttnParams& P = s->P;
  const float** dst[] = {&P.wq1, &P.bq1, &P.aq, &P.wq2, &P.bq2, &P.wk1, &P.bk1, &P.ak, &P.wk2, &P.bk2,
                         &P.w1, &P.b1, &P.s1, &P.t1, &P.a1, &P.w2, &P.b2, &P.s2, &P.t2, &P.a2,
                         &P.w3, &P.b3, &P.s3, &P.t3, &P.a3, &P.w4};
  for (int i = 0; i < NV; ++i) *dst[i] = w + off[i];
  P.d = d;
  P.L = L;
  s->emb_dtype = desc->emb_dtype;
  s->precision = desc->precision;  // DEFAULT is resolved below, once the weights have been looked at
  {  // the split-f16 planes (~0.5 MB) are always built; `precision` picks the kernels
    std::vector<uint16_t> packed;
    bool ok = true;
    const size_t o_q1 = packed.size(); ok &= pack_attn_frags(desc->wq1, 128, d / 16, false, &packed);
    const size_t o_q2 = packed.size(); ok &= pack_attn_frags(desc->wq2, 256, 8, true, &packed);
    const size_t o_1a = packed.size(); ok &= pack_attn_frags(desc->w[0], 128, 4, true, &packed);                    // rows of a
    const size_t o_1e = packed.size(); ok &= pack_attn_frags(desc->w[0] + (size_t)64 * 128, 128, d / 16, false, &packed);  // rows of e
    const size_t o_2 = packed.size(); ok &= pack_attn_frags(desc->w[1], 64, 8, true, &packed);
    const size_t o_3 = packed.size(); ok &= pack_attn_frags(desc->w[2], 32, 4, true, &packed);
    const size_t o_v = (packed.size() + 7) & ~(size_t)7;  // halves; 16-byte aligned
    if (!ok && s->precision == NANN_MLP_SPLIT_F16) {
      nann_attn_scorer_destroy(s);
      return fail(NANN_ERR_UNSUPPORTED, "attention scorer, split-f16 form: |w| must be <= 511");
    }
    if (s->precision == NANN_MLP_PRECISION_DEFAULT) s->precision = ok ? NANN_MLP_SPLIT_F16 : NANN_MLP_EXACT_F32;
    std::vector<float> pv(PV_COUNT, 0.0f);
    const float WS = kAttnWS, HS = kAttnHS;
    for (int j = 0; j < 128; ++j) {
      pv[PV_BQ1 + j] = desc->bq1[j] * WS;
      pv[PV_AQ + j] = desc->aq[j] * (HS / WS);
      pv[PV_B1 + j] = desc->b[0][j] * (WS * HS);
      // bn + prelu of a hidden layer as w = fma(acc, S, T) (= 2^4 x the normalised value: power-of-two scales are exact)
      // and w + A min(w, 0): S = scale / 2^7, T = shift x 2^4, A = alpha - 1
      pv[PV_S1 + j] = desc->bn_scale[0][j] / WS;
      pv[PV_T1 + j] = desc->bn_shift[0][j] * HS;
      pv[PV_A1 + j] = desc->alpha[0][j] - 1.0f;
    }
    for (int j = 0; j < 256; ++j) pv[PV_BQ2 + j] = desc->bq2[j] * (WS * HS);
    for (int j = 0; j < 64; ++j) {
      pv[PV_B2 + j] = desc->b[1][j] * (WS * HS);
      pv[PV_S2 + j] = desc->bn_scale[1][j] / WS;
      pv[PV_T2 + j] = desc->bn_shift[1][j] * HS;
      pv[PV_A2 + j] = desc->alpha[1][j] - 1.0f;
    }
    for (int j = 0; j < 32; ++j) {
      pv[PV_B3 + j] = desc->b[2][j] * (WS * HS);
      pv[PV_S3 + j] = desc->bn_scale[2][j] / (WS * HS);
      pv[PV_T3 + j] = desc->bn_shift[2][j];
      pv[PV_A3 + j] = desc->alpha[2][j];
      pv[PV_W4 + j] = desc->w[3][j];
    }
    const size_t bytes = o_v * 2 + pv.size() * 4;
    e = hipMalloc(reinterpret_cast<void**>(&s->dev_packed), bytes);
    if (e == hipSuccess) e = hipMemcpy(s->dev_packed, packed.data(), packed.size() * 2, hipMemcpyHostToDevice);
    if (e == hipSuccess)
      e = hipMemcpy(reinterpret_cast<char*>(s->dev_packed) + o_v * 2, pv.data(), pv.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      nann_attn_scorer_destroy(s);
      return fail(NANN_ERR_HIP, std::string("attention scorer weights: ") + hipGetErrorString(e));
    }
    const uint4* base = s->dev_packed;
    P.pq1 = base + o_q1 / 8; P.pq2 = base + o_q2 / 8; P.pw1a = base + o_1a / 8; P.pw1e = base + o_1e / 8;
    P.pw2 = base + o_2 / 8; P.pw3 = base + o_3 / 8;
    P.pvec = reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + o_v * 2);
  }
  *out = s;
  return NANN_OK;
}

void nann_attn_scorer_destroy(nann_attn_scorer* s) {
  if (!s) return;
  if (s->dev_weights) (void)hipFree(s->dev_weights);
  if (s->dev_packed) (void)hipFree(s->dev_packed);
  delete s;
}

int nann_attn_prepare(const nann_attn_scorer* s, const void* user_seq_f16, int64_t n_users, float* kt,
                      float* upad, nann_stream_t stream) {
  if (!s || !user_seq_f16 || !kt || !upad) return fail(NANN_ERR_BAD_ARGUMENT, "nann_attn_prepare: null argument");
  if (n_users <= 0) return NANN_OK;
  if (s->precision == NANN_MLP_SPLIT_F16)
    return launch_attn_prepare_split(as_stream(stream), s->P, user_seq_f16, n_users, kt, upad);
  return launch_attn_prepare(as_stream(stream), s->P, user_seq_f16, n_users, kt, upad);
}

int nann_attn_score(const nann_attn_scorer* s, const float* kt, const float* upad, const void* table,
                    int64_t n_table_rows, const int32_t* indices, int64_t n, float* out_scores,
                    int64_t* bad_i, nann_stream_t stream) {
  if (!s || !kt || !upad || !table) return fail(NANN_ERR_BAD_ARGUMENT, "nann_attn_score: null argument");
  if (bad_i) *bad_i = -1;
  if (n <= 0)  // blaze_xla_predictor.cc:259-263
    return fail(NANN_ERR_EMPTY_SCORE_BATCH, "Error when getting input address or size");
  ResultBuf* rb;
  int rc = get_result_buf(&rb);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_init_result, dim3(1), dim3(1), 0, st, rb->dev);
  const unsigned blocks = (unsigned)std::min<long long>((n + 255) / 256, 2048);
  if (s->precision == NANN_MLP_SPLIT_F16)
    rc = launch_score_attn_split(s->emb_dtype, std::min(blocks, 512u), st, s->P, kt, upad, table, n_table_rows, indices, n,
                                 out_scores, &rb->dev->bad_i);
  else
    rc = launch_score_attn(s->emb_dtype, blocks, st, s->P, kt, upad, table, n_table_rows, indices, n, out_scores,
                           &rb->dev->bad_i);
  if (rc) return rc;
  rc = fetch_result(rb, st);
  if (rc) return rc;
  if (rb->host->bad_i != 0x7fffffffffffffffll) {
    if (bad_i) *bad_i = rb->host->bad_i;
    return fail(NANN_ERR_INDEX_OUT_OF_RANGE, "indices[" + std::to_string(rb->host->bad_i) +
                                                 "] is not in [0, " + std::to_string(n_table_rows) + ")");
  }
  return NANN_OK;
}

// ---- a4: the scoring model behind BlazeXlaOp, loaded from a weights directory ------------
struct nann_model {
  int kind = NANN_MODEL_L2;
  int d = 0, seq_len = 0, emb_dtype = NANN_F16;
  nann_scorer* scorer = nullptr;
  nann_attn_scorer* attn = nullptr;
};

static int load_f32(const std::string& dir, const char* name, std::vector<std::vector<char>>* keep,
                    const float** out, int64_t expect_count) {
  keep->emplace_back();
  std::vector<int64_t> shape;
  const int rc = read_npy_host((dir + "/" + name + ".npy").c_str(), NANN_F32, nullptr, 0, /*allow_cast=*/1,
                               &keep->back(), &shape);
  if (rc) return rc;
  int64_t count = 1;
  for (int64_t v : shape) count *= v;
  if (expect_count >= 0 && count != expect_count)
    return fail(NANN_ERR_SHAPE_MISMATCH, std::string(name) + ".npy: " + std::to_string(count) + " values, expected " +
                                             std::to_string(expect_count));
  *out = reinterpret_cast<const float*>(keep->back().data());
  return NANN_OK;
}

}  // extern "C"

// optional precision.txt of a weights directory: "split" (split-f16 operands, the default) | "exact" (f32-input MFMA)
static int read_precision(const std::string& dir, int32_t* precision) {
  std::ifstream pf(dir + "/precision.txt");
  std::string prec;
  if (!pf || !(pf >> prec)) return NANN_OK;
  if (prec == "split") *precision = NANN_MLP_SPLIT_F16;
  else if (prec == "exact") *precision = NANN_MLP_EXACT_F32;
  else if (prec == "certified") *precision = NANN_MLP_CERTIFIED;
  else return fail(NANN_ERR_BAD_ARGUMENT, "precision.txt: expected exact, split or certified, got '" + prec + "'");
  return NANN_OK;
}

extern "C" {

// BlazeXlaOp.graph_def as the reference writes it: a frozen GraphDef file (convert_meta.py:361-398).  The weights of
// Model.forward (model.py:189-233) are pulled out of it by host/nann_graphdef.h; nothing of the graph is executed.
static int model_from_graphdef(const std::string& path, int32_t d, int32_t emb_dtype, int32_t seq_len, nann_model* m) {
  std::ifstream f(path, std::ifstream::binary);
  if (!f) return fail(NANN_ERR_IO, "Fail to open file: " + path);
  const std::string bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  nann_gd::Graph g;
  std::string msg;
  // text first, then binary: the reference's order (blaze_xla_kernel.cc:169-175)
  if (!nann_gd::parse_graph_any(reinterpret_cast<const uint8_t*>(bytes.data()), bytes.size(), &g, &msg))
    return fail(NANN_ERR_IO, "parse proto from " + path + " failed: " + msg);  // blaze_xla_kernel.cc:169-175
  nann_gd::AttnWeights w;
  if (!nann_gd::extract_attention(g, &w, &msg))
    return fail(NANN_ERR_UNSUPPORTED, path + ": not the reference's scorer model (model.py:189-233): " + msg);
  if (w.d != d) return fail(NANN_ERR_SHAPE_MISMATCH, path + ": the model scores " + std::to_string(w.d) + "-d item rows, the request has " + std::to_string(d));
  if (w.e != kAttnE) return fail(NANN_ERR_UNSUPPORTED, path + ": user sequence embedding dim " + std::to_string(w.e) + ", this build has 64");
  const size_t hq = 2 * (size_t)kAttnE, hq2 = 4 * (size_t)kAttnE;
  const size_t expect[] = {(size_t)d * hq, hq, hq, hq * hq2, hq2, (size_t)kAttnE * hq, hq, hq, hq * hq2, hq2};
  const std::vector<float>* att[] = {&w.wq1, &w.bq1, &w.aq, &w.wq2, &w.bq2, &w.wk1, &w.bk1, &w.ak, &w.wk2, &w.bk2};
  for (int i = 0; i < 10; ++i)
    if (att[i]->size() != expect[i]) return fail(NANN_ERR_SHAPE_MISMATCH, path + ": attention tensor " + std::to_string(i) + " has an unexpected size");
  const size_t widths[4] = {128, 64, 32, 1};
  size_t n_in = (size_t)kAttnE + (size_t)d;
  for (int l = 0; l < 4; ++l) {
    if (w.w[l].size() != n_in * widths[l]) return fail(NANN_ERR_SHAPE_MISMATCH, path + ": DNN layer " + std::to_string(l + 1) + " is not the 128-64-32-1 tower this build has");
    n_in = widths[l];
  }
  nann_attn_desc ad = {};
  ad.d = d; ad.emb_dtype = emb_dtype; ad.seq_len = seq_len;
  ad.wq1 = w.wq1.data(); ad.bq1 = w.bq1.data(); ad.aq = w.aq.data(); ad.wq2 = w.wq2.data(); ad.bq2 = w.bq2.data();
  ad.wk1 = w.wk1.data(); ad.bk1 = w.bk1.data(); ad.ak = w.ak.data(); ad.wk2 = w.wk2.data(); ad.bk2 = w.bk2.data();
  for (int l = 0; l < 4; ++l) ad.w[l] = w.w[l].data();
  for (int l = 0; l < 3; ++l) {
    ad.b[l] = w.b[l].data(); ad.bn_scale[l] = w.bn_scale[l].data(); ad.bn_shift[l] = w.bn_shift[l].data();
    ad.alpha[l] = w.alpha[l].data();
  }
  ad.precision = NANN_MLP_PRECISION_DEFAULT;
  {  // an optional <file>.precision beside the graph: "split" | "exact" (as precision.txt of the directory form)
    std::ifstream pf(path + ".precision");
    std::string prec;
    if (pf && (pf >> prec)) {
      if (prec == "split") ad.precision = NANN_MLP_SPLIT_F16;
      else if (prec == "exact") ad.precision = NANN_MLP_EXACT_F32;
      else if (prec == "certified") ad.precision = NANN_MLP_CERTIFIED;
      else return fail(NANN_ERR_BAD_ARGUMENT, path + ".precision: expected exact, split or certified, got '" + prec + "'");
    }
  }
  m->kind = NANN_MODEL_ATTENTION;
  return nann_attn_scorer_create(&ad, &m->attn);
}

int nann_model_load(const char* dir, int32_t d, int32_t emb_dtype, int32_t seq_len, nann_model** out) {
  if (!dir || !out) return fail(NANN_ERR_BAD_ARGUMENT, "nann_model_load: null argument");
  const std::string D(dir);
  nann_model* m = new nann_model();
  m->d = d; m->seq_len = seq_len; m->emb_dtype = emb_dtype;
  struct stat sb;
  if (::stat(dir, &sb) == 0 && S_ISREG(sb.st_mode)) {  // a frozen GraphDef file: what the reference's attr names
    const int rc = model_from_graphdef(D, d, emb_dtype, seq_len, m);
    if (rc) { nann_model_destroy(m); return rc; }
    *out = m;
    return NANN_OK;
  }
  std::ifstream kf(D + "/scorer.txt");
  if (!kf) { nann_model_destroy(m); return fail(NANN_ERR_IO, "Fail to open file: " + D + "/scorer.txt"); }
  std::string kind;
  kf >> kind;
  std::vector<std::vector<char>> keep;
  int rc = NANN_OK;
  if (kind == "l2" || kind == "mlp" || kind == "ip") {
    nann_scorer_desc sd = {};
    sd.kind = kind == "l2" ? NANN_SCORER_L2 : kind == "ip" ? NANN_SCORER_IP : NANN_SCORER_MLP;
    sd.d = d; sd.emb_dtype = emb_dtype;
    m->kind = kind == "l2" ? NANN_MODEL_L2 : kind == "ip" ? NANN_MODEL_IP : NANN_MODEL_MLP;
    if (kind == "mlp") {
      sd.h1 = 256; sd.h2 = 128;
      const struct { const char* n; const float** p; int64_t cnt; } w[] = {
          {"w1", &sd.w1, 2ll * d * 256}, {"b1", &sd.b1, 256}, {"alpha1", &sd.alpha1, 256}, {"w2", &sd.w2, 256 * 128},
          {"b2", &sd.b2, 128}, {"alpha2", &sd.alpha2, 128}, {"w3", &sd.w3, 128}};
      for (const auto& e : w)
        if (!rc) rc = load_f32(D, e.n, &keep, e.p, e.cnt);
      if (!rc) rc = read_precision(D, &sd.precision);
    }
    if (!rc) rc = nann_scorer_create(&sd, &m->scorer);
  } else if (kind == "attention") {
    nann_attn_desc ad = {};
    ad.d = d; ad.emb_dtype = emb_dtype; ad.seq_len = seq_len;
    m->kind = NANN_MODEL_ATTENTION;
    // every tensor with the element count nann_attn_scorer_create indexes it by: a directory exported for another d,
    // or a truncated file, is refused instead of read out of bounds
    const int64_t E = kAttnE, hq = 2 * E, hq2 = 4 * E;
    const struct { const char* n; const float** p; int64_t cnt; } w[] = {
        {"wq1", &ad.wq1, (int64_t)d * hq}, {"bq1", &ad.bq1, hq}, {"aq", &ad.aq, hq}, {"wq2", &ad.wq2, hq * hq2}, {"bq2", &ad.bq2, hq2},
        {"wk1", &ad.wk1, E * hq}, {"bk1", &ad.bk1, hq}, {"ak", &ad.ak, hq}, {"wk2", &ad.wk2, hq * hq2}, {"bk2", &ad.bk2, hq2},
        {"w0", &ad.w[0], (E + d) * 128}, {"w1", &ad.w[1], 128 * 64}, {"w2", &ad.w[2], 64 * 32}, {"w3", &ad.w[3], 32},
        {"b0", &ad.b[0], 128}, {"b1", &ad.b[1], 64}, {"b2", &ad.b[2], 32},
        {"bn_scale0", &ad.bn_scale[0], 128}, {"bn_scale1", &ad.bn_scale[1], 64}, {"bn_scale2", &ad.bn_scale[2], 32},
        {"bn_shift0", &ad.bn_shift[0], 128}, {"bn_shift1", &ad.bn_shift[1], 64}, {"bn_shift2", &ad.bn_shift[2], 32},
        {"alpha0", &ad.alpha[0], 128}, {"alpha1", &ad.alpha[1], 64}, {"alpha2", &ad.alpha[2], 32}};
    for (const auto& e : w)
      if (!rc) rc = load_f32(D, e.n, &keep, e.p, e.cnt);
    if (!rc) rc = read_precision(D, &ad.precision);
    if (!rc) rc = nann_attn_scorer_create(&ad, &m->attn);
  } else {
    rc = fail(NANN_ERR_UNSUPPORTED, "scorer.txt: expected l2, ip, mlp or attention, got '" + kind + "'");
  }
  if (rc) { nann_model_destroy(m); return rc; }
  *out = m;
  return NANN_OK;
}

// BlazeXlaOp.blaze_option_path as BlazeXlaOp::ParseAttr reads it (blaze_xla_kernel.cc:156-167): a text-format
// BlazeKernelOptions file, else the attr string itself as text format (host/nann_blaze_options.h).
int nann_blaze_options_parse(const char* attr, nann_blaze_options* out) {
  if (!attr || !out) return fail(NANN_ERR_BAD_ARGUMENT, "nann_blaze_options_parse: null argument");
  nann_gd::BlazeOptions o;
  std::string msg;
  if (!nann_gd::parse_blaze_options_attr(attr, &o, &msg)) return fail(NANN_ERR_IO, msg);
  nann_blaze_options r = {};
  r.struct_bytes = (int32_t)sizeof(nann_blaze_options);
  r.wait_ms = o.wait_ms; r.run_mode = o.run_mode; r.xla_compilation = o.xla_compilation;
  r.auto_mixed_precision = o.auto_mixed_precision; r.disable_output_padding = o.disable_output_padding;
  r.n_warmup_batchsize = o.n_warmup_batchsize; r.max_warmup_batchsize = o.max_warmup_batchsize; r.from_file = o.from_file;
  *out = r;
  return NANN_OK;
}

void nann_model_destroy(nann_model* m) {
  if (!m) return;
  if (m->scorer) nann_scorer_destroy(m->scorer);
  if (m->attn) nann_attn_scorer_destroy(m->attn);
  delete m;
}

int nann_model_kind(const nann_model* m) { return m ? m->kind : -1; }
const nann_scorer* nann_model_scorer(const nann_model* m) { return m ? m->scorer : nullptr; }

int nann_model_workspace_bytes(const nann_model* m, int64_t* nbytes) {
  if (!m || !nbytes) return fail(NANN_ERR_BAD_ARGUMENT, "nann_model_workspace_bytes: null argument");
  *nbytes = m->kind == NANN_MODEL_ATTENTION ? (int64_t)(256 * 64 + 64 * 64) * 4 : (int64_t)kMaxD * 4;
  return NANN_OK;
}

int nann_model_forward(const nann_model* m, const void* user_seq_f16, const void* item_emb, int64_t n,
                       float* logits, void* workspace, nann_stream_t stream) {
  if (!m || !user_seq_f16 || !logits || !workspace) return fail(NANN_ERR_BAD_ARGUMENT, "nann_model_forward: null argument");
  if (n <= 0)  // blaze_xla_predictor.cc:259-263
    return fail(NANN_ERR_EMPTY_SCORE_BATCH, "Error when getting input address or size");
  if (m->kind == NANN_MODEL_ATTENTION) {
    float* kt = static_cast<float*>(workspace);
    float* upad = kt + 256 * 64;
    const int rc = nann_attn_prepare(m->attn, user_seq_f16, 1, kt, upad, stream);
    if (rc) return rc;
    return nann_attn_score(m->attn, kt, upad, item_emb, n, nullptr, n, logits, nullptr, stream);
  }
  float* q = static_cast<float*>(workspace);
  const int rc = nann_user_seq_mean(user_seq_f16, 1, m->seq_len, m->d, q, stream);
  if (rc) return rc;
  return nann_score(m->scorer, q, item_emb, n, nullptr, n, logits, nullptr, stream);
}

// ---- index ---------------------------------------------------------------------------
static int64_t dtype_bytes(int dt) { return dt == NANN_F32 ? 4 : 2; }

int nann_index_create(const nann_index_desc* desc, nann_index** out) {
  if (!desc || !out) return fail(NANN_ERR_BAD_ARGUMENT, "nann_index_create: null argument");
  const nann_index_desc& h = *desc;
  if (h.n_items <= 0 || h.n_items > 0x7fffffffll) return fail(NANN_ERR_BAD_ARGUMENT, "n_items out of range");
  if (!(h.d == 64 || h.d == 128 || h.d == 256 || h.d == 512))
    return fail(NANN_ERR_UNSUPPORTED, "embedding dim must be 64, 128, 256 or 512");
  if (h.n_enter < 0 || h.n_enter > 0x7fffffffll) return fail(NANN_ERR_BAD_ARGUMENT, "n_enter out of range");
  for (int l = 0; l < 2; ++l)
    if (h.nb_nnz[l] < 0 || h.nb_nnz[l] > 0xffffffffll)
      return fail(NANN_ERR_UNSUPPORTED, "a level holds more than 2^32-1 links");
  nann_index* ix = new nann_index();
  ix->desc = h;
  {
    static std::atomic<uint64_t> next_uid{1};
    ix->uid = next_uid.fetch_add(1);
  }
  const int64_t N = h.n_items;
  // host copies of the small arrays for validation
  std::vector<int64_t> rs_host[2];
  std::vector<int32_t> ep_host((size_t)h.n_enter);
  auto fetch = [&](void* dst, const void* src, size_t bytes) -> int {
    if (!bytes) return NANN_OK;
    if (h.on_device) { HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); }
    else std::memcpy(dst, src, bytes);
    return NANN_OK;
  };
  int rc = NANN_OK;
  for (int l = 0; l < 2 && !rc; ++l) {
    rs_host[l].resize((size_t)N + 1);
    rc = fetch(rs_host[l].data(), h.nb_row_splits[l], (size_t)(N + 1) * 8);
  }
  if (!rc) rc = fetch(ep_host.data(), h.enter_points, (size_t)h.n_enter * 4);
  if (rc) { delete ix; return rc; }
  for (int l = 0; l < 2; ++l) {
    const auto& rs = rs_host[l];
    if (rs[0] != 0 || rs[(size_t)N] != h.nb_nnz[l]) {
      delete ix;
      return fail(NANN_ERR_INVALID_RAGGED_PARAMS, "level " + std::to_string(l) + " row_splits do not span its values");
    }
    int64_t md = 0;
    for (int64_t i = 0; i < N; ++i) {
      const int64_t len = rs[(size_t)i + 1] - rs[(size_t)i];
      if (len < 0) { delete ix; return fail(NANN_ERR_INVALID_RAGGED_PARAMS, "row_splits not monotone"); }
      md = std::max(md, len);
    }
    ix->max_deg[l] = md;
  }
  for (int64_t i = 0; i < h.n_enter; ++i) {
    if (ep_host[(size_t)i] < 0 || ep_host[(size_t)i] >= N) { delete ix; return fail(NANN_ERR_INDEX_OUT_OF_RANGE, "enter point out of range"); }
    if (i && ep_host[(size_t)i] <= ep_host[(size_t)i - 1]) { delete ix; return fail(NANN_ERR_BAD_ARGUMENT, "enter points must be ascending and unique"); }
  }
  ix->bm_words = (uint32_t)(((N + 31) / 32 + 3) / 4 * 4);
  if (!h.on_device) {  // one-time H2D, what HugeConst's GPU kernel does (huge_const_op.cc:187-218)
    auto up = [&](const void* src, size_t bytes, const void** dst) -> int {
      void* d = nullptr;
      HIP_TRY(hipMalloc(&d, std::max<size_t>(bytes, 16)));
      ix->owned.push_back(d);
      if (bytes) HIP_TRY(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
      *dst = d;
      return NANN_OK;
    };
    nann_index_desc& dd = ix->desc;
    rc = up(h.item_embs, (size_t)N * h.d * dtype_bytes(h.emb_dtype), &dd.item_embs);
    if (!rc) rc = up(h.item_ids, (size_t)N * 8, reinterpret_cast<const void**>(&dd.item_ids));
    for (int l = 0; l < 2 && !rc; ++l) {
      rc = up(h.nb_values[l], (size_t)h.nb_nnz[l] * 4, reinterpret_cast<const void**>(&dd.nb_values[l]));
      if (!rc) rc = up(h.nb_row_splits[l], (size_t)(N + 1) * 8, reinterpret_cast<const void**>(&dd.nb_row_splits[l]));
    }
    if (!rc) rc = up(h.enter_points, (size_t)h.n_enter * 4, reinterpret_cast<const void**>(&dd.enter_points));
    if (rc) { nann_index_destroy(ix); return rc; }
    ix->owns = true;
    dd.on_device = 1;
  }
  choose_pivots(ix, ep_host);  // the batch order's pivots (never fails the creation: without them, input order)
  probe_index(ix);  // what a beam visits on this graph: 64 queries, one small launch (never fails the creation)
  *out = ix;
  return NANN_OK;
}

void nann_index_destroy(nann_index* ix) {
  if (!ix) return;
  ProjCache::drop_index(ix->uid);  // the scorers' pre-projected tables of this index go with it (retired, then freed)
  for (void* p : ix->owned) (void)hipFree(p);
  if (ix->pivots) (void)hipFree(ix->pivots);
  delete ix;
}

int nann_index_probe_info(const nann_index* ix, float out[5]) {
  if (!ix || !out) return fail(NANN_ERR_BAD_ARGUMENT, "nann_index_probe_info: null argument");
  out[0] = ix->probe_valid ? (float)ix->probe_queries : 0.0f;
  out[1] = (float)ix->probe_ef;
  out[2] = ix->probe_new_per_row_mean;
  out[3] = ix->probe_new_per_row_q90;
  out[4] = ix->probe_new_per_row_max;
  return NANN_OK;
}

int nann_index_info(const nann_index* ix, int64_t out[6]) {
  if (!ix || !out) return fail(NANN_ERR_BAD_ARGUMENT, "nann_index_info: null argument");
  out[0] = ix->desc.n_items; out[1] = ix->desc.d; out[2] = ix->desc.n_enter;
  out[3] = ix->max_deg[0]; out[4] = ix->max_deg[1]; out[5] = ix->bm_words;
  return NANN_OK;
}

// The three setters are PROCESS DEFAULTS of the fields of nann_search_options that a call leaves at -1 (round 5: the knobs
// themselves travel with the call -- nann_search_opt --, so two threads sharing a handle no longer share a plan).
int nann_set_search_reserve(int32_t workgroups) {
  if (workgroups < 0) return fail(NANN_ERR_BAD_ARGUMENT, "nann_set_search_reserve: negative");
  g_slot_reserve.store(workgroups, std::memory_order_relaxed);
  return NANN_OK;
}

void nann_search_options_init(nann_search_options* o) {
  if (!o) return;
  o->struct_bytes = (int32_t)sizeof(*o);
  o->traversal_mode = o->slot_reserve = o->preprojection = o->mlp_form = -1;
}

int nann_set_traversal_mode(int32_t mode) {
  if (mode < NANN_TRAVERSAL_AUTO || mode > NANN_TRAVERSAL_LDS_HASH32)
    return fail(NANN_ERR_BAD_ARGUMENT, "nann_set_traversal_mode: unknown mode");
  g_traversal_mode.store(mode, std::memory_order_relaxed);
  return NANN_OK;
}

}  // extern "C"


// The pre-projected table of (scorer, index): found, or built on `st` by `build(table)` (a one-time wait per pair,
// ~10-20 ms per million items: nann_*_prepare moves it ahead of traffic).  *out stays null -- with NANN_OK -- when there
// is to be no table: pre-projection switched off, or no room for it in HBM (the caller then runs the kernels that
// read the embedding rows; ADVICE r3: a failed hipMalloc must not fail the search).  pin: count a prepare call.
template <typename Build>
static int projection_for(ProjCache& c, const nann_index* ix, int width, hipStream_t st, Build build, bool pin, bool enabled,
                          std::shared_ptr<ProjTable>* out) {
  const size_t bytes = (size_t)ix->desc.n_items * (size_t)width * 4;
  return c.acquire(ix->uid, bytes, enabled, pin, [&](float* t) -> int {
    const int rc = build(t);
    if (rc) return rc;
    // the table becomes visible to searches on OTHER streams when acquire() returns: it must be complete by then
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(NANN_ERR_HIP, std::string("pre-projection: ") + hipGetErrorString(e));
    return NANN_OK;
  }, out);
}

static void projection_used(ProjCache& c, const std::shared_ptr<ProjTable>& tab, hipStream_t st) { c.used(tab, st); }

static int projection_release(ProjCache& c, const nann_index* ix) {
  if (c.release(ix->uid)) return NANN_OK;
  return fail(NANN_ERR_BAD_ARGUMENT, "release: no pre-projected table of this index");
}

static int mlp_projection(const nann_scorer* sc, const nann_index* ix, hipStream_t st, bool pin, bool enabled, std::shared_ptr<ProjTable>* out) {
  return projection_for(sc->proj, ix, kMlpProjWidth, st, [&](float* t) {
    return launch_mlp_preproject(ix->desc.emb_dtype, ix->desc.item_embs, (long long)ix->desc.n_items, ix->desc.d, sc->mlp.w1, t, st);
  }, pin, enabled, out);
}

static int attn_projection(const nann_attn_scorer* sc, const nann_index* ix, hipStream_t st, bool pin, bool enabled, std::shared_ptr<ProjTable>* out) {
  return projection_for(sc->proj, ix, kAttnProjWidth, st, [&](float* t) {
    return launch_attn_preproject(ix->desc.emb_dtype, sc->P, ix->desc.item_embs, (long long)ix->desc.n_items, t, st);
  }, pin, enabled, out);
}

// ---- who scores a call ---------------------------------------------------------------------------------------------------
// A nann_scorer or a nann_model as the host paths dispatch on it: the calls below, nann_traverse.hip, nann_flat.hip (FlatBy)
struct ScoredBy {
  const nann_scorer* scorer = nullptr;   // l2 / ip / mlp: the scorer, a model's own included
  const nann_attn_scorer* at = nullptr;  // the attention model
  const nann_model* mean_of = nullptr;   // an l2 / ip / mlp model: the query is the mean of its sequence
  ProjCache* cache = nullptr;            // MLP / attention: the cache the pair's pre-projected table belongs to,
  int width = 0;                         //   and the table's floats per row (0: the scorer reads the index's rows)
  const char* what = "scorer";           // the handle's word in a message
  bool mismatch = false;                 // handle and index disagree on d / dtype (ix may be null: no index to disagree with)
};
static ScoredBy scored_by(const nann_index* ix, const nann_scorer* scorer, const nann_model* m) {
  ScoredBy by;
  int d = 0, dt = 0;
  if (m) {
    by.what = "model";
    d = m->d; dt = m->emb_dtype;
    if (m->kind == NANN_MODEL_ATTENTION) {
      by.at = m->attn;
      by.cache = &m->attn->proj; by.width = kAttnProjWidth;
      scorer = nullptr;
    } else {
      by.mean_of = m;
      scorer = m->scorer;
    }
  } else if (scorer) {
    d = scorer->desc.d; dt = scorer->desc.emb_dtype;
  }
  by.scorer = scorer;
  if (scorer && scorer->desc.kind == NANN_SCORER_MLP) { by.cache = &scorer->proj; by.width = kMlpProjWidth; }
  by.mismatch = ix && (d != ix->desc.d || dt != ix->desc.emb_dtype);
  return by;
}

extern "C" {

// ---- lifecycle of the pre-projected tables (ProjCache) -------------------------------------------------------
int nann_set_preprojection(int32_t enabled) {
  g_preproject.store(enabled ? 1 : 0, std::memory_order_relaxed);
  return NANN_OK;
}
static int prepare_impl(const ScoredBy& by, const nann_index* ix, hipStream_t st) {
  if (!by.cache) return NANN_OK;  // L2, inner product: nothing to pre-project
  if (by.mismatch) return fail(NANN_ERR_BAD_ARGUMENT, "scorer and index disagree on d / dtype");  // ("scorer" under a model too: the message is pinned as it was)
  std::shared_ptr<ProjTable> tab;
  const bool enabled = resolve_options(nullptr).preproject != 0;
  const int rc = by.at ? attn_projection(by.at, ix, st, true, enabled, &tab) : mlp_projection(by.scorer, ix, st, true, enabled, &tab);
  if (rc) return rc;
  if (!tab) return fail(NANN_ERR_CAPACITY, "no room in HBM for the pre-projected table (or pre-projection is switched off): "
                                           "searches of this pair will read the embedding table");
  return NANN_OK;
}
static int release_impl(const ScoredBy& by, const nann_index* ix) { return by.cache ? projection_release(*by.cache, ix) : NANN_OK; }
static int table_bytes_impl(const ScoredBy& by, const nann_index* ix, int64_t* table_bytes, int64_t* resident_bytes) {
  if (table_bytes) *table_bytes = ix ? (int64_t)ix->desc.n_items * by.width * 4 : 0;
  if (resident_bytes) *resident_bytes = by.cache ? (int64_t)by.cache->resident() : 0;
  return NANN_OK;
}

int nann_scorer_prepare(const nann_scorer* scorer, const nann_index* ix, nann_stream_t stream) {
  if (!scorer || !ix) return fail(NANN_ERR_BAD_ARGUMENT, "nann_scorer_prepare: null argument");
  return prepare_impl(scored_by(ix, scorer, nullptr), ix, as_stream(stream));
}
int nann_scorer_release(const nann_scorer* scorer, const nann_index* ix) {
  if (!scorer || !ix) return fail(NANN_ERR_BAD_ARGUMENT, "nann_scorer_release: null argument");
  return release_impl(scored_by(ix, scorer, nullptr), ix);
}
int nann_scorer_table_bytes(const nann_scorer* scorer, const nann_index* ix, int64_t* table_bytes, int64_t* resident_bytes) {
  if (!scorer) return fail(NANN_ERR_BAD_ARGUMENT, "nann_scorer_table_bytes: null scorer");
  return table_bytes_impl(scored_by(ix, scorer, nullptr), ix, table_bytes, resident_bytes);
}
int nann_model_prepare(const nann_model* m, const nann_index* ix, nann_stream_t stream) {
  if (!m || !ix) return fail(NANN_ERR_BAD_ARGUMENT, "nann_model_prepare: null argument");
  return prepare_impl(scored_by(ix, nullptr, m), ix, as_stream(stream));
}
int nann_model_release(const nann_model* m, const nann_index* ix) {
  if (!m || !ix) return fail(NANN_ERR_BAD_ARGUMENT, "nann_model_release: null argument");
  return release_impl(scored_by(ix, nullptr, m), ix);
}
int nann_model_table_bytes(const nann_model* m, const nann_index* ix, int64_t* table_bytes, int64_t* resident_bytes) {
  if (!m) return fail(NANN_ERR_BAD_ARGUMENT, "nann_model_table_bytes: null model");
  return table_bytes_impl(scored_by(ix, nullptr, m), ix, table_bytes, resident_bytes);
}

// ---- merge ------------------------------------------------------------------------------
int nann_merge_topk(const float* scores, const int64_t* ids, int64_t n_queries, int32_t n_shards,
                    int32_t k_in, int32_t k_out, float* out_scores, int64_t* out_ids,
                    nann_stream_t stream) {
  const int64_t n_in = (int64_t)n_shards * k_in;
  if (k_out < 0 || k_out > kMaxK) return fail(NANN_ERR_UNSUPPORTED, "k_out must be in [0, 1024]");
  if (n_in < k_out) return fail(NANN_ERR_TOPK_K_GT_N, "fewer candidates than k_out");
  if (n_queries <= 0 || k_out == 0) return NANN_OK;
  hipLaunchKernelGGL(k_merge_topk, dim3((unsigned)n_queries), dim3(kNT), 0, as_stream(stream), scores,
                     ids, (int)n_in, (int)k_out, out_scores, out_ids);
  HIP_TRY(hipGetLastError());
  return NANN_OK;
}

int nann_merge_topk_host(const float* scores, const int64_t* ids, int64_t n_queries, int32_t n_shards,
                         int32_t k_in, int32_t k_out, float* out_scores, int64_t* out_ids) {
  const int64_t n_in = (int64_t)n_shards * k_in;
  if (k_out < 0) return fail(NANN_ERR_BAD_ARGUMENT, "k_out < 0");
  if (n_in < k_out) return fail(NANN_ERR_TOPK_K_GT_N, "fewer candidates than k_out");
  std::vector<int32_t> idx((size_t)n_in);
  for (int64_t qi = 0; qi < n_queries; ++qi) {
    const float* s = scores + qi * n_in;
    for (int64_t i = 0; i < n_in; ++i) idx[(size_t)i] = (int32_t)i;
    std::partial_sort(idx.begin(), idx.begin() + k_out, idx.end(), [s](int32_t x, int32_t y) {
      if (s[y] < s[x]) return true;   // value descending
      if (s[y] > s[x]) return false;
      return x < y;                   // ties -> lower position (shard-major)
    });
    for (int32_t i = 0; i < k_out; ++i) {
      out_scores[qi * k_out + i] = s[idx[(size_t)i]];
      out_ids[qi * k_out + i] = ids[qi * n_in + idx[(size_t)i]];
    }
  }
  return NANN_OK;
}

}  // extern "C"
