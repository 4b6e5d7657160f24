// nann_scorers.hip -- the stand-alone scorers behind BlazeXlaOp, kernels and entry points: the L2 / inner-product / MLP scorer
// (nann_scorer_create, nann_score) with the mean of a user sequence (nann_user_seq_mean), the attention scorer
// (nann_attn_scorer_create, nann_attn_prepare, nann_attn_score), and the model loaded from a weights directory or a frozen
// GraphDef (nann_model_load ... nann_model_forward, nann_blaze_options_parse).  A source of nann_core.o; what it shares with
// the other host sources -- the layouts of the three objects among it -- is in nann_host.h.
// The ABI is documented in include/nann_hip.h.  Reference citations are relative to /root/reference/.
#include "nann_host.h"
#include "host/nann_graphdef_text.h"
#include "host/nann_blaze_options.h"
#include "host/nann_npy.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

#include <sys/stat.h>

using namespace nann;

// ===========================================================================
// kernels
// ===========================================================================

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
static uint16_t f32_to_f16_rne(float f) { return nann_npy::f32_to_f16_rne(f); }

// .npy -> host bytes in `expect_dtype` (the scorer-model loader; HugeConst, nann_ops.hip, copies straight from the file image)
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

extern "C" {

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

}  // extern "C"
