// nann_hip.hip -- the core of libnann_hip.so's C ABI (gfx950 only): the error string and the device facts, the memory and
// stream wrappers, the options of a search call, the index, the life cycle of the pre-projected tables, the two merges.
// The ABI is documented in include/nann_hip.h; what the host sources share in nann_host.h.  The drop-in ops are in
// nann_ops.hip, the scorers and the weights-directory model in nann_scorers.hip.  Reference citations are relative to
// /root/reference/.
#include "nann_host.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>

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

// per-device facts, queried once
int nann::device_info(DeviceInfo* out) {
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

// the result block of the calling thread on the current device (ResultBuf, nann_host.h)
int nann::get_result_buf(ResultBuf** out) {
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

int nann::fetch_result(ResultBuf* rb, hipStream_t st) {
  HIP_TRY(hipMemcpyAsync(rb->host, rb->dev, sizeof(OpResult), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return NANN_OK;
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

// ---- options of a search call (SearchOpt, nann_host.h) ----------------------------------------------------------------
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
SearchOpt nann::resolve_options(const nann_search_options* u) {
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
int nann::check_options(const nann_search_options* u) {
  if (!u) return NANN_OK;
  if (u->struct_bytes < 0 || (u->struct_bytes > 0 && u->struct_bytes < 8)) return fail(NANN_ERR_BAD_ARGUMENT, "nann_search_options: struct_bytes");
  const SearchOpt o = resolve_options(u);
  if (o.mode < NANN_TRAVERSAL_AUTO || o.mode > NANN_TRAVERSAL_LDS_HASH32) return fail(NANN_ERR_BAD_ARGUMENT, "nann_search_options: unknown traversal_mode");
  if (o.mlp_form < NANN_MLP_FORM_AUTO || o.mlp_form > NANN_MLP_FORM_PHASED) return fail(NANN_ERR_BAD_ARGUMENT, "nann_search_options: unknown mlp_form");
  return NANN_OK;
}

// ===========================================================================
// C ABI
// ===========================================================================
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

void nann::projection_used(ProjCache& c, const std::shared_ptr<ProjTable>& tab, hipStream_t st) { c.used(tab, st); }

static int projection_release(ProjCache& c, const nann_index* ix) {
  if (c.release(ix->uid)) return NANN_OK;
  return fail(NANN_ERR_BAD_ARGUMENT, "release: no pre-projected table of this index");
}

int nann::mlp_projection(const nann_scorer* sc, const nann_index* ix, hipStream_t st, bool pin, bool enabled, std::shared_ptr<ProjTable>* out) {
  return projection_for(sc->proj, ix, kMlpProjWidth, st, [&](float* t) {
    return launch_mlp_preproject(ix->desc.emb_dtype, ix->desc.item_embs, (long long)ix->desc.n_items, ix->desc.d, sc->mlp.w1, t, st);
  }, pin, enabled, out);
}

int nann::attn_projection(const nann_attn_scorer* sc, const nann_index* ix, hipStream_t st, bool pin, bool enabled, std::shared_ptr<ProjTable>* out) {
  return projection_for(sc->proj, ix, kAttnProjWidth, st, [&](float* t) {
    return launch_attn_preproject(ix->desc.emb_dtype, sc->P, ix->desc.item_embs, (long long)ix->desc.n_items, t, st);
  }, pin, enabled, out);
}

// ---- who scores a call (ScoredBy, nann_host.h) -----------------------------------------------------------------------------
ScoredBy nann::scored_by(const nann_index* ix, const nann_scorer* scorer, const nann_model* m) {
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
