// nann_host.h -- what the host sources of nann_core.o share: nann_hip.hip (the core), nann_ops.hip, nann_scorers.hip,
// nann_flat.hip, nann_traverse.hip, nann_comm.hip, nann_hnsw_build.hip.  Every name is declared once, here, in namespace nann
// with external or inline linkage, next to the name of the source that defines it; the object layouts behind the handles of
// include/nann_hip.h are global, as the handles are.  A helper that one source alone uses stays file-local in that source.
// (fail and NANN_HIP_TRY, which the kernel headers' launchers use too, are declared in nann_search.h.)
#pragma once
#include "nann_search.h"
#include "nann_attn.h"
#include "host/nann_projcache.h"

#include <memory>
#include <string>
#include <vector>

#define HIP_TRY(expr)                                                                    \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess)                                                                \
      return fail(NANN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));      \
  } while (0)

namespace nann {

inline hipStream_t as_stream(nann_stream_t s) { return reinterpret_cast<hipStream_t>(s); }
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---- nann_hip.hip: the error string and the device facts -------------------------------------------------------------------
extern thread_local std::string g_err;  // what fail() stores and nann_last_error() returns; the index probe puts it back
struct DeviceInfo {
  bool ok = false;
  int cus = 0;
  size_t lds_max = 0;
};
int device_info(DeviceInfo* out);  // per-device facts, queried once

// ---- nann_hip.hip: the result block of a call that returns data-dependent counts (OpResult, nann_search.h) ------------------
// one per host thread and device; the drop-in ops and the stand-alone scorers fetch their counts and bad_i through it
struct ResultBuf {
  OpResult* dev = nullptr;
  OpResult* host = nullptr;
  int device = -1;
};
int get_result_buf(ResultBuf** out);
int fetch_result(ResultBuf* rb, hipStream_t st);

// ---- nann_ops.hip: a file into memory (HugeConst; the weights of a model directory) -----------------------------------------
int read_whole_file(const char* path, std::vector<unsigned char>* out);

// ---- the pre-projected tables -----------------------------------------------------------------------------------------------
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
typedef ProjCacheT<HipProjBackend> ProjCache;
typedef ProjTableT<HipProjBackend> ProjTable;

// ---- nann_hip.hip: the options of a search call -------------------------------------------------------------------------
// Every knob of the planner is a field of nann_search_options (include/nann_hip.h, round 5); a field left at -1 takes the
// PROCESS DEFAULT: what nann_set_traversal_mode / nann_set_search_reserve / nann_set_preprojection last stored, else the
// environment read ONCE (A/B tooling: NANN_PREPROJECT=0, NANN_SEARCH_SLOT_RESERVE=n, NANN_MLP_FORM=fused|phased,
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
SearchOpt resolve_options(const nann_search_options* u);
int check_options(const nann_search_options* u);

}  // namespace nann

// the result block as a call that looks for a bad index wants it: bad_i at its largest (nann_ops.hip; nann_score too)
__global__ void k_init_result(nann::OpResult* res);

// ---- the objects behind the handles of include/nann_hip.h ---------------------------------------------------------------
struct nann_scorer {
  nann_scorer_desc desc;
  float* dev_weights = nullptr;  // MLP weights block in HBM
  uint4* dev_packed = nullptr;   // split-f16 planes in MFMA A-fragment order
  float4* dev_packed_x = nullptr;  // W2 as f32 A fragments (exact form, layer 2 resident in LDS)
  float* dev_cert = nullptr;       // certified form: the filter's c_j (certified_bound)
  nann::MlpParams mlp = {};
  mutable nann::ProjCache proj;
};

struct nann_attn_scorer {
  nann::AttnParams P = {};
  int emb_dtype = 0;
  int precision = NANN_MLP_EXACT_F32;  // NANN_MLP_SPLIT_F16: the split-f16 kernels (nann_attn_split.h, nann_attn_proj.h)
  float* dev_weights = nullptr;
  uint4* dev_packed = nullptr;         // split form: A fragments + pre-scaled vectors
  mutable nann::ProjCache proj;
};

// a4: the scoring model behind BlazeXlaOp, loaded from a weights directory (nann_scorers.hip)
struct nann_model {
  int kind = NANN_MODEL_L2;
  int d = 0, seq_len = 0, emb_dtype = NANN_F16;
  nann_scorer* scorer = nullptr;
  nann_attn_scorer* attn = nullptr;
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

// the int8 code table of an index's rows (nann_flat.hip; kernels in nann_sq8.h).  Borrows the index: `uid` is the index's at
// creation, what a call holds its index against.
struct nann_sq8 {
  uint64_t uid = 0;
  int64_t n_items = 0;
  int32_t d = 0;
  int8_t* codes = nullptr;    // i8[n_items, d]
  float* scales = nullptr;    // f32[n_items]
  int32_t* norms = nullptr;   // i32[n_items]
  int64_t bytes = 0;          // device bytes held
  uint64_t serial = 0;        // process-unique: what a nann_sq8_bounds holds its table against
};

// the per-row error terms of a code table (nann_flat.hip; k_sq8_row_err in nann_sq8.h).  Borrows index and table: `uid` and
// `serial` are theirs at creation.
struct nann_sq8_bounds {
  uint64_t uid = 0, serial = 0;
  int64_t n_items = 0;
  float* err = nullptr;       // f32[n_items]: >= |x_i - scale_i codes_i|
  float* xhat = nullptr;      // f32[n_items]: >= scale_i sqrt(norm_i)
};

namespace nann {

// ---- nann_hip.hip: who scores a call ---------------------------------------------------------------------------------------
// A nann_scorer or a nann_model as the host paths dispatch on it: the prepare / release calls, nann_traverse.hip, nann_flat.hip (FlatBy)
struct ScoredBy {
  const nann_scorer* scorer = nullptr;   // l2 / ip / mlp: the scorer, a model's own included
  const nann_attn_scorer* at = nullptr;  // the attention model
  const nann_model* mean_of = nullptr;   // an l2 / ip / mlp model: the query is the mean of its sequence
  ProjCache* cache = nullptr;            // MLP / attention: the cache the pair's pre-projected table belongs to,
  int width = 0;                         //   and the table's floats per row (0: the scorer reads the index's rows)
  const char* what = "scorer";           // the handle's word in a message
  bool mismatch = false;                 // handle and index disagree on d / dtype (ix may be null: no index to disagree with)
};
ScoredBy scored_by(const nann_index* ix, const nann_scorer* scorer, const nann_model* m);

// ---- nann_hip.hip: the pre-projected table of (scorer, index) ---------------------------------------------------------------
// found, or built on `st` (a one-time wait per pair, ~10-20 ms per million items: nann_*_prepare moves it ahead of
// traffic).  *out stays null -- with NANN_OK -- when there is to be no table: pre-projection switched off, or no room for it
// in HBM (the caller then runs the kernels that read the embedding rows; ADVICE r3: a failed hipMalloc must not fail the
// search).  pin: count a prepare call.  projection_used: hands a table back behind the launch that read it.
int mlp_projection(const nann_scorer* sc, const nann_index* ix, hipStream_t st, bool pin, bool enabled, std::shared_ptr<ProjTable>* out);
int attn_projection(const nann_attn_scorer* sc, const nann_index* ix, hipStream_t st, bool pin, bool enabled, std::shared_ptr<ProjTable>* out);
void projection_used(ProjCache& c, const std::shared_ptr<ProjTable>& tab, hipStream_t st);

// ---- nann_flat.hip: a caller's structs into the launch arguments, and the shapes the traversal's forms check the same way --
struct FilterArgs;    // nann_filter.h
struct PredArgs;      // nann_predicate.h
struct GroupCapArgs;  // nann_groupcap.h
struct MmrArgs;       // nann_mmr.h
struct FuseArgs;      // nann_fuse.h
int resolve_filter(const nann_filter* f, const nann_index* ix, FilterArgs* out);
int resolve_predicates(const nann_predicates* p, PredArgs* out);
int resolve_groups(const nann_groups* g, const char* who, GroupCapArgs* a);
int resolve_diversity(const nann_diversity* dv, const char* who, MmrArgs* a);
int mmr_index(const nann_index* ix, const char* who, MmrArgs* a);
int union_check(int64_t n_users, int64_t n_lists, int64_t k_in, int64_t k, const char* who);
int fuse_shape_check(int64_t n_users, int64_t n_lists, int64_t k_in, int64_t k, const char* who);
int fusion_check(const nann_fusion* f, const char* who);
void fusion_into(const nann_fusion* f, FuseArgs* a);

// ---- nann_traverse.hip: what nann_index_create measures, and the batch order ----------------------------------------------
void probe_index(nann_index* ix);
void choose_pivots(nann_index* ix, const std::vector<int32_t>& enter);
int launch_order(const nann_index* ix, const float* q, int n, int32_t* key, int32_t* perm, unsigned int* heads,
                 unsigned int* header, hipStream_t st);

}  // namespace nann
