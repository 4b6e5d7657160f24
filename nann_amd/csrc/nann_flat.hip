// nann_flat.hip -- the host side of the flat retrieval calls, the ones that do not walk the graph: the exhaustive search
// (nann_search_all, nann_search_all_filtered, nann_search_all_model, nann_search_all_model_filtered; kernels in nann_scan.h),
// its range form (nann_search_all_range, nann_search_all_range_model; selection kernels in nann_range.h), its wide form for k up
// to 16384 (nann_search_all_wide, nann_search_all_model_wide, and the selection alone, nann_select_wide; kernels in nann_wide.h)
// and the candidate-list search (nann_search_candidates, nann_search_candidates_model; kernels in nann_cand.h), each with its
// *_workspace_bytes; the union top-k on its own (nann_union_topk; kernel in nann_union.h) and behind the exhaustive search
// over a user's interest vectors (nann_search_all_multi); the fused top-k in the same two places (nann_fuse_topk,
// nann_search_all_multi_fused; kernel in nann_fuse.h); the group cap on its own (nann_group_cap_topk; kernel in
// nann_groupcap.h) and behind the filtered exhaustive search at a fetch width (nann_search_all_grouped, nann_search_all_model_grouped);
// the MMR re-ranking on its own (nann_mmr_topk; kernel in nann_mmr.h) and behind the same search (nann_search_all_diverse,
// nann_search_all_model_diverse); the attribute predicates on their own (nann_predicate_topk, nann_predicate_count; kernels in
// nann_predicate.h) and inside the filtered exhaustive search (nann_search_all_where, nann_search_all_model_where); the int8
// code table of an index (nann_sq8_create, ..) and the exhaustive search over it with an exact re-rank (nann_search_all_sq8;
// kernels in nann_sq8.h), its certified form that returns nann_search_all's bits (nann_sq8_bounds, nann_search_all_sq8_exact) and
// the certified range form that returns nann_search_all_range's (nann_search_all_range_sq8_exact).
//
// A source of nann_core.o.  What it takes from the other host sources, and what the traversal's forms (nann_traverse.hip) take
// from it -- resolve_filter, resolve_predicates, resolve_groups, resolve_diversity, mmr_index, union_check, fuse_shape_check,
// fusion_check, fusion_into -- is declared in nann_host.h.
//
// Every entry point is one walk over the steps below, each written once:
//   flat_by            who scores the call, from a nann_scorer or a nann_model: scored_by, and what the flat kernels take
//   flat_check         the shape of the call (flat_cand_check: with the nann_candidates struct around it)
//   flat_all_bytes     the size of a workspace, per family; the *_workspace_bytes calls and the searches both take it from
//   flat_cand_bytes    here, staged query in front and filter staging behind included
//   flat_workspace     the caller's workspace against that size
//   flat_stage_mean    an l2 / mlp model: the mean of the sequence into the head of the workspace, the scorer form behind it
//   flat_table         the pre-projected table of an MLP or attention pair; projection_used hands it back behind the launch
//   flat_ids_of, flat_rows_of, flat_lists_of   the index's and the lists' fields into ScanArgs / CandArgs / CandAttnArgs
// A new flat form is an entry point at the bottom that calls flat_all or flat_cand (or a third walk made of the same steps).
//
// The ORDER in which a call looks at its arguments is part of its contract -- with two faults present, which one the caller is
// told -- and the families differ in it for no deeper reason than their history.  The walks keep every order as it was and say
// where they branch for it (tests/test_flat_contract_gpu.py pins them).
#include "nann_host.h"
#include "nann_scan.h"
#include "nann_cand.h"
#include "nann_union.h"
#include "nann_fuse.h"
#include "nann_groupcap.h"
#include "nann_mmr.h"
#include "nann_sq8.h"

#include <algorithm>
#include <atomic>
#include <cfloat>

#include <memory>
#include <string>

using namespace nann;

// ---- who scores a call ---------------------------------------------------------------------------------------------------
// ScoredBy (nann_host.h: the scorer or the attention scorer, mean_of, cache, what, mismatch), and what the flat kernels take
struct FlatBy : ScoredBy {
  int kind = NANN_SCORER_L2;     // the scorer's nann_scorer_kind, or kScanAttn for the attention model
  int exact = 0;                 // MLP / attention: the f32 form (also the MLP's certified precision), else split-f16
  MlpParams mlp = {};            // MLP
  AttnParams attn = {};          // attention
  const char* unit = "queries";  // what the handle scores for, in a message
};

static int flat_by(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, const char* who, FlatBy* by) {
  *by = FlatBy{};
  if (!ix || !(scorer || m)) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  static_cast<ScoredBy&>(*by) = scored_by(ix, scorer, m);
  if (m) by->unit = "users";
  if (by->at) {
    by->kind = kScanAttn;
    by->attn = by->at->P;
    by->exact = by->at->precision != NANN_MLP_SPLIT_F16;
  } else if (!by->scorer) {
    return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  } else {
    by->kind = by->scorer->desc.kind;
    if (by->kind == NANN_SCORER_MLP) {
      by->mlp = by->scorer->mlp;
      by->exact = by->scorer->desc.precision == NANN_MLP_EXACT_F32 || by->scorer->desc.precision == NANN_MLP_CERTIFIED;
    } else if (by->kind != NANN_SCORER_L2 && by->kind != NANN_SCORER_IP) {  // (L2 and the inner product read the index's rows: no table)
      return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": unknown scorer kind");
    }
  }
  return NANN_OK;
}

// ---- the shape of a call -------------------------------------------------------------------------------------------------
static int flat_bad_k(int32_t k) { return fail(NANN_ERR_BAD_ARGUMENT, "Need k >= 0, got " + std::to_string(k)); }  // topk_op.cc:60-61

// lists: the candidate family (n_cand rows in all).  The exhaustive family holds k against n_items as TopKV2 does, and names a
// negative k behind a mismatched handle; the candidate family names it in front.
static int flat_check(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, int64_t n, int32_t k, bool lists,
                      int64_t n_cand, const char* who, FlatBy* by, int max_k = kMaxK) {  // max_k: kWideMaxK for the wide form
  const int rc = flat_by(ix, scorer, m, who, by);
  if (rc) return rc;
  if (n < 0) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": n_" + by->unit + " < 0");
  if (lists) {
    if (n_cand < 0) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": n_cand < 0");
    if (k < 0) return flat_bad_k(k);
  }
  if (by->mismatch) return fail(NANN_ERR_BAD_ARGUMENT, std::string(by->what) + " and index disagree on d / dtype");
  if (!lists) {
    if (k < 0) return flat_bad_k(k);
    if (ix->desc.n_items < k)  // topk_op.cc:67-71
      return fail(NANN_ERR_TOPK_K_GT_N, "input must have at least k columns. Had " + std::to_string(ix->desc.n_items) +
                                            ", needed " + std::to_string(k));
  }
  if (k > max_k) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": k <= " + std::to_string(max_k));
  if (lists) {
    if (n_cand > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": list positions are 32-bit");
    if (n > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": too many " + by->unit + " in one call");
  }
  // (the last two cannot fail for an index nann_index_create has made -- it takes these d only, and at most 2^31 - 1 rows --
  // so their place in the order is free)
  const int d = ix->desc.d;
  if (by->kind != kScanAttn && !(d == 64 || d == 128 || d == 256 || d == 512))  // the forms that read embedding rows
    return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": d must be 64, 128, 256 or 512");
  if (ix->desc.n_items > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": row numbers are 32-bit");
  return NANN_OK;
}

// the caller's nann_candidates, around the checks of the call
static int flat_cand_check(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, int64_t n, int32_t k,
                           const nann_candidates* cand, const char* who, FlatBy* by) {
  if (!cand) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  if (cand->struct_bytes != 0 && cand->struct_bytes != (int32_t)sizeof(nann_candidates))
    return fail(NANN_ERR_BAD_ARGUMENT, "nann_candidates: struct_bytes");
  const int rc = flat_check(ix, scorer, m, n, k, true, cand->n_cand, who, by);
  if (rc) return rc;
  if (cand->n_cand > 0 && !cand->rows) return fail(NANN_ERR_BAD_ARGUMENT, "nann_candidates: rows is null while n_cand > 0");
  if (n > 0 && !cand->row_splits)
    return fail(NANN_ERR_BAD_ARGUMENT, std::string("nann_candidates: row_splits is null while n_") + by->unit + " > 0");
  return NANN_OK;
}

// the caller's nann_filter as the kernels take it, over n_items rows; NULL denies nothing
static int resolve_filter_rows(const nann_filter* f, long long n_items, FilterArgs* out) {
  *out = FilterArgs{};
  out->n_items = n_items;
  if (!f) return NANN_OK;
  if (f->struct_bytes != 0 && f->struct_bytes != (int32_t)sizeof(nann_filter)) return fail(NANN_ERR_BAD_ARGUMENT, "nann_filter: struct_bytes");
  if (f->n_excl < 0) return fail(NANN_ERR_BAD_ARGUMENT, "nann_filter: n_excl < 0");
  if (f->excl_row_splits && f->n_excl > 0 && !f->excl_rows) return fail(NANN_ERR_BAD_ARGUMENT, "nann_filter: excl_row_splits without excl_rows");
  out->deny_bits = f->deny_bits;
  if (f->excl_row_splits && f->n_excl > 0) {
    out->splits = f->excl_row_splits;
    out->rows = f->excl_rows;
    out->n_excl = (long long)f->n_excl;
  }
  return NANN_OK;
}
int nann::resolve_filter(const nann_filter* f, const nann_index* ix, FilterArgs* out) {
  return resolve_filter_rows(f, (long long)ix->desc.n_items, out);
}

// the caller's nann_predicates as the kernels take it (nann_predicate.h); NULL holds no condition.  Touches nothing but the struct.
int nann::resolve_predicates(const nann_predicates* p, PredArgs* out) {
  *out = PredArgs{};
  if (!p) return NANN_OK;
  if (p->struct_bytes != 0 && p->struct_bytes != (int32_t)sizeof(nann_predicates)) return fail(NANN_ERR_BAD_ARGUMENT, "nann_predicates: struct_bytes");
  if (p->n_labels < 0) return fail(NANN_ERR_BAD_ARGUMENT, "nann_predicates: n_labels < 0");
  if (p->label_splits && p->n_labels > 0 && !p->labels) return fail(NANN_ERR_BAD_ARGUMENT, "nann_predicates: label_splits without labels");
  if (p->label_splits && !p->label_of_row) return fail(NANN_ERR_BAD_ARGUMENT, "nann_predicates: label_splits without label_of_row");
  if ((p->value_lo || p->value_hi) && !p->value_of_row) return fail(NANN_ERR_BAD_ARGUMENT, "nann_predicates: value bounds without value_of_row");
  if ((p->tags_all || p->tags_any || p->tags_none) && !p->tags_of_row)
    return fail(NANN_ERR_BAD_ARGUMENT, "nann_predicates: tag conditions without tags_of_row");
  out->label_of_row = p->label_of_row;
  out->value_of_row = p->value_of_row;
  out->tags_of_row = reinterpret_cast<const unsigned long long*>(p->tags_of_row);
  if (p->label_splits && p->n_labels > 0) {
    out->label_splits = p->label_splits;
    out->labels = p->labels;
    out->n_labels = (long long)p->n_labels;
  }
  out->value_lo = p->value_lo;
  out->value_hi = p->value_hi;
  out->tags_all = reinterpret_cast<const unsigned long long*>(p->tags_all);
  out->tags_any = reinterpret_cast<const unsigned long long*>(p->tags_any);
  out->tags_none = reinterpret_cast<const unsigned long long*>(p->tags_none);
  return NANN_OK;
}

// the caller's nann_groups into the launch arguments of the cap (nann_groupcap.h).  `who`: the entry point in a message.
int nann::resolve_groups(const nann_groups* g, const char* who, GroupCapArgs* a) {
  if (!g) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null nann_groups");
  if (g->struct_bytes != 0 && g->struct_bytes != (int32_t)sizeof(nann_groups)) return fail(NANN_ERR_BAD_ARGUMENT, "nann_groups: struct_bytes");
  if (!g->group_of_row) return fail(NANN_ERR_BAD_ARGUMENT, "nann_groups: group_of_row is null");
  if (!g->caps && g->cap < 1) return fail(NANN_ERR_BAD_ARGUMENT, "nann_groups: cap < 1 without caps");
  a->group_of_row = g->group_of_row;
  a->cap = g->cap;
  a->caps = g->caps;
  return NANN_OK;
}

// ---- the workspace -------------------------------------------------------------------------------------------------------
// An l2 / mlp model: [q f32[n, d], the means | the workspace of the scorer form].  Exhaustive: the ScanLayout of the kind (the
// attention model's has each chunk's kt / upad in the place of the queries; nann_scan.h), and behind it a filtered call's
// staging area of its final selection.  Candidates: CandLayout, or CandAttnLayout under the attention model.
static size_t flat_mean_bytes(const FlatBy& by, int64_t n) {
  return by.mean_of ? ((size_t)n * (size_t)by.mean_of->d * 4 + 255) & ~(size_t)255 : 0;
}
static size_t flat_all_bytes(const nann_index* ix, const FlatBy& by, int64_t n, int32_t k, bool filtered, ScanLayout* L) {
  *L = scan_layout((long long)ix->desc.n_items, ix->desc.d, by.kind, (long long)n, k);
  return flat_mean_bytes(by, n) + L->total + (filtered ? scan_filter_stage_bytes(L->chunk, k) : 0);
}
static size_t flat_cand_bytes(const FlatBy& by, int64_t n, int64_t n_cand) {
  if (by.kind == kScanAttn) return cand_attn_layout((long long)n, (long long)n_cand).total;
  return flat_mean_bytes(by, n) + cand_layout(by.kind, (long long)n, (long long)n_cand).total;
}

// `form`: "" or "_filtered" -- `need` is what <who><form>_workspace_bytes gives
static int flat_workspace(const void* workspace, int64_t workspace_bytes, size_t need, const char* who, const char* form) {
  if (!workspace || workspace_bytes < (int64_t)need)
    return fail(NANN_ERR_CAPACITY, std::string("workspace smaller than ") + who + form + "_workspace_bytes()");
  if (reinterpret_cast<uintptr_t>(workspace) & 255u) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": workspace must be 256-byte aligned");
  return NANN_OK;
}

// An l2 / mlp model: the query is the mean of the sequence (nann_search_model), into the head of the workspace; *q, *workspace
// and *workspace_bytes are then the scorer form's.
static int flat_stage_mean(const FlatBy& by, const void* comm_seq_f16, int64_t n, const float** q, void** workspace,
                           int64_t* workspace_bytes, nann_stream_t stream) {
  float* mean = static_cast<float*>(*workspace);
  const int rc = nann_user_seq_mean(comm_seq_f16, n, by.mean_of->seq_len, by.mean_of->d, mean, stream);
  if (rc) return rc;
  const size_t qb = flat_mean_bytes(by, n);
  *q = mean;
  *workspace = static_cast<unsigned char*>(*workspace) + qb;
  *workspace_bytes -= (int64_t)qb;
  return NANN_OK;
}

// ---- the pre-projected table ---------------------------------------------------------------------------------------------
// The MLP scorer and the attention model score from the pre-projected table of their pair, obtained as search_impl does; the
// caller hands it back with projection_used(*by.cache, ..) behind its launch.
static int flat_table(const FlatBy& by, const nann_index* ix, const nann_search_options* options, hipStream_t st,
                      const char* who, std::shared_ptr<ProjTable>* tab) {
  if (!resolve_options(options).preproject)
    return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": the " + by.what + " scores from its pre-projected table and preprojection is switched off");
  const int rc = by.at ? attn_projection(by.at, ix, st, false, true, tab) : mlp_projection(by.scorer, ix, st, false, true, tab);
  if (rc) return rc;
  if (!*tab) return fail(NANN_ERR_CAPACITY, std::string(who) + ": no room in HBM for the pre-projected table of this (" + by.what + ", index) pair");
  return NANN_OK;
}

// ---- the launch arguments ------------------------------------------------------------------------------------------------
// ScanArgs, CandArgs and CandAttnArgs name what they share alike: every one the index's ids, the first two its rows as well,
// the last two the caller's lists
template <class A> static void flat_ids_of(const nann_index* ix, A* a) {
  a->item_ids = ix->desc.item_ids;
  a->n_items = (long long)ix->desc.n_items;
}
template <class A> static void flat_rows_of(const nann_index* ix, A* a) {
  flat_ids_of(ix, a);
  a->emb = ix->desc.item_embs;
  a->d = ix->desc.d;
  a->dt = ix->desc.emb_dtype;
}
template <class A> static void flat_lists_of(const nann_candidates* cand, int cus, A* a) {
  a->cus = cus;
  a->row_splits = cand->row_splits;
  a->rows = cand->rows;
  a->n_cand = (long long)cand->n_cand;
}

// ---- exhaustive search (nann_scan.h): test_all of main.py:194-237 for a batch, under a scorer or whatever model the node names
// x: q f32[n, d] with a scorer, comm_seq f16[n, seq_len, E] with a model.  `who`: the entry point in a message; a filtered
// call speaks under its unfiltered twin's name.
static int flat_all_size(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, int64_t n, int32_t k, bool filtered,
                         int64_t* nbytes, const char* who) {
  if (!nbytes) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  FlatBy by;
  const int rc = flat_check(ix, scorer, m, n, k, false, 0, who, &by);
  if (rc) return rc;
  ScanLayout L;
  *nbytes = n == 0 || k == 0 ? 0 : (int64_t)flat_all_bytes(ix, by, n, k, filtered, &L);
  return NANN_OK;
}

static int flat_all(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, const void* x, int64_t n, int32_t k,
                    int64_t* out_item_ids, float* out_scores, int32_t* out_index, void* workspace, int64_t workspace_bytes,
                    const nann_search_options* options, bool filtered, const nann_filter* filter, int32_t* n_out,
                    nann_stream_t stream, const char* who, const PredArgs* pred = nullptr) {  // pred: a filtered call's predicates
  FlatBy by;
  int rc = flat_check(ix, scorer, m, n, k, false, 0, who, &by);
  if (rc) return rc;
  if (n == 0 || k == 0) return NANN_OK;
  if (!x || !out_item_ids) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  ScanLayout L;
  const size_t need = flat_all_bytes(ix, by, n, k, filtered, &L);
  const char* form = pred ? "_where" : filtered ? "_filtered" : "";
  // a model form looks at its workspace before its options, a scorer form at its options and its filter first
  if (m) {
    rc = flat_workspace(workspace, workspace_bytes, need, who, form);
    if (rc) return rc;
    if (by.mean_of) {  // (the mean is on the stream before the scorer form has looked at the options)
      const float* q = nullptr;
      rc = flat_stage_mean(by, x, n, &q, &workspace, &workspace_bytes, stream);
      if (rc) return rc;
      return flat_all(ix, by.scorer, nullptr, q, n, k, out_item_ids, out_scores, out_index, workspace, workspace_bytes, options,
                      filtered, filter, n_out, stream, "nann_search_all", pred);
    }
  }
  rc = check_options(options);
  if (rc) return rc;
  ScanFilter sf = {};
  if (!m) {
    if (filtered) rc = resolve_filter(filter, ix, &sf.f);
    if (rc) return rc;
    rc = flat_workspace(workspace, workspace_bytes, need, who, form);
    if (rc) return rc;
  }
  hipStream_t st = as_stream(stream);
  ScanArgs a = {};
  std::shared_ptr<ProjTable> tab;
  if (by.cache) {
    rc = flat_table(by, ix, options, st, who, &tab);
    if (rc) return rc;
    DeviceInfo di;
    rc = device_info(&di);
    if (rc) return rc;
    a.proj = tab->table;
    a.mlp_workgroups = di.cus;
  }
  if (m && filtered) rc = resolve_filter(filter, ix, &sf.f);  // (the attention model: its filter behind its table)
  if (rc) return rc;
  if (filtered) {  // the staging area of the final selection lies behind the unfiltered workspace
    sf.stage = static_cast<unsigned char*>(workspace) + L.total;
    sf.n_out = n_out;
    sf.pred = pred;
    a.filter = &sf;
  }
  flat_rows_of(ix, &a);
  a.kind = by.kind;
  a.exact = by.exact;
  a.mlp = by.mlp;
  a.attn = by.attn;
  rc = launch_scan(a, L, static_cast<const float*>(x), (long long)n, k, static_cast<unsigned char*>(workspace), out_item_ids,
                   out_scores, out_index, st);
  if (tab) projection_used(*by.cache, tab, st);
  return rc;
}

// ---- range search (nann_range.h): every row at or above a per-query cut, under a scorer or a model ----------------------------
// The third walk over the same steps.  There is no k: flat_check runs at k = 0, the workspace is the unfiltered ScanLayout at
// k = 0 -- no candidate lists -- with the block counts of the range selection behind it, and launch_scan takes the range form.
// Every check stands in front of the first launch, the mean of an l2 / mlp model included: a failing call writes nothing.
static int flat_range_check(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, int64_t n, const char* who,
                            FlatBy* by) {
  const int rc = flat_check(ix, scorer, m, n, 0, false, 0, who, by);
  if (rc) return rc;
  if (n > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": too many " + by->unit + " in one call");
  return NANN_OK;
}
static size_t flat_range_bytes(const nann_index* ix, const FlatBy& by, int64_t n, ScanLayout* L) {
  const size_t scan = flat_all_bytes(ix, by, n, 0, false, L);
  return scan + range_counts_bytes(L->chunk, (long long)ix->desc.n_items);
}

static int flat_range_size(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, int64_t n, int64_t* nbytes,
                           const char* who) {
  if (!nbytes) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  FlatBy by;
  const int rc = flat_range_check(ix, scorer, m, n, who, &by);
  if (rc) return rc;
  ScanLayout L;
  *nbytes = n == 0 ? 0 : (int64_t)flat_range_bytes(ix, by, n, &L);
  return NANN_OK;
}

static int flat_range(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, const void* x, int64_t n,
                      const float* thresholds, int64_t capacity, int64_t* out_row_splits, int64_t* out_item_ids, float* out_scores,
                      int32_t* out_index, void* workspace, int64_t workspace_bytes, const nann_search_options* options,
                      const nann_filter* filter, nann_stream_t stream, const char* who) {
  FlatBy by;
  int rc = flat_range_check(ix, scorer, m, n, who, &by);
  if (rc) return rc;
  if (capacity < 0) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": capacity < 0");
  if (n == 0) return NANN_OK;
  if (!x || !thresholds || !out_row_splits) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  if (capacity > 0 && !out_item_ids) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": out_item_ids is null while capacity > 0");
  rc = check_options(options);
  if (rc) return rc;
  ScanFilter sf = {};
  rc = resolve_filter(filter, ix, &sf.f);
  if (rc) return rc;
  ScanLayout L;
  const size_t need = flat_range_bytes(ix, by, n, &L);
  rc = flat_workspace(workspace, workspace_bytes, need, who, "");
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  ScanArgs a = {};
  std::shared_ptr<ProjTable> tab;
  if (by.cache) {
    rc = flat_table(by, ix, options, st, who, &tab);
    if (rc) return rc;
    DeviceInfo di;
    rc = device_info(&di);
    if (rc) return rc;
    a.proj = tab->table;
    a.mlp_workgroups = di.cus;
  }
  if (by.mean_of) {  // (behind every check: the mean is the first thing on the stream)
    const float* q = nullptr;
    rc = flat_stage_mean(by, x, n, &q, &workspace, &workspace_bytes, stream);
    if (rc) return rc;
    x = q;
  }
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  ScanRange r = {};
  r.thr = thresholds;
  r.capacity = (long long)capacity;
  r.row_splits = out_row_splits;
  r.counts = reinterpret_cast<int32_t*>(ws + L.total);
  r.n_blocks = range_n_blocks((long long)ix->desc.n_items);
  a.range = &r;
  if (sf.f.deny_bits || filter_has_lists(sf.f)) a.filter = &sf;  // (stage and n_out stay null: the range form reads `f` only)
  flat_rows_of(ix, &a);
  a.kind = by.kind;
  a.exact = by.exact;
  a.mlp = by.mlp;
  a.attn = by.attn;
  rc = launch_scan(a, L, static_cast<const float*>(x), (long long)n, 0, ws, out_item_ids, out_scores, out_index, st);
  if (tab) projection_used(*by.cache, tab, st);
  return rc;
}

// ---- wide exhaustive search (nann_wide.h): the top k for k up to kWideMaxK, under a scorer or a model ------------------------
// The fourth walk over the same steps: nann_search_all_where's checks in its order -- the predicates, flat_check with the wide
// limit, the nulls, then a model form its workspace before its options and a scorer form its options and filter first -- and, as
// the range form, every check in front of the first launch, the mean of an l2 / mlp model included.  The workspace is the
// unfiltered ScanLayout at k = 0 -- no slab lists -- with the histograms, counters and staging list of the selection behind it.
static size_t flat_wide_bytes(const nann_index* ix, const FlatBy& by, int64_t n, int32_t k, ScanLayout* L) {
  const size_t scan = flat_all_bytes(ix, by, n, 0, false, L);
  return scan + wide_bytes(L->chunk, (long long)ix->desc.n_items, k);
}

static int flat_wide_size(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, int64_t n, int32_t k, int64_t* nbytes,
                          const char* who) {
  if (!nbytes) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  FlatBy by;
  const int rc = flat_check(ix, scorer, m, n, k, false, 0, who, &by, kWideMaxK);
  if (rc) return rc;
  ScanLayout L;
  *nbytes = n == 0 || k == 0 ? 0 : (int64_t)flat_wide_bytes(ix, by, n, k, &L);
  return NANN_OK;
}

static int flat_wide(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, const void* x, int64_t n, int32_t k,
                     int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* n_out, void* workspace,
                     int64_t workspace_bytes, const nann_search_options* options, const nann_filter* filter,
                     const nann_predicates* predicates, nann_stream_t stream, const char* who) {
  PredArgs pa;
  int rc = resolve_predicates(predicates, &pa);
  if (rc) return rc;
  FlatBy by;
  rc = flat_check(ix, scorer, m, n, k, false, 0, who, &by, kWideMaxK);
  if (rc) return rc;
  if (n == 0 || k == 0) return NANN_OK;
  if (!x || !out_item_ids) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  ScanLayout L;
  const size_t need = flat_wide_bytes(ix, by, n, k, &L);
  ScanFilter sf = {};
  if (m) {
    rc = flat_workspace(workspace, workspace_bytes, need, who, "");
    if (rc) return rc;
    rc = check_options(options);
    if (rc) return rc;
    if (by.mean_of) rc = resolve_filter(filter, ix, &sf.f);  // (an l2 / mlp model goes on as its scorer form: the filter next)
    if (rc) return rc;
  } else {
    rc = check_options(options);
    if (rc) return rc;
    rc = resolve_filter(filter, ix, &sf.f);
    if (rc) return rc;
    rc = flat_workspace(workspace, workspace_bytes, need, who, "");
    if (rc) return rc;
  }
  hipStream_t st = as_stream(stream);
  ScanArgs a = {};
  std::shared_ptr<ProjTable> tab;
  if (by.cache) {
    rc = flat_table(by, ix, options, st, who, &tab);
    if (rc) return rc;
    DeviceInfo di;
    rc = device_info(&di);
    if (rc) return rc;
    a.proj = tab->table;
    a.mlp_workgroups = di.cus;
  }
  if (m && !by.mean_of) rc = resolve_filter(filter, ix, &sf.f);  // (the attention model: its filter behind its table)
  if (rc) {
    if (tab) projection_used(*by.cache, tab, st);
    return rc;
  }
  if (by.mean_of) {  // (behind every check: the mean is the first thing on the stream)
    const float* q = nullptr;
    rc = flat_stage_mean(by, x, n, &q, &workspace, &workspace_bytes, stream);
    if (rc) return rc;
    x = q;
  }
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  const ScanWide w = wide_carve(ws + L.total, L.chunk, (long long)ix->desc.n_items, k, n_out);
  a.wide = &w;
  if (predicates) sf.pred = &pa;
  if (sf.f.deny_bits || filter_has_lists(sf.f) || sf.pred) a.filter = &sf;  // (stage and n_out stay null: the wide form reads `f` and `pred` only)
  flat_rows_of(ix, &a);
  a.kind = by.kind;
  a.exact = by.exact;
  a.mlp = by.mlp;
  a.attn = by.attn;
  rc = launch_scan(a, L, static_cast<const float*>(x), (long long)n, k, ws, out_item_ids, out_scores, out_index, st);
  if (tab) projection_used(*by.cache, tab, st);
  return rc;
}

// the selection alone over a caller's matrix: rows in pieces of at most kWideMaxChunk whose block counters stay within 64 MB
static int select_wide_check(int64_t n_rows, int64_t n_cols, int32_t k, const char* who) {
  if (n_rows < 0 || n_cols < 0) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": negative size");
  if (k < 0) return flat_bad_k(k);
  if (n_cols < k)
    return fail(NANN_ERR_TOPK_K_GT_N, "input must have at least k columns. Had " + std::to_string(n_cols) + ", needed " + std::to_string(k));
  if (k > kWideMaxK) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": k <= " + std::to_string(kWideMaxK));
  if (n_cols > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": column numbers are 32-bit");
  return NANN_OK;
}
static int select_wide_chunk(int64_t n_rows, int64_t n_cols) {
  const long long by_counts = ((long long)64 << 20) / ((long long)range_n_blocks((long long)n_cols) * 8);
  return (int)std::max<long long>(1, std::min<long long>({(long long)kWideMaxChunk, (long long)n_rows, by_counts}));
}

// ---- candidate-list search (nann_cand.h): the top k of every query's own list of rows, under a scorer or a model -------------
static int flat_cand_size(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, int64_t n, int64_t n_cand,
                          int32_t k, int64_t* nbytes, const char* who) {
  if (!nbytes) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  FlatBy by;
  const int rc = flat_check(ix, scorer, m, n, k, true, n_cand, who, &by);
  if (rc) return rc;
  *nbytes = n == 0 || k == 0 ? 0 : (int64_t)flat_cand_bytes(by, n, n_cand);
  return NANN_OK;
}

static int flat_cand(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, const void* x, int64_t n, int32_t k,
                     const nann_candidates* cand, int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* out_pos,
                     int32_t* n_out, int32_t* status, void* workspace, int64_t workspace_bytes, const nann_search_options* options,
                     nann_stream_t stream, const char* who) {
  FlatBy by;
  int rc = flat_cand_check(ix, scorer, m, n, k, cand, who, &by);
  if (rc) return rc;
  if (n == 0 || k == 0) return NANN_OK;
  if (!x || !out_item_ids || !status) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  rc = check_options(options);  // (both forms of this family: the options, then the workspace)
  if (rc) return rc;
  rc = flat_workspace(workspace, workspace_bytes, flat_cand_bytes(by, n, cand->n_cand), who, "");
  if (rc) return rc;
  if (by.mean_of) {
    const float* q = nullptr;
    rc = flat_stage_mean(by, x, n, &q, &workspace, &workspace_bytes, stream);
    if (rc) return rc;
    return flat_cand(ix, by.scorer, nullptr, q, n, k, cand, out_item_ids, out_scores, out_index, out_pos, n_out, status, workspace,
                     workspace_bytes, options, stream, "nann_search_candidates");
  }
  hipStream_t st = as_stream(stream);
  DeviceInfo di;
  rc = device_info(&di);
  if (rc) return rc;
  std::shared_ptr<ProjTable> tab;
  if (by.cache) rc = flat_table(by, ix, options, st, who, &tab);
  if (rc) return rc;
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  if (by.at) {
    CandAttnArgs a = {};
    flat_ids_of(ix, &a);
    flat_lists_of(cand, di.cus, &a);
    a.attn = by.attn;
    a.exact = by.exact;
    a.proj = tab->table;
    rc = launch_cand_attn(a, cand_attn_layout((long long)n, a.n_cand), x, (long long)n, k, ws, out_item_ids, out_scores, out_index,
                          out_pos, n_out, status, st);
  } else {
    CandArgs a = {};
    flat_rows_of(ix, &a);
    flat_lists_of(cand, di.cus, &a);
    a.kind = by.kind;
    a.exact = by.exact;
    a.mlp = by.mlp;
    if (tab) a.proj = tab->table;
    rc = launch_cand(a, cand_layout(by.kind, (long long)n, a.n_cand), static_cast<const float*>(x), (long long)n, k, ws, out_item_ids,
                     out_scores, out_index, out_pos, n_out, status, st);
  }
  if (tab) projection_used(*by.cache, tab, st);
  return rc;
}

// ---- union top-k (nann_union.h): a user's n_lists result lists -> the k best distinct rows -----------------------------------
// the shape of a union: n_in = n_lists * k_in entries per user.  `who`: the entry point in a message.
int nann::union_check(int64_t n_users, int64_t n_lists, int64_t k_in, int64_t k, const char* who) {
  if (n_users < 0 || n_lists < 0 || k_in < 0) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": negative size");
  if (k < 0) return flat_bad_k((int32_t)k);
  if (k > n_lists * k_in) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": k exceeds the n_lists * k_in entries a user brings");
  if (k > kMaxK) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": k <= 1024");
  if (n_lists * k_in > NANN_UNION_MAX_IN)
    return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": at most NANN_UNION_MAX_IN = 8192 entries per user");
  if (n_users > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": too many users in one call");
  return NANN_OK;
}

// ---- exhaustive multi-vector search: flat_all over the n_users * n_vec vectors at k into a staging area, then the union ------
// workspace: [flat_all's, rounded up to 256 | item ids i64[n, k], scores f32[n, k], rows i32[n, k] of the n = n_users * n_vec
// vectors, rounded up | the union's]
struct FlatMultiBytes {
  size_t inner, stage_off, union_off, total;
};
static size_t flat_multi_stage_bytes(int64_t n, int32_t k) { return ((size_t)n * (size_t)k * 16 + 255) & ~(size_t)255; }
static int flat_all_multi_check(const nann_index* ix, const nann_scorer* scorer, int64_t n_users, int32_t n_vec, int32_t k,
                                const char* who, FlatBy* by) {
  if (n_vec < 1) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": n_vec < 1");
  if (n_users > 0x7fffffffll / n_vec) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": too many vectors in one call");
  int rc = flat_check(ix, scorer, nullptr, n_users * n_vec, k, false, 0, who, by);
  if (rc) return rc;
  return union_check(n_users, n_vec, k, k, who);
}
static FlatMultiBytes flat_all_multi_bytes(const nann_index* ix, const FlatBy& by, int64_t n_users, int32_t n_vec, int32_t k) {
  ScanLayout L;
  FlatMultiBytes b;
  b.inner = flat_all_bytes(ix, by, n_users * n_vec, k, false, &L);
  b.stage_off = (b.inner + 255) & ~(size_t)255;
  b.union_off = b.stage_off + flat_multi_stage_bytes(n_users * n_vec, k);
  b.total = b.union_off + union_ws_bytes((long long)n_users, (long long)n_vec * k);
  return b;
}

static int flat_all_multi(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_users, int32_t n_vec, int32_t k,
                          int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* out_vec, int32_t* n_out,
                          void* workspace, int64_t workspace_bytes, const nann_search_options* options, nann_stream_t stream,
                          const char* who) {
  FlatBy by;
  int rc = flat_all_multi_check(ix, scorer, n_users, n_vec, k, who, &by);
  if (rc) return rc;
  if (n_users == 0 || k == 0) return NANN_OK;
  if (!q || !out_item_ids) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  rc = check_options(options);
  if (rc) return rc;
  const FlatMultiBytes b = flat_all_multi_bytes(ix, by, n_users, n_vec, k);
  rc = flat_workspace(workspace, workspace_bytes, b.total, who, "");
  if (rc) return rc;
  const int64_t n = n_users * n_vec;
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  int64_t* s_ids = reinterpret_cast<int64_t*>(ws + b.stage_off);
  float* s_scores = reinterpret_cast<float*>(ws + b.stage_off + (size_t)n * k * 8);
  int32_t* s_rows = reinterpret_cast<int32_t*>(ws + b.stage_off + (size_t)n * k * 12);
  rc = flat_all(ix, scorer, nullptr, q, n, k, s_ids, s_scores, s_rows, workspace, (int64_t)b.inner, options, false, nullptr, nullptr,
                stream, "nann_search_all");
  if (rc) return rc;
  UnionArgs a = {};
  a.scores = s_scores;
  a.rows = s_rows;
  a.n_lists = n_vec;
  a.k_in = k;
  a.k = k;
  flat_ids_of(ix, &a);
  a.best = reinterpret_cast<unsigned long long*>(ws + b.union_off);
  a.out_index = out_index;
  a.out_scores = out_scores;
  a.out_item_ids = out_item_ids;
  a.out_list = out_vec;
  a.n_out = n_out;
  return launch_union_topk(a, (long long)n_users, as_stream(stream));
}

// ---- fused top-k (nann_fuse.h): a user's n_lists result lists -> the k best distinct rows by an accumulated score -------------
// the shape of a fuse: the union's refusals in their order, then the width of out_lists
int nann::fuse_shape_check(int64_t n_users, int64_t n_lists, int64_t k_in, int64_t k, const char* who) {
  const int rc = union_check(n_users, n_lists, k_in, k, who);
  if (rc) return rc;
  if (n_lists > NANN_FUSE_MAX_LISTS) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": at most NANN_FUSE_MAX_LISTS = 64 lists per user");
  return NANN_OK;
}
// the caller's nann_fusion: null, struct_bytes, mode, rrf_c, weights_per_user, in this order.  Nothing of it is dereferenced.
int nann::fusion_check(const nann_fusion* f, const char* who) {
  if (!f) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null fusion");
  if (f->struct_bytes != 0 && f->struct_bytes != (int32_t)sizeof(nann_fusion)) return fail(NANN_ERR_BAD_ARGUMENT, "nann_fusion: struct_bytes");
  if (f->mode < NANN_FUSE_SUM || f->mode > NANN_FUSE_RRF) return fail(NANN_ERR_BAD_ARGUMENT, "nann_fusion: unknown mode");
  if (f->mode == NANN_FUSE_RRF && !(f->rrf_c >= 0.0f && f->rrf_c <= FLT_MAX))
    return fail(NANN_ERR_BAD_ARGUMENT, "nann_fusion: rrf_c must be a finite value >= 0");
  if (f->weights_per_user != 0 && f->weights_per_user != 1) return fail(NANN_ERR_BAD_ARGUMENT, "nann_fusion: weights_per_user must be 0 or 1");
  return NANN_OK;
}
void nann::fusion_into(const nann_fusion* f, FuseArgs* a) {
  a->mode = f->mode;
  a->rrf_c = f->rrf_c;
  a->weights = f->weights;
  a->weights_per_user = f->weights_per_user;
}

// ---- exhaustive multi-vector search, fused: flat_all over the n_users * n_vec vectors at k = fetch into the staging area of
// flat_all_multi, then the fuse at k.  workspace: [flat_all's at fetch, rounded up to 256 | the staging area | the fuse's]
static int flat_all_multi_fused_check(const nann_index* ix, const nann_scorer* scorer, int64_t n_users, int32_t n_vec, int32_t fetch,
                                      int64_t k, const char* who, FlatBy* by) {
  if (n_vec < 1) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": n_vec < 1");
  if (n_users > 0x7fffffffll / n_vec) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": too many vectors in one call");
  int rc = flat_check(ix, scorer, nullptr, n_users * n_vec, fetch, false, 0, who, by);
  if (rc) return rc;
  if (k < 0 || k > (int64_t)n_vec * fetch) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": k must lie in [0, n_vec * fetch]");
  return fuse_shape_check(n_users, n_vec, fetch, k, who);
}
static FlatMultiBytes flat_all_multi_fused_bytes(const nann_index* ix, const FlatBy& by, int64_t n_users, int32_t n_vec, int32_t fetch) {
  ScanLayout L;
  FlatMultiBytes b;
  b.inner = flat_all_bytes(ix, by, n_users * n_vec, fetch, false, &L);
  b.stage_off = (b.inner + 255) & ~(size_t)255;
  b.union_off = b.stage_off + flat_multi_stage_bytes(n_users * n_vec, fetch);
  b.total = b.union_off + fuse_ws_bytes((long long)n_users, (long long)n_vec * fetch);
  return b;
}

static int flat_all_multi_fused(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_users, int32_t n_vec,
                                int32_t fetch, int32_t k, const nann_fusion* fusion, int64_t* out_item_ids, float* out_scores,
                                int32_t* out_index, uint64_t* out_lists, int32_t* n_out, void* workspace, int64_t workspace_bytes,
                                const nann_search_options* options, nann_stream_t stream, const char* who) {
  FlatBy by;
  int rc = flat_all_multi_fused_check(ix, scorer, n_users, n_vec, fetch, k, who, &by);
  if (rc) return rc;
  rc = fusion_check(fusion, who);
  if (rc) return rc;
  if (n_users == 0 || k == 0) return NANN_OK;
  if (!q || !out_item_ids) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  rc = check_options(options);
  if (rc) return rc;
  const FlatMultiBytes b = flat_all_multi_fused_bytes(ix, by, n_users, n_vec, fetch);
  rc = flat_workspace(workspace, workspace_bytes, b.total, who, "");
  if (rc) return rc;
  const int64_t n = n_users * n_vec;
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  int64_t* s_ids = reinterpret_cast<int64_t*>(ws + b.stage_off);
  float* s_scores = reinterpret_cast<float*>(ws + b.stage_off + (size_t)n * fetch * 8);
  int32_t* s_rows = reinterpret_cast<int32_t*>(ws + b.stage_off + (size_t)n * fetch * 12);
  rc = flat_all(ix, scorer, nullptr, q, n, fetch, s_ids, s_scores, s_rows, workspace, (int64_t)b.inner, options, false, nullptr, nullptr,
                stream, "nann_search_all");
  if (rc) return rc;
  FuseArgs a = {};
  a.scores = s_scores;
  a.rows = s_rows;
  a.n_lists = n_vec;
  a.k_in = fetch;
  a.k = k;
  flat_ids_of(ix, &a);
  fusion_into(fusion, &a);
  a.ws = ws + b.union_off;
  a.out_index = out_index;
  a.out_scores = out_scores;
  a.out_item_ids = out_item_ids;
  a.out_lists = reinterpret_cast<unsigned long long*>(out_lists);
  a.n_out = n_out;
  return launch_fuse_topk(a, (long long)n_users, as_stream(stream));
}

// ---- exhaustive search under a group cap: flat_all, filtered, at k = the fetch width F into a staging list, then the cap ------
// workspace: [flat_all's filtered workspace at k = F, rounded up to 256 | item ids i64[n, F], scores f32[n, F], rows i32[n, F],
// n_out i32[n], rounded up]
struct FlatGroupedBytes {
  size_t inner, stage_off, total;
};
static int flat_all_grouped_check(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, int64_t n, int32_t fetch,
                                  const char* who, FlatBy* by) {
  const int rc = flat_check(ix, scorer, m, n, fetch, false, 0, who, by);  // (nann_search_all's checks, held against F)
  if (rc) return rc;
  if (n > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": too many " + by->unit + " in one call");
  return NANN_OK;
}
static FlatGroupedBytes flat_all_grouped_bytes(const nann_index* ix, const FlatBy& by, int64_t n, int32_t fetch) {
  ScanLayout L;
  FlatGroupedBytes b;
  b.inner = flat_all_bytes(ix, by, n, fetch, true, &L);
  b.stage_off = (b.inner + 255) & ~(size_t)255;
  b.total = b.stage_off + (((size_t)n * (size_t)fetch * 16 + (size_t)n * 4 + 255) & ~(size_t)255);
  return b;
}
static int flat_all_grouped_size(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, int64_t n, int32_t fetch,
                                 int64_t* nbytes, const char* who) {
  if (!nbytes) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  FlatBy by;
  const int rc = flat_all_grouped_check(ix, scorer, m, n, fetch, who, &by);
  if (rc) return rc;
  *nbytes = n == 0 || fetch == 0 ? 0 : (int64_t)flat_all_grouped_bytes(ix, by, n, fetch).total;
  return NANN_OK;
}

static int flat_all_grouped(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, const void* x, int64_t n,
                            int32_t fetch, int32_t k, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                            int32_t* out_group, void* workspace, int64_t workspace_bytes, const nann_search_options* options,
                            const nann_filter* filter, const nann_groups* groups, int32_t* n_out, nann_stream_t stream,
                            const char* who, const char* inner_who) {
  FlatBy by;
  int rc = flat_all_grouped_check(ix, scorer, m, n, fetch, who, &by);
  if (rc) return rc;
  if (k < 0 || k > fetch) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": k must lie in [0, fetch]");
  GroupCapArgs a = {};
  rc = resolve_groups(groups, who, &a);
  if (rc) return rc;
  if (n == 0 || k == 0) return NANN_OK;
  if (!x || !out_item_ids) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  rc = check_options(options);
  if (rc) return rc;
  rc = resolve_filter(filter, ix, &a.f);  // (a malformed filter fails the call here; the inner search resolves it for itself)
  if (rc) return rc;
  const FlatGroupedBytes b = flat_all_grouped_bytes(ix, by, n, fetch);
  rc = flat_workspace(workspace, workspace_bytes, b.total, who, "");
  if (rc) return rc;
  unsigned char* stage = static_cast<unsigned char*>(workspace) + b.stage_off;
  int64_t* s_ids = reinterpret_cast<int64_t*>(stage);
  float* s_scores = reinterpret_cast<float*>(stage + (size_t)n * fetch * 8);
  int32_t* s_rows = reinterpret_cast<int32_t*>(stage + (size_t)n * fetch * 12);
  int32_t* s_n = reinterpret_cast<int32_t*>(stage + (size_t)n * fetch * 16);
  rc = flat_all(ix, scorer, m, x, n, fetch, s_ids, s_scores, s_rows, workspace, (int64_t)b.inner, options, true, filter, s_n, stream,
                inner_who);
  if (rc) return rc;
  a.f = FilterArgs{};  // (the staged list holds allowed rows only: filter first, then cap)
  a.f.n_items = (long long)ix->desc.n_items;
  a.item_ids = ix->desc.item_ids;
  a.in_rows = s_rows;
  a.in_scores = s_scores;
  a.k_in = fetch;
  a.n_valid = s_n;
  a.nv_stride = 1;
  a.k = k;
  a.out_index = out_index;
  a.out_scores = out_scores;
  a.out_item_ids = out_item_ids;
  a.out_group = out_group;
  a.n_out = n_out;
  return launch_group_cap(a, (long long)n, as_stream(stream));
}

// ---- MMR re-ranking (nann_mmr.h) ---------------------------------------------------------------------------------------------
// the caller's nann_diversity into the launch arguments: null, struct_bytes, sim, lambda, in this order.  `who`: the entry point
// in a message.  Touches nothing but the struct.
int nann::resolve_diversity(const nann_diversity* dv, const char* who, MmrArgs* a) {
  if (!dv) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null nann_diversity");
  if (dv->struct_bytes != 0 && dv->struct_bytes != (int32_t)sizeof(nann_diversity)) return fail(NANN_ERR_BAD_ARGUMENT, "nann_diversity: struct_bytes");
  if (dv->sim == NANN_SCORER_MLP) return fail(NANN_ERR_UNSUPPORTED, "nann_diversity: the similarity is NANN_SCORER_L2 or NANN_SCORER_IP, not a learned scorer");
  if (dv->sim != NANN_SCORER_L2 && dv->sim != NANN_SCORER_IP) return fail(NANN_ERR_BAD_ARGUMENT, "nann_diversity: unknown sim");
  if (!(dv->lambda >= 0.0f && dv->lambda <= 1.0f)) return fail(NANN_ERR_BAD_ARGUMENT, "nann_diversity: lambda must lie in [0, 1]");
  a->metric = dv->sim == NANN_SCORER_IP ? MT_IP : MT_L2;
  a->lambda = dv->lambda;
  a->lambdas = dv->lambdas;
  return NANN_OK;
}
// the index's fields the step reads; its d against the kernel's instances
int nann::mmr_index(const nann_index* ix, const char* who, MmrArgs* a) {
  const int d = ix->desc.d;
  if (!(d == 64 || d == 128 || d == 256 || d == 512)) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": d must be 64, 128, 256 or 512");
  if (ix->desc.n_items > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": row numbers are 32-bit");
  a->emb = ix->desc.item_embs;
  a->d = d;
  a->dt = ix->desc.emb_dtype;
  a->item_ids = ix->desc.item_ids;
  a->f.n_items = (long long)ix->desc.n_items;
  return NANN_OK;
}

// ---- exhaustive search, diversified: flat_all_grouped's walk -- the same checks, workspace and staging list, the filtered
// exhaustive search at k = F -- with k_mmr in the place of the cap ------------------------------------------------------------
static int flat_all_diverse(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, const void* x, int64_t n,
                            int32_t fetch, int32_t k, int64_t* out_item_ids, float* out_scores, int32_t* out_index, float* out_mmr,
                            int32_t* out_pos, void* workspace, int64_t workspace_bytes, const nann_search_options* options,
                            const nann_filter* filter, const nann_diversity* diversity, int32_t* n_out, nann_stream_t stream,
                            const char* who, const char* inner_who) {
  FlatBy by;
  int rc = flat_all_grouped_check(ix, scorer, m, n, fetch, who, &by);
  if (rc) return rc;
  if (k < 0 || k > fetch) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": k must lie in [0, fetch]");
  MmrArgs a = {};
  rc = resolve_diversity(diversity, who, &a);
  if (rc) return rc;
  if (n == 0 || k == 0) return NANN_OK;
  if (!x || !out_item_ids) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  rc = check_options(options);
  if (rc) return rc;
  FilterArgs f;
  rc = resolve_filter(filter, ix, &f);  // (a malformed filter fails the call here; the inner search resolves it for itself)
  if (rc) return rc;
  rc = mmr_index(ix, who, &a);  // (the staged list holds allowed rows only: a.f stays empty but for n_items)
  if (rc) return rc;
  const FlatGroupedBytes b = flat_all_grouped_bytes(ix, by, n, fetch);
  rc = flat_workspace(workspace, workspace_bytes, b.total, who, "");
  if (rc) return rc;
  unsigned char* stage = static_cast<unsigned char*>(workspace) + b.stage_off;
  int64_t* s_ids = reinterpret_cast<int64_t*>(stage);
  float* s_scores = reinterpret_cast<float*>(stage + (size_t)n * fetch * 8);
  int32_t* s_rows = reinterpret_cast<int32_t*>(stage + (size_t)n * fetch * 12);
  int32_t* s_n = reinterpret_cast<int32_t*>(stage + (size_t)n * fetch * 16);
  rc = flat_all(ix, scorer, m, x, n, fetch, s_ids, s_scores, s_rows, workspace, (int64_t)b.inner, options, true, filter, s_n, stream,
                inner_who);
  if (rc) return rc;
  a.in_rows = s_rows;
  a.in_scores = s_scores;
  a.k_in = fetch;
  a.n_valid = s_n;
  a.nv_stride = 1;
  a.k = k;
  a.out_index = out_index;
  a.out_scores = out_scores;
  a.out_mmr = out_mmr;
  a.out_pos = out_pos;
  a.out_item_ids = out_item_ids;
  a.n_out = n_out;
  return launch_mmr(a, (long long)n, as_stream(stream));
}

// ---- scalar-quantised exhaustive search (nann_sq8.h): per chunk the int8 scan and nann_search_all's selection at k = fetch, the
// fetched rows in ascending order, then the candidate-list search over them at k ---------------------------------------------
// workspace: [the ScanLayout at k = fetch | Sq8Layout: the chunk's encoded queries, fetch lists, sorted lists, row_splits,
// status, and the candidate-list search's CandLayout for one chunk].  Nothing in it grows with n_queries beyond a chunk.
static int flat_sq8_check(const nann_index* ix, const nann_sq8* t, const nann_scorer* scorer, int64_t n, int32_t fetch, int32_t k,
                          const char* who, FlatBy* by) {
  if (!t) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  int rc = flat_by(ix, scorer, nullptr, who, by);
  if (rc) return rc;
  if (by->kind == NANN_SCORER_MLP)
    return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": the scorer is NANN_SCORER_L2 or NANN_SCORER_IP, not a learned scorer");
  rc = flat_check(ix, scorer, nullptr, n, fetch, false, 0, who, by);  // (nann_search_all's checks, held against fetch)
  if (rc) return rc;
  if (k < 0 || k > fetch) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": k must lie in [0, fetch]");
  if (t->uid != ix->uid || t->n_items != ix->desc.n_items || t->d != ix->desc.d)
    return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": the code table was made from another index");
  if (n > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": too many queries in one call");
  return NANN_OK;
}
static Sq8Layout flat_sq8_bytes(const nann_index* ix, const FlatBy& by, int64_t n, int32_t fetch, ScanLayout* L) {
  *L = scan_layout((long long)ix->desc.n_items, ix->desc.d, by.kind, (long long)n, fetch);
  return sq8_layout(*L, ix->desc.d, fetch, cand_layout(by.kind, L->chunk, (long long)L->chunk * fetch).total);
}

static int flat_all_sq8(const nann_index* ix, const nann_sq8* t, const nann_scorer* scorer, const float* q, int64_t n, int32_t fetch,
                        int32_t k, int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* out_fetch_index,
                        float* out_fetch_scores, void* workspace, int64_t workspace_bytes, const nann_search_options* options,
                        nann_stream_t stream, const char* who) {
  FlatBy by;
  int rc = flat_sq8_check(ix, t, scorer, n, fetch, k, who, &by);
  if (rc) return rc;
  if (n == 0 || k == 0) return NANN_OK;
  if (!q || !out_item_ids) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  rc = check_options(options);
  if (rc) return rc;
  ScanLayout L;
  const Sq8Layout S = flat_sq8_bytes(ix, by, n, fetch, &L);
  rc = flat_workspace(workspace, workspace_bytes, S.total, who, "");
  if (rc) return rc;
  DeviceInfo di;
  rc = device_info(&di);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  Sq8Args a = {};
  a.codes = t->codes;
  a.scales = t->scales;
  a.norms = t->norms;
  a.item_ids = ix->desc.item_ids;
  a.n_items = (long long)ix->desc.n_items;
  a.d = ix->desc.d;
  a.metric = by.kind == NANN_SCORER_IP ? MT_IP : MT_L2;
  CandArgs ca = {};
  flat_rows_of(ix, &ca);
  ca.cus = di.cus;
  ca.kind = by.kind;
  ca.row_splits = reinterpret_cast<const int64_t*>(ws + S.off_splits);
  ca.rows = reinterpret_cast<const int32_t*>(ws + S.off_sorted);
  int32_t* status = reinterpret_cast<int32_t*>(ws + S.off_status);  // (always 0: the lists are the fetch stage's own)
  for (int64_t c0 = 0; c0 < n; c0 += L.chunk) {
    const int n_q = (int)std::min<int64_t>(L.chunk, n - c0);
    const float* qc = q + (size_t)c0 * a.d;
    rc = launch_sq8_fetch(a, L, S, qc, n_q, fetch, ws, out_fetch_index ? out_fetch_index + (size_t)c0 * fetch : nullptr,
                          out_fetch_scores ? out_fetch_scores + (size_t)c0 * fetch : nullptr, st);
    if (rc) return rc;
    ca.n_cand = (long long)n_q * fetch;
    rc = launch_cand(ca, cand_layout(by.kind, n_q, ca.n_cand), qc, n_q, k, ws + S.off_cand, out_item_ids + (size_t)c0 * k,
                     out_scores ? out_scores + (size_t)c0 * k : nullptr, out_index ? out_index + (size_t)c0 * k : nullptr, nullptr,
                     nullptr, status, st);
    if (rc) return rc;
  }
  return NANN_OK;
}

// ---- the certified form (nann_search_all_sq8_exact; nann_sq8.h) -----------------------------------------------
// Per chunk: flat_all_sq8's two steps with the result kept in the workspace (stage a), the survivor pass over the score buffer
// the scan has left in the ScanLayout (stage b), and the candidate-list search over the final lists (stage c).
// workspace: Sq8ExactLayout.  Nothing in it grows with n_queries beyond a chunk.
static int flat_sq8_exact_check(const nann_index* ix, const nann_sq8* t, const nann_sq8_bounds* b, const nann_scorer* scorer, int64_t n,
                                int32_t fetch, int64_t cap, int32_t k, const char* who, FlatBy* by, ScanLayout* L, Sq8ExactLayout* X) {
  if (!b) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  int rc = flat_sq8_check(ix, t, scorer, n, fetch, k, who, by);
  if (rc) return rc;
  if (b->uid != ix->uid || b->serial != t->serial || b->n_items != t->n_items)
    return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": the bounds were made from another index or code table");
  if (cap < fetch) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": cap must be at least fetch");
  *L = scan_layout((long long)ix->desc.n_items, ix->desc.d, by->kind, (long long)n, fetch);
  if (cap > cand_max_list(L->chunk))  // (a chunk's final lists are one candidate-list search)
    return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": cap beyond the longest list of a candidate-list search, " +
                                          std::to_string(cand_max_list(L->chunk)) + " at this chunk");
  *X = sq8_exact_layout(*L, by->kind, ix->desc.d, fetch, (long long)cap, k, (long long)ix->desc.n_items);
  return NANN_OK;
}

static int flat_all_sq8_exact(const nann_index* ix, const nann_sq8* t, const nann_sq8_bounds* b, const nann_scorer* scorer,
                              const float* q, int64_t n, int32_t fetch, int64_t cap, int32_t k, int64_t* out_item_ids,
                              float* out_scores, int32_t* out_index, int32_t* out_certified, int32_t* out_n_survivors,
                              void* workspace, int64_t workspace_bytes, const nann_search_options* options, nann_stream_t stream,
                              const char* who) {
  FlatBy by;
  ScanLayout L;
  Sq8ExactLayout X;
  int rc = flat_sq8_exact_check(ix, t, b, scorer, n, fetch, cap, k, who, &by, &L, &X);
  if (rc) return rc;
  if (n == 0 || k == 0) return NANN_OK;
  if (!q || !out_item_ids || !out_certified || !out_n_survivors) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  rc = check_options(options);
  if (rc) return rc;
  rc = flat_workspace(workspace, workspace_bytes, X.total, who, "");
  if (rc) return rc;
  DeviceInfo di;
  rc = device_info(&di);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  const Sq8Layout& S = X.S;
  Sq8Args a = {};
  a.codes = t->codes;
  a.scales = t->scales;
  a.norms = t->norms;
  a.item_ids = ix->desc.item_ids;
  a.n_items = (long long)ix->desc.n_items;
  a.d = ix->desc.d;
  a.metric = by.kind == NANN_SCORER_IP ? MT_IP : MT_L2;
  CandArgs ca = {};
  flat_rows_of(ix, &ca);
  ca.cus = di.cus;
  ca.kind = by.kind;
  int32_t* status = reinterpret_cast<int32_t*>(ws + S.off_status);  // (always 0: the lists are the call's own)
  for (int64_t c0 = 0; c0 < n; c0 += L.chunk) {
    const int n_q = (int)std::min<int64_t>(L.chunk, n - c0);
    const float* qc = q + (size_t)c0 * a.d;
    // (a) the fetch stage and its exact re-rank, as nann_search_all_sq8 runs them; the result stays in the workspace
    rc = launch_sq8_fetch(a, L, S, qc, n_q, fetch, ws, nullptr, nullptr, st);
    if (rc) return rc;
    ca.row_splits = reinterpret_cast<const int64_t*>(ws + S.off_splits);
    ca.rows = reinterpret_cast<const int32_t*>(ws + S.off_sorted);
    ca.n_cand = (long long)n_q * fetch;
    rc = launch_cand(ca, cand_layout(by.kind, n_q, ca.n_cand), qc, n_q, k, ws + S.off_cand,
                     reinterpret_cast<int64_t*>(ws + X.off_a_ids), reinterpret_cast<float*>(ws + X.off_a_scores), nullptr, nullptr,
                     nullptr, status, st);
    if (rc) return rc;
    // (b) the survivors of every query, or its fetch list, as compact lists in ascending row order
    rc = launch_sq8_survivors(a, L, X, qc, b->err, b->xhat, n_q, fetch, k, ws, out_certified + c0, out_n_survivors + c0, st);
    if (rc) return rc;
    // (c) the exact top k of the lists
    ca.row_splits = reinterpret_cast<const int64_t*>(ws + X.off_xsplits);
    ca.rows = reinterpret_cast<const int32_t*>(ws + X.off_rows);
    ca.n_cand = (long long)n_q * X.cap;
    rc = launch_cand(ca, cand_layout(by.kind, n_q, ca.n_cand), qc, n_q, k, ws + S.off_cand, out_item_ids + (size_t)c0 * k,
                     out_scores ? out_scores + (size_t)c0 * k : nullptr, out_index ? out_index + (size_t)c0 * k : nullptr, nullptr,
                     nullptr, status, st);
    if (rc) return rc;
  }
  return NANN_OK;
}

// ---- the certified range form (nann_search_all_range_sq8_exact; nann_sq8.h) ------------------------------------
// The caller's threshold is the cut: per chunk the int8 scan and the survivor pass at tau = thresholds[q], the candidate-list
// search's scorer over the survivor lists, and the ragged selection over those exact scores.  No fetch stage, no top-k.
// workspace: Sq8RangeLayout behind the ScanLayout at k = 0.  Nothing in it grows with n_queries beyond a chunk.
static int flat_sq8_range_check(const nann_index* ix, const nann_sq8* t, const nann_sq8_bounds* b, const nann_scorer* scorer, int64_t n,
                                int64_t cap, const char* who, FlatBy* by, ScanLayout* L, Sq8RangeLayout* R) {
  if (ix && ix->desc.emb_dtype == NANN_F32) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": 16-bit rows (f16, bf16) only");
  if (!b) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  int rc = flat_sq8_check(ix, t, scorer, n, 0, 0, who, by);  // (nann_search_all_range's checks of the shape: there is no k)
  if (rc) return rc;
  if (b->uid != ix->uid || b->serial != t->serial || b->n_items != t->n_items)
    return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": the bounds were made from another index or code table");
  if (cap < 1) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": cap must be at least 1");
  *L = scan_layout((long long)ix->desc.n_items, ix->desc.d, by->kind, (long long)n, 0);
  if (cap > cand_max_list(L->chunk))  // (a chunk's survivor lists are one candidate-list plan)
    return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": cap beyond the longest list of a candidate-list search, " +
                                          std::to_string(cand_max_list(L->chunk)) + " at this chunk");
  *R = sq8_range_layout(*L, by->kind, ix->desc.d, (long long)cap, (long long)ix->desc.n_items);
  return NANN_OK;
}

static int flat_range_sq8_exact(const nann_index* ix, const nann_sq8* t, const nann_sq8_bounds* b, const nann_scorer* scorer,
                                const float* q, int64_t n, const float* thresholds, int64_t cap, int64_t capacity,
                                int64_t* out_row_splits, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                                int32_t* out_certified, int32_t* out_n_survivors, void* workspace, int64_t workspace_bytes,
                                const nann_search_options* options, nann_stream_t stream, const char* who) {
  FlatBy by;
  ScanLayout L;
  Sq8RangeLayout R;
  int rc = flat_sq8_range_check(ix, t, b, scorer, n, cap, who, &by, &L, &R);
  if (rc) return rc;
  if (capacity < 0) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": capacity < 0");
  if (n == 0) return NANN_OK;
  if (!q || !thresholds || !out_row_splits || !out_certified || !out_n_survivors)
    return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  if (capacity > 0 && !out_item_ids) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": out_item_ids is null while capacity > 0");
  rc = check_options(options);
  if (rc) return rc;
  rc = flat_workspace(workspace, workspace_bytes, R.total, who, "");
  if (rc) return rc;
  DeviceInfo di;
  rc = device_info(&di);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  Sq8Args a = {};
  a.codes = t->codes;
  a.scales = t->scales;
  a.norms = t->norms;
  a.item_ids = ix->desc.item_ids;
  a.n_items = (long long)ix->desc.n_items;
  a.d = ix->desc.d;
  a.metric = by.kind == NANN_SCORER_IP ? MT_IP : MT_L2;
  CandArgs ca = {};
  flat_rows_of(ix, &ca);
  ca.cus = di.cus;
  ca.kind = by.kind;
  ca.row_splits = reinterpret_cast<const int64_t*>(ws + R.off_xsplits);
  ca.rows = reinterpret_cast<const int32_t*>(ws + R.off_rows);
  for (int64_t c0 = 0; c0 < n; c0 += L.chunk) {
    const int n_q = (int)std::min<int64_t>(L.chunk, n - c0);
    const float* qc = q + (size_t)c0 * a.d;
    // the survivors of every certified query as compact lists in ascending row order; an uncertified query's list is empty
    rc = launch_sq8_range_survivors(a, L, R, qc, thresholds + c0, b->err, b->xhat, n_q, ws, out_certified + c0, out_n_survivors + c0, st);
    if (rc) return rc;
    // their exact scores, by list position
    ca.n_cand = (long long)n_q * R.cap;
    const CandLayout CL = cand_layout(by.kind, n_q, ca.n_cand);
    rc = launch_cand_scores(ca, CL, qc, n_q, ws + R.off_cand, st);
    if (rc) return rc;
    // the rows at or above the threshold, into the caller's ragged outputs
    rc = launch_sq8_range_select(a, R, R.off_cand + CL.off_scores, thresholds, (long long)c0, n_q, (long long)capacity, ws,
                                 out_row_splits, out_item_ids, out_scores, out_index, st);
    if (rc) return rc;
  }
  return NANN_OK;
}

// ---- the entry points (include/nann_hip.h) -----------------------------------------------------------------------------------
extern "C" {

int nann_mmr_topk(const nann_index* ix, const float* scores, const int32_t* rows, const int32_t* n_valid, int64_t n_queries,
                  int32_t k_in, const nann_diversity* diversity, int32_t k, int32_t* out_index, float* out_scores,
                  float* out_mmr, int32_t* out_pos, int64_t* out_item_ids, int32_t* n_out, nann_stream_t stream) {
  const char* who = "nann_mmr_topk";
  if (n_queries < 0 || k_in < 0) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": negative size");
  if (k < 0) return flat_bad_k(k);
  if (k > k_in) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": k exceeds the k_in entries a query brings");
  if (k_in > kMaxK) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": k_in <= 1024");
  if (n_queries > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": too many queries in one call");
  MmrArgs a = {};
  int rc = resolve_diversity(diversity, who, &a);
  if (rc) return rc;
  if (n_queries == 0 || k == 0) return NANN_OK;
  if (!ix || !scores || !rows || !out_index) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  rc = mmr_index(ix, who, &a);  // (the first read of the index)
  if (rc) return rc;
  a.in_rows = rows;
  a.in_scores = scores;
  a.k_in = k_in;
  a.n_valid = n_valid;
  a.nv_stride = 1;
  a.k = k;
  a.out_index = out_index;
  a.out_scores = out_scores;
  a.out_mmr = out_mmr;
  a.out_pos = out_pos;
  a.out_item_ids = out_item_ids;
  a.n_out = n_out;
  return launch_mmr(a, (long long)n_queries, as_stream(stream));
}

int nann_search_all_diverse_workspace_bytes(const nann_index* ix, const nann_scorer* scorer, int64_t n_queries, int32_t fetch,
                                            int64_t* nbytes) {
  return flat_all_grouped_size(ix, scorer, nullptr, n_queries, fetch, nbytes, "nann_search_all_diverse_workspace_bytes");
}
int nann_search_all_diverse(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries, int32_t fetch,
                            int32_t k, int64_t* out_item_ids, float* out_scores, int32_t* out_index, float* out_mmr,
                            int32_t* out_pos, void* workspace, int64_t workspace_bytes, const nann_search_options* options,
                            const nann_filter* filter, const nann_diversity* diversity, int32_t* n_out, nann_stream_t stream) {
  return flat_all_diverse(ix, scorer, nullptr, q, n_queries, fetch, k, out_item_ids, out_scores, out_index, out_mmr, out_pos,
                          workspace, workspace_bytes, options, filter, diversity, n_out, stream, "nann_search_all_diverse",
                          "nann_search_all");
}
int nann_search_all_model_diverse_workspace_bytes(const nann_index* ix, const nann_model* m, int64_t n_users, int32_t fetch,
                                                  int64_t* nbytes) {
  return flat_all_grouped_size(ix, nullptr, m, n_users, fetch, nbytes, "nann_search_all_model_diverse_workspace_bytes");
}
int nann_search_all_model_diverse(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_users,
                                  int32_t fetch, int32_t k, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                                  float* out_mmr, int32_t* out_pos, void* workspace, int64_t workspace_bytes,
                                  const nann_search_options* options, const nann_filter* filter,
                                  const nann_diversity* diversity, int32_t* n_out, nann_stream_t stream) {
  if (!m) return fail(NANN_ERR_BAD_ARGUMENT, "nann_search_all_model_diverse: null argument");
  return flat_all_diverse(ix, nullptr, m, comm_seq_f16, n_users, fetch, k, out_item_ids, out_scores, out_index, out_mmr, out_pos,
                          workspace, workspace_bytes, options, filter, diversity, n_out, stream, "nann_search_all_model_diverse",
                          "nann_search_all_model");
}

int nann_group_cap_topk(const float* scores, const int32_t* rows, const int32_t* n_valid, int64_t n_queries, int32_t k_in,
                        int64_t n_items, const int64_t* item_ids, const nann_groups* groups, const nann_filter* filter, int32_t k,
                        int32_t* out_index, float* out_scores, int64_t* out_item_ids, int32_t* out_group, int32_t* out_pos,
                        int32_t* n_out, nann_stream_t stream) {
  const char* who = "nann_group_cap_topk";
  if (n_queries < 0 || k_in < 0 || n_items < 0) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": negative size");
  if (k < 0) return flat_bad_k(k);
  if (k > k_in) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": k exceeds the k_in entries a query brings");
  if (k_in > kMaxK) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": k_in <= 1024");
  if (n_queries > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": too many queries in one call");
  if (n_items > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": row numbers are 32-bit");
  GroupCapArgs a = {};
  int rc = resolve_groups(groups, who, &a);
  if (rc) return rc;
  if (n_queries == 0 || k == 0) return NANN_OK;
  if (!rows || !out_index) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  if (out_item_ids && !item_ids) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": out_item_ids without item_ids");
  rc = resolve_filter_rows(filter, (long long)n_items, &a.f);
  if (rc) return rc;
  a.in_rows = rows;
  a.in_scores = scores;
  a.k_in = k_in;
  a.n_valid = n_valid;
  a.nv_stride = 1;
  a.k = k;
  a.item_ids = item_ids;
  a.out_index = out_index;
  a.out_scores = out_scores;
  a.out_item_ids = out_item_ids;
  a.out_group = out_group;
  a.out_pos = out_pos;
  a.n_out = n_out;
  return launch_group_cap(a, (long long)n_queries, as_stream(stream));
}

int nann_search_all_grouped_workspace_bytes(const nann_index* ix, const nann_scorer* scorer, int64_t n_queries, int32_t fetch,
                                            int64_t* nbytes) {
  return flat_all_grouped_size(ix, scorer, nullptr, n_queries, fetch, nbytes, "nann_search_all_grouped_workspace_bytes");
}
int nann_search_all_grouped(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries, int32_t fetch,
                            int32_t k, int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* out_group,
                            void* workspace, int64_t workspace_bytes, const nann_search_options* options,
                            const nann_filter* filter, const nann_groups* groups, int32_t* n_out, nann_stream_t stream) {
  return flat_all_grouped(ix, scorer, nullptr, q, n_queries, fetch, k, out_item_ids, out_scores, out_index, out_group, workspace,
                          workspace_bytes, options, filter, groups, n_out, stream, "nann_search_all_grouped", "nann_search_all");
}
int nann_search_all_model_grouped_workspace_bytes(const nann_index* ix, const nann_model* m, int64_t n_users, int32_t fetch,
                                                  int64_t* nbytes) {
  return flat_all_grouped_size(ix, nullptr, m, n_users, fetch, nbytes, "nann_search_all_model_grouped_workspace_bytes");
}
int nann_search_all_model_grouped(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_users,
                                  int32_t fetch, int32_t k, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                                  int32_t* out_group, void* workspace, int64_t workspace_bytes,
                                  const nann_search_options* options, const nann_filter* filter, const nann_groups* groups,
                                  int32_t* n_out, nann_stream_t stream) {
  if (!m) return fail(NANN_ERR_BAD_ARGUMENT, "nann_search_all_model_grouped: null argument");
  return flat_all_grouped(ix, nullptr, m, comm_seq_f16, n_users, fetch, k, out_item_ids, out_scores, out_index, out_group, workspace,
                          workspace_bytes, options, filter, groups, n_out, stream, "nann_search_all_model_grouped",
                          "nann_search_all_model");
}

int nann_union_topk_workspace_bytes(int64_t n_users, int32_t n_lists, int32_t k_in, int64_t* nbytes) {
  if (!nbytes) return fail(NANN_ERR_BAD_ARGUMENT, "nann_union_topk_workspace_bytes: null argument");
  const int rc = union_check(n_users, n_lists, k_in, 0, "nann_union_topk_workspace_bytes");
  if (rc) return rc;
  *nbytes = (int64_t)union_ws_bytes((long long)n_users, (long long)n_lists * k_in);
  return NANN_OK;
}
int nann_union_topk(const float* scores, const int32_t* rows, const int32_t* n_valid, int64_t n_users, int32_t n_lists,
                    int32_t k_in, int64_t n_items, const int64_t* item_ids, int32_t k, int32_t* out_index, float* out_scores,
                    int64_t* out_item_ids, int32_t* out_list, int32_t* n_out, void* workspace, int64_t workspace_bytes,
                    nann_stream_t stream) {
  const char* who = "nann_union_topk";
  if (n_items < 0) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": negative size");
  const int rc = union_check(n_users, n_lists, k_in, k, who);
  if (rc) return rc;
  if (n_items > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": row numbers are 32-bit");
  if (n_users == 0 || k == 0) return NANN_OK;
  if (!scores || !rows || !out_index) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  if (out_item_ids && !item_ids) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": out_item_ids without item_ids");
  const int rw = flat_workspace(workspace, workspace_bytes, union_ws_bytes((long long)n_users, (long long)n_lists * k_in), who, "");
  if (rw) return rw;
  UnionArgs a = {};
  a.scores = scores;
  a.rows = rows;
  a.n_valid = n_valid;
  a.nv_stride = 1;
  a.n_lists = n_lists;
  a.k_in = k_in;
  a.k = k;
  a.n_items = (long long)n_items;
  a.item_ids = item_ids;
  a.best = static_cast<unsigned long long*>(workspace);
  a.out_index = out_index;
  a.out_scores = out_scores;
  a.out_item_ids = out_item_ids;
  a.out_list = out_list;
  a.n_out = n_out;
  return launch_union_topk(a, (long long)n_users, as_stream(stream));
}

int nann_search_all_multi_workspace_bytes(const nann_index* ix, const nann_scorer* scorer, int64_t n_users, int32_t n_vec,
                                          int32_t k, int64_t* nbytes) {
  const char* who = "nann_search_all_multi_workspace_bytes";
  if (!nbytes) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  FlatBy by;
  const int rc = flat_all_multi_check(ix, scorer, n_users, n_vec, k, who, &by);
  if (rc) return rc;
  *nbytes = n_users == 0 || k == 0 ? 0 : (int64_t)flat_all_multi_bytes(ix, by, n_users, n_vec, k).total;
  return NANN_OK;
}
int nann_search_all_multi(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_users, int32_t n_vec,
                          int32_t k, int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* out_vec,
                          int32_t* n_out, void* workspace, int64_t workspace_bytes, const nann_search_options* options,
                          nann_stream_t stream) {
  return flat_all_multi(ix, scorer, q, n_users, n_vec, k, out_item_ids, out_scores, out_index, out_vec, n_out, workspace,
                        workspace_bytes, options, stream, "nann_search_all_multi");
}

int nann_fuse_topk_workspace_bytes(int64_t n_users, int32_t n_lists, int32_t k_in, int64_t* nbytes) {
  if (!nbytes) return fail(NANN_ERR_BAD_ARGUMENT, "nann_fuse_topk_workspace_bytes: null argument");
  const int rc = fuse_shape_check(n_users, n_lists, k_in, 0, "nann_fuse_topk_workspace_bytes");
  if (rc) return rc;
  *nbytes = (int64_t)fuse_ws_bytes((long long)n_users, (long long)n_lists * k_in);
  return NANN_OK;
}
int nann_fuse_topk(const float* scores, const int32_t* rows, const int32_t* n_valid, int64_t n_users, int32_t n_lists,
                   int32_t k_in, int64_t n_items, const int64_t* item_ids, int32_t k, const nann_fusion* fusion,
                   int32_t* out_index, float* out_scores, int64_t* out_item_ids, uint64_t* out_lists, int32_t* n_out,
                   void* workspace, int64_t workspace_bytes, nann_stream_t stream) {
  const char* who = "nann_fuse_topk";
  if (n_items < 0) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": negative size");
  int rc = union_check(n_users, n_lists, k_in, k, who);
  if (rc) return rc;
  if (n_items > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": row numbers are 32-bit");
  if (n_lists > NANN_FUSE_MAX_LISTS) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": at most NANN_FUSE_MAX_LISTS = 64 lists per user");
  rc = fusion_check(fusion, who);
  if (rc) return rc;
  if (n_users == 0 || k == 0) return NANN_OK;
  if (!scores || !rows || !out_index) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  if (out_item_ids && !item_ids) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": out_item_ids without item_ids");
  rc = flat_workspace(workspace, workspace_bytes, fuse_ws_bytes((long long)n_users, (long long)n_lists * k_in), who, "");
  if (rc) return rc;
  FuseArgs a = {};
  a.scores = scores;
  a.rows = rows;
  a.n_valid = n_valid;
  a.nv_stride = 1;
  a.n_lists = n_lists;
  a.k_in = k_in;
  a.k = k;
  a.n_items = (long long)n_items;
  a.item_ids = item_ids;
  fusion_into(fusion, &a);
  a.ws = static_cast<unsigned char*>(workspace);
  a.out_index = out_index;
  a.out_scores = out_scores;
  a.out_item_ids = out_item_ids;
  a.out_lists = reinterpret_cast<unsigned long long*>(out_lists);
  a.n_out = n_out;
  return launch_fuse_topk(a, (long long)n_users, as_stream(stream));
}

int nann_search_all_multi_fused_workspace_bytes(const nann_index* ix, const nann_scorer* scorer, int64_t n_users, int32_t n_vec,
                                                int32_t fetch, int64_t* nbytes) {
  const char* who = "nann_search_all_multi_fused_workspace_bytes";
  if (!nbytes) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  FlatBy by;
  const int rc = flat_all_multi_fused_check(ix, scorer, n_users, n_vec, fetch, 0, who, &by);
  if (rc) return rc;
  *nbytes = n_users == 0 || fetch == 0 ? 0 : (int64_t)flat_all_multi_fused_bytes(ix, by, n_users, n_vec, fetch).total;
  return NANN_OK;
}
int nann_search_all_multi_fused(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_users, int32_t n_vec,
                                int32_t fetch, int32_t k, const nann_fusion* fusion, int64_t* out_item_ids, float* out_scores,
                                int32_t* out_index, uint64_t* out_lists, int32_t* n_out, void* workspace,
                                int64_t workspace_bytes, const nann_search_options* options, nann_stream_t stream) {
  return flat_all_multi_fused(ix, scorer, q, n_users, n_vec, fetch, k, fusion, out_item_ids, out_scores, out_index, out_lists, n_out,
                              workspace, workspace_bytes, options, stream, "nann_search_all_multi_fused");
}

int nann_search_all_workspace_bytes(const nann_index* ix, const nann_scorer* scorer, int64_t n_queries, int32_t k, int64_t* nbytes) {
  return flat_all_size(ix, scorer, nullptr, n_queries, k, false, nbytes, "nann_search_all_workspace_bytes");
}
int nann_search_all(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries, int32_t k,
                    int64_t* out_item_ids, float* out_scores, int32_t* out_index, void* workspace, int64_t workspace_bytes,
                    const nann_search_options* options, nann_stream_t stream) {
  return flat_all(ix, scorer, nullptr, q, n_queries, k, out_item_ids, out_scores, out_index, workspace, workspace_bytes, options,
                  false, nullptr, nullptr, stream, "nann_search_all");
}
int nann_search_all_filtered_workspace_bytes(const nann_index* ix, const nann_scorer* scorer, int64_t n_queries, int32_t k,
                                             int64_t* nbytes) {
  return flat_all_size(ix, scorer, nullptr, n_queries, k, true, nbytes, "nann_search_all_workspace_bytes");
}
int nann_search_all_filtered(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries, int32_t k,
                             int64_t* out_item_ids, float* out_scores, int32_t* out_index, void* workspace,
                             int64_t workspace_bytes, const nann_search_options* options, const nann_filter* filter,
                             int32_t* n_out, nann_stream_t stream) {
  return flat_all(ix, scorer, nullptr, q, n_queries, k, out_item_ids, out_scores, out_index, workspace, workspace_bytes, options,
                  true, filter, n_out, stream, "nann_search_all");
}

// ---- attribute predicates (nann_predicate.h): the filtered forms with the predicates resolved in front of everything else
int nann_search_all_where_workspace_bytes(const nann_index* ix, const nann_scorer* scorer, int64_t n_queries, int32_t k,
                                          int64_t* nbytes) {
  return flat_all_size(ix, scorer, nullptr, n_queries, k, true, nbytes, "nann_search_all_workspace_bytes");
}
int nann_search_all_where(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries, int32_t k,
                          int64_t* out_item_ids, float* out_scores, int32_t* out_index, void* workspace,
                          int64_t workspace_bytes, const nann_search_options* options, const nann_filter* filter,
                          const nann_predicates* predicates, int32_t* n_out, nann_stream_t stream) {
  PredArgs pa;
  const int rc = resolve_predicates(predicates, &pa);
  if (rc) return rc;
  return flat_all(ix, scorer, nullptr, q, n_queries, k, out_item_ids, out_scores, out_index, workspace, workspace_bytes, options,
                  true, filter, n_out, stream, "nann_search_all", &pa);
}
int nann_search_all_model_where_workspace_bytes(const nann_index* ix, const nann_model* m, int64_t n_users, int32_t k,
                                                int64_t* nbytes) {
  return flat_all_size(ix, nullptr, m, n_users, k, true, nbytes, "nann_search_all_model_workspace_bytes");
}
int nann_search_all_model_where(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_users,
                                int32_t k, int64_t* out_item_ids, float* out_scores, int32_t* out_index, void* workspace,
                                int64_t workspace_bytes, const nann_search_options* options, const nann_filter* filter,
                                const nann_predicates* predicates, int32_t* n_out, nann_stream_t stream) {
  PredArgs pa;
  const int rc = resolve_predicates(predicates, &pa);
  if (rc) return rc;
  return flat_all(ix, nullptr, m, comm_seq_f16, n_users, k, out_item_ids, out_scores, out_index, workspace, workspace_bytes,
                  options, true, filter, n_out, stream, "nann_search_all_model", &pa);
}

int nann_predicate_topk(const float* scores, const int32_t* rows, const int32_t* n_valid, int64_t n_queries, int32_t k_in,
                        int64_t n_items, const int64_t* item_ids, const nann_predicates* predicates, const nann_filter* filter,
                        int32_t k, int32_t* out_index, float* out_scores, int64_t* out_item_ids, int32_t* out_pos, int32_t* n_out,
                        nann_stream_t stream) {
  const char* who = "nann_predicate_topk";
  if (n_queries < 0 || k_in < 0 || n_items < 0) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": negative size");
  if (k < 0) return flat_bad_k(k);
  if (k > k_in) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": k exceeds the k_in entries a query brings");
  if (k_in > kMaxK) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": k_in <= 1024");
  if (n_queries > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": too many queries in one call");
  if (n_items > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": row numbers are 32-bit");
  PredCompactArgs a = {};
  int rc = resolve_predicates(predicates, &a.p);
  if (rc) return rc;
  if (n_queries == 0 || k == 0) return NANN_OK;
  if (!rows || !out_index) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  if (out_item_ids && !item_ids) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": out_item_ids without item_ids");
  rc = resolve_filter_rows(filter, (long long)n_items, &a.f);
  if (rc) return rc;
  a.in_rows = rows;
  a.in_scores = scores;
  a.in_stride = a.n_in = k_in;
  a.n_valid = n_valid;
  a.nv_stride = 1;
  a.k = k;
  a.item_ids = item_ids;
  a.out_index = out_index;
  a.out_scores = out_scores;
  a.out_item_ids = out_item_ids;
  a.out_pos = out_pos;
  a.n_out = n_out;
  return launch_pred_compact(a, (long long)n_queries, as_stream(stream));
}

int nann_predicate_count(int64_t n_items, const nann_predicates* predicates, const nann_filter* filter, int64_t n_queries,
                         int64_t* out_counts, nann_stream_t stream) {
  const char* who = "nann_predicate_count";
  if (n_queries < 0 || n_items < 0) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": negative size");
  if (n_items > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": row numbers are 32-bit");
  PredArgs pa;
  int rc = resolve_predicates(predicates, &pa);
  if (rc) return rc;
  FilterArgs fa;
  rc = resolve_filter_rows(filter, (long long)n_items, &fa);
  if (rc) return rc;
  if (n_queries == 0) return NANN_OK;
  if (!out_counts) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  static_assert(sizeof(long long) == sizeof(int64_t), "the counts are 64-bit");
  return launch_pred_count(fa, pa, (long long)n_queries, reinterpret_cast<long long*>(out_counts), as_stream(stream));
}

int nann_search_all_model_workspace_bytes(const nann_index* ix, const nann_model* m, int64_t n_users, int32_t k, int64_t* nbytes) {
  return flat_all_size(ix, nullptr, m, n_users, k, false, nbytes, "nann_search_all_model_workspace_bytes");
}
int nann_search_all_model(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_users, int32_t k,
                          int64_t* out_item_ids, float* out_scores, int32_t* out_index, void* workspace, int64_t workspace_bytes,
                          const nann_search_options* options, nann_stream_t stream) {
  return flat_all(ix, nullptr, m, comm_seq_f16, n_users, k, out_item_ids, out_scores, out_index, workspace, workspace_bytes,
                  options, false, nullptr, nullptr, stream, "nann_search_all_model");
}
int nann_search_all_model_filtered_workspace_bytes(const nann_index* ix, const nann_model* m, int64_t n_users, int32_t k,
                                                   int64_t* nbytes) {
  return flat_all_size(ix, nullptr, m, n_users, k, true, nbytes, "nann_search_all_model_workspace_bytes");
}
int nann_search_all_model_filtered(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_users,
                                   int32_t k, int64_t* out_item_ids, float* out_scores, int32_t* out_index, void* workspace,
                                   int64_t workspace_bytes, const nann_search_options* options, const nann_filter* filter,
                                   int32_t* n_out, nann_stream_t stream) {
  return flat_all(ix, nullptr, m, comm_seq_f16, n_users, k, out_item_ids, out_scores, out_index, workspace, workspace_bytes,
                  options, true, filter, n_out, stream, "nann_search_all_model");
}

int nann_search_all_range_workspace_bytes(const nann_index* ix, const nann_scorer* scorer, int64_t n_queries, int64_t* nbytes) {
  return flat_range_size(ix, scorer, nullptr, n_queries, nbytes, "nann_search_all_range_workspace_bytes");
}
int nann_search_all_range(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries, const float* thresholds,
                          int64_t capacity, int64_t* out_row_splits, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                          void* workspace, int64_t workspace_bytes, const nann_search_options* options, const nann_filter* filter,
                          nann_stream_t stream) {
  return flat_range(ix, scorer, nullptr, q, n_queries, thresholds, capacity, out_row_splits, out_item_ids, out_scores, out_index,
                    workspace, workspace_bytes, options, filter, stream, "nann_search_all_range");
}
int nann_search_all_range_model_workspace_bytes(const nann_index* ix, const nann_model* m, int64_t n_users, int64_t* nbytes) {
  return flat_range_size(ix, nullptr, m, n_users, nbytes, "nann_search_all_range_model_workspace_bytes");
}
int nann_search_all_range_model(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_users,
                                const float* thresholds, int64_t capacity, int64_t* out_row_splits, int64_t* out_item_ids,
                                float* out_scores, int32_t* out_index, void* workspace, int64_t workspace_bytes,
                                const nann_search_options* options, const nann_filter* filter, nann_stream_t stream) {
  return flat_range(ix, nullptr, m, comm_seq_f16, n_users, thresholds, capacity, out_row_splits, out_item_ids, out_scores,
                    out_index, workspace, workspace_bytes, options, filter, stream, "nann_search_all_range_model");
}

// ---- wide exhaustive search (nann_wide.h)
int nann_search_all_wide_workspace_bytes(const nann_index* ix, const nann_scorer* scorer, int64_t n_queries, int32_t k, int64_t* nbytes) {
  return flat_wide_size(ix, scorer, nullptr, n_queries, k, nbytes, "nann_search_all_wide_workspace_bytes");
}
int nann_search_all_wide(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries, int32_t k,
                         int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* n_out, void* workspace,
                         int64_t workspace_bytes, const nann_search_options* options, const nann_filter* filter,
                         const nann_predicates* predicates, nann_stream_t stream) {
  return flat_wide(ix, scorer, nullptr, q, n_queries, k, out_item_ids, out_scores, out_index, n_out, workspace, workspace_bytes,
                   options, filter, predicates, stream, "nann_search_all_wide");
}
int nann_search_all_model_wide_workspace_bytes(const nann_index* ix, const nann_model* m, int64_t n_users, int32_t k, int64_t* nbytes) {
  return flat_wide_size(ix, nullptr, m, n_users, k, nbytes, "nann_search_all_model_wide_workspace_bytes");
}
int nann_search_all_model_wide(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_users, int32_t k,
                               int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* n_out, void* workspace,
                               int64_t workspace_bytes, const nann_search_options* options, const nann_filter* filter,
                               const nann_predicates* predicates, nann_stream_t stream) {
  return flat_wide(ix, nullptr, m, comm_seq_f16, n_users, k, out_item_ids, out_scores, out_index, n_out, workspace, workspace_bytes,
                   options, filter, predicates, stream, "nann_search_all_model_wide");
}
int nann_select_wide_workspace_bytes(int64_t n_rows, int64_t n_cols, int32_t k, int64_t* nbytes) {
  const char* who = "nann_select_wide_workspace_bytes";
  if (!nbytes) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  const int rc = select_wide_check(n_rows, n_cols, k, who);
  if (rc) return rc;
  *nbytes = n_rows == 0 || k == 0 ? 0 : (int64_t)wide_bytes(select_wide_chunk(n_rows, n_cols), (long long)n_cols, k);
  return NANN_OK;
}
int nann_select_wide(const float* values, int64_t n_rows, int64_t n_cols, int32_t k, float* out_values, int32_t* out_indices,
                     int32_t* n_out, void* workspace, int64_t workspace_bytes, nann_stream_t stream) {
  const char* who = "nann_select_wide";
  int rc = select_wide_check(n_rows, n_cols, k, who);
  if (rc) return rc;
  if (n_rows == 0 || k == 0) return NANN_OK;
  if (!values || !out_indices) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  if (reinterpret_cast<uintptr_t>(values) & 15u) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": values must be 16-byte aligned");
  const int chunk = select_wide_chunk(n_rows, n_cols);
  rc = flat_workspace(workspace, workspace_bytes, wide_bytes(chunk, (long long)n_cols, k), who, "");
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  const size_t limit = (size_t)n_rows * (size_t)n_cols;
  for (int64_t r0 = 0; r0 < n_rows; r0 += chunk) {
    const int n_q = (int)std::min<int64_t>(chunk, n_rows - r0);
    const ScanWide w = wide_carve(static_cast<unsigned char*>(workspace), chunk, (long long)n_cols, k, nullptr);
    rc = launch_wide(w, values, limit, (long long)n_cols, (long long)r0, n_q, nullptr, nullptr, out_values ? out_values + (size_t)r0 * k : nullptr,
                     out_indices + (size_t)r0 * k, n_out ? n_out + r0 : nullptr, st);
    if (rc) return rc;
  }
  return NANN_OK;
}

int nann_search_candidates_workspace_bytes(const nann_index* ix, const nann_scorer* scorer, int64_t n_queries, int64_t n_cand,
                                           int32_t k, int64_t* nbytes) {
  return flat_cand_size(ix, scorer, nullptr, n_queries, n_cand, k, nbytes, "nann_search_candidates_workspace_bytes");
}
int nann_search_candidates(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries, int32_t k,
                           const nann_candidates* cand, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                           int32_t* out_pos, int32_t* n_out, int32_t* status, void* workspace, int64_t workspace_bytes,
                           const nann_search_options* options, nann_stream_t stream) {
  return flat_cand(ix, scorer, nullptr, q, n_queries, k, cand, out_item_ids, out_scores, out_index, out_pos, n_out, status,
                   workspace, workspace_bytes, options, stream, "nann_search_candidates");
}
int nann_search_candidates_model_workspace_bytes(const nann_index* ix, const nann_model* m, int64_t n_users, int64_t n_cand,
                                                 int32_t k, int64_t* nbytes) {
  return flat_cand_size(ix, nullptr, m, n_users, n_cand, k, nbytes, "nann_search_candidates_model_workspace_bytes");
}
int nann_search_candidates_model(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_users, int32_t k,
                                 const nann_candidates* cand, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                                 int32_t* out_pos, int32_t* n_out, int32_t* status, void* workspace, int64_t workspace_bytes,
                                 const nann_search_options* options, nann_stream_t stream) {
  return flat_cand(ix, nullptr, m, comm_seq_f16, n_users, k, cand, out_item_ids, out_scores, out_index, out_pos, n_out, status,
                   workspace, workspace_bytes, options, stream, "nann_search_candidates_model");
}

// ---- the int8 code table and the search over it (nann_sq8.h) ---------------------------------------------------------------
int nann_sq8_create(const nann_index* ix, nann_stream_t stream, nann_sq8** out) {
  const char* who = "nann_sq8_create";
  if (!ix || !out) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  *out = nullptr;
  const int d = ix->desc.d, dt = ix->desc.emb_dtype;
  if (dt != NANN_F16 && dt != NANN_BF16) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": 16-bit rows (f16, bf16) only");
  if (!(d == 64 || d == 128 || d == 256 || d == 512)) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": d must be 64, 128, 256 or 512");
  if (ix->desc.n_items > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": row numbers are 32-bit");
  std::unique_ptr<nann_sq8, void (*)(nann_sq8*)> t(new nann_sq8(), nann_sq8_destroy);
  static std::atomic<uint64_t> next_serial{1};
  t->uid = ix->uid;
  t->serial = next_serial.fetch_add(1);
  t->n_items = ix->desc.n_items;
  t->d = d;
  const size_t n = (size_t)std::max<int64_t>(t->n_items, 1);  // (an empty index: one element each, never read)
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t->codes), n * d));
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t->scales), n * 4));
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t->norms), n * 4));
  t->bytes = (int64_t)(n * d + n * 8);
  const int rc = launch_sq8_encode(ix->desc.item_embs, dt, (long long)t->n_items, d, t->codes, t->scales, t->norms, as_stream(stream));
  if (rc) return rc;
  *out = t.release();
  return NANN_OK;
}
void nann_sq8_destroy(nann_sq8* t) {
  if (!t) return;
  if (t->codes) (void)hipFree(t->codes);
  if (t->scales) (void)hipFree(t->scales);
  if (t->norms) (void)hipFree(t->norms);
  delete t;
}
int nann_sq8_info(const nann_sq8* t, int64_t out[4]) {
  if (!t || !out) return fail(NANN_ERR_BAD_ARGUMENT, "nann_sq8_info: null argument");
  out[0] = t->n_items;
  out[1] = t->d;
  out[2] = t->bytes;
  out[3] = 0;
  return NANN_OK;
}
int nann_sq8_view(const nann_sq8* t, const int8_t** codes, const float** scales, const int32_t** norms) {
  if (!t) return fail(NANN_ERR_BAD_ARGUMENT, "nann_sq8_view: null argument");
  if (codes) *codes = t->codes;
  if (scales) *scales = t->scales;
  if (norms) *norms = t->norms;
  return NANN_OK;
}
int nann_sq8_encode(const float* x, int64_t n, int32_t d, int8_t* codes, float* scales, int32_t* norms, nann_stream_t stream) {
  const char* who = "nann_sq8_encode";
  if (n < 0) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": n < 0");
  if (!(d == 64 || d == 128 || d == 256 || d == 512)) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": d must be 64, 128, 256 or 512");
  if (n == 0) return NANN_OK;
  if (!x || !codes || !scales || !norms) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  return launch_sq8_encode(x, NANN_F32, (long long)n, d, codes, scales, norms, as_stream(stream));
}
int nann_search_all_sq8_workspace_bytes(const nann_index* ix, const nann_sq8* t, const nann_scorer* scorer, int64_t n_queries,
                                        int32_t fetch, int32_t k, int64_t* nbytes) {
  const char* who = "nann_search_all_sq8_workspace_bytes";
  if (!nbytes) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  FlatBy by;
  const int rc = flat_sq8_check(ix, t, scorer, n_queries, fetch, k, who, &by);
  if (rc) return rc;
  ScanLayout L;
  *nbytes = n_queries == 0 || k == 0 ? 0 : (int64_t)flat_sq8_bytes(ix, by, n_queries, fetch, &L).total;
  return NANN_OK;
}
int nann_search_all_sq8(const nann_index* ix, const nann_sq8* t, const nann_scorer* scorer, const float* q, int64_t n_queries,
                        int32_t fetch, int32_t k, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                        int32_t* out_fetch_index, float* out_fetch_scores, void* workspace, int64_t workspace_bytes,
                        const nann_search_options* options, nann_stream_t stream) {
  return flat_all_sq8(ix, t, scorer, q, n_queries, fetch, k, out_item_ids, out_scores, out_index, out_fetch_index, out_fetch_scores,
                      workspace, workspace_bytes, options, stream, "nann_search_all_sq8");
}


// ---- the certified form: the per-row error terms and the search (nann_sq8.h) -------------------------------------
int nann_sq8_bounds_create(const nann_index* ix, const nann_sq8* t, nann_stream_t stream, nann_sq8_bounds** out) {
  const char* who = "nann_sq8_bounds_create";
  if (!ix || !t || !out) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  *out = nullptr;
  if (t->uid != ix->uid || t->n_items != ix->desc.n_items || t->d != ix->desc.d)
    return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": the code table was made from another index");
  std::unique_ptr<nann_sq8_bounds, void (*)(nann_sq8_bounds*)> b(new nann_sq8_bounds(), nann_sq8_bounds_destroy);
  b->uid = ix->uid;
  b->serial = t->serial;
  b->n_items = t->n_items;
  const size_t n = (size_t)std::max<int64_t>(t->n_items, 1);  // (an empty index: one element each, never read)
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&b->err), n * 4));
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&b->xhat), n * 4));
  const int rc = launch_sq8_row_err(ix->desc.item_embs, ix->desc.emb_dtype, (long long)t->n_items, t->d, t->codes, t->scales, t->norms,
                                    b->err, b->xhat, as_stream(stream));
  if (rc) return rc;
  *out = b.release();
  return NANN_OK;
}
void nann_sq8_bounds_destroy(nann_sq8_bounds* b) {
  if (!b) return;
  if (b->err) (void)hipFree(b->err);
  if (b->xhat) (void)hipFree(b->xhat);
  delete b;
}
int nann_sq8_bounds_view(const nann_sq8_bounds* b, const float** err, const float** xhat) {
  if (!b) return fail(NANN_ERR_BAD_ARGUMENT, "nann_sq8_bounds_view: null argument");
  if (err) *err = b->err;
  if (xhat) *xhat = b->xhat;
  return NANN_OK;
}
int nann_search_all_sq8_exact_workspace_bytes(const nann_index* ix, const nann_sq8* t, const nann_sq8_bounds* b,
                                              const nann_scorer* scorer, int64_t n_queries, int32_t fetch, int64_t cap, int32_t k,
                                              int64_t* nbytes) {
  const char* who = "nann_search_all_sq8_exact_workspace_bytes";
  if (!nbytes) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  FlatBy by;
  ScanLayout L;
  Sq8ExactLayout X;
  const int rc = flat_sq8_exact_check(ix, t, b, scorer, n_queries, fetch, cap, k, who, &by, &L, &X);
  if (rc) return rc;
  *nbytes = n_queries == 0 || k == 0 ? 0 : (int64_t)X.total;
  return NANN_OK;
}
int nann_search_all_sq8_exact_layout(const nann_index* ix, const nann_sq8* t, const nann_sq8_bounds* b, const nann_scorer* scorer,
                                     int64_t n_queries, int32_t fetch, int64_t cap, int32_t k, int64_t out[8]) {
  const char* who = "nann_search_all_sq8_exact_layout";
  if (!out) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  FlatBy by;
  ScanLayout L;
  Sq8ExactLayout X;
  const int rc = flat_sq8_exact_check(ix, t, b, scorer, n_queries, fetch, cap, k, who, &by, &L, &X);
  if (rc) return rc;
  out[0] = L.chunk;
  out[1] = X.cap;
  out[2] = (int64_t)X.off_xsplits;
  out[3] = (int64_t)X.off_rows;
  out[4] = (int64_t)X.off_terms;
  out[5] = (int64_t)sizeof(Sq8QTerms);
  out[6] = (int64_t)X.off_a_scores;
  out[7] = (int64_t)X.total;
  return NANN_OK;
}
int nann_search_all_sq8_exact(const nann_index* ix, const nann_sq8* t, const nann_sq8_bounds* b, const nann_scorer* scorer,
                              const float* q, int64_t n_queries, int32_t fetch, int64_t cap, int32_t k, int64_t* out_item_ids,
                              float* out_scores, int32_t* out_index, int32_t* out_certified, int32_t* out_n_survivors,
                              void* workspace, int64_t workspace_bytes, const nann_search_options* options, nann_stream_t stream) {
  return flat_all_sq8_exact(ix, t, b, scorer, q, n_queries, fetch, cap, k, out_item_ids, out_scores, out_index, out_certified,
                            out_n_survivors, workspace, workspace_bytes, options, stream, "nann_search_all_sq8_exact");
}

// ---- the certified range form (nann_sq8.h) ------------------------------------------------------------------------
int nann_search_all_range_sq8_exact_workspace_bytes(const nann_index* ix, const nann_sq8* t, const nann_sq8_bounds* b,
                                                    const nann_scorer* scorer, int64_t n_queries, int64_t cap, int64_t* nbytes) {
  const char* who = "nann_search_all_range_sq8_exact_workspace_bytes";
  if (!nbytes) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  FlatBy by;
  ScanLayout L;
  Sq8RangeLayout R;
  const int rc = flat_sq8_range_check(ix, t, b, scorer, n_queries, cap, who, &by, &L, &R);
  if (rc) return rc;
  *nbytes = n_queries == 0 ? 0 : (int64_t)R.total;
  return NANN_OK;
}
int nann_search_all_range_sq8_exact(const nann_index* ix, const nann_sq8* t, const nann_sq8_bounds* b, const nann_scorer* scorer,
                                    const float* q, int64_t n_queries, const float* thresholds, int64_t cap, int64_t capacity,
                                    int64_t* out_row_splits, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                                    int32_t* out_certified, int32_t* out_n_survivors, void* workspace, int64_t workspace_bytes,
                                    const nann_search_options* options, nann_stream_t stream) {
  return flat_range_sq8_exact(ix, t, b, scorer, q, n_queries, thresholds, cap, capacity, out_row_splits, out_item_ids, out_scores,
                              out_index, out_certified, out_n_survivors, workspace, workspace_bytes, options, stream,
                              "nann_search_all_range_sq8_exact");
}

}  // extern "C"
