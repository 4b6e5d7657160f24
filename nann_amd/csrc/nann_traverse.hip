// nann_traverse.hip -- the host side of the calls that walk the graph: the serving traversal (nann_search_opt,
// nann_search_model_opt and their five deprecated spellings, nann_search_filtered, nann_search_model_filtered, nann_search_multi,
// nann_search_multi_fused, nann_search_grouped, nann_search_model_grouped, nann_search_diverse, nann_search_model_diverse, nann_search_where,
// nann_search_model_where;
// kernels in nann_search.h), the evaluation traversal (nann_search_eval, nann_search_eval_ex, nann_search_eval_model; nann_eval.h), each
// with its *_workspace_bytes, and what nann_index_create measures for them: the probe and the pivots of the batch order.
//
// A source of nann_core.o.  What it takes from the other host sources (nann_flat.hip's resolve_* and shape checks among it), and
// what they take from it -- probe_index and choose_pivots for nann_index_create, launch_order -- is declared in nann_host.h.
//
// Every entry point is one walk -- traverse, traverse_filtered around it, evaluate -- over the steps below, each written once:
//   scored_by (nann_host.h)   who scores the call.  The flat family's too: FlatBy derives from ScoredBy; flat_by adds what only
//                      its kernels take, and keeps its own refusals (a null handle, an unknown kind) where the flat calls pin them
//   slots_bytes, traverse_bytes, eval_bytes   the layout of a workspace, [header | slots | tail | batch order] [staged model
//                      query] [filter staging]: every *_workspace_bytes, workspace check and carve-off takes its number from it
//   short_workspace, disagree   the two refusals every walk has
//   stage_model_query  a model form: kt / upad of the attention model, or the mean of the sequence, behind the inner workspace
//   index_fields_of    the index's fields into SearchArgs / EvalArgs
//   plan_search / search_impl, eval_plan / eval_impl   plan, fill the arguments, launch: moved here as they were
//
// The ORDER in which a call looks at its arguments is part of its contract -- with two faults present, which one the caller is
// told -- and the scorer and the model forms differ in it for no deeper reason than their history.  The walks keep every order
// as it was and say where they branch for it (tests/test_traverse_contract_gpu.py pins them).
#include "nann_host.h"
#include "nann_eval.h"
#include "nann_order_kernels.h"
#include "nann_filter.h"
#include "nann_predicate.h"
#include "nann_union.h"
#include "nann_fuse.h"
#include "nann_groupcap.h"
#include "nann_mmr.h"

using namespace nann;

// ---- the plan ------------------------------------------------------------------------------------------------------------
constexpr int64_t kPhaseTail = 8192;  // behind the slots: reserved (round 4's first pipeline of phases kept its block prefix here)
// (SearchOpt::reserve: workgroup slots the persistent traversal grid leaves FREE -- a host that overlaps another stream's
// kernels with the search, the exchange step of a sharded search, DESIGN.md 7, keeps a few for them; the grid otherwise
// owns every CU's LDS until its first workgroups exit.)

static int bit_length(uint64_t v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }

constexpr int kKindAttn = 2;      // plan_search: the attention model (NANN_MODEL_ATTENTION); 0 / 1 = NANN_SCORER_L2 / NANN_SCORER_MLP.  These are
                                  //   PLAN kinds, not nann_scorer_kind: the inner product (NANN_SCORER_IP, also 2) plans as L2 (search_impl)
constexpr int kKindMlpSplit = 3;  //   the MLP scorer in split-f16 form (two slice buffers: the scratch of an attention plan)
constexpr int kKindMlpRes = 4;    //   the MLP scorer, either precision, on the pre-projected table with layer 2 resident in LDS
                                  //   (nann_mlp5.h): 16K-slot set under the weights, or the HBM bitmap
// kind: scorer kind of the call, or -1 = "any" (workspace sizing: the largest plan)
static int plan_search(const nann_index* ix, const int32_t t[6], int64_t n_queries, int kind, SearchPlan* p, const SearchOpt& opt,
                       bool mlp_exact_hint = false) {
  for (int i = 0; i < 6; ++i)
    if (t[i] < 0 || t[i] > kMaxK) return fail(NANN_ERR_UNSUPPORTED, "level_topn entries must be in [0, 1024]");
  DeviceInfo di;
  int rc = device_info(&di);
  if (rc) return rc;
  const int64_t E = ix->desc.n_enter;
  const int64_t raw1 = (int64_t)t[0] * ix->max_deg[1];
  const int64_t raw0 = (int64_t)std::max(t[1], std::max(t[2], t[3])) * ix->max_deg[0];
  const int64_t max_raw = std::max<int64_t>(std::max(raw1, raw0), 1);
  const int64_t max_cand = std::max<int64_t>(std::max<int64_t>(E, t[0] + raw1), std::max<int64_t>(raw0, 1));
  if (max_cand > 0x3fffffffll) return fail(NANN_ERR_UNSUPPORTED, "candidate bound too large");
  p->max_cand = (int)max_cand;
  p->max_raw = (int)max_raw;
  p->pool_cap = std::max(t[1] + t[2] + t[3] + t[4], 1);
  const size_t tail = kMaxD * 4 + 256;  // q + misc behind the phase scratch
  const size_t bm_bytes = (size_t)ix->bm_words * 4;
  // scratch behind the visited set: "any" (workspace sizing) assumes the largest, so that its slots can hold the HBM
  // bitmap of whatever plan the call ends up with
  const size_t big_scratch = (size_t)std::max(kAttnScratch, kMlpSplitScratch);
  const bool res = kind == kKindMlpRes;
  const size_t bm_scratch = kind == kKindAttn ? (size_t)kAttnScratch
                            : kind == kKindMlpSplit ? (size_t)kMlpSplitScratch
                            : res ? (size_t)kMlpResBytes
                            : kind < 0 ? big_scratch : (size_t)kPhaseScratch;
  const bool bitmap_fits = !res && bm_bytes + bm_scratch + tail <= di.lds_max;  // resident layer 2 owns the LDS: HBM bitmap
  const int mode = opt.mode;
  // the bitmap plan: what MLP traversals run, what oversized shards run, and the fallback of the hash plan
  const int bm_vis = (bitmap_fits && mode != NANN_TRAVERSAL_HBM_BITMAP) ? VIS_LDS_BITMAP : VIS_HBM_BITMAP;
  const size_t bm_lds = bm_scratch + tail + (bm_vis == VIS_LDS_BITMAP ? bm_bytes : 0);
  const int bm_per_cu = (bm_vis == VIS_LDS_BITMAP || res) ? 1 : 2;
  // the hash-set plans.  Which table:
  // the visited set of a level holds its marks plus every id the level's rounds keep.  Measured on
  // HNSW(M=32) graphs (profiles/): the rows a beam walks are ~2.75x the mean degree and ~45% of the
  // gathered ids are new.  16K slots (two queries per CU) when that estimate leaves headroom, 32K
  // slots (one query per CU) for wider beams; beyond that the bitmap.  A wrong guess costs speed,
  // not correctness: overflowing queries are rerun on the bitmap kernel.
  // set entries are (remainder, probe step) tags cut from a bijection of the id space (nann_device.h, vis_key): any
  // shard below 2^27 items gets 12 position bits (rounds 1-2 stored the id: 10 position bits at 4M items)
  // bit_length(n_items), not (n_items - 1): a shard of exactly 2^20 items would otherwise take the direct form, where
  // id 2^20 - 1 at position 4095 encodes as the empty value 0xffffffff
  const int id_bits = std::max(16, bit_length((uint64_t)std::max<int64_t>(ix->desc.n_items, 1)));
  const bool tag_fits = id_bits <= 27;
  const double mean_deg0 = (double)ix->desc.nb_nnz[0] / (double)std::max<int64_t>(ix->desc.n_items, 1);
  const double walk_deg = std::min<double>((double)ix->max_deg[0], 2.75 * mean_deg0);
  // Round 5: the estimate is MEASURED per index where it can be (probe_index: 64 queries at nann_index_create, the new nodes a
  // level-0 round finds per frontier row; a high quantile of the probe's queries, so the estimate sits on the tail).  Rounds 1-4
  // guessed it from the mean degree (2.75 x mean degree walked, 45 % new: fitted to the device builder's graphs, mean degree
  // ~17) and sent a dense graph (keepPrunedConnections, mean degree 52) to the one-workgroup-per-CU 32K plan at 0.67 of the
  // roofline, where the 16K plan holds its ~8 k visited ids at 0.84 with no rerun (profiles/rd5c_dense_graph.txt).  The ratio
  // falls as the beam widens (neighbourhoods overlap more), so a probe at ef <= 64 overestimates wider beams: safe side.
  const double rows_walked = (double)t[1] + t[2] + t[3];
  const double est_guess = t[1] + 0.45 * walk_deg * rows_walked;
  // (the 90th percentile of the probe's queries x 1.15, not their maximum: on the exact k-NN graph -- every row at the cap -- one
  // of 64 probe queries found 41 new nodes per row against a mean of 13.6 and a q90 of ~20, and planning on that outlier sent
  // configs[1] to the 32K plan at 0.65 although the real sets hold ~8 k ids; a query in the tail is rerun on the bitmap kernel,
  // which is what the rerun is for: profiles/rd5u_knn_graph.txt)
  const double est_visited = ix->probe_valid ? std::min(t[1] + std::min(1.15 * (double)ix->probe_new_per_row_q90, (double)ix->probe_new_per_row_max) * rows_walked,
                                                        t[1] + (double)ix->max_deg[0] * rows_walked)
                                             : est_guess;
  // the 16K / 32K-slot set holds 16320 / 32704 ids; a measured estimate may come closer to that than a guessed one
  // (measured estimate: up to ~92 % of the capacity a set really has since a filling set cuts its pieces -- 16 256 / 32 640
  //  less the 512 below which a query is handed back; ef = 192 on the shipped graph, estimate 14.7 k: 1.72 M q/s on the 16K plan
  //  with no rerun against 1.47 M on the 32K plan, profiles/rd5ag_planner_thresholds.txt)
  // Beyond 2^20 items the entries are (tag, probe step) pairs and a probe sequence may be 62 steps long at most (longer: the
  // query is rerun); at a load of 0.92 that is 0.5 % PER INSERT, at 0.80 below 1e-6 -- such shards plan with 0.80 of the set
  // (test_a_set_that_fills_up_cuts_its_pieces: tag sets ending at 0.87 / 0.96 load rerun 1 / 12 of 12 queries).
  const bool tag_entries = id_bits > 20;
  const double fit16 = !ix->probe_valid ? 11000.0 : tag_entries ? 13000.0 : 15000.0;
  const double fit32 = !ix->probe_valid ? 24000.0 : tag_entries ? 26000.0 : 30500.0;
  const double worst_visited = t[1] + (double)ix->max_deg[0] * ((double)t[1] + t[2] + t[3]);
  const size_t hash16_lds = (size_t)vis_slots(VIS_LDS_HASH) * 4 + hash_phase_scratch<512, 16384>() + tail;
  const size_t hash32_lds = (size_t)vis_slots(VIS_LDS_HASH32) * 4 + hash_phase_scratch<kNT, 32768>() + tail;
  const bool hash_ok = (kind == NANN_SCORER_L2 || kind < 0) && tag_fits && 2 * hash16_lds <= di.lds_max &&
                       hash32_lds <= di.lds_max;
  int hash_vis = -1;
  if (mode == NANN_TRAVERSAL_LDS_HASH) hash_vis = VIS_LDS_HASH;
  else if (mode == NANN_TRAVERSAL_LDS_HASH32) hash_vis = VIS_LDS_HASH32;
  else if (mode == NANN_TRAVERSAL_AUTO && (kind == NANN_SCORER_L2 || kind < 0)) {
    if (worst_visited <= 16320.0 || est_visited <= fit16) hash_vis = VIS_LDS_HASH;
    else if (worst_visited <= 32704.0 || est_visited <= fit32) hash_vis = VIS_LDS_HASH32;
    // small batches: with at most one query per CU the second 512-thread workgroup of the 16K-slot plan has nothing to
    // overlap with, and a query is served faster by ONE 1024-thread workgroup owning the CU (measured at configs[1]:
    // B = 1 0.196 -> 0.160 ms, B = 64 0.206 -> 0.165 ms; profiles/r3d_*)
    if (hash_vis == VIS_LDS_HASH && kind == NANN_SCORER_L2 && n_queries <= (int64_t)di.cus) hash_vis = VIS_LDS_HASH32;
  }
  // attention model / split-f16 MLP: 16K slots, one workgroup per CU -- when the level's visited ids are expected to fit
  // (a beam too wide for the set would send nearly every query through both kernels)
  const bool fits16 = worst_visited <= 16320.0 || est_visited <= fit16 || mode == NANN_TRAVERSAL_LDS_HASH;
  const bool own_hash_plan = (kind == kKindAttn || kind == kKindMlpSplit || res) && tag_fits && fits16;
  if ((mode == NANN_TRAVERSAL_LDS_HASH || mode == NANN_TRAVERSAL_LDS_HASH32) && !hash_ok && kind >= 0 &&
      !(own_hash_plan && mode == NANN_TRAVERSAL_LDS_HASH))
    return fail(NANN_ERR_UNSUPPORTED, "hash-set traversal: shards below 2^27 items; the 32K-slot set: L2 scorer only");
  unsigned long long off[9];
  // the slot's last region: the HBM bitmap of a bitmap plan, and where a resident-layer-2 traversal parks its 16K-slot
  // set while it scores (nann_mlp5.h); "any" sizes for both
  uint32_t gbm_words = bm_vis == VIS_HBM_BITMAP ? ix->bm_words : 0u;
  if (res || kind < 0 || kind == kKindAttn) gbm_words = std::max<uint32_t>(std::max<uint32_t>(gbm_words, ix->bm_words), (uint32_t)vis_slots(kind < 0 ? VIS_LDS_HASH32 : VIS_LDS_HASH));
  p->slot_bytes = slot_layout(p->max_cand, p->max_raw, p->pool_cap, gbm_words, off);
  p->id_bits = id_bits;
  p->fb_vis = bm_vis;
  p->fb_lds_bytes = bm_lds;
  p->fb_slots = (int)std::max<int64_t>(1, std::min<int64_t>(n_queries, (int64_t)di.cus * bm_per_cu));
  if (own_hash_plan && mode != NANN_TRAVERSAL_LDS_BITMAP && mode != NANN_TRAVERSAL_HBM_BITMAP) {
    // attention model / split-f16 MLP: 16K-slot set + two weight-slice buffers, one 512-thread workgroup per CU
    p->vis = VIS_LDS_HASH;
    p->nt = 512;
    p->lds_bytes = res ? (size_t)kMlpResBytes + hash_phase_scratch<512, 16384>() + tail  // [W2 (set over its head) | vectors | phase scratch]
                       : (size_t)vis_slots(VIS_LDS_HASH) * 4 + bm_scratch + tail;
    p->slots = (int)std::max<int64_t>(1, std::min<int64_t>(n_queries, (int64_t)di.cus));
  } else if (hash_ok && hash_vis == VIS_LDS_HASH) {
    p->vis = VIS_LDS_HASH;
    p->nt = 512;
    p->lds_bytes = hash16_lds;
    p->slots = (int)std::max<int64_t>(1, std::min<int64_t>(n_queries, (int64_t)di.cus * 2));
  } else if (hash_ok && hash_vis == VIS_LDS_HASH32) {
    p->vis = VIS_LDS_HASH32;
    p->nt = kNT;
    p->lds_bytes = hash32_lds;
    p->slots = (int)std::max<int64_t>(1, std::min<int64_t>(n_queries, (int64_t)di.cus));
  } else {
    p->vis = bm_vis;
    p->nt = kNT;  // (the MLP kernels run kMlpNT threads; the launcher knows)
    p->lds_bytes = bm_lds;
    p->slots = p->fb_slots;
  }
  // the MLP's pipeline of phases (nann_mlp6.h): traversal stages at the 16K-slot plan's geometry, one slot per query of a chunk
  // Where it pays (profiles/r4tu_mlp_batch_sweep_phased_vs_fused.txt, r4x_mlp_loop_ab.txt; configs[2]): exact f32 at every
  // batch size (batch 32: 3.4x -- the scoring launch spreads 32 queries' rows over the chip, the fused kernel holds 32 CUs --,
  // 128: 1.7x, >= 256: +3..8 %); split-f16 below ~160 queries (batch 32: 1.64x).  Above that the fused split-f16 kernel, which
  // runs the same software-pipelined block loop, is level with it or ahead: 256-512 queries +8..19 % (one query per CU finishes
  // sooner than 12 launches), 1024: within 2 % either way box to box, 4096: +2.7 %.  nann_search_options.mlp_form forces either.
  const bool exact_form = mlp_exact_hint;
  const bool pays = exact_form || n_queries <= 160;
  const bool no_forced_bitmap = mode != NANN_TRAVERSAL_LDS_BITMAP && mode != NANN_TRAVERSAL_HBM_BITMAP;
  const bool want_phased = opt.mlp_form == NANN_MLP_FORM_PHASED || (opt.mlp_form == NANN_MLP_FORM_AUTO && pays);
  p->phased = res && own_hash_plan && no_forced_bitmap && 2 * hash16_lds <= di.lds_max && want_phased;
  p->phase_vis = VIS_LDS_HASH;
  p->phase_per_cu = 2;
  p->phase_lds_bytes = hash16_lds;
  // Wide beams (ef = 256: a level's visited ids need the 32K-slot set): the fused kernel keeps its bitmap in HBM because the
  // resident weights leave no room for a set; the pipeline's traversal stages own the LDS and run the L2 kernel's 32K-slot
  // plan (one 1024-thread workgroup per CU).  Both precisions, every batch size (profiles/r5g_*).
  const bool fits32 = worst_visited <= 32704.0 || est_visited <= fit32;
  if (res && !own_hash_plan && tag_fits && fits32 && no_forced_bitmap && mode != NANN_TRAVERSAL_LDS_HASH && hash32_lds <= di.lds_max &&
      opt.mlp_form != NANN_MLP_FORM_FUSED) {
    p->phased = true;
    p->phase_vis = VIS_LDS_HASH32;
    p->phase_per_cu = 1;
    p->phase_lds_bytes = hash32_lds;
    gbm_words = std::max<uint32_t>(gbm_words, (uint32_t)vis_slots(VIS_LDS_HASH32));  // where the 32K-slot set is parked
    p->slot_bytes = slot_layout(p->max_cand, p->max_raw, p->pool_cap, gbm_words, off);
  }
  // few queries (at most one per CU): a query's stages run faster on ONE 1024-thread workgroup per CU than on one of two
  // 512-thread workgroups that has no partner to overlap with (the L2 kernel's small-batch rule, above)
  if (p->phased && p->phase_vis == VIS_LDS_HASH && opt.small32 && n_queries <= (int64_t)di.cus && tag_fits && hash32_lds <= di.lds_max) {
    p->phase_vis = VIS_LDS_HASH32;
    p->phase_per_cu = 1;
    p->phase_lds_bytes = hash32_lds;
    gbm_words = std::max<uint32_t>(gbm_words, (uint32_t)vis_slots(VIS_LDS_HASH32));
    p->slot_bytes = slot_layout(p->max_cand, p->max_raw, p->pool_cap, gbm_words, off);
  }
  p->phase_slots = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_queries, kPhaseChunk), (int64_t)di.cus * p->phase_per_cu));
  p->phase_score_wgs = di.cus;
  p->est_visited = (float)est_visited;
  p->worst_visited = (float)worst_visited;
  if (kind < 0)  // sizing: the widest plan (two workgroups per CU, or one slot per query of a phased chunk)
    p->slots = (int)std::max<int64_t>(1, std::min<int64_t>(n_queries, std::max<int64_t>((int64_t)di.cus * 2, kPhaseChunk)));
  else if (const int reserve = opt.reserve) {  // leave workgroup slots to kernels of other streams (nann_search_options.slot_reserve)
    const int per_cu = p->vis == VIS_LDS_HASH && p->nt == 512 && !res && kind != kKindAttn && kind != kKindMlpSplit ? 2
                       : p->vis == VIS_HBM_BITMAP && !res ? 2 : 1;
    p->slots = std::max(1, std::min(p->slots, di.cus * per_cu - reserve));
    p->fb_slots = std::max(1, std::min(p->fb_slots, di.cus * bm_per_cu - reserve));
    // the pipeline of phases keeps the same promise (it ignored the reserve): its traversal stages leave `reserve`
    // slots, its scoring launches -- one workgroup owns a CU's LDS -- the CUs those slots stand for
    p->phase_slots = std::max(1, std::min(p->phase_slots, di.cus * p->phase_per_cu - reserve));
    p->phase_score_wgs = std::max(1, di.cus - (reserve + 1) / 2);
  }
  return NANN_OK;
}

// L2 instantiations live in nann_l2_inst.hip (one object per row dtype), MLP ones in
// nann_mlp_inst.hip (one per embedding dim): the heavy kernels compile in parallel.
// kind: nann_scorer_kind.  lean: the caller found the launch eligible (takes_lean_kernel): k_search_lean instead of k_search.
static int launch_search_any(int lpr, int dt, int kind, int split, int vis, int nt, int slots, size_t lds_bytes,
                             const SearchArgs& a, hipStream_t st, bool lean = false) {
  if (kind == NANN_SCORER_MLP) {
    if (lpr == 8) return launch_search_mlp_d64(dt, split, vis, slots, lds_bytes, a, st);
    if (lpr == 16) return launch_search_mlp_d128(dt, split, vis, slots, lds_bytes, a, st);
    if (lpr == 32) return launch_search_mlp_d256(dt, split, vis, slots, lds_bytes, a, st);
    return fail(NANN_ERR_UNSUPPORTED, "MLP scorer: d <= 256 only");
  }
  if (lean && kind == NANN_SCORER_IP) {
    if (dt == NANN_F16) return launch_search_lean_ip_f16(lpr, vis, nt, slots, lds_bytes, a, st);
    if (dt == NANN_BF16) return launch_search_lean_ip_bf16(lpr, vis, nt, slots, lds_bytes, a, st);
    return launch_search_lean_ip_f32(lpr, vis, nt, slots, lds_bytes, a, st);
  }
  if (lean && kind == NANN_SCORER_L2) {
    if (dt == NANN_F16) return launch_search_lean_l2_f16(lpr, vis, nt, slots, lds_bytes, a, st);
    if (dt == NANN_BF16) return launch_search_lean_l2_bf16(lpr, vis, nt, slots, lds_bytes, a, st);
    return launch_search_lean_l2_f32(lpr, vis, nt, slots, lds_bytes, a, st);
  }
  if (kind == NANN_SCORER_IP) {
    if (dt == NANN_F16) return launch_search_ip_f16(lpr, vis, nt, slots, lds_bytes, a, st);
    if (dt == NANN_BF16) return launch_search_ip_bf16(lpr, vis, nt, slots, lds_bytes, a, st);
    return launch_search_ip_f32(lpr, vis, nt, slots, lds_bytes, a, st);
  }
  if (kind != NANN_SCORER_L2) return fail(NANN_ERR_BAD_ARGUMENT, "nann_search: unknown scorer kind");
  if (dt == NANN_F16) return launch_search_l2_f16(lpr, vis, nt, slots, lds_bytes, a, st);
  if (dt == NANN_BF16) return launch_search_l2_bf16(lpr, vis, nt, slots, lds_bytes, a, st);
  return launch_search_l2_f32(lpr, vis, nt, slots, lds_bytes, a, st);
}
// A plain call -- flat scorer, hash-set plan, the launch's own level_topn, no tick buffer, ids the set holds directly -- takes
// the lean kernel for its main launch (NANN_LEAN_KERNEL=0: never); every other launch, the capacity rerun among them, the general one.
static bool takes_lean_kernel(const SearchOpt& opt, int kind, int vis, const SearchArgs& a) {
  return opt.lean && (kind == NANN_SCORER_L2 || kind == NANN_SCORER_IP) && lean_eligible(vis, a);
}

// ---- the two refusals every walk has (`who`: the call whose <who>_workspace_bytes() names the size) -------------------------
static int short_workspace(const char* who) {
  return fail(NANN_ERR_CAPACITY, std::string("workspace smaller than ") + who + "_workspace_bytes()");
}
static int disagree(const ScoredBy& by) { return fail(NANN_ERR_BAD_ARGUMENT, std::string(by.what) + " and index disagree on d / dtype"); }

// ---- the workspace ------------------------------------------------------------------------------------------------------
// Serving: [WsHeader, 256 bytes | the plan's slots | kPhaseTail | the batch order, order_ws_bytes(n)], behind it under a model
// [a 256-byte gap | the staged query], behind that for a filtered call, from the next 256-byte boundary, [the staging area of
// the final selection: item ids i64[n, F], scores f32[n, F], rows i32[n, F]].  Evaluation: [header | slots] [gap | staged query].
static unsigned long long slots_bytes(unsigned long long slot_bytes, int64_t slots, bool tail) {
  return 256 + slot_bytes * (unsigned long long)slots + (tail ? kPhaseTail : 0);
}
static int64_t up256_i64(int64_t v) { return (v + 255) & ~255ll; }

// the batch order: behind the slots, at the last 256-byte boundary that leaves order_ws_bytes(n) behind it; false: no room
static bool order_offset(const SearchPlan& p, int64_t n_queries, int64_t workspace_bytes, unsigned long long* off) {
  const unsigned long long slots_end = slots_bytes(p.slot_bytes, std::max(p.slots, p.fb_slots), true);
  *off = ((unsigned long long)workspace_bytes - order_ws_bytes(n_queries)) & ~255ull;
  return (unsigned long long)workspace_bytes >= ((slots_end + 255) & ~255ull) + order_ws_bytes(n_queries);
}

// what a model form stages per query: kt f32[256, 64] and upad f32[64, 64] of the attention model, else the mean f32[d]
static size_t model_query_bytes(const nann_model* m, int64_t n_queries) {
  const size_t per = m->kind == NANN_MODEL_ATTENTION ? (size_t)(256 * 64 + 64 * 64) * 4 : (size_t)m->d * 4;
  return ((size_t)n_queries * per + 255) & ~(size_t)255;
}
static size_t filter_stage_bytes(int64_t n_queries, int f) {
  return ((size_t)std::max<int64_t>(n_queries, 0) * (size_t)std::max(f, 0) * 16 + 255) & ~(size_t)255;
}

struct TraverseBytes {
  int64_t search = 0;     // the scorer form's workspace, at the head
  int64_t query_off = 0;  // a model form: where its staged query lies,
  int64_t inner = 0;      //   and the unfiltered call's workspace with it (a scorer form: == search)
  int64_t stage_off = 0;  // a filtered form: where its staging area lies,
  int64_t total = 0;      //   and the call's workspace with it (unfiltered: == inner)
};
// m: the model of a model form, else null.  The scorer form sizes for the widest plan, whatever the options (kind "any").
static int traverse_bytes(const nann_index* ix, const nann_model* m, const int32_t level_topn[6], int64_t n_queries, bool filtered,
                          TraverseBytes* b) {
  SearchPlan p;
  const int rc = plan_search(ix, level_topn, n_queries, m && m->kind == NANN_MODEL_ATTENTION ? kKindAttn : -1, &p, resolve_options(nullptr));
  if (rc) return rc;
  b->search = (int64_t)(slots_bytes(p.slot_bytes, std::max(p.slots, p.fb_slots), true) + order_ws_bytes(n_queries));
  b->query_off = up256_i64(b->search);
  b->inner = m ? b->search + 256 + (int64_t)model_query_bytes(m, n_queries) : b->search;
  b->stage_off = up256_i64(b->inner);
  b->total = filtered ? b->stage_off + (int64_t)filter_stage_bytes(n_queries, level_topn[5]) : b->inner;
  return NANN_OK;
}
// a filtered call speaks under its unfiltered twin's name
static int traverse_size(const nann_index* ix, const nann_model* m, bool model, const int32_t level_topn[6], int64_t n_queries,
                         bool filtered, int64_t* nbytes) {
  if (!ix || (model && !m) || !level_topn || !nbytes)
    return fail(NANN_ERR_BAD_ARGUMENT, std::string(model ? "nann_search_model" : "nann_search") + "_workspace_bytes: null argument");
  TraverseBytes b;
  const int rc = traverse_bytes(ix, m, level_topn, n_queries, filtered, &b);
  if (rc) return rc;
  *nbytes = b.total;
  return NANN_OK;
}

// ---- the staged model query -----------------------------------------------------------------------------------------------
// the per-user side once per request (build_opt_graph.py:91-107) into qbuf, handed back as the scorer form takes it
static int stage_model_query(const ScoredBy& by, const void* comm_seq_f16, int64_t n_queries, unsigned char* qbuf, bool f32_form,
                             nann_stream_t stream, const float** q, const float** kt, const float** upad) {
  float* buf = reinterpret_cast<float*>(qbuf);
  if (by.at) {
    float* u = buf + (size_t)n_queries * 256 * 64;
    *kt = buf; *upad = u;
    // f32_form: (the evaluation job always runs the f32 form of the model, whatever precision serving uses)
    return f32_form ? launch_attn_prepare(as_stream(stream), by.at->P, comm_seq_f16, n_queries, buf, u)
                    : nann_attn_prepare(by.at, comm_seq_f16, n_queries, buf, u, stream);
  }
  *q = buf;
  return nann_user_seq_mean(comm_seq_f16, n_queries, by.mean_of->seq_len, by.mean_of->d, buf, stream);
}

// ---- the launch arguments: SearchArgs and EvalArgs name the index's fields alike --------------------------------------------
template <class A> static void index_fields_of(const nann_index* ix, A* a) {
  a->emb = ix->desc.item_embs;
  a->item_ids = ix->desc.item_ids;
  for (int l = 0; l < 2; ++l) { a->nbv[l] = ix->desc.nb_values[l]; a->nbrs[l] = ix->desc.nb_row_splits[l]; }
  a->enter = ix->desc.enter_points;
  a->n_enter = (int)ix->desc.n_enter;
  a->n_items = (uint32_t)ix->desc.n_items;
  a->d = ix->desc.d;
  a->bm_words = ix->bm_words;
}

// the traversal for (index, scorer | attention model): plan, fill the arguments, launch (+ the
// fallback launch of the hash-set plans).  tq: optional device i32[n_queries, 6], level_topn per query (level_topn then
// holds the per-launch maxima).
static int search_impl(const nann_index* ix, const ScoredBy& by, const float* q, const float* kt, const float* upad, int64_t n_queries,
                       const int32_t level_topn[6], const int32_t* tq, void* workspace, int64_t workspace_bytes,
                       int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* status,
                       int32_t* counters, int64_t* phase_ticks, const nann_search_options* options, nann_search_plan* plan_out,
                       hipStream_t st) {
  const nann_scorer* scorer = by.scorer;
  const nann_attn_scorer* attn = by.at;
  if (n_queries > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, "too many queries in one call");
  int rc = check_options(options);
  if (rc) return rc;
  SearchOpt opt = resolve_options(options);
  // the inner product takes every plan L2 takes (the same traversal with another term in its scoring call): it plans as L2, and
  // only the launch and the batch order (pivot distances: an L2 notion) tell the two apart
  const bool ip = !attn && scorer->desc.kind == NANN_SCORER_IP;
  const int kind = attn ? kKindAttn : ip ? NANN_SCORER_L2 : scorer->desc.kind;
  if (!attn && kind != NANN_SCORER_L2 && kind != NANN_SCORER_MLP) return fail(NANN_ERR_BAD_ARGUMENT, "nann_search: unknown scorer kind");
  const bool mlp = !attn && kind == NANN_SCORER_MLP;
  const bool mlp_split = mlp && scorer->desc.precision == NANN_MLP_SPLIT_F16;
  // certified: the filter lives in the pipeline of phases only -- a forced fused form is the phased one; every other plan
  // runs the exact form's kernels
  const bool mlp_cert = mlp && scorer->desc.precision == NANN_MLP_CERTIFIED;
  if (mlp_cert && opt.mlp_form == NANN_MLP_FORM_FUSED) opt.mlp_form = NANN_MLP_FORM_PHASED;
  // the item-only part of the scorer, pre-projected per (scorer, index): found or built here (nann_*_prepare does it
  // ahead of traffic); without a table -- switched off, or no room in HBM -- the kernels that read the embedding rows run
  std::shared_ptr<ProjTable> tab;
  ProjCache* cache = by.cache;
  if (attn) rc = attn_projection(attn, ix, st, false, opt.preproject != 0, &tab);  // both precisions run on the table of item-only layers (nann_attn_proj.h; nann_attn_kernels.h PROJ)
  else if (mlp) rc = mlp_projection(scorer, ix, st, false, opt.preproject != 0, &tab);
  if (rc) return rc;
  const bool mlp_res = mlp && tab;  // layer 2 resident in LDS, either precision (nann_mlp5.h)
  SearchPlan p;
  rc = plan_search(ix, level_topn, n_queries, mlp_res ? kKindMlpRes : mlp_split ? kKindMlpSplit : kind, &p, opt, mlp && !mlp_split);
  if (rc) return rc;
  if (plan_out) {  // what this call runs (host-side facts; the number of reruns lives in the workspace: nann_search_reruns)
    const bool ph = mlp_res && p.phased;
    const int v = ph ? p.phase_vis : p.vis;
    plan_out->visited_set = v == VIS_LDS_HASH ? NANN_TRAVERSAL_LDS_HASH : v == VIS_LDS_HASH32 ? NANN_TRAVERSAL_LDS_HASH32
                            : v == VIS_LDS_BITMAP ? NANN_TRAVERSAL_LDS_BITMAP : NANN_TRAVERSAL_HBM_BITMAP;
    plan_out->fallback_visited_set = p.fb_vis == VIS_LDS_BITMAP ? NANN_TRAVERSAL_LDS_BITMAP : NANN_TRAVERSAL_HBM_BITMAP;
    // (the split-f16 hash-set kernel that reads the embedding rows runs its second mapping at d <= 128: launch_search_mlp_d64 / _d128)
    const bool mlp2 = mlp_split && !mlp_res && p.vis == VIS_LDS_HASH && ix->desc.d <= 128;
    plan_out->threads = ph ? (p.phase_vis == VIS_LDS_HASH32 ? kNT : 512) : mlp2 ? kMlp2NT : ((mlp || attn) && p.nt == kNT ? 512 : p.nt);
    plan_out->workgroups = ph ? p.phase_slots : p.slots;
    plan_out->phased = ph ? 1 : 0;
    plan_out->table = tab ? 1 : 0;
    plan_out->est_visited = p.est_visited;
    plan_out->worst_visited = p.worst_visited;
    plan_out->lean = 0;  // (set where the launch is chosen, below)
  }
  const int64_t need_slots = p.phased ? std::max<int64_t>(std::min<int64_t>(n_queries, kPhaseChunk), p.fb_slots) : std::max(p.slots, p.fb_slots);
  // (against the plan this call runs, not the widest one nann_search_workspace_bytes sized for: a shorter workspace may do)
  if (!workspace || workspace_bytes < (int64_t)slots_bytes(p.slot_bytes, need_slots, p.phased))
    return short_workspace("nann_search");
  SearchArgs a;
  index_fields_of(ix, &a);
  a.q = q;
  a.n_queries = (int)n_queries;
  for (int i = 0; i < 6; ++i) a.t[i] = level_topn[i];
  a.tq = tq;
  a.ws = static_cast<unsigned char*>(workspace);
  a.slot_bytes = p.slot_bytes;
  a.max_cand = p.max_cand; a.max_raw = p.max_raw; a.pool_cap = p.pool_cap;
  a.out_ids = out_item_ids; a.out_scores = out_scores; a.out_index = out_index;
  a.status = status; a.counters = counters;
  a.phase_ticks = reinterpret_cast<long long*>(phase_ticks);
  a.id_bits = p.id_bits;
  a.redo = 0;
  a.phase = 0;
  a.proj = tab ? tab->table : nullptr;
  a.mlp = MlpParams{};
  a.attn = AttnParams{};
  a.kt = kt; a.upad = upad;
  const int dt = ix->desc.emb_dtype;
  const bool hashed = p.vis == VIS_LDS_HASH || p.vis == VIS_LDS_HASH32;
  // L2 hash-set plans with more queries than slots: the main launch takes the batch in locality order (nann_order.h);
  // the rerun launch, the MLP / attention scorers and the bitmap plans keep input order.  The order lives behind the
  // slots, at the last 256-byte boundary that leaves order_ws_bytes(n) behind it (nann_search_workspace_bytes counts
  // them: order_offset); a workspace sized without them runs in input order.  WsHeader (query queues, hand-back counter)
  // starts every call at zero: the order's last kernel clears it on its way, every other plan with a memset.
  unsigned long long order_off = 0;
  if (opt.order && hashed && !attn && !ip && kind == NANN_SCORER_L2 && ix->n_pivots >= 2 && n_queries > p.slots &&
      order_offset(p, n_queries, workspace_bytes, &order_off)) {
    unsigned char* ow = static_cast<unsigned char*>(workspace) + order_off;
    unsigned int* heads = reinterpret_cast<unsigned int*>(ow);
    int32_t* perm = reinterpret_cast<int32_t*>(ow + kOrderSegs * kOrderHeadStride * 4);
    int32_t* key = perm + n_queries;
    rc = launch_order(ix, q, (int)n_queries, key, perm, heads, static_cast<unsigned int*>(workspace), st);
    if (rc) return rc;
    a.perm = perm;
    a.xheads = heads;
  } else {
    HIP_TRY(hipMemsetAsync(workspace, 0, 256, st));
  }
  // main launch, then -- hash-set plans -- the rerun of the queries whose set could have overflowed on the bitmap
  // kernel (its workgroups leave at once when there is none)
  auto both = [&](auto&& launch_on) -> int {
    int r2 = launch_on(p.vis, p.nt, p.slots, p.lds_bytes);
    if (!r2 && hashed) {
      a.redo = 1;
      a.perm = nullptr;
      a.xheads = nullptr;
      r2 = launch_on(p.fb_vis, kNT, p.fb_slots, p.fb_lds_bytes);
    }
    if (cache) projection_used(*cache, tab, st);
    return r2;
  };
  if (attn) {
    a.attn = attn->P;
    if (tab) {  // the default form: q_ and the e rows of DNN layer 1 pre-projected per (model, index) (nann_attn_proj.h)
      auto launch = attn->precision == NANN_MLP_SPLIT_F16 ? launch_search_attn_proj : launch_search_attn_xproj;
      // split-f16 on the 16K-slot plan: the form with keys and weights resident for a scoring call (the bitmap plans and the
      // overflow rerun keep the slice-ring form)
      const bool resident = attn->precision == NANN_MLP_SPLIT_F16;
      return both([&](int vis, int, int slots, size_t lds) {
        if (resident && vis == VIS_LDS_HASH && !a.redo) return launch_search_attn_res(slots, lds, a, st);
        return launch(vis, slots, lds, a, st);
      });
    }
    auto launch = attn->precision == NANN_MLP_SPLIT_F16 ? launch_search_attn_split : launch_search_attn;
    return both([&](int vis, int, int slots, size_t lds) { return launch(ix->desc.d, dt, vis, slots, lds, a, st); });
  }
  a.mlp = scorer->mlp;
  a.phase = 0;
  const int exact = scorer->desc.kind == NANN_SCORER_MLP && (scorer->desc.precision == NANN_MLP_EXACT_F32 || mlp_cert);
  if (mlp_res && p.phased) {
    // The default form of both precisions at beams that fit the 16K-slot set: the pipeline of phases (nann_mlp6.h).  Per
    // chunk of <= 1024 queries: traversal stage 0, then for every round its scoring launch and the
    // traversal stage behind it; last the rerun of the queries whose set could have overflowed (fused kernel, HBM bitmap).
    DeviceInfo di;
    rc = device_info(&di);
    if (rc) return rc;
    const int k5 = level_topn[5];
    for (int64_t c0 = 0; c0 < n_queries && !rc; c0 += kPhaseChunk) {
      SearchArgs c = a;
      c.n_queries = (int)std::min<int64_t>(kPhaseChunk, n_queries - c0);
      c.q = q + (size_t)c0 * a.d;
      if (tq) c.tq = tq + (size_t)c0 * 6;
      c.out_ids = out_item_ids + (size_t)c0 * k5;
      if (out_scores) c.out_scores = out_scores + (size_t)c0 * k5;
      if (out_index) c.out_index = out_index + (size_t)c0 * k5;
      c.status = status + c0;
      if (counters) c.counters = counters + (size_t)c0 * 3 * NANN_NUM_ROUNDS;
      if (phase_ticks) c.phase_ticks = reinterpret_cast<long long*>(phase_ticks) + (size_t)c0 * NANN_NUM_PHASES;
      if (c0 && mlp_cert) {  // (the certified form's refined counts add up over the chunks)
        HIP_TRY(hipMemsetAsync(workspace, 0, offsetof(WsHeader, refined), st));
        HIP_TRY(hipMemsetAsync(static_cast<unsigned char*>(workspace) + offsetof(WsHeader, pad2), 0, 256 - offsetof(WsHeader, pad2), st));
      } else if (c0) HIP_TRY(hipMemsetAsync(workspace, 0, 256, st));
      const int slots = (int)std::min<int64_t>(c.n_queries, (int64_t)p.phase_slots);
      for (int ph = 0; ph <= NANN_NUM_ROUNDS && !rc; ++ph) {
        c.phase = ph;
        rc = launch_search_mlp_phase(p.phase_vis, slots, p.phase_lds_bytes, c, st);
        if (!rc && ph < NANN_NUM_ROUNDS) {
          rc = mlp_cert ? launch_mlp_phase_certified(c, ph, p.phase_score_wgs, st)
                        : launch_mlp_phase_score(exact, c, ph, p.phase_score_wgs, st);
        }
      }
      if (!rc) {
        c.redo = 1;
        c.phase = 0;
        rc = launch_search_mlp_res(exact, p.fb_vis, p.fb_slots, p.fb_lds_bytes, c, st);
      }
    }
    if (cache) projection_used(*cache, tab, st);
    return rc;
  }
  if (mlp_res)  // wide beams / large shards / forced plans: the fused kernel with layer 2 resident in LDS (nann_mlp5.h)
    return both([&](int vis, int, int slots, size_t lds) {
      return launch_search_mlp_res(exact, vis, slots, lds, a, st);
    });
  if (plan_out) plan_out->lean = takes_lean_kernel(opt, scorer->desc.kind, p.vis, a) ? 1 : 0;
  return both([&](int vis, int nt, int slots, size_t lds) {
    return launch_search_any(ix->desc.d / 8, dt, scorer->desc.kind, mlp_split, vis, nt, slots, lds, a, st,
                             takes_lean_kernel(opt, scorer->desc.kind, vis, a));
  });
}

// ---- the probe of nann_index_create ---------------------------------------------------------------------------------
// plan_search has to know how many ids a level's visited set will hold BEFORE it launches (16K-slot set, two workgroups per
// CU; 32K-slot set, one; bitmap).  That is a property of the graph -- degrees, and how much the neighbourhoods of a beam's
// rows overlap -- which no formula over the mean degree captures for every builder.  So the index
// measures it once: 64 of its own rows as queries, ef = min(64, #enter points), L2 scorer, on the HBM-bitmap plan (which
// cannot overflow); from the kernel's per-round counters, new nodes found per frontier row over the three level-0 rounds.
__global__ void k_probe_queries(const void* emb, int dt, int d, long long n_items, int nq, float* q) {
  const int j = blockIdx.x;
  const long long row = (long long)j * (n_items / nq);
  for (int k = threadIdx.x; k < d; k += blockDim.x) {
    float v;
    if (dt == NANN_F32) v = static_cast<const float*>(emb)[row * d + k];
    else {
      const uint32_t h = static_cast<const uint16_t*>(emb)[row * d + k];
      v = dt == NANN_F16 ? half_bits_to_float(h) : bf16_bits_to_float(h);
    }
    q[(size_t)j * d + k] = v;
  }
}

// ---- the pivots of the batch order ------------------------------------------------------------------------------------
// Farthest-point sample of the enter points (the graph's upper levels, spread over the corpus by construction): P of
// them, P = order_pivots(n_enter, d).  Their rows are gathered to f32 once on the NULL stream (blocking, like the probe).
__global__ void k_order_gather(const void* emb, int dt, int d, const int32_t* rows, int m, float* out) {
  for (int k = threadIdx.x; k < d; k += blockDim.x) out[(size_t)blockIdx.x * d + k] = order_row_elem(emb, dt, (size_t)rows[blockIdx.x] * d + k);
}

// key and order kernels on `st`: key[n] (scratch), perm[n], the segment heads and the workspace header zeroed
static_assert(sizeof(WsHeader) <= kOrderHeaderWords * 4 && kOrderHeaderWords * 4 == 256, "k_order_perm clears the header");
int nann::launch_order(const nann_index* ix, const float* q, int n, int32_t* key, int32_t* perm, unsigned int* heads,
                        unsigned int* header, hipStream_t st) {
  const int d = ix->desc.d, P = ix->n_pivots;
  const size_t lds = ((size_t)d * P + kOrderMaxPivots + (size_t)kOrderKeyQueries * d) * 4;
  if (lds > 48 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_order_key), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_order_key, dim3((unsigned)((n + kOrderKeyQueries - 1) / kOrderKeyQueries)), dim3(256), lds, st,
                     ix->pivots, d, P, q, n, key);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_order_perm, dim3(1), dim3(kOrderSortThreads), 0, st, key, n, P, perm, heads, header);
  HIP_TRY(hipGetLastError());
  return NANN_OK;
}

void nann::choose_pivots(nann_index* ix, const std::vector<int32_t>& enter) {
  const int d = ix->desc.d;
  const int P = order_pivots((int64_t)enter.size(), d);
  if (P < 2) return;
  constexpr size_t kMaxCand = 1024;  // candidates: the enter points, strided down to at most this many
  const size_t E = enter.size(), m = std::min(E, kMaxCand);
  std::vector<int32_t> cand(m);
  for (size_t i = 0; i < m; ++i) cand[i] = enter[i * E / m];
  int32_t* rows = nullptr;
  float* buf = nullptr;
  std::vector<float> x(m * (size_t)d);
  bool ok = hipMalloc(&rows, m * 4) == hipSuccess && hipMalloc(&buf, m * (size_t)d * 4) == hipSuccess &&
            hipMemcpy(rows, cand.data(), m * 4, hipMemcpyHostToDevice) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(k_order_gather, dim3((unsigned)m), dim3(128), 0, nullptr, ix->desc.item_embs, ix->desc.emb_dtype, d, rows, (int)m, buf);
    ok = hipGetLastError() == hipSuccess && hipMemcpy(x.data(), buf, x.size() * 4, hipMemcpyDeviceToHost) == hipSuccess;
  }
  if (buf) (void)hipFree(buf);
  if (rows) (void)hipFree(rows);
  if (!ok) return;
  std::vector<size_t> piv;
  std::vector<double> dist(m, INFINITY);
  size_t cur = 0;
  for (int p = 0; p < P; ++p) {
    piv.push_back(cur);
    size_t far = cur;
    for (size_t i = 0; i < m; ++i) {
      double s = 0.0;
      for (int k = 0; k < d; ++k) { const double t = (double)x[i * d + k] - (double)x[cur * d + k]; s += t * t; }
      dist[i] = std::min(dist[i], s);
      if (dist[i] > dist[far]) far = i;
    }
    if (dist[far] <= 0.0) break;  // (fewer distinct rows than P)
    cur = far;
  }
  if (piv.size() < 2) return;
  const size_t np = piv.size();
  std::vector<float> t((size_t)d * np + kOrderMaxPivots, 0.0f);  // [d][np], then the norms
  for (size_t p = 0; p < np; ++p) {
    float s = 0.0f;
    for (int k = 0; k < d; ++k) {
      const float v = x[piv[p] * d + k];
      t[(size_t)k * np + p] = v;
      s += v * v;
    }
    t[(size_t)d * np + p] = s;
  }
  float* dev = nullptr;
  if (hipMalloc(&dev, t.size() * 4) != hipSuccess) return;
  if (hipMemcpy(dev, t.data(), t.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(dev); return; }
  ix->pivots = dev;
  ix->n_pivots = (int)piv.size();
}

void nann::probe_index(nann_index* ix) {
  ix->probe_valid = false;
  // opt-out: NANN_INDEX_PROBE=0 -- the planner then falls back to its degree-based guess.  The probe allocates,
  // launches on the NULL stream and copies back with blocking copies: it SYNCHRONISES the device (include/nann_hip.h says so).
  static const bool enabled = [] { const char* e = std::getenv("NANN_INDEX_PROBE"); return !(e && e[0] == '0'); }();
  if (!enabled) return;
  const std::string saved_error = nann::g_err;  // a probe that fails must not leave ITS message behind a successful create
  struct RestoreError { const std::string& s; ~RestoreError() { nann::g_err = s; } } restore{saved_error};
  const int d = ix->desc.d;
  const int64_t E = ix->desc.n_enter, N = ix->desc.n_items;
  if (E < 8 || N < 4096) return;  // (toy indices: the degree-based guess)
  const int nq = 64, e = (int)std::min<int64_t>(64, E);
  const int32_t t[6] = {e, e, e, e, e, std::min(e, 10)};
  nann_scorer_desc sd{};
  sd.kind = NANN_SCORER_L2; sd.d = d; sd.emb_dtype = ix->desc.emb_dtype;
  nann_scorer* sc = nullptr;
  if (nann_scorer_create(&sd, &sc) != NANN_OK) return;
  nann_search_options o;
  nann_search_options_init(&o);
  o.traversal_mode = NANN_TRAVERSAL_HBM_BITMAP;
  o.slot_reserve = 0;
  int64_t ws_bytes = 0;
  const size_t n_ctr = (size_t)nq * 3 * NANN_NUM_ROUNDS;
  unsigned char* buf = nullptr;
  std::vector<int32_t> h_ctr(n_ctr), h_st((size_t)nq);
  bool ok = nann_search_workspace_bytes(ix, t, nq, &ws_bytes) == NANN_OK;
  const size_t off_q = ((size_t)ws_bytes + 255) & ~(size_t)255, off_ids = off_q + (size_t)nq * d * 4,
               off_st = off_ids + (size_t)nq * t[5] * 8, off_ctr = off_st + (size_t)nq * 4, total = off_ctr + n_ctr * 4;
  ok = ok && hipMalloc(reinterpret_cast<void**>(&buf), total) == hipSuccess;
  if (ok) {
    hipStream_t st = nullptr;
    hipLaunchKernelGGL(k_probe_queries, dim3(nq), dim3(128), 0, st, ix->desc.item_embs, ix->desc.emb_dtype, d, (long long)N, nq,
                       reinterpret_cast<float*>(buf + off_q));
    ok = search_impl(ix, scored_by(ix, sc, nullptr), reinterpret_cast<const float*>(buf + off_q), nullptr, nullptr, nq, t, nullptr, buf, ws_bytes,
                     reinterpret_cast<int64_t*>(buf + off_ids), nullptr, nullptr, reinterpret_cast<int32_t*>(buf + off_st),
                     reinterpret_cast<int32_t*>(buf + off_ctr), nullptr, &o, nullptr, st) == NANN_OK;
    ok = ok && hipMemcpy(h_ctr.data(), buf + off_ctr, n_ctr * 4, hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(h_st.data(), buf + off_st, (size_t)nq * 4, hipMemcpyDeviceToHost) == hipSuccess;
  }
  if (buf) (void)hipFree(buf);
  nann_scorer_destroy(sc);
  // only the probe's own non-sticky error (a failed hipMalloc, say) is cleared; a sticky device error stays set and the
  // caller's next HIP call reports it
  if (!ok) (void)hipGetLastError();
  if (!ok) return;
  double sum = 0.0, mx = 0.0;
  int n_valid = 0;
  std::vector<double> ratios;
  for (int j = 0; j < nq; ++j) {
    if (h_st[(size_t)j] != NANN_OK) continue;
    const int32_t* c = h_ctr.data() + (size_t)j * 3 * NANN_NUM_ROUNDS;  // [F | G | S][round]
    double rows = 0.0, fresh = 0.0;
    for (int r = 2; r <= 4; ++r) { rows += c[0 * NANN_NUM_ROUNDS + r]; fresh += c[2 * NANN_NUM_ROUNDS + r]; }
    if (rows <= 0.0) continue;
    const double ratio = fresh / rows;
    sum += ratio; mx = std::max(mx, ratio);
    ratios.push_back(ratio);
    ++n_valid;
  }
  if (n_valid < 8) return;  // (a corpus whose clusters a beam exhausts: nothing to learn from failed requests)
  ix->probe_valid = true;
  ix->probe_ef = e;
  ix->probe_queries = n_valid;
  std::sort(ratios.begin(), ratios.end());
  ix->probe_new_per_row_mean = (float)(sum / n_valid);
  ix->probe_new_per_row_q90 = (float)ratios[(size_t)(0.9 * (double)(n_valid - 1))];
  ix->probe_new_per_row_max = (float)mx;
}

// ---- the serving traversal: under a scorer (x: q f32[n, d]) or whatever model the node names (x: comm_seq f16[n, seq_len, E]) ----
// the pointers a call cannot do without: a model form's include its sequences and its workspace (a scorer form reports a null
// workspace as a short one)
static bool traverse_null(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, bool model, const void* x,
                          const int32_t* level_topn_max, const void* out_item_ids, const void* status, const void* workspace) {
  return !ix || !level_topn_max || !out_item_ids || !status || (model ? !m || !x || !workspace : !scorer);
}

// tq: optional device i32[n_queries, 6], level_topn per query.  `who`: the entry point in a message.
static int traverse(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, bool model, const void* x, int64_t n_queries,
                    const int32_t level_topn_max[6], const int32_t* tq, void* workspace, int64_t workspace_bytes,
                    int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* status, int32_t* counters,
                    int64_t* phase_ticks, const nann_search_options* options, nann_search_plan* plan, nann_stream_t stream,
                    const char* who) {
  if (traverse_null(ix, scorer, m, model, x, level_topn_max, out_item_ids, status, workspace))
    return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  if (n_queries <= 0) return NANN_OK;
  const ScoredBy by = scored_by(ix, scorer, m);
  if (by.mismatch) return disagree(by);
  hipStream_t st = as_stream(stream);
  // a scorer form looks at its options before its workspace (search_impl), and holds the workspace to the plan it runs
  if (!model) {
    if (tq && phase_ticks) return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": phase ticks with a uniform level_topn only");
    return search_impl(ix, by, static_cast<const float*>(x), nullptr, nullptr, n_queries, level_topn_max, tq, workspace,
                       workspace_bytes, out_item_ids, out_scores, out_index, status, counters, phase_ticks, options, plan, st);
  }
  // a model form looks at its workspace first and holds it to the size it named: its query is staged before search_impl reads the options
  TraverseBytes b;
  int rc = traverse_bytes(ix, m, level_topn_max, n_queries, false, &b);
  if (rc) return rc;
  if (workspace_bytes < b.inner) return short_workspace("nann_search_model");
  const float *q = nullptr, *kt = nullptr, *upad = nullptr;
  rc = stage_model_query(by, x, n_queries, static_cast<unsigned char*>(workspace) + b.query_off, false, stream, &q, &kt, &upad);
  if (rc) return rc;
  return search_impl(ix, by, q, kt, upad, n_queries, level_topn_max, tq, workspace, b.search, out_item_ids, out_scores, out_index,
                     status, counters, nullptr, options, plan, st);
}

// ---- the traversal, filtered at its final selection: the inner search at the fetch width F = level_topn_max[5] into the
// staging area behind its own workspace (under `inner_who`, its unfiltered twin's name), then k_filter_compact ------------
static int traverse_filtered(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, bool model, const void* x,
                             int64_t n_queries, const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace,
                             int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* status,
                             int32_t* counters, int64_t* phase_ticks, const nann_search_options* options, nann_search_plan* plan,
                             const nann_filter* filter, int32_t k, int32_t* n_out, nann_stream_t stream, const char* who,
                             const char* inner_who, const PredArgs* pred = nullptr) {  // pred: a _where form's predicates, resolved
  if (traverse_null(ix, scorer, m, model, x, level_topn_max, out_item_ids, status, workspace))
    return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  const int f = level_topn_max[5];
  if (k < 0 || k > f) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": k must lie in [0, level_topn_max[5]]");  // (also of an empty batch)
  if (n_queries <= 0) return NANN_OK;
  FilterArgs fa;
  int rc = resolve_filter(filter, ix, &fa);  // (a malformed filter fails the call before anything is launched)
  if (rc) return rc;
  TraverseBytes b;
  rc = traverse_bytes(ix, m, level_topn_max, n_queries, true, &b);
  if (rc) return rc;
  // (both forms: the filtered call's own workspace ahead of everything the inner search looks at, its options included)
  if (!workspace || workspace_bytes < b.total) return short_workspace(who);
  unsigned char* stage = static_cast<unsigned char*>(workspace) + b.stage_off;
  int64_t* s_ids = reinterpret_cast<int64_t*>(stage);
  float* s_scores = reinterpret_cast<float*>(stage + (size_t)n_queries * f * 8);
  int32_t* s_rows = reinterpret_cast<int32_t*>(stage + (size_t)n_queries * f * 12);
  rc = traverse(ix, scorer, m, model, x, n_queries, level_topn_max, level_topn, workspace, b.inner, s_ids, s_scores, s_rows, status,
                counters, phase_ticks, options, plan, stream, inner_who);
  if (rc) return rc;
  // (the shape both compactions hold their launch to stands since before the inner search: 0 <= k <= f above, and plan_search
  // refuses a level_topn entry beyond kMaxK before the inner search launches anything)
  if (pred) {  // k_pred_compact in the place of k_filter_compact: a query's own level_topn[5] entries, none when it failed
    PredCompactArgs pc = {};
    pc.f = fa;
    pc.p = *pred;
    pc.in_rows = s_rows;
    pc.in_scores = s_scores;
    pc.in_stride = pc.n_in = f;
    pc.n_valid = level_topn ? level_topn + 5 : nullptr;
    pc.nv_stride = 6;
    pc.status = status;
    pc.k = k;
    pc.item_ids = ix->desc.item_ids;
    pc.out_item_ids = out_item_ids;
    pc.out_scores = out_scores;
    pc.out_index = out_index;
    pc.n_out = n_out;
    return launch_pred_compact(pc, (long long)n_queries, as_stream(stream));
  }
  return launch_filter_compact(fa, s_rows, s_scores, f, f, level_topn, status, 0, n_queries, k, ix->desc.item_ids, out_item_ids,
                               out_scores, out_index, n_out, as_stream(stream));
}

// ---- the traversal under a group cap: traverse_filtered's walk -- the same checks in the same order, the same workspace and
// staging layout, the same inner search at the fetch width F = level_topn_max[5] -- with k_group_cap (nann_groupcap.h), which
// applies the filter and then the cap, in the place of k_filter_compact -----------------------------------------------------
static int traverse_grouped(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, bool model, const void* x,
                            int64_t n_queries, const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace,
                            int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* status,
                            int32_t* counters, int64_t* phase_ticks, const nann_search_options* options, nann_search_plan* plan,
                            const nann_filter* filter, const nann_groups* groups, int32_t k, int32_t* out_group, int32_t* n_out,
                            nann_stream_t stream, const char* who, const char* inner_who) {
  if (traverse_null(ix, scorer, m, model, x, level_topn_max, out_item_ids, status, workspace))
    return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  const int f = level_topn_max[5];
  if (k < 0 || k > f) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": k must lie in [0, level_topn_max[5]]");  // (also of an empty batch)
  GroupCapArgs a = {};
  int rc = resolve_groups(groups, who, &a);
  if (rc) return rc;
  if (n_queries <= 0) return NANN_OK;
  rc = resolve_filter(filter, ix, &a.f);  // (a malformed filter fails the call before anything is launched)
  if (rc) return rc;
  TraverseBytes b;
  rc = traverse_bytes(ix, m, level_topn_max, n_queries, true, &b);
  if (rc) return rc;
  if (!workspace || workspace_bytes < b.total) return short_workspace(who);
  unsigned char* stage = static_cast<unsigned char*>(workspace) + b.stage_off;
  int64_t* s_ids = reinterpret_cast<int64_t*>(stage);
  float* s_scores = reinterpret_cast<float*>(stage + (size_t)n_queries * f * 8);
  int32_t* s_rows = reinterpret_cast<int32_t*>(stage + (size_t)n_queries * f * 12);
  rc = traverse(ix, scorer, m, model, x, n_queries, level_topn_max, level_topn, workspace, b.inner, s_ids, s_scores, s_rows, status,
                counters, phase_ticks, options, plan, stream, inner_who);
  if (rc) return rc;
  a.in_rows = s_rows;
  a.in_scores = s_scores;
  a.k_in = f;
  a.n_valid = level_topn ? level_topn + 5 : nullptr;  // a query's own level_topn[5]
  a.nv_stride = 6;
  a.status = status;
  a.k = k;
  a.item_ids = ix->desc.item_ids;
  a.out_index = out_index;
  a.out_scores = out_scores;
  a.out_item_ids = out_item_ids;
  a.out_group = out_group;
  a.n_out = n_out;
  return launch_group_cap(a, (long long)n_queries, as_stream(stream));
}

// ---- the traversal, diversified: traverse_grouped's walk -- the same checks in the same order, the same workspace and staging
// layout, the same inner search at the fetch width F = level_topn_max[5] -- with k_mmr (nann_mmr.h), which applies the filter
// and then re-ranks, in the place of the cap ----------------------------------------------------------------------------------
static int traverse_diverse(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, bool model, const void* x,
                            int64_t n_queries, const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace,
                            int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* status,
                            int32_t* counters, int64_t* phase_ticks, const nann_search_options* options, nann_search_plan* plan,
                            const nann_filter* filter, const nann_diversity* diversity, int32_t k, float* out_mmr,
                            int32_t* out_pos, int32_t* n_out, nann_stream_t stream, const char* who, const char* inner_who) {
  if (traverse_null(ix, scorer, m, model, x, level_topn_max, out_item_ids, status, workspace))
    return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  const int f = level_topn_max[5];
  if (k < 0 || k > f) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": k must lie in [0, level_topn_max[5]]");  // (also of an empty batch)
  MmrArgs a = {};
  int rc = resolve_diversity(diversity, who, &a);
  if (rc) return rc;
  if (n_queries <= 0) return NANN_OK;
  FilterArgs fa;
  rc = resolve_filter(filter, ix, &fa);  // (a malformed filter fails the call before anything is launched)
  if (rc) return rc;
  rc = mmr_index(ix, who, &a);
  if (rc) return rc;
  a.f = fa;
  TraverseBytes b;
  rc = traverse_bytes(ix, m, level_topn_max, n_queries, true, &b);
  if (rc) return rc;
  if (!workspace || workspace_bytes < b.total) return short_workspace(who);
  unsigned char* stage = static_cast<unsigned char*>(workspace) + b.stage_off;
  int64_t* s_ids = reinterpret_cast<int64_t*>(stage);
  float* s_scores = reinterpret_cast<float*>(stage + (size_t)n_queries * f * 8);
  int32_t* s_rows = reinterpret_cast<int32_t*>(stage + (size_t)n_queries * f * 12);
  rc = traverse(ix, scorer, m, model, x, n_queries, level_topn_max, level_topn, workspace, b.inner, s_ids, s_scores, s_rows, status,
                counters, phase_ticks, options, plan, stream, inner_who);
  if (rc) return rc;
  a.in_rows = s_rows;
  a.in_scores = s_scores;
  a.k_in = f;
  a.n_valid = level_topn ? level_topn + 5 : nullptr;  // a query's own level_topn[5]
  a.nv_stride = 6;
  a.status = status;
  a.k = k;
  a.out_index = out_index;
  a.out_scores = out_scores;
  a.out_mmr = out_mmr;
  a.out_pos = out_pos;
  a.out_item_ids = out_item_ids;
  a.n_out = n_out;
  return launch_mmr(a, (long long)n_queries, as_stream(stream));
}

// ---- the traversal over a user's interest vectors: the inner search over the n_users * n_vec vectors at the fetch width
// F = level_topn_max[5] into the staging area a filtered call has behind its workspace, then the union top-k (nann_union.h)
// of each user's n_vec lists, its workspace behind the staging area ---------------------------------------------------------
// fused: the nann_search_multi_fused form -- the fuse (nann_fuse.h) stands where the union does, with its own limit and workspace
static int traverse_multi_check(int64_t n_users, int32_t n_vec, const int32_t level_topn_max[6], int64_t k, const char* who,
                                bool fused = false) {
  if (n_vec < 1) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": n_vec < 1");
  const int64_t f = level_topn_max[5];
  if (k < 0 || k > (int64_t)n_vec * f) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": k must lie in [0, n_vec * level_topn_max[5]]");
  if (n_users > 0 && n_users > 0x7fffffffll / n_vec) return fail(NANN_ERR_UNSUPPORTED, "too many queries in one call");
  if (fused) return fuse_shape_check(std::max<int64_t>(n_users, 0), n_vec, f, k, who);
  return union_check(std::max<int64_t>(n_users, 0), n_vec, f, k, who);
}
// b->total: the filtered layout over the vectors (its end is where the union's workspace starts); *total: with the union's
static int traverse_multi_bytes(const nann_index* ix, const int32_t level_topn_max[6], int64_t n_users, int32_t n_vec,
                                TraverseBytes* b, int64_t* total, bool fused = false) {
  const int rc = traverse_bytes(ix, nullptr, level_topn_max, n_users * n_vec, true, b);
  if (rc) return rc;
  const long long n_in = (long long)n_vec * level_topn_max[5];
  *total = up256_i64(b->total) + (int64_t)(fused ? fuse_ws_bytes((long long)n_users, n_in) : union_ws_bytes((long long)n_users, n_in));
  return NANN_OK;
}

static int traverse_multi(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_users, int32_t n_vec,
                          const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace, int64_t workspace_bytes,
                          int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* out_vec, int32_t* n_out,
                          int32_t* status, int32_t* counters, const nann_search_options* options, nann_search_plan* plan, int32_t k,
                          nann_stream_t stream, const char* who, bool fused = false, const nann_fusion* fusion = nullptr,
                          uint64_t* out_lists = nullptr) {
  if (traverse_null(ix, scorer, nullptr, false, q, level_topn_max, out_item_ids, status, workspace))
    return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  int rc = traverse_multi_check(n_users, n_vec, level_topn_max, k, who, fused);  // (also of an empty batch)
  if (rc) return rc;
  if (fused) rc = fusion_check(fusion, who);
  if (rc) return rc;
  if (n_users <= 0 || k == 0) return NANN_OK;  // (nothing to return: no inner search either, as nann_union_topk)
  if (!q) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  const int64_t n = n_users * n_vec;
  const int f = level_topn_max[5];
  TraverseBytes b;
  int64_t total = 0;
  rc = traverse_multi_bytes(ix, level_topn_max, n_users, n_vec, &b, &total, fused);
  if (rc) return rc;
  // (the call's own workspace ahead of everything the inner search looks at, its options included)
  if (!workspace || workspace_bytes < total) return short_workspace(who);
  if (reinterpret_cast<uintptr_t>(workspace) & 255u) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": workspace must be 256-byte aligned");
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  unsigned char* stage = ws + b.stage_off;
  int64_t* s_ids = reinterpret_cast<int64_t*>(stage);
  float* s_scores = reinterpret_cast<float*>(stage + (size_t)n * f * 8);
  int32_t* s_rows = reinterpret_cast<int32_t*>(stage + (size_t)n * f * 12);
  rc = traverse(ix, scorer, nullptr, false, q, n, level_topn_max, level_topn, workspace, b.inner, s_ids, s_scores, s_rows, status,
                counters, nullptr, options, plan, stream, "nann_search_opt");
  if (rc) return rc;
  if (fused) {  // the fuse (nann_fuse.h) in the place of the union, over the same lists
    FuseArgs a = {};
    a.scores = s_scores;
    a.rows = s_rows;
    a.n_valid = level_topn ? level_topn + 5 : nullptr;
    a.nv_stride = 6;
    a.status = status;
    a.n_lists = n_vec;
    a.k_in = f;
    a.k = k;
    a.n_items = (long long)ix->desc.n_items;
    a.item_ids = ix->desc.item_ids;
    fusion_into(fusion, &a);
    a.ws = ws + up256_i64(b.total);
    a.out_index = out_index;
    a.out_scores = out_scores;
    a.out_item_ids = out_item_ids;
    a.out_lists = reinterpret_cast<unsigned long long*>(out_lists);
    a.n_out = n_out;
    return launch_fuse_topk(a, (long long)n_users, as_stream(stream));
  }
  UnionArgs a = {};
  a.scores = s_scores;
  a.rows = s_rows;
  a.n_valid = level_topn ? level_topn + 5 : nullptr;  // a vector's own level_topn[5]
  a.nv_stride = 6;
  a.status = status;
  a.n_lists = n_vec;
  a.k_in = f;
  a.k = k;
  a.n_items = (long long)ix->desc.n_items;
  a.item_ids = ix->desc.item_ids;
  a.best = reinterpret_cast<unsigned long long*>(ws + up256_i64(b.total));
  a.out_index = out_index;
  a.out_scores = out_scores;
  a.out_item_ids = out_item_ids;
  a.out_list = out_vec;
  a.n_out = n_out;
  return launch_union_topk(a, (long long)n_users, as_stream(stream));
}

// ---- the entry points (include/nann_hip.h) -----------------------------------------------------------------------------------
extern "C" {

int nann_search_diverse_workspace_bytes(const nann_index* ix, const int32_t level_topn[6], int64_t n_queries, int64_t* nbytes) {
  return traverse_size(ix, nullptr, false, level_topn, n_queries, true, nbytes);
}
int nann_search_diverse(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries,
                        const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace, int64_t workspace_bytes,
                        int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* status, int32_t* counters,
                        int64_t* phase_ticks, const nann_search_options* options, nann_search_plan* plan,
                        const nann_filter* filter, const nann_diversity* diversity, int32_t k, float* out_mmr, int32_t* out_pos,
                        int32_t* n_out, nann_stream_t stream) {
  return traverse_diverse(ix, scorer, nullptr, false, q, n_queries, level_topn_max, level_topn, workspace, workspace_bytes,
                          out_item_ids, out_scores, out_index, status, counters, phase_ticks, options, plan, filter, diversity, k,
                          out_mmr, out_pos, n_out, stream, "nann_search_diverse", "nann_search_opt");
}
int nann_search_model_diverse_workspace_bytes(const nann_index* ix, const nann_model* m, const int32_t level_topn[6],
                                              int64_t n_queries, int64_t* nbytes) {
  return traverse_size(ix, m, true, level_topn, n_queries, true, nbytes);
}
int nann_search_model_diverse(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_queries,
                              const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace,
                              int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                              int32_t* status, int32_t* counters, const nann_search_options* options, nann_search_plan* plan,
                              const nann_filter* filter, const nann_diversity* diversity, int32_t k, float* out_mmr,
                              int32_t* out_pos, int32_t* n_out, nann_stream_t stream) {
  return traverse_diverse(ix, nullptr, m, true, comm_seq_f16, n_queries, level_topn_max, level_topn, workspace, workspace_bytes,
                          out_item_ids, out_scores, out_index, status, counters, nullptr, options, plan, filter, diversity, k,
                          out_mmr, out_pos, n_out, stream, "nann_search_model_diverse", "nann_search_model");
}

int nann_search_grouped_workspace_bytes(const nann_index* ix, const int32_t level_topn[6], int64_t n_queries, int64_t* nbytes) {
  return traverse_size(ix, nullptr, false, level_topn, n_queries, true, nbytes);
}
int nann_search_grouped(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries,
                        const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace, int64_t workspace_bytes,
                        int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* status, int32_t* counters,
                        int64_t* phase_ticks, const nann_search_options* options, nann_search_plan* plan,
                        const nann_filter* filter, const nann_groups* groups, int32_t k, int32_t* out_group, int32_t* n_out,
                        nann_stream_t stream) {
  return traverse_grouped(ix, scorer, nullptr, false, q, n_queries, level_topn_max, level_topn, workspace, workspace_bytes,
                          out_item_ids, out_scores, out_index, status, counters, phase_ticks, options, plan, filter, groups, k,
                          out_group, n_out, stream, "nann_search_grouped", "nann_search_opt");
}
int nann_search_model_grouped_workspace_bytes(const nann_index* ix, const nann_model* m, const int32_t level_topn[6],
                                              int64_t n_queries, int64_t* nbytes) {
  return traverse_size(ix, m, true, level_topn, n_queries, true, nbytes);
}
int nann_search_model_grouped(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_queries,
                              const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace,
                              int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                              int32_t* status, int32_t* counters, const nann_search_options* options, nann_search_plan* plan,
                              const nann_filter* filter, const nann_groups* groups, int32_t k, int32_t* out_group,
                              int32_t* n_out, nann_stream_t stream) {
  return traverse_grouped(ix, nullptr, m, true, comm_seq_f16, n_queries, level_topn_max, level_topn, workspace, workspace_bytes,
                          out_item_ids, out_scores, out_index, status, counters, nullptr, options, plan, filter, groups, k,
                          out_group, n_out, stream, "nann_search_model_grouped", "nann_search_model");
}

int nann_search_multi_workspace_bytes(const nann_index* ix, const int32_t level_topn[6], int64_t n_users, int32_t n_vec,
                                      int64_t* nbytes) {
  const char* who = "nann_search_multi_workspace_bytes";
  if (!ix || !level_topn || !nbytes) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  int rc = traverse_multi_check(n_users, n_vec, level_topn, 0, who);
  if (rc) return rc;
  TraverseBytes b;
  int64_t total = 0;
  rc = traverse_multi_bytes(ix, level_topn, std::max<int64_t>(n_users, 0), n_vec, &b, &total);
  if (rc) return rc;
  *nbytes = total;
  return NANN_OK;
}
int nann_search_multi(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_users, int32_t n_vec,
                      const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace, int64_t workspace_bytes,
                      int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* out_vec, int32_t* n_out,
                      int32_t* status, int32_t* counters, const nann_search_options* options, nann_search_plan* plan, int32_t k,
                      nann_stream_t stream) {
  return traverse_multi(ix, scorer, q, n_users, n_vec, level_topn_max, level_topn, workspace, workspace_bytes, out_item_ids,
                        out_scores, out_index, out_vec, n_out, status, counters, options, plan, k, stream, "nann_search_multi");
}

int nann_search_multi_fused_workspace_bytes(const nann_index* ix, const int32_t level_topn[6], int64_t n_users, int32_t n_vec,
                                            int64_t* nbytes) {
  const char* who = "nann_search_multi_fused_workspace_bytes";
  if (!ix || !level_topn || !nbytes) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  int rc = traverse_multi_check(n_users, n_vec, level_topn, 0, who, true);
  if (rc) return rc;
  TraverseBytes b;
  int64_t total = 0;
  rc = traverse_multi_bytes(ix, level_topn, std::max<int64_t>(n_users, 0), n_vec, &b, &total, true);
  if (rc) return rc;
  *nbytes = total;
  return NANN_OK;
}
int nann_search_multi_fused(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_users, int32_t n_vec,
                            const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace,
                            int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                            uint64_t* out_lists, int32_t* n_out, int32_t* status, int32_t* counters,
                            const nann_search_options* options, nann_search_plan* plan, int32_t k, const nann_fusion* fusion,
                            nann_stream_t stream) {
  return traverse_multi(ix, scorer, q, n_users, n_vec, level_topn_max, level_topn, workspace, workspace_bytes, out_item_ids,
                        out_scores, out_index, nullptr, n_out, status, counters, options, plan, k, stream, "nann_search_multi_fused",
                        true, fusion, out_lists);
}

int nann_search_workspace_bytes(const nann_index* ix, const int32_t level_topn[6], int64_t n_queries, int64_t* nbytes) {
  return traverse_size(ix, nullptr, false, level_topn, n_queries, false, nbytes);
}
int nann_search_opt(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries,
                    const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace, int64_t workspace_bytes,
                    int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* status, int32_t* counters,
                    int64_t* phase_ticks, const nann_search_options* options, nann_search_plan* plan, nann_stream_t stream) {
  return traverse(ix, scorer, nullptr, false, q, n_queries, level_topn_max, level_topn, workspace, workspace_bytes, out_item_ids,
                  out_scores, out_index, status, counters, phase_ticks, options, plan, stream, "nann_search_opt");
}
int nann_search(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries,
                const int32_t level_topn[6], void* workspace, int64_t workspace_bytes,
                int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* status,
                int32_t* counters, nann_stream_t stream) {
  return nann_search_opt(ix, scorer, q, n_queries, level_topn, nullptr, workspace, workspace_bytes, out_item_ids, out_scores,
                         out_index, status, counters, nullptr, nullptr, nullptr, stream);  // deprecated: thin wrapper
}
int nann_search_ex(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries,
                   const int32_t level_topn[6], void* workspace, int64_t workspace_bytes,
                   int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* status,
                   int32_t* counters, int64_t* phase_ticks, nann_stream_t stream) {
  return nann_search_opt(ix, scorer, q, n_queries, level_topn, nullptr, workspace, workspace_bytes, out_item_ids, out_scores,
                         out_index, status, counters, phase_ticks, nullptr, nullptr, stream);  // deprecated: thin wrapper
}
int nann_search_v(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries,
                  const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace,
                  int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                  int32_t* status, int32_t* counters, nann_stream_t stream) {
  return nann_search_opt(ix, scorer, q, n_queries, level_topn_max, level_topn, workspace, workspace_bytes, out_item_ids,
                         out_scores, out_index, status, counters, nullptr, nullptr, nullptr, stream);  // deprecated: thin wrapper
}

int nann_search_reruns(const void* workspace, int64_t* n_rerun, nann_stream_t stream) {
  if (!workspace || !n_rerun) return fail(NANN_ERR_BAD_ARGUMENT, "nann_search_reruns: null argument");
  unsigned int v = 0;
  HIP_TRY(hipMemcpyAsync(&v, static_cast<const unsigned char*>(workspace) + offsetof(WsHeader, n_redo), 4, hipMemcpyDeviceToHost, as_stream(stream)));
  HIP_TRY(hipStreamSynchronize(as_stream(stream)));
  *n_rerun = v;
  return NANN_OK;
}

int nann_search_refined(const void* workspace, int64_t out[NANN_NUM_ROUNDS], nann_stream_t stream) {
  if (!workspace || !out) return fail(NANN_ERR_BAD_ARGUMENT, "nann_search_refined: null argument");
  unsigned long long v[NANN_NUM_ROUNDS] = {};
  HIP_TRY(hipMemcpyAsync(v, static_cast<const unsigned char*>(workspace) + offsetof(WsHeader, refined), sizeof(v), hipMemcpyDeviceToHost, as_stream(stream)));
  HIP_TRY(hipStreamSynchronize(as_stream(stream)));
  for (int r = 0; r < NANN_NUM_ROUNDS; ++r) out[r] = (int64_t)v[r];
  return NANN_OK;
}

// the serving signature: comm_seq + level_topn -> top_k, for whatever model the node names
int nann_search_model_workspace_bytes(const nann_index* ix, const nann_model* m, const int32_t level_topn[6],
                                      int64_t n_queries, int64_t* nbytes) {
  return traverse_size(ix, m, true, level_topn, n_queries, false, nbytes);
}
int nann_search_model_opt(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_queries,
                          const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace,
                          int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                          int32_t* status, int32_t* counters, const nann_search_options* options, nann_search_plan* plan,
                          nann_stream_t stream) {
  return traverse(ix, nullptr, m, true, comm_seq_f16, n_queries, level_topn_max, level_topn, workspace, workspace_bytes, out_item_ids,
                  out_scores, out_index, status, counters, nullptr, options, plan, stream, "nann_search_model");
}
int nann_search_model(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_queries,
                      const int32_t level_topn[6], void* workspace, int64_t workspace_bytes,
                      int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* status,
                      int32_t* counters, nann_stream_t stream) {
  return nann_search_model_opt(ix, m, comm_seq_f16, n_queries, level_topn, nullptr, workspace, workspace_bytes, out_item_ids,
                               out_scores, out_index, status, counters, nullptr, nullptr, stream);  // deprecated: thin wrapper
}

int nann_search_model_v(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_queries,
                        const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace,
                        int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                        int32_t* status, int32_t* counters, nann_stream_t stream) {
  return nann_search_model_opt(ix, m, comm_seq_f16, n_queries, level_topn_max, level_topn, workspace, workspace_bytes,
                               out_item_ids, out_scores, out_index, status, counters, nullptr, nullptr, stream);  // deprecated: thin wrapper
}

int nann_search_filtered_workspace_bytes(const nann_index* ix, const int32_t level_topn[6], int64_t n_queries, int64_t* nbytes) {
  return traverse_size(ix, nullptr, false, level_topn, n_queries, true, nbytes);
}
int nann_search_filtered(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries,
                         const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace, int64_t workspace_bytes,
                         int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* status, int32_t* counters,
                         int64_t* phase_ticks, const nann_search_options* options, nann_search_plan* plan,
                         const nann_filter* filter, int32_t k, int32_t* n_out, nann_stream_t stream) {
  return traverse_filtered(ix, scorer, nullptr, false, q, n_queries, level_topn_max, level_topn, workspace, workspace_bytes,
                           out_item_ids, out_scores, out_index, status, counters, phase_ticks, options, plan, filter, k, n_out, stream,
                           "nann_search_filtered", "nann_search_opt");
}
int nann_search_model_filtered_workspace_bytes(const nann_index* ix, const nann_model* m, const int32_t level_topn[6],
                                               int64_t n_queries, int64_t* nbytes) {
  return traverse_size(ix, m, true, level_topn, n_queries, true, nbytes);
}
int nann_search_model_filtered(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_queries,
                               const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace,
                               int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                               int32_t* status, int32_t* counters, const nann_search_options* options, nann_search_plan* plan,
                               const nann_filter* filter, int32_t k, int32_t* n_out, nann_stream_t stream) {
  return traverse_filtered(ix, nullptr, m, true, comm_seq_f16, n_queries, level_topn_max, level_topn, workspace, workspace_bytes,
                           out_item_ids, out_scores, out_index, status, counters, nullptr, options, plan, filter, k, n_out, stream,
                           "nann_search_model_filtered", "nann_search_model");
}


// the filtered traversal plus the attribute predicates (nann_predicate.h): the workspace is the filtered call's
int nann_search_where_workspace_bytes(const nann_index* ix, const int32_t level_topn[6], int64_t n_queries, int64_t* nbytes) {
  return traverse_size(ix, nullptr, false, level_topn, n_queries, true, nbytes);
}
int nann_search_where(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries,
                      const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace, int64_t workspace_bytes,
                      int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* status, int32_t* counters,
                      int64_t* phase_ticks, const nann_search_options* options, nann_search_plan* plan,
                      const nann_filter* filter, const nann_predicates* predicates, int32_t k, int32_t* n_out,
                      nann_stream_t stream) {
  PredArgs pa;  // (the predicates in front of everything else of the call, its handles and an empty batch included)
  const int rc = resolve_predicates(predicates, &pa);
  if (rc) return rc;
  return traverse_filtered(ix, scorer, nullptr, false, q, n_queries, level_topn_max, level_topn, workspace, workspace_bytes,
                           out_item_ids, out_scores, out_index, status, counters, phase_ticks, options, plan, filter, k, n_out, stream,
                           "nann_search_where", "nann_search_opt", &pa);
}
int nann_search_model_where_workspace_bytes(const nann_index* ix, const nann_model* m, const int32_t level_topn[6],
                                            int64_t n_queries, int64_t* nbytes) {
  return traverse_size(ix, m, true, level_topn, n_queries, true, nbytes);
}
int nann_search_model_where(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_queries,
                            const int32_t level_topn_max[6], const int32_t* level_topn, void* workspace,
                            int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores, int32_t* out_index,
                            int32_t* status, int32_t* counters, const nann_search_options* options, nann_search_plan* plan,
                            const nann_filter* filter, const nann_predicates* predicates, int32_t k, int32_t* n_out,
                            nann_stream_t stream) {
  PredArgs pa;
  const int rc = resolve_predicates(predicates, &pa);
  if (rc) return rc;
  return traverse_filtered(ix, nullptr, m, true, comm_seq_f16, n_queries, level_topn_max, level_topn, workspace, workspace_bytes,
                           out_item_ids, out_scores, out_index, status, counters, nullptr, options, plan, filter, k, n_out, stream,
                           "nann_search_model_where", "nann_search_model", &pa);
}

}  // extern "C"

// ---- the evaluation graph's traversal (nann_eval.h) ---------------------------------------------------------------------------
// l2: the L2 scorer's instances may keep `seen` in LDS (nann_eval.h) -- a window of the index's bitmap beside their scratch.
// seen_lds: 0 = the slot form, 1 = the LDS form, 2 = the LDS form with more than one window.  l2 == false also sizes the
// workspace: the most slots any plan of this index takes.
struct EvalPlan {
  int cat_cap = 0, slots = 0, seen_lds = 0, n_windows = 1;
  int use_dirty = 0;  // the second-level bitmap of `seen` fits the phase scratch (what the slot form asks; the LDS form always has it)
  int threads = 0;    // eval_plans: the workgroup size of the instance that runs
  unsigned long long slot_bytes = 0;
  uint32_t vis_words = 0, lds_words = 0, win_owners = 0;
};
static int eval_plan(const nann_index* ix, int64_t n_queries, bool l2, EvalPlan* p) {
  DeviceInfo di;
  const int rc = device_info(&di);
  if (rc) return rc;
  // result || next: a frontier holds at most kEvalMaxK rows, a set at most every item
  const int64_t deg = std::max<int64_t>(std::max(ix->max_deg[0], ix->max_deg[1]), 1);
  const int64_t nxt = std::max<int64_t>(std::min<int64_t>(ix->desc.n_items, (int64_t)kEvalMaxK * deg), ix->desc.n_enter);
  if (kEvalMaxK + nxt > 0x3fffffffll) return fail(NANN_ERR_UNSUPPORTED, "candidate bound too large");
  p->cat_cap = (int)(kEvalMaxK + nxt);
  const size_t lds = eval_l2_lds_base() + eval_seen_lds_bytes(ix->bm_words);
  static const bool force_hbm = [] { const char* e = std::getenv("NANN_EVAL_SEEN"); return e && std::string(e) == "hbm"; }();
  // (a thread of the LDS form owns 32 words of the bitmaps' current window; a round sweeps the id space window by window:
  //  nann_eval.h, kEvalWinOwners / kEvalMaxWindows)
  const bool lds_ok = lds <= di.lds_max && !force_hbm && eval_windows(ix->bm_words) <= kEvalMaxWindows && deg < 65536;  // (a row's length rides in 16 bits of its packed bounds)
  p->win_owners = eval_win_owners(ix->bm_words);
  p->n_windows = (int)eval_windows(ix->bm_words);
  p->seen_lds = (l2 && lds_ok) ? (p->n_windows > 1 ? 2 : 1) : 0;
  p->lds_words = (uint32_t)(eval_seen_lds_bytes(ix->bm_words) / 4);
  p->vis_words = eval_vis_words(ix->bm_words);
  unsigned long long off[7];
  p->slot_bytes = eval_slot_layout(ix->bm_words, p->vis_words, p->cat_cap, off);
  // workgroups per CU: two (the slot form: 2048 threads) unless the LDS bitmap leaves room for one
  const int per_cu = p->seen_lds ? 1 : 2;
  p->slots = (int)std::max<int64_t>(1, std::min<int64_t>(n_queries, (int64_t)di.cus * per_cu));
  // the second-level bitmap (nann_eval.h, round 6): one bit per word of `seen`, overlaid on the phase scratch behind the scan
  // scratch -- 256 bytes + 4 per owner of 1 024 items, so it fits shards of up to 256 x (eval_dirty_room() - 256) = 4 718 592
  // items (tests/eval_matrix.py restates the figure); beyond, the slot form keeps round 4's full scans
  p->use_dirty = 256 + (size_t)((ix->bm_words + 31u) >> 5) * 4 <= eval_dirty_room() ? 1 : 0;
  return NANN_OK;
}

// What a call of the evaluation traversal may be scored by (eval_scored_by) and the plan it runs (eval_plans): the one copy
// of the checks and of the choice, which eval_impl launches with and nann_search_eval_plan reports.  pl: the plan of this call;
// sizing: the plan the workspace was sized by (nann_search_eval_workspace_bytes).
static int eval_scored_by(const ScoredBy& by, int64_t n_queries) {
  const nann_scorer* scorer = by.scorer;
  const nann_attn_scorer* attn = by.at;
  if (n_queries > 0x7fffffffll) return fail(NANN_ERR_UNSUPPORTED, "too many queries in one call");
  // the evaluation traversal has an L2, an MLP and an attention form; anything else is refused before a launch or a write
  if (!attn && scorer->desc.kind == NANN_SCORER_IP)
    return fail(NANN_ERR_UNSUPPORTED, "nann_search_eval: the inner-product scorer (NANN_SCORER_IP) is not supported by the evaluation traversal");
  if (!attn && scorer->desc.kind != NANN_SCORER_L2 && scorer->desc.kind != NANN_SCORER_MLP)
    return fail(NANN_ERR_BAD_ARGUMENT, "nann_search_eval: unknown scorer kind");
  return NANN_OK;
}
static int eval_model_kind(const nann_model* m, const char* who) {
  if (m->kind == NANN_MODEL_IP)  // (before the mean of the users' sequences is launched)
    return fail(NANN_ERR_UNSUPPORTED, std::string(who) + ": an inner-product model (NANN_MODEL_IP) is not supported by the evaluation traversal");
  return NANN_OK;
}
static int eval_plans(const nann_index* ix, const ScoredBy& by, int64_t n_queries, EvalPlan* pl, EvalPlan* sizing) {
  const bool l2 = !by.at && by.scorer->desc.kind == NANN_SCORER_L2;
  int rc = eval_plan(ix, n_queries, l2, pl);
  if (!rc) rc = eval_plan(ix, n_queries, false, sizing);  // (the workspace the caller sized: nann_search_eval_workspace_bytes)
  pl->threads = by.at ? kAttnNT : l2 ? kNT : kMlpNT;      // (launch_eval_attn / launch_eval_l2 / launch_eval_mlp_d*)
  return rc;
}

static int eval_impl(const nann_index* ix, const ScoredBy& by, const float* q, const float* kt, const float* upad, int64_t n_queries, const int32_t num_scoring[3],
                     const int32_t top_k[3], int32_t topk_eval, void* workspace, int64_t workspace_bytes,
                     int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* n_out, int32_t* status,
                     int32_t* counters, hipStream_t st) {
  const nann_scorer* scorer = by.scorer;
  const nann_attn_scorer* attn = by.at;
  int rc = eval_scored_by(by, n_queries);
  if (rc) return rc;
  if (num_scoring[2] != 1) return fail(NANN_ERR_BAD_ARGUMENT, "num_scoring_per_level[2] must be 1 (model.py:347)");
  for (int l = 0; l < 3; ++l)
    if (top_k[l] < 1 || top_k[l] > kEvalMaxK || num_scoring[l] < 0)
      return fail(NANN_ERR_UNSUPPORTED, "top_k_per_level entries must be in [1, 2048]");
  if (topk_eval < 1 || topk_eval > kEvalMaxK) return fail(NANN_ERR_UNSUPPORTED, "topk_eval must be in [1, 2048]");
  EvalArgs a;
  const bool l2 = !attn && scorer->desc.kind == NANN_SCORER_L2;
  EvalPlan pl, sizing;
  rc = eval_plans(ix, by, n_queries, &pl, &sizing);
  if (rc) return rc;
  const int slots = pl.slots, seen_lds = pl.seen_lds;
  a.cat_cap = pl.cat_cap;
  a.slot_bytes = sizing.slot_bytes;  // every plan lays its slots out at the sizing stride (its own arrays sit at the front)
  // (against the slots this call's plan takes: a scorer form may do with less than nann_search_eval_workspace_bytes named)
  if (!workspace || workspace_bytes < (int64_t)slots_bytes(a.slot_bytes, slots, false)) return short_workspace("nann_search_eval");
  index_fields_of(ix, &a);
  a.q = q;
  a.n_queries = (int)n_queries;
  for (int l = 0; l < 3; ++l) { a.num_scoring[l] = num_scoring[l]; a.top_k[l] = top_k[l]; }
  a.topk_eval = topk_eval;
  a.ws = static_cast<unsigned char*>(workspace);
  a.use_dirty = pl.use_dirty;
  a.vis_words = pl.vis_words;
  a.lds_words = pl.lds_words;
  a.win_owners = pl.win_owners;
  a.n_windows = pl.n_windows;
  a.out_ids = out_item_ids; a.out_scores = out_scores; a.out_index = out_index; a.n_out = n_out; a.status = status;
  a.counters = counters;
  a.mlp = MlpParams{};
  a.attn = AttnParams{};
  a.kt = kt; a.upad = upad;
  HIP_TRY(hipMemsetAsync(workspace, 0, 256, st));
  const int dt = ix->desc.emb_dtype, d = ix->desc.d;
  // measurement builds of nann_eval.h (-DNANN_EVAL_TICKS=1, tools/build_res_variant.py): per-phase ticks of the launch on stderr
  static const bool want_ticks = [] { const char* e = std::getenv("NANN_EVAL_TICKS"); return e && e[0] == '1'; }();
  a.ticks = nullptr;
  if (want_ticks && l2) {
    static unsigned long long* g_ticks = nullptr;
    if (!g_ticks) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&g_ticks), 16 * 8));
    HIP_TRY(hipMemsetAsync(g_ticks, 0, 16 * 8, st));
    a.ticks = g_ticks;
    rc = launch_eval_l2(d / 8, dt, seen_lds, slots, a, st);
    unsigned long long h[16];
    HIP_TRY(hipMemcpyAsync(h, g_ticks, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::fprintf(stderr, "EVALTICKS users %lld (100 MHz ticks, sum over users) entry_score %llu entry_topk %llu level_start %llu gather %llu scan %llu score %llu topk %llu select %llu | scan: pass1 %llu wgscan %llu (emit = scan)\n",
                 (long long)n_queries, h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], h[9]);
    return rc;
  }
  if (attn) {
    a.attn = attn->P;
    return launch_eval_attn(d, dt, slots, a, st);
  }
  if (scorer->desc.kind == NANN_SCORER_MLP) {
    a.mlp = scorer->mlp;  // (always the f32 MFMA form: the evaluation job is the accuracy reference)
    if (d == 64) return launch_eval_mlp_d64(dt, slots, a, st);
    if (d == 128) return launch_eval_mlp_d128(dt, slots, a, st);
    if (d == 256) return launch_eval_mlp_d256(dt, slots, a, st);
    return fail(NANN_ERR_UNSUPPORTED, "MLP scorer: d in {64, 128, 256}");
  }
  return launch_eval_l2(d / 8, dt, seen_lds, slots, a, st);
}

// [header | the sizing plan's slots] [a 256-byte gap | a model's staged query]; the gap is counted under a scorer too
static int eval_bytes(const nann_index* ix, const nann_model* m, int64_t n_queries, TraverseBytes* b) {
  EvalPlan sizing;
  const int rc = eval_plan(ix, n_queries, false, &sizing);  // (the most slots, the widest `visited` any scorer's plan takes)
  if (rc) return rc;
  b->search = (int64_t)slots_bytes(sizing.slot_bytes, sizing.slots, false);
  b->query_off = up256_i64(b->search);
  b->inner = b->total = b->search + 256 + (m ? (int64_t)model_query_bytes(m, n_queries) : 0);
  return NANN_OK;
}

// x: q f32[n, d] with a scorer, comm_seq f16[n, seq_len, E] with a model.  `who`: the entry point in a message.
static int evaluate(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, bool model, const void* x, int64_t n_queries,
                    const int32_t num_scoring[3], const int32_t top_k[3], int32_t topk_eval, void* workspace, int64_t workspace_bytes,
                    int64_t* out_item_ids, float* out_scores, int32_t* out_index, int32_t* n_out, int32_t* status, int32_t* counters,
                    nann_stream_t stream, const char* who) {
  if (!ix || !x || !num_scoring || !top_k || !out_item_ids || !n_out || !status || (model ? !m || !workspace : !scorer))
    return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": null argument");
  if (n_queries <= 0) return NANN_OK;
  const ScoredBy by = scored_by(ix, scorer, m);
  if (by.mismatch) return disagree(by);
  hipStream_t st = as_stream(stream);
  // a scorer form looks at the shape of the call before its workspace (eval_impl), and holds the workspace to the plan it runs
  if (!model)
    return eval_impl(ix, by, static_cast<const float*>(x), nullptr, nullptr, n_queries, num_scoring, top_k, topk_eval, workspace,
                     workspace_bytes, out_item_ids, out_scores, out_index, n_out, status, counters, st);
  int rc = eval_model_kind(m, who);
  if (rc) return rc;
  TraverseBytes b;
  rc = eval_bytes(ix, m, n_queries, &b);
  if (rc) return rc;
  if (workspace_bytes < b.total) return short_workspace("nann_search_eval");
  const float *q = nullptr, *kt = nullptr, *upad = nullptr;
  rc = stage_model_query(by, x, n_queries, static_cast<unsigned char*>(workspace) + b.query_off, true, stream, &q, &kt, &upad);
  if (rc) return rc;
  return eval_impl(ix, by, q, kt, upad, n_queries, num_scoring, top_k, topk_eval, workspace, b.search, out_item_ids, out_scores,
                   out_index, n_out, status, nullptr, st);
}

extern "C" {

int nann_search_eval_workspace_bytes(const nann_index* ix, const nann_model* m, int64_t n_queries, int64_t* nbytes) {
  if (!ix || !nbytes) return fail(NANN_ERR_BAD_ARGUMENT, "nann_search_eval_workspace_bytes: null argument");
  TraverseBytes b;
  const int rc = eval_bytes(ix, m, n_queries, &b);
  if (rc) return rc;
  *nbytes = b.total;
  return NANN_OK;
}
int nann_search_eval_plan(const nann_index* ix, const nann_scorer* scorer, const nann_model* m, int64_t n_queries,
                          nann_eval_plan* out) {
  const char* who = "nann_search_eval_plan";
  if (!ix || !out || (!scorer == !m)) return fail(NANN_ERR_BAD_ARGUMENT, std::string(who) + ": an index, a plan and one of scorer / model");
  const ScoredBy by = scored_by(ix, scorer, m);
  if (by.mismatch) return disagree(by);
  int rc = m ? eval_model_kind(m, who) : NANN_OK;
  if (!rc) rc = eval_scored_by(by, n_queries);
  EvalPlan pl, sizing;
  if (!rc) rc = eval_plans(ix, by, std::max<int64_t>(n_queries, 0), &pl, &sizing);
  if (rc) return rc;
  out->struct_bytes = (int32_t)sizeof(nann_eval_plan);
  out->form = pl.seen_lds;
  out->n_windows = pl.n_windows;
  out->slots = pl.slots;
  out->threads = pl.threads;
  out->use_dirty = pl.use_dirty;
  return NANN_OK;
}
int nann_search_eval(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries,
                     const int32_t num_scoring_per_level[3], const int32_t top_k_per_level[3], int32_t topk_eval,
                     void* workspace, int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores,
                     int32_t* out_index, int32_t* n_out, int32_t* status, nann_stream_t stream) {
  return evaluate(ix, scorer, nullptr, false, q, n_queries, num_scoring_per_level, top_k_per_level, topk_eval, workspace,
                  workspace_bytes, out_item_ids, out_scores, out_index, n_out, status, nullptr, stream, "nann_search_eval");
}
int nann_search_eval_ex(const nann_index* ix, const nann_scorer* scorer, const float* q, int64_t n_queries,
                        const int32_t num_scoring_per_level[3], const int32_t top_k_per_level[3], int32_t topk_eval,
                        void* workspace, int64_t workspace_bytes, int64_t* out_item_ids, float* out_scores,
                        int32_t* out_index, int32_t* n_out, int32_t* status, int32_t* counters, nann_stream_t stream) {
  return evaluate(ix, scorer, nullptr, false, q, n_queries, num_scoring_per_level, top_k_per_level, topk_eval, workspace,
                  workspace_bytes, out_item_ids, out_scores, out_index, n_out, status, counters, stream, "nann_search_eval_ex");
}
int nann_search_eval_model(const nann_index* ix, const nann_model* m, const void* comm_seq_f16, int64_t n_queries,
                           const int32_t num_scoring_per_level[3], const int32_t top_k_per_level[3],
                           int32_t topk_eval, void* workspace, int64_t workspace_bytes, int64_t* out_item_ids,
                           float* out_scores, int32_t* out_index, int32_t* n_out, int32_t* status,
                           nann_stream_t stream) {
  return evaluate(ix, nullptr, m, true, comm_seq_f16, n_queries, num_scoring_per_level, top_k_per_level, topk_eval, workspace,
                  workspace_bytes, out_item_ids, out_scores, out_index, n_out, status, nullptr, stream, "nann_search_eval_model");
}

}  // extern "C"
