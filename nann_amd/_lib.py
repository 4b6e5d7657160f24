"""ctypes view of libnann_hip.so (the C ABI in include/nann_hip.h).

There is no fallback: if the HIP extension is missing this module raises, and
every op in nann_amd goes through it.
"""
import ctypes as C
import os

from . import build as _build

_LIB = None

OK = 0
STATUS_NAMES = {
    0: "OK", 1: "INVALID_RAGGED_PARAMS", 2: "INVALID_RAGGED_INDICES", 3: "INVALID_RAGGED_INPUT",
    4: "TOPK_K_GT_N", 5: "INDEX_OUT_OF_RANGE", 6: "EMPTY_SCORE_BATCH", 7: "BAD_ARGUMENT",
    8: "TOPK_SCALAR_INPUT", 100: "HIP", 101: "NO_DEVICE", 102: "UNSUPPORTED", 103: "CAPACITY",
    104: "IO", 105: "DTYPE_MISMATCH", 106: "SHAPE_MISMATCH",
}
F16, BF16, F32, I32, I64, F64 = 0, 1, 2, 3, 4, 5
SCORER_L2, SCORER_MLP, SCORER_IP = 0, 1, 2
MLP_DEFAULT, MLP_SPLIT_F16, MLP_EXACT_F32, MLP_CERTIFIED = 0, 1, 2, 3
NUM_ROUNDS = 5
NUM_PHASES = 19
UNION_MAX_IN = 8192  # NANN_UNION_MAX_IN: most entries (n_lists * k_in) a user brings to nann_union_topk
FUSE_MAX_LISTS = 64  # NANN_FUSE_MAX_LISTS: most lists a user brings to nann_fuse_topk (out_lists is one u64 per entry)
WIDE_MAX_K = 16384   # NANN_WIDE_MAX_K: largest k of nann_search_all_wide, nann_search_all_model_wide and nann_select_wide
FUSE_SUM, FUSE_SUM_FLOOR, FUSE_MINMAX, FUSE_RRF = 0, 1, 2, 3
INTERESTS_MAX_VEC = 16   # NANN_INTERESTS_MAX_VEC: most interest vectors nann_user_seq_interests makes of a sequence
INTERESTS_MAX_ITER = 32  # NANN_INTERESTS_MAX_ITER: most Lloyd rounds it runs
PHASE_NAMES = ("zero", "walk", "expand", "score", "topk", "other", "tk_load", "tk_search",
               "tk_collect", "tk_sort", "ex_pass1", "ex_loop", "ex_walkbusy",
               "ex_lookup", "ex_load", "ex_insert", "ex_bar_a", "ex_check", "ex_rank")

# every symbol include/nann_hip.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "nann_abi_version", "nann_last_error", "nann_device_count", "nann_malloc", "nann_free",
    "nann_memcpy", "nann_stream_synchronize", "nann_stream_create", "nann_stream_destroy", "nann_host_malloc",
    "nann_host_free", "nann_huge_const_load", "nann_group_gather_count",
    "nann_group_gather_fill", "nann_group_gather_unique_scratch_bytes", "nann_group_gather_unique", "nann_bitmap_ref_difference", "nann_bloom_filter_difference", "nann_gather_rows", "nann_topk",
    "nann_scorer_create", "nann_scorer_destroy", "nann_user_seq_mean", "nann_user_seq_interests", "nann_score",
    "nann_index_create", "nann_index_destroy", "nann_index_info", "nann_index_probe_info", "nann_search_workspace_bytes",
    "nann_search", "nann_search_v", "nann_search_ex", "nann_search_opt", "nann_search_options_init", "nann_search_reruns", "nann_search_refined", "nann_search_model_opt", "nann_set_traversal_mode", "nann_set_search_reserve", "nann_search_model_workspace_bytes",
    "nann_search_model", "nann_search_model_v",
    "nann_scorer_prepare", "nann_scorer_release", "nann_scorer_table_bytes", "nann_set_preprojection",
    "nann_model_prepare", "nann_model_release", "nann_model_table_bytes", "nann_search_eval_workspace_bytes", "nann_search_eval_plan", "nann_search_eval", "nann_search_eval_ex", "nann_search_eval_model",
    "nann_search_all_workspace_bytes", "nann_search_all", "nann_search_all_model_workspace_bytes", "nann_search_all_model",
    "nann_search_all_filtered_workspace_bytes", "nann_search_all_filtered", "nann_search_all_model_filtered_workspace_bytes",
    "nann_search_all_model_filtered", "nann_search_filtered_workspace_bytes", "nann_search_filtered",
    "nann_search_model_filtered_workspace_bytes", "nann_search_model_filtered",
    "nann_search_all_range_workspace_bytes", "nann_search_all_range",
    "nann_search_all_range_model_workspace_bytes", "nann_search_all_range_model",
    "nann_search_candidates_workspace_bytes", "nann_search_candidates",
    "nann_search_candidates_model_workspace_bytes", "nann_search_candidates_model",
    "nann_union_topk_workspace_bytes", "nann_union_topk", "nann_search_multi_workspace_bytes", "nann_search_multi",
    "nann_search_all_multi_workspace_bytes", "nann_search_all_multi",
    "nann_fuse_topk_workspace_bytes", "nann_fuse_topk", "nann_search_multi_fused_workspace_bytes", "nann_search_multi_fused",
    "nann_search_all_multi_fused_workspace_bytes", "nann_search_all_multi_fused",
    "nann_group_cap_topk", "nann_search_grouped_workspace_bytes", "nann_search_grouped",
    "nann_search_model_grouped_workspace_bytes", "nann_search_model_grouped",
    "nann_search_all_grouped_workspace_bytes", "nann_search_all_grouped",
    "nann_search_all_model_grouped_workspace_bytes", "nann_search_all_model_grouped",
    "nann_mmr_topk", "nann_search_diverse_workspace_bytes", "nann_search_diverse",
    "nann_search_model_diverse_workspace_bytes", "nann_search_model_diverse",
    "nann_search_all_diverse_workspace_bytes", "nann_search_all_diverse",
    "nann_search_all_model_diverse_workspace_bytes", "nann_search_all_model_diverse",
    "nann_predicate_topk", "nann_predicate_count", "nann_search_where_workspace_bytes", "nann_search_where",
    "nann_search_model_where_workspace_bytes", "nann_search_model_where",
    "nann_search_all_where_workspace_bytes", "nann_search_all_where",
    "nann_search_all_model_where_workspace_bytes", "nann_search_all_model_where",
    "nann_merge_topk", "nann_merge_topk_host",
    "nann_attn_scorer_create", "nann_attn_scorer_destroy", "nann_attn_prepare", "nann_attn_score",
    "nann_blaze_options_parse", "nann_model_load", "nann_model_destroy", "nann_model_kind", "nann_model_scorer", "nann_model_workspace_bytes", "nann_model_forward",
    "nann_comm_get_unique_id", "nann_comm_create", "nann_comm_destroy", "nann_comm_ranks", "nann_comm_set_timing", "nann_comm_last_breakdown", "nann_comm_wait", "nann_comm_abort", "nann_sharded_topk_workspace_bytes",
    "nann_sharded_topk", "nann_merge_records", "nann_hnsw_draw_levels", "nann_hnsw_build_device", "nann_hnsw_build_device_ex",
    "nann_hnsw_append_device", "nann_hnsw_export_count", "nann_hnsw_export_fill",
    "nann_hnsw_build_device_metric", "nann_hnsw_append_device_metric",
    "nann_hnsw_remove_count", "nann_hnsw_remove_device",
    "nann_hnsw_update_device", "nann_hnsw_orphan_bits",
    "nann_sq8_create", "nann_sq8_destroy", "nann_sq8_info", "nann_sq8_view", "nann_sq8_encode",
    "nann_search_all_sq8_workspace_bytes", "nann_search_all_sq8",
    "nann_sq8_bounds_create", "nann_sq8_bounds_destroy", "nann_sq8_bounds_view",
    "nann_search_all_sq8_exact_workspace_bytes", "nann_search_all_sq8_exact_layout", "nann_search_all_sq8_exact",
    "nann_search_all_range_sq8_exact_workspace_bytes", "nann_search_all_range_sq8_exact",
    "nann_search_all_wide_workspace_bytes", "nann_search_all_wide",
    "nann_search_all_model_wide_workspace_bytes", "nann_search_all_model_wide",
    "nann_select_wide_workspace_bytes", "nann_select_wide",
]


class SearchOptions(C.Structure):
    """nann_search_options (include/nann_hip.h): -1 = the process default of the field"""
    _fields_ = [("struct_bytes", C.c_int32), ("traversal_mode", C.c_int32), ("slot_reserve", C.c_int32),
                ("preprojection", C.c_int32), ("mlp_form", C.c_int32)]


class Fusion(C.Structure):
    """nann_fusion: how nann_fuse_topk and the _fused searches turn a row's entries in several lists into one score"""
    _fields_ = [("struct_bytes", C.c_int32), ("mode", C.c_int32), ("rrf_c", C.c_float), ("weights_per_user", C.c_int32),
                ("weights", C.c_void_p)]


class SearchPlan(C.Structure):
    """nann_search_plan: what the planner chose for a call"""
    _fields_ = [("visited_set", C.c_int32), ("fallback_visited_set", C.c_int32), ("threads", C.c_int32),
                ("workgroups", C.c_int32), ("phased", C.c_int32), ("table", C.c_int32),
                ("est_visited", C.c_float), ("worst_visited", C.c_float), ("lean", C.c_int32)]


class EvalPlan(C.Structure):
    """nann_eval_plan: the form of the evaluation traversal a call runs (nann_search_eval_plan)"""
    _fields_ = [("struct_bytes", C.c_int32), ("form", C.c_int32), ("n_windows", C.c_int32), ("slots", C.c_int32),
                ("threads", C.c_int32), ("use_dirty", C.c_int32)]


class Filter(C.Structure):
    """nann_filter: a deny bitmap for every query and an exclusion list per query (device pointers, borrowed per call)"""
    _fields_ = [("struct_bytes", C.c_int32), ("deny_bits", C.c_void_p), ("excl_row_splits", C.c_void_p),
                ("excl_rows", C.c_void_p), ("n_excl", C.c_int64)]


class Groups(C.Structure):
    """nann_groups: the group of every row and the cap -- one for the call, or one per query (device pointers, borrowed per call)"""
    _fields_ = [("struct_bytes", C.c_int32), ("group_of_row", C.c_void_p), ("cap", C.c_int32), ("caps", C.c_void_p)]


class Predicates(C.Structure):
    """nann_predicates: the attribute columns of the rows and the per-query label / range / tag conditions (device pointers,
    borrowed per call)"""
    _fields_ = [("struct_bytes", C.c_int32), ("label_of_row", C.c_void_p), ("value_of_row", C.c_void_p),
                ("tags_of_row", C.c_void_p), ("label_splits", C.c_void_p), ("labels", C.c_void_p), ("n_labels", C.c_int64),
                ("value_lo", C.c_void_p), ("value_hi", C.c_void_p), ("tags_all", C.c_void_p), ("tags_any", C.c_void_p),
                ("tags_none", C.c_void_p)]


class Diversity(C.Structure):
    """nann_diversity: lambda -- one for the call, or one per query (a device pointer, borrowed per call) -- and the similarity"""
    _fields_ = [("struct_bytes", C.c_int32), ("lam", C.c_float), ("lambdas", C.c_void_p), ("sim", C.c_int32)]


class Candidates(C.Structure):
    """nann_candidates: a list of rows per query (device pointers, borrowed per call)"""
    _fields_ = [("struct_bytes", C.c_int32), ("row_splits", C.c_void_p), ("rows", C.c_void_p), ("n_cand", C.c_int64)]


class ScorerDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("d", C.c_int32), ("emb_dtype", C.c_int32),
                ("h1", C.c_int32), ("h2", C.c_int32),
                ("w1", C.c_void_p), ("b1", C.c_void_p), ("alpha1", C.c_void_p),
                ("w2", C.c_void_p), ("b2", C.c_void_p), ("alpha2", C.c_void_p),
                ("w3", C.c_void_p), ("precision", C.c_int32)]


class AttnDesc(C.Structure):
    _fields_ = ([("d", C.c_int32), ("emb_dtype", C.c_int32), ("seq_len", C.c_int32)] +
                [(n, C.c_void_p) for n in ("wq1", "bq1", "aq", "wq2", "bq2", "wk1", "bk1", "ak", "wk2", "bk2")] +
                [("w", C.c_void_p * 4), ("b", C.c_void_p * 3), ("bn_scale", C.c_void_p * 3),
                 ("bn_shift", C.c_void_p * 3), ("alpha", C.c_void_p * 3), ("precision", C.c_int32)])


class IndexDesc(C.Structure):
    _fields_ = [("n_items", C.c_int64), ("d", C.c_int32), ("emb_dtype", C.c_int32),
                ("item_embs", C.c_void_p), ("item_ids", C.c_void_p),
                ("nb_values", C.c_void_p * 2), ("nb_row_splits", C.c_void_p * 2),
                ("nb_nnz", C.c_int64 * 2),
                ("enter_points", C.c_void_p), ("n_enter", C.c_int64),
                ("on_device", C.c_int32)]


def lib_path():
    # NANN_HIP_LIB: load another build of the same ABI (kernel-variant experiments, tools/)
    return os.environ.get("NANN_HIP_LIB") or _build.LIB


def lib():
    """Load (building first if the sources are newer) the HIP extension."""
    global _LIB
    if _LIB is None:
        path = lib_path()
        # the default library is rebuilt when its sources changed since it was linked (content
        # hash, nann_amd/build.py); a library named by NANN_HIP_LIB is loaded as it is
        if not os.path.exists(path) or (not os.environ.get("NANN_HIP_LIB") and _build.is_stale()):
            try:
                _build.build()
            except Exception as e:  # no hipcc and no prebuilt library: fail loudly
                raise ImportError(
                    f"nann_amd: HIP extension {path} is missing and could not be built ({e}); "
                    "there is no CPU fallback") from e
        L = C.CDLL(path)
        L.nann_last_error.restype = C.c_char_p
        for name in SYMBOLS:
            getattr(L, name)  # AttributeError if the ABI is incomplete
        L.nann_scorer_destroy.restype = None
        L.nann_attn_scorer_destroy.restype = None
        L.nann_index_destroy.restype = None
        L.nann_comm_destroy.restype = None
        L.nann_model_destroy.restype = None
        L.nann_model_scorer.restype = C.c_void_p  # a borrowed handle (the default restype would cut it to 32 bits)
        # (ix, scorer, n_queries, k, *nbytes) / (ix, scorer, q, n_queries, k, out_item_ids, out_scores, out_index, workspace,
        #  workspace_bytes, options, stream)
        L.nann_search_all_workspace_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]
        L.nann_search_all_workspace_bytes.restype = C.c_int
        L.nann_search_all.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(SearchOptions), C.c_void_p]
        L.nann_search_all.restype = C.c_int
        # (ix, model, n_users, k, *nbytes) / (ix, model, comm_seq_f16, n_users, k, out_item_ids, out_scores, out_index, workspace,
        #  workspace_bytes, options, stream)
        L.nann_search_all_model_workspace_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]
        L.nann_search_all_model_workspace_bytes.restype = C.c_int
        L.nann_search_all_model.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(SearchOptions), C.c_void_p]
        L.nann_search_all_model.restype = C.c_int
        # the filtered twins: the same lists, then (filter, n_out, stream) in the place of (stream)
        for name, twin in (("nann_search_all_filtered", L.nann_search_all), ("nann_search_all_model_filtered", L.nann_search_all_model)):
            fn = getattr(L, name)
            fn.argtypes = twin.argtypes[:-1] + [C.POINTER(Filter), C.c_void_p, C.c_void_p]
            fn.restype = C.c_int
            wb = getattr(L, name + "_workspace_bytes")
            wb.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]
            wb.restype = C.c_int
        # the range forms: (ix, scorer | model, n, *nbytes) / (ix, scorer | model, q | comm_seq_f16, n, thresholds, capacity,
        #  out_row_splits, out_item_ids, out_scores, out_index, workspace, workspace_bytes, options, filter, stream)
        for name in ("nann_search_all_range", "nann_search_all_range_model"):
            fn = getattr(L, name)
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 5 + \
                          [C.c_int64, C.POINTER(SearchOptions), C.POINTER(Filter), C.c_void_p]
            fn.restype = C.c_int
            wb = getattr(L, name + "_workspace_bytes")
            wb.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
            wb.restype = C.c_int
        # (ix, scorer | model, q, n_queries, level_topn_max, level_topn, workspace, workspace_bytes, out_item_ids, out_scores,
        #  out_index, status, counters, [phase_ticks,] options, plan, filter, k, n_out, stream)
        head = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_int64,
                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        tail = [C.POINTER(SearchOptions), C.POINTER(SearchPlan), C.POINTER(Filter), C.c_int32, C.c_void_p, C.c_void_p]
        L.nann_search_filtered.argtypes = head + [C.c_void_p] + tail
        L.nann_search_filtered.restype = C.c_int
        L.nann_search_model_filtered.argtypes = head + tail
        L.nann_search_model_filtered.restype = C.c_int
        L.nann_search_filtered_workspace_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int64)]
        L.nann_search_filtered_workspace_bytes.restype = C.c_int
        L.nann_search_model_filtered_workspace_bytes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int64,
                                                                 C.POINTER(C.c_int64)]
        L.nann_search_model_filtered_workspace_bytes.restype = C.c_int
        # the grouped forms: (scores, rows, n_valid, n_queries, k_in, n_items, item_ids, groups, filter, k, out_index, out_scores,
        #  out_item_ids, out_group, out_pos, n_out, stream)
        L.nann_group_cap_topk.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.POINTER(Groups),
                                                             C.POINTER(Filter), C.c_int32] + [C.c_void_p] * 7
        L.nann_group_cap_topk.restype = C.c_int
        # the filtered traversal's list with (filter, groups, k, out_group, n_out, stream) in the place of (filter, k, n_out, stream)
        gtail = [C.POINTER(SearchOptions), C.POINTER(SearchPlan), C.POINTER(Filter), C.POINTER(Groups), C.c_int32, C.c_void_p,
                 C.c_void_p, C.c_void_p]
        L.nann_search_grouped.argtypes = head + [C.c_void_p] + gtail
        L.nann_search_grouped.restype = C.c_int
        L.nann_search_model_grouped.argtypes = head + gtail
        L.nann_search_model_grouped.restype = C.c_int
        L.nann_search_grouped_workspace_bytes.argtypes = list(L.nann_search_filtered_workspace_bytes.argtypes)
        L.nann_search_grouped_workspace_bytes.restype = C.c_int
        L.nann_search_model_grouped_workspace_bytes.argtypes = list(L.nann_search_model_filtered_workspace_bytes.argtypes)
        L.nann_search_model_grouped_workspace_bytes.restype = C.c_int
        # (ix, scorer | model, n, fetch, *nbytes) / (ix, scorer | model, q | comm_seq_f16, n, fetch, k, out_item_ids, out_scores,
        #  out_index, out_group, workspace, workspace_bytes, options, filter, groups, n_out, stream)
        for name in ("nann_search_all_grouped", "nann_search_all_model_grouped"):
            fn = getattr(L, name)
            fn.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 5 + \
                          [C.c_int64, C.POINTER(SearchOptions), C.POINTER(Filter), C.POINTER(Groups), C.c_void_p, C.c_void_p]
            fn.restype = C.c_int
            wb = getattr(L, name + "_workspace_bytes")
            wb.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]
            wb.restype = C.c_int
        # the diverse forms: (ix, scores, rows, n_valid, n_queries, k_in, diversity, k, out_index, out_scores, out_mmr, out_pos,
        #  out_item_ids, n_out, stream)
        L.nann_mmr_topk.argtypes = [C.c_void_p] * 4 + [C.c_int64, C.c_int32, C.POINTER(Diversity), C.c_int32] + [C.c_void_p] * 7
        L.nann_mmr_topk.restype = C.c_int
        # the filtered traversal's list with (filter, diversity, k, out_mmr, out_pos, n_out, stream) in the place of its tail
        dtail = [C.POINTER(SearchOptions), C.POINTER(SearchPlan), C.POINTER(Filter), C.POINTER(Diversity), C.c_int32, C.c_void_p,
                 C.c_void_p, C.c_void_p, C.c_void_p]
        L.nann_search_diverse.argtypes = head + [C.c_void_p] + dtail
        L.nann_search_diverse.restype = C.c_int
        L.nann_search_model_diverse.argtypes = head + dtail
        L.nann_search_model_diverse.restype = C.c_int
        L.nann_search_diverse_workspace_bytes.argtypes = list(L.nann_search_filtered_workspace_bytes.argtypes)
        L.nann_search_diverse_workspace_bytes.restype = C.c_int
        L.nann_search_model_diverse_workspace_bytes.argtypes = list(L.nann_search_model_filtered_workspace_bytes.argtypes)
        L.nann_search_model_diverse_workspace_bytes.restype = C.c_int
        # (ix, scorer | model, n, fetch, *nbytes) / (ix, scorer | model, q | comm_seq_f16, n, fetch, k, out_item_ids, out_scores,
        #  out_index, out_mmr, out_pos, workspace, workspace_bytes, options, filter, diversity, n_out, stream)
        for name in ("nann_search_all_diverse", "nann_search_all_model_diverse"):
            fn = getattr(L, name)
            fn.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 6 + \
                          [C.c_int64, C.POINTER(SearchOptions), C.POINTER(Filter), C.POINTER(Diversity), C.c_void_p, C.c_void_p]
            fn.restype = C.c_int
            wb = getattr(L, name + "_workspace_bytes")
            wb.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]
            wb.restype = C.c_int
        # the predicate forms: (scores, rows, n_valid, n_queries, k_in, n_items, item_ids, predicates, filter, k, out_index,
        #  out_scores, out_item_ids, out_pos, n_out, stream) / (n_items, predicates, filter, n_queries, out_counts, stream)
        L.nann_predicate_topk.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.POINTER(Predicates),
                                                             C.POINTER(Filter), C.c_int32] + [C.c_void_p] * 6
        L.nann_predicate_topk.restype = C.c_int
        L.nann_predicate_count.argtypes = [C.c_int64, C.POINTER(Predicates), C.POINTER(Filter), C.c_int64, C.c_void_p, C.c_void_p]
        L.nann_predicate_count.restype = C.c_int
        # the filtered traversal's list with (filter, predicates, k, n_out, stream) in the place of (filter, k, n_out, stream)
        wtail = [C.POINTER(SearchOptions), C.POINTER(SearchPlan), C.POINTER(Filter), C.POINTER(Predicates), C.c_int32, C.c_void_p,
                 C.c_void_p]
        L.nann_search_where.argtypes = head + [C.c_void_p] + wtail
        L.nann_search_where.restype = C.c_int
        L.nann_search_model_where.argtypes = head + wtail
        L.nann_search_model_where.restype = C.c_int
        L.nann_search_where_workspace_bytes.argtypes = list(L.nann_search_filtered_workspace_bytes.argtypes)
        L.nann_search_where_workspace_bytes.restype = C.c_int
        L.nann_search_model_where_workspace_bytes.argtypes = list(L.nann_search_model_filtered_workspace_bytes.argtypes)
        L.nann_search_model_where_workspace_bytes.restype = C.c_int
        # the filtered exhaustive search's list with (filter, predicates, n_out, stream) in the place of (filter, n_out, stream)
        for name, twin in (("nann_search_all_where", L.nann_search_all), ("nann_search_all_model_where", L.nann_search_all_model)):
            fn = getattr(L, name)
            fn.argtypes = twin.argtypes[:-1] + [C.POINTER(Filter), C.POINTER(Predicates), C.c_void_p, C.c_void_p]
            fn.restype = C.c_int
            wb = getattr(L, name + "_workspace_bytes")
            wb.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]
            wb.restype = C.c_int
        # the wide forms: (ix, scorer | model, n, k, *nbytes) / (ix, scorer | model, q | comm_seq_f16, n, k, out_item_ids, out_scores,
        #  out_index, n_out, workspace, workspace_bytes, options, filter, predicates, stream)
        for name in ("nann_search_all_wide", "nann_search_all_model_wide"):
            fn = getattr(L, name)
            fn.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.c_int32] + [C.c_void_p] * 5 + \
                          [C.c_int64, C.POINTER(SearchOptions), C.POINTER(Filter), C.POINTER(Predicates), C.c_void_p]
            fn.restype = C.c_int
            wb = getattr(L, name + "_workspace_bytes")
            wb.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]
            wb.restype = C.c_int
        # (n_rows, n_cols, k, *nbytes) / (values, n_rows, n_cols, k, out_values, out_indices, n_out, workspace, workspace_bytes, stream)
        L.nann_select_wide_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]
        L.nann_select_wide_workspace_bytes.restype = C.c_int
        L.nann_select_wide.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p]
        L.nann_select_wide.restype = C.c_int
        # (ix, scorer, n_queries, n_cand, k, *nbytes) / (ix, scorer, q, n_queries, k, cand, out_item_ids, out_scores, out_index,
        #  out_pos, n_out, status, workspace, workspace_bytes, options, stream)
        L.nann_search_candidates_workspace_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32,
                                                             C.POINTER(C.c_int64)]
        L.nann_search_candidates_workspace_bytes.restype = C.c_int
        L.nann_search_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(Candidates)] + \
                                            [C.c_void_p] * 7 + [C.c_int64, C.POINTER(SearchOptions), C.c_void_p]
        L.nann_search_candidates.restype = C.c_int
        # the model form: (ix, model, comm_seq_f16, ...) in the place of (ix, scorer, q, ...)
        L.nann_search_candidates_model_workspace_bytes.argtypes = list(L.nann_search_candidates_workspace_bytes.argtypes)
        L.nann_search_candidates_model_workspace_bytes.restype = C.c_int
        L.nann_search_candidates_model.argtypes = list(L.nann_search_candidates.argtypes)
        L.nann_search_candidates_model.restype = C.c_int
        # (comm_seq_f16, n_users, seq_len, d, n_vec, n_iter, q, weights, n_interests, assign, stream)
        L.nann_user_seq_interests.argtypes = [C.c_void_p, C.c_int64] + [C.c_int32] * 4 + [C.c_void_p] * 5
        L.nann_user_seq_interests.restype = C.c_int
        # (n_users, n_lists, k_in, *nbytes) / (scores, rows, n_valid, n_users, n_lists, k_in, n_items, item_ids, k, out_index,
        #  out_scores, out_item_ids, out_list, n_out, workspace, workspace_bytes, stream)
        L.nann_union_topk_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
        L.nann_union_topk_workspace_bytes.restype = C.c_int
        L.nann_union_topk.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_int32] + \
                                     [C.c_void_p] * 6 + [C.c_int64, C.c_void_p]
        L.nann_union_topk.restype = C.c_int
        # (ix, level_topn, n_users, n_vec, *nbytes) / (ix, scorer, q, n_users, n_vec, level_topn_max, level_topn, workspace,
        #  workspace_bytes, out_item_ids, out_scores, out_index, out_vec, n_out, status, counters, options, plan, k, stream)
        L.nann_search_multi_workspace_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int64, C.c_int32, C.POINTER(C.c_int64)]
        L.nann_search_multi_workspace_bytes.restype = C.c_int
        L.nann_search_multi.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p,
                                                           C.c_int64] + [C.c_void_p] * 7 + \
                                       [C.POINTER(SearchOptions), C.POINTER(SearchPlan), C.c_int32, C.c_void_p]
        L.nann_search_multi.restype = C.c_int
        # (ix, scorer, n_users, n_vec, k, *nbytes) / (ix, scorer, q, n_users, n_vec, k, out_item_ids, out_scores, out_index,
        #  out_vec, n_out, workspace, workspace_bytes, options, stream)
        L.nann_search_all_multi_workspace_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                                            C.POINTER(C.c_int64)]
        L.nann_search_all_multi_workspace_bytes.restype = C.c_int
        L.nann_search_all_multi.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 6 + \
                                           [C.c_int64, C.POINTER(SearchOptions), C.c_void_p]
        L.nann_search_all_multi.restype = C.c_int
        # the union's arguments with (fusion) behind k and out_lists u64 in the place of out_list
        L.nann_fuse_topk_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
        L.nann_fuse_topk_workspace_bytes.restype = C.c_int
        L.nann_fuse_topk.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_int32,
                                                        C.POINTER(Fusion)] + [C.c_void_p] * 6 + [C.c_int64, C.c_void_p]
        L.nann_fuse_topk.restype = C.c_int
        # nann_search_multi's with out_lists in the place of out_vec and (fusion) behind k
        L.nann_search_multi_fused_workspace_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int64, C.c_int32,
                                                              C.POINTER(C.c_int64)]
        L.nann_search_multi_fused_workspace_bytes.restype = C.c_int
        L.nann_search_multi_fused.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p,
                                                                 C.c_int64] + [C.c_void_p] * 7 + \
                                             [C.POINTER(SearchOptions), C.POINTER(SearchPlan), C.c_int32, C.POINTER(Fusion), C.c_void_p]
        L.nann_search_multi_fused.restype = C.c_int
        # (ix, scorer, n_users, n_vec, fetch, *nbytes) / (ix, scorer, q, n_users, n_vec, fetch, k, fusion, out_item_ids,
        #  out_scores, out_index, out_lists, n_out, workspace, workspace_bytes, options, stream)
        L.nann_search_all_multi_fused_workspace_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                                                  C.POINTER(C.c_int64)]
        L.nann_search_all_multi_fused_workspace_bytes.restype = C.c_int
        L.nann_search_all_multi_fused.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Fusion)] + \
                                                 [C.c_void_p] * 6 + [C.c_int64, C.POINTER(SearchOptions), C.c_void_p]
        L.nann_search_all_multi_fused.restype = C.c_int
        # the int8 code table: (ix, stream, *out) / (t) / (t, out[4]) / (t, *codes, *scales, *norms) / (x, n, d, codes, scales,
        # norms, stream); the search over it: (ix, t, scorer, n_queries, fetch, k, *nbytes) / (ix, t, scorer, q, n_queries, fetch,
        # k, out_item_ids, out_scores, out_index, out_fetch_index, out_fetch_scores, workspace, workspace_bytes, options, stream)
        L.nann_sq8_create.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.nann_sq8_create.restype = C.c_int
        L.nann_sq8_destroy.argtypes = [C.c_void_p]
        L.nann_sq8_destroy.restype = None
        L.nann_sq8_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.nann_sq8_info.restype = C.c_int
        L.nann_sq8_view.argtypes = [C.c_void_p] + [C.POINTER(C.c_void_p)] * 3
        L.nann_sq8_view.restype = C.c_int
        L.nann_sq8_encode.argtypes = [C.c_void_p, C.c_int64, C.c_int32] + [C.c_void_p] * 4
        L.nann_sq8_encode.restype = C.c_int
        L.nann_search_all_sq8_workspace_bytes.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
        L.nann_search_all_sq8_workspace_bytes.restype = C.c_int
        L.nann_search_all_sq8.argtypes = [C.c_void_p] * 4 + [C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 6 + \
                                         [C.c_int64, C.POINTER(SearchOptions), C.c_void_p]
        L.nann_search_all_sq8.restype = C.c_int
        # the certified form: (ix, t, stream, *out) / (b) / (b, *err, *xhat); (ix, t, b, scorer, n_queries, fetch, cap, k, *nbytes or
        # out[8]) / (ix, t, b, scorer, q, n_queries, fetch, cap, k, out_item_ids, out_scores, out_index, out_certified,
        # out_n_survivors, workspace, workspace_bytes, options, stream)
        L.nann_sq8_bounds_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.nann_sq8_bounds_create.restype = C.c_int
        L.nann_sq8_bounds_destroy.argtypes = [C.c_void_p]
        L.nann_sq8_bounds_destroy.restype = None
        L.nann_sq8_bounds_view.argtypes = [C.c_void_p] + [C.POINTER(C.c_void_p)] * 2
        L.nann_sq8_bounds_view.restype = C.c_int
        head = [C.c_void_p] * 4 + [C.c_int64, C.c_int32, C.c_int64, C.c_int32]
        L.nann_search_all_sq8_exact_workspace_bytes.argtypes = head + [C.POINTER(C.c_int64)]
        L.nann_search_all_sq8_exact_workspace_bytes.restype = C.c_int
        L.nann_search_all_sq8_exact_layout.argtypes = head + [C.POINTER(C.c_int64)]
        L.nann_search_all_sq8_exact_layout.restype = C.c_int
        L.nann_search_all_sq8_exact.argtypes = [C.c_void_p] * 5 + [C.c_int64, C.c_int32, C.c_int64, C.c_int32] + [C.c_void_p] * 6 + \
                                               [C.c_int64, C.POINTER(SearchOptions), C.c_void_p]
        L.nann_search_all_sq8_exact.restype = C.c_int
        # the range form: (ix, t, b, scorer, n, cap, *nbytes) / (ix, t, b, scorer, q, n, thresholds, cap, capacity, out_row_splits,
        #  out_item_ids, out_scores, out_index, out_certified, out_n_survivors, workspace, workspace_bytes, options, stream)
        L.nann_search_all_range_sq8_exact_workspace_bytes.argtypes = [C.c_void_p] * 4 + [C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
        L.nann_search_all_range_sq8_exact_workspace_bytes.restype = C.c_int
        L.nann_search_all_range_sq8_exact.argtypes = [C.c_void_p] * 5 + [C.c_int64, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 7 + \
                                                     [C.c_int64, C.POINTER(SearchOptions), C.c_void_p]
        L.nann_search_all_range_sq8_exact.restype = C.c_int
        # (ix, scorer or NULL, model or NULL, n_queries, *plan)
        L.nann_search_eval_plan.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.POINTER(EvalPlan)]
        L.nann_search_eval_plan.restype = C.c_int
        # (item_embs, n_old, n_new, d, emb_dtype, M, ef_construction, keep_pruned, levels, adj0, up_row, adj_up, stream)
        L.nann_hnsw_append_device.argtypes = [C.c_void_p, C.c_int64, C.c_int64] + [C.c_int32] * 5 + [C.c_void_p] * 5
        L.nann_hnsw_append_device.restype = C.c_int
        # the metric forms: (..., keep_pruned, metric, levels, ...)
        L.nann_hnsw_build_device_metric.argtypes = [C.c_void_p, C.c_int64] + [C.c_int32] * 6 + [C.c_void_p] * 5
        L.nann_hnsw_build_device_metric.restype = C.c_int
        L.nann_hnsw_append_device_metric.argtypes = [C.c_void_p, C.c_int64, C.c_int64] + [C.c_int32] * 6 + [C.c_void_p] * 5
        L.nann_hnsw_append_device_metric.restype = C.c_int
        # (adj0, up_row, adj_up, levels, n, M, start_level, row_splits0, row_splits1, ...): count (nnz, n_enter, stream),
        # fill (nnz, values0, values1, enter_points, stream)
        head = [C.c_void_p] * 4 + [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.nann_hnsw_export_count.argtypes = head + [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p]
        L.nann_hnsw_export_count.restype = C.c_int
        L.nann_hnsw_export_fill.argtypes = head + [C.POINTER(C.c_int64)] + [C.c_void_p] * 4
        L.nann_hnsw_export_fill.restype = C.c_int
        # (remove_bits, levels, n, kept_rows, new_levels, *n_keep, *n_up_rows, stream)
        L.nann_hnsw_remove_count.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64),
                                             C.POINTER(C.c_int64), C.c_void_p]
        L.nann_hnsw_remove_count.restype = C.c_int
        # (item_embs, n, d, emb_dtype, M, keep_pruned, metric, levels, adj0, up_row, adj_up, remove_bits, n_keep, out_adj0,
        #  out_up_row, out_adj_up, stats, stream)
        L.nann_hnsw_remove_device.argtypes = [C.c_void_p, C.c_int64] + [C.c_int32] * 5 + [C.c_void_p] * 5 + [C.c_int64] + \
                                              [C.c_void_p] * 3 + [C.POINTER(C.c_int64), C.c_void_p]
        L.nann_hnsw_remove_device.restype = C.c_int
        # (item_embs, n, d, emb_dtype, M, ef_construction, keep_pruned, metric, levels, adj0, up_row, adj_up, update_bits, out_adj0,
        #  out_up_row, out_adj_up, stats, stream)
        L.nann_hnsw_update_device.argtypes = [C.c_void_p, C.c_int64] + [C.c_int32] * 6 + [C.c_void_p] * 8 + [C.POINTER(C.c_int64), C.c_void_p]
        L.nann_hnsw_update_device.restype = C.c_int
        # (adj0, n, M, out_bits, *n_orphans, stream)
        L.nann_hnsw_orphan_bits.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]
        L.nann_hnsw_orphan_bits.restype = C.c_int
        _LIB = L
    return _LIB


def last_error():
    return lib().nann_last_error().decode("utf-8", "replace")
