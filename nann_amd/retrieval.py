"""The traversal schedule of the reference's serving graph on the MI355X.

`build_model()` in NANN_impls/nann/delivery/build_opt_graph.py:69-149 chains
GroupGather / BitmapRefDifference / GatherV2 / BlazeXlaOp / TopKV2 ~40 times
per request.  Two equivalent executions of that schedule live here:

  * `search()`        one fused launch for a whole batch of queries
                      (nann_search in include/nann_hip.h) -- the product path;
  * `search_all()`    its referee: every item scored for a batch of queries, top k
                      per query (nann_search_all; main.py:194-237 `test_all`);
  * `search_all_model()` the same under any ops.Model, the reference's attention +
                      DNN model included, from `comm_seq` (nann_search_all_model);
  * `make_filter()`   a deny bitmap for every query and an exclusion list per query; search(), search_model(),
                      and search_all() take it as `filter=`, search_all_model_filtered() as an argument
                      (the nann_*_filtered calls: the reference has no such feature);
  * `search_all_range()` / `search_all_range_model()` every row scoring at or above a per-query cut instead of the best k,
                      ragged outputs (nann_search_all_range[_model]: the reference has no such call);
  * `search_all_wide()` / `search_all_model_wide()` the exact top k for k up to 16 384 rows per query, where search_all stops at
                      1 024; filter= and predicates= are optional (nann_search_all_wide, nann_search_all_model_wide);
  * `search_candidates()` / `search_candidates_model()` the exact top k of every query's own list of rows, under a
                      scorer / under any ops.Model, the attention model included (nann_search_candidates[_model]);
  * `search_multi()` / `search_all_multi()` / `union_topk()` several interest vectors per user: the k best distinct rows by
                      the best score any vector gives a row, through the traversal / exhaustively, and the union step on its
                      own for result lists from anywhere (nann_search_multi, nann_search_all_multi, nann_union_topk);
  * `search_grouped()` / `search_model_grouped()` / `search_all_grouped()` / `search_all_model_grouped()` / `cap_groups()`
                      at most m rows of one group (seller, category, brand: make_groups) among the k a query returns,
                      through the traversal / exhaustively, and the cap on its own for ranked lists from anywhere
                      (nann_search_grouped, nann_search_all_grouped, their _model forms, nann_group_cap_topk);
  * `search_diverse()` / `search_model_diverse()` / `search_all_diverse()` / `search_all_model_diverse()` / `mmr()`
                      diversified results: MMR re-ranking (make_diversity) of the fetched top-F into k picks, through the
                      traversal / exhaustively, and the step on its own for lists from anywhere
                      (nann_search_diverse, nann_search_all_diverse, their _model forms, nann_mmr_topk);
  * `fuse_topk()` / `fuse_results()` / `search_multi_fused()` / `search_all_multi_fused()` fused result lists: reciprocal rank
                      fusion or a weighted sum of raw, floor-shifted or min-max-normalised scores (make_fusion) over a user's
                      lists -- the step on its own, over the results of several searches (hybrid retrieval), and behind the
                      multi-vector traversal / exhaustive search (nann_fuse_topk, nann_search_multi_fused,
                      nann_search_all_multi_fused);
  * `search_per_op()` the same schedule spelled op by op with the drop-in ops
                      of nann_amd.ops, line for line against build_model(), so
                      that each op is exercised in the composition the
                      reference uses it in (plumbing/parity, not performance).
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib, ops
from ._lib import lib
from .ops import _check, _ptr, _stream


class Index:
    """Device-resident corpus + graph: what the serving graph's HugeConst nodes
    hold (build_opt_graph.py:83-90) plus the baked enter_points Const (:70)."""

    def __init__(self, item_embs, item_ids, nb_values, nb_row_splits, enter_points, device=None):
        dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")

        def put(a, dt):
            if isinstance(a, torch.Tensor):
                return a.to(device=dev, dtype=dt).contiguous()
            return torch.as_tensor(np.ascontiguousarray(a)).to(device=dev, dtype=dt).contiguous()

        if isinstance(item_embs, np.ndarray) and item_embs.dtype == np.uint16:  # bf16 bit patterns
            self.item_embs = torch.as_tensor(item_embs.view(np.int16)).to(dev).view(torch.bfloat16)
        elif isinstance(item_embs, torch.Tensor):
            self.item_embs = item_embs.to(dev).contiguous()
        else:
            self.item_embs = torch.as_tensor(np.ascontiguousarray(item_embs)).to(dev)
        self.item_ids = put(item_ids, torch.int64)
        self.nb_values = [put(nb_values[l], torch.int32) for l in (0, 1)]
        self.nb_row_splits = [put(nb_row_splits[l], torch.int64) for l in (0, 1)]
        self.enter_points = put(enter_points, torch.int32)
        self.n_items, self.d = self.item_embs.shape
        desc = _lib.IndexDesc()
        desc.n_items, desc.d = self.n_items, self.d
        desc.emb_dtype = ops._DT[self.item_embs.dtype]
        desc.item_embs = self.item_embs.data_ptr()
        desc.item_ids = self.item_ids.data_ptr()
        for l in (0, 1):
            desc.nb_values[l] = self.nb_values[l].data_ptr()
            desc.nb_row_splits[l] = self.nb_row_splits[l].data_ptr()
            desc.nb_nnz[l] = self.nb_values[l].numel()
        desc.enter_points = self.enter_points.data_ptr()
        desc.n_enter = self.enter_points.numel()
        desc.on_device = 1
        self.handle = C.c_void_p(0)
        with torch.cuda.device(dev):
            _check(lib().nann_index_create(C.byref(desc), C.byref(self.handle)), "index")
        info = (C.c_int64 * 6)()
        _check(lib().nann_index_info(self.handle, info))
        self.max_deg = (int(info[3]), int(info[4]))
        pr = (C.c_float * 5)()
        _check(lib().nann_index_probe_info(self.handle, pr))
        # the probe launch of nann_index_create: new level-0 nodes per frontier row on this graph (what the planner sizes
        # a query's visited set with); None for toy indices / corpora whose probe requests all failed
        self.probe = ({"queries": int(pr[0]), "ef": int(pr[1]), "new_per_row_mean": round(float(pr[2]), 3),
                       "new_per_row_q90": round(float(pr[3]), 3), "new_per_row_max": round(float(pr[4]), 3)} if pr[0] > 0 else None)
        self.bitmap_words = int(math.ceil(self.n_items / 32))  # build_opt_graph.py:114
        self.device = dev
        self._ws = None

    @classmethod
    def from_files(cls, index_dir, item_embs_dir, start_level=2):
        """Load the reference's on-disk artefacts straight into HBM through HugeConst, with the
        dtype casts build_model() requests (build_opt_graph.py:70,83-90): `item_embs.npy` -> f16,
        `item_ids.npy` i64, `neighbors_level_{l}_values.npy` -> i32, `..._row_splits.npy` i64,
        `enter_points.npy` -> i32 (files as written by build_hnsw_index.py:41-67)."""
        import os
        assert start_level == 2, "the serving graph walks levels 1 and 0 below the entry layer"
        hc = {
            "embs": ops.huge_const(os.path.join(item_embs_dir, "item_embs.npy"), np.float16),
            "ids": ops.huge_const(os.path.join(item_embs_dir, "item_ids.npy"), np.int64),
            "ep": ops.huge_const(os.path.join(index_dir, "enter_points.npy"), np.int32),
        }
        for l in (0, 1):
            hc[f"v{l}"] = ops.huge_const(os.path.join(index_dir, f"neighbors_level_{l}_values.npy"), np.int32)
            hc[f"rs{l}"] = ops.huge_const(os.path.join(index_dir, f"neighbors_level_{l}_row_splits.npy"), np.int64)
        ix = cls(hc["embs"].tensor, hc["ids"].tensor, [hc["v0"].tensor, hc["v1"].tensor],
                 [hc["rs0"].tensor, hc["rs1"].tensor], hc["ep"].tensor)
        ix._huge_consts = hc  # the HugeConst objects own the HBM the tensors view
        return ix

    @classmethod
    def from_dict(cls, g, device=None):
        return cls(g["item_embs"], g["item_ids"], g["nb_values"], g["nb_row_splits"], g["enter_points"],
                   device=device)

    def __del__(self):
        try:  # at interpreter shutdown the module globals may already be gone
            if getattr(self, "handle", None) and self.handle.value:
                lib().nann_index_destroy(self.handle)
                self.handle = C.c_void_p(0)
        except Exception:
            pass

    def workspace(self, level_topn, n_queries):
        t = (C.c_int32 * 6)(*[int(x) for x in level_topn])
        nbytes = C.c_int64(0)
        _check(lib().nann_search_workspace_bytes(self.handle, t, C.c_int64(n_queries), C.byref(nbytes)))
        # a fresh buffer per call (torch's caching allocator makes it cheap and stream-ordered):
        # concurrent searches on one Index from several threads/streams must not share scratch
        return torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=self.device)


TRAVERSAL_MODES = {"auto": 0, "lds_bitmap": 1, "hbm_bitmap": 2, "lds_hash": 3, "lds_hash32": 4}


def set_traversal_mode(mode="auto"):
    """Where nann_search keeps a query's visited set (include/nann_hip.h, nann_traversal_mode):
    "auto" | "lds_bitmap" | "hbm_bitmap" | "lds_hash" | "lds_hash32".  Results are identical in every mode; the
    knob exists for the parity tests and for tuning.  The process default of search_options(traversal=...)."""
    _check(lib().nann_set_traversal_mode(C.c_int32(TRAVERSAL_MODES[mode])), "traversal mode")


MLP_FORMS = {"auto": 0, "fused": 1, "phased": 2}


def search_options(traversal=None, slot_reserve=None, preprojection=None, mlp_form=None):
    """nann_search_options for one call; None = the process default of the field (nann_set_* / built-in)."""
    o = _lib.SearchOptions()
    lib().nann_search_options_init(C.byref(o))
    if traversal is not None:
        o.traversal_mode = TRAVERSAL_MODES[traversal]
    if slot_reserve is not None:
        o.slot_reserve = int(slot_reserve)
    if preprojection is not None:
        o.preprojection = 1 if preprojection else 0
    if mlp_form is not None:
        o.mlp_form = MLP_FORMS[mlp_form]
    return o


class SearchResult:
    __slots__ = ("item_ids", "scores", "index", "status", "counters", "phase_ticks", "plan", "_ws", "slot_reserve", "n_out")

    def __init__(self, item_ids, scores, index, status, counters, phase_ticks=None, plan=None, ws=None, slot_reserve=None,
                 n_out=None):
        self.item_ids, self.scores, self.index, self.status, self.counters = (
            item_ids, scores, index, status, counters)
        self.n_out = n_out  # filtered calls: i32[B], valid entries at the head of each row (None: an unfiltered call)
        self.phase_ticks = phase_ticks
        self.plan = plan  # dict: what the planner chose (nann_search_plan)
        self._ws = ws
        self.slot_reserve = slot_reserve  # nann_search_options.slot_reserve of the call (None: no options were passed)

    def reruns(self):
        """queries of this call that the hash-set kernel handed back to the bitmap kernel (synchronises the stream;
        read it before the next search on the same index reuses the workspace)"""
        n = C.c_int64(0)
        _check(lib().nann_search_reruns(_ptr(self._ws), C.byref(n), _stream()), "reruns")
        return n.value

    def refined(self):
        """rows of this call rescored exactly per round (precision="certified" in the pipeline of phases; zeros
        elsewhere): a list of NUM_ROUNDS ints, to set against counters[:, 2, :].sum(0) (synchronises the stream;
        read it before the next search on the same index reuses the workspace)"""
        out = (C.c_int64 * _lib.NUM_ROUNDS)()
        _check(lib().nann_search_refined(_ptr(self._ws), out, _stream()), "refined")
        return list(out)


def _level_topn_args(level_topn, b, dev):
    """level_topn as the C ABI takes it: uniform i32[6] -> (maxima, NULL); per query [B, 6] (the reference feeds
    `level_topn` per request, build_opt_graph.py:75,151-159) -> (column maxima [host], device i32[B, 6])."""
    lt = np.asarray(level_topn.cpu() if isinstance(level_topn, torch.Tensor) else level_topn, dtype=np.int64)
    if lt.ndim == 1:
        assert lt.shape[0] == 6
        return (C.c_int32 * 6)(*[int(x) for x in lt]), None, int(lt[5])
    assert lt.shape == (b, 6), "per-query level_topn: [n_queries, 6]"
    mx = np.maximum(lt.max(axis=0), 0)
    tq = torch.as_tensor(lt.astype(np.int32)).to(dev).contiguous()
    return (C.c_int32 * 6)(*[int(x) for x in mx]), tq, int(mx[5])


_VIS_NAMES = {v: k for k, v in TRAVERSAL_MODES.items()}


def _plan_dict(p):
    return {"visited_set": _VIS_NAMES.get(p.visited_set, p.visited_set), "fallback_visited_set": _VIS_NAMES.get(p.fallback_visited_set),
            "threads": p.threads, "workgroups": p.workgroups, "phased": bool(p.phased), "table": bool(p.table),
            "est_visited": round(float(p.est_visited), 1), "worst_visited": round(float(p.worst_visited), 1),
            "lean": int(p.lean)}


class Filter:
    """What make_filter returns: the tensors of a nann_filter (they may live on the CPU: the bit layout is testable without a
    GPU) and its ctypes struct, which borrows their memory.
      deny_bits   i32[ceil(n_items / 32)] or None: row r is denied for every query when bit (r & 31) of word (r >> 5) is set
      row_splits  i64[n_queries + 1] or None; rows i32[n_excl]: query i excludes rows[row_splits[i] : row_splits[i + 1]]"""
    __slots__ = ("deny_bits", "row_splits", "rows", "n_queries", "n_items", "device", "struct")

    def __init__(self, deny_bits, row_splits, rows, n_items, device):
        self.deny_bits, self.row_splits, self.rows, self.n_items, self.device = deny_bits, row_splits, rows, n_items, device
        self.n_queries = None if row_splits is None else int(row_splits.numel()) - 1
        st = _lib.Filter()
        st.struct_bytes = C.sizeof(_lib.Filter)
        st.deny_bits = deny_bits.data_ptr() if deny_bits is not None else None
        st.excl_row_splits = row_splits.data_ptr() if row_splits is not None else None
        st.excl_rows = rows.data_ptr() if rows is not None and rows.numel() else None
        st.n_excl = int(rows.numel()) if rows is not None else 0
        self.struct = st


def _sorted_item_ids(index):
    """(item ids ascending, the row of each): built once per Index and cached on it"""
    c = getattr(index, "_sorted_ids", None)
    if c is None:
        vals, perm = torch.sort(index.item_ids)
        c = index._sorted_ids = (vals, perm)
    return c


def _rows_of_item_ids(index, ids):
    """internal rows of item ids (any array-like) on the device of index.item_ids; an unknown id is dropped"""
    vals, perm = _sorted_item_ids(index)
    ids = torch.as_tensor(np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids, dtype=np.int64)).reshape(-1).to(vals.device)
    if vals.numel() == 0 or ids.numel() == 0:
        return ids[:0]
    pos = torch.searchsorted(vals, ids).clamp_(max=vals.numel() - 1)
    return perm[pos][vals[pos] == ids]


def _i64(a):
    return torch.as_tensor(np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a, dtype=np.int64)).reshape(-1)


def make_filter(index, deny_rows=None, deny_item_ids=None, exclude_rows=None, exclude_item_ids=None, device=None):
    """A nann_filter for searches on `index`: rows denied for EVERY query (deny_rows: internal row numbers; deny_item_ids:
    item ids) and, per query, a list of excluded rows (exclude_rows / exclude_item_ids: one 1-D array per query of the
    batch the filter will be used with; both given: their union).  Item ids map to rows through a sorted copy of
    index.item_ids, built once per Index (an unknown id denies nothing; of rows that share an item id one is found).  Rows
    outside [0, n_items) deny nothing: deny_rows drops them here, the lists keep them and the kernels skip them.
    device: where the tensors live (default: the index's; "cpu" builds the same bits without a GPU).  -> Filter."""
    dev = torch.device(device if device is not None else index.device)
    n = int(index.n_items)
    deny = []
    if deny_rows is not None:
        deny.append(_i64(deny_rows))
    if deny_item_ids is not None:
        deny.append(_rows_of_item_ids(index, deny_item_ids).cpu().to(torch.int64))
    bits = None
    if deny:
        r = torch.cat(deny)
        r = r[(r >= 0) & (r < n)]
        words = (n + 31) // 32
        flags = torch.zeros(words * 32, dtype=torch.bool)
        flags[r] = True
        w = (flags.view(words, 32).to(torch.int64) << torch.arange(32, dtype=torch.int64)).sum(1)
        bits = torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32).to(dev).contiguous()
    splits = rows = None
    if exclude_rows is not None or exclude_item_ids is not None:
        nq = len(exclude_rows if exclude_rows is not None else exclude_item_ids)
        assert exclude_rows is None or exclude_item_ids is None or len(exclude_rows) == len(exclude_item_ids)
        per = []
        for i in range(nq):
            parts = []
            if exclude_rows is not None:
                parts.append(_i64(exclude_rows[i]))
            if exclude_item_ids is not None:
                parts.append(_rows_of_item_ids(index, exclude_item_ids[i]).cpu().to(torch.int64))
            per.append(torch.cat(parts))
        lens = torch.tensor([0] + [int(p.numel()) for p in per], dtype=torch.int64)
        splits = torch.cumsum(lens, 0).to(dev).contiguous()
        flat = torch.cat(per) if per else torch.zeros(0, dtype=torch.int64)
        assert flat.numel() == 0 or (int(flat.min()) >= -(1 << 31) and int(flat.max()) < (1 << 31)), "row numbers are 32-bit"
        rows = flat.to(torch.int32).to(dev).contiguous()
    return Filter(bits, splits, rows, n, dev)


def pool_width(level_topn):
    """The widest useful fetch width of a filtered search: the last stage of the traversal ranks a pool of level_topn[1] + ...
    + level_topn[4] distinct rows, and a list holds at most 1024."""
    return min(int(sum(int(x) for x in list(level_topn)[1:5])), 1024)


def _filter_args(filter, b, index):
    """(POINTER(nann_filter) or None) for a batch of b queries on `index`"""
    if filter is None:
        return None
    assert filter.n_items == index.n_items, "the filter was made for another index"
    assert filter.device == index.device, "the filter's tensors must live on the index's device"
    assert filter.n_queries is None or filter.n_queries == b, "the filter's exclusion lists: one per query of the batch"
    return C.byref(filter.struct)


def search(index, scorer, q, level_topn, want_counters=True, want_phase_ticks=False, options=None, filter=None, k=None):
    """Fused execution of build_model()'s schedule for a batch of queries.
    q: f32[B, d] CUDA tensor (ops.user_seq_mean of `comm_seq`).  level_topn: i32[6] for the whole batch, or
    [B, 6] per query (nann_search_v; rows of the outputs are level_topn.max(0)[5] wide, zero behind a query's
    own k).  options: search_options(...) for this call (nann_search_opt).  Asynchronous: the returned tensors are valid
    once the current stream reaches them.  status[b] != 0 marks a request the reference would have failed.
    filter (make_filter) and / or k: the filtered call (nann_search_filtered) -- level_topn[5] is then the FETCH WIDTH F
    (pool_width(level_topn) ranks the whole pool), the outputs are [B, k] (k = F when not given): the first k allowed entries
    of the unfiltered answer at F, result.n_out[b] of them at the head of row b and zeros behind."""
    q = q.to(device=index.device, dtype=torch.float32).contiguous()
    return _traverse(index, scorer, q, False, level_topn, want_counters, want_phase_ticks, options, filter, k)


# (model form, filtered) -> (the call that sizes the workspace -- None: index.workspace --, the search call)
_TRAVERSE_CALLS = {(False, False): (None, "nann_search_opt"), (True, False): ("nann_search_model_workspace_bytes", "nann_search_model_opt"),
                   (False, True): ("nann_search_filtered_workspace_bytes", "nann_search_filtered"),
                   (True, True): ("nann_search_model_filtered_workspace_bytes", "nann_search_model_filtered")}


def _traverse(index, by, x, model, level_topn, want_counters, want_phase_ticks, options, filter, k, predicates=None):
    """The traversal family's call (_TRAVERSE_CALLS) for the b rows of x -- queries of a scorer `by`, sequences of a model one; with
    a filter or a k the _filtered twin, with predicates the _where one -- into fresh outputs and a workspace of the size its
    _workspace_bytes twin gives."""
    dev, b = index.device, x.shape[0]
    t, tq, k_fetch = _level_topn_args(level_topn, b, dev)
    filtered = filter is not None or k is not None or predicates is not None
    k = int(k) if filtered and k is not None else k_fetch
    kk = max(k, 0) if filtered else k
    out_ids = torch.empty((b, kk), dtype=torch.int64, device=dev)
    out_scores = torch.empty((b, kk), dtype=torch.float32, device=dev)
    out_index = torch.empty((b, kk), dtype=torch.int32, device=dev)
    n_out = torch.zeros(b, dtype=torch.int32, device=dev) if filtered else None
    status = torch.empty(b, dtype=torch.int32, device=dev)
    counters = torch.zeros((b, 3, _lib.NUM_ROUNDS), dtype=torch.int32, device=dev) if want_counters else None
    ticks = torch.zeros((b, _lib.NUM_PHASES), dtype=torch.int64, device=dev) if want_phase_ticks else None
    assert not (want_phase_ticks and tq is not None), "phase ticks: uniform level_topn only"
    L, (size_call, search_call) = lib(), _TRAVERSE_CALLS[model, filtered]
    if predicates is not None:
        size_call, search_call = size_call.replace("_filtered", "_where"), search_call.replace("_filtered", "_where")
    if size_call is None:
        ws = index.workspace(list(t), b)
    else:
        nbytes = C.c_int64(0)
        handles = (index.handle, by.handle) if model else (index.handle,)  # (a model form is sized for its model)
        _check(getattr(L, size_call)(*handles, t, C.c_int64(b), C.byref(nbytes)), "search")
        ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    plan = _lib.SearchPlan()
    ticks_arg = () if model else (_ptr(ticks),)  # the model forms have no phase ticks
    filter_args = (_filter_args(filter, b, index), k, _ptr(n_out)) if filtered else ()  # what the filtered forms end on
    if predicates is not None:
        filter_args = (filter_args[0], _predicates_args(predicates, b, int(index.n_items), dev)) + filter_args[1:]
    with torch.cuda.device(dev):
        _check(getattr(L, search_call)(index.handle, by.handle, _ptr(x), C.c_int64(b), t, _ptr(tq), _ptr(ws), C.c_int64(ws.numel()),
                                       _ptr(out_ids), _ptr(out_scores), _ptr(out_index), _ptr(status), _ptr(counters), *ticks_arg,
                                       C.byref(options) if options is not None else None, C.byref(plan), *filter_args, _stream()), "search")
    return SearchResult(out_ids, out_scores, out_index, status, counters, ticks, _plan_dict(plan), ws,
                        slot_reserve=int(options.slot_reserve) if options is not None else None, n_out=n_out)


def search_model(index, model, comm_seq, level_topn, want_counters=True, options=None, filter=None, k=None):
    """The serving signature (build_opt_graph.py:151-159) for a batch: comm_seq f16[B, seq_len, E] +
    level_topn (i32[6], or [B, 6] per request) -> SearchResult, scored by `model` (ops.Model: l2 / mlp / the
    reference's attention + DNN model -- the per-user projection runs once per request, then the fused traversal;
    nann_search_model_opt).  filter / k: as search() takes them (nann_search_model_filtered)."""
    seq = comm_seq.to(device=index.device, dtype=torch.float16).contiguous()
    return _traverse(index, model, seq, True, level_topn, want_counters, False, options, filter, k)


class SearchAllResult:
    """Outputs of search_all: the top k of EVERY item per query, TopKV2 order (device tensors).  A filtered call: the top k
    of every ALLOWED item, n_out[b] valid entries at the head of row b and zeros behind (n_out is None unfiltered)."""
    __slots__ = ("item_ids", "scores", "index", "_ws", "n_out")

    def __init__(self, item_ids, scores, index, ws=None, n_out=None):
        self.item_ids, self.scores, self.index, self._ws, self.n_out = item_ids, scores, index, ws, n_out


def search_all(index, scorer, q, k, options=None, filter=None):
    """Exhaustive search for a batch (nann_search_all; the reference's test_all job, main.py:194-237): every item of
    `index` scored for every query, top k per query -- descending, ties -> lower internal row number.  `scorer`:
    ops.Scorer with q f32[B, d], or an ops.Model of kind l2 / mlp with q = comm_seq f16[B, seq_len, d] (its
    ops.user_seq_mean is the query); an attention model raises NotImplementedError (score it user by user:
    evaluate.test_all).  options: search_options(preprojection=...).  Asynchronous on torch's current stream.
    An MLP scorer reads its pre-projected table; without one the call raises ops.NannError with status 103 (no room in
    HBM) or 102 (pre-projection switched off).  filter (make_filter): the top k of the ALLOWED rows
    (nann_search_all_filtered), result.n_out[b] of them -- the ground truth of a filtered search()."""
    dev = index.device
    handle = scorer.handle
    if isinstance(scorer, ops.Model):
        if scorer.kind == "attention":
            raise NotImplementedError("search_all: l2 / mlp scorers only; the attention model is scored user by user")
        q = ops.user_seq_mean(q.to(dev))
        handle = C.c_void_p(lib().nann_model_scorer(scorer.handle))  # (borrowed: the model owns it)
    q = q.to(device=dev, dtype=torch.float32).contiguous()
    return _flat_all(index, handle, q, k, options, filter, "nann_search_all", "search_all")


def _flat_all(index, handle, x, k, options, filter, symbol, what, predicates=None):
    """The exhaustive family's call: `symbol` (with _filtered under a filter, _where under predicates) for the b rows of x -- the
    queries of a scorer `handle`, the sequences of a model one -- into fresh outputs and a workspace of the size its
    _workspace_bytes twin gives."""
    dev = index.device
    b, k = x.shape[0], int(k)
    kk = max(k, 0)
    out_ids = torch.empty((b, kk), dtype=torch.int64, device=dev)
    out_scores = torch.empty((b, kk), dtype=torch.float32, device=dev)
    out_index = torch.empty((b, kk), dtype=torch.int32, device=dev)
    n_out = None
    if predicates is not None:
        symbol += "_where"
        n_out = torch.zeros(b, dtype=torch.int32, device=dev)
    elif filter is not None:
        symbol += "_filtered"
        n_out = torch.zeros(b, dtype=torch.int32, device=dev)
    nbytes = C.c_int64(0)
    _check(getattr(lib(), symbol + "_workspace_bytes")(index.handle, handle, b, k, C.byref(nbytes)), what)
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        tail = (_filter_args(filter, b, index), _ptr(n_out)) if filter is not None else ()
        if predicates is not None:
            tail = (_filter_args(filter, b, index), _predicates_args(predicates, b, int(index.n_items), dev), _ptr(n_out))
        _check(getattr(lib(), symbol)(index.handle, handle, _ptr(x), b, k, _ptr(out_ids), _ptr(out_scores), _ptr(out_index),
                                      _ptr(ws), ws.numel(), C.byref(options) if options is not None else None, *tail, _stream()),
               what)
    return SearchAllResult(out_ids, out_scores, out_index, ws, n_out)


class Sq8:
    """The int8 code table of an index's rows (nann_sq8; make_sq8).  It borrows the index -- the object keeps it alive -- and
    is STALE once the index's rows were refreshed in place: make a new one.  codes() i8[n_items, d], scales() f32[n_items],
    norms() i32[n_items] are torch views of the table's device memory, valid until release()."""

    def __init__(self, index):
        self.index = index
        self.handle = C.c_void_p(0)
        with torch.cuda.device(index.device):
            _check(lib().nann_sq8_create(index.handle, _stream(), C.byref(self.handle)), "make_sq8")
        info = (C.c_int64 * 4)()
        _check(lib().nann_sq8_info(self.handle, info))
        self.n_items, self.d, self.nbytes = int(info[0]), int(info[1]), int(info[2])

    def _views(self):
        if not self.handle.value:
            raise ValueError("Sq8: released")
        p = [C.c_void_p(0) for _ in range(3)]
        _check(lib().nann_sq8_view(self.handle, *[C.byref(v) for v in p]))
        return [v.value for v in p]

    def _wrap(self, ptr, shape, dtype):
        with torch.cuda.device(self.index.device):
            return ops._wrap_device_pointer(ptr, shape, dtype, self)

    def codes(self):
        return self._wrap(self._views()[0], (self.n_items, self.d), torch.int8)

    def scales(self):
        return self._wrap(self._views()[1], (self.n_items,), torch.float32)

    def norms(self):
        return self._wrap(self._views()[2], (self.n_items,), torch.int32)

    def release(self):
        """Free the table's device memory (the views die with it).  Synchronise streams that still read it first."""
        if self.handle.value:
            lib().nann_sq8_destroy(self.handle)
            self.handle = C.c_void_p(0)

    def __del__(self):
        try:  # at interpreter shutdown the module globals may already be gone
            if getattr(self, "handle", None) and self.handle.value:
                lib().nann_sq8_destroy(self.handle)
                self.handle = C.c_void_p(0)
        except Exception:
            pass


def make_sq8(index):
    """The int8 code table of `index`'s rows (nann_sq8_create): per row d codes, a scale and a norm -- half the bytes of the
    16-bit rows next to them, which the re-rank of search_all_sq8 still reads.  f16 / bf16 rows, d in {64, 128, 256, 512};
    an f32 index raises ops.UnimplementedError.  Encoded on torch's current stream.  Re-create it after the rows of the
    index were refreshed in place."""
    return Sq8(index)


class Sq8Result:
    """Outputs of search_all_sq8: item_ids i64[B, k], scores f32[B, k] (exact, nann_score's bits), index i32[B, k]; with
    return_fetch the approximate stage's lists fetch_index i32[B, fetch], fetch_scores f32[B, fetch], else None."""
    __slots__ = ("item_ids", "scores", "index", "fetch_index", "fetch_scores", "fetch", "_ws")

    def __init__(self, item_ids, scores, index, fetch_index, fetch_scores, fetch, ws=None):
        self.item_ids, self.scores, self.index = item_ids, scores, index
        self.fetch_index, self.fetch_scores, self.fetch, self._ws = fetch_index, fetch_scores, fetch, ws


def search_all_sq8(index, sq8, scorer, q, k, fetch=None, options=None, return_fetch=False):
    """Scalar-quantised exhaustive search (nann_search_all_sq8): every row's int8 code scored against the query's on the
    integer matrix cores, the `fetch` best rows by that approximate score re-ranked by the EXACT score, top k of those --
    descending, ties -> lower internal row number; the scores are search_all's bits for the rows returned.  `scorer`: an l2
    or ip ops.Scorer with q f32[B, d] (an MLP scorer raises ops.UnimplementedError).  sq8: make_sq8(index).
    fetch=None means min(4 * k, 1024, n_items): a convenience default, NOT a tuned one -- recall against search_all grows
    with fetch, and so does the selection's time; measure on your corpus (tools/sq8_rate.py).  k <= fetch <= 1024.
    return_fetch: also return the approximate stage's lists.  Asynchronous on torch's current stream."""
    dev = index.device
    q = q.to(device=dev, dtype=torch.float32).contiguous()
    b, k = q.shape[0], int(k)
    fetch = min(4 * k, 1024, int(index.n_items)) if fetch is None else int(fetch)
    kk, ff = max(k, 0), max(fetch, 0)
    out_ids = torch.empty((b, kk), dtype=torch.int64, device=dev)
    out_scores = torch.empty((b, kk), dtype=torch.float32, device=dev)
    out_index = torch.empty((b, kk), dtype=torch.int32, device=dev)
    f_index = torch.empty((b, ff), dtype=torch.int32, device=dev) if return_fetch else None
    f_scores = torch.empty((b, ff), dtype=torch.float32, device=dev) if return_fetch else None
    nbytes = C.c_int64(0)
    _check(lib().nann_search_all_sq8_workspace_bytes(index.handle, sq8.handle, scorer.handle, b, fetch, k, C.byref(nbytes)),
           "search_all_sq8")
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(lib().nann_search_all_sq8(index.handle, sq8.handle, scorer.handle, _ptr(q), b, fetch, k, _ptr(out_ids),
                                         _ptr(out_scores), _ptr(out_index), _ptr(f_index), _ptr(f_scores), _ptr(ws), ws.numel(),
                                         C.byref(options) if options is not None else None, _stream()), "search_all_sq8")
    return Sq8Result(out_ids, out_scores, out_index, f_index, f_scores, fetch, ws)


class Sq8Bounds:
    """The per-row error terms of a code table (nann_sq8_bounds; make_sq8_bounds): err() f32[n_items] >= |x_i - scale_i codes_i|,
    xhat() f32[n_items] >= scale_i sqrt(norm_i), torch views of device memory valid until release().  It borrows the index and
    the table -- the object keeps both alive -- and goes STALE with the table."""

    def __init__(self, index, sq8):
        self.index, self.sq8 = index, sq8
        self.handle = C.c_void_p(0)
        with torch.cuda.device(index.device):
            _check(lib().nann_sq8_bounds_create(index.handle, sq8.handle, _stream(), C.byref(self.handle)), "make_sq8_bounds")
        self.n_items = sq8.n_items

    def _views(self):
        if not self.handle.value:
            raise ValueError("Sq8Bounds: released")
        p = [C.c_void_p(0) for _ in range(2)]
        _check(lib().nann_sq8_bounds_view(self.handle, *[C.byref(v) for v in p]))
        with torch.cuda.device(self.index.device):
            return [ops._wrap_device_pointer(v.value, (self.n_items,), torch.float32, self) for v in p]

    def err(self):
        return self._views()[0]

    def xhat(self):
        return self._views()[1]

    def release(self):
        """Free the device memory (the views die with it).  Synchronise streams that still read it first."""
        if self.handle.value:
            lib().nann_sq8_bounds_destroy(self.handle)
            self.handle = C.c_void_p(0)

    def __del__(self):
        try:  # at interpreter shutdown the module globals may already be gone
            if getattr(self, "handle", None) and self.handle.value:
                lib().nann_sq8_bounds_destroy(self.handle)
                self.handle = C.c_void_p(0)
        except Exception:
            pass


def make_sq8_bounds(index, sq8):
    """The error terms of `sq8`'s rows (nann_sq8_bounds_create), what search_all_sq8_exact certifies with: 8 bytes per row.
    Computed on torch's current stream.  Re-create it with the table."""
    return Sq8Bounds(index, sq8)


class Sq8ExactResult:
    """Outputs of search_all_sq8_exact: item_ids i64[B, k], scores f32[B, k], index i32[B, k]; certified i32[B] (1: the row is
    search_all's, bit for bit), n_survivors i32[B] (rows the bound could not exclude, whatever the cap)."""
    __slots__ = ("item_ids", "scores", "index", "certified", "n_survivors", "fetch", "cap", "_ws")

    def __init__(self, item_ids, scores, index, certified, n_survivors, fetch, cap, ws=None):
        self.item_ids, self.scores, self.index = item_ids, scores, index
        self.certified, self.n_survivors, self.fetch, self.cap, self._ws = certified, n_survivors, fetch, cap, ws


def search_all_sq8_exact(index, sq8, bounds, scorer, q, k, fetch=None, cap=2048, fallback=True, options=None):
    """Certified scalar-quantised exhaustive search (nann_search_all_sq8_exact): search_all's result BIT FOR BIT -- item ids,
    scores, index, ties to the lower row -- from the int8 scan.  Per query: search_all_sq8's fetch and exact re-rank at `fetch`
    give a cut; every row whose exact score a rigorous error bound cannot put below the cut survives; the exact top k of the
    survivors is the answer.  result.certified[b] == 1 iff at most `cap` rows survived (and the query is finite); an uncertified
    row of the result is search_all_sq8's answer at the same fetch.  `scorer`: an l2 or ip ops.Scorer with q f32[B, d]; sq8:
    make_sq8(index); bounds: make_sq8_bounds(index, sq8).  fetch=None means min(max(k, 1), 1024, n_items); k <= fetch <= cap.
    fallback=True: the wrapper reads `certified` back -- ONE synchronisation of the stream with the host -- and re-runs the
    uncertified queries through search_all, so that the result is exact for EVERY query (certified and n_survivors stay as the
    device call left them).  fallback=False: asynchronous on torch's current stream, nothing read back."""
    dev = index.device
    q = q.to(device=dev, dtype=torch.float32).contiguous()
    b, k = q.shape[0], int(k)
    fetch = min(max(k, 1), 1024, int(index.n_items)) if fetch is None else int(fetch)
    cap = int(cap)
    kk = max(k, 0)
    out_ids = torch.empty((b, kk), dtype=torch.int64, device=dev)
    out_scores = torch.empty((b, kk), dtype=torch.float32, device=dev)
    out_index = torch.empty((b, kk), dtype=torch.int32, device=dev)
    certified = torch.zeros(b, dtype=torch.int32, device=dev)
    n_surv = torch.zeros(b, dtype=torch.int32, device=dev)
    nbytes = C.c_int64(0)
    bh = bounds.handle if bounds is not None else None
    _check(lib().nann_search_all_sq8_exact_workspace_bytes(index.handle, sq8.handle, bh, scorer.handle, b, fetch, cap, k,
                                                           C.byref(nbytes)), "search_all_sq8_exact")
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(lib().nann_search_all_sq8_exact(index.handle, sq8.handle, bh, scorer.handle, _ptr(q), b, fetch, cap, k, _ptr(out_ids),
                                               _ptr(out_scores), _ptr(out_index), _ptr(certified), _ptr(n_surv), _ptr(ws), ws.numel(),
                                               C.byref(options) if options is not None else None, _stream()), "search_all_sq8_exact")
    if fallback and b > 0 and k > 0:
        todo = torch.nonzero(certified == 0).flatten()  # (the synchronisation)
        if todo.numel() > 0:
            r = search_all(index, scorer, q[todo], k, options=options)
            out_ids[todo], out_scores[todo], out_index[todo] = r.item_ids, r.scores, r.index
    return Sq8ExactResult(out_ids, out_scores, out_index, certified, n_surv, fetch, cap, ws)


def search_all_model(index, model, comm_seq, k, options=None):
    """Exhaustive search under a model (nann_search_all_model; the reference's test_all job, main.py:194-237, which scores
    its own attention + DNN model): every item of `index` scored for every user of comm_seq f16[B, seq_len, E], top k per
    user -- descending, ties -> lower internal row number -> SearchAllResult.  `model`: an ops.Model of any kind (l2 / mlp:
    the bits of search_all(index, model, comm_seq, k); attention: scored on the device from the model's pre-projected
    table, split-f16 scores bit-identical to the traversal's); an ops.Scorer raises TypeError (search_all takes those).
    options: search_options(preprojection=...).  Asynchronous on torch's current stream.  An attention or MLP model reads
    its pre-projected table; without one the call raises ops.NannError with status 103 (no room in HBM) or 102
    (pre-projection switched off).  With a filter: search_all_model_filtered."""
    return _search_all_model(index, model, comm_seq, k, options, None)


def search_all_model_filtered(index, model, comm_seq, k, filter, options=None):
    """search_all_model over the ALLOWED rows (nann_search_all_model_filtered): `filter` as search_all takes it (make_filter),
    result.n_out[b] valid entries at the head of row b and zeros behind.  A function of its own: search_all_model's argument
    list is pinned by its callers."""
    return _search_all_model(index, model, comm_seq, k, options, filter)


def _search_all_model(index, model, comm_seq, k, options, filter):
    if not isinstance(model, ops.Model):
        raise TypeError("search_all_model: an ops.Model (an ops.Scorer goes through search_all)")
    seq = comm_seq.to(device=index.device, dtype=torch.float16).contiguous()
    return _flat_all(index, model.handle, seq, k, options, filter, "nann_search_all_model", "search_all_model")


class WideResult:
    """Outputs of search_all_wide, [B, k] device tensors: the top k of every query's rows that do not score -inf, TopKV2 order,
    n_out[b] = min(k, such rows) valid entries at the head of row b and zeros behind."""
    __slots__ = ("item_ids", "scores", "index", "n_out", "_ws")

    def __init__(self, item_ids, scores, index, n_out, ws=None):
        self.item_ids, self.scores, self.index, self.n_out, self._ws = item_ids, scores, index, n_out, ws


def search_all_wide(index, scorer, q, k, filter=None, predicates=None, options=None):
    """Exhaustive search for k up to _lib.WIDE_MAX_K = 16384 rows per query (nann_search_all_wide; the reference has no such
    call): every item of `index` scored as search_all scores it -- the same score bits -- and the exact top k per query, descending,
    ties to the lower row, by a selection whose cost does not grow with k -> WideResult.  A row scoring -inf is never returned
    (search_all_range's rule), so a filtered or predicated call needs no separate form: filter (make_filter) and predicates
    (make_predicates) are optional.  `scorer`: ops.Scorer with q f32[B, d], or an ops.Model of kind l2 / mlp with q = comm_seq (the
    attention model: search_all_model_wide).  Asynchronous on torch's current stream."""
    dev = index.device
    handle = scorer.handle
    if isinstance(scorer, ops.Model):
        if scorer.kind == "attention":
            raise NotImplementedError("search_all_wide: l2 / mlp scorers only; the attention model goes through search_all_model_wide")
        q = ops.user_seq_mean(q.to(dev))
        handle = C.c_void_p(lib().nann_model_scorer(scorer.handle))  # (borrowed: the model owns it)
    q = q.to(device=dev, dtype=torch.float32).contiguous()
    return _flat_wide(index, handle, q, k, filter, predicates, options, "nann_search_all_wide", "search_all_wide")


def search_all_model_wide(index, model, comm_seq, k, filter=None, predicates=None, options=None):
    """search_all_wide under a model (nann_search_all_model_wide): comm_seq f16[B, seq_len, E], `model` an ops.Model of any kind,
    the attention model included -- the score bits of search_all_model."""
    if not isinstance(model, ops.Model):
        raise TypeError("search_all_model_wide: an ops.Model (an ops.Scorer goes through search_all_wide)")
    seq = comm_seq.to(device=index.device, dtype=torch.float16).contiguous()
    return _flat_wide(index, model.handle, seq, k, filter, predicates, options, "nann_search_all_model_wide", "search_all_model_wide")


def _flat_wide(index, handle, x, k, filter, predicates, options, symbol, what):
    dev = index.device
    b, k = x.shape[0], int(k)
    kk = max(k, 0)
    out_ids = torch.empty((b, kk), dtype=torch.int64, device=dev)
    out_scores = torch.empty((b, kk), dtype=torch.float32, device=dev)
    out_index = torch.empty((b, kk), dtype=torch.int32, device=dev)
    n_out = torch.zeros(b, dtype=torch.int32, device=dev)
    nbytes = C.c_int64(0)
    _check(getattr(lib(), symbol + "_workspace_bytes")(index.handle, handle, b, k, C.byref(nbytes)), what)
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        pa = _predicates_args(predicates, b, int(index.n_items), dev) if predicates is not None else None
        _check(getattr(lib(), symbol)(index.handle, handle, _ptr(x), b, k, _ptr(out_ids), _ptr(out_scores), _ptr(out_index),
                                      _ptr(n_out), _ptr(ws), ws.numel(), C.byref(options) if options is not None else None,
                                      _filter_args(filter, b, index), pa, _stream()), what)
    return WideResult(out_ids, out_scores, out_index, n_out, ws)


# positions of the score buffer per workgroup of the range selection (csrc/nann_range.h: kRangeBlockRows)
RANGE_BLOCK_ROWS = 2048


class RangeResult:
    """Outputs of search_all_range (device tensors): ragged, query b owns the positions row_splits[b] .. row_splits[b + 1] of
    item_ids / scores / index (internal rows), in ascending row order (sort=True: score descending, ties to the lower row).
    row_splits i64[B + 1] holds the TRUE counts whatever the capacity; total = row_splits[B] (a host int); truncated: total >
    capacity -- the entry tensors then hold the head [0, capacity) of the whole result."""
    __slots__ = ("row_splits", "item_ids", "scores", "index", "total", "truncated", "_ws")

    def __init__(self, row_splits, item_ids, scores, index, total, truncated, ws=None):
        self.row_splits, self.item_ids, self.scores, self.index = row_splits, item_ids, scores, index
        self.total, self.truncated, self._ws = total, truncated, ws


def search_all_range(index, scorer, q, thresholds, capacity=None, filter=None, options=None, sort=False):
    """Range search for a batch (nann_search_all_range; the reference has no such call): every item of `index` scored for
    every query as search_all scores it -- the same score bits -- and every row with score >= thresholds[b] returned, denied
    rows and rows scoring -inf never, a NaN threshold nothing -> RangeResult.  `scorer`: ops.Scorer with q f32[B, d], or an
    ops.Model of kind l2 / mlp with q = comm_seq (its ops.user_seq_mean is the query; the attention model: search_all_range_model).
    thresholds: a float for every query, or a tensor / array of B floats.  capacity: entries of the outputs; what does not fit
    is dropped and result.truncated is set.  capacity=None runs a count-only call, reads the total on the host, then runs the
    filling call at exactly that capacity: THE INDEX IS SCORED TWICE, and the call synchronises.  filter: make_filter.
    sort=True reorders each segment by (score descending, row ascending) with torch on the device."""
    dev = index.device
    handle = scorer.handle
    if isinstance(scorer, ops.Model):
        if scorer.kind == "attention":
            raise NotImplementedError("search_all_range: l2 / mlp scorers only; the attention model goes through search_all_range_model")
        q = ops.user_seq_mean(q.to(dev))
        handle = C.c_void_p(lib().nann_model_scorer(scorer.handle))  # (borrowed: the model owns it)
    q = q.to(device=dev, dtype=torch.float32).contiguous()
    return _flat_range(index, handle, q, thresholds, capacity, filter, options, sort, "nann_search_all_range", "search_all_range")


def search_all_range_model(index, model, comm_seq, thresholds, capacity=None, filter=None, options=None, sort=False):
    """search_all_range under a model (nann_search_all_range_model): comm_seq f16[B, seq_len, E], `model` an ops.Model of any
    kind, the attention model included -- the score bits of search_all_model.  Everything else as search_all_range."""
    if not isinstance(model, ops.Model):
        raise TypeError("search_all_range_model: an ops.Model (an ops.Scorer goes through search_all_range)")
    seq = comm_seq.to(device=index.device, dtype=torch.float16).contiguous()
    return _flat_range(index, model.handle, seq, thresholds, capacity, filter, options, sort, "nann_search_all_range_model",
                       "search_all_range_model")


def _flat_range(index, handle, x, thresholds, capacity, filter, options, sort, symbol, what):
    dev, b = index.device, x.shape[0]
    if isinstance(thresholds, (int, float)):
        thr = torch.full((b,), float(thresholds), dtype=torch.float32, device=dev)
    else:
        thr = torch.as_tensor(thresholds).to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        assert thr.numel() == b, "thresholds: one per query of the batch"
    L = lib()
    nbytes = C.c_int64(0)
    _check(getattr(L, symbol + "_workspace_bytes")(index.handle, handle, b, C.byref(nbytes)), what)
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    splits = torch.zeros(b + 1, dtype=torch.int64, device=dev)

    def call(cap, ids, scores, rows):
        with torch.cuda.device(dev):
            _check(getattr(L, symbol)(index.handle, handle, _ptr(x), b, _ptr(thr), cap, _ptr(splits), _ptr(ids), _ptr(scores),
                                      _ptr(rows), _ptr(ws), ws.numel(), C.byref(options) if options is not None else None,
                                      _filter_args(filter, b, index), _stream()), what)

    counted = capacity is None
    if counted:  # count, read the total, fill: the index is scored twice
        call(0, None, None, None)
        capacity = int(splits[b].item()) if b else 0
    capacity = int(capacity)
    assert capacity >= 0, "capacity >= 0"
    ids = torch.zeros(capacity, dtype=torch.int64, device=dev)
    scores = torch.zeros(capacity, dtype=torch.float32, device=dev)
    rows = torch.zeros(capacity, dtype=torch.int32, device=dev)
    if capacity > 0:
        call(capacity, ids, scores, rows)
    elif not counted:
        call(0, None, None, None)
    total = int(splits[b].item()) if b else 0
    if sort:
        _range_sort(splits, ids, scores, rows, min(total, capacity))
    return RangeResult(splits, ids, scores, rows, total, total > capacity, ws)


def _range_sort(splits, ids, scores, rows, n):
    """the first n entries of a ragged result, each segment reordered by (score descending, row ascending), in place"""
    if n <= 1:
        return
    seg = torch.searchsorted(splits[1:].contiguous(), torch.arange(n, device=splits.device), right=True)  # the query of every entry
    # stable sorts, last key first: row ascending (the entries already are, within a query), score descending, query ascending
    order = torch.sort(scores[:n], descending=True, stable=True).indices
    order = order[torch.sort(seg[order], stable=True).indices]
    ids[:n], scores[:n], rows[:n] = ids[:n][order], scores[:n][order], rows[:n][order]


class Sq8RangeResult(RangeResult):
    """Outputs of search_all_range_sq8_exact: a RangeResult with certified i32[B] (1: the query's segment is search_all_range's,
    bit for bit; 0: the segment is empty unless the fallback has filled it) and n_survivors i32[B] (rows the bound could not put
    below the threshold, whatever the cap).  total and truncated are read from row_splits on first use -- a synchronisation,
    which a call with fallback=False has not paid before."""
    __slots__ = ("certified", "n_survivors", "cap", "capacity", "_total")

    def __init__(self, row_splits, item_ids, scores, index, certified, n_survivors, cap, capacity, total=None, ws=None):
        self.row_splits, self.item_ids, self.scores, self.index, self._ws = row_splits, item_ids, scores, index, ws
        self.certified, self.n_survivors, self.cap, self.capacity, self._total = certified, n_survivors, cap, capacity, total

    @property
    def total(self):
        if self._total is None:
            self._total = int(self.row_splits[-1].item())
        return self._total

    @property
    def truncated(self):
        return self.total > self.capacity


def search_all_range_sq8_exact(index, sq8, bounds, scorer, q, thresholds, cap=4096, capacity=None, fallback=True, options=None,
                               sort=False):
    """Certified scalar-quantised range search (nann_search_all_range_sq8_exact): search_all_range's result BIT FOR BIT -- rows
    in ascending row order, score bits, item ids, counts -- from the int8 scan.  The threshold is the cut: per query every row
    whose exact score a rigorous error bound cannot put below thresholds[b] survives, the survivors alone are scored exactly,
    and those at or above the threshold are returned -> Sq8RangeResult.  result.certified[b] == 1 iff at most min(cap, n_items)
    rows survived and the threshold and the query are finite; an uncertified query's segment is EMPTY.  Under an l2 scorer a
    finite threshold above 0 is certified with an empty segment (no l2 score exceeds 0).  `scorer`: an l2 or ip ops.Scorer with
    q f32[B, d]; sq8: make_sq8(index); bounds: make_sq8_bounds(index, sq8).  There is no filter.
    cap=4096 is a convenience default, NOT a tuned value: the workspace holds 8 bytes per (query of a chunk, cap position), and
    the survivors outnumber the matches by a factor that depends on the corpus (tools/sq8_range_rate.py measures it).
    capacity=None means B * min(cap, n_items): that size cannot truncate a certified result, so there is ONE call, the index is
    scored once and nothing synchronises -- what search_all_range's count-then-fill cannot offer.
    fallback=True: the wrapper reads `certified` back -- ONE synchronisation -- runs the uncertified queries through
    search_all_range and splices their segments in, in query order, so that the result equals search_all_range's for EVERY query
    (certified and n_survivors stay as the device call left them).  fallback=False: asynchronous on torch's current stream.
    sort=True reorders each segment by (score descending, row ascending) with torch on the device."""
    dev = index.device
    q = q.to(device=dev, dtype=torch.float32).contiguous()
    b, cap = q.shape[0], int(cap)
    if isinstance(thresholds, (int, float)):
        thr = torch.full((b,), float(thresholds), dtype=torch.float32, device=dev)
    else:
        thr = torch.as_tensor(thresholds).to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        assert thr.numel() == b, "thresholds: one per query of the batch"
    fit = capacity is None  # (the fallback then sizes the spliced result to its total)
    capacity = b * max(min(cap, int(index.n_items)), 0) if fit else int(capacity)
    assert capacity >= 0, "capacity >= 0"
    L = lib()
    nbytes = C.c_int64(0)
    bh = bounds.handle if bounds is not None else None
    th = sq8.handle if sq8 is not None else None
    _check(L.nann_search_all_range_sq8_exact_workspace_bytes(index.handle, th, bh, scorer.handle, b, cap, C.byref(nbytes)),
           "search_all_range_sq8_exact")
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    splits = torch.zeros(b + 1, dtype=torch.int64, device=dev)
    ids = torch.zeros(capacity, dtype=torch.int64, device=dev)
    scores = torch.zeros(capacity, dtype=torch.float32, device=dev)
    rows = torch.zeros(capacity, dtype=torch.int32, device=dev)
    certified = torch.zeros(b, dtype=torch.int32, device=dev)
    n_surv = torch.zeros(b, dtype=torch.int32, device=dev)
    some = capacity > 0
    with torch.cuda.device(dev):
        _check(L.nann_search_all_range_sq8_exact(index.handle, th, bh, scorer.handle, _ptr(q), b, _ptr(thr), cap, capacity,
                                                 _ptr(splits), _ptr(ids) if some else None, _ptr(scores) if some else None,
                                                 _ptr(rows) if some else None, _ptr(certified), _ptr(n_surv), _ptr(ws), ws.numel(),
                                                 C.byref(options) if options is not None else None, _stream()),
               "search_all_range_sq8_exact")
    total = None
    if fallback and b > 0:
        todo = torch.nonzero(certified == 0).flatten()  # (the synchronisation)
        if todo.numel() > 0:
            splits, ids, scores, rows = _range_splice(splits, ids, scores, rows, None if fit else capacity, todo,
                                                      search_all_range(index, scorer, q[todo], thr[todo], options=options))
            capacity = ids.numel()
        total = int(splits[b].item())
    if sort and b > 0:
        _range_sort(splits, ids, scores, rows, min(int(splits[b].item()) if total is None else total, capacity))
    return Sq8RangeResult(splits, ids, scores, rows, certified, n_surv, cap, capacity, total if b else 0, ws)


def _range_splice(splits, ids, scores, rows, capacity, todo, other):
    """A ragged result whose segments of the queries `todo` are empty, with the segments of `other` -- a full (untruncated) ragged
    result over exactly those queries -- put in their places, in query order; the entries are the head [0, capacity) of the whole
    (capacity=None: the whole)."""
    dev, b = splits.device, splits.numel() - 1
    counts = splits[1:] - splits[:-1]
    o_begin = torch.zeros(b, dtype=torch.int64, device=dev)
    o_begin[todo] = other.row_splits[:-1]
    counts[todo] = other.row_splits[1:] - other.row_splits[:-1]
    from_other = torch.zeros(b, dtype=torch.bool, device=dev)
    from_other[todo] = True
    new_splits = torch.zeros(b + 1, dtype=torch.int64, device=dev)
    new_splits[1:] = torch.cumsum(counts, 0)
    n = int(new_splits[b].item())
    if capacity is None:
        capacity = n
    n = min(n, capacity)
    seg = torch.searchsorted(new_splits[1:].contiguous(), torch.arange(n, device=dev), right=True)  # the query of every entry
    off = torch.arange(n, device=dev) - new_splits[seg]
    # an entry of a certified query lay at or in front of its new place: inside the head the first call has filled
    src = torch.where(from_other[seg], ids.numel() + o_begin[seg] + off, splits[seg] + off)
    out = []
    for mine, theirs in ((ids, other.item_ids), (scores, other.scores), (rows, other.index)):
        fresh = torch.zeros(capacity, dtype=mine.dtype, device=dev)
        fresh[:n] = torch.cat([mine, theirs])[src]
        out.append(fresh)
    return [new_splits] + out


# candidates per work item of the scoring kernels of search_candidates (csrc/nann_cand.h: kCandRows, kCandMlpRows)
CANDIDATE_BLOCK_ROWS = 1024
CANDIDATE_MLP_BLOCK_ROWS = 4096
CANDIDATE_ATTN_BLOCK_ROWS = 256  # search_candidates_model under the attention model (kCandAttnRows)


class CandidateResult:
    """Outputs of search_candidates (device tensors): per query the top min(k, len) of its own list, TopKV2 order, ties to
    the lower position in the list -- n_out[b] valid entries at the head of row b of item_ids / scores / index (internal rows) /
    pos (positions within the query's list) and zeros behind.  status[b]: 0, 3 (the query's range in row_splits is ill-formed)
    or 5 (it lists a row outside the index); such a query has n_out[b] = 0."""
    __slots__ = ("item_ids", "scores", "index", "pos", "n_out", "status", "_ws", "_lists")

    def __init__(self, item_ids, scores, index, pos, n_out, status, ws=None, lists=None):
        self.item_ids, self.scores, self.index, self.pos, self.n_out, self.status = item_ids, scores, index, pos, n_out, status
        self._ws, self._lists = ws, lists


def _rows_of_item_ids_kept(index, ids):
    """_rows_of_item_ids with every position kept: the row of each item id, -1 for an unknown one"""
    vals, perm = _sorted_item_ids(index)
    ids = _i64(ids).to(vals.device)
    if vals.numel() == 0 or ids.numel() == 0:
        return torch.full_like(ids, -1)
    pos = torch.searchsorted(vals, ids).clamp_(max=vals.numel() - 1)
    return torch.where(vals[pos] == ids, perm[pos], torch.full_like(ids, -1))


def _candidate_lists(index, candidates, candidate_item_ids):
    """(row_splits i64[B + 1], rows i32[n_cand]) on the index's device"""
    dev = index.device
    given = candidates if candidates is not None else candidate_item_ids
    if isinstance(given, tuple) and len(given) == 2 and all(isinstance(t, torch.Tensor) for t in given):
        splits, flat = given[0].to(torch.int64), given[1].reshape(-1)
    else:
        per = [_i64(p) for p in given]
        splits = torch.cumsum(torch.tensor([0] + [int(p.numel()) for p in per], dtype=torch.int64), 0)
        flat = torch.cat(per) if per else torch.zeros(0, dtype=torch.int64)
    if candidates is None:
        flat = _rows_of_item_ids_kept(index, flat)
    elif flat.dtype != torch.int32:
        assert flat.numel() == 0 or (int(flat.min()) >= -(1 << 31) and int(flat.max()) < (1 << 31)), "row numbers are 32-bit"
    return splits.to(dev).contiguous(), flat.to(device=dev, dtype=torch.int32).contiguous()


def search_candidates(index, scorer, q, candidates=None, candidate_item_ids=None, k=200, options=None):
    """Candidate-list search (nann_search_candidates): query b brings a list of rows of its own, the rows are scored and the
    best min(k, len) returned -- descending, ties -> lower position in the list; a row listed twice is scored and may be
    returned twice -> CandidateResult.  The cost grows with the lists, not with the index.
    candidates: one 1-D integer array of internal row numbers per query, or a (row_splits i64[B + 1], rows) pair of tensors;
    candidate_item_ids: the same in item ids (exactly one of the two), mapped through the sorted copy of index.item_ids that
    make_filter uses -- an unknown id becomes row -1 and fails its query alone (status 5).
    `scorer`: ops.Scorer with q f32[B, d], or an ops.Model of kind l2 / mlp with q = comm_seq f16[B, seq_len, d]; an attention
    model raises NotImplementedError here (search_candidates_model serves every kind of model).  options: search_options(preprojection=...).  An MLP scorer reads its pre-projected
    table, as in search_all.  Asynchronous on torch's current stream."""
    assert (candidates is None) != (candidate_item_ids is None), "candidates or candidate_item_ids, one of the two"
    dev = index.device
    handle = scorer.handle
    if isinstance(scorer, ops.Model):
        if scorer.kind == "attention":
            raise NotImplementedError("search_candidates: l2 / mlp scorers only")
        q = ops.user_seq_mean(q.to(dev))
        handle = C.c_void_p(lib().nann_model_scorer(scorer.handle))  # (borrowed: the model owns it)
    q = q.to(device=dev, dtype=torch.float32).contiguous()
    return _flat_candidates(index, handle, q, candidates, candidate_item_ids, k, options, "nann_search_candidates",
                            "search_candidates", "query", ())


def _flat_candidates(index, handle, x, candidates, candidate_item_ids, k, options, symbol, what, unit, keep):
    """The candidate family's call: `symbol` for the b rows of x (queries or sequences, as _flat_all takes them) and their
    lists, as nann_candidates.  The result keeps the lists' tensors alive, and `keep` with them."""
    dev = index.device
    b, k = x.shape[0], int(k)
    splits, rows = _candidate_lists(index, candidates, candidate_item_ids)
    assert splits.numel() == b + 1, "one candidate list per %s of the batch" % unit
    cand = _lib.Candidates()
    cand.struct_bytes = C.sizeof(_lib.Candidates)
    cand.row_splits = splits.data_ptr()
    cand.rows = rows.data_ptr() if rows.numel() else None
    cand.n_cand = int(rows.numel())
    kk = max(k, 0)
    out_ids = torch.zeros((b, kk), dtype=torch.int64, device=dev)
    out_scores = torch.zeros((b, kk), dtype=torch.float32, device=dev)
    out_index = torch.zeros((b, kk), dtype=torch.int32, device=dev)
    out_pos = torch.zeros((b, kk), dtype=torch.int32, device=dev)
    n_out = torch.zeros(b, dtype=torch.int32, device=dev)
    status = torch.zeros(b, dtype=torch.int32, device=dev)
    nbytes = C.c_int64(0)
    _check(getattr(lib(), symbol + "_workspace_bytes")(index.handle, handle, b, cand.n_cand, k, C.byref(nbytes)), what)
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(getattr(lib(), symbol)(index.handle, handle, _ptr(x), b, k, C.byref(cand), _ptr(out_ids), _ptr(out_scores),
                                      _ptr(out_index), _ptr(out_pos), _ptr(n_out), _ptr(status), _ptr(ws), ws.numel(),
                                      C.byref(options) if options is not None else None, _stream()), what)
    return CandidateResult(out_ids, out_scores, out_index, out_pos, n_out, status, ws, (splits, rows) + tuple(keep))


def search_candidates_model(index, model, comm_seq, candidates=None, candidate_item_ids=None, k=200, options=None):
    """Candidate-list search under a model (nann_search_candidates_model): search_candidates for the users of comm_seq
    f16[B, seq_len, E] -- user b brings a list of rows of its own, the rows are scored by `model` and the best min(k, len)
    returned, descending, ties -> lower position in the list, no dedup -> CandidateResult.  candidates / candidate_item_ids: as
    search_candidates takes them (exactly one of the two).  `model`: an ops.Model of any kind (l2 / mlp: the bits of
    search_candidates(index, model, comm_seq, ...); attention: scored on the device from the model's pre-projected table, both
    precisions bit-identical to search_all_model's score of the same (user, row)); an ops.Scorer raises TypeError
    (search_candidates takes those).  options: search_options(preprojection=...).  Asynchronous on torch's current stream.  An
    attention or MLP model reads its pre-projected table; without one the call raises ops.NannError with status 103 (no room
    in HBM) or 102 (pre-projection switched off).  The workspace holds the keys of at most 128 users at a time, however many
    the batch has."""
    if not isinstance(model, ops.Model):
        raise TypeError("search_candidates_model: an ops.Model (an ops.Scorer goes through search_candidates)")
    assert (candidates is None) != (candidate_item_ids is None), "candidates or candidate_item_ids, one of the two"
    seq = comm_seq.to(device=index.device, dtype=torch.float16).contiguous()
    return _flat_candidates(index, model.handle, seq, candidates, candidate_item_ids, k, options, "nann_search_candidates_model",
                            "search_candidates_model", "user", (seq,))


UNION_MAX_IN = _lib.UNION_MAX_IN  # most entries (n_lists * k_in, n_vec * F, n_vec * k) a user brings to a union


class MultiResult:
    """Outputs of union_topk / search_multi / search_all_multi, [n_users, k] device tensors: the k best DISTINCT rows of a user
    by the best score any of its lists (interest vectors) gives a row, n_out[u] valid entries at the head of row u and zeros
    behind.  vec: the list (vector) an entry came from.  status: i32[n_users, n_vec], what the inner search of search_multi
    reported per vector (None elsewhere); plan: its planner's choice (None elsewhere).  item_ids is None for a union_topk
    without an index."""
    __slots__ = ("item_ids", "scores", "index", "vec", "n_out", "status", "plan", "_ws")

    def __init__(self, item_ids, scores, index, vec, n_out, status=None, plan=None, ws=None):
        self.item_ids, self.scores, self.index, self.vec, self.n_out = item_ids, scores, index, vec, n_out
        self.status, self.plan, self._ws = status, plan, ws


def _multi_outputs(n_users, k, dev, item_ids=True):
    kk = max(int(k), 0)
    return (torch.zeros((n_users, kk), dtype=torch.int64, device=dev) if item_ids else None,
            torch.zeros((n_users, kk), dtype=torch.float32, device=dev), torch.zeros((n_users, kk), dtype=torch.int32, device=dev),
            torch.zeros((n_users, kk), dtype=torch.int32, device=dev), torch.zeros(n_users, dtype=torch.int32, device=dev))


def union_topk(scores, rows, k, n_valid=None, index=None):
    """Union top-k (nann_union_topk): scores f32 / rows i32 [n_users, n_lists, k_in] CUDA tensors, a user's n_lists result
    lists from anywhere; only the first n_valid[u][l] (i32[n_users, n_lists]; None: k_in) entries of a list count, and rows
    outside [0, index.n_items) -- without an index: negative rows -- are dropped.  Per row the entry with the largest score
    represents it (ties -> the lower position l * k_in + j), and the k best representatives are returned, descending, ties ->
    the lower position -> MultiResult (item_ids only with an index).  n_lists * k_in <= UNION_MAX_IN, k <= 1024.
    Asynchronous on torch's current stream."""
    dev = scores.device
    scores = scores.to(dtype=torch.float32).contiguous()
    rows = rows.to(device=dev, dtype=torch.int32).contiguous()
    assert scores.dim() == 3 and rows.shape == scores.shape, "scores, rows: [n_users, n_lists, k_in]"
    n_users, n_lists, k_in = scores.shape
    if n_valid is not None:
        n_valid = n_valid.to(device=dev, dtype=torch.int32).contiguous()
        assert n_valid.shape == (n_users, n_lists), "n_valid: [n_users, n_lists]"
    k = int(k)
    out_ids, out_scores, out_index, out_list, n_out = _multi_outputs(n_users, k, dev, index is not None)
    nbytes = C.c_int64(0)
    _check(lib().nann_union_topk_workspace_bytes(n_users, n_lists, k_in, C.byref(nbytes)), "union_topk")
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    n_items = int(index.n_items) if index is not None else (1 << 31) - 1
    with torch.cuda.device(dev):
        _check(lib().nann_union_topk(_ptr(scores), _ptr(rows), _ptr(n_valid), n_users, n_lists, k_in, n_items,
                                     _ptr(index.item_ids) if index is not None else None, k, _ptr(out_index), _ptr(out_scores),
                                     _ptr(out_ids), _ptr(out_list), _ptr(n_out), _ptr(ws), ws.numel(), _stream()), "union_topk")
    return MultiResult(out_ids, out_scores, out_index, out_list, n_out, ws=ws)


def search_multi(index, scorer, q, level_topn, k=None, options=None):
    """Multi-vector traversal (nann_search_multi): q f32[n_users, n_vec, d], n_vec interest vectors per user.  search() runs
    unchanged over the n_users * n_vec vectors at the fetch width F = level_topn[5] (level_topn: i32[6], or [n_users * n_vec,
    6] per vector), then each user's n_vec lists are united: the k (default F) best distinct rows by the best score any vector
    gives a row -> MultiResult; result.vec names the vector, result.status [n_users, n_vec] what the inner search reported -- a
    failed vector contributes nothing.  A user with fewer interests repeats one of them.  `scorer`: an ops.Scorer of any kind
    search() takes.  n_vec * F <= UNION_MAX_IN, k <= 1024.  Asynchronous on torch's current stream."""
    dev = index.device
    q = q.to(device=dev, dtype=torch.float32).contiguous()
    assert q.dim() == 3, "q: [n_users, n_vec, d]"
    n_users, n_vec = int(q.shape[0]), int(q.shape[1])
    t, tq, k_fetch = _level_topn_args(level_topn, n_users * n_vec, dev)
    k = int(k) if k is not None else k_fetch
    out_ids, out_scores, out_index, out_vec, n_out = _multi_outputs(n_users, k, dev)
    status = torch.zeros((n_users, n_vec), dtype=torch.int32, device=dev)
    nbytes = C.c_int64(0)
    _check(lib().nann_search_multi_workspace_bytes(index.handle, t, n_users, n_vec, C.byref(nbytes)), "search_multi")
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    plan = _lib.SearchPlan()
    with torch.cuda.device(dev):
        _check(lib().nann_search_multi(index.handle, scorer.handle, _ptr(q), n_users, n_vec, t, _ptr(tq), _ptr(ws), ws.numel(),
                                       _ptr(out_ids), _ptr(out_scores), _ptr(out_index), _ptr(out_vec), _ptr(n_out), _ptr(status),
                                       None, C.byref(options) if options is not None else None, C.byref(plan), k, _stream()),
               "search_multi")
    return MultiResult(out_ids, out_scores, out_index, out_vec, n_out, status, _plan_dict(plan), ws)


def search_all_multi(index, scorer, q, k, options=None):
    """Exhaustive multi-vector search (nann_search_all_multi), the ground truth of search_multi: search_all over the n_users *
    n_vec vectors of q f32[n_users, n_vec, d] at k, then the union per user -> MultiResult.  Its scores are exactly the k
    largest of max over the user's vectors of a row's score.  `scorer`: an ops.Scorer.  n_vec * k <= UNION_MAX_IN.
    Asynchronous on torch's current stream."""
    dev = index.device
    q = q.to(device=dev, dtype=torch.float32).contiguous()
    assert q.dim() == 3, "q: [n_users, n_vec, d]"
    n_users, n_vec, k = int(q.shape[0]), int(q.shape[1]), int(k)
    out_ids, out_scores, out_index, out_vec, n_out = _multi_outputs(n_users, k, dev)
    nbytes = C.c_int64(0)
    _check(lib().nann_search_all_multi_workspace_bytes(index.handle, scorer.handle, n_users, n_vec, k, C.byref(nbytes)),
           "search_all_multi")
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(lib().nann_search_all_multi(index.handle, scorer.handle, _ptr(q), n_users, n_vec, k, _ptr(out_ids), _ptr(out_scores),
                                           _ptr(out_index), _ptr(out_vec), _ptr(n_out), _ptr(ws), ws.numel(),
                                           C.byref(options) if options is not None else None, _stream()), "search_all_multi")
    return MultiResult(out_ids, out_scores, out_index, out_vec, n_out, ws=ws)


FUSE_MAX_LISTS = _lib.FUSE_MAX_LISTS  # most lists (vectors) a user brings to a fuse
FUSION_MODES = {"sum": _lib.FUSE_SUM, "sum_floor": _lib.FUSE_SUM_FLOOR, "minmax": _lib.FUSE_MINMAX, "rrf": _lib.FUSE_RRF}


class Fusion:
    """How fuse_topk and the _fused searches turn a row's entries in several lists into one score (make_fusion).  mode: a
    key of FUSION_MODES; weights: None, f32[n_lists] (per call) or f32[n_users, n_lists] (per user), moved to the device of
    the call when it is made; rrf_c: the constant of reciprocal rank fusion."""
    __slots__ = ("mode", "weights", "rrf_c")

    def __init__(self, mode, weights, rrf_c):
        self.mode, self.weights, self.rrf_c = mode, weights, rrf_c


def make_fusion(mode="rrf", weights=None, rrf_c=60.0):
    """A Fusion.  mode: "rrf" (a list adds w / (rrf_c + rank), rank from 1), "sum" (w * score), "sum_floor" (w * (score - the
    list's least score): what makes negative L2 scores addable) or "minmax" (w * the score's place between the list's least
    and greatest score, in [0, 1]).  weights: None (1.0), 1-D [n_lists] for a per-call weight or 2-D [n_users, n_lists] for a
    per-user weight -- a tensor, an array or a sequence; used as given, negative and zero weights included."""
    assert mode in FUSION_MODES, "mode: one of %s" % sorted(FUSION_MODES)
    rrf_c = float(rrf_c)
    assert 0.0 <= rrf_c < math.inf, "rrf_c: a finite value >= 0"
    if weights is not None:
        weights = torch.as_tensor(weights).to(dtype=torch.float32)
        assert weights.dim() in (1, 2), "weights: [n_lists] or [n_users, n_lists]"
    return Fusion(mode, weights, rrf_c)


def _fusion_args(fusion, n_users, n_lists, dev):
    """-> (the nann_fusion struct, what it borrows)"""
    w = fusion.weights
    if w is not None:
        w = w.to(device=dev, dtype=torch.float32).contiguous()
        assert tuple(w.shape) in ((n_lists,), (n_users, n_lists)), "weights: [n_lists] or [n_users, n_lists]"
    f = _lib.Fusion(C.sizeof(_lib.Fusion), FUSION_MODES[fusion.mode], fusion.rrf_c, int(w is not None and w.dim() == 2),
                    w.data_ptr() if w is not None and w.numel() else None)
    return f, w


class FusedResult:
    """Outputs of fuse_topk / fuse_results / search_multi_fused / search_all_multi_fused, [n_users, k] device tensors: the k
    best DISTINCT rows of a user by the score accumulated over the lists that contain a row, n_out[u] valid entries at the head
    of row u and zeros behind.  lists: int64, the u64 mask of the lists that contain the row (bit l = list l; bit 63 is the
    sign).  status: i32[n_users, n_vec], what the inner search of search_multi_fused reported per vector (None elsewhere);
    plan: its planner's choice (None elsewhere).  item_ids is None for a fuse_topk without an index."""
    __slots__ = ("item_ids", "scores", "index", "lists", "n_out", "status", "plan", "_ws")

    def __init__(self, item_ids, scores, index, lists, n_out, status=None, plan=None, ws=None):
        self.item_ids, self.scores, self.index, self.lists, self.n_out = item_ids, scores, index, lists, n_out
        self.status, self.plan, self._ws = status, plan, ws


def _fused_outputs(n_users, k, dev, item_ids=True):
    kk = max(int(k), 0)
    return (torch.zeros((n_users, kk), dtype=torch.int64, device=dev) if item_ids else None,
            torch.zeros((n_users, kk), dtype=torch.float32, device=dev), torch.zeros((n_users, kk), dtype=torch.int32, device=dev),
            torch.zeros((n_users, kk), dtype=torch.int64, device=dev), torch.zeros(n_users, dtype=torch.int32, device=dev))


def fuse_topk(scores, rows, fusion, k, n_valid=None, index=None):
    """Fused top-k (nann_fuse_topk): scores f32 / rows i32 [n_users, n_lists, k_in] CUDA tensors, a user's n_lists result lists
    from anywhere, on any scales; only the first n_valid[u][l] (i32[n_users, n_lists]; None: k_in) entries of a list count, and
    rows outside [0, index.n_items) -- without an index: negative rows -- are dropped.  Within a list a row counts once, at its
    first entry; every list that contains a row adds one term to the row's score (make_fusion), in list order, and the k rows
    with the largest sums are returned, descending, ties -> the row that appears first -> FusedResult (item_ids only with an
    index).  n_lists <= FUSE_MAX_LISTS, n_lists * k_in <= UNION_MAX_IN, k <= 1024.  Asynchronous on torch's current stream."""
    dev = scores.device
    scores = scores.to(dtype=torch.float32).contiguous()
    rows = rows.to(device=dev, dtype=torch.int32).contiguous()
    assert scores.dim() == 3 and rows.shape == scores.shape, "scores, rows: [n_users, n_lists, k_in]"
    n_users, n_lists, k_in = scores.shape
    if n_valid is not None:
        n_valid = n_valid.to(device=dev, dtype=torch.int32).contiguous()
        assert n_valid.shape == (n_users, n_lists), "n_valid: [n_users, n_lists]"
    k = int(k)
    f, _borrowed = _fusion_args(fusion, n_users, n_lists, dev)
    out_ids, out_scores, out_index, out_lists, n_out = _fused_outputs(n_users, k, dev, index is not None)
    nbytes = C.c_int64(0)
    _check(lib().nann_fuse_topk_workspace_bytes(n_users, n_lists, k_in, C.byref(nbytes)), "fuse_topk")
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    n_items = int(index.n_items) if index is not None else (1 << 31) - 1
    with torch.cuda.device(dev):
        _check(lib().nann_fuse_topk(_ptr(scores), _ptr(rows), _ptr(n_valid), n_users, n_lists, k_in, n_items,
                                    _ptr(index.item_ids) if index is not None else None, k, C.byref(f), _ptr(out_index),
                                    _ptr(out_scores), _ptr(out_ids), _ptr(out_lists), _ptr(n_out), _ptr(ws), ws.numel(), _stream()),
               "fuse_topk")
    return FusedResult(out_ids, out_scores, out_index, out_lists, n_out, ws=ws)


def _stack_results(results):
    """the index / scores of result objects [n_users, k_i], padded to the widest -> (scores f32, rows i32) [n_users, n_results,
    k_max] and n_valid i32[n_users, n_results]: a result's n_out, or its width where it has none"""
    assert len(results) > 0, "results: at least one"
    n_users = int(results[0].index.shape[0])
    dev = results[0].index.device
    width = max(int(r.index.shape[1]) for r in results)
    scores = torch.zeros((n_users, len(results), width), dtype=torch.float32, device=dev)
    rows = torch.zeros((n_users, len(results), width), dtype=torch.int32, device=dev)
    n_valid = torch.zeros((n_users, len(results)), dtype=torch.int32, device=dev)
    for l, r in enumerate(results):
        assert r.index.dim() == 2 and r.index.shape == r.scores.shape and int(r.index.shape[0]) == n_users, \
            "results: index and scores [n_users, k] of one batch"
        w = int(r.index.shape[1])
        scores[:, l, :w] = r.scores.to(device=dev, dtype=torch.float32)
        rows[:, l, :w] = r.index.to(device=dev, dtype=torch.int32)
        n_out = getattr(r, "n_out", None)
        n_valid[:, l] = n_out.to(device=dev, dtype=torch.int32) if n_out is not None else w
    return scores, rows, n_valid


def fuse_results(results, fusion, k, index):
    """Hybrid retrieval: fuse what several searches of ONE batch returned -- a Python list of result objects of any search here
    (SearchResult, SearchAllResult, CandidateResult, MultiResult, ...), list l = results[l].  Their index / scores are padded
    to the widest, a result's n_out (its width where it has none) says how many of its entries count, and fuse_topk does the
    rest -> FusedResult; bit l of result.lists = results[l] holds the row."""
    scores, rows, n_valid = _stack_results(results)
    return fuse_topk(scores, rows, fusion, k, n_valid=n_valid, index=index)


def search_multi_fused(index, scorer, q, level_topn, fusion, k=None, options=None):
    """search_multi with the fuse in the place of the union (nann_search_multi_fused): q f32[n_users, n_vec, d]; search() runs
    unchanged over the n_users * n_vec vectors at the fetch width F = level_topn[5], then each user's n_vec lists are fused
    (make_fusion): the k (default F) rows with the largest accumulated score -> FusedResult; result.lists names the vectors whose
    list holds the row, result.status [n_users, n_vec] what the inner search reported -- a failed vector contributes nothing.
    A row beyond depth F in a vector's list loses that vector's term: F is the caller's trade-off.  n_vec <= FUSE_MAX_LISTS,
    n_vec * F <= UNION_MAX_IN, k <= 1024.  Asynchronous on torch's current stream."""
    dev = index.device
    q = q.to(device=dev, dtype=torch.float32).contiguous()
    assert q.dim() == 3, "q: [n_users, n_vec, d]"
    n_users, n_vec = int(q.shape[0]), int(q.shape[1])
    t, tq, k_fetch = _level_topn_args(level_topn, n_users * n_vec, dev)
    k = int(k) if k is not None else k_fetch
    f, _borrowed = _fusion_args(fusion, n_users, n_vec, dev)
    out_ids, out_scores, out_index, out_lists, n_out = _fused_outputs(n_users, k, dev)
    status = torch.zeros((n_users, n_vec), dtype=torch.int32, device=dev)
    nbytes = C.c_int64(0)
    _check(lib().nann_search_multi_fused_workspace_bytes(index.handle, t, n_users, n_vec, C.byref(nbytes)), "search_multi_fused")
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    plan = _lib.SearchPlan()
    with torch.cuda.device(dev):
        _check(lib().nann_search_multi_fused(index.handle, scorer.handle, _ptr(q), n_users, n_vec, t, _ptr(tq), _ptr(ws), ws.numel(),
                                             _ptr(out_ids), _ptr(out_scores), _ptr(out_index), _ptr(out_lists), _ptr(n_out),
                                             _ptr(status), None, C.byref(options) if options is not None else None, C.byref(plan),
                                             k, C.byref(f), _stream()), "search_multi_fused")
    return FusedResult(out_ids, out_scores, out_index, out_lists, n_out, status, _plan_dict(plan), ws)


def search_all_multi_fused(index, scorer, q, k, fusion, fetch=None, options=None):
    """Exhaustive multi-vector search, fused (nann_search_all_multi_fused): search_all over the n_users * n_vec vectors of q
    f32[n_users, n_vec, d] at `fetch` (default k), the per-vector depth, then the fuse per user at k -> FusedResult.  Unlike the
    union's, this answer depends on the depth: a row beyond `fetch` in a vector's list loses that vector's term.  n_vec <=
    FUSE_MAX_LISTS, n_vec * fetch <= UNION_MAX_IN.  Asynchronous on torch's current stream."""
    dev = index.device
    q = q.to(device=dev, dtype=torch.float32).contiguous()
    assert q.dim() == 3, "q: [n_users, n_vec, d]"
    n_users, n_vec, k = int(q.shape[0]), int(q.shape[1]), int(k)
    fetch = int(fetch) if fetch is not None else k
    f, _borrowed = _fusion_args(fusion, n_users, n_vec, dev)
    out_ids, out_scores, out_index, out_lists, n_out = _fused_outputs(n_users, k, dev)
    nbytes = C.c_int64(0)
    _check(lib().nann_search_all_multi_fused_workspace_bytes(index.handle, scorer.handle, n_users, n_vec, fetch, C.byref(nbytes)),
           "search_all_multi_fused")
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(lib().nann_search_all_multi_fused(index.handle, scorer.handle, _ptr(q), n_users, n_vec, fetch, k, C.byref(f),
                                                 _ptr(out_ids), _ptr(out_scores), _ptr(out_index), _ptr(out_lists), _ptr(n_out),
                                                 _ptr(ws), ws.numel(), C.byref(options) if options is not None else None,
                                                 _stream()), "search_all_multi_fused")
    return FusedResult(out_ids, out_scores, out_index, out_lists, n_out, ws=ws)


class Interests:
    """What ops.user_seq_interests made of a batch of behaviour sequences (search_seq_multi / search_all_seq_multi return it
    next to their result): q f32[n_users, n_vec, d], the interest vectors the search ran on; weights f32[n_users, n_vec], each
    vector's share of the user's non-pad history rows; n_interests i32[n_users], how many of the n_vec slots are distinct
    interests (the others repeat slot 0 with weight 0)."""
    __slots__ = ("q", "weights", "n_interests")

    def __init__(self, q, weights, n_interests):
        self.q, self.weights, self.n_interests = q, weights, n_interests


def _seq_interests(index, comm_seq, n_vec, n_iter, fusion):
    """-> (Interests, the fusion to run: one that brings no weights gets the interests' as its per-user weights)"""
    q, w, n = ops.user_seq_interests(torch.as_tensor(comm_seq).to(index.device), n_vec, n_iter=n_iter)
    if fusion is not None and fusion.weights is None:
        fusion = Fusion(fusion.mode, w, fusion.rrf_c)
    return Interests(q, w, n), fusion


def search_seq_multi(index, scorer, comm_seq, n_vec, level_topn, k=None, fusion=None, n_iter=8, options=None):
    """Multi-vector traversal from a behaviour sequence: comm_seq f16[n_users, L, d] -> ops.user_seq_interests (at most n_vec
    interest vectors per user, n_iter Lloyd rounds), then search_multi over them -> (MultiResult, Interests).  With a Fusion
    (make_fusion) search_multi_fused runs in the union's place -> (FusedResult, Interests); a Fusion whose weights is None gets
    the interests' weights as its per-user weights, one that brings weights keeps them.  A composition in Python: two
    calls on torch's current stream, no host read-back between them."""
    interests, fusion = _seq_interests(index, comm_seq, n_vec, n_iter, fusion)
    if fusion is None:
        return search_multi(index, scorer, interests.q, level_topn, k=k, options=options), interests
    return search_multi_fused(index, scorer, interests.q, level_topn, fusion, k=k, options=options), interests


def search_all_seq_multi(index, scorer, comm_seq, n_vec, k, fusion=None, fetch=None, n_iter=8, options=None):
    """search_seq_multi over the exhaustive forms, its ground truth: ops.user_seq_interests, then search_all_multi at k ->
    (MultiResult, Interests), or with a Fusion search_all_multi_fused at (k, fetch) -> (FusedResult, Interests); the Fusion's
    weights as in search_seq_multi."""
    interests, fusion = _seq_interests(index, comm_seq, n_vec, n_iter, fusion)
    if fusion is None:
        return search_all_multi(index, scorer, interests.q, k, options=options), interests
    return search_all_multi_fused(index, scorer, interests.q, k, fusion, fetch=fetch, options=options), interests


class Groups:
    """What make_groups returns: the tensors of a nann_groups (they may live on the CPU: testable without a GPU) and its
    ctypes struct, which borrows their memory.
      group_of_row  i32[n_items]: the group id of every internal row; < 0 = ungrouped (never capped, counts against nothing)
      cap           at most this many rows of one group among a query's answer (>= 1), for every query when caps is None
      caps          i32[n_queries] or None: one cap per query; <= 0: the query is uncapped"""
    __slots__ = ("group_of_row", "cap", "caps", "n_queries", "n_items", "device", "struct")

    def __init__(self, group_of_row, cap, caps, n_items, device):
        self.group_of_row, self.cap, self.caps, self.n_items, self.device = group_of_row, int(cap), caps, n_items, device
        self.n_queries = None if caps is None else int(caps.numel())
        st = _lib.Groups()
        st.struct_bytes = C.sizeof(_lib.Groups)
        st.group_of_row = group_of_row.data_ptr()
        st.cap = int(cap)
        st.caps = caps.data_ptr() if caps is not None else None
        self.struct = st


def make_groups(index, group_of_row=None, group_of_item_id=None, cap=1, caps=None, device=None):
    """A nann_groups for capped searches on `index`: at most `cap` rows of one group in a query's answer.  group_of_row: the
    group id of every internal row, [n_items] (negative: ungrouped); or group_of_item_id = (item_ids, groups), two 1-D arrays
    of one length, mapped through index.item_ids -- an unknown id names nothing, an item that is not named is ungrouped.
    caps: one cap per query of the batch the groups will be used with (<= 0: that query is uncapped) in the place of `cap`.
    device: where the tensors live (default: the index's; "cpu" builds them without a GPU).  -> Groups."""
    dev = torch.device(device if device is not None else index.device)
    n = int(index.n_items)
    assert (group_of_row is None) != (group_of_item_id is None), "one of group_of_row and group_of_item_id"
    if group_of_row is not None:
        g = _i64(group_of_row)
        assert g.numel() == n, "group_of_row: one group id per row of the index"
    else:
        ids, grp = _i64(group_of_item_id[0]), _i64(group_of_item_id[1])
        assert ids.numel() == grp.numel(), "group_of_item_id: (item_ids, groups) of one length"
        g = torch.full((n,), -1, dtype=torch.int64)
        vals, perm = _sorted_item_ids(index)
        if vals.numel() and ids.numel():
            pos = torch.searchsorted(vals, ids.to(vals.device)).clamp_(max=vals.numel() - 1)
            found = (vals[pos] == ids.to(vals.device)).cpu()
            g[perm[pos].cpu()[found]] = grp[found]
    assert g.numel() == 0 or (int(g.min()) >= -(1 << 31) and int(g.max()) < (1 << 31)), "group ids are 32-bit"
    assert caps is not None or int(cap) >= 1, "cap >= 1"
    if caps is not None:
        caps = _i64(caps).clamp(min=-(1 << 31), max=(1 << 31) - 1).to(torch.int32).to(dev).contiguous()
    return Groups(g.to(torch.int32).to(dev).contiguous(), cap, caps, n, dev)


class GroupedResult:
    """Outputs of cap_groups / search_grouped / search_model_grouped / search_all_grouped / search_all_model_grouped, [B, k]
    device tensors: the first k entries of a ranked list that keep to the cap, n_out[b] of them at the head of row b and zeros
    behind.  group: the group id of each returned row.  pos (cap_groups only): the entry's position in the input list.  status,
    counters, plan: the inner search's (the traversal forms; None elsewhere).  item_ids is None for a cap_groups without an
    index.  A row with n_out == k holds the capped answer over the full ranking; n_out < k: the fetch width cut it short."""
    __slots__ = ("item_ids", "scores", "index", "group", "n_out", "pos", "status", "counters", "plan", "_ws")

    def __init__(self, item_ids, scores, index, group, n_out, pos=None, status=None, counters=None, plan=None, ws=None):
        self.item_ids, self.scores, self.index, self.group, self.n_out = item_ids, scores, index, group, n_out
        self.pos, self.status, self.counters, self.plan, self._ws = pos, status, counters, plan, ws


def _groups_args(groups, b, n_items, dev):
    """POINTER(nann_groups) for a batch of b queries over n_items rows"""
    assert isinstance(groups, Groups), "groups: what make_groups returns"
    assert n_items is None or groups.n_items == n_items, "the groups were made for another index"
    assert groups.group_of_row.device == torch.empty(0, device=dev).device, "the groups' tensors must live on the device of the call"
    assert groups.n_queries is None or groups.n_queries == b, "the groups' caps: one per query of the batch"
    return C.byref(groups.struct)


def _grouped_outputs(b, k, dev, item_ids=True):
    """(item ids, scores, rows, groups) [b, k] and n_out [b]: the cap kernel writes every element of a row, zeros behind n_out"""
    kk = max(int(k), 0)
    return (torch.empty((b, kk), dtype=torch.int64, device=dev) if item_ids else None,
            torch.empty((b, kk), dtype=torch.float32, device=dev), torch.empty((b, kk), dtype=torch.int32, device=dev),
            torch.empty((b, kk), dtype=torch.int32, device=dev), torch.zeros(b, dtype=torch.int32, device=dev))


def cap_groups(scores, rows, groups, k, n_valid=None, index=None, filter=None):
    """The group cap on its own (nann_group_cap_topk): scores f32 / rows i32 [B, k_in] CUDA tensors, a RANKED list per query
    from anywhere -- union_topk's, search_candidates' output -- of which the first n_valid[b] (i32[B]; None: k_in) entries
    count.  Walking a list in order, an entry is kept while fewer than the cap of valid entries of its group stand before it;
    the first k kept entries are returned, order unchanged -> GroupedResult (item_ids only with an index; pos: each entry's
    position in its list).  filter (make_filter): denied rows are dropped first and use no quota.  Rows outside [0, n_items)
    are dropped.  k_in <= 1024, k <= k_in.  Asynchronous on torch's current stream."""
    dev = rows.device
    rows = rows.to(dtype=torch.int32).contiguous()
    assert rows.dim() == 2, "rows: [n_queries, k_in]"
    b, k_in = rows.shape
    if scores is not None:
        scores = scores.to(device=dev, dtype=torch.float32).contiguous()
        assert scores.shape == rows.shape, "scores: the shape of rows"
    if n_valid is not None:
        n_valid = n_valid.to(device=dev, dtype=torch.int32).contiguous()
        assert n_valid.shape == (b,), "n_valid: [n_queries]"
    k = int(k)
    n_items = groups.n_items
    out_ids, out_scores, out_index, out_group, n_out = _grouped_outputs(b, k, dev, index is not None)
    out_pos = torch.empty_like(out_index)
    with torch.cuda.device(dev):
        _check(lib().nann_group_cap_topk(_ptr(scores), _ptr(rows), _ptr(n_valid), b, k_in, n_items,
                                         _ptr(index.item_ids) if index is not None else None,
                                         _groups_args(groups, b, int(index.n_items) if index is not None else None, dev),
                                         _filter_args(filter, b, index) if index is not None else
                                         (C.byref(filter.struct) if filter is not None else None), k, _ptr(out_index),
                                         _ptr(out_scores), _ptr(out_ids), _ptr(out_group), _ptr(out_pos), _ptr(n_out), _stream()),
               "cap_groups")
    return GroupedResult(out_ids, out_scores, out_index, out_group, n_out, pos=out_pos)


def search_grouped(index, scorer, q, level_topn, groups, k=None, filter=None, want_counters=True, options=None):
    """search() under a group cap (nann_search_grouped): the unchanged traversal at the fetch width F = level_topn[5]
    (level_topn: i32[6], or [B, 6] per query), then the first k (default F) entries of its ranked answer that keep to the cap
    of `groups` (make_groups) -- after `filter` (make_filter), where one is given, has dropped its rows -> GroupedResult with
    the inner search's status / counters / plan.  A failed query gets n_out = 0.  Asynchronous on torch's current stream."""
    q = q.to(device=index.device, dtype=torch.float32).contiguous()
    return _traverse_grouped(index, scorer, q, False, level_topn, groups, k, filter, want_counters, options)


def search_model_grouped(index, model, comm_seq, level_topn, groups, k=None, filter=None, want_counters=True, options=None):
    """search_model() under a group cap (nann_search_model_grouped): comm_seq f16[B, seq_len, E], scored by `model`; the rest
    as search_grouped."""
    seq = comm_seq.to(device=index.device, dtype=torch.float16).contiguous()
    return _traverse_grouped(index, model, seq, True, level_topn, groups, k, filter, want_counters, options)


def _traverse_grouped(index, by, x, model, level_topn, groups, k, filter, want_counters, options):
    dev, b = index.device, x.shape[0]
    t, tq, k_fetch = _level_topn_args(level_topn, b, dev)
    k = int(k) if k is not None else k_fetch
    out_ids, out_scores, out_index, out_group, n_out = _grouped_outputs(b, k, dev)
    status = torch.zeros(b, dtype=torch.int32, device=dev)
    counters = torch.zeros((b, 3, _lib.NUM_ROUNDS), dtype=torch.int32, device=dev) if want_counters else None
    L = lib()
    nbytes = C.c_int64(0)
    if model:
        _check(L.nann_search_model_grouped_workspace_bytes(index.handle, by.handle, t, C.c_int64(b), C.byref(nbytes)), "search_grouped")
    else:
        _check(L.nann_search_grouped_workspace_bytes(index.handle, t, C.c_int64(b), C.byref(nbytes)), "search_grouped")
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    plan = _lib.SearchPlan()
    ticks_arg = () if model else (None,)  # the model form has no phase ticks
    call = L.nann_search_model_grouped if model else L.nann_search_grouped
    with torch.cuda.device(dev):
        _check(call(index.handle, by.handle, _ptr(x), C.c_int64(b), t, _ptr(tq), _ptr(ws), C.c_int64(ws.numel()), _ptr(out_ids),
                    _ptr(out_scores), _ptr(out_index), _ptr(status), _ptr(counters), *ticks_arg,
                    C.byref(options) if options is not None else None, C.byref(plan), _filter_args(filter, b, index),
                    _groups_args(groups, b, int(index.n_items), dev), k, _ptr(out_group), _ptr(n_out), _stream()), "search_grouped")
    return GroupedResult(out_ids, out_scores, out_index, out_group, n_out, status=status, counters=counters,
                         plan=_plan_dict(plan), ws=ws)


def search_all_grouped(index, scorer, q, k, groups, fetch=None, filter=None, options=None):
    """Exhaustive search under a group cap (nann_search_all_grouped): search_all over the allowed rows at k = fetch (default:
    min(n_items, 1024)), then the first k entries of that ranking that keep to the cap -> GroupedResult.  With fetch =
    n_items it is the capped answer over the whole ranking: the ground truth of search_grouped wherever n_out == k.
    `scorer`: an ops.Scorer with q f32[B, d].  0 <= k <= fetch <= min(n_items, 1024).  Asynchronous on torch's current stream."""
    q = q.to(device=index.device, dtype=torch.float32).contiguous()
    return _flat_all_grouped(index, scorer.handle, q, k, groups, fetch, filter, options, "nann_search_all_grouped",
                             "search_all_grouped")


def search_all_model_grouped(index, model, comm_seq, k, groups, fetch=None, filter=None, options=None):
    """search_all_grouped under a model (nann_search_all_model_grouped): comm_seq f16[B, seq_len, E], an ops.Model of any kind."""
    if not isinstance(model, ops.Model):
        raise TypeError("search_all_model_grouped: an ops.Model (an ops.Scorer goes through search_all_grouped)")
    seq = comm_seq.to(device=index.device, dtype=torch.float16).contiguous()
    return _flat_all_grouped(index, model.handle, seq, k, groups, fetch, filter, options, "nann_search_all_model_grouped",
                             "search_all_model_grouped")


def _flat_all_grouped(index, handle, x, k, groups, fetch, filter, options, symbol, what):
    dev = index.device
    b, k = x.shape[0], int(k)
    fetch = int(fetch) if fetch is not None else min(int(index.n_items), 1024)
    out_ids, out_scores, out_index, out_group, n_out = _grouped_outputs(b, k, dev)
    nbytes = C.c_int64(0)
    _check(getattr(lib(), symbol + "_workspace_bytes")(index.handle, handle, b, fetch, C.byref(nbytes)), what)
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(getattr(lib(), symbol)(index.handle, handle, _ptr(x), b, fetch, k, _ptr(out_ids), _ptr(out_scores), _ptr(out_index),
                                      _ptr(out_group), _ptr(ws), ws.numel(), C.byref(options) if options is not None else None,
                                      _filter_args(filter, b, index), _groups_args(groups, b, int(index.n_items), dev),
                                      _ptr(n_out), _stream()), what)
    return GroupedResult(out_ids, out_scores, out_index, out_group, n_out, ws=ws)


class Diversity:
    """What make_diversity returns: the parameters of an MMR re-ranking (nann_diversity).
      lam   lambda in [0, 1] for every query when lams is None: 1 = relevance only, 0 = the first entry, then the farthest rows
      lams  f32[n_queries] or None: one lambda per query, read as 0 below 0 or NaN and as 1 above 1
      sim   "l2" | "ip" | None: the similarity between rows; None: "ip" under an inner-product scorer or model, else "l2" """
    __slots__ = ("lam", "lams", "sim", "n_queries")

    def __init__(self, lam, lams, sim):
        self.lam, self.lams, self.sim = float(lam), lams, sim
        self.n_queries = None if lams is None else int(lams.numel())


def make_diversity(lam=0.5, lams=None, sim=None):
    """The parameters of an MMR re-ranking: the k picks out of a fetched list maximise, one at a time, lam * score -
    (1 - lam) * (the greatest similarity to a row picked before).  lams: one lambda per query of the batch in the place of `lam`.
    sim: "l2" (-||a - b||^2) or "ip" (<a, b>) over the index's rows; None takes the scorer's metric where it has one of these
    -> Diversity."""
    assert sim in (None, "l2", "ip"), 'sim: "l2", "ip" or None'
    lam = float(lam)
    assert 0.0 <= lam <= 1.0, "lam must lie in [0, 1]"
    if lams is not None:
        lams = torch.as_tensor(lams).to(torch.float32).reshape(-1).contiguous()
    return Diversity(lam, lams, sim)


class DiverseResult:
    """Outputs of mmr / search_diverse / search_model_diverse / search_all_diverse / search_all_model_diverse, [B, k] device
    tensors in PICK order, n_out[b] = min(k, valid entries) of them at the head of row b and zeros behind.  scores: the
    original score of each pick, carried through; mmr: the value it was picked at (lam * score at the first pick, lam * score
    - (1 - lam) * penalty after); pos: its position in the list that was re-ranked.  status, counters, plan: the inner search's
    (the traversal forms; None elsewhere).  The answer is MMR over the fetched list, not over the table: a wider fetch may
    change every pick behind the first."""
    __slots__ = ("item_ids", "scores", "index", "mmr", "pos", "n_out", "status", "counters", "plan", "_ws")

    def __init__(self, item_ids, scores, index, mmr, pos, n_out, status=None, counters=None, plan=None, ws=None):
        self.item_ids, self.scores, self.index, self.mmr, self.pos, self.n_out = item_ids, scores, index, mmr, pos, n_out
        self.status, self.counters, self.plan, self._ws = status, counters, plan, ws


def _diversity_args(diversity, b, dev, by=None):
    """(POINTER(nann_diversity), what it borrows) for a batch of b queries scored by `by` (an ops.Scorer / ops.Model or None)"""
    assert isinstance(diversity, Diversity), "diversity: what make_diversity returns"
    assert diversity.n_queries is None or diversity.n_queries == b, "the diversity's lams: one per query of the batch"
    sim = diversity.sim if diversity.sim is not None else ("ip" if getattr(by, "kind", None) == "ip" else "l2")
    lams = diversity.lams.to(dev) if diversity.lams is not None else None
    st = _lib.Diversity()
    st.struct_bytes = C.sizeof(_lib.Diversity)
    st.lam = diversity.lam
    st.lambdas = lams.data_ptr() if lams is not None else None
    st.sim = _lib.SCORER_IP if sim == "ip" else _lib.SCORER_L2
    return C.byref(st), (st, lams)


def _diverse_outputs(b, k, dev):
    """(item ids, scores, rows, mmr values, positions) [b, k] and n_out [b]: the kernel writes every element of a row"""
    kk = max(int(k), 0)
    return (torch.empty((b, kk), dtype=torch.int64, device=dev), torch.empty((b, kk), dtype=torch.float32, device=dev),
            torch.empty((b, kk), dtype=torch.int32, device=dev), torch.empty((b, kk), dtype=torch.float32, device=dev),
            torch.empty((b, kk), dtype=torch.int32, device=dev), torch.zeros(b, dtype=torch.int32, device=dev))


def mmr(index, scores, rows, diversity, k, n_valid=None):
    """The MMR re-ranking on its own (nann_mmr_topk): scores f32 / rows i32 [B, k_in] CUDA tensors, a list of rows of `index`
    per query from anywhere -- search's, union_topk's, search_candidates' output -- of which the first n_valid[b] (i32[B]; None:
    k_in) entries count.  Entries whose row lies outside the index or whose score is not finite are dropped; a repeated row
    is two candidates.  -> DiverseResult, the picks in pick order.  k_in <= 1024, k <= k_in.  Asynchronous on torch's current
    stream."""
    dev = index.device
    rows = rows.to(device=dev, dtype=torch.int32).contiguous()
    assert rows.dim() == 2, "rows: [n_queries, k_in]"
    b, k_in = rows.shape
    scores = scores.to(device=dev, dtype=torch.float32).contiguous()
    assert scores.shape == rows.shape, "scores: the shape of rows"
    if n_valid is not None:
        n_valid = n_valid.to(device=dev, dtype=torch.int32).contiguous()
        assert n_valid.shape == (b,), "n_valid: [n_queries]"
    k = int(k)
    out_ids, out_scores, out_index, out_mmr, out_pos, n_out = _diverse_outputs(b, k, dev)
    dv, keep = _diversity_args(diversity, b, dev)
    with torch.cuda.device(dev):
        _check(lib().nann_mmr_topk(index.handle, _ptr(scores), _ptr(rows), _ptr(n_valid), b, k_in, dv, k, _ptr(out_index),
                                   _ptr(out_scores), _ptr(out_mmr), _ptr(out_pos), _ptr(out_ids), _ptr(n_out), _stream()), "mmr")
    return DiverseResult(out_ids, out_scores, out_index, out_mmr, out_pos, n_out, ws=keep)


def search_diverse(index, scorer, q, level_topn, diversity, k=None, filter=None, want_counters=True, options=None):
    """search() with diversified results (nann_search_diverse): the unchanged traversal at the fetch width F = level_topn[5]
    (level_topn: i32[6], or [B, 6] per query), then k (default F) MMR picks out of its answer -- without the rows `filter`
    (make_filter) denies, where one is given -> DiverseResult with the inner search's status / counters / plan.  A failed query
    gets n_out = 0.  Asynchronous on torch's current stream."""
    q = q.to(device=index.device, dtype=torch.float32).contiguous()
    return _traverse_diverse(index, scorer, q, False, level_topn, diversity, k, filter, want_counters, options)


def search_model_diverse(index, model, comm_seq, level_topn, diversity, k=None, filter=None, want_counters=True, options=None):
    """search_model() with diversified results (nann_search_model_diverse): comm_seq f16[B, seq_len, E], scored by `model`;
    the rest as search_diverse."""
    seq = comm_seq.to(device=index.device, dtype=torch.float16).contiguous()
    return _traverse_diverse(index, model, seq, True, level_topn, diversity, k, filter, want_counters, options)


def _traverse_diverse(index, by, x, model, level_topn, diversity, k, filter, want_counters, options):
    dev, b = index.device, x.shape[0]
    t, tq, k_fetch = _level_topn_args(level_topn, b, dev)
    k = int(k) if k is not None else k_fetch
    out_ids, out_scores, out_index, out_mmr, out_pos, n_out = _diverse_outputs(b, k, dev)
    status = torch.zeros(b, dtype=torch.int32, device=dev)
    counters = torch.zeros((b, 3, _lib.NUM_ROUNDS), dtype=torch.int32, device=dev) if want_counters else None
    L = lib()
    nbytes = C.c_int64(0)
    if model:
        _check(L.nann_search_model_diverse_workspace_bytes(index.handle, by.handle, t, C.c_int64(b), C.byref(nbytes)), "search_diverse")
    else:
        _check(L.nann_search_diverse_workspace_bytes(index.handle, t, C.c_int64(b), C.byref(nbytes)), "search_diverse")
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    plan = _lib.SearchPlan()
    ticks_arg = () if model else (None,)  # the model form has no phase ticks
    call = L.nann_search_model_diverse if model else L.nann_search_diverse
    dv, keep = _diversity_args(diversity, b, dev, by)
    with torch.cuda.device(dev):
        _check(call(index.handle, by.handle, _ptr(x), C.c_int64(b), t, _ptr(tq), _ptr(ws), C.c_int64(ws.numel()), _ptr(out_ids),
                    _ptr(out_scores), _ptr(out_index), _ptr(status), _ptr(counters), *ticks_arg,
                    C.byref(options) if options is not None else None, C.byref(plan), _filter_args(filter, b, index),
                    dv, k, _ptr(out_mmr), _ptr(out_pos), _ptr(n_out), _stream()), "search_diverse")
    return DiverseResult(out_ids, out_scores, out_index, out_mmr, out_pos, n_out, status=status, counters=counters,
                         plan=_plan_dict(plan), ws=(ws, keep))


def search_all_diverse(index, scorer, q, k, diversity, fetch=None, filter=None, options=None):
    """Exhaustive search with diversified results (nann_search_all_diverse): search_all over the allowed rows at k = fetch
    (default: min(n_items, 1024)), then k MMR picks out of that exact top-fetch -> DiverseResult.  `scorer`: an ops.Scorer
    with q f32[B, d].  0 <= k <= fetch <= min(n_items, 1024).  Asynchronous on torch's current stream."""
    q = q.to(device=index.device, dtype=torch.float32).contiguous()
    return _flat_all_diverse(index, scorer, scorer.handle, q, k, diversity, fetch, filter, options, "nann_search_all_diverse",
                             "search_all_diverse")


def search_all_model_diverse(index, model, comm_seq, k, diversity, fetch=None, filter=None, options=None):
    """search_all_diverse under a model (nann_search_all_model_diverse): comm_seq f16[B, seq_len, E], an ops.Model of any kind."""
    if not isinstance(model, ops.Model):
        raise TypeError("search_all_model_diverse: an ops.Model (an ops.Scorer goes through search_all_diverse)")
    seq = comm_seq.to(device=index.device, dtype=torch.float16).contiguous()
    return _flat_all_diverse(index, model, model.handle, seq, k, diversity, fetch, filter, options,
                             "nann_search_all_model_diverse", "search_all_model_diverse")


def _flat_all_diverse(index, by, handle, x, k, diversity, fetch, filter, options, symbol, what):
    dev = index.device
    b, k = x.shape[0], int(k)
    fetch = int(fetch) if fetch is not None else min(int(index.n_items), 1024)
    out_ids, out_scores, out_index, out_mmr, out_pos, n_out = _diverse_outputs(b, k, dev)
    nbytes = C.c_int64(0)
    _check(getattr(lib(), symbol + "_workspace_bytes")(index.handle, handle, b, fetch, C.byref(nbytes)), what)
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    dv, keep = _diversity_args(diversity, b, dev, by)
    with torch.cuda.device(dev):
        _check(getattr(lib(), symbol)(index.handle, handle, _ptr(x), b, fetch, k, _ptr(out_ids), _ptr(out_scores), _ptr(out_index),
                                      _ptr(out_mmr), _ptr(out_pos), _ptr(ws), ws.numel(),
                                      C.byref(options) if options is not None else None, _filter_args(filter, b, index), dv,
                                      _ptr(n_out), _stream()), what)
    return DiverseResult(out_ids, out_scores, out_index, out_mmr, out_pos, n_out, ws=(ws, keep))


class Attributes:
    """What make_attributes returns: the attribute columns of an index's rows, each [n_items] or None (they may live on the CPU).
      label_of_row  i32: one label per row (a category, a region)
      value_of_row  f32: one number per row (a price); NaN passes no range
      tags_of_row   i64, read as u64: a set of up to 64 tags, bit t = tag t"""
    __slots__ = ("label_of_row", "value_of_row", "tags_of_row", "n_items", "device")

    def __init__(self, label_of_row, value_of_row, tags_of_row, n_items, device):
        self.label_of_row, self.value_of_row, self.tags_of_row = label_of_row, value_of_row, tags_of_row
        self.n_items, self.device = n_items, device


def _u64_as_i64(a):
    """tag words (ints, numpy uint64 / int64, an int64 tensor) as an int64 tensor of the same bits"""
    if isinstance(a, torch.Tensor):
        return a.cpu().to(torch.int64).reshape(-1)
    if not (isinstance(a, np.ndarray) and a.dtype == np.uint64):  # (python ints one by one: numpy would read 2^64 - 1 next to 0 as a float)
        flat = a.reshape(-1).tolist() if isinstance(a, np.ndarray) else list(np.asarray(a, dtype=object).reshape(-1))
        a = np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in flat], dtype=np.uint64)
    return torch.from_numpy(np.ascontiguousarray(a.reshape(-1)).view(np.int64).copy())


def make_attributes(index, label_of_row=None, value_of_row=None, tags_of_row=None, label_of_item_id=None, value_of_item_id=None,
                    tags_of_item_id=None, device=None):
    """The attribute columns of `index` for predicate searches, built once per index.  *_of_row: one entry per internal row,
    [n_items]; or *_of_item_id = (item_ids, values), two 1-D arrays of one length, mapped through index.item_ids -- an unknown id
    names nothing, and an item that is not named gets label -1, value NaN (which passes no range) and no tag.  Tags are int64
    tensors (or uint64 arrays) read as 64 bits.  device: where the tensors live (default: the index's; "cpu" builds them
    without a GPU).  -> Attributes."""
    dev = torch.device(device if device is not None else index.device)
    n = int(index.n_items)

    def column(of_row, of_item_id, conv, dtype, missing, name):
        assert of_row is None or of_item_id is None, "%s: one of %s_of_row and %s_of_item_id" % (name, name, name)
        if of_row is not None:
            c = conv(of_row)
            assert c.numel() == n, "%s_of_row: one entry per row of the index" % name
            return c.to(dtype).to(dev).contiguous()
        if of_item_id is None:
            return None
        ids, vals = _i64(of_item_id[0]), conv(of_item_id[1])
        assert ids.numel() == vals.numel(), "%s_of_item_id: (item_ids, values) of one length" % name
        c = torch.full((n,), missing, dtype=dtype)
        sv, perm = _sorted_item_ids(index)
        if sv.numel() and ids.numel():
            pos = torch.searchsorted(sv, ids.to(sv.device)).clamp_(max=sv.numel() - 1)
            found = (sv[pos] == ids.to(sv.device)).cpu()
            c[perm[pos].cpu()[found]] = vals.to(dtype)[found]
        return c.to(dev).contiguous()

    def f32(a):
        return torch.as_tensor(np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float32)).reshape(-1)

    def i32(a):
        a = _i64(a)
        assert a.numel() == 0 or (int(a.min()) >= -(1 << 31) and int(a.max()) < (1 << 31)), "labels are 32-bit"
        return a

    return Attributes(column(label_of_row, label_of_item_id, i32, torch.int32, -1, "label"),
                      column(value_of_row, value_of_item_id, f32, torch.float32, float("nan"), "value"),
                      column(tags_of_row, tags_of_item_id, _u64_as_i64, torch.int64, 0, "tags"), n, dev)


class Predicates:
    """What make_predicates returns: the per-query conditions of one batch over an Attributes (tensors on its device) and the
    ctypes nann_predicates, which borrows their memory and the attribute columns'.
      label_splits i64[n_queries + 1], labels i32[n_labels]: query i allows labels[label_splits[i] : label_splits[i + 1]]
      value_lo, value_hi f32[n_queries];  tags_all, tags_any, tags_none i64[n_queries] read as u64 -- each or None"""
    __slots__ = ("attributes", "label_splits", "labels", "value_lo", "value_hi", "tags_all", "tags_any", "tags_none", "n_queries",
                 "n_items", "device", "struct")

    def __init__(self, attributes, n_queries, label_splits, labels, value_lo, value_hi, tags_all, tags_any, tags_none):
        self.attributes, self.n_queries, self.n_items, self.device = attributes, int(n_queries), attributes.n_items, attributes.device
        self.label_splits, self.labels, self.value_lo, self.value_hi = label_splits, labels, value_lo, value_hi
        self.tags_all, self.tags_any, self.tags_none = tags_all, tags_any, tags_none
        st = _lib.Predicates()
        st.struct_bytes = C.sizeof(_lib.Predicates)

        def ptr(t):
            return t.data_ptr() if t is not None and t.numel() else None
        st.label_of_row, st.value_of_row, st.tags_of_row = (ptr(attributes.label_of_row), ptr(attributes.value_of_row),
                                                             ptr(attributes.tags_of_row))
        st.label_splits = label_splits.data_ptr() if label_splits is not None else None
        st.labels = ptr(labels)
        st.n_labels = int(labels.numel()) if labels is not None else 0
        st.value_lo, st.value_hi = ptr(value_lo), ptr(value_hi)
        st.tags_all, st.tags_any, st.tags_none = ptr(tags_all), ptr(tags_any), ptr(tags_none)
        self.struct = st


def make_predicates(attributes, n_queries, label_in=None, value_range=None, tags_all=None, tags_any=None, tags_none=None):
    """The per-query conditions of a batch of n_queries over `attributes` (make_attributes), ragged and built per batch.
      label_in     one 1-D array of allowed labels per query (any order, duplicates, any number); None or an empty array: no
                   label test for that query
      value_range  (lo, hi): each None (unbounded), a number for every query, or an array [n_queries]; a row passes iff
                   lo <= value <= hi, so lo > hi matches nothing and a NaN bound passes nothing
      tags_all / tags_any / tags_none   a 64-bit word for every query or an array [n_queries]: the row's tags hold every bit of
                   `all`, at least one of `any` (when it is not 0) and none of `none`
    A row passes a query iff every test that is given passes.  -> Predicates."""
    assert isinstance(attributes, Attributes), "attributes: what make_attributes returns"
    dev, nq = attributes.device, int(n_queries)
    splits = labels = None
    if label_in is not None:
        assert attributes.label_of_row is not None, "label_in needs the attributes' label_of_row"
        assert len(label_in) == nq, "label_in: one list per query of the batch"
        per = [_i64(l) if l is not None else torch.zeros(0, dtype=torch.int64) for l in label_in]
        lens = torch.tensor([0] + [int(p.numel()) for p in per], dtype=torch.int64)
        splits = torch.cumsum(lens, 0).to(dev).contiguous()
        flat = torch.cat(per) if per else torch.zeros(0, dtype=torch.int64)
        assert flat.numel() == 0 or (int(flat.min()) >= -(1 << 31) and int(flat.max()) < (1 << 31)), "labels are 32-bit"
        labels = flat.to(torch.int32).to(dev).contiguous()

    def per_query(v, conv, dtype):
        if v is None:
            return None
        if isinstance(v, (int, float)):
            v = [v] * nq
        t = conv(v).to(dtype)
        assert t.numel() == nq, "a per-query condition: one entry per query of the batch"
        return t.to(dev).contiguous()

    def f32(a):
        return torch.as_tensor(np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float32)).reshape(-1)

    lo = hi = None
    if value_range is not None:
        assert attributes.value_of_row is not None, "value_range needs the attributes' value_of_row"
        lo, hi = per_query(value_range[0], f32, torch.float32), per_query(value_range[1], f32, torch.float32)
    tags = [per_query(t, _u64_as_i64, torch.int64) for t in (tags_all, tags_any, tags_none)]
    assert all(t is None for t in tags) or attributes.tags_of_row is not None, "tag conditions need the attributes' tags_of_row"
    return Predicates(attributes, nq, splits, labels, lo, hi, *tags)


def _predicates_args(predicates, b, n_items, dev):
    """POINTER(nann_predicates) for a batch of b queries over n_items rows on `dev`"""
    assert isinstance(predicates, Predicates), "predicates: what make_predicates returns"
    assert n_items is None or predicates.n_items == n_items, "the predicates' attributes were made for another index"
    assert torch.empty(0, device=predicates.device).device == torch.empty(0, device=dev).device, \
        "the predicates' tensors must live on the device of the call"
    assert predicates.n_queries == b, "the predicates: one set of conditions per query of the batch"
    return C.byref(predicates.struct)


class PredicateResult:
    """Outputs of predicate_topk, [B, k] device tensors: the first k entries of a ranked list that pass, n_out[b] of them at the
    head of row b and zeros behind.  pos: each entry's position in its input list.  item_ids is None without an index."""
    __slots__ = ("item_ids", "scores", "index", "pos", "n_out")

    def __init__(self, item_ids, scores, index, pos, n_out):
        self.item_ids, self.scores, self.index, self.pos, self.n_out = item_ids, scores, index, pos, n_out


def predicate_topk(scores, rows, predicates, k, n_valid=None, index=None, filter=None):
    """The predicate step on its own (nann_predicate_topk): scores f32 / rows i32 [B, k_in] CUDA tensors, a RANKED list per query
    from anywhere -- union_topk's, search_candidates' output -- of which the first n_valid[b] (i32[B]; None: k_in) entries count.
    The first k entries whose row passes `predicates` (make_predicates) and `filter` (make_filter) are returned, order unchanged
    -> PredicateResult (item_ids only with an index).  Its n_out is the n_valid of a cap_groups or mmr behind it.  k_in <= 1024,
    k <= k_in.  Asynchronous on torch's current stream."""
    dev = rows.device
    rows = rows.to(dtype=torch.int32).contiguous()
    assert rows.dim() == 2, "rows: [n_queries, k_in]"
    b, k_in = rows.shape
    if scores is not None:
        scores = scores.to(device=dev, dtype=torch.float32).contiguous()
        assert scores.shape == rows.shape, "scores: the shape of rows"
    if n_valid is not None:
        n_valid = n_valid.to(device=dev, dtype=torch.int32).contiguous()
        assert n_valid.shape == (b,), "n_valid: [n_queries]"
    k = int(k)
    kk = max(k, 0)
    out_ids = torch.empty((b, kk), dtype=torch.int64, device=dev) if index is not None else None
    out_scores = torch.empty((b, kk), dtype=torch.float32, device=dev)
    out_index = torch.empty((b, kk), dtype=torch.int32, device=dev)
    out_pos = torch.empty((b, kk), dtype=torch.int32, device=dev)
    n_out = torch.zeros(b, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _check(lib().nann_predicate_topk(_ptr(scores), _ptr(rows), _ptr(n_valid), b, k_in, predicates.n_items,
                                         _ptr(index.item_ids) if index is not None else None,
                                         _predicates_args(predicates, b, int(index.n_items) if index is not None else None, dev),
                                         _filter_args(filter, b, index) if index is not None else
                                         (C.byref(filter.struct) if filter is not None else None), k, _ptr(out_index),
                                         _ptr(out_scores), _ptr(out_ids), _ptr(out_pos), _ptr(n_out), _stream()), "predicate_topk")
    return PredicateResult(out_ids, out_scores, out_index, out_pos, n_out)


def predicate_count(predicates, filter=None):
    """The selectivity (nann_predicate_count): i64[n_queries] on the device, the rows of the index that pass each query's
    conditions and `filter`.  With count / n_items = s, a traversal at fetch width F finds about s * F passing rows: where that is
    well above k, search_where is the call; where it is not, search_all_where.  Asynchronous on torch's current stream."""
    dev, b = predicates.device, predicates.n_queries
    out = torch.zeros(b, dtype=torch.int64, device=dev)
    if filter is not None:
        assert filter.n_items == predicates.n_items and filter.device == dev, "the filter was made for another index or device"
        assert filter.n_queries is None or filter.n_queries == b, "the filter's exclusion lists: one per query of the batch"
    with torch.cuda.device(dev):
        _check(lib().nann_predicate_count(predicates.n_items, C.byref(predicates.struct),
                                          C.byref(filter.struct) if filter is not None else None, b, _ptr(out), _stream()),
               "predicate_count")
    return out


def search_where(index, scorer, q, level_topn, predicates, k=None, filter=None, want_counters=True, options=None):
    """search() under attribute predicates (nann_search_where): the unchanged traversal at the fetch width F = level_topn[5]
    (i32[6], or [B, 6] per query), then the first k (default F) entries of its ranked answer whose row passes `predicates`
    (make_predicates) and `filter` -> SearchResult, n_out[b] entries at the head of row b and zeros behind.  n_out < k: the list
    was cut short -- widen F, or call search_all_where (predicate_count tells in advance).  A failed query gets n_out = 0."""
    q = q.to(device=index.device, dtype=torch.float32).contiguous()
    return _traverse(index, scorer, q, False, level_topn, want_counters, False, options, filter, k, predicates)


def search_model_where(index, model, comm_seq, level_topn, predicates, k=None, filter=None, want_counters=True, options=None):
    """search_model() under attribute predicates (nann_search_model_where): comm_seq f16[B, seq_len, E]; the rest as search_where."""
    seq = comm_seq.to(device=index.device, dtype=torch.float16).contiguous()
    return _traverse(index, model, seq, True, level_topn, want_counters, False, options, filter, k, predicates)


def search_all_where(index, scorer, q, k, predicates, filter=None, options=None):
    """Exhaustive search over the rows that PASS (nann_search_all_where): the exact top k of every query's passing rows, TopKV2
    order -> SearchAllResult with n_out[b] = min(k, passing rows) valid entries at the head of row b and zeros behind; scores
    have the bits of search_all's.  The ground truth of search_where.  `scorer`: an ops.Scorer with q f32[B, d]."""
    q = q.to(device=index.device, dtype=torch.float32).contiguous()
    return _flat_all(index, scorer.handle, q, k, options, filter, "nann_search_all", "search_all_where", predicates)


def search_all_model_where(index, model, comm_seq, k, predicates, filter=None, options=None):
    """search_all_where under a model (nann_search_all_model_where): comm_seq f16[B, seq_len, E], an ops.Model of any kind."""
    if not isinstance(model, ops.Model):
        raise TypeError("search_all_model_where: an ops.Model (an ops.Scorer goes through search_all_where)")
    seq = comm_seq.to(device=index.device, dtype=torch.float16).contiguous()
    return _flat_all(index, model.handle, seq, k, options, filter, "nann_search_all_model", "search_all_model_where", predicates)


def prepare(index, scorer):
    """Build the pre-projected table of (scorer | model, index) now and pin it (nann_scorer_prepare /
    nann_model_prepare): no request pays for it.  Returns (table_bytes, resident_bytes)."""
    is_model = isinstance(scorer, ops.Model)
    L = lib()
    with torch.cuda.device(index.device):
        _check((L.nann_model_prepare if is_model else L.nann_scorer_prepare)(scorer.handle, index.handle, _stream()),
               "prepare")
    return table_bytes(index, scorer)


def release(index, scorer):
    is_model = isinstance(scorer, ops.Model)
    L = lib()
    _check((L.nann_model_release if is_model else L.nann_scorer_release)(scorer.handle, index.handle), "release")


def table_bytes(index, scorer):
    is_model = isinstance(scorer, ops.Model)
    L = lib()
    tb, rb = C.c_int64(0), C.c_int64(0)
    _check((L.nann_model_table_bytes if is_model else L.nann_scorer_table_bytes)(
        scorer.handle, index.handle if index is not None else None, C.byref(tb), C.byref(rb)), "table_bytes")
    return tb.value, rb.value


class EvalResult:
    """Outputs of search_eval: rows [b, :n_out[b]] are valid (the rest is zero)."""

    def __init__(self, item_ids, scores, index, n_out, status):
        self.item_ids, self.scores, self.index, self.n_out, self.status = item_ids, scores, index, n_out, status


EVAL_FORMS = ("slot", "lds", "windows")


def search_eval_plan(index, scorer, n_queries):
    """The plan search_eval runs for a batch of n_queries users of (index, scorer | model), asked of the host alone
    (nann_search_eval_plan: nothing is launched) -> dict(form 0 slot / 1 lds / 2 windows, form_name, n_windows, slots, threads,
    use_dirty).  Raises what search_eval raises for the scorer (the inner product is unsupported)."""
    is_model = isinstance(scorer, ops.Model)
    p = _lib.EvalPlan()
    _check(lib().nann_search_eval_plan(index.handle, None if is_model else scorer.handle, scorer.handle if is_model else None,
                                       C.c_int64(int(n_queries)), C.byref(p)), "search_eval_plan")
    assert p.struct_bytes == C.sizeof(_lib.EvalPlan), p.struct_bytes
    return {"form": p.form, "form_name": EVAL_FORMS[p.form], "n_windows": p.n_windows, "slots": p.slots, "threads": p.threads,
            "use_dirty": p.use_dirty}


def search_eval(index, scorer, q, num_scoring=(3, 1, 1), top_k_per_level=(400, 200, 100), topk_eval=200, want_counters=False):
    """Model.retrieval() (model.py:299-362) for a batch of users in ONE kernel (nann_search_eval /
    nann_search_eval_model).  `scorer`: ops.Scorer with q f32[B, d], or ops.Model with q = comm_seq
    f16[B, seq_len, E].  Same results as search_eval_per_op, user by user."""
    is_model = isinstance(scorer, ops.Model)
    dev = index.device
    q = q.to(device=dev, dtype=torch.float16 if is_model else torch.float32).contiguous()
    b, k = q.shape[0], int(topk_eval)
    ns = (C.c_int32 * 3)(*[int(x) for x in num_scoring])
    tk = (C.c_int32 * 3)(*[int(x) for x in top_k_per_level])
    out_ids = torch.empty((b, k), dtype=torch.int64, device=dev)
    out_scores = torch.empty((b, k), dtype=torch.float32, device=dev)
    out_index = torch.empty((b, k), dtype=torch.int32, device=dev)
    n_out = torch.empty(b, dtype=torch.int32, device=dev)
    status = torch.empty(b, dtype=torch.int32, device=dev)
    nbytes = C.c_int64(0)
    _check(lib().nann_search_eval_workspace_bytes(index.handle, scorer.handle if is_model else None, C.c_int64(b),
                                                  C.byref(nbytes)))
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    counters = None
    with torch.cuda.device(dev):
        if want_counters and not is_model:  # F, G, S per user (nann_search_eval_ex)
            counters = torch.zeros((b, 3), dtype=torch.int32, device=dev)
            _check(lib().nann_search_eval_ex(index.handle, scorer.handle, _ptr(q), C.c_int64(b), ns, tk, C.c_int32(k), _ptr(ws),
                                             C.c_int64(ws.numel()), _ptr(out_ids), _ptr(out_scores), _ptr(out_index),
                                             _ptr(n_out), _ptr(status), _ptr(counters), _stream()), "search_eval")
        else:
            fn = lib().nann_search_eval_model if is_model else lib().nann_search_eval
            _check(fn(index.handle, scorer.handle, _ptr(q), C.c_int64(b), ns, tk, C.c_int32(k), _ptr(ws),
                      C.c_int64(ws.numel()), _ptr(out_ids), _ptr(out_scores), _ptr(out_index), _ptr(n_out), _ptr(status),
                      _stream()), "search_eval")
    res = EvalResult(out_ids, out_scores, out_index, n_out, status)
    res.counters = counters
    return res


# -----------------------------------------------------------------------------
# build_model() spelled with the per-op drop-ins (one query)
def _fake_row_splits(x):
    """build_opt_graph.py:29-30"""
    return torch.tensor([0, x.numel()], dtype=torch.int64, device=x.device)


def _set_difference(a, flags):
    """build_opt_graph.py:33-36"""
    values, _, flags = ops.bitmap_ref_difference(a, _fake_row_splits(a), flags)
    return values, flags


def _ragged_gather(values, row_splits, idx):
    """build_opt_graph.py:39-49"""
    out, _ = ops.group_gather(values, row_splits, idx.to(torch.int64), _fake_row_splits(idx), unique=False)
    return out


def _top_k(ids, scores, k):
    """build_opt_graph.py:52-66"""
    scores, indices = ops.top_k(scores, k)
    return ops.gather(ids, indices), scores


def search_per_op(index, scorer, q, level_topn):
    """One query through the op-by-op schedule (build_opt_graph.py:109-149).
    Raises the error the reference graph would raise.  Returns
    (item_ids i64[k], scores f32[k], internal index i32[k])."""
    q = q.reshape(-1)
    t = [int(x) for x in level_topn]

    def forward(idx):  # :91-107
        if idx.numel() == 0:
            raise ops.InternalError(6, "Error when getting input address or size")
        s = ops.blaze_score(scorer, q, table=index.item_embs, indices=idx)
        if idx.numel() == 1:  # tf.squeeze -> scalar; TopKV2/ConcatV2 reject it
            raise ops.InvalidArgumentError(8, "input must be >= 1-D, got shape []")
        return s

    enter_points = index.enter_points
    # level 2
    scores = forward(enter_points)                                          # :111
    idx_results, scores_result = _top_k(enter_points, scores, t[0])         # :112
    # level 1
    idx_next = _ragged_gather(index.nb_values[1], index.nb_row_splits[1], idx_results)   # :116
    flags = torch.zeros(index.bitmap_words, dtype=torch.int32, device=index.device)      # :115-118
    idx_results, _ = _set_difference(idx_results, flags)                    # :119-120
    idx_next, _ = _set_difference(idx_next, flags)                          # :121-122
    scores_next = forward(idx_next)                                         # :124
    idx_result, scores_result = _top_k(torch.cat([idx_results, idx_next]),
                                       torch.cat([scores_result, scores_next]), t[1])    # :125-127
    # level 0
    idx_candidate = idx_result
    flags.zero_()                                                           # :131
    idx_candidate, _ = _set_difference(idx_candidate, flags)                # :132-133
    for i in range(3):                                                      # :135
        idx_next = _ragged_gather(index.nb_values[0], index.nb_row_splits[0], idx_candidate)   # :136
        idx_next, _ = _set_difference(idx_next, flags)                      # :137
        scores_next = forward(idx_next)                                     # :138
        idx_candidate, scores_candidate = _top_k(idx_next, scores_next, t[i + 2])   # :139
        idx_result = torch.cat([idx_result, idx_candidate])                 # :140
        scores_result = torch.cat([scores_result, scores_candidate])        # :141
    idx_result, scores_result = _top_k(idx_result, scores_result, t[5])     # :143
    item_ids = ops.gather(index.item_ids.view(torch.int32).reshape(-1, 2), idx_result)   # :144
    return item_ids.reshape(-1).view(torch.int64), scores_result, idx_result


# -----------------------------------------------------------------------------
# f3: the eval-graph traversal (Model.retrieval / search_level, model.py:299-362) spelled with
# the same drop-in ops.  It differs from the serving schedule in its frontier rule (new nodes
# that score at least the worst kept result), in the min(k, n) guard of its top_k (model.py:268)
# and in visiting neighbours as an ascending set (tf.unique + tf.sets, :316-321).
def search_eval_per_op(index, scorer, q, num_scoring=(3, 1, 1), top_k_per_level=(400, 200, 100),
                       topk_eval=200, backend=None, stats=None):
    """One query through Model.retrieval().  num_scoring / top_k_per_level are indexed by level
    (0, 1, start level 2), as config.py:50-58 lists them.  Returns
    (item_ids i64[<=topk_eval], scores f32, internal index i32).  `backend`: the module providing
    group_gather / bitmap_ref_difference / blaze_score / top_k / gather (default: nann_amd.ops, the
    HIP kernels; the CPU tests pass a stand-in to check this host logic against the oracle).  `stats`: a dict that
    receives F / G / S (rows walked, neighbours gathered, rows scored incl. the enter points: the fused kernel's counters)."""
    B = ops if backend is None else backend
    assert int(num_scoring[2]) == 1                                          # model.py:347
    n_f = n_g = 0
    n_s = int(index.enter_points.numel())
    q = q.reshape(-1)

    def get_scores(idx):                                                     # :240-262
        if idx.numel() == 0:  # plain TF scoring of an empty batch: an empty tensor, the level loop goes on
            return torch.empty(0, dtype=torch.float32, device=idx.device)   # (only the serving graph's BlazeXlaOp fails here)
        return B.blaze_score(scorer, q, table=index.item_embs, indices=idx)

    def top_k(ids, scores, k):                                               # :264-283, k = min(k, n)
        k = min(int(k), int(ids.numel()))
        scores, indices = B.top_k(scores, k)
        return B.gather(ids, indices), scores

    results = index.enter_points
    scores = get_scores(results)                                             # :350-351
    results, scores = top_k(results, scores, top_k_per_level[2])             # :353
    for level in (1, 0):                                                     # :355-356
        flags = torch.zeros(index.bitmap_words, dtype=torch.int32, device=index.enter_points.device)
        idx_result, scores_result = results, scores
        _, _, flags = B.bitmap_ref_difference(results, _fake_row_splits(results), flags)   # visited = idx_ep (:311)
        idx_candidate = results
        for _ in range(int(num_scoring[level])):
            nxt, _ = B.group_gather(index.nb_values[level], index.nb_row_splits[level],
                                    idx_candidate.to(torch.int64), _fake_row_splits(idx_candidate),
                                    unique=False)                            # :316
            n_f += int(idx_candidate.numel())
            n_g += int(nxt.numel())
            nxt, _, flags = B.bitmap_ref_difference(nxt, _fake_row_splits(nxt), flags)   # unique, minus visited, visited |= (:317-321)
            n_s += int(nxt.numel())
            idx_next = torch.sort(nxt).values                                # tf.sets results are ascending
            scores_next = get_scores(idx_next)                               # :323
            idx_result, scores_result = top_k(torch.cat([idx_result, idx_next]),
                                              torch.cat([scores_result, scores_next]),
                                              top_k_per_level[level])        # :326-328
            mask = scores_next >= scores_result[-1]                          # :330
            idx_candidate = idx_next[mask]                                   # :331
        results, scores = idx_result, scores_result
    if stats is not None:
        stats.update(F=n_f, G=n_g, S=n_s)
    results, scores = results[:topk_eval], scores[:topk_eval]                # :358
    item_ids = B.gather(index.item_ids.view(torch.int32).reshape(-1, 2), results)   # :360
    return item_ids.reshape(-1).view(torch.int64), scores, results
