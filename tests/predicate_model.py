"""Test-side model of the attribute predicates (nann_predicates, include/nann_hip.h), written from the words of the contract and
not from the kernels: numpy, vectorised (`passes`, `where_topk`, `count`: what the device tests compare against) and a plain
Python restatement entry by entry (`restate_passes`, `restate_topk`: what test_predicate_cpu.py holds the numpy model to).
Nothing under nann_amd/ imports it.

A predicate set `pred` is a dict of numpy arrays, every key optional:
  label_of_row i32[n_items], value_of_row f32[n_items], tags_of_row u64[n_items]          the attribute columns
  label_splits i64[n_queries + 1], labels i32[n_labels]                                    query i allows labels[splits[i] .. splits[i + 1])
  value_lo, value_hi f32[n_queries];  tags_all, tags_any, tags_none u64[n_queries]
Row r passes query i iff every test that is present passes: the label test is present iff the query's range, clamped to
[0, n_labels], is not empty; the value test iff one of the bounds is given (a missing side is unbounded; lo <= v <= hi as IEEE
compares: NaN passes nothing); the tags test iff one of the three words is given (a missing one is 0).
A filter is (deny bool[n_items] or None, exclude: one array of rows per query, or None)."""
import numpy as np


def label_range(pred, query):
    """the clamped range [b, e) of the query's label list; (0, 0) without one"""
    if pred.get("label_splits") is None or pred.get("labels") is None or len(pred["labels"]) == 0:
        return 0, 0
    n = len(pred["labels"])
    b = min(max(int(pred["label_splits"][query]), 0), n)
    e = max(b, min(max(int(pred["label_splits"][query + 1]), 0), n))
    return b, e


def passes(pred, query, rows):
    """rows: int array of in-range rows -> bool array: which of them pass query `query`"""
    rows = np.asarray(rows, np.int64)
    ok = np.ones(rows.shape, bool)
    if pred is None:
        return ok
    b, e = label_range(pred, query)
    if e > b:
        ok &= np.isin(np.asarray(pred["label_of_row"], np.int32)[rows], np.asarray(pred["labels"], np.int32)[b:e])
    lo, hi = pred.get("value_lo"), pred.get("value_hi")
    if lo is not None or hi is not None:
        v = np.asarray(pred["value_of_row"], np.float32)[rows]
        with np.errstate(invalid="ignore"):
            if lo is not None:
                ok &= np.float32(lo[query]) <= v
            if hi is not None:
                ok &= v <= np.float32(hi[query])
    ta, ty, tn = pred.get("tags_all"), pred.get("tags_any"), pred.get("tags_none")
    if ta is not None or ty is not None or tn is not None:
        t = np.asarray(pred["tags_of_row"], np.uint64)[rows]
        all_, any_, none_ = (np.uint64(0) if w is None else np.uint64(w[query]) for w in (ta, ty, tn))
        ok &= (t & all_) == all_
        if any_ != 0:
            ok &= (t & any_) != 0
        ok &= (t & none_) == 0
    return ok


def _allowed(filter, query, rows, n_items):
    """rows i64[...] -> bool: in range and not taken out by the filter"""
    ok = (rows >= 0) & (rows < n_items)
    if filter is None:
        return ok
    deny, exclude = filter
    if deny is not None and n_items > 0:
        ok &= ~np.asarray(deny, bool)[np.where(ok, rows, 0)]
    if exclude is not None and len(exclude[query]):
        ok &= ~np.isin(rows, np.asarray(exclude[query], np.int64))
    return ok


def where_topk(rows, scores, n_valid, filter, pred, k, n_items, item_ids=None, q0=0):
    """rows i32[n_queries, k_in] ranked lists, scores f32 the same or None, n_valid i32[n_queries] or None; row i of the lists is
    query q0 + i of the filter and the predicates -> dict of index i32, scores f32, pos i32, item_ids i64 (with item_ids), each
    [n_queries, k], and n_out i32[n_queries]: the first k valid entries that pass, order kept, zeros behind"""
    rows = np.asarray(rows, np.int32)
    n_q, k_in = rows.shape
    sc = np.zeros((n_q, k_in), np.float32) if scores is None else np.asarray(scores, np.float32)
    out = {"index": np.zeros((n_q, k), np.int32), "scores": np.zeros((n_q, k), np.float32), "pos": np.zeros((n_q, k), np.int32),
           "n_out": np.zeros(n_q, np.int32)}
    if item_ids is not None:
        out["item_ids"] = np.zeros((n_q, k), np.int64)
    for i in range(n_q):
        r = rows[i].astype(np.int64)
        nv = k_in if n_valid is None else min(max(int(np.asarray(n_valid)[i]), 0), k_in)
        ok = (np.arange(k_in) < nv) & _allowed(filter, q0 + i, r, n_items)
        ok[ok] = passes(pred, q0 + i, r[ok])
        p = np.nonzero(ok)[0][:max(k, 0)]
        m = len(p)
        out["n_out"][i] = m
        out["index"][i, :m] = rows[i, p]
        out["scores"][i, :m] = sc[i, p]                            # the entry's own bits: a NaN stays that NaN
        out["pos"][i, :m] = p
        if item_ids is not None:
            out["item_ids"][i, :m] = np.asarray(item_ids, np.int64)[r[p]]
    return out


def count(pred, filter, n_queries, n_items):
    """-> i64[n_queries]: the rows of [0, n_items) that pass each query and the filter"""
    rows = np.arange(n_items, dtype=np.int64)
    out = np.zeros(n_queries, np.int64)
    for i in range(n_queries):
        ok = _allowed(filter, i, rows, n_items)
        ok[ok] = passes(pred, i, rows[ok])
        out[i] = ok.sum()
    return out


# ---- the plain restatement ------------------------------------------------------------------------------------------------
def restate_passes(pred, query, row):
    """one (query, row) pair, in plain Python"""
    import math
    if pred is None:
        return True
    if pred.get("label_splits") is not None and pred.get("labels") is not None and len(pred["labels"]) > 0:
        n = len(pred["labels"])
        b, e = int(pred["label_splits"][query]), int(pred["label_splits"][query + 1])
        b = 0 if b < 0 else n if b > n else b
        e = 0 if e < 0 else n if e > n else e
        if e > b:
            allowed = set(int(x) for x in pred["labels"][b:e])
            if int(pred["label_of_row"][row]) not in allowed:
                return False
    lo, hi = pred.get("value_lo"), pred.get("value_hi")
    if lo is not None or hi is not None:
        v = float(np.float32(pred["value_of_row"][row]))
        if math.isnan(v):
            return False
        if lo is not None:
            x = float(np.float32(lo[query]))
            if math.isnan(x) or not x <= v:
                return False
        if hi is not None:
            x = float(np.float32(hi[query]))
            if math.isnan(x) or not v <= x:
                return False
    ta, ty, tn = pred.get("tags_all"), pred.get("tags_any"), pred.get("tags_none")
    if ta is not None or ty is not None or tn is not None:
        t = int(pred["tags_of_row"][row])
        a = 0 if ta is None else int(ta[query])
        y = 0 if ty is None else int(ty[query])
        z = 0 if tn is None else int(tn[query])
        if (t & a) != a or (y != 0 and (t & y) == 0) or (t & z) != 0:
            return False
    return True


def restate_topk(rows, n_valid, filter, pred, k, n_items, query):
    """one query's list, in plain Python -> [(position, row)] of the answer"""
    k_in = len(rows)
    n = k_in if n_valid is None else min(max(int(n_valid), 0), k_in)
    deny, exclude = filter if filter is not None else (None, None)
    banned = set() if exclude is None else set(int(r) for r in exclude[query])
    out = []
    for j in range(n):
        r = int(rows[j])
        if not 0 <= r < n_items or (deny is not None and deny[r]) or r in banned:
            continue
        if restate_passes(pred, query, r) and len(out) < k:
            out.append((j, r))
    return out
