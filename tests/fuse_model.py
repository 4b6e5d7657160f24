"""Test-side model of the fused top-k (nann_fuse_topk, include/nann_hip.h), written from the words of the contract and not from
the kernel: numpy (`model`, what the device tests compare against) and a plain Python restatement with a dict (`restate`, what
test_fuse_cpu.py holds the numpy model to).  Nothing under nann_amd/ imports it.

A user brings n_lists lists of k_in (score, row) entries; entry p = l * k_in + j is VALID iff j < clamp(n_valid[l], 0, k_in) and
0 <= row < n_items.  Within one list a row counts once, at its lowest valid j, and that j is its rank.  A list that contains a
row adds one term to the row's fused score -- w * s, w * (s - lo_l), w * ((s - lo_l) / (hi_l - lo_l)) or w / (rrf_c + (j + 1))
-- every step one f32 operation, the terms added to +0.0f in ascending l.  The answer: the distinct valid rows, taken in
ascending order of their first p, in TopKV2 order of the fused score -- descending, ties -> the lower first p -- cut at k; zeros
behind.  Every f32 step is taken on np.float32 values (arrays of them where a list is handled at once: the same IEEE operation
per element), so the bits are the contract's."""
import numpy as np

from union_model import MAX_IN, score_key  # noqa: F401  (the limit and the key are the union's)

MAX_LISTS = 64  # NANN_FUSE_MAX_LISTS
SUM, SUM_FLOOR, MINMAX, RRF = 0, 1, 2, 3
MODES = {"sum": SUM, "sum_floor": SUM_FLOOR, "minmax": MINMAX, "rrf": RRF}
F = np.float32


def _weights_of(weights, u, n_lists):
    """the n_lists weights of user u: None -> 1.0f, 1-D per call, 2-D per user"""
    if weights is None:
        return np.ones(n_lists, F)
    w = np.asarray(weights, F)
    return w if w.ndim == 1 else w[u]


def _terms(mode, w, s, j, lo, hi, rrf_c):
    """the terms of one list's counting entries (arrays over them), each step a single f32 operation"""
    with np.errstate(all="ignore"):
        if mode == SUM:
            return (w * s).astype(F)
        if mode == SUM_FLOOR:
            return (w * (s - lo).astype(F)).astype(F)
        if mode == MINMAX:
            span = F(hi - lo)
            quot = (s - lo).astype(F) / span if hi != lo else np.ones(len(s), F)
            return (w * quot.astype(F)).astype(F)
        if mode == RRF:
            return (w / (F(rrf_c) + (j + 1).astype(F)).astype(F)).astype(F)
    raise AssertionError(mode)


def fuse_user(scores, rows, n_valid, n_items, mode, w, rrf_c=60.0):
    """one user: scores f32[n_lists, k_in], rows i32[n_lists, k_in], n_valid i32[n_lists] or None, w f32[n_lists] -> (row,
    fused f32, mask u64, first p) arrays over the distinct valid rows in ascending first p"""
    scores, rows = np.asarray(scores, F), np.asarray(rows, np.int64)
    n_lists, k_in = scores.shape
    nv = np.full(n_lists, k_in, np.int64) if n_valid is None else np.clip(np.asarray(n_valid, np.int64), 0, k_in)
    valid = (np.arange(k_in)[None, :] < nv[:, None]) & (rows >= 0) & (rows < n_items)
    flat = rows.reshape(-1)
    pos = np.flatnonzero(valid.reshape(-1))
    distinct, first_at = np.unique(flat[pos], return_index=True)  # (the first occurrence in ascending p)
    first = pos[first_at]
    acc = np.zeros(len(distinct), F)  # +0.0f
    mask = np.zeros(len(distinct), np.uint64)
    for l in range(n_lists):
        js = np.flatnonzero(valid[l])
        if not len(js):
            continue
        folded = scores[l, js] + F(0.0)  # -0 read as +0
        lo, hi = F(folded.min()), F(folded.max())
        in_list, at = np.unique(rows[l, js], return_index=True)  # a row counts once, at its lowest valid j
        j = js[at]
        slot = np.searchsorted(distinct, in_list)
        acc[slot] = (acc[slot] + _terms(mode, F(w[l]), scores[l, j], j, lo, hi, rrf_c)).astype(F)
        mask[slot] |= np.uint64(1) << np.uint64(l)
    order = np.argsort(first, kind="stable")
    return distinct[order], acc[order], mask[order], first[order]


def model(scores, rows, n_valid, n_items, k, mode, weights=None, rrf_c=60.0, item_ids=None):
    """scores f32[n_users, n_lists, k_in], rows i32 the same, n_valid i32[n_users, n_lists] or None, weights None / f32[n_lists]
    / f32[n_users, n_lists] -> dict of index i32, scores f32, lists u64, item_ids i64 (with item_ids), each [n_users, k], and
    n_out i32[n_users]"""
    scores, rows = np.asarray(scores, F), np.asarray(rows, np.int32)
    n_users, n_lists, k_in = scores.shape
    assert n_lists <= MAX_LISTS
    k = max(int(k), 0)
    out = {"index": np.zeros((n_users, k), np.int32), "scores": np.zeros((n_users, k), F),
           "lists": np.zeros((n_users, k), np.uint64), "n_out": np.zeros(n_users, np.int32)}
    if item_ids is not None:
        out["item_ids"] = np.zeros((n_users, k), np.int64)
    for u in range(n_users):
        r, fused, mask, first = fuse_user(scores[u], rows[u], None if n_valid is None else np.asarray(n_valid)[u], n_items, mode,
                                          _weights_of(weights, u, n_lists), rrf_c)
        # TopKV2 over the rows in ascending first p: score descending through the key, ties -> the lower first p
        top = np.lexsort((first, -score_key(fused).astype(np.int64)))[:k]
        m = len(top)
        out["n_out"][u] = m
        out["index"][u, :m] = r[top]
        out["scores"][u, :m] = fused[top]
        out["lists"][u, :m] = mask[top]
        if item_ids is not None:
            out["item_ids"][u, :m] = np.asarray(item_ids, np.int64)[r[top]]
    return out


def restate(scores, rows, n_valid, n_items, k, mode, w, rrf_c=60.0):
    """one user, in plain Python with a dict -> [(row, fused np.float32, mask int)] of the answer.  scores / rows: lists of
    lists, w: a list of n_lists weights.  The f32 steps are np.float32 scalar operations, so the bits can be compared."""
    n_lists, k_in = len(scores), len(scores[0]) if len(scores) else 0
    fused = {}  # row -> [score, mask, first p]; a dict keeps insertion order = ascending first p
    with np.errstate(all="ignore"):
        for l in range(n_lists):
            count = k_in if n_valid is None else min(max(int(n_valid[l]), 0), k_in)
            entries = [(j, int(rows[l][j]), F(scores[l][j])) for j in range(count) if 0 <= int(rows[l][j]) < n_items]
            if not entries:
                continue
            lo = hi = entries[0][2] + F(0.0)
            for _, _, s in entries:
                lo = s + F(0.0) if s < lo else lo
                hi = s + F(0.0) if s > hi else hi
            seen = set()
            for j, r, s in entries:
                if r not in fused:
                    fused[r] = [F(0.0), 0, l * k_in + j]
                if r in seen:
                    continue
                seen.add(r)
                wl = F(w[l])
                if mode == SUM:
                    term = wl * s
                elif mode == SUM_FLOOR:
                    term = wl * F(s - lo)
                elif mode == MINMAX:
                    term = wl * (F(F(s - lo) / F(hi - lo)) if hi != lo else F(1.0))
                else:
                    term = wl / F(F(rrf_c) + F(j + 1))
                fused[r][0] = F(fused[r][0] + F(term))
                fused[r][1] |= 1 << l
    ranked = sorted(fused.items(), key=lambda e: float(e[1][0]), reverse=True)  # (stable; reverse keeps the order of equals;
    return [(r, s, m) for r, (s, m, _) in ranked[:max(k, 0)]]                  #  Python compares -0.0 == 0.0)
