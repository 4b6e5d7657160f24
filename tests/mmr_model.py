"""Test-side model of the MMR re-ranking (nann_mmr_topk, include/nann_hip.h "diversified results"), written from the contract's
words in numpy; nothing under nann_amd/ imports it.  Similarities come from ip_reference's canonical l2_scores / ip_scores over
widen()ed rows, keys are the `s + 0.0f` monotone map, and every product and difference is one np.float32 operation."""
import numpy as np

from ip_reference import ip_scores, l2_scores, widen


def key(x):
    """TopKV2's order as one integer: x + 0.0f, then the monotone u32 map of the bits (larger value -> larger key)"""
    u = int((np.float32(x) + np.float32(0.0)).view(np.uint32))
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def keys_of(x):
    """key() of every element of an f32 array, as i64"""
    u = (np.asarray(x, np.float32) + np.float32(0.0)).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)


def clamp_lambda(x):
    """a per-query lambda as the contract reads it: !(x >= 0) ? 0 : (x > 1 ? 1 : x)"""
    x = np.float32(x)
    if not (x >= np.float32(0.0)):
        return np.float32(0.0)
    return np.float32(1.0) if x > np.float32(1.0) else x


def valid_entries(scores, rows, n_valid, n_items, deny=None, exclude=None):
    """positions j of the valid entries of one query, ascending"""
    k_in = len(rows)
    n = k_in if n_valid is None else max(0, min(int(n_valid), k_in))
    gone = set() if exclude is None else {int(r) for r in exclude}
    out = []
    for j in range(n):
        r = int(rows[j])
        if not (0 <= r < n_items) or not np.isfinite(scores[j]):
            continue
        if deny is not None and deny[r]:
            continue
        if r in gone:
            continue
        out.append(j)
    return out


def select(scores, rows, n_valid, table_f32, lam, sim, k, deny=None, exclude=None):
    """one query -> [(j, v_j at the pick)] in pick order.  table_f32: widen() of the index's rows; sim: "l2" | "ip" """
    score_fn = ip_scores if sim == "ip" else l2_scores
    scores = np.asarray(scores, np.float32)
    a = np.float32(lam)
    b = np.float32(1.0) - a
    cand = np.asarray(valid_entries(scores, rows, n_valid, len(table_f32), deny, exclude), np.int64)  # ascending j
    n_pick = min(int(k), len(cand))
    if n_pick == 0:
        return []
    X = table_f32[np.asarray(rows)[cand].astype(np.int64)]  # the candidates' rows
    r = (a * scores[cand]).astype(np.float32)
    v = r.copy()
    p = np.zeros(len(cand), np.float32)
    open_ = np.ones(len(cand), bool)
    picks = []
    for step in range(n_pick):
        keys = keys_of(v)
        keys[~open_] = -1
        t = int(np.argmax(keys))  # (the first of the greatest: ties to the lower j)
        picks.append((int(cand[t]), v[t]))
        open_[t] = False
        if step + 1 == n_pick:
            break
        s = score_fn(X[t], X).astype(np.float32)
        p = s if step == 0 else np.where(s > p, s, p)
        v = (r - (b * p).astype(np.float32)).astype(np.float32)
    return picks


def model(scores, rows, n_valid, table, lam, sim, k, lams=None, item_ids=None, deny=None, exclude=None, status=None):
    """A batch -> dict of index i32, scores f32, mmr f32, pos i32, item_ids i64 [B, k] and n_out i32 [B], zeros behind n_out.
    table: the index's rows (f16 / f32 arrays or uint16 bf16 bits); lams: per-query lambdas, clamped as the contract says;
    exclude: one list of rows per query; status: a non-zero word empties the query."""
    rows = np.asarray(rows, np.int32)
    scores = np.asarray(scores, np.float32)
    B, k = rows.shape[0], int(k)
    T = widen(table)
    out = {"index": np.zeros((B, k), np.int32), "scores": np.zeros((B, k), np.float32), "mmr": np.zeros((B, k), np.float32),
           "pos": np.zeros((B, k), np.int32), "item_ids": np.zeros((B, k), np.int64), "n_out": np.zeros(B, np.int32)}
    for i in range(B):
        nv = None if n_valid is None else int(n_valid[i])
        if status is not None and int(status[i]) != 0:
            nv = 0
        a = np.float32(lam) if lams is None else clamp_lambda(lams[i])
        picks = select(scores[i], rows[i], nv, T, a, sim, k, deny, None if exclude is None else exclude[i])
        out["n_out"][i] = len(picks)
        for n, (j, vj) in enumerate(picks):
            out["index"][i, n] = rows[i, j]
            out["scores"][i, n] = scores[i, j]
            out["mmr"][i, n] = vj
            out["pos"][i, n] = j
            if item_ids is not None:
                out["item_ids"][i, n] = item_ids[rows[i, j]]
    return out
