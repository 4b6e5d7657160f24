"""Test-side model of the union top-k (nann_union_topk, include/nann_hip.h), written from the words of the contract and not
from the kernel: numpy (`model`, what the device tests compare against) and a plain Python restatement with a dict
(`restate`, what test_union_cpu.py holds the numpy model to).  Nothing under nann_amd/ imports it.

A user brings n_lists lists of k_in (score, row) entries; entry p = l * k_in + j is VALID iff j < clamp(n_valid[l], 0, k_in) and
0 <= row < n_items.  Among the valid entries of a row the one with the largest score represents it (-0 == +0; ties -> the lowest
p).  The answer: the representatives in TopKV2 order -- score descending, ties -> the lower p -- cut at k; zeros behind."""
import numpy as np

MAX_IN = 8192  # NANN_UNION_MAX_IN


def score_key(s):
    """the monotone u32 image of f32 scores TopKV2 compares through: larger score -> larger key, -0 folded into +0"""
    s = np.ascontiguousarray(np.asarray(s, np.float32) + np.float32(0.0))
    u = s.view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def select(scores, rows, n_valid, n_items, k):
    """one user: scores f32[n_lists, k_in], rows i32[n_lists, k_in], n_valid i32[n_lists] or None -> the positions p of the
    answer, in order (at most k)"""
    scores, rows = np.asarray(scores, np.float32), np.asarray(rows, np.int64)
    n_lists, k_in = scores.shape
    nv = np.full(n_lists, k_in, np.int64) if n_valid is None else np.clip(np.asarray(n_valid, np.int64), 0, k_in)
    pos = np.arange(n_lists * k_in)
    r, key = rows.reshape(-1), score_key(scores.reshape(-1)).astype(np.int64)
    valid = (pos % max(k_in, 1) < nv[pos // max(k_in, 1)]) & (r >= 0) & (r < n_items)
    p = pos[valid]
    # the representative of a row: the first of its entries by (key descending, p ascending)
    order = p[np.lexsort((p, -key[p], r[p]))]
    reps = order[np.concatenate(([True], r[order][1:] != r[order][:-1]))] if len(order) else order
    return reps[np.lexsort((reps, -key[reps]))][:max(k, 0)]


def model(scores, rows, n_valid, n_items, k, item_ids=None):
    """scores f32[n_users, n_lists, k_in], rows i32 the same, n_valid i32[n_users, n_lists] or None -> dict of index i32,
    scores f32, item_ids i64 (with item_ids), list i32, each [n_users, k], and n_out i32[n_users]"""
    scores, rows = np.asarray(scores, np.float32), np.asarray(rows, np.int32)
    n_users, n_lists, k_in = scores.shape
    out = {"index": np.zeros((n_users, k), np.int32), "scores": np.zeros((n_users, k), np.float32),
           "list": np.zeros((n_users, k), np.int32), "n_out": np.zeros(n_users, np.int32)}
    if item_ids is not None:
        out["item_ids"] = np.zeros((n_users, k), np.int64)
    for u in range(n_users):
        p = select(scores[u], rows[u], None if n_valid is None else np.asarray(n_valid)[u], n_items, k)
        m = len(p)
        out["n_out"][u] = m
        out["index"][u, :m] = rows[u].reshape(-1)[p]
        out["scores"][u, :m] = scores[u].reshape(-1)[p]  # the representative's own bits: a -0 stays a -0
        out["list"][u, :m] = p // max(k_in, 1)
        if item_ids is not None:
            out["item_ids"][u, :m] = np.asarray(item_ids, np.int64)[out["index"][u, :m]]
    return out


def restate(scores, rows, n_valid, n_items, k):
    """one user, in plain Python -> [(row, score, list)] of the answer.  Walking the entries in ascending p and replacing a
    row's representative on a strictly larger score only keeps the lowest p among equals (Python compares -0.0 == 0.0); sorted()
    is stable, so equal scores stay in ascending p."""
    n_lists, k_in = len(scores), len(scores[0]) if len(scores) else 0
    best = {}
    for l in range(n_lists):
        count = k_in if n_valid is None else min(max(int(n_valid[l]), 0), k_in)
        for j in range(count):
            r, s = int(rows[l][j]), float(scores[l][j])
            if not 0 <= r < n_items:
                continue
            if r not in best or s > best[r][0]:
                best[r] = (s, l * k_in + j, l)
    reps = sorted(((s, p, r, l) for r, (s, p, l) in best.items()), key=lambda e: e[1])
    ranked = sorted(reps, key=lambda e: e[0], reverse=True)  # (reverse=True keeps the order of equal elements)
    return [(r, s, l) for s, p, r, l in ranked[:max(k, 0)]]
