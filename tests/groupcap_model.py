"""Test-side model of the group cap (nann_group_cap_topk, include/nann_hip.h), written from the words of the contract and not
from the kernel: numpy, vectorised (`model`, what the device tests compare against), a plain Python restatement with a dict and
a loop (`restate`, what test_groupcap_cpu.py holds the numpy model to), and a model of the kernel's PARALLEL SCHEME (`scheme`:
the 16 chunks of 64 entries, the slot table, the per-(slot, chunk) byte counts and the compaction), which the same test holds
to the contract model.  Nothing under nann_amd/ imports it.

A query brings a ranked list of k_in (row, score) entries; entry j is VALID iff j < clamp(n_valid, 0, k_in), 0 <= row < n_items
and the row is not denied.  Walking the valid entries in ascending j, an entry is KEPT iff its group g = group_of_row[row] is
negative, the query is uncapped (cap <= 0), or fewer than cap valid entries before it have group g.  The answer: the first k kept
entries, order unchanged; zeros behind."""
import numpy as np

MAX_IN = 1024   # entries of the longest list
CHUNK = 64      # entries of a wavefront
SLOTS = 2048    # slots of the kernel's group table


def group_hash(g):
    """the kernel's hash of a group id, restated: the slot a group starts probing at"""
    return ((int(g) * 2654435761) & 0xFFFFFFFF) >> 21


def _valid(rows, n_valid, n_items, deny, exclude):
    """rows i64[k_in] of one query -> bool[k_in]"""
    k_in = len(rows)
    nv = k_in if n_valid is None else min(max(int(n_valid), 0), k_in)
    ok = (np.arange(k_in) < nv) & (rows >= 0) & (rows < n_items)
    if deny is not None and n_items > 0:
        ok &= ~np.asarray(deny, bool)[np.where(ok, rows, 0)]
    if exclude is not None and len(exclude):
        ok &= ~np.isin(rows, np.asarray(exclude, np.int64))
    return ok


def select(rows, n_valid, n_items, group_of_row, cap, k, deny=None, exclude=None):
    """one query -> the positions j of the answer, in order (at most k)"""
    rows = np.asarray(rows, np.int64)
    ok = _valid(rows, n_valid, n_items, deny, exclude)
    g = np.where(ok, np.asarray(group_of_row, np.int64)[np.where(ok, rows, 0)] if n_items else -1, -1)
    grouped = ok & (g >= 0)
    kept = ok.copy()
    if cap > 0 and grouped.any():
        idx = np.nonzero(grouped)[0]
        order = idx[np.argsort(g[idx], kind="stable")]            # by group, list order within a group
        gs = g[order]
        first = np.concatenate(([True], gs[1:] != gs[:-1]))
        start = np.maximum.accumulate(np.where(first, np.arange(len(gs)), 0))
        rank = np.empty(len(rows), np.int64)
        rank[order] = np.arange(len(gs)) - start                  # the entry's rank among the valid entries of its group
        kept[idx] = rank[idx] < cap
    return np.nonzero(kept)[0][:max(k, 0)]


def scheme(rows, n_valid, n_items, group_of_row, cap, k, deny=None, exclude=None):
    """one query, the way the kernel's workgroup goes about it -> positions, like select.  Chunk c holds entries 64 c .. 64 c +
    63; a group's slot comes from an open-addressing table; per[slot][c] holds the chunk's population of the slot; an entry's
    rank is the populations of the chunks before its own plus its place among the lanes of its chunk that share its slot; the
    kept entries are placed by a count per chunk and an exclusive prefix over the counts."""
    rows = np.asarray(rows, np.int64)
    n = len(rows)
    assert n <= MAX_IN
    ok = _valid(rows, n_valid, n_items, deny, exclude)
    g = np.where(ok, np.asarray(group_of_row, np.int64)[np.where(ok, rows, 0)] if n_items else -1, -1)
    keep = ok.copy()
    n_chunks = MAX_IN // CHUNK
    if cap > 0:
        tab = np.full(SLOTS, -1, np.int64)
        slot = np.full(n, -1, np.int64)
        for j in range(n):                                         # (any insertion order gives every group one slot)
            if g[j] < 0:
                continue
            h = group_hash(g[j])
            while tab[h] != -1 and tab[h] != g[j]:
                h = (h + 1) & (SLOTS - 1)
            tab[h] = g[j]
            slot[j] = h
        assert (tab >= 0).sum() <= MAX_IN                          # never more than half full
        per = np.zeros((SLOTS, n_chunks), np.uint8)
        in_chunk = np.zeros(n, np.int64)
        for c in range(n_chunks):
            lanes = np.arange(c * CHUNK, min((c + 1) * CHUNK, n))
            is_open = slot[lanes] >= 0
            rounds = 0
            while is_open.any():                                   # the slot of the lowest open lane, its sharers, their places
                s = slot[lanes[np.argmax(is_open)]]
                mine = slot[lanes] == s
                in_chunk[lanes[mine]] = np.arange(mine.sum())
                per[s, c] = mine.sum()
                is_open &= ~mine
                rounds += 1
            assert rounds <= CHUNK
        for j in range(n):
            if slot[j] >= 0:
                keep[j] = int(per[slot[j], :j // CHUNK].sum()) + in_chunk[j] < cap
    counts = np.array([keep[c * CHUNK:(c + 1) * CHUNK].sum() for c in range(n_chunks)])
    base = np.concatenate(([0], np.cumsum(counts)[:-1]))
    out = []
    for j in range(n):
        if keep[j]:
            pos = base[j // CHUNK] + keep[(j // CHUNK) * CHUNK:j].sum()
            if pos < k:
                out.append((pos, j))
    assert [p for p, _ in sorted(out)] == list(range(len(out)))    # every place taken once, none skipped
    return np.array([j for _, j in sorted(out)], np.int64)


def model(scores, rows, n_valid, n_items, group_of_row, cap, k, caps=None, item_ids=None, deny=None, exclude=None, pick=select):
    """scores f32[n_queries, k_in] or None, rows i32 the same, n_valid i32[n_queries] or None, caps i32[n_queries] or None,
    deny bool[n_items] or None, exclude: one array of rows per query or None -> dict of index i32, scores f32, item_ids i64
    (with item_ids), group i32, pos i32, each [n_queries, k], and n_out i32[n_queries]"""
    rows = np.asarray(rows, np.int32)
    n_q, k_in = rows.shape
    sc = np.zeros((n_q, k_in), np.float32) if scores is None else np.asarray(scores, np.float32)
    out = {"index": np.zeros((n_q, k), np.int32), "scores": np.zeros((n_q, k), np.float32), "group": np.zeros((n_q, k), np.int32),
           "pos": np.zeros((n_q, k), np.int32), "n_out": np.zeros(n_q, np.int32)}
    if item_ids is not None:
        out["item_ids"] = np.zeros((n_q, k), np.int64)
    for i in range(n_q):
        p = pick(rows[i], None if n_valid is None else np.asarray(n_valid)[i], n_items, group_of_row,
                 int(cap) if caps is None else int(np.asarray(caps)[i]), k, deny, None if exclude is None else exclude[i])
        m = len(p)
        out["n_out"][i] = m
        out["index"][i, :m] = rows[i, p]
        out["scores"][i, :m] = sc[i, p]                            # the entry's own bits: a NaN stays that NaN
        out["group"][i, :m] = np.asarray(group_of_row, np.int32)[rows[i, p]]
        out["pos"][i, :m] = p
        if item_ids is not None:
            out["item_ids"][i, :m] = np.asarray(item_ids, np.int64)[rows[i, p]]
    return out


def restate(rows, n_valid, n_items, group_of_row, cap, k, deny=None, exclude=None):
    """one query, in plain Python -> [(position, row, group)] of the answer"""
    k_in = len(rows)
    count = k_in if n_valid is None else min(max(int(n_valid), 0), k_in)
    banned = set() if exclude is None else set(int(r) for r in exclude)
    seen, out = {}, []
    for j in range(count):
        r = int(rows[j])
        if not 0 <= r < n_items or (deny is not None and deny[r]) or r in banned:
            continue
        g = int(group_of_row[r])
        if g >= 0 and cap > 0:
            before = seen.get(g, 0)
            seen[g] = before + 1
            if before >= cap:
                continue
        if len(out) < k:
            out.append((j, r, g))
    return out
