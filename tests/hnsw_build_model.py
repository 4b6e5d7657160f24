"""Test-side model of the device HNSW builder (nann_amd/csrc/nann_hnsw_build.hip): build, append and remove restated as plain
sequential Python over ids and one distance matrix -- no lanes, no shuffles, no sorting networks; every order is a sort by key.
Restated from include/nann_hip.h (nann_hnsw_build_device*, nann_hnsw_append_device*, nann_hnsw_remove_*), DESIGN.md 4.6 and
Malkov & Yashunin alg. 1-4.  Shared by test_index_build_model_cpu.py and test_index_build_exact_gpu.py; nothing under nann_amd/
imports it.

The arrays the device calls write are a pure function of (rows, levels, M, ef_construction, keep_pruned, metric): back-link
pairs go through a stable sort, one wavefront handles a target, distances are one fixed tree of fmaf and adds.  So the model is
held to them entry for entry.

Distances: one matrix per (corpus, metric), in the canonical order tests/ip_reference.py restates (per chunk of 8 elements
acc = fmaf(., ., acc) from +0, the d / 8 partials added in the xor butterfly); L2 dist = sum, IP dist = 0 - <a, b>.  16-bit
rows are widened exactly.  The tree is symmetric in its two rows, bit for bit, so the matrix is built once and indexed.

Order: everything is ordered by the key (distance with -0 taken as +0, then id), ascending -- what hb_key encodes.

MUTANTS are test-only switches, one per rule, that make the model subtly wrong the way a kernel could be; the CPU tests show that
each changes the arrays of some tested case, i.e. that the comparison with the device would notice it."""
import struct

import numpy as np

import ip_reference as R

MUTANTS = ("dominate_le",        # <= in the domination test
           "gpw_only",           # kept members beyond the first GPW(d) ignored by the domination test
           "tie_high_id",        # ties to the higher id
           "backlink_reverse",   # a target's incoming back-links in reverse batch order
           "drop_new_at_64",     # at cap 64 the new link is dropped, not the farthest of the 65
           "ef_39",              # beam of ef_construction - 1
           "batch_third",        # a batch is at most a third of the graph, not a quarter
           "pool_uncut",         # the repair pool is not cut to its 64 nearest
           "ip_raw_bits",        # IP keys ordered by the raw f32 bit pattern, as L2's non-negative distances may be
           "beam_expanded_last") # in the beam, at equal distance, expanded entries behind the others whatever their ids

COUNTERS = ("select_over_gpw", "reselect", "reselect_cap64", "ties", "zero_dist", "levels_ge3", "batches_gt1", "pool_over_64",
            "select_fill", "batches_of_one", "taller_than_entry", "repaired", "copied", "neg_dist", "pos_dist")

MAX_BATCH = 16384
MAX_POOL = 64
APPEND_DIV = 64


def gpw(d):
    """kept members the device's selection compares a candidate with per step"""
    return 64 // (d // 8)


def distance_matrix(rows, metric):
    """f32[n, n] distances of all pairs in the canonical order; rows: f16 array or bf16 bit patterns (uint16)"""
    x = R.widen(rows)
    n, d = x.shape
    L = d // 8
    xs = x.reshape(n, L, 8)
    out = np.empty((n, n), np.float32)
    lanes = np.arange(L)
    step = max(1, (1 << 20) // (n * L))
    for i0 in range(0, n, step):  # rows [i0, i0 + step) against rows [i0, n): the tree is symmetric, the rest is mirrored
        a_blk, b_blk = xs[i0:i0 + step], xs[i0:]
        acc = np.zeros((len(a_blk), len(b_blk), L), np.float32)
        for k in range(8):
            a = np.broadcast_to(a_blk[:, None, :, k], acc.shape)
            b = np.broadcast_to(b_blk[None, :, :, k], acc.shape)
            if metric == "l2":
                t = (a - b).astype(np.float32)
                acc = R.fma32(t, t, acc)
            else:
                acc = R.fma32(a, b, acc)
        s = 1
        while s < L:
            acc = (acc + acc[:, :, lanes ^ s]).astype(np.float32)
            s *= 2
        out[i0:i0 + step, i0:] = acc[:, :, 0]
        out[i0:, i0:i0 + step] = acc[:, :, 0].T
    return out if metric == "l2" else (np.float32(0.0) - out).astype(np.float32)


def _f32_bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def up_rows_of(levels):
    """the prefix rule: first upper row of every node (-1: one level), and the number of upper rows"""
    lv = np.asarray(levels, np.int64)
    first = np.cumsum(lv - 1) - (lv - 1)
    return np.where(lv > 1, first, -1).astype(np.int32), int((lv - 1).sum())


class Model:
    """The graph as lists: row[node][level] = the ids of the row's dense prefix, in slot order."""

    def __init__(self, dist, d, levels, M, ef_construction=40, keep_pruned=False, metric="l2", mutant=None):
        assert mutant is None or mutant in MUTANTS, mutant
        self.D = dist.tolist() if isinstance(dist, np.ndarray) else dist  # f32 values as Python floats: exact
        self.d, self.M, self.metric, self.mutant = int(d), int(M), metric, mutant
        self.keep_pruned = bool(keep_pruned)
        self.ef = int(ef_construction) - (1 if mutant == "ef_39" else 0)
        self.levels = [int(v) for v in levels]
        self.n = len(self.levels)
        self.row = [[[] for _ in range(lv)] for lv in self.levels]
        self.batch_of = [-1] * self.n        # the batch that inserted a node (-1: it was there before the batches)
        self.touched = {}                    # (node, level) -> the last batch that wrote the row
        self.n_batches = 0
        self.counters = dict.fromkeys(COUNTERS, 0)

    # ---- order ----
    def key(self, dist, i):
        dist = dist + 0.0
        if self.mutant == "tie_high_id":
            return (dist, -i)
        if self.mutant == "ip_raw_bits" and self.metric == "ip":
            return (_f32_bits(dist), i)
        return (dist, i)

    def cap(self, level):
        return 2 * self.M if level == 0 else self.M

    # ---- alg. 4 ----
    def select(self, base, cands, cap):
        """cands ascending by key to base -> the row: the kept candidates (and, with keep_pruned, the nearest discarded ones up to
        cap) in the candidates' order"""
        D, Db, ctr = self.D, self.D[base], self.counters
        le = self.mutant == "dominate_le"
        limit = gpw(self.d) if self.mutant == "gpw_only" else None
        kept, flag = [], [False] * len(cands)
        over = False
        for i, c in enumerate(cands):
            if len(kept) >= cap:
                break
            dc, Dc = D[c][base], D[c]
            over = over or len(kept) > gpw(self.d)
            pool = kept if limit is None else kept[:limit]
            if le:
                dominated = any(Dc[s] <= dc for s in pool)
            else:
                dominated = any(Dc[s] < dc for s in pool)
            if not dominated:
                kept.append(c)
                flag[i] = True
        ctr["select_over_gpw"] += over
        ctr["ties"] += sum(1 for a, b in zip(cands, cands[1:]) if Db[a] == Db[b])
        ctr["zero_dist"] += sum(1 for c in cands if Db[c] == 0.0)
        ctr["neg_dist"] += sum(1 for c in cands if Db[c] < 0.0)
        ctr["pos_dist"] += sum(1 for c in cands if Db[c] > 0.0)
        if self.keep_pruned and len(kept) < cap:
            free = cap - len(kept)
            for i in range(len(cands)):
                if free == 0:
                    break
                if not flag[i]:
                    flag[i] = True
                    free -= 1
                    ctr["select_fill"] += 1
        return [c for i, c in enumerate(cands) if flag[i]]

    # ---- alg. 2 ----
    def search(self, u, entry, level, ef):
        """-> the beam's ids, best first.  Rows are read as they stand: the caller writes a batch's rows after its searches."""
        Du, key = self.D[u], self.key
        order = (lambda e: (e[0], e[3], e[1])) if self.mutant == "beam_expanded_last" else (lambda e: (e[0], e[1]))
        k = key(Du[entry], entry)
        beam = [[k[0], k[1], entry, False]]
        visited = {entry}
        while True:
            cur = next((e for e in beam if not e[3]), None)
            if cur is None:
                break
            cur[3] = True
            for v in self.row[cur[2]][level]:
                if v not in visited:          # an id that fell out of the beam stays visited
                    visited.add(v)
                    k = key(Du[v], v)
                    beam.append([k[0], k[1], v, False])
            beam.sort(key=order)
            del beam[ef:]
        return [e[2] for e in beam]

    # ---- Faiss add_link ----
    def backlink(self, target, level, sources):
        row, cap, Dt, key = self.row[target][level], self.cap(level), self.D[target], self.key
        for s in sources:
            if len(row) < cap:
                row.append(s)
                continue
            self.counters["reselect"] += 1
            cands = sorted(row + [s], key=lambda v: key(Dt[v], v))
            if len(cands) > MAX_POOL:         # cap 64: the farthest of the 65 is dropped before the walk
                self.counters["reselect_cap64"] += 1
                if self.mutant == "drop_new_at_64":
                    cands.remove(s)
                else:
                    del cands[MAX_POOL:]
            row[:] = self.select(target, cands, cap)

    # ---- alg. 1, batched ----
    def insert(self, order, pos0, base, entry, T, batch_cap):
        levels, ctr = self.levels, self.counters
        div = 3 if self.mutant == "batch_third" else 4
        pos = pos0
        while pos < len(order):
            lv = levels[order[pos]]
            limit = 1 if lv > T else min(MAX_BATCH, batch_cap, max(1, (base + pos) // div))
            end = pos
            while end < len(order) and end - pos < limit and levels[order[end]] == lv:
                end += 1
            nodes = order[pos:end]
            b = self.n_batches
            self.n_batches += 1
            ctr["batches_gt1" if len(nodes) > 1 else "batches_of_one"] += 1
            ctr["taller_than_entry"] += lv > T
            for u in nodes:
                self.batch_of[u] = b
            entries = [entry] * len(nodes)
            for level in range(T - 1, -1, -1):
                link = level <= lv - 1
                rows = []
                for bi, u in enumerate(nodes):
                    beam = self.search(u, entries[bi], level, self.ef if link else 1)
                    entries[bi] = beam[0]
                    if link:
                        rows.append(self.select(u, beam, self.cap(level)))
                if not link:
                    continue
                incoming = {}
                for u, kept in zip(nodes, rows):  # batch position order
                    self.row[u][level] = list(kept)
                    self.touched[(u, level)] = b
                    for t in kept:
                        incoming.setdefault(t, []).append(u)
                for t, sources in incoming.items():
                    self.backlink(t, level, sources[::-1] if self.mutant == "backlink_reverse" else sources)
                    self.touched[(t, level)] = b
            if lv > T:
                T, entry = lv, nodes[0]
            pos = end

    def insertion_order(self, first, last):
        return sorted(range(first, last), key=lambda i: -self.levels[i])  # stable: ascending id inside a level count

    # ---- arrays ----
    def arrays(self):
        """-> adj0 i32[n, 2M], up_row i32[n], adj_up i32[max(upper rows, 1), M] as the device calls leave them (-1: empty slot)"""
        M = self.M
        up_row, n_up = up_rows_of(self.levels)
        adj0 = np.full((self.n, 2 * M), -1, np.int32)
        adj_up = np.full((max(n_up, 1), M), -1, np.int32)
        for i, rows in enumerate(self.row):
            adj0[i, :len(rows[0])] = rows[0]
            for l in range(1, len(rows)):
                adj_up[up_row[i] + l - 1, :len(rows[l])] = rows[l]
        return adj0, up_row, adj_up

    def load(self, adj0, adj_up, n_old):
        """the rows of nodes [0, n_old) from a graph's arrays (dense prefixes)"""
        up_row, _ = up_rows_of(self.levels)
        for i in range(n_old):
            for l in range(self.levels[i]):
                r = adj0[i] if l == 0 else adj_up[up_row[i] + l - 1]
                r = [int(v) for v in r]
                self.row[i][l] = r[:r.index(-1)] if -1 in r else r


def _finish(m):
    m.counters["levels_ge3"] = sum(1 for lv in m.levels if lv >= 3)
    adj0, up_row, adj_up = m.arrays()
    return {"adj0": adj0, "up_row": up_row, "adj_up": adj_up, "counters": dict(m.counters), "batch_of": np.array(m.batch_of),
            "touched": dict(m.touched), "n_batches": m.n_batches}


def build(dist, d, levels, M, ef_construction=40, keep_pruned=False, metric="l2", mutant=None):
    """nann_hnsw_build_device_metric.  dist: distance_matrix(rows, metric) (or its .tolist()), d: the rows' width"""
    m = Model(dist, d, levels, M, ef_construction, keep_pruned, metric, mutant)
    order = m.insertion_order(0, m.n)
    # order[0] is the entry point: it goes in without links
    m.insert(order, 1, 0, order[0], m.levels[order[0]], 1 << 31)
    return _finish(m)


def append(dist, d, levels, n_old, adj0, adj_up, M, ef_construction=40, keep_pruned=False, metric="l2", mutant=None):
    """nann_hnsw_append_device_metric: levels and dist over n_old + n_new nodes, adj0 / adj_up the old graph's arrays (rows of
    the old nodes are read from their heads)"""
    m = Model(dist, d, levels, M, ef_construction, keep_pruned, metric, mutant)
    m.load(np.asarray(adj0), np.asarray(adj_up), n_old)
    n_new = m.n - n_old
    if n_new:
        entry = max(range(n_old), key=lambda i: (m.levels[i], -i))  # the lowest id among the nodes with the most levels
        m.insert(m.insertion_order(n_old, m.n), 0, n_old, entry, m.levels[entry], max(1, -(-n_new // APPEND_DIV)))
    return _finish(m)


def remove(dist, d, levels, adj0, adj_up, mask, M, keep_pruned=False, metric="l2", mutant=None):
    """nann_hnsw_remove_count + nann_hnsw_remove_device.  mask: bool[n], True = the row leaves.  -> the new arrays, new levels,
    kept_rows and stats {rows repaired, level-0 rows that came out empty, rows whose pool exceeded 64, survivors}"""
    mask = np.asarray(mask, bool)
    old = Model(dist, d, levels, M, 40, keep_pruned, metric, mutant)
    old.load(np.asarray(adj0), np.asarray(adj_up), old.n)
    kept_rows = np.nonzero(~mask)[0]
    new_id = {int(o): i for i, o in enumerate(kept_rows)}
    new = Model(old.D, d, [old.levels[o] for o in kept_rows], M, 40, keep_pruned, metric, mutant)
    new.counters = old.counters
    gone = mask.tolist()
    stats = [0, 0, 0, len(kept_rows)]
    for p in map(int, kept_rows):
        Dp = old.D[p]
        for level, row in enumerate(old.row[p]):
            if not any(gone[e] for e in row):
                out = row  # copied slot for slot
                old.counters["copied"] += 1
            else:
                pool = {e for e in row if not gone[e]}
                for r in row:
                    if gone[r]:
                        pool.update(f for f in old.row[r][level] if not gone[f])  # one hop
                pool.discard(p)
                cands = sorted(pool, key=lambda v: old.key(Dp[v], v))
                if old.mutant != "pool_uncut":
                    del cands[MAX_POOL:]
                out = old.select(p, cands, old.cap(level))
                stats[0] += 1
                stats[1] += level == 0 and not out
                stats[2] += len(pool) > MAX_POOL
            new.row[new_id[p]][level] = [new_id[e] for e in out]
    old.counters["repaired"], old.counters["pool_over_64"] = stats[0], stats[2]
    res = _finish(new)
    res.update(levels=np.array(new.levels, np.int32), kept_rows=kept_rows.astype(np.int32), stats=np.array(stats, np.int64))
    return res
