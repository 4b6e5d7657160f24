"""Test-side model of nann_hnsw_update_device and nann_hnsw_orphan_bits (nann_amd/csrc/nann_hnsw_build.hip), restated on
hnsw_build_model.Model from include/nann_hip.h: the repair loop of hnsw_build_model.remove without the renumbering (DETACH),
then Model.insert as hnsw_build_model.append calls it (RE-INSERT).  Shared by test_index_update_model_cpu.py and
test_index_update_gpu.py; nothing under nann_amd/ imports it.

dist is the distance matrix of the table AS THE CALL SEES IT: the marked rows already hold their new embeddings.  The detach phase
reads distances among staying nodes only, which the refresh did not change.

WRONG are test-only switches, one per rule of the update, that make the model wrong the way the host code could be; the CPU test
shows that each changes the arrays of some case."""
import numpy as np

import hnsw_build_model as HM

WRONG = ("no_one_hop",        # the pool is the row's staying entries alone
         "entry_among_all",   # the entry point is chosen among all nodes, marked ones included
         "build_batch_cap")   # batch_cap is the build's (unbounded), not ceil(n_marked / 64)


def update(dist, d, levels, adj0, adj_up, mask, M, ef_construction=40, keep_pruned=False, metric="l2", mutant=None, wrong=None):
    """mask: bool[n], True = the row is refreshed.  -> the new arrays (row numbers unchanged), counters and stats {rows repaired,
    level-0 rows of staying nodes that came out of the detach empty, rows whose pool exceeded 64, rows updated}"""
    assert wrong is None or wrong in WRONG, wrong
    mask = np.asarray(mask, bool)
    m = HM.Model(dist, d, levels, M, ef_construction, keep_pruned, metric, mutant)
    m.load(np.asarray(adj0), np.asarray(adj_up), m.n)
    old = [[list(r) for r in rows] for rows in m.row]
    gone = mask.tolist()
    marked = [i for i in range(m.n) if gone[i]]
    staying = [i for i in range(m.n) if not gone[i]]
    assert staying, "every row marked: that is a build"
    stats = [0, 0, 0, len(marked)]
    # ---- detach
    for p in marked:
        m.row[p] = [[] for _ in range(m.levels[p])]
    for p in staying:
        Dp = m.D[p]
        for level, row in enumerate(old[p]):
            if not any(gone[e] for e in row):
                m.counters["copied"] += 1  # slot for slot: the row stays as it was loaded
                continue
            pool = {e for e in row if not gone[e]}
            if wrong != "no_one_hop":
                for r in row:
                    if gone[r]:
                        pool.update(f for f in old[r][level] if not gone[f])  # one hop
            pool.discard(p)
            cands = sorted(pool, key=lambda v: m.key(Dp[v], v))
            del cands[HM.MAX_POOL:]
            out = m.select(p, cands, m.cap(level))
            stats[0] += 1
            stats[1] += level == 0 and not out
            stats[2] += len(pool) > HM.MAX_POOL
            m.row[p][level] = out
    m.counters["repaired"], m.counters["pool_over_64"] = stats[0], stats[2]
    # ---- re-insert
    if marked:
        among = range(m.n) if wrong == "entry_among_all" else staying
        entry = max(among, key=lambda i: (m.levels[i], -i))  # the lowest id among the staying nodes with the most levels
        order = sorted(marked, key=lambda i: -m.levels[i])   # stable: ascending id inside a level count
        cap = 1 << 31 if wrong == "build_batch_cap" else max(1, -(-len(marked) // HM.APPEND_DIV))
        m.insert(order, 0, len(staying), entry, m.levels[entry], cap)
    res = HM._finish(m)
    res["stats"] = np.array(stats, np.int64)
    return res


def orphans(adj0):
    """nann_hnsw_orphan_bits: the rows whose level-0 row is empty or that no level-0 row names, ascending; entries outside
    [0, n) are skipped"""
    valid = (adj0 >= 0) & (adj0 < len(adj0))
    return np.nonzero(~valid.any(1) | ~np.isin(np.arange(len(adj0)), adj0[valid]))[0]


def self_hits(dist, d, levels, adj0, adj_up, M, rows, metric="l2"):
    """how many of `rows` a beam search for the row's own embedding returns first (the row, or one at no greater distance): a
    descent from the entry point with ef = 1, then ef = 40 on level 0"""
    m = HM.Model(dist, d, levels, M, 40, False, metric)
    m.load(np.asarray(adj0), np.asarray(adj_up), m.n)
    entry = max(range(m.n), key=lambda i: (m.levels[i], -i))
    hits = 0
    for r in map(int, rows):
        at = entry
        for level in range(m.levels[entry] - 1, 0, -1):
            at = m.search(r, at, level, 1)[0]
        first = m.search(r, at, 0, 40)[0]
        hits += first == r or m.D[r][first] <= m.D[r][r]
    return hits
