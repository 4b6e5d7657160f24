"""Shared by test_index_build_ip.py (CPU) and test_index_build_ip_gpu.py: the corpus on which an L2-linked graph is a poor
structure to search by inner product -- clustered rows whose norms vary by 16x (ip_reference.scaled_rows), queries near
unscaled rows -- the brute-force truth under the inner product, and recall of the serving schedule restated in
ip_reference.py.  Everything is computed once per (n, d, dtype) and left unchanged."""
import numpy as np

import ip_reference as R

NQ, K, M, EF_CONSTRUCTION, SEED = 64, 50, 32, 40, 9
_CACHE = {}


def corpus(n, d, dtype="f16"):
    """-> dict(rows: the table in its dtype (f16 array | bf16 bit patterns), wide: its f32 widening, q f32[64, d])"""
    key = (n, d, dtype)
    if key not in _CACHE:
        from nann_amd import synth
        x0 = synth.make_corpus(n, d, n_clusters=16, noise=1.0)[0].astype(np.float32)
        x = R.scaled_rows(x0, 7)
        rows = R.to_bf16_bits(x) if dtype == "bf16" else x.astype(np.float16)
        wide = R.widen(rows)
        rng = np.random.default_rng(3)
        q = (x0[rng.integers(0, n, NQ)] + rng.normal(0, 0.5, (NQ, d))).astype(np.float32)
        _CACHE[key] = {"rows": rows, "wide": wide, "q": q}
    return _CACHE[key]


def host_truth(c):
    """brute force on the host, in the canonical order -> (scores f32[64, n], top-50 rows i64[64, 50]); kept with the corpus"""
    if "truth" not in c:
        c["truth_scores"] = np.stack([R.ip_scores(c["q"][b], c["wide"]) for b in range(NQ)])
        c["truth"] = np.stack([R.topk_stable(c["truth_scores"][b], K) for b in range(NQ)])
    return c["truth_scores"], c["truth"]


def both_signs(scores):
    """the order-preserving key of the device builder is exercised only where distances take both signs"""
    return bool((scores < 0).any() and (scores > 0).any())


def level_topn(n_enter):
    return [min(16, int(n_enter)), 64, 64, 64, 64, K]


def recall(truth, got, status):
    """recall@K over ALL queries: a query with non-zero status counts as zero hits"""
    hits = sum(len(set(truth[b].tolist()) & set(np.asarray(got[b]).tolist())) for b in range(len(truth)) if status[b] == 0)
    return hits / truth.size


def host_recall(c, ex):
    """(recall@50, queries that succeeded) of the serving schedule scored by inner product on the graph `ex` (an export:
    nb_values, nb_row_splits, enter_points)"""
    g = {"nb_values": [np.asarray(v) for v in ex["nb_values"]], "nb_row_splits": [np.asarray(r) for r in ex["nb_row_splits"]],
         "enter_points": np.asarray(ex["enter_points"]), "item_ids": np.arange(len(c["wide"]), dtype=np.int64)}
    t = level_topn(len(g["enter_points"]))
    got, status = [], []
    for b in range(NQ):
        q = c["q"][b]
        try:
            _, _, idx = R.py_search(g, q, t, lambda ids: R.ip_scores(q, c["wide"][np.asarray(ids)]))
            got.append(idx)
            status.append(0)
        except R.Failed as e:
            got.append(np.zeros(0, np.int32))
            status.append(e.status)
    return recall(host_truth(c)[1], got, status), int((np.asarray(status) == 0).sum())


def check_export(ex, n, m):
    """the structural rules tests/test_index_build_gpu.py asks of a build (its _check_export, restated)"""
    levels = ex["levels"]
    assert len(levels) == n
    assert (np.asarray(ex["enter_points"]) == np.nonzero(levels > 2)[0]).all()
    for level, cap in ((0, 2 * m), (1, m)):
        v, rs = np.asarray(ex["nb_values"][level]), np.asarray(ex["nb_row_splits"][level])
        assert v.dtype == np.int64 and rs.dtype == np.int64 and len(rs) == n + 1
        deg = np.diff(rs)
        assert rs[0] == 0 and rs[-1] == len(v) and deg.min() >= 0 and deg.max() <= cap
        assert len(v) and v.min() >= 0 and v.max() < n
        rows = np.repeat(np.arange(n), deg)
        assert (v != rows).all(), "self loop"
        assert len(np.unique(rows * n + v)) == len(v), "a link twice in one row"
        assert (deg[levels <= level] == 0).all(), "a row for a node that is absent on this level"  # build_hnsw_index.py:53
        assert (levels[v] > level).all(), "a link to a node that is absent on this level"
    assert (np.diff(np.asarray(ex["nb_row_splits"][0])) > 0).mean() > 0.999  # every node (but the first) found neighbours
