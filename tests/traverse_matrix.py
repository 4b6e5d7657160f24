"""The workload of the traversal matrix (test_traverse_matrix_gpu.py) and its expected values, none of which come from a
device: one small host-built graph per d with its rows scaled (norms vary 16x, so L2 and the inner product rank them
differently), 24 queries, and per (d, row dtype, scorer) the reference's answer -- oracle.search_batch for L2,
ip_reference.py_search over ip_scores for the inner product -- in one layout (status, item ids, scores, rows, counters).
Shared by the GPU matrix and the CPU tests that check the workload itself (test_traverse_matrix_cpu.py, test_ip_cpu.py);
nothing under nann_amd/ imports it."""
import numpy as np

import ip_reference as R

N_ITEMS, NQ = 4000, 24
DIMS = (64, 128, 256, 512)
DTYPES = ("f16", "bf16", "f32")
SCORERS = ("l2", "ip")
TOPN = [16, 16, 24, 32, 32, 20]
TOPN_ODD = [8, 12, 16, 16, 16, 10]   # the odd requests of the per-request launches
MIN_OK = 18                          # of the 24 queries the reference must serve at least this many
_CACHE = {}


def graph(d):
    """synth.make_index(4000, d, ef=16, four clusters) built on the host + its 24 queries f32[24, d]"""
    from nann_amd import synth
    from oracle import oracle as O
    key = ("graph", d)
    if key not in _CACHE:
        g = synth.make_index(N_ITEMS, d, ef=16, seed=1234, noise=1.0, n_clusters=4)
        q = np.stack([O.user_seq_mean(s) for s in synth.make_queries(g["item_embs"], g["assign"], NQ, seed=5)])
        _CACHE[key] = (g, q)
    return _CACHE[key]


def table(d, dtype):
    """-> (the rows in the table's dtype -- f16, bf16 bit patterns (uint16) or f32 --, their f32 widening)"""
    key = ("table", d, dtype)
    if key not in _CACHE:
        x = R.scaled_rows(R.widen(graph(d)[0]["item_embs"]), seed=d)
        t = x.astype(np.float16) if dtype == "f16" else R.to_bf16_bits(x) if dtype == "bf16" else x
        _CACHE[key] = (t, R.widen(t))
    return _CACHE[key]


def level_topn_rows():
    """the int32[24, 6] input of the per-request launches: even rows TOPN, odd rows TOPN_ODD"""
    return np.asarray([TOPN if b % 2 == 0 else TOPN_ODD for b in range(NQ)], np.int32)


def py_batch(d, dtype, score_fn, topn, sel=None):
    """py_search of the queries `sel` (default: all) under score_fn (R.ip_scores / R.l2_scores), in oracle.search_batch's
    layout: (status i32[n], item ids i64[n, k], scores f32[n, k], rows i32[n, k], counters i64[n, 3, 5]); a request the
    reference fails keeps its status and zeros"""
    g, q = graph(d)
    wide = table(d, dtype)[1]
    sel = np.arange(NQ) if sel is None else np.asarray(sel)
    n, k = len(sel), topn[5]
    st, ids, sc = np.zeros(n, np.int32), np.zeros((n, k), np.int64), np.zeros((n, k), np.float32)
    rows, ctr = np.zeros((n, k), np.int32), np.zeros((n, 3, R.NUM_ROUNDS), np.int64)
    for i, b in enumerate(sel):
        try:
            ids[i], sc[i], rows[i], ctr[i] = R.py_search(g, q[b], topn, lambda r: score_fn(q[b], wide[np.asarray(r)]), counters=True)
        except R.Failed as e:
            st[i] = e.status
    return st, ids, sc, rows, ctr


def oracle_batch(d, dtype, topn, sel=None):
    """oracle.search_batch under L2 on the table in `dtype`, for the queries `sel` (default: all)"""
    from oracle import oracle as O
    g, q = graph(d)
    key = ("oix", d, dtype)
    if key not in _CACHE:
        _CACHE[key] = O.Index(table(d, dtype)[0], g["item_ids"], g["nb_values"], g["nb_row_splits"], g["enter_points"])
    code = {"f16": O.EMB_F16, "bf16": O.EMB_BF16, "f32": O.EMB_F32}[dtype]
    return O.search_batch(_CACHE[key], O.Scorer("l2", d, code), q if sel is None else q[np.asarray(sel)], topn)


def expected(d, dtype, scorer, topn=TOPN, sel=None, ip_score_fn=R.ip_scores):
    """the reference's answer for one case (cached).  ip_score_fn: what the inner-product case is scored with -- the
    mutation check of the matrix swaps it for R.l2_scores"""
    key = ("exp", d, dtype, scorer, tuple(topn), None if sel is None else tuple(sel), ip_score_fn.__name__)
    if key not in _CACHE:
        _CACHE[key] = oracle_batch(d, dtype, topn, sel) if scorer == "l2" else py_batch(d, dtype, ip_score_fn, topn, sel)
    return _CACHE[key]


def expected_per_request(d, dtype, scorer):
    """the per-request launches: the reference run once per setting on that setting's queries
    -> [(queries, level_topn, answer)] for the even and the odd requests"""
    even, odd = np.arange(0, NQ, 2), np.arange(1, NQ, 2)
    return [(even, TOPN, expected(d, dtype, scorer, TOPN, even)), (odd, TOPN_ODD, expected(d, dtype, scorer, TOPN_ODD, odd))]


def check_conditions(d, dtype, scorer):
    """What the case's inputs must satisfy for a pass to mean something, asserted on the reference alone: enough requests
    succeed, uniformly and over the two per-request settings together, and on an inner-product case L2 would have returned
    another row list for at least one query."""
    exp = expected(d, dtype, scorer)
    assert int((exp[0] == 0).sum()) >= MIN_OK, ("the reference serves too few requests", d, dtype, scorer, exp[0])
    per = expected_per_request(d, dtype, scorer)
    assert sum(int((e[0] == 0).sum()) for _, _, e in per) >= MIN_OK, ("per-request settings", d, dtype, scorer, [e[0] for _, _, e in per])
    if scorer == "ip":
        l2 = expected(d, dtype, "ip", ip_score_fn=R.l2_scores)  # (the same schedule scored with L2's arithmetic)
        ok = (exp[0] == 0) & (l2[0] == 0)
        assert (exp[3][ok] != l2[3][ok]).any(axis=1).any(), ("L2 ranks every query like the inner product", d, dtype)
