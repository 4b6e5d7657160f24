"""-m gpu: appending rows to a built HNSW graph (nann_hnsw_append_device) and the export on the device
(nann_hnsw_export_count / _fill) -- the structural invariants tests/test_index_build_gpu.py asks of a build, asked of an
appended graph; what an append may do to old rows; determinism; the validation pass that refuses a malformed graph before
anything is written; serving on the appended graph bit-identical to the oracle; quality against a rebuild of the same rows
(contents are not a parity target, quality is); and the device export against the torch export."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from gpu_util import cuda, require_gpu

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu

ARRAYS = ("adj0", "up_row", "adj_up")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _rows(n, d, dtype="f16", seed=1234):
    from nann_amd import synth
    embs, assign = synth.make_corpus(n, d, n_clusters=16, noise=1.0, seed=seed)
    rows = cuda(embs)
    return (rows.to(torch.bfloat16) if dtype == "bf16" else rows), assign


def _export_np(state):
    from nann_amd import index_build
    ex = index_build.export_hnsw_gpu(state)
    assert ex["enter_points"].dtype == torch.int32 and ex["enter_points"].is_cuda
    for l in (0, 1):
        assert ex["nb_values"][l].dtype == torch.int32 and ex["nb_row_splits"][l].dtype == torch.int64
    return {"levels": state["levels"], "enter_points": ex["enter_points"].cpu().numpy(),
            "nb_values": [v.cpu().numpy().astype(np.int64) for v in ex["nb_values"]],
            "nb_row_splits": [r.cpu().numpy() for r in ex["nb_row_splits"]]}


def _check_export(ex, n, m):
    """the structural checks tests/test_index_build_gpu.py makes of a build"""
    levels = ex["levels"]
    assert len(levels) == n
    assert (ex["enter_points"] == np.nonzero(levels > 2)[0]).all()
    for level, cap in ((0, 2 * m), (1, m)):
        v, rs = ex["nb_values"][level], ex["nb_row_splits"][level]
        assert rs.dtype == np.int64 and len(rs) == n + 1
        deg = np.diff(rs)
        assert rs[0] == 0 and rs[-1] == len(v) and deg.min() >= 0 and deg.max() <= cap   # caps
        if level == 0 or (levels > 1).sum() >= 2:
            assert len(v)
        if len(v):
            assert v.min() >= 0 and v.max() < n                                              # ids in range
        rows = np.repeat(np.arange(n), deg)
        assert (v != rows).all(), "self loop"
        assert len(np.unique(rows * n + v)) == len(v), "a link twice in one row"
        assert (deg[levels <= level] == 0).all(), "a row for a node that is absent on this level"
        assert (levels[v] > level).all(), "a link to a node that is absent on this level"
    if n > 1:
        assert (np.diff(ex["nb_row_splits"][0]) > 0).sum() >= n - 1  # every node (but a build's first) has neighbours


def _old_links_are_a_subset(before, after):
    """for every old node and level: the entries < n_old of its row after the append are among its entries before"""
    n_old = before["adj0"].shape[0]
    n_up_old = int((before["levels"] - 1).sum())
    for name, rows in (("adj0", n_old), ("adj_up", n_up_old)):
        a, b = after[name][:rows], before[name][:rows]
        old = (a >= 0) & (a < n_old)
        for r0 in range(0, rows, 4096):  # [rows, cap, cap] comparisons, a slab at a time
            aa, bb, oo = a[r0:r0 + 4096], b[r0:r0 + 4096], old[r0:r0 + 4096]
            found = (aa[:, :, None] == bb[:, None, :]).any(2)
            assert bool((found | ~oo).all()), f"{name}: an old link that the row did not have"


def _same_arrays(s, t):
    return all(torch.equal(s[k], t[k]) for k in ARRAYS)


def _clone(state):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else (v.copy() if isinstance(v, np.ndarray) else v)) for k, v in state.items()}


@pytest.mark.parametrize("n_old,n_new,d,dtype,m", [(6000, 2000, 64, "f16", 16), (3000, 1000, 128, "bf16", 32), (2000, 500, 256, "f16", 8)])
def test_append_invariants_and_determinism(n_old, n_new, d, dtype, m):
    from nann_amd import index_build
    n = n_old + n_new
    rows, _ = _rows(n, d, dtype)
    base = index_build.build_hnsw_gpu(rows[:n_old], m, 40, seed=5, want_state=True)
    st0 = base["state"]
    keep = _clone(st0)
    a = index_build.append_hnsw_gpu(st0, rows[n_old:], seed=7)
    assert set(a) == set(base) and set(a["state"]) == set(st0)
    sa = a["state"]
    assert sa["adj0"].shape == (n, 2 * m) and sa["up_row"].shape == (n,) and sa["item_embs"].shape == (n, d)
    assert (sa["levels"][:n_old] == st0["levels"]).all() and sa["levels"].min() >= 1
    ex = _export_np(sa)
    _check_export(ex, n, m)
    assert (np.diff(ex["nb_row_splits"][0])[n_old:] > 0).all(), "an appended node without a level-0 row"
    _old_links_are_a_subset(keep, sa)
    b = index_build.append_hnsw_gpu(st0, rows[n_old:], seed=7)
    assert _same_arrays(sa, b["state"]) and (b["state"]["levels"] == sa["levels"]).all()
    assert _same_arrays(st0, keep) and torch.equal(st0["item_embs"], keep["item_embs"]) and (st0["levels"] == keep["levels"]).all()
    # the rows of a graph's tail past the prefix rule: up_row of the new nodes continues the running sum of levels - 1
    lv = sa["levels"].astype(np.int64)
    want = np.where(lv > 1, np.cumsum(lv - 1) - (lv - 1), -1)
    assert (sa["up_row"].cpu().numpy() == want).all()


# ---- the C calls with levels of the test's choosing ---------------------------------------------------------------
def _build_raw(rows, levels, m):
    from nann_amd import _lib
    from nann_amd.ops import _check, _ptr, _stream, _DT
    n, d = rows.shape
    levels = np.ascontiguousarray(levels, np.int32)
    st = {"item_embs": rows, "adj0": torch.empty((n, 2 * m), dtype=torch.int32, device=rows.device),
          "up_row": torch.empty(n, dtype=torch.int32, device=rows.device),
          "adj_up": torch.empty((max(int((levels - 1).sum()), 1), m), dtype=torch.int32, device=rows.device),
          "levels": levels, "M": m, "ef_construction": 40, "keep_pruned": False}
    torch.cuda.synchronize()
    _check(_lib.lib().nann_hnsw_build_device_ex(_ptr(rows), n, d, _DT[rows.dtype], m, 40, 0, C.c_void_p(levels.ctypes.data),
                                                _ptr(st["adj0"]), _ptr(st["up_row"]), _ptr(st["adj_up"]), _stream()), "build")
    return st


def _append_raw(state, rows, levels, fill=-7):
    """nann_hnsw_append_device on grown COPIES of the state's arrays (tails filled with junk: they are to be ignored) ->
    (status, grown state)"""
    from nann_amd import _lib
    from nann_amd.ops import _ptr, _stream, _DT
    m, n_old = state["M"], state["adj0"].shape[0]
    levels = np.ascontiguousarray(levels, np.int32)
    n = len(levels)
    n_up_old = int((np.maximum(state["levels"], 1) - 1).sum())
    n_up = max(int((np.maximum(levels, 1) - 1).sum()), 1)
    dev = rows.device
    st = {"item_embs": rows, "adj0": torch.full((n, 2 * m), fill, dtype=torch.int32, device=dev),
          "up_row": torch.full((n,), fill, dtype=torch.int32, device=dev),
          "adj_up": torch.full((n_up, m), fill, dtype=torch.int32, device=dev),
          "levels": levels, "M": m, "ef_construction": 40, "keep_pruned": False}
    st["adj0"][:n_old] = state["adj0"]
    st["up_row"][:n_old] = state["up_row"]
    st["adj_up"][:n_up_old] = state["adj_up"][:n_up_old]
    torch.cuda.synchronize()
    rc = _lib.lib().nann_hnsw_append_device(_ptr(rows), n_old, n - n_old, rows.shape[1], _DT[rows.dtype], m, 40, 0,
                                            C.c_void_p(levels.ctypes.data), _ptr(st["adj0"]), _ptr(st["up_row"]), _ptr(st["adj_up"]),
                                            _stream())
    return rc, st


def _drawn_levels(n, m, seed):
    from nann_amd import _lib
    lv = np.zeros(n, np.int32)
    assert _lib.lib().nann_hnsw_draw_levels(C.c_int64(n), C.c_int32(m), C.c_uint64(seed), C.c_void_p(lv.ctypes.data), None) == 0
    return lv


def _row(state, node, level):
    """the slots of node's row on `level`, -1 slots dropped"""
    if level == 0:
        r = state["adj0"][node]
    else:
        r = state["adj_up"][int(state["up_row"][node]) + level - 1]
    r = r.cpu().numpy()
    return r[r >= 0]


def test_append_edges():
    from nann_amd import index_build
    m = 16
    rows, _ = _rows(7000, 64)
    base = index_build.build_hnsw_gpu(rows[:2000], m, 40, seed=5, want_state=True)["state"]
    # one row
    one = index_build.append_hnsw_gpu(base, rows[2000:2001], seed=3)["state"]
    _check_export(_export_np(one), 2001, m)
    assert len(_row(one, 2000, 0)) > 0
    # no row: the arrays as they were
    none = index_build.append_hnsw_gpu(base, rows[:0], seed=3)["state"]
    assert _same_arrays(none, base) and none["adj0"] is not base["adj0"]
    # a graph of one node
    single = index_build.build_hnsw_gpu(rows[:1], m, 40, seed=5, want_state=True)["state"]
    grown = index_build.append_hnsw_gpu(single, rows[1:501], seed=3)["state"]
    ex = _export_np(grown)
    _check_export(ex, 501, m)
    assert (np.diff(ex["nb_row_splits"][0]) > 0).all()
    # three appends in a row
    st = index_build.build_hnsw_gpu(rows[:4000], m, 40, seed=5, want_state=True)["state"]
    for k in range(3):
        before = _clone(st)
        st = index_build.append_hnsw_gpu(st, rows[4000 + 1000 * k: 5000 + 1000 * k], seed=10 + k)["state"]
        _old_links_are_a_subset(before, st)
    ex = _export_np(st)
    _check_export(ex, 7000, m)
    assert (np.diff(ex["nb_row_splits"][0]) > 0).all()


def test_append_a_node_with_more_levels_than_the_graph():
    """Every old node has at most 2 levels; a new node has 4.  It goes in alone, is linked on the levels the graph has (1 and 0),
    its rows on levels 2 and 3 stay empty, and it is the entry point of whatever follows.  With a SECOND new node of 4 levels
    behind it, that node is searched from the first on levels 3 and 2, where the first has rows and no links: they link to
    each other there -- the insertion's own back-link, as in a build, whose second node links to its first the same way."""
    m, n_old = 16, 2000
    rows, _ = _rows(2600, 64)
    old_levels = np.minimum(_drawn_levels(n_old, m, 5), 2)
    base = _build_raw(rows[:n_old].contiguous(), old_levels, m)
    new_levels = np.minimum(_drawn_levels(300, m, 6), 2)
    first, second = n_old + 5, n_old + 9
    # (a) one such node
    lv = np.concatenate([old_levels, new_levels])
    lv[first] = 4
    rc, st = _append_raw(base, rows[:2300].contiguous(), lv)
    assert rc == 0
    ex = _export_np(st)
    _check_export(ex, 2300, m)
    assert len(_row(st, first, 0)) > 0 and len(_row(st, first, 1)) > 0
    assert len(_row(st, first, 2)) == 0 and len(_row(st, first, 3)) == 0
    assert list(ex["enter_points"]) == [first]
    # (b) a second one behind it
    lv[second] = 4
    rc, st = _append_raw(base, rows[:2300].contiguous(), lv)
    assert rc == 0
    ex = _export_np(st)
    _check_export(ex, 2300, m)
    assert len(_row(st, first, 0)) > 0 and len(_row(st, first, 1)) > 0 and len(_row(st, second, 0)) > 0 and len(_row(st, second, 1)) > 0
    for level in (2, 3):  # nothing on these levels but the two nodes' link to each other
        assert list(_row(st, first, level)) == [second] and list(_row(st, second, level)) == [first]
    assert list(ex["enter_points"]) == [first, second]
    # a further append on top of the result
    more = np.concatenate([lv, _drawn_levels(300, m, 8)])
    rc, st2 = _append_raw(st, rows, more)
    assert rc == 0
    ex = _export_np(st2)
    _check_export(ex, 2600, m)
    assert (np.diff(ex["nb_row_splits"][0])[n_old:] > 0).all()


def test_append_refuses_a_malformed_graph_before_it_writes():
    from nann_amd import _lib
    m, n_old, n = 16, 3000, 3400
    rows, _ = _rows(n, 64)
    levels = np.concatenate([_drawn_levels(n_old, m, 5), _drawn_levels(n - n_old, m, 6)])
    base = _build_raw(rows[:n_old].contiguous(), levels[:n_old], m)
    cnt0 = (base["adj0"] >= 0).sum(1).cpu().numpy()
    up = base["up_row"].cpu().numpy()
    roomy = int(np.nonzero((cnt0 >= 1) & (cnt0 <= 2 * m - 2))[0][0])        # a level-0 row with two free slots
    upper = int(np.nonzero(levels[:n_old] > 1)[0][0])                        # a node with a level-1 row
    flat = int(np.nonzero(levels[:n_old] == 1)[0][0])                        # a node without one

    def range_(s): s["adj0"][5, 0] = n_old
    def hole(s): s["adj0"][roomy, cnt0[roomy] + 1] = 3
    def level(s): s["adj_up"][int(up[upper]), 0] = flat
    def up_row(s): s["up_row"][10] = int(up[10]) + 1
    cases = [(range_, "outside [-1, n_old)"), (hole, "follows a -1"), (level, "no row on that level"), (up_row, "up_row differs")]
    for damage, words in cases:
        bad = _clone(base)
        damage(bad)
        rc, st = _append_raw(bad, rows, levels)
        assert rc == 7, (damage.__name__, rc)
        assert words in _lib.last_error(), (damage.__name__, _lib.last_error())
        n_up_old = int((levels[:n_old] - 1).sum())
        assert torch.equal(st["adj0"][:n_old], bad["adj0"]) and bool((st["adj0"][n_old:] == -7).all())
        assert torch.equal(st["up_row"][:n_old], bad["up_row"]) and bool((st["up_row"][n_old:] == -7).all())
        assert torch.equal(st["adj_up"][:n_up_old], bad["adj_up"][:n_up_old]) and bool((st["adj_up"][n_up_old:] == -7).all())
    zero = levels.copy()
    zero[17] = 0
    rc, st = _append_raw(base, rows, zero)
    assert rc == 7 and "levels" in _lib.last_error()
    assert torch.equal(st["adj0"][:n_old], base["adj0"]) and bool((st["adj0"][n_old:] == -7).all())
    assert torch.equal(st["up_row"][:n_old], base["up_row"]) and bool((st["up_row"][n_old:] == -7).all())
    # ... and the process goes on: the graph as it was built is accepted
    rc, st = _append_raw(base, rows, levels)
    assert rc == 0
    _check_export(_export_np(st), n, m)


# ---- serving and quality: 40 000 x 64 f16 in 16 clusters (2 500 a cluster >= 30 x ef at ef = 64) ---------------------
# M = 16: the entry layer (levels > 2, one node in M^2) has to hold the ef = 64 nodes the first top-k asks for -- ~156 of 40 000
# at M = 16, ~39 at M = 32, where every request fails k > n as in the reference (topk_op.cc:67-71)
N, D, M, EF, N_OLD = 40_000, 64, 16, 64, 30_000
TOPN = [EF] * 5 + [100]
_SHARED = {}


def _case(name):
    """(rows in insertion order, n_old, appended state, None, queries)"""
    if name in _SHARED:
        return _SHARED[name]
    from nann_amd import index_build, ops, synth
    embs, assign = synth.make_corpus(N, D, n_clusters=16, noise=1.0)
    if name == "random":
        order = np.random.default_rng(99).permutation(N)
        n_old = N_OLD
        seqs = synth.make_queries_from_centres(D, 64, n_clusters=16, noise=1.0)
    else:  # the novel cluster: clusters 0-14 are the graph, cluster 15 is appended, the queries are drawn at its centre
        order = np.concatenate([np.nonzero(assign != 15)[0], np.nonzero(assign == 15)[0]])
        n_old = int((assign != 15).sum())
        many = 4096
        seqs = synth.make_queries_from_centres(D, many, n_clusters=16, noise=1.0)
        rng = np.random.default_rng(4321)  # the function's own draws: lengths, then clusters
        rng.integers(7, 51, size=many)
        cl = rng.integers(0, 16, size=many)
        seqs = seqs[cl == 15][:64]
        assert len(seqs) == 64
        s32 = seqs.astype(np.float32)
        mean = s32.sum(1) / (np.abs(s32).sum(2) > 0).sum(1, keepdims=True)
        centres = synth.make_centres(D, 16) / np.sqrt(D)
        nearest = ((mean[:, None, :] - centres[None]) ** 2).sum(2).argmin(1)
        assert (nearest == 15).mean() > 0.9, "the queries are not cluster 15's"
    rows = cuda(embs[order])
    base = index_build.build_hnsw_gpu(rows[:n_old], M, 40, seed=5, want_state=True)["state"]
    app = index_build.append_hnsw_gpu(base, rows[n_old:], seed=7)["state"]
    q = ops.user_seq_mean(torch.as_tensor(seqs).cuda())
    _SHARED[name] = (rows, n_old, app, None, q)
    return _SHARED[name]


def _index(rows, ex):
    from nann_amd import retrieval, synth
    return retrieval.Index(rows, synth.make_item_ids(N), ex["nb_values"], ex["nb_row_splits"], ex["enter_points"])


def test_serving_on_the_appended_graph_matches_the_oracle(oracle):
    from nann_amd import index_build, ops, retrieval, synth
    rows, n_old, app, _, q = _case("random")
    ex = index_build.export_hnsw_gpu(app)  # device tensors straight into the Index: no host round trip
    dix = _index(rows, ex)
    sc = ops.Scorer("l2", D)
    r = retrieval.search(dix, sc, q, TOPN)
    torch.cuda.synchronize()
    st = r.status.cpu().numpy()
    assert (st == 0).mean() >= 0.95
    oix = oracle.Index(rows.cpu().numpy(), synth.make_item_ids(N), [v.cpu().numpy() for v in ex["nb_values"]],
                       [s.cpu().numpy() for s in ex["nb_row_splits"]], ex["enter_points"].cpu().numpy())
    est, eids, esc, eidx, ectr = oracle.search_batch(oix, oracle.Scorer("l2", D, oracle.EMB_F16), q[:16].cpu().numpy(), TOPN, n_threads=8)
    ok = est == 0
    assert (st[:16] == est).all() and ok.any()
    assert (r.index.cpu().numpy()[:16][ok] == eidx[ok]).all() and (r.item_ids.cpu().numpy()[:16][ok] == eids[ok]).all()
    assert (r.scores.cpu().numpy()[:16][ok].view(np.uint32) == esc[ok].view(np.uint32)).all()
    assert (r.counters.cpu().numpy()[:16][ok] == ectr[ok]).all()


def _recall_and_degree(rows, ex, q):
    from nann_amd import ops, retrieval
    dix = _index(rows, ex)
    sc = ops.Scorer("l2", D)
    r = retrieval.search(dix, sc, q, TOPN)
    truth = retrieval.search_all(dix, sc, q, 100)
    torch.cuda.synchronize()
    got, want = r.index.cpu().numpy(), truth.index.cpu().numpy()
    ok = r.status.cpu().numpy() == 0
    hits = sum(len(set(got[b].tolist()) & set(want[b].tolist())) for b in range(len(got)) if ok[b])
    n0 = ex["nb_values"][0].numel() if isinstance(ex["nb_values"][0], torch.Tensor) else len(ex["nb_values"][0])
    return hits / want.size, n0 / N, float(ok.mean())


def _built(rows, q, order=None):
    """(recall@100, mean L0 degree, share of valid requests) of a build_hnsw_gpu of `rows`, taken in `order` when one is given.
    The queries are the same; recall is against the exhaustive search of the index that is asked, so row numbers never have
    to be mapped between the two orders -- the sets of rows are the same."""
    from nann_amd import index_build
    r = rows if order is None else rows[torch.as_tensor(order).cuda()].contiguous()
    ex = index_build.build_hnsw_gpu(r, M, 40, seed=5)
    return _recall_and_degree(r, {"nb_values": [v.astype(np.int32) for v in ex["nb_values"]], "nb_row_splits": ex["nb_row_splits"],
                                  "enter_points": ex["enter_points"].astype(np.int32)}, q)


@pytest.mark.parametrize("name", ["random", "novel_cluster"])
def test_append_quality_against_a_rebuild(name):
    """recall@100 of the L2 traversal (truth: the exhaustive search) on the appended graph within 0.02 of a graph
    build_hnsw_gpu makes of the same rows, mean level-0 degree within 10 % of it -- the margins the device builder is given
    against the host builder, for the same reason.  Two yardsticks.  The build of the rows IN THE SAME ORDER is trusted only
    where it serves: on the novel cluster it puts the whole cluster into its last batch, every request there fails k > n
    (status 4) and its recall is 0 -- a bound nothing can miss.  The build of the same rows in SHUFFLED order (the order a
    build is meant for) always holds.  Measured on the MI355X, appended / same order / shuffled -- random split: 0.944 / 0.942 /
    0.961 (the shuffled build is a yardstick for the cluster case: in the random split it is a build of one more random
    order, and the margin is asked against the order the issue names); novel cluster: 0.919 / 0.000 / 0.915.  With one batch
    (no third term in the batch rule) the novel cluster gives 0.000, with ceil(n_new / 8) 0.890, / 32 0.897: the case fails
    there."""
    from nann_amd import index_build
    rows, n_old, app, _, q = _case(name)
    a = _recall_and_degree(rows, index_build.export_hnsw_gpu(app), q)
    same = _built(rows, q)
    shuffled = _built(rows, q, np.random.default_rng(3).permutation(N))
    print(f"append quality [{name}]: n_old {n_old}, (recall@100, mean L0 degree, valid) appended {a}, rebuilt in the same order {same}, "
          f"rebuilt in shuffled order {shuffled}")
    assert a[2] >= 0.95 and shuffled[2] >= 0.95, (a, shuffled)
    if name == "random":
        assert same[2] >= 0.95, same
        yardsticks = [same]
    else:
        yardsticks = [shuffled] + ([same] if same[2] >= 0.95 else [])
    for b in yardsticks:
        assert a[0] >= b[0] - 0.02, (a, b)
        assert abs(a[1] - b[1]) / b[1] < 0.1, (a, b)


def test_device_export_equals_the_torch_export():
    from nann_amd import _lib, index_build
    from nann_amd.ops import _ptr, _stream
    rows, _ = _rows(5000, 64)
    built = index_build.build_hnsw_gpu(rows[:4000], 16, 40, seed=5, want_state=True)
    grown = index_build.append_hnsw_gpu(built["state"], rows[4000:], seed=7)
    for t in (built, grown):
        ex = index_build.export_hnsw_gpu(t["state"])
        assert ex["enter_points"].cpu().numpy().tobytes() == t["enter_points"].astype(np.int32).tobytes()
        for l in (0, 1):
            assert (ex["nb_values"][l].cpu().numpy().astype(np.int64) == t["nb_values"][l]).all() and len(t["nb_values"][l]) == ex["nb_values"][l].numel()
            assert ex["nb_row_splits"][l].cpu().numpy().tobytes() == t["nb_row_splits"][l].tobytes()
    # hand-made arrays, M = 2: holes in the middle of rows are dropped, the order of the rest is kept
    st = {"adj0": cuda(np.array([[1, -1, 2, -1], [-1, -1, 0, 3], [-1, -1, -1, -1], [0, 1, 2, -1]], np.int32)),
          "up_row": cuda(np.array([-1, 0, 1, -1], np.int32)), "adj_up": cuda(np.array([[-1, 2], [1, -1], [-1, -1]], np.int32)),
          "levels": np.array([1, 2, 3, 1], np.int32), "M": 2}
    ex = index_build.export_hnsw_gpu(st)
    assert ex["nb_values"][0].cpu().tolist() == [1, 2, 0, 3, 0, 1, 2] and ex["nb_row_splits"][0].cpu().tolist() == [0, 2, 4, 4, 7]
    assert ex["nb_values"][1].cpu().tolist() == [2, 1] and ex["nb_row_splits"][1].cpu().tolist() == [0, 0, 1, 2, 2]
    assert ex["enter_points"].cpu().tolist() == [2]
    # row_splits of another graph (here: this one's, shifted by one) are refused by fill, and nothing lands behind values[nnz)
    lvp = C.c_void_p(st["levels"].ctypes.data)
    nnz = (C.c_int64 * 2)(7, 2)
    v0, v1 = torch.full((7 + 8,), -9, dtype=torch.int32, device="cuda"), torch.full((2 + 8,), -9, dtype=torch.int32, device="cuda")
    enter = torch.empty(1, dtype=torch.int32, device="cuda")
    shifted = ex["nb_row_splits"][0] + 1
    torch.cuda.synchronize()
    rc = _lib.lib().nann_hnsw_export_fill(_ptr(st["adj0"]), _ptr(st["up_row"]), _ptr(st["adj_up"]), lvp, 4, 2, 2, _ptr(shifted),
                                          _ptr(ex["nb_row_splits"][1]), nnz, _ptr(v0), _ptr(v1), _ptr(enter), _stream())
    assert rc == 7 and "row_splits" in _lib.last_error()
    assert bool((v0[7:] == -9).all()) and bool((v1[2:] == -9).all())
    # an up_row that points outside adj_up is refused, not followed
    st["up_row"] = cuda(np.array([-1, 0, 7, -1], np.int32))
    rs = [torch.empty(5, dtype=torch.int64, device="cuda") for _ in range(2)]
    nnz, n_enter = (C.c_int64 * 2)(), C.c_int64(0)
    torch.cuda.synchronize()
    rc = _lib.lib().nann_hnsw_export_count(_ptr(st["adj0"]), _ptr(st["up_row"]), _ptr(st["adj_up"]), C.c_void_p(st["levels"].ctypes.data),
                                           4, 2, 2, _ptr(rs[0]), _ptr(rs[1]), nnz, C.byref(n_enter), _stream())
    assert rc == 7 and "up_row" in _lib.last_error()
