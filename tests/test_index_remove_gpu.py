"""-m gpu: removing rows from a built HNSW graph (nann_hnsw_remove_count / nann_hnsw_remove_device): a hand-made graph with an
exact answer; the invariants of the result against a numpy model of the candidate pool, determinism, the input left as it was;
the edges; the validation pass that refuses a malformed graph, or a wrong n_keep, before anything is written; serving on the
compacted graph bit-identical to the oracle; quality against a rebuild of the survivors (contents are not a parity target,
quality is).  The helper shapes are those of tests/test_index_append_gpu.py.

One property of that file's _check_export is asked in the form a removal can meet.  A build or an append leaves every node
(but a build's first) with neighbours; a removal adds no back-links and follows one hop only, so a node whose candidate pool is
empty comes out with an empty row -- counted in stats[1], not healed (include/nann_hip.h).  Here: a repaired row is non-empty
WHENEVER its pool is non-empty (the numpy model), and the rows without neighbours are at most the build's one plus stats[1]."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from gpu_util import cuda, require_gpu

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu

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


def _check_export(ex, n, m, may_be_empty=0):
    """the structural checks tests/test_index_build_gpu.py makes of a build; may_be_empty: the rows a removal counted as left
    without neighbours (stats[1])"""
    levels = ex["levels"]
    assert len(levels) == n
    assert (ex["enter_points"] == np.nonzero(levels > 2)[0]).all()
    for level, cap in ((0, 2 * m), (1, m)):
        v, rs = ex["nb_values"][level], ex["nb_row_splits"][level]
        assert rs.dtype == np.int64 and len(rs) == n + 1
        deg = np.diff(rs)
        assert rs[0] == 0 and rs[-1] == len(v) and deg.min() >= 0 and deg.max() <= cap   # caps
        if n > 1 and (level == 0 or (levels > 1).sum() >= 2):
            assert len(v)
        if len(v):
            assert v.min() >= 0 and v.max() < n                                              # ids in range
        rows = np.repeat(np.arange(n), deg)
        assert (v != rows).all(), "self loop"
        assert len(np.unique(rows * n + v)) == len(v), "a link twice in one row"
        assert (deg[levels <= level] == 0).all(), "a row for a node that is absent on this level"
        assert (levels[v] > level).all(), "a link to a node that is absent on this level"
    if n > 1:
        assert (np.diff(ex["nb_row_splits"][0]) > 0).sum() >= n - 1 - may_be_empty


def _same_arrays(s, t):
    n_up = int((np.asarray(s["levels"]) - 1).sum())
    return torch.equal(s["adj0"], t["adj0"]) and torch.equal(s["up_row"], t["up_row"]) and torch.equal(s["adj_up"][:n_up], t["adj_up"][:n_up])


def _clone(state):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else (v.copy() if isinstance(v, np.ndarray) else v)) for k, v in state.items()}


def _pack(mask):
    """bool[n] -> the deny bitmap's packed words, numpy uint32[ceil(n / 32)]"""
    n = len(mask)
    flags = np.zeros((n + 31) // 32 * 32, bool)
    flags[:n] = mask
    return (flags.reshape(-1, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)


# ---- the numpy model: the candidate pool of every surviving row, from the OLD arrays ---------------------------------
def _old_rows(state):
    """[(level, node ids that have a row on it, their rows [k, cap])] of a state, on the host"""
    adj0, up, adj_up, lv = state["adj0"].cpu().numpy(), state["up_row"].cpu().numpy(), state["adj_up"].cpu().numpy(), np.asarray(state["levels"])
    out = [(0, np.arange(len(lv)), adj0)]
    for level in range(1, int(lv.max())):
        nodes = np.nonzero(lv > level)[0]
        out.append((level, nodes, adj_up[up[nodes] + level - 1]))
    return out


def _dist(x, p, c, metric):
    """(distances of rows c to row p in float64, a bound on what f32 accumulation of the d terms may differ from them by)"""
    a, b = x[p][None, :], x[c]
    if metric == "ip":
        return -(a * b).sum(1), 1e-4 * np.sqrt((a * a).sum()) * np.sqrt((b * b).sum(1))
    dd = ((a - b) ** 2).sum(1)
    return dd, 1e-4 * dd


def _check_removal(old, removed, res):
    """the properties of a removal: `old` the state it was given, `removed` bool[n], `res` what remove_hnsw_gpu returned"""
    st, stats = res["state"], res["stats"]
    m, metric = old["M"], old.get("metric", "l2")
    n = len(removed)
    keep = np.nonzero(~removed)[0]
    n_keep = len(keep)
    new_id = np.full(n, -1, np.int64)
    new_id[keep] = np.arange(n_keep)
    lv_old = np.asarray(old["levels"])
    # renumbering: order kept, levels kept, the rows gathered, up_row by the prefix rule
    assert (res["kept_rows"].cpu().numpy() == keep).all() and res["kept_rows"].dtype == torch.int32
    assert (st["levels"] == lv_old[keep]).all() and st["levels"].dtype == np.int32
    assert torch.equal(st["item_embs"], old["item_embs"][torch.as_tensor(keep).cuda()])
    lv = st["levels"].astype(np.int64)
    n_up = int((lv - 1).sum())
    assert st["adj0"].shape == (n_keep, 2 * m) and st["up_row"].shape == (n_keep,) and st["adj_up"].shape == (max(n_up, 1), m)
    assert (st["up_row"].cpu().numpy() == np.where(lv > 1, np.cumsum(lv - 1) - (lv - 1), -1)).all()
    for k in ("M", "ef_construction", "keep_pruned"):
        assert st[k] == old[k]
    assert st["metric"] == metric
    # every surviving row against the pool the old arrays give
    x = old["item_embs"].float().cpu().numpy().astype(np.float64)
    new_rows = {level: rows for level, _, rows in _old_rows(st)}
    repaired = beyond = emptied = 0
    for level, nodes, rows in _old_rows(old):
        cap = 2 * m if level == 0 else m
        at = {int(v): i for i, v in enumerate(nodes)}
        alive = nodes[~removed[nodes]]
        got_rows = new_rows[level] if len(alive) else np.zeros((0, cap), np.int64)
        assert len(got_rows) == len(alive) and got_rows.shape[1] == cap
        for i, p in enumerate(alive):
            p = int(p)
            row = rows[at[p]]
            got = got_rows[i]
            fill = int((got >= 0).sum())
            assert (got[:fill] >= 0).all() and (got[fill:] == -1).all(), "not a dense prefix"
            assert got.max(initial=-1) < n_keep
            back = keep[got[:fill]]  # old ids
            entries = row[row >= 0]
            holes = entries[removed[entries]]
            if len(holes) == 0:
                assert (got == np.where(row >= 0, new_id[np.maximum(row, 0)], -1)).all(), "a row without removed entries was not copied"
                continue
            repaired += 1
            pool = set(entries[~removed[entries]].tolist())
            for r in holes:
                e = rows[at[int(r)]]
                e = e[e >= 0]
                pool.update(e[~removed[e]].tolist())
            pool.discard(p)
            beyond += len(pool) > 64
            assert set(back.tolist()) <= pool, "an entry from outside the pool"
            assert len(set(back.tolist())) == fill and fill <= cap
            assert (fill > 0) == (len(pool) > 0), "an empty row with a pool to choose from"
            emptied += level == 0 and fill == 0
            if fill:  # the heuristic always keeps the nearest member of the pool: it heads the row
                members = np.array(sorted(pool))
                dd, tol = _dist(x, p, members, metric)
                first = int(np.nonzero(members == back[0])[0][0])
                assert dd[first] <= (dd + tol).min() + tol[first], "the row does not start with the nearest of its pool"
    assert list(stats) == [repaired, emptied, beyond, n_keep], (list(stats), [repaired, emptied, beyond, n_keep])
    ex = _export_np(st)
    _check_export(ex, n_keep, m, may_be_empty=emptied + int((np.diff(_export_np(old)["nb_row_splits"][0])[keep] == 0).sum()))
    return ex


def _random_mask(n, share, seed):
    return np.random.default_rng(seed).random(n) < share


# ---- 1. a hand-made graph with an exact answer -----------------------------------------------------------------------
def _hand_made(keep_pruned):
    xs = [0, 1, 2, 3, 4, 10]
    embs = np.zeros((6, 64), np.float16)
    embs[:, 0] = xs
    adj0 = np.array([[1, 2, -1, -1], [0, 2, -1, -1], [1, 3, -1, -1], [2, 4, -1, -1], [3, 5, -1, -1], [4, -1, -1, -1]], np.int32)
    return {"item_embs": cuda(embs), "adj0": cuda(adj0), "up_row": cuda(np.full(6, -1, np.int32)), "adj_up": cuda(np.full((1, 2), -1, np.int32)),
            "levels": np.ones(6, np.int32), "M": 2, "ef_construction": 40, "keep_pruned": keep_pruned, "metric": "l2"}


def test_hand_made_graph_has_the_exact_answer():
    """M = 2, rows e_i = (x_i, 0, ...) with x = 0, 1, 2, 3, 4, 10; node 2 leaves.  Node 0: pool {1: 1, 3: 9}, 3 is dominated by 1
    (4 < 9).  Node 1: pool {0: 1, 3: 4}, 3 is kept (9 >= 4).  Old node 3: pool {4: 1, 1: 4}, 1 is kept, ascending by distance.  Old
    nodes 4 and 5 are copied.  Small integers: exact in f16 and f32, no tolerance."""
    from nann_amd import index_build
    pad = lambda rows: [r + [-1] * (4 - len(r)) for r in rows]
    st = _hand_made(False)
    before = _clone(st)
    r = index_build.remove_hnsw_gpu(st, remove_rows=[2], want_export=False)
    assert r["state"]["adj0"].cpu().tolist() == pad([[1], [0, 2], [3, 1], [2, 4], [3]])
    assert r["kept_rows"].cpu().tolist() == [0, 1, 3, 4, 5]
    assert list(r["stats"]) == [3, 0, 0, 5]
    assert r["state"]["up_row"].cpu().tolist() == [-1] * 5 and (r["state"]["levels"] == 1).all()
    assert r["state"]["item_embs"][:, 0].cpu().tolist() == [0, 1, 3, 4, 10]
    assert _same_arrays(st, before) and torch.equal(st["item_embs"], before["item_embs"])
    # keepPrunedConnections: the dominated 3 (new id 2) fills row 0's free slot
    r = index_build.remove_hnsw_gpu(_hand_made(True), deny_bits=np.array([0, 0, 1, 0, 0, 0], bool), want_export=False)
    assert r["state"]["adj0"].cpu().tolist() == pad([[1, 2], [0, 2], [3, 1], [2, 4], [3]])
    assert list(r["stats"]) == [3, 0, 0, 5]


# ---- 2. invariants and determinism -----------------------------------------------------------------------------------
# the fifth case: keepPrunedConnections fills the rows of the M = 32 graph up to their 64 slots, so that pools go far beyond 64
@pytest.mark.parametrize("n,d,dtype,m,metric,keep_pruned", [(8000, 64, "f16", 16, "l2", False), (4000, 128, "bf16", 32, "l2", False),
                                                            (2500, 256, "f16", 8, "l2", False), (8000, 64, "f16", 16, "ip", False),
                                                            (4000, 128, "bf16", 32, "l2", True)])
def test_remove_invariants_and_determinism(n, d, dtype, m, metric, keep_pruned):
    from nann_amd import index_build
    rows, _ = _rows(n, d, dtype)
    st0 = index_build.build_hnsw_gpu(rows, m, 40, seed=5, want_state=True, metric=metric, keep_pruned=keep_pruned)["state"]
    keep = _clone(st0)
    removed = _random_mask(n, 0.25, 11)
    a = index_build.remove_hnsw_gpu(st0, deny_bits=removed)
    assert set(a) == {"levels", "enter_points", "nb_values", "nb_row_splits", "state", "kept_rows", "stats"} and set(a["state"]) == set(st0)
    _check_removal(keep, removed, a)
    print(f"remove [{n} x {d} {dtype} M {m} {metric} keep_pruned {keep_pruned}]: stats {list(a['stats'])}")
    if keep_pruned:
        assert a["stats"][2] > 0, "no pool beyond 64: the case does not test what it is here for"
    b = index_build.remove_hnsw_gpu(st0, remove_rows=np.nonzero(removed)[0])
    assert _same_arrays(a["state"], b["state"]) and (b["state"]["levels"] == a["state"]["levels"]).all() and (a["stats"] == b["stats"]).all()
    assert torch.equal(a["kept_rows"], b["kept_rows"]) and torch.equal(a["state"]["item_embs"], b["state"]["item_embs"])
    assert _same_arrays(st0, keep) and torch.equal(st0["item_embs"], keep["item_embs"]) and (st0["levels"] == keep["levels"]).all()
    assert torch.equal(st0["adj_up"], keep["adj_up"])


# ---- 3. edges ----------------------------------------------------------------------------------------------------------
def test_remove_edges():
    from nann_amd import index_build, retrieval
    m, n = 16, 3001
    rows, _ = _rows(n + 500, 64)
    base = index_build.build_hnsw_gpu(rows[:n], m, 40, seed=5, want_state=True)["state"]
    keep = _clone(base)
    lv = base["levels"]
    n_up = int((lv - 1).sum())
    # nothing removed: the arrays bit for bit
    none = index_build.remove_hnsw_gpu(base, remove_rows=[])
    assert _same_arrays(none["state"], base) and none["state"]["adj0"] is not base["adj0"]
    assert none["kept_rows"].cpu().tolist() == list(range(n)) and list(none["stats"]) == [0, 0, 0, n]
    assert torch.equal(none["state"]["item_embs"], base["item_embs"])
    # rows outside the graph remove nothing, a row named twice is removed once
    r = index_build.remove_hnsw_gpu(base, remove_rows=torch.tensor([7, -3, n, 7, n + 40]))
    assert r["stats"][3] == n - 1
    # all but one
    for survivor in (0, int(np.argmax(lv))):
        mask = np.ones(n, bool)
        mask[survivor] = False
        one = index_build.remove_hnsw_gpu(base, deny_bits=mask, want_export=False)
        s = one["state"]
        assert s["adj0"].shape == (1, 2 * m) and bool((s["adj0"] == -1).all()) and one["kept_rows"].cpu().tolist() == [survivor]
        assert bool((s["adj_up"][:int(lv[survivor]) - 1] == -1).all()) and list(s["levels"]) == [lv[survivor]]
    # every node with more than one level: adj_up unused, no enter points
    flat = index_build.remove_hnsw_gpu(base, deny_bits=lv > 1)
    ex = _check_removal(keep, lv > 1, flat)
    assert len(ex["enter_points"]) == 0 and len(ex["nb_values"][1]) == 0 and (flat["state"]["up_row"] == -1).all()
    # the entry point (the lowest id among the most levels), then an append on top of the result
    mask = np.zeros(n, bool)
    mask[int(np.argmax(lv))] = True
    r = index_build.remove_hnsw_gpu(base, deny_bits=mask)
    _check_removal(keep, mask, r)
    grown = index_build.append_hnsw_gpu(r["state"], rows[n:], seed=9)["state"]
    _check_export(_export_np(grown), n - 1 + 500, m, may_be_empty=int(r["stats"][1]) + 1)
    # bits at and beyond n in the last word (n = 3001: bit 25 of word 93 is the first of them) are ignored
    mask = _random_mask(n, 0.25, 3)
    words = _pack(mask)
    dirty = words.copy()
    dirty[-1] |= np.uint32(0xffffffff) << np.uint32(n & 31)
    assert dirty[-1] != words[-1]
    a = index_build.remove_hnsw_gpu(base, deny_bits=words.view(np.int32))
    b = index_build.remove_hnsw_gpu(base, deny_bits=cuda(dirty.view(np.int32)))
    assert _same_arrays(a["state"], b["state"]) and (a["stats"] == b["stats"]).all() and torch.equal(a["kept_rows"], b["kept_rows"])
    _check_removal(keep, mask, a)
    # ... and a filter's deny_bits goes in as it is
    f = retrieval.make_filter(type("Ix", (), {"device": "cuda", "n_items": n})(), deny_rows=np.nonzero(mask)[0])
    c = index_build.remove_hnsw_gpu(base, deny_bits=f.deny_bits)
    assert _same_arrays(a["state"], c["state"])
    # a node all of whose neighbours are removed
    deg = (base["adj0"] >= 0).sum(1).cpu().numpy()
    p = int(np.nonzero(deg >= 2)[0][0])
    mask = np.zeros(n, bool)
    nb = base["adj0"][p].cpu().numpy()
    mask[nb[nb >= 0]] = True
    _check_removal(keep, mask, index_build.remove_hnsw_gpu(base, deny_bits=mask))
    # two removals in a row
    m1 = _random_mask(n, 0.25, 21)
    r1 = index_build.remove_hnsw_gpu(base, deny_bits=m1)
    s1 = _clone(r1["state"])
    m2 = _random_mask(len(s1["levels"]), 0.25, 22)
    r2 = index_build.remove_hnsw_gpu(r1["state"], deny_bits=m2)
    _check_removal(s1, m2, r2)
    assert (r1["kept_rows"][r2["kept_rows"].long()].cpu().numpy() == np.nonzero(~m1)[0][~m2]).all()
    with pytest.raises(ValueError):
        index_build.remove_hnsw_gpu(base)
    with pytest.raises(ValueError):
        index_build.remove_hnsw_gpu(base, remove_rows=[1], deny_bits=mask)
    assert _same_arrays(base, keep)


# ---- 4. refusal before writing -------------------------------------------------------------------------------------------
def _remove_raw(state, rows, bits, n_keep, n_up_keep, fill=-7):
    """nann_hnsw_remove_device into arrays filled with junk -> (status, the three arrays)"""
    from nann_amd import _lib
    from nann_amd.ops import _ptr, _stream, _DT
    m, n = state["M"], state["adj0"].shape[0]
    levels = np.ascontiguousarray(state["levels"], np.int32)
    out = [torch.full((max(n_keep, 1), 2 * m), fill, dtype=torch.int32, device="cuda"), torch.full((max(n_keep, 1),), fill, dtype=torch.int32, device="cuda"),
           torch.full((max(n_up_keep, 1), m), fill, dtype=torch.int32, device="cuda")]
    stats = (C.c_int64 * 4)(-7, -7, -7, -7)
    torch.cuda.synchronize()
    rc = _lib.lib().nann_hnsw_remove_device(_ptr(rows), n, rows.shape[1], _DT[rows.dtype], m, 0, _lib.SCORER_L2, C.c_void_p(levels.ctypes.data),
                                            _ptr(state["adj0"]), _ptr(state["up_row"]), _ptr(state["adj_up"]), _ptr(bits), n_keep,
                                            _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), stats, _stream())
    torch.cuda.synchronize()
    return rc, out, list(stats)


def test_remove_refuses_a_malformed_graph_before_it_writes():
    from nann_amd import _lib, index_build
    m, n = 16, 3000
    rows, _ = _rows(n, 64)
    base = index_build.build_hnsw_gpu(rows, m, 40, seed=5, want_state=True)["state"]
    levels = base["levels"]
    mask = _random_mask(n, 0.25, 11)
    bits = cuda(_pack(mask).view(np.int32))
    n_keep, n_up_keep = int((~mask).sum()), int((levels[~mask] - 1).sum())
    cnt0 = (base["adj0"] >= 0).sum(1).cpu().numpy()
    up = base["up_row"].cpu().numpy()
    roomy = int(np.nonzero((cnt0 >= 1) & (cnt0 <= 2 * m - 2))[0][0])        # a level-0 row with two free slots
    upper = int(np.nonzero(levels > 1)[0][0])                                # a node with a level-1 row
    flat = int(np.nonzero(levels == 1)[0][0])                                # a node without one

    def range_(s): s["adj0"][5, 0] = n
    def hole(s): s["adj0"][roomy, cnt0[roomy] + 1] = 3
    def level(s): s["adj_up"][int(up[upper]), 0] = flat
    def up_row(s): s["up_row"][10] = int(up[10]) + 1
    untouched = lambda out, stats: all(bool((o == -7).all()) for o in out) and stats == [-7] * 4
    cases = [(range_, "outside [-1, n_old)"), (hole, "follows a -1"), (level, "no row on that level"), (up_row, "up_row differs")]
    for damage, words in cases:
        bad = _clone(base)
        damage(bad)
        rc, out, stats = _remove_raw(bad, rows, bits, n_keep, n_up_keep)
        assert rc == 7, (damage.__name__, rc)
        assert words in _lib.last_error() and "nann_hnsw_remove_device" in _lib.last_error(), (damage.__name__, _lib.last_error())
        assert untouched(out, stats), damage.__name__
    for wrong in (n_keep - 1, n_keep + 1, n):
        rc, out, stats = _remove_raw(base, rows, bits, wrong, n_up_keep)
        assert rc == 7 and "n_keep" in _lib.last_error(), (wrong, rc, _lib.last_error())
        assert untouched(out, stats), wrong
    # ... and the process goes on: the graph as it was built is accepted, and gives what the Python call gives
    rc, out, stats = _remove_raw(base, rows, bits, n_keep, n_up_keep)
    assert rc == 0 and stats[3] == n_keep
    want = index_build.remove_hnsw_gpu(base, deny_bits=mask, want_export=False)
    assert torch.equal(out[0], want["state"]["adj0"]) and torch.equal(out[1], want["state"]["up_row"])
    assert torch.equal(out[2][:n_up_keep], want["state"]["adj_up"][:n_up_keep]) and stats == list(want["stats"])


# ---- 5, 6. serving and quality: 40 000 x 64 f16 in 16 clusters, M = 16 (the append file's corpus) ------------------------------
# 30 000 survivors keep ~117 nodes with levels > 2: the entry layer still holds the ef = 64 nodes the first top-k asks for
N, D, M, EF = 40_000, 64, 16, 64
TOPN = [EF] * 5 + [100]
_SHARED = {}


def _case(name):
    """(built state over the rows in shuffled order, removed bool[N], what remove_hnsw_gpu returned, queries, item ids)"""
    if name in _SHARED:
        return _SHARED[name]
    from nann_amd import index_build, ops, synth
    embs, assign = synth.make_corpus(N, D, n_clusters=16, noise=1.0)
    order = np.random.default_rng(99).permutation(N)  # the order a build is meant for
    rows = cuda(embs[order])
    if name == "random":
        removed = _random_mask(N, 0.25, 7)
    else:  # the withdrawn seller: one whole cluster leaves
        removed = assign[order] == 15
    base = index_build.build_hnsw_gpu(rows, M, 40, seed=5, want_state=True)["state"]
    res = index_build.remove_hnsw_gpu(base, deny_bits=removed, want_export=False)
    seqs = synth.make_queries_from_centres(D, 64, n_clusters=16, noise=1.0)
    q = ops.user_seq_mean(torch.as_tensor(seqs).cuda())
    _SHARED[name] = (base, removed, res, q, synth.make_item_ids(N))
    return _SHARED[name]


def test_serving_on_the_compacted_graph_matches_the_oracle(oracle):
    from nann_amd import index_build, ops, retrieval
    base, removed, res, q, ids = _case("random")
    st = res["state"]
    kept_ids = ids[res["kept_rows"].cpu().numpy()]
    ex = index_build.export_hnsw_gpu(st)  # device tensors straight into the Index: no host round trip
    dix = retrieval.Index(st["item_embs"], kept_ids, ex["nb_values"], ex["nb_row_splits"], ex["enter_points"])
    sc = ops.Scorer("l2", D)
    r = retrieval.search(dix, sc, q, TOPN)
    torch.cuda.synchronize()
    status = r.status.cpu().numpy()
    assert (status == 0).mean() >= 0.95
    oix = oracle.Index(st["item_embs"].cpu().numpy(), kept_ids, [v.cpu().numpy() for v in ex["nb_values"]],
                       [s.cpu().numpy() for s in ex["nb_row_splits"]], ex["enter_points"].cpu().numpy())
    est, eids, esc, eidx, ectr = oracle.search_batch(oix, oracle.Scorer("l2", D, oracle.EMB_F16), q[:16].cpu().numpy(), TOPN, n_threads=8)
    ok = est == 0
    assert (status[:16] == est).all() and ok.any()
    assert (r.index.cpu().numpy()[:16][ok] == eidx[ok]).all() and (r.item_ids.cpu().numpy()[:16][ok] == eids[ok]).all()
    assert (r.scores.cpu().numpy()[:16][ok].view(np.uint32) == esc[ok].view(np.uint32)).all()
    assert (r.counters.cpu().numpy()[:16][ok] == ectr[ok]).all()
    assert set(np.unique(r.item_ids.cpu().numpy()[status == 0]).tolist()) <= set(kept_ids.tolist())  # no withdrawn item is served


def _recall_and_degree(rows, ex, q):
    """(recall@100 against the exhaustive search of the same index -- a failed request has no hits --, mean level-0 degree, share
    of valid requests)"""
    from nann_amd import ops, retrieval, synth
    n = rows.shape[0]
    dix = retrieval.Index(rows, synth.make_item_ids(n), ex["nb_values"], ex["nb_row_splits"], ex["enter_points"])
    sc = ops.Scorer("l2", D)
    r = retrieval.search(dix, sc, q, TOPN)
    truth = retrieval.search_all(dix, sc, q, 100)
    torch.cuda.synchronize()
    got, want = r.index.cpu().numpy(), truth.index.cpu().numpy()
    ok = r.status.cpu().numpy() == 0
    hits = sum(len(set(got[b].tolist()) & set(want[b].tolist())) for b in range(len(got)) if ok[b])
    return round(hits / want.size, 4), round(ex["nb_values"][0].numel() / n, 3), float(ok.mean())


def _drop_only(base, removed):
    """the compaction that merely drops removed entries and renumbers, in torch from the old arrays: the yardstick that says what
    the repair is worth"""
    keep = torch.as_tensor(~removed).cuda()
    new_id = torch.cumsum(keep.to(torch.int32), 0, dtype=torch.int32) - 1
    lv = np.asarray(base["levels"])

    def renumber(a):
        gone = (a < 0) | ~keep[a.clamp(min=0).long()]
        return torch.where(gone, torch.full_like(a, -1), new_id[a.clamp(min=0).long()])
    owner = torch.as_tensor(np.repeat(np.arange(len(lv)), lv - 1)).cuda()
    n_up = len(owner)
    lvk = lv[~removed].astype(np.int64)
    up_row = np.where(lvk > 1, np.cumsum(lvk - 1) - (lvk - 1), -1).astype(np.int32)
    adj_up = renumber(base["adj_up"][:n_up])[keep[owner]] if n_up else base["adj_up"]
    if adj_up.shape[0] == 0:
        adj_up = torch.full((1, base["M"]), -1, dtype=torch.int32, device="cuda")
    return {"adj0": renumber(base["adj0"])[keep].contiguous(), "up_row": cuda(up_row), "adj_up": adj_up.contiguous(),
            "levels": lv[~removed].astype(np.int32), "M": base["M"]}


@pytest.mark.parametrize("name", ["random", "cluster"])
def test_remove_quality_against_a_rebuild(name):
    """recall@100 of the L2 traversal (truth: the exhaustive search of the same index, a failed request counted as zero hits) on
    the compacted graph within 0.02 of a graph build_hnsw_gpu makes of the survivors in the same order -- the project's own
    builder-against-builder margin (device against host, append against rebuild), for the same reason: contents are not a parity
    target, quality is.  Mean level-0 degree is reported, not gated.  Measured on the MI355X, (recall@100, mean level-0 degree,
    valid share) compacted / rebuilt / drop-only, and stats:
    random 25 % (9 888 of 40 000): (0.9906, 10.606, 1.0) / (0.9469, 14.708, 1.0) / (0.9891, 11.041, 1.0), stats [29306, 0, 12513, 30112];
    one cluster (2 498 of 40 000): (0.9455, 14.622, 1.0) / (0.9213, 14.642, 1.0) / (0.9400, 14.646, 1.0), stats [322, 2, 0, 37502].
    The margin holds here.  At 1M x 128, M 32 (tools/hnsw_remove_rate.py, not gated) it does not: the compacted graph is 0.028 / 0.037
    under the rebuild at 10 % / 25 % removed and under the drop-only compaction too -- re-selecting a whole row discards the
    survivors that back-links had appended without selection (Remove)."""
    from nann_amd import index_build
    base, removed, res, q, _ = _case(name)
    st = res["state"]
    compacted = _recall_and_degree(st["item_embs"], index_build.export_hnsw_gpu(st), q)
    built = index_build.build_hnsw_gpu(st["item_embs"], M, 40, seed=5, want_state=True)["state"]
    rebuilt = _recall_and_degree(st["item_embs"], index_build.export_hnsw_gpu(built), q)
    dropped = _recall_and_degree(st["item_embs"], index_build.export_hnsw_gpu(_drop_only(base, removed)), q)
    print(f"remove quality [{name}]: {int(removed.sum())} of {N} removed, (recall@100, mean L0 degree, valid) compacted {compacted}, "
          f"rebuilt {rebuilt}, drop-only {dropped}, stats {list(res['stats'])}")
    assert compacted[2] >= 0.95 and rebuilt[2] >= 0.95, (compacted, rebuilt)
    assert compacted[0] >= rebuilt[0] - 0.02, (compacted, rebuilt)
