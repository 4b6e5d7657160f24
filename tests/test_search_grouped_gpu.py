"""-m gpu: the searches under a group cap.  search_grouped / search_model_grouped (nann_search_grouped, nann_search_model_grouped)
against the numpy cap model (groupcap_model.model) applied to what the existing retrieval.search / search_model returns for the
same queries at the same fetch width F -- search is pinned to the oracle elsewhere, and the match is bitwise because the same
call produced the cap's input.  search_all_grouped / search_all_model_grouped against the model over the references' brute-force
ranking of the allowed rows.  Index of the traversal tests: 2 000 rows x 64-d f16 on the shipped builder's graph, level_topn
[8, 16, 32, 32, 32, F = 50]; the exhaustive tests: 300 rows.  Groups: row % G for G in {1, 7, n_items}, rows 50 .. 79 ungrouped."""
import ctypes as C

import numpy as np
import pytest
import torch

import groupcap_model as GM
import ip_reference as R
from gpu_util import bits, cuda, queries_for, require_gpu, synth_index
from test_search_all_gpu import _brute, _ring

pytestmark = pytest.mark.gpu
N, D, F = 2000, 64, 50
TOPN = [8, 16, 32, 32, 32, F]
NS, FETCH, K_SHORT, CAP_SHORT = 300, 20, 14, 2      # the exhaustive tests; the case of a fetch width below n_items
BAD_ARGUMENT, TOPK_K_GT_N, UNSUPPORTED, CAPACITY = 7, 4, 102, 103
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _group_of_row(n, g):
    gor = (np.arange(n) % g).astype(np.int32)
    gor[50:80] = -1
    return gor


def _got(r):
    torch.cuda.synchronize()
    return {"item_ids": r.item_ids.cpu().numpy(), "scores": r.scores.cpu().numpy(), "index": r.index.cpu().numpy(),
            "group": r.group.cpu().numpy(), "n_out": r.n_out.cpu().numpy()}


def _same(got, exp, what=""):
    for name in ("n_out", "index", "group", "item_ids", "scores"):
        g, e = (bits(got[name]), bits(exp[name])) if name == "scores" else (got[name], exp[name])
        assert g.shape == e.shape and (g == e).all(), (what, name)


# ---- the traversal forms ----------------------------------------------------------------------------------------------------
def _index():
    return synth_index(N, D, 64)


def _queries(oracle, n, seed=4321):
    seqs = queries_for(_index()[0], n, seed=seed)
    return seqs, np.stack([oracle.user_seq_mean(s) for s in seqs]).astype(np.float32)


def _scorer(kind):
    from nann_amd import ops, synth
    if kind in ("l2", "ip"):
        return ops.Scorer(kind, D)
    return ops.Scorer("mlp", D, torch.float16, synth.make_mlp_weights(D), precision={"mlp_exact": "exact", "mlp_split": "split"}[kind])


def _expect_from(r, level_topn, dix, gor, cap, k, caps=None, deny=None, exclude=None):
    """the cap model over an unfiltered search's answer -> (model dict, status)"""
    torch.cuda.synchronize()
    status = r.status.cpu().numpy()
    lt = np.asarray(level_topn)
    width = np.full(len(status), lt[5]) if lt.ndim == 1 else lt[:, 5]
    n_valid = np.where(status != 0, 0, width).astype(np.int32)
    exp = GM.model(r.scores.cpu().numpy(), r.index.cpu().numpy(), n_valid, dix.n_items, gor, cap, k, caps=caps,
                   item_ids=dix.item_ids.cpu().numpy(), deny=deny, exclude=exclude)
    return exp, status


@pytest.mark.parametrize("kind", ["l2", "ip", "mlp_exact", "mlp_split"])
def test_search_grouped_is_the_cap_over_search(oracle, kind):
    from nann_amd import retrieval
    dix = _index()[2]
    sc = _scorer(kind)
    _, q = _queries(oracle, 12)
    plain = retrieval.search(dix, sc, cuda(q), TOPN)
    for g, cap, k in ((1, 3, 20), (7, 2, 14), (7, 1, 5), (N, 1, F)):
        gor = _group_of_row(N, g)
        exp, status = _expect_from(plain, TOPN, dix, gor, cap, k)
        groups = retrieval.make_groups(dix, group_of_row=gor, cap=cap)
        r = retrieval.search_grouped(dix, sc, cuda(q), TOPN, groups, k=k)
        _same(_got(r), exp, (kind, g, cap, k))
        assert (r.status.cpu().numpy() == status).all() and (status == 0).all()
        assert (r.counters.cpu().numpy() == plain.counters.cpu().numpy()).all() and r.plan == plain.plan
        if g == N:
            assert (exp["n_out"] == F).all() and (exp["index"] == plain.index.cpu().numpy()).all()  # nothing capped: search itself
        if g == 1:
            ungrouped = ((plain.index.cpu().numpy() >= 50) & (plain.index.cpu().numpy() < 80)).sum(1)
            assert (exp["n_out"] == np.minimum(k, cap + ungrouped)).all()


def test_filter_first_then_cap_and_caps_per_query(oracle):
    from nann_amd import retrieval
    dix = _index()[2]
    sc = _scorer("l2")
    _, q = _queries(oracle, 12, seed=21)
    plain = retrieval.search(dix, sc, cuda(q), TOPN)
    rows = plain.index.cpu().numpy()
    rng = np.random.default_rng(5)
    deny = rng.random(N) < 0.3
    exclude = [np.concatenate([rows[i, :6], rng.integers(0, N, 20)]).astype(np.int64) for i in range(12)]
    gor = _group_of_row(N, 7)
    caps = np.array([1, 2, 0, 3, -1, 1, 2, 50, 1, 2, 3, 4], np.int32)
    flt = retrieval.make_filter(dix, deny_rows=np.nonzero(deny)[0], exclude_rows=exclude)
    exp, _ = _expect_from(plain, TOPN, dix, gor, 1, 30, caps=caps, deny=deny, exclude=exclude)
    r = retrieval.search_grouped(dix, sc, cuda(q), TOPN, retrieval.make_groups(dix, group_of_row=gor, caps=caps), k=30, filter=flt)
    got = _got(r)
    _same(got, exp)
    for i in range(12):
        kept = got["index"][i, :got["n_out"][i]]
        assert not deny[kept].any() and not np.isin(kept, exclude[i]).any()
    # the filter alone, through the existing filtered call: the uncapped queries (caps <= 0) return exactly its answer
    only = retrieval.search(dix, sc, cuda(q), TOPN, filter=flt, k=30)
    torch.cuda.synchronize()
    for i in (2, 4):
        assert (got["index"][i] == only.index.cpu().numpy()[i]).all() and got["n_out"][i] == only.n_out.cpu().numpy()[i]


def test_a_failed_query_fails_alone(oracle):
    from nann_amd import retrieval
    dix = _index()[2]
    sc = _scorer("l2")
    _, q = _queries(oracle, 8, seed=13)
    lt = np.tile(np.array(TOPN, np.int32), (8, 1))
    lt[4] = [8, 4, 4, 4, 4, F]       # query 4: a pool of 16 rows cannot give 50
    lt[6, 5] = 20                    # query 6 asks for 20 only
    plain = retrieval.search(dix, sc, cuda(q), lt)
    gor = _group_of_row(N, 7)
    exp, status = _expect_from(plain, lt, dix, gor, 2, 14)
    assert status[4] != 0 and (np.delete(status, 4) == 0).all()
    r = retrieval.search_grouped(dix, sc, cuda(q), lt, retrieval.make_groups(dix, group_of_row=gor, cap=2), k=14)
    got = _got(r)
    _same(got, exp)
    assert (r.status.cpu().numpy() == status).all()
    assert got["n_out"][4] == 0 and not got["index"][4].any() and not got["item_ids"][4].any() and not bits(got["scores"][4]).any()
    assert (np.delete(got["n_out"], 4) > 0).all()


def test_the_model_form(oracle, tmp_path):
    from nann_amd import ops, retrieval
    dix = _index()[2]
    seqs, q = _queries(oracle, 12)
    ops.save_scorer_dir(str(tmp_path / "l2"), "l2")
    m = ops.Model(str(tmp_path / "l2"), D, seqs.shape[1])
    plain = retrieval.search_model(dix, m, cuda(seqs, torch.float16), TOPN)
    gor = _group_of_row(N, 7)
    exp, status = _expect_from(plain, TOPN, dix, gor, 2, 14)
    groups = retrieval.make_groups(dix, group_of_row=gor, cap=2)
    r = retrieval.search_model_grouped(dix, m, cuda(seqs, torch.float16), TOPN, groups, k=14)
    _same(_got(r), exp)
    assert (r.status.cpu().numpy() == status).all() and r.plan == plain.plan
    # ... and the bits of the scorer form over the sequences' means
    _same(_got(retrieval.search_grouped(dix, _scorer("l2"), cuda(q), TOPN, groups, k=14)), exp)


def test_search_multi_then_cap_groups(oracle):
    """the documented composition: the union of a user's vectors, then the cap over the union's ranked list"""
    import union_model as UM
    from nann_amd import retrieval
    dix = _index()[2]
    sc = _scorer("l2")
    n_users, n_vec = 5, 4
    _, q = _queries(oracle, n_users * n_vec, seed=31)
    q = q.reshape(n_users, n_vec, D)
    per = retrieval.search(dix, sc, cuda(q.reshape(-1, D)), TOPN)
    torch.cuda.synchronize()
    assert (per.status.cpu().numpy() == 0).all()
    union = UM.model(per.scores.cpu().numpy().reshape(n_users, n_vec, F), per.index.cpu().numpy().reshape(n_users, n_vec, F), None,
                     N, 120, item_ids=dix.item_ids.cpu().numpy())
    gor = _group_of_row(N, 7)
    exp = GM.model(union["scores"], union["index"], union["n_out"], N, gor, 3, 21, item_ids=dix.item_ids.cpu().numpy())
    multi = retrieval.search_multi(dix, sc, cuda(q), TOPN, k=120)
    r = retrieval.cap_groups(multi.scores, multi.index, retrieval.make_groups(dix, group_of_row=gor, cap=3), 21, n_valid=multi.n_out,
                             index=dix)
    got = _got(r)
    _same(got, exp)
    assert (r.pos.cpu().numpy() == exp["pos"]).all() and (got["n_out"] == 21).all()


# ---- the exhaustive forms ---------------------------------------------------------------------------------------------------
def _small():
    """300 rows x 64-d f16 with ten duplicated rows (ties across rows): (embs, item ids, oracle index)"""
    if "small" not in _CACHE:
        from oracle import oracle as O
        rng = np.random.default_rng(31)
        embs = rng.standard_normal((NS, D)).astype(np.float16)
        embs[100:110] = embs[0:10]
        ids = np.arange(NS, dtype=np.int64) * 7 + 3
        nbv, rs, ep = _ring(NS)
        _CACHE["small"] = (embs, ids, O.Index(embs, ids, nbv, rs, ep))
    return _CACHE["small"]


def _small_device():
    if "small_dev" not in _CACHE:
        from nann_amd import retrieval
        embs, ids, _ = _small()
        _CACHE["small_dev"] = retrieval.Index(embs, ids, *_ring(NS))
    return _CACHE["small_dev"]


def _ranking(oracle, metric, q, deny):
    """every query's brute-force ranking of the allowed rows, from the references -> (rows i32[B, n_allowed], scores f32)"""
    embs, _, oix = _small()
    if metric == "ip":
        full = np.stack([R.ip_scores(v, R.widen(embs)) for v in q])
    else:
        rows, scores = _brute(oracle, oix, oracle.Scorer("l2", D, oracle.EMB_F16), q, NS)
        full = np.empty((len(q), NS), np.float32)
        np.put_along_axis(full, rows.astype(np.int64), scores, axis=1)
    allowed = np.nonzero(~deny)[0]
    tops = np.stack([allowed[R.topk_stable(s[allowed], len(allowed))] for s in full])
    return tops.astype(np.int32), np.take_along_axis(full, tops, axis=1)


def _deny_small():
    return np.random.default_rng(17).random(NS) < 0.2


def _exhaustive_expect(oracle, metric, q, g, cap, k, fetch, deny):
    rows, scores = _ranking(oracle, metric, q, deny)
    _, ids, _ = _small()
    return GM.model(scores[:, :fetch], rows[:, :fetch], None, NS, _group_of_row(NS, g), cap, k, item_ids=ids)


def _q_small(seed=40):
    return np.random.default_rng(seed).standard_normal((16, D)).astype(np.float32)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_search_all_grouped_over_the_whole_ranking(oracle, metric):
    from nann_amd import ops, retrieval
    dix = _small_device()
    sc = ops.Scorer(metric, D)
    q = _q_small()
    none = np.zeros(NS, bool)
    for g, cap, k in ((1, 3, 10), (7, 2, 14), (7, 40, 300), (NS, 1, 300)):
        groups = retrieval.make_groups(dix, group_of_row=_group_of_row(NS, g), cap=cap)
        exp = _exhaustive_expect(oracle, metric, q, g, cap, k, NS, none)
        _same(_got(retrieval.search_all_grouped(dix, sc, cuda(q), k, groups, fetch=NS)), exp, (metric, g, cap, k))
    # under a filter: the ranking of the allowed rows
    deny = _deny_small()
    flt = retrieval.make_filter(dix, deny_rows=np.nonzero(deny)[0])
    groups = retrieval.make_groups(dix, group_of_row=_group_of_row(NS, 7), cap=2)
    n_allowed = int((~deny).sum())
    exp = _exhaustive_expect(oracle, metric, q, 7, 2, 14, n_allowed, deny)
    got = _got(retrieval.search_all_grouped(dix, sc, cuda(q), 14, groups, fetch=NS, filter=flt))
    _same(got, exp, (metric, "filtered"))
    assert (got["n_out"] == 14).all() and not deny[got["index"]].any()


# (queries whose answer at FETCH = 20 is complete, n_out == k; queries it cuts short) at k = 14, cap = 2, of 16 queries, under
# _deny_small(): counted once on the references, written down so that a pass with every query cut short cannot go unnoticed
COUNTS = {("l2", 7): (11, 5), ("ip", 7): (11, 5), ("l2", 1): (0, 16), ("ip", 1): (0, 16), ("l2", NS): (16, 0), ("ip", NS): (16, 0)}


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("g", [1, 7, NS])
def test_a_fetch_width_below_n_items_gives_a_prefix(oracle, metric, g):
    from nann_amd import ops, retrieval
    dix = _small_device()
    sc = ops.Scorer(metric, D)
    q = _q_small(seed=41)
    deny = _deny_small()
    flt = retrieval.make_filter(dix, deny_rows=np.nonzero(deny)[0])
    groups = retrieval.make_groups(dix, group_of_row=_group_of_row(NS, g), cap=CAP_SHORT)
    whole = _exhaustive_expect(oracle, metric, q, g, CAP_SHORT, K_SHORT, int((~deny).sum()), deny)
    short = _exhaustive_expect(oracle, metric, q, g, CAP_SHORT, K_SHORT, FETCH, deny)
    got = _got(retrieval.search_all_grouped(dix, sc, cuda(q), K_SHORT, groups, fetch=FETCH, filter=flt))
    _same(got, short, (metric, g))
    complete = got["n_out"] == K_SHORT
    print("complete %d, cut short %d" % (complete.sum(), (~complete).sum()))
    assert (int(complete.sum()), int((~complete).sum())) == COUNTS[metric, g]
    for i in range(16):
        m = got["n_out"][i]
        assert m <= whole["n_out"][i]
        for name in ("index", "group", "item_ids"):
            assert (got[name][i, :m] == whole[name][i, :m]).all(), (i, name)        # a prefix of the answer over the whole ranking
        assert (bits(got["scores"][i, :m]) == bits(whole["scores"][i, :m])).all()
        if complete[i]:
            assert all((got[name][i] == whole[name][i]).all() for name in ("index", "group", "item_ids"))
    if g == 1:
        ungrouped = ((short["index"] >= 50) & (short["index"] < 80) & (np.arange(K_SHORT) < short["n_out"][:, None])).sum(1)
        assert (got["n_out"] - ungrouped == min(CAP_SHORT, K_SHORT)).all()


def test_search_all_model_grouped(oracle, tmp_path):
    from nann_amd import ops, retrieval
    dix = _small_device()
    rng = np.random.default_rng(43)
    seqs = rng.standard_normal((16, 5, D)).astype(np.float16)
    q = np.stack([oracle.user_seq_mean(s) for s in seqs]).astype(np.float32)
    ops.save_scorer_dir(str(tmp_path / "l2"), "l2")
    m = ops.Model(str(tmp_path / "l2"), D, 5)
    deny = _deny_small()
    flt = retrieval.make_filter(dix, deny_rows=np.nonzero(deny)[0])
    groups = retrieval.make_groups(dix, group_of_row=_group_of_row(NS, 7), cap=2)
    exp = _exhaustive_expect(oracle, "l2", q, 7, 2, 14, int((~deny).sum()), deny)
    _same(_got(retrieval.search_all_model_grouped(dix, m, cuda(seqs, torch.float16), 14, groups, fetch=NS, filter=flt)), exp)
    exp = _exhaustive_expect(oracle, "l2", q, 7, 2, 14, NS, np.zeros(NS, bool))
    _same(_got(retrieval.search_all_model_grouped(dix, m, cuda(seqs, torch.float16), 14, groups, fetch=NS)), exp)
    with pytest.raises(TypeError):
        retrieval.search_all_model_grouped(dix, ops.Scorer("l2", D), cuda(seqs, torch.float16), 14, groups)


# ---- refusals launch nothing ------------------------------------------------------------------------------------------------
def _canaries(b, k):
    return {"item_ids": torch.full((b, k), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64).cuda(), "scores": torch.full((b, k), 777.0).cuda(),
            "index": torch.full((b, k), 0x5A5A5A5A, dtype=torch.int32).cuda(), "group": torch.full((b, k), 0x5A5A5A5A, dtype=torch.int32).cuda(),
            "n_out": torch.full((b,), 0x5A5A5A5A, dtype=torch.int32).cuda(), "status": torch.full((b,), 0x5A5A5A5A, dtype=torch.int32).cuda()}


def _untouched(o):
    torch.cuda.synchronize()
    assert (o["item_ids"].cpu() == 0x5A5A5A5A5A5A5A5A).all() and (o["scores"].cpu() == 777.0).all()
    assert all((o[n].cpu() == 0x5A5A5A5A).all() for n in ("index", "group", "n_out", "status"))


def _struct(gor, cap=2, struct_bytes=None, null_rows=False):
    from nann_amd import _lib
    g = _lib.Groups()
    g.struct_bytes = C.sizeof(_lib.Groups) if struct_bytes is None else struct_bytes
    g.group_of_row = None if null_rows else gor.data_ptr()
    g.cap = cap
    return g


def test_search_grouped_refusals_launch_nothing(oracle):
    from nann_amd import _lib
    from nann_amd.ops import _ptr, _stream
    L = _lib.lib()
    dix = _index()[2]
    sc = _scorer("l2")
    b, k = 6, 20
    _, q = _queries(oracle, b, seed=14)
    qd = cuda(q)
    gor = cuda(_group_of_row(N, 7), torch.int32)
    t = (C.c_int32 * 6)(*TOPN)
    nb, plain = C.c_int64(-1), C.c_int64(-1)
    assert L.nann_search_grouped_workspace_bytes(dix.handle, t, b, C.byref(nb)) == 0
    assert L.nann_search_filtered_workspace_bytes(dix.handle, t, b, C.byref(plain)) == 0 and nb.value == plain.value > 0
    ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    o = _canaries(b, k)

    def call(groups, kk=k, ws_bytes=nb.value):
        return L.nann_search_grouped(dix.handle, sc.handle, _ptr(qd), b, t, None, _ptr(ws), ws_bytes, _ptr(o["item_ids"]),
                                     _ptr(o["scores"]), _ptr(o["index"]), _ptr(o["status"]), None, None, None, None, None,
                                     C.byref(groups) if groups is not None else None, kk, _ptr(o["group"]), _ptr(o["n_out"]), _stream())

    ok = _struct(gor)
    assert call(ok, kk=F + 1) == BAD_ARGUMENT and b"level_topn_max[5]" in L.nann_last_error()
    assert call(ok, kk=-1) == BAD_ARGUMENT
    assert call(None) == BAD_ARGUMENT and b"nann_search_grouped" in L.nann_last_error()
    assert call(_struct(gor, struct_bytes=12)) == BAD_ARGUMENT
    assert call(_struct(gor, null_rows=True)) == BAD_ARGUMENT
    assert call(_struct(gor, cap=0)) == BAD_ARGUMENT and b"cap < 1" in L.nann_last_error()
    assert call(ok, ws_bytes=nb.value - 1) == CAPACITY and b"nann_search_grouped_workspace_bytes" in L.nann_last_error()
    _untouched(o)
    assert call(ok) == 0
    torch.cuda.synchronize()
    n_out = o["n_out"].cpu().numpy()
    assert (o["status"].cpu() == 0).all() and (n_out > 0).all() and (n_out <= k).all()
    assert all((o["group"].cpu().numpy()[i, :n_out[i]] < 7).all() for i in range(b))


def test_search_all_grouped_refusals_launch_nothing(oracle):
    from nann_amd import _lib, ops
    from nann_amd.ops import _ptr, _stream
    L = _lib.lib()
    dix = _small_device()
    sc = ops.Scorer("l2", D)
    b, k = 4, 14
    qd = cuda(_q_small()[:b])
    gor = cuda(_group_of_row(NS, 7), torch.int32)
    nb, inner = C.c_int64(-1), C.c_int64(-1)
    assert L.nann_search_all_grouped_workspace_bytes(dix.handle, sc.handle, b, NS + 1, C.byref(nb)) == TOPK_K_GT_N
    assert L.nann_search_all_grouped_workspace_bytes(dix.handle, sc.handle, b, -1, C.byref(nb)) == BAD_ARGUMENT
    assert nb.value == -1
    assert L.nann_search_all_grouped_workspace_bytes(dix.handle, sc.handle, b, 100, C.byref(nb)) == 0
    assert L.nann_search_all_filtered_workspace_bytes(dix.handle, sc.handle, b, 100, C.byref(inner)) == 0
    assert nb.value == (inner.value + 255) // 256 * 256 + (b * 100 * 16 + b * 4 + 255) // 256 * 256   # the staging list and its n_out
    ws = torch.empty(nb.value + 256, dtype=torch.uint8, device="cuda")
    base = (ws.data_ptr() + 255) // 256 * 256
    o = _canaries(b, k)

    def call(groups, fetch=100, kk=k, w=base, ws_bytes=nb.value):
        return L.nann_search_all_grouped(dix.handle, sc.handle, _ptr(qd), b, fetch, kk, _ptr(o["item_ids"]), _ptr(o["scores"]),
                                         _ptr(o["index"]), _ptr(o["group"]), C.c_void_p(w) if w else None, ws_bytes, None, None,
                                         C.byref(groups) if groups is not None else None, _ptr(o["n_out"]), _stream())

    ok = _struct(gor)
    assert call(ok, kk=101) == BAD_ARGUMENT and b"[0, fetch]" in L.nann_last_error()
    assert call(ok, kk=-1) == BAD_ARGUMENT
    assert call(ok, fetch=NS + 1) == TOPK_K_GT_N
    assert call(ok, fetch=1025, kk=k) in (TOPK_K_GT_N, UNSUPPORTED)       # (beyond n_items here; beyond 1024 on a larger index)
    assert call(None) == BAD_ARGUMENT
    assert call(_struct(gor, cap=0)) == BAD_ARGUMENT
    assert call(_struct(gor, struct_bytes=8)) == BAD_ARGUMENT
    assert call(ok, ws_bytes=nb.value - 1) == CAPACITY and b"nann_search_all_grouped_workspace_bytes" in L.nann_last_error()
    assert call(ok, w=0) == CAPACITY
    assert call(ok, w=base + 64) == BAD_ARGUMENT and b"256-byte aligned" in L.nann_last_error()
    o["status"].fill_(0x5A5A5A5A)
    _untouched(o)
    assert call(ok, kk=0) == 0
    _untouched(o)
    assert call(ok) == 0
    torch.cuda.synchronize()
    assert (o["n_out"].cpu() == 14).all()
