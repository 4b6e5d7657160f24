"""-m gpu: the searches with diversified results.  search_diverse / search_model_diverse (nann_search_diverse,
nann_search_model_diverse) against the numpy MMR model (mmr_model.model) applied to what the existing retrieval.search /
search_model returns for the same queries at the same fetch width F -- search is pinned to the oracle elsewhere, and the match
is bitwise because the same call produced the model's input, whatever precision scored it.  search_all_diverse /
search_all_model_diverse against the model over what search_all returns at k = fetch.  Index of the traversal tests: 2 000 rows x
64-d f16 on the shipped builder's graph, level_topn [8, 16, 32, 32, 32, F = 50]; the exhaustive tests: 300 rows."""
import ctypes as C

import numpy as np
import pytest
import torch

import mmr_model as MM
from gpu_util import bits, cuda, queries_for, require_gpu, synth_index
from test_search_all_gpu import _ring

pytestmark = pytest.mark.gpu
N, D, F = 2000, 64, 50
TOPN = [8, 16, 32, 32, 32, F]
NS = 300
BAD_ARGUMENT, TOPK_K_GT_N, UNSUPPORTED, CAPACITY = 7, 4, 102, 103
OUTPUTS = ("n_out", "index", "pos", "item_ids", "scores", "mmr")
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _got(r):
    torch.cuda.synchronize()
    return {n: getattr(r, n).cpu().numpy() for n in OUTPUTS}


def _same(got, exp, what=""):
    for name in OUTPUTS:
        g, e = (bits(got[name]), bits(exp[name])) if name in ("scores", "mmr") else (got[name], exp[name])
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


def _expect_from(r, level_topn, lam, sim, k, lams=None, deny=None, exclude=None):
    """the MMR model over an unfiltered search's answer -> (model dict, status)"""
    torch.cuda.synchronize()
    g, _, dix = _index()
    status = r.status.cpu().numpy()
    lt = np.asarray(level_topn)
    width = np.full(len(status), lt[5]) if lt.ndim == 1 else lt[:, 5]
    exp = MM.model(r.scores.cpu().numpy(), r.index.cpu().numpy(), width, g["item_embs"], lam, sim, k, lams=lams,
                   item_ids=dix.item_ids.cpu().numpy(), deny=deny, exclude=exclude, status=status)
    return exp, status


@pytest.mark.parametrize("kind", ["l2", "ip", "mlp_exact", "mlp_split"])
def test_search_diverse_is_mmr_over_search(oracle, kind):
    from nann_amd import retrieval
    dix = _index()[2]
    sc = _scorer(kind)
    _, q = _queries(oracle, 12)
    plain = retrieval.search(dix, sc, cuda(q), TOPN)
    default = "ip" if kind == "ip" else "l2"
    for lam, sim, k in ((0.5, None, 20), (0.5, "ip", F), (0.0, "l2", 14), (0.25, None, 1)):
        exp, status = _expect_from(plain, TOPN, lam, sim or default, k)
        r = retrieval.search_diverse(dix, sc, cuda(q), TOPN, retrieval.make_diversity(lam=lam, sim=sim), k=k)
        _same(_got(r), exp, (kind, lam, sim, k))
        assert (r.status.cpu().numpy() == status).all() and (status == 0).all() and (exp["n_out"] == k).all()
        assert (r.counters.cpu().numpy() == plain.counters.cpu().numpy()).all() and r.plan == plain.plan
    # diversity does something here: at lambda 0.5 the picks are not the plain prefix for every query
    half = _got(retrieval.search_diverse(dix, sc, cuda(q), TOPN, retrieval.make_diversity(lam=0.5), k=20))
    assert (half["index"] != plain.index.cpu().numpy()[:, :20]).any()


@pytest.mark.parametrize("kind", ["l2", "ip", "mlp_split"])
def test_lambda_one_is_the_plain_calls_first_k(oracle, kind):
    from nann_amd import retrieval
    dix = _index()[2]
    sc = _scorer(kind)
    _, q = _queries(oracle, 12, seed=77)
    plain = retrieval.search(dix, sc, cuda(q), TOPN)
    got = _got(retrieval.search_diverse(dix, sc, cuda(q), TOPN, retrieval.make_diversity(lam=1.0), k=20))
    assert (got["index"] == plain.index.cpu().numpy()[:, :20]).all() and (got["item_ids"] == plain.item_ids.cpu().numpy()[:, :20]).all()
    assert (bits(got["scores"]) == bits(plain.scores.cpu().numpy()[:, :20])).all()
    assert (got["mmr"] == got["scores"]).all()                               # b = 0: v = 1 * s - 0 * p
    assert (got["pos"] == np.arange(20)).all() and (got["n_out"] == 20).all()


def test_filter_first_then_mmr_and_lambdas_per_query(oracle):
    from nann_amd import retrieval
    dix = _index()[2]
    sc = _scorer("l2")
    _, q = _queries(oracle, 12, seed=21)
    plain = retrieval.search(dix, sc, cuda(q), TOPN)
    rows = plain.index.cpu().numpy()
    rng = np.random.default_rng(5)
    deny = rng.random(N) < 0.3
    exclude = [np.concatenate([rows[i, :6], rng.integers(0, N, 20)]).astype(np.int64) for i in range(12)]
    lams = np.array([0.0, 0.5, 1.0, 2.0, np.nan, 0.25, 0.75, 0.5, 1.0, 0.1, 0.9, -3.0], np.float32)
    flt = retrieval.make_filter(dix, deny_rows=np.nonzero(deny)[0], exclude_rows=exclude)
    exp, _ = _expect_from(plain, TOPN, 0.5, "l2", 30, lams=lams, deny=deny, exclude=exclude)
    r = retrieval.search_diverse(dix, sc, cuda(q), TOPN, retrieval.make_diversity(lams=lams), k=30, filter=flt)
    got = _got(r)
    _same(got, exp)
    for i in range(12):
        kept = got["index"][i, :got["n_out"][i]]
        assert got["n_out"][i] > 0 and not deny[kept].any() and not np.isin(kept, exclude[i]).any()      # a denied row never appears
    # the filter alone, through the existing filtered call: the queries with lambda 1 return exactly its answer
    only = retrieval.search(dix, sc, cuda(q), TOPN, filter=flt, k=30)
    torch.cuda.synchronize()
    for i in (2, 3, 8):
        assert (got["index"][i] == only.index.cpu().numpy()[i]).all() and got["n_out"][i] == only.n_out.cpu().numpy()[i]
    # a deny bitmap alone, an exclusion list alone
    for kw, mk in ((dict(deny=deny), dict(deny_rows=np.nonzero(deny)[0])), (dict(exclude=exclude), dict(exclude_rows=exclude))):
        exp, _ = _expect_from(plain, TOPN, 0.5, "l2", 30, **kw)
        r = retrieval.search_diverse(dix, sc, cuda(q), TOPN, retrieval.make_diversity(), k=30, filter=retrieval.make_filter(dix, **mk))
        _same(_got(r), exp, tuple(kw))


def test_a_failed_query_fails_alone(oracle):
    from nann_amd import retrieval
    dix = _index()[2]
    sc = _scorer("l2")
    _, q = _queries(oracle, 8, seed=13)
    lt = np.tile(np.array(TOPN, np.int32), (8, 1))
    lt[4] = [8, 4, 4, 4, 4, F]       # query 4: a pool of 16 rows cannot give 50
    lt[6, 5] = 20                    # query 6 asks for 20 only
    plain = retrieval.search(dix, sc, cuda(q), lt)
    exp, status = _expect_from(plain, lt, 0.5, "l2", 30)
    assert status[4] != 0 and (np.delete(status, 4) == 0).all()
    r = retrieval.search_diverse(dix, sc, cuda(q), lt, retrieval.make_diversity(), k=30)
    got = _got(r)
    _same(got, exp)
    assert (r.status.cpu().numpy() == status).all()
    assert got["n_out"][4] == 0 and not got["index"][4].any() and not got["item_ids"][4].any() and not bits(got["scores"][4]).any()
    assert got["n_out"][6] == 20 and (np.delete(got["n_out"], [4, 6]) == 30).all()


def test_the_model_form(oracle, tmp_path):
    from nann_amd import ops, retrieval
    dix = _index()[2]
    seqs, q = _queries(oracle, 12)
    for kind in ("l2", "ip"):
        ops.save_scorer_dir(str(tmp_path / kind), kind)
        m = ops.Model(str(tmp_path / kind), D, seqs.shape[1])
        plain = retrieval.search_model(dix, m, cuda(seqs, torch.float16), TOPN)
        exp, status = _expect_from(plain, TOPN, 0.5, kind, 14)                       # sim=None follows the model's kind
        dv = retrieval.make_diversity()
        r = retrieval.search_model_diverse(dix, m, cuda(seqs, torch.float16), TOPN, dv, k=14)
        _same(_got(r), exp, kind)
        assert (r.status.cpu().numpy() == status).all() and r.plan == plain.plan
        # ... and the bits of the scorer form over the sequences' means
        _same(_got(retrieval.search_diverse(dix, _scorer(kind), cuda(q), TOPN, dv, k=14)), exp, kind)


def test_search_then_mmr_is_search_diverse(oracle):
    """the step on its own over the plain call's outputs: the documented composition"""
    from nann_amd import retrieval
    dix = _index()[2]
    sc = _scorer("l2")
    _, q = _queries(oracle, 6, seed=31)
    plain = retrieval.search(dix, sc, cuda(q), TOPN)
    dv = retrieval.make_diversity(lam=0.4, sim="l2")
    a = _got(retrieval.mmr(dix, plain.scores, plain.index, dv, 25))
    b = _got(retrieval.search_diverse(dix, sc, cuda(q), TOPN, dv, k=25))
    _same(a, b)


# ---- the exhaustive forms ---------------------------------------------------------------------------------------------------
def _small():
    """300 rows x 64-d f16 with ten duplicated rows (ties across rows): (embs, item ids, device index)"""
    if "small" not in _CACHE:
        from nann_amd import retrieval
        rng = np.random.default_rng(31)
        embs = rng.standard_normal((NS, D)).astype(np.float16)
        embs[100:110] = embs[0:10]
        ids = np.arange(NS, dtype=np.int64) * 7 + 3
        _CACHE["small"] = (embs, ids, retrieval.Index(embs, ids, *_ring(NS)))
    return _CACHE["small"]


def _deny_small():
    return np.random.default_rng(17).random(NS) < 0.2


def _q_small(seed=40):
    return np.random.default_rng(seed).standard_normal((16, D)).astype(np.float32)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_search_all_diverse_is_mmr_over_search_all(oracle, metric):
    from nann_amd import ops, retrieval
    embs, ids, dix = _small()
    sc = ops.Scorer(metric, D)
    q = _q_small()
    for fetch, k, lam in ((NS, 40, 0.5), (20, 14, 0.5), (20, 20, 0.0), (64, 10, 1.0)):
        plain = retrieval.search_all(dix, sc, cuda(q), fetch)
        torch.cuda.synchronize()
        exp = MM.model(plain.scores.cpu().numpy(), plain.index.cpu().numpy(), None, embs, lam, metric, k, item_ids=ids)
        got = _got(retrieval.search_all_diverse(dix, sc, cuda(q), k, retrieval.make_diversity(lam=lam), fetch=fetch))
        _same(got, exp, (metric, fetch, k, lam))
        if lam == 1.0:
            assert (got["index"] == plain.index.cpu().numpy()[:, :k]).all()
    # under a filter: MMR over the top fetch of the allowed rows
    deny = _deny_small()
    flt = retrieval.make_filter(dix, deny_rows=np.nonzero(deny)[0])
    for fetch in (20, NS):
        plain = retrieval.search_all(dix, sc, cuda(q), fetch, filter=flt)
        torch.cuda.synchronize()
        exp = MM.model(plain.scores.cpu().numpy(), plain.index.cpu().numpy(), plain.n_out.cpu().numpy(), embs, 0.5, metric, 14,
                       item_ids=ids)
        got = _got(retrieval.search_all_diverse(dix, sc, cuda(q), 14, retrieval.make_diversity(), fetch=fetch, filter=flt))
        _same(got, exp, (metric, "filtered", fetch))
        assert (got["n_out"] == 14).all() and not deny[got["index"]].any()


def test_search_all_model_diverse(oracle, tmp_path):
    from nann_amd import ops, retrieval
    embs, ids, dix = _small()
    rng = np.random.default_rng(43)
    seqs = rng.standard_normal((16, 5, D)).astype(np.float16)
    q = np.stack([oracle.user_seq_mean(s) for s in seqs]).astype(np.float32)
    ops.save_scorer_dir(str(tmp_path / "l2"), "l2")
    m = ops.Model(str(tmp_path / "l2"), D, 5)
    dv = retrieval.make_diversity(lam=0.3)
    by_scorer = _got(retrieval.search_all_diverse(dix, ops.Scorer("l2", D), cuda(q), 14, dv, fetch=40))
    _same(_got(retrieval.search_all_model_diverse(dix, m, cuda(seqs, torch.float16), 14, dv, fetch=40)), by_scorer)
    plain = retrieval.search_all(dix, ops.Scorer("l2", D), cuda(q), 40)
    torch.cuda.synchronize()
    _same(by_scorer, MM.model(plain.scores.cpu().numpy(), plain.index.cpu().numpy(), None, embs, 0.3, "l2", 14, item_ids=ids))
    with pytest.raises(TypeError):
        retrieval.search_all_model_diverse(dix, ops.Scorer("l2", D), cuda(seqs, torch.float16), 14, dv)


# ---- refusals launch nothing ------------------------------------------------------------------------------------------------
def _canaries(b, k):
    return {"item_ids": torch.full((b, k), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64).cuda(), "scores": torch.full((b, k), 777.0).cuda(),
            "mmr": torch.full((b, k), 777.0).cuda(), "index": torch.full((b, k), 0x5A5A5A5A, dtype=torch.int32).cuda(),
            "pos": torch.full((b, k), 0x5A5A5A5A, dtype=torch.int32).cuda(),
            "n_out": torch.full((b,), 0x5A5A5A5A, dtype=torch.int32).cuda(), "status": torch.full((b,), 0x5A5A5A5A, dtype=torch.int32).cuda()}


def _untouched(o):
    torch.cuda.synchronize()
    assert (o["item_ids"].cpu() == 0x5A5A5A5A5A5A5A5A).all() and (o["scores"].cpu() == 777.0).all() and (o["mmr"].cpu() == 777.0).all()
    assert all((o[n].cpu() == 0x5A5A5A5A).all() for n in ("index", "pos", "n_out", "status"))


def _struct(lam=0.5, sim=0, struct_bytes=None):
    from nann_amd import _lib
    d = _lib.Diversity()
    d.struct_bytes = C.sizeof(_lib.Diversity) if struct_bytes is None else struct_bytes
    d.lam, d.lambdas, d.sim = lam, None, sim
    return d


def test_search_diverse_refusals_launch_nothing(oracle):
    from nann_amd import _lib
    from nann_amd.ops import _ptr, _stream
    L = _lib.lib()
    dix = _index()[2]
    sc = _scorer("l2")
    b, k = 6, 20
    _, q = _queries(oracle, b, seed=14)
    qd = cuda(q)
    t = (C.c_int32 * 6)(*TOPN)
    nb, plain = C.c_int64(-1), C.c_int64(-1)
    assert L.nann_search_diverse_workspace_bytes(dix.handle, t, b, C.byref(nb)) == 0
    assert L.nann_search_filtered_workspace_bytes(dix.handle, t, b, C.byref(plain)) == 0 and nb.value == plain.value > 0
    ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    o = _canaries(b, k)

    def call(dv, kk=k, ws_bytes=nb.value):
        return L.nann_search_diverse(dix.handle, sc.handle, _ptr(qd), b, t, None, _ptr(ws), ws_bytes, _ptr(o["item_ids"]),
                                     _ptr(o["scores"]), _ptr(o["index"]), _ptr(o["status"]), None, None, None, None, None,
                                     C.byref(dv) if dv is not None else None, kk, _ptr(o["mmr"]), _ptr(o["pos"]), _ptr(o["n_out"]),
                                     _stream())

    ok = _struct()
    assert call(ok, kk=F + 1) == BAD_ARGUMENT and b"level_topn_max[5]" in L.nann_last_error()
    assert call(ok, kk=-1) == BAD_ARGUMENT
    assert call(None) == BAD_ARGUMENT and b"nann_search_diverse" in L.nann_last_error()
    assert call(_struct(struct_bytes=12)) == BAD_ARGUMENT
    assert call(_struct(sim=1)) == UNSUPPORTED
    assert call(_struct(sim=9)) == BAD_ARGUMENT
    assert call(_struct(lam=1.5)) == BAD_ARGUMENT and b"lambda" in L.nann_last_error()
    assert call(_struct(lam=float("nan"))) == BAD_ARGUMENT
    assert call(ok, ws_bytes=nb.value - 1) == CAPACITY and b"nann_search_diverse_workspace_bytes" in L.nann_last_error()
    _untouched(o)
    assert call(ok) == 0
    torch.cuda.synchronize()
    assert (o["status"].cpu() == 0).all() and (o["n_out"].cpu() == k).all()
    assert (o["pos"].cpu().numpy() < F).all() and (o["pos"].cpu().numpy()[:, 0] == 0).all()


def test_search_all_diverse_refusals_launch_nothing(oracle):
    from nann_amd import _lib, ops
    from nann_amd.ops import _ptr, _stream
    L = _lib.lib()
    dix = _small()[2]
    sc = ops.Scorer("l2", D)
    b, k = 4, 14
    qd = cuda(_q_small()[:b])
    nb, grouped = C.c_int64(-1), C.c_int64(-1)
    assert L.nann_search_all_diverse_workspace_bytes(dix.handle, sc.handle, b, NS + 1, C.byref(nb)) == TOPK_K_GT_N
    assert L.nann_search_all_diverse_workspace_bytes(dix.handle, sc.handle, b, -1, C.byref(nb)) == BAD_ARGUMENT
    assert nb.value == -1
    assert L.nann_search_all_diverse_workspace_bytes(dix.handle, sc.handle, b, 100, C.byref(nb)) == 0
    assert L.nann_search_all_grouped_workspace_bytes(dix.handle, sc.handle, b, 100, C.byref(grouped)) == 0 and nb.value == grouped.value > 0
    ws = torch.empty(nb.value + 256, dtype=torch.uint8, device="cuda")
    base = (ws.data_ptr() + 255) // 256 * 256
    o = _canaries(b, k)

    def call(dv, fetch=100, kk=k, w=base, ws_bytes=nb.value):
        return L.nann_search_all_diverse(dix.handle, sc.handle, _ptr(qd), b, fetch, kk, _ptr(o["item_ids"]), _ptr(o["scores"]),
                                         _ptr(o["index"]), _ptr(o["mmr"]), _ptr(o["pos"]), C.c_void_p(w) if w else None, ws_bytes,
                                         None, None, C.byref(dv) if dv is not None else None, _ptr(o["n_out"]), _stream())

    ok = _struct()
    assert call(ok, kk=101) == BAD_ARGUMENT and b"[0, fetch]" in L.nann_last_error()
    assert call(ok, kk=-1) == BAD_ARGUMENT
    assert call(ok, fetch=NS + 1) == TOPK_K_GT_N
    assert call(ok, fetch=1025, kk=k) in (TOPK_K_GT_N, UNSUPPORTED)       # (beyond n_items here; beyond 1024 on a larger index)
    assert call(None) == BAD_ARGUMENT
    assert call(_struct(lam=-0.5)) == BAD_ARGUMENT
    assert call(_struct(sim=1)) == UNSUPPORTED
    assert call(_struct(struct_bytes=8)) == BAD_ARGUMENT
    assert call(ok, ws_bytes=nb.value - 1) == CAPACITY and b"nann_search_all_diverse_workspace_bytes" in L.nann_last_error()
    assert call(ok, w=0) == CAPACITY
    assert call(ok, w=base + 64) == BAD_ARGUMENT and b"256-byte aligned" in L.nann_last_error()
    o["status"].fill_(0x5A5A5A5A)
    _untouched(o)
    assert call(ok, kk=0) == 0
    _untouched(o)
    assert call(ok) == 0
    torch.cuda.synchronize()
    assert (o["n_out"].cpu() == 14).all()
