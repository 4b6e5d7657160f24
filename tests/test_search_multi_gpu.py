"""-m gpu: the multi-vector searches.  search_multi (nann_search_multi) against the numpy union model (union_model.model)
applied to what the existing retrieval.search returns for the same n_users * n_vec vectors as queries -- search is pinned to the
oracle elsewhere, and the match is bitwise because the same call produced the union's inputs.  search_all_multi
(nann_search_all_multi) against the model over the references' brute force.  Index of the traversal tests: 2 000 rows x 64-d
f16 on the shipped builder's graph, level_topn [8, 16, 32, 32, 32, F = 50]; the exhaustive tests: 300 rows."""
import ctypes as C

import numpy as np
import pytest
import torch

import ip_reference as R
import union_model as UM
from gpu_util import bits, cuda, queries_for, require_gpu, synth_index
from test_search_all_gpu import _brute, _indices

pytestmark = pytest.mark.gpu
N, D, F = 2000, 64, 50
TOPN = [8, 16, 32, 32, 32, F]
BAD_ARGUMENT, UNSUPPORTED, CAPACITY = 7, 102, 103
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _index():
    return synth_index(N, D, 64)


def _queries(oracle, n_users, n_vec, seed=4321):
    """f32[n_users, n_vec, D]: every vector the mean of a synthetic user sequence"""
    g = _index()[0]
    seqs = queries_for(g, n_users * n_vec, seed=seed)
    return np.stack([oracle.user_seq_mean(s) for s in seqs]).reshape(n_users, n_vec, D).astype(np.float32)


def _scorer(kind):
    from nann_amd import ops, synth
    if kind in ("l2", "ip"):
        return ops.Scorer(kind, D)
    return ops.Scorer("mlp", D, torch.float16, synth.make_mlp_weights(D), precision={"mlp_exact": "exact", "mlp_split": "split"}[kind])


def _expect_from_search(dix, sc, q, level_topn, k):
    """the union model over retrieval.search's answer for the vectors as queries -> (model dict, status [n_users, n_vec])"""
    from nann_amd import retrieval
    n_users, n_vec = q.shape[:2]
    r = retrieval.search(dix, sc, cuda(q.reshape(-1, D)), level_topn)
    torch.cuda.synchronize()
    status = r.status.cpu().numpy().reshape(n_users, n_vec)
    lt = np.asarray(level_topn)
    width = np.full((n_users, n_vec), lt[5]) if lt.ndim == 1 else lt[:, 5].reshape(n_users, n_vec)
    fetch = r.scores.shape[1]
    n_valid = np.where(status != 0, 0, width).astype(np.int32)
    exp = UM.model(r.scores.cpu().numpy().reshape(n_users, n_vec, fetch), r.index.cpu().numpy().reshape(n_users, n_vec, fetch),
                   n_valid, dix.n_items, k, item_ids=dix.item_ids.cpu().numpy())
    return exp, status


def _got(r):
    torch.cuda.synchronize()
    return {"item_ids": r.item_ids.cpu().numpy(), "scores": r.scores.cpu().numpy(), "index": r.index.cpu().numpy(),
            "list": r.vec.cpu().numpy(), "n_out": r.n_out.cpu().numpy()}


def _same(got, exp, what=""):
    for name in ("n_out", "index", "list", "item_ids", "scores"):
        g, e = (bits(got[name]), bits(exp[name])) if name == "scores" else (got[name], exp[name])
        assert g.shape == e.shape and (g == e).all(), (what, name)


# ---- search_multi ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["l2", "ip", "mlp_exact", "mlp_split"])
def test_search_multi_is_the_union_of_search(oracle, kind):
    from nann_amd import retrieval
    dix = _index()[2]
    sc = _scorer(kind)
    q = _queries(oracle, 5, 4)
    for k in (F, 120):
        exp, status = _expect_from_search(dix, sc, q, TOPN, k)
        assert (exp["n_out"] >= F).all() and len(set(exp["list"].reshape(-1).tolist())) > 1  # (the case is no one-list case)
        r = retrieval.search_multi(dix, sc, cuda(q), TOPN, k=k)
        _same(_got(r), exp, (kind, k))
        assert (r.status.cpu().numpy() == status).all()
        assert r.plan == retrieval.search(dix, sc, cuda(q.reshape(-1, D)), TOPN).plan


def test_one_vector_reproduces_search(oracle):
    from nann_amd import ops, retrieval
    dix = _index()[2]
    sc = ops.Scorer("l2", D)
    q = _queries(oracle, 7, 1, seed=11)
    plain = retrieval.search(dix, sc, cuda(q.reshape(-1, D)), TOPN)
    for k in (20, F):
        r = retrieval.search_multi(dix, sc, cuda(q), TOPN, k=k)
        torch.cuda.synchronize()
        assert (r.item_ids.cpu().numpy() == plain.item_ids.cpu().numpy()[:, :k]).all()
        assert (r.index.cpu().numpy() == plain.index.cpu().numpy()[:, :k]).all()
        assert (bits(r.scores.cpu().numpy()) == bits(plain.scores.cpu().numpy()[:, :k])).all()
        assert (r.n_out.cpu().numpy() == k).all() and not r.vec.cpu().numpy().any()


def test_a_repeated_vector_changes_nothing(oracle):
    """a user with two interests passes one of them twice more: the rows and scores of the answer stay"""
    from nann_amd import ops, retrieval
    dix = _index()[2]
    sc = ops.Scorer("l2", D)
    q2 = _queries(oracle, 3, 2, seed=12)
    q4 = np.concatenate([q2, q2[:, 1:2], q2[:, 1:2]], axis=1)
    a, b = _got(retrieval.search_multi(dix, sc, cuda(q2), TOPN, k=80)), _got(retrieval.search_multi(dix, sc, cuda(q4), TOPN, k=80))
    for name in ("n_out", "index", "item_ids", "list"):  # (list too: the first copy, at the lower position, represents)
        assert (a[name] == b[name]).all(), name
    assert (bits(a["scores"]) == bits(b["scores"])).all()


def test_a_failed_vector_fails_alone(oracle):
    from nann_amd import ops, retrieval
    dix = _index()[2]
    sc = ops.Scorer("l2", D)
    n_users, n_vec = 4, 3
    q = _queries(oracle, n_users, n_vec, seed=13)
    lt = np.tile(np.array(TOPN, np.int32), (n_users * n_vec, 1))
    lt[4] = [8, 4, 4, 4, 4, F]       # user 1, vector 1: a pool of 16 rows cannot give 50
    lt[7, 5] = 20                    # user 2, vector 1 asks for 20 only
    exp, status = _expect_from_search(dix, sc, q, lt, 100)
    assert status[1, 1] != 0 and (np.delete(status.reshape(-1), 4) == 0).all()
    r = retrieval.search_multi(dix, sc, cuda(q), lt, k=100)
    _same(_got(r), exp)
    assert (r.status.cpu().numpy() == status).all()
    got = _got(r)
    assert got["n_out"][1] > 0 and 1 not in got["list"][1, :got["n_out"][1]].tolist()
    assert (got["list"][2, :got["n_out"][2]] == 1).sum() <= 20


def _multi_c(dix, sc, q, n_users, n_vec, topn, k, outs, ws, ws_bytes):
    from nann_amd import _lib
    from nann_amd.ops import _ptr, _stream
    t = (C.c_int32 * 6)(*topn)
    st = _lib.lib().nann_search_multi(dix.handle, sc.handle, _ptr(q), n_users, n_vec, t, None, ws, ws_bytes, _ptr(outs["item_ids"]),
                                      _ptr(outs["scores"]), _ptr(outs["index"]), _ptr(outs["vec"]), _ptr(outs["n_out"]),
                                      _ptr(outs["status"]), None, None, None, k, _stream())
    torch.cuda.synchronize()
    return st


def test_refusals_launch_nothing(oracle):
    from nann_amd import _lib, ops
    L = _lib.lib()
    dix = _index()[2]
    sc = ops.Scorer("l2", D)
    n_users, n_vec, k = 2, 3, 60

    def outs(nu, kk, nv):
        return {"item_ids": torch.full((nu, kk), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64).cuda(),
                "scores": torch.full((nu, kk), 777.0).cuda(), "index": torch.full((nu, kk), 0x5A5A5A5A, dtype=torch.int32).cuda(),
                "vec": torch.full((nu, kk), 0x5A5A5A5A, dtype=torch.int32).cuda(),
                "n_out": torch.full((nu,), 0x5A5A5A5A, dtype=torch.int32).cuda(),
                "status": torch.full((nu, nv), 0x5A5A5A5A, dtype=torch.int32).cuda()}

    def untouched(o):
        assert (o["item_ids"].cpu() == 0x5A5A5A5A5A5A5A5A).all() and (o["scores"].cpu() == 777.0).all()
        assert all((o[n].cpu() == 0x5A5A5A5A).all() for n in ("index", "vec", "n_out", "status"))

    q = cuda(_queries(oracle, n_users, n_vec, seed=14))
    nb = C.c_int64(-1)
    t = (C.c_int32 * 6)(*TOPN)
    assert L.nann_search_multi_workspace_bytes(dix.handle, t, n_users, n_vec, C.byref(nb)) == 0 and nb.value > 0
    plain = C.c_int64(-1)
    assert L.nann_search_filtered_workspace_bytes(dix.handle, t, n_users * n_vec, C.byref(plain)) == 0
    assert nb.value == (plain.value + 255) // 256 * 256 + 256 * -(-(n_users * n_vec * F * 8) // 256)  # + 8 B per entry
    ws = torch.empty(nb.value + 256, dtype=torch.uint8, device="cuda")
    base = (ws.data_ptr() + 255) // 256 * 256
    o = outs(n_users, k, n_vec)
    assert _multi_c(dix, sc, q, n_users, n_vec, TOPN, n_vec * F + 1, o, C.c_void_p(base), nb.value) == BAD_ARGUMENT  # k > n_vec * F
    assert _multi_c(dix, sc, q, n_users, n_vec, TOPN, -1, o, C.c_void_p(base), nb.value) == BAD_ARGUMENT
    assert _multi_c(dix, sc, q, n_users, 0, TOPN, k, o, C.c_void_p(base), nb.value) == BAD_ARGUMENT                 # n_vec < 1
    assert _multi_c(dix, sc, q, n_users, n_vec, TOPN, k, o, C.c_void_p(base), nb.value - 1) == CAPACITY             # short
    assert _multi_c(dix, sc, q, n_users, n_vec, TOPN, k, o, None, nb.value) == CAPACITY
    assert _multi_c(dix, sc, q, n_users, n_vec, TOPN, k, o, C.c_void_p(base + 64), nb.value) == BAD_ARGUMENT        # misaligned
    assert b"256-byte aligned" in L.nann_last_error()
    untouched(o)
    # n_vec * F = 2731 * 3 = 8193 entries per user: one more than NANN_UNION_MAX_IN
    wide = TOPN[:5] + [3]
    qw = torch.zeros((1, 2731, D), dtype=torch.float32, device="cuda")
    ow = outs(1, k, 2731)
    assert _multi_c(dix, sc, qw, 1, 2731, wide, k, ow, C.c_void_p(base), nb.value) == UNSUPPORTED
    assert b"NANN_UNION_MAX_IN" in L.nann_last_error()
    assert L.nann_search_multi_workspace_bytes(dix.handle, (C.c_int32 * 6)(*wide), 1, 2731, C.byref(plain)) == UNSUPPORTED
    # k > 1024 within n_vec * F
    big = TOPN[:5] + [1024]
    assert _multi_c(dix, sc, q, n_users, 2, big, 1025, o, C.c_void_p(base), nb.value) == UNSUPPORTED
    untouched(ow)
    untouched(o)
    # k == 0 or no users: NANN_OK, no inner search, nothing written -- status included
    assert _multi_c(dix, sc, q, n_users, n_vec, TOPN, 0, o, C.c_void_p(base), nb.value) == 0
    assert _multi_c(dix, sc, q, 0, n_vec, TOPN, k, o, C.c_void_p(base), nb.value) == 0
    untouched(o)
    # and the same call, accepted, writes every output
    assert _multi_c(dix, sc, q, n_users, n_vec, TOPN, k, o, C.c_void_p(base), nb.value) == 0
    assert (o["status"].cpu() == 0).all() and (o["n_out"].cpu() == k).all() and (o["vec"].cpu() < n_vec).all()


# ---- search_all_multi -----------------------------------------------------------------------------------------------------
def _small(oracle):
    """300 rows x 64-d f16 with ten duplicated rows (ties across rows): (embs, oracle index, device index)"""
    if "small" not in _CACHE:
        rng = np.random.default_rng(31)
        embs = rng.standard_normal((300, D)).astype(np.float16)
        embs[100:110] = embs[0:10]
        _CACHE["small"] = (embs,) + _indices(embs)
    return _CACHE["small"]


def _full_scores(oracle, metric, q):
    """every row's score for every vector of q f32[n, D] -> f32[n, 300], from the references"""
    embs, oix, _ = _small(oracle)
    if metric == "ip":
        return np.stack([R.ip_scores(v, R.widen(embs)) for v in q])
    rows, scores = _brute(oracle, oix, oracle.Scorer("l2", D, oracle.EMB_F16), q, 300)
    full = np.empty((len(q), 300), np.float32)
    np.put_along_axis(full, rows.astype(np.int64), scores, axis=1)
    return full


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("n_vec", [1, 3, 8])
def test_search_all_multi_is_the_union_of_brute_force(oracle, metric, n_vec):
    from nann_amd import ops, retrieval
    embs, oix, dix = _small(oracle)
    n_users = 4
    rng = np.random.default_rng(40 + n_vec)
    q = rng.standard_normal((n_users, n_vec, D)).astype(np.float32)
    if n_vec > 2:
        q[:, 2] = q[:, 0]  # a repeated interest
    full = _full_scores(oracle, metric, q.reshape(-1, D)).reshape(n_users, n_vec, 300)
    sc = ops.Scorer(metric, D)
    for k in (1, 37, 300):
        tops = np.stack([[R.topk_stable(full[u, m], k) for m in range(n_vec)] for u in range(n_users)])
        exp = UM.model(np.take_along_axis(full, tops, axis=2), tops.astype(np.int32), None, 300, k, item_ids=oix.ids)
        got = _got(retrieval.search_all_multi(dix, sc, cuda(q), k))
        _same(got, exp, (metric, n_vec, k))
        best = full.max(axis=1)  # the per-row maximum over a user's vectors
        for u in range(n_users):
            assert (bits(got["scores"][u]) == bits(best[u][R.topk_stable(best[u], k)])).all()


def test_filters_compose_through_union_topk(oracle):
    """the documented composition: search_all(filter=) over the vectors as queries, then union_topk with n_valid = its n_out"""
    from nann_amd import ops, retrieval
    embs, oix, dix = _small(oracle)
    n_users, n_vec, k = 3, 4, 100
    rng = np.random.default_rng(50)
    q = rng.standard_normal((n_users, n_vec, D)).astype(np.float32)
    deny = rng.random(300) < 0.8
    allowed = np.nonzero(~deny)[0]
    assert 0 < len(allowed) < k
    sc = ops.Scorer("l2", D)
    flt = retrieval.make_filter(dix, deny_rows=np.nonzero(deny)[0])
    per = retrieval.search_all(dix, sc, cuda(q.reshape(-1, D)), k, filter=flt)
    r = retrieval.union_topk(per.scores.view(n_users, n_vec, k), per.index.view(n_users, n_vec, k), k,
                             n_valid=per.n_out.view(n_users, n_vec), index=dix)
    full = _full_scores(oracle, "l2", q.reshape(-1, D)).reshape(n_users, n_vec, 300)
    rows = np.zeros((n_users, n_vec, k), np.int32)
    scores = np.zeros((n_users, n_vec, k), np.float32)
    for u in range(n_users):
        for m in range(n_vec):
            t = allowed[R.topk_stable(full[u, m][allowed], len(allowed))]
            rows[u, m, :len(t)], scores[u, m, :len(t)] = t, full[u, m][t]
    exp = UM.model(scores, rows, np.full((n_users, n_vec), len(allowed), np.int32), 300, k, item_ids=oix.ids)
    got = _got(r)
    _same(got, exp)
    assert (got["n_out"] == len(allowed)).all() and not deny[got["index"][:, :len(allowed)]].any()


def test_search_all_multi_refusals(oracle):
    from nann_amd import _lib, ops
    from nann_amd.ops import _ptr, _stream
    L = _lib.lib()
    embs, oix, dix = _small(oracle)
    sc = ops.Scorer("l2", D)
    q = torch.zeros((2, 9, D), dtype=torch.float32, device="cuda")
    nb = C.c_int64(-1)
    assert L.nann_search_all_multi_workspace_bytes(dix.handle, sc.handle, 2, 3, 301, C.byref(nb)) == 4      # TOPK_K_GT_N
    assert L.nann_search_all_multi_workspace_bytes(dix.handle, sc.handle, 2, 0, 10, C.byref(nb)) == BAD_ARGUMENT
    assert L.nann_search_all_multi_workspace_bytes(dix.handle, sc.handle, 2, 82, 100, C.byref(nb)) == UNSUPPORTED  # 8200 entries
    assert nb.value == -1
    assert L.nann_search_all_multi_workspace_bytes(dix.handle, sc.handle, 2, 9, 100, C.byref(nb)) == 0 and nb.value > 0
    ids = torch.full((2, 100), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64).cuda()
    ws = torch.empty(nb.value + 256, dtype=torch.uint8, device="cuda")
    base = (ws.data_ptr() + 255) // 256 * 256
    call = lambda w, wb: L.nann_search_all_multi(dix.handle, sc.handle, _ptr(q), 2, 9, 100, _ptr(ids), None, None, None, None, w, wb,
                                                 None, _stream())
    assert call(C.c_void_p(base), nb.value - 1) == CAPACITY
    assert call(C.c_void_p(base + 128), nb.value) == BAD_ARGUMENT
    torch.cuda.synchronize()
    assert (ids.cpu() == 0x5A5A5A5A5A5A5A5A).all()
    assert call(C.c_void_p(base), nb.value) == 0  # out_item_ids alone: the optional outputs are NULL
    torch.cuda.synchronize()
    assert (ids.cpu() != 0x5A5A5A5A5A5A5A5A).all()
