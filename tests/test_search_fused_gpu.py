"""-m gpu: the fused multi-vector searches and the hybrid convenience.  search_multi_fused (nann_search_multi_fused) against the
numpy fuse model (fuse_model.model) applied to what the existing retrieval.search returns for the same n_users * n_vec vectors
as queries -- search is pinned to the oracle elsewhere, and the match is bitwise because the same call produced the fuse's
inputs.  search_all_multi_fused (nann_search_all_multi_fused) against the model over the references' brute force at the fetch
depth.  fuse_results against the model over the stacked lists.  The indexes are test_search_multi_gpu.py's: 2 000 rows x 64-d
f16 on the shipped builder's graph with level_topn [8, 16, 32, 32, 32, F = 50]; the exhaustive tests: 300 rows."""
import ctypes as C

import numpy as np
import pytest
import torch

import fuse_model as FM
import ip_reference as R
from gpu_util import bits, cuda, require_gpu
from test_search_multi_gpu import D, F, TOPN, _full_scores, _index, _queries, _scorer, _small

pytestmark = pytest.mark.gpu
BAD_ARGUMENT, UNSUPPORTED, CAPACITY = 7, 102, 103


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _got(r):
    torch.cuda.synchronize()
    return {"item_ids": r.item_ids.cpu().numpy(), "scores": r.scores.cpu().numpy(), "index": r.index.cpu().numpy(),
            "lists": r.lists.cpu().numpy().view(np.uint64), "n_out": r.n_out.cpu().numpy()}


def _same(got, exp, what=""):
    for name in ("n_out", "index", "lists", "item_ids", "scores"):
        g, e = (bits(got[name]), bits(exp[name])) if name == "scores" else (got[name], exp[name])
        assert g.shape == e.shape and (g == e).all(), (what, name)


def _expect_from_search(dix, sc, q, level_topn, k, mode, weights=None, rrf_c=60.0):
    """the fuse model over retrieval.search's answer for the vectors as queries -> (model dict, status [n_users, n_vec])"""
    from nann_amd import retrieval
    n_users, n_vec = q.shape[:2]
    r = retrieval.search(dix, sc, cuda(q.reshape(-1, D)), level_topn)
    torch.cuda.synchronize()
    status = r.status.cpu().numpy().reshape(n_users, n_vec)
    lt = np.asarray(level_topn)
    width = np.full((n_users, n_vec), lt[5]) if lt.ndim == 1 else lt[:, 5].reshape(n_users, n_vec)
    fetch = r.scores.shape[1]
    n_valid = np.where(status != 0, 0, width).astype(np.int32)
    exp = FM.model(r.scores.cpu().numpy().reshape(n_users, n_vec, fetch), r.index.cpu().numpy().reshape(n_users, n_vec, fetch),
                   n_valid, dix.n_items, k, mode, weights=weights, rrf_c=rrf_c, item_ids=dix.item_ids.cpu().numpy())
    return exp, status


# ---- search_multi_fused ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["l2", "ip", "mlp_exact"])
def test_search_multi_fused_is_the_fuse_of_search(oracle, kind):
    from nann_amd import retrieval
    dix = _index()[2]
    sc = _scorer(kind)
    q = _queries(oracle, 5, 4)
    w = np.array([1.0, 0.5, 2.0, 0.25], np.float32)
    for mode, weights, k in (("rrf", None, F), ("rrf", w, 120), ("minmax", w, 120), ("minmax", None, F)):
        exp, status = _expect_from_search(dix, sc, q, TOPN, k, FM.MODES[mode], weights=weights, rrf_c=20.0)
        masks = exp["lists"][:, :F].astype(object)
        assert (exp["n_out"] >= F).all() and any(bin(int(m)).count("1") > 1 for m in masks.reshape(-1))  # (lists do overlap)
        r = retrieval.search_multi_fused(dix, sc, cuda(q), TOPN, retrieval.make_fusion(mode, weights=weights, rrf_c=20.0), k=k)
        _same(_got(r), exp, (kind, mode, k))
        assert (r.status.cpu().numpy() == status).all()
    assert r.plan == retrieval.search(dix, sc, cuda(q.reshape(-1, D)), TOPN).plan


def test_a_failed_vector_contributes_nothing(oracle):
    from nann_amd import ops, retrieval
    dix = _index()[2]
    sc = ops.Scorer("l2", D)
    n_users, n_vec = 4, 3
    q = _queries(oracle, n_users, n_vec, seed=13)
    lt = np.tile(np.array(TOPN, np.int32), (n_users * n_vec, 1))
    lt[4] = [8, 4, 4, 4, 4, F]       # user 1, vector 1: a pool of 16 rows cannot give 50
    lt[7, 5] = 20                    # user 2, vector 1 asks for 20 only
    w = np.arange(1, n_users * n_vec + 1, dtype=np.float32).reshape(n_users, n_vec)  # per user
    for mode in ("rrf", "sum_floor"):
        exp, status = _expect_from_search(dix, sc, q, lt, 100, FM.MODES[mode], weights=w)
        assert status[1, 1] != 0 and (np.delete(status.reshape(-1), 4) == 0).all()
        r = retrieval.search_multi_fused(dix, sc, cuda(q), lt, retrieval.make_fusion(mode, weights=w), k=100)
        got = _got(r)
        _same(got, exp, mode)
        assert (r.status.cpu().numpy() == status).all()
        assert got["n_out"][1] > 0 and not (got["lists"][1] & np.uint64(2)).any()    # vector 1 of user 1 is in no mask
        held = (got["lists"][2, :got["n_out"][2]] & np.uint64(2)) != 0
        assert 0 < held.sum() <= 20


def _fused_c(dix, sc, q, n_users, n_vec, topn, k, outs, ws, ws_bytes, fusion):
    from nann_amd import _lib
    from nann_amd.ops import _ptr, _stream
    t = (C.c_int32 * 6)(*topn)
    st = _lib.lib().nann_search_multi_fused(dix.handle, sc.handle, _ptr(q), n_users, n_vec, t, None, ws, ws_bytes,
                                            _ptr(outs["item_ids"]), _ptr(outs["scores"]), _ptr(outs["index"]), _ptr(outs["lists"]),
                                            _ptr(outs["n_out"]), _ptr(outs["status"]), None, None, None, k,
                                            C.byref(fusion) if fusion is not None else None, _stream())
    torch.cuda.synchronize()
    return st


def test_refusals_launch_nothing(oracle):
    from nann_amd import _lib, ops
    L = _lib.lib()
    dix = _index()[2]
    sc = ops.Scorer("l2", D)
    n_users, n_vec, k = 2, 3, 60
    C64 = 0x5A5A5A5A5A5A5A5A

    def outs(nu, kk, nv):
        return {"item_ids": torch.full((nu, kk), C64, dtype=torch.int64).cuda(), "lists": torch.full((nu, kk), C64, dtype=torch.int64).cuda(),
                "scores": torch.full((nu, kk), 777.0).cuda(), "index": torch.full((nu, kk), 0x5A5A5A5A, dtype=torch.int32).cuda(),
                "n_out": torch.full((nu,), 0x5A5A5A5A, dtype=torch.int32).cuda(),
                "status": torch.full((nu, nv), 0x5A5A5A5A, dtype=torch.int32).cuda()}

    def untouched(o):
        assert (o["item_ids"].cpu() == C64).all() and (o["lists"].cpu() == C64).all() and (o["scores"].cpu() == 777.0).all()
        assert all((o[n].cpu() == 0x5A5A5A5A).all() for n in ("index", "n_out", "status"))

    fusion = lambda **kw: _lib.Fusion(**{**dict(struct_bytes=C.sizeof(_lib.Fusion), mode=FM.RRF, rrf_c=60.0, weights_per_user=0,
                                                weights=None), **kw})
    q = cuda(_queries(oracle, n_users, n_vec, seed=14))
    nb = C.c_int64(-1)
    t = (C.c_int32 * 6)(*TOPN)
    assert L.nann_search_multi_fused_workspace_bytes(dix.handle, t, n_users, n_vec, C.byref(nb)) == 0 and nb.value > 0
    plain = C.c_int64(-1)
    assert L.nann_search_filtered_workspace_bytes(dix.handle, t, n_users * n_vec, C.byref(plain)) == 0
    assert nb.value == (plain.value + 255) // 256 * 256 + 256 * -(-(n_users * n_vec * F * 24) // 256)  # + 24 B per entry
    ws = torch.empty(nb.value + 256, dtype=torch.uint8, device="cuda")
    base = (ws.data_ptr() + 255) // 256 * 256
    at = C.c_void_p(base)
    o = outs(n_users, k, n_vec)
    f = fusion()
    assert _fused_c(dix, sc, q, n_users, n_vec, TOPN, n_vec * F + 1, o, at, nb.value, f) == BAD_ARGUMENT  # k > n_vec * F
    assert _fused_c(dix, sc, q, n_users, n_vec, TOPN, -1, o, at, nb.value, f) == BAD_ARGUMENT
    assert _fused_c(dix, sc, q, n_users, 0, TOPN, k, o, at, nb.value, f) == BAD_ARGUMENT                   # n_vec < 1
    assert _fused_c(dix, sc, q, n_users, n_vec, TOPN, k, o, at, nb.value, None) == BAD_ARGUMENT            # no fusion
    assert _fused_c(dix, sc, q, n_users, n_vec, TOPN, k, o, at, nb.value, fusion(mode=4)) == BAD_ARGUMENT
    assert _fused_c(dix, sc, q, n_users, n_vec, TOPN, k, o, at, nb.value, fusion(rrf_c=-1.0)) == BAD_ARGUMENT
    assert _fused_c(dix, sc, q, n_users, n_vec, TOPN, k, o, at, nb.value, fusion(struct_bytes=12)) == BAD_ARGUMENT
    assert _fused_c(dix, sc, q, n_users, n_vec, TOPN, k, o, at, nb.value, fusion(weights_per_user=2)) == BAD_ARGUMENT
    assert _fused_c(dix, sc, q, n_users, n_vec, TOPN, k, o, at, nb.value - 1, f) == CAPACITY               # short
    assert _fused_c(dix, sc, q, n_users, n_vec, TOPN, k, o, None, nb.value, f) == CAPACITY
    assert _fused_c(dix, sc, q, n_users, n_vec, TOPN, k, o, C.c_void_p(base + 64), nb.value, f) == BAD_ARGUMENT  # misaligned
    assert b"256-byte aligned" in L.nann_last_error()
    untouched(o)
    # 65 vectors of 3 entries: within NANN_UNION_MAX_IN, one more list than the mask has bits; 2731 x 3 = 8193 entries
    wide = TOPN[:5] + [3]
    ow = outs(1, k, 2731)
    qw = torch.zeros((1, 2731, D), dtype=torch.float32, device="cuda")
    assert _fused_c(dix, sc, qw, 1, 65, wide, k, ow, at, nb.value, f) == UNSUPPORTED and b"NANN_FUSE_MAX_LISTS" in L.nann_last_error()
    assert _fused_c(dix, sc, qw, 1, 2731, wide, k, ow, at, nb.value, f) == UNSUPPORTED and b"NANN_UNION_MAX_IN" in L.nann_last_error()
    assert L.nann_search_multi_fused_workspace_bytes(dix.handle, (C.c_int32 * 6)(*wide), 1, 65, C.byref(plain)) == UNSUPPORTED
    big = TOPN[:5] + [1024]
    assert _fused_c(dix, sc, q, n_users, 2, big, 1025, o, at, nb.value, f) == UNSUPPORTED                  # k > 1024
    untouched(ow)
    untouched(o)
    # k == 0 or no users: NANN_OK, no inner search, nothing written -- status included
    assert _fused_c(dix, sc, q, n_users, n_vec, TOPN, 0, o, at, nb.value, f) == 0
    assert _fused_c(dix, sc, q, 0, n_vec, TOPN, k, o, at, nb.value, f) == 0
    untouched(o)
    # and the same call, accepted, writes every output
    assert _fused_c(dix, sc, q, n_users, n_vec, TOPN, k, o, at, nb.value, f) == 0
    assert (o["status"].cpu() == 0).all() and (o["n_out"].cpu() == k).all()
    assert ((o["lists"].cpu() > 0) & (o["lists"].cpu() < 2 ** n_vec)).all()


# ---- search_all_multi_fused -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("n_vec", [1, 3, 8])
def test_search_all_multi_fused_is_the_fuse_of_brute_force(oracle, metric, n_vec):
    from nann_amd import ops, retrieval
    embs, oix, dix = _small(oracle)
    n_users = 4
    rng = np.random.default_rng(40 + n_vec)
    q = rng.standard_normal((n_users, n_vec, D)).astype(np.float32)
    if n_vec > 2:
        q[:, 2] = q[:, 0]  # a repeated interest adds its term twice
    full = _full_scores(oracle, metric, q.reshape(-1, D)).reshape(n_users, n_vec, 300)
    sc = ops.Scorer(metric, D)
    w = rng.standard_normal((n_users, n_vec)).astype(np.float32)
    for k in (1, 37):
        for fetch in (k, 2 * k):
            tops = np.stack([[R.topk_stable(full[u, m], fetch) for m in range(n_vec)] for u in range(n_users)])
            lists = np.take_along_axis(full, tops, axis=2)
            for mode, weights in (("rrf", None), ("minmax", w), ("sum_floor", w[0]), ("sum", w)):
                kk = min(k, n_vec * fetch)
                exp = FM.model(lists, tops.astype(np.int32), None, 300, kk, FM.MODES[mode], weights=weights, item_ids=oix.ids)
                r = retrieval.search_all_multi_fused(dix, sc, cuda(q), kk, retrieval.make_fusion(mode, weights=weights),
                                                     fetch=None if fetch == k else fetch)
                _same(_got(r), exp, (metric, n_vec, k, fetch, mode))


def test_search_all_multi_fused_refusals(oracle):
    from nann_amd import _lib, ops
    from nann_amd.ops import _ptr, _stream
    L = _lib.lib()
    embs, oix, dix = _small(oracle)
    sc = ops.Scorer("l2", D)
    q = torch.zeros((2, 9, D), dtype=torch.float32, device="cuda")
    nb = C.c_int64(-1)
    assert L.nann_search_all_multi_fused_workspace_bytes(dix.handle, sc.handle, 2, 3, 301, C.byref(nb)) == 4      # TOPK_K_GT_N
    assert L.nann_search_all_multi_fused_workspace_bytes(dix.handle, sc.handle, 2, 0, 10, C.byref(nb)) == BAD_ARGUMENT
    assert L.nann_search_all_multi_fused_workspace_bytes(dix.handle, sc.handle, 2, 82, 100, C.byref(nb)) == UNSUPPORTED  # 8200
    assert L.nann_search_all_multi_fused_workspace_bytes(dix.handle, sc.handle, 2, 65, 100, C.byref(nb)) == UNSUPPORTED  # 65 lists
    assert nb.value == -1
    assert L.nann_search_all_multi_fused_workspace_bytes(dix.handle, sc.handle, 2, 9, 100, C.byref(nb)) == 0 and nb.value > 0
    ids = torch.full((2, 150), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64).cuda()
    ws = torch.empty(nb.value + 256, dtype=torch.uint8, device="cuda")
    base = (ws.data_ptr() + 255) // 256 * 256
    f = _lib.Fusion(C.sizeof(_lib.Fusion), FM.RRF, 60.0, 0, None)
    call = lambda w, wb, k=150, fu=f: L.nann_search_all_multi_fused(dix.handle, sc.handle, _ptr(q), 2, 9, 100, k,
                                                                    C.byref(fu) if fu is not None else None, _ptr(ids), None,
                                                                    None, None, None, w, wb, None, _stream())
    assert call(C.c_void_p(base), nb.value, k=901) == BAD_ARGUMENT and b"n_vec * fetch" in L.nann_last_error()
    assert call(C.c_void_p(base), nb.value, k=-1) == BAD_ARGUMENT
    assert call(C.c_void_p(base), nb.value, fu=None) == BAD_ARGUMENT
    assert call(C.c_void_p(base), nb.value, fu=_lib.Fusion(C.sizeof(_lib.Fusion), 5, 60.0, 0, None)) == BAD_ARGUMENT
    assert call(C.c_void_p(base), nb.value - 1) == CAPACITY
    assert call(C.c_void_p(base + 128), nb.value) == BAD_ARGUMENT
    torch.cuda.synchronize()
    assert (ids.cpu() == 0x5A5A5A5A5A5A5A5A).all()
    assert call(C.c_void_p(base), nb.value) == 0  # k = 150 > fetch = 100; out_item_ids alone: the optional outputs are NULL
    torch.cuda.synchronize()
    assert (ids.cpu() != 0x5A5A5A5A5A5A5A5A).all()


# ---- fuse_results: the hybrid convenience ---------------------------------------------------------------------------------
def test_fuse_results_over_a_traversal_and_an_exhaustive_search(oracle):
    from nann_amd import ops, retrieval
    dix = _index()[2]
    sc = ops.Scorer("l2", D)
    q = cuda(_queries(oracle, 6, 1, seed=15).reshape(6, D))
    a = retrieval.search(dix, sc, q, TOPN)          # [6, 50], no n_out: its width counts
    b = retrieval.search_all(dix, sc, q, 30)        # [6, 30], padded to 50
    flt = retrieval.make_filter(dix, deny_rows=np.arange(0, dix.n_items - 12))
    c = retrieval.search_all(dix, sc, q, 30, filter=flt)  # [6, 30] with n_out = 12
    torch.cuda.synchronize()
    assert (a.status.cpu().numpy() == 0).all() and (c.n_out.cpu().numpy() == 12).all()
    scores = np.zeros((6, 3, F), np.float32)
    rows = np.zeros((6, 3, F), np.int32)
    scores[:, 0], rows[:, 0] = a.scores.cpu().numpy(), a.index.cpu().numpy()
    scores[:, 1, :30], rows[:, 1, :30] = b.scores.cpu().numpy(), b.index.cpu().numpy()
    scores[:, 2, :30], rows[:, 2, :30] = c.scores.cpu().numpy(), c.index.cpu().numpy()
    n_valid = np.tile(np.array([F, 30, 12], np.int32), (6, 1))
    for mode, weights in (("rrf", None), ("rrf", [1.0, 2.0, 0.5]), ("minmax", [1.0, 1.0, 1.0])):
        exp = FM.model(scores, rows, n_valid, dix.n_items, 60, FM.MODES[mode], weights=weights, item_ids=dix.item_ids.cpu().numpy())
        r = retrieval.fuse_results([a, b, c], retrieval.make_fusion(mode, weights=weights), 60, dix)
        got = _got(r)
        _same(got, exp, mode)
        assert r.status is None and (got["n_out"] >= F).all()
        assert (got["lists"][:, 0] & np.uint64(3) == np.uint64(3)).any()  # the traversal and the exhaustive search agree on a best row
