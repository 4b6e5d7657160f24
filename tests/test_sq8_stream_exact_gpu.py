"""-m gpu: the certified scalar-quantised searches without a score buffer (nann_search_all_sq8_stream_exact,
nann_search_all_range_sq8_stream_exact) BIT FOR BIT against the exhaustive reference -- every (query, row) scored exactly (the
oracle's L2 scorer; ip_reference's canonical order for the inner product), then TopKV2 or the range rule -- and their survivor
counts against sq8_exact_model's predicate.  No tolerance appears.  n_items = 1024 + 33: a second block of the int8 scan that is
one full 32-row group and a ragged one; 129 queries = two chunks and a partial last tile."""
import ctypes as C

import numpy as np
import pytest
import torch

import ip_reference as R
import range_model as RM
import sq8_exact_model as X
import sq8_model as M
import sq8_range_model as RG
from gpu_util import bits, cuda, require_gpu
from test_sq8_exact_gpu import _index, _rows, _scorer, _status

pytestmark = pytest.mark.gpu
F = np.float32
N, NQ = 1024 + 33, 129
# 70 copies of one row: a tie that straddles the 1st and the 64th place, 32-row group boundaries and the block boundary
TIES = [31, 32] + list(range(100, 165)) + [1023, 1024, N - 1]
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def case(d, dtype, metric):
    """made once: rows, queries (query 0 = the planted row, of the greatest norm: its copies share the best score under either
    metric), the device index, table, bounds and scorer, the model's approximate scores and terms, the exact score of every pair"""
    key = (d, dtype)
    if key not in _CACHE:
        from nann_amd import retrieval
        x = _rows(N, d, 7 + d, dtype)
        w = M.widen(x)
        big = w[np.argmax((w.astype(np.float64) ** 2).sum(axis=1))] * F(2.0)      # (exact in either dtype: no other row equals it)
        x[TIES] = big.astype(np.float16) if dtype == "f16" else R.to_bf16_bits(big)
        q = np.random.default_rng(d).standard_normal((NQ, d)).astype(F)
        q[0] = M.widen(x[TIES[:1]])[0]
        dix = _index(x)
        t = retrieval.make_sq8(dix)
        xe, qe = M.encode(x), M.encode(q)
        _CACHE[key] = (x, q, dix, t, retrieval.make_sq8_bounds(dix, t), xe, qe, X.row_terms(x, xe), X.row_terms(q, qe))
    x, q, dix, t, b, xe, qe, xt, qt = _CACHE[key]
    if (key, metric) not in _CACHE:
        from oracle import oracle as O
        if metric == "l2":
            osc = O.Scorer("l2", d, O.EMB_F16 if dtype == "f16" else O.EMB_BF16)
            exact = np.stack([O.score_rows(osc, v, x)[1] for v in q])
        else:
            exact = np.stack([R.ip_scores(v, M.widen(x)) for v in q])
        _CACHE[key, metric] = (M.approx_scores(qe, xe, metric), exact)
    sc = _scorer(metric, d, torch.float16 if dtype == "f16" else torch.bfloat16)
    return (x, q, dix, t, b, xt, qt, sc) + _CACHE[key, metric]


def model_topk(approx, exact, xt, qt, metric, d, k, fetch, n_sample):
    """(tau: the k-th exact score of the sample's fetch list, its re-ranked rows and scores, the survivors bool[NQ, N])"""
    f_rows, _ = M.fetch(approx[:, :n_sample], fetch)
    a_rows, a_scores = M.rerank(f_rows, lambda i, rows: exact[i][rows], k)
    tau = a_scores[:, k - 1]
    w, ok = X.query_terms(tau, qt[0], qt[1], metric, d)
    assert ok.all()
    return tau, a_rows, a_scores, X.survives(approx, xt[0], xt[1], tau, qt[0], qt[1], w, metric, d)


def topk(dix, t, b, sc, q, k, **kw):
    from nann_amd import retrieval
    r = retrieval.search_all_sq8_stream_exact(dix, t, b, sc, cuda(q), k, **kw)
    torch.cuda.synchronize()
    return [a.cpu().numpy() for a in (r.index, r.scores, r.item_ids, r.certified, r.n_survivors)]


def ranged(dix, t, b, sc, q, thr, **kw):
    from nann_amd import retrieval
    r = retrieval.search_all_range_sq8_stream_exact(dix, t, b, sc, cuda(q), cuda(thr), **kw)
    torch.cuda.synchronize()
    return [a.cpu().numpy() for a in (r.row_splits, r.index, r.scores, r.item_ids, r.certified, r.n_survivors)]


def same_topk(got, rows, scores, ids_of, which, what):
    assert (got[0][which] == rows[which]).all() and (bits(got[1][which]) == bits(scores[which])).all(), what
    assert (got[2][which] == ids_of[rows[which]]).all(), what


def thresholds(exact, metric):
    """cycled over the queries: just above the best score (no match), the best score itself (a threshold equal to a row's score;
    query 0: its 70 copies), the 100th best; query 3: a finite threshold above +0"""
    s = -np.sort(-exact, axis=1)
    thr = np.where(np.arange(NQ) % 3 == 2, np.nextafter(s[:, 0], F(np.inf)), np.where(np.arange(NQ) % 3 == 0, s[:, 0], s[:, 99])).astype(F)
    thr[3] = F(1e-30)
    return thr


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d", [64, 512])
def test_topk_equals_the_exhaustive_reference(d, dtype, metric):
    x, q, dix, t, b, xt, qt, sc, approx, exact = case(d, dtype, metric)
    ids_of = dix.item_ids.cpu().numpy()
    for k, fetch in ((1, 1), (1, 128), (64, 64), (64, 128)):
        ref = [M.topk(s, k) for s in exact]
        rows, scores = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
        assert rows[0].tolist() == TIES[:k] and bits(exact[0, TIES[-1]]) == bits(scores[0, -1])   # the tie straddles the k-th place
        for sample_rows in (fetch, N):
            keep = model_topk(approx, exact, xt, qt, metric, d, k, fetch, sample_rows)[3]
            for nq in (1, 33, NQ):
                got = topk(dix, t, b, sc, q[:nq], k, fetch=fetch, sample_rows=sample_rows, cap=N, fallback=False)
                what = (k, fetch, sample_rows, nq)
                assert got[3].all(), what                                         # a cap of n_items cannot be exceeded
                assert (got[4] == keep.sum(axis=1)[:nq]).all(), what
                same_topk(got, rows, scores, ids_of, np.arange(nq), what)


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d", [64, 512])
def test_range_equals_the_exhaustive_reference(d, dtype, metric):
    x, q, dix, t, b, xt, qt, sc, approx, exact = case(d, dtype, metric)
    ids_of = dix.item_ids.cpu().numpy()
    thr = thresholds(exact, metric)
    model = RG.survivors(approx, xt, qt, thr, metric, d, N)
    ref = RM.reference(exact, thr, ids_of, NQ * N)
    counts = np.diff(ref[0])
    # the preconditions, on the reference: 0 matches, 1 (or the 70 copies, where they are a query's best rows), about 100
    assert (counts[2::3] == 0).all() and counts[0] == len(TIES) and np.isin(counts[6::3], (1, len(TIES))).all()
    assert (counts[1::3] >= 100).all() and (counts[1::3] < 100 + len(TIES)).all()
    assert model.certified.all() and (model.above[3] and model.n_survivors[3] == 0) == (metric == "l2")
    for nq in (1, 33, NQ):
        got = ranged(dix, t, b, sc, q[:nq], thr[:nq], cap=N, fallback=False)
        total = int(ref[0][nq])
        assert (got[0] == ref[0][:nq + 1]).all() and got[4].all() and (got[5] == model.n_survivors[:nq]).all(), nq
        assert (got[1][:total] == ref[1][:total]).all() and (got[3][:total] == ref[3][:total]).all(), nq
        assert (bits(got[2][:total]) == bits(ref[2][:total])).all(), nq


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_a_cap_below_the_survivor_count_is_uncertified(metric):
    d, k, fetch, sample_rows = 64, 10, 32, 300
    x, q, dix, t, b, xt, qt, sc, approx, exact = case(d, "f16", metric)
    ids_of = dix.item_ids.cpu().numpy()
    ref = [M.topk(s, k) for s in exact]
    rows, scores = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
    tau, a_rows, a_scores, keep = model_topk(approx, exact, xt, qt, metric, d, k, fetch, sample_rows)
    n_surv = keep.sum(axis=1)
    cap = int(np.median(n_surv))
    over = n_surv > cap
    assert cap >= fetch and over.sum() >= 20 and (~over).sum() >= 20
    got = topk(dix, t, b, sc, q, k, fetch=fetch, sample_rows=sample_rows, cap=cap, fallback=False)
    assert (got[3] == ~over).all() and (got[4] == n_surv).all()                   # the true count, beyond the cap
    same_topk(got, rows, scores, ids_of, ~over, "certified")
    same_topk(got, a_rows, a_scores, ids_of, over, "the sample's fetch list")
    got = topk(dix, t, b, sc, q, k, fetch=fetch, sample_rows=sample_rows, cap=cap, fallback=True)
    same_topk(got, rows, scores, ids_of, np.arange(NQ), "fallback")
    # the range form at a cap below the 100 matches of every third query: those segments are empty, the others exact
    thr = thresholds(exact, metric)
    model = RG.survivors(approx, xt, qt, thr, metric, d, 64)
    assert 30 < (~model.certified).sum() < NQ - 30
    ref = RM.reference(exact, thr, ids_of, NQ * N)
    got = ranged(dix, t, b, sc, q, thr, cap=64, fallback=False)
    assert (got[4] == model.certified).all() and (got[5] == model.n_survivors).all()
    assert (np.diff(got[0])[~model.certified] == 0).all()
    g, e = RG.segments(got[:4]), RG.segments(ref)
    assert all((a == o).all() for i in np.flatnonzero(model.certified) for a, o in zip(g[i], e[i]))
    got = ranged(dix, t, b, sc, q, thr, cap=64, fallback=True)
    total = int(ref[0][-1])
    assert (got[0] == ref[0]).all() and (got[1] == ref[1][:total]).all() and (bits(got[2]) == bits(ref[2][:total])).all()


@pytest.mark.parametrize("what,status", [("mlp", 102), ("bounds", 7), ("k > fetch", 7)])
def test_refusals_stand_in_front_of_any_launch(what, status):
    """raw calls without a workspace: a refusal by the arguments comes first, nothing is written"""
    from nann_amd import _lib, ops, retrieval, synth
    from nann_amd.ops import _ptr, _stream
    x, q, dix, t, b, xt, qt, sc, approx, exact = case(64, "f16", "l2")
    if what == "mlp":
        sc = ops.Scorer("mlp", 64, torch.float16, synth.make_mlp_weights(64), precision="exact")
    if what == "bounds":
        b = retrieval.make_sq8_bounds(dix, retrieval.make_sq8(dix))              # the same index, another table
    k = 11 if what == "k > fetch" else 10
    qd, thr = cuda(q[:4]), cuda(np.zeros(4, F))
    out = [torch.full((4 * 16,), -77, dtype=dt, device="cuda") for dt in (torch.int64, torch.float32, torch.int32, torch.int32, torch.int32)]
    splits = torch.full((5,), -77, dtype=torch.int64, device="cuda")
    L, nb = _lib.lib(), C.c_int64(-1)
    assert L.nann_search_all_sq8_stream_exact_workspace_bytes(dix.handle, t.handle, b.handle, sc.handle, 4, 10, 0, N, k, C.byref(nb)) == status
    assert L.nann_search_all_sq8_stream_exact(dix.handle, t.handle, b.handle, sc.handle, _ptr(qd), 4, 10, 0, N, k, *[_ptr(o) for o in out],
                                              None, 0, None, _stream()) == status
    if what != "k > fetch":                                                       # (the range form has no k)
        assert L.nann_search_all_range_sq8_stream_exact_workspace_bytes(dix.handle, t.handle, b.handle, sc.handle, 4, N, C.byref(nb)) == status
        assert L.nann_search_all_range_sq8_stream_exact(dix.handle, t.handle, b.handle, sc.handle, _ptr(qd), 4, _ptr(thr), N, 16, _ptr(splits),
                                                        *[_ptr(o) for o in out], None, 0, None, _stream()) == status
    torch.cuda.synchronize()
    assert all((o == -77).all() for o in out + [splits]) and nb.value == -1
    assert _status(lambda: retrieval.search_all_sq8_stream_exact(dix, t, b, sc, qd, k, fetch=10, cap=N)) == status
