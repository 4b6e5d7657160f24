"""-m gpu: the scalar-quantised exhaustive search (nann_sq8 / nann_search_all_sq8, retrieval.search_all_sq8) against the numpy
model of its contract (sq8_model), BIT FOR BIT: the codes, the approximate scores and the order of the fetch stage; the exact
scores of the result against nann_score (ops.blaze_score) and, at fetch = n_items, against retrieval.search_all.  No tolerance
appears anywhere.  The indices carry a ring graph (search_all_sq8 never reads it) so that nann_index_create sees a valid one."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import sq8_model as M
from gpu_util import bits, cuda, require_gpu

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu
_CACHE = {}
F = np.float32


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


# ---- helpers --------------------------------------------------------------------------------------------------------------
def _ring(n, deg=8):
    deg = min(deg, n - 1)
    nbv = ((np.arange(n, dtype=np.int64)[:, None] + 1 + np.arange(deg)) % n).astype(np.int32).reshape(-1)
    rs = (np.arange(n + 1, dtype=np.int64) * deg)
    step = max(n // 64, 1)
    return [nbv, nbv.copy()], [rs, rs.copy()], np.arange(0, n, step, dtype=np.int32)[:64]


def _index(embs):
    from nann_amd import retrieval
    n = embs.shape[0]
    nbv, rs, ep = _ring(n)
    return retrieval.Index(embs, np.arange(n, dtype=np.int64) * 7 + 3, nbv, rs, ep)


def _rows(n, d, seed, dtype="f16"):
    """Gaussian rows, every row at a magnitude of its own (the scales differ), as f16 or bf16 bit patterns"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, d)) * np.exp(rng.uniform(-2.0, 2.0, (n, 1)))).astype(F)
    if dtype == "f16":
        return x.astype(np.float16)
    return (x.view(np.uint32) >> 16).astype(np.uint16)


def _case(n, d, seed=0):
    """(rows f16, device index, code table, its model, 130 queries f32, their model) -- made once"""
    key = (n, d, seed)
    if key not in _CACHE:
        from nann_amd import retrieval
        x = _rows(n, d, seed + n + d)
        dix = _index(x)
        q = np.random.default_rng(seed + d).standard_normal((130, d)).astype(F)
        q[5] *= F(0.01)
        _CACHE[key] = (x, dix, retrieval.make_sq8(dix), M.encode(x), q, M.encode(q))
    return _CACHE[key]


def _approx(n, d, metric):
    key = ("approx", n, d, metric)
    if key not in _CACHE:
        x, dix, t, xe, q, qe = _case(n, d)
        _CACHE[key] = M.approx_scores(qe, xe, metric)
    return _CACHE[key]


def _scorer(metric, d, dtype=torch.float16):
    from nann_amd import ops
    key = ("scorer", metric, d, dtype)
    if key not in _CACHE:
        _CACHE[key] = ops.Scorer(metric, d, dtype)
    return _CACHE[key]


def _run(dix, t, sc, q, k, fetch):
    from nann_amd import retrieval
    r = retrieval.search_all_sq8(dix, t, sc, cuda(q, torch.float32), k, fetch=fetch, return_fetch=True)
    torch.cuda.synchronize()
    return (r.index.cpu().numpy(), r.scores.cpu().numpy(), r.item_ids.cpu().numpy(), r.fetch_index.cpu().numpy(),
            r.fetch_scores.cpu().numpy())


def _exact_on_device(dix, sc, q):
    """exact_of for sq8_model.rerank: nann_score's bits for (query qi, rows)"""
    from nann_amd import ops

    def of(qi, rows):
        s = ops.blaze_score(sc, cuda(q[qi]), table=dix.item_embs, indices=cuda(rows.astype(np.int32)))
        return s.cpu().numpy()
    return of


def _status(fn):
    from nann_amd import ops
    try:
        fn()
    except ops.NannError as e:
        return e.status
    return 0


# ---- 1. the lane map ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
def test_lane_map_one_hot_queries(d):
    """queries e_j for every j < d against rows whose codes differ in every (row, j): query j's scores are column j of the code
    matrix, so one misplaced (lane, k) position of either operand, or a row / query swap in the store, changes a bit"""
    from nann_amd import retrieval
    n = 96
    rng = np.random.default_rng(d)
    c = rng.integers(-126, 127, (n, d)).astype(np.int32)
    c[np.arange(n), (np.arange(n) * 5 + 3) % d] = 127          # amax = 127 / 128: scale = 2^-7, code = 128 x
    m = min(n, d)
    assert len({tuple(col) for col in c.T}) == d and len({tuple(row) for row in c}) == n and (c[:m, :m] != c[:m, :m].T).any()
    x = (c.astype(F) / F(128.0)).astype(np.float16)
    dix = _index(x)
    t = retrieval.make_sq8(dix)
    xe = M.encode(x)
    assert (xe[0] == c).all()
    assert (t.codes().cpu().numpy() == c).all() and (bits(t.scales().cpu().numpy()) == bits(xe[1])).all()
    q = np.eye(d, dtype=F)
    qe = M.encode(q)
    assert (qe[0] == 127 * np.eye(d, dtype=np.int32)).all()
    for metric in ("ip", "l2"):
        approx = M.approx_scores(qe, xe, metric)
        if metric == "ip":
            assert (approx == ((qe[1][:, None] * xe[1][None, :]) * (127 * c.T).astype(F))).all()
        e_rows, e_scores = M.fetch(approx, n)
        rows, scores, ids, f_rows, f_scores = _run(dix, t, _scorer(metric, d), q, 1, n)
        assert (f_rows == e_rows).all(), metric
        assert (bits(f_scores) == bits(e_scores)).all(), metric


# ---- 2. the encoder -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d", [64, 128, 512])
def test_encode_equals_the_model(d, dtype):
    from nann_amd import ops, retrieval
    n = 1007
    x = _rows(n, d, d, dtype)
    x[3] = 0
    x[4, 7] = 0x8000 if dtype == "bf16" else -0.0
    if dtype == "f16":
        x[9, 11] = 65504.0
        x[10] = np.float16(6e-8)                          # subnormal rows
    x[11, :] = x[11, 0]                                   # every element at amax
    dix = _index(x)
    t = retrieval.make_sq8(dix)
    codes, scales, norms = M.encode(x)
    assert (t.n_items, t.d) == (n, d) and t.nbytes == n * d + 8 * n
    assert (t.codes().cpu().numpy() == codes).all()
    assert (bits(t.scales().cpu().numpy()) == bits(scales)).all()
    assert (t.norms().cpu().numpy() == norms).all()
    assert (codes[3] == 0).all() and scales[3] == 0 and np.abs(codes[11]).min() == 127
    q = np.random.default_rng(d + 1).standard_normal((37, d)).astype(F)
    q[2] = 0
    q[3] *= F(1e-30)
    q[4, 5] = F(3e38)
    got = [a.cpu().numpy() for a in ops.sq8_encode(cuda(q))]
    exp = M.encode(q)
    assert (got[0] == exp[0]).all() and (bits(got[1]) == bits(exp[1])).all() and (got[2] == exp[2]).all()
    t.release()
    with pytest.raises(ValueError):
        t.codes()


# ---- 3. the scan against the model ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("n", [1007, 16417])
@pytest.mark.parametrize("d", [64, 128, 256, 512])
def test_fetch_stage_bitwise(d, n, metric):
    """n = 1007: a row-tile tail in one slab; n = 16417: two slabs and a tail.  n_queries 1, 33 (a query-tile tail), 130 (two
    chunks); fetch 1, 200, 1024 (min(fetch, n_items))"""
    x, dix, t, xe, q, qe = _case(n, d)
    approx = _approx(n, d, metric)
    sc = _scorer(metric, d)
    for fetch in (1, 200, min(1024, n)):
        e_rows, e_scores = M.fetch(approx, fetch)
        for b in (1, 33, 130):
            rows, scores, ids, f_rows, f_scores = _run(dix, t, sc, q[:b], min(fetch, 10), fetch)
            assert (f_rows == e_rows[:b]).all(), (fetch, b)
            assert (bits(f_scores) == bits(e_scores[:b])).all(), (fetch, b)
            assert (ids == dix.item_ids.cpu().numpy()[rows]).all()


# ---- 4. ties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_ties_go_to_the_lower_row_in_both_stages(metric):
    """n = 32768 is two slabs of 16384 rows; blocks of identical rows straddle row 16384, in a run and scattered"""
    from nann_amd import retrieval
    key = "ties"
    if key not in _CACHE:
        n, d = 32768, 64
        x = _rows(n, d, 77)
        x[16380:16390] = x[16380]                       # a run across the slab boundary
        for r in (5, 16379, 16390, 30000):              # a scattered block, copies on either side of it
            x[r] = x[100]
        dix = _index(x)
        _CACHE[key] = (x, dix, retrieval.make_sq8(dix), M.encode(x))
    x, dix, t, xe = _CACHE[key]
    q = np.stack([x[16380].astype(F), x[100].astype(F), x[16380].astype(F) * F(1.5) + F(0.001)])
    sc = _scorer(metric, 64)
    approx = M.approx_scores(M.encode(q), xe, metric)
    for fetch, k in ((4, 3), (64, 12), (1024, 1024)):
        e_rows, e_scores = M.fetch(approx, fetch)
        rows, scores, ids, f_rows, f_scores = _run(dix, t, sc, q, k, fetch)
        assert (f_rows == e_rows).all() and (bits(f_scores) == bits(e_scores)).all(), fetch
        m_rows, m_scores = M.rerank(f_rows, _exact_on_device(dix, sc, q), k)
        assert (rows == m_rows).all() and (bits(scores) == bits(m_scores)).all(), fetch
    # the blocks are there, in row order, in both stages (L2: the query's own copies lead the list)
    rows, scores, ids, f_rows, f_scores = _run(dix, t, sc, q, 12, 64)
    run, block = list(range(16380, 16390)), [5, 100, 16379, 16390, 30000]
    for lst, sco in ((f_rows, f_scores), (rows, scores)):
        for b, members in ((0, run), (1, block), (2, run)):
            at = [int(np.flatnonzero(lst[b] == r)[0]) for r in members if (lst[b] == r).any()]
            if metric == "l2":
                assert len(at) == len(members), (b, "every copy of the nearest row is in the list")
            assert at == sorted(at) and (np.diff(at) == 1).all(), (b, at)
            assert len(set(bits(sco[b][at]).tolist())) <= 1
    if metric == "l2":
        assert f_rows[0, :10].tolist() == run and rows[0, :10].tolist() == run and f_rows[1, :5].tolist() == block


# ---- 5. the re-rank --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_rerank_scores_are_nann_score_bits_and_the_models_selection(metric):
    from nann_amd import ops
    x, dix, t, xe, q, qe = _case(16417, 128)
    sc = _scorer(metric, 128)
    b = 33
    for fetch, k in ((200, 50), (1024, 200), (7, 7)):
        rows, scores, ids, f_rows, f_scores = _run(dix, t, sc, q[:b], k, fetch)
        exact_of = _exact_on_device(dix, sc, q)
        for i in range(b):
            assert (bits(exact_of(i, rows[i])) == bits(scores[i])).all(), (fetch, i)
        m_rows, m_scores = M.rerank(f_rows, exact_of, k)
        assert (rows == m_rows).all() and (bits(scores) == bits(m_scores)).all(), fetch
        assert (ids == dix.item_ids.cpu().numpy()[rows]).all()
        assert all(set(rows[i]) <= set(f_rows[i]) for i in range(b))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_fetch_everything_equals_search_all(metric, dtype):
    from nann_amd import retrieval
    n, d = 1000, 128
    x = _rows(n, d, 31, dtype)
    x[500:503] = x[20]                                   # exact ties in the final order
    dix = _index(x)
    t = retrieval.make_sq8(dix)
    sc = _scorer(metric, d, torch.float16 if dtype == "f16" else torch.bfloat16)
    q = np.random.default_rng(8).standard_normal((33, d)).astype(F)
    q[0] = M.widen(x[20:21])[0]
    for k in (1, 200, 1000):
        ref = retrieval.search_all(dix, sc, cuda(q), k)
        rows, scores, ids, f_rows, f_scores = _run(dix, t, sc, q, k, n)
        assert (rows == ref.index.cpu().numpy()).all(), k
        assert (bits(scores) == bits(ref.scores.cpu().numpy())).all(), k
        assert (ids == ref.item_ids.cpu().numpy()).all(), k
        assert (np.sort(f_rows, axis=1) == np.arange(n)).all()


# ---- 6. batch independence ---------------------------------------------------------------------------------------------------
def test_answer_does_not_depend_on_the_batch():
    x, dix, t, xe, q, qe = _case(16417, 128)
    for metric in ("l2", "ip"):
        sc = _scorer(metric, 128)
        batch = _run(dix, t, sc, q, 50, 200)
        alone = _run(dix, t, sc, q[77:78], 50, 200)
        for a, b in zip(batch, alone):
            if a.dtype == np.float32:
                assert (bits(a[77]) == bits(b[0])).all()
            else:
                assert (a[77] == b[0]).all()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------
def test_failure_codes_and_the_workspace_rule():
    from nann_amd import _lib, ops, retrieval, synth
    from nann_amd.ops import _ptr, _stream
    x, dix, t, xe, q, qe = _case(1007, 64)
    x2, dix2, t2 = _case(16417, 64)[:3]
    sc = _scorer("l2", 64)
    qd = cuda(q[:4])
    run = lambda **kw: retrieval.search_all_sq8(kw.pop("ix", dix), kw.pop("t", t), kw.pop("sc", sc), qd, **kw)  # noqa: E731
    assert _status(lambda: run(ix=dix2, t=t2, k=10, fetch=1025)) == 102          # fetch > 1024
    assert _status(lambda: run(k=11, fetch=10)) == 7                             # k > fetch
    assert _status(lambda: run(k=10, fetch=1008)) == 4                           # fetch > n_items
    assert _status(lambda: run(k=-1, fetch=10)) == 7 and _status(lambda: run(k=1, fetch=-1)) == 7
    mlp = ops.Scorer("mlp", 64, torch.float16, synth.make_mlp_weights(64), precision="exact")
    assert _status(lambda: run(sc=mlp, k=10, fetch=20)) == 102                   # an MLP scorer
    assert _status(lambda: run(t=t2, k=10, fetch=20)) == 7                       # a table from another index (other n_items)
    assert b"another index" in _lib.lib().nann_last_error()
    dix3 = _index(x)                                                             # the same rows, another index all the same
    assert _status(lambda: run(ix=dix3, k=10, fetch=20)) == 7
    x32 = _index(M.widen(x[:200]))
    assert _status(lambda: retrieval.make_sq8(x32)) == 102                       # f32 rows
    assert _status(lambda: run(k=10, fetch=20)) == 0
    # k == 0 / no queries: NANN_OK, nothing written; the workspace: one byte short -> CAPACITY, off the grid -> BAD_ARGUMENT
    L = _lib.lib()
    nb = C.c_int64(-1)
    assert L.nann_search_all_sq8_workspace_bytes(dix.handle, t.handle, sc.handle, 4, 20, 0, C.byref(nb)) == 0 and nb.value == 0
    assert L.nann_search_all_sq8_workspace_bytes(dix.handle, t.handle, sc.handle, 0, 20, 10, C.byref(nb)) == 0 and nb.value == 0
    assert L.nann_search_all_sq8_workspace_bytes(dix.handle, t.handle, sc.handle, 4, 20, 10, C.byref(nb)) == 0 and nb.value > 0
    nb1024 = C.c_int64(-1)
    assert L.nann_search_all_sq8_workspace_bytes(dix.handle, t.handle, sc.handle, 4096, 20, 10, C.byref(nb1024)) == 0
    nb128 = C.c_int64(-1)
    assert L.nann_search_all_sq8_workspace_bytes(dix.handle, t.handle, sc.handle, 128, 20, 10, C.byref(nb128)) == 0
    assert nb1024.value == nb128.value                                           # bounded by the chunk
    page = 4096
    ws = torch.full((nb.value + 256 + page,), 0xA5, dtype=torch.uint8, device="cuda")
    out_ids = torch.full((4, 10), -77, dtype=torch.int64, device="cuda")
    f_idx = torch.full((4, 20), -77, dtype=torch.int32, device="cuda")

    def call(wsp, nbytes, n=4, k=10):
        st = L.nann_search_all_sq8(dix.handle, t.handle, sc.handle, _ptr(qd), n, 20, k, _ptr(out_ids), None, None, _ptr(f_idx), None,
                                   wsp, nbytes, None, _stream())
        torch.cuda.synchronize()
        return st
    assert call(_ptr(ws), nb.value - 1) == 103
    assert call(C.c_void_p(ws.data_ptr() + 8), nb.value) == 7 and b"aligned" in L.nann_last_error()
    assert call(_ptr(ws), nb.value, n=0) == 0 and call(_ptr(ws), nb.value, k=0) == 0
    assert (out_ids == -77).all() and (f_idx == -77).all() and (ws == 0xA5).all()
    assert call(_ptr(ws), nb.value) == 0                                         # NULL out_scores / out_index / out_fetch_scores
    assert (ws[nb.value:] == 0xA5).all(), "the call wrote behind its workspace"
    ref = _run(dix, t, sc, q[:4], 10, 20)
    assert (out_ids.cpu().numpy() == ref[2]).all() and (f_idx.cpu().numpy() == ref[3]).all()
