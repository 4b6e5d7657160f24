"""-m gpu: the certified scalar-quantised search (nann_sq8_bounds / nann_search_all_sq8_exact, retrieval.search_all_sq8_exact):
the error terms against float64 and the numpy model, the survivor lists against the model's predicate row for row, the result
against retrieval.search_all BIT FOR BIT on inputs where the plain two-stage call at the same fetch is wrong, the overflow path
with guard words, batch independence, a NaN query, the refusals.  The only tolerance is the one the contract states for err and
xhat (at most 2^-10 above the real value).  Inputs and indices are test_sq8_gpu.py's, restated."""
import ctypes as C

import numpy as np
import pytest
import torch

import sq8_exact_model as X
import sq8_model as M
from gpu_util import bits, cuda, require_gpu

pytestmark = pytest.mark.gpu
_CACHE = {}
F = np.float32
CAP = 2048


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
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, d)) * np.exp(rng.uniform(-2.0, 2.0, (n, 1)))).astype(F)
    if dtype == "f16":
        return x.astype(np.float16)
    return (x.view(np.uint32) >> 16).astype(np.uint16)


def _case(n, d, dtype="f16"):
    """(rows, device index, code table, bounds, the table's model, 130 queries f32, their model) -- made once"""
    key = (n, d, dtype)
    if key not in _CACHE:
        from nann_amd import retrieval
        x = _rows(n, d, n + d, dtype)
        dix = _index(x)
        t = retrieval.make_sq8(dix)
        q = np.random.default_rng(d).standard_normal((130, d)).astype(F)
        q[5] *= F(0.01)
        _CACHE[key] = (x, dix, t, retrieval.make_sq8_bounds(dix, t), M.encode(x), q, M.encode(q))
    return _CACHE[key]


def _scorer(metric, d, dtype=torch.float16):
    from nann_amd import ops
    key = ("scorer", metric, d, dtype)
    if key not in _CACHE:
        _CACHE[key] = ops.Scorer(metric, d, dtype)
    return _CACHE[key]


def _np(r):
    torch.cuda.synchronize()
    return (r.index.cpu().numpy(), r.scores.cpu().numpy(), r.item_ids.cpu().numpy())


def _exact(dix, t, b, sc, q, k, fetch=None, cap=CAP, fallback=False):
    from nann_amd import retrieval
    r = retrieval.search_all_sq8_exact(dix, t, b, sc, cuda(q, torch.float32), k, fetch=fetch, cap=cap, fallback=fallback)
    return _np(r) + (r.certified.cpu().numpy(), r.n_survivors.cpu().numpy(), r)


def _layout(dix, t, b, sc, n_q, fetch, cap, k):
    from nann_amd import _lib
    out = (C.c_int64 * 8)()
    assert _lib.lib().nann_search_all_sq8_exact_layout(dix.handle, t.handle, b.handle, sc.handle, n_q, fetch, cap, k, out) == 0
    return dict(zip(("chunk", "cap", "off_splits", "off_rows", "off_terms", "term_bytes", "off_a_scores", "total"), [int(v) for v in out]))


def _status(fn):
    from nann_amd import ops
    try:
        fn()
    except ops.NannError as e:
        return e.status
    return 0


# ---- 1. err and xhat --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d", [64, 128, 512])
def test_err_and_xhat_bound_the_real_values(d, dtype):
    from nann_amd import retrieval
    n = 1007
    x = _rows(n, d, d, dtype)
    dix = _index(x)
    t = retrieval.make_sq8(dix)
    b = retrieval.make_sq8_bounds(dix, t)
    err, xhat = b.err().cpu().numpy(), b.xhat().cpu().numpy()
    enc = M.encode(x)
    r_err, r_xhat = X.real_terms(x, enc)
    assert (err.astype(np.float64) >= r_err).all() and (err <= r_err * (1 + 2.0 ** -10)).all()
    assert (xhat.astype(np.float64) >= r_xhat).all() and (xhat <= r_xhat * (1 + 2.0 ** -10)).all()
    m_err, m_xhat = X.row_terms(x, enc)                   # and the stated order of operations, bit for bit
    assert (bits(err) == bits(m_err)).all() and (bits(xhat) == bits(m_xhat)).all()
    b.release()
    with pytest.raises(ValueError):
        b.err()


# ---- 2. the survivors -------------------------------------------------------------------------------------------------------
def _survivor_check(n, d, metric, k):
    """the device's n_survivors for 130 queries (two chunks) and, chunk by chunk, its survivor lists and query terms against the
    model's predicate on the device's err, xhat and cut"""
    from nann_amd import retrieval
    x, dix, t, b, xe, q, qe = _case(n, d)
    sc = _scorer(metric, d)
    approx = M.approx_scores(qe, xe, metric)
    err, xhat = b.err().cpu().numpy(), b.xhat().cpu().numpy()
    plain = retrieval.search_all_sq8(dix, t, sc, cuda(q, torch.float32), k, fetch=k)
    torch.cuda.synchronize()
    tau = plain.scores.cpu().numpy()[:, k - 1]
    eq, qhat = X.row_terms(q, qe)
    w, ok = X.query_terms(tau, eq, qhat, metric, d)
    keep = X.survives(approx, err, xhat, tau, eq, qhat, w, metric, d)
    assert ok.all()
    rows, scores, ids, cert, n_surv, _ = _exact(dix, t, b, sc, q, k)
    assert (n_surv == keep.sum(axis=1)).all()
    assert (cert == (keep.sum(axis=1) <= CAP)).all() and cert.all()
    for lo, hi in ((0, 128), (128, 130)):
        lay = _layout(dix, t, b, sc, hi - lo, k, CAP, k)
        assert lay["chunk"] == hi - lo and lay["term_bytes"] == 32
        r = _exact(dix, t, b, sc, q[lo:hi], k)
        assert (r[4] == n_surv[lo:hi]).all()
        ws = r[5]._ws.cpu().numpy()
        n_q = hi - lo
        splits = ws[lay["off_splits"]:lay["off_splits"] + 8 * (n_q + 1)].view(np.int64)
        lists = ws[lay["off_rows"]:lay["off_rows"] + 4 * int(splits[-1])].view(np.int32)
        terms = ws[lay["off_terms"]:lay["off_terms"] + 32 * n_q].view(np.uint32).reshape(n_q, 8)
        assert (terms[:, 0] == bits(tau[lo:hi])).all()
        assert (terms[:, 1] == bits(eq[lo:hi])).all() and (terms[:, 2] == bits(qhat[lo:hi])).all()
        assert (terms[:, 3] == bits(w[lo:hi])).all() and (terms[:, 4:6] == 1).all()
        assert splits[0] == 0 and (np.diff(splits) == n_surv[lo:hi]).all()
        for i in range(n_q):
            assert (lists[splits[i]:splits[i + 1]] == np.flatnonzero(keep[lo + i])).all(), i


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_survivors_equal_the_models_predicate_over_several_blocks(metric):
    """n = 16417: nine range blocks of 2048 positions, the last one ragged, and a query's first block misaligned"""
    _survivor_check(16417, 128, metric, 200)


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d", [64, 256])
def test_survivors_equal_the_models_predicate_over_two_chunks(d, metric):
    _survivor_check(1007, d, metric, 10)


# ---- 3. exactness -----------------------------------------------------------------------------------------------------------
def _exactness(n, d, metric, k, dtype="f16"):
    from nann_amd import retrieval
    x, dix, t, b, xe, q, qe = _case(n, d, dtype)
    sc = _scorer(metric, d, torch.float16 if dtype == "f16" else torch.bfloat16)
    qd = cuda(q, torch.float32)
    ref = _np(retrieval.search_all(dix, sc, qd, k))
    plain = _np(retrieval.search_all_sq8(dix, t, sc, qd, k, fetch=k))
    rows, scores, ids, cert, n_surv, _ = _exact(dix, t, b, sc, q, k, fetch=k)
    print("n=%d d=%d %s %s k=%d: survivors mean %.1f max %d; plain sq8 wrong for %d of 130 queries"
          % (n, d, metric, dtype, k, n_surv.mean(), n_surv.max(), (plain[0] != ref[0]).any(axis=1).sum()))
    assert (plain[0] != ref[0]).any(), "the plain two-stage call is already exact here: the case shows nothing"
    assert cert.all() and (n_surv <= CAP).all() and (n_surv >= k).all()
    assert (rows == ref[0]).all()
    assert (bits(scores) == bits(ref[1])).all()
    assert (ids == ref[2]).all()


@pytest.mark.parametrize("k", [10, 200])
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d", [64, 128, 512])
@pytest.mark.parametrize("n", [1007, 16417])
def test_equals_search_all_bit_for_bit(n, d, metric, k):
    _exactness(n, d, metric, k)


def test_equals_search_all_bit_for_bit_bf16():
    _exactness(16417, 128, "l2", 200, "bf16")


# ---- 4. overflow ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_overflow_returns_the_plain_answer_and_writes_nothing_past_cap(metric):
    from nann_amd import _lib, retrieval
    from nann_amd.ops import _ptr, _stream
    n, d, k, nq = 4099, 64, 10, 5
    key = ("same", n)
    if key not in _CACHE:
        x = np.repeat(_rows(1, d, 5), n, axis=0)
        dix = _index(x)
        t = retrieval.make_sq8(dix)
        _CACHE[key] = (x, dix, t, retrieval.make_sq8_bounds(dix, t))
    x, dix, t, b = _CACHE[key]
    sc = _scorer(metric, d)
    q = np.random.default_rng(2).standard_normal((nq, d)).astype(F)
    qd = cuda(q, torch.float32)
    plain = _np(retrieval.search_all_sq8(dix, t, sc, qd, k, fetch=k))
    rows, scores, ids, cert, n_surv, _ = _exact(dix, t, b, sc, q, k, fetch=k, cap=CAP)
    assert (cert == 0).all() and (n_surv == n).all()
    assert (rows == plain[0]).all() and (bits(scores) == bits(plain[1])).all() and (ids == plain[2]).all()
    assert (rows == np.arange(k)).all()
    # guard words behind every buffer of the caller, and the room of the lists behind the copied fetch lists untouched
    L = _lib.lib()
    nb = C.c_int64(0)
    assert L.nann_search_all_sq8_exact_workspace_bytes(dix.handle, t.handle, b.handle, sc.handle, nq, k, CAP, k, C.byref(nb)) == 0
    lay = _layout(dix, t, b, sc, nq, k, CAP, k)
    assert lay["total"] == nb.value and lay["cap"] == CAP
    G = 64
    ws = torch.full((nb.value + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    o_ids = torch.full((nq * k + G,), -77, dtype=torch.int64, device="cuda")
    o_sc = torch.full((nq * k + G,), -77.0, dtype=torch.float32, device="cuda")
    o_ix = torch.full((nq * k + G,), -77, dtype=torch.int32, device="cuda")
    o_ce = torch.full((nq + G,), -77, dtype=torch.int32, device="cuda")
    o_ns = torch.full((nq + G,), -77, dtype=torch.int32, device="cuda")
    assert L.nann_search_all_sq8_exact(dix.handle, t.handle, b.handle, sc.handle, _ptr(qd), nq, k, CAP, k, _ptr(o_ids), _ptr(o_sc),
                                       _ptr(o_ix), _ptr(o_ce), _ptr(o_ns), _ptr(ws), nb.value, None, _stream()) == 0
    torch.cuda.synchronize()
    for buf, used in ((o_ids, nq * k), (o_sc, nq * k), (o_ix, nq * k), (o_ce, nq), (o_ns, nq)):
        assert (buf[used:] == -77).all()
    assert (o_ix[:nq * k].cpu().numpy().reshape(nq, k) == plain[0]).all() and (o_ce[:nq] == 0).all() and (o_ns[:nq] == n).all()
    assert (ws[nb.value:] == 0xA5).all(), "the call wrote behind its workspace"
    w = ws.cpu().numpy()
    splits = w[lay["off_splits"]:lay["off_splits"] + 8 * (nq + 1)].view(np.int64)
    assert splits.tolist() == [i * k for i in range(nq + 1)]                  # the fetch lists, not 4099 survivors each
    room = w[lay["off_rows"]:lay["off_rows"] + 4 * nq * CAP].view(np.uint32)
    assert (room[:nq * k].reshape(nq, k) == np.arange(k)).all() and (room[nq * k:] == 0xA5A5A5A5).all()
    # with the fallback the result is search_all's
    ref = _np(retrieval.search_all(dix, sc, qd, k))
    rows, scores, ids, cert, n_surv, _ = _exact(dix, t, b, sc, q, k, fetch=k, cap=CAP, fallback=True)
    assert (rows == ref[0]).all() and (bits(scores) == bits(ref[1])).all() and (ids == ref[2]).all() and (cert == 0).all()
    # and a cap that holds every row certifies: the ties at tau all survive, the lower rows win
    rows, scores, ids, cert, n_surv, _ = _exact(dix, t, b, sc, q, k, fetch=k, cap=n)
    assert cert.all() and (n_surv == n).all() and (rows == ref[0]).all() and (bits(scores) == bits(ref[1])).all()


# ---- 5. batch independence, non-finite queries ---------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_answer_does_not_depend_on_the_batch(metric):
    x, dix, t, b, xe, q, qe = _case(16417, 128)
    sc = _scorer(metric, 128)
    batch = _exact(dix, t, b, sc, q, 50, fetch=50)[:5]
    for i in (77, 129):
        alone = _exact(dix, t, b, sc, q[i:i + 1], 50, fetch=50)[:5]
        for a, o in zip(batch, alone):
            assert (bits(a[i]) == bits(o[0])).all() if a.dtype == np.float32 else (a[i] == o[0]).all()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_a_nan_query_is_uncertified_and_leaves_its_neighbours_alone(metric):
    from nann_amd import retrieval
    x, dix, t, b, xe, q, qe = _case(1007, 64)
    sc = _scorer(metric, 64)
    clean = _exact(dix, t, b, sc, q[:8], 10, fetch=10)[:5]
    bad = q[:8].copy()
    bad[3, 7] = np.nan
    got = _exact(dix, t, b, sc, bad, 10, fetch=10)[:5]
    assert got[3].tolist() == [1, 1, 1, 0, 1, 1, 1, 1]
    others = [0, 1, 2, 4, 5, 6, 7]
    for a, o in zip(clean, got):
        assert (bits(a[others]) == bits(o[others])).all() if a.dtype == np.float32 else (a[others] == o[others]).all()
    plain = _np(retrieval.search_all_sq8(dix, t, sc, cuda(bad, torch.float32), 10, fetch=10))
    assert (got[0][3] == plain[0][3]).all() and (bits(got[1][3]) == bits(plain[1][3])).all()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_failure_codes():
    from nann_amd import _lib, ops, retrieval, synth
    from nann_amd.ops import _ptr, _stream
    x, dix, t, b, xe, q, qe = _case(1007, 64)
    x2, dix2, t2, b2 = _case(16417, 64)[:4]
    sc = _scorer("l2", 64)
    qd = cuda(q[:4])
    run = lambda **kw: retrieval.search_all_sq8_exact(kw.pop("ix", dix), kw.pop("t", t), kw.pop("b", b), kw.pop("sc", sc), qd,  # noqa: E731
                                                      fallback=False, **kw)
    assert _status(lambda: run(b=None, k=10)) == 7                               # a NULL bounds object
    assert _status(lambda: run(b=b2, k=10)) == 7                                 # bounds made from another index
    assert b"another index or code table" in _lib.lib().nann_last_error()
    t_again = retrieval.make_sq8(dix)                                            # the same index, another table
    assert _status(lambda: run(t=t_again, k=10)) == 7
    assert _status(lambda: run(k=10, fetch=20, cap=19)) == 7                     # cap < fetch
    assert _status(lambda: run(k=10, fetch=20, cap=2 ** 31)) == 102              # cap beyond the longest candidate list
    assert b"longest list" in _lib.lib().nann_last_error()
    assert _status(lambda: run(k=11, fetch=10)) == 7 and _status(lambda: run(k=10, fetch=1008)) == 4
    mlp = ops.Scorer("mlp", 64, torch.float16, synth.make_mlp_weights(64), precision="exact")
    assert _status(lambda: run(sc=mlp, k=10)) == 102                             # an MLP scorer
    assert _status(lambda: run(k=10)) == 0
    L = _lib.lib()
    nb, nb0, nb_big = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    size = lambda n, k, out: L.nann_search_all_sq8_exact_workspace_bytes(dix.handle, t.handle, b.handle, sc.handle, n, 20, CAP, k, C.byref(out))  # noqa: E731
    assert size(4, 0, nb0) == 0 and nb0.value == 0 and size(0, 10, nb0) == 0 and nb0.value == 0
    assert size(128, 10, nb) == 0 and size(4096, 10, nb_big) == 0 and nb.value == nb_big.value   # bounded by the chunk
    assert size(4, 10, nb) == 0 and nb.value > 0
    ws = torch.full((nb.value + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    outs = [torch.full((4, 10), -77, dtype=dt, device="cuda") for dt in (torch.int64, torch.float32, torch.int32)]
    flags = [torch.full((4,), -77, dtype=torch.int32, device="cuda") for _ in range(2)]

    def call(nbytes, n=4, k=10):
        st = L.nann_search_all_sq8_exact(dix.handle, t.handle, b.handle, sc.handle, _ptr(qd), n, 20, CAP, k, *[_ptr(o) for o in outs],
                                         *[_ptr(f) for f in flags], _ptr(ws), nbytes, None, _stream())
        torch.cuda.synchronize()
        return st
    assert call(nb.value - 1) == 103                                             # a short workspace
    assert call(nb.value, k=0) == 0 and call(nb.value, n=0) == 0                 # nothing to do: nothing written
    assert all((o == -77).all() for o in outs + flags) and (ws == 0xA5).all()
    assert call(nb.value) == 0 and (flags[0] == 1).all() and (ws[nb.value:] == 0xA5).all()
    ref = _exact(dix, t, b, sc, q[:4], 10, fetch=20)
    assert (outs[2].cpu().numpy() == ref[0]).all() and (outs[0].cpu().numpy() == ref[2]).all()
