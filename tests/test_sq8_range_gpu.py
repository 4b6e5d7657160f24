"""-m gpu: the certified scalar-quantised range search (nann_search_all_range_sq8_exact, retrieval.search_all_range_sq8_exact)
against retrieval.search_all_range BIT FOR BIT -- row_splits, index, item ids, score bits -- and its two counters against the
numpy model (sq8_range_model) for every query; the overflow path and the fallback; thresholds that are not finite and the L2
rule above +0; the count-only call, truncation with guard words on both sides of every output, batch independence; the
refusals.  No tolerance appears.  The shapes: n = 1 007 and 2 051 (2 051 crosses a block of 2 048 positions, neither is a
multiple of 4, so a query's first block is misaligned), 130 queries = two chunks of 128 + 2.  The thresholds are bit patterns of
the device's own exact scores, so that a threshold at a duplicated row's score is a threshold at a tie."""
import ctypes as C

import numpy as np
import pytest
import torch

import sq8_exact_model as X
import sq8_model as M
import sq8_range_model as RG
from gpu_util import bits, cuda, require_gpu

pytestmark = pytest.mark.gpu
_CACHE = {}
F = np.float32
OK, BAD, UNSUPPORTED, CAPACITY = 0, 7, 102, 103
S = -77


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


# ---- helpers --------------------------------------------------------------------------------------------------------------
def _ring(n, deg=8):
    nbv = ((np.arange(n, dtype=np.int64)[:, None] + 1 + np.arange(deg)) % n).astype(np.int32).reshape(-1)
    rs = (np.arange(n + 1, dtype=np.int64) * deg)
    return [nbv, nbv.copy()], [rs, rs.copy()], np.arange(0, n, max(n // 64, 1), dtype=np.int32)[:64]


def _index(embs):
    from nann_amd import retrieval
    n = embs.shape[0]
    nbv, rs, ep = _ring(n)
    return retrieval.Index(embs, np.arange(n, dtype=np.int64) * 7 + 3, nbv, rs, ep)


def _scorer(metric, d, dtype="f16"):
    from nann_amd import ops
    key = ("scorer", metric, d, dtype)
    if key not in _CACHE:
        _CACHE[key] = ops.Scorer(metric, d, torch.float16 if dtype == "f16" else torch.bfloat16)
    return _CACHE[key]


def _case(n, d, dtype, metric):
    """made once per (shape, metric): the rows and queries of sq8_range_model.gpu_case, the device index, table and bounds, the
    model's terms and approximate scores, the device's exact score of every (query, row) -- search_all_range at -inf -- and the
    cycled thresholds taken from those bits"""
    key = (n, d, dtype)
    if key not in _CACHE:
        from nann_amd import retrieval
        x, q = RG.gpu_case(n, d, dtype)
        dix = _index(x)
        t = retrieval.make_sq8(dix)
        xe, qe = M.encode(x), M.encode(q)
        _CACHE[key] = (x, q, dix, t, retrieval.make_sq8_bounds(dix, t), xe, qe, X.row_terms(x, xe), X.row_terms(q, qe))
    x, q, dix, t, b, xe, qe, xt, qt = _CACHE[key]
    key = (n, d, dtype, metric)
    if key not in _CACHE:
        from nann_amd import retrieval
        sc = _scorer(metric, d, dtype)
        r = retrieval.search_all_range(dix, sc, cuda(q), float("-inf"))
        torch.cuda.synchronize()
        assert r.total == n * len(q)                                      # every score is finite: row order, query by query
        exact = r.scores.cpu().numpy().reshape(len(q), n)
        thr = RG.case_thresholds(exact, metric)                           # query 4: a tie of rows 11, 400, n - 2; L2: +0 and -0
        _CACHE[key] = (sc, M.approx_scores(qe, xe, metric), exact, thr)
    return (x, q, dix, t, b, xt, qt) + _CACHE[key]


def _np(r):
    torch.cuda.synchronize()
    return (r.row_splits.cpu().numpy(), r.index.cpu().numpy(), r.scores.cpu().numpy(), r.item_ids.cpu().numpy())


def _ref(dix, sc, q, thr):
    from nann_amd import retrieval
    return _np(retrieval.search_all_range(dix, sc, cuda(q), cuda(np.asarray(thr, F))))


def _got(dix, t, b, sc, q, thr, cap=RG.GPU_CAP, fallback=False, **kw):
    from nann_amd import retrieval
    r = retrieval.search_all_range_sq8_exact(dix, t, b, sc, cuda(q), cuda(np.asarray(thr, F)), cap=cap, fallback=fallback, **kw)
    return _np(r), r.certified.cpu().numpy(), r.n_survivors.cpu().numpy(), r


def _same_segments(got, ref, which, what=""):
    """the segments of the queries `which` hold the same rows, score bits and item ids"""
    g, e = RG.segments(got), RG.segments(ref)
    for i in which:
        for a, o, name in zip(g[i], e[i], ("index", "score bits", "item_ids")):
            assert a.shape == o.shape and (a == o).all(), (what, i, name)


def _same_result(got, ref, what=""):
    total = int(ref[0][-1])
    assert (got[0] == ref[0]).all(), (what, "row_splits")
    assert (got[1][:total] == ref[1][:total]).all() and (got[3][:total] == ref[3][:total]).all(), what
    assert (bits(got[2][:total]) == bits(ref[2][:total])).all(), what


def _status(fn):
    from nann_amd import ops
    try:
        fn()
    except ops.NannError as e:
        return e.status
    return 0


# ---- 1. results and counters -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("n,d,dtype", RG.GPU_SHAPES)
def test_equals_search_all_range_bit_for_bit(n, d, dtype, metric):
    x, q, dix, t, b, xt, qt, sc, approx, exact, thr = _case(n, d, dtype, metric)
    model = RG.survivors(approx, xt, qt, thr, metric, d, RG.GPU_CAP)
    ref = _ref(dix, sc, q, thr)
    got, cert, n_surv, r = _got(dix, t, b, sc, q, thr)
    matches = np.diff(ref[0])
    by_approx = sum(int((RG.RM.match(approx[i], thr[i]) != RG.RM.match(exact[i], thr[i])).any()) for i in range(len(q)))
    print("n=%d d=%d %s %s: survivors mean %.1f max %d, matches mean %.1f max %d; thresholding the approximate score is wrong for %d "
          "of %d queries" % (n, d, dtype, metric, n_surv.mean(), n_surv.max(), matches.mean(), matches.max(), by_approx, len(q)))
    assert by_approx > 0, "thresholding the approximate score is already exact here: the case shows nothing"
    assert (n_surv == model.n_survivors).all()
    assert (cert == model.certified).all()
    assert model.certified.all(), "the cap of these cases holds every query (test_sq8_range_cpu.py)"
    assert matches[4] >= 3 and {11, 400, n - 2} <= set(RG.segments(ref)[4][0].tolist())       # the tie is in the reference ...
    _same_result(got, ref)                                                                      # ... and in the result
    assert r.total == int(ref[0][-1]) and not r.truncated
    assert (got[1][r.total:] == 0).all()                                  # behind the total the wrapper's zeros stand


# ---- 2. a cap below a query's survivor count ----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_overflow_is_uncertified_and_empty_and_the_fallback_repairs_it(metric):
    n, d, dtype = 2051, 128, "f16"
    x, q, dix, t, b, xt, qt, sc, approx, exact, thr = _case(n, d, dtype, metric)
    model = RG.survivors(approx, xt, qt, thr, metric, d, RG.GPU_SMALL_CAP)
    assert model.certified.any() and not model.certified.all()
    ref = _ref(dix, sc, q, thr)
    got, cert, n_surv, r = _got(dix, t, b, sc, q, thr, cap=RG.GPU_SMALL_CAP)
    assert (n_surv == model.n_survivors).all() and (cert == model.certified).all()
    assert (n_surv[cert == 0] > RG.GPU_SMALL_CAP).all()                   # the true count, beyond the cap
    lens = np.diff(got[0])
    assert (lens[cert == 0] == 0).all()                                   # an uncertified segment is empty
    _same_segments(got, ref, np.flatnonzero(cert))                        # the neighbours are search_all_range's
    assert r.capacity == len(q) * RG.GPU_SMALL_CAP and not r.truncated
    full, cert2, n_surv2, r2 = _got(dix, t, b, sc, q, thr, cap=RG.GPU_SMALL_CAP, fallback=True)
    assert (cert2 == cert).all() and (n_surv2 == n_surv).all()            # as the device call left them
    _same_result(full, ref, "fallback")
    assert r2.total == int(ref[0][-1]) and not r2.truncated and len(full[1]) == r2.total
    # a caller's capacity below the total: the head of the whole result, as search_all_range truncates
    room = r2.total - 5
    head, _, _, r3 = _got(dix, t, b, sc, q, thr, cap=RG.GPU_SMALL_CAP, fallback=True, capacity=room)
    assert r3.truncated and r3.total == r2.total and len(head[1]) == room and (head[0] == ref[0]).all()
    assert (head[1] == ref[1][:room]).all() and (bits(head[2]) == bits(ref[2][:room])).all() and (head[3] == ref[3][:room]).all()
    # sort=True orders a segment as search_all_range's sort does
    from nann_amd import retrieval
    want = _np(retrieval.search_all_range(dix, sc, cuda(q), cuda(thr), sort=True))
    have, *_ = _got(dix, t, b, sc, q, thr, cap=RG.GPU_SMALL_CAP, fallback=True, sort=True)
    _same_result(have, want, "sorted")


# ---- 3. thresholds ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_thresholds_that_are_not_finite_and_positive_ones(metric):
    n, d, dtype = 1007, 64, "f16"
    x, q, dix, t, b, xt, qt, sc, approx, exact, _ = _case(n, d, dtype, metric)
    q8 = q[:8]
    thr = np.array([np.nan, -np.inf, np.inf, 1.5, exact[4].max(), F(1e-30), np.sort(exact[6])[-20], np.nan], F)
    model = RG.survivors(approx[:8], xt, (qt[0][:8], qt[1][:8]), thr, metric, d, RG.GPU_CAP)
    ref = _ref(dix, sc, q8, thr)
    got, cert, n_surv, _ = _got(dix, t, b, sc, q8, thr)
    assert (cert == model.certified).all() and (n_surv == model.n_survivors).all()
    assert cert[[0, 1, 2, 7]].tolist() == [0, 0, 0, 0]                    # NaN, -inf, +inf: never certified
    assert (np.diff(got[0])[[0, 1, 2, 7]] == 0).all()
    assert cert[4] == 1 and cert[6] == 1
    if metric == "l2":
        assert cert[[3, 5]].tolist() == [1, 1] and n_surv[[3, 5]].tolist() == [0, 0]     # above +0: certified, nothing survives
        assert (np.diff(ref[0])[[3, 5]] == 0).all()                                        # and search_all_range agrees
    _same_segments(got, ref, np.flatnonzero(cert))
    assert np.diff(got[0])[6] == 20
    full, *_ = _got(dix, t, b, sc, q8, thr, fallback=True)
    _same_result(full, ref, "fallback")                                   # -inf: every row, through search_all_range


# ---- 4. outputs ---------------------------------------------------------------------------------------------------------------
class _Out:
    """sentinel-filled outputs with G guard words on both sides of each"""
    G = 64

    def __init__(self, nq, room):
        mk = lambda m, dt: torch.full((m + 2 * self.G,), S, dtype=dt, device="cuda")  # noqa: E731
        self.nq, self.room = nq, room
        self.splits, self.ids, self.scores, self.index = mk(nq + 1, torch.int64), mk(room, torch.int64), mk(room, torch.float32), mk(room, torch.int32)
        self.cert, self.surv = mk(nq, torch.int32), mk(nq, torch.int32)

    def ptr(self, t):
        return t.data_ptr() + self.G * t.element_size()

    def guards_hold(self):
        for t, m in ((self.splits, self.nq + 1), (self.ids, self.room), (self.scores, self.room), (self.index, self.room),
                     (self.cert, self.nq), (self.surv, self.nq)):
            if not (bool((t[:self.G] == S).all()) and bool((t[self.G + m:] == S).all())):
                return False
        return True

    def body(self, t, m):
        return t[self.G:self.G + m].cpu().numpy()


def _raw(dix, t, b, sc, qd, thr_d, cap, capacity, out, ws, nbytes, null_entries=False, n=None, cert=True, surv=True):
    from nann_amd import _lib
    from nann_amd.ops import _ptr, _stream
    entries = (None, None, None) if null_entries else (out.ptr(out.ids), out.ptr(out.scores), out.ptr(out.index))
    st = _lib.lib().nann_search_all_range_sq8_exact(
        dix.handle, t.handle if t is not None else None, b.handle if b is not None else None, sc.handle, _ptr(qd),
        qd.shape[0] if n is None else n, _ptr(thr_d), cap, capacity, out.ptr(out.splits), *entries,
        out.ptr(out.cert) if cert else None, out.ptr(out.surv) if surv else None, _ptr(ws), nbytes, None, _stream())
    torch.cuda.synchronize()
    return st


def _workspace(dix, t, b, sc, nq, cap):
    from nann_amd import _lib
    nb = C.c_int64(-1)
    assert _lib.lib().nann_search_all_range_sq8_exact_workspace_bytes(dix.handle, t.handle, b.handle, sc.handle, nq, cap, C.byref(nb)) == OK
    assert nb.value % 256 == 0 and nb.value > 0
    return torch.full((nb.value + 4096,), 0xA5, dtype=torch.uint8, device="cuda"), nb.value


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_count_only_truncation_and_guard_words(metric):
    n, d, dtype = 2051, 64, "f16"
    x, q, dix, t, b, xt, qt, sc, approx, exact, thr = _case(n, d, dtype, metric)
    ref = _ref(dix, sc, q, thr)
    total = int(ref[0][-1])
    qd, thr_d = cuda(q), cuda(thr)
    ws, nbytes = _workspace(dix, t, b, sc, len(q), RG.GPU_CAP)
    # count-only: capacity 0, NULL entry outputs
    out = _Out(len(q), 16)
    assert _raw(dix, t, b, sc, qd, thr_d, RG.GPU_CAP, 0, out, ws, nbytes, null_entries=True) == OK
    assert (out.body(out.splits, len(q) + 1) == ref[0]).all() and (out.body(out.cert, len(q)) == 1).all()
    assert (out.body(out.ids, 16) == S).all() and out.guards_hold()
    # a capacity in the middle of a segment of the second chunk's neighbourhood, one in the first chunk, and one beyond the total
    for capacity in (total - 7, int(ref[0][60]) + 3, total + 50):
        out = _Out(len(q), capacity)
        assert _raw(dix, t, b, sc, qd, thr_d, RG.GPU_CAP, capacity, out, ws, nbytes) == OK
        assert out.guards_hold(), capacity
        m = min(total, capacity)
        assert (out.body(out.splits, len(q) + 1) == ref[0]).all()                          # the true totals, whatever the capacity
        assert (out.body(out.index, capacity)[:m] == ref[1][:m]).all() and (out.body(out.ids, capacity)[:m] == ref[3][:m]).all()
        assert (bits(out.body(out.scores, capacity)[:m]) == bits(ref[2][:m])).all()
        for buf in (out.index, out.ids, out.scores):
            assert (out.body(buf, capacity)[m:] == S).all(), capacity                      # [min(total, capacity), capacity) untouched
    assert bool((ws[nbytes:] == 0xA5).all()), "the call wrote behind its workspace"


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_a_segment_does_not_depend_on_the_batch(metric):
    n, d, dtype = 2051, 128, "f16"
    x, q, dix, t, b, xt, qt, sc, approx, exact, thr = _case(n, d, dtype, metric)
    batch, cert, n_surv, _ = _got(dix, t, b, sc, q, thr)
    segs = RG.segments(batch)
    for i in (77, 129):
        alone, c1, s1, _ = _got(dix, t, b, sc, q[i:i + 1], thr[i:i + 1])
        assert c1[0] == cert[i] and s1[0] == n_surv[i]
        for a, o in zip(RG.segments(alone)[0], segs[i]):
            assert a.shape == o.shape and (a == o).all(), i


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------
def test_failure_codes():
    from nann_amd import _lib, ops, retrieval, synth
    n, d = 1007, 64
    x, q, dix, t, b, xt, qt, sc, approx, exact, thr = _case(n, d, "f16", "l2")
    x2, _, dix2, t2, b2 = _case(2051, 64, "f16", "l2")[:5]
    qd, thr_d = cuda(q[:4]), cuda(thr[:4])
    run = lambda **kw: retrieval.search_all_range_sq8_exact(kw.pop("ix", dix), kw.pop("t", t), kw.pop("b", b), kw.pop("sc", sc), qd,  # noqa: E731
                                                            thr_d, fallback=False, **kw)
    assert _status(lambda: run(t=None)) == BAD and _status(lambda: run(b=None)) == BAD          # a NULL table, NULL bounds
    assert _status(lambda: run(t=t2)) == BAD                                                    # a table of another index
    assert b"another index" in _lib.lib().nann_last_error()
    assert _status(lambda: run(b=b2)) == BAD                                                    # bounds of another index
    assert b"another index or code table" in _lib.lib().nann_last_error()
    t_again = retrieval.make_sq8(dix)                                                           # the same index, another table
    assert _status(lambda: run(t=t_again)) == BAD
    assert _status(lambda: run(cap=0)) == BAD and _status(lambda: run(cap=-3)) == BAD           # cap < 1
    assert _status(lambda: run(cap=2 ** 31)) == UNSUPPORTED                                     # beyond the longest candidate list
    assert b"longest list" in _lib.lib().nann_last_error()
    mlp = ops.Scorer("mlp", 64, torch.float16, synth.make_mlp_weights(64), precision="exact")
    assert _status(lambda: run(sc=mlp)) == UNSUPPORTED                                          # an MLP scorer
    f32 = _index(M.widen(x).astype(np.float32))
    assert _status(lambda: run(ix=f32, sc=ops.Scorer("l2", 64, torch.float32))) == UNSUPPORTED  # an index with f32 rows
    assert b"16-bit rows" in _lib.lib().nann_last_error()
    assert _status(lambda: run()) == 0 and _status(lambda: run(cap=n + 5)) == 0                 # a cap above n_items counts as n_items
    L = _lib.lib()
    size = lambda nq, cap, out: L.nann_search_all_range_sq8_exact_workspace_bytes(dix.handle, t.handle, b.handle, sc.handle, nq, cap, C.byref(out))  # noqa: E731
    nb, nb_big, nb0 = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    assert size(128, 512, nb) == OK and size(4096, 512, nb_big) == OK and nb.value == nb_big.value   # bounded by the chunk
    assert size(0, 512, nb0) == OK and nb0.value == 0 and size(-1, 512, nb0) == BAD
    ws, nbytes = _workspace(dix, t, b, sc, 4, 512)
    out = _Out(4, 64)
    assert _raw(dix, t, b, sc, qd, thr_d, 512, 64, out, ws, nbytes - 1) == CAPACITY             # a short workspace
    assert _raw(dix, t, b, sc, qd, thr_d, 512, -1, out, ws, nbytes) == BAD                      # capacity < 0
    assert _raw(dix, t, b, sc, qd, thr_d, 512, 64, out, ws, nbytes, null_entries=True) == BAD   # capacity > 0 without entry outputs
    assert _raw(dix, t, b, sc, qd, thr_d, 512, 64, out, ws, nbytes, cert=False) == BAD          # a NULL out_certified
    assert _raw(dix, t, b, sc, qd, thr_d, 512, 64, out, ws, nbytes, surv=False) == BAD          # a NULL out_n_survivors
    assert _raw(dix, t, b, sc, qd, thr_d, 512, 64, out, ws, nbytes, n=0, cert=False, surv=False) == OK   # nothing to do
    for buf, m in ((out.splits, 5), (out.ids, 64), (out.scores, 64), (out.index, 64), (out.cert, 4), (out.surv, 4)):
        assert (out.body(buf, m) == S).all()                                                    # every refusal wrote nothing
    assert out.guards_hold() and bool((ws == 0xA5).all())
    assert _raw(dix, t, b, sc, qd, thr_d, 512, 64, out, ws, nbytes) == OK and (out.body(out.cert, 4) == 1).all()
    assert out.guards_hold() and bool((ws[nbytes:] == 0xA5).all())
