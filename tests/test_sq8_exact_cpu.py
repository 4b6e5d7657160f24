"""CPU: the certified scalar-quantised search (nann_sq8_bounds / nann_search_all_sq8_exact) as far as it can be held without a
GPU -- the six symbols and the build lists, the refusals in front of any device call, and the numpy model of the contract
(sq8_exact_model): the soundness of the bound against float64 and against an f32 left-to-right accumulation, the survivor set
against the exhaustive top k, the three-stage call against a plain exhaustive top k, the cap, and the adversarial cases.  No
tolerance appears anywhere: every comparison is an inequality the proof of DESIGN.md 4.21 states, or an equality."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sq8_exact_model as X
import sq8_model as M
from nann_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nann_sq8_bounds_create", "nann_sq8_bounds_destroy", "nann_sq8_bounds_view", "nann_search_all_sq8_exact_workspace_bytes",
           "nann_search_all_sq8_exact_layout", "nann_search_all_sq8_exact")
OK, BAD_ARGUMENT = 0, 7
F = np.float32
CAP = 2048
_CACHE = {}


def _header():
    return open(os.path.join(ROOT, "include", "nann_hip.h")).read()


# ---- the ABI and the build ------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_bound():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = C.CDLL(build.build())
    bound = _lib.lib()
    for s in SYMBOLS:
        assert re.search(r"\b(int|void) %s\s*\(" % s, code), s
        assert hasattr(lib, s), s
        assert s in _lib.SYMBOLS, s
        assert getattr(bound, s).argtypes, s
    assert re.search(r"typedef struct nann_sq8_bounds nann_sq8_bounds;", code)
    assert bound.nann_sq8_bounds_destroy.restype is None
    assert "#define NANN_ABI_VERSION 6" in _header() and bound.nann_abi_version() == 6


def test_the_kernels_ride_in_the_scan_object():
    assert len(build.UNITS) == 17
    src = open(os.path.join(build.SRC_DIR, "nann_sq8.h")).read()
    for kern in ("k_sq8_row_err", "k_sq8_exact_terms", "k_sq8_surv_count", "k_sq8_exact_lists", "k_sq8_surv_fill"):
        assert re.search(r"void %s\(" % kern, src), kern
    inst = open(os.path.join(build.SRC_DIR, "nann_sq8_inst.hip")).read()
    assert "k_range_scan" in inst and "k_sq8_surv_fill<METRIC>" in inst
    assert not re.search(r"atomic\w*\(", src[src.index("the certified form ----"):])   # ascending row order, no atomic call
    report = ("remark: unit.hip:1:1: Function Name: _ZN4nann16k_sq8_surv_countILi0EEEvPKfxS2_S2_PKNS_9Sq8QTermsEfPi [-Rpass-analysis=kernel-resource-usage]\n"
              "remark: unit.hip:1:1:     ScratchSize [bytes/lane]: %d [-Rpass-analysis=kernel-resource-usage]\n")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        good, bad = os.path.join(tmp, "good.log"), os.path.join(tmp, "bad.log")
        open(good, "w").write(report % 0)
        open(bad, "w").write(report % 24)
        build.check_resources(good)
        with pytest.raises(RuntimeError, match="k_sq8_surv_count.*24 bytes of scratch.*survivor pass"):
            build.check_resources(bad)


def test_refusals_without_a_device():
    L = _lib.lib()
    out = C.c_void_p(0)
    assert L.nann_sq8_bounds_create(None, None, None, C.byref(out)) == BAD_ARGUMENT and b"null" in L.nann_last_error()
    L.nann_sq8_bounds_destroy(None)  # a no-op
    p = C.c_void_p(0)
    assert L.nann_sq8_bounds_view(None, C.byref(p), None) == BAD_ARGUMENT
    nb = C.c_int64(-1)
    assert L.nann_search_all_sq8_exact_workspace_bytes(None, None, None, None, 4, 8, 2048, 4, C.byref(nb)) == BAD_ARGUMENT
    assert L.nann_search_all_sq8_exact_workspace_bytes(None, None, None, None, 4, 8, 2048, 4, None) == BAD_ARGUMENT
    assert L.nann_search_all_sq8_exact(None, None, None, None, None, 4, 8, 2048, 4, None, None, None, None, None, None, 0, None,
                                       None) == BAD_ARGUMENT
    assert nb.value == -1


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _rows(n, d, seed, dtype="f16"):
    """test_sq8_gpu.py's generator, restated: Gaussian rows, every row at a magnitude of its own (e^-2 .. e^2)"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, d)) * np.exp(rng.uniform(-2.0, 2.0, (n, 1)))).astype(F)
    if dtype == "f16":
        return x.astype(np.float16)
    return (x.view(np.uint32) >> 16).astype(np.uint16)


def _queries(d, n_q=33, seed=0):
    q = np.random.default_rng(seed + d).standard_normal((n_q, d)).astype(F)
    q[5] *= F(0.01)
    return q


def _exact_f32_left_to_right(q, x, metric):
    """[n_q, n] f32: the exact score accumulated in float32 from element 0 upwards, one rounding per product and per sum"""
    xf = M.widen(x)
    acc = np.zeros((q.shape[0], xf.shape[0]), F)
    for j in range(xf.shape[1]):
        if metric == "ip":
            acc = acc + q[:, j, None] * xf[None, :, j]
        else:
            t = q[:, j, None] - xf[None, :, j]
            acc = acc + t * t
    return acc if metric == "ip" else -acc


def _exact_f64_all(q, x, metric):
    """[n_q, n] f32: sq8_model.exact_f64's score for every row"""
    of = M.exact_f64(q, x, metric)
    rows = np.arange(x.shape[0])
    return np.stack([of(i, rows) for i in range(q.shape[0])])


def _case(n, d, dtype, metric):
    key = (n, d, dtype, metric)
    if key not in _CACHE:
        x = _rows(n, d, n + d, dtype)
        q = _queries(d)
        enc = M.encode(x)
        terms = X.row_terms(x, enc)
        q_enc = M.encode(q)
        approx = M.approx_scores(q_enc, enc, metric)
        e64 = _exact_f64_all(q, x, metric)
        _CACHE.clear()   # (one case at a time: the arrays of n = 16417, d = 512 are large)
        _CACHE[key] = (x, q, enc, terms, q_enc, approx, e64)
    return _CACHE[key]


GRID = [(n, d, dtype, metric) for n in (1007, 16417) for d in (64, 128, 512) for dtype in ("f16", "bf16") for metric in ("l2", "ip")]


# ---- the error terms ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d", [64, 128, 512])
def test_err_and_xhat_bound_the_real_values_from_above(d, dtype):
    x = _rows(1007, d, d, dtype)
    x[3] = 0
    enc = M.encode(x)
    err, xhat = X.row_terms(x, enc)
    r_err, r_xhat = X.real_terms(x, enc)
    assert (err.astype(np.float64) >= r_err).all() and (xhat.astype(np.float64) >= r_xhat).all()
    live = np.arange(1007) != 3
    assert (err[live] <= r_err[live] * (1 + 2.0 ** -10)).all() and (xhat[live] <= r_xhat[live] * (1 + 2.0 ** -10)).all()
    assert xhat[3] == X.ABS and X.ABS <= err[3] <= F(2) * X.ABS       # the zero row: the absolute terms alone
    q = _queries(d)
    qe = M.encode(q)
    eq, qhat = X.row_terms(q, qe)
    r_eq, r_qhat = X.real_terms(q, qe)
    assert (eq >= r_eq).all() and (qhat >= r_qhat).all()


# ---- soundness ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,dtype,metric", GRID)
def test_the_bound_is_sound_and_the_call_is_exact(n, d, dtype, metric):
    x, q, enc, (err, xhat), q_enc, approx, e64 = _case(n, d, dtype, metric)
    eq, qhat = X.row_terms(q, q_enc)
    # the upper bound holds for every (query, row), against both restatements of the exact f32 score
    ub = X.upper_bound(approx, err, xhat, eq, qhat, metric, d)
    e32 = _exact_f32_left_to_right(q, x, metric)
    assert (ub >= e64).all()
    assert (ub >= e32).all()
    of = lambda qi, rows: e64[qi, rows]  # noqa: E731
    rows_all = np.arange(n, dtype=np.int32)
    worst = 0
    for k in (10, 200):
        r = X.search_exact(q, x, metric, k, CAP, k, of, x_enc=enc, x_terms=(err, xhat))
        w, ok = X.query_terms(r.tau, eq, qhat, metric, d)
        keep = X.survives(approx, err, xhat, r.tau, eq, qhat, w, metric, d)
        assert ok.all()
        # a row the predicate drops lies below the cut under the bound, and under both exact scores
        assert (ub[~keep] < np.broadcast_to(r.tau[:, None], keep.shape)[~keep]).all()
        for e in (e64, e32):
            assert (e[~keep] < np.broadcast_to(r.tau[:, None], keep.shape)[~keep]).all()
        # the survivors hold the exhaustive top k -- under either exact score -- and the call returns it
        for i in range(len(q)):
            for e in (e64, e32):
                top, _ = M.topk(e[i], k)
                assert keep[i, top].all(), (k, i)
            er, es = M.topk(e64[i], k, rows_all)
            assert (r.rows[i] == er).all() and (r.scores[i].view(np.uint32) == es.view(np.uint32)).all(), (k, i)
        # the cap is honest: every query certified
        assert r.certified.all() and (r.n_survivors >= k).all()
        worst = max(worst, int(r.n_survivors.max()))
    print("n=%d d=%d %s %s: most survivors %d" % (n, d, dtype, metric, worst))
    assert worst <= CAP


# ---- adversarial cases -------------------------------------------------------------------------------------------------------
def _check(q, x, metric, fetch, cap, k):
    """every query certified and equal to the exhaustive top k, or overflowing and equal to the plain two-stage call"""
    e64 = _exact_f64_all(q, x, metric)
    of = lambda qi, rows: e64[qi, rows]  # noqa: E731
    r = X.search_exact(q, x, metric, fetch, cap, k, of)
    plain = M.search(q, x, metric, fetch, k, of)
    rows_all = np.arange(x.shape[0], dtype=np.int32)
    for i in range(len(q)):
        if r.certified[i]:
            er, es = M.topk(e64[i], k, rows_all)
            assert (r.rows[i] == er).all() and (r.scores[i].view(np.uint32) == es.view(np.uint32)).all(), i
            assert r.n_survivors[i] <= cap and len(r.lists[i]) == r.n_survivors[i]
        else:
            assert r.n_survivors[i] > min(cap, x.shape[0]) or not np.isfinite(r.tau[i]), i
            assert (r.rows[i] == plain[0][i]).all() and (r.scores[i].view(np.uint32) == plain[1][i].view(np.uint32)).all(), i
    return r, e64


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_duplicate_rows_that_straddle_rank_k(metric):
    rng = np.random.default_rng(3)
    x = _rows(700, 64, 11)
    copies = [9, 120, 121, 400, 655]
    x[copies] = x[300]
    q = (x[300].astype(F) * F(1.25) + rng.standard_normal(64).astype(F) * F(0.01))[None, :]
    e64 = _exact_f64_all(q, x, metric)
    order, _ = M.topk(e64[0], 700)
    first = int(np.flatnonzero(np.isin(order, copies + [300]))[0])
    k = first + 3                                   # three of the six equal rows inside the top k, three behind it
    r, _ = _check(q, x, metric, k, CAP, k)
    assert r.certified[0]
    assert set(copies + [300]) <= set(r.lists[0].tolist())            # ties at tau survive
    assert r.rows[0, first:first + 3].tolist() == sorted(copies + [300])[:3]


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_zero_rows_zero_queries_small_queries_and_lossless_rows(metric):
    rng = np.random.default_rng(4)
    x = _rows(900, 64, 12)
    x[17] = 0
    c = rng.integers(-127, 128, (40, 64)).astype(np.int32)            # rows whose quantisation error is zero
    c[np.arange(40), rng.integers(0, 64, 40)] = 127
    x[100:140] = (c.astype(F) / F(128.0)).astype(np.float16)
    enc = M.encode(x)
    err, xhat = X.row_terms(x, enc)
    r_err, _ = X.real_terms(x, enc)
    assert (r_err[100:140] == 0).all() and (err[100:140] > 0).all()
    q = _queries(64, 9, seed=2)
    q[1] = 0
    q[2] = x[17].astype(F)
    q[3] = x[110].astype(F)
    for k, fetch in ((10, 10), (1, 1), (1, 7), (200, 200)):
        r, _ = _check(q, x, metric, fetch, CAP, k)
        assert r.certified.all()
    r, _ = _check(q, x, metric, 30, 40, 30)                            # a cap that some queries overflow and some do not
    assert not r.certified.all() and r.certified.any()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_k_equals_fetch_equals_n_items(metric):
    x = _rows(257, 64, 13)
    q = _queries(64, 6, seed=3)
    r, _ = _check(q, x, metric, 257, CAP, 257)
    assert r.certified.all() and (r.n_survivors == 257).all()
    r, _ = _check(q, x, metric, 257, 257, 257)
    assert r.certified.all()


def test_a_nan_query_is_never_certified():
    x = _rows(500, 64, 14)
    q = _queries(64, 6, seed=4)[:4]
    q[2, 7] = np.nan
    for metric in ("l2", "ip"):
        e64 = _exact_f64_all(q, x, metric)
        of = lambda qi, rows: e64[qi, rows]  # noqa: E731
        with np.errstate(invalid="ignore"):
            r = X.search_exact(q, x, metric, 20, CAP, 10, of)
        assert r.certified.tolist() == [True, True, False, True]
