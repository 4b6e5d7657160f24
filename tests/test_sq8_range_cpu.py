"""CPU: the certified scalar-quantised range search (nann_search_all_range_sq8_exact) as far as it can be held without a GPU --
the two symbols, the build's rule for the new kernels and the refusals in front of any device call; and the numpy model of the
contract (sq8_range_model): the soundness of the survivor predicate at a caller's threshold against float64 and against an f32
left-to-right accumulation, the model against range_model for every certified query, an input on which thresholding the
approximate score gives another answer, and the cases of test_sq8_range_gpu.py against their cap.  No tolerance appears
anywhere: every comparison is an inequality the proof of DESIGN.md 4.21 / 4.22 states, or an equality."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import range_model as RM
import sq8_exact_model as X
import sq8_model as M
import sq8_range_model as RG
from nann_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nann_search_all_range_sq8_exact_workspace_bytes", "nann_search_all_range_sq8_exact")
OK, BAD_ARGUMENT = 0, 7
F = np.float32
_CACHE = {}


# ---- the ABI and the build ------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "nann_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = C.CDLL(build.build())
    bound = _lib.lib()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % s, code), s
        assert hasattr(lib, s), s
        assert s in _lib.SYMBOLS, s
        assert getattr(bound, s).argtypes, s
    assert "#define NANN_ABI_VERSION 6" in header and bound.nann_abi_version() == 6
    decl = code[code.index("int nann_search_all_range_sq8_exact("):]
    decl = decl[:decl.index(";")]
    assert "nann_filter" not in decl                                    # there is no filter argument, and the header says why
    doc = header[header.index("certified scalar-quantised RANGE search"):header.index("int nann_search_all_range_sq8_exact_workspace_bytes")]
    assert "NO filter argument" in doc and "threshold above +0" in doc and "0.0f - (a sum of squares)" in doc


def test_refusals_without_a_device():
    from nann_amd import ops
    L = _lib.lib()
    nb = C.c_int64(-1)
    size, call = L.nann_search_all_range_sq8_exact_workspace_bytes, L.nann_search_all_range_sq8_exact
    assert size(None, None, None, None, 4, 4096, C.byref(nb)) == BAD_ARGUMENT and b"null" in L.nann_last_error()
    assert size(None, None, None, None, 4, 4096, None) == BAD_ARGUMENT
    sc = ops.Scorer("l2", 64)                                            # a scorer needs no device; an index does
    assert size(None, None, None, sc.handle, 4, 4096, C.byref(nb)) == BAD_ARGUMENT
    assert size(None, None, None, sc.handle, 0, 4096, C.byref(nb)) == BAD_ARGUMENT     # n_queries == 0 excuses no handle
    assert nb.value == -1
    tail = (None, None, None, None, None, None, None, 0, None, None)
    assert call(None, None, None, None, None, 4, None, 4096, 0, *tail) == BAD_ARGUMENT
    assert call(None, None, None, sc.handle, None, 4, None, 4096, 0, *tail) == BAD_ARGUMENT
    assert call(None, None, None, sc.handle, None, 0, None, 0, -1, *tail) == BAD_ARGUMENT


def test_the_kernels_ride_in_the_scan_object_and_may_have_no_scratch(tmp_path):
    assert len(build.UNITS) == 17
    src = open(os.path.join(build.SRC_DIR, "nann_sq8.h")).read()
    for kern in ("k_sq8_range_lists", "k_sq8_range_count", "k_sq8_range_fill"):
        assert re.search(r"void %s\(" % kern, src), kern
    part = src[src.index("// ---- the certified range form ----"):]
    assert not re.search(r"atomic\w*\(", part)                           # a match's place is decided by no atomic
    inst = open(os.path.join(build.SRC_DIR, "nann_sq8_inst.hip")).read()
    part = inst[inst.index("// ---- the certified range form ----"):]
    for reused in ("k_sq8_exact_terms<METRIC>", "k_sq8_surv_count<METRIC>", "k_range_scan", "k_sq8_surv_fill<METRIC>", "k_range_splits"):
        assert reused in part, reused
    assert "k_scan_slab_topk" not in part and "k_cand_topk" not in part  # no top-k anywhere in the chain
    report = ("remark: unit.hip:1:1: Function Name: _ZN4nann%d%sEPKfPKxPKiS1_xS5_PKlxS7_xPlPfPi [-Rpass-analysis=kernel-resource-usage]\n"
              "remark: unit.hip:1:1:     ScratchSize [bytes/lane]: %d [-Rpass-analysis=kernel-resource-usage]\n")
    for kern in ("k_sq8_range_lists", "k_sq8_range_count", "k_sq8_range_fill"):
        good, bad = str(tmp_path / "good.log"), str(tmp_path / "bad.log")
        open(good, "w").write(report % (len(kern), kern, 0))
        open(bad, "w").write(report % (len(kern), kern, 16))
        build.check_resources(good)
        with pytest.raises(RuntimeError, match=kern + ".*16 bytes of scratch.*certified range selection"):
            build.check_resources(bad)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
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


def _case(n, d, dtype, metric):
    """the rows and queries of test_sq8_range_gpu.py's case, their codes and terms, approximate and float64 scores"""
    key = (n, d, dtype, metric)
    if key not in _CACHE:
        x, q = RG.gpu_case(n, d, dtype)
        xe, qe = M.encode(x), M.encode(q)
        _CACHE.clear()
        _CACHE[key] = (x, q, X.row_terms(x, xe), X.row_terms(q, qe), M.approx_scores(qe, xe, metric), RG.exact_f64_all(q, x, metric))
    return _CACHE[key]


# ---- soundness: the lemma of 4.21 asks nothing of tau but finiteness -----------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d", [64, 512])
def test_every_row_at_or_above_the_threshold_survives(d, dtype, metric):
    x, q, xt, qt, approx, e64 = _case(1007, d, dtype, metric)
    q, approx, e64, qt = q[:33], approx[:33], e64[:33], (qt[0][:33], qt[1][:33])
    e32 = _exact_f32_left_to_right(q, x, metric)
    differs = 0
    for pick in range(4):   # every query at the 1st, the 37th, the 300th score and between the 10th and the 11th
        thr = np.array([RG.threshold_of(e64[i], pick) for i in range(len(q))], F)
        r = RG.survivors(approx, xt, qt, thr, metric, d, 1007)
        assert r.certified.all()
        for e in (e64, e32):
            at_or_above = np.stack([RM.match(e[i], thr[i]) for i in range(len(q))])
            assert r.keep[at_or_above].all(), pick
            assert (e[~r.keep] < np.broadcast_to(thr[:, None], r.keep.shape)[~r.keep]).all(), pick   # a dropped row lies below
        by_approx = np.stack([RM.match(approx[i], thr[i]) for i in range(len(q))])
        by_exact = np.stack([RM.match(e64[i], thr[i]) for i in range(len(q))])
        differs += int((by_approx != by_exact).any(axis=1).sum())
    # a kernel that thresholds the approximate score returns another set on these inputs: the GPU comparison can fail
    assert differs > 0, "thresholding the approximate score is already exact here: the case shows nothing"


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_one_query_where_the_approximate_score_gives_another_answer(metric):
    x, q, xt, qt, approx, e64 = _case(1007, 64, "f16", metric)
    thr = RG.cycle_thresholds(e64)
    found = [i for i in range(len(q)) if (RM.match(approx[i], thr[i]) != RM.match(e64[i], thr[i])).any()]
    assert found, "no query separates {a >= t} from {S >= t}"
    i = found[0]
    r, res = RG.search_range(approx, e64, xt, qt, thr, metric, 64, RG.GPU_CAP, np.arange(1007, dtype=np.int64), 1007 * len(q))
    assert r.certified[i]
    got = RG.segments(res)[i][0]
    assert (got == np.flatnonzero(RM.match(e64[i], thr[i]))).all()       # the model returns the exact set ...
    assert not np.array_equal(got, np.flatnonzero(RM.match(approx[i], thr[i])))   # ... which the approximate score misses


# ---- the model against range_model, and the GPU cases against their cap --------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("n,d,dtype", RG.GPU_SHAPES)
def test_the_model_equals_range_search_and_the_gpu_cases_fit_their_cap(n, d, dtype, metric):
    x, q, xt, qt, approx, e64 = _case(n, d, dtype, metric)
    ids = np.arange(n, dtype=np.int64) * 7 + 3
    thr = RG.case_thresholds(e64, metric)
    room = n * len(q)
    r, res = RG.search_range(approx, e64, xt, qt, thr, metric, d, RG.GPU_CAP, ids, room)
    print("n=%d d=%d %s %s: most survivors %d at cap %d" % (n, d, dtype, metric, r.n_survivors.max(), RG.GPU_CAP))
    assert (r.n_survivors <= RG.GPU_CAP).all() and r.certified.all()      # what the GPU file relies on
    exp = RM.reference(e64, thr, ids, room)
    assert (res[0] == exp[0]).all()
    for got, want in zip(RG.segments(res), RG.segments(exp)):
        assert all((g == w).all() for g, w in zip(got, want))
    # the case meant to overflow: some queries certified, some not; an uncertified segment is empty, the others are unchanged
    r2, res2 = RG.search_range(approx, e64, xt, qt, thr, metric, d, RG.GPU_SMALL_CAP, ids, room)
    assert (r2.n_survivors == r.n_survivors).all()                        # the true count, whatever the cap
    assert (r2.certified == (r.n_survivors <= RG.GPU_SMALL_CAP)).all() and r2.certified.any() and not r2.certified.all()
    at_300 = [i for i in range(2, len(q), 4) if i not in (4, 8, 12)]
    assert (r2.n_survivors[at_300] > RG.GPU_SMALL_CAP).all()              # every threshold at the 300th score overflows
    assert (e64[4] >= thr[4]).sum() >= 3 and r.n_survivors[4] >= 3        # the tie of rows 11, 400 and n - 2
    for i, (got, want) in enumerate(zip(RG.segments(res2), RG.segments(exp))):
        if r2.certified[i]:
            assert all((g == w).all() for g, w in zip(got, want)), i
        else:
            assert len(got[0]) == 0, i


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_thresholds_that_are_not_finite_and_the_l2_rule_above_zero(metric):
    x, q, xt, qt, approx, e64 = _case(1007, 64, "f16", metric)
    n_q = 8
    thr = np.array([np.nan, -np.inf, np.inf, 1.5, 0.0, -0.0, np.float32(1e-30), e64[7].max()], F)
    r, res = RG.search_range(approx[:n_q], e64[:n_q], xt, (qt[0][:n_q], qt[1][:n_q]), thr, metric, 64, 1007,
                             np.arange(1007, dtype=np.int64), 1007 * n_q)
    assert not r.certified[:3].any()                                      # NaN, -inf, +inf: never certified, empty
    assert all(len(s[0]) == 0 for s in RG.segments(res)[:3])
    if metric == "l2":
        assert r.above.tolist() == [False, False, False, True, False, False, True, False]
        assert r.certified[3] and r.certified[6] and r.n_survivors[3] == 0 and r.n_survivors[6] == 0
        assert len(RG.segments(res)[3][0]) == 0 and len(RG.segments(res)[6][0]) == 0
        assert r.certified[4] and r.certified[5]                          # +0 and -0 take the normal path
    else:
        assert not r.above.any() and r.certified[3:].all()
    exp = RM.reference(e64[:n_q], thr, np.arange(1007, dtype=np.int64), 1007 * n_q)
    for i, (got, want) in enumerate(zip(RG.segments(res), RG.segments(exp))):
        if r.certified[i]:
            assert all((g == w).all() for g, w in zip(got, want)), i
