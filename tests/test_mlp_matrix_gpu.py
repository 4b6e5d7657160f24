"""-m gpu: every compiled kernel of the MLP scorer against references that are not the device.

The MLP scorer compiles to the 61 kernels of KERNELS below (nann_mlp_inst.hip once per d, nann_mlp_res_inst.hip): the
traversal that reads the embedding rows, per (d, row dtype), exact f32 and split-f16 on both bitmap plans and split-f16 on
the 16K-slot hash set; the traversal on the pre-projected table with layer 2 resident (one instance per precision and
plan, every d and dtype); the pipeline of phases -- two stage kernels, four scoring launches, the certifying select --; the
kernel that builds the table; the stand-alone scorer; the evaluation traversal.  Each is a code object of its own, so each is
launched here: 6 cases (d, row dtype) x the launches of LAUNCHES, every traversal asserting the plan it got and looking up the
kernels that plan names in KERNELS.  test_mlp_matrix_cpu.py holds KERNELS to the build's own list of kernels.

The workload and both references are mlp_matrix.py's.  Exact and certified launches equal the oracle bit for bit (status, item
ids, score bits, rows, counters).  Split-f16 launches: every score within 1e-5 max(1, |ref|) of the float64 MLP of the row
returned with it, and on the DECISIVE queries (mlp_matrix.py: every cut of the reference's schedule wider than 3e-5) the
oracle's row set and counters, with no allowance for a diverged query."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import mlp_matrix as W
from gpu_util import bits, cuda, require_gpu, traversal_mode
from test_traverse_matrix_gpu import _assert_equal

pytestmark = pytest.mark.gpu

LPR = {64: 8, 128: 16, 256: 32}                    # lanes per row: d / 8
DT = {"f16": 0, "bf16": 1}
VIS = {"lds_bitmap": 0, "hbm_bitmap": 1, "lds_hash": 2, "lds_hash32": 3}
# SC of k_search: NANN_SCORER_MLP (exact f32, embedding rows), kScorerMlpSplit (split-f16, embedding rows), kScorerMlpRes /
# kScorerMlpXRes (split / exact on the table, layer 2 resident), kScorerMlpPhase (a traversal stage of the pipeline)
SC_ROWS = {"exact": 1, "split": 2}
SC_RES = {"split": 7, "exact": 8}
SC_PHASE = 9


def rows_threads(d, precision, mode):
    """NT of the traversal that reads the embedding rows: the split form's second mapping (kMlp2NT) on the hash set at d <= 128"""
    return 256 if precision == "split" and mode == "lds_hash" and d <= 128 else 512


# every kernel the dispatch of nann_mlp_inst.hip and nann_mlp_res_inst.hip can reach, template arguments in order
KERNELS = tuple(
    [("k_search", LPR[d], dt, VIS[m], SC_ROWS[p], rows_threads(d, p, m))                              # 12 + 12 + 6
     for d in LPR for dt in DT.values() for p, m in (("exact", "lds_bitmap"), ("exact", "hbm_bitmap"), ("split", "lds_bitmap"),
                                                     ("split", "hbm_bitmap"), ("split", "lds_hash"))] +
    [("k_search", 16, 0, VIS[m], SC_RES[p], 512) for m in ("lds_hash", "hbm_bitmap") for p in SC_RES] +  # 4
    [("k_search", 16, 0, VIS["lds_hash"], SC_PHASE, 512), ("k_search", 16, 0, VIS["lds_hash32"], SC_PHASE, 1024)] +
    [("k_mlp_phase_score", 1, 0), ("k_mlp_phase_score", 0, 0), ("k_mlp_phase_score", 0, 2), ("k_mlp_phase_score", 1, 1),
     ("k_mlp_phase_certify", 256)] +
    [("k_mlp_preproject", dt) for dt in DT.values()] +
    [("k_score_mlp", d, dt, 0) for d in LPR for dt in DT.values()] +                                  # exact: 6
    [("k_score_mlp", 256, dt, 1) for dt in DT.values()] +                                            # split at d = 256: 2
    [("k_score_mlp2", d, dt) for d in (64, 128) for dt in DT.values()] +                             # split at d <= 128: 4
    [("k_search_eval", LPR[d], dt, 1, 512, 0) for d in LPR for dt in DT.values()])                  # 6

# the launches of one case: (what, precision, forced plan or None)
LAUNCHES = (
    ("rows", "exact", "lds_bitmap"), ("rows", "exact", "hbm_bitmap"),
    ("rows", "split", "lds_hash"), ("rows", "split", "lds_bitmap"), ("rows", "split", "hbm_bitmap"),
    ("rows_per_request", "exact", "lds_bitmap"), ("rows_per_request", "split", "lds_hash"),
    ("fused", "exact", "lds_hash"), ("fused", "split", "lds_hash"), ("fused", "exact", "hbm_bitmap"), ("fused", "split", "hbm_bitmap"),
    ("phased", "exact", None), ("phased", "split", None), ("phased", "certified", None),
    ("phased_wide", "exact", None), ("phased_wide", "split", None),
    ("eval", "exact", None), ("score", "exact", None), ("score", "split", None))


def claimed(d, dtype, launch):
    """the KERNELS entries a launch of this case enters; a traversal's first: the kernel its plan names"""
    what, precision, mode = launch
    if what in ("rows", "rows_per_request"):
        return [("k_search", LPR[d], DT[dtype], VIS[mode], SC_ROWS[precision], rows_threads(d, precision, mode))]
    if what == "fused":  # the first call on a table builds it
        return [("k_search", 16, 0, VIS[mode], SC_RES[precision], 512)] + ([("k_mlp_preproject", DT[dtype])] if mode == "lds_hash" else [])
    if what in ("phased", "phased_wide"):
        stage = ("k_search", 16, 0, VIS["lds_hash"], SC_PHASE, 512) if what == "phased_wide" else ("k_search", 16, 0, VIS["lds_hash32"], SC_PHASE, 1024)
        score = {"exact": [("k_mlp_phase_score", 1, 0)], "split": [("k_mlp_phase_score", 0, 0)],
                 "certified": [("k_mlp_phase_score", 0, 2), ("k_mlp_phase_certify", 256), ("k_mlp_phase_score", 1, 1), ("k_mlp_preproject", DT[dtype])]}
        return [stage] + score[precision]
    if what == "eval":
        return [("k_search_eval", LPR[d], DT[dtype], 1, 512, 0)]
    assert what == "score"
    if precision == "split" and d <= 128:
        return [("k_score_mlp2", d, DT[dtype])]
    return [("k_score_mlp", d, DT[dtype], int(precision == "split"))]


_TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16}
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _device_index(d, dtype):
    """-> (device index, its row tensor, the 24 queries on the device)"""
    from nann_amd import retrieval
    key = (d, dtype)
    if key not in _CACHE:
        g, q = W.graph(d)
        t = W.table(d, dtype)[0]
        rows = torch.as_tensor(t.view(np.int16)).cuda().view(torch.bfloat16) if dtype == "bf16" else torch.as_tensor(t).cuda()
        _CACHE[key] = (retrieval.Index(rows, g["item_ids"], g["nb_values"], g["nb_row_splits"], g["enter_points"]), rows, cuda(q))
    return _CACHE[key]


def _launch(dix, sc, q, topn, case, launch, options):
    """one retrieval.search; asserts the plan against the launch's claim and that the kernel it names is in KERNELS -> the
    five outputs on the host"""
    from nann_amd import retrieval
    what, precision, mode = launch
    first = claimed(case[0], case[1], launch)[0]
    with traversal_mode(mode or "auto"):
        r = retrieval.search(dix, sc, q, topn, options=options)
        torch.cuda.synchronize()
    on_table = what not in ("rows", "rows_per_request")
    phased = what in ("phased", "phased_wide")
    assert r.plan["table"] == on_table and r.plan["phased"] == phased, (launch, r.plan)
    if mode:
        assert r.plan["visited_set"] == mode, (launch, r.plan)
    sc_code = SC_PHASE if phased else SC_RES["split" if precision == "split" else "exact"] if on_table else SC_ROWS[precision]
    ran = ("k_search", 16 if on_table else LPR[dix.d], 0 if on_table else DT[case[1]], VIS[r.plan["visited_set"]], sc_code, r.plan["threads"])
    assert ran == first and ran in KERNELS, (launch, ran, r.plan)
    assert all(k in KERNELS for k in claimed(case[0], case[1], launch)), launch
    if r.plan["visited_set"] in ("lds_hash", "lds_hash32"):
        assert r.reruns() == 0, "the set overflowed: the answers would be the fallback kernel's"
    return tuple(getattr(r, f).cpu().numpy() for f in ("status", "item_ids", "scores", "index", "counters"))


def _assert_split(got, case, topn, sel, what, scores64=W.scores64, expected=W.expected_exact):
    """a split-f16 launch's outputs for the queries `sel` (None: all) under `topn`.  Every query: the oracle's status, scores
    descending and within SPLIT_TOL of float64 for the row returned with each, item ids that belong to the rows.  Every decisive
    query: the oracle's row set and counters.  (scores64 / expected: what the mutation checks replace.)"""
    d, dtype = case
    g, q = W.graph(d)
    st, ids, sc, rows, ctr = got
    est, _, _, erows, ectr = expected(d, dtype, topn, sel)
    dec = W.decisive(d, dtype, topn, sel)
    k = topn[5]
    assert (st == est).all(), (what, "status", st, est)
    n_dec = 0
    for i, b in enumerate(np.arange(W.NQ) if sel is None else sel):
        if est[i]:
            continue
        ref = scores64(d, dtype, q[b], rows[i, :k])
        err = np.abs(sc[i, :k].astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
        assert err.max() <= W.SPLIT_TOL, (what, "query", b, "score against float64", float(err.max()))
        assert (np.diff(sc[i, :k]) <= 0).all(), (what, "query", b, "scores descend")
        assert (ids[i, :k] == np.asarray(g["item_ids"])[rows[i, :k]]).all(), (what, "query", b, "item ids of the rows")
        if dec[i]:
            n_dec += 1
            assert set(rows[i, :k].tolist()) == set(erows[i].tolist()) and len(set(rows[i, :k].tolist())) == k, (what, "query", b, "row set")
            assert (ctr[i] == ectr[i]).all(), (what, "query", b, "counters", ctr[i], ectr[i])
    return n_dec


def _nann_score(sc, q, table, idx):
    """nann_score through the C ABI -> (status, first bad position): what ops.blaze_score raises on"""
    from nann_amd import _lib
    from nann_amd.ops import _ptr, _stream
    out = torch.zeros(len(idx), dtype=torch.float32, device="cuda")
    idx_d = cuda(idx, torch.int32)
    bad = C.c_int64(-7)
    st = _lib.lib().nann_score(sc.handle, _ptr(q), _ptr(table), C.c_int64(table.shape[0]), _ptr(idx_d), C.c_int64(len(idx)), _ptr(out),
                               C.byref(bad), _stream())
    torch.cuda.synchronize()
    return st, bad.value


def _check_score(case, sc, precision, table, q_host):
    """the stand-alone scorer over gathered rows at every n of SCORE_N, and its report of an index out of range"""
    from nann_amd import ops
    d, dtype = case
    q = cuda(q_host)
    idx = np.random.default_rng(d).integers(0, W.N_ITEMS, max(W.SCORE_N)).astype(np.int32)  # with repeats
    exact_all = W.oracle_scores_all(d, dtype, q_host)
    ref_all = W.scores64(d, dtype, q_host, np.arange(W.N_ITEMS))

    def run(n):
        s = ops.blaze_score(sc, q, table=table, indices=cuda(idx[:n], torch.int32))
        torch.cuda.synchronize()
        assert s.shape == (n,)
        return s.cpu().numpy()

    longest = None
    for n in W.SCORE_N:
        got = longest = run(n)
        if precision == "exact":
            assert (bits(got) == bits(exact_all[idx[:n]])).all(), (case, precision, n, "score bits")
        else:
            ref = ref_all[idx[:n]]
            err = np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
            assert err.max() <= W.SPLIT_TOL, (case, precision, n, float(err.max()))
    assert (bits(run(37)) == bits(longest[:37])).all(), (case, precision, "a shorter call is the head of a longer one")
    n = max(W.SCORE_N)
    one, two = idx.copy(), idx.copy()
    one[n - 1] = W.N_ITEMS
    two[n // 2], two[n - 1] = -1, W.N_ITEMS
    assert _nann_score(sc, q, table, one) == (5, n - 1), (case, precision)  # NANN_ERR_INDEX_OUT_OF_RANGE
    assert _nann_score(sc, q, table, two) == (5, n // 2), (case, precision, "the smaller bad position")


def _check_eval(case, dix, sc, q):
    from nann_amd import retrieval
    r = retrieval.search_eval(dix, sc, q[:W.EVAL_QUERIES], *W.EVAL_CFG)
    torch.cuda.synchronize()
    st, n_out = r.status.cpu().numpy(), r.n_out.cpu().numpy()
    ids, scs, idx = r.item_ids.cpu().numpy(), r.scores.cpu().numpy(), r.index.cpu().numpy()
    n_ok = 0
    for b, (rc, eids, esc, eidx) in enumerate(W.expected_eval(*case)):
        assert st[b] == rc, (case, b, st[b], rc)
        if rc:
            assert n_out[b] == 0 and not ids[b].any()
            continue
        n = len(eids)
        n_ok += 1
        assert n_out[b] == n
        assert (idx[b, :n] == eidx).all() and (ids[b, :n] == eids).all(), (case, b, "evaluation rows")
        assert (bits(scs[b, :n]) == bits(esc)).all(), (case, b, "evaluation score bits")
        assert not ids[b, n:].any() and not scs[b, n:].any()
    assert n_ok >= W.EVAL_QUERIES - 1


@pytest.mark.parametrize("dtype", W.DTYPES)
@pytest.mark.parametrize("d", W.DIMS)
def test_every_mlp_kernel_equals_its_reference(d, dtype):
    from nann_amd import ops, retrieval
    case = (d, dtype)
    W.check_conditions(d, dtype)          # on the references alone: a pass below means something
    exp = W.expected_exact(d, dtype)
    dix, table, q = _device_index(d, dtype)
    assert dix.d == d
    scorers = {p: ops.Scorer("mlp", d, _TORCH_DT[dtype], W.weights(d), precision=p) for p in ("exact", "split", "certified")}
    tq = W.level_topn_rows()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    reps = math.ceil((cus + 1) / W.NQ)
    exact_phased = None
    for launch in LAUNCHES:
        what, precision, mode = launch
        tag = case + launch
        sc = scorers[precision]
        if what == "eval":
            _check_eval(case, dix, sc, q)
        elif what == "score":
            _check_score(case, sc, precision, table, W.graph(d)[1][0])
        elif what == "rows_per_request":
            got = _launch(dix, sc, q, tq, case, launch, retrieval.search_options(preprojection=False))
            assert got[1].shape == (W.NQ, max(W.TOPN[5], W.TOPN_ODD[5]))
            n_dec = 0
            for sel, topn in W.per_request():
                part = tuple(o[sel] for o in got)
                if precision == "exact":
                    _assert_equal(part, W.expected_exact(d, dtype, topn, sel), tag + (tuple(topn),), k=topn[5])
                else:
                    n_dec += _assert_split(part, case, topn, sel, tag + (tuple(topn),))
            assert precision == "exact" or n_dec >= W.MIN_DECISIVE
        else:
            wide = what == "phased_wide"
            if what == "rows":
                options = retrieval.search_options(preprojection=False)
            else:
                options = retrieval.search_options(mlp_form="fused" if what == "fused" else "phased")
            builds = ("k_mlp_preproject", DT[dtype]) in claimed(d, dtype, launch)
            if builds:
                assert retrieval.table_bytes(dix, sc)[1] == 0, (tag, "the table was there before its first call")
            got = _launch(dix, sc, q.repeat(reps, 1) if wide else q, W.TOPN, case, launch, options)
            if builds:
                assert retrieval.table_bytes(dix, sc)[1] > 0, tag
            if wide:
                assert got[0].shape[0] == reps * W.NQ > cus
                for o in got:  # every repeat equals its original
                    u = (bits(o) if o.dtype == np.float32 else o).reshape((reps, W.NQ) + o.shape[1:])
                    assert (u == u[:1]).all(), (tag, "repeats")
                got = tuple(o[:W.NQ] for o in got)
            if precision == "split":
                assert _assert_split(got, case, W.TOPN, None, tag) >= W.MIN_DECISIVE
            else:
                _assert_equal(got, exp, tag)
            if launch == ("phased", "exact", None):
                exact_phased = got
            if precision == "certified":  # bit for bit the exact launch, failed requests included
                for a, b in zip(got, exact_phased):
                    assert (bits(a) == bits(b)).all() if a.dtype == np.float32 else (a == b).all(), (tag, "certified against exact")
