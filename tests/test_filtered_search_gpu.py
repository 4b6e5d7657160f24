"""-m gpu: the traversal filtered at its final selection (nann_search_filtered / nann_search_model_filtered;
retrieval.search(..., filter=, k=)) against the CPU oracle as it stands: oracle.search_batch at the same level_topn -- whose
level_topn[5] is the fetch width F -- gives every query's ranked list, the denied rows are dropped from it in numpy and the
first k kept.  Index: gpu_util.synth_index(20000, 64, ef=64); 48 queries, L2."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_util import bits, cuda, queries_for, require_gpu, synth_index

pytestmark = pytest.mark.gpu
N, D, NQ = 20000, 64, 48
TOPN = [64, 64, 64, 64, 64, 256]
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


# ---- helpers -----------------------------------------------------------------------------------------------------------
def _case(oracle):
    """(graph, oracle index, device index, queries f32[48, 64], the oracle's answer at TOPN)"""
    if "case" not in _CACHE:
        g, oix, dix = synth_index(N, D, 64)
        seqs = queries_for(g, NQ)
        q = np.stack([oracle.user_seq_mean(s) for s in seqs])
        exp = oracle.search_batch(oix, oracle.Scorer("l2", D, oracle.EMB_F16), q, TOPN, n_threads=8)
        assert (exp[0] == 0).all()
        _CACHE["case"] = (g, oix, dix, seqs, q, exp)
    return _CACHE["case"]


def _deny(frac):
    return np.random.default_rng(7).random(N) < frac


def _lists(exp_idx):
    """every query's own unfiltered top 10 plus 50 random rows"""
    rng = np.random.default_rng(8)
    return [np.concatenate([exp_idx[i, :10], rng.integers(0, N, 50)]).astype(np.int64) for i in range(exp_idx.shape[0])]


def _expect(exp, widths, deny, lists, k, item_ids):
    """the first k allowed of the first widths[i] entries of every query's list (status != 0: none)
    -> (ids, rows, scores) [B, k] with zeros behind, n_out [B]"""
    st, _, e_sc, e_idx, _ = exp
    b = len(st)
    ids = np.zeros((b, k), np.int64)
    rows = np.zeros((b, k), np.int32)
    scores = np.zeros((b, k), np.float32)
    n_out = np.zeros(b, np.int32)
    for i in range(b):
        if st[i]:
            continue
        r, s = e_idx[i, :widths[i]], e_sc[i, :widths[i]]
        allowed = np.ones(N, bool) if deny is None else ~deny
        if lists is not None:
            allowed = allowed.copy()
            allowed[lists[i]] = False
        keep = allowed[r]
        m = min(k, int(keep.sum()))
        rows[i, :m], scores[i, :m], ids[i, :m] = r[keep][:m], s[keep][:m], item_ids[r[keep][:m]]
        n_out[i] = m
    return ids, rows, scores, n_out


def _got(r):
    torch.cuda.synchronize()
    return r.item_ids.cpu().numpy(), r.index.cpu().numpy(), r.scores.cpu().numpy(), r.n_out.cpu().numpy()


def _assert_same(got, exp, what=""):
    assert (got[3] == exp[3]).all(), (what, got[3], exp[3])
    assert (got[0] == exp[0]).all() and (got[1] == exp[1]).all(), what
    assert (bits(got[2]) == bits(exp[2])).all(), what


def _filter(dix, deny, lists):
    from nann_amd import retrieval
    return retrieval.make_filter(dix, deny_rows=None if deny is None else np.nonzero(deny)[0], exclude_rows=lists)


# ---- 1. bitmap + lists ------------------------------------------------------------------------------------------------
def test_bitmap_and_lists_bitwise(oracle):
    from nann_amd import ops, retrieval
    g, oix, dix, seqs, q, exp = _case(oracle)
    deny, lists, k = _deny(0.3), _lists(exp[3]), 100
    want = _expect(exp, [256] * NQ, deny, lists, k, oix.ids)
    # the fixture keeps the case meaningful: every query has k allowed rows among its 256, and loses rows of its top k
    allowed_of_256 = _expect(exp, [256] * NQ, deny, lists, 256, oix.ids)[3]
    print("allowed rows among the 256 fetched: min %d, max %d" % (allowed_of_256.min(), allowed_of_256.max()))
    assert (allowed_of_256 >= k).all() and (want[3] == k).all()
    assert (want[1] != exp[3][:, :k]).any(axis=1).all()
    sc = ops.Scorer("l2", D)
    r = retrieval.search(dix, sc, cuda(q), TOPN, filter=_filter(dix, deny, lists), k=k)
    _assert_same(_got(r), want)
    plain = retrieval.search(dix, sc, cuda(q), TOPN)
    torch.cuda.synchronize()
    assert (r.status.cpu().numpy() == plain.status.cpu().numpy()).all() and (r.status.cpu().numpy() == 0).all()
    assert (r.counters.cpu().numpy() == plain.counters.cpu().numpy()).all()
    assert (r.counters.cpu().numpy() == exp[4]).all()
    assert r.plan == plain.plan
    assert r.reruns() == plain.reruns()
    _CACHE["main_bits"] = _got(r)


# ---- 2. fewer allowed rows than k -------------------------------------------------------------------------------------
def test_shortfall(oracle):
    from nann_amd import ops, retrieval
    g, oix, dix, seqs, q, exp = _case(oracle)
    deny, k = _deny(0.9), 100
    want = _expect(exp, [256] * NQ, deny, None, k, oix.ids)
    print("allowed rows among the 256 fetched: min %d, max %d" % (want[3].min(), want[3].max()))
    assert (want[3] < k).all() and (want[3] > 0).all()
    got = _got(retrieval.search(dix, ops.Scorer("l2", D), cuda(q), TOPN, filter=_filter(dix, deny, None), k=k))
    _assert_same(got, want)
    for i in range(NQ):
        assert (got[0][i, got[3][i]:] == 0).all() and (got[1][i, got[3][i]:] == 0).all() and (got[2][i, got[3][i]:] == 0).all()


# ---- 3. level_topn per query ------------------------------------------------------------------------------------------
def test_per_query_fetch_widths_and_a_failed_query(oracle):
    from nann_amd import ops, retrieval
    g, oix, dix, seqs, q, exp = _case(oracle)
    widths = np.array([256, 128, 64] * (NQ // 3))
    table = np.tile(np.asarray(TOPN, np.int32), (NQ, 1))
    table[:, 5] = widths
    bad = 10
    table[bad, 2] = 65  # beyond the launch's maximum of 64: that query fails, alone
    # a query's answer at its own level_topn is the head of its list at 256: the last stage ranks the same pool
    osc = oracle.Scorer("l2", D, oracle.EMB_F16)
    for w in (128, 64):
        sel = np.nonzero(widths == w)[0]
        e = oracle.search_batch(oix, osc, q[sel], TOPN[:5] + [w], n_threads=8)
        assert (e[0] == 0).all() and (e[3] == exp[3][sel, :w]).all() and (bits(e[2]) == bits(exp[2][sel, :w])).all()
    deny, lists, k = _deny(0.3), _lists(exp[3]), 60
    st = exp[0].copy()
    st[bad] = 7
    want = _expect((st,) + exp[1:], widths, deny, lists, k, oix.ids)
    assert want[3][bad] == 0 and (want[3][widths == 64] < k).any() and (want[3][widths == 256] == k).all()
    mx = (C.c_int32 * 6)(*TOPN)  # the launch's maxima
    from nann_amd import _lib
    from nann_amd.ops import _ptr, _stream
    L = _lib.lib()
    nb = C.c_int64(0)
    assert L.nann_search_filtered_workspace_bytes(dix.handle, mx, NQ, C.byref(nb)) == 0
    ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
    tq = cuda(table, torch.int32)
    out_ids = torch.full((NQ, k), -77, dtype=torch.int64, device="cuda")
    out_scores = torch.full((NQ, k), -77.0, dtype=torch.float32, device="cuda")
    out_index = torch.full((NQ, k), -77, dtype=torch.int32, device="cuda")
    status = torch.full((NQ,), -77, dtype=torch.int32, device="cuda")
    n_out = torch.full((NQ,), -77, dtype=torch.int32, device="cuda")
    flt = _filter(dix, deny, lists)
    sc, qd = ops.Scorer("l2", D), cuda(q)
    assert L.nann_search_filtered(dix.handle, sc.handle, _ptr(qd), NQ, mx, _ptr(tq), _ptr(ws), ws.numel(),
                                  _ptr(out_ids), _ptr(out_scores), _ptr(out_index), _ptr(status), None, None, None, None,
                                  C.byref(flt.struct), k, _ptr(n_out), _stream()) == 0
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == st).all()
    _assert_same((out_ids.cpu().numpy(), out_index.cpu().numpy(), out_scores.cpu().numpy(), n_out.cpu().numpy()), want)
    assert (out_ids[bad] == 0).all() and (out_scores[bad] == 0).all() and (out_index[bad] == 0).all()


# ---- 4. no filter, F = k ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("traversal", [None, "hbm_bitmap"])
def test_null_filter_at_full_width_is_the_unfiltered_call(oracle, traversal):
    from nann_amd import ops, retrieval
    g, oix, dix, seqs, q, exp = _case(oracle)
    sc = ops.Scorer("l2", D)
    opt = None if traversal is None else retrieval.search_options(traversal=traversal)
    plain = retrieval.search(dix, sc, cuda(q), TOPN, options=opt)
    r = retrieval.search(dix, sc, cuda(q), TOPN, options=opt, k=256)
    got = _got(r)
    assert (got[3] == 256).all()
    assert (got[0] == plain.item_ids.cpu().numpy()).all() and (got[1] == plain.index.cpu().numpy()).all()
    assert (bits(got[2]) == bits(plain.scores.cpu().numpy())).all()
    assert (got[1] == exp[3]).all() and (bits(got[2]) == bits(exp[2])).all()
    assert r.plan == plain.plan
    if traversal is not None:  # the options reached the inner search
        assert r.plan["visited_set"] == traversal


# ---- 5. the serving signature -----------------------------------------------------------------------------------------
def test_model_form_gives_the_same_bits(oracle, tmp_path):
    from nann_amd import ops, retrieval
    g, oix, dix, seqs, q, exp = _case(oracle)
    deny, lists, k = _deny(0.3), _lists(exp[3]), 100
    want = _expect(exp, [256] * NQ, deny, lists, k, oix.ids)
    ops.save_scorer_dir(str(tmp_path / "l2"), "l2")
    m = ops.Model(str(tmp_path / "l2"), D, seqs.shape[1])
    r = retrieval.search_model(dix, m, cuda(seqs, torch.float16), TOPN, filter=_filter(dix, deny, lists), k=k)
    got = _got(r)
    _assert_same(got, want)
    assert (r.status.cpu().numpy() == 0).all() and (r.counters.cpu().numpy() == exp[4]).all()
    if "main_bits" in _CACHE:
        assert all((a == b).all() for a, b in zip(got[:2] + (bits(got[2]), got[3]), _CACHE["main_bits"][:2] +
                                                 (bits(_CACHE["main_bits"][2]), _CACHE["main_bits"][3])))


# ---- 6. errors --------------------------------------------------------------------------------------------------------
def test_k_outside_the_fetch_width_and_a_short_workspace(oracle):
    from nann_amd import _lib, ops
    from nann_amd.ops import _ptr, _stream
    g, oix, dix, seqs, q, exp = _case(oracle)
    L = _lib.lib()
    mx = (C.c_int32 * 6)(*TOPN)
    nb, inner = C.c_int64(0), C.c_int64(0)
    assert L.nann_search_filtered_workspace_bytes(dix.handle, mx, NQ, C.byref(nb)) == 0
    assert L.nann_search_workspace_bytes(dix.handle, mx, C.c_int64(NQ), C.byref(inner)) == 0
    assert nb.value >= inner.value + 16 * 256 * NQ  # the staging area: 16 B x F per query
    ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
    qd = cuda(q)
    sc = ops.Scorer("l2", D)
    out_ids = torch.full((NQ, 256), -77, dtype=torch.int64, device="cuda")
    status = torch.full((NQ,), -77, dtype=torch.int32, device="cuda")
    n_out = torch.full((NQ,), -77, dtype=torch.int32, device="cuda")

    def call(k, ws_bytes):
        st = L.nann_search_filtered(dix.handle, sc.handle, _ptr(qd), NQ, mx, None, _ptr(ws), ws_bytes, _ptr(out_ids), None, None,
                                    _ptr(status), None, None, None, None, None, k, _ptr(n_out), _stream())
        torch.cuda.synchronize()
        return st

    assert call(257, nb.value) == 7 and b"level_topn_max[5]" in L.nann_last_error()
    assert call(-1, nb.value) == 7
    assert call(100, nb.value - 1) == 103
    assert call(100, inner.value) == 103  # (the unfiltered size is not enough)
    assert (out_ids == -77).all() and (status == -77).all() and (n_out == -77).all()
    assert call(256, nb.value) == 0
    assert (n_out == 256).all() and (out_ids.cpu().numpy() == exp[1]).all()
