"""-m gpu: the wide exhaustive search (nann_search_all_wide / retrieval.search_all_wide) against the CPU oracle's brute force, and
the selection alone (nann_select_wide / ops.select_wide) on crafted matrices against np.lexsort.  No tolerance anywhere: rows,
score bits and item ids.  The oracle's full ranking of a query is computed once (k = n); its top k is the head of it, for every
k -- (score descending, row ascending) is a total order."""
import ctypes as C

import numpy as np
import pytest
import torch

import wide_model as M
from gpu_util import bits, cuda, require_gpu
from test_search_all_gpu import _brute, _ring, _rows

pytestmark = pytest.mark.gpu
_CACHE = {}
N = 20001   # odd: query rows fall on every alignment in the score buffer


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _indices(embs):
    from nann_amd import retrieval
    from oracle import oracle as O
    n = embs.shape[0]
    ids = np.arange(n, dtype=np.int64) * 7 + 3
    if n == 1:
        nbv, rs, ep = [np.zeros(1, np.int32)] * 2, [np.array([0, 1], np.int64)] * 2, np.zeros(1, np.int32)
    else:
        nbv, rs, ep = _ring(n)
    return O.Index(embs, ids, nbv, rs, ep), retrieval.Index(embs, ids, nbv, rs, ep)


def _case(oracle, name):
    """(oracle index, device index, queries f32[5, 64], the oracle's full ranking under L2: rows, scores)"""
    if name not in _CACHE:
        rng = np.random.default_rng(len(name))
        if name == "random":
            embs = _rows(N, 64, "f16", seed=91)
            q = rng.standard_normal((5, 64)).astype(np.float32)
        elif name == "protos":  # 37 prototype vectors in turn: every score value about 540 times, in every block
            protos = _rows(37, 64, "f16", seed=92)
            embs = np.ascontiguousarray(protos[np.arange(N) % 37])
            q = protos[[0, 5, 11, 36, 20]].astype(np.float32) + np.float32(0.25)
        else:                   # every row the same
            embs = np.ascontiguousarray(np.tile(_rows(1, 64, "f16", seed=93), (N, 1)))
            q = rng.standard_normal((5, 64)).astype(np.float32)
        oix, dix = _indices(embs)
        full = _brute(oracle, oix, oracle.Scorer("l2", 64, oracle.EMB_F16), q, N)
        _CACHE[name] = (oix, dix, q) + full
    return _CACHE[name]


def _wide(dix, sc, q, k, **kw):
    from nann_amd import retrieval
    r = retrieval.search_all_wide(dix, sc, cuda(q, torch.float32), k, **kw)
    torch.cuda.synchronize()
    return r.index.cpu().numpy(), r.scores.cpu().numpy(), r.item_ids.cpu().numpy(), r.n_out.cpu().numpy()


def _assert_top(got, exp_rows, exp_scores, item_ids, k, what=""):
    rows, scores, ids, n_out = got
    assert rows.shape == (exp_rows.shape[0], k) and (n_out == k).all(), what
    assert (rows == exp_rows[:, :k]).all(), what
    assert (bits(scores) == bits(exp_scores[:, :k])).all(), what
    assert (ids == item_ids[exp_rows[:, :k]]).all(), what


# ---- 1. L2 against the oracle, and against search_all where both exist ------------------------------------------------------
@pytest.mark.parametrize("k", [1, 200, 1024, 1025, 4097, 16384])
def test_l2_bitwise(oracle, k):
    from nann_amd import ops, retrieval
    oix, dix, q, exp_rows, exp_scores = _case(oracle, "random")
    sc = ops.Scorer("l2", 64)
    got = _wide(dix, sc, q, k)
    _assert_top(got, exp_rows, exp_scores, oix.ids, k, k)
    if k <= 1024:
        r = retrieval.search_all(dix, sc, cuda(q), k)
        torch.cuda.synchronize()
        assert (r.index.cpu().numpy() == got[0]).all() and (bits(r.scores.cpu().numpy()) == bits(got[1])).all()
        assert (r.item_ids.cpu().numpy() == got[2]).all()


@pytest.mark.parametrize("n", [1, 2045, 2048, 2049])
def test_the_whole_table_comes_back_sorted(oracle, n):
    from nann_amd import ops
    embs = _rows(n, 64, "f16", seed=n)
    oix, dix = _indices(embs)
    q = np.random.default_rng(n).standard_normal((3, 64)).astype(np.float32)
    exp_rows, exp_scores = _brute(oracle, oix, oracle.Scorer("l2", 64, oracle.EMB_F16), q, n)
    _assert_top(_wide(dix, ops.Scorer("l2", 64), q, n), exp_rows, exp_scores, oix.ids, n, n)


def test_inner_product(oracle):
    from nann_amd import ops
    import ip_reference as R   # (the oracle has no inner product: the test-side reference the other IP tests hold the kernels to)
    oix, dix, q, _, _ = _case(oracle, "random")
    rows = R.widen(oix.embs)
    s = np.stack([R.ip_scores(v, rows) for v in q[:3]])
    exp_rows = np.stack([R.topk_stable(v, 4097) for v in s]).astype(np.int32)
    exp_scores = np.take_along_axis(s, exp_rows.astype(np.int64), axis=1)
    _assert_top(_wide(dix, ops.Scorer("ip", 64), q[:3], 4097), exp_rows, exp_scores, oix.ids, 4097)


# ---- 2. ties ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1025, 4097])
def test_a_cut_inside_a_tie_class_takes_the_lower_rows(oracle, k):
    from nann_amd import ops
    oix, dix, q, exp_rows, exp_scores = _case(oracle, "protos")
    # the corpus does what it was built for: the k-th score ties with the one behind it, and the rows of a class ascend
    assert (bits(exp_scores[:, k - 1]) == bits(exp_scores[:, k])).all() and (exp_rows[:, k - 1] < exp_rows[:, k]).all()
    _assert_top(_wide(dix, ops.Scorer("l2", 64), q, k), exp_rows, exp_scores, oix.ids, k, k)


def test_all_rows_identical(oracle):
    from nann_amd import ops
    oix, dix, q, exp_rows, exp_scores = _case(oracle, "same")
    for k in (1, 2049, 16384):
        got = _wide(dix, ops.Scorer("l2", 64), q, k)
        assert (got[0] == np.arange(k)[None]).all(), k
        _assert_top(got, exp_rows, exp_scores, oix.ids, k, k)


# ---- 3. batch independence ------------------------------------------------------------------------------------------------------
def test_answer_does_not_depend_on_the_batch():
    from nann_amd import ops
    embs = _rows(4099, 64, "f16", seed=17)
    _, dix = _indices(embs)
    q = np.random.default_rng(18).standard_normal((130, 64)).astype(np.float32)   # more than the 128 queries of a chunk
    sc = ops.Scorer("l2", 64)
    rows, scores, ids, n_out = _wide(dix, sc, q, 2000)
    assert (n_out == 2000).all()
    for i in (0, 1, 63, 127, 128, 129):
        r1, s1, i1, n1 = _wide(dix, sc, q[i:i + 1], 2000)
        assert (r1[0] == rows[i]).all() and (bits(s1[0]) == bits(scores[i])).all() and (i1[0] == ids[i]).all(), i
    assert (np.diff(scores.astype(np.float64), axis=1) <= 0).all()


# ---- 4. the selection alone, on crafted scores -----------------------------------------------------------------------------------
def _select(values, k):
    from nann_amd import ops
    v, i, n = ops.select_wide(cuda(values, torch.float32), k)
    torch.cuda.synchronize()
    return v.cpu().numpy(), i.cpu().numpy(), n.cpu().numpy()


def _assert_reference(values, k, what):
    v, i, n = _select(values, k)
    for r in range(values.shape[0]):
        ev, ei, en = M.reference(values[r], k)
        assert n[r] == en, (what, r)
        assert (i[r] == ei).all() and (bits(v[r]) == bits(ev)).all(), (what, r)
    return v, i, n


C_COLS = 40003


def test_select_mixed_zeros_tie_in_row_order():
    rng = np.random.default_rng(31)
    z = np.where(rng.integers(0, 2, (3, C_COLS)) == 1, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    z[2, ::5] = np.float32(-1.0)
    for k in (1, 4097, 16384):
        v, i, n = _assert_reference(z, k, ("zeros", k))
        assert (i[:2] == np.arange(k)[None]).all() and (np.signbit(v[0]) == np.signbit(z[0, :k])).all()  # the original bits


def test_select_fewer_valid_rows_than_k():
    rng = np.random.default_rng(32)
    m = np.full((4, C_COLS), -np.inf, np.float32)
    for r, cnt in enumerate((700, 0, 4096, 1)):
        at = rng.permutation(C_COLS)[:cnt]
        m[r, at] = rng.integers(0, 50, cnt).astype(np.float32)
    v, i, n = _assert_reference(m, 4097, "few valid")
    assert n.tolist() == [700, 0, 4096, 1]
    assert (v[0, 700:] == 0).all() and (i[0, 700:] == 0).all() and (v[1] == 0).all() and (i[1] == 0).all()


def test_select_denormals():
    rng = np.random.default_rng(33)
    d = (rng.integers(-3000, 3000, (2, C_COLS)).astype(np.float64) * 2.0 ** -149).astype(np.float32)
    for k in (1, 1025, 16384):
        _assert_reference(d, k, ("denormals", k))


def test_select_copies_of_one_value_straddle_the_cut():
    rng = np.random.default_rng(34)
    m = rng.standard_normal((3, C_COLS)).astype(np.float32)
    for r in range(3):
        m[r, rng.permutation(C_COLS)[:3000]] = np.float32(1.0)   # about 5900 values lie above 1.0
    for k in (6500, 7500, 8500):
        v, i, n = _assert_reference(m, k, ("copies", k))
        assert (v[:, k - 1] == 1.0).all() and ((m > 1.0).sum(1) < k).all() and ((m >= 1.0).sum(1) > k).all()


def test_select_a_row_shorter_than_a_block_and_a_single_row():
    rng = np.random.default_rng(35)
    m = rng.integers(-3, 3, (9, 17)).astype(np.float32)          # rows begin at every alignment; many ties
    _assert_reference(m, 17, "n_cols = k = 17")
    _assert_reference(m[:, :1].copy(), 1, "n_cols = 1")
    v, i, n = _select(m[0], 5)                                    # one row, 1-D in and out
    ev, ei, en = M.reference(m[0], 5)
    assert v.shape == (5,) and (i == ei).all() and (bits(v) == bits(ev)).all() and int(n) == en


def test_select_more_rows_than_a_chunk():
    rng = np.random.default_rng(36)
    m = rng.integers(-50, 50, (261, 2051)).astype(np.float32)    # three launches of at most 128 rows; a row is a block plus three
    m[rng.random(m.shape) < 0.3] = -np.inf
    _assert_reference(m, 1500, "261 rows")


# ---- 5. the contract in front of a launch -----------------------------------------------------------------------------------------
def test_status_codes_and_empty_calls(oracle):
    from nann_amd import _lib, ops
    from nann_amd.ops import _ptr, _stream
    oix, dix, q, exp_rows, exp_scores = _case(oracle, "random")
    L = _lib.lib()
    sc = ops.Scorer("l2", 64)
    qd = cuda(q)
    nb = C.c_int64(-1)
    size = lambda b, k: L.nann_search_all_wide_workspace_bytes(dix.handle, sc.handle, b, k, C.byref(nb))
    assert size(5, -1) == 7 and size(5, 16385) == 102 and b"k <= 16384" in L.nann_last_error()
    assert size(5, N + 1) == 4 and size(0, 8) == 0 and nb.value == 0 and size(5, 0) == 0 and nb.value == 0
    assert size(5, 4097) == 0 and nb.value > 0
    need = nb.value
    assert L.nann_search_all_workspace_bytes(dix.handle, sc.handle, 5, 1025, C.byref(nb)) == 102   # the slab form keeps its limit
    ids = torch.full((5, 4097), -77, dtype=torch.int64, device="cuda")
    n_out = torch.full((5,), -77, dtype=torch.int32, device="cuda")
    ws = torch.zeros(need + 256, dtype=torch.uint8, device="cuda")

    def call(b, k, out=ids, w=ws, wb=need, x=qd):
        st = L.nann_search_all_wide(dix.handle, sc.handle, _ptr(x), b, k, _ptr(out), None, None, _ptr(n_out), _ptr(w), wb, None,
                                    None, None, _stream())
        torch.cuda.synchronize()
        return st

    assert call(5, -1) == 7 and call(5, 16385) == 102 and call(5, N + 1) == 4 and b"at least k" in L.nann_last_error()
    assert call(5, 4097, out=None) == 7 and call(5, 4097, x=None) == 7
    assert call(5, 4097, wb=need - 1) == 103 and call(5, 4097, w=ws[16:], wb=need) == 7
    assert call(0, 4097) == 0 and call(5, 0) == 0
    assert (ids == -77).all() and (n_out == -77).all()                                           # nothing launched
    assert call(5, 4097) == 0                                                                      # NULL out_scores / out_index
    assert (ids.cpu().numpy() == oix.ids[exp_rows[:, :4097]]).all() and (n_out == 4097).all()
