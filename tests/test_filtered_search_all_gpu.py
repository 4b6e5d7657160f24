"""-m gpu: filtered exhaustive search (nann_search_all_filtered / nann_search_all_model_filtered; retrieval.search_all(...,
filter=)) against the CPU oracle as it stands: oracle.brute_force(k = n_items) ranks EVERY row of a query, the denied rows are
dropped from that list in numpy and the first k kept.  Ids, rows and score bits are compared.  The corpora carry a ring graph
(the scan never reads it); helpers and the duplicate-row corpus are those of test_search_all_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_util import bits, cuda, require_gpu
from test_search_all_gpu import _brute, _indices, _rows, _tie_corpus

pytestmark = pytest.mark.gpu
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


# ---- helpers -----------------------------------------------------------------------------------------------------------
def _expect(full_rows, full_scores, deny, lists, k):
    """the first k allowed entries of every query's full ranking -> (rows [B, k], scores [B, k], n_out [B]), zeros behind"""
    b, n = full_rows.shape
    rows = np.zeros((b, k), np.int32)
    scores = np.zeros((b, k), np.float32)
    n_out = np.zeros(b, np.int32)
    for i in range(b):
        allowed = np.ones(n, bool) if deny is None else ~deny
        if lists is not None:
            li = np.asarray(lists[i], np.int64)
            li = li[(li >= 0) & (li < n)]
            allowed = allowed.copy()
            allowed[li] = False
        keep = allowed[full_rows[i]]
        m = min(k, int(keep.sum()))
        rows[i, :m] = full_rows[i][keep][:m]
        scores[i, :m] = full_scores[i][keep][:m]
        n_out[i] = m
    return rows, scores, n_out


def _run(dix, scorer, q, k, flt):
    from nann_amd import retrieval
    r = retrieval.search_all(dix, scorer, cuda(q, torch.float32), k, filter=flt)
    torch.cuda.synchronize()
    return r.index.cpu().numpy(), r.scores.cpu().numpy(), r.item_ids.cpu().numpy(), r.n_out.cpu().numpy()


def _assert_same(got, exp, item_ids, what=""):
    rows, scores, ids, n_out = got
    exp_rows, exp_scores, exp_n = exp
    assert (n_out == exp_n).all(), (what, n_out, exp_n)
    assert (rows == exp_rows).all(), what
    assert (bits(scores) == bits(exp_scores)).all(), what
    exp_ids = item_ids[exp_rows]
    exp_ids[np.arange(exp_rows.shape[1])[None, :] >= exp_n[:, None]] = 0
    assert (ids == exp_ids).all(), what


def _main_case(oracle):
    """40 000 x 64 f16 (three slabs), 150 queries (chunks of 128 + 22, a partial 16-query tile), every row ranked by the oracle"""
    if "main" not in _CACHE:
        n, d = 40000, 64
        embs = _rows(n, d, "f16", seed=40)
        oix, dix = _indices(embs)
        rng = np.random.default_rng(41)
        q = rng.standard_normal((150, d)).astype(np.float32)
        q[:40] = embs[rng.integers(0, n, 40)].astype(np.float32) + 0.05 * rng.standard_normal((40, d)).astype(np.float32)
        full = _brute(oracle, oix, oracle.Scorer("l2", d, oracle.EMB_F16), q, n)
        deny = np.random.default_rng(42).random(n) < 0.3
        lists = []
        for i in range(150):  # 0-300 rows per query: some of its own best rows, the rest anywhere
            m = int(rng.integers(0, 301))
            near = full[0][i, :60][rng.random(60) < 0.5][:m]
            lists.append(np.concatenate([near, rng.integers(0, n, max(m - len(near), 0))]).astype(np.int64))
        lists[0] = np.zeros(0, np.int64)
        lists[1] = np.concatenate([lists[1], lists[1][:20], full[0][1, :5], full[0][1, :5]])
        lists[2] = np.concatenate([[-1, n, 2 ** 31 - 1], lists[2], [n + 5, -(2 ** 31)]])
        _CACHE["main"] = (embs, oix, dix, q, full, deny, lists)
    return _CACHE["main"]


def _call_c(dix, scorer, q, k, out_ids, out_scores, out_index, ws, flt=None, n_out=None, ws_bytes=None, n_queries=None):
    from nann_amd import _lib
    from nann_amd.ops import _ptr, _stream
    st = _lib.lib().nann_search_all_filtered(dix.handle, scorer.handle, _ptr(q), q.shape[0] if n_queries is None else n_queries, k,
                                             _ptr(out_ids), _ptr(out_scores), _ptr(out_index), _ptr(ws),
                                             (ws.numel() if ws is not None else 0) if ws_bytes is None else ws_bytes, None,
                                             C.byref(flt.struct) if flt is not None else None, _ptr(n_out), _stream())
    torch.cuda.synchronize()
    return st


def _ws_bytes(dix, scorer, n_queries, k, filtered=True):
    from nann_amd import _lib
    nb = C.c_int64(-1)
    L = _lib.lib()
    fn = L.nann_search_all_filtered_workspace_bytes if filtered else L.nann_search_all_workspace_bytes
    return fn(dix.handle, scorer.handle, n_queries, k, C.byref(nb)), nb.value


# ---- 1. bitmap + lists ------------------------------------------------------------------------------------------------
def test_bitmap_and_lists_bitwise(oracle):
    from nann_amd import ops, retrieval
    embs, oix, dix, q, full, deny, lists = _main_case(oracle)
    flt = retrieval.make_filter(dix, deny_rows=np.nonzero(deny)[0], exclude_rows=lists)
    exp = _expect(full[0], full[1], deny, lists, 200)
    assert (exp[2] == 200).all()
    # the filter bites: most queries lose rows of their unfiltered top 200 to the bitmap, and some to their list
    assert (exp[0] != full[0][:, :200]).any(axis=1).sum() >= 140
    assert sum(len(set(lists[i][(lists[i] >= 0) & (lists[i] < 40000)].tolist()) & set(full[0][i, :200].tolist())) > 0 for i in range(150)) >= 100
    _assert_same(_run(dix, ops.Scorer("l2", 64), q, 200, flt), exp, oix.ids)


# ---- 2. each part alone; no filter ------------------------------------------------------------------------------------
def test_bitmap_only_lists_only_and_null(oracle):
    from nann_amd import ops, retrieval
    embs, oix, dix, q, full, deny, lists = _main_case(oracle)
    sc = ops.Scorer("l2", 64)
    _assert_same(_run(dix, sc, q, 200, retrieval.make_filter(dix, deny_rows=np.nonzero(deny)[0])),
                 _expect(full[0], full[1], deny, None, 200), oix.ids, "bitmap only")
    _assert_same(_run(dix, sc, q, 200, retrieval.make_filter(dix, exclude_rows=lists)),
                 _expect(full[0], full[1], None, lists, 200), oix.ids, "lists only")
    # no filter at all: the bits of nann_search_all, n_out == k -- a NULL pointer and a struct of NULL pointers
    plain = retrieval.search_all(dix, sc, cuda(q), 200)
    torch.cuda.synchronize()
    assert (plain.index.cpu().numpy() == full[0][:, :200]).all()
    empty = _run(dix, sc, q, 200, retrieval.make_filter(dix))
    qd = cuda(q)
    st, nb = _ws_bytes(dix, sc, 150, 200)
    assert st == 0
    ws = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    out_ids = torch.full((150, 200), -77, dtype=torch.int64, device="cuda")
    out_scores = torch.full((150, 200), -77.0, dtype=torch.float32, device="cuda")
    out_index = torch.full((150, 200), -77, dtype=torch.int32, device="cuda")
    n_out = torch.full((150,), -77, dtype=torch.int32, device="cuda")
    assert _call_c(dix, sc, qd, 200, out_ids, out_scores, out_index, ws, None, n_out) == 0
    null = (out_index.cpu().numpy(), out_scores.cpu().numpy(), out_ids.cpu().numpy(), n_out.cpu().numpy())
    for got in (empty, null):
        assert (got[3] == 200).all()
        assert (got[0] == plain.index.cpu().numpy()).all() and (got[2] == plain.item_ids.cpu().numpy()).all()
        assert (bits(got[1]) == bits(plain.scores.cpu().numpy())).all()
    # NULL out_scores / out_index / n_out: the ids alone
    out_ids.fill_(-77)
    flt = retrieval.make_filter(dix, deny_rows=np.nonzero(deny)[0])
    assert _call_c(dix, sc, qd, 200, out_ids, None, None, ws, flt, None) == 0
    assert (out_ids.cpu().numpy() == oix.ids[_expect(full[0], full[1], deny, None, 200)[0]]).all()


# ---- 3. fewer allowed rows than k -------------------------------------------------------------------------------------
def test_shortfall_and_junk_bits_in_the_tail_word(oracle):
    from nann_amd import ops, retrieval
    n, k = 1000, 100
    embs = _rows(n, 64, "f16", seed=3)
    oix, dix = _indices(embs)
    rng = np.random.default_rng(30)
    q = rng.standard_normal((5, 64)).astype(np.float32)
    full = _brute(oracle, oix, oracle.Scorer("l2", 64, oracle.EMB_F16), q, n)
    keep = rng.permutation(n)[:37]
    deny = np.ones(n, bool)
    deny[keep] = False
    lists = [[], keep[:10], keep, np.concatenate([keep, keep, [-1, n]]), keep[36:]]
    flt = retrieval.make_filter(dix, deny_rows=np.nonzero(deny)[0], exclude_rows=lists)
    assert flt.deny_bits.numel() == 32
    flt.deny_bits[31] |= -256  # rows 1000..1023 of the last word: junk the kernels must ignore
    exp = _expect(full[0], full[1], deny, lists, k)
    assert exp[2].tolist() == [37, 27, 0, 0, 36]
    got = _run(dix, ops.Scorer("l2", 64), q, k, flt)
    _assert_same(got, exp, oix.ids)
    assert (got[0][0, 37:] == 0).all() and (got[1][0, 37:] == 0).all() and (got[2][0, 37:] == 0).all()
    assert (got[2][2] == 0).all() and (got[2][3] == 0).all()
    # the junk alone denies nothing, and k = n with one row denied returns n - 1 rows
    only_junk = retrieval.make_filter(dix, deny_rows=[999])
    only_junk.deny_bits[31] |= -256
    deny1 = np.zeros(n, bool)
    deny1[999] = True
    _assert_same(_run(dix, ops.Scorer("l2", 64), q, n, only_junk), _expect(full[0], full[1], deny1, None, n), oix.ids, "k = n")


# ---- 4. ties ----------------------------------------------------------------------------------------------------------
def test_a_denied_lower_row_hands_its_place_to_the_higher_one(oracle):
    from nann_amd import ops, retrieval
    embs, oix, dix = _tie_corpus()
    n = embs.shape[0]
    q = embs[[5, 777, 10000, 20010, 12345]].astype(np.float32)
    full = _brute(oracle, oix, oracle.Scorer("l2", 128, oracle.EMB_F16), q, n)
    # the query's own row is in the corpus more than once: score +0 at the head, in row order
    assert (full[1][:, :2] == 0).all() and (np.diff(full[0][:, :2], axis=1) > 0).all()
    deny = np.zeros(n, bool)
    deny[full[0][:, 0]] = True  # the lower row of every tied pair
    exp = _expect(full[0], full[1], deny, None, 200)
    assert (exp[0][:, 0] == full[0][:, 1]).all() and (exp[1][:, 0] == 0).all()
    _assert_same(_run(dix, ops.Scorer("l2", 128), q, 200, retrieval.make_filter(dix, deny_rows=np.nonzero(deny)[0])), exp, oix.ids)
    # ... and per query, through the lists
    lists = [[int(r)] for r in full[0][:, 0]]
    _assert_same(_run(dix, ops.Scorer("l2", 128), q, 4, retrieval.make_filter(dix, exclude_rows=lists)),
                 _expect(full[0], full[1], None, lists, 4), oix.ids)


# ---- 5. MLP -----------------------------------------------------------------------------------------------------------
def test_mlp_exact_bitwise(oracle):
    from nann_amd import ops, retrieval, synth
    n, d = 5000, 64
    embs, assign = synth.make_corpus(n, d, seed=55)
    oix, dix = _indices(embs)
    w = synth.make_mlp_weights(d)
    q = np.stack([oracle.user_seq_mean(s) for s in synth.make_queries(embs, assign, 9, seed=56)])
    full = _brute(oracle, oix, oracle.Scorer("mlp", d, oracle.EMB_F16, w), q, n)
    rng = np.random.default_rng(57)
    deny = rng.random(n) < 0.4
    lists = [np.concatenate([full[0][i, :30:3], rng.integers(0, n, 40)]) for i in range(9)]
    flt = retrieval.make_filter(dix, deny_rows=np.nonzero(deny)[0], exclude_rows=lists)
    exp = _expect(full[0], full[1], deny, lists, 200)
    assert (exp[2] == 200).all()
    _assert_same(_run(dix, ops.Scorer("mlp", d, torch.float16, w, precision="exact"), q, 200, flt), exp, oix.ids)


# ---- 6. the attention model -------------------------------------------------------------------------------------------
def test_attention_model_split_against_its_own_unfiltered_ranking(tmp_path):
    """Expected: the first 200 allowed rows of the device's own unfiltered search_all_model(k = 1024) -- valid because at most
    200 rows are denied, so the first 400 of that list hold 200 allowed ones (1024 - 200 >= 200)."""
    from nann_amd import retrieval
    from test_search_all_model_gpu import _corpus, _model
    n = 1500
    host, oix, dix, code, tdt, seqs = _corpus(n, 64)
    m = _model(tmp_path, 64, "split")
    seq = cuda(seqs, torch.float16)
    plain = retrieval.search_all_model(dix, m, seq, 1024)
    torch.cuda.synchronize()
    p_rows, p_scores = plain.index.cpu().numpy(), plain.scores.cpu().numpy()
    deny = np.zeros(n, bool)
    deny[np.random.default_rng(60).permutation(n)[:200]] = True
    assert (deny[p_rows[:, :200]].sum(axis=1) >= 5).all()  # (every user loses rows of its top 200)
    exp = _expect(p_rows, p_scores, deny, None, 200)
    assert (exp[2] == 200).all()
    r = retrieval.search_all_model_filtered(dix, m, seq, 200, retrieval.make_filter(dix, deny_rows=np.nonzero(deny)[0]))
    torch.cuda.synchronize()
    assert (r.n_out.cpu().numpy() == 200).all()
    assert (r.item_ids.cpu().numpy() == oix.ids[exp[0]]).all()
    assert (bits(r.scores.cpu().numpy()) == bits(exp[1])).all()
    assert (r.index.cpu().numpy() == exp[0]).all()


# ---- 7. errors: the codes of the unfiltered twin ----------------------------------------------------------------------
def test_errors_follow_the_unfiltered_twin():
    from nann_amd import _lib, ops, retrieval
    L = _lib.lib()
    embs = _rows(1000, 64, "f16", seed=3)
    oix, dix = _indices(embs)
    sc = ops.Scorer("l2", 64)
    qd = cuda(np.random.default_rng(4).standard_normal((5, 64)).astype(np.float32))
    flt = retrieval.make_filter(dix, deny_rows=[1, 2, 3], exclude_rows=[[4]] * 5)
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda")
    out = torch.full((5, 1001), -77, dtype=torch.int64, device="cuda")
    n_out = torch.full((5,), -77, dtype=torch.int32, device="cuda")
    # k > n_items -> TOPK_K_GT_N, k < 0 -> BAD_ARGUMENT: from both functions, as nann_search_all
    assert _ws_bytes(dix, sc, 5, 1001)[0] == _ws_bytes(dix, sc, 5, 1001, filtered=False)[0] == 4
    assert _call_c(dix, sc, qd, 1001, out, None, None, ws, flt, n_out) == 4 and b"at least k" in L.nann_last_error()
    assert _ws_bytes(dix, sc, 5, -1)[0] == 7 and _call_c(dix, sc, qd, -1, out, None, None, ws, flt, n_out) == 7
    # k > 1024 -> UNSUPPORTED (on a corpus that has that many rows)
    embs_t, oix_t, dix_t = _tie_corpus()
    sc_t = ops.Scorer("l2", 128)
    qt = cuda(embs_t[:2].astype(np.float32))
    assert _ws_bytes(dix_t, sc_t, 2, 1025)[0] == _ws_bytes(dix_t, sc_t, 2, 1025, filtered=False)[0] == 102
    assert _call_c(dix_t, sc_t, qt, 1025, torch.empty((2, 1025), dtype=torch.int64, device="cuda"), None, None, ws,
                   retrieval.make_filter(dix_t, deny_rows=[0]), None) == 102
    # a workspace one byte short -> CAPACITY (the filtered one is the larger: it holds the staging area); misaligned ->
    # BAD_ARGUMENT; nothing written by any of these
    st, nb = _ws_bytes(dix, sc, 5, 10)
    assert st == 0 and nb > _ws_bytes(dix, sc, 5, 10, filtered=False)[1] > 0
    ws2 = torch.zeros(nb + 256, dtype=torch.uint8, device="cuda")
    out10 = torch.full((5, 10), -77, dtype=torch.int64, device="cuda")
    assert _call_c(dix, sc, qd, 10, out10, None, None, ws2, flt, n_out, ws_bytes=nb - 1) == 103
    assert _call_c(dix, sc, qd, 10, out10, None, None, ws2[8:], flt, n_out, ws_bytes=nb) == 7 and b"aligned" in L.nann_last_error()
    assert _call_c(dix, sc, qd, 10, out10, None, None, ws2, flt, n_out, n_queries=-1) == 7
    # a malformed struct -> BAD_ARGUMENT
    bad = retrieval.make_filter(dix, exclude_rows=[[4]] * 5)
    bad.struct.n_excl = -1
    assert _call_c(dix, sc, qd, 10, out10, None, None, ws2, bad, n_out, ws_bytes=nb) == 7
    assert (out10 == -77).all() and (out == -77).all() and (n_out == -77).all()
    # k == 0, n_queries == 0 -> OK, nothing written; then the size reported is enough
    assert _call_c(dix, sc, qd, 0, out10, None, None, ws2, flt, n_out) == 0
    assert _call_c(dix, sc, qd, 10, out10, None, None, ws2, flt, n_out, n_queries=0) == 0
    assert (out10 == -77).all() and (n_out == -77).all()
    assert _call_c(dix, sc, qd, 10, out10, None, None, ws2, flt, n_out, ws_bytes=nb) == 0
    assert (n_out == 10).all() and not (out10 == -77).any()
