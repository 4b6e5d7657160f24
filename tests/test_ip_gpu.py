"""-m gpu: the inner-product scorer (NANN_SCORER_IP) through every call that accepts it.  The reference is ip_reference.py:
the canonical order restated in numpy with a correctly rounded fma (score bits), TopKV2's order restated with a stable sort,
and the serving schedule restated over a score callable.  Rows are scaled by per-row factors in [0.25, 4] and queries are not
normalised, so that the inner product and L2 rank them differently: a kernel that ran L2 arithmetic would not pass.

Indices for the flat calls carry the ring graph of test_search_all_gpu.py (those calls never read the graph); the traversal
runs on the synthetic HNSW graphs of gpu_util.synth_index with their rows scaled."""
import ctypes as C

import numpy as np
import pytest
import torch

import ip_reference as R
from gpu_util import MODES, bits, cuda, queries_for, require_gpu, synth_index, traversal_mode
from test_search_all_gpu import _ring

pytestmark = pytest.mark.gpu
_CACHE = {}
_TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


# ---- helpers ------------------------------------------------------------------------------------------------------------
def _table(x, dtype):
    """rows x f32 in the table's dtype -> (device tensor, their f32 widening)"""
    if dtype == "f16":
        h = x.astype(np.float16)
        return torch.as_tensor(h).cuda(), h.astype(np.float32)
    if dtype == "bf16":
        b = R.to_bf16_bits(x)
        return torch.as_tensor(b.view(np.int16)).cuda().view(torch.bfloat16), R.widen(b)
    return torch.as_tensor(x).cuda(), x


def _flat_case(n, d, dtype):
    """scaled random rows under a ring graph -> dict(table, wide, dix, ids)"""
    from nann_amd import retrieval
    key = ("flat", n, d, dtype)
    if key not in _CACHE:
        x = R.scaled_rows(np.random.default_rng(n + d).standard_normal((n, d)).astype(np.float32), seed=n)
        table, wide = _table(x, dtype)
        ids = np.arange(n, dtype=np.int64) * 7 + 3
        nbv, rs, ep = _ring(n)
        _CACHE[key] = {"table": table, "wide": wide, "ids": ids, "dix": retrieval.Index(table, ids, nbv, rs, ep)}
    return _CACHE[key]


def _graph_case(d, dtype):
    """synth_index(20000, d, 32) with its rows scaled, in `dtype` -> dict(g, table, wide, dix, q f32[40, d] on the device)"""
    from nann_amd import ops, retrieval
    key = ("graph", d, dtype)
    if key not in _CACHE:
        g, _, _ = synth_index(20000, d, 32)
        x = R.scaled_rows(R.widen(g["item_embs"]), seed=d)
        table, wide = _table(x, dtype)
        dix = retrieval.Index(table, g["item_ids"], g["nb_values"], g["nb_row_splits"], g["enter_points"])
        q = ops.user_seq_mean(cuda(queries_for(g, 40, seed=31)))
        _CACHE[key] = {"g": g, "table": table, "wide": wide, "dix": dix, "q": q, "ids": np.asarray(g["item_ids"])}
    return _CACHE[key]


def _queries(b, d, seed):
    return (np.random.default_rng(seed).standard_normal((b, d)) * 1.5).astype(np.float32)


def _scorer(d, dtype, kind="ip"):
    from nann_amd import ops
    return ops.Scorer(kind, d, _TORCH_DT[dtype])


def _score(sc, q, table, idx=None):
    """nann_score of one query: over the table's rows in order, or over table[idx]"""
    from nann_amd import ops
    s = ops.blaze_score(sc, cuda(q), item_emb=table) if idx is None else ops.blaze_score(sc, cuda(q), table=table, indices=cuda(idx, torch.int32))
    torch.cuda.synchronize()
    return s.cpu().numpy()


def _search(dix, sc, q, topn, mode="auto", **kw):
    from nann_amd import retrieval
    with traversal_mode(mode):
        r = retrieval.search(dix, sc, q, topn, **kw)
        torch.cuda.synchronize()
    return r


def _np(r):
    return (r.status.cpu().numpy(), r.item_ids.cpu().numpy(), r.scores.cpu().numpy(), r.index.cpu().numpy(), r.counters.cpu().numpy())


# ---- 1. nann_score ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dtype", [(64, "f16"), (128, "f16"), (128, "bf16"), (256, "f32"), (512, "bf16")])
def test_score_bits_equal_the_canonical_order(d, dtype):
    c = _flat_case(300, d, dtype)
    sc = _scorer(d, dtype)
    q = _queries(1, d, seed=d)[0]
    rng = np.random.default_rng(d + 1)
    for n in (1, 127, 128, 129, 300):
        got = _score(sc, q, c["table"][:n])
        assert (bits(got) == bits(R.ip_scores(q, c["wide"][:n]))).all(), (n, "rows in order")
        idx = rng.integers(0, 300, n)  # shuffled, with repeats
        got = _score(sc, q, c["table"], idx)
        assert (bits(got) == bits(R.ip_scores(q, c["wide"][idx]))).all(), (n, "gathered")
    # and it is not L2 on this data
    assert (bits(_score(sc, q, c["table"])) != bits(R.l2_scores(q, c["wide"]))).all()


def test_score_status_codes():
    from nann_amd import _lib
    from nann_amd.ops import _ptr, _stream
    c = _flat_case(300, 128, "f16")
    sc = _scorer(128, "f16")
    q = cuda(_queries(1, 128, seed=2)[0])
    idx = np.arange(20, dtype=np.int32)
    idx[9], idx[5] = -1, 300
    idx_d = cuda(idx, torch.int32)
    out = torch.zeros(20, dtype=torch.float32, device="cuda")
    bad = C.c_int64(-7)
    L = _lib.lib()
    st = L.nann_score(sc.handle, _ptr(q), _ptr(c["table"]), C.c_int64(300), _ptr(idx_d), C.c_int64(20), _ptr(out), C.byref(bad), _stream())
    assert st == 5 and bad.value == 5  # NANN_ERR_INDEX_OUT_OF_RANGE, the first bad position
    st = L.nann_score(sc.handle, _ptr(q), _ptr(c["table"]), C.c_int64(300), None, C.c_int64(0), _ptr(out), C.byref(bad), _stream())
    assert st == 6  # NANN_ERR_EMPTY_SCORE_BATCH
    torch.cuda.synchronize()


# ---- 2. exhaustive search -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items", [700, 20011])
@pytest.mark.parametrize("d,dtype", [(64, "f16"), (128, "bf16"), (512, "f32")])
def test_search_all_equals_score_plus_topk(d, dtype, n_items):
    """700: not a multiple of the 256 rows of a workgroup; 20011: two slabs.  17 queries: one full tile of 16 plus one."""
    from nann_amd import ops, retrieval
    c = _flat_case(n_items, d, dtype)
    sc = _scorer(d, dtype)
    q = _queries(17, d, seed=n_items + d)
    scores = np.stack([_score(sc, q[i], c["table"]) for i in range(17)])
    if n_items == 700:
        exp = np.stack([R.ip_scores(q[i], c["wide"]) for i in range(17)])
        assert (bits(scores) == bits(exp)).all()
    for k in (1, 10, 200):
        r = retrieval.search_all(c["dix"], sc, cuda(q), k)
        torch.cuda.synchronize()
        rows, got, ids = r.index.cpu().numpy(), r.scores.cpu().numpy(), r.item_ids.cpu().numpy()
        for i in range(17):
            top = R.topk_stable(scores[i], k)
            assert (rows[i] == top).all(), (k, i)
            assert (bits(got[i]) == bits(scores[i][top])).all(), (k, i)
            assert (ids[i] == c["ids"][top]).all(), (k, i)
    if n_items == 700:
        with pytest.raises(ops.NannError) as e:
            retrieval.search_all(c["dix"], sc, cuda(q), 701)
        assert e.value.status == 4  # NANN_ERR_TOPK_K_GT_N


# ---- 3. candidate lists -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dtype", [(128, "f16"), (64, "f32")])
def test_search_candidates_equals_score_plus_topk(d, dtype):
    from nann_amd import retrieval
    n, k = 700, 200
    c = _flat_case(n, d, dtype)
    sc = _scorer(d, dtype)
    rng = np.random.default_rng(d)
    dup = rng.integers(0, 40, 120)                 # 120 draws of 40 rows: duplicates
    long_ = rng.integers(0, n, retrieval.CANDIDATE_BLOCK_ROWS + 476)  # longer than one block of kCandRows
    out_of_range = rng.integers(0, n, 30)
    out_of_range[11] = n                           # one row >= n_items: status 5, a zeroed row
    lists = [np.zeros(0, np.int64), np.array([17]), dup, long_, out_of_range, rng.integers(0, n, 7), rng.integers(0, n, 260),
             rng.integers(0, n, 25)]
    q = _queries(8, d, seed=d + 5)
    splits = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    rows = np.concatenate(lists).astype(np.int32)
    splits[8] = splits[7] - 1                      # the last query's range ends before it begins: status 3
    failed = {4: 5, 7: 3}

    def run(sp, rw):
        r = retrieval.search_candidates(c["dix"], sc, cuda(q), candidates=(cuda(sp, torch.int64), cuda(rw, torch.int32)), k=k)
        torch.cuda.synchronize()
        return {f: getattr(r, f).cpu().numpy() for f in ("index", "pos", "scores", "item_ids", "n_out", "status")}

    got = run(splits, rows)
    for i, l in enumerate(lists):
        if i in failed:
            assert got["status"][i] == failed[i] and got["n_out"][i] == 0
            assert not got["index"][i].any() and not got["pos"][i].any() and not got["item_ids"][i].any() and not bits(got["scores"][i]).any()
            continue
        m = min(k, len(l))
        assert got["status"][i] == 0 and got["n_out"][i] == m, i
        if m:
            s = _score(sc, q[i], c["table"], l)
            pos = R.topk_stable(s, m)
            assert (got["pos"][i, :m] == pos).all(), i
            assert (got["index"][i, :m] == l[pos]).all(), i
            assert (bits(got["scores"][i, :m]) == bits(s[pos])).all(), i
            assert (got["item_ids"][i, :m] == c["ids"][l[pos]]).all(), i
        assert not got["index"][i, m:].any() and not got["pos"][i, m:].any() and not bits(got["scores"][i, m:]).any()
    # the same call with the two bad queries mended (an in-range row, a well-formed empty list): the other queries' answers stay
    rows2, splits2 = rows.copy(), splits.copy()
    rows2[splits[4] + 11] = 3
    splits2[8] = splits2[7]
    again = run(splits2, rows2)
    assert again["status"].tolist() == [0] * 8
    good = [i for i in range(8) if i not in failed]
    for f in ("index", "pos", "item_ids", "n_out"):
        assert (again[f][good] == got[f][good]).all(), f
    assert (bits(again["scores"][good]) == bits(got["scores"][good])).all()


# ---- 4. the traversal ---------------------------------------------------------------------------------------------------
TOPNS = [[32] * 5 + [20], [16, 32, 64, 64, 64, 20]]


def _per_op(c, sc, b, topn):
    """(status, ids, scores, rows) of query b through the op-by-op schedule"""
    from nann_amd import ops, retrieval
    try:
        ids, scores, idx = retrieval.search_per_op(c["dix"], sc, c["q"][b], topn)
    except ops.NannError as e:
        return e.status, None, None, None
    torch.cuda.synchronize()
    return 0, ids.cpu().numpy(), scores.cpu().numpy(), idx.cpu().numpy()


@pytest.mark.parametrize("topn", TOPNS, ids=["even", "uneven"])
@pytest.mark.parametrize("d,dtype", [(64, "f16"), (128, "f16"), (128, "bf16"), (64, "f32")])
def test_traversal_equals_the_per_op_schedule(d, dtype, topn):
    c = _graph_case(d, dtype)
    sc = _scorer(d, dtype)
    auto = _search(c["dix"], sc, c["q"], topn)
    assert auto.reruns() >= 0
    base = _np(auto)
    assert (base[0] == 0).mean() > 0.5, "the workload should be mostly valid requests"
    for mode in MODES:
        got = _np(_search(c["dix"], sc, c["q"], topn, mode))
        ok = base[0] == 0
        assert (got[0] == base[0]).all(), mode
        assert (got[1][ok] == base[1][ok]).all() and (got[3][ok] == base[3][ok]).all(), mode
        assert (bits(got[2][ok]) == bits(base[2][ok])).all(), mode
        assert (got[4][ok] == base[4][ok]).all(), (mode, "counters")
        assert (got[1][~ok] == 0).all()
    qh = c["q"].cpu().numpy()
    for b in range(6):
        st, ids, scores, idx = _per_op(c, sc, b, topn)
        assert base[0][b] == st, b
        if st:
            continue
        assert (base[1][b] == ids).all() and (base[3][b] == idx).all() and (bits(base[2][b]) == bits(scores)).all(), b
        if (d, dtype) == (64, "f16"):  # and the schedule restated on the CPU, scored in the restated order
            pids, ps, pidx = R.py_search(c["g"], qh[b], topn, lambda i: R.ip_scores(qh[b], c["wide"][np.asarray(i)]))
            assert (pidx == idx).all() and (pids == ids).all() and (bits(ps) == bits(scores)).all(), b
            lids, _, lidx = R.py_search(c["g"], qh[b], topn, lambda i: R.l2_scores(qh[b], c["wide"][np.asarray(i)]))
            assert lidx.tolist() != idx.tolist(), "L2 would have ranked this query the same: the data catches nothing"


@pytest.mark.parametrize("mode", ["auto"] + MODES)
def test_failing_requests_get_the_per_op_codes(mode):
    c = _graph_case(64, "f16")
    sc = _scorer(64, "f16")
    E = len(c["g"]["enter_points"])
    for topn in ([E + 1, 8, 8, 8, 8, 8], [8, 8, 8, 8, 8, 33]):
        key = ("codes", tuple(topn))
        if key not in _CACHE:
            _CACHE[key] = [_per_op(c, sc, b, topn)[0] for b in range(2)]
        exp = _CACHE[key]
        assert all(exp), topn
        got = _np(_search(c["dix"], sc, c["q"][:8], topn, mode))
        assert (got[0][:2] == exp).all() and (got[0] == exp[0]).all(), (topn, got[0], exp)
        assert (got[1] == 0).all()


@pytest.mark.parametrize("mode", ["lds_hash", "lds_bitmap"])
def test_batch_size_independence(mode):
    from nann_amd import ops
    c = _graph_case(128, "f16")
    sc = _scorer(128, "f16")
    q = ops.user_seq_mean(cuda(queries_for(c["g"], 1400, seed=99)))
    topn = [32] * 5 + [20]
    full = _np(_search(c["dix"], sc, q, topn, mode))  # more queries than workgroup slots: slots are reused
    for b in (0, 255, 256, 511, 512, 1399):
        one = _np(_search(c["dix"], sc, q[b:b + 1], topn, mode))
        assert one[0][0] == full[0][b]
        assert (one[1][0] == full[1][b]).all() and (bits(one[2][0]) == bits(full[2][b])).all()


# ---- 5. filters ---------------------------------------------------------------------------------------------------------
def test_filtered_search_is_the_allowed_head_of_the_unfiltered_answer():
    from nann_amd import retrieval
    c = _graph_case(128, "f16")
    sc = _scorer(128, "f16")
    topn = [32] * 5 + [64]  # the fetch width F = 64
    plain = _np(_search(c["dix"], sc, c["q"], topn))
    deny = np.random.default_rng(7).random(20000) < 0.3
    f = retrieval.make_filter(c["dix"], deny_rows=np.nonzero(deny)[0])
    r = _search(c["dix"], sc, c["q"], topn, filter=f, k=10)
    n_out, rows, scores, ids = r.n_out.cpu().numpy(), r.index.cpu().numpy(), r.scores.cpu().numpy(), r.item_ids.cpu().numpy()
    assert (r.status.cpu().numpy() == plain[0]).all()
    checked = 0
    for b in range(40):
        if plain[0][b]:
            continue
        keep = ~deny[plain[3][b]]
        m = min(10, int(keep.sum()))
        assert n_out[b] == m
        assert (rows[b, :m] == plain[3][b][keep][:m]).all() and (bits(scores[b, :m]) == bits(plain[2][b][keep][:m])).all()
        assert (ids[b, :m] == plain[1][b][keep][:m]).all()
        checked += int((rows[b, :m] != plain[3][b][:m]).any())
    assert checked > 0, "the filter should have removed rows from some query's head"


def test_filtered_search_all_is_the_topk_of_the_allowed_rows():
    from nann_amd import retrieval
    c = _flat_case(700, 128, "bf16")
    sc = _scorer(128, "bf16")
    q = _queries(17, 128, seed=9)
    deny = np.random.default_rng(8).random(700) < 0.4
    allowed = np.nonzero(~deny)[0]
    r = retrieval.search_all(c["dix"], sc, cuda(q), 10, filter=retrieval.make_filter(c["dix"], deny_rows=np.nonzero(deny)[0]))
    torch.cuda.synchronize()
    rows, got = r.index.cpu().numpy(), r.scores.cpu().numpy()
    assert (r.n_out.cpu().numpy() == 10).all()
    for i in range(17):
        s = _score(sc, q[i], c["table"])
        top = allowed[R.topk_stable(s[allowed], 10)]
        assert (rows[i] == top).all() and (bits(got[i]) == bits(s[top])).all(), i


# ---- 6. a model directory that says `ip` --------------------------------------------------------------------------------
def test_ip_model_directory_gives_the_scorer_calls_bits(tmp_path):
    from nann_amd import ops, retrieval
    c = _graph_case(128, "f16")
    path = str(tmp_path / "ip")
    ops.save_scorer_dir(path, "ip")
    m = ops.Model(path, 128)
    assert m.kind == "ip"
    sc = _scorer(128, "f16")
    seq = cuda(queries_for(c["g"], 12, seed=41))
    q = ops.user_seq_mean(seq)
    topn = [32] * 5 + [20]
    a, b = retrieval.search_model(c["dix"], m, seq, topn), retrieval.search(c["dix"], sc, q, topn)
    torch.cuda.synchronize()
    for x, y in zip(_np(a), _np(b)):
        assert (bits(x) == bits(y)).all() if x.dtype == np.float32 else (x == y).all()
    a, b = retrieval.search_all_model(c["dix"], m, seq, 50), retrieval.search_all(c["dix"], sc, q, 50)
    torch.cuda.synchronize()
    assert torch.equal(a.index, b.index) and torch.equal(a.item_ids, b.item_ids) and torch.equal(a.scores.view(torch.int32), b.scores.view(torch.int32))
    lists = [np.random.default_rng(i).integers(0, 20000, 40 + 30 * i) for i in range(12)]
    a = retrieval.search_candidates_model(c["dix"], m, seq, candidates=lists, k=50)
    b = retrieval.search_candidates(c["dix"], sc, q, candidates=lists, k=50)
    torch.cuda.synchronize()
    for f in ("index", "pos", "item_ids", "n_out", "status"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert torch.equal(a.scores.view(torch.int32), b.scores.view(torch.int32))
    rows = c["table"][:257]
    fw = m.forward(seq[:1], rows)
    bs = ops.blaze_score(sc, q[0], item_emb=rows)
    torch.cuda.synchronize()
    assert torch.equal(fw.reshape(-1).view(torch.int32), bs.view(torch.int32))
    assert (bits(bs.cpu().numpy()) == bits(R.ip_scores(q[0].cpu().numpy(), c["wide"][:257]))).all()


# ---- 7. the evaluation traversal refuses it -----------------------------------------------------------------------------
def test_search_eval_is_unimplemented_for_ip(tmp_path):
    from nann_amd import _lib, ops, retrieval
    from nann_amd.ops import _ptr, _stream
    c = _graph_case(64, "f16")
    sc = _scorer(64, "f16")
    with pytest.raises(ops.UnimplementedError) as e:
        retrieval.search_eval(c["dix"], sc, c["q"][:4], top_k_per_level=(40, 20, 10), topk_eval=10)
    assert e.value.status == 102 and "inner-product" in str(e.value)
    with pytest.raises(ops.UnimplementedError):
        retrieval.search_eval(c["dix"], sc, c["q"][:4], top_k_per_level=(40, 20, 10), topk_eval=10, want_counters=True)
    path = str(tmp_path / "ip")
    ops.save_scorer_dir(path, "ip")
    m = ops.Model(path, 64)
    seq = cuda(queries_for(c["g"], 4, seed=43))
    with pytest.raises(ops.UnimplementedError) as e:
        retrieval.search_eval(c["dix"], m, seq, top_k_per_level=(40, 20, 10), topk_eval=10)
    assert e.value.status == 102
    # nothing is written: the outputs and the workspace keep the pattern they were given
    L = _lib.lib()
    nb = C.c_int64(0)
    assert L.nann_search_eval_workspace_bytes(c["dix"].handle, m.handle, C.c_int64(4), C.byref(nb)) == 0
    ws = torch.full((nb.value,), 0x5a, dtype=torch.uint8, device="cuda")
    out_ids = torch.full((4, 10), -3, dtype=torch.int64, device="cuda")
    out_scores = torch.full((4, 10), -3.0, dtype=torch.float32, device="cuda")
    out_index = torch.full((4, 10), -3, dtype=torch.int32, device="cuda")
    n_out = torch.full((4,), -3, dtype=torch.int32, device="cuda")
    status = torch.full((4,), -3, dtype=torch.int32, device="cuda")
    ns, tk = (C.c_int32 * 3)(3, 1, 1), (C.c_int32 * 3)(40, 20, 10)
    for fn, handle, x in ((L.nann_search_eval, sc.handle, c["q"][:4].contiguous()), (L.nann_search_eval_model, m.handle, seq)):
        st = fn(c["dix"].handle, handle, _ptr(x), C.c_int64(4), ns, tk, C.c_int32(10), _ptr(ws), C.c_int64(ws.numel()), _ptr(out_ids),
                _ptr(out_scores), _ptr(out_index), _ptr(n_out), _ptr(status), _stream())
        torch.cuda.synchronize()
        assert st == 102
        assert (ws == 0x5a).all() and (out_ids == -3).all() and (out_scores == -3.0).all() and (out_index == -3).all()
        assert (n_out == -3).all() and (status == -3).all()


# ---- 8. L2 is untouched -------------------------------------------------------------------------------------------------
def test_l2_after_ip_on_shared_handles_still_equals_the_oracle(oracle):
    """one index, IP calls first, then the L2 scorer on the same handles: search, search_all and search_candidates against
    the oracle bit for bit"""
    from nann_amd import ops, retrieval
    from test_candidates_cpu import candidate_topk
    g, oix, dix = synth_index(20000, 64, 32)
    q = np.stack([oracle.user_seq_mean(s) for s in queries_for(g, 24, seed=51)])
    topn = [32] * 5 + [20]
    lists = [np.random.default_rng(i).integers(0, 20000, 300) for i in range(24)]
    ip, l2 = ops.Scorer("ip", 64), ops.Scorer("l2", 64)
    osc = oracle.Scorer("l2", 64, oracle.EMB_F16)
    r_ip = _np(_search(dix, ip, cuda(q), topn))
    retrieval.search_all(dix, ip, cuda(q), 20)
    retrieval.search_candidates(dix, ip, cuda(q), candidates=lists, k=20)
    got = _np(_search(dix, l2, cuda(q), topn))
    exp = oracle.search_batch(oix, osc, q, topn, n_threads=8)
    ok = exp[0] == 0
    assert (got[0] == exp[0]).all() and (got[1][ok] == exp[1][ok]).all() and (bits(got[2][ok]) == bits(exp[2][ok])).all() and \
        (got[3][ok] == exp[3][ok]).all() and (got[4][ok] == exp[4][ok]).all()
    assert (r_ip[3][ok] != got[3][ok]).any()
    ra = retrieval.search_all(dix, l2, cuda(q[:4]), 20)
    rc = retrieval.search_candidates(dix, l2, cuda(q[:4]), candidates=lists[:4], k=20)
    torch.cuda.synchronize()
    for i in range(4):
        st, bi, bv = oracle.brute_force(oix, osc, q[i], 20)
        assert st == 0 and (ra.index[i].cpu().numpy() == bi).all() and (bits(ra.scores[i].cpu().numpy()) == bits(bv)).all()
        pos, rows, s = candidate_topk(oracle, osc, q[i], g["item_embs"], lists[i], 20)
        assert (rc.pos[i].cpu().numpy() == pos).all() and (rc.index[i].cpu().numpy() == rows).all()
        assert (bits(rc.scores[i].cpu().numpy()) == bits(s)).all()
