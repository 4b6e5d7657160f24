"""-m gpu: exhaustive search on the device (nann_search_all / retrieval.search_all) against the CPU oracle's brute force
(oracle_brute_force: every row scored, TopKV2 sorted=true -- descending, ties -> lower row number).  Inputs are seeded and
generated here.  search_all never reads the graph; the indices these tests bring their own rows for carry a ring graph (every
node linked to its next eight, 64 enter points) so that nann_index_create sees a valid one."""
import ctypes as C
import os
import sys
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from gpu_util import bits, cuda, require_gpu, tolerant_parity

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


# ---- helpers -----------------------------------------------------------------------------------------------------------
def _ring(n, deg=8):
    deg = min(deg, n - 1)
    nbv = ((np.arange(n, dtype=np.int64)[:, None] + 1 + np.arange(deg)) % n).astype(np.int32).reshape(-1)
    rs = (np.arange(n + 1, dtype=np.int64) * deg)
    step = max(n // 64, 1)
    return [nbv, nbv.copy()], [rs, rs.copy()], np.arange(0, n, step, dtype=np.int32)[:64]


def _indices(embs, item_ids=None):
    """(oracle index, device index) over `embs` (f16 / f32 arrays, or uint16 bf16 bit patterns)"""
    from nann_amd import retrieval
    from oracle import oracle as O
    n = embs.shape[0]
    ids = (np.arange(n, dtype=np.int64) * 7 + 3) if item_ids is None else item_ids
    nbv, rs, ep = _ring(n)
    return O.Index(embs, ids, nbv, rs, ep), retrieval.Index(embs, ids, nbv, rs, ep)


def _rows(n, d, dtype, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    if dtype == "f32":
        return x
    if dtype == "f16":
        return x.astype(np.float16)
    return (x.view(np.uint32) >> 16).astype(np.uint16)  # bf16 bit patterns (truncated)


_TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def _oracle_dt(O, dtype):
    return {"f16": O.EMB_F16, "bf16": O.EMB_BF16, "f32": O.EMB_F32}[dtype]


def _brute(O, oix, osc, q, k, threads=16):
    """oracle.brute_force per query -> (rows i32[B, k], scores f32[B, k])"""
    def one(v):
        rc, bi, bv = O.brute_force(oix, osc, v, k)
        assert rc == 0
        return bi, bv
    with ThreadPoolExecutor(threads) as ex:  # (the oracle is a C call: the threads run side by side)
        out = list(ex.map(one, list(np.asarray(q, np.float32))))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _run(dix, scorer, q, k, options=None):
    from nann_amd import retrieval
    r = retrieval.search_all(dix, scorer, cuda(q, torch.float32), k, options=options)
    torch.cuda.synchronize()
    return r.index.cpu().numpy(), r.scores.cpu().numpy(), r.item_ids.cpu().numpy()


def _assert_bitwise(got, exp_rows, exp_scores, item_ids, what=""):
    rows, scores, ids = got
    assert (rows == exp_rows).all(), what
    assert (bits(scores) == bits(exp_scores)).all(), what
    assert (ids == item_ids[exp_rows]).all(), what


def _call_c(dix, scorer, q, k, out_ids, out_scores, out_index, ws, ws_bytes=None, n_queries=None, options=None):
    from nann_amd import _lib
    from nann_amd.ops import _ptr, _stream
    st = _lib.lib().nann_search_all(dix.handle, scorer.handle, _ptr(q), q.shape[0] if n_queries is None else n_queries, k,
                                    _ptr(out_ids), _ptr(out_scores), _ptr(out_index), _ptr(ws),
                                    (ws.numel() if ws is not None else 0) if ws_bytes is None else ws_bytes,
                                    C.byref(options) if options is not None else None, _stream())
    torch.cuda.synchronize()
    return st


def _ws_bytes(dix, scorer, n_queries, k):
    from nann_amd import _lib
    nb = C.c_int64(-1)
    st = _lib.lib().nann_search_all_workspace_bytes(dix.handle, scorer.handle, n_queries, k, C.byref(nb))
    return st, nb.value


# ---- 1. L2, bitwise, every d x row dtype ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("d", [64, 128, 256, 512])
def test_l2_bitwise_every_shape(oracle, d, dtype):
    from nann_amd import ops
    n = 20011
    embs = _rows(n, d, dtype, seed=d + len(dtype))
    oix, dix = _indices(embs)
    rng = np.random.default_rng(d)
    q = rng.standard_normal((33, d)).astype(np.float32)
    q[3] = _rows(1, d, "f32", seed=1)[0] * 0.25
    sc = ops.Scorer("l2", d, _TORCH_DT[dtype])
    osc = oracle.Scorer("l2", d, _oracle_dt(oracle, dtype))
    for k in (1, 10, 200, 1024):
        exp_rows, exp_scores = _brute(oracle, oix, osc, q, k)
        for b in (1, 7, 33):
            _assert_bitwise(_run(dix, sc, q[:b], k), exp_rows[:b], exp_scores[:b], oix.ids, (d, dtype, k, b))


# ---- 2. ties ----------------------------------------------------------------------------------------------------------
def _tie_corpus():
    if "tie" not in _CACHE:
        rng = np.random.default_rng(2024)
        n = 20011
        base = rng.standard_normal(((n + 2) // 3, 128)).astype(np.float16)
        embs = np.ascontiguousarray(np.tile(base, (3, 1))[rng.permutation(3 * base.shape[0])][:n])
        _CACHE["tie"] = (embs,) + _indices(embs)
    return _CACHE["tie"]


def test_ties_go_to_the_lower_row(oracle):
    from nann_amd import ops
    embs, oix, dix = _tie_corpus()
    q = embs[[5, 777, 10000, 20010, 12345]].astype(np.float32)
    sc, osc = ops.Scorer("l2", 128), oracle.Scorer("l2", 128, oracle.EMB_F16)
    for k in (1, 2, 4, 200, 1024):
        exp_rows, exp_scores = _brute(oracle, oix, osc, q, k)
        if k >= 4:  # the corpus does what it was built for: the query's own row three times (score +0), in row order
            assert (exp_scores[:, :2] == 0).all() and (np.diff(exp_rows[:, :2], axis=1) > 0).all()
        _assert_bitwise(_run(dix, sc, q, k), exp_rows, exp_scores, oix.ids, k)


# ---- 3. batch independence, empty calls -------------------------------------------------------------------------------
def test_answer_does_not_depend_on_the_batch(oracle):
    from nann_amd import ops
    embs, oix, dix = _tie_corpus()
    rng = np.random.default_rng(7)
    sc = ops.Scorer("l2", 128)
    probe = (embs[4242].astype(np.float32) + 0.01 * rng.standard_normal(128).astype(np.float32))
    alone = _run(dix, sc, probe[None], 200)
    exp_rows, exp_scores = _brute(oracle, oix, oracle.Scorer("l2", 128, oracle.EMB_F16), probe[None], 200)
    _assert_bitwise(alone, exp_rows, exp_scores, oix.ids)
    for b in (5, 64, 1027):
        for at in (0, b - 1, b // 2):
            q = rng.standard_normal((b, 128)).astype(np.float32)
            q[at] = probe
            rows, scores, ids = _run(dix, sc, q, 200)
            assert (rows[at] == alone[0][0]).all() and (bits(scores[at]) == bits(alone[1][0])).all(), (b, at)
            assert (ids[at] == alone[2][0]).all()


def test_empty_calls_write_nothing():
    from nann_amd import ops
    embs, oix, dix = _tie_corpus()
    sc = ops.Scorer("l2", 128)
    q = cuda(embs[:4].astype(np.float32))
    out_ids = torch.full((4, 8), -77, dtype=torch.int64, device="cuda")
    out_scores = torch.full((4, 8), -77.0, dtype=torch.float32, device="cuda")
    out_index = torch.full((4, 8), -77, dtype=torch.int32, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    assert _call_c(dix, sc, q, 8, out_ids, out_scores, out_index, ws, n_queries=0) == 0
    assert _call_c(dix, sc, q, 0, out_ids, out_scores, out_index, ws) == 0
    assert (out_ids == -77).all() and (out_scores == -77.0).all() and (out_index == -77).all()
    assert _ws_bytes(dix, sc, 0, 8) == (0, 0) and _ws_bytes(dix, sc, 4, 0) == (0, 0)


# ---- 4. edges ---------------------------------------------------------------------------------------------------------
def test_edges_k_equals_n_errors_null_outputs_nan(oracle):
    from nann_amd import _lib, ops
    sc, osc = ops.Scorer("l2", 64), oracle.Scorer("l2", 64, oracle.EMB_F16)
    embs = _rows(1000, 64, "f16", seed=3)
    oix, dix = _indices(embs)
    rng = np.random.default_rng(4)
    q = rng.standard_normal((5, 64)).astype(np.float32)
    exp_rows, exp_scores = _brute(oracle, oix, osc, q, 1000)
    _assert_bitwise(_run(dix, sc, q, 1000), exp_rows, exp_scores, oix.ids, "k = n")
    L = _lib.lib()
    assert _ws_bytes(dix, sc, 5, 1001)[0] == 4                       # TOPK_K_GT_N, as the oracle (k = n + 1 -> 4)
    assert oracle.brute_force(oix, osc, q[0], 1001)[0] == 4
    assert _ws_bytes(dix, sc, 5, -1)[0] == 7
    qd = cuda(q)
    out_ids = torch.full((5, 1001), -77, dtype=torch.int64, device="cuda")
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda")
    assert _call_c(dix, sc, qd, 1001, out_ids, None, None, ws) == 4 and b"at least k" in L.nann_last_error()
    assert _call_c(dix, sc, qd, -1, out_ids, None, None, ws) == 7
    assert (out_ids == -77).all()                                    # nothing launched
    # k > 1024 -> UNSUPPORTED (on a corpus that has that many rows)
    embs_t, oix_t, dix_t = _tie_corpus()
    sc_t = ops.Scorer("l2", 128)
    qt = cuda(embs_t[:2].astype(np.float32))
    assert _ws_bytes(dix_t, sc_t, 2, 1025)[0] == 102
    assert _call_c(dix_t, sc_t, qt, 1025, torch.empty((2, 1025), dtype=torch.int64, device="cuda"), None, None, ws) == 102
    # a workspace one byte short -> CAPACITY; exactly the reported size with NULL out_scores / out_index -> the answer
    st, nb = _ws_bytes(dix, sc, 5, 10)
    assert st == 0 and nb > 0
    ws2 = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    out10 = torch.full((5, 10), -77, dtype=torch.int64, device="cuda")
    assert _call_c(dix, sc, qd, 10, out10, None, None, ws2, ws_bytes=nb - 1) == 103
    assert (out10 == -77).all()
    assert _call_c(dix, sc, qd, 10, out10, None, None, ws2) == 0
    assert (out10.cpu().numpy() == oix.ids[exp_rows[:, :10]]).all()
    # a workspace off the 256-byte grid, a negative batch -> BAD_ARGUMENT, nothing written
    ws3 = torch.zeros(nb + 256, dtype=torch.uint8, device="cuda")
    out10.fill_(-77)
    assert _call_c(dix, sc, qd, 10, out10, None, None, ws3[8:], ws_bytes=nb) == 7 and b"aligned" in L.nann_last_error()
    assert _call_c(dix, sc, qd, 10, out10, None, None, ws2, n_queries=-1) == 7
    assert _ws_bytes(dix, sc, -1, 10)[0] == 7
    assert (out10 == -77).all()
    # a NaN query next to healthy ones: its rows are 0..k-1 (what the oracle returns), theirs do not change
    qn = q.copy()
    qn[2, 7] = np.nan
    rc, bi, _ = oracle.brute_force(oix, osc, qn[2], 10)
    assert rc == 0 and bi.tolist() == list(range(10))
    rows, scores, ids = _run(dix, sc, qn, 10)
    assert rows[2].tolist() == list(range(10)) and np.isnan(scores[2]).all()
    keep = [0, 1, 3, 4]
    assert (rows[keep] == exp_rows[keep, :10]).all() and (bits(scores[keep]) == bits(exp_scores[keep, :10])).all()


@pytest.mark.parametrize("n", [1, 63])
def test_tiny_corpora(oracle, n):
    from nann_amd import ops
    embs = _rows(n, 64, "f16", seed=n)
    oix, dix = _indices(embs)
    q = np.random.default_rng(n).standard_normal((3, 64)).astype(np.float32)
    sc, osc = ops.Scorer("l2", 64), oracle.Scorer("l2", 64, oracle.EMB_F16)
    for k in sorted({1, n}):
        exp_rows, exp_scores = _brute(oracle, oix, osc, q, k)
        _assert_bitwise(_run(dix, sc, q, k), exp_rows, exp_scores, oix.ids, (n, k))


# ---- 5 / 6. MLP -------------------------------------------------------------------------------------------------------
def _mlp_case(oracle, d, metric):
    """(embs, oracle index, device index, weights, queries f32[24, d], oracle rows, oracle scores) at n = 30 000, k = 200; the
    index carries a built graph (the fallback test also runs the traversal on it)"""
    key = ("mlp", d, metric)
    if key not in _CACHE:
        from gpu_util import queries_for, synth_index
        from nann_amd import synth
        g, oix, dix = synth_index(30000, d, 64)
        embs = g["item_embs"]
        w = synth.make_mlp_weights_metric(d, embs) if metric else synth.make_mlp_weights(d)
        q = np.stack([oracle.user_seq_mean(s) for s in queries_for(g, 24, seed=9)])
        exp = _brute(oracle, oix, oracle.Scorer("mlp", d, oracle.EMB_F16, w), q, 200)
        _CACHE[key] = (embs, oix, dix, w, q) + exp
    return _CACHE[key]


@pytest.mark.parametrize("metric", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_mlp_exact_and_certified_bitwise(oracle, d, metric):
    from nann_amd import ops, retrieval
    embs, oix, dix, w, q, exp_rows, exp_scores = _mlp_case(oracle, d, metric)
    exact = ops.Scorer("mlp", d, torch.float16, w, precision="exact")
    got_built_in_call = _run(dix, exact, q, 200)          # an unprepared pair: the table is built inside the call
    _assert_bitwise(got_built_in_call, exp_rows, exp_scores, oix.ids, "exact, table built in the call")
    cert = ops.Scorer("mlp", d, torch.float16, w, precision="certified")
    retrieval.prepare(dix, cert)                          # a pinned table is found
    try:
        got_cert = _run(dix, cert, q, 200)
    finally:
        retrieval.release(dix, cert)
    _assert_bitwise(got_cert, exp_rows, exp_scores, oix.ids, "certified, table prepared")
    assert all((a == b).all() for a, b in zip(map(bits, (got_cert[1],)), map(bits, (got_built_in_call[1],))))
    assert (got_cert[0] == got_built_in_call[0]).all()


def test_mlp_without_a_table(oracle):
    """options.preprojection = 0 -> NANN_ERR_UNSUPPORTED from the C call; with the process default off the harness falls back to
    the per-query loop and still gives the right figure"""
    from nann_amd import _lib, evaluate, ops, retrieval
    embs, oix, dix, w, q, exp_rows, exp_scores = _mlp_case(oracle, 64, False)
    sc = ops.Scorer("mlp", 64, torch.float16, w, precision="exact")
    with pytest.raises(ops.UnimplementedError) as e:
        _run(dix, sc, q[:2], 200, options=retrieval.search_options(preprojection=False))
    assert e.value.status == 102 and "preprojection" in str(e.value)
    topn = [64] * 5 + [200]
    qd = cuda(q[:6])
    on = evaluate.recall_vs_bruteforce(dix, sc, qd, topn, batched=True)
    L = _lib.lib()
    L.nann_set_preprojection(0)
    try:
        with pytest.raises(ops.UnimplementedError):
            _run(dix, sc, q[:2], 200)
        assert evaluate._search_all_or_none(dix, sc, qd, 200) is None   # (the loop it is, then)
        off = evaluate.recall_vs_bruteforce(dix, sc, qd, topn, batched=True)
        loop = evaluate.recall_vs_bruteforce(dix, sc, qd, topn)
    finally:
        L.nann_set_preprojection(1)
    assert 0.0 < on <= 1.0
    assert off == loop == on  # (the exact scorer: table or rows, loop or batch, the same ground truth and the same traversal)


@pytest.mark.parametrize("metric", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_mlp_split_within_tolerance(oracle, d, metric):
    from nann_amd import ops
    embs, oix, dix, w, q, exp_rows, exp_scores = _mlp_case(oracle, d, metric)
    rows, scores, ids = _run(dix, ops.Scorer("mlp", d, torch.float16, w, precision="split"), q, 200)
    verdicts = [tolerant_parity(rows[b], scores[b], exp_rows[b], exp_scores[b], rtol=1e-5) for b in range(len(q))]
    assert set(verdicts) <= {"exact", "near-tie"}, verdicts
    assert (ids == oix.ids[rows]).all()


# ---- 7 / 9. the existing device path, shards --------------------------------------------------------------------------
def _corpus_200k():
    if "200k" not in _CACHE:
        from nann_amd import synth
        embs, assign = synth.make_corpus(200_000, 128, seed=31)
        _CACHE["200k"] = (embs, assign) + _indices(embs)
    return _CACHE["200k"]


def test_equals_the_per_query_device_loop():
    from nann_amd import ops, synth
    embs, assign, oix, dix = _corpus_200k()
    q = ops.user_seq_mean(cuda(synth.make_queries(embs, assign, 64, seed=5)))
    sc = ops.Scorer("l2", 128)
    rows, scores, ids = _run(dix, sc, q.cpu().numpy(), 200)
    for b in range(64):
        v, i = ops.top_k(ops.blaze_score(sc, q[b], item_emb=dix.item_embs), 200)
        assert (i.cpu().numpy() == rows[b]).all() and (bits(v.cpu().numpy()) == bits(scores[b])).all(), b
    assert (ids == oix.ids[rows]).all()


def test_shards_merge_to_the_whole():
    """per-shard search_all + nann_merge_topk = search_all over the whole corpus: the outputs are what nann_sharded_topk takes"""
    from nann_amd import _lib, ops, synth
    from nann_amd.ops import _ptr, _stream
    embs, assign, oix, dix = _corpus_200k()
    q = ops.user_seq_mean(cuda(synth.make_queries(embs, assign, 16, seed=6))).cpu().numpy()
    sc = ops.Scorer("l2", 128)
    k = 200
    rows, scores, ids = _run(dix, sc, q, k)
    cut = [0, 50_000, 100_000, 150_000, 200_000]
    sh_scores = torch.empty((16, 4, k), dtype=torch.float32, device="cuda")
    sh_ids = torch.empty((16, 4, k), dtype=torch.int64, device="cuda")
    for s in range(4):
        _, sdix = _indices(np.ascontiguousarray(embs[cut[s]:cut[s + 1]]), oix.ids[cut[s]:cut[s + 1]])
        _, sscores, sids = _run(sdix, sc, q, k)
        sh_scores[:, s] = cuda(sscores)
        sh_ids[:, s] = cuda(sids)
    out_scores = torch.empty((16, k), dtype=torch.float32, device="cuda")
    out_ids = torch.empty((16, k), dtype=torch.int64, device="cuda")
    assert _lib.lib().nann_merge_topk(_ptr(sh_scores), _ptr(sh_ids), C.c_int64(16), C.c_int32(4), C.c_int32(k), C.c_int32(k),
                                      _ptr(out_scores), _ptr(out_ids), _stream()) == 0
    torch.cuda.synchronize()
    assert (out_ids.cpu().numpy() == ids).all() and (bits(out_scores.cpu().numpy()) == bits(scores)).all()


# ---- 8. the headline shape --------------------------------------------------------------------------------------------
def test_headline_shape_1m(oracle):
    # (1M rows still give a chunk of kScanMaxChunk = 128 queries; the byte-limited chunk: test_zz_search_all_big_gpu.py)
    import bench
    from nann_amd import ops, retrieval
    from oracle import oracle as O
    g = bench.make_index(1_000_000, 128, 128, "hnsw", 1.0, "f16", 0, torch.device("cuda"), bench.usable_cores(),
                         cache_dir=os.environ.get("NANN_TEST_INDEX_CACHE"))
    oix = O.Index(g["item_embs"], g["item_ids"], g["nb_values"], g["nb_row_splits"], g["enter_points"])
    dix = retrieval.Index.from_dict(g)
    seq = bench.make_query_batches(128, 256, 1, 1.0, torch.device("cuda"), seed=4321,
                                   n_clusters=bench.n_clusters_for(1_000_000, 128))[0]
    q = ops.user_seq_mean(seq)
    sc = ops.Scorer("l2", 128)
    k = 200
    st, nb1024 = _ws_bytes(dix, sc, 1024, k)
    assert st == 0 and 0 < nb1024 < (1 << 30)
    st, nb = _ws_bytes(dix, sc, 256, k)
    assert st == 0 and 0 < nb < (1 << 30)
    page = 4096
    buf = torch.full((nb + page,), 0xA5, dtype=torch.uint8, device="cuda")  # exactly the reported size + a canary page
    out_ids = torch.empty((256, k), dtype=torch.int64, device="cuda")
    out_scores = torch.empty((256, k), dtype=torch.float32, device="cuda")
    out_index = torch.empty((256, k), dtype=torch.int32, device="cuda")
    assert _call_c(dix, sc, q, k, out_ids, out_scores, out_index, buf, ws_bytes=nb) == 0
    assert (buf[nb:] == 0xA5).all(), "the call wrote behind its workspace"
    rows, scores, ids = out_index.cpu().numpy(), out_scores.cpu().numpy(), out_ids.cpu().numpy()
    sample = [0, 85, 170, 255]
    exp_rows, exp_scores = _brute(oracle, oix, oracle.Scorer("l2", 128, oracle.EMB_F16), q[sample].cpu().numpy(), k, threads=4)
    assert (rows[sample] == exp_rows).all() and (bits(scores[sample]) == bits(exp_scores)).all()
    assert (ids == oix.ids[rows]).all()
    for b in range(16, 32):
        v, i = ops.top_k(ops.blaze_score(sc, q[b], item_emb=dix.item_embs), k)
        assert (i.cpu().numpy() == rows[b]).all() and (bits(v.cpu().numpy()) == bits(scores[b])).all(), b
    # k = 1024 on 62 slabs: the merge sees 63 488 candidates, more than wg_topk keeps in registers (its form that re-reads the
    # keys from memory, with row numbers and the id map riding along); against the per-query device loop and the oracle
    rows, scores, ids = _run(dix, sc, q[:6].cpu().numpy(), 1024)
    for b in range(6):
        v, i = ops.top_k(ops.blaze_score(sc, q[b], item_emb=dix.item_embs), 1024)
        assert (i.cpu().numpy() == rows[b]).all() and (bits(v.cpu().numpy()) == bits(scores[b])).all(), b
    exp_rows, exp_scores = _brute(oracle, oix, oracle.Scorer("l2", 128, oracle.EMB_F16), q[:2].cpu().numpy(), 1024, threads=2)
    assert (rows[:2] == exp_rows).all() and (bits(scores[:2]) == bits(exp_scores)).all()
    assert (ids == oix.ids[rows]).all()


# ---- 10. the recall harness -------------------------------------------------------------------------------------------
def test_harness_batched_equals_unbatched(oracle, tmp_path):
    from gpu_util import queries_for, synth_index
    from nann_amd import evaluate, ops, synth
    g, oix, dix = synth_index(20000, 64, 32)
    seqs = queries_for(g, 24, seed=3)
    sc = ops.Scorer("l2", 64)
    truths = []
    for s in seqs:
        qv = ops.user_seq_mean(cuda(s)[None])[0]
        _, bi = ops.top_k(ops.blaze_score(sc, qv, item_emb=dix.item_embs), 1)
        truths.append(int(dix.item_ids[bi.long()].cpu()[0]))
    loop = evaluate.test_all(dix, sc, seqs, truths, topk_eval=(10, 50))
    batch = evaluate.test_all(dix, sc, seqs, truths, topk_eval=(10, 50), batched=True)
    assert batch["recall"][10].avg == 1.0
    for m in ("precision", "recall", "f1"):
        for k in (10, 50):
            assert (batch[m][k].sum, batch[m][k].count) == (loop[m][k].sum, loop[m][k].count), (m, k)
    q = ops.user_seq_mean(cuda(seqs))
    topn = [32] * 5 + [20]
    assert evaluate.recall_vs_bruteforce(dix, sc, q, topn, batched=True) == evaluate.recall_vs_bruteforce(dix, sc, q, topn)
    # an l2 ops.Model takes comm_seq and gives the scorer's answer; an attention model takes the loop either way
    from nann_amd import retrieval
    ops.save_scorer_dir(str(tmp_path / "l2"), "l2")
    m_l2 = ops.Model(str(tmp_path / "l2"), 64, seq_len=seqs.shape[1])
    r_m = retrieval.search_all(dix, m_l2, cuda(seqs), 50)
    r_s = retrieval.search_all(dix, sc, q, 50)
    torch.cuda.synchronize()
    assert (r_m.index == r_s.index).all() and (r_m.scores.view(torch.int32) == r_s.scores.view(torch.int32)).all()
    ops.save_scorer_dir(str(tmp_path / "attn"), "attention", synth.make_attn_weights(64), precision="exact")
    m_at = ops.Model(str(tmp_path / "attn"), 64, seq_len=seqs.shape[1])
    with pytest.raises(NotImplementedError):
        retrieval.search_all(dix, m_at, cuda(seqs), 50)
    a_loop = evaluate.test_all(dix, m_at, seqs[:4], truths[:4], topk_eval=(10,))
    a_batch = evaluate.test_all(dix, m_at, seqs[:4], truths[:4], topk_eval=(10,), batched=True)
    assert all((a_batch[m][10].sum, a_batch[m][10].count) == (a_loop[m][10].sum, a_loop[m][10].count)
               for m in ("precision", "recall", "f1"))


# ---- 11. two threads, one index, one MLP scorer ------------------------------------------------------------------------
def test_two_threads_share_index_and_scorer(oracle):
    from nann_amd import ops, retrieval
    embs, oix, dix, w, q, exp_rows, exp_scores = _mlp_case(oracle, 64, False)
    sc = ops.Scorer("mlp", 64, torch.float16, w, precision="exact")  # unprepared: the threads race for the table's build
    halves = [q[:12], q[12:]]
    got, errors = [None, None], []
    start = threading.Barrier(2)

    def work(i):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                qd = cuda(halves[i], torch.float32)
                start.wait()
                for _ in range(3):
                    r = retrieval.search_all(dix, sc, qd, 200)
                stream.synchronize()
                got[i] = (r.index.cpu().numpy(), r.scores.cpu().numpy(), r.item_ids.cpu().numpy())
        except Exception as e:  # noqa: BLE001 -- reported by the asserting thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    _assert_bitwise(got[0], exp_rows[:12], exp_scores[:12], oix.ids, "thread 0")
    _assert_bitwise(got[1], exp_rows[12:], exp_scores[12:], oix.ids, "thread 1")
