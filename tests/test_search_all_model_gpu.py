"""-m gpu: exhaustive search under a model (nann_search_all_model / retrieval.search_all_model) -- the reference's test_all job
with the model it scores, attention + DNN 128-64-32-1 -- against the CPU oracle's brute force (oracle_brute_force with the
attention scorer: every row through oracle_attn_score_rows, then TopKV2 sorted=true).  Inputs are seeded and generated here:
n = 20 000 rows, synth.make_attn_weights(d, 64), synth.make_queries(.., seq_len=50) (the model's sequence is [L, 64]: at
d = 128 the first 64 columns of a history row), k = 200.  The scan never reads the graph; the corpora these tests bring their
own rows for carry a ring graph.  The device scores every row within 1e-5 max(1, |s|) of the oracle (the contract of every
attention-scorer test), so a device list equals the oracle's up to near-ties: tolerant_parity "exact" or "near-tie", never
"diverged"."""
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
L_SEQ, K, RTOL = 50, 200, 1e-5


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


def _seq64(seqs):
    """the attention model's comm_seq f16[B, L, 64] from histories of d-wide rows"""
    return np.ascontiguousarray(seqs[:, :, :64])


def _corpus(n, d, rows="f16", seed=77):
    """(host rows, oracle index, device index, oracle dtype code, torch dtype, users f16[16, 50, 64]) over a clustered corpus
    with a ring graph"""
    key = ("corpus", n, d, rows, seed)
    if key not in _CACHE:
        from nann_amd import retrieval, synth
        from oracle import oracle as O
        embs, assign = synth.make_corpus(n, d, n_clusters=min(64, max(n // 8, 1)), noise=1.0, seed=seed)
        ids = np.arange(n, dtype=np.int64) * 7 + 3
        nbv, rs, ep = _ring(n)
        seqs = _seq64(synth.make_queries(embs, assign, 16, seq_len=L_SEQ, seed=seed + 1))
        if rows == "bf16":
            dev = cuda(embs.astype(np.float32)).to(torch.bfloat16)
            host = dev.view(torch.int16).cpu().numpy().view(np.uint16)
            _CACHE[key] = (host, O.Index(host, ids, nbv, rs, ep), retrieval.Index(dev, ids, nbv, rs, ep), O.EMB_BF16,
                           torch.bfloat16, seqs)
        else:
            _CACHE[key] = (embs, O.Index(embs, ids, nbv, rs, ep), retrieval.Index(embs, ids, nbv, rs, ep), O.EMB_F16,
                           torch.float16, seqs)
    return _CACHE[key]


def _weights(d):
    from nann_amd import synth
    return synth.make_attn_weights(d, 64)


def _model(tmp_path, d, precision, tdt=torch.float16, name=None):
    from nann_amd import ops
    path = str(tmp_path / (name or ("attn_%s_%d" % (precision, d))))
    ops.save_scorer_dir(path, "attention", _weights(d), precision=precision)
    return ops.Model(path, d, L_SEQ, emb_dtype=tdt)


def _oracle_scorer(O, d, code):
    am = O.AttnModel(d, 64, L_SEQ, code, _weights(d))
    return O.Scorer("attention", d, code, attn_model=am), am


def _brute(O, oix, osc, seqs, k, threads=16):
    """oracle.brute_force per user -> (rows i32[B, k], scores f32[B, k])"""
    def one(s):
        rc, bi, bv = O.brute_force(oix, osc, s.astype(np.float32).ravel(), k)
        assert rc == 0
        return bi, bv
    with ThreadPoolExecutor(threads) as ex:  # (the oracle is a C call: the threads run side by side)
        out = list(ex.map(one, list(seqs)))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _run(dix, model, seqs, k, options=None):
    from nann_amd import retrieval
    r = retrieval.search_all_model(dix, model, cuda(seqs, torch.float16), k, options=options)
    torch.cuda.synchronize()
    return r.index.cpu().numpy(), r.scores.cpu().numpy(), r.item_ids.cpu().numpy()


def _sorted_by_own_scores(rows, scores):
    """descending by score (-0 = +0), ties -> lower row"""
    s = scores + np.float32(0.0)
    return all((s[i] > s[i + 1]) or (s[i] == s[i + 1] and rows[i] < rows[i + 1]) for i in range(len(rows) - 1))


def _call_c(dix, model, seq, k, out_ids, out_scores, out_index, ws, ws_bytes=None, n_users=None, options=None):
    from nann_amd import _lib
    from nann_amd.ops import _ptr, _stream
    st = _lib.lib().nann_search_all_model(dix.handle, model.handle, _ptr(seq), seq.shape[0] if n_users is None else n_users, k,
                                          _ptr(out_ids), _ptr(out_scores), _ptr(out_index), _ptr(ws),
                                          (ws.numel() if ws is not None else 0) if ws_bytes is None else ws_bytes,
                                          C.byref(options) if options is not None else None, _stream())
    torch.cuda.synchronize()
    return st


def _ws_bytes(dix, model, n_users, k):
    from nann_amd import _lib
    nb = C.c_int64(-1)
    st = _lib.lib().nann_search_all_model_workspace_bytes(dix.handle, model.handle, n_users, k, C.byref(nb))
    return st, nb.value


# ---- 1. parity with the oracle's brute force --------------------------------------------------------------------------
@pytest.mark.parametrize("d,precision,rows", [(64, "split", "f16"), (64, "exact", "f16"), (128, "split", "f16"),
                                              (128, "exact", "f16"), (64, "split", "bf16")])
def test_parity_with_the_oracle(oracle, tmp_path, d, precision, rows):
    host, oix, dix, code, tdt, seqs = _corpus(20000, d, rows)
    osc, am = _oracle_scorer(oracle, d, code)
    exp_rows, exp_scores = _brute(oracle, oix, osc, seqs, K)
    got_rows, got_scores, got_ids = _run(dix, _model(tmp_path, d, precision, tdt), seqs, K)
    verdicts = []
    for u in range(len(seqs)):
        verdicts.append(tolerant_parity(got_rows[u], got_scores[u], exp_rows[u], exp_scores[u], rtol=RTOL))
        rc, own = oracle.attn_score_rows(am, seqs[u].astype(np.float32), host[got_rows[u]])
        assert rc == 0
        err = np.abs(got_scores[u] - own) / np.maximum(1.0, np.abs(own))
        print("user %d: %s, max score error on the returned rows %.3g" % (u, verdicts[-1], err.max()))
        assert (err <= RTOL).all(), (u, float(err.max()))
        assert _sorted_by_own_scores(got_rows[u], got_scores[u]), u
    assert set(verdicts) <= {"exact", "near-tie"}, verdicts
    assert (got_ids == oix.ids[got_rows]).all()


# ---- 2. the selection is a top-k of the device's own scores -----------------------------------------------------------
@pytest.mark.parametrize("precision", ["split", "exact"])
def test_selection_is_topk_of_the_devices_own_scores(tmp_path, precision):
    host, oix, dix, code, tdt, seqs = _corpus(1000, 64)
    m = _model(tmp_path, 64, precision)
    all_rows, all_scores, _ = _run(dix, m, seqs[:5], 1000)   # k = n: every row's score, sorted
    for u in range(5):
        assert sorted(all_rows[u].tolist()) == list(range(1000)) and _sorted_by_own_scores(all_rows[u], all_scores[u])
    rows, scores, ids = _run(dix, m, seqs[:5], 50)
    assert (rows == all_rows[:, :50]).all() and (bits(scores) == bits(all_scores[:, :50])).all()
    assert (ids == oix.ids[rows]).all()


# ---- 3. batch independence --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["split", "exact"])
def test_answer_does_not_depend_on_the_batch(tmp_path, precision):
    from nann_amd import synth
    host, oix, dix, code, tdt, seqs = _corpus(20000, 64)
    m = _model(tmp_path, 64, precision)
    probe = seqs[3]
    alone = _run(dix, m, probe[None], K)
    filler = _seq64(synth.make_queries(host, np.zeros(len(host), np.int32), 130, seq_len=L_SEQ, seed=5))
    for b, at in ((3, 1), (130, 129)):   # 130 users cross the 128-user chunk
        batch = filler[:b].copy()
        batch[at] = probe
        rows, scores, ids = _run(dix, m, batch, K)
        assert (rows[at] == alone[0][0]).all() and (bits(scores[at]) == bits(alone[1][0])).all(), (b, at)
        assert (ids[at] == alone[2][0]).all()


# ---- 4. the same bits as the traversal --------------------------------------------------------------------------------
def test_same_bits_as_the_traversal(tmp_path):
    from gpu_util import queries_for, synth_index
    from nann_amd import retrieval
    g, oix, dix = synth_index(20000, 64, 32)
    seqs = _seq64(queries_for(g, 16, seed=17))
    m = _model(tmp_path, 64, "split")
    r = retrieval.search_model(dix, m, cuda(seqs), [32] * 5 + [20])
    torch.cuda.synchronize()
    st, t_rows, t_scores = r.status.cpu().numpy(), r.index.cpu().numpy(), r.scores.cpu().numpy()
    rows, scores, _ = _run(dix, m, seqs, K)
    assert (st == 0).sum() >= 8, st
    for u in np.nonzero(st == 0)[0]:
        scan = {int(i): s for i, s in zip(rows[u], bits(scores[u]))}
        common = [(int(i), s) for i, s in zip(t_rows[u], bits(t_scores[u])) if int(i) in scan]
        assert len(common) >= 1, u
        assert all(scan[i] == s for i, s in common), (u, [(i, hex(s), hex(scan[i])) for i, s in common if scan[i] != s][:4])


# ---- 5. edges ---------------------------------------------------------------------------------------------------------
def test_contract_errors_and_no_ops(tmp_path):
    from nann_amd import _lib, ops, retrieval
    L = _lib.lib()
    host, oix, dix, code, tdt, seqs = _corpus(1000, 64)
    m = _model(tmp_path, 64, "split")
    seq = cuda(seqs[:4], torch.float16)
    out_ids = torch.full((4, 1001), -77, dtype=torch.int64, device="cuda")
    out_scores = torch.full((4, 1001), -77.0, dtype=torch.float32, device="cuda")
    out_index = torch.full((4, 1001), -77, dtype=torch.int32, device="cuda")
    ws = torch.zeros(1 << 25, dtype=torch.uint8, device="cuda")
    # k < 0, n_users < 0 -> BAD_ARGUMENT; k > n_items -> TOPK_K_GT_N; k == 0 or n_users == 0 -> OK; nothing written by any of them
    assert _ws_bytes(dix, m, 4, -1)[0] == 7 and _ws_bytes(dix, m, -1, 10)[0] == 7
    assert _call_c(dix, m, seq, -1, out_ids, out_scores, out_index, ws) == 7
    assert _call_c(dix, m, seq, 10, out_ids, out_scores, out_index, ws, n_users=-1) == 7
    assert _ws_bytes(dix, m, 4, 1001)[0] == 4
    assert _call_c(dix, m, seq, 1001, out_ids, out_scores, out_index, ws) == 4 and b"at least k" in L.nann_last_error()
    assert _call_c(dix, m, seq, 10, out_ids, out_scores, out_index, ws, n_users=0) == 0
    assert _call_c(dix, m, seq, 0, out_ids, out_scores, out_index, ws) == 0
    assert _ws_bytes(dix, m, 0, 8) == (0, 0) and _ws_bytes(dix, m, 4, 0) == (0, 0)
    assert (out_ids == -77).all() and (out_scores == -77.0).all() and (out_index == -77).all()
    # k > 1024 -> UNSUPPORTED (on a corpus that has that many rows)
    host_b, oix_b, dix_b, _, _, seqs_b = _corpus(4097, 64)
    assert _ws_bytes(dix_b, m, 2, 1025)[0] == 102
    assert _call_c(dix_b, m, cuda(seqs_b[:2], torch.float16), 1025, torch.empty((2, 1025), dtype=torch.int64, device="cuda"),
                   None, None, ws) == 102
    # model and index disagree on d -> BAD_ARGUMENT
    m128 = _model(tmp_path, 128, "split")
    assert _ws_bytes(dix, m128, 4, 10)[0] == 7 and b"disagree" in L.nann_last_error()
    assert _call_c(dix, m128, seq, 10, out_ids, None, None, ws) == 7
    # a workspace one byte short -> CAPACITY; off the 256-byte grid -> BAD_ARGUMENT; nothing written
    st, nb = _ws_bytes(dix, m, 4, 10)
    assert st == 0 and nb > 0
    ws2 = torch.zeros(nb + 256, dtype=torch.uint8, device="cuda")
    out10 = torch.full((4, 10), -77, dtype=torch.int64, device="cuda")
    assert _call_c(dix, m, seq, 10, out10, None, None, ws2, ws_bytes=nb - 1) == 103
    assert _call_c(dix, m, seq, 10, out10, None, None, ws2[8:], ws_bytes=nb) == 7 and b"aligned" in L.nann_last_error()
    assert (out10 == -77).all()
    # preprojection = 0 -> UNSUPPORTED, with the reason in the last error
    off = retrieval.search_options(preprojection=False)
    assert _call_c(dix, m, seq, 10, out10, None, None, ws2, ws_bytes=nb, options=off) == 102
    assert b"preprojection" in L.nann_last_error()
    with pytest.raises(ops.NannError) as e:
        _run(dix, m, seqs[:2], 10, options=off)
    assert e.value.status == 102 and "preprojection" in str(e.value)
    assert (out10 == -77).all()
    # exactly the reported size, out_scores / out_index NULL -> the answer
    assert _call_c(dix, m, seq, 10, out10, None, None, ws2, ws_bytes=nb) == 0
    rows, _, ids = _run(dix, m, seqs[:4], 10)
    assert (out10.cpu().numpy() == ids).all() and (ids == oix.ids[rows]).all()
    # an ops.Scorer is search_all's
    with pytest.raises(TypeError):
        retrieval.search_all_model(dix, ops.Scorer("l2", 64), seq, 10)


@pytest.mark.parametrize("precision", ["split", "exact"])
@pytest.mark.parametrize("n", [1, 63, 4097])
def test_small_corpora(oracle, tmp_path, n, precision):
    """n = 1, 63 (less than a 32-row block pair, a corpus no larger than k with k = n) and 4097 (one row into a second block)"""
    host, oix, dix, code, tdt, seqs = _corpus(n, 64)
    osc, am = _oracle_scorer(oracle, 64, code)
    k = min(n, K)
    exp_rows, exp_scores = _brute(oracle, oix, osc, seqs[:3], k)
    rows, scores, ids = _run(dix, _model(tmp_path, 64, precision), seqs[:3], k)
    for u in range(3):
        assert tolerant_parity(rows[u], scores[u], exp_rows[u], exp_scores[u], rtol=RTOL) in ("exact", "near-tie"), (n, u)
        rc, own = oracle.attn_score_rows(am, seqs[u].astype(np.float32), host[rows[u]])
        assert rc == 0 and (np.abs(scores[u] - own) <= RTOL * np.maximum(1.0, np.abs(own))).all()
        assert _sorted_by_own_scores(rows[u], scores[u])
    assert (ids == oix.ids[rows]).all()


# ---- 6. l2 and mlp models: the bits of search_all ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["l2", "mlp"])
def test_l2_and_mlp_models_equal_search_all(tmp_path, kind):
    from nann_amd import ops, retrieval, synth
    host, oix, dix, code, tdt, _ = _corpus(20000, 64)
    seqs = synth.make_queries(host, np.zeros(len(host), np.int32), 9, seq_len=L_SEQ, seed=8)  # [9, 50, 64]
    ops.save_scorer_dir(str(tmp_path / kind), kind, synth.make_mlp_weights(64) if kind == "mlp" else None,
                        precision=None if kind == "l2" else "exact")
    m = ops.Model(str(tmp_path / kind), 64, L_SEQ)
    rows, scores, ids = _run(dix, m, seqs, K)
    r = retrieval.search_all(dix, m, cuda(seqs), K)
    torch.cuda.synchronize()
    assert (rows == r.index.cpu().numpy()).all() and (bits(scores) == bits(r.scores.cpu().numpy())).all()
    assert (ids == r.item_ids.cpu().numpy()).all()


# ---- 7. lifecycle of the table ----------------------------------------------------------------------------------------
def _table_bytes(model, dix):
    from nann_amd import _lib
    tb, rb = C.c_int64(-1), C.c_int64(-1)
    assert _lib.lib().nann_model_table_bytes(model.handle, dix.handle, C.byref(tb), C.byref(rb)) == 0
    return tb.value, rb.value


@pytest.mark.parametrize("precision", ["split", "exact"])
def test_table_built_in_the_call_or_prepared(tmp_path, precision):
    from nann_amd import retrieval
    host, oix, dix, code, tdt, seqs = _corpus(20000, 64)
    m = _model(tmp_path, 64, precision)
    built_in_call = _run(dix, m, seqs[:6], K)             # an unprepared pair: the table is built inside the call
    m2 = _model(tmp_path, 64, precision, name="again")
    retrieval.prepare(dix, m2)                            # a pinned table is found
    try:
        before = _table_bytes(m2, dix)
        assert before[0] == 20000 * 384 * 4 and before[1] >= before[0]
        prepared = _run(dix, m2, seqs[:6], K)
        assert _table_bytes(m2, dix) == before
    finally:
        retrieval.release(dix, m2)
    assert (prepared[0] == built_in_call[0]).all() and (bits(prepared[1]) == bits(built_in_call[1])).all()


def test_two_threads_share_index_and_model(tmp_path):
    from nann_amd import retrieval
    host, oix, dix, code, tdt, seqs = _corpus(20000, 64)
    ref = _run(dix, _model(tmp_path, 64, "split", name="ref"), seqs, K)
    m = _model(tmp_path, 64, "split", name="shared")  # unprepared: the threads race for the table's build
    halves = [seqs[:8], seqs[8:]]
    got, errors = [None, None], []
    start = threading.Barrier(2)

    def work(i):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                sd = cuda(halves[i], torch.float16)
                start.wait()
                for _ in range(3):
                    r = retrieval.search_all_model(dix, m, sd, K)
                stream.synchronize()
                got[i] = (r.index.cpu().numpy(), r.scores.cpu().numpy())
        except Exception as e:  # noqa: BLE001 -- reported by the asserting thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i, sl in enumerate((slice(0, 8), slice(8, 16))):
        assert (got[i][0] == ref[0][sl]).all() and (bits(got[i][1]) == bits(ref[1][sl])).all(), i


# ---- 8. the recall harness --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["split", "exact"])
def test_harness_model_scan(oracle, tmp_path, precision):
    from nann_amd import _lib, evaluate
    host, oix, dix, code, tdt, seqs = _corpus(20000, 64)
    osc, _ = _oracle_scorer(oracle, 64, code)
    top1, _ = _brute(oracle, oix, osc, seqs[:8], 1)
    truths = [int(oix.ids[r[0]]) for r in top1]
    m = _model(tmp_path, 64, precision)
    us = seqs[:8]
    scan = evaluate.test_all(dix, m, us, truths, topk_eval=(10,), batched=True, model_scan=True)
    assert scan["recall"][10].avg == 1.0
    assert evaluate._search_all_or_none(dix, m, cuda(us), 10) is None          # the default: the loop, as before
    assert evaluate._search_all_or_none(dix, m, cuda(us), 10, model_scan=True) is not None
    L = _lib.lib()
    L.nann_set_preprojection(0)
    try:
        assert evaluate._search_all_or_none(dix, m, cuda(us), 10, model_scan=True) is None   # (the loop it is, then)
        loop = evaluate.test_all(dix, m, us, truths, topk_eval=(10,), batched=True, model_scan=True)
    finally:
        L.nann_set_preprojection(1)
    for name in ("precision", "recall", "f1"):
        assert (loop[name][10].sum, loop[name][10].count) == (scan[name][10].sum, scan[name][10].count), name
