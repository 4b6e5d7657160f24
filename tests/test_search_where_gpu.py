"""-m gpu: the four searches under attribute predicates, bitwise against the numpy model (predicate_model) applied to the output
of an existing, unchanged call.
  search_all_where / search_all_model_where: the model over the FULL ranking -- retrieval.search_all / search_all_model at
    k = n_items where n_items <= 1 024, ops.blaze_score (nann_score) plus a stable sort, ties to the lower row, beyond it.
    L2 and IP, f16 and bf16 rows, one MLP scorer and the attention model; a batch of one chunk + 1 queries, so that a second
    chunk's queries are addressed by their number in the call.
  search_where / search_model_where: the model over retrieval.search / search_model at the same level_topn (2 000 rows on the
    shipped builder's graph, F = 50): per-query level_topn, a failed query, k < F."""
import os
import re

import numpy as np
import pytest
import torch

import predicate_cases as PC
import predicate_model as PM
from gpu_util import bits, cuda, queries_for, require_gpu, synth_index
from test_search_all_gpu import _indices, _rows

pytestmark = pytest.mark.gpu
D, K = 64, 200
N_SMALL = 1000
N, F = 2000, 50
TOPN = [8, 16, 32, 32, 32, F]
L_SEQ = 8
_CACHE = {}


def _const(header, name):
    from nann_amd import build
    src = open(os.path.join(build.SRC_DIR, header)).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


CHUNK = _const("nann_scan.h", "kScanMaxChunk")      # most queries scored per chunk
TILE = _const("nann_predicate.h", "kPredTileRows")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _got(r):
    torch.cuda.synchronize()
    return {"item_ids": r.item_ids.cpu().numpy(), "scores": r.scores.cpu().numpy(), "index": r.index.cpu().numpy(),
            "n_out": r.n_out.cpu().numpy()}


def _same(got, exp, what=""):
    for name in ("n_out", "index", "item_ids", "scores"):
        g, e = (bits(got[name]), bits(exp[name])) if name == "scores" else (got[name], exp[name])
        assert g.shape == e.shape and (g == e).all(), (what, name)


def _small(dtype):
    if dtype not in _CACHE:
        _CACHE[dtype] = _indices(_rows(N_SMALL, D, dtype, seed=61))[1]
    return _CACHE[dtype]


def _case(n, n_q, seed):
    """(predicate dict, filter) for n_q queries over n rows: deny bitmap and exclusion lists included"""
    rng = np.random.default_rng(seed)
    return PC.make(rng, n, n_q, 7), PC.make_filter(rng, n, n_q)


def _check_exhaustive(dix, full, call, n_q, seed, what):
    """full: retrieval result of the unfiltered call at k = n_items; call(predicates, filter) -> the _where result at K"""
    torch.cuda.synchronize()
    n = int(dix.n_items)
    rows, scores = full.index.cpu().numpy(), full.scores.cpu().numpy()
    pred, flt = _case(n, n_q, seed)
    exp = PM.where_topk(rows, scores, None, flt, pred, K, n, item_ids=dix.item_ids.cpu().numpy())
    p, f = PC.on_device(dix, pred, n_q, flt)
    got = _got(call(p, f))
    _same(got, exp, what)
    assert (exp["n_out"] == PM.count(pred, flt, n_q, n).clip(max=K)).all()           # n_out = min(k, passing rows)
    assert (exp["n_out"] == 0).any() and ((exp["n_out"] > 0) & (exp["n_out"] < K)).any() and (exp["n_out"] == K).any()
    # ... and without a filter
    exp = PM.where_topk(rows, scores, None, None, pred, K, n, item_ids=dix.item_ids.cpu().numpy())
    _same(_got(call(p, None)), exp, (what, "unfiltered"))
    return pred, flt, p, f


@pytest.mark.parametrize("metric,dtype", [("l2", "f16"), ("ip", "f16"), ("l2", "bf16"), ("ip", "bf16")])
def test_search_all_where_is_the_model_over_the_full_ranking(metric, dtype):
    from nann_amd import ops, retrieval
    dix = _small(dtype)
    sc = ops.Scorer(metric, D, {"f16": torch.float16, "bf16": torch.bfloat16}[dtype])
    n_q = CHUNK + 1
    q = np.random.default_rng(7).standard_normal((n_q, D)).astype(np.float32)
    full = retrieval.search_all(dix, sc, cuda(q), N_SMALL)
    pred, flt, p, f = _check_exhaustive(dix, full, lambda p, f: retrieval.search_all_where(dix, sc, cuda(q), K, p, filter=f), n_q, 11,
                                        (metric, dtype))
    if (metric, dtype) != ("l2", "f16"):
        return
    # a query's answer does not depend on its batch: the last query alone, under its own conditions
    i = n_q - 1
    one = {k: (v[i:i + 1] if k in ("value_lo", "value_hi", "tags_all", "tags_any", "tags_none") else v) for k, v in pred.items()}
    s = pred["label_splits"]
    one["label_splits"], one["labels"] = np.array([0, s[i + 1] - s[i]], np.int64), pred["labels"][s[i]:s[i + 1]]
    p1, f1 = PC.on_device(dix, one, 1, (flt[0], flt[1][i:i + 1]))
    alone = _got(retrieval.search_all_where(dix, sc, cuda(q[i:i + 1]), K, p1, filter=f1))
    whole = _got(retrieval.search_all_where(dix, sc, cuda(q), K, p, filter=f))
    for name in ("n_out", "index", "item_ids"):
        assert (alone[name][0] == whole[name][i]).all(), name
    assert (bits(alone["scores"][0]) == bits(whole["scores"][i])).all()
    # the count the planner reads equals what the exhaustive form returned at k = n_items
    cnt = retrieval.predicate_count(p, filter=f)
    every = _got(retrieval.search_all_where(dix, sc, cuda(q), N_SMALL, p, filter=f))
    assert (cnt.cpu().numpy() == every["n_out"]).all()


def test_search_all_where_under_an_mlp_scorer():
    from nann_amd import ops, retrieval, synth
    dix = _small("f16")
    sc = ops.Scorer("mlp", D, torch.float16, synth.make_mlp_weights(D), precision="exact")
    n_q = CHUNK + 1
    q = np.random.default_rng(8).standard_normal((n_q, D)).astype(np.float32)
    full = retrieval.search_all(dix, sc, cuda(q), N_SMALL)
    _check_exhaustive(dix, full, lambda p, f: retrieval.search_all_where(dix, sc, cuda(q), K, p, filter=f), n_q, 12, "mlp")


def test_search_all_model_where_under_the_attention_model(tmp_path):
    from nann_amd import ops, retrieval, synth
    dix = _small("f16")
    ops.save_scorer_dir(str(tmp_path / "attn"), "attention", synth.make_attn_weights(D, 64), precision="split")
    m = ops.Model(str(tmp_path / "attn"), D, L_SEQ)
    n_q = CHUNK + 1
    seqs = cuda(np.random.default_rng(9).standard_normal((n_q, L_SEQ, 64)).astype(np.float16), torch.float16)
    full = retrieval.search_all_model(dix, m, seqs, N_SMALL)
    _check_exhaustive(dix, full, lambda p, f: retrieval.search_all_model_where(dix, m, seqs, K, p, filter=f), n_q, 13, "attention")
    with pytest.raises(TypeError):
        retrieval.search_all_model_where(dix, ops.Scorer("l2", D), seqs, K, None)


def test_search_all_model_where_under_an_l2_model(tmp_path):
    from nann_amd import ops, retrieval
    dix = _small("f16")
    ops.save_scorer_dir(str(tmp_path / "l2"), "l2")
    m = ops.Model(str(tmp_path / "l2"), D, L_SEQ)
    n_q = 17
    seqs = cuda(np.random.default_rng(10).standard_normal((n_q, L_SEQ, D)).astype(np.float16), torch.float16)
    full = retrieval.search_all_model(dix, m, seqs, N_SMALL)
    _check_exhaustive(dix, full, lambda p, f: retrieval.search_all_model_where(dix, m, seqs, K, p, filter=f), n_q, 14, "l2 model")


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_beyond_one_list_the_ranking_comes_from_the_scorer(metric):
    """three scatter tiles + 17 rows: the full ranking is nann_score's logits under a stable sort, ties to the lower row"""
    from nann_amd import ops, retrieval
    n, n_q = 3 * TILE + 17, 17
    embs = _rows(n, D, "f16", seed=62)
    embs[TILE:TILE + 40] = embs[0:40]                       # ties across a tile boundary
    dix = _indices(embs)[1]
    sc = ops.Scorer(metric, D)
    q = np.random.default_rng(15).standard_normal((n_q, D)).astype(np.float32)
    scores = np.stack([ops.blaze_score(sc, cuda(v), item_emb=dix.item_embs).cpu().numpy() for v in q])
    order = np.stack([np.argsort(-s, kind="stable") for s in scores]).astype(np.int32)
    ranked = np.take_along_axis(scores, order.astype(np.int64), axis=1)
    pred, flt = _case(n, n_q, 16)
    ids = dix.item_ids.cpu().numpy()
    p, f = PC.on_device(dix, pred, n_q, flt)
    _same(_got(retrieval.search_all_where(dix, sc, cuda(q), K, p, filter=f)), PM.where_topk(order, ranked, None, flt, pred, K, n, item_ids=ids),
          metric)
    # the unchanged call agrees with that ranking: the reference of this test is the one the other tests use
    plain = retrieval.search_all(dix, sc, cuda(q), K)
    torch.cuda.synchronize()
    assert (plain.index.cpu().numpy() == order[:, :K]).all() and (bits(plain.scores.cpu().numpy()) == bits(ranked[:, :K])).all()
    cnt = retrieval.predicate_count(p, filter=f)
    torch.cuda.synchronize()
    assert (cnt.cpu().numpy() == PM.count(pred, flt, n_q, n)).all()


# ---- the traversal forms ----------------------------------------------------------------------------------------------------
def _queries(oracle, n, seed=4321):
    seqs = queries_for(synth_index(N, D, 64)[0], n, seed=seed)
    return seqs, np.stack([oracle.user_seq_mean(s) for s in seqs]).astype(np.float32)


def _expect_from(r, level_topn, dix, pred, flt, k):
    """the model over an unfiltered search's answer -> (model dict, status)"""
    torch.cuda.synchronize()
    status = r.status.cpu().numpy()
    lt = np.asarray(level_topn)
    width = np.full(len(status), lt[5]) if lt.ndim == 1 else lt[:, 5]
    n_valid = np.where(status != 0, 0, width).astype(np.int32)
    exp = PM.where_topk(r.index.cpu().numpy(), r.scores.cpu().numpy(), n_valid, flt, pred, k, int(dix.n_items),
                        item_ids=dix.item_ids.cpu().numpy())
    return exp, status


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_search_where_is_the_model_over_search(oracle, metric):
    from nann_amd import ops, retrieval
    dix = synth_index(N, D, 64)[2]
    sc = ops.Scorer(metric, D)
    n_q = 24
    _, q = _queries(oracle, n_q)
    plain = retrieval.search(dix, sc, cuda(q), TOPN)
    pred, flt = _case(N, n_q, 21)
    p, f = PC.on_device(dix, pred, n_q, flt)
    for k, ff, fl in ((F, f, flt), (20, f, flt), (7, None, None)):                  # k = F, k < F, no filter
        exp, status = _expect_from(plain, TOPN, dix, pred, fl, k)
        r = retrieval.search_where(dix, sc, cuda(q), TOPN, p, k=k, filter=ff)
        _same(_got(r), exp, (metric, k))
        assert (r.status.cpu().numpy() == status).all() and (status == 0).all()
        assert (r.counters.cpu().numpy() == plain.counters.cpu().numpy()).all() and r.plan == plain.plan
    assert (exp["n_out"] == 0).any() and (exp["n_out"] == 7).any()
    # no condition at all: the filtered call's answer
    none, _ = PC.on_device(dix, {}, n_q)
    only = retrieval.search(dix, sc, cuda(q), TOPN, filter=f, k=20)
    r = _got(retrieval.search_where(dix, sc, cuda(q), TOPN, none, k=20, filter=f))
    torch.cuda.synchronize()
    assert (r["index"] == only.index.cpu().numpy()).all() and (r["n_out"] == only.n_out.cpu().numpy()).all()
    assert (bits(r["scores"]) == bits(only.scores.cpu().numpy())).all()


def test_per_query_level_topn_and_a_failed_query(oracle):
    from nann_amd import ops, retrieval
    dix = synth_index(N, D, 64)[2]
    sc = ops.Scorer("l2", D)
    n_q = 17
    _, q = _queries(oracle, n_q, seed=13)
    lt = np.tile(np.array(TOPN, np.int32), (n_q, 1))
    lt[4] = [8, 4, 4, 4, 4, F]       # query 4: a pool of 16 rows cannot give 50
    lt[6, 5] = 20                    # query 6 asks for 20 only
    lt[16, 5] = 33                   # ... and one of the second 16-query group
    plain = retrieval.search(dix, sc, cuda(q), lt)
    pred, flt = _case(N, n_q, 22)
    exp, status = _expect_from(plain, lt, dix, pred, flt, 14)
    assert status[4] != 0 and (np.delete(status, 4) == 0).all()
    p, f = PC.on_device(dix, pred, n_q, flt)
    r = retrieval.search_where(dix, sc, cuda(q), lt, p, k=14, filter=f)
    got = _got(r)
    _same(got, exp)
    assert (r.status.cpu().numpy() == status).all()
    assert got["n_out"][4] == 0 and not got["index"][4].any() and not got["item_ids"][4].any() and not bits(got["scores"][4]).any()
    # query 6 sees its own 20 entries only: the model over the first 20 columns
    six = PM.where_topk(plain.index.cpu().numpy()[6:7, :20], plain.scores.cpu().numpy()[6:7, :20], None, flt, pred, 14, N, q0=6)
    assert got["n_out"][6] == six["n_out"][0] and (got["index"][6] == six["index"][0]).all()


def test_the_model_form(oracle, tmp_path):
    from nann_amd import ops, retrieval
    dix = synth_index(N, D, 64)[2]
    n_q = 17
    seqs, q = _queries(oracle, n_q)
    ops.save_scorer_dir(str(tmp_path / "l2"), "l2")
    m = ops.Model(str(tmp_path / "l2"), D, seqs.shape[1])
    plain = retrieval.search_model(dix, m, cuda(seqs, torch.float16), TOPN)
    pred, flt = _case(N, n_q, 23)
    exp, status = _expect_from(plain, TOPN, dix, pred, flt, 14)
    p, f = PC.on_device(dix, pred, n_q, flt)
    r = retrieval.search_model_where(dix, m, cuda(seqs, torch.float16), TOPN, p, k=14, filter=f)
    _same(_got(r), exp)
    assert (r.status.cpu().numpy() == status).all() and r.plan == plain.plan
    # ... and the bits of the scorer form over the sequences' means
    _same(_got(retrieval.search_where(dix, ops.Scorer("l2", D), cuda(q), TOPN, p, k=14, filter=f)), exp)


def test_refusals_launch_nothing(oracle):
    import ctypes as C
    from nann_amd import _lib, ops
    from nann_amd.ops import _ptr, _stream
    L = _lib.lib()
    dix = _small("f16")
    sc = ops.Scorer("l2", D)
    b, k = 4, 14
    qd = cuda(np.random.default_rng(3).standard_normal((b, D)).astype(np.float32))
    nb, inner = C.c_int64(-1), C.c_int64(-1)
    assert L.nann_search_all_where_workspace_bytes(dix.handle, sc.handle, b, k, C.byref(nb)) == 0
    assert L.nann_search_all_filtered_workspace_bytes(dix.handle, sc.handle, b, k, C.byref(inner)) == 0 and nb.value == inner.value > 0
    ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    o = {"item_ids": torch.full((b, k), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64).cuda(), "scores": torch.full((b, k), 777.0).cuda(),
         "index": torch.full((b, k), 0x5A5A5A5A, dtype=torch.int32).cuda(), "n_out": torch.full((b,), 0x5A5A5A5A, dtype=torch.int32).cuda()}
    col = cuda(np.zeros(N_SMALL, np.float32))

    def call(p, ws_bytes=nb.value):
        return L.nann_search_all_where(dix.handle, sc.handle, _ptr(qd), b, k, _ptr(o["item_ids"]), _ptr(o["scores"]), _ptr(o["index"]),
                                       _ptr(ws), ws_bytes, None, None, C.byref(p) if p is not None else None, _ptr(o["n_out"]), _stream())

    bad = _lib.Predicates()
    bad.struct_bytes = C.sizeof(_lib.Predicates)
    bad.value_lo = col.data_ptr()                          # a bound without its column
    assert call(bad) == 7 and b"without value_of_row" in L.nann_last_error()
    bad.value_of_row, bad.struct_bytes = col.data_ptr(), 17
    assert call(bad) == 7 and b"struct_bytes" in L.nann_last_error()
    bad.struct_bytes, bad.n_labels = 0, -1
    assert call(bad) == 7 and b"n_labels < 0" in L.nann_last_error()
    bad.n_labels = 0
    assert call(bad, ws_bytes=nb.value - 1) == 103
    torch.cuda.synchronize()
    assert (o["item_ids"].cpu() == 0x5A5A5A5A5A5A5A5A).all() and (o["scores"].cpu() == 777.0).all()
    assert (o["index"].cpu() == 0x5A5A5A5A).all() and (o["n_out"].cpu() == 0x5A5A5A5A).all()
    assert call(bad) == 0 and call(None) == 0              # lo = 0 over a column of zeros, no upper bound: every row passes
    torch.cuda.synchronize()
    assert (o["n_out"].cpu() == k).all()


def test_the_traversal_forms_refuse_a_malformed_struct_and_launch_nothing(oracle):
    import ctypes as C
    from nann_amd import _lib, ops
    from nann_amd.ops import _ptr, _stream
    L = _lib.lib()
    dix = synth_index(N, D, 64)[2]
    sc = ops.Scorer("l2", D)
    b, k = 6, 20
    _, q = _queries(oracle, b, seed=14)
    qd = cuda(q)
    t = (C.c_int32 * 6)(*TOPN)
    nb, plain = C.c_int64(-1), C.c_int64(-1)
    assert L.nann_search_where_workspace_bytes(dix.handle, t, b, C.byref(nb)) == 0
    assert L.nann_search_filtered_workspace_bytes(dix.handle, t, b, C.byref(plain)) == 0 and nb.value == plain.value > 0
    ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    o = {"item_ids": torch.full((b, k), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64).cuda(), "scores": torch.full((b, k), 777.0).cuda(),
         "index": torch.full((b, k), 0x5A5A5A5A, dtype=torch.int32).cuda(), "n_out": torch.full((b,), 0x5A5A5A5A, dtype=torch.int32).cuda(),
         "status": torch.full((b,), 0x5A5A5A5A, dtype=torch.int32).cuda()}
    col = cuda(np.zeros(N, np.float32))

    def call(p, n=b, kk=k):
        return L.nann_search_where(dix.handle, sc.handle, _ptr(qd), n, t, None, _ptr(ws), nb.value, _ptr(o["item_ids"]), _ptr(o["scores"]),
                                   _ptr(o["index"]), _ptr(o["status"]), None, None, None, None, None, C.byref(p) if p is not None else None,
                                   kk, _ptr(o["n_out"]), _stream())

    bad = _lib.Predicates()
    bad.struct_bytes = C.sizeof(_lib.Predicates)
    bad.tags_none = col.data_ptr()                         # a condition without its column
    assert call(bad) == 7 and b"without tags_of_row" in L.nann_last_error()
    assert call(bad, n=0) == 7 and call(bad, kk=F + 1) == 7 and b"without tags_of_row" in L.nann_last_error()   # in front of the rest
    bad.tags_none, bad.value_of_row, bad.value_lo, bad.struct_bytes = None, col.data_ptr(), col.data_ptr(), 95
    assert call(bad) == 7 and b"struct_bytes" in L.nann_last_error()
    bad.struct_bytes, bad.n_labels = C.sizeof(_lib.Predicates), -1
    assert call(bad) == 7 and b"n_labels < 0" in L.nann_last_error()
    bad.n_labels, bad.label_of_row, bad.label_splits = 3, col.data_ptr(), col.data_ptr()
    assert call(bad) == 7 and b"label_splits without labels" in L.nann_last_error()
    torch.cuda.synchronize()
    assert (o["item_ids"].cpu() == 0x5A5A5A5A5A5A5A5A).all() and (o["scores"].cpu() == 777.0).all()
    assert all((o[n].cpu() == 0x5A5A5A5A).all() for n in ("index", "n_out", "status"))
    bad.n_labels, bad.label_splits = 0, None
    assert call(bad) == 0                                  # lo = 0 over a column of zeros: every fetched row passes
    torch.cuda.synchronize()
    assert (o["status"].cpu() == 0).all() and (o["n_out"].cpu() == k).all()
