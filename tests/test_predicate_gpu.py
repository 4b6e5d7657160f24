"""-m gpu: nann_predicate_topk and nann_predicate_count (k_pred_compact, k_pred_count; csrc/nann_predicate.h) against the numpy
model (predicate_model), bitwise.  The input lists are cut from what the existing, unchanged retrieval.search_all returns at
k = min(n_items, 1024) for an L2 index of 64-d f16 rows -- stretched to k_in by repeating entries (repeated rows, tied scores) and
salted with rows out of range -- so the model is applied to the output of a call pinned elsewhere.  n_items: 1, 63, 1 000, one
scatter tile + 1, three tiles + 17 (the tile from the header); queries: 1, 17 (across a 16-query group), 64; k_in: 1, 64, 65,
1 000, 1 024 -- as the five pairs of SHAPES, every value once, not as their cross product.  Every batch of 17 or more holds queries with no, some and all entries passing (predicate_cases)."""
import os
import re

import numpy as np
import pytest
import torch

import predicate_cases as PC
import predicate_model as PM
from gpu_util import bits, cuda, require_gpu
from test_search_all_gpu import _indices, _rows

pytestmark = pytest.mark.gpu
D = 64
_CACHE = {}


def _tile():
    from nann_amd import build
    src = open(os.path.join(build.SRC_DIR, "nann_predicate.h")).read()
    return int(re.search(r"constexpr int kPredTileRows = (\d+);", src).group(1))


TILE = _tile()
N_ITEMS = [1, 63, 1000, TILE + 1, 3 * TILE + 17]
SHAPES = [(1, 1), (17, 64), (17, 65), (64, 1000), (17, 1024)]   # (queries, k_in)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _ranked(n):
    """(device index, rows i32[64, w], scores f32[64, w]) with w = min(n, 1024): search_all's answer for 64 seeded queries"""
    if n not in _CACHE:
        from nann_amd import ops, retrieval
        _, dix = _indices(_rows(n, D, "f16", seed=n + 5))
        q = np.random.default_rng(n).standard_normal((64, D)).astype(np.float32)
        r = retrieval.search_all(dix, ops.Scorer("l2", D), cuda(q), min(n, 1024))
        torch.cuda.synchronize()
        _CACHE[n] = (dix, r.index.cpu().numpy(), r.scores.cpu().numpy())
    return _CACHE[n]


def _lists(rng, n, n_q, k_in):
    """ranked lists [n_q, k_in] cut from search_all's: entry j is entry j * w // k_in' of the answer -- repeats where k_in > w
    -- with a few rows out of range and a few entries standing twice"""
    _, rows, scores = _ranked(n)
    w = rows.shape[1]
    pick = np.arange(k_in) * w // k_in if k_in > w else np.arange(k_in)
    lr, ls = rows[:n_q, pick].copy(), scores[:n_q, pick].copy()
    if k_in >= 64:
        lr[:, 7] = lr[:, 3]                                    # a row twice, with its score: a tie
        ls[:, 7] = ls[:, 3]
        lr[:, 11], lr[:, 13] = -1, n                           # rows out of range
        if n_q > 2:
            lr[2, 20] = np.iinfo(np.int32).max
    return np.ascontiguousarray(lr), np.ascontiguousarray(ls)


def _got(r):
    torch.cuda.synchronize()
    return {"item_ids": r.item_ids.cpu().numpy(), "scores": r.scores.cpu().numpy(), "index": r.index.cpu().numpy(),
            "pos": r.pos.cpu().numpy(), "n_out": r.n_out.cpu().numpy()}


def _same(got, exp, what=""):
    for name in ("n_out", "index", "pos", "item_ids", "scores"):
        g, e = (bits(got[name]), bits(exp[name])) if name == "scores" else (got[name], exp[name])
        assert g.shape == e.shape and (g == e).all(), (what, name)


@pytest.mark.parametrize("n", N_ITEMS)
def test_predicate_topk_is_the_model(n):
    from nann_amd import retrieval
    dix = _ranked(n)[0]
    ids = dix.item_ids.cpu().numpy()
    rng = np.random.default_rng(100 + n)
    seen = set()
    for c, (n_q, k_in) in enumerate(SHAPES):
        rows, scores = _lists(rng, n, n_q, k_in)
        tests = [7, 7, 5, 6, 3][c]                             # (labels + tags, unfiltered: where a query can pass every entry)
        pred = PC.make(rng, n, n_q, tests)
        flt = PC.make_filter(rng, n, n_q, hot=rows) if c % 2 else None
        n_valid = [None, rng.integers(-1, k_in + 2, n_q).astype(np.int32), None, np.full(n_q, k_in, np.int32), None][c]
        if c == 1:
            n_valid[0] = 0
        k = [k_in, max(k_in // 2, 1), k_in, 200, 1024][c]
        exp = PM.where_topk(rows, scores, n_valid, flt, pred, k, n, item_ids=ids)
        p, f = PC.on_device(dix, pred, n_q, flt)
        r = retrieval.predicate_topk(cuda(scores), cuda(rows), p, k, n_valid=None if n_valid is None else cuda(n_valid), index=dix,
                                     filter=f)
        got = _got(r)
        _same(got, exp, (n, n_q, k_in))
        valid = np.minimum(np.maximum(n_valid, 0), k_in) if n_valid is not None else np.full(n_q, k_in)
        for i in range(n_q):
            inside = ((rows[i, :valid[i]] >= 0) & (rows[i, :valid[i]] < n)).sum()
            seen.add("none" if exp["n_out"][i] == 0 and inside else "all" if exp["n_out"][i] == min(k, inside) and inside else "some")
    if n >= 63:
        assert seen == {"none", "some", "all"}, seen
    # without scores, item ids and an index: zeros for scores, rows and positions as before
    n_q, k_in = SHAPES[1]
    rows, _ = _lists(rng, n, n_q, k_in)
    pred = PC.make(rng, n, n_q, 7)
    p, _ = PC.on_device(PC.index_like(n, ids, "cuda"), pred, n_q)
    exp = PM.where_topk(rows, None, None, None, pred, k_in, n)
    r = retrieval.predicate_topk(None, cuda(rows), p, k_in)
    torch.cuda.synchronize()
    assert r.item_ids is None and (r.index.cpu().numpy() == exp["index"]).all() and (r.n_out.cpu().numpy() == exp["n_out"]).all()
    assert (r.pos.cpu().numpy() == exp["pos"]).all() and not bits(r.scores.cpu().numpy()).any()


@pytest.mark.parametrize("n", N_ITEMS)
def test_predicate_count_is_the_model(n):
    from nann_amd import retrieval
    ix = PC.index_like(n, np.arange(n, dtype=np.int64), "cuda")
    rng = np.random.default_rng(200 + n)
    for c, n_q in enumerate((1, 17, 64)):
        for tests in ((7, 1, 6) if c == 1 else (7,)):
            pred = PC.make(rng, n, n_q, tests)
            flt = PC.make_filter(rng, n, n_q) if c else None
            p, f = PC.on_device(ix, pred, n_q, flt)
            got = retrieval.predicate_count(p, filter=f)
            torch.cuda.synchronize()
            exp = PM.count(pred, flt, n_q, n)
            assert got.dtype == torch.int64 and (got.cpu().numpy() == exp).all(), (n, n_q, tests)
            if n >= 1000 and n_q >= 17 and tests == 7:
                assert exp[1::8].max() == 0 and 0 < exp[0] < n          # a query that passes nothing, one that passes most
    # no condition at all: the rows the filter leaves
    flt = PC.make_filter(rng, n, 17)
    p, f = PC.on_device(ix, {}, 17, flt)
    got = retrieval.predicate_count(p, filter=f)
    torch.cuda.synchronize()
    assert (got.cpu().numpy() == PM.count(None, flt, 17, n)).all()
    assert (retrieval.predicate_count(p).cpu().numpy() == n).all()


def test_a_union_filtered_by_predicate_and_handed_on_to_the_cap():
    """the documented composition: predicate_topk's n_out is the n_valid of cap_groups behind it"""
    import groupcap_model as GM
    from nann_amd import retrieval
    n, n_q, k_in = 1000, 17, 200
    dix = _ranked(n)[0]
    ids = dix.item_ids.cpu().numpy()
    rng = np.random.default_rng(9)
    rows, scores = _lists(rng, n, n_q, k_in)
    pred = PC.make(rng, n, n_q, 7)
    p, _ = PC.on_device(dix, pred, n_q)
    gor = (np.arange(n) % 7).astype(np.int32)
    first = retrieval.predicate_topk(cuda(scores), cuda(rows), p, k_in, index=dix)
    r = retrieval.cap_groups(first.scores, first.index, retrieval.make_groups(dix, group_of_row=gor, cap=2), 10, n_valid=first.n_out,
                             index=dix)
    torch.cuda.synchronize()
    mid = PM.where_topk(rows, scores, None, None, pred, k_in, n)
    exp = GM.model(mid["scores"], mid["index"], mid["n_out"], n, gor, 2, 10, item_ids=ids)
    assert (r.n_out.cpu().numpy() == exp["n_out"]).all() and (r.index.cpu().numpy() == exp["index"]).all()
    assert (bits(r.scores.cpu().numpy()) == bits(exp["scores"])).all() and (r.item_ids.cpu().numpy() == exp["item_ids"]).all()
