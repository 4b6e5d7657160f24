"""-m gpu: the wide exhaustive search under a filter and under predicates, against numpy over the oracle's scores: a denied row
carries -inf into the selection and never comes back, n_out counts the allowed rows where they are fewer than k, and
search_all_where agrees where both exist."""
import numpy as np
import pytest
import torch

import wide_model as M
from gpu_util import bits, cuda, require_gpu
from test_wide_gpu import N, _case, _wide

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _matrix(rows, scores):
    """the oracle's full ranking -> scores f32[B, n] by row number"""
    out = np.empty(scores.shape, np.float32)
    np.put_along_axis(out, rows.astype(np.int64), scores, axis=1)
    return out


def _assert_masked(got, masked, item_ids, k, what=""):
    rows, scores, ids, n_out = got
    for i in range(masked.shape[0]):
        ev, ei, en = M.reference(masked[i], k)
        assert n_out[i] == en, (what, i)
        assert (rows[i] == ei).all() and (bits(scores[i]) == bits(ev)).all(), (what, i)
        assert (ids[i, :en] == item_ids[ei[:en]]).all() and (ids[i, en:] == 0).all(), (what, i)
        assert (masked[i, rows[i, :en]] != -np.inf).all(), (what, i)   # a denied row never appears


def test_a_bitmap_over_most_rows_leaves_fewer_than_k(oracle):
    from nann_amd import ops, retrieval
    oix, dix, q, exp_rows, exp_scores = _case(oracle, "random")
    full = _matrix(exp_rows, exp_scores)
    deny = np.random.default_rng(41).random(N) < 0.95
    masked = full.copy()
    masked[:, deny] = -np.inf
    allowed = int((~deny).sum())
    assert 500 < allowed < 4097
    flt = retrieval.make_filter(dix, deny_rows=np.nonzero(deny)[0])
    got = _wide(dix, ops.Scorer("l2", 64), q, 4097, filter=flt)
    assert (got[3] == allowed).all()
    _assert_masked(got, masked, oix.ids, 4097, "bitmap")
    got = _wide(dix, ops.Scorer("l2", 64), q, 200, filter=flt)       # and a k below the allowed count
    assert (got[3] == 200).all()
    _assert_masked(got, masked, oix.ids, 200, "bitmap, k = 200")


def test_exclusion_lists_per_query(oracle):
    from nann_amd import ops, retrieval
    oix, dix, q, exp_rows, exp_scores = _case(oracle, "random")
    full = _matrix(exp_rows, exp_scores)
    rng = np.random.default_rng(42)
    # every query loses every other row of its own top 3000, and some rows at random; query 3 loses nothing
    lists = [np.concatenate([exp_rows[i, :3000:2], rng.integers(0, N, 500)]).astype(np.int64) for i in range(5)]
    lists[3] = np.zeros(0, np.int64)
    masked = full.copy()
    for i in range(5):
        masked[i, lists[i]] = -np.inf
    flt = retrieval.make_filter(dix, exclude_rows=lists)
    sc = ops.Scorer("l2", 64)
    _assert_masked(_wide(dix, sc, q, 4097, filter=flt), masked, oix.ids, 4097, "lists")
    both = retrieval.make_filter(dix, deny_rows=np.arange(0, N, 3), exclude_rows=lists)
    masked[:, ::3] = -np.inf
    _assert_masked(_wide(dix, sc, q, 2049, filter=both), masked, oix.ids, 2049, "bitmap + lists")


def test_predicates_and_search_all_where_agrees(oracle):
    from nann_amd import ops, retrieval
    oix, dix, q, exp_rows, exp_scores = _case(oracle, "random")
    full = _matrix(exp_rows, exp_scores)
    rng = np.random.default_rng(43)
    label = rng.integers(0, 10, N).astype(np.int32)
    value = rng.random(N).astype(np.float32)
    at = retrieval.make_attributes(dix, label_of_row=label, value_of_row=value)
    label_in = [[1, 2, 3], [], [7], [0, 1, 2, 3, 4, 5, 6, 7, 8], [9, 9]]
    lo = np.array([0.0, 0.5, 0.0, 0.25, 0.9], np.float32)
    pred = retrieval.make_predicates(at, 5, label_in=label_in, value_range=(lo, None))
    masked = full.copy()
    for i in range(5):
        ok = value >= lo[i]
        if label_in[i]:
            ok &= np.isin(label, label_in[i])
        masked[i, ~ok] = -np.inf
    passing = (masked != -np.inf).sum(1)
    assert passing.min() < 1024 < 4097 < passing.max()            # both sides of both k
    sc = ops.Scorer("l2", 64)
    _assert_masked(_wide(dix, sc, q, 4097, predicates=pred), masked, oix.ids, 4097, "predicates")
    flt = retrieval.make_filter(dix, deny_rows=np.arange(1, N, 2))
    masked[:, 1::2] = -np.inf
    got = _wide(dix, sc, q, 1024, predicates=pred, filter=flt)
    _assert_masked(got, masked, oix.ids, 1024, "predicates + bitmap")
    r = retrieval.search_all_where(dix, sc, cuda(q, torch.float32), 1024, pred, filter=flt)
    torch.cuda.synchronize()
    n_out = r.n_out.cpu().numpy()
    assert (n_out == got[3]).all()
    for i in range(5):
        m = n_out[i]
        assert (r.index.cpu().numpy()[i, :m] == got[0][i, :m]).all() and (bits(r.scores.cpu().numpy()[i, :m]) == bits(got[1][i, :m])).all()
        assert (r.item_ids.cpu().numpy()[i, :m] == got[2][i, :m]).all()
