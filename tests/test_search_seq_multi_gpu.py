"""-m gpu: the multi-vector searches from a behaviour sequence (retrieval.search_seq_multi / search_all_seq_multi): the
interests call in front of the existing multi-vector searches.  The exhaustive forms on a 3 000 x 64 f16 index built here
(no graph is walked) against the same searches fed the numpy model's q and weights, bitwise; a planted case in which the mean
query lands in the empty space between two tastes; one traversal case on a small graph from the shipped builder."""
import numpy as np
import pytest
import torch

import interests_model as IM
from gpu_util import bits, cuda, queries_for, require_gpu, synth_index
from test_search_all_gpu import _indices

pytestmark = pytest.mark.gpu
N, D = 3000, 64  # (the narrowest rows an index takes: d is 64, 128, 256 or 512)
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _planted_index():
    """item clusters of 1 000 rows each at +10 e1 (rows 0-999), -10 e1 (1000-1999) and the origin (2000-2999), noise 0.25"""
    if "ix" not in _CACHE:
        rng = np.random.default_rng(17)
        embs = (rng.standard_normal((N, D)) * 0.25).astype(np.float32)
        embs[:1000, 0] += 10.0
        embs[1000:2000, 0] -= 10.0
        embs = embs.astype(np.float16)
        _CACHE["ix"] = (embs, _indices(embs)[1])
    return _CACHE["ix"]


def _histories(embs, n_users, seq_len, seed, pads=True):
    """a user's history: half of its rows from each outer cluster, interleaved, a pad row at the end"""
    rng = np.random.default_rng(seed)
    seq = np.zeros((n_users, seq_len, D), np.float16)
    for u in range(n_users):
        half = (seq_len - int(pads)) // 2
        rows = np.concatenate([rng.integers(0, 1000, half), rng.integers(1000, 2000, half)])
        seq[u, :2 * half] = embs[rng.permutation(rows)]
    return seq


def _bits16(seq):
    return np.ascontiguousarray(seq).view(np.uint16)


def _got(r, names):
    torch.cuda.synchronize()
    return {n: getattr(r, n).cpu().numpy() for n in names}


def _same(a, b, what=""):
    assert set(a) == set(b)
    for name in a:
        g, e = (bits(a[name]), bits(b[name])) if name == "scores" else (a[name], b[name])
        assert g.shape == e.shape and (g == e).all(), (what, name)


MULTI = ("item_ids", "scores", "index", "vec", "n_out")
FUSED = ("item_ids", "scores", "index", "lists", "n_out")


def test_search_all_seq_multi_is_search_all_multi_over_the_models_vectors():
    from nann_amd import ops, retrieval
    embs, dix = _planted_index()
    sc = ops.Scorer("l2", D)
    seq = _histories(embs, 6, 21, seed=1)
    seq[4] = 0                   # a user without history
    seq[5, 1:] = seq[5, :1]      # a user with one interest
    exp = IM.model(_bits16(seq), 3, 4)
    r, interests = retrieval.search_all_seq_multi(dix, sc, cuda(seq), 3, 50, n_iter=4)
    assert isinstance(r, retrieval.MultiResult) and isinstance(interests, retrieval.Interests)
    assert (bits(interests.q.cpu().numpy()) == bits(exp["q"])).all()
    assert (bits(interests.weights.cpu().numpy()) == bits(exp["weights"])).all()
    assert (interests.n_interests.cpu().numpy() == exp["n_interests"]).all() and exp["n_interests"].tolist()[4:] == [0, 1]
    _same(_got(r, MULTI), _got(retrieval.search_all_multi(dix, sc, cuda(exp["q"]), 50), MULTI), "union")
    # with a Fusion that brings no weights: the interests' weights, per user
    for mode in ("sum_floor", "rrf"):
        r, interests = retrieval.search_all_seq_multi(dix, sc, cuda(seq), 3, 50, fusion=retrieval.make_fusion(mode), fetch=60, n_iter=4)
        assert isinstance(r, retrieval.FusedResult)
        ref = retrieval.search_all_multi_fused(dix, sc, cuda(exp["q"]), 50, retrieval.make_fusion(mode, weights=exp["weights"]), fetch=60)
        _same(_got(r, FUSED), _got(ref, FUSED), mode)
        unweighted = retrieval.search_all_multi_fused(dix, sc, cuda(exp["q"]), 50, retrieval.make_fusion(mode), fetch=60)
        assert not (bits(_got(unweighted, FUSED)["scores"]) == bits(_got(r, FUSED)["scores"])).all()  # (the weights did count)


def test_a_fusion_with_its_own_weights_is_used_as_given():
    from nann_amd import ops, retrieval
    embs, dix = _planted_index()
    sc = ops.Scorer("l2", D)
    seq = _histories(embs, 4, 21, seed=2)
    exp = IM.model(_bits16(seq), 2, 8)
    for own in (np.array([0.25, 3.0], np.float32), np.arange(1, 9, dtype=np.float32).reshape(4, 2)):
        fusion = retrieval.make_fusion("sum_floor", weights=own)
        r, interests = retrieval.search_all_seq_multi(dix, sc, cuda(seq), 2, 40, fusion=fusion)
        ref = retrieval.search_all_multi_fused(dix, sc, cuda(exp["q"]), 40, retrieval.make_fusion("sum_floor", weights=own))
        _same(_got(r, FUSED), _got(ref, FUSED), own.shape)
        assert fusion.weights.tolist() == own.tolist()                               # (and the caller's object is untouched)
        assert (bits(interests.weights.cpu().numpy()) == bits(exp["weights"])).all()  # the interests still report their own


def test_two_tastes_the_mean_misses_both_and_two_vectors_find_both():
    from nann_amd import ops, retrieval
    embs, dix = _planted_index()
    sc = ops.Scorer("l2", D)
    seq = _histories(embs, 5, 21, seed=3)
    mean = retrieval.search_all(dix, sc, ops.user_seq_mean(cuda(seq)), 20)
    r, interests = retrieval.search_all_seq_multi(dix, sc, cuda(seq), 2, 20)
    torch.cuda.synchronize()
    rows_mean, rows = mean.index.cpu().numpy(), r.index.cpu().numpy()
    assert (interests.n_interests.cpu().numpy() == 2).all() and (r.n_out.cpu().numpy() == 20).all()
    assert (rows_mean >= 2000).all()                       # the mean query: wholly in the origin cluster
    for u in range(5):
        assert (rows[u] < 1000).any() and ((rows[u] >= 1000) & (rows[u] < 2000)).any() and (rows[u] < 2000).all(), u
    w = interests.weights.cpu().numpy()
    assert (w == 0.5).all()                                # ten rows of each taste, the pad row counts for neither


def test_search_seq_multi_is_search_multi_on_the_same_vectors():
    from nann_amd import ops, retrieval
    g, _, dix = synth_index(2000, 64, 64)
    topn = [8, 16, 32, 32, 32, 50]
    sc = ops.Scorer("l2", 64)
    seq = np.asarray(queries_for(g, 4, seed=99))
    r, interests = retrieval.search_seq_multi(dix, sc, cuda(seq), 3, topn, k=50, n_iter=3)
    assert (bits(interests.q.cpu().numpy()) == bits(IM.model(_bits16(seq.astype(np.float16)), 3, 3)["q"])).all()
    ref = retrieval.search_multi(dix, sc, interests.q, topn, k=50)
    _same(_got(r, MULTI + ("status",)), _got(ref, MULTI + ("status",)), "traversal")
    assert r.plan == ref.plan
    f, _ = retrieval.search_seq_multi(dix, sc, cuda(seq), 3, topn, k=50, fusion=retrieval.make_fusion("rrf"), n_iter=3)
    ref = retrieval.search_multi_fused(dix, sc, interests.q, topn, retrieval.make_fusion("rrf", weights=interests.weights), k=50)
    _same(_got(f, FUSED + ("status",)), _got(ref, FUSED + ("status",)), "traversal, fused")
