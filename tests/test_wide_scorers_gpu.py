"""-m gpu: the wide exhaustive search under the MLP scorer and the attention model at k = 2000.  The exact MLP is held to the
oracle's bits.  The split-f16 forms are held to search_all_range[_model] at a threshold of -inf -- the same scoring path, the same
bits for every row -- stably sorted by score: that isolates the selection, so no tolerance is needed here either."""
import numpy as np
import pytest
import torch

from gpu_util import bits, cuda, require_gpu
from test_search_all_gpu import _brute
from test_wide_gpu import _assert_top, _indices

pytestmark = pytest.mark.gpu
K = 2000


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _sorted_range(r, b):
    """a RangeResult at -inf (every row, ascending row order) -> per query (rows, scores, item ids) by (score descending, row
    ascending), the first K"""
    torch.cuda.synchronize()
    splits, rows, scores, ids = (t.cpu().numpy() for t in (r.row_splits, r.index, r.scores, r.item_ids))
    out = []
    for i in range(b):
        lo, hi = splits[i], splits[i + 1]
        order = np.argsort(-(scores[lo:hi] + np.float32(0.0)).astype(np.float64), kind="stable")[:K]
        out.append((rows[lo:hi][order], scores[lo:hi][order], ids[lo:hi][order]))
    return out


def _assert_same_as_range(w, exp):
    torch.cuda.synchronize()
    rows, scores, ids, n_out = (t.cpu().numpy() for t in (w.index, w.scores, w.item_ids, w.n_out))
    assert (n_out == K).all()
    for i, (er, es, ei) in enumerate(exp):
        assert len(er) == K
        assert (rows[i] == er).all() and (bits(scores[i]) == bits(es)).all() and (ids[i] == ei).all(), i


def _mlp_case(oracle):
    from nann_amd import synth
    n, d = 5000, 64
    embs, assign = synth.make_corpus(n, d, seed=61)
    oix, dix = _indices(embs)
    w = synth.make_mlp_weights(d)
    q = np.stack([oracle.user_seq_mean(s) for s in synth.make_queries(embs, assign, 5, seed=62)])
    return oix, dix, w, q


def test_mlp_exact_is_the_oracles_bits(oracle):
    from nann_amd import ops, retrieval
    oix, dix, w, q = _mlp_case(oracle)
    exp_rows, exp_scores = _brute(oracle, oix, oracle.Scorer("mlp", 64, oracle.EMB_F16, w), q, K)
    r = retrieval.search_all_wide(dix, ops.Scorer("mlp", 64, torch.float16, w, precision="exact"), cuda(q, torch.float32), K)
    torch.cuda.synchronize()
    got = tuple(t.cpu().numpy() for t in (r.index, r.scores, r.item_ids, r.n_out))
    _assert_top(got, exp_rows, exp_scores, oix.ids, K)


def test_mlp_split_selects_from_the_range_forms_scores(oracle):
    from nann_amd import ops, retrieval
    oix, dix, w, q = _mlp_case(oracle)
    sc = ops.Scorer("mlp", 64, torch.float16, w, precision="split")
    x = cuda(q, torch.float32)
    exp = _sorted_range(retrieval.search_all_range(dix, sc, x, -np.inf, capacity=5 * 5000), 5)
    _assert_same_as_range(retrieval.search_all_wide(dix, sc, x, K), exp)


def test_attention_model_selects_from_the_range_forms_scores(tmp_path):
    from nann_amd import retrieval
    from test_search_all_model_gpu import _corpus, _model
    n, b = 4099, 5
    host, oix, dix, code, tdt, seqs = _corpus(n, 64)
    model = _model(tmp_path, 64, "split")
    x = cuda(seqs[:b], torch.float16)
    exp = _sorted_range(retrieval.search_all_range_model(dix, model, x, -np.inf, capacity=b * n), b)
    _assert_same_as_range(retrieval.search_all_model_wide(dix, model, x, K), exp)
