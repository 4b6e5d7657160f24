"""GPU: IVF-SQ8 (nann_search_lists_sq8, retrieval.search_lists_sq8) against a numpy model of its contract, bit for bit -- the
fetch lists by approximate score over a query's concatenation (sq8_model), the exact re-rank of the fetched positions with
nann_score's bits, ties to the lower position in both stages -- and against search_lists where the fetch covers every query."""
import numpy as np
import pytest
import torch

import sq8_model as M
from gpu_util import bits, cuda, require_gpu
from lists_model import expansion, partition_csr
from test_sq8_gpu import _exact_on_device, _index, _rows, _scorer

pytestmark = pytest.mark.gpu
N, N_LISTS, B, N_PROBE = 3000, 12, 40, 3
# the 16-row group, the wavefront's 64 rows and the 256-row block from both sides; three long lists; 150 rows are in no list
LENGTHS = [0, 1, 15, 16, 17, 255, 256, 257, 700, 300, 290]
LENGTHS.append(N - 150 - sum(LENGTHS))
FIELDS = ("item_ids", "scores", "index", "pos", "n_out", "status")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _list_of_row():
    lor = np.full(N, -1, np.int32)
    lor[np.random.default_rng(11).permutation(N)[:sum(LENGTHS)]] = np.repeat(np.arange(N_LISTS), LENGTHS)
    return lor


def _probes():
    """list 8 by 33 queries (two full tiles and a tile of one), list 7 by 17 (a split), list 5 by 16 (one full tile), list 6 by
    query 33 alone; query 34 names list 9 twice, 35 has a negative slot, 36 names only the empty list, 37 a list >= n_lists"""
    p = np.zeros((B, N_PROBE), np.int32)
    p[:33, 0] = 8
    p[:17, 1] = 7
    p[17:33, 1] = 5
    p[:33, 2] = np.arange(33) % 5  # lists 0 .. 4
    p[33:] = [[6, 2, 3], [9, 9, 2], [11, -1, 3], [0, -1, 0], [4, N_LISTS, 1], [10, 9, 4], [11, 1, 2]]
    return p


def _case(d, dtype):
    """rows with twins in the same list and in different ones, queries next to some of the twins"""
    lor = _list_of_row()
    x = _rows(N, d, d, dtype)
    in8, in7 = np.flatnonzero(lor == 8), np.flatnonzero(lor == 7)
    x[in8[[3, 40]]] = x[in8[1]]   # three twins in list 8 ...
    x[in7[[2, 9]]] = x[in8[1]]    # ... and two more in list 7
    x[in8[[100, 101]]] = x[in7[5]]
    q = np.random.default_rng(d + 3).standard_normal((B, d)).astype(np.float32)
    q[:8] = M.widen(x[in8[1]:in8[1] + 1]) * np.linspace(0.9, 1.1, 8, dtype=np.float32)[:, None]
    q[8:12] = M.widen(x[in7[5]:in7[5] + 1])
    return lor, x, q


def _model(lists, approx, exact, item_ids, fetch, k):
    """the contract in numpy: per query the fetch over its concatenation C by approximate score (positions), their re-rank by
    exact score; approx / exact: f32[B, N] over the rows of the table"""
    out = {f: np.zeros((B, k), t) for f, t in (("item_ids", np.int64), ("scores", np.float32), ("index", np.int32), ("pos", np.int32))}
    out.update(n_out=np.zeros(B, np.int32), status=np.zeros(B, np.int32), fetch_pos=np.zeros((B, fetch), np.int32),
               fetch_scores=np.full((B, fetch), -np.inf, np.float32))
    for i, c in enumerate(lists):
        if c is None:
            out["status"][i] = 5
            continue
        ff, kk = min(fetch, len(c)), min(k, fetch, len(c))
        f_pos, f_scores = M.fetch([approx[i, c]], ff)
        out["fetch_pos"][i, :ff], out["fetch_scores"][i, :ff] = f_pos[0], f_scores[0]
        pos, scores = M.rerank(f_pos, lambda _, p: exact[i, c[p]], kk)
        out["pos"][i, :kk], out["scores"][i, :kk], out["index"][i, :kk] = pos[0], scores[0], c[pos[0]]
        out["item_ids"][i, :kk], out["n_out"][i] = item_ids[c[pos[0]]], kk
    return out


def _numpy(r, fields):
    torch.cuda.synchronize()
    return {f: getattr(r, f).cpu().numpy() for f in fields}


def _same(got, exp, what):
    for f, e in exp.items():
        same = bits(got[f]) == bits(e) if e.dtype == np.float32 else got[f] == e
        assert same.all(), (what, f, np.argwhere(~same)[:5].tolist())


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d", [64, 128, 512])
def test_equals_the_model_and_search_lists(d, dtype, metric):
    from nann_amd import retrieval
    lor, x, q = _case(d, dtype)
    dix = _index(x)
    part, t = retrieval.make_partition(dix, lor, N_LISTS), retrieval.make_sq8(dix)
    sc = _scorer(metric, d, torch.float16 if dtype == "f16" else torch.bfloat16)
    probes = _probes()
    splits, rows = partition_csr(lor, N_LISTS)
    lists = [expansion(splits, rows, p) for p in probes]
    assert max(len(c) for c in lists if c is not None) <= 1024  # fetch = 1024 covers every query of the batch
    assert sorted(np.bincount(probes[probes >= 0], minlength=N_LISTS + 1)[[6, 5, 7, 8]].tolist()) == [1, 16, 17, 33]
    approx = M.approx_scores(M.encode(q), M.encode(x), metric)
    of = _exact_on_device(dix, sc, q)
    exact = np.stack([of(i, np.arange(N)) for i in range(B)])  # nann_score's bits, once
    dq, dp = cuda(q, torch.float32), cuda(probes, torch.int32)
    got = _numpy(retrieval.search_lists_sq8(dix, part, t, sc, dq, dp, 20, fetch=64, return_fetch=True), FIELDS + ("fetch_pos", "fetch_scores"))
    _same(got, _model(lists, approx, exact, dix.item_ids.cpu().numpy(), 64, 20), (d, dtype, metric))
    assert got["status"].tolist() == [0] * 37 + [5, 0, 0] and got["n_out"][36] == 0
    # fetch >= len_i: search_lists' result, bit for bit
    wide = _numpy(retrieval.search_lists_sq8(dix, part, t, sc, dq, dp, 50, fetch=1024), FIELDS)
    _same(wide, _numpy(retrieval.search_lists(dix, part, sc, dq, dp, 50), FIELDS), (d, dtype, metric, "search_lists"))


def test_answer_does_not_depend_on_the_batch():
    from nann_amd import retrieval
    lor, x, q = _case(128, "f16")
    dix = _index(x)
    part, t, sc = retrieval.make_partition(dix, lor, N_LISTS), retrieval.make_sq8(dix), _scorer("l2", 128)
    fields = FIELDS + ("fetch_pos", "fetch_scores")
    run = lambda n: _numpy(retrieval.search_lists_sq8(dix, part, t, sc, cuda(q[:n], torch.float32), cuda(_probes()[:n], torch.int32),
                                                      20, fetch=64, return_fetch=True), fields)
    batch, alone = run(B), run(16)
    _same(alone, {f: v[:16] for f, v in batch.items()}, "batch")
