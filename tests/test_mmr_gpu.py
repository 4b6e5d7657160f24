"""-m gpu: the MMR re-ranking on its own (nann_mmr_topk / retrieval.mmr) against the numpy model of the contract (mmr_model),
bit for bit on every output.  Tables: 2 000 seeded rows per (d, row dtype), the first 80 of them 8 clusters of ten bit-identical
rows.  Lists are unranked on purpose (random scores): every position of a list can be the next pick."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mmr_model as MM
from gpu_util import bits, cuda, require_gpu
from test_search_all_gpu import _ring, _rows

pytestmark = pytest.mark.gpu
N = 2000
_CACHE = {}
OUTPUTS = ("n_out", "index", "pos", "item_ids", "scores", "mmr")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _case(d, dtype):
    """(rows of the table, item ids, device index)"""
    key = (d, dtype)
    if key not in _CACHE:
        from nann_amd import retrieval
        embs = _rows(N, d, dtype, seed=7 * d + len(dtype))
        embs[:80] = embs[np.arange(80) % 8 + 100]          # rows 0 .. 79: 8 clusters of ten bit-identical rows
        ids = np.arange(N, dtype=np.int64) * 7 + 3
        _CACHE[key] = (embs, ids, retrieval.Index(embs, ids, *_ring(N)))
    return _CACHE[key]


def _lists(b, k_in, seed, lo=0, hi=N):
    rng = np.random.default_rng(seed)
    return rng.integers(lo, hi, (b, k_in)).astype(np.int32), rng.standard_normal((b, k_in)).astype(np.float32)


def _numpy(r):
    torch.cuda.synchronize()
    return {"n_out": r.n_out.cpu().numpy(), "index": r.index.cpu().numpy(), "pos": r.pos.cpu().numpy(),
            "item_ids": r.item_ids.cpu().numpy(), "scores": r.scores.cpu().numpy(), "mmr": r.mmr.cpu().numpy()}


def _run(dix, scores, rows, n_valid, lam, sim, k, lams=None):
    from nann_amd import retrieval
    dv = retrieval.make_diversity(lam=lam, lams=lams, sim=sim)
    nv = None if n_valid is None else cuda(np.asarray(n_valid, np.int32))
    return _numpy(retrieval.mmr(dix, cuda(scores), cuda(rows), dv, k, n_valid=nv))


def _same(got, exp, what=""):
    for name in OUTPUTS:
        g, e = (bits(got[name]), bits(exp[name])) if name in ("scores", "mmr") else (got[name], exp[name])
        assert g.shape == e.shape and (g == e).all(), (what, name)


def _check(d, dtype, scores, rows, n_valid, lam, sim, k, lams=None, what=""):
    embs, ids, dix = _case(d, dtype)
    exp = MM.model(scores, rows, n_valid, embs, lam, sim, k, lams=lams, item_ids=ids)
    got = _run(dix, scores, rows, n_valid, lam, sim, k, lams=lams)
    _same(got, exp, (d, dtype, sim, lam, k, what))
    return got


def _boundary(d, dtype):
    """the longest list whose rows the kernel keeps in LDS, from the constants its header exports"""
    from nann_amd import build
    src = open(os.path.join(build.SRC_DIR, "nann_mmr.h")).read()
    c = {n: int(re.search(r"constexpr int %s = (\d+);" % n, src).group(1)) for n in ("kMmrLdsBytes", "kMmrStateBytes", "kMmrRowPad")}
    row_bytes = d * (4 if dtype == "f32" else 2)
    return (c["kMmrLdsBytes"] - c["kMmrStateBytes"]) // (row_bytes + c["kMmrRowPad"])


# ---- every (d, row dtype): list lengths, k, n_valid, both metrics ------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("d", [64, 128, 256])
def test_every_shape_equals_the_model(d, dtype):
    seed = 1000 * d + len(dtype)
    # k_in = 1: k in {0, 1}
    rows, scores = _lists(3, 1, seed)
    for k in (0, 1):
        got = _check(d, dtype, scores, rows, [1, 0, 6], 0.5, "l2", k)
        assert got["n_out"].tolist() == [k, 0, k]
    # k_in = 63, k = k_in; n_valid in {0, 1, k_in + 5, negative, none of these}: k > #valid for most
    rows, scores = _lists(5, 63, seed + 1)
    got = _check(d, dtype, scores, rows, [0, 1, 68, -2, 40], 0.5, "ip", 63)
    assert got["n_out"].tolist() == [0, 1, 63, 0, 40]
    # k_in = 64, k = 1 and k = k_in
    rows, scores = _lists(2, 64, seed + 2)
    _check(d, dtype, scores, rows, None, 0.5, "l2", 1)
    _check(d, dtype, scores, rows, None, 0.0, "l2", 64)
    # k_in = 65: one entry beyond a wavefront; lambda 0 and 1
    rows, scores = _lists(2, 65, seed + 3)
    _check(d, dtype, scores, rows, None, 0.0, "ip", 65)
    got = _check(d, dtype, scores, rows, [65, 70], 1.0, "l2", 65)
    order = np.stack([np.lexsort((np.arange(65), -(s + np.float32(0)))) for s in scores])
    assert (got["pos"] == order).all()                                   # lambda == 1: score descending, position ascending
    # k_in = 257 and 1024, a few dozen picks, both metrics
    rows, scores = _lists(2, 257, seed + 4)
    _check(d, dtype, scores, rows, [257, 200], 0.5, "ip", 30)
    rows, scores = _lists(2, 1024, seed + 5)
    _check(d, dtype, scores, rows, [1029, 1000], 0.5, "l2", 20)
    _check(d, dtype, scores, rows, None, 0.3, "ip", 12)


def test_the_longest_list_picked_to_the_end():
    rows, scores = _lists(1, 1024, 77)
    got = _check(128, "f16", scores, rows, None, 0.5, "l2", 1024)
    assert got["n_out"].tolist() == [1024] and sorted(got["pos"][0].tolist()) == list(range(1024))


def test_d_512():
    rows, scores = _lists(2, 130, 78)
    _check(512, "f16", scores, rows, None, 0.5, "l2", 40)
    _check(512, "f16", scores, rows, None, 0.5, "ip", 40)


# ---- lambdas per query -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", ["l2", "ip"])
def test_lambdas_mixed_in_one_batch(sim):
    lams = np.array([0.0, 0.5, 1.0, 2.0, np.nan, 0.25, -1.0], np.float32)
    rows, scores = _lists(1, 65, 91)
    rows, scores = np.repeat(rows, len(lams), 0), np.repeat(scores, len(lams), 0)       # one list under every lambda
    got = _check(128, "f16", scores, rows, None, 0.9, sim, 65, lams=lams)
    assert (got["pos"][2] == got["pos"][3]).all() and (got["pos"][0] == got["pos"][4]).all() and (got["pos"][0] == got["pos"][6]).all()
    assert (got["pos"][1] != got["pos"][2]).any()
    # each of the batch's lambdas, as the one lambda of a call of its own: the same answer
    embs, ids, dix = _case(128, "f16")
    for i, lam in enumerate([0.0, 0.5, 1.0, 1.0, 0.0, 0.25, 0.0]):
        alone = _run(dix, scores[i:i + 1], rows[i:i + 1], None, lam, sim, 65)
        for name in OUTPUTS:
            assert (bits(alone[name]) == bits(got[name][i:i + 1])).all() if name in ("scores", "mmr") else (alone[name] == got[name][i:i + 1]).all()


# ---- ties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("sim", ["l2", "ip"])
def test_clusters_of_identical_rows(dtype, sim):
    """every list row is one of 8 vectors: equal similarities everywhere, +0 between copies under L2; a few equal scores on top"""
    rows, scores = _lists(4, 200, 55, lo=0, hi=80)
    scores[:, ::3] = np.float32(0.5)
    scores[1] = np.float32(1.0)                                          # every r equal: positions alone decide step 0
    scores[2, ::2] = np.float32(-0.0)
    for lam in (0.0, 0.5, 1.0):
        _check(128, dtype, scores, rows, None, lam, sim, 60, what="clusters")
    embs, _, _ = _case(128, dtype)
    if sim == "l2":
        a = MM.widen(embs)[:8]
        assert (bits(MM.l2_scores(a[3], a[[3]])) == 0).all()             # the similarity of a row to its copy is +0


# ---- invalid entries, duplicates ----------------------------------------------------------------------------------------------
def test_malformed_entries_are_dropped():
    rows, scores = _lists(3, 100, 66)
    rows[0, ::7] = [-1, N, N + 5, 2 ** 31 - 1, -2 ** 31, -7, N, -1, N, N + 1, -3, N, -1, N, N]
    scores[1, ::5] = np.array([np.nan, np.inf, -np.inf, np.nan] * 5, np.float32)
    rows[2, :] = rows[2, 0]                                               # one row, a hundred times: a hundred candidates
    rows[1, 50:60] = rows[1, 40:50]
    got = _check(128, "f16", scores, rows, None, 0.5, "l2", 100)
    assert got["n_out"].tolist() == [85, 80, 100]
    assert (got["index"][2] == rows[2, 0]).all() and sorted(got["pos"][2].tolist()) == list(range(100))
    # nothing valid at all
    rows[:] = -1
    got = _check(128, "f16", scores, rows, None, 0.5, "l2", 10)
    assert not got["n_out"].any() and not got["index"].any()


# ---- the two paths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dtype", [(128, "f16"), (128, "bf16"), (128, "f32"), (64, "f16"), (256, "f32")])
def test_both_sides_of_the_lds_boundary(d, dtype):
    edge = _boundary(d, dtype)
    assert 1 < edge < 1024
    outs = []
    for k_in in (edge, edge + 1):
        rows, scores = _lists(2, edge + 1, 88 + d)
        scores[:, edge] = np.float32(9.0)                                 # the entry only the longer list has is its first pick
        for sim in ("l2", "ip"):
            outs.append(_check(d, dtype, scores[:, :k_in].copy(), rows[:, :k_in].copy(), None, 0.5, sim, 24, what=("edge", k_in)))
    assert (outs[2]["pos"][:, 0] == edge).all() and (outs[0]["pos"][:, 0] != edge).all()
    # the same list through both paths: n_valid cuts the longer call's list to the shorter one's
    embs, ids, dix = _case(d, dtype)
    rows, scores = _lists(2, edge + 1, 188 + d)
    for sim in ("l2", "ip"):
        lds = _run(dix, scores[:, :edge].copy(), rows[:, :edge].copy(), None, 0.5, sim, 24)
        tab = _run(dix, scores, rows, [edge, edge], 0.5, sim, 24)
        for name in OUTPUTS:
            assert (lds[name].view(np.uint8) == tab[name].view(np.uint8)).all(), (sim, name)


# ---- a batch larger than the device ------------------------------------------------------------------------------------------------
def test_300_queries_each_as_alone():
    rows, scores = _lists(300, 64, 99)
    nv = np.random.default_rng(5).integers(-2, 70, 300).astype(np.int32)
    nv[:10] = 64
    lams = np.random.default_rng(6).random(300).astype(np.float32)
    embs, ids, dix = _case(64, "f16")
    got = _run(dix, scores, rows, nv, 0.5, "l2", 30, lams=lams)
    exp = MM.model(scores[:10], rows[:10], nv[:10], embs, 0.5, "l2", 30, lams=lams[:10], item_ids=ids)
    _same({n: got[n][:10] for n in OUTPUTS}, exp, "the first ten against the model")
    assert (got["n_out"] == np.minimum(30, np.clip(nv, 0, 64))).all()
    from nann_amd import retrieval
    sd, rd, nd = cuda(scores), cuda(rows), cuda(nv)
    alone = [retrieval.mmr(dix, sd[i:i + 1], rd[i:i + 1], retrieval.make_diversity(lams=lams[i:i + 1], sim="l2"), 30, n_valid=nd[i:i + 1])
             for i in range(300)]
    torch.cuda.synchronize()
    for name, field in (("n_out", "n_out"), ("index", "index"), ("pos", "pos"), ("item_ids", "item_ids"), ("scores", "scores"), ("mmr", "mmr")):
        stacked = torch.cat([getattr(r, field) for r in alone]).cpu().numpy()
        assert (stacked.view(np.uint8) == got[name].view(np.uint8)).all(), name


# ---- NULL outputs ----------------------------------------------------------------------------------------------------------------
def test_null_outputs():
    from nann_amd import _lib
    from nann_amd.ops import _ptr, _stream
    L = _lib.lib()
    embs, ids, dix = _case(128, "f16")
    rows, scores = _lists(3, 70, 44)
    nv = np.array([70, 9, 0], np.int32)
    exp = MM.model(scores, rows, nv, embs, 0.5, "l2", 20, item_ids=ids)
    sd, rd, nd = cuda(scores), cuda(rows), cuda(nv)
    dv = _lib.Diversity()
    dv.struct_bytes, dv.lam, dv.lambdas, dv.sim = 0, 0.5, None, _lib.SCORER_L2       # (struct_bytes 0 is accepted)
    names = ("index", "scores", "mmr", "pos", "item_ids", "n_out")
    dts = {"index": torch.int32, "scores": torch.float32, "mmr": torch.float32, "pos": torch.int32, "item_ids": torch.int64,
           "n_out": torch.int32}
    for keep in (("index",), ("index", "n_out"), ("index", "mmr", "item_ids"), names):
        o = {n: torch.full((3,) if n == "n_out" else (3, 20), 77, dtype=dts[n], device="cuda") for n in keep}
        rc = L.nann_mmr_topk(dix.handle, _ptr(sd), _ptr(rd), _ptr(nd), 3, 70, C.byref(dv), 20, *[_ptr(o.get(n)) for n in names], _stream())
        assert rc == 0, L.nann_last_error()
        torch.cuda.synchronize()
        for n in keep:
            assert (o[n].cpu().numpy().view(np.uint8) == exp[n].view(np.uint8)).all(), (keep, n)
    # n_valid == NULL: every entry counts
    o = torch.empty((3, 20), dtype=torch.int32, device="cuda")
    assert L.nann_mmr_topk(dix.handle, _ptr(sd), _ptr(rd), None, 3, 70, C.byref(dv), 20, _ptr(o), None, None, None, None, None, _stream()) == 0
    torch.cuda.synchronize()
    assert (o.cpu().numpy() == MM.model(scores, rows, None, embs, 0.5, "l2", 20)["index"]).all()
    # k == 0 and an empty batch write nothing
    o.fill_(77)
    assert L.nann_mmr_topk(dix.handle, _ptr(sd), _ptr(rd), None, 3, 70, C.byref(dv), 0, _ptr(o), None, None, None, None, None, _stream()) == 0
    assert L.nann_mmr_topk(dix.handle, _ptr(sd), _ptr(rd), None, 0, 70, C.byref(dv), 20, _ptr(o), None, None, None, None, None, _stream()) == 0
    torch.cuda.synchronize()
    assert (o.cpu() == 77).all()
