"""-m gpu: the lean instantiation of the L2 / inner-product hash-set kernel (k_search_lean, nann_search.h).  A plain call -- uniform
level_topn, no phase ticks, at most 2^20 items -- launches it; every other call the general kernel.  It is the same kernel with
its phase timers off at compile time, so item ids, scores, rows, status and counters must be the general kernel's bit for bit:
with phase ticks requested (general kernel, same process), with NANN_LEAN_KERNEL=0 (read once per process: a child), for
failing requests, and across the capacity hand-back."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gpu_util import bits, cuda, require_gpu, traversal_mode
from test_hash_boundary_gpu import _regular_random_index

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M, NQ = 20_000, 16, 700            # 700 queries: more than a plan's slots (512 / 256), so the locality order runs
TOPN = [32] * 5 + [50]
DIMS = (64, 128)                      # 8 and 16 lanes per row
HASH_MODES = ("lds_hash", "lds_hash32")
KINDS = ("l2", "ip")
FIELDS = ("status", "item_ids", "scores", "index", "counters")
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _case(d):
    """20 000 f16 rows under a graph of the device builder at M = 16 -> dict(g, dix, q f32[700, d] on the host).  Four clusters
    of ~5 000 rows: in clusters of ~300 (gpu_util.synth_index's 64) three requests in four run out of new nodes within a
    level-0 round at this M and fail (TopKV2: k > n) before the later rounds run."""
    from nann_amd import index_build, ops, retrieval, synth
    if d not in _CACHE:
        embs, assign = synth.make_corpus(N, d, n_clusters=4, noise=1.0)
        ex = index_build.build_hnsw_gpu(cuda(embs), M, 40, seed=9)
        g = {"item_embs": embs, "item_ids": synth.make_item_ids(N), "nb_values": [v.astype(np.int32) for v in ex["nb_values"]],
             "nb_row_splits": [np.asarray(r, np.int64) for r in ex["nb_row_splits"]], "enter_points": ex["enter_points"].astype(np.int32)}
        assert len(g["enter_points"]) >= TOPN[0], len(g["enter_points"])
        q = ops.user_seq_mean(cuda(synth.make_queries(embs, assign, NQ, seed=41))).cpu().numpy()
        _CACHE[d] = {"g": g, "dix": retrieval.Index.from_dict(g), "q": q}
    return _CACHE[d]


def _scorer(kind, d):
    from nann_amd import ops
    return ops.Scorer(kind, d, torch.float16)


def _search(dix, sc, q, topn, mode, **kw):
    from nann_amd import retrieval
    with traversal_mode(mode):
        r = retrieval.search(dix, sc, cuda(q), topn, **kw)
        torch.cuda.synchronize()
    return r


def _out(r):
    return tuple(getattr(r, k).cpu().numpy() for k in FIELDS)


def _assert_equal(got, exp, what=None):
    for name, a, b in zip(FIELDS, got, exp):
        a, b = np.asarray(a), np.asarray(b)
        if a.dtype == np.float32:
            a, b = bits(a), bits(b)
        assert a.shape == b.shape and (a == b).all(), (what, name)


_CHILD = (
    "import sys, numpy as np, torch\n"
    "sys.path.insert(0, %r)\n"
    "from nann_amd import ops, retrieval\n"
    "out = {}\n"
    "for d in (64, 128):\n"
    "    z = np.load(sys.argv[1] %% d)\n"
    "    dix = retrieval.Index(z['item_embs'], z['item_ids'], [z['nb_values_0'], z['nb_values_1']],\n"
    "                          [z['nb_row_splits_0'], z['nb_row_splits_1']], z['enter_points'])\n"
    "    for kind in ('l2', 'ip'):\n"
    "        sc = ops.Scorer(kind, d, torch.float16)\n"
    "        for m in ('lds_hash', 'lds_hash32'):\n"
    "            retrieval.set_traversal_mode(m)\n"
    "            r = retrieval.search(dix, sc, torch.as_tensor(z['q']).cuda(), [int(t) for t in z['topn']])\n"
    "            torch.cuda.synchronize()\n"
    "            tag = '%%d_%%s_%%s_' %% (d, kind, m)\n"
    "            out[tag + 'lean'] = np.int32(r.plan['lean'])\n"
    "            for k in ('status', 'item_ids', 'scores', 'index', 'counters'):\n"
    "                out[tag + k] = getattr(r, k).cpu().numpy()\n"
    "np.savez(sys.argv[2], **out)\n") % ROOT


@pytest.fixture(scope="module")
def switched_off(tmp_path_factory):
    """every (d, scorer, mode) of the parity test in ONE fresh process under NANN_LEAN_KERNEL=0 -> the npz it wrote"""
    tmp = tmp_path_factory.mktemp("lean")
    for d in DIMS:
        c = _case(d)
        g = c["g"]
        np.savez(tmp / ("g%d.npz" % d), item_embs=g["item_embs"], item_ids=g["item_ids"], nb_values_0=g["nb_values"][0],
                 nb_values_1=g["nb_values"][1], nb_row_splits_0=g["nb_row_splits"][0], nb_row_splits_1=g["nb_row_splits"][1],
                 enter_points=g["enter_points"], q=c["q"], topn=np.asarray(TOPN, np.int32))
    res = tmp / "off.npz"
    env = dict(os.environ, NANN_LEAN_KERNEL="0")
    p = subprocess.run([sys.executable, "-c", _CHILD, str(tmp / "g%d.npz"), str(res)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return np.load(res)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", HASH_MODES)
@pytest.mark.parametrize("d", DIMS)
def test_lean_equals_general_bit_for_bit(switched_off, d, mode, kind):
    c = _case(d)
    sc = _scorer(kind, d)
    lean = _search(c["dix"], sc, c["q"], TOPN, mode)
    assert lean.plan["visited_set"] == mode and lean.plan["lean"] == 1, lean.plan
    assert NQ > lean.plan["workgroups"]
    general = _search(c["dix"], sc, c["q"], TOPN, mode, want_phase_ticks=True)
    assert general.plan["lean"] == 0, general.plan
    got = _out(lean)
    assert (got[0] == 0).mean() > 0.5, "most requests succeed"
    _assert_equal(got, _out(general), "phase ticks requested")
    tag = "%d_%s_%s_" % (d, kind, mode)
    assert int(switched_off[tag + "lean"]) == 0
    _assert_equal(got, tuple(switched_off[tag + k] for k in FIELDS), "NANN_LEAN_KERNEL=0")


@pytest.mark.parametrize("mode", HASH_MODES)
def test_lean_equals_the_oracle(oracle, mode):
    c = _case(64)
    g = c["g"]
    oix = oracle.Index(g["item_embs"], g["item_ids"], g["nb_values"], g["nb_row_splits"], g["enter_points"])
    exp = oracle.search_batch(oix, oracle.Scorer("l2", 64, oracle.EMB_F16), c["q"][:48], TOPN, n_threads=8)
    r = _search(c["dix"], _scorer("l2", 64), c["q"], TOPN, mode)
    assert r.plan["lean"] == 1
    _assert_equal(tuple(o[:48] for o in _out(r)), exp, mode)


def test_dispatch():
    """plan["lean"]: 1 for the plain call; 0 with phase ticks, a per-query level_topn, on the bitmap plans and under the MLP"""
    from nann_amd import ops, synth
    c = _case(128)
    dix, q = c["dix"], c["q"][:40]
    for kind in KINDS:
        sc = _scorer(kind, 128)
        for mode in HASH_MODES:
            assert _search(dix, sc, q, TOPN, mode).plan["lean"] == 1, (kind, mode)
            assert _search(dix, sc, q, TOPN, mode, want_phase_ticks=True).plan["lean"] == 0, (kind, mode)
            rows = np.tile(np.asarray(TOPN, np.int32), (len(q), 1))
            assert _search(dix, sc, q, rows, mode).plan["lean"] == 0, (kind, mode)
        for mode in ("lds_bitmap", "hbm_bitmap"):
            r = _search(dix, sc, q, TOPN, mode)
            assert r.plan["visited_set"] == mode and r.plan["lean"] == 0, (kind, mode)
    mlp = ops.Scorer("mlp", 128, torch.float16, synth.make_mlp_weights(128), precision="split")
    for mode in ("auto", "lds_hash"):
        assert _search(dix, mlp, q, TOPN, mode).plan["lean"] == 0, mode


def _halves_index(n=400, d=64, n_enter=40, seed=5):
    """A graph on which the same call fails some requests and serves others: entry nodes 0..19 lie around +e0 and lead on at
    level 1, entry nodes 20..39 lie around -e0 and have empty level-1 rows -- a query on their side finds nothing to score in
    round 1 (NANN_ERR_EMPTY_SCORE_BATCH)."""
    rng = np.random.default_rng(seed)
    embs = (rng.standard_normal((n, d)) * 0.1).astype(np.float16)
    embs[:20, 0] += 2.0
    embs[20:40, 0] -= 2.0
    len1 = np.zeros(n, np.int64)
    len1[:20] = 6
    rs1 = np.concatenate([[0], np.cumsum(len1)]).astype(np.int64)
    nb1 = rng.integers(n_enter, n, size=int(rs1[-1])).astype(np.int32)
    nb0 = rng.integers(0, n, size=n * 8).astype(np.int32)
    rs0 = np.arange(n + 1, dtype=np.int64) * 8
    return dict(item_embs=embs, item_ids=(rng.permutation(n) + 1).astype(np.int64), nb_values=[nb0, nb1], nb_row_splits=[rs0, rs1],
                enter_points=np.arange(n_enter, dtype=np.int32))


@pytest.mark.parametrize("mode", HASH_MODES)
def test_failing_requests_through_the_lean_kernel(oracle, mode):
    """status and zeroed rows of requests the reference fails: (1) every query, on an index with fewer enter points than
    level_topn[0] (TopKV2: k > n); (2) some queries of a batch, with nothing to score in round 1 -- the early returns"""
    from nann_amd import retrieval
    sc = _scorer("l2", 64)
    # (1)
    c = _case(64)
    g = dict(c["g"], enter_points=c["g"]["enter_points"][:TOPN[0] - 8])
    few = retrieval.Index.from_dict(g)
    q = c["q"][:64]
    lean = _search(few, sc, q, TOPN, mode)
    general = _search(few, sc, q, TOPN, mode, want_phase_ticks=True)
    assert (lean.plan["lean"], general.plan["lean"]) == (1, 0)
    got = _out(lean)
    assert (got[0] == oracle.ERR_TOPK_K_GT_N).all(), got[0]
    assert not got[1].any() and not bits(got[2]).any() and not got[3].any()
    _assert_equal(got, _out(general), "k > n")
    # (2)
    h = _halves_index()
    oix = oracle.Index(h["item_embs"], h["item_ids"], h["nb_values"], h["nb_row_splits"], h["enter_points"])
    dix = retrieval.Index(h["item_embs"], h["item_ids"], h["nb_values"], h["nb_row_splits"], h["enter_points"])
    rng = np.random.default_rng(6)
    q = (rng.standard_normal((24, 64)) * 0.1).astype(np.float32)
    q[:, 0] += np.where(np.arange(24) % 3 == 0, -2.0, 2.0)
    topn = [8, 8, 8, 8, 8, 10]
    exp = oracle.search_batch(oix, oracle.Scorer("l2", 64, oracle.EMB_F16), q, topn)
    assert (exp[0] == oracle.ERR_EMPTY_SCORE_BATCH).sum() >= 4 and (exp[0] == 0).sum() >= 4, exp[0]
    lean = _search(dix, sc, q, topn, mode)
    general = _search(dix, sc, q, topn, mode, want_phase_ticks=True)
    assert (lean.plan["lean"], general.plan["lean"]) == (1, 0)
    got = _out(lean)
    failed = got[0] != 0
    assert not got[1][failed].any() and not bits(got[2][failed]).any() and not got[3][failed].any()
    _assert_equal(got, _out(general), "empty score batch")
    _assert_equal(got, exp, "oracle")


def test_capacity_hand_back_from_the_lean_kernel():
    """test_hash_boundary_gpu's smallest overflowing case: beams of 200 on a degree-64 random graph of 20 k items fill the
    16K-slot set; the lean kernel hands every query to the rerun (the general bitmap kernel) like the general one does"""
    from nann_amd import retrieval
    g = _regular_random_index(20_000, 64, 320, seed=77)
    dix = retrieval.Index(g["item_embs"], g["item_ids"], g["nb_values"], g["nb_row_splits"], g["enter_points"])
    q = (np.random.default_rng(5).standard_normal((12, 64)) * 0.3).astype(np.float32)
    topn = [200] * 5 + [100]
    sc = _scorer("l2", 64)
    lean = _search(dix, sc, q, topn, "lds_hash")
    assert lean.plan["visited_set"] == "lds_hash" and lean.plan["lean"] == 1, lean.plan
    assert lean.reruns() > 0
    general = _search(dix, sc, q, topn, "lds_hash", want_phase_ticks=True)
    assert general.plan["lean"] == 0 and general.reruns() == lean.reruns()
    got = _out(lean)
    assert (got[0] == 0).all(), got[0]
    _assert_equal(got, _out(general))
