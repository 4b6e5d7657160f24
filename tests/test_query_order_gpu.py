"""-m gpu: the locality order of a batch (nann_order.h) and the per-XCD queues of k_search.  The order decides only which
slot runs which query when: ids, scores, status and counters must be the input-order run's, bit for bit, at every batch
shape, with per-query level_topn, with every query in one bucket, and across the capacity rerun."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gpu_util import bits, cuda, queries_for, require_gpu, synth_index, traversal_mode

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER_SEGS, HEAD_STRIDE = 8, 32  # nann_order.h: kOrderSegs, kOrderHeadStride (words)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _search(dix, q, topn, mode):
    from nann_amd import ops, retrieval
    sc = ops.Scorer("l2", dix.d, dix.item_embs.dtype)
    with traversal_mode(mode):
        r = retrieval.search(dix, sc, cuda(q), topn)
        torch.cuda.synchronize()
    return r


def _out(r):
    return (r.status.cpu().numpy(), r.item_ids.cpu().numpy(), r.scores.cpu().numpy(), r.index.cpu().numpy(),
            r.counters.cpu().numpy())


def _assert_equal(got, exp):
    for a, b in zip(got, exp):
        a, b = np.asarray(a), np.asarray(b)
        if a.dtype == np.float32:
            a, b = bits(a), bits(b)
        assert a.shape == b.shape and (a == b).all()


def _in_chunks(dix, q, topn, mode, chunk):
    """the same queries in batches no larger than the plan's slots: input order, no order pass"""
    parts = [_out(_search(dix, q[i:i + chunk], topn[i:i + chunk] if np.ndim(topn) == 2 else topn, mode))
             for i in range(0, len(q), chunk)]
    return tuple(np.concatenate([p[j] for p in parts]) for j in range(5))


def _order_of(r, n):
    """(perm, heads) read back from the call's workspace: order_ws_bytes(n) bytes from the last 256-byte boundary
    that leaves room for them"""
    nbytes = (ORDER_SEGS * HEAD_STRIDE * 4 + n * 8 + 255) // 256 * 256
    off = (r._ws.numel() - nbytes) // 256 * 256
    tail = r._ws[off:off + nbytes].cpu().numpy()
    heads = tail[:ORDER_SEGS * HEAD_STRIDE * 4].view(np.uint32)[::HEAD_STRIDE]
    perm = tail[ORDER_SEGS * HEAD_STRIDE * 4:ORDER_SEGS * HEAD_STRIDE * 4 + n * 4].view(np.int32)
    return perm, heads


def _queries(oracle, g, n, seed):
    return np.stack([oracle.user_seq_mean(s) for s in queries_for(g, n, seed=seed)])


@pytest.mark.parametrize("mode", ["lds_hash", "lds_hash32"])
def test_batch_shapes_match_the_oracle_and_the_order_is_a_permutation(oracle, mode):
    g, oix, dix = synth_index(20000, 64, 32)
    topn = [32] * 5 + [20]
    q = _queries(oracle, g, 4097, 77)
    exp = oracle.search_batch(oix, oracle.Scorer("l2", 64, oracle.EMB_F16), q, topn, n_threads=8)
    assert (exp[0] == 0).mean() > 0.5
    slots = _search(dix, q, topn, mode).plan["workgroups"]  # (a plan never has more slots than queries: ask with all)
    for n in (1, 7, slots - 1, slots + 1, 4096, 4097):
        r = _search(dix, q[:n], topn, mode)
        _assert_equal(_out(r), tuple(e[:n] for e in exp))
        if n > slots:  # the order ran: perm is a permutation, every segment was drained
            perm, heads = _order_of(r, n)
            assert (np.sort(perm) == np.arange(n)).all()
            seg = [n * s // ORDER_SEGS for s in range(ORDER_SEGS + 1)]
            assert all(heads[s] >= seg[s + 1] - seg[s] for s in range(ORDER_SEGS))


def test_order_on_and_off_are_bit_identical(oracle, tmp_path):
    """NANN_QUERY_ORDER=0 (read once per process: a child) against the default, on one saved graph"""
    g, oix, dix = synth_index(20000, 64, 32)
    topn = np.asarray([32] * 5 + [20], np.int32)
    q = _queries(oracle, g, 3000, 78)
    graph = tmp_path / "g.npz"
    np.savez(graph, item_embs=_host(g["item_embs"]), item_ids=_host(g["item_ids"]),
             nb_values_0=_host(g["nb_values"][0]), nb_values_1=_host(g["nb_values"][1]),
             nb_row_splits_0=_host(g["nb_row_splits"][0]), nb_row_splits_1=_host(g["nb_row_splits"][1]),
             enter_points=_host(g["enter_points"]), q=q, topn=topn)
    script = (
        "import sys, numpy as np, torch\n"
        "sys.path.insert(0, %r)\n"
        "from nann_amd import ops, retrieval\n"
        "z = np.load(sys.argv[1])\n"
        "dix = retrieval.Index(z['item_embs'], z['item_ids'], [z['nb_values_0'], z['nb_values_1']],\n"
        "                      [z['nb_row_splits_0'], z['nb_row_splits_1']], z['enter_points'])\n"
        "sc = ops.Scorer('l2', dix.d, dix.item_embs.dtype)\n"
        "out = {}\n"
        "for m in ('lds_hash', 'lds_hash32'):\n"
        "    retrieval.set_traversal_mode(m)\n"
        "    r = retrieval.search(dix, sc, torch.as_tensor(z['q']).cuda(), z['topn'])\n"
        "    torch.cuda.synchronize()\n"
        "    for k in ('status', 'item_ids', 'scores', 'index', 'counters'):\n"
        "        out[m + '_' + k] = getattr(r, k).cpu().numpy()\n"
        "np.savez(sys.argv[2], **out)\n") % ROOT
    res = tmp_path / "off.npz"
    env = dict(os.environ, NANN_QUERY_ORDER="0")
    p = subprocess.run([sys.executable, "-c", script, str(graph), str(res)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    off = np.load(res)
    exp = oracle.search_batch(oix, oracle.Scorer("l2", 64, oracle.EMB_F16), q[:64], list(topn), n_threads=8)
    for m in ("lds_hash", "lds_hash32"):
        on = _out(_search(dix, q, topn, m))
        _assert_equal(on, tuple(off[m + "_" + k] for k in ("status", "item_ids", "scores", "index", "counters")))
        _assert_equal(tuple(o[:64] for o in on), exp)


@pytest.mark.parametrize("mode", ["lds_hash", "lds_hash32"])
def test_one_bucket_drains_through_stealing(oracle, mode):
    """every query the same: one key, one busy segment; the other XCDs' slots take all their work from it"""
    g, oix, dix = synth_index(20000, 64, 32)
    topn = [32] * 5 + [20]
    q = np.repeat(_queries(oracle, g, 1, 79), 2000, axis=0)
    r = _search(dix, q, topn, mode)
    exp = oracle.search_batch(oix, oracle.Scorer("l2", 64, oracle.EMB_F16), q[:1], topn, n_threads=1)
    _assert_equal(_out(r), tuple(np.repeat(e, 2000, axis=0) for e in exp))
    perm, _ = _order_of(r, 2000)
    assert (perm == np.arange(2000)).all()  # the sort is stable


def test_per_query_level_topn_in_order(oracle):
    from nann_amd import ops
    g, oix, dix = synth_index(20000, 64, 32)
    variants = [[32] * 5 + [20], [16, 24, 32, 8, 12, 10], [8] * 5 + [5], [32, 32, 20, 20, 20, 20]]
    nq = 1500
    q = _queries(oracle, g, nq, 80)
    rows = np.asarray([variants[b % len(variants)] for b in range(nq)], np.int32)
    r = _search(dix, q, rows, "lds_hash")
    assert nq > r.plan["workgroups"]
    _assert_equal(_out(r), _in_chunks(dix, q, rows, "lds_hash", 200))
    sel = np.arange(0, 64 * len(variants), len(variants))
    exp = oracle.search_batch(oix, oracle.Scorer("l2", 64, oracle.EMB_F16), q[sel], variants[0], n_threads=8)
    got = _out(r)
    _assert_equal(tuple(o[sel] for o in got), exp)


def test_capacity_rerun_after_an_ordered_launch(oracle):
    """queries that outgrow the 16K-slot set are handed back by the ordered launch and rerun (input order) on the bitmap
    kernel: the call's answers equal the same queries' in batches that run without an order, and the oracle's"""
    g, oix, dix = synth_index(120000, 64, 256, n_clusters=4, mode="knn")
    topn = [256, 512, 512, 512, 512, 200]
    q = _queries(oracle, g, 600, 81)
    r = _search(dix, q, topn, "lds_hash")
    assert 600 > r.plan["workgroups"]
    assert r.reruns() > 0, "workload must overflow the set for some query"
    got = _out(r)
    _assert_equal(got, _in_chunks(dix, q, topn, "lds_hash", 48))
    exp = oracle.search_batch(oix, oracle.Scorer("l2", 64, oracle.EMB_F16), q[:16], topn, n_threads=8)
    _assert_equal(tuple(o[:16] for o in got), exp)
