"""-m gpu: k_order_perm (nann_order_kernels.h) on the device, both of its paths, and the workspace header it zeroes.
Batches larger than the plan's slots (the order only runs there) on a small index: after the call `key` and `perm` are
read back from the workspace and perm must be the stable sort of the query indices by key; ids, scores, status and
counters must be, bit for bit, those of the same call with NANN_QUERY_ORDER=0 (read once per process: one child process
computes every case's reference).  n <= 8 192 takes the fast path, 8 193 and 20 000 the tiled one."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gpu_util import bits, cuda, require_gpu, synth_index, traversal_mode

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER_SEGS, HEAD_STRIDE = 8, 32  # nann_order.h: kOrderSegs, kOrderHeadStride (words)
SIZES = [513, 577, 1025, 4096, 8192, 8193, 20000]
N_SAME = 2000
TOPN = [32] * 5 + [20]
MODE = "lds_hash"
FIELDS = ("status", "item_ids", "scores", "index", "counters")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """(device index, queries f32[20000, 64], {case: outputs of the input-order run})"""
    g, _, dix = synth_index(20000, 64, 32)
    rng = np.random.default_rng(4242)
    embs = _host(g["item_embs"]).astype(np.float32)
    q = embs[rng.integers(0, len(embs), max(SIZES))] + 0.05 * rng.standard_normal((max(SIZES), 64)).astype(np.float32)
    q = np.ascontiguousarray(q, np.float32)
    tmp = tmp_path_factory.mktemp("order_sort")
    graph, res = tmp / "g.npz", tmp / "off.npz"
    np.savez(graph, item_embs=_host(g["item_embs"]), item_ids=_host(g["item_ids"]),
             nb_values_0=_host(g["nb_values"][0]), nb_values_1=_host(g["nb_values"][1]),
             nb_row_splits_0=_host(g["nb_row_splits"][0]), nb_row_splits_1=_host(g["nb_row_splits"][1]),
             enter_points=_host(g["enter_points"]), q=q, topn=np.asarray(TOPN, np.int32))
    script = (
        "import sys, numpy as np, torch\n"
        "sys.path.insert(0, %r)\n"
        "from nann_amd import ops, retrieval\n"
        "z = np.load(sys.argv[1])\n"
        "dix = retrieval.Index(z['item_embs'], z['item_ids'], [z['nb_values_0'], z['nb_values_1']],\n"
        "                      [z['nb_row_splits_0'], z['nb_row_splits_1']], z['enter_points'])\n"
        "sc = ops.Scorer('l2', dix.d, dix.item_embs.dtype)\n"
        "retrieval.set_traversal_mode(%r)\n"
        "q = z['q']\n"
        "cases = {'n%%d' %% n: q[:n] for n in %r}\n"
        "cases['same'] = np.repeat(q[:1], %d, axis=0)\n"
        "out = {}\n"
        "for name, qq in cases.items():\n"
        "    r = retrieval.search(dix, sc, torch.as_tensor(qq).cuda(), z['topn'])\n"
        "    torch.cuda.synchronize()\n"
        "    for k in %r:\n"
        "        out[name + '_' + k] = getattr(r, k).cpu().numpy()\n"
        "np.savez(sys.argv[2], **out)\n") % (ROOT, MODE, SIZES, N_SAME, FIELDS)
    p = subprocess.run([sys.executable, "-c", script, str(graph), str(res)], env=dict(os.environ, NANN_QUERY_ORDER="0"),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    off = np.load(res)
    return dix, q, {k: off[k] for k in off.files}


def _search(dix, q):
    from nann_amd import ops, retrieval
    sc = ops.Scorer("l2", dix.d, dix.item_embs.dtype)
    with traversal_mode(MODE):
        r = retrieval.search(dix, sc, cuda(q), TOPN)
        torch.cuda.synchronize()
    return r


def _key_perm(r, n):
    """(key, perm) of the call, read back from its workspace: order_ws_bytes(n) bytes from the last 256-byte boundary that
    leaves room for them hold the heads, perm[n], key[n]"""
    head_bytes = ORDER_SEGS * HEAD_STRIDE * 4
    nbytes = (head_bytes + n * 8 + 255) // 256 * 256
    off = (r._ws.numel() - nbytes) // 256 * 256
    tail = r._ws[off:off + nbytes].cpu().numpy()
    perm = tail[head_bytes:head_bytes + n * 4].view(np.int32)
    key = tail[head_bytes + n * 4:head_bytes + n * 8].view(np.int32)
    return key, perm


def _check(r, n, off, case):
    assert n > r.plan["workgroups"], "the order only runs on a batch larger than the plan's slots"
    key, perm = _key_perm(r, n)
    assert key.min() >= 0 and key.max() < 128
    assert (perm == np.argsort(key, kind="stable")).all()
    for k in FIELDS:
        a, b = getattr(r, k).cpu().numpy(), off[case + "_" + k]
        if a.dtype == np.float32:
            a, b = bits(a), bits(b)
        assert a.shape == b.shape and (a == b).all(), k
    return key


@pytest.mark.parametrize("n", SIZES)
def test_perm_is_the_stable_sort_and_answers_match_input_order(setup, n):
    dix, q, off = setup
    key = _check(_search(dix, q[:n]), n, off, "n%d" % n)
    assert len(np.unique(key)) > 1
    assert (off["n%d_status" % n] == 0).mean() > 0.5


def test_identical_queries_make_one_bucket(setup):
    dix, q, off = setup
    r = _search(dix, np.repeat(q[:1], N_SAME, axis=0))
    key = _check(r, N_SAME, off, "same")
    assert len(np.unique(key)) == 1
    assert (_key_perm(r, N_SAME)[1] == np.arange(N_SAME)).all()


def test_header_is_zeroed_in_a_workspace_of_ones(setup, monkeypatch):
    """the ordered path issues no memset: k_order_perm clears the header (queues, hand-back counter) itself"""
    dix, q, off = setup
    n = 1025
    ws = torch.full((dix.workspace(TOPN, n).numel(),), 0xFF, dtype=torch.uint8, device=dix.device)
    monkeypatch.setattr(dix, "workspace", lambda level_topn, n_queries: ws)
    r = _search(dix, q[:n])
    assert r._ws is ws
    _check(r, n, off, "n%d" % n)
    assert r.reruns() == 0


def test_two_batch_sizes_on_one_workspace(setup, monkeypatch):
    dix, q, off = setup
    ws = torch.empty(dix.workspace(TOPN, 4096).numel(), dtype=torch.uint8, device=dix.device)
    monkeypatch.setattr(dix, "workspace", lambda level_topn, n_queries: ws)
    for n in (4096, 577, 1025):
        r = _search(dix, q[:n])
        assert r._ws is ws
        _check(r, n, off, "n%d" % n)
        assert r.reruns() == 0
