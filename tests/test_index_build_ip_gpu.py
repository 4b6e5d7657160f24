"""-m gpu: the device HNSW builder and append with metric="ip" (nann_hnsw_build_device_metric / nann_hnsw_append_device_metric):
the structural invariants and determinism of a build asked of an IP-linked graph at every d and row dtype; metric="l2" is the
builder as it was; recall of the inner-product traversal on the IP-linked graph against the L2-linked one and against the host
builder's; and an append under IP.  The corpus is ip_build_cases.py's: row norms vary by 16x, and distances take both signs, so
the beam's order-preserving keys are exercised.  Truth is the exhaustive search with the same scorer."""
import numpy as np
import pytest
import torch

import ip_build_cases as cases
from gpu_util import require_gpu

pytestmark = pytest.mark.gpu
_SHARED = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _table(c, dtype="f16"):
    if dtype == "bf16":
        return torch.as_tensor(c["rows"].view(np.int16)).cuda().view(torch.bfloat16)
    return torch.as_tensor(c["rows"]).cuda()


def _ip_recall(table, ex, c):
    """(recall@50 of the IP traversal on graph `ex` over `table` against search_all with the same scorer -- a query with
    non-zero status counts as zero hits --, share of queries with status 0); asserts first that the scores take both signs"""
    from nann_amd import ops, retrieval
    n, d = table.shape
    q = torch.as_tensor(c["q"]).cuda()
    assert cases.both_signs((q @ table.float().T).cpu().numpy()), "the truth scores have one sign"
    dix = retrieval.Index(table, np.arange(n, dtype=np.int64), ex["nb_values"], ex["nb_row_splits"], ex["enter_points"])
    sc = ops.Scorer("ip", d, table.dtype)
    r = retrieval.search(dix, sc, q, cases.level_topn(len(ex["enter_points"])))
    truth = retrieval.search_all(dix, sc, q, cases.K)
    torch.cuda.synchronize()
    st = r.status.cpu().numpy()
    return cases.recall(truth.index.cpu().numpy(), r.index.cpu().numpy(), st), float((st == 0).mean())


def _case_20k():
    """20 000 x 64 f16: the corpus, its table, and the device IP build (with its state) -- shared by the recall and append tests"""
    if "c" not in _SHARED:
        from nann_amd import index_build
        c = cases.corpus(20_000, 64)
        table = _table(c)
        ip = index_build.build_hnsw_gpu(table, cases.M, cases.EF_CONSTRUCTION, seed=cases.SEED, metric="ip", want_state=True)
        _SHARED.update(c=c, table=table, ip=ip, ip_recall=_ip_recall(table, ip, c))
    return _SHARED


@pytest.mark.parametrize("n,d,dtype", [(40_000, 64, "f16"), (24_000, 128, "bf16"), (20_000, 256, "f16")])
def test_ip_build_invariants_and_determinism(n, d, dtype):
    from nann_amd import index_build
    c = cases.corpus(n, d, dtype)
    table = _table(c, dtype)
    a = index_build.build_hnsw_gpu(table, cases.M, cases.EF_CONSTRUCTION, seed=5, metric="ip", want_state=True)
    cases.check_export(a, n, cases.M)
    assert a["state"]["metric"] == "ip"
    b = index_build.build_hnsw_gpu(table, cases.M, cases.EF_CONSTRUCTION, seed=5, metric="ip", want_state=True)
    for k in ("adj0", "up_row", "adj_up"):
        assert torch.equal(a["state"][k], b["state"][k]), k
    assert (a["enter_points"] == b["enter_points"]).all()
    for l in (0, 1):
        assert (a["nb_values"][l] == b["nb_values"][l]).all() and (a["nb_row_splits"][l] == b["nb_row_splits"][l]).all()
    # ... and it is not the L2 graph of these rows
    l2 = index_build.build_hnsw_gpu(table, cases.M, cases.EF_CONSTRUCTION, seed=5)
    assert len(l2["nb_values"][0]) != len(a["nb_values"][0]) or (l2["nb_values"][0] != a["nb_values"][0]).any()
    print(f"mean level-0 degree {n} x {d} {dtype}: ip {len(a['nb_values'][0]) / n:.2f}, l2 {len(l2['nb_values'][0]) / n:.2f}")


def test_l2_metric_is_the_default_build_on_the_device():
    from nann_amd import index_build
    s = _case_20k()
    a = index_build.build_hnsw_gpu(s["table"], cases.M, cases.EF_CONSTRUCTION, seed=cases.SEED, want_state=True, want_raw=True)
    b = index_build.build_hnsw_gpu(s["table"], cases.M, cases.EF_CONSTRUCTION, seed=cases.SEED, want_state=True, want_raw=True, metric="l2")
    assert a["state"]["metric"] == b["state"]["metric"] == "l2"
    for k in ("adj0", "up_row", "adj_up"):
        assert torch.equal(a["state"][k], b["state"][k]), k
    assert (a["levels"] == b["levels"]).all() and (a["enter_points"] == b["enter_points"]).all()
    for l in (0, 1):
        assert (a["nb_values"][l] == b["nb_values"][l]).all() and (a["nb_row_splits"][l] == b["nb_row_splits"][l]).all()
    for k in a["raw"]:
        assert (a["raw"][k] == b["raw"][k]).all(), k
    _SHARED["l2"] = a


def test_ip_recall_on_the_device_built_graph():
    """At 20 000 x 64 f16: the IP traversal on the device's IP-linked graph recalls at least 0.25 more than on its L2-linked
    graph (the host builder's gap is 0.6), at least the host IP graph's recall - 0.02 (the margin the device builder is given
    against the host builder under L2), and at least 95 % of the queries succeed.  Measured on the MI355X: device IP graph 0.868
    (all queries succeed), device L2 graph 0.252 (83 % succeed), host IP graph 0.872."""
    from nann_amd import index_build
    s = _case_20k()
    c, table = s["c"], s["table"]
    ip, ok = s["ip_recall"]
    l2_graph = _SHARED.get("l2") or index_build.build_hnsw_gpu(table, cases.M, cases.EF_CONSTRUCTION, seed=cases.SEED)
    l2, l2_ok = _ip_recall(table, l2_graph, c)
    raw = index_build.build_hnsw(c["wide"], cases.M, cases.EF_CONSTRUCTION, seed=cases.SEED, n_threads=1, metric="ip")
    host, host_ok = _ip_recall(table, index_build.export_levels(raw, 2), c)
    deg = {"ip": len(s["ip"]["nb_values"][0]) / 20_000, "l2": len(l2_graph["nb_values"][0]) / 20_000}
    msg = f"recall@50 under IP (share of queries with status 0): device IP graph {ip:.3f} ({ok:.2f}), device L2 graph {l2:.3f} " \
          f"({l2_ok:.2f}), host IP graph {host:.3f} ({host_ok:.2f}); mean level-0 degree {deg}"
    print(msg)
    assert ip >= l2 + 0.25, msg
    assert ip >= host - 0.02, msg
    assert ok >= 0.95, msg


def test_append_under_ip():
    """16 000 rows built and 4 000 appended under IP: the invariants of a build, the input state untouched, the device export an
    Index the IP traversal accepts, recall@50 within 0.02 of the 20 000-row IP build's (the margin tests/test_index_append_gpu.py
    gives an append).  Measured on the MI355X: appended 0.868, built 0.868."""
    from nann_amd import index_build
    s = _case_20k()
    c, table = s["c"], s["table"]
    n_old, n = 16_000, 20_000
    base = index_build.build_hnsw_gpu(table[:n_old].contiguous(), cases.M, cases.EF_CONSTRUCTION, seed=cases.SEED, metric="ip", want_state=True)
    st0 = base["state"]
    keep = {k: (v.clone() if isinstance(v, torch.Tensor) else (v.copy() if isinstance(v, np.ndarray) else v)) for k, v in st0.items()}
    a = index_build.append_hnsw_gpu(st0, table[n_old:], seed=7)
    sa = a["state"]
    assert sa["metric"] == "ip" and set(sa) == set(st0) and sa["adj0"].shape == (n, 2 * cases.M)
    assert (sa["levels"][:n_old] == st0["levels"]).all()
    cases.check_export(a, n, cases.M)
    assert (np.diff(a["nb_row_splits"][0])[n_old:] > 0).all(), "an appended node without a level-0 row"
    # the input state is as it was
    for k, v in keep.items():
        assert (torch.equal(st0[k], v) if isinstance(v, torch.Tensor) else np.array_equal(st0[k], v)), k
    # the same append again gives the same arrays
    b = index_build.append_hnsw_gpu(st0, table[n_old:], seed=7, want_export=False)["state"]
    for k in ("adj0", "up_row", "adj_up"):
        assert torch.equal(sa[k], b[k]), k
    # the device export is an Index the IP traversal accepts (_ip_recall builds it from device tensors), and equals the torch export
    ex = index_build.export_hnsw_gpu(sa)
    assert ex["enter_points"].is_cuda and (ex["enter_points"].cpu().numpy() == a["enter_points"]).all()
    for l in (0, 1):
        assert (ex["nb_values"][l].cpu().numpy() == a["nb_values"][l]).all()
    got, ok = _ip_recall(sa["item_embs"], ex, c)
    built, _ = s["ip_recall"]
    msg = f"recall@50 under IP: appended 16 000 + 4 000 {got:.3f} ({ok:.2f} of the queries succeed), built 20 000 {built:.3f}"
    print(msg)
    assert got >= built - 0.02, msg
