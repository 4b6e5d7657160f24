"""CPU: the HNSW builders take a metric.  The host builder with metric="ip" links rows by dist(a, b) = -<a, b>, and on a corpus
whose row norms carry information (ip_build_cases.py) the inner-product search recalls far better on that graph than on the
L2-linked one; metric="l2" is the builder as it was; the device entry points nann_hnsw_build_device_metric /
nann_hnsw_append_device_metric are exported and check their arguments, the metric among them, before any device call."""
import ctypes as C

import numpy as np
import pytest

import ip_build_cases as cases
from nann_amd import _lib

L2, MLP, IP = _lib.SCORER_L2, _lib.SCORER_MLP, _lib.SCORER_IP


def test_host_ip_graph_recalls_better_under_ip_than_the_l2_graph():
    """20 000 x 64, M 32, ef_construction 40, seed 9, one thread; recall@50 of the serving schedule scored by inner product
    against brute force, a failed query counted as zero hits.  Measured: IP-linked 0.872 (64 of 64 queries succeed), L2-linked
    0.247 (56 of 64).  The margin asked, 0.25, is under half that gap: the device builder's batching and another compiler's
    summation may move both sides."""
    from nann_amd import index_build
    c = cases.corpus(20_000, 64)
    scores, _ = cases.host_truth(c)
    assert cases.both_signs(scores), "the truth scores have one sign: the corpus does not exercise signed distances"
    got = {}
    for metric in ("ip", "l2"):
        kw = {"metric": "ip"} if metric == "ip" else {}
        raw = index_build.build_hnsw(c["wide"], cases.M, cases.EF_CONSTRUCTION, seed=cases.SEED, n_threads=1, **kw)
        ex = index_build.export_levels(raw, 2)
        ex["levels"] = raw["levels"]
        if metric == "ip":
            cases.check_export(ex, 20_000, cases.M)
        got[metric] = cases.host_recall(c, ex) + (len(ex["nb_values"][0]) / 20_000,)
    print("host builder, (recall@50 under IP, queries that succeeded, mean level-0 degree):", got)
    assert got["ip"][0] >= got["l2"][0] + 0.25, f"IP-linked {got['ip']}, L2-linked {got['l2']}"


def test_host_l2_metric_is_the_default_build():
    from nann_amd import index_build, synth
    embs = synth.make_corpus(3000, 64, n_clusters=8, noise=1.0, seed=5)[0].astype(np.float32)
    a = index_build.build_hnsw(embs, 32, seed=2, n_threads=1)
    b = index_build.build_hnsw(embs, 32, seed=2, n_threads=1, metric="l2")
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and (a[k] == b[k]).all(), k
    c = index_build.build_hnsw(embs, 32, seed=2, n_threads=1, metric="ip")
    assert (c["levels"] == a["levels"]).all() and (c["neighbors"] != a["neighbors"]).any()


def test_python_builders_refuse_other_metrics(tmp_path):
    from nann_amd import index_build
    x = np.zeros((8, 64), np.float32)
    for bad in ("cosine", "L2", "", None, 2):
        with pytest.raises(ValueError, match="metric"):
            index_build.build_hnsw(x, metric=bad)
        with pytest.raises(ValueError, match="metric"):
            index_build.build_and_save_index(x, 2, 32, str(tmp_path), metric=bad)
        with pytest.raises(ValueError, match="metric"):
            index_build.build_hnsw_gpu(x.astype(np.float16), metric=bad)  # refused before a device is touched
        with pytest.raises(ValueError, match="metric"):
            index_build.append_hnsw_gpu({"metric": bad}, x.astype(np.float16), seed=1)


def test_libraries_export_the_three_calls():
    from nann_amd import index_build
    L = _lib.lib()
    for name in ("nann_hnsw_build_device_metric", "nann_hnsw_append_device_metric"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.nann_abi_version() == 6  # symbols were added, nothing else changed
    assert hasattr(index_build._lib(), "nann_hnsw_build_metric") and hasattr(index_build._lib(), "nann_hnsw_build")


def _ptrs(embs, arrays):
    buf = np.zeros(16, np.int32)
    p = lambda on: C.c_void_p(buf.ctypes.data if on else 0)
    return buf, p(embs), [p(a) for a in arrays]


def _build(L, metric, embs=1, n=100, d=64, dtype=_lib.F16, m=16, ef=40, levels=None, arrays=(1, 1, 1)):
    """nann_hnsw_build_device_metric with host addresses that are never dereferenced: every case is refused before a device call"""
    lv = np.ones(n, np.int32) if levels is None else levels
    buf, e, a = _ptrs(embs, arrays)
    return L.nann_hnsw_build_device_metric(e, n, d, dtype, m, ef, 0, metric, C.c_void_p(lv.ctypes.data), a[0], a[1], a[2], None)


def _append(L, metric, embs=1, n_old=100, n_new=10, d=64, dtype=_lib.F16, m=16, ef=40, levels=None, arrays=(1, 1, 1)):
    lv = np.ones(n_old + max(n_new, 0), np.int32) if levels is None else levels
    buf, e, a = _ptrs(embs, arrays)
    return L.nann_hnsw_append_device_metric(e, n_old, n_new, d, dtype, m, ef, 0, metric, C.c_void_p(lv.ctypes.data), a[0], a[1], a[2], None)


@pytest.mark.parametrize("call", [_build, _append], ids=["build", "append"])
def test_metric_and_argument_checks_need_no_device(call):
    L = _lib.lib()
    who = "nann_hnsw_build_device" if call is _build else "nann_hnsw_append_device"
    # the metric: a model is unsupported, anything else that is not L2 or IP is a bad argument
    assert call(L, MLP) == 102 and who in _lib.last_error() and "model" in _lib.last_error()
    for bad in (7, -1, 3):
        assert call(L, bad) == 7 and "metric" in _lib.last_error(), bad
    # the other checks are the old calls', under either metric (none of these reaches a device either)
    for metric in (L2, IP):
        assert call(L, metric, arrays=(0, 0, 0)) == 7 and who in _lib.last_error()
        assert call(L, metric, embs=0) == 7
        assert call(L, metric, arrays=(1, 0, 1)) == 7
        assert call(L, metric, d=100) == 102 and "d must be" in _lib.last_error()
        assert call(L, metric, m=40) == 102 and "M" in _lib.last_error()
        assert call(L, metric, m=1) == 102
        assert call(L, metric, dtype=_lib.F32) == 102
        assert call(L, metric, ef=41) == 102
        lv = np.ones(110, np.int32)
        lv[55] = 0
        assert call(L, metric, levels=lv) == 7 and "levels" in _lib.last_error()
        lv = np.ones(110, np.int32)
        lv[3] = 2  # an upper row and no adj_up
        assert call(L, metric, levels=lv, arrays=(1, 1, 0)) == 7
    assert _append(L, IP, n_old=0) == 7 and _append(L, IP, n_new=-1) == 7
    assert _build(L, IP, n=0) == 7


def test_host_builder_metric_codes():
    from nann_amd import index_build
    H = index_build._lib()
    x = np.zeros((4, 8), np.float32)
    lv, off = np.zeros(4, np.int32), np.zeros(5, np.int64)
    n_slots, max_levels = C.c_int64(0), C.c_int32(0)
    call = lambda metric, xp=x.ctypes.data: H.nann_hnsw_build_metric(
        C.c_void_p(xp), C.c_int64(4), C.c_int32(8), C.c_int32(4), C.c_int32(40), C.c_uint64(1), C.c_int32(1), C.c_int32(metric),
        C.c_void_p(lv.ctypes.data), C.c_void_p(off.ctypes.data), None, C.byref(n_slots), None, C.byref(max_levels))
    assert call(L2) == 0 and call(IP) == 0 and n_slots.value >= 4 * 8
    assert call(MLP) == 102 and call(7) == 7 and call(IP, xp=0) == 7
