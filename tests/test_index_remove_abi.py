"""CPU: the removal calls of the device HNSW builder (nann_hnsw_remove_count, nann_hnsw_remove_device) are exported, and their
argument checks come before any device call -- as the append's do -- so they answer without a GPU."""
import ctypes as C

import numpy as np

from nann_amd import _lib

NEW = ("nann_hnsw_remove_count", "nann_hnsw_remove_device")


def test_library_exports_the_two_calls():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.nann_abi_version() == 6  # symbols were added, nothing else changed


_BUF = np.zeros(16, np.int64)


def _p(on):
    """a host address that is never dereferenced (every case here is refused before a device call), or null"""
    return C.c_void_p(_BUF.ctypes.data if on else 0)


def _remove(L, embs=1, n=100, d=64, dtype=_lib.F16, m=16, keep_pruned=0, metric=_lib.SCORER_L2, levels=None, graph=(1, 1, 1), bits=1,
            n_keep=90, outs=(1, 1, 1), stats=True):
    lv = np.ones(max(n, 1), np.int32) if levels is None else levels
    st = (C.c_int64 * 4)() if stats else None
    return L.nann_hnsw_remove_device(_p(embs), n, d, dtype, m, keep_pruned, metric, C.c_void_p(lv.ctypes.data), _p(graph[0]), _p(graph[1]),
                                     _p(graph[2]), _p(bits), n_keep, _p(outs[0]), _p(outs[1]), _p(outs[2]), st, None)


def test_remove_argument_checks_need_no_device():
    L = _lib.lib()
    assert _remove(L, embs=0) == 7 and "nann_hnsw_remove_device" in _lib.last_error()
    assert _remove(L, graph=(0, 1, 1)) == 7
    assert _remove(L, graph=(1, 0, 1)) == 7
    assert _remove(L, bits=0) == 7
    for outs in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert _remove(L, outs=outs) == 7
    assert _remove(L, n=0) == 7
    assert _remove(L, n=-5) == 7
    # every survivor removed: a graph keeps at least one node
    assert _remove(L, n_keep=0) == 7 and "n_keep" in _lib.last_error()
    assert _remove(L, n_keep=-1) == 7
    assert _remove(L, n_keep=101) == 7
    # d, dtype and M: the build's limits
    assert _remove(L, d=100) == 102 and "d must be" in _lib.last_error()
    assert _remove(L, dtype=_lib.F32) == 102
    assert _remove(L, m=40) == 102 and "M" in _lib.last_error()
    assert _remove(L, m=1) == 102
    # the metric: a model does not link rows, anything else is no scorer kind
    assert _remove(L, metric=_lib.SCORER_MLP) == 102 and "model" in _lib.last_error()
    assert _remove(L, metric=7) == 7 and "metric" in _lib.last_error()
    assert _remove(L, metric=-1) == 7
    # more than 2^31 - 1 nodes: refused before levels is read
    assert _remove(L, n=2 ** 31, n_keep=5, levels=np.ones(4, np.int32)) == 102 and "2^31" in _lib.last_error()
    lv = np.ones(100, np.int32)
    lv[57] = 0
    assert _remove(L, levels=lv) == 7 and "levels" in _lib.last_error()
    lv = np.ones(100, np.int32)
    lv[3] = 2  # an upper row and no adj_up
    assert _remove(L, levels=lv, graph=(1, 1, 0)) == 7 and "adj_up" in _lib.last_error()


def _count(L, bits=1, levels=1, n=100, kept=1, new_levels=1, n_keep=True, n_up=True, lv=None):
    lv = np.ones(max(min(n, 1000), 1), np.int32) if lv is None else lv
    new = np.zeros(len(lv), np.int32)
    a, b = C.c_int64(0), C.c_int64(0)
    return L.nann_hnsw_remove_count(_p(bits), C.c_void_p(lv.ctypes.data if levels else 0), n, _p(kept),
                                    C.c_void_p(new.ctypes.data if new_levels else 0), C.byref(a) if n_keep else None,
                                    C.byref(b) if n_up else None, None)


def test_remove_count_argument_checks_need_no_device():
    L = _lib.lib()
    assert _count(L, bits=0) == 7 and "nann_hnsw_remove_count" in _lib.last_error()
    assert _count(L, levels=0) == 7
    assert _count(L, kept=0) == 7
    assert _count(L, new_levels=0) == 7
    assert _count(L, n_keep=False) == 7
    assert _count(L, n_up=False) == 7
    assert _count(L, n=0) == 7
    assert _count(L, n=2 ** 31) == 102  # refused before levels is read
    lv = np.ones(100, np.int32)
    lv[99] = -2
    assert _count(L, lv=lv) == 7 and "levels" in _lib.last_error()
