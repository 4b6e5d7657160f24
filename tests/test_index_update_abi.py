"""CPU: the in-place update of the device HNSW builder (nann_hnsw_update_device) and the call that says which rows to heal
(nann_hnsw_orphan_bits) are exported, and their argument checks come before any device call -- as the append's and the
removal's do -- so they answer without a GPU."""
import ctypes as C

import numpy as np

from nann_amd import _lib

NEW = ("nann_hnsw_update_device", "nann_hnsw_orphan_bits")


def test_library_exports_the_two_calls():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.nann_abi_version() == 6  # symbols were added, nothing else changed


_BUF = np.zeros(16, np.int64)


def _p(on):
    """a host address that is never dereferenced (every case here is refused before a device call), or null"""
    return C.c_void_p(_BUF.ctypes.data if on else 0)


def _update(L, embs=1, n=100, d=64, dtype=_lib.F16, m=16, ef=40, keep_pruned=0, metric=_lib.SCORER_L2, levels=None, graph=(1, 1, 1),
            bits=1, outs=(1, 1, 1), stats=True):
    lv = np.ones(max(n, 1), np.int32) if levels is None else levels
    st = (C.c_int64 * 4)() if stats else None
    return L.nann_hnsw_update_device(_p(embs), n, d, dtype, m, ef, keep_pruned, metric, C.c_void_p(lv.ctypes.data), _p(graph[0]),
                                     _p(graph[1]), _p(graph[2]), _p(bits), _p(outs[0]), _p(outs[1]), _p(outs[2]), st, None)


def test_update_argument_checks_need_no_device():
    L = _lib.lib()
    assert _update(L, embs=0) == 7 and "nann_hnsw_update_device" in _lib.last_error()
    assert _update(L, graph=(0, 1, 1)) == 7
    assert _update(L, graph=(1, 0, 1)) == 7
    assert _update(L, bits=0) == 7
    for outs in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert _update(L, outs=outs) == 7 and "nann_hnsw_update_device" in _lib.last_error()
    assert _update(L, n=0) == 7
    assert _update(L, n=-5) == 7
    lv = np.ones(100, np.int32)
    assert L.nann_hnsw_update_device(_p(1), 100, 64, _lib.F16, 16, 40, 0, _lib.SCORER_L2, None, _p(1), _p(1), _p(1), _p(1), _p(1), _p(1),
                                     _p(1), None, None) == 7  # levels
    # d, dtype, M and ef_construction: the build's limits
    assert _update(L, d=100) == 102 and "d must be" in _lib.last_error() and "nann_hnsw_update_device" in _lib.last_error()
    assert _update(L, dtype=_lib.F32) == 102
    assert _update(L, m=40) == 102 and "M" in _lib.last_error()
    assert _update(L, m=1) == 102
    assert _update(L, ef=41) == 102 and "ef_construction" in _lib.last_error()
    # the metric: a model does not link rows, anything else is no scorer kind
    assert _update(L, metric=_lib.SCORER_MLP) == 102 and "model" in _lib.last_error()
    assert _update(L, metric=7) == 7 and "metric" in _lib.last_error()
    assert _update(L, metric=-1) == 7
    # more than 2^31 - 1 nodes: refused before levels is read
    assert _update(L, n=2 ** 31, levels=np.ones(4, np.int32)) == 102 and "2^31" in _lib.last_error()
    lv[57] = 0
    assert _update(L, levels=lv) == 7 and "levels" in _lib.last_error() and "nann_hnsw_update_device" in _lib.last_error()
    lv = np.ones(100, np.int32)
    lv[3] = 2  # an upper row and no adj_up
    assert _update(L, levels=lv, graph=(1, 1, 0)) == 7 and "adj_up" in _lib.last_error()


def _orphans(L, adj0=1, n=100, m=16, bits=1, count=True):
    c = C.c_int64(-7)
    return L.nann_hnsw_orphan_bits(_p(adj0), n, m, _p(bits), C.byref(c) if count else None, None), c.value


def test_orphan_bits_argument_checks_need_no_device():
    L = _lib.lib()
    assert _orphans(L, adj0=0) == (7, -7) and "nann_hnsw_orphan_bits" in _lib.last_error()
    assert _orphans(L, bits=0)[0] == 7
    assert _orphans(L, count=False)[0] == 7
    assert _orphans(L, n=0)[0] == 7
    assert _orphans(L, n=2 ** 31)[0] == 102 and "2^31" in _lib.last_error()
    assert _orphans(L, m=1)[0] == 102 and "M" in _lib.last_error()
    assert _orphans(L, m=33)[0] == 102 and "nann_hnsw_orphan_bits" in _lib.last_error()
