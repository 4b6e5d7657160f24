"""CPU: the append and export calls of the device HNSW builder (nann_hnsw_append_device, nann_hnsw_export_count / _fill) are
exported, and their argument checks come before any device call -- as the build's do -- so they answer without a GPU."""
import ctypes as C

import numpy as np

from nann_amd import _lib

NEW = ("nann_hnsw_append_device", "nann_hnsw_export_count", "nann_hnsw_export_fill")


def test_library_exports_the_three_calls():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.nann_abi_version() == 6  # symbols were added, nothing else changed


def _append(L, embs=1, n_old=100, n_new=10, d=64, dtype=_lib.F16, m=16, ef=40, levels=None, arrays=(1, 1, 1)):
    """the call with host addresses that are never dereferenced: every case here is refused before a device call"""
    lv = np.ones(n_old + max(n_new, 0), np.int32) if levels is None else levels
    buf = np.zeros(16, np.int32)
    p = lambda on: C.c_void_p(buf.ctypes.data if on else 0)
    return L.nann_hnsw_append_device(p(embs), n_old, n_new, d, dtype, m, ef, 0, C.c_void_p(lv.ctypes.data), p(arrays[0]), p(arrays[1]),
                                     p(arrays[2]), None)


def test_append_argument_checks_need_no_device():
    L = _lib.lib()
    assert _append(L, arrays=(0, 0, 0)) == 7 and "nann_hnsw_append_device" in _lib.last_error()
    assert _append(L, embs=0) == 7
    assert _append(L, arrays=(1, 0, 1)) == 7
    assert _append(L, n_old=0) == 7
    assert _append(L, n_new=-1) == 7
    assert _append(L, d=100) == 102 and "d must be" in _lib.last_error()
    assert _append(L, m=40) == 102 and "M" in _lib.last_error()
    assert _append(L, m=1) == 102
    assert _append(L, dtype=_lib.F32) == 102
    assert _append(L, ef=41) == 102
    assert _append(L, n_old=2 ** 31 - 1, n_new=1, levels=np.ones(4, np.int32)) == 102  # refused before levels is read
    lv = np.ones(110, np.int32)
    lv[105] = 0
    assert _append(L, levels=lv) == 7 and "levels" in _lib.last_error()
    lv = np.ones(110, np.int32)
    lv[3] = 2  # an upper row and no adj_up
    assert _append(L, levels=lv, arrays=(1, 1, 0)) == 7


def test_export_argument_checks_need_no_device():
    L = _lib.lib()
    lv = np.ones(8, np.int32)
    buf = np.zeros(16, np.int64)
    p, z = C.c_void_p(buf.ctypes.data), C.c_void_p(0)
    nnz, n_enter = (C.c_int64 * 2)(), C.c_int64(0)
    lvp = C.c_void_p(lv.ctypes.data)
    count = lambda adj0=p, n=8, m=16, start=2, rs=p: L.nann_hnsw_export_count(adj0, p, p, lvp, n, m, start, rs, rs, nnz, C.byref(n_enter), None)
    fill = lambda adj0=p, n=8, m=16, start=2, rs=p, nz=nnz, v=p: L.nann_hnsw_export_fill(adj0, p, p, lvp, n, m, start, rs, rs, nz, v, v, p, None)
    for call in (count, fill):
        assert call(start=1) == 102 and "start_level" in _lib.last_error()
        assert call(start=3) == 102
        assert call(adj0=z) == 7
        assert call(n=0) == 7
        assert call(m=40) == 102
        assert call(rs=z) == 7
    assert fill(nz=None) == 7
    nnz[0] = 3  # values to write and nowhere to write them
    assert fill(v=z) == 7 and "values" in _lib.last_error()
    nnz[0] = -1
    assert fill() == 7
