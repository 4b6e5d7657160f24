"""CPU: the numpy model of the shared-list search on a hand-written case; the new calls are exported and refuse null handles
before any device call."""
import ctypes as C

import numpy as np

from lists_model import expansion, partition_csr
from nann_amd import _lib

NEW = ("nann_partition_create", "nann_partition_destroy", "nann_partition_info", "nann_partition_view",
       "nann_search_lists_workspace_bytes", "nann_search_lists")


def test_model_on_a_hand_written_case():
    splits, rows = partition_csr([2, -1, 0, 2, 0, -5, 2, 3], 5)  # lists 1 and 4 are empty
    assert splits.tolist() == [0, 2, 2, 5, 6, 6] and rows.tolist() == [2, 4, 0, 3, 6, 7]
    assert expansion(splits, rows, [2, -1, 0, 2]).tolist() == [0, 3, 6, 2, 4, 0, 3, 6]  # slot order, a list named twice
    assert expansion(splits, rows, [-1, 1, 4]).tolist() == []
    assert expansion(splits, rows, [0, 5]) is None


def test_library_exports_the_calls():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.nann_abi_version() == 6  # symbols were added, nothing else changed


def test_null_handles_are_refused_without_a_device():
    L = _lib.lib()
    buf = np.zeros(16, np.int64)
    p, out, nbytes = C.c_void_p(buf.ctypes.data), C.c_void_p(0), C.c_int64(0)
    assert L.nann_partition_create(None, p, 4, None, C.byref(out)) == 7 and "nann_partition_create" in _lib.last_error()
    assert L.nann_partition_info(None, (C.c_int64 * 4)()) == 7
    assert L.nann_partition_view(None, None, None) == 7
    L.nann_partition_destroy(None)
    assert L.nann_search_lists_workspace_bytes(p, None, p, 1, 1, 1, C.byref(nbytes)) == 7  # (no partition: nothing is dereferenced)
    assert L.nann_search_lists_workspace_bytes(p, p, p, 1, 1, 1, None) == 7
    assert L.nann_search_lists(p, None, p, p, 1, p, 1, 1, p, p, p, p, p, p, p, 1 << 20, None) == 7
    assert "nann_search_lists" in _lib.last_error()
