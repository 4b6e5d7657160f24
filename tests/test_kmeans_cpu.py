"""CPU: the coarse quantiser (nann_kmeans_assign, nann_kmeans_train) as far as it can be held without a GPU -- the four symbols,
and the refusals that stand in front of any device call."""
import ctypes as C
import os
import re

import numpy as np

from nann_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nann_kmeans_assign_workspace_bytes", "nann_kmeans_assign", "nann_kmeans_train_workspace_bytes", "nann_kmeans_train")
BAD_ARGUMENT = 7


def test_the_symbols_are_declared_exported_and_bound():
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nann_hip.h")).read(), flags=re.S)
    lib, bound = C.CDLL(build.build()), _lib.lib()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % s, code), s
        assert hasattr(lib, s) and s in _lib.SYMBOLS and getattr(bound, s).argtypes, s
    assert bound.nann_abi_version() == 6


def test_refusals_without_a_device():
    """zeroed memory stands in for the index and the arrays: the null pointers, n_lists < 1 and n_iter < 0 are named first"""
    L = _lib.lib()
    zeros = np.zeros(1 << 12, np.int64)
    p, size = C.c_void_p(zeros.ctypes.data), C.byref(C.c_int64(0))
    calls = {
        "assign_size": lambda ix, n_lists, out: L.nann_kmeans_assign_workspace_bytes(ix, n_lists, 1, out),
        "assign": lambda ix, n_lists, out: L.nann_kmeans_assign(ix, p, n_lists, 0, 1, out and p, None, p, 1 << 20, None),
        "train_size": lambda ix, n_lists, out: L.nann_kmeans_train_workspace_bytes(ix, n_lists, out),
        "train": lambda ix, n_lists, out: L.nann_kmeans_train(ix, p, n_lists, 1, out and p, p, None, p, 1 << 20, None),
    }
    for name, call in calls.items():
        for ix, out in ((None, size), (p, None)):
            assert call(ix, 4, out) == BAD_ARGUMENT and "null argument" in _lib.last_error(), name
        for n_lists in (0, -3):
            assert call(p, n_lists, size) == BAD_ARGUMENT and "n_lists < 1" in _lib.last_error(), name
    assert L.nann_kmeans_assign(p, None, 4, 0, 1, p, None, p, 1 << 20, None) == BAD_ARGUMENT
    assert L.nann_kmeans_train(p, p, 4, 1, p, None, None, p, 1 << 20, None) == BAD_ARGUMENT and "null argument" in _lib.last_error()
    assert L.nann_kmeans_train(p, p, 4, -1, p, p, None, p, 1 << 20, None) == BAD_ARGUMENT and "n_iter < 0" in _lib.last_error()
