"""CPU: IVF-SQ8 (nann_search_lists_sq8) as far as it can be held without a GPU -- the two symbols, the refusals that stand in front
of any device call, and the scratch rule of the int8 list scan."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from nann_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nann_search_lists_sq8_workspace_bytes", "nann_search_lists_sq8")
BAD_ARGUMENT, UNSUPPORTED = 7, 102


def test_the_symbols_are_declared_exported_and_bound():
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nann_hip.h")).read(), flags=re.S)
    lib, bound = C.CDLL(build.build()), _lib.lib()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % s, code), s
        assert hasattr(lib, s) and s in _lib.SYMBOLS and getattr(bound, s).argtypes, s
    assert bound.nann_abi_version() == 6


def _size(L, handles, n, n_probe, fetch, k):
    return L.nann_search_lists_sq8_workspace_bytes(*handles, n, n_probe, fetch, k, C.byref(C.c_int64(0)))


def _search(L, handles, n, n_probe, fetch, k):
    p = handles[0]
    return L.nann_search_lists_sq8(*handles, p, n, p, n_probe, fetch, k, p, p, p, p, p, p, None, None, p, 1 << 20, None)


@pytest.mark.parametrize("call", [_size, _search])
def test_refusals_without_a_device(call):
    """zeroed memory stands in for the handles: an index and an L2 scorer of d = 0 that agree, a partition and a table of uid 0"""
    L = _lib.lib()
    zeros = np.zeros(1 << 12, np.int64)
    p = C.c_void_p(zeros.ctypes.data)
    for i in range(4):  # a null handle, each of the four
        assert call(L, [None if j == i else p for j in range(4)], 1, 1, 8, 4) == BAD_ARGUMENT and "null argument" in _lib.last_error()
    for fetch, k in ((8, 9), (8, -1), (0, 1)):
        assert call(L, [p] * 4, 1, 1, fetch, k) == BAD_ARGUMENT and "k must lie in [0, fetch]" in _lib.last_error()
    assert call(L, [p] * 4, 1, 1, 1025, 4) == UNSUPPORTED and "k <= 1024" in _lib.last_error()
    for n, n_probe, fetch in ((-1, 1, 8), (1, 1, -8)):
        assert call(L, [p] * 4, n, n_probe, fetch, 4 if fetch > 0 else 0) == BAD_ARGUMENT
    assert _lib.last_error().startswith("Need k >= 0")
    assert L.nann_search_lists_sq8_workspace_bytes(p, p, p, p, 1, 1, 8, 4, None) == BAD_ARGUMENT


REPORT = """remark: unit.hip:1:1: Function Name: _ZN4nann16k_lists_scan_sq8ILi2ELi0EEEvPKaPKfPKixS6_PKNS_9ListsHeadEPKxPKNS_9ListsTileES2_S4_S6_Pfx [-Rpass-analysis=kernel-resource-usage]
remark: unit.hip:1:1:     VGPRs: 70 [-Rpass-analysis=kernel-resource-usage]
remark: unit.hip:1:1:     ScratchSize [bytes/lane]: %d [-Rpass-analysis=kernel-resource-usage]
remark: unit.hip:1:1:     Occupancy [waves/SIMD]: 5 [-Rpass-analysis=kernel-resource-usage]
"""


def test_the_build_refuses_an_int8_list_scan_with_a_scratch_frame(tmp_path):
    good, bad = tmp_path / "good.log", tmp_path / "bad.log"
    good.write_text(REPORT % 0)
    bad.write_text(REPORT % 16)
    build.check_resources(str(good))
    with pytest.raises(RuntimeError, match="k_lists_scan_sq8.*16 bytes of scratch.*int8 list scan"):
        build.check_resources(str(bad))
