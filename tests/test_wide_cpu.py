"""CPU: the wide selection as far as it can be held without a GPU -- the numpy model of the design (wide_model: digit passes on
score_key, cut, quota, gather in row order, composite sort) against oracle.topk and np.lexsort on the corpora where a selection
can go wrong, each wrong variant shown to move a result, the six symbols, the scratch rule of the streaming kernels, and every
refusal that stands in front of a launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import wide_model as M
from nann_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nann_search_all_wide_workspace_bytes", "nann_search_all_wide", "nann_search_all_model_wide_workspace_bytes",
           "nann_search_all_model_wide", "nann_select_wide_workspace_bytes", "nann_select_wide")
OK, TOPK_K_GT_N, BAD_ARGUMENT, UNSUPPORTED, CAPACITY = 0, 4, 7, 102, 103
F = np.float32


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def _same(a, b):
    return (bits(a[0]) == bits(b[0])).all() and (a[1] == b[1]).all() and a[2] == b[2]


# ---- the corpora ----------------------------------------------------------------------------------------------------------
def _corpora():
    rng = np.random.default_rng(11)
    n = 5000
    out = {}
    out["random"] = (rng.standard_normal(n).astype(F), (1, 7, 1024, 1025, 4097, n))
    ties = rng.integers(0, 9, n).astype(F) * F(0.5) - F(2.0)            # nine values, about 555 rows each
    out["ties"] = (ties, (1, 300, 556, 1025, 2000, 4097, n))
    out["equal"] = (np.full(n, F(-3.25)), (1, 2, 1025, n))
    zeros = np.where(rng.integers(0, 2, n) == 1, F(0.0), F(-0.0)).astype(F)
    out["zeros"] = (zeros, (1, 100, 2500, n))
    mixed = zeros.copy()
    mixed[::3] = rng.standard_normal(len(mixed[::3])).astype(F)
    out["zeros_mixed"] = (mixed, (1, 1000, 2500, 4000, n))
    den = (rng.integers(-400, 400, n).astype(np.int64) * 3).astype(np.float64) * 2.0 ** -149
    out["denormals"] = (den.astype(F), (1, 17, 1025, 4999, n))
    few = np.full(n, -np.inf, F)
    at = rng.permutation(n)[:700]
    few[at] = rng.integers(0, 5, 700).astype(F)
    out["few_valid"] = (few, (1, 699, 700, 701, 2048, n))
    out["all_denied"] = (np.full(n, -np.inf, F), (1, 100))
    out["one"] = (np.array([1.5], F), (0, 1))
    wide = rng.standard_normal(40003).astype(F)
    wide[rng.integers(0, 40003, 6000)] = F(0.125)
    out["long"] = (wide, (16384,))
    return out


CORPORA = _corpora()


@pytest.mark.parametrize("name", sorted(CORPORA))
def test_the_model_is_the_contract(name):
    scores, ks = CORPORA[name]
    for k in ks:
        assert _same(M.select(scores, k), M.reference(scores, k)), (name, k)


def test_the_model_is_topkv2_where_no_row_is_denied(oracle):
    for name in ("random", "ties", "equal", "zeros", "zeros_mixed", "denormals"):
        scores, ks = CORPORA[name]
        for k in ks:
            rc, ev, ei = oracle.topk(scores, k)
            assert rc == 0
            v, i, n_out = M.select(scores, k)
            assert n_out == k and (i == ei).all() and (bits(v) == bits(ev)).all(), (name, k)


def test_score_key_orders_floats_and_ties_the_zeros():
    v = np.array([-np.inf, -3.0e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3.0e38, np.inf], F)
    k = M.score_key(v).astype(np.int64)
    assert k[4] == k[5] and (np.diff(np.delete(k, 4)) > 0).all()
    assert M.score_key(F(-np.inf)) == 0x007FFFFF
    assert sum(b for _, b in M.PASSES) == 32 and M.PASSES[0][0] + M.PASSES[0][1] == 32
    assert all(hi[0] == lo[0] + lo[1] for hi, lo in zip(M.PASSES, M.PASSES[1:]))


def test_the_cut_is_the_kth_key():
    for scores in (CORPORA["random"][0], CORPORA["ties"][0], CORPORA["denormals"][0]):
        keys = M.score_key(scores)
        for k in (1, 2, 777, 1025, 4999):
            T, n_gt, m = M.cut(keys, k)
            assert T == np.sort(keys)[::-1][k - 1]
            assert n_gt == (keys > T).sum() and n_gt < k and m == k - n_gt and m <= (keys == T).sum()


# ---- each wrong variant moves a result ------------------------------------------------------------------------------------
def test_without_the_quota_the_result_moves():
    scores, _ = CORPORA["ties"]
    k = 1025                                              # cuts inside a tie class
    good, bad = M.select(scores, k), M.select(scores, k, "no_quota")
    assert _same(good, M.reference(scores, k)) and not _same(bad, good)


def test_ties_in_descending_row_order_move_the_result():
    scores, _ = CORPORA["ties"]
    good, bad = M.select(scores, 300), M.select(scores, 300, "ties_desc")
    assert (bits(good[0]) == bits(bad[0])).all() and not (good[1] == bad[1]).all()


def test_negative_zero_below_positive_zero_moves_the_result():
    scores, _ = CORPORA["zeros"]
    good, bad = M.select(scores, 100), M.select(scores, 100, "neg_zero_below")
    assert (good[1] == np.arange(100)).all()              # all tie: row order
    assert not (good[1] == bad[1]).all() and (bad[0] == 0).all() and not np.signbit(bad[0]).any()


# ---- the ABI and the build ------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "nann_hip.h")).read()


def test_the_six_symbols_are_declared_exported_and_bound():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = C.CDLL(build.build())
    bound = _lib.lib()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % s, code), s
        assert hasattr(lib, s), s
        assert s in _lib.SYMBOLS, s
        assert getattr(bound, s).argtypes, s
    assert "#define NANN_WIDE_MAX_K 16384" in _header() and _lib.WIDE_MAX_K == 16384 == M.MAX_K
    assert "#define NANN_ABI_VERSION 6" in _header() and bound.nann_abi_version() == 6


def test_the_kernels_ride_in_the_scan_object():
    assert len(build.UNITS) == 17
    assert "nann_wide.h" in build.DEPS
    assert not any("wide" in src for _, parts in build.UNITS for src, _ in parts)   # instantiated behind nann_scan_inst.hip
    scan = open(os.path.join(build.SRC_DIR, "nann_scan.h")).read()
    assert '#include "nann_wide.h"' in scan and "const ScanWide* wide;" in scan


REPORT = """remark: unit.hip:1:1: Function Name: _ZN4nann11k_wide_histILi1EEEvPKfmxxPKiPj [-Rpass-analysis=kernel-resource-usage]
remark: unit.hip:1:1:     VGPRs: 20 [-Rpass-analysis=kernel-resource-usage]
remark: unit.hip:1:1:     ScratchSize [bytes/lane]: %d [-Rpass-analysis=kernel-resource-usage]
remark: unit.hip:1:1:     Occupancy [waves/SIMD]: 8 [-Rpass-analysis=kernel-resource-usage]
remark: unit.hip:1:1: Function Name: _ZN4nann11k_wide_fillEPKfmxxPKiS3_iPy [-Rpass-analysis=kernel-resource-usage]
remark: unit.hip:1:1:     ScratchSize [bytes/lane]: %d [-Rpass-analysis=kernel-resource-usage]
remark: unit.hip:1:1: Function Name: _ZN4nann11k_wide_sortEPKyPKiiiPKfxxPKlPlPfPiSA_ [-Rpass-analysis=kernel-resource-usage]
remark: unit.hip:1:1:     ScratchSize [bytes/lane]: 16 [-Rpass-analysis=kernel-resource-usage]
"""


def test_the_build_refuses_a_streaming_kernel_with_a_scratch_frame(tmp_path):
    good, bad_hist, bad_fill = tmp_path / "good.log", tmp_path / "hist.log", tmp_path / "fill.log"
    good.write_text(REPORT % (0, 0))
    bad_hist.write_text(REPORT % (12, 0))
    bad_fill.write_text(REPORT % (0, 12))
    build._check_wide_scratch(str(good))                 # (the sort kernel's frame is no business of the rule)
    build.check_resources(str(good))
    with pytest.raises(RuntimeError, match="k_wide_hist.*12 bytes of scratch.*wide selection"):
        build._check_wide_scratch(str(bad_hist))
    with pytest.raises(RuntimeError, match="k_wide_fill.*12 bytes of scratch"):
        build._check_wide_scratch(str(bad_fill))
    with pytest.raises(RuntimeError, match="k_wide_fill"):
        build.check_resources(str(bad_fill))             # (what the build runs over every unit's report)


# ---- the refusals in front of any launch ----------------------------------------------------------------------------------
def test_refusals_without_a_device():
    L = _lib.lib()
    nb = C.c_int64(-1)
    # the search calls: nothing to look at without an index
    assert L.nann_search_all_wide_workspace_bytes(None, None, 4, 8, C.byref(nb)) == BAD_ARGUMENT and b"null" in L.nann_last_error()
    assert L.nann_search_all_model_wide_workspace_bytes(None, None, 4, 8, C.byref(nb)) == BAD_ARGUMENT
    assert L.nann_search_all_wide(None, None, None, 4, 8, None, None, None, None, None, 0, None, None, None, None) == BAD_ARGUMENT
    assert L.nann_search_all_model_wide(None, None, None, 4, 8, None, None, None, None, None, 0, None, None, None, None) == BAD_ARGUMENT
    assert nb.value == -1
    # the selection alone checks its shape without a handle.  The pointers below are never followed: every call ends at a check.
    vals, out, ws = C.c_void_p(0x10000), C.c_void_p(0x20000), C.c_void_p(0x40000)
    size = lambda n_rows, n_cols, k: L.nann_select_wide_workspace_bytes(n_rows, n_cols, k, C.byref(nb))
    call = lambda n_rows, n_cols, k, v=vals, o=out, w=ws, wb=1 << 40: L.nann_select_wide(v, n_rows, n_cols, k, None, o, None, w, wb, None)
    assert size(3, 40003, 4097) == OK and nb.value > 0 and nb.value % 256 == 0
    need = nb.value
    assert L.nann_select_wide_workspace_bytes(3, 40003, 4097, None) == BAD_ARGUMENT
    for f in (size, call):
        assert f(3, 40003, -1) == BAD_ARGUMENT and b"Need k >= 0, got -1" in L.nann_last_error()
        assert f(3, 40003, 16385) == UNSUPPORTED and b"k <= 16384" in L.nann_last_error()
        assert f(3, 100, 101) == TOPK_K_GT_N and b"at least k columns. Had 100, needed 101" in L.nann_last_error()
        assert f(3, 16384, 16385) == TOPK_K_GT_N                         # (k against the row first, as TopKV2)
        assert f(-1, 100, 5) == BAD_ARGUMENT and f(3, -1, 0) == BAD_ARGUMENT
        assert f(3, 1 << 31, 5) == UNSUPPORTED and b"32-bit" in L.nann_last_error()
        assert f(0, 100, 5) == OK and f(3, 100, 0) == OK and f(0, 0, 0) == OK
    assert size(0, 100, 5) == OK and nb.value == 0
    assert size(3, 100, 0) == OK and nb.value == 0
    assert size(1 << 40, (1 << 31) - 1, 16384) == OK and nb.value > 0   # any n_rows, any n_cols: bounded by a chunk of rows
    assert nb.value < 1 << 30
    assert call(3, 40003, 4097, v=None) == BAD_ARGUMENT and b"null" in L.nann_last_error()
    assert call(3, 40003, 4097, o=None) == BAD_ARGUMENT and b"null" in L.nann_last_error()
    assert call(3, 40003, 4097, v=C.c_void_p(0x10004)) == BAD_ARGUMENT and b"16-byte" in L.nann_last_error()
    assert call(3, 40003, 4097, w=None) == CAPACITY
    assert call(3, 40003, 4097, wb=need - 1) == CAPACITY and b"nann_select_wide_workspace_bytes" in L.nann_last_error()
    assert call(3, 40003, 4097, w=C.c_void_p(0x40010), wb=need) == BAD_ARGUMENT and b"256-byte aligned" in L.nann_last_error()
