"""CPU: the range search (nann_search_all_range and its model form) as far as it can be held without a GPU -- the four symbols,
their null-handle status, the contract in the header, the build lists, and the count -> scan -> fill scheme of
csrc/nann_range.h restated in numpy (range_model.model) against a plain np.nonzero (range_model.reference)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import range_model as RM
from nann_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nann_search_all_range_workspace_bytes", "nann_search_all_range", "nann_search_all_range_model_workspace_bytes",
           "nann_search_all_range_model")
BAD_ARGUMENT = 7


def _header():
    return open(os.path.join(ROOT, "include", "nann_hip.h")).read()


def test_the_four_symbols_are_declared_exported_and_bound():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = C.CDLL(build.build())
    for s in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % s, code), s
        assert hasattr(lib, s), s
        assert s in _lib.SYMBOLS, s
    assert "#define NANN_ABI_VERSION 6" in _header()


def test_null_handles_are_bad_arguments_without_a_gpu():
    L = _lib.lib()
    nb = C.c_int64(-1)
    assert L.nann_search_all_range_workspace_bytes(None, None, 3, C.byref(nb)) == BAD_ARGUMENT
    assert L.nann_search_all_range_model_workspace_bytes(None, None, 3, C.byref(nb)) == BAD_ARGUMENT
    assert nb.value == -1
    assert L.nann_search_all_range(None, None, None, 3, None, 0, None, None, None, None, None, 0, None, None, None) == BAD_ARGUMENT
    assert L.nann_search_all_range_model(None, None, None, 3, None, 0, None, None, None, None, None, 0, None, None, None) == BAD_ARGUMENT
    assert b"null argument" in L.nann_last_error()


def test_the_header_states_the_contract():
    text = _header()
    section = text[text.index("range search: every row scoring at or above"):text.index("int nann_search_all_range_workspace_bytes")]
    section = " ".join(section.replace("\n *", " ").split())
    for phrase in ("score(i, r) >= thresholds[i] and score(i, r) != -inf",  # the match rule
                   "a NaN score or a NaN threshold matches nothing",
                   "TRUE counts, whatever the capacity",
                   "a position at or beyond capacity is dropped, never written",  # the capacity guard
                   "left untouched",
                   "ASCENDING ROW ORDER",
                   "does not depend on the batch",  # batch independence
                   "The reference has no such call",
                   "bit-identical to what nann_search_all / nann_search_all_model return"):
        assert phrase in section, phrase


def test_the_new_files_are_in_the_build_lists():
    assert "nann_range.h" in build.DEPS
    assert os.path.exists(os.path.join(build.SRC_DIR, "nann_range.h"))
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = text[text.index("\n## 2. Build"):text.index("\n## 3. ")]
    assert "nann_range.h" in section
    assert len(build.UNITS) == 17
    # the kernels ride in an existing object: the scan's
    scan = open(os.path.join(build.SRC_DIR, "nann_scan_inst.hip")).read() + open(os.path.join(build.SRC_DIR, "nann_scan.h")).read()
    assert '#include "nann_range.h"' in scan


def test_the_model_and_the_kernels_agree_on_the_block():
    from nann_amd import retrieval
    src = open(os.path.join(build.SRC_DIR, "nann_range.h")).read()
    nt = int(re.search(r"constexpr int kRangeNT = (\d+);", src).group(1))
    passes = int(re.search(r"constexpr int kRangePasses = (\d+);", src).group(1))
    assert nt * 4 * passes == RM.BLOCK == retrieval.RANGE_BLOCK_ROWS
    assert nt == RM.SCAN_STEP


# ---- the numpy model of count -> scan -> fill against np.nonzero ---------------------------------------------------------
def _scores(b, n, seed):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((b, n)).astype(np.float32)
    flat = s.reshape(-1)
    k = max(1, flat.size // 50)
    flat[rng.integers(0, flat.size, k)] = -np.inf   # denied rows
    flat[rng.integers(0, flat.size, k)] = np.nan
    flat[rng.integers(0, flat.size, k)] = 0.0
    flat[rng.integers(0, flat.size, k)] = -0.0
    return s


def _thresholds(scores, seed):
    b = scores.shape[0]
    rng = np.random.default_rng(seed)
    thr = np.zeros(b, np.float32)
    for i in range(b):
        finite = scores[i][np.isfinite(scores[i])]
        choice = i % 7
        if choice == 0 or not len(finite):
            thr[i] = -np.inf
        elif choice == 1:
            thr[i] = np.nextafter(finite.max(), np.float32(np.inf))
        elif choice == 2:
            thr[i] = finite.max()
        elif choice == 3:
            thr[i] = np.nan
        elif choice == 4:
            thr[i] = 0.0
        elif choice == 5:
            thr[i] = np.median(finite)
        else:
            thr[i] = finite[rng.integers(0, len(finite))]
    return thr


def _same(got, exp, what):
    for g, e, name in zip(got, exp, ("row_splits", "index", "scores", "item_ids")):
        if name == "scores":
            g, e = g.view(np.uint32), e.view(np.uint32)
        assert (g == e).all(), (what, name)


B = RM.BLOCK
SIZES = [1, 63, 64, 65, B - 4, B - 3, B - 1, B, B + 1, 3 * B + 7]


@pytest.mark.parametrize("n", SIZES)
def test_model_equals_nonzero(n):
    b = 9
    scores = _scores(b, n, seed=n)
    thr = _thresholds(scores, seed=n + 1)
    ids = np.arange(n, dtype=np.int64) * 7 + 3
    total = int(RM.reference(scores, thr, ids, 0)[0][-1])
    assert total > 0
    for capacity in sorted({0, 1, max(total - 1, 0), total, total + 5, total // 2}):
        _same(RM.model(scores, thr, ids, capacity), RM.reference(scores, thr, ids, capacity), (n, capacity))


def test_row_splits_carry_over_the_chunk_border():
    """three chunks of at most 4 queries: the second and third continue the splits of the one before"""
    n, b = 301, 11
    scores = _scores(b, n, seed=5)
    thr = _thresholds(scores, seed=6)
    ids = np.arange(n, dtype=np.int64)[::-1].copy()
    ref = RM.reference(scores, thr, ids, 10 ** 4)
    assert (np.diff(ref[0]) > 0).sum() >= 6
    for chunk in (1, 4, 11, 128):
        _same(RM.model(scores, thr, ids, 10 ** 4, chunk=chunk), ref, chunk)
    cut = int(ref[0][6]) + 3  # three entries into a middle query's segment
    _same(RM.model(scores, thr, ids, cut, chunk=4), RM.reference(scores, thr, ids, cut), "cut")


def test_block_prefix_over_more_blocks_than_one_scan_step():
    """small blocks and a short scan step: the prefix loop runs several times and carries"""
    n = 1000
    scores = _scores(3, n, seed=8)
    thr = np.array([-np.inf, 0.0, 0.5], np.float32)
    ids = np.arange(n, dtype=np.int64) + 100
    ref = RM.reference(scores, thr, ids, 4000)
    for block, step in ((8, 4), (16, 256), (64, 3)):
        assert RM.n_blocks(n, block) > step or step == 256
        _same(RM.model(scores, thr, ids, 4000, block=block, scan_step=step), ref, (block, step))


def test_the_match_rule():
    s = np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf, np.nan], np.float32)
    assert RM.match(s, 0.0).tolist() == [False, False, True, True, True, True, False]
    assert RM.match(s, -0.0).tolist() == [False, False, True, True, True, True, False]
    assert RM.match(s, -np.inf).tolist() == [False, True, True, True, True, True, False]
    assert not RM.match(s, np.nan).any()
    assert RM.match(s, np.inf).tolist() == [False] * 5 + [True, False]
