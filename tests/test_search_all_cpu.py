"""Exhaustive search (nann_search_all), the parts that need no GPU: the ABI, the argument checks that run in front of any
device call, and a numpy model of the selection design -- top-k per slab of rows, then TopKV2 over the slabs' lists laid end
to end in slab order (csrc/nann_scan.h) -- against the oracle on inputs built to break ties the wrong way."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLAB_ROWS = 16384  # kScanSlabRows
MAX_K = 1024       # kMaxK


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_library_exports_search_all_and_header_documents_it():
    from nann_amd import _lib
    L = _lib.lib()  # builds for gfx950 when the sources changed
    assert L.nann_abi_version() == 6
    header = open(os.path.join(ROOT, "include", "nann_hip.h")).read()
    for name in ("nann_search_all_workspace_bytes", "nann_search_all"):
        assert name in _lib.SYMBOLS and getattr(L, name) is not None
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert "main.py:194-237" in header and "util.py:9-11" in header
    assert "#define NANN_ABI_VERSION 6" in header


def test_null_handles_are_bad_arguments_without_a_device():
    from nann_amd import _lib
    L = _lib.lib()
    nbytes = C.c_int64(-1)
    assert L.nann_search_all_workspace_bytes(None, None, 4, 10, C.byref(nbytes)) == 7
    assert b"null argument" in L.nann_last_error()
    assert L.nann_search_all(None, None, None, 4, 10, None, None, None, None, 0, None, None) == 7
    assert b"nann_search_all" in L.nann_last_error()


def test_build_refuses_a_scan_kernel_with_scratch(tmp_path):
    """k_scan_l2 stages the table through registers into LDS; a scratch frame there triples its memory traffic without changing a
    bit of its answers, so the build checks the compiler's resource report (build._check_scan_scratch) -- on a report that has one,
    on one that has none, and on the report of the library that was just built."""
    from nann_amd import _lib, build
    head = "remark: x:1:0: Function Name: _ZN4nann9k_scan_l2ILi16ELi0ELi16EEEvPKvxPKfiiPf\n"
    other = "remark: x:1:0: Function Name: _ZN4nann8k_searchILi16ELi0ELi1ELi0ELi1024EEEvNS_10SearchArgsE\nremark: x:1:0:     ScratchSize [bytes/lane]: 64\n"
    bad, good = tmp_path / "bad.log", tmp_path / "good.log"
    bad.write_text(other + head + "remark: x:1:0:     ScratchSize [bytes/lane]: 144\n")
    good.write_text(head + "remark: x:1:0:     ScratchSize [bytes/lane]: 0\n" + other)
    with pytest.raises(RuntimeError, match="scratch"):
        build._check_scan_scratch(str(bad))
    build._check_scan_scratch(str(good))
    _lib.lib()
    log = os.path.join(build.OUT_DIR, "nann_scan.d", "compile.log")
    if os.path.exists(log):  # (a library named by NANN_HIP_LIB or shipped prebuilt has no report beside it)
        text = open(log).read()
        sizes = re.findall(r"Function Name: (\S*k_scan_l2\S*)(?:.*\n)*?.*ScratchSize \[bytes/lane\]: (\d+)", text)
        assert len(sizes) == 12 and all(int(b) == 0 for _, b in sizes), sizes
        build._check_scan_scratch(log)


# ---- the selection design as a numpy model ----------------------------------------------------------------------------
def score_key(v):
    """csrc/nann_device.h score_key: monotone u32 image of a score, -0 folded into +0"""
    u = (np.asarray(v, np.float32) + np.float32(0.0)).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def topk_by_position(scores, k):
    """wg_topk: descending, ties -> lower POSITION"""
    order = np.argsort(~score_key(scores), kind="stable")[:k]
    return order.astype(np.int64)


def slab_bounds(n, slab_rows=SLAB_ROWS):
    n_slabs = (n + slab_rows - 1) // slab_rows
    return [n * s // n_slabs for s in range(n_slabs + 1)]


def select_model(scores, k, slab_rows=SLAB_ROWS, list_order=None):
    """k_scan_slab_topk + k_scan_merge: per slab the top k as (score, row), then top k of the lists in slab order.
    list_order: another order of the slabs' lists (the trap: position is then no longer row order)."""
    b = slab_bounds(len(scores), slab_rows)
    lists = []
    for s in range(len(b) - 1):
        pos = topk_by_position(scores[b[s]:b[s + 1]], k)
        assert len(pos) == k, "a slab's list is always k long"
        lists.append((scores[b[s]:b[s + 1]][pos], pos + b[s]))
    if list_order is not None:
        lists = [lists[i] for i in list_order]
    cs = np.concatenate([l[0] for l in lists])
    cr = np.concatenate([l[1] for l in lists])
    pos = topk_by_position(cs, k)
    return cr[pos].astype(np.int32), cs[pos]


def _expect(oracle, scores, k):
    rc, ov, oi = oracle.topk(scores, k)
    assert rc == 0
    return oi, ov


def _same(got, exp):
    return (got[0] == exp[0]).all() and (got[1].view(np.uint32) == exp[1].view(np.uint32)).all()


def test_slabs_always_hold_k_rows():
    """two or more slabs -> each at least SLAB_ROWS / 2 >= MAX_K rows and at most SLAB_ROWS; one slab -> all n >= k rows"""
    rng = np.random.default_rng(5)
    sizes = [1, 63, 1000, SLAB_ROWS - 1, SLAB_ROWS, SLAB_ROWS + 1, 20011, 2 * SLAB_ROWS + 1, 200_000, 1_000_000,
             (1 << 31) - 1] + rng.integers(1, 1 << 31, 200).tolist()
    for n in sizes:
        b = slab_bounds(int(n))
        lens = np.diff(np.asarray(b, dtype=np.int64))
        assert b[0] == 0 and b[-1] == n and lens.max() <= SLAB_ROWS
        if len(lens) > 1:
            assert lens.min() >= SLAB_ROWS // 2 >= MAX_K


@pytest.mark.parametrize("slab_rows", [64, 100, SLAB_ROWS])
def test_selection_model_equals_oracle_on_tie_corpora(oracle, slab_rows):
    rng = np.random.default_rng(11)
    n = 20011 if slab_rows == SLAB_ROWS else 1000
    kmax = min(MAX_K, slab_rows // 2)
    ks = sorted({1, 2, 4, 7, kmax - 1, kmax})
    base = rng.standard_normal((n + 2) // 3).astype(np.float32)
    cases = {
        "every score three times, scattered": rng.permutation(np.tile(base, 3))[:n],
        "all equal": np.full(n, np.float32(-1.5)),
        "signed zeros tie": np.where(rng.integers(0, 2, n) == 1, np.float32(0.0), np.float32(-0.0)).astype(np.float32),
        "few distinct values": rng.integers(-3, 4, n).astype(np.float32),
        "infinities": np.where(rng.integers(0, 4, n) == 0, -np.inf, rng.integers(0, 3, n)).astype(np.float32),
    }
    for name, scores in cases.items():
        for k in ks:
            assert _same(select_model(scores, k, slab_rows), _expect(oracle, scores, k)), (name, k)


def test_selection_model_k_equals_n_and_single_slab(oracle):
    rng = np.random.default_rng(12)
    for n in (1, 63, 1000):
        scores = rng.integers(0, 5, n).astype(np.float32)
        for k in {1, n // 2, n} - {0}:
            assert _same(select_model(scores, k), _expect(oracle, scores, k)), (n, k)


def test_all_nan_row_returns_the_first_rows():
    scores = np.full(3000, np.nan, np.float32)
    rows, _ = select_model(scores, 10, 64 * 16)
    assert rows.tolist() == list(range(10))


def test_list_order_is_what_breaks_ties(oracle):
    """the design's one assumption, shown by breaking it: lists taken in another order than slab order put a higher row in
    front of a lower one with the same score"""
    scores = np.zeros(1000, np.float32)
    exp = _expect(oracle, scores, 8)
    assert _same(select_model(scores, 8, 100), exp)
    n_slabs = len(slab_bounds(1000, 100)) - 1
    got = select_model(scores, 8, 100, list_order=list(range(n_slabs))[::-1])
    assert not (got[0] == exp[0]).all()


def test_brute_force_oracle_is_topk_of_all_scores(oracle):
    """oracle.brute_force (the reference of the GPU tests) = oracle.topk over oracle.score_rows of every row"""
    rng = np.random.default_rng(13)
    base = rng.standard_normal((70, 64)).astype(np.float16)
    embs = np.tile(base, (3, 1))[rng.permutation(210)]
    ix = oracle.Index(embs, np.arange(210, dtype=np.int64) * 7 + 3, [np.zeros(0, np.int32)] * 2,
                      [np.zeros(211, np.int64)] * 2, np.zeros(1, np.int32))
    sc = oracle.Scorer("l2", 64, oracle.EMB_F16)
    q = embs[17].astype(np.float32)
    rc, bi, bv = oracle.brute_force(ix, sc, q, 20)
    rc2, scores = oracle.score_rows(sc, q, embs)
    assert rc == 0 and rc2 == 0
    assert _same((bi, bv), _expect(oracle, scores, 20))
    assert _same(select_model(scores, 20, 64), (bi, bv))
