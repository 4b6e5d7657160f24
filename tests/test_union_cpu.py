"""CPU: the union top-k and the multi-vector searches as far as they can be held without a GPU -- the numpy model of the
contract (union_model.model) against its plain Python restatement on random small cases, the exactness of "union of per-vector
top-k lists" on the oracle alone, the six symbols, the constant, the build lists, and every refusal of nann_union_topk, which
stands in front of the first launch and so needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ip_reference as R
import union_model as UM
from nann_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nann_union_topk_workspace_bytes", "nann_union_topk", "nann_search_multi_workspace_bytes", "nann_search_multi",
           "nann_search_all_multi_workspace_bytes", "nann_search_all_multi")
OK, BAD_ARGUMENT, UNSUPPORTED, CAPACITY = 0, 7, 102, 103


def _header():
    return open(os.path.join(ROOT, "include", "nann_hip.h")).read()


# ---- the model against the restatement ------------------------------------------------------------------------------------
VALUES = np.array([-np.inf, -1.5, -0.0, 0.0, 0.25, 2.0], np.float32)


def _case(rng):
    """one user: most entries collide (pools of 3-50 rows), scores quantised to 4 of VALUES (so +-0 and -inf meet), n_valid
    anywhere from negative to beyond k_in, a few rows outside [0, n_items)"""
    n_lists, k_in = int(rng.integers(1, 7)), int(rng.integers(1, 13))
    n_items = int(rng.integers(3, 51))
    vals = rng.choice(VALUES, 4, replace=False)
    scores = vals[rng.integers(0, 4, (n_lists, k_in))].astype(np.float32)
    rows = rng.integers(0, n_items, (n_lists, k_in)).astype(np.int32)
    bad = rng.random((n_lists, k_in)) < 0.05
    rows[bad] = rng.choice(np.array([-1, -7, n_items, n_items + 3, 2 ** 31 - 1, -2 ** 31], np.int64), int(bad.sum())).astype(np.int32)
    n_valid = None if rng.random() < 0.2 else rng.integers(-2, k_in + 3, n_lists).astype(np.int32)
    if n_valid is not None and rng.random() < 0.1:
        n_valid[:] = 0
    k = int(rng.integers(0, n_lists * k_in + 1))
    return scores, rows, n_valid, n_items, k


def test_model_equals_the_restatement_on_1000_cases():
    rng = np.random.default_rng(20240611)
    seen_tie = seen_dup = seen_empty = 0
    for _ in range(1000):
        scores, rows, n_valid, n_items, k = _case(rng)
        got = UM.model(scores[None], rows[None], None if n_valid is None else n_valid[None], n_items, k)
        exp = UM.restate(scores.tolist(), rows.tolist(), None if n_valid is None else n_valid.tolist(), n_items, k)
        m = int(got["n_out"][0])
        assert m == len(exp)
        assert got["index"][0, :m].tolist() == [e[0] for e in exp]
        assert (got["scores"][0, :m].view(np.uint32) == np.array([e[1] for e in exp], np.float32).view(np.uint32)).all()
        assert got["list"][0, :m].tolist() == [e[2] for e in exp]
        assert not got["index"][0, m:].any() and not got["scores"][0, m:].view(np.uint32).any() and not got["list"][0, m:].any()
        assert len(set(got["index"][0, :m].tolist())) == m  # distinct rows
        seen_dup += m < min(k, scores.size)
        seen_empty += m == 0 and k > 0
        seen_tie += m > 1 and (np.diff(UM.score_key(got["scores"][0, :m]).astype(np.int64)) == 0).any()
    assert seen_tie > 100 and seen_dup > 100 and seen_empty > 5


def test_the_key_is_monotone_and_folds_the_zeros():
    s = np.array([-np.inf, -3.0, -1e-30, -0.0, 0.0, 1e-30, 3.0, np.inf], np.float32)
    key = UM.score_key(s).astype(np.int64)
    assert key[3] == key[4]
    assert (np.diff(key)[[0, 1, 2, 4, 5, 6]] > 0).all()


def test_the_representative_and_the_order_by_hand():
    # row 5: 1.0 at p = 1 and p = 4 -> p = 1 represents it; row 9 at -0.0 (p = 2) ties row 7 at +0.0 (p = 3): p = 2 first
    scores = np.array([[0.5, 1.0, -0.0], [0.0, 1.0, 9.0]], np.float32)
    rows = np.array([[5, 5, 9], [7, 5, -1]], np.int32)
    got = UM.model(scores[None], rows[None], None, 10, 6)
    assert got["n_out"][0] == 3
    assert got["index"][0].tolist() == [5, 9, 7, 0, 0, 0]
    assert got["list"][0].tolist() == [0, 0, 1, 0, 0, 0]
    assert got["scores"][0].view(np.uint32).tolist() == np.array([1.0, -0.0, 0.0, 0, 0, 0], np.float32).view(np.uint32).tolist()
    # n_valid cuts row 9 off; a negative count is an empty list
    got = UM.model(scores[None], rows[None], np.array([[2, -3]], np.int32), 10, 6)
    assert got["n_out"][0] == 1 and got["index"][0, 0] == 5 and got["list"][0, 0] == 0


# ---- the union of per-vector top-k lists is exact -------------------------------------------------------------------------
def _oracle_l2_scores(O, embs):
    """v -> the oracle's L2 score of every row for query v (its brute force at k = n, scattered back by row)"""
    n, d = embs.shape
    nbv = ((np.arange(n, dtype=np.int64)[:, None] + 1 + np.arange(8)) % n).astype(np.int32).reshape(-1)
    rs = np.arange(n + 1, dtype=np.int64) * 8
    oix = O.Index(embs, np.arange(n, dtype=np.int64), [nbv, nbv.copy()], [rs, rs.copy()], np.arange(0, n, 5, dtype=np.int32))
    osc = O.Scorer("l2", d, O.EMB_F16)

    def score(v, _wide):
        rc, bi, bv = O.brute_force(oix, osc, v, n)
        assert rc == 0 and sorted(bi.tolist()) == list(range(n))
        full = np.empty(n, np.float32)
        full[bi] = bv
        return full
    return score


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_union_of_per_vector_topk_is_the_topk_of_the_row_maximum(oracle, metric):
    """on the references alone (L2: the oracle's brute force; the inner product: ip_reference): the sorted scores of
    union(per-vector brute-force top k) are, bit for bit, the k largest of max over the vectors of a row's score"""
    n, d = 300, 64
    rng = np.random.default_rng(11 if metric == "l2" else 12)
    embs = rng.standard_normal((n, d)).astype(np.float16)
    embs[100:110] = embs[0:10]  # duplicate rows: ties across rows
    wide = R.widen(embs)
    score = _oracle_l2_scores(oracle, embs) if metric == "l2" else R.ip_scores
    for n_vec in range(1, 9):
        for k in (1, 7, 50, 300):
            q = rng.standard_normal((n_vec, d)).astype(np.float32)
            if n_vec > 2:
                q[2] = q[0]  # a repeated interest
            full = np.stack([score(v, wide) for v in q])  # [n_vec, n]
            tops = [R.topk_stable(s, k) for s in full]
            rows = np.stack(tops).astype(np.int32)
            scores = np.stack([s[t] for s, t in zip(full, tops)])
            got = UM.model(scores[None], rows[None], None, n, k)
            assert got["n_out"][0] == k
            best = full.max(axis=0)
            exp = best[R.topk_stable(best, k)]
            assert (got["scores"][0].view(np.uint32) == exp.view(np.uint32)).all(), (n_vec, k)
            assert (full[got["list"][0], got["index"][0]].view(np.uint32) == got["scores"][0].view(np.uint32)).all()


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_the_six_symbols_are_declared_exported_and_bound():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = C.CDLL(build.build())
    for s in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % s, code), s
        assert hasattr(lib, s), s
        assert s in _lib.SYMBOLS, s
    assert "#define NANN_ABI_VERSION 6" in _header()
    assert not any(s.startswith(("nann_search_multi_model", "nann_search_all_multi_model")) for s in _lib.SYMBOLS)


def test_the_limit_is_8192_everywhere():
    from nann_amd import retrieval
    assert re.search(r"#define NANN_UNION_MAX_IN 8192\b", _header())
    assert _lib.UNION_MAX_IN == retrieval.UNION_MAX_IN == UM.MAX_IN == 8192
    src = open(os.path.join(build.SRC_DIR, "nann_union.h")).read()
    assert "NANN_UNION_MAX_IN == 8192" in src


def test_the_kernel_rides_in_the_candidate_object():
    assert "nann_union.h" in build.DEPS
    assert len(build.UNITS) == 17
    assert '#include "nann_union.h"' in open(os.path.join(build.SRC_DIR, "nann_cand_inst.hip")).read()
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "nann_union.h" in text[text.index("\n## 2. Build"):text.index("\n## 3. ")]


def test_the_header_states_the_contract():
    text = _header()
    section = text[text.index("multi-vector queries: union top-k"):text.index("8(f3): the evaluation graph")]
    section = " ".join(section.replace("\n *", " ").split())
    for phrase in ("The reference has no such call",
                   "j < clamp(n_valid[u][l], 0, k_in) and its row lies in [0, n_items)",
                   "malformed input never faults",
                   "ties -> the lowest p",
                   "n_out[u] = min(k, distinct valid rows)",
                   "-inf is a score like any other",
                   "does not depend on the batch",
                   "A failed vector contributes nothing",
                   "repeats one of them",
                   "nann_search_filtered over the n_users * n_vec vectors, then nann_union_topk with n_valid = its n_out",
                   "There is no _model form: a comm_seq is ONE user sequence",
                   "the k largest of max_m s(q_m, r)"):
        assert phrase in section, phrase


# ---- every refusal of nann_union_topk, without a device --------------------------------------------------------------------
def _union(L, n_users=2, n_lists=3, k_in=4, n_items=100, k=5, scores=1, rows=1, item_ids=None, out_index=1, out_item_ids=None,
           ws=256 * 4, ws_bytes=None):
    """nann_union_topk with made-up addresses (256-byte aligned where it matters): nothing is dereferenced by a refused call"""
    p = lambda v: C.c_void_p(0x10000 * v) if isinstance(v, int) and v else (C.c_void_p(v) if v else None)
    need = C.c_int64(-1)
    if ws_bytes is None:
        L.nann_union_topk_workspace_bytes(max(n_users, 0), max(n_lists, 0), max(k_in, 0), C.byref(need))
        ws_bytes = max(need.value, 0)
    return L.nann_union_topk(p(scores), p(rows), None, n_users, n_lists, k_in, n_items, p(item_ids), k, p(out_index), None,
                             p(out_item_ids), None, None, C.c_void_p(ws) if ws else None, ws_bytes, None)


def test_union_topk_refusals_need_no_device():
    L = _lib.lib()
    assert _union(L, n_users=-1) == BAD_ARGUMENT
    assert _union(L, n_lists=-1, k=0) == BAD_ARGUMENT
    assert _union(L, k_in=-1, k=0) == BAD_ARGUMENT
    assert _union(L, n_items=-1) == BAD_ARGUMENT
    assert _union(L, k=-1) == BAD_ARGUMENT
    assert _union(L, k=13) == BAD_ARGUMENT                      # k > n_lists * k_in = 12
    assert b"k exceeds" in L.nann_last_error()
    assert _union(L, out_item_ids=3) == BAD_ARGUMENT            # out_item_ids without item_ids
    assert b"out_item_ids without item_ids" in L.nann_last_error()
    assert _union(L, scores=0) == BAD_ARGUMENT
    assert _union(L, rows=0) == BAD_ARGUMENT
    assert _union(L, out_index=0) == BAD_ARGUMENT
    assert b"null argument" in L.nann_last_error()
    assert _union(L, ws=256 * 4 + 64) == BAD_ARGUMENT           # off the 256-byte grid
    assert b"256-byte aligned" in L.nann_last_error()
    assert _union(L, n_lists=2, k_in=1024, k=1025) == UNSUPPORTED   # k > 1024
    assert _union(L, n_lists=8, k_in=1025, k=5) == UNSUPPORTED      # 8200 entries
    assert _union(L, n_lists=8193, k_in=1, k=5) == UNSUPPORTED      # 8193 entries
    assert b"NANN_UNION_MAX_IN" in L.nann_last_error()
    assert _union(L, n_lists=8, k_in=1024, k=1024, ws_bytes=2 * 8192 * 8 - 1) == CAPACITY  # one byte short at the limit
    assert _union(L, ws=0) == CAPACITY
    assert _union(L, ws_bytes=0) == CAPACITY
    assert b"nann_union_topk_workspace_bytes" in L.nann_last_error()
    # nothing to do: NANN_OK whatever the pointers, nothing read or written
    assert _union(L, n_users=0, scores=0, rows=0, out_index=0, ws=0, ws_bytes=0) == OK
    assert _union(L, k=0, scores=0, rows=0, out_index=0, ws=0, ws_bytes=0) == OK
    # ... out_item_ids without item_ids included: the pointers are looked at behind the early NANN_OK
    assert _union(L, n_users=0, out_item_ids=3) == OK
    assert _union(L, k=0, out_item_ids=3) == OK
    # and the sizes ahead of the pointers
    assert _union(L, k=13, scores=0, out_item_ids=3) == BAD_ARGUMENT and b"k exceeds" in L.nann_last_error()
    assert _union(L, n_lists=8193, k_in=1, k=5, scores=0, out_item_ids=3) == UNSUPPORTED


def test_workspace_bytes_leaves_its_output_untouched_on_failure():
    L = _lib.lib()
    nb = C.c_int64(-1)
    assert L.nann_union_topk_workspace_bytes(-1, 3, 4, C.byref(nb)) == BAD_ARGUMENT
    assert L.nann_union_topk_workspace_bytes(2, -3, 4, C.byref(nb)) == BAD_ARGUMENT
    assert L.nann_union_topk_workspace_bytes(2, 3, -4, C.byref(nb)) == BAD_ARGUMENT
    assert L.nann_union_topk_workspace_bytes(2, 9, 1000, C.byref(nb)) == UNSUPPORTED
    assert nb.value == -1
    assert L.nann_union_topk_workspace_bytes(2, 3, 4, None) == BAD_ARGUMENT
    assert L.nann_union_topk_workspace_bytes(2, 3, 4, C.byref(nb)) == OK and nb.value == 256      # 2 x 12 x 8 B, rounded up
    assert L.nann_union_topk_workspace_bytes(3, 8, 1024, C.byref(nb)) == OK and nb.value == 3 * 8192 * 8
    assert L.nann_union_topk_workspace_bytes(0, 3, 4, C.byref(nb)) == OK and nb.value == 0


def test_null_handles_of_the_composed_calls_are_bad_arguments_without_a_gpu():
    L = _lib.lib()
    nb = C.c_int64(-1)
    t = (C.c_int32 * 6)(8, 16, 32, 32, 32, 50)
    assert L.nann_search_multi_workspace_bytes(None, t, 3, 2, C.byref(nb)) == BAD_ARGUMENT
    assert L.nann_search_all_multi_workspace_bytes(None, None, 3, 2, 10, C.byref(nb)) == BAD_ARGUMENT
    assert nb.value == -1
    assert L.nann_search_multi(None, None, None, 3, 2, t, None, None, 0, None, None, None, None, None, None, None, None, None, 10,
                               None) == BAD_ARGUMENT
    assert L.nann_search_all_multi(None, None, None, 3, 2, 10, None, None, None, None, None, None, 0, None, None) == BAD_ARGUMENT
    assert L.nann_search_all_multi(None, None, None, 3, 0, 10, None, None, None, None, None, None, 0, None, None) == BAD_ARGUMENT
    assert b"n_vec < 1" in L.nann_last_error()
