"""CPU: the fused top-k and the fused multi-vector searches as far as they can be held without a GPU -- the numpy model of the
contract (fuse_model.model) against its plain Python restatement on random small cases, cross-checks of the model against the
union's and against itself, the six symbols, the constants, the build lists, every refusal of nann_fuse_topk, which stands in
front of the first launch and so needs no device, and the Python helpers that touch no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import fuse_model as FM
import union_model as UM
from nann_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nann_fuse_topk_workspace_bytes", "nann_fuse_topk", "nann_search_multi_fused_workspace_bytes",
           "nann_search_multi_fused", "nann_search_all_multi_fused_workspace_bytes", "nann_search_all_multi_fused")
OK, BAD_ARGUMENT, UNSUPPORTED, CAPACITY = 0, 7, 102, 103
F = np.float32


def _header():
    return open(os.path.join(ROOT, "include", "nann_hip.h")).read()


# ---- the model against the restatement ------------------------------------------------------------------------------------
VALUES = np.array([-np.inf, -1.5, -0.0, 0.0, 0.25, 2.0, 7.5], F)
WEIGHTS = np.array([-1.5, 0.0, 0.25, 1.0, 2.0], F)


def _case(rng, mode):
    """one user: most entries collide (pools of 3-50 rows, now and then 7), scores quantised to 4 of VALUES (so +-0 meet, and
    -inf under SUM and RRF), duplicates within a list, n_valid anywhere from negative to beyond k_in or none, a few rows outside
    [0, n_items), single-entry lists, weights of both layouts.  Where -inf stands among the scores the weights are positive:
    0 * -inf and a sum of +inf and -inf are outside the contract."""
    n_lists, k_in = int(rng.integers(1, 7)), int(rng.integers(1, 13))
    n_items = 7 if rng.random() < 0.2 else int(rng.integers(3, 51))
    pool = VALUES if mode in (FM.SUM, FM.RRF) else VALUES[1:]
    vals = rng.choice(pool, 4, replace=False)
    scores = vals[rng.integers(0, 4, (n_lists, k_in))].astype(F)
    if rng.random() < 0.15:
        scores[:] = F(1.25)  # equal scores everywhere
    rows = rng.integers(0, n_items, (n_lists, k_in)).astype(np.int32)
    bad = rng.random((n_lists, k_in)) < 0.05
    rows[bad] = rng.choice(np.array([-1, -7, n_items, n_items + 3, 2 ** 31 - 1, -2 ** 31], np.int64), int(bad.sum())).astype(np.int32)
    n_valid = None if rng.random() < 0.2 else rng.integers(-2, k_in + 3, n_lists).astype(np.int32)
    if n_valid is not None and rng.random() < 0.1:
        n_valid[:] = 0
    if n_valid is not None and rng.random() < 0.2:
        n_valid[rng.integers(0, n_lists)] = 1  # a single-entry list: hi == lo
    layout = int(rng.integers(0, 3))  # 0: none, 1: per call, 2: per user
    w = np.ones(n_lists, F) if layout == 0 else rng.choice(WEIGHTS, n_lists).astype(F)
    if layout != 0 and np.isinf(scores).any():
        w = np.abs(w) + F(0.5)
    k = int(rng.integers(0, n_lists * k_in + 1))
    return scores, rows, n_valid, n_items, k, layout, w.astype(F)


def test_model_equals_the_restatement_on_1000_cases():
    rng = np.random.default_rng(20241020)
    seen = {"tie": 0, "dup": 0, "empty": 0, "multi": 0, "inf": 0, "single": 0}
    for i in range(1000):
        mode = i % 4
        scores, rows, n_valid, n_items, k, layout, w = _case(rng, mode)
        rrf_c = float(rng.choice([0.0, 1.0, 60.0]))
        # the user stands second in a batch of two, so that a per-user weight is looked up at u * n_lists + l
        other = np.zeros_like(scores)
        weights = None if layout == 0 else (w if layout == 1 else np.stack([np.full_like(w, 9.0), w]))
        got = FM.model(np.stack([other, scores]), np.stack([rows, rows]), None if n_valid is None else np.stack([n_valid, n_valid]),
                       n_items, k, mode, weights=weights, rrf_c=rrf_c)
        exp = FM.restate(scores.tolist(), rows.tolist(), None if n_valid is None else n_valid.tolist(), n_items, k, mode,
                         w.tolist(), rrf_c)
        m = int(got["n_out"][1])
        assert m == len(exp), i
        assert got["index"][1, :m].tolist() == [e[0] for e in exp], i
        assert (got["scores"][1, :m].view(np.uint32) == np.array([e[1] for e in exp], F).view(np.uint32)).all(), i
        assert got["lists"][1, :m].tolist() == [e[2] for e in exp], i
        assert not got["index"][1, m:].any() and not got["scores"][1, m:].view(np.uint32).any() and not got["lists"][1, m:].any()
        assert len(set(got["index"][1, :m].tolist())) == m  # distinct rows
        assert not np.isnan(got["scores"]).any()
        seen["dup"] += m < min(k, scores.size)
        seen["empty"] += m == 0 and k > 0
        seen["tie"] += m > 1 and (np.diff(UM.score_key(got["scores"][1, :m]).astype(np.int64)) == 0).any()
        seen["multi"] += any(bin(e[2]).count("1") > 1 for e in exp)
        seen["inf"] += bool(np.isinf(got["scores"][1, :m]).any())
        seen["single"] += n_valid is not None and (np.clip(n_valid, 0, scores.shape[1]) == 1).any()
    assert seen["tie"] > 100 and seen["dup"] > 100 and seen["empty"] > 5 and seen["multi"] > 300, seen
    assert seen["inf"] > 20 and seen["single"] > 50, seen


def test_the_terms_by_hand():
    # list 0: rows 5, 5, 9 with 0.5, 1.0, -0.0 -- row 5 counts at j = 0 (0.5), not at its better j = 1; list 1: rows 7, 5, -1
    scores = np.array([[0.5, 1.0, -0.0], [0.0, 4.0, 9.0]], F)
    rows = np.array([[5, 5, 9], [7, 5, -1]], np.int32)
    w = np.array([2.0, 0.5], F)
    got = FM.model(scores[None], rows[None], None, 10, 6, FM.SUM, weights=w)
    # row 5: 2 * 0.5 + 0.5 * 4 = 3; row 9: 2 * -0 = -0 -> +0 + -0 = +0; row 7: 0.5 * 0 = 0: the tie goes to row 9 (p = 2 < 3)
    assert got["n_out"][0] == 3 and got["index"][0].tolist() == [5, 9, 7, 0, 0, 0]
    assert got["scores"][0].view(np.uint32).tolist() == np.array([3.0, 0.0, 0.0, 0, 0, 0], F).view(np.uint32).tolist()
    assert got["lists"][0].tolist() == [3, 1, 2, 0, 0, 0]
    # SUM_FLOOR: lo_0 = -0 read as +0 over (0.5, 1.0, -0.0), lo_1 = 0 over (0.0, 4.0) -- the invalid 9.0 does not count
    got = FM.model(scores[None], rows[None], None, 10, 6, FM.SUM_FLOOR, weights=w)
    assert got["index"][0, :3].tolist() == [5, 9, 7] and got["scores"][0, :3].tolist() == [3.0, 0.0, 0.0]
    # MINMAX: list 0 spans [0, 1], list 1 [0, 4]: row 5 -> 2 * 0.5 + 0.5 * 1
    got = FM.model(scores[None], rows[None], None, 10, 6, FM.MINMAX, weights=w)
    assert got["index"][0, :3].tolist() == [5, 9, 7] and got["scores"][0, :3].tolist() == [1.5, 0.0, 0.0]
    # RRF at c = 1: row 5 -> 2 / 2 + 0.5 / 3, row 9 -> 2 / 4, row 7 -> 0.5 / 2; the rank of row 9 is its j = 2 though j = 1 is ignored
    got = FM.model(scores[None], rows[None], None, 10, 6, FM.RRF, weights=w, rrf_c=1.0)
    assert got["index"][0, :3].tolist() == [5, 9, 7]
    assert got["scores"][0, :3].view(np.uint32).tolist() == \
        np.array([F(F(2) / F(2)) + F(F(0.5) / F(3)), F(2) / F(4), F(0.5) / F(2)], F).view(np.uint32).tolist()
    # n_valid cuts row 9 off; a negative count is an empty list; a single-entry list has hi == lo: the quotient is 1
    got = FM.model(scores[None], rows[None], np.array([[1, -3]], np.int32), 10, 6, FM.MINMAX, weights=w)
    assert got["n_out"][0] == 1 and got["index"][0, 0] == 5 and got["scores"][0, 0] == 2.0 and got["lists"][0, 0] == 1


# ---- cross-checks on the models alone ---------------------------------------------------------------------------------------
def test_one_list_sum_is_the_union():
    rng = np.random.default_rng(3)
    for _ in range(100):
        k_in, n_items = int(rng.integers(1, 30)), 40
        rows = rng.permutation(n_items)[:k_in].astype(np.int32)[None, None]  # no duplicates within the list
        rows[0, 0, rng.random(k_in) < 0.1] = -1
        scores = VALUES[rng.integers(0, len(VALUES), (1, 1, k_in))]
        n_valid = rng.integers(-1, k_in + 2, (1, 1)).astype(np.int32)
        k = int(rng.integers(0, k_in + 1))
        a = FM.model(scores, rows, n_valid, n_items, k, FM.SUM, weights=np.ones(1, F))
        b = UM.model(scores, rows, n_valid, n_items, k)
        assert (a["index"] == b["index"]).all() and (a["n_out"] == b["n_out"]).all()
        assert (a["scores"].view(np.uint32) == (b["scores"] + F(0.0)).view(np.uint32)).all()  # +0 + -0 = +0
        assert (a["lists"][0, :a["n_out"][0]] == 1).all()


def test_one_list_rrf_is_the_list_without_repeats():
    rng = np.random.default_rng(4)
    for _ in range(100):
        k_in = int(rng.integers(1, 30))
        rows = rng.integers(-1, 12, (1, 1, k_in)).astype(np.int32)
        scores = rng.standard_normal((1, 1, k_in)).astype(F)  # (RRF does not look at them)
        got = FM.model(scores, rows, None, 11, k_in, FM.RRF)
        firsts = [r for j, r in enumerate(rows[0, 0].tolist()) if 0 <= r < 11 and r not in rows[0, 0, :j].tolist()]
        assert got["n_out"][0] == len(firsts) and got["index"][0, :len(firsts)].tolist() == firsts


def test_minmax_terms_lie_between_zero_and_the_weight():
    rng = np.random.default_rng(5)
    for _ in range(200):
        k_in = int(rng.integers(1, 20))
        scores = (rng.standard_normal((1, k_in)) * 10.0 ** rng.integers(-3, 4)).astype(F)
        rows = rng.integers(0, 9, (1, k_in)).astype(np.int32)
        w = F(rng.choice([0.0, 0.25, 1.0, 3.0]))
        _, fused, _, _ = FM.fuse_user(scores, rows, None, 9, FM.MINMAX, np.array([w], F))
        assert (fused >= 0).all() and (fused <= w).all()
        if len(set(rows[0].tolist())) == k_in:
            assert fused.max() == w  # no row stands twice: the list's best entry counts, and sits at the ceiling


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_the_six_symbols_are_declared_exported_and_bound():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = C.CDLL(build.build())
    bound = _lib.lib()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % s, code), s
        assert hasattr(lib, s), s
        assert s in _lib.SYMBOLS, s
        assert getattr(bound, s).argtypes, s
    assert "#define NANN_ABI_VERSION 6" in _header()
    assert not any(s.startswith(("nann_search_multi_fused_model", "nann_search_all_multi_fused_model", "nann_search_model_multi"))
                   for s in _lib.SYMBOLS)
    assert C.sizeof(_lib.Fusion) == 24 and _lib.Fusion.weights.offset == 16
    assert re.search(r"typedef struct nann_fusion \{[^}]*int32_t struct_bytes;[^}]*int32_t mode;[^}]*float\s+rrf_c;[^}]*"
                     r"int32_t weights_per_user;[^}]*const float\* weights;[^}]*\} nann_fusion;", code)


def test_the_limit_is_64_everywhere():
    from nann_amd import retrieval
    assert re.search(r"#define NANN_FUSE_MAX_LISTS 64\b", _header())
    assert _lib.FUSE_MAX_LISTS == retrieval.FUSE_MAX_LISTS == FM.MAX_LISTS == 64
    assert "NANN_FUSE_MAX_LISTS == 64" in open(os.path.join(build.SRC_DIR, "nann_fuse.h")).read()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"NANN_FUSE_SUM = 0, NANN_FUSE_SUM_FLOOR = 1, NANN_FUSE_MINMAX = 2, NANN_FUSE_RRF = 3", code)
    assert (_lib.FUSE_SUM, _lib.FUSE_SUM_FLOOR, _lib.FUSE_MINMAX, _lib.FUSE_RRF) == (FM.SUM, FM.SUM_FLOOR, FM.MINMAX, FM.RRF) == (0, 1, 2, 3)
    assert retrieval.FUSION_MODES == FM.MODES


def test_the_kernel_rides_in_the_candidate_object():
    assert "nann_fuse.h" in build.DEPS
    assert len(build.UNITS) == 17
    src = open(os.path.join(build.SRC_DIR, "nann_cand_inst.hip")).read()
    assert '#include "nann_fuse.h"' in src and "#define NANN_FUSE_IMPL" in src
    assert "-ffp-contract=off" in build.FLAGS
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = text[text.index("\n## 2. Build"):text.index("\n## 3. ")]
    assert "nann_fuse.h" in section and "seventeen translation units" in section


def test_the_header_states_the_contract():
    text = _header()
    section = text[text.index("fused result lists: reciprocal rank fusion"):text.index("8(f3): the evaluation graph")]
    assert text.index("attribute predicates: per-query label") < text.index("fused result lists: reciprocal rank fusion")
    section = " ".join(section.replace("\n *", " ").split())
    for phrase in ("The reference has no such call",
                   "j < clamp(n_valid[u][l], 0, k_in) and its row lies in [0, n_items)",
                   "a list whose status word is non-zero counts as 0 entries",
                   "malformed input never faults",
                   "a row COUNTS ONCE, at its lowest valid j",
                   "whether or not the entries before it are valid",
                   "Every step is a single f32 operation",
                   "no FMA contraction",
                   "w * (s - lo_l)",
                   "w * ((s - lo_l) / (hi_l - lo_l))",
                   "the quotient is read as 1.0f",
                   "w / (rrf_c + (float)(j + 1))",
                   "with -0 read as +0",
                   "a missing list must not look better than a present one",
                   "the margin over the floors",
                   "starts from +0.0f",
                   "in ascending l, one f32 add each",
                   "ties -> the lower first p",
                   "n_out[u] = min(k, distinct valid rows)",
                   "does not depend on the batch",
                   "bit l is set iff list l contains the row",
                   "NULL means 1.0f",
                   "no host read-back",
                   "-inf is a score like any other",
                   "Nothing is launched and nothing is written by a refused call",
                   "a failed vector contributes nothing",
                   "has no exactness property",
                   "the caller's trade-off",
                   "equals ONE query with the weighted sum of the vectors",
                   "There are no _model forms"):
        assert phrase in section, phrase


# ---- every refusal of nann_fuse_topk, without a device ----------------------------------------------------------------------
def _fusion(mode=FM.RRF, rrf_c=60.0, per_user=0, struct_bytes=None, weights=0):
    return _lib.Fusion(C.sizeof(_lib.Fusion) if struct_bytes is None else struct_bytes, mode, rrf_c, per_user,
                       0x70000 if weights else None)


def _fuse(L, n_users=2, n_lists=3, k_in=4, n_items=100, k=5, scores=1, rows=1, item_ids=None, out_index=1, out_item_ids=None,
          ws=256 * 4, ws_bytes=None, fusion="default"):
    """nann_fuse_topk with made-up addresses (256-byte aligned where it matters): nothing is dereferenced by a refused call"""
    p = lambda v: C.c_void_p(0x10000 * v) if isinstance(v, int) and v else (C.c_void_p(v) if v else None)
    need = C.c_int64(-1)
    if ws_bytes is None:
        L.nann_fuse_topk_workspace_bytes(max(n_users, 0), min(max(n_lists, 0), 64), max(k_in, 0), C.byref(need))
        ws_bytes = max(need.value, 0)
    f = _fusion(weights=1) if fusion == "default" else fusion
    return L.nann_fuse_topk(p(scores), p(rows), None, n_users, n_lists, k_in, n_items, p(item_ids), k,
                            C.byref(f) if f is not None else None, p(out_index), None, p(out_item_ids), None, None,
                            C.c_void_p(ws) if ws else None, ws_bytes, None)


def test_fuse_topk_refusals_need_no_device():
    L = _lib.lib()
    # the union's, in its order
    assert _fuse(L, n_users=-1) == BAD_ARGUMENT
    assert _fuse(L, n_lists=-1, k=0) == BAD_ARGUMENT
    assert _fuse(L, k_in=-1, k=0) == BAD_ARGUMENT
    assert _fuse(L, n_items=-1) == BAD_ARGUMENT
    assert _fuse(L, k=-1) == BAD_ARGUMENT
    assert _fuse(L, k=13) == BAD_ARGUMENT                      # k > n_lists * k_in = 12
    assert b"k exceeds" in L.nann_last_error()
    assert _fuse(L, n_lists=2, k_in=1024, k=1025) == UNSUPPORTED   # k > 1024
    assert _fuse(L, n_lists=8, k_in=1025, k=5) == UNSUPPORTED      # 8200 entries
    assert b"NANN_UNION_MAX_IN" in L.nann_last_error()
    assert _fuse(L, n_items=2 ** 31) == UNSUPPORTED
    # then the lists: 65 of them within 8192 entries
    assert _fuse(L, n_lists=65, k_in=2, k=5) == UNSUPPORTED
    assert b"NANN_FUSE_MAX_LISTS" in L.nann_last_error()
    assert _fuse(L, n_lists=8193, k_in=1, k=5) == UNSUPPORTED and b"NANN_UNION_MAX_IN" in L.nann_last_error()  # (the entries first)
    assert _fuse(L, n_lists=65, k_in=2, k=5, fusion=None) == UNSUPPORTED                                       # (ahead of the struct)
    # then the struct
    assert _fuse(L, fusion=None) == BAD_ARGUMENT and b"null fusion" in L.nann_last_error()
    assert _fuse(L, fusion=_fusion(struct_bytes=8)) == BAD_ARGUMENT and b"struct_bytes" in L.nann_last_error()
    assert _fuse(L, fusion=_fusion(mode=4)) == BAD_ARGUMENT and b"unknown mode" in L.nann_last_error()
    assert _fuse(L, fusion=_fusion(mode=-1)) == BAD_ARGUMENT
    for c in (-1.0, float("nan"), float("inf"), -0.5):
        assert _fuse(L, fusion=_fusion(rrf_c=c)) == BAD_ARGUMENT and b"rrf_c" in L.nann_last_error()
    assert _fuse(L, fusion=_fusion(per_user=2)) == BAD_ARGUMENT and b"weights_per_user" in L.nann_last_error()
    assert _fuse(L, fusion=_fusion(per_user=-1)) == BAD_ARGUMENT
    assert _fuse(L, fusion=_fusion(struct_bytes=8, mode=9)) == BAD_ARGUMENT and b"struct_bytes" in L.nann_last_error()  # (its order)
    # the struct ahead of the early NANN_OK, the early NANN_OK ahead of the pointers
    assert _fuse(L, n_users=0, fusion=None) == BAD_ARGUMENT
    assert _fuse(L, k=0, fusion=_fusion(mode=7)) == BAD_ARGUMENT
    assert _fuse(L, n_users=0, scores=0, rows=0, out_index=0, ws=0, ws_bytes=0) == OK
    assert _fuse(L, k=0, scores=0, rows=0, out_index=0, ws=0, ws_bytes=0) == OK
    assert _fuse(L, n_users=0, out_item_ids=3) == OK
    assert _fuse(L, k=0, out_item_ids=3) == OK
    # rrf_c is RRF's alone; struct_bytes 0 is accepted (the remaining faults of these calls are the short workspace)
    assert _fuse(L, fusion=_fusion(mode=FM.SUM, rrf_c=-1.0), ws_bytes=0) == CAPACITY
    assert _fuse(L, fusion=_fusion(struct_bytes=0), ws_bytes=0) == CAPACITY
    assert _fuse(L, fusion=_fusion(rrf_c=0.0), ws_bytes=0) == CAPACITY
    # then the pointers, out_item_ids without item_ids, the workspace's size, its alignment
    assert _fuse(L, scores=0) == BAD_ARGUMENT
    assert _fuse(L, rows=0) == BAD_ARGUMENT
    assert _fuse(L, out_index=0) == BAD_ARGUMENT
    assert b"null argument" in L.nann_last_error()
    assert _fuse(L, out_item_ids=3) == BAD_ARGUMENT and b"out_item_ids without item_ids" in L.nann_last_error()
    assert _fuse(L, scores=0, out_item_ids=3, ws=0) == BAD_ARGUMENT and b"null argument" in L.nann_last_error()
    assert _fuse(L, out_item_ids=3, ws=0) == BAD_ARGUMENT and b"out_item_ids" in L.nann_last_error()
    assert _fuse(L, n_lists=8, k_in=1024, k=1024, ws_bytes=2 * 8192 * 24 - 1) == CAPACITY  # one byte short at the limit
    assert _fuse(L, ws=0) == CAPACITY
    assert _fuse(L, ws_bytes=0) == CAPACITY
    assert b"nann_fuse_topk_workspace_bytes" in L.nann_last_error()
    assert _fuse(L, ws=256 * 4 + 64, ws_bytes=0) == CAPACITY   # the size ahead of the alignment
    assert _fuse(L, ws=256 * 4 + 64) == BAD_ARGUMENT           # off the 256-byte grid
    assert b"256-byte aligned" in L.nann_last_error()


def test_workspace_bytes_leaves_its_output_untouched_on_failure():
    L = _lib.lib()
    nb = C.c_int64(-1)
    assert L.nann_fuse_topk_workspace_bytes(-1, 3, 4, C.byref(nb)) == BAD_ARGUMENT
    assert L.nann_fuse_topk_workspace_bytes(2, -3, 4, C.byref(nb)) == BAD_ARGUMENT
    assert L.nann_fuse_topk_workspace_bytes(2, 3, -4, C.byref(nb)) == BAD_ARGUMENT
    assert L.nann_fuse_topk_workspace_bytes(2, 9, 1000, C.byref(nb)) == UNSUPPORTED
    assert L.nann_fuse_topk_workspace_bytes(2, 65, 4, C.byref(nb)) == UNSUPPORTED
    assert nb.value == -1
    assert L.nann_fuse_topk_workspace_bytes(2, 3, 4, None) == BAD_ARGUMENT
    assert L.nann_fuse_topk_workspace_bytes(2, 3, 4, C.byref(nb)) == OK and nb.value == 768      # 2 x 12 x 24 B, rounded up
    assert L.nann_fuse_topk_workspace_bytes(3, 8, 1024, C.byref(nb)) == OK and nb.value == 3 * 8192 * 24
    assert L.nann_fuse_topk_workspace_bytes(2, 64, 128, C.byref(nb)) == OK and nb.value == 2 * 8192 * 24
    assert L.nann_fuse_topk_workspace_bytes(0, 3, 4, C.byref(nb)) == OK and nb.value == 0


def test_null_handles_of_the_composed_calls_are_bad_arguments_without_a_gpu():
    L = _lib.lib()
    nb = C.c_int64(-1)
    t = (C.c_int32 * 6)(8, 16, 32, 32, 32, 50)
    f = _fusion()
    assert L.nann_search_multi_fused_workspace_bytes(None, t, 3, 2, C.byref(nb)) == BAD_ARGUMENT
    assert L.nann_search_all_multi_fused_workspace_bytes(None, None, 3, 2, 10, C.byref(nb)) == BAD_ARGUMENT
    assert nb.value == -1
    assert L.nann_search_multi_fused(None, None, None, 3, 2, t, None, None, 0, None, None, None, None, None, None, None, None, None,
                                     10, C.byref(f), None) == BAD_ARGUMENT
    assert L.nann_search_all_multi_fused(None, None, None, 3, 2, 10, 10, C.byref(f), None, None, None, None, None, None, 0, None,
                                         None) == BAD_ARGUMENT
    assert L.nann_search_all_multi_fused(None, None, None, 3, 0, 10, 10, C.byref(f), None, None, None, None, None, None, 0, None,
                                         None) == BAD_ARGUMENT
    assert b"n_vec < 1" in L.nann_last_error()


# ---- the Python helpers that need no device ---------------------------------------------------------------------------------
def test_make_fusion():
    from nann_amd import retrieval
    f = retrieval.make_fusion()
    assert (f.mode, f.weights, f.rrf_c) == ("rrf", None, 60.0)
    f = retrieval.make_fusion("sum_floor", weights=[1, 2.5, -3])
    assert f.mode == "sum_floor" and f.weights.dtype == torch.float32 and f.weights.tolist() == [1.0, 2.5, -3.0]
    f = retrieval.make_fusion("minmax", weights=np.ones((4, 3)), rrf_c=0)
    assert tuple(f.weights.shape) == (4, 3) and f.rrf_c == 0.0
    s, kept = retrieval._fusion_args(f, 4, 3, "cpu")
    assert (s.struct_bytes, s.mode, s.weights_per_user) == (24, FM.MINMAX, 1) and s.weights == kept.data_ptr()
    s, kept = retrieval._fusion_args(retrieval.make_fusion("rrf", weights=[1.0, 2.0, 3.0], rrf_c=10), 4, 3, "cpu")
    assert (s.mode, s.weights_per_user, s.rrf_c) == (FM.RRF, 0, 10.0) and s.weights == kept.data_ptr()
    s, kept = retrieval._fusion_args(retrieval.make_fusion("sum"), 4, 3, "cpu")
    assert s.mode == FM.SUM and s.weights is None and kept is None
    for bad in (dict(mode="max"), dict(rrf_c=-1.0), dict(rrf_c=float("inf")), dict(rrf_c=float("nan")), dict(weights=np.ones((2, 2, 2)))):
        with pytest.raises(AssertionError):
            retrieval.make_fusion(**bad)
    with pytest.raises(AssertionError):
        retrieval._fusion_args(retrieval.make_fusion(weights=[1.0, 2.0]), 4, 3, "cpu")  # two weights for three lists


class _Result:
    def __init__(self, index, scores, n_out=None):
        self.index, self.scores = torch.as_tensor(index, dtype=torch.int32), torch.as_tensor(scores, dtype=torch.float32)
        if n_out is not None:
            self.n_out = torch.as_tensor(n_out, dtype=torch.int32)


def test_fuse_results_pads_to_the_widest():
    from nann_amd import retrieval
    a = _Result([[1, 2, 3], [4, 5, 6]], [[3.0, 2.0, 1.0], [6.0, 5.0, 4.0]])                # no n_out: its width counts
    b = _Result([[7, 8, 9, 10, 11], [12, 13, 0, 0, 0]], np.arange(10.0).reshape(2, 5), n_out=[5, 2])
    scores, rows, n_valid = retrieval._stack_results([a, b])
    assert tuple(scores.shape) == tuple(rows.shape) == (2, 2, 5) and scores.dtype == torch.float32 and rows.dtype == torch.int32
    assert rows[:, 0].tolist() == [[1, 2, 3, 0, 0], [4, 5, 6, 0, 0]] and rows[:, 1].tolist() == b.index.tolist()
    assert scores[:, 0].tolist() == [[3.0, 2.0, 1.0, 0.0, 0.0], [6.0, 5.0, 4.0, 0.0, 0.0]] and scores[:, 1].tolist() == b.scores.tolist()
    assert n_valid.tolist() == [[3, 5], [3, 2]]
    # and the model over what it stacked is the hybrid answer: row ids from both lists, the padding never counts
    exp = FM.model(scores.numpy(), rows.numpy(), n_valid.numpy(), 100, 8, FM.RRF)
    assert exp["n_out"].tolist() == [8, 5] and 0 not in exp["index"][0].tolist() and 0 not in exp["index"][1, :5].tolist()
    with pytest.raises(AssertionError):
        retrieval._stack_results([])
    with pytest.raises(AssertionError):
        retrieval._stack_results([a, _Result([[1, 2]], [[1.0, 2.0]])])  # another batch
