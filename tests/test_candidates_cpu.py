"""Candidate-list search (nann_search_candidates), the parts that need no GPU: the ABI, the well-formedness rule of the row
splits restated in numpy (and why it makes the accepted ranges disjoint), the work-item plan of csrc/nann_cand.h as a numpy
model, the sorted-allow-list property on the oracle alone, and the argument checks that run in front of any device call."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED, RANGE = 3, 5  # NANN_ERR_INVALID_RAGGED_INPUT, NANN_ERR_INDEX_OUT_OF_RANGE

# the hand-written split vectors (the GPU test runs the same ones on the device): name -> (splits, n_cand, well-formed?)
SPLIT_CASES = {
    "monotone": ([0, 3, 3, 10], 10, [True, True, True]),
    "inverted": ([0, 5, 2, 8], 10, [True, False, False]),          # query 2 begins (2) before an earlier split (5)
    "out of [0, n_cand]": ([-1, 4, 12, 12], 10, [False, False, False]),  # begins below 0; ends beyond n_cand; begins beyond n_cand
    "[0, 10, 5, 20]": ([0, 10, 5, 20], 20, [True, False, False]),  # query 1 inverted, query 2 begins before an earlier split
    "all equal": ([4, 4, 4, 4], 10, [True, True, True]),
}


def well_formed(splits, n_cand):
    """the contract, word for word: 0 <= s[i] <= s[i+1] <= n_cand and s[i] >= s[j] for every j < i"""
    s = [int(v) for v in splits]
    return np.array([0 <= s[i] <= s[i + 1] <= n_cand and all(s[i] >= s[j] for j in range(i)) for i in range(len(s) - 1)], bool)


def well_formed_running_max(splits, n_cand):
    """what k_cand_plan computes: s[i] >= s[j] for every j < i  <=>  s[i] is the running maximum of s[0 .. i]"""
    s = np.asarray(splits, np.int64)
    b, e = s[:-1], s[1:]
    return (b >= 0) & (b <= e) & (e <= n_cand) & (b >= np.maximum.accumulate(s)[:-1])


def plan_model(splits, n_cand, rows_per_item):
    """k_cand_plan + cand_item: (begin, len, status per query; the (query, begin, count) of every work item, found by the
    bisection the scoring kernels run on the exclusive prefix sum of the block counts)"""
    s = np.asarray(splits, np.int64)
    ok = well_formed_running_max(s, n_cand)
    begin = np.where(ok, s[:-1], 0)
    length = np.where(ok, s[1:] - s[:-1], 0)
    nb = (length + rows_per_item - 1) // rows_per_item
    off = np.concatenate([[0], np.cumsum(nb)])
    items = []
    for w in range(int(off[-1])):
        lo, hi = 0, len(nb)
        while hi - lo > 1:
            mid = lo + (hi - lo) // 2
            if off[mid] <= w:
                lo = mid
            else:
                hi = mid
        at = (w - int(off[lo])) * rows_per_item
        items.append((lo, int(begin[lo]) + at, min(rows_per_item, int(length[lo]) - at)))
    return begin, length, np.where(ok, 0, RAGGED), items


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_library_exports_search_candidates_and_header_documents_it():
    from nann_amd import _lib
    L = _lib.lib()  # builds for gfx950 when the sources changed
    assert L.nann_abi_version() == 6
    header = open(os.path.join(ROOT, "include", "nann_hip.h")).read()
    for name in ("nann_search_candidates_workspace_bytes", "nann_search_candidates"):
        assert name in _lib.SYMBOLS and getattr(L, name) is not None
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert re.search(r"\}\s*nann_candidates;", header) and "#define NANN_ABI_VERSION 6" in header
    assert "reference has no such call" in header and "WELL-FORMED" in header
    # the ctypes struct has the header's fields in the header's order
    fields = re.search(r"typedef struct \{([^}]*)\}\s*nann_candidates;", header).group(1)
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [f[0] for f in _lib.Candidates._fields_]


def test_block_sizes_are_read_from_one_place():
    from nann_amd import retrieval
    src = open(os.path.join(ROOT, "nann_amd", "csrc", "nann_cand.h")).read()
    assert int(re.search(r"constexpr int kCandRows = (\d+);", src).group(1)) == retrieval.CANDIDATE_BLOCK_ROWS
    assert int(re.search(r"constexpr int kCandMlpRows = (\d+);", src).group(1)) == retrieval.CANDIDATE_MLP_BLOCK_ROWS
    scan = open(os.path.join(ROOT, "nann_amd", "csrc", "nann_scan.h")).read()
    assert int(re.search(r"constexpr int kScanMlpRows = (\d+);", scan).group(1)) == retrieval.CANDIDATE_MLP_BLOCK_ROWS


def test_l2_scorer_keeps_the_traversal_addressing_flag():
    """the `near` argument of wg_score_l2_part is textually the expression k_search passes"""
    text = lambda rel: open(os.path.join(ROOT, "nann_amd", "csrc", rel)).read()
    expr = "(unsigned long long)a.n_items * (unsigned)(a.d * 2) <= 0xffffffffull && a.n_items <= (1u << 24)"
    assert expr in text("nann_search.h") and expr in text("nann_cand.h")


def test_null_arguments_are_bad_arguments_without_a_device():
    from nann_amd import _lib
    L = _lib.lib()
    nbytes = C.c_int64(-1)
    assert L.nann_search_candidates_workspace_bytes(None, None, 4, 100, 10, C.byref(nbytes)) == 7
    assert b"null argument" in L.nann_last_error() and nbytes.value == -1
    assert L.nann_search_candidates_workspace_bytes(None, None, 4, 100, 10, None) == 7
    cand = _lib.Candidates()
    cand.struct_bytes = C.sizeof(_lib.Candidates)
    args = (None, None, None, None, None, None, None, 0, None, None)
    assert L.nann_search_candidates(None, None, None, 4, 10, None, *args) == 7          # no lists
    assert b"nann_search_candidates" in L.nann_last_error()
    assert L.nann_search_candidates(None, None, None, 4, 10, C.byref(cand), *args) == 7  # no handles
    assert b"null argument" in L.nann_last_error()
    cand.struct_bytes = C.sizeof(_lib.Candidates) + 8
    assert L.nann_search_candidates(None, None, None, 4, 10, C.byref(cand), *args) == 7
    assert b"struct_bytes" in L.nann_last_error()


# ---- the well-formedness rule ------------------------------------------------------------------------------------------
def test_well_formedness_rule_and_disjoint_ranges():
    for name, (splits, n_cand, expect) in SPLIT_CASES.items():
        assert well_formed(splits, n_cand).tolist() == expect, name
        assert well_formed_running_max(splits, n_cand).tolist() == expect, name
    rng = np.random.default_rng(41)
    seen_bad = seen_good = 0
    for _ in range(1000):
        nq = int(rng.integers(1, 12))
        n_cand = int(rng.integers(0, 40))
        kind = rng.integers(0, 3)
        if kind == 0:    # anything
            s = rng.integers(-5, n_cand + 6, nq + 1)
        elif kind == 1:  # sorted, a few entries disturbed
            s = np.sort(rng.integers(0, n_cand + 1, nq + 1))
            for at in rng.integers(0, nq + 1, rng.integers(0, 3)):
                s[at] = rng.integers(-5, n_cand + 6)
        else:            # sorted
            s = np.sort(rng.integers(0, n_cand + 1, nq + 1))
        ok = well_formed(s, n_cand)
        assert (ok == well_formed_running_max(s, n_cand)).all(), s
        seen_bad += int((~ok).sum())
        seen_good += int(ok.sum())
        # accepted ranges are pairwise disjoint, in range, and in query order: one writer per position of the score buffer
        owner = np.full(n_cand, -1)
        end_before = 0
        for i in np.flatnonzero(ok):
            b, e = int(s[i]), int(s[i + 1])
            assert end_before <= b <= e <= n_cand, (s, i)
            assert (owner[b:e] == -1).all(), (s, i)
            owner[b:e] = i
            end_before = e
    assert seen_bad > 500 and seen_good > 500


def test_plan_model_covers_every_accepted_position_once():
    """every position of a well-formed list belongs to exactly one work item of at most C candidates; ill-formed and empty lists
    have none; the number of items stays within n_cand / C + n_queries, the bound the persistent grids are sized by"""
    rng = np.random.default_rng(43)
    cases = [(s, n) for s, n, _ in SPLIT_CASES.values()]
    for c in (1, 4, 7):
        for _ in range(100):
            n_cand = int(rng.integers(0, 60))
            s = np.sort(rng.integers(0, n_cand + 1, int(rng.integers(2, 10))))
            if rng.integers(0, 2):
                s[rng.integers(0, len(s))] = rng.integers(-3, n_cand + 4)
            cases.append((s, n_cand))
        for s, n_cand in cases:
            begin, length, status, items = plan_model(s, n_cand, c)
            ok = well_formed(s, n_cand)
            assert ((status == 0) == ok).all() and (length[~ok] == 0).all()
            assert len(items) <= n_cand // c + len(ok)
            cover = np.zeros(n_cand, int)
            for qi, b, cnt in items:
                assert ok[qi] and 1 <= cnt <= c and begin[qi] <= b and b + cnt <= begin[qi] + length[qi]
                cover[b:b + cnt] += 1
            want = np.zeros(n_cand, int)
            for i in np.flatnonzero(ok):
                want[int(s[i]):int(s[i + 1])] = 1
            assert (cover == want).all(), (s, n_cand, c)


# ---- the semantics the GPU test relies on, on the oracle alone ---------------------------------------------------------
def candidate_topk(oracle, osc, q, embs, rows, k):
    """the expected answer everywhere: oracle.score_rows on the gathered rows, oracle.topk of min(k, len) -> (pos, rows, scores)"""
    rows = np.asarray(rows, np.int64)
    kk = min(k, len(rows))
    if kk == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.float32)
    rc, scores = oracle.score_rows(osc, q, embs[rows])
    assert rc == 0
    rc, ov, oi = oracle.topk(scores, kk)
    assert rc == 0
    return oi, rows[oi], ov


def test_sorted_allow_list_equals_filtered_brute_force(oracle):
    """candidate top-k over the ASCENDING allowed rows = brute force over every row with the denied ones dropped, first k:
    position order in a sorted duplicate-free list is row order, so both break ties the same way"""
    rng = np.random.default_rng(17)
    n, d = 600, 64
    base = rng.standard_normal((n // 3, d)).astype(np.float16)
    embs = np.ascontiguousarray(np.tile(base, (3, 1))[rng.permutation(n)])  # every row three times: ties everywhere
    ix = oracle.Index(embs, np.arange(n, dtype=np.int64) * 7 + 3, [np.zeros(0, np.int32)] * 2, [np.zeros(n + 1, np.int64)] * 2,
                      np.zeros(1, np.int32))
    sc = oracle.Scorer("l2", d, oracle.EMB_F16)
    for trial in range(6):
        q = embs[int(rng.integers(0, n))].astype(np.float32)
        allowed = np.sort(rng.choice(n, int(rng.integers(1, n)), replace=False))
        rc, bi, bv = oracle.brute_force(ix, sc, q, n)
        assert rc == 0
        keep = np.isin(bi, allowed)
        for k in (1, 10, 200):
            pos, rows, scores = candidate_topk(oracle, sc, q, embs, allowed, k)
            kk = min(k, len(allowed))
            assert (rows == bi[keep][:kk]).all() and (scores.view(np.uint32) == bv[keep][:kk].view(np.uint32)).all(), (trial, k)
            assert (allowed[pos] == rows).all()
    # and the order that is NOT guaranteed: a descending list puts the higher of two tied rows first
    q = embs[5].astype(np.float32)
    twins = np.flatnonzero((embs == embs[5]).all(1))
    assert len(twins) == 3
    _, rows, _ = candidate_topk(oracle, sc, q, embs, twins[::-1], 3)
    assert rows.tolist() == twins[::-1].tolist()
