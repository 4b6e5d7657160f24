"""CPU: the attribute predicates (nann_predicates; include/nann_hip.h, csrc/nann_predicate.h).  The numpy model the device tests
compare against (predicate_model) held to a plain per-entry restatement on random cases; the ABI -- ten symbols, the header's
words, the build; every refusal of the C calls that needs no device; make_attributes / make_predicates on the CPU."""
import ctypes as C
import os
import re
import types

import numpy as np
import torch

import predicate_model as PM
from nann_amd import _lib, build, retrieval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARGUMENT, UNSUPPORTED = 0, 7, 102
SYMBOLS = ["nann_predicate_topk", "nann_predicate_count", "nann_search_where_workspace_bytes", "nann_search_where",
           "nann_search_model_where_workspace_bytes", "nann_search_model_where", "nann_search_all_where_workspace_bytes",
           "nann_search_all_where", "nann_search_all_model_where_workspace_bytes", "nann_search_all_model_where"]


def _header():
    return open(os.path.join(ROOT, "include", "nann_hip.h")).read()


# ---- the model against its restatement ------------------------------------------------------------------------------------
def _case(rng, c):
    """one random case: a predicate set over n_items rows and n_q queries, a filter, ranked lists.  The subset of the three
    tests goes by c % 8, so that every subset comes up; the oddities by the further digits of c."""
    n_items = int(rng.choice([1, 5, 40, 200]))
    n_q = int(rng.integers(1, 5))
    tests = c % 8
    pred = {}
    if tests & 1:
        pred["label_of_row"] = rng.integers(-3, 12, n_items).astype(np.int32)
        if c % 5 == 0:
            pred["label_of_row"][rng.integers(0, n_items)] = np.iinfo(np.int32).min
        lists = []
        for i in range(n_q):
            kind = (c // 8 + i) % 6
            if kind == 0:
                lists.append(np.zeros(0, np.int32))                                    # empty: no label test
            elif kind == 1:
                lists.append(np.tile(rng.integers(-3, 12, 150), 4).astype(np.int32))  # 600 entries, with duplicates
            elif kind == 2:
                lists.append(np.array([np.iinfo(np.int32).min, 3, 3], np.int32))
            else:
                lists.append(rng.integers(-3, 12, int(rng.integers(1, 9))).astype(np.int32))
        splits = np.concatenate(([0], np.cumsum([len(l) for l in lists]))).astype(np.int64)
        labels = np.concatenate(lists).astype(np.int32)
        odd = (c // 48) % 4
        if odd == 1:
            splits[rng.integers(0, n_q + 1)] = -5                                      # below 0: clamped
        elif odd == 2:
            splits[rng.integers(0, n_q + 1)] = len(labels) + 7                         # beyond n_labels: clamped, or inverted
        elif odd == 3 and n_q > 1:
            splits[1], splits[2 if n_q > 1 else 1] = splits[2 if n_q > 1 else 1], splits[1]   # inverted
        pred["label_splits"], pred["labels"] = splits, labels
    if tests & 2:
        v = rng.standard_normal(n_items).astype(np.float32)
        v[rng.random(n_items) < 0.1] = np.nan
        v[rng.random(n_items) < 0.05] = np.inf
        pred["value_of_row"] = v
        lo = rng.standard_normal(n_q).astype(np.float32) - 0.5
        hi = lo + rng.random(n_q).astype(np.float32) * 2
        if c % 3 == 0:
            hi[0] = lo[0] - 1                                                          # lo > hi: nothing
        if c % 7 == 0:
            lo[-1] = np.nan
        if c % 11 == 0:
            hi[0] = np.nan
        side = (c // 8) % 3
        if side != 1:
            pred["value_lo"] = lo
        if side != 2:
            pred["value_hi"] = hi
    if tests & 4:
        t = rng.integers(0, 2 ** 63, n_items, dtype=np.uint64) & rng.integers(0, 2 ** 63, n_items, dtype=np.uint64)
        t[rng.random(n_items) < 0.5] |= np.uint64(1) << np.uint64(63)                 # tag bit 63
        pred["tags_of_row"] = t
        words = {"tags_all": np.array([(1 << 63) if i % 2 else (1 << int(rng.integers(0, 63))) for i in range(n_q)], np.uint64),
                 "tags_any": np.array([0 if i % 3 == 0 else (1 << 63) | 6 for i in range(n_q)], np.uint64),
                 "tags_none": np.array([(1 << int(rng.integers(0, 64))) for _ in range(n_q)], np.uint64)}
        keep = (c // 8) % 7 + 1
        for bit, name in enumerate(words):
            if keep >> bit & 1:
                pred[name] = words[name]
    deny = rng.random(n_items) < 0.2 if c % 2 else None
    exclude = [rng.integers(-2, n_items + 2, int(rng.integers(0, 6))) for _ in range(n_q)] if c % 4 >= 2 else None
    k_in = int(rng.choice([1, 7, 64, 130]))
    rows = rng.integers(-2, n_items + 2, (n_q, k_in)).astype(np.int32)                 # out-of-range rows in the list, repeats
    n_valid = [None, np.zeros(n_q, np.int32), rng.integers(-1, k_in + 3, n_q).astype(np.int32), np.full(n_q, k_in, np.int32)][c % 4]
    return n_items, n_q, pred or None, (deny, exclude), rows, n_valid, int(rng.integers(0, k_in + 1))


def test_the_model_equals_the_restatement_on_1200_cases():
    rng = np.random.default_rng(2024)
    seen = set()
    for c in range(1200):
        n_items, n_q, pred, flt, rows, n_valid, k = _case(rng, c)
        seen.add(c % 8)
        scores = rng.standard_normal(rows.shape).astype(np.float32)
        got = PM.where_topk(rows, scores, n_valid, flt, pred, k, n_items)
        cnt = PM.count(pred, flt, n_q, n_items)
        for i in range(n_q):
            exp = PM.restate_topk(rows[i], None if n_valid is None else n_valid[i], flt, pred, k, n_items, i)
            m = got["n_out"][i]
            assert m == len(exp), (c, i)
            assert got["pos"][i, :m].tolist() == [p for p, _ in exp] and got["index"][i, :m].tolist() == [r for _, r in exp], (c, i)
            assert (got["scores"][i, :m] == scores[i, got["pos"][i, :m]]).all()
            assert not got["index"][i, m:].any() and not got["scores"][i, m:].any() and not got["pos"][i, m:].any()
            every = [r for r in range(n_items) if PM.restate_topk([r], None, flt, pred, 1, n_items, i)]
            assert cnt[i] == len(every), (c, i)
            assert PM.passes(pred, i, np.arange(n_items)).tolist() == [PM.restate_passes(pred, i, r) for r in range(n_items)], (c, i)
    assert seen == set(range(8))


def test_by_hand():
    pred = {"label_of_row": np.array([7, 12, 3, 7], np.int32), "value_of_row": np.array([1.0, np.nan, 5.0, 9.0], np.float32),
            "tags_of_row": np.array([0b011, 0b111, (1 << 63) | 1, 0], np.uint64),
            "label_splits": np.array([0, 2, 2, 3], np.int64), "labels": np.array([12, 7, 3], np.int32),
            "value_lo": np.array([0.0, 2.0, 6.0], np.float32), "value_hi": np.array([10.0, 9.0, 5.0], np.float32),
            "tags_none": np.array([0b100, 0, 0], np.uint64)}
    rows = np.arange(4)
    assert PM.passes(pred, 0, rows).tolist() == [True, False, False, True]       # 7 or 12, in [0, 10], not tag 2; row 1: its value is NaN
    pred["tags_none"][0] = 0b001
    assert PM.passes(pred, 0, rows).tolist() == [False, False, False, True]      # row 0 carries tag 0
    pred["tags_none"][0] = 0
    assert PM.passes(pred, 1, rows).tolist() == [False, False, True, True]       # an empty label range: no label test
    assert PM.passes(pred, 2, rows).tolist() == [False, False, False, False]     # lo > hi
    assert PM.count(pred, (np.array([False, False, False, True]), None), 3, 4).tolist() == [1, 1, 0]


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_the_ten_symbols_are_declared_exported_and_bound():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = C.CDLL(build.build())
    assert len(SYMBOLS) == 10
    for s in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % s, code), s
        assert hasattr(lib, s), s
        assert s in _lib.SYMBOLS, s
    assert "#define NANN_ABI_VERSION 6" in _header()
    assert sorted(_lib.SYMBOLS) == sorted(set(re.findall(r"\b(nann_[a-z0-9_]+)\s*\(", code)))
    assert C.sizeof(_lib.Predicates) == 96
    for name in ("Attributes", "make_attributes", "Predicates", "make_predicates", "predicate_topk", "predicate_count",
                 "search_where", "search_model_where", "search_all_where", "search_all_model_where"):
        assert hasattr(retrieval, name), name


def test_the_kernels_ride_in_the_filter_object():
    assert "nann_predicate.h" in build.DEPS
    assert len(build.UNITS) == 17
    inst = open(os.path.join(build.SRC_DIR, "nann_filter_inst.hip")).read()
    assert '#include "nann_predicate.h"' in inst
    src = open(os.path.join(build.SRC_DIR, "nann_predicate.h")).read()
    for kernel in ("k_pred_scatter", "k_pred_compact", "k_pred_count"):
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, src), kernel
    assert re.search(r"constexpr int kPredTileRows = \d+;", src)
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "nann_predicate.h" in text[text.index("\n## 2. Build"):text.index("\n## 3. ")]


def test_the_header_states_the_contract():
    text = _header()
    section = text[text.index("attribute predicates: per-query label, range and tag conditions"):text.index("8(f3): the evaluation graph")]
    section = " ".join(section.replace("\n *", " ").split())
    for phrase in ("The reference has no such feature",
                   "BORROWED for the call",
                   "any order, duplicates allowed, any number",
                   "The range is clamped to [0, n_labels]",
                   "an empty or inverted range means NO label test",
                   "value_lo[i] <= value_of_row[r] <= value_hi[i], compared as IEEE does",
                   "a NaN row value or a NaN bound passes nothing",
                   "a NULL side is unbounded",
                   "lo > hi is how a caller says \"match nothing\"",
                   "(t & all) == all, any == 0 || (t & any) != 0, and (t & none) == 0",
                   "ANDed with each other and with the nann_filter",
                   "0 or sizeof(nann_predicates)",
                   "a per-query condition without its attribute column",
                   "n_labels < 0",
                   "label_splits without labels while n_labels > 0",
                   "in front of the first launch and none touches the device",
                   "Malformed device contents never fault",
                   "the arguments of nann_group_cap_topk without the groups",
                   "handed on to nann_group_cap_topk through n_valid",
                   "SELECTIVITY",
                   "the same fetch-width contract",
                   "the first k passing entries of what the unchanged traversal returns at F",
                   "The workspace is that of the filtered call",
                   "n_out[i] < k means the list was cut short: widen F",
                   "The top k over the PASSING rows is exact",
                   "n_out[i] = min(k, passing rows of query i) wherever the passing rows score above -inf",
                   "bit-identical to nann_search_all for the same (query, row)",
                   "a query's answer does not depend on its batch"):
        assert phrase in section, phrase


# ---- every refusal that needs no device -----------------------------------------------------------------------------------
def _preds(struct_bytes=None, **fields):
    """a nann_predicates with made-up addresses (v * 0x10000): nothing is dereferenced by a refused call"""
    p = _lib.Predicates()
    p.struct_bytes = C.sizeof(_lib.Predicates) if struct_bytes is None else struct_bytes
    for name, v in fields.items():
        setattr(p, name, v if name == "n_labels" else (0x10000 * v or None))
    return p


BAD_STRUCTS = [(dict(struct_bytes=95), b"struct_bytes"),
               (dict(label_splits=1, labels=2, n_labels=4), b"label_splits without label_of_row"),
               (dict(value_of_row=1, label_splits=1, labels=2, n_labels=4), b"label_splits without label_of_row"),
               (dict(value_lo=1), b"without value_of_row"),
               (dict(value_hi=1, label_of_row=2), b"without value_of_row"),
               (dict(tags_all=1), b"without tags_of_row"),
               (dict(tags_any=1, value_of_row=3), b"without tags_of_row"),
               (dict(tags_none=1), b"without tags_of_row"),
               (dict(label_of_row=1, n_labels=-1), b"n_labels < 0"),
               (dict(label_of_row=1, label_splits=2, n_labels=3), b"label_splits without labels")]


def _topk(L, n_queries=2, k_in=8, n_items=100, k=5, rows=1, item_ids=0, out_index=2, out_item_ids=0, preds=None, filter=None):
    p = lambda v: C.c_void_p(0x10000 * v) if v else None
    return L.nann_predicate_topk(None, p(rows), None, n_queries, k_in, n_items, p(item_ids),
                                 C.byref(preds) if preds is not None else None, C.byref(filter) if filter is not None else None, k,
                                 p(out_index), None, p(out_item_ids), None, None, None)


def test_predicate_topk_and_count_refusals_need_no_device():
    L = _lib.lib()
    who = b"nann_predicate_topk"
    assert _topk(L, n_queries=-1) == BAD_ARGUMENT and who in L.nann_last_error()
    assert _topk(L, k_in=-1, k=0) == BAD_ARGUMENT
    assert _topk(L, n_items=-1) == BAD_ARGUMENT and b"negative size" in L.nann_last_error()
    assert _topk(L, k=-1) == BAD_ARGUMENT
    assert _topk(L, k=9) == BAD_ARGUMENT and b"k exceeds" in L.nann_last_error()
    assert _topk(L, k_in=1025, k=5) == UNSUPPORTED and b"k_in <= 1024" in L.nann_last_error()
    assert _topk(L, n_queries=2 ** 31) == UNSUPPORTED
    assert _topk(L, n_items=2 ** 31) == UNSUPPORTED
    for fields, words in BAD_STRUCTS:
        assert _topk(L, preds=_preds(**fields)) == BAD_ARGUMENT and words in L.nann_last_error(), fields
        assert _topk(L, n_queries=0, preds=_preds(**fields)) == BAD_ARGUMENT, fields      # in front of the early NANN_OK
        assert L.nann_predicate_count(100, C.byref(_preds(**fields)), None, 2, C.c_void_p(0x10000), None) == BAD_ARGUMENT
        assert words in L.nann_last_error(), fields
    assert _topk(L, rows=0, preds=_preds(struct_bytes=0)) == BAD_ARGUMENT and b"null argument" in L.nann_last_error()  # (0 is accepted)
    assert _topk(L, rows=0) == BAD_ARGUMENT and b"null argument" in L.nann_last_error() and who in L.nann_last_error()
    assert _topk(L, out_index=0) == BAD_ARGUMENT
    assert _topk(L, out_item_ids=3) == BAD_ARGUMENT and b"out_item_ids without item_ids" in L.nann_last_error()
    bad = _lib.Filter()
    bad.struct_bytes = 7
    assert _topk(L, filter=bad) == BAD_ARGUMENT and b"nann_filter" in L.nann_last_error()
    assert _topk(L, n_queries=0, rows=0, out_index=0) == OK
    assert _topk(L, k=0, rows=0, out_index=0, out_item_ids=3) == OK
    # the count
    who = b"nann_predicate_count"
    assert L.nann_predicate_count(-1, None, None, 2, C.c_void_p(0x10000), None) == BAD_ARGUMENT and who in L.nann_last_error()
    assert L.nann_predicate_count(100, None, None, -2, C.c_void_p(0x10000), None) == BAD_ARGUMENT
    assert L.nann_predicate_count(2 ** 31, None, None, 2, C.c_void_p(0x10000), None) == UNSUPPORTED
    assert L.nann_predicate_count(100, None, C.byref(bad), 2, C.c_void_p(0x10000), None) == BAD_ARGUMENT
    assert L.nann_predicate_count(100, None, None, 2, None, None) == BAD_ARGUMENT and b"null argument" in L.nann_last_error()
    assert L.nann_predicate_count(100, None, None, 0, None, None) == OK


def test_the_search_forms_refuse_a_malformed_struct_in_front_of_everything():
    """... their handles included: the predicates are looked at first, so the refusal needs neither an index nor a device"""
    L = _lib.lib()
    t = (C.c_int32 * 6)(8, 16, 32, 32, 32, 50)
    nb = C.c_int64(-1)
    assert L.nann_search_where_workspace_bytes(None, t, 3, C.byref(nb)) == BAD_ARGUMENT
    assert L.nann_search_model_where_workspace_bytes(None, None, t, 3, C.byref(nb)) == BAD_ARGUMENT
    assert L.nann_search_all_where_workspace_bytes(None, None, 3, 10, C.byref(nb)) == BAD_ARGUMENT
    assert L.nann_search_all_model_where_workspace_bytes(None, None, 3, 10, C.byref(nb)) == BAD_ARGUMENT
    assert nb.value == -1
    for fields, words in BAD_STRUCTS:
        p = _preds(**fields)
        assert L.nann_search_all_where(None, None, None, 3, 10, None, None, None, None, 0, None, None, C.byref(p), None,
                                       None) == BAD_ARGUMENT and words in L.nann_last_error(), fields
        assert L.nann_search_all_model_where(None, None, None, 3, 10, None, None, None, None, 0, None, None, C.byref(p), None,
                                             None) == BAD_ARGUMENT and words in L.nann_last_error(), fields
        for n_queries in (3, 0):                                                           # ... and in front of an empty batch's NANN_OK
            assert L.nann_search_where(None, None, None, n_queries, t, None, None, 0, None, None, None, None, None, None, None, None,
                                       None, C.byref(p), 10, None, None) == BAD_ARGUMENT and words in L.nann_last_error(), fields
            assert L.nann_search_model_where(None, None, None, n_queries, t, None, None, 0, None, None, None, None, None, None, None,
                                             None, C.byref(p), 10, None, None) == BAD_ARGUMENT and words in L.nann_last_error(), fields
            assert L.nann_search_all_where(None, None, None, n_queries, 10, None, None, None, None, 0, None, None, C.byref(p), None,
                                           None) == BAD_ARGUMENT and words in L.nann_last_error(), fields
    ok = _preds(label_of_row=1)
    assert L.nann_search_all_where(None, None, None, 3, 10, None, None, None, None, 0, None, None, C.byref(ok), None,
                                   None) == BAD_ARGUMENT and b"nann_search_all" in L.nann_last_error()
    assert L.nann_search_where(None, None, None, 3, t, None, None, 0, None, None, None, None, None, None, None, None, None,
                               C.byref(ok), 10, None, None) == BAD_ARGUMENT and b"nann_search_where" in L.nann_last_error()
    assert L.nann_search_model_where(None, None, None, 3, t, None, None, 0, None, None, None, None, None, None, None, None,
                                     C.byref(ok), 10, None, None) == BAD_ARGUMENT and b"nann_search_model_where" in L.nann_last_error()


# ---- make_attributes / make_predicates without a GPU ------------------------------------------------------------------------
def _index(n, item_ids=None):
    ids = np.arange(n, dtype=np.int64) * 7 + 3 if item_ids is None else item_ids
    return types.SimpleNamespace(n_items=n, item_ids=torch.as_tensor(ids), device=torch.device("cpu"))


def test_make_attributes_and_make_predicates_on_the_cpu():
    ix = _index(6)
    tags = np.array([1, 2, (1 << 63) | 5, 0, 2 ** 64 - 1, 8], np.uint64)
    at = retrieval.make_attributes(ix, label_of_row=[7, 12, -1, 7, 3, -2 ** 31], value_of_row=[1.5, float("nan"), 3, 4, 5, 6],
                                   tags_of_row=tags, device="cpu")
    assert at.label_of_row.dtype == torch.int32 and at.label_of_row.tolist() == [7, 12, -1, 7, 3, -2 ** 31]
    assert at.value_of_row.dtype == torch.float32 and at.value_of_row[0] == 1.5 and torch.isnan(at.value_of_row[1])
    assert at.tags_of_row.dtype == torch.int64 and (at.tags_of_row.numpy().view(np.uint64) == tags).all()
    assert at.n_items == 6
    p = retrieval.make_predicates(at, 3, label_in=[[12, 7], [], [3, 3, 9]], value_range=(None, [10.0, 2.0, float("nan")]),
                                  tags_all=1 << 63, tags_none=[0, 4, 2 ** 64 - 1])
    assert p.label_splits.dtype == torch.int64 and p.label_splits.tolist() == [0, 2, 2, 5]
    assert p.labels.dtype == torch.int32 and p.labels.tolist() == [12, 7, 3, 3, 9]
    assert p.value_lo is None and p.value_hi.dtype == torch.float32 and p.value_hi.tolist()[:2] == [10.0, 2.0]
    assert p.tags_all.numpy().view(np.uint64).tolist() == [1 << 63] * 3 and p.tags_any is None
    assert p.tags_none.numpy().view(np.uint64).tolist() == [0, 4, 2 ** 64 - 1]
    s = p.struct
    assert s.struct_bytes == C.sizeof(_lib.Predicates) and p.n_queries == 3 and p.n_items == 6
    assert (s.label_of_row, s.value_of_row, s.tags_of_row) == (at.label_of_row.data_ptr(), at.value_of_row.data_ptr(), at.tags_of_row.data_ptr())
    assert s.label_splits == p.label_splits.data_ptr() and s.labels == p.labels.data_ptr() and s.n_labels == 5
    assert not s.value_lo and s.value_hi == p.value_hi.data_ptr()
    assert s.tags_all == p.tags_all.data_ptr() and not s.tags_any and s.tags_none == p.tags_none.data_ptr()
    # the struct, read as the model reads it, gives the model's answer
    pred = {"label_of_row": at.label_of_row.numpy(), "value_of_row": at.value_of_row.numpy(), "tags_of_row": tags,
            "label_splits": p.label_splits.numpy(), "labels": p.labels.numpy(), "value_hi": p.value_hi.numpy(),
            "tags_all": p.tags_all.numpy().view(np.uint64), "tags_none": p.tags_none.numpy().view(np.uint64)}
    assert PM.count(pred, None, 3, 6).tolist() == [0, 0, 0]
    pred["tags_all"] = np.zeros(3, np.uint64)
    assert PM.count(pred, None, 3, 6).tolist() == [2, 1, 0]
    # no condition at all: every pointer of the per-query side stays null
    e = retrieval.make_predicates(at, 2).struct
    assert not (e.label_splits or e.labels or e.value_lo or e.value_hi or e.tags_all or e.tags_any or e.tags_none) and e.n_labels == 0
    # item ids through a shuffled table: an unnamed item gets label -1, value NaN and no tag; an unknown id names nothing
    ids = np.random.default_rng(3).permutation(6).astype(np.int64) * 13 + 5
    ix = _index(6, ids)
    at = retrieval.make_attributes(ix, label_of_item_id=(ids[[4, 0]].tolist() + [999], [40, 0, 5]),
                                   value_of_item_id=(ids[[1]], [2.5]), tags_of_item_id=(ids[[2, 3]], [1 << 63, 3]), device="cpu")
    exp = np.full(6, -1)
    exp[[4, 0]] = [40, 0]
    assert at.label_of_row.tolist() == exp.tolist()
    assert at.value_of_row[1] == 2.5 and torch.isnan(at.value_of_row[[0, 2, 3, 4, 5]]).all()
    assert at.tags_of_row.numpy().view(np.uint64).tolist() == [0, 0, 1 << 63, 3, 0, 0]
    only = retrieval.make_attributes(ix, value_of_row=np.zeros(6), device="cpu")
    assert only.label_of_row is None and only.tags_of_row is None
    for bad in (lambda: retrieval.make_attributes(ix, label_of_row=[0] * 5, device="cpu"),
                lambda: retrieval.make_attributes(ix, label_of_row=[0] * 6, label_of_item_id=([], []), device="cpu"),
                lambda: retrieval.make_predicates(only, 2, label_in=[[1], [2]]),
                lambda: retrieval.make_predicates(only, 2, tags_any=1),
                lambda: retrieval.make_predicates(at, 2, label_in=[[1]]),
                lambda: retrieval.make_predicates(at, 2, value_range=([1.0], None))):
        try:
            bad()
        except AssertionError:
            continue
        raise AssertionError("accepted")
