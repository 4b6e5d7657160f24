"""CPU: the group cap and the grouped searches as far as they can be held without a GPU -- the numpy model of the contract
(groupcap_model.model) against its plain Python restatement and the model of the kernel's parallel scheme against the contract
model on 1 000 random cases, the prefix property, by-hand cases, the nine symbols, the header's words, the build lists,
make_groups on the CPU, and every refusal that stands in front of the first launch and so needs no device."""
import ctypes as C
import os
import re
import types

import numpy as np
import torch

import groupcap_model as GM
from nann_amd import _lib, build, retrieval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nann_group_cap_topk", "nann_search_grouped_workspace_bytes", "nann_search_grouped",
           "nann_search_model_grouped_workspace_bytes", "nann_search_model_grouped", "nann_search_all_grouped_workspace_bytes",
           "nann_search_all_grouped", "nann_search_all_model_grouped_workspace_bytes", "nann_search_all_model_grouped")
OK, BAD_ARGUMENT, UNSUPPORTED = 0, 7, 102


def _header():
    return open(os.path.join(ROOT, "include", "nann_hip.h")).read()


# ---- the models against the restatement -----------------------------------------------------------------------------------
def _case(rng):
    """one query: a list of 0 .. 1024 entries over few or many groups, some rows ungrouped, some out of range, some denied,
    n_valid anywhere from negative to beyond k_in, a cap of 1 .. 8 or <= 0"""
    k_in = int(rng.choice([0, 1, 2, 63, 64, 65, 200, 1024])) if rng.random() < 0.3 else int(rng.integers(0, 1025))
    n_items = int(rng.integers(1, 3000))
    n_groups = int(rng.choice([1, 2, 7, 50, 5000]))
    group_of_row = rng.integers(0, n_groups, n_items).astype(np.int32)
    group_of_row[rng.random(n_items) < 0.15] = rng.choice(np.array([-1, -9, -2 ** 31], np.int64)).astype(np.int32)
    if rng.random() < 0.2:
        group_of_row[group_of_row >= 0] *= np.int32((2 ** 31 - 1) // max(n_groups, 1))  # large ids
    rows = rng.integers(0, n_items, k_in).astype(np.int32)
    bad = rng.random(k_in) < 0.05
    rows[bad] = rng.choice(np.array([-1, -7, n_items, n_items + 3, 2 ** 31 - 1, -2 ** 31], np.int64), int(bad.sum())).astype(np.int32)
    n_valid = None if rng.random() < 0.3 else int(rng.integers(-3, k_in + 4))
    cap = int(rng.integers(1, 9)) if rng.random() < 0.85 else int(rng.integers(-2, 1))
    deny = rng.random(n_items) < 0.1 if rng.random() < 0.4 else None
    exclude = rng.integers(-2, n_items + 2, int(rng.integers(0, 40))) if rng.random() < 0.4 else None
    k = int(rng.integers(0, k_in + 1))
    return rows, n_valid, n_items, group_of_row, cap, k, deny, exclude


def test_models_equal_the_restatement_on_1000_cases():
    rng = np.random.default_rng(20241020)
    seen_capped = seen_uncapped = seen_cut = seen_empty = seen_denied = 0
    for _ in range(1000):
        rows, n_valid, n_items, gor, cap, k, deny, exclude = _case(rng)
        scores = rng.standard_normal(len(rows)).astype(np.float32)
        exp = GM.restate(rows.tolist(), n_valid, n_items, gor.tolist(), cap, k, deny, exclude)
        got = GM.model(scores[None], rows[None], None if n_valid is None else [n_valid], n_items, gor, cap, k, deny=deny,
                       exclude=None if exclude is None else [exclude])
        m = int(got["n_out"][0])
        assert m == len(exp)
        assert got["pos"][0, :m].tolist() == [e[0] for e in exp]
        assert got["index"][0, :m].tolist() == [e[1] for e in exp]
        assert got["group"][0, :m].tolist() == [e[2] for e in exp]
        assert (got["scores"][0, :m].view(np.uint32) == scores[[e[0] for e in exp]].view(np.uint32)).all()
        assert not got["index"][0, m:].any() and not got["scores"][0, m:].view(np.uint32).any() and not got["pos"][0, m:].any()
        # the model of the kernel's scheme picks the same positions
        args = (rows, n_valid, n_items, gor, cap, k, deny, exclude)
        assert GM.scheme(*args).tolist() == GM.select(*args).tolist()
        # no group above its cap
        g = got["group"][0, :m]
        if cap > 0 and (g >= 0).any():
            assert np.unique(g[g >= 0], return_counts=True)[1].max() <= cap
        full = len(GM.select(rows, n_valid, n_items, gor, 0, len(rows), deny, exclude))   # the valid entries
        seen_capped += cap > 0 and len(GM.select(*args[:4], cap, len(rows), deny, exclude)) < full
        seen_uncapped += cap <= 0
        seen_cut += m == k and k > 0
        seen_empty += m == 0 and k > 0
        seen_denied += (deny is not None or exclude is not None) and full < len(GM.select(rows, n_valid, n_items, gor, 0, len(rows)))
    assert seen_capped > 300 and seen_uncapped > 50 and seen_cut > 100 and seen_empty > 10 and seen_denied > 200


def test_the_prefix_property_for_every_f():
    rng = np.random.default_rng(7)
    for _ in range(20):
        n_items, k_in = 400, int(rng.integers(1, 300))
        gor = rng.integers(-1, int(rng.choice([1, 5, 60])), n_items).astype(np.int32)
        rows = rng.permutation(n_items)[:k_in].astype(np.int32)
        rows[rng.random(k_in) < 0.05] = -1
        cap = int(rng.integers(1, 4))
        deny = rng.random(n_items) < 0.1
        whole = GM.select(rows, None, n_items, gor, cap, k_in, deny).tolist()
        for f in range(k_in + 1):
            part = GM.select(rows[:f], None, n_items, gor, cap, f, deny).tolist()
            assert part == whole[:len(part)], f
            assert GM.select(rows, f, n_items, gor, cap, k_in, deny).tolist() == part  # n_valid = f cuts the list the same way


def test_by_hand():
    gor = np.array([0, 0, 0, 1, 1, -1, -1, 2], np.int32)       # rows 0-2: group 0; 3-4: group 1; 5-6: ungrouped; 7: group 2
    rows = np.array([[0, 3, 1, 5, 2, 4, 6, 7]], np.int32)
    scores = np.array([[8, 7, 6, np.nan, 4, -np.inf, 2, 1]], np.float32)
    got = GM.model(scores, rows, None, 8, gor, 1, 8)            # cap 1: one per group, the ungrouped all
    assert got["n_out"][0] == 5 and got["index"][0].tolist() == [0, 3, 5, 6, 7, 0, 0, 0]
    assert got["pos"][0].tolist() == [0, 1, 3, 6, 7, 0, 0, 0] and got["group"][0].tolist() == [0, 1, -1, -1, 2, 0, 0, 0]
    assert np.isnan(got["scores"][0, 2])                        # a NaN is carried through
    got = GM.model(scores, rows, None, 8, gor, 2, 3)            # cap 2, k = 3 cuts behind the third kept
    assert got["n_out"][0] == 3 and got["index"][0].tolist() == [0, 3, 1]
    # everything in one group: the first cap entries
    one = np.zeros(8, np.int32)
    assert GM.model(scores, rows, None, 8, one, 3, 8)["index"][0].tolist() == [0, 3, 1, 0, 0, 0, 0, 0]
    # everything ungrouped, or the query uncapped: the input's head
    assert GM.model(scores, rows, None, 8, np.full(8, -4, np.int32), 1, 8)["index"][0].tolist() == rows[0].tolist()
    assert GM.model(scores, rows, None, 8, one, 1, 8, caps=[0])["index"][0].tolist() == rows[0].tolist()
    # a denied row uses no quota: with row 0 denied, row 1 is the first of group 0
    deny = np.zeros(8, bool)
    deny[0] = True
    assert GM.model(scores, rows, None, 8, gor, 1, 8, deny=deny)["index"][0].tolist() == [3, 1, 5, 6, 7, 0, 0, 0]
    assert GM.model(scores, rows, None, 8, gor, 1, 8, exclude=[[0, 3]])["index"][0].tolist() == [1, 5, 4, 6, 7, 0, 0, 0]
    # a row that stands twice counts twice
    twice = np.array([[0, 0, 1]], np.int32)
    assert GM.model(None, twice, None, 8, gor, 2, 3)["index"][0].tolist() == [0, 0, 0] and \
        GM.model(None, twice, None, 8, gor, 2, 3)["n_out"][0] == 2


def test_the_hash_is_the_kernels():
    src = open(os.path.join(build.SRC_DIR, "nann_groupcap.h")).read()
    assert "((uint32_t)g * 2654435761u) >> 21" in src
    assert GM.group_hash(0) == 0 and GM.group_hash(1) == 2654435761 >> 21 and 0 <= GM.group_hash(2 ** 31 - 1) < GM.SLOTS


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_the_nine_symbols_are_declared_exported_and_bound():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = C.CDLL(build.build())
    for s in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % s, code), s
        assert hasattr(lib, s), s
        assert s in _lib.SYMBOLS, s
    assert "#define NANN_ABI_VERSION 6" in _header()
    assert sorted(_lib.SYMBOLS) == sorted(set(re.findall(r"\b(nann_[a-z0-9_]+)\s*\(", code)))
    assert C.sizeof(_lib.Groups) == 32
    for name in ("Groups", "make_groups", "GroupedResult", "cap_groups", "search_grouped", "search_model_grouped",
                 "search_all_grouped", "search_all_model_grouped"):
        assert hasattr(retrieval, name), name


def test_the_header_states_the_contract():
    text = _header()
    section = text[text.index("group caps: at most m rows per group"):text.index("8(f3): the evaluation graph")]
    section = " ".join(section.replace("\n *", " ").split())
    for phrase in ("The reference has no such call",
                   "a negative id means UNGROUPED",
                   "caps[i] <= 0: query i is uncapped",
                   "j < clamp(n_valid[i], 0, k_in)",
                   "malformed input never faults",
                   "its rank among the valid entries of its group is < m",
                   "Denied and invalid entries use no quota",
                   "A row that appears twice counts twice",
                   "NaN and -inf are scores like any other",
                   "PREFIX PROPERTY",
                   "depends only on entries 0 .. j",
                   "n_out == k has the exact answer over the full ranking",
                   "does not depend on the batch",
                   "No workspace",
                   "A failed query gets n_out = 0",
                   "fetch > n_items -> NANN_ERR_TOPK_K_GT_N"):
        assert phrase in section, phrase


def test_the_kernel_rides_in_the_filter_object():
    assert "nann_groupcap.h" in build.DEPS
    assert len(build.UNITS) == 17
    assert '#include "nann_groupcap.h"' in open(os.path.join(build.SRC_DIR, "nann_filter_inst.hip")).read()
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "nann_groupcap.h" in text[text.index("\n## 2. Build"):text.index("\n## 3. ")]


# ---- every refusal that needs no device -----------------------------------------------------------------------------------
def _groups(group_of_row=0x30000, cap=1, caps=0, struct_bytes=None):
    g = _lib.Groups()
    g.struct_bytes = C.sizeof(_lib.Groups) if struct_bytes is None else struct_bytes
    g.group_of_row = group_of_row or None
    g.cap = cap
    g.caps = caps or None
    return g


def _cap(L, n_queries=2, k_in=8, n_items=100, k=5, rows=1, item_ids=0, out_index=2, out_item_ids=0, groups="default", filter=None):
    """nann_group_cap_topk with made-up addresses: nothing is dereferenced by a refused call"""
    p = lambda v: C.c_void_p(0x10000 * v) if v else None
    g = _groups() if groups == "default" else groups
    return L.nann_group_cap_topk(None, p(rows), None, n_queries, k_in, n_items, p(item_ids), C.byref(g) if g is not None else None,
                                 C.byref(filter) if filter is not None else None, k, p(out_index), None, p(out_item_ids), None, None,
                                 None, None)


def test_group_cap_refusals_need_no_device():
    L = _lib.lib()
    who = b"nann_group_cap_topk"
    assert _cap(L, n_queries=-1) == BAD_ARGUMENT and who in L.nann_last_error()
    assert _cap(L, k_in=-1, k=0) == BAD_ARGUMENT
    assert _cap(L, n_items=-1) == BAD_ARGUMENT and b"negative size" in L.nann_last_error()
    assert _cap(L, k=-1) == BAD_ARGUMENT
    assert _cap(L, k=9) == BAD_ARGUMENT and b"k exceeds" in L.nann_last_error() and who in L.nann_last_error()
    assert _cap(L, k_in=1025, k=5) == UNSUPPORTED and b"k_in <= 1024" in L.nann_last_error()
    assert _cap(L, n_queries=2 ** 31) == UNSUPPORTED
    assert _cap(L, n_items=2 ** 31) == UNSUPPORTED
    assert _cap(L, groups=None) == BAD_ARGUMENT and b"null nann_groups" in L.nann_last_error() and who in L.nann_last_error()
    assert _cap(L, groups=_groups(struct_bytes=24)) == BAD_ARGUMENT and b"struct_bytes" in L.nann_last_error()
    assert _cap(L, rows=0, groups=_groups(struct_bytes=0)) == BAD_ARGUMENT and b"null argument" in L.nann_last_error()  # (0 is accepted: the rows are next)
    assert _cap(L, groups=_groups(group_of_row=0)) == BAD_ARGUMENT and b"group_of_row" in L.nann_last_error()
    assert _cap(L, groups=_groups(cap=0)) == BAD_ARGUMENT and b"cap < 1" in L.nann_last_error()
    assert _cap(L, rows=0) == BAD_ARGUMENT and b"null argument" in L.nann_last_error() and who in L.nann_last_error()
    assert _cap(L, out_index=0) == BAD_ARGUMENT
    assert _cap(L, out_item_ids=3) == BAD_ARGUMENT and b"out_item_ids without item_ids" in L.nann_last_error()
    bad = _lib.Filter()
    bad.struct_bytes = 7
    assert _cap(L, filter=bad) == BAD_ARGUMENT and b"nann_filter" in L.nann_last_error()
    # nothing to do: NANN_OK whatever the pointers ...
    assert _cap(L, n_queries=0, rows=0, out_index=0) == OK
    assert _cap(L, k=0, rows=0, out_index=0, out_item_ids=3) == OK
    # ... but the sizes and the groups are looked at in front of it
    assert _cap(L, n_queries=0, groups=None) == BAD_ARGUMENT
    assert _cap(L, k=0, groups=_groups(cap=-3)) == BAD_ARGUMENT
    assert _cap(L, k=9, rows=0, groups=None) == BAD_ARGUMENT and b"k exceeds" in L.nann_last_error()
    assert _cap(L, k_in=2000, k=5, groups=None) == UNSUPPORTED


def test_null_handles_of_the_search_forms_are_bad_arguments_without_a_gpu():
    L = _lib.lib()
    nb = C.c_int64(-1)
    t = (C.c_int32 * 6)(8, 16, 32, 32, 32, 50)
    g = _groups()
    assert L.nann_search_grouped_workspace_bytes(None, t, 3, C.byref(nb)) == BAD_ARGUMENT
    assert L.nann_search_model_grouped_workspace_bytes(None, None, t, 3, C.byref(nb)) == BAD_ARGUMENT
    assert L.nann_search_all_grouped_workspace_bytes(None, None, 3, 10, C.byref(nb)) == BAD_ARGUMENT
    assert L.nann_search_all_model_grouped_workspace_bytes(None, None, 3, 10, C.byref(nb)) == BAD_ARGUMENT
    assert nb.value == -1
    assert L.nann_search_grouped(None, None, None, 3, t, None, None, 0, None, None, None, None, None, None, None, None, None,
                                 C.byref(g), 10, None, None, None) == BAD_ARGUMENT
    assert b"nann_search_grouped" in L.nann_last_error()
    assert L.nann_search_model_grouped(None, None, None, 3, t, None, None, 0, None, None, None, None, None, None, None, None,
                                       C.byref(g), 10, None, None, None) == BAD_ARGUMENT
    assert b"nann_search_model_grouped" in L.nann_last_error()
    assert L.nann_search_all_grouped(None, None, None, 3, 20, 10, None, None, None, None, None, 0, None, None, C.byref(g), None,
                                     None) == BAD_ARGUMENT
    assert b"nann_search_all_grouped" in L.nann_last_error()
    assert L.nann_search_all_model_grouped(None, None, None, 3, 20, 10, None, None, None, None, None, 0, None, None, C.byref(g),
                                           None, None) == BAD_ARGUMENT
    assert b"nann_search_all_model_grouped" in L.nann_last_error()


# ---- make_groups without a GPU ----------------------------------------------------------------------------------------------
def _index(n, item_ids=None):
    ids = np.arange(n, dtype=np.int64) * 7 + 3 if item_ids is None else item_ids
    return types.SimpleNamespace(n_items=n, item_ids=torch.as_tensor(ids), device=torch.device("cpu"))


def test_make_groups_on_the_cpu():
    ix = _index(10)
    g = retrieval.make_groups(ix, group_of_row=[0, 1, 2, -1, 4, 5, -7, 2 ** 31 - 1, 8, 9], cap=3, device="cpu")
    assert g.group_of_row.dtype == torch.int32 and g.group_of_row.tolist() == [0, 1, 2, -1, 4, 5, -7, 2 ** 31 - 1, 8, 9]
    assert g.cap == 3 and g.caps is None and g.n_queries is None and g.n_items == 10
    assert g.struct.struct_bytes == C.sizeof(_lib.Groups) and g.struct.group_of_row == g.group_of_row.data_ptr()
    assert g.struct.cap == 3 and not g.struct.caps
    # item ids through a shuffled table: unnamed items are ungrouped, an unknown id names nothing
    ids = np.random.default_rng(3).permutation(10).astype(np.int64) * 13 + 5
    ix = _index(10, ids)
    g = retrieval.make_groups(ix, group_of_item_id=(ids[[4, 0, 7]].tolist() + [999], [40, 0, 70, 5]), caps=[2, 0, -1, 5], device="cpu")
    exp = np.full(10, -1)
    exp[[4, 0, 7]] = [40, 0, 70]
    assert g.group_of_row.tolist() == exp.tolist()
    assert g.caps.dtype == torch.int32 and g.caps.tolist() == [2, 0, -1, 5] and g.n_queries == 4
    assert g.struct.caps == g.caps.data_ptr()
    for bad in (dict(), dict(group_of_row=[0] * 10, group_of_item_id=([], [])), dict(group_of_row=[0] * 9),
                dict(group_of_row=[0] * 10, cap=0)):
        try:
            retrieval.make_groups(ix, device="cpu", **bad)
        except AssertionError:
            continue
        raise AssertionError(bad)
