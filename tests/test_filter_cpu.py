"""CPU: the host side of filtered retrieval (retrieval.make_filter / pool_width, the filter= and k= arguments of search).
make_filter(device="cpu") builds the tensors a nann_filter points at without a GPU: row r of the deny bitmap is bit (r & 31)
of word (r >> 5), exclusion lists are CSR over the batch.  The index here is a stand-in that carries what make_filter reads:
n_items, item_ids, device."""
import contextlib
import ctypes as C
import types

import numpy as np
import torch

from nann_amd import _lib, retrieval


def _index(n, item_ids=None):
    ids = np.arange(n, dtype=np.int64) * 7 + 3 if item_ids is None else item_ids
    return types.SimpleNamespace(n_items=n, item_ids=torch.as_tensor(ids), device=torch.device("cpu"))


def _words(f):
    return f.deny_bits.numpy().view(np.uint32)


def test_bit_r_and_31_of_word_r_shr_5():
    ix = _index(4096)
    rows = [0, 1, 31, 32, 63, 64, 1000, 4095]
    f = retrieval.make_filter(ix, deny_rows=rows, device="cpu")
    w = _words(f)
    assert f.deny_bits.dtype == torch.int32 and w.shape == (128,)
    exp = np.zeros(128, np.uint32)
    for r in rows:
        exp[r >> 5] |= np.uint32(1) << np.uint32(r & 31)
    assert (w == exp).all()
    assert w[0] == 0x80000003 and w[1] == 0x80000001 and w[2] == 1 and w[127] == 0x80000000
    # every row through the same rule, from a seeded mask; duplicates and out-of-range rows change nothing
    mask = np.random.default_rng(5).random(4096) < 0.3
    rows = np.nonzero(mask)[0]
    f = retrieval.make_filter(ix, deny_rows=np.concatenate([rows, rows[:10], [-1, 4096, 1 << 40]]), device="cpu")
    got = (_words(f)[np.arange(4096) >> 5] >> (np.arange(4096) & 31).astype(np.uint32)) & 1
    assert (got.astype(bool) == mask).all()
    assert f.row_splits is None and f.rows is None and f.n_queries is None
    assert f.struct.struct_bytes == C.sizeof(_lib.Filter) and f.struct.deny_bits == f.deny_bits.data_ptr()
    assert not f.struct.excl_row_splits and not f.struct.excl_rows and f.struct.n_excl == 0


def test_tail_word_of_1000_rows():
    ix = _index(1000)
    f = retrieval.make_filter(ix, deny_rows=np.arange(1000), device="cpu")
    w = _words(f)
    assert w.shape == (32,)                      # ceil(1000 / 32)
    assert (w[:31] == 0xFFFFFFFF).all()
    assert w[31] == (1 << (1000 - 31 * 32)) - 1  # rows 992..999: eight bits, nothing at or beyond row 1000
    f = retrieval.make_filter(ix, deny_rows=[999, 1000, 1023], device="cpu")
    assert _words(f)[31] == 1 << (999 & 31) and not _words(f)[:31].any()


def test_item_ids_map_to_rows_through_a_shuffled_table():
    rng = np.random.default_rng(11)
    n = 1000
    ids = rng.permutation(n).astype(np.int64) * 13 + 5       # row r carries item id ids[r]
    ix = _index(n, ids)
    want = [4, 17, 999, 500]
    f = retrieval.make_filter(ix, deny_item_ids=np.concatenate([ids[want], [6, -3, 10 ** 12]]), device="cpu")  # unknown ids
    exp = np.zeros(32, np.uint32)
    for r in want:
        exp[r >> 5] |= np.uint32(1) << np.uint32(r & 31)
    assert (_words(f) == exp).all()
    assert ix._sorted_ids[0].tolist() == sorted(ids.tolist())  # built once, kept on the index
    cached = ix._sorted_ids
    f = retrieval.make_filter(ix, exclude_item_ids=[ids[[3, 2]], [6], ids[[999]]], deny_rows=[1], device="cpu")
    assert ix._sorted_ids is cached
    assert f.row_splits.tolist() == [0, 2, 2, 3] and f.rows.tolist() == [3, 2, 999]
    assert _words(f)[0] == 2


def test_csr_splits_with_an_empty_list():
    ix = _index(100)
    lists = [np.array([5, 3, 5]), np.array([], dtype=np.int64), torch.tensor([99]), [-1, 100, 2 ** 31 - 1]]
    f = retrieval.make_filter(ix, exclude_rows=lists, device="cpu")
    assert f.row_splits.dtype == torch.int64 and f.row_splits.tolist() == [0, 3, 3, 4, 7]
    assert f.rows.dtype == torch.int32 and f.rows.tolist() == [5, 3, 5, 99, -1, 100, 2 ** 31 - 1]  # order, duplicates, junk kept
    assert f.n_queries == 4 and f.deny_bits is None
    assert f.struct.n_excl == 7 and f.struct.excl_rows == f.rows.data_ptr() and f.struct.excl_row_splits == f.row_splits.data_ptr()
    assert not f.struct.deny_bits
    # rows and item ids together: the union per query
    f = retrieval.make_filter(ix, exclude_rows=[[1], []], exclude_item_ids=[[3 + 7 * 8], [3]], device="cpu")
    assert f.row_splits.tolist() == [0, 2, 3] and f.rows.tolist() == [1, 8, 0]
    # every list empty: splits of zeros, no rows to point at
    f = retrieval.make_filter(ix, exclude_rows=[[], []], device="cpu")
    assert f.row_splits.tolist() == [0, 0, 0] and f.struct.n_excl == 0 and not f.struct.excl_rows


def test_pool_width():
    assert retrieval.pool_width([64, 64, 64, 64, 64, 256]) == 256
    assert retrieval.pool_width([128] * 5 + [200]) == 512
    assert retrieval.pool_width([7, 1, 2, 3, 4, 5]) == 10        # level_topn[0] and [5] take no part
    assert retrieval.pool_width([400] * 6) == 1024               # a list holds at most 1024 entries
    assert retrieval.pool_width(np.array([64, 100, 200, 300, 424, 9], np.int32)) == 1024


class _RecordingLib:
    """stands in for the ctypes library: records the symbols looked up, every call answers NANN_OK"""

    def __init__(self):
        self.looked_up = []

    def __getattr__(self, name):
        self.looked_up.append(name)
        return lambda *a: 0


def _search_on_the_stand_in(monkeypatch, **kw):
    rec = _RecordingLib()
    monkeypatch.setattr(retrieval, "lib", lambda: rec)
    monkeypatch.setattr(retrieval, "_stream", lambda: C.c_void_p(0))
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    ix = _index(100)
    ix.handle = C.c_void_p(0)
    ix.workspace = lambda t, b: torch.empty(1, dtype=torch.uint8)
    scorer = types.SimpleNamespace(handle=C.c_void_p(0))
    r = retrieval.search(ix, scorer, torch.zeros((3, 8)), [4, 4, 4, 4, 4, 8], **kw)
    return ix, rec, r


def test_search_without_a_filter_takes_the_unfiltered_path(monkeypatch):
    _, rec, r = _search_on_the_stand_in(monkeypatch, filter=None)
    assert rec.looked_up == ["nann_search_opt"]
    assert not any("filtered" in s for s in rec.looked_up)
    assert r.n_out is None and r.item_ids.shape == (3, 8)


def test_search_with_a_filter_or_a_k_takes_the_filtered_path(monkeypatch):
    ix, rec, r = _search_on_the_stand_in(monkeypatch, k=5)
    assert rec.looked_up == ["nann_search_filtered_workspace_bytes", "nann_search_filtered"]
    assert r.item_ids.shape == (3, 5) and r.n_out.shape == (3,)
    f = retrieval.make_filter(ix, deny_rows=[1], exclude_rows=[[2], [], [3]], device="cpu")
    _, rec, r = _search_on_the_stand_in(monkeypatch, filter=f)
    assert rec.looked_up == ["nann_search_filtered_workspace_bytes", "nann_search_filtered"]
    assert r.item_ids.shape == (3, 8)            # k defaults to the fetch width


def test_filtered_symbols_are_part_of_the_abi_list():
    for s in ("nann_search_all_filtered", "nann_search_all_model_filtered", "nann_search_filtered", "nann_search_model_filtered"):
        assert s in _lib.SYMBOLS and s + "_workspace_bytes" in _lib.SYMBOLS
    names = [n for n, _ in _lib.Filter._fields_]
    assert names == ["struct_bytes", "deny_bits", "excl_row_splits", "excl_rows", "n_excl"]
    assert C.sizeof(_lib.Filter) == 40           # i32 + padding, three pointers, i64: the C struct's layout
