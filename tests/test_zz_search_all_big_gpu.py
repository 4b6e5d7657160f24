"""-m gpu: the exhaustive search above 2^20 rows, where the score buffer's byte budget -- not kScanMaxChunk -- sets the chunk
(scan_layout, csrc/nann_scan_inst.hip).  At 1 200 000 x 64 f16 rows a chunk of the L2 / IP scans is 96 queries, one of the MLP /
attention scans 111 users, over 74 slabs; every batch here is one such chunk and a partial second one (104 = 96 + 8 queries, 120 =
111 + 9, 113 = 111 + 2), so everything a call addresses by the chunk's first query -- outputs, exclusion lists, predicates,
thresholds and row_splits, n_out, the staging areas -- is read at an offset that is neither 0 nor 128.

Expected values come from big_corpus.py: the oracle's score of every (query, row), and numpy over those rows; nothing from a
device.  test_search_all_big_cpu.py holds the builders to naive Python and the corpora to the properties these tests lean on.
L2, IP and the exact / certified MLP are compared bit for bit; the split MLP and the attention model by the project's rule,
|error| <= 1e-5 max(1, |s|) and tolerant_parity "exact" or "near-tie".  On corpus B every base row lies in the table 60 times:
its copies must carry one bit pattern whichever chunk and slab scored them, with no reference involved."""
import ctypes as C
import os
import resource
import sys
import time

import numpy as np
import pytest
import torch

from gpu_util import bits, cuda, require_gpu, tolerant_parity

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import big_corpus as BC  # noqa: E402

pytestmark = pytest.mark.gpu
_CACHE = {}
RTOL = 1e-5
PAGE = 4096


@pytest.fixture(scope="module", autouse=True)
def _module():
    require_gpu()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    free, total = torch.cuda.mem_get_info()
    print("\n[big corpus] module %.1f s, host peak %.0f MB, torch device peak %.0f MB, device in use at the end %.0f MB"
          % (time.time() - t0, resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0,
             torch.cuda.max_memory_allocated() / 2.0 ** 20, (total - free) / 2.0 ** 20))
    _CACHE.clear()
    BC.release()
    torch.cuda.empty_cache()


# ---- helpers -----------------------------------------------------------------------------------------------------------
def _index(embs, ids):
    from nann_amd import retrieval
    nbv, rs, ep = BC.ring(len(embs))
    return retrieval.Index(embs, ids, nbv, rs, ep)


def _a():
    """(device index over corpus A, its L2 scorer, queries on the device, full_A, ids)"""
    if "A" not in _CACHE:
        from nann_amd import ops
        a = BC.corpus_a()
        _CACHE["A"] = (_index(a["embs"], a["ids"]), ops.Scorer("l2", BC.D), cuda(a["q"], torch.float32), BC.full_a(), a["ids"])
    return _CACHE["A"]


def _b():
    """(device index over corpus B, the corpus dict)"""
    if "B" not in _CACHE:
        b = BC.corpus_b()
        _CACHE["B"] = (_index(b["table"], b["ids"]), b)
    return _CACHE["B"]


def _filter_a(dix):
    if "filter_A" not in _CACHE:
        from nann_amd import retrieval
        deny, lists = BC.filter_a()
        _CACHE["filter_A"] = retrieval.make_filter(dix, deny_rows=np.flatnonzero(deny), exclude_rows=lists)
    return _CACHE["filter_A"]


def _got(r):
    torch.cuda.synchronize()
    out = {"index": r.index.cpu().numpy(), "scores": r.scores.cpu().numpy(), "item_ids": r.item_ids.cpu().numpy()}
    if getattr(r, "n_out", None) is not None:
        out["n_out"] = r.n_out.cpu().numpy()
    return out


def _same(got, exp, what="", rows=None):
    """bit for bit: rows, score bits, item ids (and n_out where both have it); rows: the queries of `got` that exp holds"""
    for name in ("n_out", "index", "item_ids", "scores"):
        if name not in got or name not in exp:
            continue
        g = got[name] if rows is None else got[name][list(rows)]
        g, e = (bits(g), bits(exp[name])) if name == "scores" else (g, exp[name])
        assert g.shape == e.shape, (what, name, g.shape, e.shape)
        bad = np.flatnonzero((g != e).reshape(len(g), max(g[0].size if len(g) else 1, 1)).any(axis=1))
        assert len(bad) == 0, (what, name, "queries", bad.tolist()[:10])


def _range_got(r):
    torch.cuda.synchronize()
    return (r.row_splits.cpu().numpy(), r.index.cpu().numpy(), r.scores.cpu().numpy(), r.item_ids.cpu().numpy())


def _range_same(got, exp, capacity=None, what=""):
    """row_splits hold the true counts whatever the capacity; the entries are the head [0, capacity) of the whole result"""
    m = len(exp[1]) if capacity is None else min(capacity, len(exp[1]))
    assert (got[0] == exp[0]).all(), (what, "row_splits", np.flatnonzero(got[0] != exp[0])[:10].tolist())
    assert len(got[1]) >= m
    assert (got[1][:m] == exp[1][:m]).all(), (what, "rows")
    assert (bits(got[2][:m]) == bits(exp[2][:m])).all(), (what, "scores")
    assert (got[3][:m] == exp[3][:m]).all(), (what, "item ids")


def _ws_bytes(symbol, *args):
    from nann_amd import _lib
    nb = C.c_int64(-1)
    assert getattr(_lib.lib(), symbol)(*args, C.byref(nb)) == 0, symbol
    return nb.value


def _mlp_scorer(precision):
    from nann_amd import ops
    return ops.Scorer("mlp", BC.D, torch.float16, BC.mlp_weights(), precision=precision)


def _attn_model(tmp_path_factory, precision):
    key = ("attn", precision)
    if key not in _CACHE:
        from nann_amd import ops
        path = str(tmp_path_factory.mktemp("big") / ("attn_" + precision))
        ops.save_scorer_dir(path, "attention", BC.attn_weights(), precision=precision)
        _CACHE[key] = ops.Model(path, BC.D, BC.L_SEQ)
    return _CACHE[key]


def _segments(got, queries):
    """the all-rows segments of a range result -> {query: scores f32[N] by row}, after checking that each holds every row once,
    ascending, and that no other query matched anything"""
    splits, rows, scores, ids = got
    counts = np.diff(splits)
    want = np.zeros(len(counts), np.int64)
    want[list(queries)] = BC.N
    assert (counts == want).all(), np.flatnonzero(counts != want)[:10].tolist()
    out = {}
    for u in queries:
        lo = int(splits[u])
        assert (rows[lo:lo + BC.N] == np.arange(BC.N, dtype=np.int32)).all(), u
        assert (ids[lo:lo + BC.N] == BC.item_ids()).all(), u
        out[u] = scores[lo:lo + BC.N]
    return out


# ---- 1. the path is reached ---------------------------------------------------------------------------------------------------
def test_01_the_byte_budget_sets_the_chunk(tmp_path_factory):
    """through the ABI only: a workspace grows with the chunk, so it stops growing at 96 queries (flat) / 111 users (MLP,
    attention) -- not at 128 -- and is smaller one below"""
    from nann_amd import ops, retrieval
    dix, sc, qd, full, ids = _a()
    flat = lambda b, k=200: _ws_bytes("nann_search_all_workspace_bytes", dix.handle, sc.handle, b, k)
    assert flat(96) == flat(97) == flat(104) == flat(111) == flat(128) == flat(1000) and flat(95) < flat(96) and flat(80) == flat(95)
    dib, b = _b()
    ip = ops.Scorer("ip", BC.D)
    assert _ws_bytes("nann_search_all_workspace_bytes", dib.handle, ip.handle, 104, 200) == flat(104)
    mlp = _mlp_scorer("exact")
    m = lambda n: _ws_bytes("nann_search_all_workspace_bytes", dib.handle, mlp.handle, n, 200)
    assert m(111) == m(112) == m(120) == m(128) == m(1000) and m(110) < m(111) and m(96) < m(110)
    model = _attn_model(tmp_path_factory, "exact")
    a = lambda n: _ws_bytes("nann_search_all_model_workspace_bytes", dib.handle, model.handle, n, 200)
    assert a(111) == a(112) == a(113) == a(128) == a(1000) and a(110) < a(111)
    from nann_amd import _lib
    sq8, bounds = _sq8(dix)
    out = (C.c_int64 * 8)()
    assert _lib.lib().nann_search_all_sq8_exact_layout(dix.handle, sq8.handle, bounds.handle, sc.handle, BC.B_FLAT, 200, 2048, 200,
                                                       out) == 0
    assert out[0] == BC.CHUNK_FLAT


# ---- 2. search_all, L2, corpus A ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [200, 1024])
def test_02_search_all_l2_bitwise(k):
    """all 104 queries against full_A; each half of the batch, passed alone, equals its rows in the whole call"""
    from nann_amd import retrieval
    dix, sc, qd, full, ids = _a()
    exp = BC.expect_topk(full, ids, k)
    whole = _got(retrieval.search_all(dix, sc, qd, k))
    _same(whole, exp, ("whole", k))
    for lo, hi in ((0, BC.CHUNK_FLAT), (BC.CHUNK_FLAT, BC.B_FLAT)):
        part = _got(retrieval.search_all(dix, sc, qd[lo:hi], k))
        _same(part, {name: v[lo:hi] for name, v in whole.items()}, ("alone", lo, hi, k))


def test_02_search_all_writes_nothing_behind_its_workspace():
    """the C call with exactly nann_search_all_workspace_bytes and a canary page behind them, at a chunk below 128"""
    from nann_amd import _lib
    from nann_amd.ops import _ptr, _stream
    dix, sc, qd, full, ids = _a()
    k = 200
    nb = _ws_bytes("nann_search_all_workspace_bytes", dix.handle, sc.handle, BC.B_FLAT, k)
    assert 0 < nb < (1 << 30)
    buf = torch.full((nb + PAGE,), 0xA5, dtype=torch.uint8, device="cuda")
    out_ids = torch.empty((BC.B_FLAT, k), dtype=torch.int64, device="cuda")
    out_scores = torch.empty((BC.B_FLAT, k), dtype=torch.float32, device="cuda")
    out_index = torch.empty((BC.B_FLAT, k), dtype=torch.int32, device="cuda")
    assert _lib.lib().nann_search_all(dix.handle, sc.handle, _ptr(qd), BC.B_FLAT, k, _ptr(out_ids), _ptr(out_scores), _ptr(out_index),
                                      _ptr(buf), nb, None, _stream()) == 0
    torch.cuda.synchronize()
    assert (buf[nb:] == 0xA5).all(), "the call wrote behind its workspace"
    _same({"index": out_index.cpu().numpy(), "scores": out_scores.cpu().numpy(), "item_ids": out_ids.cpu().numpy()},
          BC.expect_topk(full, ids, k), "C call")


# ---- 3. filter ------------------------------------------------------------------------------------------------------------------
def test_03_filtered_lists_are_read_at_the_call_s_query_number():
    from nann_amd import retrieval
    dix, sc, qd, full, ids = _a()
    exp = BC.expect_topk(full, ids, 200, filter=BC.filter_a())
    _same(_got(retrieval.search_all(dix, sc, qd, 200, filter=_filter_a(dix))), exp, "filtered")


def test_03_a_filter_that_leaves_150_rows():
    from nann_amd import retrieval
    dix, sc, qd, full, ids = _a()
    flt = BC.filter_150()
    exp = BC.expect_topk(full, ids, 200, filter=flt)
    assert (exp["n_out"] == 150).all()
    got = _got(retrieval.search_all(dix, sc, qd, 200, filter=retrieval.make_filter(dix, deny_rows=np.flatnonzero(flt[0]))))
    _same(got, exp, "150 rows")
    assert (got["n_out"] == 150).all() and not got["index"][:, 150:].any() and not bits(got["scores"][:, 150:]).any() \
        and not got["item_ids"][:, 150:].any()


# ---- 4. predicates ----------------------------------------------------------------------------------------------------------------
def test_04_search_all_where_label_sets_across_the_seam():
    from nann_amd import retrieval
    dix, sc, qd, full, ids = _a()
    pred = BC.labels_a()
    exp = BC.expect_topk(full, ids, 200, filter=BC.filter_a(), pred=pred)
    at = retrieval.make_attributes(dix, label_of_row=pred["label_of_row"])
    p = retrieval.make_predicates(at, BC.B_FLAT, label_in=BC.label_lists(pred, BC.B_FLAT))
    _same(_got(retrieval.search_all_where(dix, sc, qd, 200, p, filter=_filter_a(dix))), exp, "where + filter")
    _same(_got(retrieval.search_all_where(dix, sc, qd, 200, p)), BC.expect_topk(full, ids, 200, pred=pred), "where")


# ---- 5. range -------------------------------------------------------------------------------------------------------------------
def test_05_range_thresholds_of_every_kind_in_both_chunks():
    from nann_amd import retrieval
    dix, sc, qd, full, ids = _a()
    thr = BC.thresholds_a()
    exp = BC.expect_range(full, ids, thr)
    total = int(exp[0][-1])
    r = retrieval.search_all_range(dix, sc, qd, thr, capacity=total)
    _range_same(_range_got(r), exp, what="range")
    assert r.total == total and not r.truncated
    # a capacity that ends in the middle of a second-chunk segment (query 98 matches 5000 rows)
    assert exp[0][99] - exp[0][98] == 5000
    cap = int(exp[0][98]) + 2500
    r = retrieval.search_all_range(dix, sc, qd, thr, capacity=cap)
    _range_same(_range_got(r), exp, capacity=cap, what="range, truncated")
    assert r.total == total and r.truncated
    # under the filter of 3
    expf = BC.expect_range(full, ids, thr, filter=BC.filter_a())
    r = retrieval.search_all_range(dix, sc, qd, thr, capacity=total, filter=_filter_a(dix))
    _range_same(_range_got(r), expf, what="range, filtered")


def test_05_range_all_rows_equal_the_oracle_row_for_row():
    """-FLT_MAX for two queries on each side of the seam, a threshold above the best score for the rest: those four segments are
    the device's score of every one of the 1 200 000 rows"""
    from nann_amd import retrieval
    dix, sc, qd, full, ids = _a()
    which = BC.ALL_ROWS["flat"]
    thr = BC.all_rows_thresholds(full, which)
    seg = _segments(_range_got(retrieval.search_all_range(dix, sc, qd, thr, capacity=len(which) * BC.N)), which)
    for u in which:
        bad = np.flatnonzero(bits(seg[u]) != bits(full[u]))
        assert len(bad) == 0, (u, len(bad), bad[:10].tolist())


# ---- 6. wide --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4097, 16384])
def test_06_wide_bitwise(k):
    from nann_amd import retrieval
    dix, sc, qd, full, ids = _a()
    exp = BC.expect_topk(full, ids, k, wide=True)
    assert (exp["n_out"] == k).all()
    got = _got(retrieval.search_all_wide(dix, sc, qd, k))
    _same(got, exp, ("wide", k))
    expf = BC.expect_topk(full, ids, k, filter=BC.filter_a(), wide=True)
    _same(_got(retrieval.search_all_wide(dix, sc, qd, k, filter=_filter_a(dix))), expf, ("wide, filtered", k))
    # search_all's score bits: the head of the wide list is the slab form's list
    narrow = _got(retrieval.search_all(dix, sc, qd, 1024))
    assert (got["index"][:, :1024] == narrow["index"]).all() and (bits(got["scores"][:, :1024]) == bits(narrow["scores"])).all()


# ---- the forms that stage search_all's whole output: one call each, user 32's vectors on both sides of the seam -------------------
def _vectors():
    dix, sc, qd, full, ids = _a()
    vm = list(BC.VEC_MAP)
    return qd[vm].contiguous(), full[vm]


def test_06_grouped_over_105_vectors():
    import groupcap_model as GM
    from nann_amd import retrieval
    dix, sc, qd, full, ids = _a()
    qv, fv = _vectors()
    g, caps = BC.groups_a()
    lists = BC.expect_topk(fv, ids, 1024)
    exp = GM.model(lists["scores"], lists["index"], None, BC.N, g, 1, 100, caps=caps, item_ids=ids)
    assert (exp["n_out"] == 100).all() and (exp["pos"][:, -1] > 100).all()              # the caps bite, the fetch width holds
    r = retrieval.search_all_grouped(dix, sc, qv, 100, retrieval.make_groups(dix, group_of_row=g, caps=caps), fetch=1024)
    got = _got(r)
    got["group"] = r.group.cpu().numpy()
    _same(got, exp, "grouped")
    assert (got["group"] == exp["group"]).all()


def test_06_multi_over_35_users_of_3_vectors():
    import union_model as UM
    from nann_amd import retrieval
    dix, sc, qd, full, ids = _a()
    qv, fv = _vectors()
    lists = BC.expect_topk(fv, ids, 200)
    shape = (BC.N_USERS, BC.N_VEC, 200)
    exp = UM.model(lists["scores"].reshape(shape), lists["index"].reshape(shape), None, BC.N, 200, item_ids=ids)
    assert (exp["n_out"] == 200).all() and len(set(exp["list"][32].tolist())) > 1         # user 32 draws on both chunks
    r = retrieval.search_all_multi(dix, sc, qv.reshape(BC.N_USERS, BC.N_VEC, BC.D), 200)
    got = _got(r)
    _same(got, exp, "multi")
    assert (r.vec.cpu().numpy() == exp["list"]).all()


# ---- 7. sq8, L2, corpus A ---------------------------------------------------------------------------------------------------------
def _sq8(dix):
    if "sq8" not in _CACHE:
        from nann_amd import retrieval
        t = retrieval.make_sq8(dix)
        _CACHE["sq8"] = (t, retrieval.make_sq8_bounds(dix, t))
    return _CACHE["sq8"]


def test_07_sq8_exact_certified_queries_are_search_all_bit_for_bit():
    from nann_amd import retrieval
    dix, sc, qd, full, ids = _a()
    t, bounds = _sq8(dix)
    model = BC.sq8_a()["exact"]
    sample = list(BC.SAMPLE["flat"])
    exp = BC.expect_topk(full, ids, BC.SQ8_K)
    r = retrieval.search_all_sq8_exact(dix, t, bounds, sc, qd, BC.SQ8_K, fetch=BC.SQ8_FETCH, cap=BC.SQ8_CAP, fallback=False)
    got = _got(r)
    cert, n_surv = r.certified.cpu().numpy(), r.n_survivors.cpu().numpy()
    assert model.certified.all() and (cert[sample] == 1).all() and (n_surv[sample] == model.n_survivors).all()
    yes = np.flatnonzero(cert == 1)
    _same(got, {name: v[yes] for name, v in exp.items() if name != "n_out"}, "certified", rows=yes)
    # a cap equal to the fetch width: the sampled flags are the model's
    r = retrieval.search_all_sq8_exact(dix, t, bounds, sc, qd, BC.SQ8_K, fetch=BC.SQ8_FETCH, cap=BC.SQ8_CAP_LOW, fallback=False)
    got = _got(r)
    cert, n_surv = r.certified.cpu().numpy(), r.n_survivors.cpu().numpy()
    assert (cert[sample] == (model.n_survivors <= BC.SQ8_CAP_LOW)).all() and (n_surv[sample] == model.n_survivors).all()
    yes = np.flatnonzero(cert == 1)
    _same(got, {name: v[yes] for name, v in exp.items() if name != "n_out"}, "certified, low cap", rows=yes)


def test_07_sq8_range_exact_certified_segments_are_search_all_range():
    from nann_amd import retrieval
    dix, sc, qd, full, ids = _a()
    t, bounds = _sq8(dix)
    model = BC.sq8_a()["range"]
    sample = list(BC.SAMPLE["flat"])
    thr = BC.thresholds_a()
    assert (thr[[i for i in range(BC.B_FLAT) if i % 4 != 3]] <= 0).all()
    splits, rows, scores, eids = BC.expect_range(full, ids, thr)
    r = retrieval.search_all_range_sq8_exact(dix, t, bounds, sc, qd, thr, cap=BC.SQ8_RANGE_CAP, fallback=False)
    g_splits, g_rows, g_scores, g_ids = _range_got(r)
    cert, n_surv = r.certified.cpu().numpy(), r.n_survivors.cpu().numpy()
    assert model.certified.all() and (cert[sample] == 1).all() and (n_surv[sample] == model.n_survivors).all()
    for i in range(BC.B_FLAT):     # a certified query's segment is search_all_range's, an uncertified one's is empty
        lo, hi, glo, ghi = int(splits[i]), int(splits[i + 1]), int(g_splits[i]), int(g_splits[i + 1])
        if not cert[i]:
            assert ghi == glo, i
            continue
        assert ghi - glo == hi - lo and (g_rows[glo:ghi] == rows[lo:hi]).all(), i
        assert (bits(g_scores[glo:ghi]) == bits(scores[lo:hi])).all() and (g_ids[glo:ghi] == eids[lo:hi]).all(), i
    assert cert.sum() >= len(sample)


def test_07_sq8_fetch_order_is_the_model_s():
    from nann_amd import retrieval
    dix, sc, qd, full, ids = _a()
    t, bounds = _sq8(dix)
    f_rows, f_scores = BC.sq8_a()["fetch"]
    sample = list(BC.SAMPLE["flat"])
    r = retrieval.search_all_sq8(dix, t, sc, qd, BC.SQ8_K, fetch=BC.SQ8_FETCH, return_fetch=True)
    torch.cuda.synchronize()
    assert (r.fetch_index.cpu().numpy()[sample] == f_rows).all()
    assert (bits(r.fetch_scores.cpu().numpy()[sample]) == bits(f_scores)).all()
    # ... and the result is the exact re-rank of the fetched rows: search_all's bits for the rows returned
    got = _got(r)
    for j, u in enumerate(sample):
        rows = np.sort(f_rows[j])
        order = rows[BC.topk_rows(full[u][rows], BC.SQ8_K)]
        assert (got["index"][u] == order).all() and (bits(got["scores"][u]) == bits(full[u][order])).all(), u


# ---- 8. IP, corpus B --------------------------------------------------------------------------------------------------------------
def test_08_ip_topk_range_and_wide_on_the_expanded_corpus():
    from nann_amd import ops, retrieval
    dib, b = _b()
    sc = ops.Scorer("ip", BC.D)
    qd = cuda(b["q"][:BC.B_FLAT], torch.float32)
    full = BC.full_b("ip")
    _same(_got(retrieval.search_all(dib, sc, qd, 200)), BC.expect_topk(full, b["ids"], 200), "ip, k = 200")
    _same(_got(retrieval.search_all_wide(dib, sc, qd, 4097)), BC.expect_topk(full, b["ids"], 4097, wide=True), "ip, wide")
    which = BC.ALL_ROWS["flat"]
    thr = BC.all_rows_thresholds(BC.base_scores("ip"), which)
    seg = _segments(_range_got(retrieval.search_all_range(dib, sc, qd, thr, capacity=len(which) * BC.N)), which)
    for u in which:
        assert BC.copies_share_bits(seg[u], b["map"]), u
        assert (bits(seg[u]) == bits(full[u])).all(), u


# ---- 9. MLP, corpus B, 120 queries ------------------------------------------------------------------------------------------------
def _mlp_runs(precision):
    """one prepared scorer -> (top 200 of the 120 queries, of queries [111, 120) alone, the all-rows segments)"""
    from nann_amd import retrieval
    dib, b = _b()
    sc = _mlp_scorer(precision)
    qd = cuda(b["q"], torch.float32)
    which = BC.ALL_ROWS["mlp"]
    thr = BC.all_rows_thresholds(BC.base_scores("mlp"), which)
    # (a threshold "above the best" by the oracle's scores: the split form may score within 1e-5 of it, so leave that much room)
    thr = np.where(thr == -BC.FLT_MAX, thr, thr + np.float32(1.0)).astype(np.float32)
    retrieval.prepare(dib, sc)
    try:
        whole = _got(retrieval.search_all(dib, sc, qd, 200))
        tail = _got(retrieval.search_all(dib, sc, qd[BC.CHUNK_MODEL:], 200))
        seg = _segments(_range_got(retrieval.search_all_range(dib, sc, qd, thr, capacity=len(which) * BC.N)), which)
    finally:
        torch.cuda.synchronize()
        retrieval.release(dib, sc)
    return whole, tail, seg


@pytest.mark.parametrize("precision", ["exact", "certified"])
def test_09_mlp_bitwise(precision):
    dib, b = _b()
    whole, tail, seg = _mlp_runs(precision)
    sample = BC.SAMPLE["mlp"]
    _same(whole, BC.expect_topk(BC.full_b("mlp", sample), b["ids"], 200), precision, rows=sample)
    assert (whole["item_ids"] == b["ids"][whole["index"]]).all()
    _same(tail, {name: v[BC.CHUNK_MODEL:] for name, v in whole.items()}, (precision, "queries [111, 120) alone"))
    for u, s in seg.items():
        assert BC.copies_share_bits(s, b["map"]), u
        assert (bits(s) == bits(BC.full_b("mlp", [u])[0])).all(), u


def test_09_mlp_split_within_tolerance():
    dib, b = _b()
    whole, tail, seg = _mlp_runs("split")
    sample = BC.SAMPLE["mlp"]
    exp = BC.expect_topk(BC.full_b("mlp", sample), b["ids"], 200)
    verdicts = [tolerant_parity(whole["index"][u], whole["scores"][u], exp["index"][j], exp["scores"][j], rtol=RTOL)
                for j, u in enumerate(sample)]
    assert set(verdicts) <= {"exact", "near-tie"}, verdicts
    assert (whole["item_ids"] == b["ids"][whole["index"]]).all()
    _same(tail, {name: v[BC.CHUNK_MODEL:] for name, v in whole.items()}, "split, queries [111, 120) alone")
    for u, s in seg.items():
        assert BC.copies_share_bits(s, b["map"]), u
        ref = BC.full_b("mlp", [u])[0]
        err = np.abs(s.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
        assert err.max() <= RTOL, (u, err.max())


# ---- 10. attention, corpus B, 113 users -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["exact", "split"])
def test_10_attention(tmp_path_factory, precision):
    from nann_amd import retrieval
    dib, b = _b()
    model = _attn_model(tmp_path_factory, precision)
    seqs = cuda(b["seqs"][:BC.B_ATTN], torch.float16)
    s_base = BC.base_scores("attn")
    sample = BC.SAMPLE["attn"]
    whole = _got(retrieval.search_all_model(dib, model, seqs, 200))
    exp = BC.expect_topk(BC.full_b("attn", sample), b["ids"], 200)
    verdicts = [tolerant_parity(whole["index"][u], whole["scores"][u], exp["index"][j], exp["scores"][j], rtol=RTOL)
                for j, u in enumerate(sample)]
    assert set(verdicts) <= {"exact", "near-tie"}, verdicts
    for u in range(BC.B_ATTN):   # the score error on the returned rows, every user
        own = s_base[u][b["map"][whole["index"][u]]]
        assert (np.abs(whole["scores"][u] - own) <= RTOL * np.maximum(1.0, np.abs(own))).all(), u
    assert (whole["item_ids"] == b["ids"][whole["index"]]).all()
    # users [111, 113) alone: bit for bit their rows in the whole call
    tail = _got(retrieval.search_all_model(dib, model, seqs[BC.CHUNK_MODEL:], 200))
    _same(tail, {name: v[BC.CHUNK_MODEL:] for name, v in whole.items()}, (precision, "users [111, 113) alone"))
    # every row of four users
    which = BC.ALL_ROWS["attn"]
    thr = BC.all_rows_thresholds(s_base, which)
    thr = np.where(thr == -BC.FLT_MAX, thr, thr + np.float32(1.0)).astype(np.float32)
    r = retrieval.search_all_range_model(dib, model, seqs, thr, capacity=len(which) * BC.N)
    seg = _segments(_range_got(r), which)
    wide = _got(retrieval.search_all_model_wide(dib, model, seqs, 4097))
    assert (wide["n_out"] == 4097).all()
    for u in which:
        assert BC.copies_share_bits(seg[u], b["map"]), u
        ref = s_base[u][b["map"]]
        err = np.abs(seg[u].astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
        assert err.max() <= RTOL, (u, err.max())
        head = BC.topk_rows(seg[u], 4097)                      # the sorted head of the device's own scores of every row
        assert (wide["index"][u] == head).all() and (bits(wide["scores"][u]) == bits(seg[u][head])).all(), u
        assert (whole["index"][u] == head[:200]).all() and (bits(whole["scores"][u]) == bits(seg[u][head[:200]])).all(), u
