"""-m "not gpu": what test_zz_search_all_big_gpu.py relies on, established on the reference alone -- that 1 200 000 rows give the
chunks 96 / 111 over 74 slabs under the constants the sources state, that the expectation builders of big_corpus.py equal naive
per-row Python, and that the two corpora have the properties that make a pass on the device mean something."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import big_corpus as BC  # noqa: E402
import predicate_model as PM  # noqa: E402
import wide_model as WM  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _drop_the_corpora():
    yield
    BC.release()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ---- the chunk rule ---------------------------------------------------------------------------------------------------------
def test_constants_give_the_chunks_the_gpu_file_is_written_for():
    c = BC.constants()
    assert BC.chunk_rule(c, BC.N, 10 ** 6, flat=False) == (BC.CHUNK_MODEL, BC.N_SLABS) == (111, 74)
    assert BC.chunk_rule(c, BC.N, 10 ** 6, flat=True) == (BC.CHUNK_FLAT, BC.N_SLABS) == (96, 74)
    # the byte budget, not kScanMaxChunk, decides: the branch no smaller corpus reaches
    assert c["kScanScoreBytes"] // (4 * BC.N) < c["kScanMaxChunk"] and c["kScanScoreBytes"] // (4 * (1 << 20)) == c["kScanMaxChunk"]
    # every batch is more than one chunk, and its second chunk is a partial one (flat: a partial tile)
    for b, flat in ((BC.B_FLAT, True), (BC.B_MLP, False), (BC.B_ATTN, False)):
        chunk = BC.chunk_rule(c, BC.N, b, flat)[0]
        assert chunk == (96 if flat else 111) and chunk < b < 2 * chunk
    assert 0 < BC.B_FLAT - BC.CHUNK_FLAT < c["kScanTileQueries"]
    # ... and the workspace sizes the ABI check reads: the same chunk from the chunk size on, a smaller one just below it
    assert BC.chunk_rule(c, BC.N, 96, True)[0] == 96 and BC.chunk_rule(c, BC.N, 95, True)[0] == 80
    assert BC.chunk_rule(c, BC.N, 111, False)[0] == 111 and BC.chunk_rule(c, BC.N, 110, False)[0] == 110
    # the sampled positions sit on both sides of each seam
    for kind, chunk, b in (("flat", 96, BC.B_FLAT), ("mlp", 111, BC.B_MLP), ("attn", 111, BC.B_ATTN)):
        for s in (BC.SAMPLE[kind], BC.ALL_ROWS[kind]):
            assert min(s) == 0 and max(s) == b - 1 and chunk - 1 in s and chunk in s and len(set(s)) == len(s)


# ---- the expectation builders against naive Python at n = 3 000 --------------------------------------------------------------
N_SMALL, B_SMALL = 3000, 6


def _small_case():
    """scores with crafted ties (every score drawn from 40 values), +0 and -0 among them, a few -inf, a filter and labels"""
    rng = np.random.default_rng(5)
    vals = np.concatenate((rng.standard_normal(38).astype(np.float32), [np.float32(0.0), np.float32(-0.0)]))
    full = vals[rng.integers(0, 40, (B_SMALL, N_SMALL))].astype(np.float32)
    full[:, rng.integers(0, N_SMALL, 30)] = -np.inf
    assert (bits(full) == 0x80000000).any() and (bits(full) == 0).any()
    deny = rng.random(N_SMALL) < 0.5
    exclude = [rng.integers(-2, N_SMALL + 2, int(m)).astype(np.int64) for m in (0, 1, 30, 300, 7, 299)]
    lab = rng.integers(0, 5, N_SMALL).astype(np.int32)
    lists = [np.array(l, np.int32) for l in ([0], [1, 2], [], [4, 4, 0], [3], [0, 1, 2, 3])]
    pred = {"label_of_row": lab, "labels": np.concatenate(lists).astype(np.int32),
            "label_splits": np.concatenate(([0], np.cumsum([len(l) for l in lists]))).astype(np.int64)}
    return full, (deny, exclude), pred


def _naive_allowed(i, r, filter, pred):
    if filter is not None:
        deny, exclude = filter
        if deny is not None and deny[r]:
            return False
        if exclude is not None and r in set(int(x) for x in exclude[i]):
            return False
    return PM.restate_passes(pred, i, r)


def _naive_topk(full, i, k, filter, pred, wide):
    rows = [r for r in range(full.shape[1]) if _naive_allowed(i, r, filter, pred) and not (wide and full[i, r] == -math.inf)]
    rows.sort(key=lambda r: (-(float(full[i, r]) + 0.0), r))
    return rows[:k]


@pytest.mark.parametrize("k", [1, 7, 200, 1024, 2999, 3000])
def test_topk_builders_equal_naive_python(k):
    full, flt, pred = _small_case()
    ids = BC.item_ids(N_SMALL)
    for filter, p, wide in ((None, None, False), (flt, None, False), (flt, pred, False), (None, None, True), (flt, None, True)):
        exp = BC.expect_topk(full, ids, k, filter=filter, pred=p, wide=wide)
        cut_in_tie = 0
        for i in range(B_SMALL):
            rows = _naive_topk(full, i, k, filter, p, wide)
            m = len(rows)
            assert exp["n_out"][i] == m and exp["index"][i, :m].tolist() == rows
            assert (bits(exp["scores"][i, :m]) == bits(full[i, rows])).all() and (exp["item_ids"][i, :m] == ids[rows]).all()
            assert not exp["index"][i, m:].any() and not bits(exp["scores"][i, m:]).any() and not exp["item_ids"][i, m:].any()
            every = _naive_topk(full, i, N_SMALL, filter, p, wide)
            cut_in_tie += m < len(every) and full[i, every[m]] == full[i, rows[-1]]
        assert cut_in_tie or k >= 2999  # the cut falls inside a group of tied rows: the "first m rows at the cut" rule is used
    # the wide builder is the contract wide_model.reference states
    for i in range(B_SMALL):
        v, r, n_out = WM.reference(full[i], k)
        exp = BC.expect_topk(full[i:i + 1], ids, k, wide=True)
        assert exp["n_out"][0] == n_out and (exp["index"][0] == r).all() and (bits(exp["scores"][0]) == bits(v)).all()


def test_a_shifted_query_number_changes_the_small_expectation():
    """row i of `full` is query q0 + i of the filter and the predicates: the builders honour q0"""
    full, flt, pred = _small_case()
    ids = BC.item_ids(N_SMALL)
    whole = BC.expect_topk(full, ids, 50, filter=flt, pred=pred)
    tail = BC.expect_topk(full[4:], ids, 50, filter=flt, pred=pred, q0=4)
    assert all((whole[name][4:] == tail[name]).all() for name in ("index", "n_out", "item_ids"))
    wrong = BC.expect_topk(full[4:], ids, 50, filter=flt, pred=pred, q0=3)
    assert (whole["index"][4:] != wrong["index"]).any(axis=1).all()


def test_range_builder_equals_naive_python():
    full, flt, _ = _small_case()
    ids = BC.item_ids(N_SMALL)
    thr = np.array([0.0, -0.0, np.float32(-math.inf), -BC.FLT_MAX, np.nan, 0.5], np.float32)
    for filter in (None, flt):
        splits, rows, scores, out_ids = BC.expect_range(full, ids, thr, filter=filter)
        at = 0
        for i in range(B_SMALL):
            naive = [r for r in range(N_SMALL) if _naive_allowed(i, r, filter, None) and float(full[i, r]) >= float(thr[i])
                     and full[i, r] != -math.inf]
            assert splits[i] == at and rows[at:at + len(naive)].tolist() == naive
            assert (bits(scores[at:at + len(naive)]) == bits(full[i, naive])).all()
            at += len(naive)
        assert splits[B_SMALL] == at == len(rows) and (out_ids == ids[rows]).all()
        assert splits[5] == splits[4]  # a NaN threshold matches nothing
    # -0 >= +0: the two zero thresholds match the same rows
    assert (np.diff(splits)[0] > 0) and BC.RM.match(full[1], thr[1]).sum() == BC.RM.match(full[1], thr[0]).sum()
    # the thresholds helpers: the m-th best score, and one above the best
    t = BC.range_thresholds(full, pattern=(1, 300, None))
    for i in range(B_SMALL):
        order = sorted(full[i].tolist(), reverse=True)
        m = (1, 300, None)[i % 3]
        assert t[i] == (np.nextafter(np.float32(order[0]), np.float32(np.inf)) if m is None else np.float32(order[m - 1]))
    t = BC.all_rows_thresholds(full, (1, 4))
    assert (t[[1, 4]] == -BC.FLT_MAX).all() and all(t[i] > full[i].max() for i in (0, 2, 3, 5))


# ---- the real corpora ---------------------------------------------------------------------------------------------------------
def test_corpus_b_sixty_copies_and_cuts_inside_a_group(oracle):
    b = BC.corpus_b()
    assert (np.bincount(b["map"], minlength=BC.N_BASE) == BC.COPIES).all() and len(b["map"]) == BC.N
    assert (b["table"][[0, 1, BC.N - 1]] == b["base"][b["map"][[0, 1, BC.N - 1]]]).all()
    # the copies are scattered: no base row's copies sit in one chunk-of-rows neighbourhood
    first, last = np.full(BC.N_BASE, BC.N), np.zeros(BC.N_BASE, np.int64)
    np.minimum.at(first, b["map"], np.arange(BC.N))
    np.maximum.at(last, b["map"], np.arange(BC.N))
    assert ((last - first) > BC.N // 2).all()
    assert 200 == 3 * BC.COPIES + 20 and 4097 == 68 * BC.COPIES + 17
    for kind in ("ip", "mlp"):
        s = BC.base_scores(kind)
        assert s.shape == ({"ip": BC.B_FLAT, "mlp": BC.B_MLP}[kind], BC.N_BASE) and np.isfinite(s).all()
        # the base row at rank 3 (68) ties with neither neighbour: the expanded ranking has its 60 copies at 180 .. 239 (4080 ..
        # 4139) and nothing else at their score, so k = 200 (4097) cuts inside that group, for every query
        top = -np.sort(-(s + np.float32(0.0)), axis=1)[:, :70]
        for g in (3, 68):
            assert ((top[:, g - 1] > top[:, g]) & (top[:, g] > top[:, g + 1])).all(), (kind, g)
    # ... which the builder then shows on an expanded row: the k-th and (k + 1)-th rows tie, and the lower rows were taken
    full = BC.full_b("ip", [0, 103])
    for k in (200, 4097):
        exp = BC.expect_topk(full, b["ids"], k + 1)
        for i in range(2):
            assert exp["scores"][i, k - 1] == exp["scores"][i, k] and exp["index"][i, k - 1] < exp["index"][i, k]
            group = np.flatnonzero(b["map"] == b["map"][exp["index"][i, k]])
            assert (np.sort(exp["index"][i][exp["scores"][i] == exp["scores"][i, k]]) == group[:k % BC.COPIES + 1]).all()
    assert BC.copies_share_bits(full[0]) and not BC.copies_share_bits(np.where(np.arange(BC.N) == 5, np.float32(1e9), full[0]))


def test_corpus_a_gives_the_cases_their_teeth(oracle):
    a, full = BC.corpus_a(), BC.full_a()
    assert full.shape == (BC.B_FLAT, BC.N) and np.isfinite(full).all() and (full <= 0).all()
    # one row against the canonical order restated in numpy: the oracle's L2 is what the builders are fed
    import ip_reference as IR
    some = np.array([0, 1, 16383, 16384, BC.N - 1])
    assert (bits(full[97][some]) == bits(IR.l2_scores(a["q"][97], IR.widen(a["embs"][some])))).all()
    # the builder's top-k is the oracle's brute force
    from oracle import oracle as O
    nbv, rs, ep = BC.ring(BC.N)
    oix = O.Index(a["embs"], a["ids"], nbv, rs, ep)
    rc, bi, bv = O.brute_force(oix, O.Scorer("l2", BC.D, O.EMB_F16), a["q"][96], 1024)
    exp = BC.expect_topk(full, a["ids"], 1024, queries=[96])
    assert rc == 0 and (exp["index"][0] == bi).all() and (bits(exp["scores"][0]) == bits(bv)).all()
    # no two queries share a top-200 list
    top = BC.expect_topk(full, a["ids"], 200)
    lists = {tuple(r) for r in top["index"].tolist()}
    assert len(lists) == BC.B_FLAT
    # the range thresholds give the intended match counts
    thr = BC.thresholds_a()
    counts = np.array([int(BC.RM.match(full[i], thr[i]).sum()) for i in range(BC.B_FLAT)])
    want = np.array([BC.RANGE_M[i % 4] or 0 for i in range(BC.B_FLAT)])
    assert (counts == want).all()
    for lo, hi in ((0, BC.CHUNK_FLAT), (BC.CHUNK_FLAT, BC.B_FLAT)):  # both chunks hold every case
        assert set(want[lo:hi].tolist()) == {0, 1, 300, 5000}
    # the filter: about half the rows denied, lists of 0 .. 300 rows that differ from query to query and bite
    deny, lists = BC.filter_a()
    assert 0.49 < deny.mean() < 0.51
    lens = np.array([len(l) for l in lists])
    assert lens.min() == 0 and lens.max() == 300 and lens[96] == 297 and len({tuple(l) for l in lists if len(l)}) == (lens > 0).sum()
    flt = BC.expect_topk(full, a["ids"], 200, filter=(deny, lists))
    assert (flt["n_out"] == 200).all()
    # ... an expectation built with the second chunk's lists or label sets shifted by one position differs for every such query
    second = list(range(BC.CHUNK_FLAT, BC.B_FLAT))
    pred = BC.labels_a()
    for shift in (-1, -BC.CHUNK_FLAT):  # read at c0 + i - 1, and at i (the chunk's offset forgotten)
        wrong_f = BC.expect_topk(full[second], a["ids"], 200, filter=(deny, lists), q0=BC.CHUNK_FLAT + shift)
        assert (wrong_f["index"] != flt["index"][second]).any(axis=1).all()
        right_p = BC.expect_topk(full[second], a["ids"], 200, filter=(deny, lists), pred=pred, q0=BC.CHUNK_FLAT)
        wrong_p = BC.expect_topk(full[second], a["ids"], 200, filter=(deny, None), pred=pred, q0=BC.CHUNK_FLAT + shift)
        assert (wrong_p["index"] != right_p["index"]).any(axis=1).all()
    # the second filter leaves 150 rows
    d150, _ = BC.filter_150()
    assert int((~d150).sum()) == 150
    few = BC.expect_topk(full, a["ids"], 200, filter=(d150, None), queries=[0, 103])
    assert (few["n_out"] == 150).all() and not few["index"][:, 150:].any()


def test_sq8_caps_certify_every_sampled_query(oracle):
    """sq8_exact_model.search_exact over corpus A for the sampled queries: the recorded caps are what the model gives"""
    m = BC.sq8_a()
    r = m["exact"]
    pow2 = lambda v: 1 << int(v - 1).bit_length()
    assert r.certified.all() and len(r.certified) == len(BC.SAMPLE["flat"]) == 8, r.n_survivors
    assert pow2(r.n_survivors.max()) == BC.SQ8_CAP                                   # SQ8_CAP = 512: all eight certified
    assert BC.SQ8_CAP_LOW == BC.SQ8_FETCH == 200 and not (r.n_survivors <= BC.SQ8_CAP_LOW).all()   # SQ8_CAP_LOW = 200: not all
    # the certified result is the exact top k
    exp = BC.expect_topk(BC.full_a(), BC.corpus_a()["ids"], BC.SQ8_K, queries=BC.SAMPLE["flat"])
    assert (r.rows == exp["index"]).all() and (bits(r.scores) == bits(exp["scores"])).all()
    # the range form at the thresholds of the range test: SQ8_RANGE_CAP = 8192
    g = m["range"]
    assert g.certified.all() and pow2(g.n_survivors.max()) == BC.SQ8_RANGE_CAP
    # a chunk's final lists are one candidate-list search: cap <= cand_max_list(96) = (2^31 - 1) / 96
    assert max(BC.SQ8_CAP, BC.SQ8_RANGE_CAP) <= 0x7fffffff // BC.CHUNK_FLAT
