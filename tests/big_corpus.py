"""Workload and expected values of the exhaustive-search tests above 2^20 rows (test_search_all_big_cpu.py,
test_zz_search_all_big_gpu.py); nothing under nann_amd/ imports it, and nothing here comes from a device.

scan_layout (csrc/nann_scan_inst.hip) scores a batch in chunks of min(kScanMaxChunk, kScanScoreBytes / (4 n_items)) queries,
clamped to [1, n_queries], the L2 / IP scans rounded down to whole tiles of kScanTileQueries.  Up to 2^20 rows that is
min(128, B); at N = 1 200 000 rows the byte budget decides: 111 for the MLP / attention scans, 96 for the flat ones, over 74 slabs.

Corpus A ("distinct"): N clustered f16 rows of width 64, ids 7 i + 3, 104 = 96 + 8 queries (means of synthetic histories).
  full_a() f32[104, N] is every query's oracle.score_rows under L2; every L2 expectation is numpy over its rows.
Corpus B ("expanded"): table[r] = base[map[r]], 20 000 base rows, map = permutation(N) % 20 000: exactly 60 copies of each base
  row, scattered.  A reference score depends on the row's content alone, so a query's N scores are s_base[q][map] at the price
  of 20 000 reference scores -- and the 60 copies of a base row must get one bit pattern from the device wherever they lie.

Everything is cached in _CACHE; release() drops it."""
import os
import re
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import predicate_model as PM  # noqa: E402
import range_model as RM  # noqa: E402

N, D = 1_200_000, 64
N_BASE, COPIES = 20_000, 60
L_SEQ = 50
B_FLAT, B_MLP, B_ATTN = 104, 120, 113       # each more than its chunk: 96 + 8, 111 + 9, 111 + 2
CHUNK_FLAT, CHUNK_MODEL, N_SLABS = 96, 111, 74
SAMPLE = {"flat": (0, 95, 96, 97, 103, 17, 50, 100), "mlp": (0, 110, 111, 112, 119, 23, 64, 115), "attn": (0, 110, 111, 112)}
ALL_ROWS = {"flat": (0, 95, 96, 103), "mlp": (0, 110, 111, 119), "attn": (0, 110, 111, 112)}  # two queries on each side of the seam
RANGE_M = (1, 300, 5000, None)              # query i matches its RANGE_M[i % 4] best rows (None: a threshold above the best)
FLT_MAX = np.float32(np.finfo(np.float32).max)
THREADS = 16
_CACHE = {}


def release():
    _CACHE.clear()


def pmap(fn, items, threads=THREADS):
    """fn over items on a thread pool (numpy and the oracle's C calls run side by side)"""
    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(fn, items))


# ---- the chunk rule, from the sources -------------------------------------------------------------------------------------
def constants():
    """kScanMaxChunk, kScanTileQueries, kScanSlabRows and the score-byte budget, as the sources state them"""
    from nann_amd import build
    head = open(os.path.join(build.SRC_DIR, "nann_scan.h")).read()
    inst = open(os.path.join(build.SRC_DIR, "nann_scan_inst.hip")).read()
    out = {name: int(re.search(r"constexpr int %s = (\d+);" % name, head).group(1))
           for name in ("kScanMaxChunk", "kScanTileQueries", "kScanSlabRows")}
    m = re.search(r"constexpr size_t kScanScoreBytes = \(size_t\)(\d+) << (\d+);", inst)
    out["kScanScoreBytes"] = int(m.group(1)) << int(m.group(2))
    return out


def chunk_rule(c, n_items, n_queries, flat):
    """the documented rule -> (queries per chunk, slabs)"""
    chunk = min(c["kScanMaxChunk"], c["kScanScoreBytes"] // (4 * n_items))
    chunk = max(1, min(chunk, n_queries))
    if flat and chunk > c["kScanTileQueries"]:
        chunk -= chunk % c["kScanTileQueries"]
    return chunk, (n_items + c["kScanSlabRows"] - 1) // c["kScanSlabRows"]


# ---- expectation builders: plain numpy over one query's scores ----------------------------------------------------------------
def topk_rows(scores, k, allowed=None):
    """rows of the top min(k, candidates) of one query: score descending (-0 = +0), ties to the lower row.  allowed: bool per row
    (None: every row).  np.partition finds the score at the cut, every row above it is taken and of the rows AT it the first m in
    row order; only those are sorted.  The scores hold no NaN."""
    scores = np.asarray(scores, np.float32)
    cand = None if allowed is None else np.flatnonzero(allowed)
    s = (scores if cand is None else scores[cand]) + np.float32(0.0)
    m = min(int(k), len(s))
    if m <= 0:
        return np.zeros(0, np.int64)
    if m < len(s):
        cut = np.partition(s, len(s) - m)[len(s) - m]
        gt = np.flatnonzero(s > cut)
        pos = np.concatenate((gt, np.flatnonzero(s == cut)[:m - len(gt)]))
    else:
        pos = np.arange(len(s))
    pos = pos[np.lexsort((pos, -s[pos]))]
    return pos if cand is None else cand[pos]


def allowed_rows(n_items, filter, query, pred=None, scores=None):
    """bool[n_items]: the rows the filter (deny bool[n] or None, exclusion lists or None) and the predicates leave to `query`;
    with scores, rows scoring -inf are out too (the rule of the range and wide forms)"""
    ok = np.ones(n_items, bool)
    if filter is not None:
        deny, exclude = filter
        if deny is not None:
            ok &= ~np.asarray(deny, bool)
        if exclude is not None and len(exclude[query]):
            e = np.asarray(exclude[query], np.int64)
            ok[e[(e >= 0) & (e < n_items)]] = False
    if pred is not None:
        rows = np.flatnonzero(ok)
        ok[rows] = PM.passes(pred, query, rows)
    if scores is not None:
        ok &= np.asarray(scores, np.float32) != -np.inf
    return ok


def expect_topk(full, item_ids, k, filter=None, pred=None, queries=None, q0=0, wide=False):
    """full f32[B, n] -> dict index i32[B, k], scores f32[B, k], item_ids i64[B, k], n_out i32[B]: zeros behind n_out.  Row i of
    `full` (or of full[queries]) is query q0 + i of the filter and the predicates.  wide: rows scoring -inf are never returned."""
    full = np.asarray(full)
    which = list(range(full.shape[0])) if queries is None else list(queries)
    n = full.shape[1]
    plain = filter is None and pred is None and not wide

    def one(i):
        ok = None if plain else allowed_rows(n, filter, q0 + i, pred, full[i] if wide else None)
        return topk_rows(full[i], k, ok)

    got = pmap(one, which)
    out = {"index": np.zeros((len(which), k), np.int32), "scores": np.zeros((len(which), k), np.float32),
           "item_ids": np.zeros((len(which), k), np.int64), "n_out": np.zeros(len(which), np.int32)}
    for j, (i, rows) in enumerate(zip(which, got)):
        m = len(rows)
        out["n_out"][j] = m
        out["index"][j, :m] = rows
        out["scores"][j, :m] = full[i][rows]
        out["item_ids"][j, :m] = item_ids[rows]
    return out


def expect_range(full, item_ids, thr, filter=None):
    """-> (row_splits i64[B + 1], index i32[total], scores f32[total], item_ids i64[total]): per query the rows with score >= thr
    that are allowed and not -inf, ascending"""
    full = np.asarray(full)
    b, n = full.shape

    def one(i):
        ok = RM.match(full[i], thr[i])
        if filter is not None:
            ok &= allowed_rows(n, filter, i)
        return np.flatnonzero(ok)

    rows = pmap(one, range(b))
    splits = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int64)
    flat = np.concatenate(rows) if b else np.zeros(0, np.int64)
    sc = np.concatenate([full[i][rows[i]] for i in range(b)]) if b else np.zeros(0, np.float32)
    return splits, flat.astype(np.int32), sc.astype(np.float32), np.asarray(item_ids, np.int64)[flat]


def mth_best(scores, m):
    """the score of a query's m-th best row"""
    s = np.asarray(scores, np.float32)
    return np.partition(s, len(s) - m)[len(s) - m]


def range_thresholds(full, pattern=RANGE_M):
    """f32[B]: query i's threshold is the score of its pattern[i % len]-th best row; None: just above its best score"""
    def one(i):
        m = pattern[i % len(pattern)]
        return np.nextafter(full[i].max(), np.float32(np.inf)) if m is None else mth_best(full[i], m)
    return np.asarray(pmap(one, range(full.shape[0])), np.float32)


def thresholds_a():
    """range_thresholds(full_a()), made once"""
    if "thr_A" not in _CACHE:
        _CACHE["thr_A"] = range_thresholds(full_a())
    return _CACHE["thr_A"]


def all_rows_thresholds(full, queries):
    """f32[B]: -FLT_MAX for `queries` (every row matches), above the best score for the rest (nothing does)"""
    thr = np.asarray(pmap(lambda i: np.nextafter(full[i].max(), np.float32(np.inf)), range(full.shape[0])), np.float32)
    thr[list(queries)] = -FLT_MAX
    return thr


# ---- corpus A -----------------------------------------------------------------------------------------------------------------
def ring(n, deg=8):
    nbv = ((np.arange(n, dtype=np.int64)[:, None] + 1 + np.arange(deg)) % n).astype(np.int32).reshape(-1)
    rs = (np.arange(n + 1, dtype=np.int64) * deg)
    return [nbv, nbv.copy()], [rs, rs.copy()], np.arange(0, n, max(n // 64, 1), dtype=np.int32)[:64]


def item_ids(n=N):
    return np.arange(n, dtype=np.int64) * 7 + 3


def _user_means(seqs):
    from oracle import oracle as O
    return np.stack([O.user_seq_mean(s) for s in seqs]).astype(np.float32)


def corpus_a():
    """dict: embs f16[N, 64], ids i64[N], q f32[104, 64]"""
    if "A" not in _CACHE:
        from nann_amd import synth
        embs, assign = synth.make_corpus(N, D, seed=2031)
        q = _user_means(synth.make_queries(embs, assign, B_FLAT, seq_len=L_SEQ, seed=2032))
        _CACHE["A"] = {"embs": embs, "ids": item_ids(), "q": q}
    return _CACHE["A"]


def full_a():
    """f32[104, N]: oracle.score_rows under L2 of every (query, row) of corpus A; read-only"""
    if "full_A" not in _CACHE:
        from oracle import oracle as O
        a = corpus_a()
        osc = O.Scorer("l2", D, O.EMB_F16)
        full = np.empty((B_FLAT, N), np.float32)

        def one(i):
            rc, s = O.score_rows(osc, a["q"][i], a["embs"])
            assert rc == 0
            full[i] = s

        pmap(one, range(B_FLAT))
        full.setflags(write=False)
        _CACHE["full_A"] = full
    return _CACHE["full_A"]


def filter_a():
    """(deny bool[N] over about half the rows, 104 exclusion lists of 0 .. 300 rows): query i's list holds every third of its
    best 3 len_i rows -- rows its unfiltered answer is known to hold, and another query's is not -- so a list read at the wrong
    query number changes the answer"""
    if "filter_A" not in _CACHE:
        full = full_a()
        rng = np.random.default_rng(2033)
        deny = rng.random(N) < 0.5
        lens = rng.integers(0, 301, B_FLAT)
        lens[[0, 95, 96, 103]] = [300, 0, 297, 150]
        lists = pmap(lambda i: topk_rows(full[i], 3 * int(lens[i]), ~deny)[::3].astype(np.int64), range(B_FLAT))
        _CACHE["filter_A"] = (deny, lists)
    return _CACHE["filter_A"]


def filter_150():
    """a deny bitmap that leaves 150 rows"""
    deny = np.ones(N, bool)
    deny[np.random.default_rng(2034).choice(N, 150, replace=False)] = False
    return deny, None


N_LABELS = 12


def labels_a():
    """predicate dict of predicate_model: a label per row, per query a set of 1 .. 4 allowed labels that differs from its
    neighbours' (query i always allows label i % 12, so 95 | 96 | 97 and 103 differ)"""
    if "labels_A" not in _CACHE:
        rng = np.random.default_rng(2035)
        lab = rng.integers(0, N_LABELS, N).astype(np.int32)
        lists = [np.unique(np.concatenate(([i % N_LABELS], rng.integers(0, N_LABELS, int(rng.integers(0, 4)))))).astype(np.int32)
                 for i in range(B_FLAT)]
        _CACHE["labels_A"] = {"label_of_row": lab, "labels": np.concatenate(lists).astype(np.int32),
                              "label_splits": np.concatenate(([0], np.cumsum([len(l) for l in lists]))).astype(np.int64)}
    return _CACHE["labels_A"]


def label_lists(pred, n_q):
    s = pred["label_splits"]
    return [pred["labels"][s[i]:s[i + 1]] for i in range(n_q)]


# ---- grouped and multi-vector forms: 35 users x 3 vectors = 105 vectors, so user 32 (vectors 96, 97, 98) begins at the seam ------
N_USERS, N_VEC = 35, 3
VEC_MAP = tuple(range(B_FLAT)) + (102,)      # vector v is query VEC_MAP[v] of corpus A: user 34 repeats its first interest
N_GROUPS = 50


def groups_a():
    """(group_of_row i32[N]: 50 groups spread over the rows, one row in ten ungrouped; caps i32[105]: 1, 2, 3, 1, ... per vector,
    so that the caps on both sides of the seam differ)"""
    if "groups_A" not in _CACHE:
        rng = np.random.default_rng(2038)
        g = rng.integers(0, N_GROUPS, N).astype(np.int32)
        g[rng.random(N) < 0.1] = -1
        _CACHE["groups_A"] = (g, (1 + np.arange(len(VEC_MAP)) % 3).astype(np.int32))
    return _CACHE["groups_A"]


# ---- the certified sq8 search over corpus A: the numpy model's verdicts for the sampled queries -----------------------------------
SQ8_K = SQ8_FETCH = 200
SQ8_CAP = 512          # the smallest power of two that holds every sampled query's survivors (333 .. 395): all eight certified
SQ8_CAP_LOW = 200      # = fetch: none of them fits, every sampled query is left uncertified
SQ8_RANGE_CAP = 8192   # the same for the range form at range_thresholds (1 .. 5212 survivors)


def sq8_a():
    """dict over the flat SAMPLE queries (in SAMPLE order): "exact" sq8_exact_model.search_exact's Result at SQ8_CAP, "fetch"
    sq8_model.fetch's (rows, scores) at SQ8_FETCH, "range" sq8_range_model.survivors' Result at SQ8_RANGE_CAP"""
    if "sq8_A" not in _CACHE:
        import sq8_exact_model as X
        import sq8_model as M
        import sq8_range_model as R
        a, full = corpus_a(), full_a()
        sample = list(SAMPLE["flat"])
        enc = M.encode(a["embs"])
        step = (N + THREADS - 1) // THREADS
        parts = pmap(lambda s: X.row_terms(a["embs"][s], tuple(e[s] for e in enc)), [slice(i, i + step) for i in range(0, N, step)])
        terms = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
        q = a["q"][sample]
        exact = X.search_exact(q, a["embs"], "l2", SQ8_FETCH, SQ8_CAP, SQ8_K, lambda qi, rows: full[sample[qi]][rows], x_enc=enc,
                               x_terms=terms)
        q_enc = M.encode(q)
        approx = M.approx_scores(q_enc, enc, "l2")
        thr = thresholds_a()[sample]
        _CACHE["sq8_A"] = {"exact": exact, "fetch": M.fetch(approx, SQ8_FETCH), "thr": thr,
                           "range": R.survivors(approx, terms, X.row_terms(q, q_enc), thr, "l2", D, SQ8_RANGE_CAP)}
    return _CACHE["sq8_A"]


# ---- corpus B -----------------------------------------------------------------------------------------------------------------
def corpus_b():
    """dict: base f16[20000, 64], map i64[N], table f16[N, 64] = base[map], ids, seqs f16[120, 50, 64] (the attention model's
    users), q f32[120, 64] (their means: the MLP's queries; the first 104 are the IP queries)"""
    if "B" not in _CACHE:
        from nann_amd import synth
        base, assign = synth.make_corpus(N_BASE, D, n_clusters=64, noise=1.0, seed=77)
        seqs = np.ascontiguousarray(synth.make_queries(base, assign, B_MLP, seq_len=L_SEQ, seed=2037)[:, :, :64])
        mp = np.random.default_rng(2036).permutation(N) % N_BASE
        _CACHE["B"] = {"base": base, "map": mp, "table": np.ascontiguousarray(base[mp]), "ids": item_ids(), "seqs": seqs,
                       "q": _user_means(seqs)}
    return _CACHE["B"]


def mlp_weights():
    from nann_amd import synth
    return synth.make_mlp_weights(D)


def attn_weights():
    from nann_amd import synth
    return synth.make_attn_weights(D, 64)


def base_scores(kind):
    """f32[B, 20000]: the reference's score of every (query, base row) of corpus B.  kind "ip": ip_reference.ip_scores, 104
    queries; "mlp": oracle.score_rows under the MLP scorer, 120; "attn": oracle.attn_score_rows, 113 users"""
    key = ("s_base", kind)
    if key not in _CACHE:
        from oracle import oracle as O
        b = corpus_b()
        if kind == "ip":
            import ip_reference as IR
            rows = IR.widen(b["base"])
            s = pmap(lambda v: IR.ip_scores(v, rows), list(b["q"][:B_FLAT]))
        elif kind == "mlp":
            osc = O.Scorer("mlp", D, O.EMB_F16, mlp_weights())
            s = pmap(lambda v: O.score_rows(osc, v, b["base"])[1], list(b["q"]))
        else:
            am = O.AttnModel(D, 64, L_SEQ, O.EMB_F16, attn_weights())
            s = pmap(lambda u: O.attn_score_rows(am, u.astype(np.float32), b["base"])[1], list(b["seqs"][:B_ATTN]))
        s = np.stack(s).astype(np.float32)
        s.setflags(write=False)
        _CACHE[key] = s
    return _CACHE[key]


def full_b(kind, queries=None):
    """f32[len(queries), N]: s_base[q][map]"""
    s, mp = base_scores(kind), corpus_b()["map"]
    which = range(s.shape[0]) if queries is None else queries
    return np.stack([s[i][mp] for i in which])


def copies_share_bits(scores_by_row, mp=None):
    """True iff the 60 copies of every base row carry one bit pattern in scores_by_row f32[N]"""
    mp = corpus_b()["map"] if mp is None else mp
    u = np.ascontiguousarray(scores_by_row, np.float32).view(np.uint32)
    first = np.zeros(N_BASE, np.uint32)
    first[mp] = u                                  # (some copy's bits)
    return bool((first[mp] == u).all())
