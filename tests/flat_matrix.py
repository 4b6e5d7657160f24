"""The workload of the flat scorer matrix (test_flat_matrix_gpu.py) and its references, none of which come from a device: per
(d, row dtype) one table of 16 643 seeded rows (ip_reference.scaled_rows: norms that vary 16-fold) whose first 257 rows are the
small table, 17 queries that are not normalised (the inner product and L2 rank the rows differently), and two references of
both metrics --
  A, the bits: ip_reference.ip_scores / l2_scores, the canonical order of DESIGN.md 2 with a correctly rounded fma
     (test_flat_matrix_cpu.py holds l2_scores to the C oracle's L2 score, bit for bit, on this workload);
  B, float64: q @ x.T and -||q - x||^2, with the DERIVED bound every f32 score in the canonical order lies within.
Shared by the GPU matrix and the CPU test of the workload itself (test_flat_matrix_cpu.py); nothing under nann_amd/ imports it.

The bound.  A lane's partial sums 8 terms, the butterfly adds log2(d / 8) levels, L2 rounds q_k - x_k once more (two units
on the square): with n = 8 + log2(d / 8) + 2 and u = 2^-24, |score - ref64| <= n u / (1 - n u) sum_k |term_k| + n 2^-150 --
the last term is the absolute error of the operations whose result is an f32 subnormal (fl(x) = x (1 + delta) + eta,
|eta| <= 2^-150), which the rows of subnormals reach.

The edge block: every table opens with EDGE = 16 rows (edge_rows() names them): +0 and -0 rows, two rows of subnormals of the
row dtype (f32 tables: one of f16-subnormal values, one of f32 subnormals), a row with one element at BIG (the largest finite
f16; 2^56 for bf16 / f32: its square times 512 is finite), a row equal to query 0 (query 0 is that row widened: its L2 score is
+0 exactly -- `0 - sum`; a kernel that negated the sum would give -0), two bit-identical rows at query 1 rounded to the row
dtype (PAIR_L2: under L2 they are query 1's best two rows, so its k = 1 cut falls between them) and two at twice query 1
(PAIR_IP: the same under the inner product), a row alternating +0 / -0, a row at the smallest normal magnitude, a row mixing
normal and subnormal elements.  Finite values only.

Which edge rows a top-1024 of the large table can hold (EDGE_REACH) follows from the arithmetic, not from a run: a row of zeros
or subnormals scores 0 under the inner product, the median of rows drawn around the origin, and the BIG row is the farthest row
of the table from every query under L2 (a query placed next to it would score every other row near 2^32, 256 apart); PAIR_IP
lies at twice query 1, farther from it than the rows of small norm.  Those (row, metric) pairs are held to reference A through
the small table, where k = n_items returns every row.

A cut (metric, table, query, k) is DECIDED when the float64 intervals [ref - bound, ref + bound] of the k best rows lie above
those of every other row: any scores inside the bound then select the same row set.  Not every cut can be: L2 cannot tell the zero-like rows apart
(q - (+-0) = q, and the subtraction absorbs a subnormal) and they are among the nearest rows to most queries, so besides the
chosen cut other k = 1 cuts fall between equal scores of PLANTED rows -- there reference A and the row order decide (the lower
row wins), which the matrix holds the device to; check_conditions asserts that no cut falls between equal scores of other rows.

Measured with these inputs (CPU; properties of the references alone; test_flat_matrix_cpu.py prints them): decided cuts of the
170 per case (2 metrics x 17 queries x (3 + 2); the 34 k = n_items cuts hold every row): 150 .. 166; reference A against
float64, the largest ratio to the bound over the 12 cases: 0.218 (L2), 0.236 (inner product)."""
import numpy as np

import ip_reference as R

DIMS = (64, 128, 256, 512)
DTYPES = ("f16", "bf16", "f32")
CASES = tuple((d, dtype) for d in DIMS for dtype in DTYPES)
METRICS = ("l2", "ip")
SCAN_SLAB_ROWS, SCAN_ROWS, SCAN_TILE = 16384, 256, 16      # kScanSlabRows, kScanRows, kScanTileQueries of nann_scan.h
N_BIG = SCAN_SLAB_ROWS + SCAN_ROWS + 3                     # two slabs, the last workgroup partly filled
N_SMALL = SCAN_ROWS + 1                                    # one full workgroup and one row
NQ = SCAN_TILE + 1                                         # one tile of queries plus one
K_BIG, K_SMALL = (1, 200, 1024), (1, N_SMALL)
REF_A_QUERIES = (0, 15, 16)                                # the ends of the first tile and the start of the second
EDGE = 16
ROW_POS0, ROW_NEG0, ROW_SUB_A, ROW_SUB_B, ROW_BIG, ROW_Q0 = 0, 1, 2, 3, 4, 5
PAIR_L2, PAIR_IP = (6, 7), (8, 9)
ROW_ALT0, ROW_MIN_NORMAL, ROW_MIXED = 10, 11, 12
PAIR = {"l2": PAIR_L2, "ip": PAIR_IP}
CHOSEN_CUT = (1, 1)                                        # (query, k): the one cut the planted tie straddles
EDGE_REACH = {"l2": {ROW_POS0, ROW_NEG0, ROW_SUB_A, ROW_SUB_B, ROW_Q0, ROW_ALT0, ROW_MIN_NORMAL} | set(PAIR_L2),
              "ip": {ROW_BIG, ROW_Q0} | set(PAIR_L2) | set(PAIR_IP)}
# of a case's 170 cuts at least this share must be decided.  Not all can be: L2 cannot tell the zero-like rows apart (q - (+-0) = q,
# and the subtraction absorbs a subnormal), they are the nearest rows to most queries, and so up to the 2 x 17 k = 1 cuts under L2
# (a fifth of the 170) fall between equal scores -- where reference A and the row order decide, not float64
MIN_DECIDED = 0.75
SCORE_WAVES, SCORE_GRID = 4, 8192                          # wavefronts of a workgroup of k_score_*, the cap of nann_score's grid
SCORE_QUERIES = (0, 16)
CAND_ROWS = 1024                                           # kCandRows of nann_cand.h
CAND_LENGTHS = (0, 1, CAND_ROWS - 1, CAND_ROWS, CAND_ROWS + 1, 2 * CAND_ROWS + 37)
CAND_SHORT = (3, 4, 5, 6, 7, 8, 9, 3, 5, 7, 9, 4)          # a dozen lists that share a block
CAND_DUP = (len(CAND_LENGTHS) + len(CAND_SHORT), 5, 30)   # that list holds the row at position 5 once more at position 30
CAND_DUP_LEN = 40
CAND_K = 64
MMR_LDS_BYTES, MMR_STATE_BYTES, MMR_ROW_PAD = 163840, 18560, 16   # kMmrLdsBytes, kMmrStateBytes, kMmrRowPad of nann_mmr.h
MMR_MAX = 1024
MMR_SHORT, MMR_PICKS = 65, 12
U = 2.0 ** -24
ETA = 2.0 ** -150
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def lpr(d):
    return d // 8


def rows_per_block(d):
    """R: rows a workgroup of k_score_* takes per trip"""
    return SCORE_WAVES * (64 // lpr(d))


def score_counts(d):
    """row counts of the stand-alone calls: both sides of a workgroup's trip, and past the grid's cap (the stride loop iterates)"""
    r = rows_per_block(d)
    return (1, r - 1, r, r + 1, 2 * r + 1, SCORE_GRID * r + 5)


def row_bytes(d, dtype):
    return d * (4 if dtype == "f32" else 2)


def mmr_edge(d, dtype):
    """the longest list whose rows k_mmr keeps in LDS (mmr_rows_in_lds of nann_mmr.h)"""
    return (MMR_LDS_BYTES - MMR_STATE_BYTES) // (row_bytes(d, dtype) + MMR_ROW_PAD)


# ---- tables and queries -------------------------------------------------------------------------------------------------------
def _store(x, dtype):
    """f32 values in the table's format: f16 (rounded), uint16 bf16 bit patterns (truncated), f32"""
    x = np.ascontiguousarray(x, np.float32)
    return x.astype(np.float16) if dtype == "f16" else R.to_bf16_bits(x) if dtype == "bf16" else x


def big_value(dtype):
    return 65504.0 if dtype == "f16" else 2.0 ** 56


def _raw_queries(d):
    return (np.random.default_rng(977 + d).standard_normal((NQ, d)) * 1.5).astype(np.float32)


def big_element(d):
    """the element of ROW_BIG that holds BIG: the first behind d / 2 where query 1 is negative and some other query positive (the
    row is then the last under query 1's inner product, where PAIR_IP must lead, and the first under another query's)"""
    q = _raw_queries(d)
    return d // 2 + int(np.nonzero((q[1, d // 2:] < 0) & (q[2:, d // 2:] > 0).any(0))[0][0])


def queries(d, dtype):
    """f32[17, d], not normalised; query 0 is representable in the row dtype (ROW_Q0 equals it)"""
    def make():
        q = _raw_queries(d)
        q[0] = R.widen(_store(q[0], dtype))
        return q
    return _cached(("q", d, dtype), make)


def _subnormal_bits(dtype, rng, d, pattern):
    """bit patterns of a row of subnormals of the 16-bit format: random ones, or the smallest and the largest in turn"""
    top = 0x400 if dtype == "f16" else 0x80
    mag = rng.integers(1, top, d) if pattern == "random" else np.where(np.arange(d) % 2 == 0, 1, top - 1)
    return (mag | (rng.integers(0, 2, d) << 15)).astype(np.uint16)


def _edge_block(d, dtype):
    """the first EDGE rows, in the table's format"""
    rng = np.random.default_rng(31 * d + len(dtype))
    q = queries(d, dtype)
    e = rng.standard_normal((EDGE, d)).astype(np.float32)
    e[[ROW_POS0, ROW_NEG0, ROW_SUB_A, ROW_SUB_B, ROW_ALT0]] = 0.0
    e[ROW_BIG, big_element(d)] = big_value(dtype)
    e[ROW_Q0] = q[0]
    e[list(PAIR_L2)] = q[1]
    e[list(PAIR_IP)] = 2.0 * q[1]
    e[ROW_ALT0, ::16] = 0.5
    e[ROW_MIN_NORMAL] = np.where(np.arange(d) % 2 == 0, 1.0, -1.0) * (2.0 ** -14 if dtype == "f16" else 2.0 ** -126)
    s = _store(e, dtype)
    if dtype == "f32":
        b = s.view(np.uint32)
        b[ROW_NEG0] = 0x80000000
        b[ROW_ALT0, 1::2] = 0x80000000
        sub16 = R.widen(_subnormal_bits("f16", rng, d, "random").view(np.float16))   # f16 subnormals: normal numbers in f32
        sub32 = R.widen(_subnormal_bits("bf16", rng, d, "random"))                   # bf16 subnormals widen to f32 subnormals
        s[ROW_SUB_A], s[ROW_SUB_B] = sub16, sub32
        s[ROW_MIXED, ::3] = sub32[::3]
    else:
        b = s.view(np.uint16)
        b[ROW_NEG0] = 0x8000
        b[ROW_ALT0, 1::2] = 0x8000
        b[ROW_SUB_A] = _subnormal_bits(dtype, rng, d, "random")
        b[ROW_SUB_B] = _subnormal_bits(dtype, rng, d, "ends")
        b[ROW_MIXED, ::3] = _subnormal_bits(dtype, rng, d, "random")[::3]
    return s


def table(d, dtype):
    """-> (the 16 643 rows in the table's format: f16 / uint16 bf16 bits / f32, their exact f32 widening); the small table is
    the first N_SMALL rows"""
    def make():
        x = R.scaled_rows(np.random.default_rng(5 * d + 1).standard_normal((N_BIG, d)).astype(np.float32), seed=d)
        s = _store(x, dtype)
        s[:EDGE] = _edge_block(d, dtype)
        wide = R.widen(s)
        assert np.isfinite(wide).all()
        return s, wide
    return _cached(("t", d, dtype), make)


def item_ids():
    return np.arange(N_BIG, dtype=np.int64) * 7 + 3


def edge_rows(d, dtype):
    """{name: f32 row} of the edge block: what the CPU test asserts the block holds"""
    w = table(d, dtype)[1]
    return {"+0": w[ROW_POS0], "-0": w[ROW_NEG0], "subnormal a": w[ROW_SUB_A], "subnormal b": w[ROW_SUB_B], "big": w[ROW_BIG],
            "query 0": w[ROW_Q0], "pair l2": w[list(PAIR_L2)], "pair ip": w[list(PAIR_IP)], "alternating zeros": w[ROW_ALT0],
            "smallest normal": w[ROW_MIN_NORMAL], "mixed": w[ROW_MIXED]}


# ---- reference A: the bits -------------------------------------------------------------------------------------------------------
_SCORE = {"ip": R.ip_scores, "l2": R.l2_scores}


def ref_a(metric, q, rows):
    """f32[n]: the canonical order's scores of the f32 rows"""
    return _SCORE[metric](q, rows)


def ref_a_small(d, dtype, metric):
    """f32[17, 257]: every query on the small table"""
    return _cached(("a_small", d, dtype, metric),
                   lambda: np.stack([ref_a(metric, q, table(d, dtype)[1][:N_SMALL]) for q in queries(d, dtype)]))


def ref_a_big(d, dtype, metric):
    """{b: f32[16 643]}: the queries REF_A_QUERIES on the large table"""
    return _cached(("a_big", d, dtype, metric), lambda: {b: ref_a(metric, queries(d, dtype)[b], table(d, dtype)[1]) for b in REF_A_QUERIES})


def canonical(metric, q, rows, seq_lanes=False, unfused=False, rev_elems=False, rev_chunks=False, negate=False):
    """The canonical order written out once more with its steps open to replacement; with none replaced it is ref_a (the CPU
    test asserts that).  seq_lanes: the partials added lane 0 .. L - 1 in sequence; unfused: multiply, round, add; rev_elems: a
    chunk's 8 elements accumulated in reverse; rev_chunks: lane l reads the row's chunk L - 1 - l against the query's chunk l;
    negate: L2 as -sum where the order says 0 - sum."""
    q = np.asarray(q, np.float32)
    x = np.asarray(rows, np.float32).reshape(len(rows), -1, 8)
    if rev_chunks:
        x = x[:, ::-1, :]
    qq = q.reshape(-1, 8)
    acc = np.zeros(x.shape[:2], np.float32)
    for k in (range(7, -1, -1) if rev_elems else range(8)):
        a, b = np.broadcast_to(qq[:, k], acc.shape), x[:, :, k]
        if metric == "l2":
            a = b = (a - b).astype(np.float32)
        acc = ((a * b).astype(np.float32) + acc).astype(np.float32) if unfused else R.fma32(a, b, acc)
    if seq_lanes:
        s = acc[:, 0]
        for lane in range(1, acc.shape[1]):
            s = (s + acc[:, lane]).astype(np.float32)
    else:
        s = R._butterfly(acc)
    if metric == "ip":
        return s
    return (-s).astype(np.float32) if negate else (np.float32(0.0) - s).astype(np.float32)


def widen_swapped(stored):
    """16-bit rows widened as the OTHER 16-bit format: bf16 bits read as f16, f16 bits read as bf16"""
    if stored.dtype == np.uint16:
        return stored.view(np.float16).astype(np.float32)
    return R.widen(stored.view(np.uint16))


# name -> (options of canonical(); the metric computed where `metric` is asked, or None; the widening or None; the dtypes it has
# a meaning for).  A device that computed one of them must fail the matrix: the CPU test asserts that each moves the bits of
# some score of every case.
WRONG_VARIANTS = {
    "the_other_metric": ({}, {"ip": "l2", "l2": "ip"}, None, DTYPES),
    "lanes_in_sequence": ({"seq_lanes": True}, None, None, DTYPES),
    "multiply_then_add": ({"unfused": True}, None, None, DTYPES),
    "elements_reversed": ({"rev_elems": True}, None, None, DTYPES),
    "chunks_reversed": ({"rev_chunks": True}, None, None, DTYPES),
    "l2_negated_sum": ({"negate": True}, None, None, DTYPES),               # moves L2 alone: +0 -> -0 at the row equal to the query
    "bf16_widened_as_f16": ({}, None, widen_swapped, ("f16", "bf16")),     # (an f16 table: read as bf16)
}


def variant_scores(name, d, dtype, metric, b, n=N_SMALL):
    """the scores a device computing the wrong variant `name` would give query b on the first n rows"""
    opts, swap, widening, _ = WRONG_VARIANTS[name]
    stored, wide = table(d, dtype)
    rows = wide[:n] if widening is None else widening(stored[:n])
    with np.errstate(over="ignore", invalid="ignore"):
        return canonical(swap[metric] if swap else metric, queries(d, dtype)[b], rows, **opts)


# ---- reference B: float64 and the derived bound -------------------------------------------------------------------------------
def n_ops(d):
    return 8 + int(np.log2(d // 8)) + 2


def ref_b(d, dtype, metric):
    """-> (float64[17, 16 643] scores, float64[17, 16 643] bound on |f32 score in the canonical order - score|)"""
    def make():
        q = queries(d, dtype).astype(np.float64)
        x = table(d, dtype)[1].astype(np.float64)
        if metric == "ip":
            ref, mag = q @ x.T, np.abs(q) @ np.abs(x).T
        else:
            mag = np.stack([((v - x) ** 2).sum(1) for v in q])
            ref = -mag
        n = n_ops(d)
        return ref, n * U / (1.0 - n * U) * mag + n * ETA
    return _cached(("b", d, dtype, metric), make)


def order_b(d, dtype, metric, n=N_BIG):
    """i64[17, n]: the rows of the table's first n in TopKV2 order of reference B (ties -> the lower row)"""
    def make():
        ref = ref_b(d, dtype, metric)[0][:, :n]
        return np.stack([np.lexsort((np.arange(n), -r)) for r in ref])
    return _cached(("order", d, dtype, metric, n), make)


def ratio_to_bound(got, ref, bound):
    """the largest |got - ref| / bound (0 where both vanish)"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    return float(np.max(err / bound)) if err.size else 0.0


def decided(d, dtype):
    """{(metric, n_rows, k): bool[17]}: the cuts of the scan's calls whose row set any scores within the bound select"""
    def make():
        out = {}
        for metric in METRICS:
            ref, bound = ref_b(d, dtype, metric)
            for n, ks in ((N_BIG, K_BIG), (N_SMALL, K_SMALL)):
                order = order_b(d, dtype, metric, n)
                lo, hi = (ref - bound)[:, :n], (ref + bound)[:, :n]
                for k in ks:
                    out[(metric, n, k)] = np.asarray([k == n or lo[b][order[b, :k]].min() > hi[b][order[b, k:]].max() for b in range(NQ)])
        return out
    return _cached(("decided", d, dtype), make)


def check_conditions(d, dtype):
    """What the case's inputs must satisfy for a pass to mean something, asserted on the references alone -> the number of
    decided cuts.  (1) the inner product and L2 disagree on every query's best 200 rows; (2) at least MIN_DECIDED of the cuts
    are decided; (3) every (row, metric) of EDGE_REACH lies in some query's best 1024 of the large table; (4) the planted
    pair is the best two rows of query 1 under its metric, so the k = 1 cut falls between two equal scores and the lower row
    wins it; on the large table a pair straddles no other cut of any query; and in reference A a cut of the scan's calls falls
    between equal scores only where both rows are planted ones (the pairs, and the zero-like rows under L2), where
    topk_stable gives the lower row."""
    for b in range(NQ):
        assert set(order_b(d, dtype, "ip")[b, :200].tolist()) != set(order_b(d, dtype, "l2")[b, :200].tolist()), (d, dtype, b, "L2 ranks like IP")
    dec = decided(d, dtype)
    n_dec = sum(int(v.sum()) for v in dec.values())
    assert n_dec >= MIN_DECIDED * NQ * len(dec), (d, dtype, "too few decided cuts", n_dec)
    for metric in METRICS:
        reached = set(np.unique(order_b(d, dtype, metric)[:, :K_BIG[-1]]).tolist()) & set(range(EDGE))
        assert EDGE_REACH[metric] <= reached, (d, dtype, metric, "edge rows outside every best 1024", sorted(EDGE_REACH[metric] - reached))
        lo, hi = PAIR[metric]
        qb, qk = CHOSEN_CUT
        small = ref_a_small(d, dtype, metric)
        assert R.topk_stable(small[qb], 2).tolist() == [lo, hi] and small[qb, lo].view(np.uint32) == small[qb, hi].view(np.uint32), (d, dtype, metric, "the pair")
        assert order_b(d, dtype, metric)[qb, :2].tolist() == [lo, hi] and not dec[(metric, N_BIG, qk)][qb] and not dec[(metric, N_SMALL, qk)][qb]
        for p in (PAIR_L2, PAIR_IP):   # on the large table, by float64: a pair straddles no other cut of any query
            for b in range(NQ):
                rank = int(np.nonzero(order_b(d, dtype, metric)[b] == p[0])[0][0])
                assert order_b(d, dtype, metric)[b, rank + 1] == p[1] and (rank + 1 not in K_BIG or (b, rank + 1, p) == (qb, qk, PAIR[metric])), (d, dtype, metric, b, rank)
        cuts = [(small[b], k, b) for b in range(NQ) for k in K_SMALL if k < N_SMALL]
        cuts += [(s, k, b) for b, s in ref_a_big(d, dtype, metric).items() for k in K_BIG]
        for s, k, b in cuts:
            top = R.topk_stable(s, k + 1)
            tie = (s[top[k - 1]] + np.float32(0.0)).view(np.uint32) == (s[top[k]] + np.float32(0.0)).view(np.uint32)
            assert not tie or max(top[k - 1], top[k]) < EDGE, (d, dtype, metric, b, k, "a cut between equal scores of rows that were not planted")
            assert (b, k) != CHOSEN_CUT or (tie and (top[k - 1], top[k]) == (lo, hi)), (d, dtype, metric, "the chosen cut does not straddle the pair")
    return n_dec


# ---- candidate lists ------------------------------------------------------------------------------------------------------------
def candidate_lists(d, dtype):
    """-> (19 ragged lists of rows of the large table (i32), the query of each): CAND_LENGTHS, a dozen short lists, and one
    that holds a row twice.  A list's first half is drawn from its query's best 1024 under either metric (so that the scan
    returns some of its rows), the rest from the whole table; the long lists open with the edge block."""
    def make():
        rng = np.random.default_rng(41 + d)
        lengths = CAND_LENGTHS + CAND_SHORT + (CAND_DUP_LEN,)
        users = np.arange(len(lengths)) % NQ
        lists = []
        for i, n in enumerate(lengths):
            near = np.concatenate([order_b(d, dtype, m)[users[i], :K_BIG[-1]] for m in METRICS])
            li = np.concatenate([rng.choice(near, n // 2), rng.integers(0, N_BIG, n - n // 2)]).astype(np.int32)
            if n >= 2 * EDGE:
                li[:EDGE] = np.arange(EDGE)
            lists.append(rng.permutation(li) if n < CAND_ROWS else li)
        i, first, second = CAND_DUP   # distinct rows that are not planted ones, but for the one listed twice
        near = np.setdiff1d(order_b(d, dtype, "l2")[users[i], :K_BIG[-1]], np.arange(EDGE))
        far = np.setdiff1d(np.arange(EDGE, N_BIG), near)
        lists[i] = rng.permutation(np.concatenate([rng.choice(near, CAND_DUP_LEN // 2, replace=False),
                                                   rng.choice(far, CAND_DUP_LEN - CAND_DUP_LEN // 2, replace=False)])).astype(np.int32)
        lists[i][second] = lists[i][first]
        return lists, users
    return _cached(("lists", d, dtype), make)


def list_scores(d, dtype, metric):
    """reference A of every list: [f32[len]]"""
    def make():
        lists, users = candidate_lists(d, dtype)
        wide = table(d, dtype)[1]
        return [ref_a(metric, queries(d, dtype)[b], wide[li]) if len(li) else np.zeros(0, np.float32) for li, b in zip(lists, users)]
    return _cached(("list_a", d, dtype, metric), make)


# ---- MMR lists ------------------------------------------------------------------------------------------------------------------
def mmr_calls(d, dtype):
    """[(k_in, rows i32[2, k_in], scores f32[2, k_in], k, lambda)]: the longest list whose rows stay in LDS, the list one longer
    (the table path), and a list of 65 picked to its end, once at lambda 0.  Unranked lists (random scores: every position can be
    the next pick); every list holds the two bit-identical rows of PAIR_L2."""
    def make():
        edge = mmr_edge(d, dtype)
        assert MMR_SHORT < edge < MMR_MAX
        rng = np.random.default_rng(7 * d + len(dtype))
        calls = []
        for k_in, k, lam in ((edge, MMR_PICKS, 0.5), (min(edge + 1, MMR_MAX), MMR_PICKS, 0.5), (MMR_SHORT, MMR_SHORT, 0.5), (MMR_SHORT, MMR_SHORT, 0.0)):
            rows = rng.integers(0, N_BIG, (2, k_in)).astype(np.int32)
            rows[:, 3], rows[:, k_in - 2] = PAIR_L2
            rows[1, :EDGE] = rng.permutation(EDGE)
            calls.append((k_in, rows, rng.standard_normal((2, k_in)).astype(np.float32), k, lam))
        return calls
    return _cached(("mmr", d, dtype), make)


def mmr_expected(d, dtype, sim):
    """mmr_model.model of every call of mmr_calls under the similarity `sim`"""
    import mmr_model as MM

    def make():
        stored = table(d, dtype)[0]
        return [MM.model(scores, rows, None, stored, lam, sim, k, item_ids=item_ids()) for _, rows, scores, k, lam in mmr_calls(d, dtype)]
    return _cached(("mmr_exp", d, dtype, sim), make)


def references(d, dtype):
    """everything the GPU case compares with, computed (and cached) in one place -> the number of decided cuts"""
    n_dec = check_conditions(d, dtype)
    for metric in METRICS:
        list_scores(d, dtype, metric)
        mmr_expected(d, dtype, metric)
    return n_dec
