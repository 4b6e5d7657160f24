"""numpy model of the certified scalar-quantised RANGE search (include/nann_hip.h, nann_search_all_range_sq8_exact; DESIGN.md
4.22), shared by test_sq8_range_cpu.py and test_sq8_range_gpu.py; nothing under nann_amd/ imports it.  Built on sq8_model (the
codes and the approximate score), sq8_exact_model (row_terms, query_terms, survives: the device's f32 steps, one numpy operation
each) and range_model (the match rule and the ragged outputs).  The cut of the survivor predicate is the caller's threshold; no
tolerance appears anywhere."""
import numpy as np

import range_model as RM
import sq8_exact_model as X
import sq8_model as M

F32 = np.float32
CHUNK = RM.CHUNK


def rows_like(n, d, seed, dtype="f16"):
    """test_sq8_exact_gpu._rows' recipe, restated: Gaussian rows, every row at a magnitude of its own (e^-2 .. e^2)"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, d)) * np.exp(rng.uniform(-2.0, 2.0, (n, 1)))).astype(F32)
    if dtype == "f16":
        return x.astype(np.float16)
    return (x.view(np.uint32) >> 16).astype(np.uint16)


def queries_like(d, n_q, seed=0):
    q = np.random.default_rng(seed + d).standard_normal((n_q, d)).astype(F32)
    if n_q > 5:
        q[5] *= F32(0.01)
    return q


class Result:
    """keep bool[n_q, n]: the survivor predicate at tau = thr; n_survivors i64[n_q] and certified bool[n_q] as the device
    reports them; above bool[n_q]: the L2 rule for a finite threshold above +0"""

    def __init__(self, keep, n_survivors, certified, above):
        self.keep, self.n_survivors, self.certified, self.above = keep, n_survivors, certified, above


def survivors(approx, x_terms, q_terms, thr, metric, d, cap):
    """approx f32[n_q, n]; x_terms = (err, xhat) of the rows; q_terms = (eq, qhat) of the queries; thr f32[n_q]"""
    thr = np.asarray(thr, F32)
    err, xhat = x_terms
    eq, qhat = q_terms
    n = approx.shape[1]
    w, ok = X.query_terms(thr, eq, qhat, metric, d)
    keep = X.survives(approx, err, xhat, thr, eq, qhat, w, metric, d)
    with np.errstate(invalid="ignore"):
        finite = (np.abs(thr) <= X.FLT_MAX) & (np.abs(eq) <= X.FLT_MAX) & (np.abs(qhat) <= X.FLT_MAX)
        above = finite & (thr > 0) if metric == "l2" else np.zeros(len(thr), bool)
    n_surv = np.where(above, 0, keep.sum(axis=1))
    certified = above | (ok & (n_surv <= min(cap, n)))
    return Result(keep, n_surv, certified, above)


def search_range(approx, exact, x_terms, q_terms, thr, metric, d, cap, item_ids, capacity):
    """the whole call: -> (Result, (row_splits, index, scores, item_ids) as range_model.reference gives them).  exact f32[n_q, n]:
    the exact scores, of which only the survivors' are read.  A certified query's segment: its survivors that match the threshold;
    an uncertified query's: empty."""
    thr = np.asarray(thr, F32)
    r = survivors(approx, x_terms, q_terms, thr, metric, d, cap)
    b, n = approx.shape
    segs = []
    for i in range(b):
        rows = np.flatnonzero(r.keep[i]) if r.certified[i] and not r.above[i] else np.zeros(0, np.int64)
        segs.append(rows[RM.match(exact[i, rows], thr[i])])
    splits = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    out_index, out_scores, out_ids = RM._outputs(capacity)
    flat = np.concatenate(segs) if b else np.zeros(0, np.int64)
    flat_scores = np.concatenate([exact[i, segs[i]] for i in range(b)]) if b else np.zeros(0, F32)
    m = min(capacity, len(flat))
    out_index[:m], out_scores[:m], out_ids[:m] = flat[:m], flat_scores[:m], item_ids[flat[:m]]
    return r, (splits, out_index, out_scores, out_ids)


def segments(res):
    """(row_splits, index, scores, item_ids) -> per query (index, score bits, item_ids); for results that were not truncated"""
    splits, index, scores, ids = res
    return [(index[splits[i]:splits[i + 1]], scores[splits[i]:splits[i + 1]].view(np.uint32), ids[splits[i]:splits[i + 1]])
            for i in range(len(splits) - 1)]


# ---- the cases test_sq8_range_gpu.py runs, stated here so that test_sq8_range_cpu.py can hold them against the model's cap -----
GPU_SHAPES = [(n, d, dtype) for n in (1007, 2051) for d in (64, 128, 512) for dtype in ("f16", "bf16")]
GPU_QUERIES = 130   # two chunks: 128 + 2
GPU_CAP = 512    # below both n: the cap, not the corpus, bounds a certified list
GPU_SMALL_CAP = 64  # the case meant to overflow: below the survivor count of a threshold at the 300th score


def gpu_case(n, d, dtype):
    """(rows, queries): rows 11 and n - 2 are copies of row 400 and query 4 lies next to it, so that a threshold at that row's
    score is a threshold at a tie of three near the head of the query's ranking"""
    x = rows_like(n, d, n + d, dtype)
    x[11] = x[400]
    x[n - 2] = x[400]
    q = queries_like(d, GPU_QUERIES, seed=d)
    q[4] = M.widen(x[400:401])[0] * F32(1.25) + np.random.default_rng(n).standard_normal(d).astype(F32) * F32(0.01)
    return x, q


def case_thresholds(exact, metric):
    """the thresholds of a GPU case from the exact scores [130, n]: cycled, query 4 at the score of the tied rows, and under L2
    queries 8 and 12 at +0 and -0"""
    thr = cycle_thresholds(exact)
    thr[4] = exact[4, 400]
    if metric == "l2":
        thr[8], thr[12] = F32(0.0), F32(-0.0)
    return thr


def threshold_of(scores, pick):
    """of one query's exact scores: pick 0 the best, 1 the 37th, 2 the 300th score, 3 the midpoint of the 10th and the 11th"""
    s = np.sort(scores)[::-1]
    return [s[0], s[36], s[299], F32((np.float64(s[9]) + np.float64(s[10])) / 2)][pick]


def cycle_thresholds(exact):
    """per query, cycled: threshold_of at pick 0, 1, 2, 3"""
    return np.array([threshold_of(exact[i], i % 4) for i in range(exact.shape[0])], F32)


def exact_f64_all(q, x, metric):
    """[n_q, n] f32: sq8_model.exact_f64's score for every row"""
    of = M.exact_f64(q, x, metric)
    rows = np.arange(np.asarray(x).shape[0])
    return np.stack([of(i, rows) for i in range(q.shape[0])])
