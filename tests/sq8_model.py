"""numpy model of the scalar-quantised exhaustive search (include/nann_hip.h, nann_sq8 / nann_search_all_sq8): the int8 code of a
vector, the approximate score of a (query, row) pair, and the two-stage selection -- fetch by approximate score, re-rank by
exact score, both in TopKV2 order (score descending, ties -> lower row).  Every float step is ONE numpy float32 operation, as
the contract asks of the device; the integer dot products are exact (taken in float64, where sums of at most 512 products of
magnitude <= 127^2 are integers far below 2^53)."""
import numpy as np

F32 = np.float32


def widen(x):
    """rows as the device holds them -> f32, exactly: f16 / f32 arrays, or uint16 bf16 bit patterns"""
    x = np.asarray(x)
    if x.dtype == np.uint16:
        return (x.astype(np.uint32) << 16).view(np.float32)
    return x.astype(np.float32)


def encode(x):
    """x [n, d] -> (codes i8[n, d], scales f32[n], norms i32[n])"""
    x = widen(x)
    amax = np.abs(x).max(axis=1).astype(F32)
    scale = (amax / F32(127.0)).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.rint((x / scale[:, None]).astype(F32))
    c = np.where(amax[:, None] == 0, F32(0), c)
    codes = np.clip(c, -127, 127).astype(np.int8)
    norms = (codes.astype(np.int32) ** 2).sum(axis=1, dtype=np.int32)
    return codes, scale, norms


def dots(qc, xc):
    """exact integer D[q, row] = sum_j qc[q, j] xc[row, j], as int32"""
    return (qc.astype(np.float64) @ xc.astype(np.float64).T).astype(np.int32)


def approx_scores(q_enc, x_enc, metric):
    """f32[n_q, n_rows]; metric 'ip' or 'l2'"""
    qc, sq, nq = q_enc
    xc, sx, nx = x_enc
    D = dots(qc, xc).astype(F32)  # |D| < 2^24: exact
    sq, sx = sq.astype(F32), sx.astype(F32)
    if metric == "ip":
        return ((sq[:, None] * sx[None, :]).astype(F32) * D).astype(F32)
    a = ((sq * sq).astype(F32) * nq.astype(F32)).astype(F32)
    b = ((sx * sx).astype(F32) * nx.astype(F32)).astype(F32)
    c = (((F32(2.0) * sq).astype(F32)[:, None] * sx[None, :]).astype(F32) * D).astype(F32)
    return (c - (a[:, None] + b[None, :]).astype(F32)).astype(F32)


def topk(scores, k, rows=None):
    """TopKV2 over one query's scores: (rows i32[k], scores f32[k]), descending, ties -> lower row (-0 ties with +0)"""
    scores = np.asarray(scores, F32)
    rows = np.arange(scores.shape[0], dtype=np.int32) if rows is None else np.asarray(rows, np.int32)
    order = np.lexsort((rows, -scores))[:k]
    return rows[order], scores[order]


def fetch(approx, n_fetch):
    """the fetch stage for a batch: (rows i32[n_q, n_fetch], scores f32[n_q, n_fetch])"""
    out = [topk(s, n_fetch) for s in approx]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def rerank(fetch_rows, exact_of, k):
    """the result stage: exact_of(qi, rows) -> the exact f32 scores of query qi against `rows`; the k best of each query's
    fetched rows by exact score, ties -> lower ROW NUMBER -> (rows i32[n_q, k], scores f32[n_q, k])"""
    out = []
    for qi, rows in enumerate(fetch_rows):
        rows = np.sort(np.asarray(rows, np.int32))
        out.append(topk(exact_of(qi, rows), k, rows))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def search(q, x, metric, n_fetch, k, exact_of):
    """the whole call on the CPU -> (rows, scores, fetch_rows, fetch_scores)"""
    approx = approx_scores(encode(q), encode(x), metric)
    f_rows, f_scores = fetch(approx, n_fetch)
    rows, scores = rerank(f_rows, exact_of, k)
    return rows, scores, f_rows, f_scores


def exact_f64(q, x, metric):
    """a float64 restatement of the exact score, for inputs on which float64 is exact: exact_of for rerank()"""
    q64, x64 = widen(q).astype(np.float64), widen(x).astype(np.float64)

    def of(qi, rows):
        if metric == "ip":
            return (x64[rows] @ q64[qi]).astype(F32)
        return (-((x64[rows] - q64[qi]) ** 2).sum(axis=1)).astype(F32)
    return of
