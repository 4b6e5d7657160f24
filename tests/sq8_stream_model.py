"""numpy model of the streamed scalar-quantised search (include/nann_hip.h, nann_search_all_sq8_stream) on top of sq8_model: the
cut from a sample of the table, the survivors of the whole table in row order, and the exact re-rank of the kept survivors."""
import numpy as np

import sq8_model as M


def n_sample(sample_rows, fetch, n_items):
    want = sample_rows if sample_rows > 0 else max(65536, -(-n_items // 16))
    return min(max(want, fetch), n_items)


def cut(approx, n_sample, fetch):
    """tau f32[n_q]: the fetch-th largest approximate score among the rows [0, n_sample)"""
    return np.stack([M.topk(s[:n_sample], fetch)[1][fetch - 1] for s in approx])


def survivors(approx, cut, cap):
    """per query (rows i32 ascending with a >= tau, truncated to the first cap), and n_survivors i32[n_q], the true counts"""
    full = [np.flatnonzero(s >= t).astype(np.int32) for s, t in zip(approx, cut)]
    return [r[:cap] for r in full], np.array([len(r) for r in full], np.int32)


def search(approx, sample_rows, fetch, cap, k, exact_of):
    """the whole call from the approximate scores f32[n_q, n_items] -> (rows i32[n_q, k], scores f32[n_q, k], complete, n_survivors,
    cut); exact_of(qi, rows) -> the exact f32 scores, as sq8_model.rerank takes it"""
    n_items = approx.shape[1]
    tau = cut(approx, n_sample(sample_rows, fetch, n_items), fetch)
    kept, n_surv = survivors(approx, tau, min(cap, n_items))
    rows, scores = M.rerank(kept, exact_of, k)
    return rows, scores, (n_surv <= min(cap, n_items)).astype(np.int32), n_surv, tau
