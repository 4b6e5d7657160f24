"""numpy model of the certified scalar-quantised search (include/nann_hip.h, nann_sq8_bounds / nann_search_all_sq8_exact;
DESIGN.md 4.21): the per-row error terms, the per-query terms, the survivor predicate and the three-stage call.  Every float
step of the device is ONE numpy float32 operation here, in the device's order, so that the terms and the predicate can be held
against the device bit for bit.  real_terms() and upper_bound() restate in float64 the real-valued quantities the bound covers;
they are what the soundness tests compare with, not what the device computes."""
import numpy as np

import sq8_model as M

F32 = np.float32
INFL = F32(1.0) + F32(2.0 ** -18)    # kSq8Infl
INFL2 = F32(1.0) + F32(2.0 ** -20)   # kSq8Infl2
ABS = F32(2.0 ** -60)                # kSq8Abs
TINY = F32(2.0 ** -100)              # kSq8Tiny
FLT_MAX = F32(3.402823466e+38)
_LANES = np.arange(64)


def gamma(d):
    """G = (d + 4) 2^-24 (exact in f32): >= the relative error of an f32 accumulation of d terms behind one subtraction each"""
    return F32(d + 4) * F32(2.0 ** -24)


def row_terms(x, enc):
    """(err f32[n], xhat f32[n]) of vectors x [n, d] and their code enc = (codes, scales, norms): k_sq8_row_err's steps.  Lane l
    of a row's wavefront takes elements l, l + 64, ... in order; the lanes' sums meet in the xor butterfly 32, 16, .., 1."""
    x = M.widen(x)
    codes, scale, norms = enc
    n, d = x.shape
    scale = scale.astype(F32)
    acc = np.zeros((n, 64), F32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for i in range(d // 64):
            sl = slice(i * 64, (i + 1) * 64)
            p = scale[:, None] * codes[:, sl].astype(F32)
            r = x[:, sl] - p
            acc = acc + r * r
        for o in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, _LANES ^ o]
        e0 = np.sqrt(acc[:, 0])
        xhat = (scale * np.sqrt(norms.astype(F32))) * INFL + ABS
        err = (e0 + F32(2.0 ** -23) * xhat) * INFL + ABS
    return err.astype(F32), xhat.astype(F32)


def real_terms(x, enc):
    """float64: (|x_i - scale_i codes_i|, scale_i sqrt(norm_i)), the quantities err and xhat bound from above"""
    x64 = M.widen(x).astype(np.float64)
    codes, scale, norms = enc
    xq = scale.astype(np.float64)[:, None] * codes.astype(np.float64)
    return np.sqrt(((x64 - xq) ** 2).sum(axis=1)), scale.astype(np.float64) * np.sqrt(norms.astype(np.float64))


def query_terms(tau, eq, qhat, metric, d):
    """k_sq8_exact_terms: tau, eq, qhat f32[n_q] -> (w f32[n_q], ok bool[n_q])"""
    tau, eq, qhat = np.asarray(tau, F32), np.asarray(eq, F32), np.asarray(qhat, F32)
    g = gamma(d)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        ok = (np.abs(tau) <= FLT_MAX) & (np.abs(eq) <= FLT_MAX) & (np.abs(qhat) <= FLT_MAX)
        if metric == "l2":
            ok &= tau <= 0
            t2 = (-tau + TINY) * (F32(1.0) + F32(2.0) * g)
            rho = np.sqrt(t2) * INFL2
            w = (rho + eq) * INFL2
        else:
            w = (qhat + eq) * INFL2
    return w.astype(F32), ok


def survives(a, err, xhat, tau, eq, qhat, w, metric, d):
    """sq8_survives for a [n_q, n] against the rows' err, xhat [n] and the queries' terms [n_q] -> bool[n_q, n].  False only where
    the exact f32 score of the row is provably below tau; a NaN anywhere keeps the row."""
    a = np.asarray(a, F32)
    err, xhat = np.asarray(err, F32)[None, :], np.asarray(xhat, F32)[None, :]
    tau, eq, qhat, w = (np.asarray(v, F32)[:, None] for v in (tau, eq, qhat, w))
    g = gamma(d)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        finite = np.abs(a) <= FLT_MAX
        if metric == "l2":
            ww = qhat + xhat
            dl = (ww * ww) * F32(2.0 ** -20) + TINY
            lo = -a - dl
            s = w + err
            hi = (s * s) * INFL
            keep = ~(lo > hi)
        else:
            cross = (eq * xhat + err * qhat) + eq * err
            gt = g * (w * (xhat + err))
            p = ((cross + gt) + F32(2.0 ** -22) * np.abs(a)) + TINY
            ub = a + p * INFL
            keep = ~(ub < tau)
    return keep | ~finite


def upper_bound(a, err, xhat, eq, qhat, metric, d):
    """float64 [n_q, n]: an upper bound of the exact f32 score of every (query, row) from the approximate score and the error
    terms alone -- what the predicate compares with tau, restated without the cut.  L2: -((1 - G) max(0, sqrt(lo) - delta)^2 -
    tiny) with lo the predicate's lower bound of |qhat_vec - xhat_vec|^2; IP: the predicate's ub."""
    a = np.asarray(a, F32)
    err, xhat = np.asarray(err, F32)[None, :], np.asarray(xhat, F32)[None, :]
    eq, qhat = np.asarray(eq, F32)[:, None], np.asarray(qhat, F32)[:, None]
    g = gamma(d)
    if metric == "l2":
        ww = qhat + xhat
        lo = (-a - ((ww * ww) * F32(2.0 ** -20) + TINY)).astype(np.float64)
        delta = eq.astype(np.float64) + err.astype(np.float64)
        r = np.maximum(0.0, np.sqrt(np.maximum(lo, 0.0)) * (1.0 - 2.0 ** -24) - delta)
        return -((1.0 - float(g)) * r * r - float(TINY))
    w = (qhat + eq) * INFL2
    cross = (eq * xhat + err * qhat) + eq * err
    p = ((cross + g * (w * (xhat + err))) + F32(2.0 ** -22) * np.abs(a)) + TINY
    return (a + p * INFL).astype(np.float64)


class Result:
    """rows i32[n_q, k], scores f32[n_q, k], certified bool[n_q], n_survivors i64[n_q], lists: the final row list of every
    query (ascending), tau f32[n_q]"""

    def __init__(self, rows, scores, certified, n_survivors, lists, tau):
        self.rows, self.scores, self.certified, self.n_survivors, self.lists, self.tau = rows, scores, certified, n_survivors, lists, tau


def search_exact(q, x, metric, n_fetch, cap, k, exact_of, x_enc=None, x_terms=None):
    """the whole certified call on the CPU.  exact_of(qi, rows) -> the exact f32 scores, as sq8_model.rerank takes it.
    (a) fetch + exact re-rank at n_fetch, tau = the k-th exact score; (b) the survivors of every row; (c) certified = terms
    finite and count <= cap; the final list is the survivors, else the sorted fetch list; its exact top k is the result."""
    q = np.asarray(q, F32)
    d = q.shape[1]
    x_enc = M.encode(x) if x_enc is None else x_enc
    err, xhat = row_terms(x, x_enc) if x_terms is None else x_terms
    q_enc = M.encode(q)
    approx = M.approx_scores(q_enc, x_enc, metric)
    f_rows, _ = M.fetch(approx, n_fetch)
    a_rows, a_scores = M.rerank(f_rows, exact_of, k)
    tau = a_scores[:, k - 1].astype(F32)
    eq, qhat = row_terms(q, q_enc)
    w, ok = query_terms(tau, eq, qhat, metric, d)
    keep = survives(approx, err, xhat, tau, eq, qhat, w, metric, d)
    n_surv = keep.sum(axis=1)
    certified = ok & (n_surv <= min(cap, x_enc[0].shape[0]))
    lists = [np.flatnonzero(keep[i]).astype(np.int32) if certified[i] else np.sort(f_rows[i]).astype(np.int32) for i in range(len(q))]
    out = [M.topk(exact_of(i, rows), k, rows) for i, rows in enumerate(lists)]
    return Result(np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), certified, n_surv, lists, tau)
