"""A numpy restatement of the wide selection (csrc/nann_wide.h), step for step: digit passes on score_key, the cut, the quota,
the gather in row order, the composite sort.  `variant` switches in one of the wrong forms the tests show to move a result:
"no_quota" (every row at the cut is taken), "ties_desc" (ties to the HIGHER row), "neg_zero_below" (-0 keyed below +0)."""
import numpy as np

PASSES = ((21, 11), (10, 11), (0, 10))  # (shift, bits) of the three digits, most significant first
MAX_K = 16384


def score_key(s, variant=None):
    """nann_device.h score_key: s + 0.0f folds -0 into +0, then the order-preserving map f32 -> u32"""
    s = np.asarray(s, np.float32)
    if variant != "neg_zero_below":
        s = s + np.float32(0.0)
    u = s.view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def cut(keys, k):
    """(T, n_gt, m) of the valid rows' keys, n_valid > k >= 1: three histogram passes, each followed by the pick of the bin, from
    the top, in which the remaining rank falls"""
    prefix, rank, n_gt = np.uint32(0), int(k), 0
    for shift, nbits in PASSES:
        hi = shift + nbits
        match = keys if hi == 32 else keys[(keys >> np.uint32(hi)) == (prefix >> np.uint32(hi))]
        hist = np.bincount(((match >> np.uint32(shift)) & np.uint32((1 << nbits) - 1)).astype(np.int64), minlength=1 << nbits)
        above = 0
        for b in range((1 << nbits) - 1, -1, -1):
            if above + hist[b] >= rank:
                break
            above += int(hist[b])
        prefix = np.uint32(prefix | np.uint32(b << shift))
        rank -= above
        n_gt += above
    return prefix, n_gt, k - n_gt


def select(scores, k, variant=None):
    """One row of scores -> (values f32[k], indices i32[k], n_out): zeros behind n_out"""
    scores = np.asarray(scores, np.float32)
    assert 0 <= k <= min(MAX_K, scores.shape[0])
    out_v, out_i = np.zeros(k, np.float32), np.zeros(k, np.int32)
    valid = scores != -np.inf
    n_valid = int(valid.sum())
    if k == 0:
        return out_v, out_i, 0
    keys = score_key(scores, variant)
    if n_valid <= k:
        T, m = np.uint32(0), k
    else:
        T, n_gt, m = cut(keys[valid], k)
        assert n_gt == int((valid & (keys > T)).sum()) and 1 <= m <= int((valid & (keys == T)).sum())
    gt, eq = valid & (keys > T), valid & (keys == T)
    eq_before = np.cumsum(eq) - eq
    taken = gt | (eq if variant == "no_quota" else eq & (eq_before < m))
    rows = np.flatnonzero(taken)[:k]                       # the gather: ascending row order, every store guarded by pos < k
    low = rows.astype(np.uint32) if variant == "ties_desc" else ~rows.astype(np.uint32)
    comp = (keys[rows].astype(np.uint64) << np.uint64(32)) | low.astype(np.uint64)
    rows = rows[np.argsort(comp)[::-1]]                    # the composites are distinct: any sort gives this order
    n_out = min(k, n_valid)
    out_i[:len(rows)] = rows
    out_v[:len(rows)] = scores[rows]                       # the original bits, not the key's
    return out_v, out_i, n_out


def reference(scores, k):
    """The contract, by np.lexsort: the rows that are not -inf by (score descending -- -0 and +0 equal --, row ascending)"""
    scores = np.asarray(scores, np.float32)
    rows = np.flatnonzero(scores != -np.inf)
    order = rows[np.lexsort((rows, -(scores[rows] + np.float32(0.0)).astype(np.float64)))][:k]
    out_v, out_i = np.zeros(k, np.float32), np.zeros(k, np.int32)
    out_v[:len(order)] = scores[order]
    out_i[:len(order)] = order
    return out_v, out_i, len(order)
