"""The numpy model of nann_user_seq_interests (include/nann_hip.h): one behaviour sequence -> up to n_vec interest vectors, their
weights and the slot of every history row.  Every value is an np.float32 and every step one f32 operation, in the order the
header gives: the k loop of a distance and the r loop of a sum are explicit chains from +0.  `model` takes a batch and is
vectorised over what the contract leaves unordered (the rows of a distance pass, the columns of a sum); `restate` is the same
contract for one user in plain Python loops over scalars, written from the header alone."""
import numpy as np

F = np.float32
MAX_VEC = 16   # NANN_INTERESTS_MAX_VEC
MAX_ITER = 32  # NANN_INTERESTS_MAX_ITER


def _dist(x, c):
    """dist(r, c) of every row of x f32[n, d]: k ascending from +0, t = x - c, acc = acc + t * t"""
    acc = np.zeros(x.shape[0], F)
    for k in range(x.shape[1]):
        t = x[:, k] - c[k]
        acc = acc + t * t
    return acc


def _sum_rows(x, rows):
    """per column, acc from +0 over `rows` in ascending order"""
    acc = np.zeros(x.shape[1], F)
    for r in rows:
        acc = acc + x[r]
    return acc


def _argmax_low(v):
    """(index, value) of the greatest value, ties to the lowest index"""
    i = int(np.argmax(v))  # numpy returns the first of equal maxima
    return i, v[i]


def user(bits, n_vec, n_iter, trace=None):
    """one user: bits u16[L, d] -> (q f32[n_vec, d], weights f32[n_vec], n_interests, assign i32[L]).  trace, a dict or None,
    counts what happened on the way (tests)"""
    L, d = bits.shape
    x = bits.view(np.float16).astype(F)
    live = np.flatnonzero(((bits & 0x7FFF) != 0).any(axis=1))  # non-pad rows, ascending
    m = len(live)
    q, w, assign = np.zeros((n_vec, d), F), np.zeros(n_vec, F), np.full(L, -1, np.int32)
    if m == 0:
        return q, w, 0, assign
    xl = x[live]
    mean = _sum_rows(x, live) / F(m)
    # ---- seeds
    if n_vec == 1:
        cent = [mean]  # the one interest is the mean itself
    else:
        dm = _dist(xl, mean)
        s, _ = _argmax_low(dm)
        if trace is not None:
            trace["seed_tie"] = trace.get("seed_tie", 0) + int((dm == dm[s]).sum() > 1)
        cent = [xl[s].copy()]
        mind = np.full(m, np.inf, F)
        while len(cent) < n_vec:
            mind = np.minimum(mind, _dist(xl, cent[-1]))
            s, v = _argmax_low(mind)
            if v == 0:
                break
            if trace is not None:
                trace["seed_tie"] = trace.get("seed_tie", 0) + int((mind == v).sum() > 1)
            cent.append(xl[s].copy())
    n_c = len(cent)

    def assign_pass():
        dd = np.stack([_dist(xl, c) for c in cent])  # [n_c, m]
        a = np.argmin(dd, axis=0)                    # the first of equal minima: the lowest cluster
        if trace is not None:
            trace["assign_tie"] = trace.get("assign_tie", 0) + int(((dd == dd.min(axis=0)).sum(axis=0) > 1).any())
        return a

    # ---- Lloyd rounds
    for _ in range(n_iter):
        a = assign_pass()
        for c in range(n_c):
            mem = live[a == c]
            if len(mem):
                cent[c] = _sum_rows(x, mem) / F(len(mem))
            elif trace is not None:
                trace["emptied"] = trace.get("emptied", 0) + 1
    # ---- final assignment, order, padding
    a = assign_pass()
    count = np.bincount(a, minlength=n_c)
    order = sorted((c for c in range(n_c) if count[c]), key=lambda c: (-count[c], c))
    if trace is not None:
        trace["dropped"] = trace.get("dropped", 0) + int(len(order) < n_c)
        trace["reordered"] = trace.get("reordered", 0) + int(order != list(range(len(order))))
    slot = np.full(n_c, -1, np.int32)
    for s, c in enumerate(order):
        slot[c] = s
        q[s] = cent[c]
        w[s] = F(count[c]) / F(m)
    q[len(order):] = q[0]
    assign[live] = slot[a]
    return q, w, len(order), assign


def model(comm_seq_f16_bits, n_vec, n_iter, trace=None):
    """comm_seq_f16_bits u16[n_users, L, d] (the f16 bit patterns) -> dict(q f32[n_users, n_vec, d], weights f32[n_users, n_vec],
    n_interests i32[n_users], assign i32[n_users, L])"""
    bits = np.ascontiguousarray(comm_seq_f16_bits).view(np.uint16)
    assert bits.ndim == 3 and 1 <= n_vec <= MAX_VEC and 0 <= n_iter <= MAX_ITER
    n, L, d = bits.shape
    out = dict(q=np.zeros((n, n_vec, d), F), weights=np.zeros((n, n_vec), F), n_interests=np.zeros(n, np.int32),
               assign=np.full((n, L), -1, np.int32))
    for u in range(n):
        out["q"][u], out["weights"][u], out["n_interests"][u], out["assign"][u] = user(bits[u], n_vec, n_iter, trace)
    return out


def restate(rows, n_vec, n_iter):
    """The contract once more for one user, scalars and lists only: rows is a list of L lists of d np.float16 values.
    -> (q: n_vec lists of d np.float32, weights: n_vec np.float32, n_interests, assign: L ints)"""
    L, d = len(rows), len(rows[0])
    x = [[F(h) for h in row] for row in rows]
    live = [r for r in range(L) if any(float(h) != 0.0 for h in rows[r])]  # +-0 compare equal to 0
    m = len(live)
    if m == 0:
        return [[F(0)] * d for _ in range(n_vec)], [F(0)] * n_vec, 0, [-1] * L

    def dist(r, c):
        acc = F(0)
        for k in range(d):
            t = F(x[r][k] - c[k])
            acc = F(acc + F(t * t))
        return acc

    def centre(mem):
        out = []
        for k in range(d):
            acc = F(0)
            for r in mem:
                acc = F(acc + x[r][k])
            out.append(F(acc / F(len(mem))))
        return out

    mean = centre(live)
    if n_vec == 1:
        cent = [mean]
    else:
        best, at = None, None
        for r in live:
            v = dist(r, mean)
            if best is None or v > best:
                best, at = v, r
        cent = [list(x[at])]
        while len(cent) < n_vec:
            best, at = None, None
            for r in live:
                v = min(dist(r, c) for c in cent)
                if best is None or v > best:
                    best, at = v, r
            if best == 0:
                break
            cent.append(list(x[at]))

    def nearest(r):
        best, at = None, None
        for c in range(len(cent)):
            v = dist(r, cent[c])
            if best is None or v < best:
                best, at = v, c
        return at

    for _ in range(n_iter):
        a = {r: nearest(r) for r in live}
        for c in range(len(cent)):
            mem = [r for r in live if a[r] == c]
            if mem:
                cent[c] = centre(mem)
    a = {r: nearest(r) for r in live}
    count = [sum(1 for r in live if a[r] == c) for c in range(len(cent))]
    order = [c for c in range(len(cent)) if count[c] > 0]
    order.sort(key=lambda c: -count[c])  # stable: ties keep the lower cluster number in front
    q = [list(cent[c]) for c in order]
    w = [F(F(count[c]) / F(m)) for c in order]
    while len(q) < n_vec:
        q.append(list(q[0]))
        w.append(F(0))
    return q, w, len(order), [order.index(a[r]) if r in a else -1 for r in range(L)]
