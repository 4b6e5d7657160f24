"""Test-side reference of the inner-product scorer (NANN_SCORER_IP): the canonical order of DESIGN.md 2 restated in numpy
with a correctly rounded f32 fma, and the serving schedule (build_opt_graph.py:109-149) restated over a score callable.
Shared by test_ip_cpu.py and test_ip_gpu.py; nothing under nann_amd/ imports it.

The canonical order, for d = 8 L: chunk l runs acc = fmaf(q_k, x_k, acc) from +0 over its 8 elements in order (16-bit rows
widened to f32 exactly); the L partials are added in the xor butterfly with strides 1, 2, 4, ...; score = sum.  L2 is the same
tree over t_k = q_k - x_k, acc = fmaf(t_k, t_k, acc), score = 0 - sum (restated here too: it is what the data of these tests
must NOT rank like)."""
from fractions import Fraction

import numpy as np

ERR_TOPK_K_GT_N = 4
ERR_EMPTY_SCORE_BATCH = 6
ERR_TOPK_SCALAR_INPUT = 8


def widen(embs):
    """rows as f32: f16 / f32 arrays, or uint16 bf16 bit patterns (every widening is exact)"""
    embs = np.asarray(embs)
    if embs.dtype == np.uint16:
        return (embs.astype(np.uint32) << 16).view(np.float32)
    return embs.astype(np.float32)


def to_bf16_bits(x):
    """f32 -> bf16 bit patterns, truncated (as tests/test_search_all_gpu.py makes its rows)"""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def fma32(a, b, c):
    """fmaf(a, b, c) on f32 arrays, correctly rounded.  The product of two f32 is exact in f64 (48 bits).  The f64 sum p + c is
    rounded once; TwoSum gives its exact error e, and where e != 0 the sum is moved to the ODD neighbour on e's side (round to
    odd).  A round-to-odd 53-bit value rounds to 24 bits as the exact value does (53 >= 24 + 2), subnormal results included."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)  # TwoSum: p + c = s + e exactly
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(e > 0, np.inf, -np.inf)
    s = np.where((e != 0) & even, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def _butterfly(p):
    """p f32[n, L] -> f32[n]: every lane adds its partner's partial, strides 1, 2, 4, ..."""
    L = p.shape[1]
    lanes = np.arange(L)
    s = 1
    while s < L:
        p = (p + p[:, lanes ^ s]).astype(np.float32)
        s *= 2
    return p[:, 0]


def ip_scores(q, rows):
    """<q, rows[i]> in the canonical order.  q f32[d]; rows f32[n, d] (widen() of the table's rows)"""
    q = np.asarray(q, np.float32)
    x = np.asarray(rows, np.float32).reshape(len(rows), -1, 8)
    qq = q.reshape(-1, 8)
    acc = np.zeros(x.shape[:2], np.float32)
    for k in range(8):
        acc = fma32(np.broadcast_to(qq[:, k], acc.shape), x[:, :, k], acc)
    return _butterfly(acc)


def l2_scores(q, rows):
    """-||q - rows[i]||^2 in L2's canonical order (the same tree)"""
    q = np.asarray(q, np.float32)
    x = np.asarray(rows, np.float32).reshape(len(rows), -1, 8)
    qq = q.reshape(-1, 8)
    acc = np.zeros(x.shape[:2], np.float32)
    for k in range(8):
        t = (np.broadcast_to(qq[:, k], acc.shape) - x[:, :, k]).astype(np.float32)
        acc = fma32(t, t, acc)
    return (np.float32(0.0) - _butterfly(acc)).astype(np.float32)


def ip_score_exact(q, row):
    """one score in the canonical order with every fma rounded from an exact rational: the check of fma32 itself"""
    def rnd(fr):  # Fraction -> the nearest f32, ties to even (through f64 would round twice: pick among the neighbours)
        if fr == 0:
            return np.float32(0.0)
        lo = np.float32(float(fr))  # a neighbour (within one f32 ulp); walk to the nearest
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - fr), int(np.float32(v).view(np.uint32)) & 1))
        return np.float32(best)

    q = np.asarray(q, np.float32)
    x = np.asarray(row, np.float32)
    L = len(q) // 8
    p = []
    for l in range(L):
        acc = np.float32(0.0)
        for k in range(8):
            acc = rnd(Fraction(float(q[8 * l + k])) * Fraction(float(x[8 * l + k])) + Fraction(float(acc)))
        p.append(acc)
    s = 1
    while s < L:
        p = [np.float32(p[l] + p[l ^ s]) for l in range(L)]
        s *= 2
    return p[0]


def topk_stable(scores, k):
    """positions of the top k: score descending, ties (-0 == +0 among them) to the lower position -- TopKV2 sorted=true"""
    scores = np.asarray(scores, np.float32)
    order = np.lexsort((np.arange(len(scores)), -(scores + np.float32(0.0))))
    return order[:k]


class Failed(Exception):
    def __init__(self, status):
        super().__init__(status)
        self.status = status


NUM_ROUNDS = 5  # NANN_NUM_ROUNDS: the entry layer, level 1, three level-0 rounds


def py_search(g, q, t, score, counters=False, on_cut=None):
    """One query through the serving schedule, written with sets and sorted() as tests/test_oracle_schedule.py writes it.
    g: dict with nb_values / nb_row_splits (level 0, level 1), enter_points, item_ids; score(ids list) -> list of f32.
    -> (item ids, scores f32, internal rows); raises Failed(status) where the reference's graph fails the request.
    counters=True: -> (item ids, scores, rows, int64[3, NUM_ROUNDS]) -- per round the frontier F (rows whose neighbour lists
    are read), the gathered ids G (duplicates and visited ones included) and the scored rows S, as oracle.search_batch lays
    them out: the entry round scores every enter point and reads no list.
    on_cut(kept, dropped): called at every top-k cut with the k-th score kept and the best score dropped (None where the cut
    drops nothing) -- what mlp_matrix.decisive measures its margins on."""
    ctr = np.zeros((3, NUM_ROUNDS), np.int64)

    def diff(values, visited):
        out = []
        for v in values:
            if v not in visited:
                visited.add(v)
                out.append(v)
        return out

    def topk(ids, scores, k):
        if len(scores) < k:
            raise Failed(ERR_TOPK_K_GT_N)
        order = sorted(range(len(scores)), key=lambda i: (-(scores[i] + 0.0), i))
        if on_cut is not None and k > 0:
            on_cut(scores[order[k - 1]], scores[order[k]] if len(order) > k else None)
        order = order[:k]
        return [ids[i] for i in order], [scores[i] for i in order]

    def forward(ids):
        if len(ids) == 0:
            raise Failed(ERR_EMPTY_SCORE_BATCH)
        s = [float(v) for v in score(ids)]
        if len(ids) == 1:
            raise Failed(ERR_TOPK_SCALAR_INPUT)
        return s

    def nbrs(level, frontier):
        v, rs = g["nb_values"][level], g["nb_row_splits"][level]
        out = []
        for f in frontier:
            out.extend(v[rs[f]:rs[f + 1]].tolist())
        return out

    ep = np.asarray(g["enter_points"]).tolist()
    ctr[2, 0] = len(ep)
    R, sR = topk(ep, forward(ep), t[0])
    C = nbrs(1, R)
    ctr[0, 1], ctr[1, 1] = len(R), len(C)
    vis = set()
    R = diff(R, vis)
    C = diff(C, vis)
    ctr[2, 1] = len(C)
    P, sP = topk(R + C, sR + forward(C), t[1])
    vis = set()
    B = diff(P, vis)
    for i in range(3):
        G = nbrs(0, B)
        C = diff(G, vis)
        ctr[:, 2 + i] = len(B), len(G), len(C)
        B, sB = topk(C, forward(C), t[2 + i])
        P, sP = P + B, sP + sB
    P, sP = topk(P, sP, t[5])
    out = (np.asarray(g["item_ids"])[np.asarray(P)], np.asarray(sP, np.float32), np.asarray(P, np.int32))
    return out + (ctr,) if counters else out


def scaled_rows(x, seed):
    """rows x f32[n, d] scaled by per-row factors in [0.25, 4], log-uniform: norms that vary by 16x"""
    rng = np.random.default_rng(seed)
    f = np.exp2(rng.uniform(-2.0, 2.0, len(x))).astype(np.float32)
    f[:2] = [0.25, 4.0]
    return (np.asarray(x, np.float32) * f[:, None]).astype(np.float32)
