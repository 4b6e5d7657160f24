"""The workload of the evaluation-traversal matrix (test_eval_matrix_gpu.py) and its expected values, none of which come from a
device.  Shared by the GPU matrix and the CPU tests that check the workload itself (test_eval_matrix_cpu.py); nothing under
nann_amd/ imports it.

Small case: traverse_matrix's 4 000-row host-built graph per d, its scaled rows and its 24 queries, under two settings of
Model.retrieval; expected values are oracle.search_eval, user by user.

Sparse case: the same graph relabelled into an id space of N rows through a strictly increasing map pi, every other row empty
(no neighbours, a zero embedding, nothing links to it).  Because pi is monotone every ascending set, every tie-break by
position and every score is the small graph's, so the expected rows are the small case's mapped through pi; the CPU tests
check that claim on the oracle itself.  The table of N x d is never built on the host as data: the oracle reads np.zeros plus
one scatter (untouched pages), the device gets a zero fill plus the same scatter."""
import numpy as np

import traverse_matrix as T

NQ = T.NQ
DIMS, DTYPES = T.DIMS, T.DTYPES
# (num_scoring_per_level, top_k_per_level, topk_eval), indexed by level (0, 1, start level 2)
CFG_SCALED = ((3, 1, 1), (200, 100, 16), 100)   # config.py's defaults (3, 1, 1) / (400, 200, 100) / 200 at this graph's size: 16 enter points
CFG_DRY = ((12, 6, 1), (300, 700, 2048), 500)   # k above the 16 enter points and the 143 rows of level 1; rounds until the frontiers run dry
CFGS = (CFG_SCALED, CFG_DRY)
CFG_CHEAP = ((2, 1, 1), (60, 40, 16), 30)       # the slot-reuse batches: hundreds of users through the oracle within seconds
ATTN_CFG = ((2, 1, 1), (100, 60, 30), 50)       # the setting the attention model's evaluation tests run
ATTN_DIMS, ATTN_DTYPES, ATTN_L, ATTN_E = (64, 128), ("f16", "bf16"), 50, 64

# ---- the window arithmetic of nann_eval.h (test_eval_matrix_cpu.py restates it from bm_words) --------------------------------
WIN_OWNERS = 992                         # kEvalWinOwners: threads' worth of 32 bitmap words in a window
WIN_ITEMS = WIN_OWNERS * 32 * 32         # 1 015 808 rows in a window
MAX_WINDOWS = 8                          # kEvalMaxWindows
N_ONE_WINDOW = WIN_ITEMS                 # form 1, 992 owners: one window, exactly full
N_TWO_WINDOWS = WIN_ITEMS + 1            # form 2, the second window holds one bit
N_SPARSE = 2 * WIN_ITEMS + 1             # 2 031 617: three windows, the last holds one bit
N_EIGHT_WINDOWS = MAX_WINDOWS * WIN_ITEMS        # 8 126 464: the largest index of the LDS form
N_SLOT = N_EIGHT_WINDOWS + 1                     # 8 126 465: nine windows -> the slot form, in process
# use_dirty (eval_plan): 256 + 4 x owners <= eval_dirty_room(), owners = ceil(bm_words / 32).  eval_dirty_room() is
# sizeof(TopkScratchT<2048>) rounded up to 256: sel 2048 x 8 + the 2 048-byte rank / bin union + misc 16 + three per-wavefront
# arrays of 16 x 4 = 18 640 -> 18 688.  So the second-level bitmap is kept up to (18 688 - 256) / 4 = 4 608 owners =
# 4 718 592 rows, and the slot form scans `seen` whole from 4 718 593 rows on (not "~7 M"): N_SLOT is above it.
DIRTY_ROOM = (2048 * 8 + 2048 + 16 + 3 * 16 * 4 + 255) // 256 * 256
N_DIRTY = (DIRTY_ROOM - 256) // 4 * 32 * 32      # the largest N with use_dirty = 1
ROW_LEN_LDS = 65535                      # the longest neighbour row of the LDS form: its length rides in 16 bits
FRONTIER_MAX = 2048                      # kEvalMaxK: a frontier above it is NANN_ERR_CAPACITY
ERR_CAPACITY = 103
CUS = 256                                # an MI355X's compute units: slots = min(users, CUS x (1 in the LDS forms, 2 in the slot form))

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def bm_words(n):
    """words of the index's bitmap: one bit per row, padded to a multiple of 4 words (nann_index_create)"""
    return ((n + 31) // 32 + 3) // 4 * 4


def windows(n):
    """(owners, windows, form of the L2 traversal) of an index of n rows with short neighbour rows"""
    owners = (bm_words(n) + 31) // 32
    per = min(owners, WIN_OWNERS)
    w = (owners + per - 1) // per
    return owners, w, 0 if w > MAX_WINDOWS else 1 if w == 1 else 2


def use_dirty(n):
    return int(256 + 4 * ((bm_words(n) + 31) // 32) <= DIRTY_ROOM)


# ---- the small case ---------------------------------------------------------------------------------------------------------
def _code(dtype):
    from oracle import oracle as O
    return {"f16": O.EMB_F16, "bf16": O.EMB_BF16, "f32": O.EMB_F32}[dtype]


def oracle_index(d, dtype):
    from oracle import oracle as O
    g = T.graph(d)[0]
    return _cached(("oix", d, dtype), lambda: O.Index(T.table(d, dtype)[0], g["item_ids"], g["nb_values"], g["nb_row_splits"], g["enter_points"]))


def run_oracle(oix, d, dtype, queries, cfg):
    """oracle.search_eval per user -> [(status, item ids, scores, rows)]"""
    from oracle import oracle as O
    osc = O.Scorer("l2", d, _code(dtype))
    return [O.search_eval(oix, osc, q, *cfg) for q in queries]


def queries(d, dtype=None):
    """the 24 queries of the small case; with a dtype, a 25th user aimed at the graph's last node -- the sparse cases put that
    node at row n - 1, which is a window of its own when n is a multiple of 1 015 808 plus one"""
    q = T.graph(d)[1]
    return q if dtype is None else np.concatenate([q, T.table(d, dtype)[1][-1:].astype(np.float32)])


def expected(d, dtype, cfg, aimed=False):
    """the oracle's answer for the 24 queries of the small case, `aimed`: and the 25th user's (cached, never changed)"""
    exp = _cached(("exp", d, dtype, cfg), lambda: run_oracle(oracle_index(d, dtype), d, dtype, queries(d, dtype), cfg))
    return exp if aimed else exp[:NQ]


def reuse_queries(d, n):
    """n users: the 24 queries tiled, every fourth tile the queries themselves (identical users at different places of the
    batch), the others perturbed by a few percent of a component -> (q f32[n, d], source i32[n]: user b is queries[source[b]]
    exactly, or -1)"""
    def make():
        q = T.graph(d)[1]
        rng = np.random.default_rng(31 * d + n)
        out = q[np.arange(n) % NQ].copy()
        src = np.arange(n) % NQ
        exact = (np.arange(n) // NQ) % 4 == 0
        out[~exact] += (rng.standard_normal((int((~exact).sum()), d)) * 0.02 * np.abs(q).mean()).astype(np.float32)
        return out, np.where(exact, src, -1).astype(np.int32)
    return _cached(("reuse_q", d, n), make)


def expected_reuse(d, dtype, n):
    return _cached(("exp_reuse", d, dtype, n), lambda: run_oracle(oracle_index(d, dtype), d, dtype, reuse_queries(d, n)[0], CFG_CHEAP))


# ---- the attention model on the small case ----------------------------------------------------------------------------------
def attn_weights(d):
    from nann_amd import synth
    return _cached(("attn_w", d), lambda: synth.make_attn_weights(d, ATTN_E))


def attn_seqs():
    """the 24 users' histories f16[24, 50, 64] (the ones the d = 64 queries are the means of)"""
    from nann_amd import synth
    g = T.graph(64)[0]
    return _cached(("attn_seqs",), lambda: synth.make_queries(g["item_embs"], g["assign"], NQ, seed=5))


def attn_oracle_model(d, dtype):
    from oracle import oracle as O
    return _cached(("attn_am", d, dtype), lambda: O.AttnModel(d, ATTN_E, ATTN_L, _code(dtype), attn_weights(d)))


def expected_attn(d, dtype):
    """oracle.search_eval under the attention scorer -> [(status, item ids, scores, rows)] (cached)"""
    def make():
        from oracle import oracle as O
        osc = O.Scorer("attention", d, _code(dtype), attn_model=attn_oracle_model(d, dtype))
        return [O.search_eval(oracle_index(d, dtype), osc, s.astype(np.float32).reshape(-1), *ATTN_CFG) for s in attn_seqs()]
    return _cached(("exp_attn", d, dtype), make)


# ---- the sparse case --------------------------------------------------------------------------------------------------------
def pi(n_nodes, n):
    """strictly increasing i64[n_nodes] into [0, n): spread evenly over the id space (so every window holds nodes), a node on
    either side of every window seam (ids j x 1 015 808 - 1 and j x 1 015 808), the last node at n - 1"""
    p = (np.arange(n_nodes, dtype=np.int64) * (n - 1)) // (n_nodes - 1)
    for seam in range(WIN_ITEMS, n, WIN_ITEMS):
        i = int(np.searchsorted(p, seam))
        assert 1 <= i < n_nodes
        p[i - 1], p[i] = seam - 1, seam
    assert p[0] == 0 and p[-1] == n - 1 and (np.diff(p) > 0).all(), "pi is not strictly increasing onto [0, n)"
    return p


def relabel(g, p, n):
    """the graph's arrays in the id space of n rows: node i becomes row p[i]; every other row has no neighbours and item id 0"""
    out = {"item_ids": np.zeros(n, np.int64), "nb_values": [], "nb_row_splits": [], "enter_points": p[np.asarray(g["enter_points"], np.int64)].astype(np.int32)}
    out["item_ids"][p] = g["item_ids"]
    for l in (0, 1):
        deg = np.zeros(n, np.int64)
        deg[p] = np.diff(np.asarray(g["nb_row_splits"][l], np.int64))
        out["nb_row_splits"].append(np.concatenate([[0], np.cumsum(deg)]).astype(np.int64))
        out["nb_values"].append(p[np.asarray(g["nb_values"][l], np.int64)].astype(np.int32))   # (p ascending: the rows keep their order)
    return out


def sparse_graph(d, n):
    """(pi, the relabelled graph) of the small graph of `d` in n rows; not cached (130 MB at 8.1 M rows)"""
    g = T.graph(d)[0]
    p = pi(T.N_ITEMS, n)
    return p, relabel(g, p, n)


def host_table(rows, p, n):
    """np.zeros + one scatter: the table the oracle reads (the zero pages are never touched)"""
    t = np.zeros((n, rows.shape[1]), rows.dtype)
    t[p] = rows
    return t


def through(exp, p, shift_from=None):
    """the small case's answers with their rows mapped through pi.  shift_from: the mutation check of the matrix -- rows at or
    behind that id are shifted by one"""
    out = []
    for rc, ids, sc, rows in exp:
        r = p[rows]
        if shift_from is not None:
            r = r + (r >= shift_from)
        out.append((rc, ids, sc, r.astype(np.int32)))
    return out


def oracle_on_sparse(d, dtype, n, cfg):
    """the oracle itself on the relabelled graph, the 25 users (what `through(expected(aimed=True))` must equal)"""
    from oracle import oracle as O
    p, sg = sparse_graph(d, n)
    oix = O.Index(host_table(T.table(d, dtype)[0], p, n), sg["item_ids"], sg["nb_values"], sg["nb_row_splits"], sg["enter_points"])
    return p, run_oracle(oix, d, dtype, queries(d, dtype), cfg)


def same_answers(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and len(x[1]) == len(y[1]) and (x[1] == y[1]).all() and (x[3] == y[3]).all() and
                                    (x[2].view(np.uint32) == y[2].view(np.uint32)).all() for x, y in zip(a, b))


# ---- a hub row of 65 535 / 65 536 neighbours (d = 64 f16) -------------------------------------------------------------------
HUB_FILL = 48.0   # every component of a filler row: |filler - q|^2 is ~64 x 48^2, far below every kept score


def hub_case(row_len):
    """the small graph of d = 64 plus filler rows 4000 .. (a constant embedding, no neighbours, nothing else links to them)
    appended to the level-0 row of one node, the hub, so that the row holds row_len distinct neighbours.  The hub is the best row
    of user 0's answer: kept from the round that finds it, so walked in the round behind.  -> dict(g, table f16, hub, oix)"""
    def make():
        from oracle import oracle as O
        g = T.graph(64)[0]
        rows = T.table(64, "f16")[0]
        hub = int(expected(64, "f16", CFG_SCALED)[0][3][0])
        rs0 = np.asarray(g["nb_row_splits"][0], np.int64)
        v0 = np.asarray(g["nb_values"][0], np.int32)
        n_fill = row_len - int(rs0[hub + 1] - rs0[hub])
        n = T.N_ITEMS + n_fill
        table = np.concatenate([rows, np.full((n_fill, 64), HUB_FILL, np.float16)])
        cut = int(rs0[hub + 1])
        nv0 = np.concatenate([v0[:cut], np.arange(T.N_ITEMS, n, dtype=np.int32), v0[cut:]])
        nrs0 = np.concatenate([rs0[:hub + 1], rs0[hub + 1:] + n_fill, np.full(n_fill, rs0[-1] + n_fill, np.int64)])
        rs1 = np.asarray(g["nb_row_splits"][1], np.int64)
        gg = {"item_ids": np.concatenate([g["item_ids"], np.arange(10 ** 7, 10 ** 7 + n_fill, dtype=np.int64)]),
              "nb_values": [nv0, np.asarray(g["nb_values"][1], np.int32)],
              "nb_row_splits": [nrs0, np.concatenate([rs1, np.full(n_fill, rs1[-1], np.int64)])],
              "enter_points": np.asarray(g["enter_points"], np.int32)}
        assert int(np.diff(nrs0).max()) == row_len == len(set(nv0[nrs0[hub]:nrs0[hub + 1]].tolist()))
        return {"g": gg, "table": table, "hub": hub,
                "oix": O.Index(table, gg["item_ids"], gg["nb_values"], gg["nb_row_splits"], gg["enter_points"])}
    return _cached(("hub", row_len), make)


def hub_users(row_len):
    """the users of the hub runs: those whose walk (the per-op spelling on the oracle's ops) has the hub in a level-0 frontier,
    four at the most, and two whose walk never meets it -> (user ids, walks hub bool[n], largest frontier walked)"""
    def make():
        c = hub_case(row_len)
        w = walks(c, T.graph(64)[1], CFG_SCALED)
        on = [b for b, fr in enumerate(w) if any(lvl == 0 and (ids == c["hub"]).any() for lvl, ids in fr)]
        off = [b for b in range(NQ) if b not in on]
        users = on[:4] + off[:2]
        return np.asarray(users), np.asarray([b in on for b in users]), max(len(ids) for b in users for _, ids in w[b])
    return _cached(("hub_users", row_len), make)


# ---- frontiers above the limit: a cluster of identical, mutually linked rows (d = 64 f16) -----------------------------------
CLUSTER = 2304
CFG_FAIL = ((6, 1, 1), (60, 40, 16), 30)   # six rounds on level 0: the cluster is reached before the level's last round


class RecordingOps:
    """test_eval_graph_cpu.OracleOps, recording every frontier a round walks: (level, the rows) per group_gather"""

    def __init__(self, oracle, nnz0):
        from test_eval_graph_cpu import OracleOps
        self._ops, self._nnz0 = OracleOps(oracle), nnz0
        self.frontiers = []

    def group_gather(self, pv, prs, iv, irs, unique=False):
        self.frontiers.append((0 if pv.numel() == self._nnz0 else 1, iv.numpy().copy()))
        return self._ops.group_gather(pv, prs, iv, irs, unique)

    def __getattr__(self, name):
        return getattr(self._ops, name)


def walks(case, queries, cfg, d=64, dtype="f16", stats=None):
    """per user: the per-op spelling of Model.retrieval (retrieval.search_eval_per_op) on the oracle's ops over the case's graph
    -> the frontiers its rounds walk, [(level, rows)]; stats: a list that receives each user's [F, G, S] (rows walked,
    neighbours gathered, rows scored).  A level's last round selects a frontier that no round walks, in the per-op spelling as
    in the kernel."""
    import torch
    from types import SimpleNamespace
    from nann_amd import retrieval
    from oracle import oracle as O
    g = case["g"]
    assert len(g["nb_values"][0]) != len(g["nb_values"][1])
    table = case["table"]
    ix = SimpleNamespace(item_embs=SimpleNamespace(numpy=lambda: table), item_ids=torch.as_tensor(np.asarray(g["item_ids"], np.int64)),
                         nb_values=[torch.as_tensor(np.asarray(v, np.int32)) for v in g["nb_values"]],
                         nb_row_splits=[torch.as_tensor(np.asarray(r, np.int64)) for r in g["nb_row_splits"]],
                         enter_points=torch.as_tensor(np.asarray(g["enter_points"], np.int32)), bitmap_words=(len(g["item_ids"]) + 31) // 32)
    osc = O.Scorer("l2", d, _code(dtype))
    out = []
    for q in queries:
        rec, st = RecordingOps(O, len(g["nb_values"][0])), {}
        retrieval.search_eval_per_op(ix, osc, torch.as_tensor(q), *cfg, backend=rec, stats=st)
        out.append(rec.frontiers)
        if stats is not None:
            stats.append([st["F"], st["G"], st["S"]])
    return out


COUNTER_USERS = tuple(range(0, NQ, 3))


def expected_counters(d, dtype, cfg):
    """[F, G, S] of the users COUNTER_USERS of the small case, counted in the per-op spelling on the oracle's ops"""
    def make():
        st = []
        walks({"g": T.graph(d)[0], "table": T.table(d, dtype)[0]}, T.graph(d)[1][list(COUNTER_USERS)], cfg, d, dtype, st)
        return np.asarray(st, np.int64)
    return _cached(("ctr", d, dtype, cfg), make)


def cluster_case():
    """the small graph of d = 64 plus CLUSTER rows 4000 .. that all hold the row of node `anchor`: row 4000 links to every
    other row of the cluster and to the anchor, every other row links to row 4000 and its two ring neighbours, the anchor
    links to row 4000.  A user aimed at the anchor finds 2 303 new rows tied at the best score in one round."""
    def make():
        from oracle import oracle as O
        g = T.graph(64)[0]
        rows = T.table(64, "f16")[0]
        anchor = int(expected(64, "f16", CFG_SCALED)[0][3][0])
        c0, n = T.N_ITEMS, T.N_ITEMS + CLUSTER
        table = np.concatenate([rows, np.repeat(rows[anchor][None], CLUSTER, axis=0)])
        rs0 = np.asarray(g["nb_row_splits"][0], np.int64)
        v0 = np.asarray(g["nb_values"][0], np.int32)
        lists = [v0[rs0[i]:rs0[i + 1]] for i in range(T.N_ITEMS)]
        lists[anchor] = np.concatenate([lists[anchor], [c0]]).astype(np.int32)
        lists.append(np.concatenate([[anchor], np.arange(c0 + 1, n)]).astype(np.int32))
        for i in range(1, CLUSTER):
            lists.append(np.asarray([c0, c0 + 1 + (i - 2) % (CLUSTER - 1), c0 + 1 + i % (CLUSTER - 1)], np.int32))
        nrs0 = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
        rs1 = np.asarray(g["nb_row_splits"][1], np.int64)
        gg = {"item_ids": np.concatenate([g["item_ids"], np.arange(10 ** 7, 10 ** 7 + CLUSTER, dtype=np.int64)]),
              "nb_values": [np.concatenate(lists).astype(np.int32), np.asarray(g["nb_values"][1], np.int32)],
              "nb_row_splits": [nrs0, np.concatenate([rs1, np.full(CLUSTER, rs1[-1], np.int64)])],
              "enter_points": np.asarray(g["enter_points"], np.int32)}
        return {"g": gg, "table": table, "anchor": anchor,
                "oix": O.Index(table, gg["item_ids"], gg["nb_values"], gg["nb_row_splits"], gg["enter_points"])}
    return _cached(("cluster",), make)


def cluster_users(n_fail, n_ok):
    """q f32[n_fail + n_ok, 64]: first n_fail users aimed at the anchor's row (perturbed, every 4th exactly it), then n_ok of
    reuse_queries"""
    c = cluster_case()
    rng = np.random.default_rng(977)
    a = c["table"][c["anchor"]].astype(np.float32)
    aimed = np.repeat(a[None], n_fail, axis=0)
    aimed[np.arange(n_fail) % 4 != 0] += (rng.standard_normal((n_fail - (n_fail + 3) // 4, 64)) * 0.01 * np.abs(a).mean()).astype(np.float32)
    return np.concatenate([aimed, reuse_queries(64, n_ok)[0]])


def predict_failures(queries, cfg=CFG_FAIL):
    """bool[n]: some round of the user walks a frontier above FRONTIER_MAX -- NANN_ERR_CAPACITY on the device"""
    return np.asarray([max(len(ids) for _, ids in fr) > FRONTIER_MAX for fr in walks(cluster_case(), queries, cfg)])
