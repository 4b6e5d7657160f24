"""The workload of the MLP matrix (test_mlp_matrix_gpu.py) and its references, none of which come from a device: per
(d, row dtype) the graph and the 24 queries of the traversal matrix (traverse_matrix.graph) with the graph's own rows, one set
of MLP weights per d with biases, PReLU slopes of both signs and a rescaled layer 2, and two references of that scorer --
the oracle (oracle.search_batch / score_rows, f32 in the kernels' order: what the exact kernels equal bit for bit) and the
model's definition in float64 numpy (scores64: shares no code with the oracle; what the split-f16 kernels are within 1e-5 of).
Shared by the GPU matrix and the CPU test of the workload itself (test_mlp_matrix_cpu.py); nothing under nann_amd/ imports it.

Decisive queries.  The split form's contract is |score - reference| <= 1e-5 max(1, |score|), so a split-f16 traversal may
order two rows otherwise than the reference does, and from there on walk another part of the graph.  It cannot where the
reference's own cuts are wide: a query is DECISIVE when at every top-k cut of its schedule the k-th score kept and the best
score dropped, in float64, are more than MARGIN = 3e-5 max(1, |kept|, |dropped|) apart.  Two scores that far apart cannot change
order under twice the contract's error (2e-5), so a kernel inside its contract keeps the same SET at every cut, and every
counter and the final row set are determined; the third 1e-5 is for the f32 oracle against float64, whose rows and counters
the comparison uses.  check_conditions asserts that most queries are decisive and that on those the oracle and the float64
schedule agree."""
import numpy as np

import ip_reference as R
import traverse_matrix as T

N_ITEMS, NQ = T.N_ITEMS, T.NQ
DIMS = (64, 128, 256)
DTYPES = ("f16", "bf16")
TOPN = [16, 16, 24, 32, 32, 20]
TOPN_ODD = [8, 12, 16, 16, 16, 10]   # the odd requests of the per-request launches
MIN_OK = 18                          # of the 24 queries the oracle must serve at least this many
MIN_DECISIVE = 16                    # ... and at least this many must be decisive
MARGIN = 3e-5
SPLIT_TOL = 1e-5                     # the split form's contract, relative to max(1, |reference|)
# the oracle's f32 chains (2d + 256 + 128 terms) against float64, relative to max(1, |reference|): the bound of
# test_mlp_traversal_scores_against_float64_numpy.  Measured over every row the oracle returns in the six cases under both
# settings: 2.7e-7 .. 3.6e-7, the worst at d = 128, bf16; d = 256 (3.4e-7 f16, 2.8e-7 bf16) is no further off than the
# shorter chains -- so the one bound holds at every d
ORACLE_TOL = 3e-6
# decisive queries of 24 at MARGIN, (uniform TOPN, the two per-request settings together), measured with these weights:
#   d = 64: f16 23, 23; bf16 24, 24     d = 128: f16 21, 23; bf16 21, 23     d = 256: f16 19, 18; bf16 23, 22
# and the oracle serves all 24 in every case under both settings
EVAL_CFG = ((2, 2, 1), (60, 40, 16), 30)
EVAL_QUERIES = 6
SCORE_N = (2, 255, 256, 257, 513, 131072 + 257)  # the stand-alone scorer: a pass is 256 rows, the grid stops at 512 blocks
_CACHE = {}


def graph(d):
    return T.graph(d)


def table(d, dtype):
    """-> (the graph's rows in the table's dtype -- f16, or bf16 bit patterns (uint16) --, their f32 widening)"""
    key = ("table", d, dtype)
    if key not in _CACHE:
        x = R.widen(graph(d)[0]["item_embs"])
        t = x.astype(np.float16) if dtype == "f16" else R.to_bf16_bits(x)
        _CACHE[key] = (t, R.widen(t))
    return _CACHE[key]


def weights(d):
    """synth.make_mlp_weights(d) with biases and slopes that are not constants and a layer 2 whose entries are rescaled one by
    one (a row / column mix-up of w2 cannot pass)"""
    from nann_amd import synth
    key = ("w", d)
    if key not in _CACHE:
        w = synth.make_mlp_weights(d)
        rng = np.random.default_rng(3)
        f32 = np.float32
        w["b1"] = (0.1 * rng.standard_normal(w["b1"].shape)).astype(f32)
        w["b2"] = (0.1 * rng.standard_normal(w["b2"].shape)).astype(f32)
        w["w2"] = (w["w2"] * rng.uniform(0.2, 3.0, w["w2"].shape)).astype(f32)
        w["alpha1"] = rng.uniform(-0.3, 1.2, w["alpha1"].shape).astype(f32)
        w["alpha2"] = rng.uniform(-0.3, 1.2, w["alpha2"].shape).astype(f32)
        _CACHE[key] = w
    return _CACHE[key]


def level_topn_rows():
    """the int32[24, 6] input of the per-request launches: even rows TOPN, odd rows TOPN_ODD"""
    return np.asarray([TOPN if b % 2 == 0 else TOPN_ODD for b in range(NQ)], np.int32)


def per_request():
    """-> [(queries, level_topn)] of the two per-request settings"""
    return [(np.arange(0, NQ, 2), TOPN), (np.arange(1, NQ, 2), TOPN_ODD)]


def oracle_scorer(d, dtype):
    from oracle import oracle as O
    key = ("osc", d, dtype)
    if key not in _CACHE:
        _CACHE[key] = O.Scorer("mlp", d, {"f16": O.EMB_F16, "bf16": O.EMB_BF16}[dtype], weights(d))
    return _CACHE[key]


def oracle_index(d, dtype):
    from oracle import oracle as O
    key = ("oix", d, dtype)
    if key not in _CACHE:
        g = graph(d)[0]
        _CACHE[key] = O.Index(table(d, dtype)[0], g["item_ids"], g["nb_values"], g["nb_row_splits"], g["enter_points"])
    return _CACHE[key]


def _sel(sel):
    return np.arange(NQ) if sel is None else np.asarray(sel)


def expected_exact(d, dtype, topn=TOPN, sel=None):
    """oracle.search_batch of the queries `sel` (default: all), cached: (status, item ids, scores, rows, counters)"""
    from oracle import oracle as O
    key = ("exact", d, dtype, tuple(topn), None if sel is None else tuple(sel))
    if key not in _CACHE:
        _CACHE[key] = O.search_batch(oracle_index(d, dtype), oracle_scorer(d, dtype), graph(d)[1][_sel(sel)], topn, n_threads=8)
    return _CACHE[key]


def expected_eval(d, dtype):
    """oracle.search_eval of the first EVAL_QUERIES queries under EVAL_CFG -> [(status, item ids, scores, rows)]"""
    from oracle import oracle as O
    key = ("eval", d, dtype)
    if key not in _CACHE:
        _CACHE[key] = [O.search_eval(oracle_index(d, dtype), oracle_scorer(d, dtype), q, *EVAL_CFG) for q in graph(d)[1][:EVAL_QUERIES]]
    return _CACHE[key]


def oracle_scores_all(d, dtype, q):
    """oracle.score_rows of every row of the table under the query q (rows are scored independently: the score of a
    gathered list is a gather of these)"""
    from oracle import oracle as O
    rc, s = O.score_rows(oracle_scorer(d, dtype), q, table(d, dtype)[0])
    assert rc == 0
    return s


def _prelu(z, a):
    return np.maximum(z, 0.0) + a * np.minimum(z, 0.0)


def scores64(d, dtype, q, rows, w=None):
    """The MLP in float64, from the model's definition: concat([q ; e]) W1 + b1 -> PReLU -> W2 + b2 -> PReLU -> w3, e = the
    table's rows `rows` widened.  w: other weights than weights(d) (the mutation checks)."""
    if w is None:
        if ("w64", d) not in _CACHE:
            _CACHE[("w64", d)] = {k: np.asarray(v, np.float64) for k, v in weights(d).items()}
        w = _CACHE[("w64", d)]
    else:
        w = {k: np.asarray(v, np.float64) for k, v in w.items()}
    e = table(d, dtype)[1][np.asarray(rows, np.int64)].astype(np.float64)
    x = np.concatenate([np.tile(np.asarray(q, np.float64), (len(e), 1)), e], axis=1)
    return _prelu(_prelu(x @ w["w1"] + w["b1"], w["alpha1"]) @ w["w2"] + w["b2"], w["alpha2"]) @ w["w3"]


def schedule64(d, dtype, topn=TOPN, sel=None):
    """ip_reference.py_search over scores64 for the queries `sel` -> [(status, rows, counters, smallest margin of its cuts)];
    the margin of a cut: (kept - dropped) / max(1, |kept|, |dropped|), inf where nothing is dropped"""
    key = ("sched", d, dtype, tuple(topn), None if sel is None else tuple(sel))
    if key not in _CACHE:
        g, q = graph(d)
        out = []
        for b in _sel(sel):
            margins = [np.inf]

            def on_cut(kept, dropped):
                if dropped is not None:
                    margins.append((kept - dropped) / max(1.0, abs(kept), abs(dropped)))
            try:
                _, _, rows, ctr = R.py_search(g, q[b], topn, lambda r: scores64(d, dtype, q[b], r), counters=True, on_cut=on_cut)
                out.append((0, rows, ctr, min(margins)))
            except R.Failed as e:
                out.append((e.status, None, None, -np.inf))
        _CACHE[key] = out
    return _CACHE[key]


def decisive(d, dtype, topn=TOPN, sel=None):
    """bool[len(sel)]: the queries whose every cut is wider than MARGIN (a query the schedule fails is not decisive)"""
    return np.asarray([st == 0 and m > MARGIN for st, _, _, m in schedule64(d, dtype, topn, sel)])


def oracle_error(d, dtype, topn=TOPN, sel=None):
    """the largest |oracle - scores64| / max(1, |scores64|) over every row the oracle returns"""
    g, q = graph(d)
    st, _, sc, rows, _ = expected_exact(d, dtype, topn, sel)
    worst = 0.0
    for i, b in enumerate(_sel(sel)):
        if st[i] == 0:
            ref = scores64(d, dtype, q[b], rows[i])
            worst = max(worst, float(np.max(np.abs(sc[i].astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref)))))
    return worst


def check_conditions(d, dtype):
    """What the case's inputs must satisfy for a pass to mean something, asserted on the references alone: the oracle serves
    enough requests and enough of them are decisive, uniformly and over the two per-request settings together; on every
    decisive query the float64 schedule and the oracle return the same rows and counters; the oracle's scores are within
    ORACLE_TOL of float64."""
    settings = [[(None, TOPN)], per_request()]
    for setting in settings:
        served = n_dec = 0
        for sel, topn in setting:
            exp = expected_exact(d, dtype, topn, sel)
            dec = decisive(d, dtype, topn, sel)
            served += int((exp[0] == 0).sum())
            n_dec += int(dec.sum())
            for i, (st, rows, ctr, _) in enumerate(schedule64(d, dtype, topn, sel)):
                if dec[i]:
                    assert exp[0][i] == 0 and set(rows.tolist()) == set(exp[3][i].tolist()) and (ctr == exp[4][i]).all(), \
                        ("the oracle and the float64 schedule part on a decisive query", d, dtype, topn, i)
            err = oracle_error(d, dtype, topn, sel)
            assert err <= ORACLE_TOL, ("the oracle against float64", d, dtype, topn, err)
        assert served >= MIN_OK, ("the oracle serves too few requests", d, dtype, len(setting), served)
        assert n_dec >= MIN_DECISIVE, ("too few decisive queries", d, dtype, len(setting), n_dec)
