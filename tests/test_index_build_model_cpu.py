"""The model of the device HNSW builder (tests/hnsw_build_model.py) on its own, without a GPU: graphs small enough to derive by
hand; the structural rules of tests/test_index_build_gpu.py::_check_export asked of the model at every case of
tests/test_index_build_exact_gpu.py; that every such case reaches the path it is there for (the model's coverage counters); and
that a model made wrong in one rule (hnsw_build_model.MUTANTS) changes the arrays of some case -- the evidence, obtained on the
CPU, that the comparison on the device would notice a kernel that is subtly wrong in that way."""
import numpy as np
import pytest

import hnsw_build_cases as HC
import hnsw_build_model as HM
import ip_reference as R


def _rows_of(a):
    return [[int(v) for v in r if v >= 0] for r in a]


def _hand(points, metric="l2", levels=None, keep_pruned=False, mutant=None, m=2):
    """a build over rows (x, y, 0, ...) of small integers (exact in f16 and f32) -> level-0 rows, the result"""
    rows = np.zeros((len(points), 64), np.float16)
    for i, p in enumerate(points):
        p = np.atleast_1d(p)
        rows[i, :len(p)] = p
    r = HM.build(HM.distance_matrix(rows, metric), 64, levels or [1] * len(points), m, 40, keep_pruned, metric, mutant)
    return _rows_of(r["adj0"]), r


# ---- distances ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["l2_bf16_d128_m8_kp", "ip_f16_d256_m4", "ip_bf16_d64_m8_spread"])
def test_distance_matrix_is_the_canonical_order_and_symmetric(name):
    c = HC.build_case(name)
    D = np.array(c["dist"], np.float32)
    wide = R.widen(c["rows"])
    for i in (0, 7, len(wide) - 1):
        ref = np.float32(0.0) - (R.l2_scores(wide[i], wide) if c["metric"] == "l2" else R.ip_scores(wide[i], wide))
        assert (D[i].view(np.uint32) == ref.view(np.uint32)).all() and (D[:, i].view(np.uint32) == ref.view(np.uint32)).all()
    assert (D.view(np.uint32) == D.T.view(np.uint32)).all()


# ---- graphs derived by hand ---------------------------------------------------------------------------------------------------
def test_hand_build_with_a_full_row_reselection():
    """M = 2 (4 slots on level 0, 2 above), rows e_i = (x_i, 0, ...), x = 0, 20, 9, 4, 1, -3, 30, 13; node 0 has 2 levels, so it
    is order[0], alone on level 1 (its upper row stays empty); every batch is one node (pos // 4 < 2 up to pos 7).  On a line
    the heuristic keeps the nearest node on either side: a farther one is nearer to that one than to the base.
      1 (20): beam {0}.  Row 1 = [0]; row 0 = [1].
      2 (9):  beam 0 (81), 1 (121).  0 kept; 1: d(1, 0) = 400 >= 121, kept.  Row 2 = [0, 1]; rows 0 = [1, 2], 1 = [0, 2].
      3 (4):  beam 0 (16), 2 (25), 1 (256).  0, 2 kept (d(2, 0) = 81 >= 25); 1: d(1, 2) = 121 < 256, out.  Row 3 = [0, 2];
              rows 0 = [1, 2, 3], 2 = [0, 1, 3].
      4 (1):  beam 0 (1), 3 (9), 2 (64), 1 (361).  0, 3 kept (16 >= 9); 2: d(2, 3) = 25 < 64, 1: d(1, 3) = 256 < 361, out.
              Row 4 = [0, 3]; rows 0 = [1, 2, 3, 4] -- full --, 3 = [0, 2, 4].
      5 (-3): beam 0 (9), 4 (16), 3 (49), 2 (144), 1 (529).  0 kept; every other is nearer to 0 than to 5.  Row 5 = [0].  Row 0
              is full: its 4 links and 5, ascending by distance to 0: 4 (1), 5 (9), 3 (16), 2 (81), 1 (400).  4 kept; 5:
              d(5, 4) = 16 >= 9, kept; 3: d(3, 4) = 9 < 16, 2: 64 < 81, 1: 361 < 400, out.  Row 0 = [4, 5].
      6 (30): from 0 the search walks 4, 3, 2, 1 (each row names the next node to the right): beam 1 (100), 2 (441), 3, 4, 0, 5.
              1 kept, the rest are nearer to 1.  Row 6 = [1]; row 1 = [0, 2, 6].
      7 (13): beam 2 (16), 1 (49), 3 (81), 4 (144), 0 (169), 5 (256), 6 (289).  2 kept; 1: d(1, 2) = 121 >= 49, kept; 3, 4, 0, 5
              are nearer to 2, 6 to 1.  Row 7 = [2, 1]; rows 2 = [0, 1, 3, 7], 1 = [0, 2, 6, 7]."""
    rows, r = _hand([0, 20, 9, 4, 1, -3, 30, 13], levels=[2, 1, 1, 1, 1, 1, 1, 1])
    assert rows == [[4, 5], [0, 2, 6, 7], [0, 1, 3, 7], [0, 2, 4], [0, 3], [0], [1], [2, 1]]
    assert r["up_row"].tolist() == [0] + [-1] * 7 and r["adj_up"].tolist() == [[-1, -1]]
    assert r["counters"]["reselect"] == 1 and r["counters"]["batches_of_one"] == 7 and r["batch_of"].tolist() == [-1, 0, 1, 2, 3, 4, 5, 6]
    # keepPrunedConnections: the discarded candidates fill a row's free slots, nearest first, in the candidates' order
    rows, _ = _hand([0, 20, 9, 4], keep_pruned=True)
    assert rows[3] == [0, 2, 1], "3 (4): 0 and 2 kept, the dominated 1 fills a free slot behind them"


def test_hand_build_with_ties():
    """M = 2, rows (x, y, 0, ...): 0 = (2, 0), 1 = (1, 2), 2 = (0, 0), 3 = (1, -2).
      1: row 1 = [0]; row 0 = [1].
      2: beam 0 (4), 1 (5).  0 kept; 1: d(1, 0) = 5, d(1, 2) = 5 -- EQUAL, and the test is strict: kept.  Row 2 = [0, 1];
         rows 0 = [1, 2], 1 = [0, 2].
      3: d(3, 0) = 5 = d(3, 2), d(3, 1) = 16.  The tie goes to the lower id: 0 first, kept; 2: d(2, 0) = 4 < 5, out; 1:
         d(1, 0) = 5 < 16, out.  Row 3 = [0]; row 0 = [1, 2, 3].
    With the tie to the higher id, 2 is walked first and dominates 0 (4 < 5): row 3 = [2].  With <=, 1 is dominated for node 2
    (5 <= 5): row 2 = [0]."""
    pts = [(2, 0), (1, 2), (0, 0), (1, -2)]
    rows, r = _hand(pts)
    assert rows == [[1, 2, 3], [0, 2], [0, 1], [0]] and r["counters"]["ties"] == 1
    assert _hand(pts, mutant="tie_high_id")[0][3] == [2]
    assert _hand(pts, mutant="dominate_le")[0][2] == [0]


def test_hand_build_with_a_duplicated_row():
    """M = 2, x = 0, 5, 5, 3: nodes 1 and 2 are the same row.
      1: row 1 = [0]; row 0 = [1].
      2: beam 1 (0), 0 (25).  1 kept; 0: d(0, 1) = 25, not < 25: kept.  Row 2 = [1, 0]; rows 1 = [0, 2], 0 = [1, 2].
      3 (3): d = 4 to 1 and to 2, 9 to 0.  Lower id first: 1 kept; 2: d(2, 1) = 0 < 4, out; 0: d(0, 1) = 25 >= 9, kept.
         Row 3 = [1, 0]; rows 1 = [0, 2, 3], 0 = [1, 2, 3]."""
    rows, r = _hand([0, 5, 5, 3])
    assert rows == [[1, 2, 3], [0, 2, 3], [1, 0], [1, 0]] and r["counters"]["zero_dist"] == 1


def test_hand_build_under_ip_with_distances_of_both_signs():
    """M = 2, dist(a, b) = -x_a x_b, x = 1, -2, 3, -1, 2.
      1 (-2): d(1, 0) = 2.  Row 1 = [0]; row 0 = [1].
      2 (3):  beam 0 (-3), 1 (6).  0 kept; 1: d(1, 0) = 2 < 6, out.  Row 2 = [0]; row 0 = [1, 2].
      3 (-1): beam 1 (-2), 0 (1), 2 (3).  1 kept; 0: d(0, 1) = 2 >= 1, kept; 2: d(2, 1) = 6 >= 3 but d(2, 0) = -3 < 3, out.
              Row 3 = [1, 0]; rows 1 = [0, 3], 0 = [1, 2, 3].
      4 (2):  beam 2 (-6), 0 (-2), 3 (2), 1 (4).  2 kept; 0: d(0, 2) = -3 < -2, out; 3: d(3, 2) = 3 >= 2, kept; 1: d(1, 2) = 6 >= 4
              but d(1, 3) = -2 < 4, out.  Row 4 = [2, 3]; rows 2 = [0, 4], 3 = [1, 0, 4].
    Ordered by the raw bit patterns, negative distances come after the positive ones, and the rows differ."""
    rows, r = _hand([1, -2, 3, -1, 2], "ip")
    assert rows == [[1, 2, 3], [0, 3], [0, 4], [1, 0, 4], [2, 3]]
    assert r["counters"]["neg_dist"] > 0 and r["counters"]["pos_dist"] > 0
    assert _hand([1, -2, 3, -1, 2], "ip", mutant="ip_raw_bits")[0] != rows


def test_hand_removal():
    """the graph of tests/test_index_remove_gpu.py::test_hand_made_graph_has_the_exact_answer: M = 2, x = 0, 1, 2, 3, 4, 10, node 2
    leaves.  Node 0: pool {1: 1, 3: 9}, 3 is dominated by 1 (4 < 9).  Node 1: pool {0: 1, 3: 4}, 3 is kept (9 >= 4).  Old node 3:
    pool {4: 1, 1: 4}, 1 is kept, ascending by distance.  Old nodes 4 and 5 are copied."""
    D = HM.distance_matrix(HC.line([0, 1, 2, 3, 4, 10]), "l2")
    adj0 = np.array([[1, 2, -1, -1], [0, 2, -1, -1], [1, 3, -1, -1], [2, 4, -1, -1], [3, 5, -1, -1], [4, -1, -1, -1]], np.int32)
    up = np.full((1, 2), -1, np.int32)
    mask = np.array([0, 0, 1, 0, 0, 0], bool)
    r = HM.remove(D, 64, [1] * 6, adj0, up, mask, 2)
    assert _rows_of(r["adj0"]) == [[1], [0, 2], [3, 1], [2, 4], [3]]
    assert r["kept_rows"].tolist() == [0, 1, 3, 4, 5] and r["stats"].tolist() == [3, 0, 0, 5]
    r = HM.remove(D, 64, [1] * 6, adj0, up, mask, 2, keep_pruned=True)
    assert _rows_of(r["adj0"]) == [[1, 2], [0, 2], [3, 1], [2, 4], [3]]


def test_hand_append_of_a_taller_node():
    """M = 2, x = 0, 10, 4 with one level each, built: rows 0 = [1, 2], 1 = [0, 2], 2 = [0, 1].  Appended: 3 (x = 6, 2 levels:
    taller than the entry point 0, so it goes in alone, linked on level 0 only, and is the entry point afterwards) and 4 (x = 7,
    2 levels).  Insertion order by descending level count, then id: 3, 4.
      3: level 0 from 0: beam 2 (4), 1 (16), 0 (36).  2 kept; 1: d(1, 2) = 36 >= 16, kept; 0: d(0, 2) = 16 < 36, out.
         Row 3 = [2, 1] on level 0, empty on level 1; rows 2 = [0, 1, 3], 1 = [0, 2, 3].
      4: level 1 from 3 (its row there is empty): beam {3}; row 4 = [3] on level 1, and 3's becomes [4].  Level 0 from 3: beam
         3 (1), 2 (9), 1 (9), 0 (49) -- the tie to the lower id, 1.  3 kept; 1: d(1, 3) = 16 >= 9, kept; 2: d(2, 3) = 4 < 9, out;
         0 out.  Row 4 = [3, 1]; rows 3 = [2, 1, 4], 1 = [0, 2, 3, 4]."""
    D = HM.distance_matrix(HC.line([0, 10, 4, 6, 7]), "l2")
    base = HM.build(D, 64, [1, 1, 1], 2)
    assert _rows_of(base["adj0"]) == [[1, 2], [0, 2], [0, 1]]
    r = HM.append(D, 64, [1, 1, 1, 2, 2], 3, base["adj0"], base["adj_up"], 2)
    assert _rows_of(r["adj0"]) == [[1, 2], [0, 2, 3, 4], [0, 1, 3], [2, 1, 4], [3, 1]]
    assert r["up_row"].tolist() == [-1, -1, -1, 0, 1] and _rows_of(r["adj_up"]) == [[4], [3]]
    assert r["counters"]["taller_than_entry"] == 1


# ---- every case of the device comparison: invariants, and that it reaches what it is there for -------------------------------------
# The counts found (model runs on the CPU, with the seeds of hnsw_build_cases.py), the counters a case is listed for:
#   build l2_f16_d64_m4          levels_ge3 71, reselect 3214, batches_gt1 24
#   build l2_bf16_d128_m8_kp     select_over_gpw 6926, select_fill 92526, reselect 9898
#   build l2_f16_d256_m16        select_over_gpw 390 (reselect 9: not what the case is for)
#   build l2_f16_d64_m32_kp      reselect_cap64 12636, select_fill 718131
#   build ip_bf16_d64_m8_spread  neg_dist 36510, pos_dist 1970, reselect 810
#   build ip_f16_d256_m4         select_over_gpw 1539, neg_dist 21301, pos_dist 1997
#   build tie_l2                 ties 8845, zero_dist 377
#   build tie_ip                 ties 10858, zero_dist 473, neg_dist 17104, pos_dist 1823
#   tiny n2 / n5 / n9            batches_of_one 1 / 4 / 8, levels_ge3 - / 1 / 1;  n64: batches_gt1 10, levels_ge3 1, reselect 134
#   append l2_d64_m8             batches_gt1 50 (of 51 batches);  append ip_d128_m8: batches_gt1 50
#   append of a taller node      taller_than_entry 1 (levels_ge3 3)
#   remove l2_random             repaired 446, copied 67;  l2_random_kp: repaired 495, copied 18, select_fill 4604
#   remove ip_random             repaired 449, copied 64 (pool_over_64 2);  ip_random_kp: repaired 500, copied 13, select_fill 4254
#   remove l2_m32_kp_cluster     repaired 217, pool_over_64 199
def _reaches(what, counters, want, least):
    print(what, {k: v for k, v in counters.items() if v})
    for k in want:
        assert counters[k] >= least, f"{what}: {k} = {counters[k]}, the case does not reach what it is there for"


@pytest.mark.parametrize("name", list(HC.BUILDS))
def test_build_cases(name):
    c, r = HC.build_case(name), HC.model_build(name)
    HC.check_arrays(c["levels"], r["adj0"], r["up_row"], r["adj_up"], c["M"])
    _reaches(name, r["counters"], c["want"], 10)
    b = r["batch_of"]
    assert (b == -1).sum() == 1 and c["levels"][np.argmin(b)] == c["levels"].max(), "order[0] goes in before the batches"
    assert (np.bincount(b[b >= 0], minlength=r["n_batches"]) > 0).all() and b.max() == r["n_batches"] - 1


TINY_WANT = {"n1": (), "n2": ("batches_of_one",), "n5": ("batches_of_one", "levels_ge3"), "n9": ("batches_of_one", "levels_ge3"),
             "n64": ("batches_gt1", "levels_ge3", "reselect")}


@pytest.mark.parametrize("name", list(HC.TINY))
def test_tiny_cases(name):
    c = HC.tiny_case(name)
    r = HM.build(c["dist"], c["d"], c["levels"], c["M"])
    HC.check_arrays(c["levels"], r["adj0"], r["up_row"], r["adj_up"], c["M"])
    _reaches(name, r["counters"], TINY_WANT[name], 1)
    if name == "n64":  # upper rows for every node, and the quarter rule at its start: batches of 1 x 7, then 2, 2, 3, ...
        assert (r["up_row"] >= 0).all() and (np.bincount(r["batch_of"][r["batch_of"] >= 0])[:10] == [1] * 7 + [2, 2, 3]).all()


def _model_base(c):
    """the model's build of an append case's first n_old rows"""
    n0 = c["n_old"]
    return HM.build([r[:n0] for r in c["dist"][:n0]], c["d"], c["levels"][:n0], c["M"], HC.EF, c["keep_pruned"], c["metric"])


@pytest.mark.parametrize("name", list(HC.APPENDS) + ["taller"])
def test_append_cases(name):
    c = HC.taller_case() if name == "taller" else HC.append_case(name)
    base = _model_base(c)
    r = HC.model_append(c, base["adj0"], base["adj_up"])
    HC.check_arrays(c["levels"], r["adj0"], r["up_row"], r["adj_up"], c["M"])
    _reaches(f"append {name}", r["counters"], c["want"], 1 if name == "taller" else 10)
    if name != "taller":
        assert np.bincount(r["batch_of"][c["n_old"]:]).max() == 4, "batch_cap = ceil(200 / 64)"


@pytest.mark.parametrize("name", list(HC.REMOVES))
def test_remove_cases(name):
    base_name, _, want = HC.REMOVES[name]
    c, base = HC.build_case(base_name), HC.model_build(base_name)
    r = HC.model_remove(name, base["adj0"], base["adj_up"])
    HC.check_arrays(r["levels"], r["adj0"], r["up_row"], r["adj_up"], c["M"], connected=False)
    mask = HC.remove_mask(name)
    assert r["stats"][3] == (~mask).sum() and (r["kept_rows"] == np.nonzero(~mask)[0]).all() and (r["levels"] == c["levels"][~mask]).all()
    _reaches(f"remove {name}", r["counters"], want, 10)


# ---- mutants ------------------------------------------------------------------------------------------------------------------
def _differ(a, b):
    return bool((a["adj0"] != b["adj0"]).any() or (a["adj_up"] != b["adj_up"]).any())


def _model(case, mutant=None):
    kind, name = case.split(":")
    if kind == "build":
        return HC.model_build(name, mutant)
    if kind == "tiny":
        c = HC.tiny_case(name)
        return HM.build(c["dist"], c["d"], c["levels"], c["M"], mutant=mutant)
    if kind == "append":
        c = HC.append_case(name)
        base = _model_base(c)
        return HC.model_append(c, base["adj0"], base["adj_up"], mutant)
    base = HC.model_build(HC.REMOVES[name][0])
    return HC.model_remove(name, base["adj0"], base["adj_up"], mutant)


# mutant -> cases of the device comparison whose arrays it changes
DISTINGUISHED_BY = {
    "dominate_le": ("build:tie_l2", "build:tie_ip"),
    "gpw_only": ("build:ip_f16_d256_m4", "build:l2_f16_d256_m16", "remove:l2_random"),
    "tie_high_id": ("build:tie_l2", "build:tie_ip"),
    "backlink_reverse": ("tiny:n64", "build:tie_l2", "append:l2_d64_m8"),
    "drop_new_at_64": ("build:l2_f16_d64_m32_kp",),
    "ef_39": ("build:ip_f16_d256_m4", "append:l2_d64_m8"),
    "batch_third": ("tiny:n64", "build:tie_ip"),
    "pool_uncut": ("remove:l2_m32_kp_cluster",),
    "ip_raw_bits": ("build:tie_ip", "build:ip_f16_d256_m4", "remove:ip_random"),
    "beam_expanded_last": ("build:tie_l2", "build:tie_ip"),
}


def test_every_mutant_is_listed():
    assert set(DISTINGUISHED_BY) == set(HM.MUTANTS)


@pytest.mark.parametrize("mutant,case", [(m, c) for m, cases in DISTINGUISHED_BY.items() for c in cases])
def test_a_wrong_rule_changes_the_arrays(mutant, case):
    assert _differ(_model(case), _model(case, mutant)), f"{mutant} leaves {case} as it is"
