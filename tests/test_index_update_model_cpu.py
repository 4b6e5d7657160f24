"""The model of the in-place update (tests/hnsw_update_model.py) on its own, without a GPU: that every case of
tests/hnsw_update_cases.py reaches the path it is there for; that the update equals a removal followed by an append of the
refreshed rows at the tail, entry for entry under the permutation, wherever no tie could order the two differently; that a
search for a refreshed row's new embedding finds the row more often on the updated graph than on the stale one; and that a model
made wrong in one rule of the update (hnsw_update_model.WRONG) changes the arrays of some case -- the evidence that the
comparison on the device would notice host code that is wrong in that way.  The base graphs are the model's own builds."""
import numpy as np
import pytest

import hnsw_build_cases as HC
import hnsw_build_model as HM
import hnsw_update_cases as UC
import hnsw_update_model as UM

_DONE = {}


def _updated(name, wrong=None):
    if (name, wrong) not in _DONE:
        base = UC.model_base(name)
        _DONE[(name, wrong)] = UC.model_update(name, base["adj0"], base["adj_up"], wrong=wrong)
    return _DONE[(name, wrong)]


@pytest.mark.parametrize("name", list(UC.CASES))
def test_every_case_reaches_its_path(name):
    u = UC.case(name)
    base, res = UC.model_base(name), _updated(name)
    ctr, stats = res["counters"], res["stats"]
    print(f"update model [{name}]: {int(u['mask'].sum())} of {len(u['mask'])} marked, stats {stats.tolist()}, batches {res['n_batches']}, "
          f"counters { {k: v for k, v in ctr.items() if v} }")
    for k in u["want"]:
        assert ctr[k] > 0, (name, k)
    assert stats[3] == u["mask"].sum() and stats[0] == ctr["repaired"]
    HC.check_arrays(u["levels"], res["adj0"], res["up_row"], res["adj_up"], u["M"], connected=False)
    assert ((res["adj0"][u["mask"]] >= 0).sum(1) > 0).all(), "a re-inserted node with an empty level-0 row"
    if name == "l2_m32_kp_cluster":
        assert stats[2] > 0 and ctr["batches_gt1"] == 0 and u["mask"].sum() <= 64
    if name.startswith("taller"):
        assert ctr["taller_than_entry"] == 1
        top = res["adj_up"][res["up_row"][10] + 1: res["up_row"][10] + 3]
        assert (top == -1).all(), "node 10's rows on levels 2 and 3: above every other node's top"
        assert (res["adj_up"][res["up_row"][10]] >= 0).any()
    if name == "all_but_one":
        assert stats[1] == 1 and ctr["batches_of_one"] == 63 and res["n_batches"] == 63
    if name == "relink":
        assert (res["adj0"] != base["adj0"]).any(1).sum() >= 1


def test_nothing_marked_is_the_identity():
    base = UC.model_base("l2_random")
    u = UC.case("l2_random")
    res = UC.model_update("l2_random", base["adj0"], base["adj_up"], mask=np.zeros(len(u["mask"]), bool))
    assert (res["adj0"] == base["adj0"]).all() and (res["adj_up"] == base["adj_up"]).all() and res["stats"].tolist() == [0] * 4


@pytest.mark.parametrize("name", UC.EQUIVALENT)
def test_update_equals_remove_then_append(name):
    """the refreshed rows appended at the tail of the compacted graph, with their levels: the same insertion order, entry point
    and batches, so -- with no tie for the renumbering to resolve differently -- the same arrays under the permutation"""
    u = UC.case(name)
    base, res = UC.model_base(name), _updated(name)
    mask, levels = u["mask"], np.asarray(u["levels"])
    perm, inv = UC.permutation(mask)
    n_stay = int((~mask).sum())
    removed = HM.remove(u["dist"], u["d"], levels, base["adj0"], base["adj_up"], mask, u["M"], u["keep_pruned"], u["metric"])
    assert (removed["kept_rows"] == perm[:n_stay]).all() and removed["stats"][:3].tolist() == res["stats"][:3].tolist()
    D = np.array(u["dist"], np.float32)[np.ix_(perm, perm)].tolist()
    lv_new = levels[perm]
    n_up_stay = HM.up_rows_of(lv_new[:n_stay])[1]
    appended = HM.append(D, u["d"], lv_new, n_stay, removed["adj0"], removed["adj_up"][:max(n_up_stay, 1)], u["M"], HC.EF, u["keep_pruned"], u["metric"])
    assert res["counters"]["ties"] == 0 and appended["counters"]["ties"] == 0, "a tie: the two numberings may order it differently"
    adj0, adj_up, _ = UC.permuted_arrays(res, levels, mask)
    assert (adj0 == appended["adj0"]).all() and (adj_up == appended["adj_up"]).all()
    assert res["n_batches"] == appended["n_batches"]


def test_self_hits_stale_updated_rebuilt():
    """marked rows of l2_random that a beam search for their new embedding returns first, on the graph left alone with the new
    table (stale), on the updated graph and on a from-scratch build of the new table (recorded, not a gate)"""
    u = UC.case("l2_random")
    base, res = UC.model_base("l2_random"), _updated("l2_random")
    rows = np.nonzero(u["mask"])[0]
    args = (u["dist"], u["d"], u["levels"])
    stale = UM.self_hits(*args, base["adj0"], base["adj_up"], u["M"], rows)
    updated = UM.self_hits(*args, res["adj0"], res["adj_up"], u["M"], rows)
    built = HM.build(u["dist"], u["d"], u["levels"], u["M"], HC.EF, u["keep_pruned"], u["metric"])
    rebuilt = UM.self_hits(*args, built["adj0"], built["adj_up"], u["M"], rows)
    print(f"self hits of {len(rows)} refreshed rows: stale {stale}, updated {updated}, rebuilt {rebuilt}")
    assert updated > stale


@pytest.mark.parametrize("wrong,cases", [("no_one_hop", ("l2_random", "l2_m32_kp_cluster")), ("entry_among_all", ("taller", "taller_alone")),
                                         ("build_batch_cap", ("l2_random", "ip_random"))])
def test_a_wrong_rule_changes_the_arrays(wrong, cases):
    changed = []
    for name in cases:
        good, bad = _updated(name), _updated(name, wrong)
        if (good["adj0"] != bad["adj0"]).any() or (good["adj_up"] != bad["adj_up"]).any():
            changed.append(name)
    assert changed, f"{wrong}: no case notices it"


def test_orphans_by_hand():
    adj0 = np.array([[1, 2], [0, -1], [-1, -1], [0, 1], [4, -1]], np.int32)  # 2 is empty, 3 is unnamed, 4 is named by itself alone
    assert UM.orphans(adj0).tolist() == [2, 3]
    adj0[1] = [9, -9]  # out of range on both sides: skipped, so row 1 is empty and 0 loses an in-link it still has from 3
    assert UM.orphans(adj0).tolist() == [1, 2, 3]
