"""The model of the shard merge (tests/merge_model.py) against the library's host code, without a GPU, on every case of
tests/merge_cases.py: nann_merge_topk_host, shard.merge_records_host and shard.pack_record_host equal it bit for bit.  And the
cases can tell: a model made wrong in one rule (merge_model.MUTANTS) changes the output of the cases named here -- the
evidence that tests/test_merge_gpu.py, which holds the device to the same model on the same cases, would notice a kernel that
is wrong in that way."""
import numpy as np
import pytest

import merge_cases as MC
import merge_model as MM


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return (bits(a[0]) == bits(b[0])).all() and (a[1] == b[1]).all()


# ---- the model by hand ----------------------------------------------------------------------------------------------------------
def test_order_by_hand():
    row = np.array([1.0, -0.0, 2.0, 0.0, 1.0, -np.inf, np.inf, 0.0], np.float32)
    assert MM.order(row, 8).tolist() == [6, 2, 0, 4, 1, 3, 7, 5]  # -0 == +0: positions 1, 3, 7 in their order
    v, i = MM.top_k(row, 5)
    assert i.tolist() == [6, 2, 0, 4, 1] and i.dtype == np.int32
    assert bits(v).tolist() == bits(np.array([np.inf, 2.0, 1.0, 1.0, -0.0], np.float32)).tolist()  # the -0 keeps its sign


def test_merge_by_hand():
    # two shards of three; 5 ties across the shards (lower shard first), 3 ties inside shard 1 (lower slot first)
    s = np.array([[[5.0, 3.0, 1.0], [5.0, 3.0, 3.0]]], np.float32)
    i = np.array([[[10, 11, 12], [20, 21, 22]]], np.int64)
    os_, oi = MM.merge(s, i, 5)
    assert oi.tolist() == [[10, 20, 11, 21, 22]] and os_.tolist() == [[5.0, 5.0, 3.0, 3.0, 3.0]]
    assert MM.merge(s, i, 5, "tie_high_shard")[1].tolist() == [[20, 10, 21, 22, 11]]


def test_pack_by_hand():
    s = np.array([[1.0, 2.0], [3.0, 4.0]], np.float32)
    i = np.array([[7, 8], [9, 1 << 40]], np.int64)
    rec = MM.pack(s, i, np.array([0, 6], np.int32))
    assert rec.size == 256 and not rec[48:].any()
    assert rec[:16].view(np.float32).tolist() == [1.0, 2.0, -np.inf, -np.inf]
    assert rec[16:48].view(np.int64).tolist() == [7, 8, 0, 0]
    assert MM.pack(s, i, None)[16:48].view(np.int64).tolist() == [7, 8, 9, 1 << 40]
    assert MM.record_bytes(9, 7) == 768 and MM.record_bytes(64, 4) == 3072


# ---- the cases are the ones the device has to see ---------------------------------------------------------------------------------
def test_the_shapes_cover_the_paths():
    shapes = set(MC.SHAPES.values())
    for must in [(8, 200, 200, 70), (8, 200, 50, 70), (1, 200, 150, 5), (1, 1, 1, 1), (3, 7, 21, 9), (2, 512, 1024, 3),
                 (5, 205, 1024, 3), (13, 1024, 1024, 3), (16, 1024, 1024, 2)]:
        assert must in shapes, must
    keys = {w * k for w, k, _, _ in shapes}
    assert {1023, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 13312, 16384} <= keys
    assert {1, 257} <= {b for _, _, _, b in shapes}
    assert MM.record_bytes(9, 7) != 9 * 7 * 12 and (9 * 7 * 4) % 8  # "odd": a padded record, ids off the 8-byte grid
    assert all(w * k <= 16384 and ko <= min(1024, w * k) for w, k, ko, _ in shapes)
    w, k, ko, _ = MC.REREAD_SHAPE[1]
    assert w * k == 17408
    for s in MC.EVERY_CONTENT_AT:
        assert all(f"{s}:{c}" in MC.MERGE_CASES for c in MC.ALL_CONTENTS)
    assert set(MC.TOPK_SHAPES) == {(1025, 1025), (1500, 1025), (4096, 2048), (4097, 4097), (16384, 1025), (16384, 16384)}


def test_the_contents_are_what_they_say():
    c = MC.merge_case("a200:failed")
    st = c["status"]
    assert st[0, 0] and st[-1, -1] and st[:, 35].all() and 0 < (st != 0).sum() < st.size
    es, ei = MC.expected("a200:failed")
    assert np.isneginf(es[35]).all() and not ei[35].any()          # every shard failed: (-inf, 0) surfaces
    assert not np.isneginf(es[0]).any() and not (ei[0] >> 40 == 1).any()  # shard 0 failed query 0: none of its ids
    c = MC.merge_case("a200:special")
    b = set(bits(c["scores"]).ravel().tolist())
    assert {0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x7f800000, 0xff800000} <= b
    es, ei = MC.expected("a200:special")
    assert (bits(es) == 0x80000000).any() and (bits(es) == 0).any()  # both zeros are among the selected
    c = MC.merge_case("a200:l2_like")
    assert len(set((bits(c["scores"]) >> 23).ravel().tolist()) - {0x17f, 0x180}) == 0 and (c["scores"] < 0).all()
    c = MC.merge_case("a200:best_last")
    assert (np.diff(c["scores"], axis=2) <= 0).all()
    assert (MC.expected("a200:best_last")[1] >> 40 == 8).all()     # every result from the last shard
    c = MC.merge_case("a200:distinct")
    assert all(len(set(r.ravel().tolist())) == 1600 for r in c["scores"])
    for name in ("a200:ties", "q257:failed"):
        ids = MC.merge_case(name)["ids"]
        assert len(np.unique(ids)) == ids.size and (ids >> 32).all()


# ---- the library's host code equals the model -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.MERGE_TOPK_CASES)
def test_merge_topk_host_equals_the_model(name):
    from nann_amd import shard
    c = MC.merge_case(name)
    sc, ii = MC.merge_inputs(name)
    assert _same(shard.merge_host(sc, ii, c["k_out"]), MM.merge(sc, ii, c["k_out"]))


@pytest.mark.parametrize("name", MC.MERGE_CASES)
def test_pack_and_merge_records_host_equal_the_model(name):
    from nann_amd import shard
    c = MC.merge_case(name)
    recv = MC.records(name)
    assert recv.shape == (c["world"], shard.record_bytes(c["b"], c["k_in"]))
    for s in range(c["world"]):
        assert (shard.pack_record_host(c["scores"][:, s], c["ids"][:, s], MC.shard_status(c, s)) == recv[s]).all(), s
    assert _same(shard.merge_records_host(recv, c["b"], c["k_in"], c["k_out"]), MC.expected(name))
    assert _same(MM.exchange(c["scores"], c["ids"], c["status"], c["k_out"]), MC.expected(name))


@pytest.mark.parametrize("n,k", MC.TOPK_SHAPES)
@pytest.mark.parametrize("content", MC.TOPK_CONTENTS)
def test_topk_model_is_a_sorted_selection(n, k, content):
    rows, vals, idx = MC.topk_case(n, k, content)
    for r, v, i in zip(rows, vals, idx):
        assert len(set(i.tolist())) == k and (bits(r[i]) == bits(v)).all()
        assert (v[:-1] >= v[1:]).all() and ((v[:-1] > v[1:]) | (i[:-1] < i[1:])).all()  # descending, ties by position
        rest = np.delete(r, i)
        assert rest.size == 0 or rest.max() <= v[-1]


# ---- the cases discriminate -------------------------------------------------------------------------------------------------------
# mutant -> cases of the device comparison whose output it changes
DISTINGUISHED_BY = {
    "tie_high_shard": ("a200:ties", "a200:all_equal", "a50:ties", "odd:ties", "e1025:ties"),
    "ids_from_shard0": ("a200:distinct", "a200:best_last", "odd:distinct", "lds_optin:distinct"),
    "id_offset_k_out": ("a50:distinct", "w1:distinct", "odd:distinct", "e2048:ties"),
    "id_stride_unpadded": ("a200:distinct", "odd:distinct", "e1023:ties"),
    "stride_unpadded": ("a200:distinct", "odd:distinct", "odd:ties", "e1023:distinct"),
    "neg_zero_below": ("a200:special", "a50:special", "w1:special"),
    "failed_keeps_scores": ("a200:failed", "w1:failed", "w1_min:failed", "odd:failed", "q257:failed"),
}


def test_every_mutant_is_listed():
    assert set(DISTINGUISHED_BY) == set(MM.MUTANTS)


@pytest.mark.parametrize("mutant,name", [(m, c) for m, cases in DISTINGUISHED_BY.items() for c in cases])
def test_a_wrong_rule_changes_the_output(mutant, name):
    assert name in MC.MERGE_CASES
    c = MC.merge_case(name)
    assert not _same(MM.exchange(c["scores"], c["ids"], c["status"], c["k_out"], mutant), MC.expected(name)), \
        f"{mutant} leaves {name} as it is"
