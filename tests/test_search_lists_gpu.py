"""GPU: the shared-list search (nann_search_lists) against its definition -- nann_search_candidates over the concatenation of
the lists a query names -- and against the per-row reference scores, bit for bit; the partition's CSR against the numpy model."""
import numpy as np
import pytest
import torch

import ip_reference as R
from gpu_util import bits, cuda, require_gpu
from lists_model import expansion, partition_csr
from test_candidates_gpu import _assert_same, _expect, _l2_case, _numpy, _queries, _run
from test_search_all_gpu import _TORCH_DT, _indices, _oracle_dt, _rows

pytestmark = pytest.mark.gpu
N = 3001  # the corpus of test_candidates_gpu._l2_case
LENGTHS = [0, 1, 255, 256, 257, 700, 300, 40]  # list 6 is probed by nobody
B = 37


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _list_of_row(seed=5):
    """LENGTHS rows per list, scattered over the corpus; every other row in no list"""
    lor = np.full(N, -1, np.int32)
    lor[np.random.default_rng(seed).permutation(N)[:sum(LENGTHS)]] = np.repeat(np.arange(len(LENGTHS)), LENGTHS)
    return lor


def _probes():
    """list 3 by every query (three tiles), list 4 by 17 (two tiles), list 2 by query 5 alone, lists 0 (empty), 1 and 5 by some;
    negative slots.  Column 2 alone (the n_probe = 1 case): query 35 names only the empty list, query 36 nothing"""
    p = np.full((B, 4), -1, np.int32)
    p[:, 0] = 3
    p[:17, 1] = 4
    p[::2, 2] = 5
    p[5, 2] = 2
    p[0::3, 3] = 1
    p[1::3, 3] = 0
    p[35] = [3, -1, 0, -1]
    p[36] = [3, -1, -1, -1]
    return p


def _search(dix, part, sc, q, probes, k):
    from nann_amd import retrieval
    return _numpy(retrieval.search_lists(dix, part, sc, cuda(q, torch.float32), cuda(probes, torch.int32), k))


def _ip_expect(q, embs, item_ids, lists, k):
    """_expect's dict under the inner product: the canonical order in numpy (ip_reference)"""
    exp = {f: [] for f in ("pos", "index", "scores", "item_ids", "n_out")}
    for v, rows in zip(q, lists):
        s = R.ip_scores(v, R.widen(embs[rows])) if len(rows) else np.zeros(0, np.float32)
        pos = R.topk_stable(s, min(k, len(rows)))
        pad = np.zeros(k - len(pos), np.int64)
        for f, a in (("pos", pos), ("index", rows[pos]), ("scores", s[pos]), ("item_ids", item_ids[rows[pos]])):
            exp[f].append(np.concatenate([a, pad.astype(a.dtype)]))
        exp["n_out"].append(len(pos))
    out = {f: np.stack(v) if f != "n_out" else np.array(v, np.int32) for f, v in exp.items()}
    out["status"] = np.zeros(len(lists), np.int32)
    return out


# ---- 1. every path of the scan: one panel, two panels, f32 panels, the deepest tree; both metrics ------------------------------
@pytest.mark.parametrize("kind", ["l2", "ip"])
@pytest.mark.parametrize("d,dtype", [(64, "f16"), (128, "bf16"), (64, "f32"), (512, "f16")])
def test_equals_candidates_on_the_expansion(oracle, d, dtype, kind):
    from nann_amd import ops, retrieval
    embs, oix, dix = _l2_case(d, dtype)
    part = retrieval.make_partition(dix, _list_of_row(), len(LENGTHS))
    splits, rows = partition_csr(_list_of_row(), len(LENGTHS))
    sc = ops.Scorer(kind, d, _TORCH_DT[dtype])
    q = _queries(B, d, seed=d + 2)
    for probes in (_probes(), _probes()[:, 2:3]):  # n_probe 4 and 1
        lists = [expansion(splits, rows, p) for p in probes]
        for k in (10, 300):
            got = _search(dix, part, sc, q, probes, k)
            assert got["n_out"].tolist() == [min(k, len(l)) for l in lists]
            _assert_same(got, _run(dix, sc, q, lists, k), (d, dtype, kind, probes.shape[1], k, "candidates"))
            if kind == "l2":
                exp = _expect(oracle, oracle.Scorer("l2", d, _oracle_dt(oracle, dtype)), q, embs, oix.ids, lists, k)
                _assert_same(got, exp, (d, dtype, k, "oracle"))
            else:
                some = [0, 5, 20]
                _assert_same({f: v[some] for f, v in got.items()},
                             _ip_expect(q[some], embs, oix.ids, [lists[i] for i in some], k), (d, dtype, k, "numpy"))


def test_many_slots_two_slabs_two_chunks(oracle):
    """150 queries x 40 slots: two chunks of queries, 5 120 pairs in a chunk's plan (a thread of the plan owns 8 places of the
    sorted order, tiles of every fill), S = 40 x 700 positions per query (two slabs of the selection), lists named many times"""
    from nann_amd import ops, retrieval
    embs, oix, dix = _l2_case(64, "f16")
    part = retrieval.make_partition(dix, _list_of_row(), len(LENGTHS))
    splits, rows = partition_csr(_list_of_row(), len(LENGTHS))
    sc = ops.Scorer("l2", 64)
    rng = np.random.default_rng(7)
    probes = rng.integers(-1, len(LENGTHS), (150, 40)).astype(np.int32)
    probes[3] = 5  # the longest concatenation the workspace is sized for
    q = _queries(150, 64, seed=8)
    lists = [expansion(splits, rows, p) for p in probes]
    _assert_same(_search(dix, part, sc, q, probes, 300), _run(dix, sc, q, lists, 300), "150 x 40")


# ---- 2. ties: the position order is the candidate call's ----------------------------------------------------------------------
def test_ties_go_to_the_lower_position_of_the_concatenation(oracle):
    from nann_amd import ops, retrieval
    embs = _rows(N, 128, "f16", seed=32).copy()
    embs[100:160] = embs[100]  # 60 identical rows, 20 in each of the three lists
    oix, dix = _indices(embs)
    lor = (np.arange(N) % 3).astype(np.int32)
    part = retrieval.make_partition(dix, lor, 3)
    splits, rows = partition_csr(lor, 3)
    sc = ops.Scorer("l2", 128)
    probes = np.array([[1, 0, -1], [0, 1, 0], [2, 2, 1]], np.int32)  # list 0 and list 2 named twice
    q = np.stack([embs[100].astype(np.float32)] * 3)
    lists = [expansion(splits, rows, p) for p in probes]
    for k in (200, 1024):
        got = _search(dix, part, sc, q, probes, k)
        _assert_same(got, _run(dix, sc, q, lists, k), ("ties", k))
        _assert_same(got, _expect(oracle, oracle.Scorer("l2", 128, oracle.EMB_F16), q, embs, oix.ids, lists, k), ("ties", k, "oracle"))
    # 20 twins per list: 40, 60 and 60 entries at score 0 lead the three answers, in position order
    for i, m in enumerate((40, 60, 60)):
        assert (got["scores"][i, :m] == 0).all() and got["scores"][i, m] < 0 and (np.diff(got["pos"][i, :m]) > 0).all()
    assert (got["index"][2, :20] == got["index"][2, 20:40]).all()  # a list named twice returns its rows twice


# ---- 3. a slot >= n_lists fails its query alone; the call-level refusals ------------------------------------------------------
def test_a_bad_slot_fails_its_query_alone(oracle):
    from nann_amd import ops, retrieval
    embs, oix, dix = _l2_case(64, "f16")
    part = retrieval.make_partition(dix, _list_of_row(), len(LENGTHS))
    sc = ops.Scorer("l2", 64)
    q = _queries(B, 64, seed=41)
    good, bad = _probes(), _probes()
    bad[[3, 16, 36], [1, 3, 0]] = [len(LENGTHS), 2 ** 31 - 1, len(LENGTHS)]
    got, ref = _search(dix, part, sc, q, bad, 50), _search(dix, part, sc, q, good, 50)
    failed = [3, 16, 36]
    assert got["status"][failed].tolist() == [5, 5, 5] and (got["n_out"][failed] == 0).all()
    assert all((got[f][failed] == 0).all() for f in ("index", "pos", "item_ids", "scores"))
    _assert_same(got, ref, "the others", only=[i for i in range(B) if i not in failed])


def test_call_level_refusals(oracle):
    from nann_amd import ops, retrieval, synth
    embs, oix, dix = _l2_case(64, "f16")
    part = retrieval.make_partition(dix, _list_of_row(), len(LENGTHS))
    sc, q = ops.Scorer("l2", 64), cuda(_queries(2, 64, seed=43), torch.float32)

    def status(call):
        with pytest.raises(ops.NannError) as e:
            call()
        return e.value.status

    assert status(lambda: retrieval.search_lists(dix, part, sc, q, np.zeros((2, 1), np.int32), 1025)) == 102
    assert status(lambda: retrieval.search_lists(dix, part, sc, q, np.zeros((2, 65), np.int32), 10)) == 102
    assert status(lambda: retrieval.search_lists(dix, part, sc, q, np.zeros((2, 1), np.int32), -1)) == 7
    mlp = ops.Scorer("mlp", 64, torch.float16, synth.make_mlp_weights(64), precision="exact")
    assert status(lambda: retrieval.search_lists(dix, part, mlp, q, np.zeros((2, 1), np.int32), 10)) == 102
    other = _indices(embs[:100])[1]
    assert status(lambda: retrieval.search_lists(other, part, sc, q, np.zeros((2, 1), np.int32), 10)) == 7
    lor = _list_of_row()
    lor[7] = len(LENGTHS)
    assert status(lambda: retrieval.make_partition(dix, lor, len(LENGTHS))) == 5
    r = retrieval.search_lists(dix, part, sc, q, np.zeros((2, 0), np.int32), 10)  # no slots: every query is empty
    torch.cuda.synchronize()
    assert r.n_out.tolist() == [0, 0] and r.status.tolist() == [0, 0]


# ---- 4. a query's answer does not depend on its batch --------------------------------------------------------------------------
def test_answer_does_not_depend_on_the_batch(oracle):
    from nann_amd import ops, retrieval
    embs, oix, dix = _l2_case(128, "bf16")
    part = retrieval.make_partition(dix, _list_of_row(), len(LENGTHS))
    sc = ops.Scorer("ip", 128, torch.bfloat16)
    q, probes = _queries(B, 128, seed=51), _probes()
    batch = _search(dix, part, sc, q, probes, 200)
    for i in (0, 5, 16, 35):
        alone = _search(dix, part, sc, q[i:i + 1], probes[i:i + 1], 200)
        _assert_same(alone, {f: v[i:i + 1] for f, v in batch.items()}, ("alone", i))


# ---- 5. the partition's CSR ----------------------------------------------------------------------------------------------------
def test_partition_view_equals_the_model():
    from nann_amd import retrieval
    n = 9001  # three row groups of the build, the last one ragged
    dix = _indices(_rows(n, 64, "f16", seed=61))[1]
    rng = np.random.default_rng(62)
    lor = rng.integers(-3, 70, n).astype(np.int32)
    lor[2000:2600] = (np.arange(600) // 7) % 70  # neighbours that share a list: peers within a wavefront
    lor[4090:4200] = 69                          # one list across a group boundary
    part = retrieval.make_partition(dix, lor, 72)  # lists 70 and 71 stay empty
    splits, rows = partition_csr(lor, 72)
    assert (part.n_lists, part.n_listed_rows, part.max_len) == (72, len(rows), int(np.diff(splits).max()))
    assert part.list_splits().cpu().numpy().tolist() == splits.tolist()
    assert (part.list_rows().cpu().numpy() == rows).all()
    empty = retrieval.make_partition(dix, np.full(n, -1, np.int32), 0)
    assert (empty.n_listed_rows, empty.max_len) == (0, 0) and empty.list_splits().cpu().numpy().tolist() == [0]


# ---- 6. IVF in one line: every cell probed is the exhaustive search ------------------------------------------------------------
@pytest.mark.parametrize("kind", ["l2", "ip"])
def test_search_partitioned_over_every_cell_equals_search_all(kind):
    from nann_amd import ops, retrieval
    embs, oix, dix = _l2_case(64, "f32")  # (f32 rows of a normal sample: no two scores of a query tie)
    part, cent = retrieval.train_partition(dix, 8, iters=3, seed=1)
    assert part.n_listed_rows == N and tuple(cent.shape) == (8, 64)
    sc, q = ops.Scorer(kind, 64, torch.float32), cuda(_queries(B, 64, seed=71), torch.float32)
    got, ref = retrieval.search_partitioned(dix, part, cent, sc, q, 50, n_probe=8), retrieval.search_all(dix, sc, q, 50)
    torch.cuda.synchronize()
    assert (got.n_out == 50).all() and (got.status == 0).all()
    assert (got.index == ref.index).all() and (got.item_ids == ref.item_ids).all()
    assert (bits(got.scores.cpu().numpy()) == bits(ref.scores.cpu().numpy())).all()
