"""-m gpu: candidate-list search on the device (nann_search_candidates / retrieval.search_candidates) against the CPU oracle.
The expected value everywhere is oracle.score_rows on the gathered rows of a list followed by oracle.topk of min(k, len):
rows = list[pos], item_ids = ids[rows] (test_candidates_cpu.candidate_topk).  Inputs are seeded and generated here; the indices
carry the ring graph of test_search_all_gpu.py, since the call never reads the graph.

Not reachable at these sizes: the `near` addressing branch of wg_score_l2_part (one 24-bit multiply-add per row address) needs
a table beyond 4 GB or more than 2^24 rows to be switched OFF, and every table here switches it on; the flag's expression is
kept textually the one k_search passes (test_candidates_cpu.test_l2_scorer_keeps_the_traversal_addressing_flag), so the far
branch is the one the traversal's own large-index tests cover."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest
import torch

from gpu_util import bits, cuda, require_gpu, tolerant_parity
from test_candidates_cpu import RAGGED, RANGE, SPLIT_CASES, candidate_topk, well_formed
from test_search_all_gpu import _TORCH_DT, _indices, _oracle_dt, _rows

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu
N = 3001
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


# ---- helpers -----------------------------------------------------------------------------------------------------------
def _lists(lengths, seed, n=N):
    """random rows with repeats, one list per length"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, n, int(m)).astype(np.int64) for m in lengths]


def _expect(oracle, osc, q, embs, item_ids, lists, k, failed=None):
    """the outputs of a call as the contract states them: n_out entries at the head of every row, zeros behind; `failed`:
    {query: status} of the queries that get a status and a zeroed row"""
    b = len(lists)
    exp = {"index": np.zeros((b, k), np.int32), "pos": np.zeros((b, k), np.int32), "scores": np.zeros((b, k), np.float32),
           "item_ids": np.zeros((b, k), np.int64), "n_out": np.zeros(b, np.int32), "status": np.zeros(b, np.int32)}
    for i, rows in enumerate(lists):
        if failed and i in failed:
            exp["status"][i] = failed[i]
            continue
        pos, r, s = candidate_topk(oracle, osc, q[i], embs, rows, k)
        m = len(pos)
        exp["n_out"][i] = m
        exp["pos"][i, :m], exp["index"][i, :m], exp["scores"][i, :m], exp["item_ids"][i, :m] = pos, r, s, item_ids[r]
    return exp


def _numpy(r):
    torch.cuda.synchronize()
    return {f: getattr(r, f).cpu().numpy() for f in ("index", "pos", "scores", "item_ids", "n_out", "status")}


def _run(dix, scorer, q, lists, k, options=None):
    from nann_amd import retrieval
    return _numpy(retrieval.search_candidates(dix, scorer, cuda(q, torch.float32), candidates=lists, k=k, options=options))


def _assert_same(got, exp, what="", only=None):
    sel = slice(None) if only is None else list(only)
    for f in ("status", "n_out", "index", "pos", "item_ids"):
        assert (got[f][sel] == exp[f][sel]).all(), (what, f)
    assert (bits(got["scores"][sel]) == bits(exp["scores"][sel])).all(), (what, "scores")


def _l2_case(d, dtype):
    key = ("l2", d, dtype)
    if key not in _CACHE:
        embs = _rows(N, d, dtype, seed=d + len(dtype))
        _CACHE[key] = (embs,) + _indices(embs)
    return _CACHE[key]


def _queries(b, d, seed):
    return np.random.default_rng(seed).standard_normal((b, d)).astype(np.float32)


# ---- 1. L2, bitwise, every d x row dtype --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("d", [64, 128, 256, 512])
def test_l2_bitwise_every_shape(oracle, d, dtype):
    from nann_amd import ops
    embs, oix, dix = _l2_case(d, dtype)
    lists = _lists([0, 1, 7, 64, 65, 199, 200, 201, 1500], seed=d)
    q = _queries(len(lists), d, seed=d + 1)
    sc, osc = ops.Scorer("l2", d, _TORCH_DT[dtype]), oracle.Scorer("l2", d, _oracle_dt(oracle, dtype))
    for k in (200, 1, 1024) if (d, dtype) == (128, "f16") else (200,):
        exp = _expect(oracle, osc, q, embs, oix.ids, lists, k)
        assert exp["n_out"].tolist() == [min(k, len(l)) for l in lists]
        _assert_same(_run(dix, sc, q, lists, k), exp, (d, dtype, k))


# ---- 2. block edges -----------------------------------------------------------------------------------------------------
def test_scoring_block_edges(oracle):
    from nann_amd import ops, retrieval
    c = retrieval.CANDIDATE_BLOCK_ROWS
    embs, oix, dix = _l2_case(64, "f16")
    sc, osc = ops.Scorer("l2", 64), oracle.Scorer("l2", 64, oracle.EMB_F16)
    lists = _lists([c - 1, c, c + 1, 2 * c + 1], seed=21)
    q = _queries(4, 64, seed=22)
    _assert_same(_run(dix, sc, q, lists, 200), _expect(oracle, osc, q, embs, oix.ids, lists, 200), "C - 1, C, C + 1, 2 C + 1")


def test_many_short_lists_share_a_block(oracle):
    from nann_amd import ops
    embs, oix, dix = _l2_case(64, "f16")
    sc, osc = ops.Scorer("l2", 64), oracle.Scorer("l2", 64, oracle.EMB_F16)
    lengths = np.random.default_rng(23).integers(0, 41, 70)
    lengths[[0, 5, 69]] = [0, 40, 0]
    lists = _lists(lengths, seed=24)
    q = _queries(70, 64, seed=25)
    for k in (200, 16):
        _assert_same(_run(dix, sc, q, lists, k), _expect(oracle, osc, q, embs, oix.ids, lists, k), ("70 short lists", k))


def test_register_path_edge_of_the_selection(oracle):
    """16 384 entries: the longest list wg_topk keeps in registers; 16 385: the form that re-reads its keys from memory"""
    from nann_amd import ops
    embs, oix, dix = _l2_case(64, "f16")
    sc, osc = ops.Scorer("l2", 64), oracle.Scorer("l2", 64, oracle.EMB_F16)
    lists = _lists([16384, 16385, 3], seed=26)
    q = _queries(3, 64, seed=27)
    _assert_same(_run(dix, sc, q, lists, 200), _expect(oracle, osc, q, embs, oix.ids, lists, 200), "16384 / 16385")


# ---- 3. ties ------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_position(oracle):
    from nann_amd import ops
    rng = np.random.default_rng(31)
    embs = _rows(N, 128, "f16", seed=32).copy()
    embs[100:150] = embs[100]  # 50 identical rows
    oix, dix = _indices(embs)
    sc, osc = ops.Scorer("l2", 128), oracle.Scorer("l2", 128, oracle.EMB_F16)
    repeated = rng.integers(0, N, 900).astype(np.int64)
    repeated[rng.choice(900, 300, replace=False)] = 777                     # one row 300 times among others
    twins = rng.permutation(np.concatenate([np.arange(100, 150), rng.integers(0, N, 400)])).astype(np.int64)
    all_equal = rng.integers(100, 150, 500).astype(np.int64)                # every score the same
    lists = [repeated, twins, all_equal]
    q = np.stack([embs[777].astype(np.float32), embs[100].astype(np.float32), _queries(1, 128, 33)[0]])
    for k in (200, 1024):
        exp = _expect(oracle, osc, q, embs, oix.ids, lists, k)
        got = _run(dix, sc, q, lists, k)
        _assert_same(got, exp, ("ties", k))
        for b in range(3):
            m = int(got["n_out"][b])
            s, p = got["scores"][b, :m], got["pos"][b, :m]
            same = bits(s[1:] + np.float32(0)) == bits(s[:-1] + np.float32(0))
            assert (np.diff(p)[same] > 0).all(), (b, k)
    assert (got["scores"][0, :300] == 0).all() and (got["index"][0, :300] == 777).all()   # the corpus does what it was built for
    assert (np.isin(got["index"][1, :50], np.arange(100, 150))).all()
    assert got["pos"][2, :500].tolist() == list(range(500))


# ---- 4. MLP -------------------------------------------------------------------------------------------------------------
MLP_LENGTHS = [0, 1, 31, 32, 33, 4095, 4096, 4097]


def _mlp_case(oracle):
    """d = 128, f16, metric weights; the lists, queries and the oracle's answer at k = 200, computed once"""
    if "mlp" not in _CACHE:
        from nann_amd import synth
        embs = _rows(N, 128, "f16", seed=41)
        oix, dix = _indices(embs)
        w = synth.make_mlp_weights_metric(128, embs)
        lists = _lists(MLP_LENGTHS, seed=42)
        q = (embs[np.random.default_rng(43).integers(0, N, len(lists))].astype(np.float32) + 0.05 * _queries(len(lists), 128, 44))
        exp = _expect(oracle, oracle.Scorer("mlp", 128, oracle.EMB_F16, w), q, embs, oix.ids, lists, 200)
        _CACHE["mlp"] = (embs, oix, dix, w, lists, q, exp)
    return _CACHE["mlp"]


@pytest.mark.parametrize("precision", ["exact", "certified"])
def test_mlp_exact_and_certified_bitwise(oracle, precision):
    from nann_amd import ops
    embs, oix, dix, w, lists, q, exp = _mlp_case(oracle)
    sc = ops.Scorer("mlp", 128, torch.float16, w, precision=precision)
    _assert_same(_run(dix, sc, q, lists, 200), exp, precision)


def test_mlp_split_within_tolerance(oracle):
    from nann_amd import ops
    embs, oix, dix, w, lists, q, exp = _mlp_case(oracle)
    got = _run(dix, ops.Scorer("mlp", 128, torch.float16, w, precision="split"), q, lists, 200)
    assert (got["status"] == 0).all() and (got["n_out"] == exp["n_out"]).all()
    for b, rows in enumerate(lists):
        m = int(exp["n_out"][b])
        if m:  # positions are the unique ids of a list's entries (its rows repeat)
            verdict = tolerant_parity(got["pos"][b, :m], got["scores"][b, :m], exp["pos"][b, :m], exp["scores"][b, :m], rtol=1e-5)
            assert verdict in ("exact", "near-tie"), (b, verdict)
            assert (got["index"][b, :m] == rows[got["pos"][b, :m]]).all()
        assert (got["item_ids"][b, :m] == oix.ids[got["index"][b, :m]]).all()
        for f in ("index", "pos", "scores", "item_ids"):
            assert (got[f][b, m:] == 0).all()


def test_mlp_without_a_table(oracle):
    from nann_amd import ops, retrieval
    embs, oix, dix, w, lists, q, exp = _mlp_case(oracle)
    sc = ops.Scorer("mlp", 128, torch.float16, w, precision="exact")
    with pytest.raises(ops.UnimplementedError) as e:
        _run(dix, sc, q, lists, 200, options=retrieval.search_options(preprojection=False))
    assert e.value.status == 102 and "preprojection" in str(e.value)


# ---- 5. cross-checks against the calls the library already has ---------------------------------------------------------
def _allow_lists(b, seed):
    rng = np.random.default_rng(seed)
    return [np.sort(rng.choice(N, int(m), replace=False)).astype(np.int64) for m in rng.integers(1, 700, b)]


def _scorers(oracle, which):
    from nann_amd import ops
    if which == "l2":
        embs, oix, dix = _l2_case(128, "f16")
        return embs, oix, dix, ops.Scorer("l2", 128), _queries(6, 128, seed=51)
    embs, oix, dix, w, lists, q, exp = _mlp_case(oracle)
    return embs, oix, dix, ops.Scorer("mlp", 128, torch.float16, w, precision="exact"), q[:6]


@pytest.mark.parametrize("which", ["l2", "mlp"])
def test_sorted_allow_lists_equal_filtered_search_all(oracle, which):
    """ascending duplicate-free lists = the top k of the allowed rows: search_all with the complement denied, query by query
    (a deny bitmap serves every query of a call, so each list is a call of its own)"""
    from nann_amd import retrieval
    embs, oix, dix, sc, q = _scorers(oracle, which)
    lists = _allow_lists(len(q), seed=52)
    lists[0] = lists[0][:37]  # fewer allowed rows than k
    got = _run(dix, sc, q, lists, 200)
    assert (got["status"] == 0).all()
    for b, allowed in enumerate(lists):
        f = retrieval.make_filter(dix, deny_rows=np.setdiff1d(np.arange(N), allowed))
        r = retrieval.search_all(dix, sc, cuda(q[b:b + 1]), 200, filter=f)
        torch.cuda.synchronize()
        m = int(r.n_out[0])
        assert m == got["n_out"][b] == min(200, len(allowed))
        assert (r.index[0, :m].cpu().numpy() == got["index"][b, :m]).all(), b
        assert (bits(r.scores[0, :m].cpu().numpy()) == bits(got["scores"][b, :m])).all(), b


@pytest.mark.parametrize("which", ["l2", "mlp"])
def test_equals_the_per_query_device_loop(oracle, which):
    from nann_amd import ops
    embs, oix, dix, sc, q = _scorers(oracle, which)
    lists = _lists([1, 33, 200, 201, 700, 1500], seed=53)
    got = _run(dix, sc, q, lists, 200)
    for b, rows in enumerate(lists):
        m = min(200, len(rows))
        v, i = ops.top_k(ops.blaze_score(sc, cuda(q[b]), table=dix.item_embs, indices=cuda(rows, torch.int32)), m)
        assert (i.cpu().numpy() == got["pos"][b, :m]).all() and (bits(v.cpu().numpy()) == bits(got["scores"][b, :m])).all(), b
        assert (rows[got["pos"][b, :m]] == got["index"][b, :m]).all()


# ---- 6. per-query failures ----------------------------------------------------------------------------------------------
def test_a_bad_row_fails_its_query_alone(oracle):
    from nann_amd import ops
    embs, oix, dix = _l2_case(128, "f16")
    sc, osc = ops.Scorer("l2", 128), oracle.Scorer("l2", 128, oracle.EMB_F16)
    lists = _lists([300, 5, 1500, 0, 64, 2100], seed=61)
    q = _queries(len(lists), 128, seed=62)
    clean = _expect(oracle, osc, q, embs, oix.ids, lists, 200)
    _assert_same(_run(dix, sc, q, lists, 200), clean, "clean")
    for victim, bad in ((0, -1), (2, N), (5, 2 ** 31 - 1), (1, -2 ** 31)):
        broken = [l.copy() for l in lists]
        broken[victim][len(broken[victim]) // 2] = bad
        got = _run(dix, sc, q, broken, 200)
        exp = _expect(oracle, osc, q, embs, oix.ids, lists, 200, failed={victim: RANGE})
        _assert_same(got, exp, (victim, bad))
        others = [b for b in range(len(lists)) if b != victim]
        _assert_same(got, clean, (victim, bad, "the others"), only=others)
    # the same under the MLP scorer, whose block functions clamp the row themselves
    membs, moix, mdix, w, mlists, mq, mexp = _mlp_case(oracle)
    msc = ops.Scorer("mlp", 128, torch.float16, w, precision="exact")
    broken = [l.copy() for l in mlists]
    broken[6][2000] = N
    got = _run(mdix, msc, mq, broken, 200)
    assert got["status"].tolist() == [0] * 6 + [RANGE, 0] and got["n_out"][6] == 0 and (got["item_ids"][6] == 0).all()
    _assert_same(got, mexp, "mlp, the others", only=[0, 1, 2, 3, 4, 5, 7])
    _assert_same(_run(dix, sc, q, lists, 200), clean, "a clean call afterwards")


def test_ill_formed_splits_fail_their_queries_alone(oracle):
    from nann_amd import ops, retrieval
    embs, oix, dix = _l2_case(128, "f16")
    sc, osc = ops.Scorer("l2", 128), oracle.Scorer("l2", 128, oracle.EMB_F16)
    q = _queries(3, 128, seed=63)
    qd = cuda(q)
    for name, (splits, n_cand, ok) in SPLIT_CASES.items():
        assert well_formed(splits, n_cand).tolist() == ok
        rows = np.random.default_rng(64).integers(0, N, n_cand).astype(np.int64)
        r = _numpy(retrieval.search_candidates(dix, sc, qd, candidates=(torch.tensor(splits, dtype=torch.int64), torch.tensor(rows)), k=8))
        lists = [rows[splits[i]:splits[i + 1]] if ok[i] else rows[:0] for i in range(3)]
        exp = _expect(oracle, osc, q, embs, oix.ids, lists, 8, failed={i: RAGGED for i in range(3) if not ok[i]})
        _assert_same(r, exp, name)
    lists = _lists([10, 0, 300], seed=65)  # the stream is still usable: a clean call gives the right answer
    _assert_same(_run(dix, sc, q, lists, 8), _expect(oracle, osc, q, embs, oix.ids, lists, 8), "afterwards")


# ---- 7. batch independence, re-entrancy ---------------------------------------------------------------------------------
def test_answer_does_not_depend_on_the_batch(oracle):
    from nann_amd import ops
    embs, oix, dix = _l2_case(128, "f16")
    sc = ops.Scorer("l2", 128)
    lists = _lists([0, 1, 7, 64, 65, 199, 200, 201, 1500, 2049], seed=71)
    q = _queries(len(lists), 128, seed=72)
    batch = _run(dix, sc, q, lists, 200)
    for b in range(len(lists)):
        alone = _run(dix, sc, q[b:b + 1], lists[b:b + 1], 200)
        for f in ("status", "n_out", "index", "pos", "item_ids"):
            assert (alone[f][0] == batch[f][b]).all(), (b, f)
        assert (bits(alone["scores"][0]) == bits(batch["scores"][b])).all(), b


def test_two_threads_share_index_and_scorer(oracle):
    from nann_amd import ops, retrieval
    embs, oix, dix, w, lists, q, exp = _mlp_case(oracle)
    sc = ops.Scorer("mlp", 128, torch.float16, w, precision="exact")  # unprepared: the threads race for the table's build
    got, errors = [None, None], []
    start = threading.Barrier(2)

    def work(i):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                qd = cuda(q, torch.float32)
                start.wait()
                for _ in range(3):
                    r = retrieval.search_candidates(dix, sc, qd, candidates=lists, k=200)
                stream.synchronize()
                got[i] = {f: getattr(r, f).cpu().numpy() for f in ("index", "pos", "scores", "item_ids", "n_out", "status")}
        except Exception as e:  # noqa: BLE001 -- reported by the asserting thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    _assert_same(got[0], exp, "thread 0")
    _assert_same(got[1], exp, "thread 1")


# ---- 8. the call-level contract -----------------------------------------------------------------------------------------
class _Call:
    """one nann_search_candidates call through ctypes with every argument replaceable; outputs pre-filled with a sentinel"""

    def __init__(self, dix, sc, q, lists, k):
        from nann_amd import _lib
        self.L = _lib.lib()
        self.dix, self.sc, self.k, self.b = dix, sc, k, len(lists)
        self.q = cuda(q, torch.float32)
        self.splits = cuda(np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64))
        self.rows = cuda(np.concatenate(lists).astype(np.int32))
        self.n_cand = int(self.rows.numel())
        st, self.nbytes = self.ws_bytes()
        assert st == 0 and self.nbytes > 0 and self.nbytes % 256 == 0
        self.ws = torch.zeros(self.nbytes + 256, dtype=torch.uint8, device="cuda")
        assert self.ws.data_ptr() % 256 == 0
        self.fill()

    def fill(self):
        kk = max(self.k, 1)
        self.out = {"item_ids": torch.full((self.b, kk), -77, dtype=torch.int64, device="cuda"),
                    "scores": torch.full((self.b, kk), -77.0, dtype=torch.float32, device="cuda"),
                    "index": torch.full((self.b, kk), -77, dtype=torch.int32, device="cuda"),
                    "pos": torch.full((self.b, kk), -77, dtype=torch.int32, device="cuda"),
                    "n_out": torch.full((self.b,), -77, dtype=torch.int32, device="cuda"),
                    "status": torch.full((self.b,), -77, dtype=torch.int32, device="cuda")}

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((t == -77).all()) for t in self.out.values())

    def ws_bytes(self, **kw):
        nb = C.c_int64(-1)
        st = self.L.nann_search_candidates_workspace_bytes(kw.get("ix", self.dix.handle), kw.get("scorer", self.sc.handle),
                                                           kw.get("n_queries", self.b), kw.get("n_cand", self.n_cand),
                                                           kw.get("k", self.k), C.byref(nb))
        return st, nb.value

    def __call__(self, **kw):
        from nann_amd import _lib
        from nann_amd.ops import _ptr, _stream
        cand = _lib.Candidates()
        cand.struct_bytes = kw.get("struct_bytes", C.sizeof(_lib.Candidates))
        cand.row_splits = kw.get("row_splits", self.splits.data_ptr())
        cand.rows = kw.get("rows", self.rows.data_ptr())
        cand.n_cand = kw.get("n_cand", self.n_cand)
        o = dict(self.out)
        for f in kw.get("null", ()):
            o[f] = None
        ws = kw.get("ws", self.ws)
        st = self.L.nann_search_candidates(kw.get("ix", self.dix.handle), kw.get("scorer", self.sc.handle), _ptr(self.q),
                                           kw.get("n_queries", self.b), kw.get("k", self.k),
                                           None if kw.get("no_cand") else C.byref(cand), _ptr(o["item_ids"]), _ptr(o["scores"]),
                                           _ptr(o["index"]), _ptr(o["pos"]), _ptr(o["n_out"]), _ptr(o["status"]), _ptr(ws),
                                           kw.get("ws_bytes", self.nbytes), None, _stream())
        torch.cuda.synchronize()
        return st


def test_call_level_contract(oracle):
    from nann_amd import ops
    embs, oix, dix = _l2_case(128, "f16")
    sc, osc = ops.Scorer("l2", 128), oracle.Scorer("l2", 128, oracle.EMB_F16)
    lists = _lists([30, 0, 500, 8], seed=81)
    q = _queries(4, 128, seed=82)
    call = _Call(dix, sc, q, lists, 16)
    L = call.L
    bad, unsupported, capacity = 7, 102, 103
    other_d = ops.Scorer("l2", 64)
    other_dt = ops.Scorer("l2", 128, torch.bfloat16)
    for what, kw, code in (("null index", {"ix": None}, bad), ("null scorer", {"scorer": None}, bad), ("null lists", {"no_cand": True}, bad),
                           ("struct_bytes", {"struct_bytes": 8}, bad), ("n_queries < 0", {"n_queries": -1}, bad),
                           ("n_cand < 0", {"n_cand": -1}, bad), ("k < 0", {"k": -1}, bad), ("rows == NULL", {"rows": None}, bad),
                           ("row_splits == NULL", {"row_splits": None}, bad), ("scorer of another d", {"scorer": other_d.handle}, bad),
                           ("scorer of another dtype", {"scorer": other_dt.handle}, bad), ("k > 1024", {"k": 1025}, unsupported),
                           ("n_cand > 2^31 - 1", {"n_cand": 2 ** 31, "ws_bytes": 1 << 40}, unsupported),
                           ("workspace one byte short", {"ws_bytes": call.nbytes - 1}, capacity),
                           ("no workspace", {"ws": None, "ws_bytes": 0}, capacity),
                           ("workspace off the 256-byte grid", {"ws": call.ws[8:]}, bad)):
        assert call(**kw) == code, (what, L.nann_last_error())
        assert call.untouched(), what
    assert b"aligned" in L.nann_last_error()
    for kw, code in (({"ix": None}, bad), ({"scorer": None}, bad), ({"n_queries": -1}, bad), ({"n_cand": -1}, bad), ({"k": -1}, bad),
                     ({"scorer": other_d.handle}, bad), ({"k": 1025}, unsupported), ({"n_cand": 2 ** 31}, unsupported)):
        assert call.ws_bytes(**kw)[0] == code, kw
    # k == 0, n_queries == 0: NANN_OK, nothing written, no workspace needed
    assert call(k=0) == 0 and call(n_queries=0) == 0 and call(k=0, ws=None, ws_bytes=0) == 0
    assert call.untouched()
    assert call.ws_bytes(k=0) == (0, 0) and call.ws_bytes(n_queries=0) == (0, 0)
    # k above n_items is served (lists may repeat rows); no list at all is served
    assert call.ws_bytes(k=1024)[0] == 0
    # exactly the reported size; the optional outputs NULL, one at a time and together
    exp = _expect(oracle, osc, q, embs, oix.ids, lists, 16)
    assert call() == 0
    _assert_same({f: t.cpu().numpy() for f, t in call.out.items()}, exp, "every output")
    for null in (("scores",), ("index",), ("pos",), ("n_out",), ("scores", "index", "pos", "n_out")):
        call.fill()
        assert call(null=null) == 0, null
        got = {f: t.cpu().numpy() for f, t in call.out.items()}
        for f in ("item_ids", "scores", "index", "pos", "n_out", "status"):
            if f in null:
                assert (got[f] == -77).all(), (null, f)
            elif f == "scores":
                assert (bits(got[f]) == bits(exp[f])).all(), (null, f)
            else:
                assert (got[f] == exp[f]).all(), (null, f)
    # n_cand == 0 with rows == NULL: every list is empty
    empty = _Call(dix, sc, q, [np.zeros(0, np.int64)] * 4, 16)
    assert empty(rows=None) == 0
    got = {f: t.cpu().numpy() for f, t in empty.out.items()}
    assert all((got[f] == 0).all() for f in got)


# ---- 9. the Python surface ----------------------------------------------------------------------------------------------
def test_candidate_item_ids(oracle):
    from nann_amd import ops, retrieval
    embs, oix, dix = _l2_case(128, "f16")
    sc = ops.Scorer("l2", 128)
    lists = _lists([40, 0, 300, 9], seed=91)
    q = cuda(_queries(4, 128, seed=92))
    by_row = _numpy(retrieval.search_candidates(dix, sc, q, candidates=lists, k=50))
    as_ids = [oix.ids[l] for l in lists]
    assert all((retrieval._rows_of_item_ids(dix, a).cpu().numpy() == l).all() for a, l in zip(as_ids, lists))
    assert all((retrieval._rows_of_item_ids_kept(dix, a).cpu().numpy() == l).all() for a, l in zip(as_ids, lists))
    by_id = _numpy(retrieval.search_candidates(dix, sc, q, candidate_item_ids=as_ids, k=50))
    _assert_same(by_id, by_row, "item ids")
    splits = torch.tensor(np.concatenate([[0], np.cumsum([len(l) for l in lists])]))
    _assert_same(_numpy(retrieval.search_candidates(dix, sc, q, candidate_item_ids=(splits, torch.tensor(np.concatenate(as_ids))), k=50)),
                 by_row, "item ids as a (row_splits, ids) pair")
    as_ids[2] = as_ids[2].copy()
    as_ids[2][150] = 5  # no row has item id 5 (ids are 7 r + 3)
    assert retrieval._rows_of_item_ids_kept(dix, as_ids[2]).cpu().numpy()[150] == -1
    unknown = _numpy(retrieval.search_candidates(dix, sc, q, candidate_item_ids=as_ids, k=50))
    assert unknown["status"].tolist() == [0, 0, RANGE, 0] and unknown["n_out"][2] == 0 and (unknown["item_ids"][2] == 0).all()
    _assert_same(unknown, by_row, "the others", only=[0, 1, 3])
    with pytest.raises(AssertionError):
        retrieval.search_candidates(dix, sc, q, k=50)


def test_models(oracle, tmp_path):
    from nann_amd import ops, retrieval, synth
    embs, oix, dix, w, lists, q, exp = _mlp_case(oracle)
    seqs = cuda(np.random.default_rng(93).standard_normal((len(lists), 5, 128)).astype(np.float16))
    ops.save_scorer_dir(str(tmp_path / "mlp"), "mlp", {name: np.ascontiguousarray(a) for name, a in w.items()}, precision="exact")
    model = ops.Model(str(tmp_path / "mlp"), 128, seq_len=5)
    assert model.kind == "mlp"
    by_model = _numpy(retrieval.search_candidates(dix, model, seqs, candidates=lists, k=200))
    sc = ops.Scorer("mlp", 128, torch.float16, w, precision="exact")
    by_scorer = _numpy(retrieval.search_candidates(dix, sc, ops.user_seq_mean(seqs), candidates=lists, k=200))
    _assert_same(by_model, by_scorer, "mlp model")
    assert (by_model["n_out"] == exp["n_out"]).all()
    ops.save_scorer_dir(str(tmp_path / "attn"), "attention", synth.make_attn_weights(64), precision="exact")
    with pytest.raises(NotImplementedError):  # (refused by its kind, before anything about it is compared with the index)
        retrieval.search_candidates(dix, ops.Model(str(tmp_path / "attn"), 64, seq_len=5), seqs, candidates=lists, k=200)
