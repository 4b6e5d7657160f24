"""-m gpu: candidate-list search under a model (nann_search_candidates_model / retrieval.search_candidates_model).  The
attention model against the CPU oracle -- oracle.attn_score_rows on the gathered rows of a list, then oracle.topk of
min(k, len) (test_candidates_model_cpu.candidate_attn_topk) -- and, bit for bit, against the device's own exhaustive scan
(search_all_model scores every (user, row) with the same block functions on the same table row); the l2 / mlp models against
search_candidates.  Inputs are seeded and generated here; corpora, models' weights and users are those of
test_search_all_model_gpu.py at 1 000 and 3 001 rows (the call never reads the graph)."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest
import torch

from gpu_util import bits, cuda, require_gpu, tolerant_parity
from test_candidates_cpu import RAGGED, RANGE, SPLIT_CASES, well_formed
from test_candidates_model_cpu import CHUNK, candidate_attn_topk
from test_search_all_model_gpu import L_SEQ, RTOL, _corpus, _model, _oracle_scorer, _seq64

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu
N, N_SMALL = 3001, 1000
FIELDS = ("index", "pos", "scores", "item_ids", "n_out", "status")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


# ---- helpers -----------------------------------------------------------------------------------------------------------
def _numpy(r):
    torch.cuda.synchronize()
    return {f: getattr(r, f).cpu().numpy() for f in FIELDS}


def _run(dix, model, seqs, lists, k, options=None):
    from nann_amd import retrieval
    return _numpy(retrieval.search_candidates_model(dix, model, cuda(seqs, torch.float16), candidates=lists, k=k, options=options))


def _assert_same(got, exp, what="", only=None):
    sel = slice(None) if only is None else list(only)
    for f in ("status", "n_out", "index", "pos", "item_ids"):
        assert (got[f][sel] == exp[f][sel]).all(), (what, f)
    assert (bits(got["scores"][sel]) == bits(exp["scores"][sel])).all(), (what, "scores")


def _same_row(a, i, b, j, what=""):
    for f in ("status", "n_out"):
        assert a[f][i] == b[f][j], (what, f)
    for f in ("index", "pos", "item_ids"):
        assert (a[f][i] == b[f][j]).all(), (what, f)
    assert (bits(a["scores"][i]) == bits(b["scores"][j])).all(), (what, "scores")


def _zeros_behind(got, b, m, what=""):
    for f in ("index", "pos", "scores", "item_ids"):
        assert (got[f][b, m:] == 0).all(), (what, b, f)


def _random_lists(lengths, seed, n):
    """random rows with repeats, one list per length"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, n, int(m)).astype(np.int64) for m in lengths]


# ---- 1. parity with the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,precision,rows", [(64, "split", "f16"), (64, "exact", "f16"), (128, "split", "f16"),
                                              (128, "exact", "f16"), (64, "split", "bf16")])
def test_parity_with_the_oracle(oracle, tmp_path, d, precision, rows):
    from nann_amd import retrieval
    r = retrieval.CANDIDATE_ATTN_BLOCK_ROWS
    host, oix, dix, code, tdt, seqs = _corpus(N, d, rows)
    osc, am = _oracle_scorer(oracle, d, code)
    lengths = [0, 1, 31, 32, 33, 255, 256, 257, r - 1, r, r + 1, 2 * r + 1]
    rng = np.random.default_rng(101)
    # duplicate-free where the corpus allows it (the oracle compares by position either way)
    lists = [rng.choice(N, m, replace=m > N).astype(np.int64) for m in lengths]
    k = 200
    got = _run(dix, _model(tmp_path, d, precision, tdt), seqs[:12], lists, k)
    assert (got["status"] == 0).all()
    assert got["n_out"].tolist() == [min(k, m) for m in lengths]
    verdicts = []
    for u, lst in enumerate(lists):
        m = min(k, len(lst))
        _zeros_behind(got, u, m, (d, precision, rows))
        if m == 0:
            continue
        pos, idx, sc = got["pos"][u, :m], got["index"][u, :m], got["scores"][u, :m]
        assert (idx == lst[pos]).all() and (got["item_ids"][u, :m] == oix.ids[idx]).all(), u
        rc, own = oracle.attn_score_rows(am, seqs[u].astype(np.float32), host[idx])
        assert rc == 0
        err = np.abs(sc - own) / np.maximum(1.0, np.abs(own))
        exp_pos, _, exp_scores = candidate_attn_topk(oracle, am, seqs[u], host, lst, k)
        verdicts.append(tolerant_parity(pos, sc, exp_pos, exp_scores, rtol=RTOL))
        print("user %d (%d rows): %s, max score error on the returned rows %.3g" % (u, len(lst), verdicts[-1], err.max()))
        assert (err <= RTOL).all(), (u, float(err.max()))
    assert set(verdicts) <= {"exact", "near-tie"}, verdicts


# ---- 2. the bits of the exhaustive scan -----------------------------------------------------------------------------------
def _stable_topk(scores, k):
    """descending, -0 = +0, ties -> the lower position"""
    key = scores + np.float32(0.0)
    return np.argsort(-key, kind="stable")[:min(k, len(scores))]


@pytest.mark.parametrize("precision", ["split", "exact"])
def test_bitwise_against_the_exhaustive_scan(tmp_path, precision):
    from nann_amd import retrieval
    host, oix, dix, code, tdt, seqs = _corpus(N_SMALL, 64)
    m = _model(tmp_path, 64, precision)
    seq = cuda(seqs[:6], torch.float16)
    r = retrieval.search_all_model(dix, m, seq, N_SMALL)  # k = n: the device's own score of every (user, row)
    torch.cuda.synchronize()
    all_rows, all_scores = r.index.cpu().numpy(), r.scores.cpu().numpy()
    score_of = np.zeros((6, N_SMALL), np.float32)
    for u in range(6):
        assert sorted(all_rows[u].tolist()) == list(range(N_SMALL))
        score_of[u, all_rows[u]] = all_scores[u]
    lists = _random_lists([7, 64, 65, 300, 1500, 0], seed=102, n=N_SMALL)
    lists[3][200] = lists[3][10]  # a row listed twice for certain
    for k in (200, 1, 1024):
        got = _run(dix, m, seqs[:6], lists, k)
        assert (got["status"] == 0).all()
        for u, lst in enumerate(lists):
            own = score_of[u, lst]
            pos = _stable_topk(own, k)
            mm = len(pos)
            assert got["n_out"][u] == mm == min(k, len(lst)), (k, u)
            _zeros_behind(got, u, mm, k)
            assert (got["pos"][u, :mm] == pos).all(), (k, u)
            assert (got["index"][u, :mm] == lst[pos]).all() and (got["item_ids"][u, :mm] == oix.ids[lst[pos]]).all(), (k, u)
            assert (bits(got["scores"][u, :mm]) == bits(own[pos])).all(), (k, u)
    # (k = 1024 returned every entry of the 300-row list) the row listed twice: twice, equal bits, the lower position first
    twice = np.flatnonzero(got["index"][3, :300] == lists[3][10])
    assert len(twice) == int((lists[3] == lists[3][10]).sum()) >= 2
    assert len(set(bits(got["scores"][3, twice]).tolist())) == 1 and (np.diff(got["pos"][3, twice]) > 0).all()


# ---- 3. batch independence across the 128-user chunk ----------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["split", "exact"])
def test_answer_does_not_depend_on_the_batch(tmp_path, precision):
    """130 users cross the chunk: the probe at position 129 is user 1 of the SECOND chunk, scored with keys [129 - 128]"""
    from nann_amd import synth
    assert CHUNK == 128
    host, oix, dix, code, tdt, seqs = _corpus(N, 64)
    m = _model(tmp_path, 64, precision)
    probe, probe_list = seqs[3], _random_lists([300], seed=103, n=N)[0]
    alone = _run(dix, m, probe[None], [probe_list], 200)
    assert alone["status"][0] == 0 and alone["n_out"][0] == 200
    filler = _seq64(synth.make_queries(host, np.zeros(len(host), np.int32), 130, seq_len=L_SEQ, seed=5))
    filler_lists = _random_lists(np.random.default_rng(104).integers(0, 41, 130), seed=105, n=N)
    for b, at in ((3, 1), (130, 129)):
        batch, lists = filler[:b].copy(), [l for l in filler_lists[:b]]
        batch[at], lists[at] = probe, probe_list
        got = _run(dix, m, batch, lists, 200)
        assert (got["status"] == 0).all() and got["n_out"].tolist() == [min(200, len(l)) for l in lists]
        _same_row(got, at, alone, 0, (b, at))


# ---- 4. failures stay with their user -------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["split", "exact"])
def test_failures_stay_with_their_user(tmp_path, precision):
    from nann_amd import retrieval
    host, oix, dix, code, tdt, seqs = _corpus(N, 64)
    m = _model(tmp_path, 64, precision)
    seq3 = cuda(seqs[:3], torch.float16)
    for name, (splits, n_cand, ok) in SPLIT_CASES.items():
        assert well_formed(splits, n_cand).tolist() == ok
        rows = np.random.default_rng(106).integers(0, N, n_cand).astype(np.int64)
        got = _numpy(retrieval.search_candidates_model(dix, m, seq3, candidates=(torch.tensor(splits, dtype=torch.int64), torch.tensor(rows)), k=8))
        clean_lists = [rows[splits[i]:splits[i + 1]] if ok[i] else rows[:0] for i in range(3)]
        clean = _run(dix, m, seqs[:3], clean_lists, 8)  # the batch without the ill-formed lists
        assert (clean["status"] == 0).all()
        for i in range(3):
            if ok[i]:
                assert got["n_out"][i] == min(8, len(clean_lists[i]))
                _same_row(got, i, clean, i, (name, i))
            else:
                assert got["status"][i] == RAGGED and got["n_out"][i] == 0, (name, i)
                _zeros_behind(got, i, 0, name)
    # a row outside [0, n_items): status 5 for its user alone
    lists = _random_lists([300, 5, 600, 0, 64], seed=107, n=N)
    clean = _run(dix, m, seqs[:5], lists, 200)
    assert (clean["status"] == 0).all() and clean["n_out"].tolist() == [200, 5, 200, 0, 64]
    for victim, bad in ((0, -1), (2, N)):
        broken = [l.copy() for l in lists]
        broken[victim][len(broken[victim]) // 2] = bad
        got = _run(dix, m, seqs[:5], broken, 200)
        assert got["status"].tolist() == [RANGE if i == victim else 0 for i in range(5)], (victim, bad)
        assert got["n_out"][victim] == 0
        _zeros_behind(got, victim, 0, (victim, bad))
        _assert_same(got, clean, (victim, bad, "the others"), only=[i for i in range(5) if i != victim])
    _assert_same(_run(dix, m, seqs[:5], lists, 200), clean, "a clean call afterwards")


# ---- 5. l2 and mlp models: the bits of search_candidates ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["l2", "mlp"])
def test_l2_and_mlp_models_equal_search_candidates(tmp_path, kind):
    from nann_amd import ops, retrieval, synth
    host, oix, dix, code, tdt, _ = _corpus(N, 64)
    seqs = synth.make_queries(host, np.zeros(len(host), np.int32), 9, seq_len=L_SEQ, seed=8)  # [9, 50, 64]
    ops.save_scorer_dir(str(tmp_path / kind), kind, synth.make_mlp_weights(64) if kind == "mlp" else None,
                        precision=None if kind == "l2" else "exact")
    m = ops.Model(str(tmp_path / kind), 64, L_SEQ)
    lists = _random_lists([0, 1, 33, 200, 201, 700, 1500, 4097, 64], seed=108, n=N)
    got = _run(dix, m, seqs, lists, 200)
    exp = _numpy(retrieval.search_candidates(dix, m, cuda(seqs), candidates=lists, k=200))
    assert (got["status"] == 0).all() and got["n_out"].tolist() == [min(200, len(l)) for l in lists]
    _assert_same(got, exp, kind)
    with pytest.raises(TypeError):  # an ops.Scorer is search_candidates'
        retrieval.search_candidates_model(dix, ops.Scorer("l2", 64), cuda(seqs), candidates=lists, k=200)


# ---- 6. the call-level contract through the C ABI -------------------------------------------------------------------------
class _Call:
    """one nann_search_candidates_model call through ctypes with every argument replaceable; outputs pre-filled with a sentinel"""

    def __init__(self, dix, model, seqs, lists, k):
        from nann_amd import _lib
        self.L = _lib.lib()
        self.dix, self.model, self.k, self.b = dix, model, k, len(lists)
        self.seq = cuda(seqs, torch.float16)
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
        st = self.L.nann_search_candidates_model_workspace_bytes(kw.get("ix", self.dix.handle), kw.get("model", self.model.handle),
                                                                 kw.get("n_users", self.b), kw.get("n_cand", self.n_cand),
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
        options = kw.get("options")
        st = self.L.nann_search_candidates_model(kw.get("ix", self.dix.handle), kw.get("model", self.model.handle),
                                                 None if kw.get("no_seq") else _ptr(self.seq), kw.get("n_users", self.b),
                                                 kw.get("k", self.k), None if kw.get("no_cand") else C.byref(cand),
                                                 _ptr(o["item_ids"]), _ptr(o["scores"]), _ptr(o["index"]), _ptr(o["pos"]),
                                                 _ptr(o["n_out"]), _ptr(o["status"]), _ptr(ws), kw.get("ws_bytes", self.nbytes),
                                                 C.byref(options) if options is not None else None, _stream())
        torch.cuda.synchronize()
        return st


def _up256(v):
    return (v + 255) // 256 * 256


def _documented_bytes(n_users, n_cand):
    """the header's layout: scores, plan, item_off, and kt 64 KB + upad 16 KB for each user of ONE chunk"""
    return _up256(4 * n_cand) + _up256(16 * n_users) + _up256(8 * (n_users + 1)) + _up256(min(n_users, CHUNK) * (64 + 16) * 1024)


def test_contract_errors_and_no_ops(tmp_path):
    from nann_amd import ops, retrieval
    host, oix, dix, code, tdt, seqs = _corpus(N_SMALL, 64)
    m = _model(tmp_path, 64, "split")
    lists = _random_lists([30, 0, 500, 8], seed=109, n=N_SMALL)
    call = _Call(dix, m, seqs[:4], lists, 16)
    L = call.L
    bad, unsupported, capacity = 7, 102, 103
    m128 = _model(tmp_path, 128, "split")
    off = retrieval.search_options(preprojection=False)
    for what, kw, code_ in (("model of another d", {"model": m128.handle}, bad), ("k > 1024", {"k": 1025}, unsupported),
                            ("preprojection = 0", {"options": off}, unsupported),
                            ("workspace one byte short", {"ws_bytes": call.nbytes - 1}, capacity),
                            ("workspace off the 256-byte grid", {"ws": call.ws[8:]}, bad),
                            ("null index", {"ix": None}, bad), ("null model", {"model": None}, bad), ("null lists", {"no_cand": True}, bad),
                            ("struct_bytes", {"struct_bytes": 8}, bad), ("n_users < 0", {"n_users": -1}, bad),
                            ("n_cand < 0", {"n_cand": -1}, bad), ("k < 0", {"k": -1}, bad), ("rows == NULL", {"rows": None}, bad),
                            ("row_splits == NULL", {"row_splits": None}, bad), ("comm_seq == NULL", {"no_seq": True}, bad),
                            ("out_item_ids == NULL", {"null": ("item_ids",)}, bad), ("status == NULL", {"null": ("status",)}, bad),
                            ("n_cand > 2^31 - 1", {"n_cand": 2 ** 31, "ws_bytes": 1 << 40}, unsupported),
                            ("no workspace", {"ws": None, "ws_bytes": 0}, capacity)):
        assert call(**kw) == code_, (what, L.nann_last_error())
        assert call.untouched(), what
        if what == "model of another d":
            assert b"disagree" in L.nann_last_error()
        if what == "preprojection = 0":
            assert b"preprojection" in L.nann_last_error()
        if what == "workspace off the 256-byte grid":
            assert b"aligned" in L.nann_last_error()
    for kw, code_ in (({"ix": None}, bad), ({"model": None}, bad), ({"n_users": -1}, bad), ({"n_cand": -1}, bad), ({"k": -1}, bad),
                      ({"model": m128.handle}, bad), ({"k": 1025}, unsupported), ({"n_cand": 2 ** 31}, unsupported),
                      ({"n_users": 2 ** 31}, unsupported)):
        assert call.ws_bytes(**kw)[0] == code_, kw
    with pytest.raises(ops.NannError) as e:
        _run(dix, m, seqs[:4], lists, 16, options=off)
    assert e.value.status == 102 and "preprojection" in str(e.value)
    # n_users == 0, k == 0: NANN_OK, nothing written, no workspace needed
    assert call(n_users=0) == 0 and call(k=0) == 0 and call(k=0, ws=None, ws_bytes=0) == 0
    assert call.untouched()
    assert call.ws_bytes(k=0) == (0, 0) and call.ws_bytes(n_users=0) == (0, 0)
    # the size is the documented function of (n_users, n_cand), the per-user side that of min(n_users, 128) users
    assert call.nbytes == _documented_bytes(4, call.n_cand)
    for nu, nc in ((130, 5000), (128, 5000), (129, 1), (1000, 0)):
        assert call.ws_bytes(n_users=nu, n_cand=nc) == (0, _documented_bytes(nu, nc)), (nu, nc)
    assert _documented_bytes(130, 5000) - _documented_bytes(128, 5000) == _up256(16 * 130) - _up256(16 * 128) + _up256(8 * 131) - _up256(8 * 129)
    # exactly the reported size: the answer of the Python call
    exp = _run(dix, m, seqs[:4], lists, 16)
    assert call() == 0
    _assert_same({f: t.cpu().numpy() for f, t in call.out.items()}, exp, "every output")
    call.fill()
    assert call(null=("scores", "index", "pos", "n_out")) == 0  # the optional outputs
    got = {f: t.cpu().numpy() for f, t in call.out.items()}
    assert (got["item_ids"] == exp["item_ids"]).all() and (got["status"] == 0).all()
    assert all((got[f] == -77).all() for f in ("scores", "index", "pos", "n_out"))
    # every list empty, rows == NULL: zeros
    empty = _Call(dix, m, seqs[:4], [np.zeros(0, np.int64)] * 4, 16)
    assert empty(rows=None) == 0
    got = {f: t.cpu().numpy() for f, t in empty.out.items()}
    assert all((got[f] == 0).all() for f in got)


# ---- 7. lifecycle of the table --------------------------------------------------------------------------------------------
def _table_bytes(model, dix):
    from nann_amd import _lib
    tb, rb = C.c_int64(-1), C.c_int64(-1)
    assert _lib.lib().nann_model_table_bytes(model.handle, dix.handle, C.byref(tb), C.byref(rb)) == 0
    return tb.value, rb.value


@pytest.mark.parametrize("precision", ["split", "exact"])
def test_table_built_in_the_call_or_prepared(tmp_path, precision):
    from nann_amd import retrieval
    host, oix, dix, code, tdt, seqs = _corpus(N, 64)
    lists = _random_lists([300, 0, 64, 1500, 33, 257], seed=110, n=N)
    m = _model(tmp_path, 64, precision)
    assert _table_bytes(m, dix)[1] == 0
    built_in_call = _run(dix, m, seqs[:6], lists, 200)    # an unprepared pair: the table is built inside the call
    tb, rb = _table_bytes(m, dix)
    assert tb == N * 384 * 4 and rb >= tb
    m2 = _model(tmp_path, 64, precision, name="again")
    retrieval.prepare(dix, m2)                            # a pinned table is found
    try:
        before = _table_bytes(m2, dix)
        assert before[0] == N * 384 * 4 and before[1] >= before[0]
        prepared = _run(dix, m2, seqs[:6], lists, 200)
        assert _table_bytes(m2, dix) == before
    finally:
        retrieval.release(dix, m2)
    assert (built_in_call["status"] == 0).all() and built_in_call["n_out"].tolist() == [200, 0, 64, 200, 33, 200]
    _assert_same(prepared, built_in_call, precision)


# ---- 8. re-entrancy -------------------------------------------------------------------------------------------------------
def test_two_threads_share_index_and_model(tmp_path):
    from nann_amd import retrieval
    host, oix, dix, code, tdt, seqs = _corpus(N, 64)
    lists = _random_lists([300, 0, 64, 700, 33, 257, 1, 512], seed=111, n=N)
    halves = [(seqs[:4], lists[:4]), (seqs[4:8], lists[4:])]
    ref_model = _model(tmp_path, 64, "split", name="ref")
    ref = [_run(dix, ref_model, s, l, 200) for s, l in halves]  # each thread's work, single-threaded
    m = _model(tmp_path, 64, "split", name="shared")  # unprepared: the threads race for the table's build
    got, errors = [None, None], []
    start = threading.Barrier(2)

    def work(i):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                sd = cuda(halves[i][0], torch.float16)
                start.wait()
                for _ in range(3):
                    r = retrieval.search_candidates_model(dix, m, sd, candidates=halves[i][1], k=200)
                stream.synchronize()
                got[i] = {f: getattr(r, f).cpu().numpy() for f in FIELDS}
        except Exception as e:  # noqa: BLE001 -- reported by the asserting thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    _assert_same(got[0], ref[0], "thread 0")
    _assert_same(got[1], ref[1], "thread 1")
