"""-m gpu: the streamed scalar-quantised search (nann_search_all_sq8_stream, retrieval.search_all_sq8_stream) against the numpy
model of its contract (sq8_stream_model on sq8_model), BIT FOR BIT: the cut, the survivor counts, completeness, and the result with
the exact scores taken from nann_score (ops.blaze_score) as test_sq8_gpu.py takes them.  No tolerance appears anywhere.
n_items = 2 * 1024 + 37: three blocks of kSq8RowsPerWg rows, a ragged last 32-row group, rows behind the table."""
import ctypes as C

import numpy as np
import pytest
import torch

import sq8_model as M
import sq8_stream_model as SM
from gpu_util import bits, cuda, require_gpu
from test_sq8_gpu import _index, _rows, _scorer, _status

pytestmark = pytest.mark.gpu
F = np.float32
N, NQ, K = 2 * 1024 + 37, 133, 10
SAMPLES = (700, 1500)   # below one block; spanning two
# the planted row's copies, either side of 32-row group and block boundaries: ten inside both samples, four between, four outside
TIES = (31, 32, 63, 64, 95, 96, 511, 512, 640, 641, 1022, 1023, 1024, 1025, 1600, 2047, 2048, N - 1)
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def inputs(d, dtype, metric):
    """(rows, queries f32[NQ, d], approximate scores of the model) -- numpy only.  Query 0 is the planted row: a row of the
    greatest norm copied to TIES, so that under either metric its copies share the best approximate score."""
    key = ("in", d, dtype, metric)
    if key not in _CACHE:
        x = _rows(N, d, 11 + d, dtype)
        w = M.widen(x)
        big = w[np.argmax((w.astype(np.float64) ** 2).sum(axis=1))] * F(2.0)
        x[list(TIES)] = big.astype(np.float16) if dtype == "f16" else (big.view(np.uint32) >> 16).astype(np.uint16)
        q = np.random.default_rng(d).standard_normal((NQ, d)).astype(F)
        q[0] = M.widen(x[TIES[0]:TIES[0] + 1])[0]
        _CACHE[key] = (x, q, M.approx_scores(M.encode(q), M.encode(x), metric))
    return _CACHE[key]


def device(d, dtype, metric):
    """(index, code table, scorer, exact_of from nann_score's bits of every (query, row)) -- made once per case"""
    from nann_amd import ops, retrieval
    key = ("dev", d, dtype)
    if key not in _CACHE:
        dix = _index(inputs(d, dtype, metric)[0])
        _CACHE[key] = (dix, retrieval.make_sq8(dix))
    dix, t = _CACHE[key]
    sc = _scorer(metric, d, torch.float16 if dtype == "f16" else torch.bfloat16)
    if ("exact", d, dtype, metric) not in _CACHE:
        q, every = inputs(d, dtype, metric)[1], cuda(np.arange(N, dtype=np.int32))
        _CACHE["exact", d, dtype, metric] = np.stack([ops.blaze_score(sc, cuda(v), table=dix.item_embs, indices=every).cpu().numpy() for v in q])
    exact = _CACHE["exact", d, dtype, metric]
    return dix, t, sc, lambda qi, rows: exact[qi][rows]


def run(dix, t, sc, q, k, fetch, sample_rows, cap, fallback=False):
    from nann_amd import retrieval
    r = retrieval.search_all_sq8_stream(dix, t, sc, cuda(q, torch.float32), k, fetch=fetch, sample_rows=sample_rows, cap=cap,
                                        fallback=fallback, return_stats=True)
    torch.cuda.synchronize()
    return [a.cpu().numpy() for a in (r.index, r.scores, r.item_ids, r.complete, r.n_survivors, r.cut)]


def same(got, exp, ids_of, what):
    rows, scores, ids, complete, n_surv, cut = got
    e_rows, e_scores, e_complete, e_surv, e_cut = exp
    assert (bits(cut) == bits(e_cut)).all() and (n_surv == e_surv).all() and (complete == e_complete).all(), what
    assert (rows == e_rows).all() and (bits(scores) == bits(e_scores)).all() and (ids == ids_of[e_rows]).all(), what


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d", [64, 128, 256, 512])
def test_stream_equals_the_model(d, dtype, metric):
    """1 query (a partial tile), 33 (two tiles), 133 (two chunks, a partial last tile); both samples; fetch k and 3k; a cap that
    every query fits.  Query 0: every copy of the planted row ties the cut and survives, inside the sample and outside, in row order."""
    x, q, approx = inputs(d, dtype, metric)
    dix, t, sc, exact_of = device(d, dtype, metric)
    ids_of = dix.item_ids.cpu().numpy()
    for sample_rows in SAMPLES:
        for fetch in (K, 3 * K):
            exp = SM.search(approx, sample_rows, fetch, N, K, exact_of)
            if fetch == K:  # the precondition of the tie case, on the model: K copies lie in either sample, so the cut is their score
                assert (approx[0, list(TIES)] == exp[4][0]).all() and exp[3][0] == len(TIES) and (approx[0] > exp[4][0]).sum() == 0
                assert exp[0][0].tolist() == list(TIES[:K])
            assert (exp[2] == 1).all() and (exp[3] >= fetch).all() and exp[3].max() > fetch
            for b in (1, 33, NQ):
                same(run(dix, t, sc, q[:b], K, fetch, sample_rows, N), [e[:b] for e in exp], ids_of, (sample_rows, fetch, b))


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_whole_table_sample_equals_search_all_sq8(metric):
    from nann_amd import retrieval
    d, dtype = 128, "f16"
    x, q, approx = inputs(d, dtype, metric)
    dix, t, sc, exact_of = device(d, dtype, metric)
    fetch = 3 * K
    # the planted copies tie one another under every query: where they straddle the cut, S_q is the fetch list plus the copies behind
    # it -- identical rows at higher row numbers, which lose every tie of the re-rank, so the result is search_all_sq8's all the same
    counts = SM.survivors(approx, SM.cut(approx, N, fetch), N)[1]
    assert (counts == fetch).sum() >= 100
    for sample_rows in (N, N + 5):
        got = run(dix, t, sc, q, K, fetch, sample_rows, N)
        ref = retrieval.search_all_sq8(dix, t, sc, cuda(q), K, fetch=fetch, return_fetch=True)
        assert (got[0] == ref.index.cpu().numpy()).all() and (bits(got[1]) == bits(ref.scores.cpu().numpy())).all()
        assert (got[2] == ref.item_ids.cpu().numpy()).all() and (got[3] == 1).all() and (got[4] == counts).all()
        assert (bits(got[5]) == bits(ref.fetch_scores.cpu().numpy()[:, -1])).all()


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d", [64, 512])
def test_overflow_keeps_the_first_cap_survivors_and_falls_back(d, metric):
    from nann_amd import retrieval
    x, q, approx = inputs(d, "f16", metric)
    dix, t, sc, exact_of = device(d, "f16", metric)
    fetch, sample_rows = 3 * K, SAMPLES[0]
    counts = SM.survivors(approx, SM.cut(approx, sample_rows, fetch), N)[1]
    cap = int(np.median(counts))
    exp = SM.search(approx, sample_rows, fetch, cap, K, exact_of)
    over = exp[2] == 0
    assert K <= cap and 20 <= over.sum() <= NQ - 20 and (exp[3] == counts).all() and (counts[over] > cap).all()
    same(run(dix, t, sc, q, K, fetch, sample_rows, cap), exp, dix.item_ids.cpu().numpy(), "truncated")
    got = run(dix, t, sc, q, K, fetch, sample_rows, cap, fallback=True)
    ref = retrieval.search_all_sq8(dix, t, sc, cuda(q), K, fetch=fetch)
    assert (got[0][over] == ref.index.cpu().numpy()[over]).all() and (bits(got[1][over]) == bits(ref.scores.cpu().numpy()[over])).all()
    assert (got[0][~over] == exp[0][~over]).all() and (got[3] == exp[2]).all() and (got[4] == counts).all()


def test_answer_does_not_depend_on_the_batch():
    for metric in ("l2", "ip"):
        x, q, approx = inputs(128, "f16", metric)
        dix, t, sc, exact_of = device(128, "f16", metric)
        batch = run(dix, t, sc, q, K, 3 * K, SAMPLES[1], 44)
        alone = run(dix, t, sc, q[130:131], K, 3 * K, SAMPLES[1], 44)
        assert 0 < batch[3].sum() < NQ
        for a, b in zip(batch, alone):
            assert a[130].tobytes() == b[0].tobytes()


def test_failure_codes_and_the_workspace_rule():
    from nann_amd import _lib, ops, synth
    from nann_amd.ops import _ptr, _stream
    from nann_amd import retrieval
    x, q, approx = inputs(64, "f16", "l2")
    dix, t, sc, exact_of = device(64, "f16", "l2")
    qd = cuda(q[:4])
    call = lambda **kw: retrieval.search_all_sq8_stream(dix, t, kw.pop("sc", sc), qd, **kw)  # noqa: E731
    assert _status(lambda: call(k=10, fetch=20, cap=9)) == 7                     # cap < k
    assert _status(lambda: call(k=10, fetch=20, sample_rows=-1)) == 7            # sample_rows < 0
    assert _status(lambda: call(k=11, fetch=10)) == 7 and _status(lambda: call(k=10, fetch=1025)) == 102
    mlp = ops.Scorer("mlp", 64, torch.float16, synth.make_mlp_weights(64), precision="exact")
    assert _status(lambda: call(sc=mlp, k=10, fetch=20)) == 102
    assert _status(lambda: call(k=10, fetch=20, cap=10)) == 0                    # k <= cap < fetch: legal, every query incomplete
    L = _lib.lib()
    nb = C.c_int64(-1)
    size = lambda n, k: L.nann_search_all_sq8_stream_workspace_bytes(dix.handle, t.handle, sc.handle, n, 20, 700, 64, k, C.byref(nb))  # noqa: E731
    assert size(4, 0) == 0 and nb.value == 0 and size(0, 10) == 0 and nb.value == 0 and size(4, 10) == 0 and nb.value > 0
    ws = torch.full((nb.value + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    out_ids = torch.full((4, 10), -77, dtype=torch.int64, device="cuda")
    complete = torch.full((4,), -77, dtype=torch.int32, device="cuda")

    def raw(nbytes, n=4, k=10):
        st = L.nann_search_all_sq8_stream(dix.handle, t.handle, sc.handle, _ptr(qd), n, 20, 700, 64, k, _ptr(out_ids), None, None,
                                          _ptr(complete), None, None, _ptr(ws), nbytes, None, _stream())
        torch.cuda.synchronize()
        return st
    assert raw(nb.value - 1) == 103 and raw(nb.value, n=0) == 0 and raw(nb.value, k=0) == 0
    assert (out_ids == -77).all() and (complete == -77).all() and (ws == 0xA5).all()
    assert raw(nb.value) == 0 and (ws[nb.value:] == 0xA5).all(), "the call wrote behind its workspace"
    ref = run(dix, t, sc, q[:4], 10, 20, 700, 64)
    assert (out_ids.cpu().numpy() == ref[2]).all() and (complete.cpu().numpy() == ref[3]).all()
