"""-m gpu: range search (nann_search_all_range / nann_search_all_range_model; retrieval.search_all_range) against the CPU oracle.
Expected values: oracle.brute_force(k = n_items) gives every row's score, range_model.reference applies `score >= thr and score
!= -inf` in numpy, rows ascending -- never the code under test (test 7 alone compares with the device's own search_all, which is
what pins "the bits of nann_search_all").  Equalities are bitwise on scores and exact on rows, row_splits and item ids; every
output is pre-filled with a sentinel and the untouched positions must still hold it.  The corpora carry a ring graph the scan
never reads; helpers are those of test_search_all_gpu.py and test_search_all_model_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import range_model as RM
from gpu_util import bits, cuda, require_gpu
from test_search_all_gpu import _TORCH_DT, _brute, _oracle_dt, _ring, _rows

pytestmark = pytest.mark.gpu
_CACHE = {}
S = RM.SENTINEL
OK, BAD, UNSUPPORTED, CAPACITY = 0, 7, 102, 103


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


# ---- helpers -----------------------------------------------------------------------------------------------------------
def _indices(embs):
    """(oracle index, device index); a single row links to itself"""
    from nann_amd import retrieval
    from oracle import oracle as O
    n = embs.shape[0]
    ids = np.arange(n, dtype=np.int64) * 7 + 3
    if n == 1:
        nbv, rs, ep = [np.zeros(1, np.int32)] * 2, [np.array([0, 1], np.int64)] * 2, np.zeros(1, np.int32)
    else:
        nbv, rs, ep = _ring(n)
    return O.Index(embs, ids, nbv, rs, ep), retrieval.Index(embs, ids, nbv, rs, ep)


def _matrix(rows, scores):
    """the oracle's full ranking -> scores f32[B, n] by row number"""
    out = np.empty(scores.shape, np.float32)
    np.put_along_axis(out, rows.astype(np.int64), scores, axis=1)
    return out


def _all_scores(oracle, oix, osc, q):
    return _matrix(*_brute(oracle, oix, osc, q, oix.ids.shape[0]))


class _Out:
    """sentinel-filled outputs of one call, `room` entries each"""

    def __init__(self, b, room):
        self.splits = torch.full((b + 1,), S, dtype=torch.int64, device="cuda")
        self.ids = torch.full((room,), S, dtype=torch.int64, device="cuda")
        self.scores = torch.full((room,), float(S), dtype=torch.float32, device="cuda")
        self.index = torch.full((room,), S, dtype=torch.int32, device="cuda")

    def numpy(self):
        torch.cuda.synchronize()
        return self.splits.cpu().numpy(), self.index.cpu().numpy(), self.scores.cpu().numpy(), self.ids.cpu().numpy()

    def untouched(self):
        return all(bool((a == S).all()) for a in self.numpy())


def _ws(dix, by, b, model=False):
    from nann_amd import _lib
    L = _lib.lib()
    nb = C.c_int64(-1)
    fn = L.nann_search_all_range_model_workspace_bytes if model else L.nann_search_all_range_workspace_bytes
    assert fn(dix.handle, by.handle, b, C.byref(nb)) == OK
    assert nb.value % 256 == 0
    return torch.zeros(max(nb.value, 256), dtype=torch.uint8, device="cuda"), nb.value


def _call(dix, by, x, thr, capacity, out, flt=None, model=False, null_entries=False, ws=None, options=None):
    """the C call; -> status"""
    from nann_amd import _lib
    from nann_amd.ops import _ptr, _stream
    L = _lib.lib()
    if ws is None:
        ws = _ws(dix, by, x.shape[0], model)[0]
    fn = L.nann_search_all_range_model if model else L.nann_search_all_range
    entries = (None, None, None) if null_entries else (_ptr(out.ids), _ptr(out.scores), _ptr(out.index))
    st = fn(dix.handle, by.handle, _ptr(x), x.shape[0], _ptr(thr), capacity, _ptr(out.splits), *entries, _ptr(ws), ws.numel(),
            C.byref(options) if options is not None else None, C.byref(flt.struct) if flt is not None else None, _stream())
    torch.cuda.synchronize()
    return st


def _range(dix, by, x, thr, room, capacity=None, **kw):
    """one call into fresh sentinel-filled outputs of `room` entries -> (row_splits, index, scores, item_ids) as numpy"""
    out = _Out(x.shape[0], room)
    assert _call(dix, by, x, cuda(np.asarray(thr, np.float32)), room if capacity is None else capacity, out, **kw) == OK
    return out.numpy()


def _assert_same(got, exp, what=""):
    for g, e, name in zip(got, exp, ("row_splits", "index", "scores", "item_ids")):
        assert g.shape == e.shape, (what, name)
        if name == "scores":
            g, e = bits(g), bits(e)
        assert (g == e).all(), (what, name, np.nonzero(g != e)[0][:5])


def _five_thresholds(full):
    """per query, cycled: above the maximum, the maximum, the median, the minimum, -inf (bit patterns of the oracle's scores)"""
    thr = np.zeros(full.shape[0], np.float32)
    for i in range(full.shape[0]):
        s = np.sort(full[i])
        thr[i] = [np.nextafter(s[-1], np.float32(np.inf)), s[-1], s[len(s) // 2], s[0], -np.inf][i % 5]
    return thr


# ---- 1. L2, shapes ----------------------------------------------------------------------------------------------------
B = RM.BLOCK
SHAPES = [(n, 64, "f16") for n in (1, 63, 64, 65, B - 1, B, B + 1, 16385, 40000)] + \
         [(5000, 128, "bf16"), (5000, 256, "f32"), (5000, 512, "f16")]


@pytest.mark.parametrize("n,d,dtype", SHAPES)
def test_l2_bitwise_every_shape(oracle, n, d, dtype):
    from nann_amd import ops
    embs = _rows(n, d, dtype, seed=n + d)
    oix, dix = _indices(embs)
    q = np.random.default_rng(n).standard_normal((17, d)).astype(np.float32)
    full = _all_scores(oracle, oix, oracle.Scorer("l2", d, _oracle_dt(oracle, dtype)), q)
    thr = _five_thresholds(full)
    room = 17 * n + 8
    exp = RM.reference(full, thr, oix.ids, room)
    counts = np.diff(exp[0])
    assert (counts[0::5] == 0).all() and (counts[1::5] >= 1).all() and (counts[3::5] == n).all() and (counts[4::5] == n).all()
    assert n == 1 or (counts[2::5] < n).all()
    _assert_same(_range(dix, ops.Scorer("l2", d, _TORCH_DT[dtype]), cuda(q), thr, room), exp, (n, d, dtype))


# ---- 2. ties and zeros ------------------------------------------------------------------------------------------------
def test_duplicated_rows_are_both_returned(oracle):
    from nann_amd import ops
    n, d = 3000, 64
    embs = _rows(n, d, "f16", seed=21)
    rng = np.random.default_rng(22)
    src, dst = rng.permutation(n)[:40].reshape(2, 20)
    embs[dst] = embs[src]
    oix, dix = _indices(embs)
    q = rng.standard_normal((20, d)).astype(np.float32)
    full = _all_scores(oracle, oix, oracle.Scorer("l2", d, oracle.EMB_F16), q)
    assert (bits(full[np.arange(20), src]) == bits(full[np.arange(20), dst])).all()
    thr = full[np.arange(20), src]  # query i: the score of its duplicated pair
    exp = RM.reference(full, thr, oix.ids, 20 * n)
    for i in range(20):
        seg = exp[1][exp[0][i]:exp[0][i + 1]]
        assert src[i] in seg and dst[i] in seg
    _assert_same(_range(dix, ops.Scorer("l2", d), cuda(q), thr, 20 * n), exp)


def test_zero_query_under_ip_and_a_nan_threshold():
    """an all-zero query scores +0 or -0 on every row: thr = +0.0 and thr = -0.0 return every row, the smallest positive number
    none, and NaN none.  Expected scores: the inner product's canonical order restated in numpy (ip_reference)."""
    from ip_reference import ip_scores, widen
    from nann_amd import ops
    n, d = 2500, 64
    embs = _rows(n, d, "f16", seed=23)
    oix, dix = _indices(embs)
    q = np.zeros((5, d), np.float32)
    q[1] = -0.0
    q[4] = np.random.default_rng(24).standard_normal(d)
    full = np.stack([ip_scores(v, widen(embs)) for v in q])
    assert (full[:4] == 0).all()
    thr = np.array([0.0, -0.0, np.float32(1e-45), np.nan, np.nan], np.float32)
    exp = RM.reference(full, thr, oix.ids, 2 * n + 4)
    assert np.diff(exp[0]).tolist() == [n, n, 0, 0, 0]
    _assert_same(_range(dix, ops.Scorer("ip", d), cuda(q), thr, 2 * n + 4), exp)


# ---- 3. chunks --------------------------------------------------------------------------------------------------------
def _chunk_case(oracle):
    if "chunk" not in _CACHE:
        n, d = 5000, 64
        embs = _rows(n, d, "f16", seed=31)
        oix, dix = _indices(embs)
        q = np.random.default_rng(32).standard_normal((257, d)).astype(np.float32)
        full = _all_scores(oracle, oix, oracle.Scorer("l2", d, oracle.EMB_F16), q)
        thr = np.array([np.sort(full[i])[::-1][[3, 40, 333, 0, 1200][i % 5]] for i in range(257)], np.float32)
        _CACHE["chunk"] = (oix, dix, q, full, thr)
    return _CACHE["chunk"]


@pytest.mark.parametrize("b", [130, 257])
def test_more_than_one_chunk(oracle, b):
    from nann_amd import ops
    oix, dix, q, full, thr = _chunk_case(oracle)
    sc = ops.Scorer("l2", 64)
    room = int(RM.reference(full[:b], thr[:b], oix.ids, 0)[0][-1]) + 16
    exp = RM.reference(full[:b], thr[:b], oix.ids, room)
    got = _range(dix, sc, cuda(q[:b]), thr[:b], room)
    _assert_same(got, exp, b)
    assert (np.diff(got[0]) >= 1).all() and got[0][128] == exp[0][128] and got[0][129] > got[0][128]  # no break at the border
    for i in (0, 127, 128, b - 1):  # each of them alone: the same segment
        alone = _range(dix, sc, cuda(q[i:i + 1]), thr[i:i + 1], 1300)
        lo, hi = exp[0][i], exp[0][i + 1]
        assert alone[0].tolist() == [0, hi - lo]
        for a, e in zip(alone[1:], exp[1:]):
            assert (bits(a[:hi - lo]) == bits(e[lo:hi])).all() if a.dtype == np.float32 else (a[:hi - lo] == e[lo:hi]).all(), i
            assert (a[hi - lo:] == S).all()


# ---- 4. capacity ------------------------------------------------------------------------------------------------------
def test_capacity_cuts_the_tail_and_nothing_else(oracle):
    from nann_amd import ops
    oix, dix, q, full, thr = _chunk_case(oracle)
    q, full = q[:64], full[:64]
    thr = np.array([np.sort(full[i])[::-1][250 + 3 * i] for i in range(64)], np.float32)  # a few hundred matches per query
    sc = ops.Scorer("l2", 64)
    total = int(RM.reference(full, thr, oix.ids, 0)[0][-1])
    room = total + 64
    whole = RM.reference(full, thr, oix.ids, room)
    assert (np.diff(whole[0]) >= 251 + 3 * np.arange(64)).all() and np.diff(whole[0]).max() < 500
    uncapped = _range(dix, sc, cuda(q), thr, room)
    _assert_same(uncapped, whole, "uncapped")
    for capacity in (total, total - 1, int(whole[0][31]) + 3, 1):
        got = _range(dix, sc, cuda(q), thr, room, capacity=capacity)
        cut = RM.reference(full, thr, oix.ids, capacity)
        _assert_same(got, cut[:1] + tuple(np.concatenate([a, np.full(room - capacity, S, a.dtype)]) for a in cut[1:]), capacity)
        assert (got[0] == uncapped[0]).all()
        for g, u in zip(got[1:], uncapped[1:]):
            assert (bits(g[:capacity]) == bits(u[:capacity])).all() if g.dtype == np.float32 else (g[:capacity] == u[:capacity]).all()
            assert (g[capacity:] == S).all(), capacity
    # count only: capacity 0, the three entry outputs NULL
    out = _Out(64, room)
    assert _call(dix, sc, cuda(q), cuda(thr), 0, out, null_entries=True) == OK
    got = out.numpy()
    assert (got[0] == whole[0]).all() and all((a == S).all() for a in got[1:])


# ---- 5. filter --------------------------------------------------------------------------------------------------------
def test_filter_denied_rows_never_come_back(oracle):
    from nann_amd import ops, retrieval
    oix, dix, q, full, thr = _chunk_case(oracle)
    b, n = 19, 5000
    q, full = q[:b], full[:b]
    rng = np.random.default_rng(51)
    deny = rng.random(n) < 0.3
    order = np.argsort(-full, axis=1, kind="stable")
    lists = [np.concatenate([order[i, :40:2], rng.integers(0, n, 30)]).astype(np.int64) for i in range(b)]
    lists[2] = np.concatenate([[-1, n, 2 ** 31 - 1], lists[2], [n + 5]])  # rows out of range deny nothing
    flt = retrieval.make_filter(dix, deny_rows=np.nonzero(deny)[0], exclude_rows=lists)
    splits = flt.row_splits.cpu().numpy().copy()
    splits[5] = splits[4] - 7  # query 4's range is inverted: empty; query 5's begins seven entries early
    flt.row_splits.copy_(torch.as_tensor(splits))
    rows = flt.rows.cpu().numpy()
    masked = full.copy()
    masked[:, deny] = -np.inf
    for i in range(b):
        lo = min(max(splits[i], 0), len(rows))
        hi = max(lo, min(max(splits[i + 1], 0), len(rows)))
        li = rows[lo:hi].astype(np.int64)
        masked[i, li[(li >= 0) & (li < n)]] = -np.inf
    thr = np.array([[np.sort(full[i])[::-1][300], -np.inf][i % 2] for i in range(b)], np.float32)
    room = b * n
    exp = RM.reference(masked, thr, oix.ids, room)
    allowed = (masked != -np.inf).sum(axis=1)
    assert (np.diff(exp[0])[1::2] == allowed[1::2]).all() and (allowed < 0.75 * n).all()  # at -inf: every allowed row, no denied one
    plain = RM.reference(full, thr, oix.ids, room)
    assert (np.diff(exp[0])[0::2] < np.diff(plain[0])[0::2]).all()  # and at a finite cut the filter bites too
    sc = ops.Scorer("l2", 64)
    _assert_same(_range(dix, sc, cuda(q), thr, room, flt=flt), exp, "bitmap + lists")
    # no filter: a NULL pointer and a struct of three NULLs
    _assert_same(_range(dix, sc, cuda(q), thr, room), plain, "NULL")
    _assert_same(_range(dix, sc, cuda(q), thr, room, flt=retrieval.make_filter(dix)), plain, "three NULLs")


# ---- 6. MLP -----------------------------------------------------------------------------------------------------------
def _mlp_case(oracle):
    if "mlp" not in _CACHE:
        from nann_amd import synth
        n, d = 5000, 64
        embs, assign = synth.make_corpus(n, d, seed=61)
        oix, dix = _indices(embs)
        w = synth.make_mlp_weights(d)
        q = np.stack([oracle.user_seq_mean(s) for s in synth.make_queries(embs, assign, 9, seed=62)])
        full = _all_scores(oracle, oix, oracle.Scorer("mlp", d, oracle.EMB_F16, w), q)
        _CACHE["mlp"] = (oix, dix, w, q, full)
    return _CACHE["mlp"]


def test_mlp_exact_bitwise(oracle):
    from nann_amd import ops
    oix, dix, w, q, full = _mlp_case(oracle)
    thr = _five_thresholds(full)
    thr[2], thr[7] = np.sort(full[2])[::-1][200], np.sort(full[7])[::-1][17]
    room = 9 * 5000
    _assert_same(_range(dix, ops.Scorer("mlp", 64, torch.float16, w, precision="exact"), cuda(q), thr, room),
                 RM.reference(full, thr, oix.ids, room))


def test_mlp_split_returns_the_oracles_set(oracle):
    """thr at the midpoint of the widest gap between adjacent sorted oracle scores near rank 200, wider than twice the tolerance
    1e-5 max(1, |s|): a device score within the tolerance falls on the oracle's side of it."""
    from nann_amd import ops
    oix, dix, w, q, full = _mlp_case(oracle)
    thr = np.zeros(9, np.float32)
    for i in range(9):
        s = np.sort(full[i].astype(np.float64))[::-1]
        j = 100 + int(np.argmax(s[100:300] - s[101:301]))
        tol = 1e-5 * max(1.0, abs(s[j]), abs(s[j + 1]))
        assert s[j] - s[j + 1] > 2 * tol, (i, s[j] - s[j + 1], tol)  # such a gap was found
        thr[i] = np.float32((s[j] + s[j + 1]) / 2)
        assert s[j + 1] + tol < thr[i] < s[j] - tol
    room = 9 * 400
    exp = RM.reference(full, thr, oix.ids, room)
    assert (np.diff(exp[0]) >= 101).all() and exp[0][-1] <= room
    got = _range(dix, ops.Scorer("mlp", 64, torch.float16, w, precision="split"), cuda(q), thr, room)
    assert (got[0] == exp[0]).all() and (got[1] == exp[1]).all() and (got[3] == exp[3]).all()
    m = exp[0][-1]
    print("largest |device - oracle| / max(1, |s|):", float(np.max(np.abs(got[2][:m] - exp[2][:m]) / np.maximum(1, np.abs(exp[2][:m])))))
    assert (np.abs(got[2][:m].astype(np.float64) - exp[2][:m]) <= 1e-5 * np.maximum(1, np.abs(exp[2][:m]))).all()
    assert (got[2][m:] == S).all()


# ---- 7. the bits of search_all, under every scorer ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["l2", "ip", "mlp_exact", "mlp_split", "attn_exact", "attn_split"])
def test_same_rows_and_bits_as_search_all(tmp_path, kind):
    """search_all*(k = 1000) gives every row's device score; with thr = its 50th score per query the range call returns exactly
    the rows whose device score is >= thr, with those bits"""
    from nann_amd import ops, retrieval, synth
    from test_search_all_model_gpu import _corpus, _model
    n, b = 1000, 9
    host, oix, dix, code, tdt, seqs = _corpus(n, 64)
    model = kind.startswith("attn")
    if model:
        by = _model(tmp_path, 64, kind[5:])
        x = cuda(seqs[:b], torch.float16)
        r = retrieval.search_all_model(dix, by, x, n)
    else:
        by = ops.Scorer(kind, 64) if kind in ("l2", "ip") else ops.Scorer("mlp", 64, torch.float16, synth.make_mlp_weights(64), precision=kind[4:])
        x = cuda(np.random.default_rng(71).standard_normal((b, 64)).astype(np.float32))
        r = retrieval.search_all(dix, by, x, n)
    torch.cuda.synchronize()
    device = _matrix(r.index.cpu().numpy(), r.scores.cpu().numpy())
    thr = r.scores.cpu().numpy()[:, 49].copy()
    exp = RM.reference(device, thr, oix.ids, b * 60)
    assert (np.diff(exp[0]) >= 50).all() and exp[0][-1] <= b * 60
    _assert_same(_range(dix, by, x, thr, b * 60, model=model), exp, kind)


# ---- 8. contract --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["l2", "mlp", "attn"])
def test_status_codes(tmp_path, kind):
    from nann_amd import _lib, ops, retrieval, synth
    from test_search_all_model_gpu import _corpus, _model
    L = _lib.lib()
    n, b = 300, 3
    dix, dix128 = _corpus(n, 64)[2], _corpus(n, 128)[2]
    model = kind == "attn"
    if model:
        by, x = _model(tmp_path, 64, "split"), cuda(_corpus(n, 64)[5][:b], torch.float16)
    else:
        by = ops.Scorer("l2", 64) if kind == "l2" else ops.Scorer("mlp", 64, torch.float16, synth.make_mlp_weights(64), precision="split")
        x = cuda(np.random.default_rng(81).standard_normal((b, 64)).astype(np.float32))
    from nann_amd.ops import _ptr, _stream
    fn = L.nann_search_all_range_model if model else L.nann_search_all_range
    fn_bytes = L.nann_search_all_range_model_workspace_bytes if model else L.nann_search_all_range_workspace_bytes
    ws, nbytes = _ws(dix, by, b, model)
    ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device="cuda")
    assert nbytes > 0 and ws.data_ptr() % 256 == 0
    thr = cuda(np.full(b, -np.inf, np.float32))
    room = b * n
    out = _Out(b, room)
    flt = retrieval.make_filter(dix, deny_rows=[1, 2, 3])
    bad_filter = retrieval.make_filter(dix, deny_rows=[1, 2, 3])
    bad_filter.struct.struct_bytes = 3
    bad_options = retrieval.search_options()
    bad_options.struct_bytes = 4
    off = retrieval.search_options(preprojection=False)

    def call(**kw):
        entries = [_ptr(out.ids), _ptr(out.scores), _ptr(out.index)]
        if "ids" in kw:
            entries[0] = kw["ids"]
        o, f = kw.get("options"), kw.get("filter")
        st = fn(kw.get("ix", dix.handle), kw.get("by", by.handle), kw.get("x", _ptr(x)), kw.get("n", b), kw.get("thr", _ptr(thr)),
                kw.get("capacity", room), kw.get("splits", _ptr(out.splits)), *entries, kw.get("ws", _ptr(ws)),
                kw.get("ws_bytes", nbytes), C.byref(o) if o is not None else None, C.byref(f.struct) if f is not None else None,
                _stream())
        torch.cuda.synchronize()
        return st

    table_off = OK if kind == "l2" else UNSUPPORTED
    cases = [("null index", dict(ix=None), BAD, b"null argument"), ("null scorer", dict(by=None), BAD, b"null argument"),
             ("n = -1", dict(n=-1), BAD, b"< 0"), ("capacity = -1", dict(capacity=-1), BAD, b"capacity < 0"),
             ("null q", dict(x=None), BAD, b"null argument"), ("null thresholds", dict(thr=None), BAD, b"null argument"),
             ("null row_splits", dict(splits=None), BAD, b"null argument"),
             ("null item ids, capacity > 0", dict(ids=None), BAD, b"out_item_ids"),
             ("index of d = 128", dict(ix=dix128.handle), BAD, b"disagree"),
             ("options.struct_bytes = 4", dict(options=bad_options), BAD, b"nann_search_options: struct_bytes"),
             ("filter.struct_bytes = 3", dict(filter=bad_filter), BAD, b"nann_filter: struct_bytes"),
             ("workspace offset by 8 bytes", dict(ws=_ptr(ws[8:])), BAD, b"aligned"),
             ("workspace one byte short", dict(ws_bytes=nbytes - 1), CAPACITY, b"workspace smaller than"),
             ("null workspace", dict(ws=None), CAPACITY, b"workspace smaller than"),
             ("n = 2^31", dict(n=2 ** 31), UNSUPPORTED, b"too many"),
             ("preprojection off", dict(options=off), table_off, b"preprojection" if table_off else None)]
    for what, kw, status, text in cases:
        got = call(**kw)
        error = L.nann_last_error()
        print(kind, what, "->", got, error)
        assert got == status, (kind, what, got, error)
        if text is not None:
            assert text in error, (kind, what, error)
        if got != OK:
            assert out.untouched(), (kind, what)
        else:
            out = _Out(b, room)
    # n == 0: OK, nothing written, whatever else is missing
    assert call(n=0) == OK and call(n=0, ws=None, ws_bytes=0, x=None, thr=None, splits=None, ids=None, capacity=0) == OK
    assert out.untouched()
    # the size call: the same codes for the arguments it has; n == 0 -> 0 bytes
    nb = C.c_int64(-1)
    assert fn_bytes(dix.handle, by.handle, 0, C.byref(nb)) == OK and nb.value == 0
    assert fn_bytes(dix.handle, by.handle, -1, C.byref(nb)) == BAD
    assert fn_bytes(dix128.handle, by.handle, b, C.byref(nb)) == BAD and b"disagree" in L.nann_last_error()
    assert fn_bytes(dix.handle, by.handle, 2 ** 31, C.byref(nb)) == UNSUPPORTED
    assert fn_bytes(dix.handle, by.handle, b, None) == BAD
    # and the call as it should be made answers, through the filter too
    assert call(filter=flt) == OK
    got = out.numpy()
    assert got[0].tolist() == [0, n - 3, 2 * (n - 3), 3 * (n - 3)]
    assert got[1][:n - 3].tolist() == [0] + list(range(4, n))


# ---- 9. Python ----------------------------------------------------------------------------------------------------------
def test_python_counts_then_fills_sorts_and_broadcasts(oracle):
    from nann_amd import ops, retrieval
    oix, dix, q, full, thr = _chunk_case(oracle)
    b = 21
    q, full, thr = q[:b], full[:b], thr[:b]
    sc = ops.Scorer("l2", 64)
    # capacity=None: the two-call C sequence -- count only, then a fill at exactly the total
    counted = _Out(b, 1)
    assert _call(dix, sc, cuda(q), cuda(thr), 0, counted, null_entries=True) == OK
    total = int(counted.numpy()[0][-1])
    two_calls = _range(dix, sc, cuda(q), thr, total)
    r = retrieval.search_all_range(dix, sc, cuda(q), cuda(thr))
    torch.cuda.synchronize()
    assert r.total == total and not r.truncated and r.item_ids.numel() == total
    _assert_same((r.row_splits.cpu().numpy(), r.index.cpu().numpy(), r.scores.cpu().numpy(), r.item_ids.cpu().numpy()), two_calls)
    _assert_same(two_calls, RM.reference(full, thr, oix.ids, total))
    # a capacity too small: truncated, the true counts, the head of the result
    cut = retrieval.search_all_range(dix, sc, cuda(q), thr, capacity=100)
    assert cut.truncated and cut.total == total and (cut.index.cpu().numpy() == two_calls[1][:100]).all()
    assert (cut.row_splits.cpu().numpy() == two_calls[0]).all()
    # sort=True: every segment by (score descending, row ascending)
    s = retrieval.search_all_range(dix, sc, cuda(q), cuda(thr), sort=True)
    rows, scores, ids, splits = s.index.cpu().numpy(), s.scores.cpu().numpy(), s.item_ids.cpu().numpy(), s.row_splits.cpu().numpy()
    assert (splits == two_calls[0]).all()
    for i in range(b):
        lo, hi = splits[i], splits[i + 1]
        seg_rows, seg_scores = two_calls[1][lo:hi], two_calls[2][lo:hi]
        order = np.lexsort((seg_rows, -seg_scores.astype(np.float64)))
        assert (rows[lo:hi] == seg_rows[order]).all() and (bits(scores[lo:hi]) == bits(seg_scores[order])).all(), i
        assert (ids[lo:hi] == oix.ids[rows[lo:hi]]).all()
    # a float threshold broadcasts
    t = float(np.sort(full.reshape(-1))[::-1][500])
    f = retrieval.search_all_range(dix, sc, cuda(q), t)
    exp = RM.reference(full, np.full(b, t, np.float32), oix.ids, 0)
    exp = RM.reference(full, np.full(b, t, np.float32), oix.ids, int(exp[0][-1]))
    assert f.total == int(exp[0][-1]) >= 501
    _assert_same((f.row_splits.cpu().numpy(), f.index.cpu().numpy(), f.scores.cpu().numpy(), f.item_ids.cpu().numpy()), exp)
