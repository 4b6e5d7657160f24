"""-m gpu: the group cap on the device (nann_group_cap_topk / retrieval.cap_groups) against the numpy model of its contract
(groupcap_model.model), bit for bit on rows, scores, item ids, groups, positions and n_out.  The calls go through the C ABI with
outputs pre-filled with a canary and guard bands around them.  The shapes are the smallest at which the kernel can go wrong:
list lengths around the wavefront (64), the pass (256) and the limit (1024), a table half full, every group probing from one
slot, groups that straddle a chunk's edge with the cap reached exactly there."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import groupcap_model as GM
from gpu_util import bits, cuda, require_gpu

pytestmark = pytest.mark.gpu
GUARD = 64
CANARY = 0x5A
ALL = ("scores", "item_ids", "group", "pos", "n_out")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


class _Out:
    """an output [n_queries, k] inside a canary-filled buffer with GUARD elements in front and behind"""

    def __init__(self, n_queries, k, dtype):
        self.n = n_queries * k
        self.shape = (n_queries, k)
        host = torch.empty(self.n + 2 * GUARD, dtype=dtype)
        host.view(torch.uint8).fill_(CANARY)
        self.canary = host[0].clone()
        self.buf = host.cuda()

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

    def get(self):
        h = self.buf.cpu()
        assert (h[:GUARD] == self.canary).all() and (h[GUARD + self.n:] == self.canary).all(), "guard band written"
        return h[GUARD:GUARD + self.n].reshape(self.shape).numpy()


def _filter(n_items, deny, exclude):
    from nann_amd import retrieval
    if deny is None and exclude is None:
        return None
    ix = types.SimpleNamespace(n_items=n_items, item_ids=None, device=torch.device("cuda"))
    return retrieval.make_filter(ix, deny_rows=None if deny is None else np.nonzero(deny)[0], exclude_rows=exclude)


def _call(scores, rows, n_valid, n_items, gor, cap, k, caps=None, item_ids=None, deny=None, exclude=None, want=ALL, stream=None):
    """nann_group_cap_topk -> dict like groupcap_model.model's; outputs not in `want` are passed as NULL"""
    from nann_amd import _lib
    from nann_amd.ops import _ptr, _stream
    L = _lib.lib()
    n_q, k_in = rows.shape
    d_scores = cuda(scores, torch.float32) if scores is not None else None
    d_rows = cuda(rows, torch.int32)
    d_nv = cuda(n_valid, torch.int32) if n_valid is not None else None
    d_ids = cuda(item_ids, torch.int64) if item_ids is not None else None
    d_gor = cuda(np.asarray(gor), torch.int32)
    d_caps = cuda(np.asarray(caps), torch.int32) if caps is not None else None
    g = _lib.Groups()
    g.struct_bytes, g.group_of_row, g.cap, g.caps = C.sizeof(_lib.Groups), d_gor.data_ptr(), int(cap), _ptr(d_caps)
    flt = _filter(n_items, deny, exclude)
    outs = {"index": _Out(n_q, k, torch.int32)}
    for name, dt in (("scores", torch.float32), ("item_ids", torch.int64), ("group", torch.int32), ("pos", torch.int32)):
        if name in want and (name != "item_ids" or item_ids is not None):
            outs[name] = _Out(n_q, k, dt)
    if "n_out" in want:
        outs["n_out"] = _Out(n_q, 1, torch.int32)
    p = lambda name: outs[name].ptr() if name in outs else None
    st = L.nann_group_cap_topk(_ptr(d_scores), _ptr(d_rows), _ptr(d_nv), n_q, k_in, n_items, _ptr(d_ids), C.byref(g),
                               C.byref(flt.struct) if flt is not None else None, k, p("index"), p("scores"), p("item_ids"),
                               p("group"), p("pos"), p("n_out"), C.c_void_p(stream.cuda_stream) if stream is not None else _stream())
    assert st == 0, _lib.last_error()
    torch.cuda.synchronize()
    got = {name: o.get() for name, o in outs.items()}
    if "n_out" in got:
        got["n_out"] = got["n_out"].reshape(-1)
    return got


def _same(got, exp, what=""):
    for name, g in got.items():
        e = exp[name]
        if name == "scores":
            g, e = bits(g), bits(e)
        assert g.shape == e.shape and (g == e).all(), (what, name)


def _check(scores, rows, n_valid, n_items, gor, cap, k, what="", caps=None, deny=None, exclude=None, **kw):
    item_ids = np.arange(n_items, dtype=np.int64) * 7 + 3
    got = _call(scores, rows, n_valid, n_items, gor, cap, k, caps=caps, item_ids=item_ids, deny=deny, exclude=exclude, **kw)
    _same(got, GM.model(scores, rows, n_valid, n_items, gor, cap, k, caps=caps, item_ids=item_ids, deny=deny, exclude=exclude), what)
    return got


def _scores(rng, shape):
    """descending like a ranked list's, with a NaN and a -inf among them: scores are carried, never compared"""
    s = -np.sort(-rng.standard_normal(shape).astype(np.float32), axis=-1)
    if s.size > 2:
        s.reshape(-1)[1], s.reshape(-1)[-1] = np.nan, -np.inf
    return s


LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024]


@pytest.mark.parametrize("k_in", LENGTHS)
def test_every_length_bitwise(k_in):
    rng = np.random.default_rng(100 + k_in)
    n_items = 3000
    if k_in == 0:  # k = 0 with it: NANN_OK and nothing written, n_out included (an empty list of a wider call: n_valid = 0 below)
        got = _call(None, np.zeros((3, 0), np.int32), None, n_items, np.zeros(n_items, np.int32), 1, 0, want=("n_out",))
        assert (got["n_out"].view(np.uint8) == CANARY).all()
        got = _check(_scores(rng, (3, 5)), rng.integers(0, n_items, (3, 5)).astype(np.int32), np.zeros(3, np.int32), n_items,
                     np.zeros(n_items, np.int32), 1, 5)
        assert not got["n_out"].any()
        return
    for n_groups, cap in ((7, 2), (40, 1), (3, 5)):
        gor = rng.integers(0, n_groups, n_items).astype(np.int32)
        gor[rng.random(n_items) < 0.1] = -1
        rows = np.stack([rng.permutation(n_items)[:k_in] for _ in range(3)]).astype(np.int32).reshape(3, k_in)
        got = _check(_scores(rng, (3, k_in)), rows, None, n_items, gor, cap, k_in, (k_in, n_groups, cap))
        if k_in >= 255:
            assert (got["n_out"] < k_in).all() and (got["n_out"] > 0).all()   # the cap bites
        if k_in and cap * n_groups < k_in // 2:
            for i in range(3):
                g = got["group"][i, :got["n_out"][i]]
                assert np.unique(g[g >= 0], return_counts=True)[1].max() == cap


@pytest.mark.parametrize("cap", [1, 3])
def test_one_group_throughout(cap):
    rng = np.random.default_rng(cap)
    n_items, k_in = 1500, 1024
    rows = np.stack([rng.permutation(n_items)[:k_in] for _ in range(2)]).astype(np.int32)
    got = _check(_scores(rng, (2, k_in)), rows, None, n_items, np.full(n_items, 12345, np.int32), cap, k_in)
    assert (got["n_out"] == cap).all() and (got["index"][:, :cap] == rows[:, :cap]).all()


def test_1024_distinct_groups_the_table_half_full():
    rng = np.random.default_rng(2)
    n_items, k_in = 1024, 1024
    gor = (rng.permutation(n_items).astype(np.int64) * 2097151 % (2 ** 31 - 1)).astype(np.int32)
    assert len(set(gor.tolist())) == 1024
    rows = np.stack([rng.permutation(n_items) for _ in range(2)]).astype(np.int32)
    got = _check(_scores(rng, (2, k_in)), rows, None, n_items, gor, 1, k_in)
    assert (got["n_out"] == 1024).all() and (got["index"] == rows).all()
    # every row twice, 512 groups: the second copy of each is over the cap
    twice = np.concatenate([rows[:, :512], rows[:, :512][:, ::-1]], axis=1)
    got = _check(_scores(rng, (2, k_in)), twice, None, n_items, gor, 1, k_in)
    assert (got["n_out"] == 512).all() and (got["index"][:, :512] == rows[:, :512]).all()


def test_1024_groups_that_start_probing_at_one_slot():
    cand = np.arange(1, 4_000_000, dtype=np.int64)
    ids = cand[(((cand * 2654435761) & 0xFFFFFFFF) >> 21) == 5][:1024]   # the kernel's hash, restated
    assert len(ids) == 1024 and all(GM.group_hash(g) == 5 for g in ids[:20])
    rng = np.random.default_rng(3)
    n_items, k_in = 1024, 1024
    gor = ids[rng.permutation(1024)].astype(np.int32)
    rows = rng.permutation(n_items).astype(np.int32)[None]
    got = _check(_scores(rng, (1, k_in)), rows, None, n_items, gor, 1, k_in)
    assert got["n_out"][0] == 1024
    # 256 of them, four entries each, cap 2
    gor4 = ids[np.arange(1024) % 256].astype(np.int32)
    got = _check(_scores(rng, (1, k_in)), rows, None, n_items, gor4, 2, k_in)
    assert got["n_out"][0] == 512


def test_ids_0_and_int_max_and_negative_ids_between():
    rng = np.random.default_rng(4)
    n_items, k_in = 600, 300
    gor = np.array([0, 2 ** 31 - 1, -1, -2 ** 31, 1, -5] * 100, np.int32)
    rows = np.stack([rng.permutation(n_items)[:k_in] for _ in range(2)]).astype(np.int32)
    got = _check(_scores(rng, (2, k_in)), rows, None, n_items, gor, 2, k_in)
    for i in range(2):
        g = got["group"][i, :got["n_out"][i]]
        assert (g == 0).sum() == 2 and (g == 2 ** 31 - 1).sum() == 2 and (g == 1).sum() == 2
        assert (g < 0).sum() == (gor[rows[i]] < 0).sum()      # every ungrouped row is kept


@pytest.mark.parametrize("edge", [64, 256, 512])
def test_a_group_that_straddles_a_chunk_edge(edge):
    """group 7 stands at positions edge - 2 .. edge + 1 alone; at cap 2 the cap is reached exactly at the edge, at cap 3 one
    entry behind it, at cap 1 one in front"""
    n_items, k_in = 2000, 1024
    gor = np.arange(n_items, dtype=np.int32) + 100            # every other row a group of its own
    rows = np.arange(k_in, dtype=np.int32)[None].copy()
    gor[edge - 2:edge + 2] = 7
    rng = np.random.default_rng(edge)
    for cap in (1, 2, 3, 4):
        got = _check(_scores(rng, (1, k_in)), rows, None, n_items, gor, cap, k_in, (edge, cap))
        kept = got["pos"][0, :got["n_out"][0]].tolist()
        assert got["n_out"][0] == k_in - (4 - cap)
        assert [p for p in range(edge - 2, edge + 2) if p in kept] == list(range(edge - 2, edge - 2 + cap))


def test_cap_at_least_k_in_returns_the_head():
    rng = np.random.default_rng(6)
    n_items, k_in = 500, 257
    gor = rng.integers(0, 3, n_items).astype(np.int32)
    rows = np.stack([rng.permutation(n_items)[:k_in] for _ in range(2)]).astype(np.int32)
    scores = _scores(rng, (2, k_in))
    for cap in (k_in, k_in + 1, 2 ** 31 - 1):
        got = _check(scores, rows, None, n_items, gor, cap, 200)
        assert (got["n_out"] == 200).all() and (got["index"] == rows[:, :200]).all() and (got["pos"] == np.arange(200)).all()


def test_k_below_and_above_the_number_kept():
    rng = np.random.default_rng(7)
    n_items, k_in = 900, 700
    gor = rng.integers(0, 50, n_items).astype(np.int32)
    rows = np.stack([rng.permutation(n_items)[:k_in] for _ in range(3)]).astype(np.int32)
    scores = _scores(rng, (3, k_in))
    kept = _check(scores, rows, None, n_items, gor, 3, k_in)["n_out"]
    assert (kept == 150).all()
    for k in (1, 149, 150, 151, 700):
        got = _check(scores, rows, None, n_items, gor, 3, k, k)
        assert (got["n_out"] == min(k, 150)).all()


def test_caps_per_query_n_valid_and_rows_out_of_range():
    rng = np.random.default_rng(8)
    n_q, n_items, k_in = 9, 400, 513
    gor = rng.integers(-1, 20, n_items).astype(np.int32)
    rows = rng.integers(0, n_items, (n_q, k_in)).astype(np.int32)      # rows repeat: a row that stands twice counts twice
    bad = rng.random(rows.shape) < 0.1
    rows[bad] = rng.choice(np.array([-1, n_items, n_items + 5, -2 ** 31, 2 ** 31 - 1], np.int64), int(bad.sum())).astype(np.int32)
    rows[0, 0], rows[-1, -1] = -1, n_items
    caps = np.array([1, 0, 3, -4, 2 ** 31 - 1, 2, -2 ** 31, 8, 1], np.int32)
    n_valid = np.array([-3, 0, 1, 64, 65, 512, 513, 514, 2 ** 31 - 1], np.int32)
    scores = _scores(rng, (n_q, k_in))
    got = _check(scores, rows, n_valid, n_items, gor, 1, 400, caps=caps)
    assert got["n_out"][0] == 0 and got["n_out"][1] == 0 and not got["index"][:2].any() and not bits(got["scores"][:2]).any()
    _check(scores, rows, None, n_items, gor, 1, 400, caps=caps)
    _check(scores, rows, n_valid, n_items, gor, 2, 400)
    _check(None, rows, n_valid, n_items, gor, 2, 400)                   # no scores: zeros are carried


def test_denied_rows_use_no_quota():
    rng = np.random.default_rng(9)
    n_q, n_items, k_in = 5, 1200, 1024
    gor = rng.integers(-1, 30, n_items).astype(np.int32)
    rows = np.stack([rng.permutation(n_items)[:k_in] for _ in range(n_q)]).astype(np.int32)
    scores = _scores(rng, (n_q, k_in))
    deny = rng.random(n_items) < 0.3
    exclude = [np.concatenate([rows[i, :40:2], rng.integers(-3, n_items + 3, 70)]).astype(np.int64) for i in range(n_q)]
    exclude[3] = np.zeros(0, np.int64)                                  # one query without a list
    plain = _check(scores, rows, None, n_items, gor, 2, k_in)
    for d, e in ((deny, None), (None, exclude), (deny, exclude)):
        got = _check(scores, rows, None, n_items, gor, 2, k_in, deny=d, exclude=e)
        for i in range(n_q):
            r = got["index"][i, :got["n_out"][i]]
            assert d is None or not d[r].any()
            assert e is None or not np.isin(r, e[i]).any()
        # the denied rows' quota went to later rows of their groups: the answers differ and are no subsets of the plain one
        assert any(not np.isin(got["index"][i, :got["n_out"][i]], plain["index"][i, :plain["n_out"][i]]).all() for i in range(n_q))


def test_each_optional_output_null_in_turn():
    rng = np.random.default_rng(10)
    n_items, k_in = 300, 130
    gor = rng.integers(-1, 9, n_items).astype(np.int32)
    rows = np.stack([rng.permutation(n_items)[:k_in] for _ in range(3)]).astype(np.int32)
    scores = _scores(rng, (3, k_in))
    item_ids = np.arange(n_items, dtype=np.int64) + 100
    exp = GM.model(scores, rows, None, n_items, gor, 2, 100, item_ids=item_ids)
    got = _call(scores, rows, None, n_items, gor, 2, 100, item_ids=None, want=())
    assert set(got) == {"index"}
    _same(got, exp)
    for leave_out in ALL:
        want = tuple(n for n in ALL if n != leave_out)
        got = _call(scores, rows, None, n_items, gor, 2, 100, item_ids=item_ids, want=want)
        assert set(got) == {"index"} | set(want)
        _same(got, exp, leave_out)


def test_a_query_does_not_depend_on_its_batch():
    rng = np.random.default_rng(11)
    n_q, n_items, k_in = 37, 800, 600
    gor = rng.integers(-1, 25, n_items).astype(np.int32)
    rows = np.stack([rng.permutation(n_items)[:k_in] for _ in range(n_q)]).astype(np.int32)
    rows[1:] = rows[0]                                                   # the same query 37 times
    scores = np.repeat(_scores(rng, (1, k_in)), n_q, axis=0)
    batch = _check(scores, rows, None, n_items, gor, 2, 300)
    alone = _check(scores[:1], rows[:1], None, n_items, gor, 2, 300)
    for name in batch:
        g, e = (bits(alone[name]), bits(batch[name])) if name == "scores" else (alone[name], batch[name])
        assert (g == e).all(), name


def test_a_non_default_stream():
    rng = np.random.default_rng(12)
    n_items, k_in = 500, 300
    gor = rng.integers(0, 10, n_items).astype(np.int32)
    rows = np.stack([rng.permutation(n_items)[:k_in] for _ in range(4)]).astype(np.int32)
    scores = _scores(rng, (4, k_in))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = _call(scores, rows, None, n_items, gor, 3, 100, stream=s)
    _same(got, GM.model(scores, rows, None, n_items, gor, 3, 100))


def test_the_python_call():
    from nann_amd import retrieval
    rng = np.random.default_rng(13)
    n_items, k_in = 200, 90
    gor = rng.integers(-1, 6, n_items).astype(np.int32)
    rows = rng.integers(-1, n_items + 1, (3, k_in)).astype(np.int32)
    scores = _scores(rng, (3, k_in))
    n_valid = np.array([90, 45, 0], np.int32)
    ix = types.SimpleNamespace(n_items=n_items, item_ids=None, device=torch.device("cuda"))
    groups = retrieval.make_groups(ix, group_of_row=gor, caps=[1, 2, 3])
    r = retrieval.cap_groups(cuda(scores), cuda(rows), groups, 60, n_valid=cuda(n_valid))
    torch.cuda.synchronize()
    exp = GM.model(scores, rows, n_valid, n_items, gor, 1, 60, caps=[1, 2, 3])
    assert r.item_ids is None and r.status is None and r.plan is None
    assert (r.index.cpu().numpy() == exp["index"]).all() and (bits(r.scores.cpu().numpy()) == bits(exp["scores"])).all()
    assert (r.group.cpu().numpy() == exp["group"]).all() and (r.pos.cpu().numpy() == exp["pos"]).all()
    assert (r.n_out.cpu().numpy() == exp["n_out"]).all()
