"""-m gpu: the fused top-k on the device (nann_fuse_topk / retrieval.fuse_topk) against the numpy model of its contract
(fuse_model.model), bit for bit on rows, fused scores, item ids, list masks and n_out.  The calls go through the C ABI with
outputs pre-filled with a canary and guard bands around them, and a workspace pre-filled with 0xA5."""
import ctypes as C

import numpy as np
import pytest
import torch

import fuse_model as FM
from gpu_util import bits, cuda, require_gpu

pytestmark = pytest.mark.gpu
GUARD = 64
CANARY = 0x5A
MODES = (FM.SUM, FM.SUM_FLOOR, FM.MINMAX, FM.RRF)
F = np.float32


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


class _Out:
    """an output [n_users, k] inside a canary-filled buffer with GUARD elements in front and behind"""

    def __init__(self, n_users, k, dtype):
        self.n = n_users * k
        self.shape = (n_users, k)
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


def _call(scores, rows, n_valid, n_items, k, mode, weights=None, rrf_c=60.0, item_ids=None,
          want=("scores", "item_ids", "lists", "n_out"), stream=None):
    """nann_fuse_topk -> dict like fuse_model.model's; outputs not in `want` are passed as NULL"""
    from nann_amd import _lib
    from nann_amd.ops import _ptr, _stream
    L = _lib.lib()
    n_users, n_lists, k_in = scores.shape
    d_scores, d_rows = cuda(scores, torch.float32), cuda(rows, torch.int32)
    d_nv = cuda(n_valid, torch.int32) if n_valid is not None else None
    d_ids = cuda(item_ids, torch.int64) if item_ids is not None else None
    d_w = cuda(weights, torch.float32) if weights is not None else None
    f = _lib.Fusion(C.sizeof(_lib.Fusion), mode, rrf_c, int(weights is not None and np.ndim(weights) == 2),
                    d_w.data_ptr() if d_w is not None else None)
    outs = {"index": _Out(n_users, k, torch.int32)}
    if "scores" in want:
        outs["scores"] = _Out(n_users, k, torch.float32)
    if "item_ids" in want and item_ids is not None:
        outs["item_ids"] = _Out(n_users, k, torch.int64)
    if "lists" in want:
        outs["lists"] = _Out(n_users, k, torch.int64)
    if "n_out" in want:
        outs["n_out"] = _Out(n_users, 1, torch.int32)
    nb = C.c_int64(-1)
    assert L.nann_fuse_topk_workspace_bytes(n_users, n_lists, k_in, C.byref(nb)) == 0
    ws = torch.full((max(nb.value, 1),), 0xA5, dtype=torch.uint8, device="cuda")  # (the kernel initialises what it uses itself)
    p = lambda name: outs[name].ptr() if name in outs else None
    st = L.nann_fuse_topk(_ptr(d_scores), _ptr(d_rows), _ptr(d_nv), n_users, n_lists, k_in, n_items, _ptr(d_ids), k, C.byref(f),
                          p("index"), p("scores"), p("item_ids"), p("lists"), p("n_out"), _ptr(ws), nb.value,
                          C.c_void_p(stream.cuda_stream) if stream is not None else _stream())
    assert st == 0, _lib.last_error()
    torch.cuda.synchronize()
    got = {name: o.get() for name, o in outs.items()}
    if "n_out" in got:
        got["n_out"] = got["n_out"].reshape(-1)
    if "lists" in got:
        got["lists"] = got["lists"].view(np.uint64)
    return got


def _same(got, exp, what=""):
    for name, g in got.items():
        e = exp[name]
        if name == "scores":
            g, e = bits(g), bits(e)
        assert g.shape == e.shape and (g == e).all(), (what, name)


def _check(scores, rows, n_valid, n_items, k, mode, what="", weights=None, rrf_c=60.0, **kw):
    item_ids = np.arange(n_items, dtype=np.int64) * 7 + 3
    got = _call(scores, rows, n_valid, n_items, k, mode, weights=weights, rrf_c=rrf_c, item_ids=item_ids, **kw)
    _same(got, FM.model(scores, rows, n_valid, n_items, k, mode, weights=weights, rrf_c=rrf_c, item_ids=item_ids), (what, mode))
    return got


# (n_users, n_lists, k_in, k): one entry; small odd sizes; n_in at the limit with long lists; n_lists at the limit with n_in =
# 8192 (mask bit 63); n_lists at the limit with one entry each
SHAPES = [(1, 1, 1, 1), (3, 2, 5, 7), (3, 3, 7, 21), (4, 4, 64, 100), (2, 8, 1024, 1024), (2, 64, 128, 1024), (2, 64, 1, 64)]
VALUES = np.array([-np.inf, -2.5, -0.0, 0.0, 0.5, 3.0], F)
KINDS = ("identical", "disjoint", "pool7", "equal", "zeros", "neg_inf", "empty_list", "dups")


def _contents(kind, shape, rng):
    """(scores, rows, n_valid, n_items) of one kind of content for a shape"""
    n_users, n_lists, k_in, _ = shape
    n_in = n_lists * k_in
    n_items = 3 * n_in + 11
    n_valid = None
    scores = rng.standard_normal((n_users, n_lists, k_in)).astype(F)
    if kind == "identical":      # every list of a user holds the same rows with the same scores
        rows = np.stack([rng.permutation(n_items)[:k_in] for _ in range(n_users)])[:, None, :].repeat(n_lists, 1)
        scores = scores[:, :1, :].repeat(n_lists, 1)
    elif kind == "disjoint":
        rows = np.stack([rng.permutation(n_items)[:n_in] for _ in range(n_users)]).reshape(n_users, n_lists, k_in)
    elif kind == "pool7":        # nearly every entry collides
        n_items = 7
        rows = rng.integers(0, 7, (n_users, n_lists, k_in))
    elif kind == "equal":        # one score everywhere: the lists a row stands in and the position order decide
        rows = rng.integers(0, n_items, (n_users, n_lists, k_in))
        scores[:] = F(1.25)
    elif kind == "zeros":        # -0 and +0 tie
        rows = rng.integers(0, max(n_in // 2, 1), (n_users, n_lists, k_in))
        scores = np.where(rng.random(scores.shape) < 0.5, F(-0.0), F(0.0)).astype(F)
    elif kind == "neg_inf":      # -inf is a score like any other (SUM and RRF)
        rows = rng.integers(0, max(n_in // 2, 1), (n_users, n_lists, k_in))
        scores = VALUES[rng.integers(0, len(VALUES), scores.shape)]
        scores[0] = -np.inf
    elif kind == "empty_list":   # a list with no valid entry: cut to nothing, or every row out of range
        rows = rng.integers(0, max(n_in // 2, 1), (n_users, n_lists, k_in))
        n_valid = np.full((n_users, n_lists), k_in, np.int32)
        n_valid[:, rng.integers(0, n_lists)] = 0
        rows[0, rng.integers(0, n_lists)] = -1
    elif kind == "dups":         # rows repeat WITHIN a list: only the first entry of a row counts, at its own rank
        rows = rng.integers(0, max(k_in // 3, 1), (n_users, n_lists, k_in)) + rng.integers(0, 3, (n_users, n_lists, 1))
    else:
        raise AssertionError(kind)
    return np.ascontiguousarray(scores, F), np.ascontiguousarray(rows, np.int32), n_valid, n_items


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_content_and_mode_bitwise(shape):
    rng = np.random.default_rng(sum(shape))
    n_users, n_lists, k_in, _ = shape
    k = min(shape[3], n_lists * k_in)
    for kind in KINDS:
        scores, rows, n_valid, n_items = _contents(kind, shape, rng)
        for mode in MODES:
            if kind == "neg_inf" and mode in (FM.SUM_FLOOR, FM.MINMAX):
                continue  # (+-inf under these two is outside the contract)
            # per-call weights; positive where -inf stands among the scores (0 * -inf and inf - inf are outside the contract)
            w = rng.standard_normal(n_lists).astype(F)
            w = np.abs(w) + F(0.25) if kind == "neg_inf" else w
            got = _check(scores, rows, n_valid, n_items, k, mode, (kind, shape), weights=None if mode == FM.RRF and kind == "equal" else w,
                         rrf_c=float(rng.choice([0.0, 1.5, 60.0])))
            if kind == "identical":
                assert (got["n_out"] == min(k, k_in)).all()
                assert (got["lists"][:, :min(k, k_in)] == np.uint64(2 ** n_lists - 1)).all()  # every list holds every row
            if kind == "disjoint":
                assert (got["n_out"] == k).all()
                m = got["lists"].astype(object)
                assert all(bin(int(v)).count("1") == 1 for v in m.reshape(-1))
            if kind == "pool7":
                assert (got["n_out"] <= 7).all()
    if n_lists == 64:
        assert (got["lists"] >> np.uint64(63)).any()  # mask bit 63 was exercised


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_n_valid_and_rows_out_of_range(shape):
    n_users, n_lists, k_in, k = shape
    k = min(k, n_lists * k_in)
    rng = np.random.default_rng(7 + sum(shape))
    n_items = max(n_lists * k_in // 3, 2)
    scores = VALUES[1:][rng.integers(0, len(VALUES) - 1, (n_users, n_lists, k_in))]
    rows = rng.integers(0, n_items, (n_users, n_lists, k_in)).astype(np.int32)
    bad = rng.random(rows.shape) < 0.1
    rows[bad] = rng.choice(np.array([-1, n_items, n_items + 5, -2 ** 31, 2 ** 31 - 1], np.int64), int(bad.sum())).astype(np.int32)
    rows.reshape(-1)[0] = -1
    rows.reshape(-1)[-1] = n_items
    n_valid = rng.integers(-3, k_in + 4, (n_users, n_lists)).astype(np.int32)  # negative and beyond k_in among them
    n_valid[-1] = 0                                                            # the last user brings nothing
    for mode in MODES:
        got = _check(scores, rows, n_valid, n_items, k, mode, shape)
        assert got["n_out"][-1] == 0
        assert not got["index"][-1].any() and not bits(got["scores"][-1]).any() and not got["item_ids"][-1].any()
        assert not got["lists"][-1].any()
    # every count at the ends of its range
    for fill in (-5, 0, 1, k_in, k_in + 9):
        _check(scores, rows, np.full((n_users, n_lists), fill, np.int32), n_items, k, MODES[fill % 4], (shape, fill))


def test_weights_per_user_negative_and_zero():
    rng = np.random.default_rng(21)
    n_users, n_lists, k_in, k, n_items = 4, 5, 33, 100, 70
    scores = rng.standard_normal((n_users, n_lists, k_in)).astype(F)
    rows = rng.integers(0, n_items, (n_users, n_lists, k_in)).astype(np.int32)
    w = rng.choice(np.array([-2.0, -0.5, 0.0, 0.0, 0.75, 1.0, 3.0], F), (n_users, n_lists)).astype(F)
    w[0] = 0.0   # a user whose lists all weigh nothing: every fused score is a zero, the first positions win
    w[1] = -1.0  # a user who ranks by the least score
    for mode in MODES:
        got = _check(scores, rows, None, n_items, k, mode, "per user", weights=w)
        assert not bits(got["scores"][0] + F(0.0)).any()
        _check(scores, rows, None, n_items, k, mode, "per call", weights=w[2])
    # the two layouts hold the same answer when every user has the per-call weights
    a = _call(scores, rows, None, n_items, k, FM.MINMAX, weights=w[2])
    b = _call(scores, rows, None, n_items, k, FM.MINMAX, weights=np.tile(w[2], (n_users, 1)))
    _same(a, b)
    # and no weights are weights of one
    _same(_call(scores, rows, None, n_items, k, FM.SUM_FLOOR), _call(scores, rows, None, n_items, k, FM.SUM_FLOOR, weights=np.ones(n_lists, F)))


def test_a_user_does_not_depend_on_its_batch():
    rng = np.random.default_rng(99)
    n_users, n_lists, k_in, k, n_items = 5, 4, 64, 100, 90
    scores = VALUES[1:][rng.integers(0, len(VALUES) - 1, (n_users, n_lists, k_in))]
    rows = rng.integers(-1, n_items + 1, (n_users, n_lists, k_in)).astype(np.int32)
    n_valid = rng.integers(0, k_in + 1, (n_users, n_lists)).astype(np.int32)
    w = rng.standard_normal((n_users, n_lists)).astype(F)
    for mode in MODES:
        batch = _check(scores, rows, n_valid, n_items, k, mode, weights=w)
        for u in (0, 3):
            alone = _check(scores[u:u + 1], rows[u:u + 1], n_valid[u:u + 1], n_items, k, mode, weights=w[u:u + 1])
            for name in batch:
                g, e = (bits(alone[name]), bits(batch[name][u:u + 1])) if name == "scores" else (alone[name], batch[name][u:u + 1])
                assert (g == e).all(), name


def test_optional_outputs_null():
    rng = np.random.default_rng(5)
    scores = rng.standard_normal((3, 2, 5)).astype(F)
    rows = rng.integers(0, 6, (3, 2, 5)).astype(np.int32)
    item_ids = np.arange(6, dtype=np.int64) + 100
    exp = FM.model(scores, rows, None, 6, 7, FM.RRF, item_ids=item_ids)
    got = _call(scores, rows, None, 6, 7, FM.RRF, item_ids=None, want=())
    assert set(got) == {"index"}
    _same(got, exp)
    for name in ("scores", "item_ids", "lists", "n_out"):  # each of the four NULL in turn, and alone
        want = tuple(n for n in ("scores", "item_ids", "lists", "n_out") if n != name)
        got = _call(scores, rows, None, 6, 7, FM.RRF, item_ids=item_ids, want=want)
        assert set(got) == set(want) | {"index"}
        _same(got, exp, name)
        _same(_call(scores, rows, None, 6, 7, FM.RRF, item_ids=item_ids, want=(name,)), exp, name)


def test_a_non_default_stream():
    rng = np.random.default_rng(6)
    scores = rng.standard_normal((4, 4, 64)).astype(F)
    rows = rng.integers(0, 50, (4, 4, 64)).astype(np.int32)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = _call(scores, rows, None, 50, 100, FM.MINMAX, stream=s)
    _same(got, FM.model(scores, rows, None, 50, 100, FM.MINMAX))


def test_the_python_call():
    from nann_amd import retrieval
    rng = np.random.default_rng(8)
    scores = rng.standard_normal((3, 3, 7)).astype(F)
    rows = rng.integers(-1, 12, (3, 3, 7)).astype(np.int32)
    n_valid = rng.integers(0, 8, (3, 3)).astype(np.int32)
    w = np.array([[1.0, 0.5, 2.0]] * 3, F) * np.array([[1.0], [-1.0], [0.25]], F)
    for mode, weights in (("rrf", None), ("sum", w[0]), ("sum_floor", w), ("minmax", w)):
        r = retrieval.fuse_topk(cuda(scores), cuda(rows), retrieval.make_fusion(mode, weights=weights, rrf_c=10.0), 21, n_valid=cuda(n_valid))
        torch.cuda.synchronize()
        exp = FM.model(scores, rows, n_valid, 2 ** 31 - 1, 21, FM.MODES[mode], weights=weights, rrf_c=10.0)
        assert r.item_ids is None and r.status is None and r.plan is None and r.lists.dtype == torch.int64
        assert (r.index.cpu().numpy() == exp["index"]).all() and (bits(r.scores.cpu().numpy()) == bits(exp["scores"])).all()
        assert (r.lists.cpu().numpy().view(np.uint64) == exp["lists"]).all() and (r.n_out.cpu().numpy() == exp["n_out"]).all()
