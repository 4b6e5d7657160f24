"""-m gpu: the union top-k on the device (nann_union_topk / retrieval.union_topk) against the numpy model of its contract
(union_model.model), bit for bit on rows, scores, item ids, lists and n_out.  The calls go through the C ABI with outputs
pre-filled with a canary and guard bands around them."""
import ctypes as C

import numpy as np
import pytest
import torch

import union_model as UM
from gpu_util import bits, cuda, require_gpu

pytestmark = pytest.mark.gpu
GUARD = 64
CANARY = 0x5A


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


def _call(scores, rows, n_valid, n_items, k, item_ids=None, want=("scores", "item_ids", "list", "n_out"), stream=None):
    """nann_union_topk -> dict like union_model.model's; outputs not in `want` are passed as NULL"""
    from nann_amd import _lib
    from nann_amd.ops import _ptr, _stream
    L = _lib.lib()
    n_users, n_lists, k_in = scores.shape
    d_scores, d_rows = cuda(scores, torch.float32), cuda(rows, torch.int32)
    d_nv = cuda(n_valid, torch.int32) if n_valid is not None else None
    d_ids = cuda(item_ids, torch.int64) if item_ids is not None else None
    outs = {"index": _Out(n_users, k, torch.int32)}
    if "scores" in want:
        outs["scores"] = _Out(n_users, k, torch.float32)
    if "item_ids" in want and item_ids is not None:
        outs["item_ids"] = _Out(n_users, k, torch.int64)
    if "list" in want:
        outs["list"] = _Out(n_users, k, torch.int32)
    if "n_out" in want:
        outs["n_out"] = _Out(n_users, 1, torch.int32)
    nb = C.c_int64(-1)
    assert L.nann_union_topk_workspace_bytes(n_users, n_lists, k_in, C.byref(nb)) == 0
    ws = torch.full((max(nb.value, 1),), 0xA5, dtype=torch.uint8, device="cuda")  # (the kernel zeroes what it uses itself)
    p = lambda name: outs[name].ptr() if name in outs else None
    st = L.nann_union_topk(_ptr(d_scores), _ptr(d_rows), _ptr(d_nv), n_users, n_lists, k_in, n_items, _ptr(d_ids), k, p("index"),
                           p("scores"), p("item_ids"), p("list"), p("n_out"), _ptr(ws), nb.value,
                           C.c_void_p(stream.cuda_stream) if stream is not None else _stream())
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


def _check(scores, rows, n_valid, n_items, k, what="", **kw):
    item_ids = np.arange(n_items, dtype=np.int64) * 7 + 3
    got = _call(scores, rows, n_valid, n_items, k, item_ids=item_ids, **kw)
    _same(got, UM.model(scores, rows, n_valid, n_items, k, item_ids=item_ids), what)
    return got


SHAPES = [(1, 1, 1, 1), (3, 2, 5, 7), (4, 4, 64, 100), (2, 8, 1024, 1024), (3, 3, 7, 21)]
VALUES = np.array([-np.inf, -2.5, -0.0, 0.0, 0.5, 3.0], np.float32)


def _contents(kind, shape, rng):
    """(scores, rows, n_items) of one kind of content for a shape"""
    n_users, n_lists, k_in, _ = shape
    n_in = n_lists * k_in
    n_items = 3 * n_in + 11
    scores = rng.standard_normal((n_users, n_lists, k_in)).astype(np.float32)
    if kind == "identical":      # every list of a user holds the same rows with the same scores
        rows = np.stack([rng.permutation(n_items)[:k_in] for _ in range(n_users)])[:, None, :].repeat(n_lists, 1)
        scores = scores[:, :1, :].repeat(n_lists, 1)
    elif kind == "disjoint":
        rows = np.stack([rng.permutation(n_items)[:n_in] for _ in range(n_users)]).reshape(n_users, n_lists, k_in)
    elif kind == "pool7":        # nearly every entry collides
        n_items = 7
        rows = rng.integers(0, 7, (n_users, n_lists, k_in))
    elif kind == "equal":        # one score everywhere: position order decides
        rows = rng.integers(0, n_items, (n_users, n_lists, k_in))
        scores[:] = np.float32(1.25)
    elif kind == "zeros":        # -0 and +0 tie
        rows = rng.integers(0, max(n_in // 2, 1), (n_users, n_lists, k_in))
        scores = np.where(rng.random(scores.shape) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    elif kind == "neg_inf":      # -inf is a score like any other
        rows = rng.integers(0, max(n_in // 2, 1), (n_users, n_lists, k_in))
        scores = VALUES[rng.integers(0, len(VALUES), scores.shape)]
        scores[0] = -np.inf
    else:
        raise AssertionError(kind)
    return np.ascontiguousarray(scores, np.float32), np.ascontiguousarray(rows, np.int32), n_items


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_content_bitwise(shape):
    rng = np.random.default_rng(sum(shape))
    for kind in ("identical", "disjoint", "pool7", "equal", "zeros", "neg_inf"):
        scores, rows, n_items = _contents(kind, shape, rng)
        k = min(shape[3], shape[1] * shape[2])
        got = _check(scores, rows, None, n_items, k, (kind, shape))
        if kind == "identical":
            assert (got["n_out"] == min(k, shape[2])).all() and not got["list"].any()  # the first list represents every row
        if kind == "disjoint":
            assert (got["n_out"] == k).all()
        if kind == "pool7":
            assert (got["n_out"] <= 7).all()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_n_valid_and_rows_out_of_range(shape):
    n_users, n_lists, k_in, k = shape
    rng = np.random.default_rng(7 + sum(shape))
    n_items = max(n_lists * k_in // 3, 2)
    scores = VALUES[rng.integers(0, len(VALUES), (n_users, n_lists, k_in))]
    rows = rng.integers(0, n_items, (n_users, n_lists, k_in)).astype(np.int32)
    bad = rng.random(rows.shape) < 0.1
    rows[bad] = rng.choice(np.array([-1, n_items, n_items + 5, -2 ** 31, 2 ** 31 - 1], np.int64), int(bad.sum())).astype(np.int32)
    rows.reshape(-1)[0] = -1
    rows.reshape(-1)[-1] = n_items
    n_valid = rng.integers(-3, k_in + 4, (n_users, n_lists)).astype(np.int32)  # negative and beyond k_in among them
    n_valid[-1] = 0                                                            # the last user brings nothing
    got = _check(scores, rows, n_valid, n_items, k, shape)
    assert got["n_out"][-1] == 0
    assert not got["index"][-1].any() and not bits(got["scores"][-1]).any() and not got["item_ids"][-1].any()
    # every count at the ends of its range
    for fill in (-5, 0, k_in, k_in + 9):
        _check(scores, rows, np.full((n_users, n_lists), fill, np.int32), n_items, k, (shape, fill))


def test_a_user_does_not_depend_on_its_batch():
    rng = np.random.default_rng(99)
    n_users, n_lists, k_in, k, n_items = 5, 4, 64, 100, 90
    scores = VALUES[rng.integers(0, len(VALUES), (n_users, n_lists, k_in))]
    rows = rng.integers(-1, n_items + 1, (n_users, n_lists, k_in)).astype(np.int32)
    n_valid = rng.integers(0, k_in + 1, (n_users, n_lists)).astype(np.int32)
    batch = _check(scores, rows, n_valid, n_items, k)
    alone = _check(scores[:1], rows[:1], n_valid[:1], n_items, k)
    for name in batch:
        g, e = (bits(alone[name]), bits(batch[name][:1])) if name == "scores" else (alone[name], batch[name][:1])
        assert (g == e).all(), name


def test_optional_outputs_null():
    rng = np.random.default_rng(5)
    scores = rng.standard_normal((3, 2, 5)).astype(np.float32)
    rows = rng.integers(0, 6, (3, 2, 5)).astype(np.int32)
    exp = UM.model(scores, rows, None, 6, 7)
    got = _call(scores, rows, None, 6, 7, item_ids=None, want=())
    assert set(got) == {"index"}
    _same(got, exp)
    item_ids = np.arange(6, dtype=np.int64) + 100
    _same(_call(scores, rows, None, 6, 7, item_ids=item_ids, want=("item_ids",)), UM.model(scores, rows, None, 6, 7, item_ids=item_ids))
    _same(_call(scores, rows, None, 6, 7, item_ids=item_ids, want=("list", "n_out")), exp)  # item_ids given, out_item_ids NULL


def test_a_non_default_stream():
    rng = np.random.default_rng(6)
    scores = rng.standard_normal((4, 4, 64)).astype(np.float32)
    rows = rng.integers(0, 50, (4, 4, 64)).astype(np.int32)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = _call(scores, rows, None, 50, 100, stream=s)
    _same(got, UM.model(scores, rows, None, 50, 100))


def test_the_python_call():
    from nann_amd import retrieval
    rng = np.random.default_rng(8)
    scores = rng.standard_normal((3, 3, 7)).astype(np.float32)
    rows = rng.integers(-1, 12, (3, 3, 7)).astype(np.int32)
    n_valid = rng.integers(0, 8, (3, 3)).astype(np.int32)
    r = retrieval.union_topk(cuda(scores), cuda(rows), 21, n_valid=cuda(n_valid))
    torch.cuda.synchronize()
    exp = UM.model(scores, rows, n_valid, 2 ** 31 - 1, 21)
    assert r.item_ids is None and r.status is None and r.plan is None
    assert (r.index.cpu().numpy() == exp["index"]).all() and (bits(r.scores.cpu().numpy()) == bits(exp["scores"])).all()
    assert (r.vec.cpu().numpy() == exp["list"]).all() and (r.n_out.cpu().numpy() == exp["n_out"]).all()
