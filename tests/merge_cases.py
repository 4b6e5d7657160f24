"""Named cases of the shard merge and of TopKV2 beyond k = 1024: a shape and a content each.  tests/test_merge_model_cpu.py
runs the host code and the mutants of tests/merge_model.py over them, tests/test_merge_gpu.py the device.

A merge case `shape:content` is (world, k_in, k_out, n_queries) with per-shard lists scores f32[B, world, k_in], ids
i64[B, world, k_in] and status i32[world, B] (None: the call gets no status).  Ids are unique over (query, shard, slot) and
go beyond 32 bits, so a result names the slots it was taken from."""
import functools
import zlib

import numpy as np

import merge_model as MM

# name -> (world, k_in, k_out, n_queries)
SHAPES = {
    "a200": (8, 200, 200, 70),        # configs[3]'s exchange: 8 shards' top-200
    "a50": (8, 200, 50, 70),          # k_out < k_in at world > 1
    "w1": (1, 200, 150, 5),           # one shard
    "w1_min": (1, 1, 1, 1),
    "odd": (3, 7, 21, 9),             # k_out == world * k_in; 756 bytes of record, 768 of stride, ids at an odd word
    "e1023": (3, 341, 1023, 3),       # world * k_in on either side of the register-slot edges of the selection
    "e1024": (2, 512, 1024, 3),
    "e1025": (5, 205, 1024, 3),
    "e2048": (4, 512, 300, 3),
    "e2049": (3, 683, 1024, 2),
    "e4096": (8, 512, 512, 2),
    "e4097": (17, 241, 241, 2),
    "e8192": (16, 512, 1000, 2),
    "e8193": (3, 2731, 200, 2),
    "lds_optin": (13, 1024, 1024, 3),  # 13 312 keys = 53 KB of dynamic LDS: the opt-in
    "limit": (16, 1024, 1024, 2),      # 16 384 keys: the most the call takes
    "q1": (8, 200, 200, 1),
    "q257": (4, 50, 64, 257),
}
ALL_CONTENTS = ("distinct", "ties", "all_equal", "l2_like", "special", "failed", "best_last")
FEW_CONTENTS = ("distinct", "ties", "failed")
EVERY_CONTENT_AT = ("a200", "a50", "w1", "w1_min")
# nann_merge_topk alone goes beyond 16 384 keys (it re-reads them from memory)
REREAD_SHAPE = ("reread", (17, 1024, 1024, 2))

MERGE_CASES = [f"{s}:{c}" for s in SHAPES for c in (ALL_CONTENTS if s in EVERY_CONTENT_AT else FEW_CONTENTS)]
MERGE_TOPK_CASES = MERGE_CASES + [f"{REREAD_SHAPE[0]}:{c}" for c in FEW_CONTENTS]

# nann_topk beyond the selection kernel's k = 1024: (n_cols, k), 3 rows each
TOPK_SHAPES = [(1025, 1025), (1500, 1025), (4096, 2048), (4097, 4097), (16384, 1025), (16384, 16384)]
TOPK_CONTENTS = ("distinct", "ties", "all_equal", "special")
TOPK_ROWS = 3


def _ids(b, world, k_in):
    q, s, j = np.meshgrid(np.arange(b), np.arange(world), np.arange(k_in), indexing="ij")
    return ((s.astype(np.int64) + 1) << 40) | (q.astype(np.int64) << 16) | j.astype(np.int64)


def _distinct(rng, b, world, k_in):
    n = world * k_in
    return np.stack([(rng.permutation(n).astype(np.float32) - n // 3) / 8 for _ in range(b)]).reshape(b, world, k_in)


def _ties(rng, b, world, k_in):
    return rng.integers(0, 8, size=(b, world, k_in)).astype(np.float32) / 8


def _all_equal(rng, b, world, k_in):
    return np.full((b, world, k_in), 1.5, np.float32)


def _l2_like(rng, b, world, k_in):
    return -(1 + rng.random((b, world, k_in))).astype(np.float32)  # [-2, -1]: one binade


def _special(rng, b, world, k_in):
    tiny = np.float32(1.4e-45)  # the smallest subnormal
    pos = np.array([tiny, 2 * tiny, 1e-38, 1.0, 3.5, 3e38, np.inf], np.float32)
    # 3 % above zero, half zeros of either sign, the rest below: the zeros straddle the cut of every shape that runs this
    u = rng.random((b, world, k_in))
    s = np.where(u < 0.03, pos[rng.integers(0, len(pos), size=u.shape)],
                 np.where(u < 0.53, np.where(rng.random(u.shape) < 0.5, np.float32(0.0), np.float32(-0.0)),
                          -pos[rng.integers(0, len(pos) - 1, size=u.shape)])).astype(np.float32)
    s[:, :, k_in - k_in // 4:] = -np.inf  # a list that ran short ends in -inf
    return s


def _failed(rng, b, world, k_in):
    return -np.sort(-(rng.integers(0, 500, size=(b, world, k_in)).astype(np.float32) / 8), axis=2)  # descending, ties


def _failed_status(rng, b, world):
    st = np.zeros((world, b), np.int32)
    if b >= 5:
        st[rng.random((world, b)) < 0.2] = 6
    st[0, 0] = 4               # the first query, on the first shard
    st[world - 1, b - 1] = 6   # the last query, on the last shard
    st[:, b // 2] = 4          # a query that every shard failed
    return st


def _best_last(rng, b, world, k_in):
    s = -np.sort(-rng.random((b, world, k_in)).astype(np.float32), axis=2)  # every list descending ...
    return s + np.arange(world, dtype=np.float32)[None, :, None]           # ... and shard s + 1 above all of shard s


_CONTENT = {"distinct": _distinct, "ties": _ties, "all_equal": _all_equal, "l2_like": _l2_like, "special": _special,
            "failed": _failed, "best_last": _best_last}


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


@functools.lru_cache(maxsize=None)
def merge_case(name):
    """-> dict(world, k_in, k_out, b, scores, ids, status); the arrays are shared: do not write to them"""
    shape, content = name.split(":")
    world, k_in, k_out, b = REREAD_SHAPE[1] if shape == REREAD_SHAPE[0] else SHAPES[shape]
    rng = _rng(name)
    scores = np.ascontiguousarray(_CONTENT[content](rng, b, world, k_in), np.float32)
    if content == "failed":
        status = _failed_status(rng, b, world)
    elif content in ("ties", "special"):
        status = np.zeros((world, b), np.int32)  # a status that names no failure
    else:
        status = None
    c = dict(name=name, world=world, k_in=k_in, k_out=k_out, b=b, scores=scores, ids=_ids(b, world, k_in), status=status)
    for a in (c["scores"], c["ids"]):
        a.setflags(write=False)
    return c


def shard_status(c, s):
    return None if c["status"] is None else c["status"][s]


@functools.lru_cache(maxsize=None)
def records(name):
    """the gathered records of a case, each shard's packed from its OWN lists by the model: uint8[world, record_bytes]"""
    c = merge_case(name)
    r = np.stack([MM.pack(c["scores"][:, s], c["ids"][:, s], shard_status(c, s)) for s in range(c["world"])])
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def expected(name):
    """the model's merge of records(name) -> (scores f32[B, k_out], ids i64[B, k_out])"""
    c = merge_case(name)
    return MM.merge_records(records(name), c["world"], c["b"], c["k_in"], c["k_out"])


@functools.lru_cache(maxsize=None)
def merge_inputs(name):
    """what nann_merge_topk takes: the lists as the records carry them (failed queries as (-inf, 0)), [B, world, k_in]"""
    c = merge_case(name)
    return MM.gathered(records(name), c["world"], c["b"], c["k_in"])


@functools.lru_cache(maxsize=None)
def topk_case(n, k, content):
    """-> (rows f32[TOPK_ROWS, n], values f32[TOPK_ROWS, k], indices i32[TOPK_ROWS, k])"""
    rows = np.ascontiguousarray(_CONTENT[content](_rng(f"topk:{n}:{k}:{content}"), TOPK_ROWS, 1, n)[:, 0], np.float32)
    out = [MM.top_k(r, k) for r in rows]
    return rows, np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
