"""CPU: a numpy model of k_order_perm's fast path (nann_amd/csrc/nann_order_kernels.h, n <= kOrderFastQueries), step by
step as the kernel does it:

* thread tid holds the keys of positions t * 1024 + tid; a wavefront of a tile is a run of 64 consecutive queries;
* the lanes of a run that hold a lane's key: seven ballots, one per key bit, each ANDed in as it is or complemented;
  rank = popcount of that mask below the lane, and the highest lane of a mask writes cnt[key][run] = its size (u16);
* one exclusive scan of the [128][128] table in key-major, run-minor order: 16 consecutive entries per thread, an
  inclusive scan over the 64 threads of a wavefront, 16 wavefront totals; the prefixes go back as u16;
* perm[cnt[key][run] + rank] = i.

The result must be the stable sort of the query indices by key."""
import numpy as np
import pytest

THREADS, MAX_PIVOTS, FAST_QUERIES = 1024, 128, 8192  # nann_order.h: kOrderSortThreads, kOrderMaxPivots, kOrderFastQueries
RUNS = FAST_QUERIES // 64
W = THREADS // 64


def same_key_masks(k):
    """k: [runs, 64] keys, -1 = no query.  [runs, 64, 64] bool: mask[r, i, j] = lane j is in lane i's mask."""
    m = np.broadcast_to((k >= 0)[:, None, :], k.shape + (64,)).copy()  # ballot(k >= 0)
    for b in range(7):
        bit = ((k >> b) & 1).astype(bool)
        s = bit[:, None, :]                                            # ballot(bit): the same for every lane
        m &= np.where(bit[:, :, None], s, ~s)
    return m


def fast_path_model(key):
    n = len(key)
    assert n <= FAST_QUERIES
    k = np.full(FAST_QUERIES, -1, np.int64)
    k[:n] = key
    k = k.reshape(RUNS, 64)                      # run = t * W + w: positions run * 64 .. run * 64 + 63
    mask = same_key_masks(k)
    lanes = np.arange(64)
    rank = (mask & (lanes[None, None, :] < lanes[None, :, None])).sum(axis=2)
    last = ~(mask & (lanes[None, None, :] > lanes[None, :, None])).any(axis=2)
    cnt = np.zeros((MAX_PIVOTS, RUNS), np.uint16)
    live = (np.arange(RUNS) * 64 < n)[:, None] & (k >= 0)  # the kernel skips whole runs past n
    r, l = np.nonzero(live & last)
    assert len(set(zip(k[r, l], r))) == len(r), "two lanes write one (key, run) entry"
    cnt[k[r, l], r] = rank[r, l] + 1
    # the scan: thread tid owns entries 16 tid .. 16 tid + 15 of the flat table
    flat = cnt.reshape(THREADS, 16).astype(np.int64)
    tsum = flat.sum(axis=1)
    incl = np.cumsum(tsum.reshape(W, 64), axis=1)             # the wave scan
    wtot = incl[:, 63]
    wave_base = np.concatenate([[0], np.cumsum(wtot)[:-1]])   # every thread adds the totals of the waves below its own
    run0 = (incl - tsum.reshape(W, 64) + wave_base[:, None]).reshape(THREADS)
    excl = run0[:, None] + np.cumsum(flat, axis=1) - flat
    assert excl.max() < 1 << 16
    cnt = excl.astype(np.uint16).reshape(MAX_PIVOTS, RUNS)
    perm = np.full(n, -1, np.int64)
    r, l = np.nonzero(live)
    dst = cnt[k[r, l], r].astype(np.int64) + rank[r, l]
    assert len(np.unique(dst)) == len(dst)
    perm[dst] = r * 64 + l
    return perm


def key_sets(n, P, rng):
    i = np.arange(n)
    lone = np.full(n, P - 1)
    lone[n // 2] = 0
    return {
        "all_equal": np.full(n, P - 1),
        # non-increasing over the whole key range; strictly descending wherever n <= P
        "descending": (P - 1) - i * P // n,
        # every key is used, in turn: exactly once each at n == P, at most once at n < P
        "every_key": i % P,
        "every_key_shuffled": rng.permutation(n) % P,
        "all_but_one": lone,
        "random": rng.integers(0, P, n),
    }


@pytest.mark.parametrize("P", [2, 3, 128])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 513, 1024, 1025, 4096, 8191, 8192])
def test_fast_path_is_a_stable_sort(n, P):
    rng = np.random.default_rng(1000 * n + P)
    for name, key in key_sets(n, P, rng).items():
        key = np.asarray(key, np.int64)
        assert key.min() >= 0 and key.max() < P
        got = fast_path_model(key)
        assert (got == np.argsort(key, kind="stable")).all(), name


def test_every_key_exactly_once_and_strictly_descending():
    key = np.arange(MAX_PIVOTS)[::-1].copy()
    assert (np.diff(key) < 0).all() and len(np.unique(key)) == MAX_PIVOTS
    assert (fast_path_model(key) == np.argsort(key, kind="stable")).all()
    key = np.random.default_rng(5).permutation(MAX_PIVOTS)
    assert (fast_path_model(key) == np.argsort(key, kind="stable")).all()
