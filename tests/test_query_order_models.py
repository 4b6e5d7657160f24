"""CPU: models of the batch order (nann_amd/csrc/nann_order.h) and of k_search's per-XCD pull loop
(nann_search.h), statement by statement, with the atomic operations of concurrent workgroups applied in random order:

* k_order_perm -- histogram, exclusive prefix, then per 1024-query tile a rank inside each 64-lane wave (shuffles) and
  wave offsets by a per-key scan: must equal a stable argsort of the keys;
* the pull loop -- kOrderSegs contiguous segments of perm, one head each; a workgroup drains its XCD's segment, then
  the others in a fixed rotation: every query is taken exactly once, and no workgroup leaves while work remains, for
  any XCD assignment (all on one XCD included) and any interleaving."""
import numpy as np
import pytest

SEGS = 8


def seg_begin(n, s):
    return n * s // SEGS


def order_perm_model(key, P, threads=1024):
    n = len(key)
    W = threads // 64
    base = np.bincount(key, minlength=P)
    base = np.concatenate([[0], np.cumsum(base)[:-1]]).astype(np.int64)
    perm = np.full(n, -1, np.int64)
    for t0 in range(0, n, threads):
        wofs = np.zeros((W, P), np.int64)
        ks = np.full(threads, -1)
        m = min(threads, n - t0)
        ks[:m] = key[t0:t0 + m]
        rank = np.zeros(threads, np.int64)
        last = np.ones(threads, bool)
        for tid in range(threads):
            w, lane = divmod(tid, 64)
            for j in range(64):
                if ks[w * 64 + j] == ks[tid]:
                    if j < lane:
                        rank[tid] += 1
                    elif j > lane:
                        last[tid] = False
        for tid in range(threads):
            if ks[tid] >= 0 and last[tid]:
                wofs[tid // 64, ks[tid]] = rank[tid] + 1
        for p in range(P):
            run = base[p]
            for v in range(W):
                c = wofs[v, p]
                wofs[v, p] = run
                run += c
            base[p] = run
        for tid in range(m):
            perm[wofs[tid // 64, ks[tid]] + rank[tid]] = t0 + tid
    return perm


@pytest.mark.parametrize("n,P,seed", [(1, 2, 0), (70, 3, 1), (1025, 17, 2), (2500, 128, 3), (3000, 1, 4)])
def test_order_perm_is_a_stable_sort(n, P, seed):
    rng = np.random.default_rng(seed)
    key = rng.integers(0, P, n) if seed % 2 else np.sort(rng.integers(0, P, n))[::-1].copy()
    assert (order_perm_model(key, P) == np.argsort(key, kind="stable")).all()


def pull_loop_model(n, xcd_of_wg, rng, busy=3):
    """Workgroups pull and 'work' (a random number of steps) until the pull loop sends them away; a step is one
    workgroup's next action, in random order.  Returns the queries taken, in order, and the set of queries that were
    still untaken when each workgroup left."""
    perm = rng.permutation(n)
    heads = [0] * SEGS
    seg = [0] * len(xcd_of_wg)
    left_while_work = []
    taken = []
    alive = {w: 0 for w in range(len(xcd_of_wg))}  # remaining busy steps
    while alive:
        w = int(rng.choice(list(alive)))
        if alive[w]:
            alive[w] -= 1
            continue
        qn = n
        x = xcd_of_wg[w] % SEGS
        while seg[w] < SEGS:
            s = (x + seg[w]) % SEGS
            lo, cnt = seg_begin(n, s), seg_begin(n, s + 1) - seg_begin(n, s)
            pos = heads[s]
            heads[s] += 1  # atomicAdd
            if pos < cnt:
                qn = int(perm[lo + pos])
                break
            seg[w] += 1
        if qn >= n:
            if len(taken) < n and any(heads[s] < seg_begin(n, s + 1) - seg_begin(n, s) for s in range(SEGS)):
                left_while_work.append(w)
            del alive[w]
        else:
            taken.append(qn)
            alive[w] = int(rng.integers(0, busy))
    return taken, left_while_work


@pytest.mark.parametrize("n", [1, 7, 8, 9, 511, 513, 4097])
@pytest.mark.parametrize("placement", ["round_robin", "one_xcd", "random"])
def test_pull_loop_takes_every_query_once(n, placement):
    rng = np.random.default_rng(n)
    wgs = 64
    xcd = {"round_robin": np.arange(wgs) % SEGS, "one_xcd": np.full(wgs, 5),
           "random": rng.integers(0, 16, wgs)}[placement]
    taken, left = pull_loop_model(n, list(xcd), rng)
    assert sorted(taken) == list(range(n))
    assert left == [], "a workgroup left while a segment still held work"
