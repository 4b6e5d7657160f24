#!/usr/bin/env python3
"""Inner-product scorer next to the L2 scorer: ms per call of the same three calls under ops.Scorer("l2") and ops.Scorer("ip")
on ONE index.  bench.py's headline index (1M x 128 f16, ef 128) and its query generator, k = 200:
  search             retrieval.search, 1 024 queries, level_topn = [128] * 5 + [200]
  search_all         retrieval.search_all, 64 queries
  search_candidates  retrieval.search_candidates, 1 024 queries, one list of 5 000 random rows each
One process, every shape warmed, L2 and IP alternating inside a round, device events around a window of calls that lasts at
least a second and ends in a synchronise; median of the rounds, min..max beside it.  The figure of merit is IP time / L2 time
per call; the L2 kernels of a build are its parent's, so the L2 column is the yardstick.  The spread of the repeated L2
windows (max / min) is printed beside every ratio: IP runs a subset of L2's instructions, and a ratio above 1 by more than that
spread wants an explanation.  The two metrics must return different ids, or the tool stops: an IP call that
ranks like L2 measures nothing.
usage: tools/ip_rate.py [--rounds R] [--out FILE]
writes profiles/ip_rate.txt (or FILE) and prints the same."""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITEMS, DIM, EF, K = 1_000_000, 128, 128, 200
N_Q, N_Q_ALL, LIST_ROWS = 1024, 64, 5_000
WINDOW_MS = 1000.0


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(pairs, rounds):
    """pairs: [(name, fn)] -> {name: [ms per call, one per round]}, the functions alternating inside a round; a window is
    as many calls as fill WINDOW_MS at the pace of a first, warm, window of three"""
    for _, fn in pairs:  # warm every shape
        fn()
    torch.cuda.synchronize()
    reps = {name: max(1, math.ceil(WINDOW_MS / timed(fn, 3))) for name, fn in pairs}
    out = {name: [] for name, _ in pairs}
    for _ in range(rounds):
        for name, fn in pairs:
            out[name].append(timed(fn, reps[name]))
    return out


def fmt(ms):
    return f"{statistics.median(ms):10.3f} ms ({min(ms):.3f}..{max(ms):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ip_rate.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    sys.path.insert(0, ROOT)
    import bench
    from nann_amd import ops, retrieval
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    g = bench.make_index(ITEMS, DIM, EF, "hnsw", 1.0, "f16", 0, dev, 16)
    index = retrieval.Index.from_dict(g, device=dev)
    q = ops.user_seq_mean(bench.make_query_batches(DIM, N_Q, 1, 1.0, dev, n_clusters=bench.n_clusters_for(ITEMS, EF))[0])
    l2, ip = ops.Scorer("l2", DIM, torch.float16), ops.Scorer("ip", DIM, torch.float16)
    topn = [EF] * 5 + [K]
    rng = np.random.default_rng(2026)
    rows = torch.as_tensor(rng.integers(0, ITEMS, (N_Q, LIST_ROWS)).astype(np.int32)).to(dev)
    splits = torch.arange(N_Q + 1, dtype=torch.int64, device=dev) * LIST_ROWS
    calls = [
        (f"search, {N_Q} queries, ef {EF}", lambda sc: retrieval.search(index, sc, q, topn, want_counters=False)),
        (f"search_all, {N_Q_ALL} queries", lambda sc: retrieval.search_all(index, sc, q[:N_Q_ALL], K)),
        (f"search_candidates, {N_Q} queries x {LIST_ROWS} rows", lambda sc: retrieval.search_candidates(index, sc, q, candidates=(splits, rows), k=K)),
    ]
    lines = [f"ip_rate: {ITEMS} items x {DIM} f16, k = {K}, rounds = {args.rounds} x windows of >= {WINDOW_MS / 1e3:.0f} s (median, "
             f"min..max); device {torch.cuda.get_device_name(0)}"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    for name, call in calls:
        a, b = call(l2), call(ip)
        torch.cuda.synchronize()
        assert not torch.equal(a.item_ids, b.item_ids), f"{name}: the two metrics return the same ids"
        differ = float((a.item_ids[:, 0] != b.item_ids[:, 0]).float().mean())
        res = measure([("l2", lambda: call(l2)), ("ip", lambda: call(ip))], args.rounds)
        ratio = statistics.median(res["ip"]) / statistics.median(res["l2"])
        spread = max(res["l2"]) / min(res["l2"])
        emit(name)
        emit(f"  L2: {fmt(res['l2'])}")
        emit(f"  IP: {fmt(res['ip'])}")
        emit(f"  IP / L2 = {ratio:.3f}   (repeated L2 windows: max / min = {spread:.3f}; top-1 differs for {100 * differ:.0f} % of the queries)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
