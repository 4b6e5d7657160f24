#!/usr/bin/env python3
"""Shared-list search: ms per call of retrieval.search_lists over a trained coarse partition, next to the same question asked of
search_candidates with every query's lists expanded into a row list of its own (the reference for time), next to search_all,
and the recall@200 of the probed cells against search_all.  1M x 128 f16 rows (a clustered synthetic corpus), L2, k = 200, 1 024
trained cells, 256 and 1 024 queries, n_probe 8 / 32 / 64.
One process, every shape warmed, the variants alternating inside a round, device events around REPS calls that end in a
synchronise; median of the rounds, min..max beside it.
The kernels' shares come from a trace of a short run:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kt -- python tools/lists_rate.py --trace
  tools/lists_rate.py --stats DIR/.../kt_kernel_stats.csv        (appends them to the output file)
usage: tools/lists_rate.py [items] [dim] [--rounds R] [--out FILE] [--trace | --stats CSV]
writes profiles/lists_rate.txt (or FILE) and prints the same."""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, CELLS, REPS = 200, 1024, 3
BATCHES, PROBES = (256, 1024), (8, 32, 64)
TRACE_CALLS, TRACE_BATCH, TRACE_PROBE = 5, 1024, 32
NEW_KERNELS = ("k_lists_plan", "k_lists_tile_q", "k_lists_scan", "k_lists_pad", "k_lists_finish")
TOPK_KERNELS = ("k_scan_slab_topk",)


def kernel_shares(path):
    """kernel_stats.csv of the --trace run -> lines: every kernel of the call and its share of the call's kernel time"""
    total = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0)
            for k in NEW_KERNELS + TOPK_KERNELS:
                if k in name:
                    total[k] = total.get(k, 0.0) + ns
    missing = [k for k in NEW_KERNELS + TOPK_KERNELS if k not in total]
    assert not missing, f"{path}: no row for {missing}"
    whole = sum(total.values())
    out = [f"kernel times (rocprofv3 --kernel-trace --stats, {TRACE_CALLS} calls of search_lists, batch {TRACE_BATCH}, n_probe = "
           f"{TRACE_PROBE}, k = {K}):"]
    for k in NEW_KERNELS + TOPK_KERNELS:
        out.append(f"  {k:18s} {total[k] / TRACE_CALLS / 1e6:10.3f} ms per call = {100 * total[k] / whole:5.1f} % of its kernel time")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("items", nargs="?", type=int, default=1_000_000)
    ap.add_argument("dim", nargs="?", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lists_rate.txt"))
    ap.add_argument("--trace", action="store_true", help="a short run for a kernel trace")
    ap.add_argument("--stats", help="kernel_stats.csv of a --trace run: append the kernels' shares to the output file")
    args = ap.parse_args()
    if args.stats:
        lines = kernel_shares(args.stats)
        print("\n".join(lines))
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        return

    import numpy as np
    import torch
    from nann_amd import ops, retrieval, synth
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n, d = args.items, args.dim
    embs, _ = synth.make_corpus(n, d, n_clusters=max(64, n // 4096), noise=1.0)
    # the flat calls never read the graph: a ring (every node linked to the next eight) is a valid one
    deg = 8
    nbv = ((np.arange(n, dtype=np.int64)[:, None] + 1 + np.arange(deg)) % n).astype(np.int32).reshape(-1)
    rs = np.arange(n + 1, dtype=np.int64) * deg
    index = retrieval.Index(embs, synth.make_item_ids(n), [nbv, nbv], [rs, rs], np.arange(0, n, max(n // 64, 1), dtype=np.int32)[:64])
    sc = ops.Scorer("l2", d, torch.float16)
    cells = min(CELLS, n)
    part, cent = retrieval.train_partition(index, cells, iters=10, seed=0)
    rng = np.random.default_rng(99)
    qa = embs[rng.integers(0, n, max(BATCHES))].astype(np.float32) + 0.3 * rng.standard_normal((max(BATCHES), d)).astype(np.float32)
    qa = torch.as_tensor(qa).to(dev)

    def probes_of(q, n_probe):
        sim = 2.0 * q @ cent.T - (cent * cent).sum(1)[None, :]
        return sim.topk(min(n_probe, cells), dim=1).indices.to(torch.int32).contiguous()

    if args.trace:
        q = qa[:TRACE_BATCH]
        pr = probes_of(q, TRACE_PROBE)
        for _ in range(TRACE_CALLS):
            retrieval.search_lists(index, part, sc, q, pr, K)
        torch.cuda.synchronize()
        print(f"trace run: {TRACE_CALLS} calls of search_lists, batch {TRACE_BATCH}, n_probe = {TRACE_PROBE}, k = {K}")
        return

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / REPS

    def fmt(ms):
        return f"{statistics.median(ms):10.3f} ms ({min(ms):.3f}..{max(ms):.3f})"

    lines = [f"lists_rate: {n} items x {d} f16, L2, k = {K}, {cells} trained cells (longest {part.max_len} rows), rounds = "
             f"{args.rounds} x {REPS} calls (median, min..max); device {torch.cuda.get_device_name(0)}"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    splits, rows = part.list_splits(), part.list_rows()
    lens = splits[1:] - splits[:-1]
    for b in BATCHES:
        q = qa[:b]
        ref = retrieval.search_all(index, sc, q, K)
        all_ms = None
        for n_probe in PROBES:
            pr = probes_of(q, n_probe)
            # every query's lists expanded into a row list of its own: what a caller had to build without the call
            pl = pr.long()
            qlen = lens[pl]                                              # [b, n_probe]
            cs = torch.zeros(b + 1, dtype=torch.int64, device=dev)
            cs[1:] = qlen.sum(1).cumsum(0)
            seg = torch.repeat_interleave(torch.arange(b * n_probe, device=dev), qlen.reshape(-1))
            seg_start = torch.cumsum(qlen.reshape(-1), 0) - qlen.reshape(-1)
            flat = rows[(splits[pl].reshape(-1)[seg] + torch.arange(seg.numel(), device=dev) - seg_start[seg])].contiguous()
            pairs = [("lists", lambda: retrieval.search_lists(index, part, sc, q, pr, K)),
                     ("cand", lambda: retrieval.search_candidates(index, sc, q, candidates=(cs, flat), k=K)),
                     ("all", lambda: retrieval.search_all(index, sc, q, K))]
            for _, fn in pairs:  # warm every shape
                fn()
            torch.cuda.synchronize()
            res = {name: [] for name, _ in pairs}
            for _ in range(args.rounds):
                for name, fn in pairs:
                    if name == "all" and all_ms is not None:
                        continue
                    res[name].append(timed(fn))
            all_ms = all_ms or res["all"]
            got = retrieval.search_lists(index, part, sc, q, pr, K)
            torch.cuda.synchronize()
            hit = (got.index[:, :, None] == ref.index[:, None, :]).any(2) & (torch.arange(K, device=dev)[None, :] < got.n_out[:, None])
            recall = float(hit.sum()) / (b * K)
            lists, cand = statistics.median(res["lists"]), statistics.median(res["cand"])
            emit(f"{b} queries, n_probe = {n_probe}: {int(cs[-1]) / b:.0f} rows per query, recall@{K} vs search_all = {recall:.4f}")
            emit(f"  search_lists:                        {fmt(res['lists'])}")
            emit(f"  search_candidates on the expansion:  {fmt(res['cand'])} = {cand / lists:.2f} x")
            emit(f"  search_all:                          {fmt(all_ms)} = {statistics.median(all_ms) / lists:.2f} x")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
