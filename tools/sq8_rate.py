#!/usr/bin/env python3
"""Scalar-quantised exhaustive search (retrieval.search_all_sq8: int8 codes on the integer matrix cores, a fetch of the best F
rows by approximate score, an exact re-rank) next to retrieval.search_all at a size a user runs: 1M x 128 f16 from synth, L2,
k = 200, batches of 64 and 1 024 queries, F = k, 2k, 4k.  Reported per batch:
  A        retrieval.search_all, ms per call;
  B<F>     retrieval.search_all_sq8(fetch = F), ms per call, and recall@k of its result against A's (the share of A's rows it
           returns, mean over the queries).
One process, every shape warmed, A and the B's alternating inside a round, device events around work that ends in a synchronise;
median of the rounds, min..max beside it.  The code table is made outside the timed region (its time is printed once).
Kernel times come from a run of their own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kt -- python tools/sq8_rate.py --trace
  python tools/sq8_rate.py --stats DIR/.../kt_kernel_stats.csv      # appends the kernel times to the output file
--trace runs TRACE_CALLS calls of search_all and of search_all_sq8 (F = 2k) at 128 queries -- ONE chunk of both, so that a
launch of k_scan_sq8 and one of k_scan_l2 score the same 128 queries x every row.
usage: tools/sq8_rate.py [items] [dim] [--rounds R] [--out FILE] [--trace | --stats CSV]
writes profiles/sq8_rate.txt (or FILE) and prints the same."""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 200
BATCHES = (64, 1024)
FETCH = (K, 2 * K, 4 * K)
TRACE_CALLS, TRACE_QUERIES, TRACE_FETCH = 5, 128, 2 * K
KERNELS = ("k_scan_sq8", "k_scan_l2", "k_scan_slab_topk", "k_scan_merge", "k_sq8_encode", "k_sq8_sort_rows", "k_cand_plan",
           "k_cand_score_l2", "k_cand_topk", "k_scan_transpose_q")


def kernel_times(path):
    """kernel_stats.csv of the --trace run -> lines: calls and average time of the kernels of both calls"""
    rows = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            for k in KERNELS:
                if k in name:
                    calls, ns = rows.get(k, (0, 0.0))
                    rows[k] = (calls + int(row.get("Calls") or 0), ns + float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0))
    assert "k_scan_sq8" in rows and "k_scan_l2" in rows, f"{path}: no row for k_scan_sq8 or k_scan_l2"
    lines = [f"kernel times (rocprofv3 --kernel-trace --stats; {TRACE_CALLS} calls of search_all and of search_all_sq8(fetch = {TRACE_FETCH}) "
             f"at {TRACE_QUERIES} queries = one chunk each, k = {K}, after one warming call of each; the slab top-k and the merge run in both "
             "calls, at k and at fetch; k_sq8_encode includes the one launch that made the table):"]
    for k in KERNELS:
        if k in rows:
            calls, ns = rows[k]
            lines.append(f"  {k:20s} {calls:4d} launches, {ns / max(calls, 1) / 1e3:10.1f} us each, {ns / 1e6:9.3f} ms in all")
    sq8, l2 = rows["k_scan_sq8"], rows["k_scan_l2"]
    lines.append(f"  k_scan_l2 / k_scan_sq8 per launch = {(l2[1] / l2[0]) / (sq8[1] / sq8[0]):.2f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("items", nargs="?", type=int, default=1_000_000)
    ap.add_argument("dim", nargs="?", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sq8_rate.txt"))
    ap.add_argument("--trace", action="store_true", help="a short run for a kernel trace")
    ap.add_argument("--stats", help="kernel_stats.csv of a --trace run: append the kernel times to the output file")
    args = ap.parse_args()
    if args.stats:
        lines = kernel_times(args.stats)
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
    embs, assign = synth.make_corpus(n, d, n_clusters=max(64, n // 4096), noise=1.0)
    # neither call reads the graph: a ring (every node linked to the next eight) is a valid one
    deg = 8
    nbv = ((np.arange(n, dtype=np.int64)[:, None] + 1 + np.arange(deg)) % n).astype(np.int32).reshape(-1)
    rs = np.arange(n + 1, dtype=np.int64) * deg
    index = retrieval.Index(embs, synth.make_item_ids(n), [nbv, nbv], [rs, rs], np.arange(0, n, n // 64, dtype=np.int32)[:64])
    sc = ops.Scorer("l2", d, torch.float16)
    q_all = ops.user_seq_mean(torch.as_tensor(synth.make_queries(embs, assign, max(BATCHES), seed=99)).to(dev))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    holder = {}
    t_table = timed(lambda: holder.setdefault("t", retrieval.make_sq8(index)))
    sq8 = holder["t"]

    if args.trace:
        q = q_all[:TRACE_QUERIES]
        for _ in range(TRACE_CALLS + 1):
            retrieval.search_all(index, sc, q, K)
            retrieval.search_all_sq8(index, sq8, sc, q, K, fetch=TRACE_FETCH)
        torch.cuda.synchronize()
        print(f"trace run: {TRACE_CALLS} + 1 calls of search_all and of search_all_sq8(fetch = {TRACE_FETCH}) at {TRACE_QUERIES} queries")
        return

    lines = [f"sq8_rate: {n} items x {d} f16, L2, k = {K}, rounds = {args.rounds} (median, min..max); device "
             f"{torch.cuda.get_device_name(0)}",
             f"code table: {sq8.nbytes / 1e6:.1f} MB next to {embs.nbytes / 1e6:.1f} MB of rows, made in {t_table:.3f} ms (first launch included)"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def fmt(ms):
        return f"{statistics.median(ms):9.3f} ms ({min(ms):.3f}..{max(ms):.3f})"

    for line in lines:
        print(line, flush=True)
    for b in BATCHES:
        q = q_all[:b]
        pairs = [("A", lambda: retrieval.search_all(index, sc, q, K))]
        for f_ in FETCH:
            pairs.append((f"B{f_}", lambda f_=f_: retrieval.search_all_sq8(index, sq8, sc, q, K, fetch=f_)))
        ref = retrieval.search_all(index, sc, q, K).index.cpu().numpy()
        recall = {}
        for f_ in FETCH:
            got = retrieval.search_all_sq8(index, sq8, sc, q, K, fetch=f_).index.cpu().numpy()
            recall[f_] = float(np.mean([len(np.intersect1d(got[i], ref[i])) / K for i in range(b)]))
        for _, fn in pairs:  # warm every shape
            fn()
        torch.cuda.synchronize()
        res = {name: [] for name, _ in pairs}
        for _ in range(args.rounds):
            for name, fn in pairs:
                res[name].append(timed(fn))
        a = statistics.median(res["A"])
        emit(f"batch {b}")
        emit(f"  A  search_all:                      {fmt(res['A'])}")
        for f_ in FETCH:
            m = statistics.median(res[f"B{f_}"])
            emit(f"  B  search_all_sq8, fetch = {f_:4d}:     {fmt(res[f'B{f_}'])}   A / B = {a / m:.2f}   recall@{K} against A = {recall[f_]:.4f}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
