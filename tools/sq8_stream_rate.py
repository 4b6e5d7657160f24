#!/usr/bin/env python3
"""Streamed scalar-quantised search (retrieval.search_all_sq8_stream: a cut from a sample of the table, the survivors of an int8
scan that stores no score, an exact re-rank) next to retrieval.search_all_sq8 at the same fetch, in one build and one run:
1M x 128 f16 and 4M x 128 f16 from synth (the second shows what the chunk does: search_all_sq8 scores 32 queries per chunk
there, the streamed call 128), L2 and IP, k = 200, batches of 64 and 1 024 queries, fetch = 200 and 400, the default sample
(max(65 536, n_items / 16) rows) and cap = 8 192, fallback off.  Reported per (size, metric, batch, fetch):
  A   retrieval.search_all_sq8, ms per call, and recall@k of its result against retrieval.search_all's;
  S   retrieval.search_all_sq8_stream, ms per call, recall@k against search_all's, the share of complete queries, mean and max
      n_survivors.
One process, every shape warmed, A and S alternating inside a round, device events around work that ends in a synchronise; median
of the rounds, min..max beside it.  The code table is made outside the timed region.
Kernel times come from a run of their own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kt -- python tools/sq8_stream_rate.py --trace
  python tools/sq8_stream_rate.py --stats DIR/.../kt_kernel_stats.csv      # appends the kernel times to the output file
--trace runs TRACE_CALLS calls of both at 128 queries, 1M rows, L2, fetch = 400: ONE chunk of both.
usage: tools/sq8_stream_rate.py [--sizes N,N] [--dim D] [--rounds R] [--out FILE] [--trace | --stats CSV]
writes profiles/sq8_stream_rate.txt (or FILE) and prints the same."""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, CAP = 200, 8192
BATCHES = (64, 1024)
FETCH = (K, 2 * K)
TRACE_CALLS, TRACE_QUERIES, TRACE_FETCH = 5, 128, 2 * K
KERNELS = ("k_sq8_stream_count", "k_sq8_stream_fill", "k_sq8_stream_lists", "k_range_scan", "k_scan_sq8", "k_scan_slab_topk",
           "k_scan_merge", "k_sq8_encode", "k_sq8_sort_rows", "k_cand_plan", "k_cand_score_l2", "k_cand_topk")


def kernel_times(path):
    """kernel_stats.csv of the --trace run -> lines: calls, average and total time of the kernels of both calls"""
    rows = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            for k in KERNELS:
                if k in name:
                    calls, ns = rows.get(k, (0, 0.0))
                    rows[k] = (calls + int(row.get("Calls") or 0), ns + float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0))
    assert "k_sq8_stream_count" in rows and "k_sq8_stream_fill" in rows, f"{path}: no row for the streamed kernels"
    lines = [f"kernel times (rocprofv3 --kernel-trace --stats; {TRACE_CALLS} + 1 calls of search_all_sq8 and of search_all_sq8_stream at "
             f"{TRACE_QUERIES} queries = one chunk each, 1M rows, L2, fetch = {TRACE_FETCH}, k = {K}; the shared kernels run in both calls -- "
             "k_scan_sq8, the slab top-k and the merge over the whole table in the first, over the sample in the second):"]
    for k in KERNELS:
        if k in rows:
            calls, ns = rows[k]
            lines.append(f"  {k:20s} {calls:4d} launches, {ns / max(calls, 1) / 1e3:10.1f} us each, {ns / 1e6:9.3f} ms in all")
    new = rows["k_sq8_stream_count"][1] + rows["k_sq8_stream_fill"][1]
    lines.append(f"  k_sq8_stream_count + k_sq8_stream_fill = {new / sum(v[1] for v in rows.values()):.3f} of the listed kernels' time")
    return lines


def make_index(n, d):
    import numpy as np
    from nann_amd import retrieval, synth
    embs, assign = synth.make_corpus(n, d, n_clusters=max(64, n // 4096), noise=1.0)
    deg = 8  # no call here reads the graph: a ring is a valid one
    nbv = ((np.arange(n, dtype=np.int64)[:, None] + 1 + np.arange(deg)) % n).astype(np.int32).reshape(-1)
    rs = np.arange(n + 1, dtype=np.int64) * deg
    index = retrieval.Index(embs, synth.make_item_ids(n), [nbv, nbv], [rs, rs], np.arange(0, n, n // 64, dtype=np.int32)[:64])
    return index, embs, assign


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,4000000")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sq8_stream_rate.txt"))
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
    d = args.dim

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    if args.trace:
        index, embs, assign = make_index(1_000_000, d)
        sq8, sc = retrieval.make_sq8(index), ops.Scorer("l2", d, torch.float16)
        q = ops.user_seq_mean(torch.as_tensor(synth.make_queries(embs, assign, TRACE_QUERIES, seed=99)).to(dev))
        for _ in range(TRACE_CALLS + 1):
            retrieval.search_all_sq8(index, sq8, sc, q, K, fetch=TRACE_FETCH)
            retrieval.search_all_sq8_stream(index, sq8, sc, q, K, fetch=TRACE_FETCH, cap=CAP, fallback=False)
        torch.cuda.synchronize()
        print(f"trace run: {TRACE_CALLS} + 1 calls of search_all_sq8 and of search_all_sq8_stream(fetch = {TRACE_FETCH}) at {TRACE_QUERIES} queries")
        return

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def fmt(ms):
        return f"{statistics.median(ms):9.3f} ms ({min(ms):.3f}..{max(ms):.3f})"

    def recall(got, ref):
        return float(np.mean([len(np.intersect1d(got[i], ref[i])) / K for i in range(len(ref))]))

    emit(f"sq8_stream_rate: x {d} f16, k = {K}, cap = {CAP}, default sample, fallback off, rounds = {args.rounds} (median, min..max); "
         f"device {torch.cuda.get_device_name(0)}")
    for n in (int(s) for s in args.sizes.split(",")):
        index, embs, assign = make_index(n, d)
        sq8 = retrieval.make_sq8(index)
        q_all = ops.user_seq_mean(torch.as_tensor(synth.make_queries(embs, assign, max(BATCHES), seed=99)).to(dev))
        for metric in ("l2", "ip"):
            sc = ops.Scorer(metric, d, torch.float16)
            for b in BATCHES:
                q = q_all[:b]
                ref = retrieval.search_all(index, sc, q, K).index.cpu().numpy()
                emit(f"{n} items, {metric}, batch {b}")
                for f_ in FETCH:
                    run_a = lambda: retrieval.search_all_sq8(index, sq8, sc, q, K, fetch=f_)  # noqa: E731
                    run_s = lambda: retrieval.search_all_sq8_stream(index, sq8, sc, q, K, fetch=f_, cap=CAP, fallback=False, return_stats=True)  # noqa: E731
                    ra, rs_ = run_a(), run_s()  # (the warming calls)
                    torch.cuda.synchronize()
                    surv, done = rs_.n_survivors.cpu().numpy(), rs_.complete.cpu().numpy()
                    rec_a, rec_s = recall(ra.index.cpu().numpy(), ref), recall(rs_.index.cpu().numpy(), ref)
                    ta, ts = [], []
                    for _ in range(args.rounds):
                        ta.append(timed(run_a))
                        ts.append(timed(run_s))
                    ma, ms = statistics.median(ta), statistics.median(ts)
                    emit(f"  fetch = {f_:4d}  A search_all_sq8:        {fmt(ta)}   recall@{K} = {rec_a:.4f}")
                    emit(f"                S search_all_sq8_stream: {fmt(ts)}   recall@{K} = {rec_s:.4f}   A / S = {ma / ms:.2f}   complete "
                         f"{done.mean():.4f}   n_survivors mean {surv.mean():.0f} max {surv.max()}")
        del index, sq8
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
