#!/usr/bin/env python3
"""Certified scalar-quantised exhaustive search (retrieval.search_all_sq8_exact: the int8 scan, a survivor pass under a rigorous
error bound, an exact re-rank of the survivors -- search_all's bits) next to retrieval.search_all and retrieval.search_all_sq8
at a size a user runs: 1M x 128 f16 from synth, L2 and the inner product, k = 200, batches of 64 and 1 024 queries.  Reported
per metric and batch:
  A        retrieval.search_all, ms per call -- the yardstick;
  B<F>     retrieval.search_all_sq8(fetch = F) for F = k and 2k, ms per call and recall@k against A;
  C        retrieval.search_all_sq8_exact(fetch = k, cap = 2048, fallback=False), ms per call; the share of queries certified,
           the mean and the largest n_survivors, and whether index, scores and item ids equal A's bit for bit.
One process, every shape warmed, the calls alternating inside a round, device events around work that ends in a synchronise;
median of the rounds, min..max beside it.  Table and bounds are made outside the timed region (their time is printed once).
No ratio is a pass mark: if C is not faster than A the output says so.
Kernel times come from a run of their own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kt -- python tools/sq8_exact_rate.py --trace
  python tools/sq8_exact_rate.py --stats DIR/.../kt_kernel_stats.csv      # appends the kernel times to the output file
--trace runs TRACE_CALLS calls of search_all and of search_all_sq8_exact at 128 queries, L2 -- ONE chunk of both.
usage: tools/sq8_exact_rate.py [items] [dim] [--rounds R] [--out FILE] [--trace | --stats CSV]
writes profiles/sq8_exact_rate.txt (or FILE) and prints the same."""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 200
CAP = 2048
BATCHES = (64, 1024)
FETCH = (K, 2 * K)
TRACE_CALLS, TRACE_QUERIES = 5, 128
KERNELS = ("k_scan_sq8", "k_scan_l2", "k_scan_slab_topk", "k_scan_merge", "k_sq8_encode", "k_sq8_sort_rows", "k_sq8_row_err",
           "k_sq8_exact_terms", "k_sq8_surv_count", "k_range_scan", "k_sq8_exact_lists", "k_sq8_surv_fill", "k_cand_plan",
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
    assert "k_sq8_surv_count" in rows and "k_scan_l2" in rows, f"{path}: no row for k_sq8_surv_count or k_scan_l2"
    lines = [f"kernel times (rocprofv3 --kernel-trace --stats; {TRACE_CALLS} calls of search_all and of search_all_sq8_exact(fetch = {K}, "
             f"cap = {CAP}) at {TRACE_QUERIES} queries = one chunk each, L2, k = {K}, after one warming call of each; the slab top-k and "
             "the merge run in both calls, the candidate-list kernels twice per certified call; k_sq8_encode and k_sq8_row_err include "
             "the launches that made the table and the bounds):"]
    for k in KERNELS:
        if k in rows:
            calls, ns = rows[k]
            lines.append(f"  {k:20s} {calls:4d} launches, {ns / max(calls, 1) / 1e3:10.1f} us each, {ns / 1e6:9.3f} ms in all")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("items", nargs="?", type=int, default=1_000_000)
    ap.add_argument("dim", nargs="?", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sq8_exact_rate.txt"))
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
    # no call here reads the graph: a ring (every node linked to the next eight) is a valid one
    deg = 8
    nbv = ((np.arange(n, dtype=np.int64)[:, None] + 1 + np.arange(deg)) % n).astype(np.int32).reshape(-1)
    rs = np.arange(n + 1, dtype=np.int64) * deg
    index = retrieval.Index(embs, synth.make_item_ids(n), [nbv, nbv], [rs, rs], np.arange(0, n, n // 64, dtype=np.int32)[:64])
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
    t_bounds = timed(lambda: holder.setdefault("b", retrieval.make_sq8_bounds(index, sq8)))
    bounds = holder["b"]

    def exact(sc, q):
        return retrieval.search_all_sq8_exact(index, sq8, bounds, sc, q, K, fetch=K, cap=CAP, fallback=False)

    if args.trace:
        sc = ops.Scorer("l2", d, torch.float16)
        q = q_all[:TRACE_QUERIES]
        for _ in range(TRACE_CALLS + 1):
            retrieval.search_all(index, sc, q, K)
            exact(sc, q)
        torch.cuda.synchronize()
        print(f"trace run: {TRACE_CALLS} + 1 calls of search_all and of search_all_sq8_exact(fetch = {K}) at {TRACE_QUERIES} queries")
        return

    lines = [f"sq8_exact_rate: {n} items x {d} f16, k = {K}, cap = {CAP}, rounds = {args.rounds} (median, min..max); device "
             f"{torch.cuda.get_device_name(0)}",
             f"code table: {sq8.nbytes / 1e6:.1f} MB, made in {t_table:.3f} ms; bounds: {8 * n / 1e6:.1f} MB, made in {t_bounds:.3f} ms "
             f"(first launches included); rows: {embs.nbytes / 1e6:.1f} MB"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def fmt(ms):
        return f"{statistics.median(ms):9.3f} ms ({min(ms):.3f}..{max(ms):.3f})"

    for line in lines:
        print(line, flush=True)
    for metric in ("l2", "ip"):
        sc = ops.Scorer(metric, d, torch.float16)
        for b in BATCHES:
            q = q_all[:b]
            pairs = [("A", lambda: retrieval.search_all(index, sc, q, K))]
            for f_ in FETCH:
                pairs.append((f"B{f_}", lambda f_=f_: retrieval.search_all_sq8(index, sq8, sc, q, K, fetch=f_)))
            pairs.append(("C", lambda: exact(sc, q)))
            ref = retrieval.search_all(index, sc, q, K)
            ref_rows = ref.index.cpu().numpy()
            recall = {}
            for f_ in FETCH:
                got = retrieval.search_all_sq8(index, sq8, sc, q, K, fetch=f_).index.cpu().numpy()
                recall[f_] = float(np.mean([len(np.intersect1d(got[i], ref_rows[i])) / K for i in range(b)]))
            c = exact(sc, q)
            torch.cuda.synchronize()
            cert, surv = c.certified.cpu().numpy(), c.n_survivors.cpu().numpy()
            same = bool((c.index == ref.index).all() and (c.scores.view(torch.int32) == ref.scores.view(torch.int32)).all()
                        and (c.item_ids == ref.item_ids).all())
            for _, fn in pairs:  # warm every shape
                fn()
            torch.cuda.synchronize()
            res = {name: [] for name, _ in pairs}
            for _ in range(args.rounds):
                for name, fn in pairs:
                    res[name].append(timed(fn))
            a = statistics.median(res["A"])
            emit(f"{metric}, batch {b}")
            emit(f"  A  search_all:                           {fmt(res['A'])}")
            for f_ in FETCH:
                m = statistics.median(res[f"B{f_}"])
                emit(f"  B  search_all_sq8, fetch = {f_:4d}:          {fmt(res[f'B{f_}'])}   A / B = {a / m:.2f}   recall@{K} against A = {recall[f_]:.4f}")
            m = statistics.median(res["C"])
            emit(f"  C  search_all_sq8_exact, fetch = {K:4d}:    {fmt(res['C'])}   A / C = {a / m:.2f}   certified {cert.mean():.4f} of the queries, "
                 f"n_survivors mean {surv.mean():.1f} max {int(surv.max())}, bit-identical to A: {same}")
            emit(f"     C is {'FASTER' if m < a else 'NOT faster'} than A at this batch ({m / a:.2f} x A's time)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
