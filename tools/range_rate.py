#!/usr/bin/env python3
"""Range search (retrieval.search_all_range: every row scoring at or above a per-query cut) at a size a user runs: 1M x 128 f16
under L2, a batch of 256 queries, cuts chosen so that about 10, 200, 1 000 and 10 000 rows match per query.  The cuts for 10, 200
and 1 000 are retrieval.search_all's own k-th scores (k is capped at 1024 there); the one for 10 000 is the 10 000th of
ops.blaze_score + torch.topk per query, which carries the same bits.  Reported, ms per query:
  R   the range call at a capacity that holds the whole answer (one filling call), and its count-only form (capacity 0);
  A   retrieval.search_all(k = 200) on the same index and queries;
  C   the per-query loop ops.blaze_score + torch.nonzero(score >= cut), over 32 of the queries.
One process, every shape warmed, the calls alternating inside a round, device events around work that ends in a synchronise;
median of the rounds, min..max beside it.  These are whole-call figures.  The selection stage's share of a call comes from kernel
times, in a run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kt -- python tools/range_rate.py --trace
  python tools/range_rate.py --stats DIR/.../kt_kernel_stats.csv      # appends the shares to the output file
--trace runs the range call (about 200 matches per query) and search_all(k = 200) the same number of times and nothing else that
launches their kernels (its cuts come from the blaze_score loop), so the two calls' kernel totals can be set side by side.
usage: tools/range_rate.py [items] [dim] [--rounds R] [--out FILE] [--trace | --stats CSV]
writes profiles/range_rate.txt (or FILE) and prints the same."""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH, K, LOOP = 256, 200, 32
TARGETS = (10, 200, 1000, 10000)
TRACE_CALLS = 3
RANGE_KERNELS = ("k_range_count", "k_range_scan", "k_range_splits", "k_range_fill")
TOPK_KERNELS = ("k_scan_slab_topk", "k_scan_merge")
SHARED_KERNELS = ("k_scan_l2", "k_scan_transpose_q")


def kernel_shares(path):
    """kernel_stats.csv of the --trace run -> lines: the selection stage's share of the range call and of search_all"""
    total = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0)
            for k in RANGE_KERNELS + TOPK_KERNELS + SHARED_KERNELS:
                if k in name:
                    total[k] = total.get(k, 0.0) + ns
    missing = [k for k in RANGE_KERNELS + TOPK_KERNELS + ("k_scan_l2",) if k not in total]
    assert not missing, f"{path}: no row for {missing}"
    shared = sum(total.get(k, 0.0) for k in SHARED_KERNELS) / 2  # both calls ran the scan the same number of times
    sel_range = sum(total[k] for k in RANGE_KERNELS)
    sel_topk = sum(total[k] for k in TOPK_KERNELS)
    out =[f"kernel times (rocprofv3 --kernel-trace --stats, {TRACE_CALLS} calls of each form, batch {BATCH}, about {K} matches per query / k = {K}):"]
    for k in SHARED_KERNELS + RANGE_KERNELS + TOPK_KERNELS:
        if k in total:
            out.append(f"  {k:20s} {total[k] / 1e6:10.3f} ms in all")
    out.append(f"  range call:  selection (count + scan + splits + fill) {sel_range / TRACE_CALLS / 1e6:.3f} ms of "
               f"{(sel_range + shared) / TRACE_CALLS / 1e6:.3f} ms kernel time per call = {100 * sel_range / (sel_range + shared):.1f} %")
    out.append(f"  search_all:  selection (slab top-k + merge)           {sel_topk / TRACE_CALLS / 1e6:.3f} ms of "
               f"{(sel_topk + shared) / TRACE_CALLS / 1e6:.3f} ms kernel time per call = {100 * sel_topk / (sel_topk + shared):.1f} %")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("items", nargs="?", type=int, default=1_000_000)
    ap.add_argument("dim", nargs="?", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_rate.txt"))
    ap.add_argument("--trace", action="store_true", help="a short run for a kernel trace")
    ap.add_argument("--stats", help="kernel_stats.csv of a --trace run: append the selection stages' shares to the output file")
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
    embs, assign = synth.make_corpus(n, d, n_clusters=max(64, n // 4096), noise=1.0)
    # the scan never reads the graph: a ring (every node linked to the next eight) is a valid one
    deg = 8
    nbv = ((np.arange(n, dtype=np.int64)[:, None] + 1 + np.arange(deg)) % n).astype(np.int32).reshape(-1)
    rs = np.arange(n + 1, dtype=np.int64) * deg
    index = retrieval.Index(embs, synth.make_item_ids(n), [nbv, nbv], [rs, rs], np.arange(0, n, max(n // 64, 1), dtype=np.int32)[:64])
    sc = ops.Scorer("l2", d, torch.float16)
    rng = np.random.default_rng(99)
    # queries near rows of the corpus: the question a range search is asked (near-duplicates, a recall set)
    q = embs[rng.integers(0, n, BATCH)].astype(np.float32) + 0.3 * rng.standard_normal((BATCH, d)).astype(np.float32)
    q = torch.as_tensor(q).to(dev)

    def kth_by_loop(k):
        return torch.stack([torch.topk(ops.blaze_score(sc, q[b], item_emb=index.item_embs), k).values[-1] for b in range(BATCH)])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    if args.trace:
        thr = kth_by_loop(K).contiguous()
        total = retrieval.search_all_range(index, sc, q, thr, capacity=0).total
        for _ in range(TRACE_CALLS):
            retrieval.search_all_range(index, sc, q, thr, capacity=total)
            retrieval.search_all(index, sc, q, K)
        torch.cuda.synchronize()
        print(f"trace run: {TRACE_CALLS} calls of each form, batch {BATCH}, {total} matches in all")
        return

    lines = [f"range_rate: {n} items x {d} f16, L2, batch {BATCH}, rounds = {args.rounds} (median, min..max); device "
             f"{torch.cuda.get_device_name(0)}"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def fmt(ms, per):
        return f"{statistics.median(ms):9.3f} ms ({min(ms):.3f}..{max(ms):.3f}) = {statistics.median(ms) / per:.5f} ms per query"

    top = retrieval.search_all(index, sc, q, 1024).scores
    cuts = {t: (top[:, t - 1].contiguous() if t <= 1024 else kth_by_loop(t).contiguous()) for t in TARGETS}
    totals = {t: retrieval.search_all_range(index, sc, q, cuts[t], capacity=0).total for t in TARGETS}

    def loop_c(thr):
        for b in range(LOOP):
            torch.nonzero(ops.blaze_score(sc, q[b], item_emb=index.item_embs) >= thr[b])

    pairs = [("A", lambda: retrieval.search_all(index, sc, q, K))]
    for t in TARGETS:
        pairs.append((f"R{t}", lambda t=t: retrieval.search_all_range(index, sc, q, cuts[t], capacity=totals[t])))
        pairs.append((f"N{t}", lambda t=t: retrieval.search_all_range(index, sc, q, cuts[t], capacity=0)))
        pairs.append((f"C{t}", lambda t=t: loop_c(cuts[t])))
    for _, fn in pairs:  # warm every shape
        fn()
    torch.cuda.synchronize()
    res = {name: [] for name, _ in pairs}
    for _ in range(args.rounds):
        for name, fn in pairs:
            res[name].append(timed(fn))
    emit(f"  A  search_all(k = {K}):                         {fmt(res['A'], BATCH)}")
    for t in TARGETS:
        emit(f"about {t} matches per query ({totals[t]} in all, {totals[t] / BATCH:.1f} per query)")
        emit(f"  R  search_all_range, one filling call:         {fmt(res[f'R{t}'], BATCH)}"
             f" = {statistics.median(res[f'R{t}']) / statistics.median(res['A']):.2f} x A's time")
        emit(f"  R  search_all_range, count only (capacity 0):  {fmt(res[f'N{t}'], BATCH)}")
        c_per = statistics.median(res[f"C{t}"]) / LOOP
        emit(f"  C  blaze_score + nonzero loop, {LOOP} queries:     {fmt(res[f'C{t}'], LOOP)}"
             f" = {c_per / (statistics.median(res[f'R{t}']) / BATCH):.1f} x R's time per query")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
