#!/usr/bin/env python3
"""The wide exhaustive search (retrieval.search_all_wide: the exact top k for k up to 16 384) at a size a user runs: 1M x 128 f16
under L2, batches of 256 and 1 024 queries, k = 200, 1 024, 2 048, 4 096 and 16 384.  Reported, ms per call:
  W   retrieval.search_all_wide(k);
  A   retrieval.search_all(k), at the two k where both exist (200 and 1 024);
  R   at the wide k, the way round that existed before: retrieval.search_all_range at a guessed threshold -- the query's k-th
      score, which a caller does not know, moved 2 % further out so that no guess comes up short -- at a capacity that holds the
      answer, then a torch sort of every segment (sort=True);
  C   at the wide k, the per-query loop ops.blaze_score + torch.topk, over 32 of the queries, scaled to the batch.
One process, every shape warmed, the calls alternating inside a round, device events around work that ends in a synchronise;
median of the rounds, min..max beside it.  These are whole-call figures.  The selection stages' share of a call comes from kernel
times, in a run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kt -- python tools/wide_rate.py --trace
  python tools/wide_rate.py --stats DIR/.../kt_kernel_stats.csv      # appends the shares to the output file
--trace runs search_all_wide(k = 1 024) and search_all(k = 1 024) on 256 queries the same number of times and nothing else that
launches their kernels, so the two calls' kernel totals can be set side by side.
usage: tools/wide_rate.py [items] [dim] [--rounds R] [--out FILE] [--trace | --stats CSV]
writes profiles/wide_rate.txt (or FILE) and prints the same."""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCHES = (256, 1024)
KS = (200, 1024, 2048, 4096, 16384)
BOTH = (200, 1024)   # the k at which search_all exists as well
LOOP = 32
TRACE_CALLS, TRACE_K, TRACE_BATCH = 3, 1024, 256
CUT_KERNELS = ("k_wide_hist", "k_wide_pick")
GATHER_KERNELS = ("k_wide_count", "k_range_scan", "k_wide_fill")
SORT_KERNELS = ("k_wide_sort",)
TOPK_KERNELS = ("k_scan_slab_topk", "k_scan_merge")
SHARED_KERNELS = ("k_scan_l2", "k_scan_transpose_q")


def kernel_shares(path):
    """kernel_stats.csv of the --trace run -> lines: the three stages' share of the wide call, the selection's of search_all"""
    total = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0)
            for k in CUT_KERNELS + GATHER_KERNELS + SORT_KERNELS + TOPK_KERNELS + SHARED_KERNELS:
                if k in name:
                    total[k] = total.get(k, 0.0) + ns
    missing = [k for k in CUT_KERNELS + GATHER_KERNELS + SORT_KERNELS + TOPK_KERNELS + ("k_scan_l2",) if k not in total]
    assert not missing, f"{path}: no row for {missing}"
    shared = sum(total.get(k, 0.0) for k in SHARED_KERNELS) / 2  # both calls ran the scan the same number of times
    stage = {"cut (3 x hist + pick)": sum(total[k] for k in CUT_KERNELS),
             "gather (count + scan + fill)": sum(total[k] for k in GATHER_KERNELS),
             "sort": sum(total[k] for k in SORT_KERNELS)}
    sel_wide = sum(stage.values())
    sel_topk = sum(total[k] for k in TOPK_KERNELS)
    out = [f"kernel times (rocprofv3 --kernel-trace --stats, {TRACE_CALLS} calls of each form, batch {TRACE_BATCH}, k = {TRACE_K}):"]
    for k in SHARED_KERNELS + CUT_KERNELS + GATHER_KERNELS + SORT_KERNELS + TOPK_KERNELS:
        if k in total:
            out.append(f"  {k:20s} {total[k] / 1e6:10.3f} ms in all")
    for name, ns in stage.items():
        out.append(f"  search_all_wide: {name:30s} {ns / TRACE_CALLS / 1e6:.3f} ms per call = "
                   f"{100 * ns / (sel_wide + shared):.1f} % of its kernel time")
    out.append(f"  search_all_wide: selection in all {sel_wide / TRACE_CALLS / 1e6:.3f} ms of "
               f"{(sel_wide + shared) / TRACE_CALLS / 1e6:.3f} ms kernel time per call = {100 * sel_wide / (sel_wide + shared):.1f} %")
    out.append(f"  search_all:      selection (slab top-k + merge) {sel_topk / TRACE_CALLS / 1e6:.3f} ms of "
               f"{(sel_topk + shared) / TRACE_CALLS / 1e6:.3f} ms kernel time per call = {100 * sel_topk / (sel_topk + shared):.1f} %")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("items", nargs="?", type=int, default=1_000_000)
    ap.add_argument("dim", nargs="?", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_rate.txt"))
    ap.add_argument("--trace", action="store_true", help="a short run for a kernel trace")
    ap.add_argument("--stats", help="kernel_stats.csv of a --trace run: append the stages' shares to the output file")
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
    qa = embs[rng.integers(0, n, max(BATCHES))].astype(np.float32) + 0.3 * rng.standard_normal((max(BATCHES), d)).astype(np.float32)
    qa = torch.as_tensor(qa).to(dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    if args.trace:
        q = qa[:TRACE_BATCH]
        for _ in range(TRACE_CALLS):
            retrieval.search_all_wide(index, sc, q, TRACE_K)
            retrieval.search_all(index, sc, q, TRACE_K)
        torch.cuda.synchronize()
        print(f"trace run: {TRACE_CALLS} calls of each form, batch {TRACE_BATCH}, k = {TRACE_K}")
        return

    lines = [f"wide_rate: {n} items x {d} f16, L2, rounds = {args.rounds} (median, min..max), ms per call; device "
             f"{torch.cuda.get_device_name(0)}"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def fmt(ms):
        return f"{statistics.median(ms):9.3f} ms ({min(ms):.3f}..{max(ms):.3f})"

    for batch in BATCHES:
        q = qa[:batch].contiguous()
        wide_k = [k for k in KS if k not in BOTH and k <= n]
        # the guessed thresholds of R: the k-th score moved 2 % further out (L2 scores are negative: times 1.02)
        guess, room = {}, {}
        for k in wide_k:
            guess[k] = (retrieval.search_all_wide(index, sc, q, k).scores[:, k - 1] * 1.02).contiguous()
            room[k] = retrieval.search_all_range(index, sc, q, guess[k], capacity=0).total

        def loop_c(k):
            for b in range(LOOP):
                torch.topk(ops.blaze_score(sc, q[b], item_emb=index.item_embs), k)

        pairs = []
        for k in KS:
            if k > n:
                continue
            pairs.append((f"W{k}", lambda k=k: retrieval.search_all_wide(index, sc, q, k)))
            if k in BOTH:
                pairs.append((f"A{k}", lambda k=k: retrieval.search_all(index, sc, q, k)))
            else:
                pairs.append((f"R{k}", lambda k=k: retrieval.search_all_range(index, sc, q, guess[k], capacity=room[k], sort=True)))
                pairs.append((f"C{k}", lambda k=k: loop_c(k)))
        for _, fn in pairs:  # warm every shape
            fn()
        torch.cuda.synchronize()
        res = {name: [] for name, _ in pairs}
        for _ in range(args.rounds):
            for name, fn in pairs:
                res[name].append(timed(fn))
        emit(f"batch {batch}")
        for k in KS:
            if k > n:
                continue
            w = statistics.median(res[f"W{k}"])
            emit(f"  k = {k}")
            emit(f"    W  search_all_wide:                          {fmt(res[f'W{k}'])}")
            if k in BOTH:
                a = statistics.median(res[f"A{k}"])
                emit(f"    A  search_all:                               {fmt(res[f'A{k}'])} = {a / w:.2f} x W's time")
            else:
                r = statistics.median(res[f"R{k}"])
                c = statistics.median(res[f"C{k}"]) * batch / LOOP
                emit(f"    R  search_all_range at a guess + torch sort:  {fmt(res[f'R{k}'])} = {r / w:.2f} x W's time"
                     f" ({room[k] / batch:.0f} matches per query)")
                emit(f"    C  blaze_score + torch.topk loop, {LOOP} queries: {fmt(res[f'C{k}'])}, scaled to the batch "
                     f"{c:.1f} ms = {c / w:.1f} x W's time")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
