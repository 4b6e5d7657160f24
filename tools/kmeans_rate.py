#!/usr/bin/env python3
"""The coarse quantiser on the device: seconds per retrieval.train_partition(method="device") next to method="torch" (the
baseline: blocked f32 GEMMs, argmin, index_add_), same seeds, 10 rounds, 1M x 128 f16 rows (a clustered synthetic corpus), 1 024 and
4 096 cells; and recall@200 of search_partitioned at n_probe 8 and 32 over either partition against search_all, beside the
spread of the torch path over its own seeds.
One process, both methods warmed, alternating inside a round, a host clock around REPS calls that end in one synchronise; median
of the rounds, min..max beside it.  A call is all of train_partition on either side: the seeds, the rounds, make_partition with
its one read-back, and the allocation of the outputs and the workspace.
The kernels' times come from a trace of a short run:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kt -- python tools/kmeans_rate.py --trace [--cells C]
  tools/kmeans_rate.py --stats DIR/.../kt_kernel_stats.csv [--cells C]   (appends them, with the assign kernel's two floors, to the output file)
usage: tools/kmeans_rate.py [items] [dim] [--rounds R] [--out FILE] [--trace | --stats CSV] [--cells C]
writes profiles/kmeans_rate.txt (or FILE) and prints the same."""
import argparse
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, CELLS, ITERS, REPS, BATCH, PROBES, SEEDS = 200, (1024, 4096), 10, 8, 1024, (8, 32), (0, 1, 2)
HBM_BYTES_PER_S, F16_FLOPS = 8.0e12, 2.5e15  # the table values of the MI355X
# the kernels of a training call (matched as substrings; the three k_lists_* are the CSR build of nann_partition_create)
KERNELS = ("k_kmeans_prepare", "k_kmeans_assign", "k_kmeans_inertia", "k_kmeans_clear", "k_lists_count", "k_lists_group_prefix",
           "k_lists_splits", "k_lists_fill", "k_kmeans_seg_splits", "k_kmeans_partial", "k_kmeans_mean")
CSR = ("k_kmeans_clear", "k_lists_count", "k_lists_group_prefix", "k_lists_splits", "k_lists_fill")
UPDATE = ("k_kmeans_seg_splits", "k_kmeans_partial", "k_kmeans_mean")


def kernel_shares(path, n, d, cells):
    """kernel_stats.csv of the --trace run (one training call of ITERS rounds = ITERS + 1 assigns) -> lines"""
    total = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0)
            for k in KERNELS:
                if k in name:
                    total[k] = total.get(k, 0.0) + ns
    missing = [k for k in KERNELS if k not in total]
    assert not missing, f"{path}: no row for {missing}"
    whole = sum(total.values())
    assign_ms = total["k_kmeans_assign"] / (ITERS + 1) / 1e6
    read_ms = n * d * 2 / HBM_BYTES_PER_S * 1e3
    mfma_ms = 2 * 2.0 * n * cells * d / F16_FLOPS * 1e3
    out = [f"kernel times (rocprofv3 --kernel-trace --stats, one nann_kmeans_train of {ITERS} rounds, {n} x {d} f16, {cells} cells):"]
    for k in KERNELS:
        out.append(f"  {k:22s} {total[k] / 1e6:10.3f} ms = {100 * total[k] / whole:5.1f} % of the call's kernel time")
    out.append(f"k_kmeans_assign: {assign_ms:.3f} ms per round; floor 1, one read of the rows ({n * d * 2 / 1e6:.0f} MB at 8 TB/s): {read_ms:.3f} ms; "
               f"floor 2, the split MFMA work (2 terms x 2 n n_lists d flops at 2.5 PFLOP/s): {mfma_ms:.3f} ms; "
               f"the {'MFMA' if mfma_ms > read_ms else 'read'} floor binds: {max(mfma_ms, read_ms) / assign_ms:.2f} of it reached")
    per_round = whole / ITERS
    out.append(f"of a round's kernel time: the CSR build {100 * sum(total[k] for k in CSR) / ITERS / per_round:.1f} %, "
               f"the update {100 * sum(total[k] for k in UPDATE) / ITERS / per_round:.1f} %")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("items", nargs="?", type=int, default=1_000_000)
    ap.add_argument("dim", nargs="?", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--cells", type=int, default=1024, help="the cells of the --trace run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_rate.txt"))
    ap.add_argument("--trace", action="store_true", help="a short run for a kernel trace")
    ap.add_argument("--stats", help="kernel_stats.csv of a --trace run: append the kernels' times to the output file")
    args = ap.parse_args()
    n, d = args.items, args.dim
    if args.stats:
        lines = kernel_shares(args.stats, n, d, min(args.cells, n))
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
    embs, _ = synth.make_corpus(n, d, n_clusters=max(64, n // 4096), noise=1.0)
    # the flat calls never read the graph: a ring (every node linked to the next eight) is a valid one
    deg = 8
    nbv = ((np.arange(n, dtype=np.int64)[:, None] + 1 + np.arange(deg)) % n).astype(np.int32).reshape(-1)
    rs = np.arange(n + 1, dtype=np.int64) * deg
    index = retrieval.Index(embs, synth.make_item_ids(n), [nbv, nbv], [rs, rs], np.arange(0, n, max(n // 64, 1), dtype=np.int32)[:64])

    def train(method, cells, seed=0, reps=1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = retrieval.train_partition(index, cells, iters=ITERS, seed=seed, method=method)
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) / reps

    if args.trace:
        train("device", min(args.cells, n))
        print(f"trace run: one train_partition(method='device'), {ITERS} rounds, {min(args.cells, n)} cells")
        return

    sc = ops.Scorer("l2", d, torch.float16)
    rng = np.random.default_rng(99)
    q = embs[rng.integers(0, n, BATCH)].astype(np.float32) + 0.3 * rng.standard_normal((BATCH, d)).astype(np.float32)
    q = torch.as_tensor(q).to(dev)
    truth = retrieval.search_all(index, sc, q, K).index

    def recall(part, cent, n_probe):
        got = retrieval.search_partitioned(index, part, cent, sc, q, K, n_probe)
        torch.cuda.synchronize()
        return float((got.index[:, :, None] == truth[:, None, :]).any(2).sum()) / truth.numel()

    def fmt(s):
        return f"{statistics.median(s):8.4f} s ({min(s):.4f}..{max(s):.4f})"

    lines = [f"kmeans_rate: {n} items x {d} f16, train_partition, {ITERS} rounds, seconds per call over {args.rounds} windows of {REPS} calls (median, "
             f"min..max; a call includes make_partition and every allocation); recall@{K} of search_partitioned vs search_all, {BATCH} queries; device {torch.cuda.get_device_name(0)}"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    for cells in CELLS:
        cells = min(cells, n)
        res = {"torch": [], "device": []}
        for m in res:  # warm both
            train(m, cells)
        for _ in range(args.rounds):
            for m in res:
                res[m].append(train(m, cells, reps=REPS)[1])
        emit(f"{cells} cells: method='torch' {fmt(res['torch'])}   method='device' {fmt(res['device'])} = "
             f"{statistics.median(res['torch']) / statistics.median(res['device']):.2f} x the torch path's rate")
        (dp, dc), _ = train("device", cells)
        by_seed = [train("torch", cells, seed)[0] for seed in SEEDS]
        for n_probe in PROBES:
            r_t = [recall(p, c, n_probe) for p, c in by_seed]
            r_d = recall(dp, dc, n_probe)
            emit(f"  n_probe = {n_probe}: recall torch, seeds {SEEDS}: {' '.join('%.4f' % r for r in r_t)} (spread {max(r_t) - min(r_t):.4f}); "
                 f"device, seed 0: {r_d:.4f} (device - torch at seed 0: {r_d - r_t[0]:+.4f}); longest list torch {by_seed[0][0].max_len}, device {dp.max_len}")
        del by_seed, dp, dc
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
