#!/usr/bin/env python3
"""IVF-SQ8: ms per call of retrieval.search_lists_sq8 over a trained coarse partition and the int8 code table, next to
search_lists at the same probes, search_candidates with every query's lists expanded into a row list of its own, and
search_all_sq8 over the whole table; and its recall@200 against search_lists at the same probes.  1M x 128 f16 rows (a clustered
synthetic corpus), L2, k = 200, fetch = 200 and 400, 1 024 trained cells, 1 024 queries, n_probe 8 / 32 / 64.
One process, every shape warmed, the variants alternating inside a round, device events around REPS calls that end in a
synchronise; median of the rounds, min..max beside it.
The kernels' shares come from a trace of a short run:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kt -- python tools/lists_sq8_rate.py --trace
  tools/lists_sq8_rate.py --stats DIR/.../kt_kernel_stats.csv        (appends them to the output file)
usage: tools/lists_sq8_rate.py [items] [dim] [--rounds R] [--out FILE] [--trace | --stats CSV]
writes profiles/lists_sq8_rate.txt (or FILE) and prints the same."""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, FETCHES, CELLS, REPS, BATCH, PROBES = 200, (200, 400), 1024, 3, 1024, (8, 32, 64)
TRACE_CALLS, TRACE_PROBE, TRACE_FETCH = 5, 32, 400
# the kernels of a call, in launch order (k_lists_scan_sq8 is the new scan; the names are matched as substrings)
KERNELS = ("k_lists_plan", "k_sq8_encode", "k_lists_scan_sq8", "k_lists_pad", "k_scan_slab_topk", "k_lists_fetch_sq8", "k_cand_plan",
           "k_cand_score_l2", "k_lists_finish_sq8")


def kernel_shares(path):
    """kernel_stats.csv of the --trace run -> lines: every kernel of the call and its share of the call's kernel time"""
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
    out = [f"kernel times (rocprofv3 --kernel-trace --stats, {TRACE_CALLS} calls of search_lists_sq8, batch {BATCH}, n_probe = "
           f"{TRACE_PROBE}, fetch = {TRACE_FETCH}, k = {K}):"]
    for k in KERNELS:
        out.append(f"  {k:18s} {total[k] / TRACE_CALLS / 1e6:10.3f} ms per call = {100 * total[k] / whole:5.1f} % of its kernel time")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("items", nargs="?", type=int, default=1_000_000)
    ap.add_argument("dim", nargs="?", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lists_sq8_rate.txt"))
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
    t = retrieval.make_sq8(index)
    rng = np.random.default_rng(99)
    q = embs[rng.integers(0, n, BATCH)].astype(np.float32) + 0.3 * rng.standard_normal((BATCH, d)).astype(np.float32)
    q = torch.as_tensor(q).to(dev)
    b = BATCH

    def probes_of(n_probe):
        sim = 2.0 * q @ cent.T - (cent * cent).sum(1)[None, :]
        return sim.topk(min(n_probe, cells), dim=1).indices.to(torch.int32).contiguous()

    if args.trace:
        pr = probes_of(TRACE_PROBE)
        for _ in range(TRACE_CALLS):
            retrieval.search_lists_sq8(index, part, t, sc, q, pr, K, fetch=TRACE_FETCH)
        torch.cuda.synchronize()
        print(f"trace run: {TRACE_CALLS} calls of search_lists_sq8, batch {b}, n_probe = {TRACE_PROBE}, fetch = {TRACE_FETCH}, k = {K}")
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

    lines = [f"lists_sq8_rate: {n} items x {d} f16, L2, k = {K}, {cells} trained cells (longest {part.max_len} rows), {b} queries, rounds = "
             f"{args.rounds} x {REPS} calls (median, min..max); device {torch.cuda.get_device_name(0)}"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    splits, rows = part.list_splits(), part.list_rows()
    lens = splits[1:] - splits[:-1]
    all_ms = None
    for n_probe in PROBES:
        pr = probes_of(n_probe)
        # every query's lists expanded into a row list of its own: what a caller had to build without the calls
        pl = pr.long()
        qlen = lens[pl]                                              # [b, n_probe]
        cs = torch.zeros(b + 1, dtype=torch.int64, device=dev)
        cs[1:] = qlen.sum(1).cumsum(0)
        seg = torch.repeat_interleave(torch.arange(b * n_probe, device=dev), qlen.reshape(-1))
        seg_start = torch.cumsum(qlen.reshape(-1), 0) - qlen.reshape(-1)
        flat = rows[(splits[pl].reshape(-1)[seg] + torch.arange(seg.numel(), device=dev) - seg_start[seg])].contiguous()
        pairs = [(f"sq8 fetch {f}", (lambda f=f: retrieval.search_lists_sq8(index, part, t, sc, q, pr, K, fetch=f))) for f in FETCHES]
        pairs += [("lists", lambda: retrieval.search_lists(index, part, sc, q, pr, K)),
                  ("cand", lambda: retrieval.search_candidates(index, sc, q, candidates=(cs, flat), k=K)),
                  ("all_sq8", lambda: retrieval.search_all_sq8(index, t, sc, q, K, fetch=FETCHES[-1]))]
        for _, fn in pairs:  # warm every shape
            fn()
        torch.cuda.synchronize()
        res = {name: [] for name, _ in pairs}
        for _ in range(args.rounds):
            for name, fn in pairs:
                if name == "all_sq8" and all_ms is not None:
                    continue
                res[name].append(timed(fn))
        all_ms = all_ms or res["all_sq8"]
        ref = retrieval.search_lists(index, part, sc, q, pr, K)
        lists = statistics.median(res["lists"])
        emit(f"n_probe = {n_probe}: {int(cs[-1]) / b:.0f} rows per query")
        emit(f"  search_lists:                        {fmt(res['lists'])}")
        for f in FETCHES:
            got = retrieval.search_lists_sq8(index, part, t, sc, q, pr, K, fetch=f)
            torch.cuda.synchronize()
            valid = torch.arange(K, device=dev)[None, :]
            hit = (got.pos[:, :, None] == ref.pos[:, None, :]) & (valid < got.n_out[:, None])[:, :, None] & (valid < ref.n_out[:, None])[:, None, :]
            recall = float(hit.any(2).sum()) / max(int(ref.n_out.sum()), 1)
            ms = res[f"sq8 fetch {f}"]
            emit(f"  search_lists_sq8, fetch = {f}:         {fmt(ms)} = {lists / statistics.median(ms):.2f} x search_lists' rate, "
                 f"recall@{K} vs search_lists = {recall:.4f}")
        emit(f"  search_candidates on the expansion:  {fmt(res['cand'])} = {lists / statistics.median(res['cand']):.2f} x")
        emit(f"  search_all_sq8, fetch = {FETCHES[-1]}:         {fmt(all_ms)} = {lists / statistics.median(all_ms):.2f} x")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
