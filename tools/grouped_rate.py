#!/usr/bin/env python3
"""Group caps (retrieval.search_grouped: at most `cap` rows of one group among the k a query returns) at a size a user runs: 1M x
128 f16 under L2 on the shipped builder's graph, top-200 at the fetch widths F = 512 and 1 024 (level_topn = [F/4] * 5 + [F]: the
last stage ranks its whole pool), 256 and 1 024 queries, about 10 000 groups of uneven size (group = floor(10 000 u^2), u uniform:
the largest holds ~1 % of the rows, the smallest ~0.005 %), caps 1 and 3.  Reported per (queries, F, cap), ms per call:
  G   retrieval.search_grouped(k = 200): the traversal at F and the cap kernel, one call;
  F   retrieval.search(filter = None, k = 200) at the same F: the existing filtered call, the traversal and k_filter_compact --
      the same inner search on the same commit, so G - F is the cap stage against the plain compaction;
  T   retrieval.search at F followed by the cap in torch on the device: a gather of the groups, a stable sort by group, a
      cummax for each run's start, a scatter of the ranks back, a cumsum for the places, four scatters.
and, at 256 queries, the exhaustive pair A = search_all_grouped(fetch = F) against B = search_all(filter = empty, k = F).  The mean
n_out and the share of queries with n_out < k at each (F, cap) stand beside them: what a host needs to choose F.
One process, every shape warmed, the calls alternating inside a round, device events around work that ends in a synchronise;
median of the rounds, min..max beside it.  The cap kernel's share of a call's kernel time comes from kernel times, in a run of
its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kt -- python tools/grouped_rate.py --trace
  python tools/grouped_rate.py --stats DIR/.../kt_kernel_stats.csv      # appends the share to the output file
usage: tools/grouped_rate.py [items] [dim] [--rounds R] [--out FILE] [--trace | --stats CSV]
writes profiles/grouped_rate.txt (or FILE) and prints the same."""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, EF_BUILD, N_GROUPS = 200, 128, 10_000
QUERIES = (256, 1024)
FETCH = (512, 1024)
CAPS = (1, 3)
TRACE_CALLS = 3
CAP_KERNEL = "k_group_cap"
SEARCH_KERNELS = ("k_search", "k_order_key", "k_order_perm")


def kernel_share(path):
    """kernel_stats.csv of the --trace run -> lines: the cap kernel's share of search_grouped's kernel time"""
    total = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0)
            for k in (CAP_KERNEL,) + SEARCH_KERNELS:
                if k in name:
                    total[k] = total.get(k, 0.0) + ns
    assert CAP_KERNEL in total and "k_search" in total, f"{path}: no row for the cap or the traversal kernel"
    cap, search = total[CAP_KERNEL], sum(total.get(k, 0.0) for k in SEARCH_KERNELS)
    calls = TRACE_CALLS * len(FETCH) * len(CAPS)
    return [f"kernel times (rocprofv3 --kernel-trace --stats, {TRACE_CALLS} calls at each of F {FETCH} x cap {CAPS}, {QUERIES[0]} queries, "
            f"k = {K}; the traversal's total includes the index's 64-query probe):",
            f"  {CAP_KERNEL:16s} {cap / 1e6:10.3f} ms in all = {cap / calls / 1e6:.4f} ms per call",
            f"  traversal        {search / 1e6:10.3f} ms in all = {search / calls / 1e6:.4f} ms per call",
            f"  the cap kernel is {100 * cap / (cap + search):.1f} % of search_grouped's kernel time"]


def torch_cap(torch, scores, rows, group_of_row, item_ids, cap, k):
    """the cap on the device in torch: scores / rows [B, F] of a search, ranked -> (item ids, scores, rows) [B, k], n_out [B]"""
    b, f = rows.shape
    g = group_of_row[rows.long()]
    by_group = torch.sort(g, dim=1, stable=True)                       # runs of equal groups, list order within a run
    ar = torch.arange(f, device=rows.device).expand(b, f)
    first = torch.ones_like(g, dtype=torch.bool)
    first[:, 1:] = by_group.values[:, 1:] != by_group.values[:, :-1]
    start = torch.cummax(torch.where(first, ar, torch.zeros_like(ar)), dim=1).values
    rank = torch.empty((b, f), dtype=ar.dtype, device=rows.device).scatter_(1, by_group.indices, ar - start)
    keep = (g < 0) | (rank < cap)
    place = torch.cumsum(keep, dim=1) - 1
    place = torch.where(keep & (place < k), place, torch.full_like(place, k))  # (column k: the bin)
    out_rows = torch.zeros((b, k + 1), dtype=rows.dtype, device=rows.device).scatter_(1, place, rows)[:, :k]
    out_scores = torch.zeros((b, k + 1), dtype=scores.dtype, device=rows.device).scatter_(1, place, scores)[:, :k]
    n_out = keep.sum(1).clamp(max=k).to(torch.int32)
    live = torch.arange(k, device=rows.device).expand(b, k) < n_out[:, None]
    return torch.where(live, item_ids[out_rows.long()], torch.zeros_like(item_ids[:1])), out_scores, out_rows, n_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("items", nargs="?", type=int, default=1_000_000)
    ap.add_argument("dim", nargs="?", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_rate.txt"))
    ap.add_argument("--trace", action="store_true", help="a short run for a kernel trace")
    ap.add_argument("--stats", help="kernel_stats.csv of a --trace run: append the cap kernel's share to the output file")
    args = ap.parse_args()
    if args.stats:
        lines = kernel_share(args.stats)
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
    g = synth.make_index(n, d, ef=EF_BUILD, device="cuda")
    index = retrieval.Index.from_dict(g)
    sc = ops.Scorer("l2", d, torch.float16)
    gor = np.floor(N_GROUPS * np.random.default_rng(5).random(n) ** 2).astype(np.int32)
    groups = {cap: retrieval.make_groups(index, group_of_row=gor, cap=cap) for cap in CAPS}
    d_gor = groups[CAPS[0]].group_of_row
    topn = {f: [f // 4] * 5 + [f] for f in FETCH}
    q = {nq: ops.user_seq_mean(torch.as_tensor(synth.make_queries(g["item_embs"], g["assign"], nq, seed=77)).to(dev)).contiguous()
         for nq in QUERIES}
    empty = retrieval.make_filter(index, deny_rows=[])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    if args.trace:
        for f in FETCH:
            for cap in CAPS:
                for _ in range(TRACE_CALLS):
                    retrieval.search_grouped(index, sc, q[QUERIES[0]], topn[f], groups[cap], k=K, want_counters=False)
        torch.cuda.synchronize()
        print(f"trace run: {TRACE_CALLS} calls of search_grouped at each of F {FETCH} x cap {CAPS}, {QUERIES[0]} queries")
        return

    lines = [f"grouped_rate: {n} items x {d} f16, L2, top-{K}, {len(np.unique(gor))} groups (largest {np.bincount(gor).max()} rows, "
             f"smallest {np.bincount(gor).min()}), rounds = {args.rounds} (median, min..max); device {torch.cuda.get_device_name(0)}"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def fmt(ms, nq):
        return f"{statistics.median(ms):8.3f} ms ({min(ms):.3f}..{max(ms):.3f}) = {statistics.median(ms) / nq:.5f} ms per query"

    def search_then_torch(nq, f, cap):
        r = retrieval.search(index, sc, q[nq], topn[f], want_counters=False)
        return torch_cap(torch, r.scores, r.index, d_gor, index.item_ids, cap, K)

    for nq in QUERIES:
        for f in FETCH:
            pairs = [("F", lambda: retrieval.search(index, sc, q[nq], topn[f], want_counters=False, k=K))]
            for cap in CAPS:
                pairs.append((f"G{cap}", lambda cap=cap: retrieval.search_grouped(index, sc, q[nq], topn[f], groups[cap], k=K,
                                                                                    want_counters=False)))
                pairs.append((f"T{cap}", lambda cap=cap: search_then_torch(nq, f, cap)))
            n_out = {}
            for cap in CAPS:  # the kernel and the torch restatement agree on every output
                r = retrieval.search_grouped(index, sc, q[nq], topn[f], groups[cap], k=K, want_counters=False)
                t = search_then_torch(nq, f, cap)
                torch.cuda.synchronize()
                assert int((r.status != 0).sum()) == 0, "a query failed"
                assert torch.equal(r.n_out, t[3]) and torch.equal(r.index, t[2]) and torch.equal(r.item_ids, t[0]) and \
                    torch.equal(r.scores, t[1]), "search_grouped and the torch cap disagree"
                n_out[cap] = r.n_out.float()
            for _, fn in pairs:  # warm every shape
                fn()
            torch.cuda.synchronize()
            res = {name: [] for name, _ in pairs}
            for _ in range(args.rounds):
                for name, fn in pairs:
                    res[name].append(timed(fn))
            base = statistics.median(res["F"])
            emit(f"{nq} queries, F = {f} (level_topn {topn[f]}), k = {K}")
            emit(f"  F   search(filter = None, k):          {fmt(res['F'], nq)}")
            for cap in CAPS:
                gm, tm = statistics.median(res[f"G{cap}"]), statistics.median(res[f"T{cap}"])
                emit(f"  G{cap}  search_grouped(cap = {cap}):            {fmt(res[f'G{cap}'], nq)}")
                emit(f"  T{cap}  search + the cap in torch:          {fmt(res[f'T{cap}'], nq)}")
                emit(f"      G - F = {gm - base:+.3f} ms ({100 * (gm - base) / base:+.1f} % of F); T - F = {tm - base:+.3f} ms; "
                     f"G = {gm / tm:.3f} x T's time; mean n_out {float(n_out[cap].mean()):.1f}, n_out < k for "
                     f"{100 * float((n_out[cap] < K).float().mean()):.1f} % of the queries")
    nq = QUERIES[0]
    for f in FETCH:
        pairs = [("B", lambda: retrieval.search_all(index, sc, q[nq], f, filter=empty)),
                 ("A", lambda: retrieval.search_all_grouped(index, sc, q[nq], K, groups[CAPS[-1]], fetch=f))]
        for _, fn in pairs:
            fn()
        torch.cuda.synchronize()
        res = {name: [] for name, _ in pairs}
        for _ in range(args.rounds):
            for name, fn in pairs:
                res[name].append(timed(fn))
        a, b = statistics.median(res["A"]), statistics.median(res["B"])
        r = retrieval.search_all_grouped(index, sc, q[nq], K, groups[CAPS[-1]], fetch=f)
        torch.cuda.synchronize()
        emit(f"exhaustive, {nq} queries, fetch = {f}, cap = {CAPS[-1]}, k = {K}")
        emit(f"  B   search_all(filter = empty, k = F): {fmt(res['B'], nq)}")
        emit(f"  A   search_all_grouped(fetch = F):     {fmt(res['A'], nq)}")
        emit(f"      A - B = {a - b:+.3f} ms ({100 * (a - b) / b:+.1f} % of B); mean n_out {float(r.n_out.float().mean()):.1f}, n_out < k "
             f"for {100 * float((r.n_out < K).float().mean()):.1f} % of the queries")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
