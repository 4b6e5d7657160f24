#!/usr/bin/env python3
"""Multi-vector search (retrieval.search_multi: the k best distinct rows of a user by the best score any of its interest vectors
gives a row) at a size a user runs: 1M x 128 f16 under L2 on the shipped builder's graph, ef 128, top-200, 256 users with 4 and
with 8 interest vectors each.  Reported per n_vec, ms per call and per user:
  M   retrieval.search_multi(k = 200): the traversal over n_users * n_vec vectors and the union kernel, one call;
  S   retrieval.search over the same n_users * n_vec vectors as queries: the inner search alone;
  T   S followed by the union in torch on the device: a stable sort by score, a stable sort by row, the first of every run of
      equal rows kept (what torch.unique cannot say: which duplicate carries the best score), torch.topk, two gathers.
M - S is what the union kernel adds to a call, T - S what the torch union adds.  One process, every shape warmed, the calls
alternating inside a round, device events around work that ends in a synchronise; median of the rounds, min..max beside it.
The union kernel's share of a call's kernel time comes from kernel times, in a run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kt -- python tools/multi_rate.py --trace
  python tools/multi_rate.py --stats DIR/.../kt_kernel_stats.csv      # appends the share to the output file
--trace runs search_multi (n_vec 4, then 8) and nothing else that launches the traversal's kernels but the index's own probe.
usage: tools/multi_rate.py [items] [dim] [--rounds R] [--out FILE] [--trace | --stats CSV]
writes profiles/multi_rate.txt (or FILE) and prints the same."""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

USERS, K, EF = 256, 200, 128
N_VECS = (4, 8)
TRACE_CALLS = 3
UNION_KERNEL = "k_union_topk"
SEARCH_KERNELS = ("k_search", "k_order_key", "k_order_perm")


def kernel_share(path):
    """kernel_stats.csv of the --trace run -> lines: the union kernel's share of search_multi's kernel time"""
    total = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0)
            for k in (UNION_KERNEL,) + SEARCH_KERNELS:
                if k in name:
                    total[k] = total.get(k, 0.0) + ns
    assert UNION_KERNEL in total and "k_search" in total, f"{path}: no row for the union or the traversal kernel"
    union, search = total[UNION_KERNEL], sum(total.get(k, 0.0) for k in SEARCH_KERNELS)
    calls = TRACE_CALLS * len(N_VECS)
    return [f"kernel times (rocprofv3 --kernel-trace --stats, {TRACE_CALLS} calls at each of n_vec {N_VECS}, {USERS} users, k = {K}; the "
            f"traversal's total includes the index's 64-query probe):",
            f"  {UNION_KERNEL:16s} {union / 1e6:10.3f} ms in all = {union / calls / 1e6:.4f} ms per call",
            f"  traversal        {search / 1e6:10.3f} ms in all = {search / calls / 1e6:.4f} ms per call",
            f"  the union kernel is {100 * union / (union + search):.1f} % of search_multi's kernel time"]


def torch_union(torch, scores, rows, item_ids, n_users, k):
    """the union on the device in torch: scores / rows [n_users * n_vec, F] of a search -> (item ids, scores, rows) [n_users, k]"""
    s, r = scores.view(n_users, -1), rows.view(n_users, -1)
    by_score = torch.sort(s, dim=1, descending=True, stable=True)
    by_row = torch.sort(torch.gather(r, 1, by_score.indices), dim=1, stable=True)  # runs of equal rows, the best score first
    s2 = torch.gather(by_score.values, 1, by_row.indices)
    first = torch.ones_like(by_row.values, dtype=torch.bool)
    first[:, 1:] = by_row.values[:, 1:] != by_row.values[:, :-1]
    top = torch.topk(torch.where(first, s2, torch.full_like(s2, float("-inf"))), k, dim=1)
    out_rows = torch.gather(by_row.values, 1, top.indices)
    return item_ids[out_rows.long()], top.values, out_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("items", nargs="?", type=int, default=1_000_000)
    ap.add_argument("dim", nargs="?", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_rate.txt"))
    ap.add_argument("--trace", action="store_true", help="a short run for a kernel trace")
    ap.add_argument("--stats", help="kernel_stats.csv of a --trace run: append the union kernel's share to the output file")
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
    g = synth.make_index(n, d, ef=EF, device="cuda")
    index = retrieval.Index.from_dict(g)
    sc = ops.Scorer("l2", d, torch.float16)
    topn = [EF, EF, EF, EF, EF, K]
    # a user's interests: the means of n_vec behaviour sequences drawn around different clusters
    q = {nv: ops.user_seq_mean(torch.as_tensor(synth.make_queries(g["item_embs"], g["assign"], USERS * nv, seed=77 + nv)).to(dev))
             .view(USERS, nv, d).contiguous() for nv in N_VECS}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    if args.trace:
        for nv in N_VECS:
            for _ in range(TRACE_CALLS):
                retrieval.search_multi(index, sc, q[nv], topn, k=K)
        torch.cuda.synchronize()
        print(f"trace run: {TRACE_CALLS} calls of search_multi at each of n_vec {N_VECS}, {USERS} users")
        return

    lines = [f"multi_rate: {n} items x {d} f16, L2, ef {EF}, top-{K}, {USERS} users, rounds = {args.rounds} (median, min..max); device "
             f"{torch.cuda.get_device_name(0)}"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def fmt(ms):
        return f"{statistics.median(ms):8.3f} ms ({min(ms):.3f}..{max(ms):.3f}) = {statistics.median(ms) / USERS:.5f} ms per user"

    def search_then_torch(nv):
        r = retrieval.search(index, sc, q[nv].view(-1, d), topn, want_counters=False)
        return torch_union(torch, r.scores, r.index, index.item_ids, USERS, K)

    pairs = []
    for nv in N_VECS:
        pairs.append((f"M{nv}", lambda nv=nv: retrieval.search_multi(index, sc, q[nv], topn, k=K)))
        pairs.append((f"S{nv}", lambda nv=nv: retrieval.search(index, sc, q[nv].view(-1, d), topn, want_counters=False)))
        pairs.append((f"T{nv}", lambda nv=nv: search_then_torch(nv)))
    for nv in N_VECS:  # the two unions agree on the score values of every user (rows may differ among equal scores)
        m = retrieval.search_multi(index, sc, q[nv], topn, k=K)
        t = search_then_torch(nv)
        torch.cuda.synchronize()
        assert int((m.status != 0).sum()) == 0 and bool((m.n_out == K).all()), "a vector failed or a user has fewer than k distinct rows"
        assert torch.equal(m.scores, t[1]), "search_multi and the torch union disagree"
    for _, fn in pairs:  # warm every shape
        fn()
    torch.cuda.synchronize()
    res = {name: [] for name, _ in pairs}
    for _ in range(args.rounds):
        for name, fn in pairs:
            res[name].append(timed(fn))
    for nv in N_VECS:
        m, s, t = (statistics.median(res[f"{c}{nv}"]) for c in "MST")
        emit(f"n_vec {nv}: {USERS * nv} vectors, {nv * K} entries per user")
        emit(f"  M  search_multi(k = {K}):            {fmt(res[f'M{nv}'])}")
        emit(f"  S  search over the vectors:          {fmt(res[f'S{nv}'])}")
        emit(f"  T  S + torch sort / sort / topk:     {fmt(res[f'T{nv}'])}")
        emit(f"     the union adds {m - s:.3f} ms to a call as a kernel ({100 * (m - s) / s:.1f} % of S) and {t - s:.3f} ms in torch "
             f"({100 * (t - s) / s:.1f} % of S); M = {m / t:.3f} x T's time")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
