#!/usr/bin/env python3
"""Fused multi-vector search (retrieval.search_multi_fused: the k best distinct rows of a user by a score accumulated over the
lists of its interest vectors) at a size a user runs: 1M x 128 f16 under L2 on the shipped builder's graph, ef 128, top-200, 256
users with 4 and with 8 interest vectors each, for each fusion mode.  Reported per n_vec, ms per call:
  S        retrieval.search over the n_users * n_vec vectors as queries: the inner search alone;
  U        retrieval.search_multi(k = 200): S and the union kernel -- U - S is yardstick (a), what the simpler union adds;
  F<mode>  retrieval.search_multi_fused(k = 200) per mode: S and the fuse kernel -- F - S is what the fusion adds;
  T<mode>  S followed by the same fusion in torch on the device: the terms, torch.unique over (user, row) keys, scatter_add
           into a slot per distinct row, torch.topk, two gathers -- T - S is yardstick (b).  Its additions come in no defined
           order, so its scores are held to the kernel's within a tolerance only.
One process, every shape warmed, the calls alternating inside a round, device events around work that ends in a synchronise;
median of the rounds, min..max beside it.
The fuse kernel's share of a call's kernel time comes from kernel times, in a run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kt -- python tools/fuse_rate.py --trace
  python tools/fuse_rate.py --stats DIR/.../kt_kernel_stats.csv      # appends the share to the output file
--trace runs search_multi_fused (every mode at n_vec 4, then 8) and nothing else that launches the traversal's kernels but the
index's own probe.
usage: tools/fuse_rate.py [items] [dim] [--rounds R] [--out FILE] [--trace | --stats CSV]
writes profiles/fuse_rate.txt (or FILE) and prints the same."""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

USERS, K, EF = 256, 200, 128
N_VECS = (4, 8)
MODES = ("rrf", "sum", "sum_floor", "minmax")
RRF_C = 60.0
TRACE_CALLS = 3
FUSE_KERNEL = "k_fuse_topk"
SEARCH_KERNELS = ("k_search", "k_order_key", "k_order_perm")


def kernel_share(path):
    """kernel_stats.csv of the --trace run -> lines: the fuse kernel's share of search_multi_fused's kernel time"""
    total = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0)
            for k in (FUSE_KERNEL,) + SEARCH_KERNELS:
                if k in name:
                    total[k] = total.get(k, 0.0) + ns
    assert FUSE_KERNEL in total and "k_search" in total, f"{path}: no row for the fuse or the traversal kernel"
    fuse, search = total[FUSE_KERNEL], sum(total.get(k, 0.0) for k in SEARCH_KERNELS)
    calls = TRACE_CALLS * len(N_VECS) * len(MODES)
    return [f"kernel times (rocprofv3 --kernel-trace --stats, {TRACE_CALLS} calls per mode at each of n_vec {N_VECS}, {USERS} users, "
            f"k = {K}; the traversal's total includes the index's 64-query probe):",
            f"  {FUSE_KERNEL:16s} {fuse / 1e6:10.3f} ms in all = {fuse / calls / 1e6:.4f} ms per call",
            f"  traversal        {search / 1e6:10.3f} ms in all = {search / calls / 1e6:.4f} ms per call",
            f"  the fuse kernel is {100 * fuse / (fuse + search):.1f} % of search_multi_fused's kernel time"]


def torch_fuse(torch, scores, rows, item_ids, n_items, n_users, k, mode):
    """the fusion on the device in torch: scores / rows [n_users * n_vec, F] of a search (no row twice in a list, every entry
    valid) -> (item ids, fused scores, rows) [n_users, k]"""
    n_vec = scores.shape[0] // n_users
    f = scores.shape[1]
    if mode == "rrf":
        term = (1.0 / (RRF_C + torch.arange(1, f + 1, device=scores.device, dtype=torch.float32))).expand_as(scores)
    elif mode == "sum":
        term = scores
    else:
        lo = scores.min(dim=1, keepdim=True).values
        term = scores - lo
        if mode == "minmax":
            span = scores.max(dim=1, keepdim=True).values - lo
            term = torch.where(span > 0, term / span, torch.ones_like(term))
    n_in = n_vec * f
    user = torch.arange(n_users, device=scores.device).view(n_users, 1)
    key = (user * n_items + rows.view(n_users, n_in).long()).reshape(-1)
    uniq, inverse = torch.unique(key, return_inverse=True)  # sorted: a user's distinct rows stand together
    start = torch.searchsorted(uniq, (user * n_items).view(-1))
    slot = inverse.view(n_users, n_in) - start.view(n_users, 1)
    acc = torch.zeros((n_users, n_in), dtype=torch.float32, device=scores.device)
    acc.scatter_add_(1, slot, term.reshape(n_users, n_in))
    taken = torch.zeros((n_users, n_in), dtype=torch.bool, device=scores.device)
    taken.scatter_(1, slot, True)
    top = torch.topk(torch.where(taken, acc, torch.full_like(acc, float("-inf"))), k, dim=1)
    out_rows = (uniq[top.indices + start.view(n_users, 1)] - user * n_items).to(torch.int32)
    return item_ids[out_rows.long()], top.values, out_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("items", nargs="?", type=int, default=1_000_000)
    ap.add_argument("dim", nargs="?", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_rate.txt"))
    ap.add_argument("--trace", action="store_true", help="a short run for a kernel trace")
    ap.add_argument("--stats", help="kernel_stats.csv of a --trace run: append the fuse kernel's share to the output file")
    args = ap.parse_args()
    if args.stats:
        lines = kernel_share(args.stats)
        print("\n".join(lines))
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        return

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
    fusions = {m: retrieval.make_fusion(m, rrf_c=RRF_C) for m in MODES}
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
            for m in MODES:
                for _ in range(TRACE_CALLS):
                    retrieval.search_multi_fused(index, sc, q[nv], topn, fusions[m], k=K)
        torch.cuda.synchronize()
        print(f"trace run: {TRACE_CALLS} calls of search_multi_fused per mode at each of n_vec {N_VECS}, {USERS} users")
        return

    lines = [f"fuse_rate: {n} items x {d} f16, L2, ef {EF}, top-{K}, {USERS} users, rrf_c {RRF_C:g}, no weights, rounds = {args.rounds} "
             f"(median, min..max); device {torch.cuda.get_device_name(0)}"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def fmt(ms):
        return f"{statistics.median(ms):8.3f} ms ({min(ms):.3f}..{max(ms):.3f})"

    def search_then_torch(nv, m):
        r = retrieval.search(index, sc, q[nv].view(-1, d), topn, want_counters=False)
        return torch_fuse(torch, r.scores, r.index, index.item_ids, index.n_items, USERS, K, m)

    pairs = []
    for nv in N_VECS:
        pairs.append((f"S{nv}", lambda nv=nv: retrieval.search(index, sc, q[nv].view(-1, d), topn, want_counters=False)))
        pairs.append((f"U{nv}", lambda nv=nv: retrieval.search_multi(index, sc, q[nv], topn, k=K)))
        for m in MODES:
            pairs.append((f"F{m}{nv}", lambda nv=nv, m=m: retrieval.search_multi_fused(index, sc, q[nv], topn, fusions[m], k=K)))
            pairs.append((f"T{m}{nv}", lambda nv=nv, m=m: search_then_torch(nv, m)))
    for nv in N_VECS:  # the two fusions agree on every user's score values, within what an undefined order of additions moves
        for m in MODES:
            r = retrieval.search_multi_fused(index, sc, q[nv], topn, fusions[m], k=K)
            t = search_then_torch(nv, m)
            torch.cuda.synchronize()
            assert int((r.status != 0).sum()) == 0 and bool((r.n_out == K).all()), "a vector failed or a user has fewer than k distinct rows"
            assert torch.allclose(r.scores, t[1], rtol=1e-4, atol=1e-6), f"search_multi_fused and the torch fusion disagree ({m})"
    for _, fn in pairs:  # warm every shape
        fn()
    torch.cuda.synchronize()
    res = {name: [] for name, _ in pairs}
    for _ in range(args.rounds):
        for name, fn in pairs:
            res[name].append(timed(fn))
    med = lambda name: statistics.median(res[name])
    for nv in N_VECS:
        s, u = med(f"S{nv}"), med(f"U{nv}")
        emit(f"n_vec {nv}: {USERS * nv} vectors, {nv * K} entries per user")
        emit(f"  S  search over the vectors:          {fmt(res[f'S{nv}'])}")
        emit(f"  U  search_multi(k = {K}):            {fmt(res[f'U{nv}'])}   (a) the union adds {u - s:.3f} ms")
        for m in MODES:
            f_, t = med(f"F{m}{nv}"), med(f"T{m}{nv}")
            emit(f"  F  search_multi_fused, {m:9s}:      {fmt(res[f'F{m}{nv}'])}   the fusion adds {f_ - s:.3f} ms "
                 f"= {(f_ - s) / max(u - s, 1e-9):.2f} x (a)")
            emit(f"  T  S + torch unique / scatter_add:   {fmt(res[f'T{m}{nv}'])}   (b) the torch fusion adds {t - s:.3f} ms; "
                 f"F - S = {(f_ - s) / max(t - s, 1e-9):.3f} x (b)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
