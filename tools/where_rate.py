#!/usr/bin/env python3
"""Attribute predicates (retrieval.search_all_where / search_where) at a size a user runs: 1M x 128 f16 under L2 on the shipped
builder's graph, top-200, 256 and 1 024 queries.  Every row carries one of 1 000 labels, uniformly; a query allows a random set of
500, 100, 10 or 1 of them: selectivities of 50 %, 10 %, 1 % and 0.1 %.  Reported per (queries, selectivity), ms per call:
  (a) exhaustive
      W   retrieval.search_all_where(k = 200): scoring, k_pred_scatter, selection, k_pred_compact;
      A   retrieval.search_all(k = 200): the same call without any condition, on the same commit -- W - A is what the
          predicates add;
      T   (256 queries) what a host does without the feature, query by query: ops.blaze_score over the table, a mask from a
          1 000-entry lookup table gathered by label, masked_fill(-inf), ops.top_k.
  (b) traversal at the fetch widths F = 512 and 1 024 (level_topn = [F/4] * 5 + [F])
      S   retrieval.search_where(k = 200);
      F   retrieval.search(filter = None, k = 200) at the same F: the existing filtered call -- S - F is the predicate's compaction
          against the plain one;
      and the mean n_out with the share of queries cut short (n_out < k), which is what tells a host to widen F or to take (a).
One process, every shape warmed, the calls alternating inside a round, device events around work that ends in a synchronise;
median of the rounds, min..max beside it.  The predicate kernels' share of a call's kernel time comes from kernel times, in a run
of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kt -- python tools/where_rate.py --trace
  python tools/where_rate.py --stats DIR/.../kt_kernel_stats.csv      # appends the shares to the output file
usage: tools/where_rate.py [items] [dim] [--rounds R] [--out FILE] [--trace | --stats CSV] [--trace-allowed 500|100|10|1]
writes profiles/where_rate.txt (or FILE) and prints the same."""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, EF_BUILD, N_LABELS = 200, 128, 1000
QUERIES = (256, 1024)
FETCH = (512, 1024)
ALLOWED = (500, 100, 10, 1)          # labels a query allows, of N_LABELS
TRACE_CALLS, TRACE_ALLOWED = 3, 100  # the trace: the 10 % selectivity
KERNELS = ("k_pred_scatter", "k_pred_compact", "k_scan_l2", "k_scan_slab_topk", "k_scan_merge", "k_search")


def kernel_share(path, trace_allowed):
    """kernel_stats.csv of the --trace run -> lines: the predicate kernels next to the scoring and the traversal"""
    total = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0)
            calls = float(row.get("Calls") or 0)
            for k in KERNELS:
                if k in name:
                    t = total.setdefault(k, [0.0, 0.0])
                    t[0] += ns
                    t[1] += calls
    assert "k_pred_scatter" in total and "k_scan_l2" in total, f"{path}: no row for the scatter or the scan kernel"
    lines = [f"kernel times (rocprofv3 --kernel-trace --stats; {TRACE_CALLS} calls of search_all_where and of search_where (F = {FETCH[0]}) "
             f"at {QUERIES[0]} queries, {trace_allowed} of {N_LABELS} labels allowed, k = {K}; k_search includes the index's 64-query probe):"]
    for k in KERNELS:
        if k in total:
            lines.append(f"  {k:18s} {total[k][0] / 1e6:10.3f} ms in all, {int(total[k][1])} launches")
    sc, l2 = total["k_pred_scatter"][0], total["k_scan_l2"][0]
    flat = sum(total.get(k, [0.0])[0] for k in ("k_pred_scatter", "k_pred_compact", "k_scan_l2", "k_scan_slab_topk", "k_scan_merge"))
    lines.append(f"  k_pred_scatter takes {sc / l2:.3f} x the scoring kernel's time and is {100 * sc / flat:.1f} % of the exhaustive kernels' time")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("items", nargs="?", type=int, default=1_000_000)
    ap.add_argument("dim", nargs="?", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "where_rate.txt"))
    ap.add_argument("--trace", action="store_true", help="a short run for a kernel trace")
    ap.add_argument("--trace-allowed", type=int, default=TRACE_ALLOWED, choices=ALLOWED, help="labels a query allows in the trace run")
    ap.add_argument("--stats", help="kernel_stats.csv of a --trace run: append the predicate kernels' share to the output file")
    args = ap.parse_args()
    if args.stats:
        lines = kernel_share(args.stats, args.trace_allowed)
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
    rng = np.random.default_rng(5)
    attrs = retrieval.make_attributes(index, label_of_row=rng.integers(0, N_LABELS, n))
    d_label = attrs.label_of_row.long()
    topn = {f: [f // 4] * 5 + [f] for f in FETCH}
    q = {nq: ops.user_seq_mean(torch.as_tensor(synth.make_queries(g["item_embs"], g["assign"], nq, seed=77)).to(dev)).contiguous()
         for nq in QUERIES}
    allowed = {(nq, a): [rng.choice(N_LABELS, a, replace=False) for _ in range(nq)] for nq in QUERIES for a in ALLOWED}
    preds = {key: retrieval.make_predicates(attrs, key[0], label_in=lists) for key, lists in allowed.items()}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    if args.trace:
        nq = QUERIES[0]
        for _ in range(TRACE_CALLS):
            retrieval.search_all_where(index, sc, q[nq], K, preds[nq, args.trace_allowed])
            retrieval.search_where(index, sc, q[nq], topn[FETCH[0]], preds[nq, args.trace_allowed], k=K, want_counters=False)
        torch.cuda.synchronize()
        print(f"trace run: {TRACE_CALLS} calls of search_all_where and search_where, {nq} queries, {args.trace_allowed} labels allowed")
        return

    lines = [f"where_rate: {n} items x {d} f16, L2, top-{K}, {N_LABELS} labels, rounds = {args.rounds} (median, min..max); "
             f"device {torch.cuda.get_device_name(0)}"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def fmt(ms, nq):
        return f"{statistics.median(ms):8.3f} ms ({min(ms):.3f}..{max(ms):.3f}) = {statistics.median(ms) / nq:.5f} ms per query"

    def measure(pairs, rounds):
        for _, fn in pairs:  # warm every shape
            fn()
        torch.cuda.synchronize()
        res = {name: [] for name, _ in pairs}
        for _ in range(rounds):
            for name, fn in pairs:
                res[name].append(timed(fn))
        return res

    def torch_where(nq, a):
        """query by query: the logits of every row, a mask from the allowed labels, the top k"""
        out = []
        for i in range(nq):
            s = ops.blaze_score(sc, q[nq][i], item_emb=index.item_embs)
            table = torch.zeros(N_LABELS, dtype=torch.bool, device=dev)
            table[torch.as_tensor(allowed[nq, a][i], device=dev)] = True
            out.append(ops.top_k(s.masked_fill(~table[d_label], float("-inf")), K))
        return out

    emit("(a) exhaustive")
    for nq in QUERIES:
        for a in ALLOWED:
            p = preds[nq, a]
            pairs = [("A", lambda: retrieval.search_all(index, sc, q[nq], K)),
                     ("W", lambda p=p: retrieval.search_all_where(index, sc, q[nq], K, p))]
            res = measure(pairs, args.rounds)
            am, wm = statistics.median(res["A"]), statistics.median(res["W"])
            r = retrieval.search_all_where(index, sc, q[nq], K, p)
            cnt = retrieval.predicate_count(p)
            torch.cuda.synchronize()
            assert torch.equal(r.n_out.long(), cnt.clamp(max=K)), "n_out is not min(k, passing rows)"
            emit(f"{nq} queries, {a} of {N_LABELS} labels allowed ({100 * a / N_LABELS:g} %; mean passing rows {float(cnt.float().mean()):.0f}), k = {K}")
            emit(f"  A   search_all(k):                     {fmt(res['A'], nq)}")
            emit(f"  W   search_all_where(k):               {fmt(res['W'], nq)}")
            emit(f"      W - A = {wm - am:+.3f} ms ({100 * (wm - am) / am:+.1f} % of A); mean n_out {float(r.n_out.float().mean()):.1f}")
            if nq == QUERIES[0]:
                t = measure([("T", lambda a=a: torch_where(nq, a))], max(args.rounds // 2, 1))["T"]
                emit(f"  T   blaze_score + torch mask + top_k:  {fmt(t, nq)}; W = {wm / statistics.median(t):.3f} x T's time")
    emit("(b) traversal")
    for nq in QUERIES:
        for f in FETCH:
            base = measure([("F", lambda: retrieval.search(index, sc, q[nq], topn[f], want_counters=False, k=K))], args.rounds)["F"]
            bm = statistics.median(base)
            emit(f"{nq} queries, F = {f} (level_topn {topn[f]}), k = {K}")
            emit(f"  F   search(filter = None, k):          {fmt(base, nq)}")
            for a in ALLOWED:
                p = preds[nq, a]
                s = measure([("S", lambda p=p: retrieval.search_where(index, sc, q[nq], topn[f], p, k=K, want_counters=False))],
                            args.rounds)["S"]
                r = retrieval.search_where(index, sc, q[nq], topn[f], p, k=K, want_counters=False)
                torch.cuda.synchronize()
                failed = int((r.status != 0).sum())
                if failed:  # (a corpus too small for the pool of this F)
                    emit(f"      {failed} of {nq} queries failed in the traversal: their n_out is 0")
                sm = statistics.median(s)
                emit(f"  S   search_where, {100 * a / N_LABELS:4g} % pass:        {fmt(s, nq)}")
                emit(f"      S - F = {sm - bm:+.3f} ms ({100 * (sm - bm) / bm:+.1f} % of F); mean n_out {float(r.n_out.float().mean()):.1f}, "
                     f"n_out < k for {100 * float((r.n_out < K).float().mean()):.1f} % of the queries")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
