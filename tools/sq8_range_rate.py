#!/usr/bin/env python3
"""Certified scalar-quantised range search (retrieval.search_all_range_sq8_exact: the int8 scan, a survivor pass at the caller's
threshold, an exact re-scoring of the survivors only -- search_all_range's bits) next to retrieval.search_all_range at a size a
user runs: 1M x 128 f16 from synth, L2 and the inner product, batches of 256 and 1 024 queries, thresholds that give about 10,
100, 1 000 and 10 000 matches per query (the score of a query's m-th best row, from a float32 matrix product in torch).
Reported per metric, batch and threshold:
  A        retrieval.search_all_range at capacity = the total (known from a call before: ONE scoring of the index), ms per call;
  C<cap>   retrieval.search_all_range_sq8_exact(cap, capacity = the total, fallback=False) for cap = 4 096 and 16 384, ms per call;
           the share of queries certified, the mean and the largest n_survivors / matches over the certified queries with a
           match, and whether row_splits, index, score bits and item ids of the certified queries equal A's;
and per metric and batch
  D        retrieval.search_all_sq8_exact(k = 200, fetch = 200, cap = 2048, fallback=False), ms per call -- the top-k form.
One process, every shape warmed, the calls alternating inside a round, device events around work that ends in a synchronise;
median of the rounds, min..max beside it.  Table and bounds are made outside the timed region.  No ratio is a pass mark: where C
is not faster than A the output says so.  An uncertified query costs C its scan and returns nothing: read C's time next to its
certified share.
Kernel times come from a run of their own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kt -- python tools/sq8_range_rate.py --trace
  python tools/sq8_range_rate.py --stats DIR/.../kt_kernel_stats.csv      # appends the kernel times to the output file
--trace runs TRACE_CALLS calls of search_all_range and of search_all_range_sq8_exact at 128 queries, L2, about 100 matches per
query -- ONE chunk of both.
usage: tools/sq8_range_rate.py [items] [dim] [--rounds R] [--out FILE] [--trace | --stats CSV]
writes profiles/sq8_range_rate.txt (or FILE) and prints the same."""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 200
CAPS = (4096, 16384)
BATCHES = (256, 1024)
MATCHES = (10, 100, 1000, 10000)
TRACE_CALLS, TRACE_QUERIES, TRACE_MATCHES = 5, 128, 100
NEW = ("k_sq8_range_lists", "k_sq8_range_count", "k_sq8_range_fill")
KERNELS = ("k_scan_sq8", "k_scan_l2", "k_range_count", "k_range_fill", "k_sq8_encode", "k_sq8_row_err", "k_sq8_exact_terms",
           "k_sq8_surv_count", "k_range_scan", "k_sq8_surv_fill", "k_cand_plan", "k_cand_score_l2", "k_range_splits",
           "k_scan_transpose_q") + NEW


def kernel_times(path):
    """kernel_stats.csv of the --trace run -> lines: calls and average time of the kernels of both calls, and the new kernels'
    share of the certified call's kernel time"""
    rows = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            hit = [k for k in KERNELS if k in name]
            if hit:
                k = max(hit, key=len)  # (k_range_count is a part of k_sq8_range_count's name)
                calls, ns = rows.get(k, (0, 0.0))
                rows[k] = (calls + int(row.get("Calls") or 0), ns + float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0))
    assert "k_sq8_range_count" in rows and "k_scan_l2" in rows, f"{path}: no row for k_sq8_range_count or k_scan_l2"
    lines = [f"kernel times (rocprofv3 --kernel-trace --stats; {TRACE_CALLS} calls of search_all_range and of search_all_range_sq8_exact("
             f"cap = {CAPS[0]}) at {TRACE_QUERIES} queries = one chunk each, L2, about {TRACE_MATCHES} matches per query, after one warming "
             "call of each; k_range_scan runs once in the first call and twice in the second; k_sq8_encode and k_sq8_row_err include the "
             "launches that made the table and the bounds):"]
    for k in KERNELS:
        if k in rows:
            calls, ns = rows[k]
            lines.append(f"  {k:20s} {calls:4d} launches, {ns / max(calls, 1) / 1e3:10.1f} us each, {ns / 1e6:9.3f} ms in all")
    per_call = lambda k: rows[k][1] / max(rows[k][0], 1) if k in rows else 0.0  # noqa: E731
    # one certified call: every kernel of its chain once, k_range_scan twice; without k_sq8_encode and k_sq8_row_err on the chunk's
    # queries, whose averages are mixed with the launches over the whole table
    chain = ("k_scan_sq8", "k_sq8_exact_terms", "k_sq8_surv_count", "k_sq8_surv_fill", "k_cand_plan",
             "k_cand_score_l2", "k_range_splits") + NEW
    call_ns = sum(per_call(k) for k in chain) + 2 * per_call("k_range_scan")
    new_ns = sum(per_call(k) for k in NEW)
    lines.append(f"  one certified call: {call_ns / 1e3:.1f} us of kernel time (the averages above, k_range_scan twice, k_sq8_encode and k_sq8_row_err left out); the new kernels "
                 f"{new_ns / 1e3:.1f} us = {100 * new_ns / call_ns:.1f} %, k_scan_sq8 {per_call('k_scan_sq8') / 1e3:.1f} us = "
                 f"{100 * per_call('k_scan_sq8') / call_ns:.1f} %")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("items", nargs="?", type=int, default=1_000_000)
    ap.add_argument("dim", nargs="?", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sq8_range_rate.txt"))
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
    index = retrieval.Index(embs, synth.make_item_ids(n), [nbv, nbv], [rs, rs], np.arange(0, n, max(n // 64, 1), dtype=np.int32)[:64])
    n_q = TRACE_QUERIES if args.trace else max(BATCHES)
    q_all = ops.user_seq_mean(torch.as_tensor(synth.make_queries(embs, assign, n_q, seed=99)).to(dev))
    matches = tuple(m for m in MATCHES if m <= n)

    def thresholds(metric):
        """f32[len(matches), n_q]: per query the score of its m-th best row by a float32 product in torch -- near the exact
        scorer's value, which is all 'about m matches' asks"""
        x = torch.as_tensor(embs).to(dev).float()
        out = torch.empty((len(matches), n_q), dtype=torch.float32, device=dev)
        for c0 in range(0, n_q, 128):
            qc = q_all[c0:c0 + 128]
            s = qc @ x.T
            if metric == "l2":
                s = 2 * s - (x * x).sum(1)[None, :] - (qc * qc).sum(1)[:, None]
            top = torch.topk(s, max(matches), dim=1).values
            for j, m in enumerate(matches):
                out[j, c0:c0 + 128] = top[:, m - 1]
        return out

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    sq8 = retrieval.make_sq8(index)
    bounds = retrieval.make_sq8_bounds(index, sq8)

    def certified(sc, q, thr, cap, capacity):
        return retrieval.search_all_range_sq8_exact(index, sq8, bounds, sc, q, thr, cap=cap, capacity=capacity, fallback=False)

    if args.trace:
        sc = ops.Scorer("l2", d, torch.float16)
        thr = thresholds("l2")[matches.index(TRACE_MATCHES) if TRACE_MATCHES in matches else 0]
        total = retrieval.search_all_range(index, sc, q_all, thr).total
        for _ in range(TRACE_CALLS + 1):
            retrieval.search_all_range(index, sc, q_all, thr, capacity=total)
            certified(sc, q_all, thr, CAPS[0], total)
        torch.cuda.synchronize()
        print(f"trace run: {TRACE_CALLS} + 1 calls of search_all_range and of search_all_range_sq8_exact(cap = {CAPS[0]}) at "
              f"{TRACE_QUERIES} queries, {total} matches in all")
        return

    lines = [f"sq8_range_rate: {n} items x {d} f16, caps {CAPS}, rounds = {args.rounds} (median, min..max); device "
             f"{torch.cuda.get_device_name(0)}",
             "A = search_all_range(capacity = total); C = search_all_range_sq8_exact(cap, capacity = total, fallback=False); "
             f"D = search_all_sq8_exact(k = {K}, fetch = {K}, cap = 2048, fallback=False)"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def fmt(ms):
        return f"{statistics.median(ms):9.3f} ms ({min(ms):.3f}..{max(ms):.3f})"

    def same(c, ref, cert):
        """the certified queries' segments of c against ref's: counts, rows, score bits, item ids"""
        cs, rs_ = c.row_splits.cpu().numpy(), ref.row_splits.cpu().numpy()
        if not (np.diff(cs)[cert] == np.diff(rs_)[cert]).all():
            return False
        cols = [(c.index.cpu().numpy(), ref.index.cpu().numpy()), (c.scores.cpu().numpy().view(np.uint32), ref.scores.cpu().numpy().view(np.uint32)),
                (c.item_ids.cpu().numpy(), ref.item_ids.cpu().numpy())]
        for i in np.flatnonzero(cert):
            for a, o in cols:
                if not (a[cs[i]:cs[i + 1]] == o[rs_[i]:rs_[i + 1]]).all():
                    return False
        return True

    for line in lines:
        print(line, flush=True)
    for metric in ("l2", "ip"):
        sc = ops.Scorer(metric, d, torch.float16)
        thr_all = thresholds(metric)
        for b in BATCHES:
            q = q_all[:b]
            emit(f"{metric}, batch {b}")
            top = lambda: retrieval.search_all_sq8_exact(index, sq8, bounds, sc, q, K, fetch=K, cap=2048, fallback=False)  # noqa: E731
            top()
            torch.cuda.synchronize()
            emit(f"  D  search_all_sq8_exact, k = {K}:                 {fmt([timed(top) for _ in range(args.rounds)])}")
            for j, m in enumerate(matches):
                thr = thr_all[j, :b].contiguous()
                ref = retrieval.search_all_range(index, sc, q, thr)
                total = ref.total
                n_match = np.diff(ref.row_splits.cpu().numpy())
                pairs = [("A", lambda: retrieval.search_all_range(index, sc, q, thr, capacity=total))]
                facts = {}
                for cap in CAPS:
                    pairs.append((f"C{cap}", lambda cap=cap: certified(sc, q, thr, cap, total)))
                    c = certified(sc, q, thr, cap, total)
                    torch.cuda.synchronize()
                    cert = c.certified.cpu().numpy() == 1
                    surv = c.n_survivors.cpu().numpy()
                    live = cert & (n_match > 0)
                    ratio = surv[live] / n_match[live] if live.any() else np.zeros(1)
                    facts[cap] = (cert.mean(), ratio.mean(), ratio.max(), same(c, ref, cert))
                for _, fn in pairs:  # warm every shape
                    fn()
                torch.cuda.synchronize()
                res = {name: [] for name, _ in pairs}
                for _ in range(args.rounds):
                    for name, fn in pairs:
                        res[name].append(timed(fn))
                a = statistics.median(res["A"])
                emit(f"  about {m} matches per query (mean {n_match.mean():.1f}, max {int(n_match.max())})")
                emit(f"    A  search_all_range:                            {fmt(res['A'])}   {a / b:.4f} ms per query")
                for cap in CAPS:
                    t = statistics.median(res[f"C{cap}"])
                    share, r_mean, r_max, ok = facts[cap]
                    emit(f"    C  search_all_range_sq8_exact, cap = {cap:5d}:    {fmt(res[f'C{cap}'])}   A / C = {a / t:.2f}   certified "
                         f"{share:.4f} of the queries, n_survivors / matches mean {r_mean:.2f} max {r_max:.2f}, certified segments "
                         f"bit-identical to A: {ok}")
                    if share == 1.0:
                        emit(f"       C is {'FASTER' if t < a else 'NOT faster'} than A here ({t / a:.2f} x A's time)")
                    else:
                        emit(f"       C's time is not A's work here: {1 - share:.4f} of the queries came back uncertified and empty, and "
                             "would still have to go through A")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
