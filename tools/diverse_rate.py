#!/usr/bin/env python3
"""Diversified results (retrieval.search_diverse: MMR re-ranking of the fetched top-F on the device) at a size a user runs: 1M x
128 f16 under L2 on the shipped builder's graph, top-200 at the fetch widths F = 512 and 1 024 (level_topn = [F/4] * 5 + [F]: the
last stage ranks its whole pool), 256 and 1 024 queries, lambda = 0.5, the similarity L2.  Reported per (queries, F), ms per call:
  D   retrieval.search_diverse(k = 200): the traversal at F and the MMR kernel, one call;
  F   retrieval.search(filter = None, k = 200) at the same F: the existing filtered call, the traversal and k_filter_compact --
      the same inner search on the same commit, so D - F is the MMR stage against the plain compaction;
  T   retrieval.search at F followed by the same MMR in torch on the device: a gather of the rows into [B, F, d], a bmm Gram
      matrix turned into -||a - b||^2, and a loop of k steps (argmax, a gather of the pick's Gram row, maximum, multiply-subtract,
      a scatter that retires the pick).  T - F is the reference for D - F: the device stage should be the faster one.
and the mean pairwise similarity (-||a - b||^2 over the pairs of a returned list, averaged over the queries) at lambda 1 and 0.5:
what the re-ranking buys.  torch sums a row's terms in another order than the kernel, so its picks may part from the kernel's at a
near-tie and never meet again; the share of equal picks is reported, not asserted.
The kernel's two scoring paths (nann_mmr.h: candidate rows copied into LDS once | scored from the table every step) are compared
at F = 512, where the LDS path applies, on retrieval.mmr alone over one fetched list: this process times the shipped library, a
child process the table-only build variant:
  python tools/build_res_variant.py mmr_table --unit nann_cand_inst.hip -DNANN_MMR_TABLE_ONLY
  python tools/diverse_rate.py --table-lib nann_amd/_build/var_mmr_table/libnann_hip.so
One process per library, every shape warmed, the calls alternating inside a round, device events around work that ends in a
synchronise; median of the rounds, min..max beside it.  The MMR kernel's share of a call's kernel time comes from kernel times, in
a run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kt -- python tools/diverse_rate.py --trace
  python tools/diverse_rate.py --stats DIR/.../kt_kernel_stats.csv      # appends the share to the output file
usage: tools/diverse_rate.py [items] [dim] [--rounds R] [--out FILE] [--table-lib LIB] [--trace | --stats CSV | --mmr-only]
writes profiles/diverse_rate.txt (or FILE) and prints the same."""
import argparse
import csv
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, EF_BUILD, LAM = 200, 128, 0.5
QUERIES = (256, 1024)
FETCH = (512, 1024)
AB_FETCH = 512
TRACE_CALLS = 3
MMR_KERNEL = "k_mmr"
SEARCH_KERNELS = ("k_search", "k_order_key", "k_order_perm")


def kernel_share(path):
    """kernel_stats.csv of the --trace run -> lines: the MMR kernel's share of search_diverse's kernel time"""
    total = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0)
            for k in (MMR_KERNEL,) + SEARCH_KERNELS:
                if k in name:
                    total[k] = total.get(k, 0.0) + ns
    assert MMR_KERNEL in total and "k_search" in total, f"{path}: no row for the MMR or the traversal kernel"
    mmr, search = total[MMR_KERNEL], sum(total.get(k, 0.0) for k in SEARCH_KERNELS)
    calls = TRACE_CALLS * len(FETCH)
    return [f"kernel times (rocprofv3 --kernel-trace --stats, {TRACE_CALLS} calls at each of F {FETCH}, {QUERIES[0]} queries, k = {K}; "
            f"the traversal's total includes the index's 64-query probe):",
            f"  {MMR_KERNEL:16s} {mmr / 1e6:10.3f} ms in all = {mmr / calls / 1e6:.4f} ms per call",
            f"  traversal        {search / 1e6:10.3f} ms in all = {search / calls / 1e6:.4f} ms per call",
            f"  the MMR kernel is {100 * mmr / (mmr + search):.1f} % of search_diverse's kernel time"]


def torch_mmr(torch, scores, rows, table, lam, k):
    """MMR on the device in torch: scores / rows [B, F] of a search -> picked positions [B, k] (every entry valid, k <= F)"""
    b, f = rows.shape
    x = table[rows.long()].float()                                     # [B, F, d]
    sq = (x * x).sum(2)
    gram = -(sq[:, :, None] + sq[:, None, :] - 2.0 * torch.bmm(x, x.transpose(1, 2)))
    r = lam * scores
    v = r.clone()
    p = torch.full_like(r, float("-inf"))
    picks = torch.empty((b, k), dtype=torch.long, device=rows.device)
    gone = torch.full((b, 1), float("-inf"), device=rows.device)
    for n in range(k):
        t = torch.argmax(v, dim=1, keepdim=True)
        picks[:, n:n + 1] = t
        p = torch.maximum(p, torch.gather(gram, 1, t[:, :, None].expand(b, 1, f))[:, 0])
        v = (r - (1.0 - lam) * p).scatter_(1, picks[:, :n + 1], gone.expand(b, n + 1))
    return picks


def pairwise(torch, table, rows):
    """mean over queries of the mean -||a - b||^2 over the pairs of distinct positions of a returned list"""
    x = table[rows.long()].float()
    sq = (x * x).sum(2)
    gram = -(sq[:, :, None] + sq[:, None, :] - 2.0 * torch.bmm(x, x.transpose(1, 2)))
    k = rows.shape[1]
    off = gram.sum((1, 2)) - torch.diagonal(gram, dim1=1, dim2=2).sum(1)
    return float((off / (k * (k - 1))).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("items", nargs="?", type=int, default=1_000_000)
    ap.add_argument("dim", nargs="?", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diverse_rate.txt"))
    ap.add_argument("--table-lib", help="the NANN_MMR_TABLE_ONLY build of the library: time the table path next to the LDS path")
    ap.add_argument("--trace", action="store_true", help="a short run for a kernel trace")
    ap.add_argument("--stats", help="kernel_stats.csv of a --trace run: append the MMR kernel's share to the output file")
    ap.add_argument("--mmr-only", action="store_true", help="time retrieval.mmr alone at F = %d and print it (the A/B's child)" % AB_FETCH)
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
    topn = {f: [f // 4] * 5 + [f] for f in FETCH}
    q = {nq: ops.user_seq_mean(torch.as_tensor(synth.make_queries(g["item_embs"], g["assign"], nq, seed=77)).to(dev)).contiguous()
         for nq in QUERIES}
    dv = {lam: retrieval.make_diversity(lam=lam, sim="l2") for lam in (LAM, 1.0)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def mmr_alone():
        """retrieval.mmr over one fetched list at F = AB_FETCH -> {queries: [ms per round]}"""
        out = {}
        for nq in QUERIES:
            r = retrieval.search(index, sc, q[nq], topn[AB_FETCH], want_counters=False)
            fn = lambda: retrieval.mmr(index, r.scores, r.index, dv[LAM], K)  # noqa: E731
            fn()
            torch.cuda.synchronize()
            out[nq] = [timed(fn) for _ in range(args.rounds)]
        return out

    if args.mmr_only:
        for nq, ms in mmr_alone().items():
            print(f"MMR_ONLY {nq} " + " ".join(f"{v:.4f}" for v in ms), flush=True)
        return

    if args.trace:
        for f in FETCH:
            for _ in range(TRACE_CALLS):
                retrieval.search_diverse(index, sc, q[QUERIES[0]], topn[f], dv[LAM], k=K, want_counters=False)
        torch.cuda.synchronize()
        print(f"trace run: {TRACE_CALLS} calls of search_diverse at each of F {FETCH}, {QUERIES[0]} queries")
        return

    lines = [f"diverse_rate: {n} items x {d} f16, L2, top-{K}, lambda = {LAM}, sim = l2, rounds = {args.rounds} (median, min..max); "
             f"device {torch.cuda.get_device_name(0)}"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def fmt(ms, nq):
        return f"{statistics.median(ms):8.3f} ms ({min(ms):.3f}..{max(ms):.3f}) = {statistics.median(ms) / nq:.5f} ms per query"

    def search_then_torch(nq, f):
        r = retrieval.search(index, sc, q[nq], topn[f], want_counters=False)
        return r, torch_mmr(torch, r.scores, r.index, index.item_embs, LAM, K)

    for nq in QUERIES:
        for f in FETCH:
            pairs = [("F", lambda: retrieval.search(index, sc, q[nq], topn[f], want_counters=False, k=K)),
                     ("D", lambda: retrieval.search_diverse(index, sc, q[nq], topn[f], dv[LAM], k=K, want_counters=False)),
                     ("T", lambda: search_then_torch(nq, f))]
            half = retrieval.search_diverse(index, sc, q[nq], topn[f], dv[LAM], k=K, want_counters=False)
            one = retrieval.search_diverse(index, sc, q[nq], topn[f], dv[1.0], k=K, want_counters=False)
            _, picks = search_then_torch(nq, f)
            torch.cuda.synchronize()
            assert int((half.status != 0).sum()) == 0 and int((half.n_out != K).sum()) == 0, "a query failed"
            agree = float((half.pos.long() == picks).float().mean())
            sim_half, sim_one = pairwise(torch, index.item_embs, half.index), pairwise(torch, index.item_embs, one.index)
            for _, fn in pairs:  # warm every shape
                fn()
            torch.cuda.synchronize()
            res = {name: [] for name, _ in pairs}
            for _ in range(args.rounds):
                for name, fn in pairs:
                    res[name].append(timed(fn))
            base, dm, tm = (statistics.median(res[x]) for x in "FDT")
            emit(f"{nq} queries, F = {f} (level_topn {topn[f]}), k = {K}")
            emit(f"  F   search(filter = None, k):          {fmt(res['F'], nq)}")
            emit(f"  D   search_diverse(lambda = {LAM}):       {fmt(res['D'], nq)}")
            emit(f"  T   search + MMR in torch:             {fmt(res['T'], nq)}")
            emit(f"      D - F = {dm - base:+.3f} ms ({100 * (dm - base) / base:+.1f} % of F); T - F = {tm - base:+.3f} ms; "
                 f"(D - F) / (T - F) = {(dm - base) / (tm - base):.3f}; D = {dm / tm:.3f} x T's time")
            emit(f"      mean pairwise -||a - b||^2 of a returned list: {sim_one:.3f} at lambda 1, {sim_half:.3f} at lambda {LAM}; "
                 f"picks equal to torch's: {100 * agree:.1f} %")
    own = mmr_alone()
    from nann_amd import build as B
    emit(f"retrieval.mmr alone, F = {AB_FETCH}, k = {K}, lambda = {LAM} ({os.path.relpath(os.environ.get('NANN_HIP_LIB') or B.LIB, ROOT)})")
    for nq in QUERIES:
        emit(f"  shipped library, {nq:5d} queries:          {fmt(own[nq], nq)}")
    if args.table_lib:
        env = dict(os.environ, NANN_HIP_LIB=os.path.abspath(args.table_lib))
        child = subprocess.run([sys.executable, os.path.abspath(__file__), str(n), str(d), "--rounds", str(args.rounds), "--mmr-only"],
                               env=env, check=True, capture_output=True, text=True).stdout
        for line in child.splitlines():
            if line.startswith("MMR_ONLY "):
                nq, ms = int(line.split()[1]), [float(v) for v in line.split()[2:]]
                emit(f"  table-only variant, {nq:5d} queries:       {fmt(ms, nq)}")
                emit(f"      LDS path / table path = {statistics.median(own[nq]) / statistics.median(ms):.3f}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
