#!/usr/bin/env python3
"""Filtered retrieval: what the filter costs next to the unfiltered calls, and what the traversal's recall is against the
filtered exhaustive answer.  bench.py's headline index (1M x 128 f16, HNSW built on the device), its query generator.
  exhaustive  1 024 queries, k = 200: nann_search_all (unfiltered) | nann_search_all_filtered with no filter | a 10 % bitmap plus
              200-row lists | a 50 % bitmap
  traversal   4 096 queries, beams [128] * 5: nann_search_opt at level_topn[5] = 200 (unfiltered) | nann_search_filtered at
              F = 512, k = 200 with the 10 % bitmap plus 200-row lists
  recall      filtered traversal (F = 512, k = 200) against filtered exhaustive search at deny fractions 0, 0.1, 0.5, 0.9
              (evaluate.recall_vs_bruteforce), with the mean n_out of the traversal
One process, every shape warmed, the variants alternating inside a round, device events around REPS calls that end in a
synchronise; median of the rounds, min..max beside it.  These are whole-call times.
--parent-tree DIR: a checkout of the parent commit with its library built (git worktree add DIR HEAD~1; python -m
nann_amd.build in it).  Its unfiltered calls are then timed too, by a child process that imports nann_amd from DIR, once before
and once after this process's rounds (a second process cannot alternate call by call).  Without it the unfiltered calls of this
build stand for the parent: this change touches none of their kernels or launches.
usage: tools/filtered_rate.py [--rounds R] [--parent-tree DIR] [--out FILE]
writes profiles/filtered_rate.txt (or FILE) and prints the same."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITEMS, DIM, EF, K, F = 1_000_000, 128, 128, 200, 512
N_ALL, N_TRAV, REPS = 1024, 4096, 5
TOPN_PLAIN = [EF] * 5 + [K]
TOPN_FETCH = [EF] * 5 + [F]


def timed(fn, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(pairs, rounds):
    """pairs: [(name, fn)] -> {name: [ms per call, one per round]}, the functions alternating inside a round"""
    for _, fn in pairs:  # warm every shape
        fn()
    torch.cuda.synchronize()
    out = {name: [] for name, _ in pairs}
    for _ in range(rounds):
        for name, fn in pairs:
            out[name].append(timed(fn))
    return out


def fmt(ms):
    return f"{statistics.median(ms):8.3f} ms ({min(ms):.3f}..{max(ms):.3f})"


def setup(root):
    """(index, L2 scorer, queries f32[4096, 128]) from the tree at `root`: bench.py's headline index and queries"""
    sys.path.insert(0, root)
    import bench
    from nann_amd import ops, retrieval
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    g = bench.make_index(ITEMS, DIM, EF, "hnsw", 1.0, "f16", 0, dev, 16)
    index = retrieval.Index.from_dict(g, device=dev)
    seqs = bench.make_query_batches(DIM, N_TRAV, 1, 1.0, dev, n_clusters=bench.n_clusters_for(ITEMS, EF))
    q = ops.user_seq_mean(seqs[0])
    return index, ops.Scorer("l2", DIM, torch.float16), q


def baseline(root, rounds):
    """the unfiltered calls of the tree at `root` -> {"all": [ms], "trav": [ms]}"""
    index, sc, q = setup(root)
    from nann_amd import retrieval
    return measure([("all", lambda: retrieval.search_all(index, sc, q[:N_ALL], K)),
                    ("trav", lambda: retrieval.search(index, sc, q, TOPN_PLAIN, want_counters=False))], rounds)


def parent_times(tree, rounds):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--baseline-of", tree, "--rounds", str(rounds)],
                       capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError("the parent's baseline run failed:\n" + p.stderr[-3000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--baseline-of", default=None, help=argparse.SUPPRESS)  # the child of --parent-tree
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filtered_rate.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if args.baseline_of:
        print(json.dumps(baseline(os.path.abspath(args.baseline_of), args.rounds)))
        return
    parent = [parent_times(args.parent_tree, args.rounds)] if args.parent_tree else []
    index, sc, q = setup(ROOT)
    from nann_amd import evaluate, retrieval
    lines = [f"filtered_rate: {ITEMS} items x {DIM} f16, k = {K}, rounds = {args.rounds} x {REPS} calls (median, min..max); device "
             f"{torch.cuda.get_device_name(0)}"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(2025)
    u = rng.random(ITEMS)
    plain = retrieval.search(index, sc, q, TOPN_PLAIN, want_counters=False)
    seen = plain.index.cpu().numpy()[:, :20]  # 200-row lists: the query's own best 20 ("seen") and 180 rows anywhere
    lists = np.concatenate([seen, rng.integers(0, ITEMS, (N_TRAV, 180))], axis=1)

    def flt(frac, with_lists, nq):
        return retrieval.make_filter(index, deny_rows=np.nonzero(u < frac)[0] if frac > 0 else None,
                                     exclude_rows=list(lists[:nq]) if with_lists else None)

    qa = q[:N_ALL]
    f_none, f_10, f_50 = retrieval.make_filter(index), flt(0.1, True, N_ALL), flt(0.5, False, N_ALL)
    t_10 = flt(0.1, True, N_TRAV)
    res = measure([("all", lambda: retrieval.search_all(index, sc, qa, K)),
                   ("all_null", lambda: retrieval.search_all(index, sc, qa, K, filter=f_none)),
                   ("all_10", lambda: retrieval.search_all(index, sc, qa, K, filter=f_10)),
                   ("all_50", lambda: retrieval.search_all(index, sc, qa, K, filter=f_50)),
                   ("trav", lambda: retrieval.search(index, sc, q, TOPN_PLAIN, want_counters=False)),
                   ("trav_null", lambda: retrieval.search(index, sc, q, TOPN_FETCH, want_counters=False, k=K)),
                   ("trav_10", lambda: retrieval.search(index, sc, q, TOPN_FETCH, want_counters=False, filter=t_10, k=K))],
                  args.rounds)
    if args.parent_tree:
        parent.append(parent_times(args.parent_tree, args.rounds))

    def section(title, base_key, rows):
        emit(title)
        base = statistics.median(res[base_key])
        if parent:
            both = parent[0][base_key] + parent[1][base_key]
            emit(f"  parent commit, unfiltered (own process, before and after): {fmt(both)}")
            emit(f"  this build,    unfiltered (alternating with the rows below): {fmt(res[base_key])} = "
                 f"{base / statistics.median(both):.3f} x the parent")
            base = statistics.median(both)
        else:
            emit(f"  unfiltered (the parent's kernels and launches, unchanged):    {fmt(res[base_key])}")
        for key, what in rows:
            emit(f"  {what:61s} {fmt(res[key])} = {statistics.median(res[key]) / base:.3f} x")

    section(f"exhaustive search, {N_ALL} queries (nann_search_all | nann_search_all_filtered)", "all",
            [("all_null", "no filter (final selection and n_out only):"), ("all_10", "10 % bitmap + 200-row lists:"),
             ("all_50", "50 % bitmap:")])
    section(f"traversal, {N_TRAV} queries, beams {TOPN_PLAIN[:5]} (nann_search_opt at level_topn[5] = {K} | nann_search_filtered at "
            f"F = {F}, k = {K})", "trav",
            [("trav_null", "no filter (the wider last stage and the selection):"), ("trav_10", "10 % bitmap + 200-row lists:")])

    emit(f"recall of the filtered traversal (F = {F}, k = {K}) against the filtered exhaustive answer, {N_ALL} queries, bitmap only")
    emit("  deny fraction   recall@200   mean n_out (traversal)   mean n_out (exhaustive)")
    for frac in (0.0, 0.1, 0.5, 0.9):
        f = flt(frac, False, N_ALL) if frac > 0 else f_none
        rec = evaluate.recall_vs_bruteforce(index, sc, qa, TOPN_FETCH, filter=f, k=K)
        n_t = retrieval.search(index, sc, qa, TOPN_FETCH, want_counters=False, filter=f, k=K).n_out.float().mean().item()
        n_e = retrieval.search_all(index, sc, qa, K, filter=f).n_out.float().mean().item()
        emit(f"  {frac:13.1f}   {rec:10.4f}   {n_t:22.1f}   {n_e:23.1f}")
    rec_plain = evaluate.recall_vs_bruteforce(index, sc, qa, TOPN_PLAIN, batched=True)
    emit(f"  (unfiltered traversal at level_topn[5] = {K} against unfiltered exhaustive search: {rec_plain:.4f})")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
