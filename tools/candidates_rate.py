#!/usr/bin/env python3
"""Candidate-list search: ms per call of retrieval.search_candidates next to the two ways the same question is answered
without it, and next to the bytes the lists imply.  bench.py's headline index (1M x 128 f16) and its query generator, k = 200,
1 024 queries, one list of 500 / 5 000 / 50 000 random rows per query; L2 scorer and split-f16 MLP scorer.
  candidates  nann_search_candidates on the whole batch
  loop        per query blaze_score(table, indices) + top_k, the only form there was (timed on the first LOOP_QUERIES
              queries, stated per 1 024)
  filtered    search_all(filter = the complement of the list as a deny bitmap): a bitmap serves every query of a call, so this
              is the price of ONE allowed set shared by the batch -- nann_search_all_filtered scores every row of the index
  bound       the rows the lists name, 256 B each (L2) or 1 KB of the pre-projected table each (MLP), at the ~6.3 TB/s an
              MI355X streams: a bound, not a target (random rows of 256 B do not stream)
One process, every shape warmed, the variants alternating inside a round, device events around REPS calls that end in a
synchronise; median of the rounds, min..max beside it.  The figure of merit is the ratio to the loop of the same build.
usage: tools/candidates_rate.py [--rounds R] [--out FILE]
writes profiles/candidates_rate.txt (or FILE) and prints the same."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITEMS, DIM, EF, K = 1_000_000, 128, 128, 200
N_Q, LOOP_QUERIES, REPS = 1024, 32, 3
LENGTHS = (500, 5_000, 50_000)
HBM_STREAM = 6.3e12  # bytes / s, achievable


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


def fmt(ms, scale=1.0):
    return f"{statistics.median(ms) * scale:10.3f} ms ({min(ms) * scale:.3f}..{max(ms) * scale:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "candidates_rate.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    sys.path.insert(0, ROOT)
    import bench
    from nann_amd import ops, retrieval, synth
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    g = bench.make_index(ITEMS, DIM, EF, "hnsw", 1.0, "f16", 0, dev, 16)
    index = retrieval.Index.from_dict(g, device=dev)
    q = ops.user_seq_mean(bench.make_query_batches(DIM, N_Q, 1, 1.0, dev, n_clusters=bench.n_clusters_for(ITEMS, EF))[0])
    scorers = [("L2", ops.Scorer("l2", DIM, torch.float16), 2 * DIM),
               ("MLP split-f16", ops.Scorer("mlp", DIM, torch.float16, synth.make_mlp_weights_metric(DIM, g["item_embs"]),
                                            precision="split"), 4 * 256)]
    retrieval.prepare(index, scorers[1][1])  # the table is built before anything is timed
    lines = [f"candidates_rate: {ITEMS} items x {DIM} f16, k = {K}, {N_Q} queries, rounds = {args.rounds} x {REPS} calls (median, "
             f"min..max); device {torch.cuda.get_device_name(0)}"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(2026)
    for length in LENGTHS:
        rows = torch.as_tensor(rng.integers(0, ITEMS, (N_Q, length)).astype(np.int32)).to(dev)
        splits = torch.arange(N_Q + 1, dtype=torch.int64, device=dev) * length
        deny = np.ones(ITEMS, bool)
        deny[rows[0].cpu().numpy()] = False
        flt = retrieval.make_filter(index, deny_rows=np.nonzero(deny)[0])
        for name, sc, row_bytes in scorers:
            def loop():
                for b in range(LOOP_QUERIES):
                    ops.top_k(ops.blaze_score(sc, q[b], table=index.item_embs, indices=rows[b]), K)

            res = measure([("cand", lambda: retrieval.search_candidates(index, sc, q, candidates=(splits, rows), k=K)),
                           ("loop", loop),
                           ("filtered", lambda: retrieval.search_all(index, sc, q, K, filter=flt))], args.rounds)
            per_batch = N_Q / LOOP_QUERIES
            cand, loop_ms = statistics.median(res["cand"]), statistics.median(res["loop"]) * per_batch
            bound = N_Q * length * row_bytes / HBM_STREAM * 1e3
            emit(f"{name}, lists of {length} rows")
            emit(f"  search_candidates, {N_Q} queries:                          {fmt(res['cand'])}")
            emit(f"  blaze_score(indices) + top_k loop, per {N_Q} queries:       {fmt(res['loop'], per_batch)} = {loop_ms / cand:.1f} x")
            emit(f"  search_all(filter = complement of ONE list), {N_Q} queries: {fmt(res['filtered'])} = "
                 f"{statistics.median(res['filtered']) / cand:.2f} x")
            emit(f"  the lists' rows at {HBM_STREAM / 1e12:.1f} TB/s ({row_bytes} B per row): {bound:10.3f} ms = {bound / cand:.3f} of the call")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
