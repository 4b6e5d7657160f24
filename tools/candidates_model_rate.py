#!/usr/bin/env python3
"""Candidate-list search under the attention model: ms per call of retrieval.search_candidates_model next to the two ways the
same question is answered without it.  1M x 128 f16 items, the attention + DNN model in both precisions, k = 200, 1 024 users,
one list of 500 / 5 000 random rows per user.
  candidates  nann_search_candidates_model on the whole batch
  loop        AttnScorer.prepare once for the batch, then per user AttnScorer.score(table, indices) + top_k -- the stand-alone
              scorer, the only form there was (timed on the first LOOP_USERS users, stated per 1 024)
  filtered    search_all_model_filtered(filter = the complement of ONE user's list as a deny bitmap) for that one user:
              nann_search_all_model_filtered scores every row of the index
One process, every shape warmed, the variants alternating inside a round, device events around REPS calls that end in a
synchronise, a different batch of lists on every call; median of the rounds, min..max beside it.  The model's pre-projected
table is built and pinned before anything is timed (the loop reads the embedding rows and needs none).  No ratio here is an
acceptance criterion.
usage: tools/candidates_model_rate.py [--rounds R] [--out FILE]
writes profiles/candidates_model_rate.txt (or FILE) and prints the same."""
import argparse
import itertools
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nann_amd import ops, retrieval, synth  # noqa: E402

ITEMS, DIM, K, L_SEQ = 1_000_000, 128, 200, 50
N_USERS, LOOP_USERS, REPS, N_BATCHES = 1024, 32, 3, 4
LENGTHS = (500, 5_000)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "candidates_model_rate.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n, d = ITEMS, DIM
    embs, assign = synth.make_corpus(n, d, n_clusters=max(64, n // 4096), noise=1.0)
    deg = 8  # the call never reads the graph: a ring is a valid one
    nbv = ((np.arange(n, dtype=np.int64)[:, None] + 1 + np.arange(deg)) % n).astype(np.int32).reshape(-1)
    rs = np.arange(n + 1, dtype=np.int64) * deg
    index = retrieval.Index(embs, synth.make_item_ids(n), [nbv, nbv], [rs, rs], np.arange(0, n, max(n // 64, 1), dtype=np.int32)[:64])
    seqs = synth.make_queries(embs[:200_000], assign[:200_000], N_USERS, seq_len=L_SEQ, seed=99)
    seqs = torch.as_tensor(np.ascontiguousarray(seqs[:, :, :64])).to(dev)  # the model's sequence is [L, 64]
    w = synth.make_attn_weights(d, 64)
    lines = [f"candidates_model_rate: attention + DNN 128-64-32-1 model, {n} items x {d} f16, k = {K}, {N_USERS} users, "
             f"R = {retrieval.CANDIDATE_ATTN_BLOCK_ROWS}, rounds = {args.rounds} x {REPS} calls (median, min..max); "
             f"device {torch.cuda.get_device_name(0)}"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(2026)
    with tempfile.TemporaryDirectory() as tmp:
        for prec in ("split", "exact"):
            path = os.path.join(tmp, prec)
            ops.save_scorer_dir(path, "attention", w, precision=prec)
            model = ops.Model(path, d, L_SEQ)
            scorer = ops.AttnScorer(d, L_SEQ, torch.float16, w, precision=prec)
            retrieval.prepare(index, model)
            for length in LENGTHS:
                splits = torch.arange(N_USERS + 1, dtype=torch.int64, device=dev) * length
                batches = [torch.as_tensor(rng.integers(0, n, (N_USERS, length)).astype(np.int32)).to(dev) for _ in range(N_BATCHES)]
                turn = {name: itertools.cycle(range(N_BATCHES)) for name in ("cand", "loop")}
                deny = np.ones(n, bool)
                deny[batches[0][0].cpu().numpy()] = False
                flt = retrieval.make_filter(index, deny_rows=np.nonzero(deny)[0])

                def cand():
                    retrieval.search_candidates_model(index, model, seqs, candidates=(splits, batches[next(turn["cand"])]), k=K)

                def loop():
                    rows = batches[next(turn["loop"])]
                    kt, upad = scorer.prepare(seqs[:LOOP_USERS])
                    for u in range(LOOP_USERS):
                        ops.top_k(scorer.score(kt[u], upad[u], table=index.item_embs, indices=rows[u]), K)

                res = measure([("cand", cand), ("loop", loop),
                               ("filtered", lambda: retrieval.search_all_model_filtered(index, model, seqs[:1], K, flt))], args.rounds)
                per_batch = N_USERS / LOOP_USERS
                c, loop_ms = statistics.median(res["cand"]), statistics.median(res["loop"]) * per_batch
                emit(f"{prec}, lists of {length} rows")
                emit(f"  search_candidates_model, {N_USERS} users:                       {fmt(res['cand'])} = {c / N_USERS:.5f} ms per user")
                emit(f"  prepare + score(indices) + top_k loop, per {N_USERS} users:     {fmt(res['loop'], per_batch)} = {loop_ms / c:.1f} x")
                emit(f"  search_all_model_filtered(complement of one list), ONE user: {fmt(res['filtered'])} = "
                     f"{statistics.median(res['filtered']) / (c / N_USERS):.1f} x the call's time per user")
            retrieval.release(index, model)
            del model, scorer
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
