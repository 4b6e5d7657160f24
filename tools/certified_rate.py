#!/usr/bin/env python3
"""The certified MLP form (NANN_MLP_CERTIFIED) against split-f16 and exact f32 at BASELINE configs[2]'s shape: 1M x 128-d
f16 items (the device HNSW builder, as bench.py), ef 128, top 200, metric weights, batches of 1024, steady state.
Prints queries/s per precision, the refined fraction per round (nann_search_refined over counters' S_r) and whether the
certified answers equal the exact ones bit for bit; the last line is one JSON object.
usage: tools/certified_rate.py [--steps K] [--warmup W] [--items N]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (its corpus / graph / query generators, unchanged)
from nann_amd import ops, retrieval, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--items", type=int, default=1 << 20)
    ap.add_argument("--batch", type=int, default=1024)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    items, dim, ef, topk = args.items, 128, 128, 200
    t0 = time.time()
    g = bench.make_index(items, dim, ef, "hnsw", 1.0, "f16", 0, dev, 16)
    index = retrieval.Index.from_dict(g)
    w = synth.make_mlp_weights_metric(dim, g["item_embs"][:: max(1, items // 65536)])  # (bench.py's sample)
    n_batches = args.steps + args.warmup
    seqs = bench.make_query_batches(dim, args.batch, n_batches, 1.0, dev, n_clusters=bench.n_clusters_for(items, ef))
    qs = [ops.user_seq_mean(seqs[j]) for j in range(n_batches)]
    topn = [ef] * 5 + [topk]
    print(f"setup {time.time() - t0:.1f} s: {items} items, batch {args.batch}, level_topn {topn}", flush=True)

    res = {"workload": "configs[2] shape: MLP scorer, 1M x 128 f16, ef 128, top 200, metric weights",
           "batch": args.batch, "steps": args.steps, "warmup": args.warmup}
    answers = {}
    for prec in ("split", "exact", "certified"):
        sc = ops.Scorer("mlp", dim, torch.float16, w, precision=prec)
        for j in range(args.warmup):
            retrieval.search(index, sc, qs[j], topn)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        outs = [retrieval.search(index, sc, qs[args.warmup + i], topn) for i in range(args.steps)]
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        qps = args.batch * args.steps / (ms / 1e3)
        res[prec + "_qps"] = round(qps, 1)
        answers[prec] = [(o.item_ids.cpu().numpy(), o.scores.cpu().numpy().view(np.uint32), o.counters.cpu().numpy(),
                          o.status.cpu().numpy()) for o in outs]
        line = f"{prec:9s} {qps / 1e3:8.1f} k q/s ({ms / args.steps:.3f} ms per batch)"
        if prec == "certified":
            # one more call on the last batch: its refined rows per round against the rows it scored
            r = retrieval.search(index, sc, qs[-1], topn)
            refined = np.asarray(r.refined(), np.int64)
            scored = r.counters.cpu().numpy()[:, 2, :].astype(np.int64).sum(0)
            frac = refined / np.maximum(scored, 1)
            res["refined_per_round"] = refined.tolist()
            res["scored_per_round"] = scored.tolist()
            res["refined_fraction_per_round"] = [round(float(x), 4) for x in frac]
            res["refined_fraction_total"] = round(float(refined.sum() / max(scored.sum(), 1)), 4)
            line += f"; refined / scored per round {np.round(frac, 4).tolist()}, total {res['refined_fraction_total']}"
        print(line, flush=True)
        del sc
    same = all((a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[2] == b[2]).all() and (a[3] == b[3]).all()
               for a, b in zip(answers["exact"], answers["certified"]))
    res["certified_equals_exact_bitwise"] = bool(same)
    res["certified_over_exact"] = round(res["certified_qps"] / res["exact_qps"], 3)
    res["certified_over_split"] = round(res["certified_qps"] / res["split_qps"], 3)
    res["valid_queries"] = int(sum((a[3] == 0).sum() for a in answers["exact"]))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
