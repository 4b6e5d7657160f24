#!/usr/bin/env python3
"""Exhaustive search: the per-query loop (A: ops.blaze_score + ops.top_k, one query at a time -- how the ground truth of every
recall figure was computed before nann_search_all) against retrieval.search_all (B) at a size a user runs.  One process, every
shape warmed, A and B alternating, device events around work that ends in a synchronise; median of the rounds, min..max beside it.
For B also: the algorithm's operations and the table bytes it requests, the least time the hardware could take for them (the
larger of operations / peak rate and bytes / peak bandwidth) over the measured time, and which of the two binds.  These are
whole-call figures (scoring + selection + merge), not a kernel's share of peak; kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- tools/search_all_rate.py --trace` run.
The MLP scorers' pre-projected table is built and pinned (retrieval.prepare) BEFORE the timed region: B's figures are the
steady state of a prepared pair; an unprepared pair pays the build once, in its first call (~2 ms per million items), and A
needs no table.  Table bytes are priced at the 8 TB/s specification; ~6.3 TB/s is achievable, so "least time / measured" of a
row bound by table bytes is optimistic by that ratio (x 1.27 for the byte time).
usage: tools/search_all_rate.py [items] [dim] [dtype] [--rounds R] [--out FILE] [--trace]
writes profiles/search_all_rate.txt (or FILE) and prints the same."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nann_amd import ops, retrieval, synth  # noqa: E402

K = 200
PEAK_VEC_OPS = 78.6e12     # f32 vector operations / s (157.3 TFLOP/s counts an fma as two)
PEAK_MFMA = {"split": 2516e12, "exact": 157.3e12}  # f16-input / f32-input MFMA, FLOP/s
PEAK_HBM = 8.0e12          # bytes / s (spec; ~6.3e12 achievable)
TILE_L2 = 16               # queries that share one pass over the rows (csrc/nann_scan.h, kScanTileQueries)
_DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def loop_a(index, scorer, q):
    for b in range(q.shape[0]):
        ops.top_k(ops.blaze_score(scorer, q[b], item_emb=index.item_embs), K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("items", nargs="?", type=int, default=1_000_000)
    ap.add_argument("dim", nargs="?", type=int, default=128)
    ap.add_argument("dtype", nargs="?", default="f16", choices=sorted(_DT))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_all_rate.txt"))
    ap.add_argument("--trace", action="store_true", help="a short run for a kernel trace: L2 at batch 1024, the MLP forms at 64")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n, d = args.items, args.dim
    embs, assign = synth.make_corpus(n, d, n_clusters=max(64, n // 4096), noise=1.0)
    if args.dtype == "f32":
        embs = embs.astype(np.float32)
    elif args.dtype == "bf16":
        embs = (embs.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    # search_all never reads the graph: a ring (every node linked to the next eight) is a valid one
    deg = 8
    nbv = ((np.arange(n, dtype=np.int64)[:, None] + 1 + np.arange(deg)) % n).astype(np.int32).reshape(-1)
    rs = np.arange(n + 1, dtype=np.int64) * deg
    index = retrieval.Index(embs, synth.make_item_ids(n), [nbv, nbv], [rs, rs], np.arange(0, n, n // 64, dtype=np.int32)[:64])
    row_bytes = d * (4 if args.dtype == "f32" else 2)
    rng = np.random.default_rng(99)
    q_all = torch.as_tensor(rng.standard_normal((4096, d)).astype(np.float32)).to(dev)
    lines = [f"search_all_rate: {n} items x {d} {args.dtype}, k = {K}, rounds = {args.rounds} (median, min..max); device "
             f"{torch.cuda.get_device_name(0)}"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def measure(pairs):
        """pairs: [(name, fn)] -> {name: [ms per round]}, the functions alternating inside a round"""
        for _, fn in pairs:  # warm every shape
            fn()
        torch.cuda.synchronize()
        out = {name: [] for name, _ in pairs}
        for _ in range(1 if args.trace else args.rounds):
            for name, fn in pairs:
                out[name].append(timed(fn))
        return out

    def fmt(ms):
        return f"{statistics.median(ms):9.3f} ms ({min(ms):.3f}..{max(ms):.3f})"

    def bound(ms, ops_count, peak_ops, req_bytes):
        t_ops, t_bytes = ops_count / peak_ops, req_bytes / PEAK_HBM
        least = max(t_ops, t_bytes)
        which = "operations" if t_ops >= t_bytes else "table bytes"
        return (f"ops {ops_count:.3e} ({t_ops * 1e3:.3f} ms at peak), table bytes requested {req_bytes:.3e} "
                f"({t_bytes * 1e3:.3f} ms at 8 TB/s); least time / measured = {least * 1e3 / statistics.median(ms):.3f}, bound by {which}")

    # ---- L2 -------------------------------------------------------------------------------------------------------------
    sc = ops.Scorer("l2", d, _DT[args.dtype])
    batches = [1024] if args.trace else [1, 64, 1024, 4096]
    pairs = [("A", lambda: loop_a(index, sc, q_all[:64]))] if not args.trace else []
    for b in batches:
        pairs.append((f"B{b}", lambda b=b: retrieval.search_all(index, sc, q_all[:b], K)))
    res = measure(pairs)
    emit("L2 scorer")
    a_per_query = None
    if "A" in res:
        a_per_query = statistics.median(res["A"]) / 64
        emit(f"  A  blaze_score + top_k loop, 64 queries: {fmt(res['A'])} = {a_per_query:.4f} ms per query")
    for b in batches:
        ms = res[f"B{b}"]
        per = statistics.median(ms) / b
        tiles = (b + TILE_L2 - 1) // TILE_L2
        line = f"  B  search_all, batch {b:5d}: {fmt(ms)} = {per:.5f} ms per query"
        if a_per_query:
            line += f" = {a_per_query / per:.1f} x A's rate"
        emit(line)
        emit("       " + bound(ms, 2.0 * b * n * d, PEAK_VEC_OPS, float(n) * row_bytes * tiles))

    # ---- MLP (16-bit rows, d <= 256) --------------------------------------------------------------------------------------
    if args.dtype != "f32" and d <= 256:
        w = synth.make_mlp_weights(d)
        flops_row = 2.0 * 256 * 128 + 2.0 * 128  # layer 2 + output layer (layer 1 is the table; the split form runs 3 MFMA products per term)
        for prec in ("split", "exact"):
            msc = ops.Scorer("mlp", d, _DT[args.dtype], w, precision=prec)
            retrieval.prepare(index, msc)
            mb = [64] if args.trace else [64, 1024]
            pairs = [("A", lambda: loop_a(index, msc, q_all[:16]))] if not args.trace else []
            for b in mb:
                pairs.append((f"B{b}", lambda b=b: retrieval.search_all(index, msc, q_all[:b], K)))
            res = measure(pairs)
            emit(f"MLP scorer, {prec} (A scores three layers from the rows with nann_score; B layer 2 on from the pre-projected table, "
                 "built and pinned outside the timed region)")
            a_per_query = None
            if "A" in res:
                a_per_query = statistics.median(res["A"]) / 16
                emit(f"  A  blaze_score + top_k loop, 16 queries: {fmt(res['A'])} = {a_per_query:.4f} ms per query")
            for b in mb:
                ms = res[f"B{b}"]
                per = statistics.median(ms) / b
                line = f"  B  search_all, batch {b:5d}: {fmt(ms)} = {per:.5f} ms per query"
                if a_per_query:
                    line += f" = {a_per_query / per:.1f} x A's rate"
                emit(line)
                emit("       " + bound(ms, flops_row * b * n, PEAK_MFMA[prec], float(n) * 1024 * b))
            retrieval.release(index, msc)
            del msc
    if not args.trace:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
