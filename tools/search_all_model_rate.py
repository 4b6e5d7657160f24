#!/usr/bin/env python3
"""Exhaustive search under the attention model: the per-user loop (A: ops.Model.forward over the whole embedding table +
ops.top_k, one user at a time -- how evaluate.test_all scores this model without model_scan) against
retrieval.search_all_model (B) at a size a user runs.  One process, every shape warmed, A and B alternating, device events
around work that ends in a synchronise; median of the rounds, min..max beside it.
For B also: the least time the hardware could take for the table bytes the algorithm requests (1 536 B x n_items per user --
every user's pass is priced, though the scan shares a block of rows between the users that are scored together) and for its
MFMAs (split form: 220 v_mfma_f32_32x32x16_f16 per 32 rows; f32 form: 608 v_mfma_f32_32x32x2_f32), that least time over the
measured one, and which of the two binds.  These are whole-call figures (per-user projection + scoring + selection + merge),
not a kernel's share of peak; kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/search_all_model_rate.py --trace` run (tracing and timing never share a run).
The model's pre-projected table is built and pinned (retrieval.prepare) BEFORE the timed region: B's figures are the steady
state of a prepared pair; A reads the embedding rows and needs no table.  Table bytes are priced at the 8 TB/s specification;
~6.3 TB/s is achievable, so "least time / measured" of a row bound by table bytes is optimistic by that ratio (x 1.27).
usage: tools/search_all_model_rate.py [items] [dim] [--rounds R] [--out FILE] [--trace]
writes profiles/search_all_model_rate.txt (or FILE) and prints the same."""
import argparse
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nann_amd import ops, retrieval, synth  # noqa: E402

K = 200
L_SEQ = 50
A_USERS = 16
PEAK_HBM = 8.0e12          # bytes / s (spec; ~6.3e12 achievable)
TABLE_ROW_BYTES = 1536     # 384 f32 per item (csrc/nann_attn_proj.h)
# per 32 rows: (MFMAs, FLOP per MFMA, peak FLOP/s of that instruction)
MFMA = {"split": (220, 2 * 32 * 32 * 16, 2516e12), "exact": (608, 2 * 32 * 32 * 2, 157.3e12)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def loop_a(index, model, seqs):
    for u in range(seqs.shape[0]):
        ops.top_k(model.forward(seqs[u][None], index.item_embs).reshape(-1), K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("items", nargs="?", type=int, default=1_000_000)
    ap.add_argument("dim", nargs="?", type=int, default=128, choices=[64, 128])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_all_model_rate.txt"))
    ap.add_argument("--trace", action="store_true", help="a short run for a kernel trace: B at batch 64, both precisions, once")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n, d = args.items, args.dim
    embs, assign = synth.make_corpus(n, d, n_clusters=max(64, n // 4096), noise=1.0)
    # the scan never reads the graph: a ring (every node linked to the next eight) is a valid one
    deg = 8
    nbv = ((np.arange(n, dtype=np.int64)[:, None] + 1 + np.arange(deg)) % n).astype(np.int32).reshape(-1)
    rs = np.arange(n + 1, dtype=np.int64) * deg
    index = retrieval.Index(embs, synth.make_item_ids(n), [nbv, nbv], [rs, rs], np.arange(0, n, max(n // 64, 1), dtype=np.int32)[:64])
    seqs = synth.make_queries(embs[:min(n, 200_000)], assign[:min(n, 200_000)], 512, seq_len=L_SEQ, seed=99)
    seqs = torch.as_tensor(np.ascontiguousarray(seqs[:, :, :64])).to(dev)  # the model's sequence is [L, 64]
    w = synth.make_attn_weights(d, 64)
    lines = [f"search_all_model_rate: attention + DNN 128-64-32-1 model, {n} items x {d} f16, k = {K}, rounds = {args.rounds} "
             f"(median, min..max); device {torch.cuda.get_device_name(0)}"]

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
        return f"{statistics.median(ms):10.3f} ms ({min(ms):.3f}..{max(ms):.3f})"

    def bound(ms, prec, b):
        per32, flop, peak = MFMA[prec]
        t_ops = (n / 32.0) * per32 * flop * b / peak
        t_bytes = float(n) * TABLE_ROW_BYTES * b / PEAK_HBM
        least = max(t_ops, t_bytes)
        which = "MFMAs" if t_ops >= t_bytes else "table bytes"
        return (f"MFMAs {per32} per 32 rows ({t_ops * 1e3:.3f} ms at peak), table bytes requested {float(n) * TABLE_ROW_BYTES * b:.3e} "
                f"({t_bytes * 1e3:.3f} ms at 8 TB/s; ~6.3 TB/s is achievable: x 1.27); least time / measured = "
                f"{least * 1e3 / statistics.median(ms):.3f}, bound by {which}")

    batches = [64] if args.trace else [1, 64, 512]
    with tempfile.TemporaryDirectory() as tmp:
        for prec in ("split", "exact"):
            path = os.path.join(tmp, prec)
            ops.save_scorer_dir(path, "attention", w, precision=prec)
            model = ops.Model(path, d, L_SEQ)
            retrieval.prepare(index, model)
            pairs = [("A", lambda: loop_a(index, model, seqs[:A_USERS]))] if not args.trace else []
            for b in batches:
                pairs.append((f"B{b}", lambda b=b: retrieval.search_all_model(index, model, seqs[:b], K)))
            res = measure(pairs)
            emit(f"attention model, {prec} (A scores every layer from the embedding rows, user by user; B scans the pre-projected "
                 "table, built and pinned outside the timed region)")
            a_per_user = None
            if "A" in res:
                a_per_user = statistics.median(res["A"]) / A_USERS
                emit(f"  A  Model.forward + top_k loop, {A_USERS} users: {fmt(res['A'])} = {a_per_user:.4f} ms per user")
            for b in batches:
                ms = res[f"B{b}"]
                per = statistics.median(ms) / b
                line = f"  B  search_all_model, batch {b:4d}: {fmt(ms)} = {per:.5f} ms per user"
                if a_per_user:
                    line += f" = {a_per_user / per:.1f} x A's rate"
                emit(line)
                emit("       " + bound(ms, prec, b))
            retrieval.release(index, model)
            del model
    if not args.trace:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
