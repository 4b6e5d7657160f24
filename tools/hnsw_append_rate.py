#!/usr/bin/env python3
"""Appending to a built HNSW graph (index_build.append_hnsw_gpu) next to a rebuild of the same rows on the same library:
append 1 % and 10 % of a 1M x 128-d f16 corpus to a graph of the rest; seconds of the append, seconds of the full rebuild,
their ratio, and recall@200 of retrieval.search (L2, ef 128) against retrieval.search_all on the appended and on the rebuilt
graph.  Writes profiles/hnsw_append_rate.txt.  No figure here is a pass criterion.
usage: tools/hnsw_append_rate.py [items] [dim] [ef]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from nann_amd import _lib, index_build, ops, retrieval, synth  # noqa: E402


CALL = {}


def time_the_calls():
    """both C calls are synchronous: their wall time is the device work, without the Python around it (growing the arrays, the
    torch export of the returned dict)"""
    L = _lib.lib()
    for name in ("nann_hnsw_build_device_ex", "nann_hnsw_append_device"):
        def wrapped(*a, _real=getattr(L, name), _name=name):
            t = time.time()
            rc = _real(*a)
            CALL[_name] = time.time() - t
            return rc
        setattr(L, name, wrapped)


def timed(fn):
    torch.cuda.synchronize()
    t = time.time()
    out = fn()
    torch.cuda.synchronize()
    return out, time.time() - t


def recall(rows, ids, ex, q, ef, k=200):
    dix = retrieval.Index(rows, ids, ex["nb_values"], ex["nb_row_splits"], ex["enter_points"])
    sc = ops.Scorer("l2", dix.d, dix.item_embs.dtype)
    r = retrieval.search(dix, sc, q, [ef] * 5 + [k])
    truth = retrieval.search_all(dix, sc, q, k)
    torch.cuda.synchronize()
    ok = (r.status == 0).cpu().numpy()
    got, want = r.index.cpu().numpy(), truth.index.cpu().numpy()
    hits = sum(len(set(got[b].tolist()) & set(want[b].tolist())) for b in range(len(got)) if ok[b])
    return hits / max(1, int(ok.sum()) * k), float(ok.mean()), ex["nb_values"][0].numel() / dix.n_items


def main():
    items = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    dim = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    ef = int(sys.argv[3]) if len(sys.argv) > 3 else 128
    ncl = bench.n_clusters_for(items, ef)
    embs, _ = synth.make_corpus(items, dim, n_clusters=ncl, noise=1.0, seed=1234, item_seed=1334)
    ids = synth.make_item_ids(items, seed=1235)
    rows = torch.as_tensor(embs).cuda()
    q = ops.user_seq_mean(bench.make_query_batches(dim, 256, 1, 1.0, torch.device("cuda"), n_clusters=ncl)[0])
    lines = [f"hnsw_append_rate: {items} x {dim} f16, M 32, efConstruction 40; search L2 ef {ef}, recall@200 vs search_all, 256 queries"]
    time_the_calls()
    index_build.build_hnsw_gpu(rows[:20_000], 32, 40, seed=1236)  # warm-up: module load, allocator
    full, t_full = timed(lambda: index_build.build_hnsw_gpu(rows, 32, 40, seed=1236, want_state=True))
    rec_full = recall(rows, ids, index_build.export_hnsw_gpu(full["state"]), q, ef)
    c_full = CALL["nann_hnsw_build_device_ex"]
    lines.append(f"rebuild of all {items}: call {c_full:.3f} s, {t_full:.3f} s with the torch export; recall {rec_full[0]:.4f}, valid {rec_full[1]:.3f}, "
                 f"mean L0 degree {rec_full[2]:.2f}")
    del full
    for share in (0.01, 0.10):
        n_new = int(items * share)
        n_old = items - n_new
        base = index_build.build_hnsw_gpu(rows[:n_old], 32, 40, seed=1236, want_state=True)["state"]
        grown, t_app = timed(lambda: index_build.append_hnsw_gpu(base, rows[n_old:], seed=77))
        ex, t_ex = timed(lambda: index_build.export_hnsw_gpu(grown["state"]))
        rec = recall(rows, ids, ex, q, ef)
        c_app = CALL["nann_hnsw_append_device"]
        lines.append(f"append {n_new} ({share:.0%}) to {n_old}: call {c_app:.3f} s, {t_app:.3f} s with growing the arrays and the torch export, "
                     f"device export {t_ex * 1e3:.1f} ms; rebuild / append = {c_full / c_app:.1f} (calls), {t_full / t_app:.1f} (all); recall {rec[0]:.4f} "
                     f"(rebuilt {rec_full[0]:.4f}), valid {rec[1]:.3f}, mean L0 degree {rec[2]:.2f}")
        del base, grown, ex
    text = "\n".join(lines)
    print(text, flush=True)
    out = os.path.join(ROOT, "profiles", "hnsw_append_rate.txt")
    if items == 1_000_000 and dim == 128:
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
