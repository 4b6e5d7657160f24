#!/usr/bin/env python3
"""Refreshing rows of a built HNSW graph in place (index_build.update_hnsw_gpu) next to the two routes there were: a random
1 % and 10 % of a 1M x 128-d f16 corpus (M 32) get new embeddings (the rows at the same positions of a second corpus);
seconds of the update call, of (a) a build_hnsw_gpu of the new table and (b) remove + gather + append of the refreshed rows
(which renumbers every survivor); `stats`; recall@200 of retrieval.search (L2, ef 128, 256 queries) against retrieval.search_all
on the new table for the updated graph, the rebuilt graph and the stale graph (the old arrays over the new table).  Then the
heal: orphans (index_build.orphan_rows_gpu) after a 25 % removal, before and after update_hnsw_gpu re-inserts them.  Writes
profiles/hnsw_update_rate.txt.  No figure here is a pass criterion.
usage: tools/hnsw_update_rate.py [items] [dim] [ef]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from nann_amd import _lib, index_build, ops, retrieval, synth  # noqa: E402

M = 32
CALL = {}


def time_the_calls():
    """the C calls are synchronous: their wall time is the device work, without the Python around it"""
    L = _lib.lib()
    for name in ("nann_hnsw_build_device_metric", "nann_hnsw_remove_count", "nann_hnsw_remove_device", "nann_hnsw_append_device_metric",
                 "nann_hnsw_update_device", "nann_hnsw_orphan_bits"):
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


def recall(rows, ids, state, q, ef, k=200):
    """(recall@k against search_all on the same table, a failed request counted as zero hits; share of valid requests; mean
    level-0 degree) of the graph of `state` over `rows`"""
    ex = index_build.export_hnsw_gpu(state)
    dix = retrieval.Index(rows, ids, ex["nb_values"], ex["nb_row_splits"], ex["enter_points"])
    sc = ops.Scorer("l2", dix.d, dix.item_embs.dtype)
    r = retrieval.search(dix, sc, q, [ef] * 5 + [k])
    truth = retrieval.search_all(dix, sc, q, k)
    torch.cuda.synchronize()
    ok = (r.status == 0).cpu().numpy()
    got, want = r.index.cpu().numpy(), truth.index.cpu().numpy()
    hits = sum(len(set(got[b].tolist()) & set(want[b].tolist())) for b in range(len(got)) if ok[b])
    return hits / want.size, float(ok.mean()), ex["nb_values"][0].numel() / dix.n_items


def main():
    items = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    dim = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    ef = int(sys.argv[3]) if len(sys.argv) > 3 else 128
    ncl = bench.n_clusters_for(items, ef)
    embs, _ = synth.make_corpus(items, dim, n_clusters=ncl, noise=1.0, seed=1234, item_seed=1334)
    embs2, _ = synth.make_corpus(items, dim, n_clusters=ncl, noise=1.0, seed=1234, item_seed=4321)  # the same centres, other items
    ids = synth.make_item_ids(items, seed=1235)
    rows, rows2 = torch.as_tensor(embs).cuda(), torch.as_tensor(embs2).cuda()
    q = ops.user_seq_mean(bench.make_query_batches(dim, 256, 1, 1.0, torch.device("cuda"), n_clusters=ncl)[0])
    fmt = lambda r: f"{r[0]:.4f} / {r[1]:.3f} / {r[2]:.2f}"
    lines = [f"hnsw_update_rate: {items} x {dim} f16, M {M}, efConstruction 40; search L2 ef {ef}, recall@200 vs search_all on the same table "
             f"(a failed request has no hits), 256 queries"]
    time_the_calls()
    index_build.build_hnsw_gpu(rows[:20_000], M, 40, seed=1236)  # warm-up: module load, allocator
    base = index_build.build_hnsw_gpu(rows, M, 40, seed=1236, want_state=True)["state"]
    lines.append(f"the graph of all {items}: build call {CALL['nann_hnsw_build_device_metric']:.3f} s; recall / valid / mean L0 degree "
                 f"{fmt(recall(rows, ids, base, q, ef))}")
    index_build.update_hnsw_gpu(base, [0], want_export=False)  # warm-up of the update's kernels
    for share in (0.01, 0.10):
        marked = np.nonzero(np.random.default_rng(int(share * 1000)).random(items) < share)[0]
        at = torch.as_tensor(marked).cuda()
        new = rows2[at].contiguous()
        res, t_all = timed(lambda: index_build.update_hnsw_gpu(base, at, new, want_export=False))
        c_upd = CALL["nann_hnsw_update_device"]
        table = res["state"]["item_embs"]
        upd = recall(table, ids, res["state"], q, ef)
        stale = recall(table, ids, dict(base, item_embs=table), q, ef)
        stats = [int(s) for s in res["stats"]]
        del res
        built = index_build.build_hnsw_gpu(table, M, 40, seed=1236, want_state=True)["state"]
        c_build = CALL["nann_hnsw_build_device_metric"]
        reb = recall(table, ids, built, q, ef)
        del built

        def detour():
            r = index_build.remove_hnsw_gpu(base, remove_rows=at, want_export=False)
            return index_build.append_hnsw_gpu(r["state"], new, seed=1237, want_export=False)
        _, t_detour = timed(detour)
        c_detour = CALL["nann_hnsw_remove_count"] + CALL["nann_hnsw_remove_device"] + CALL["nann_hnsw_append_device_metric"]
        lines.append(f"refresh {len(marked)} ({share:.0%}): update call {c_upd:.3f} s ({t_all:.3f} s with the copy of the table and the bitmap); "
                     f"(a) build of the new table {c_build:.3f} s, rebuild / update = {c_build / c_upd:.1f}; (b) remove count + remove + append calls "
                     f"{c_detour:.3f} s ({t_detour:.3f} s with the gather and the concatenation; every survivor renumbered); stats {stats}")
        lines.append(f"    recall / valid / mean L0 degree: updated {fmt(upd)}; rebuilt {fmt(reb)}; stale graph, new table {fmt(stale)}")
    # ---- the heal of a removal
    removed = np.random.default_rng(250).random(items) < 0.25
    st = index_build.remove_hnsw_gpu(base, deny_bits=removed, want_export=False)
    kept_ids = ids[st["kept_rows"].cpu().numpy()]
    st = st["state"]
    before, t_orph = timed(lambda: index_build.orphan_rows_gpu(st))
    rec0 = recall(st["item_embs"], kept_ids, st, q, ef)
    healed, t_heal = timed(lambda: index_build.update_hnsw_gpu(st, before, want_export=False))
    after = index_build.orphan_rows_gpu(healed["state"])
    rec1 = recall(st["item_embs"], kept_ids, healed["state"], q, ef)
    lines.append(f"heal after removing {int(removed.sum())} (25%): {before.numel()} orphans of {len(kept_ids)} rows (orphan_bits call "
                 f"{CALL['nann_hnsw_orphan_bits'] * 1e3:.1f} ms), update call {CALL['nann_hnsw_update_device']:.3f} s ({t_heal:.3f} s in all), "
                 f"{after.numel()} orphans after; stats {[int(s) for s in healed['stats']]}")
    lines.append(f"    recall / valid / mean L0 degree: before the heal {fmt(rec0)}; after {fmt(rec1)}")
    text = "\n".join(lines)
    print(text, flush=True)
    if items == 1_000_000 and dim == 128:
        with open(os.path.join(ROOT, "profiles", "hnsw_update_rate.txt"), "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
