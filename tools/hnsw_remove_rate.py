#!/usr/bin/env python3
"""Removing rows from a built HNSW graph (index_build.remove_hnsw_gpu) next to a rebuild of the survivors on the same library:
a random 1 %, 10 % and 25 % of a 1M x 128-d f16 corpus leave a graph of all of it (M 32); seconds of the two calls, seconds of a
build_hnsw_gpu of the survivors, `stats`, mean level-0 degree, and recall@200 of retrieval.search (L2, ef 128, 256 queries)
against retrieval.search_all on each index for (a) the compacted graph, (b) the rebuilt graph, (c) the old graph searched
through search(filter=, k=200) at F = the pool width, (d) a compaction that merely drops the removed entries (torch, from the
old arrays) -- so the repair's worth is a number.  Writes profiles/hnsw_remove_rate.txt.  No figure here is a pass criterion.
usage: tools/hnsw_remove_rate.py [items] [dim] [ef]"""
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
    for name in ("nann_hnsw_build_device_metric", "nann_hnsw_remove_count", "nann_hnsw_remove_device"):
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


def hits(got, want, n_got=None, n_want=None):
    return sum(len(set(got[b][:None if n_got is None else n_got[b]].tolist()) & set(want[b][:None if n_want is None else n_want[b]].tolist()))
               for b in range(len(got)))


def recall(rows, ids, ex, q, ef, k=200):
    """(recall@k against search_all on the same index, a failed request counted as zero hits; share of valid requests; mean
    level-0 degree)"""
    dix = retrieval.Index(rows, ids, ex["nb_values"], ex["nb_row_splits"], ex["enter_points"])
    sc = ops.Scorer("l2", dix.d, dix.item_embs.dtype)
    r = retrieval.search(dix, sc, q, [ef] * 5 + [k])
    truth = retrieval.search_all(dix, sc, q, k)
    torch.cuda.synchronize()
    ok = (r.status == 0).cpu().numpy()
    got, want = r.index.cpu().numpy(), truth.index.cpu().numpy()
    return hits(got[ok], want[ok]) / want.size, float(ok.mean()), ex["nb_values"][0].numel() / dix.n_items


def recall_filtered(dix, removed, q, ef, k=200):
    """the old index with the removed rows denied: search(filter=, k) at the widest useful fetch width against search_all(filter=)"""
    f = retrieval.make_filter(dix, deny_rows=np.nonzero(removed)[0])
    sc = ops.Scorer("l2", dix.d, dix.item_embs.dtype)
    topn = [ef] * 5
    width = retrieval.pool_width(topn + [0])
    r = retrieval.search(dix, sc, q, topn + [width], filter=f, k=k)
    truth = retrieval.search_all(dix, sc, q, k, filter=f)
    torch.cuda.synchronize()
    ok = (r.status == 0).cpu().numpy()
    got, want = r.index.cpu().numpy(), truth.index.cpu().numpy()
    n_got, n_want = r.n_out.cpu().numpy(), truth.n_out.cpu().numpy()
    return hits(got[ok], want[ok], n_got[ok], n_want[ok]) / max(1, int(n_want.sum())), float(ok.mean()), width


def drop_only(base, removed):
    """the compaction that merely drops removed entries and renumbers the rest, in torch from the old arrays"""
    dev = base["adj0"].device
    keep = torch.as_tensor(~removed).to(dev)
    new_id = torch.cumsum(keep.to(torch.int32), 0, dtype=torch.int32) - 1
    lv = np.asarray(base["levels"])

    def renumber(a):
        at = a.clamp(min=0).long()
        return torch.where((a < 0) | ~keep[at], torch.full_like(a, -1), new_id[at])
    owner = torch.as_tensor(np.repeat(np.arange(len(lv)), lv - 1)).to(dev)
    lvk = lv[~removed].astype(np.int64)
    up_row = np.where(lvk > 1, np.cumsum(lvk - 1) - (lvk - 1), -1).astype(np.int32)
    adj_up = renumber(base["adj_up"][:len(owner)])[keep[owner]]
    if adj_up.shape[0] == 0:
        adj_up = torch.full((1, base["M"]), -1, dtype=torch.int32, device=dev)
    return {"adj0": renumber(base["adj0"])[keep].contiguous(), "up_row": torch.as_tensor(up_row).to(dev), "adj_up": adj_up.contiguous(),
            "levels": lv[~removed].astype(np.int32), "M": base["M"]}


def main():
    items = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    dim = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    ef = int(sys.argv[3]) if len(sys.argv) > 3 else 128
    ncl = bench.n_clusters_for(items, ef)
    embs, _ = synth.make_corpus(items, dim, n_clusters=ncl, noise=1.0, seed=1234, item_seed=1334)
    ids = synth.make_item_ids(items, seed=1235)
    rows = torch.as_tensor(embs).cuda()
    q = ops.user_seq_mean(bench.make_query_batches(dim, 256, 1, 1.0, torch.device("cuda"), n_clusters=ncl)[0])
    lines = [f"hnsw_remove_rate: {items} x {dim} f16, M {M}, efConstruction 40; search L2 ef {ef}, recall@200 vs search_all on the same index "
             f"(a failed request has no hits), 256 queries"]
    time_the_calls()
    index_build.build_hnsw_gpu(rows[:20_000], M, 40, seed=1236)  # warm-up: module load, allocator
    base = index_build.build_hnsw_gpu(rows, M, 40, seed=1236, want_state=True)["state"]
    ex_old = index_build.export_hnsw_gpu(base)
    old_ix = retrieval.Index(rows, ids, ex_old["nb_values"], ex_old["nb_row_splits"], ex_old["enter_points"])
    rec = recall(rows, ids, ex_old, q, ef)
    lines.append(f"the graph of all {items}: build call {CALL['nann_hnsw_build_device_metric']:.3f} s; recall {rec[0]:.4f}, valid {rec[1]:.3f}, "
                 f"mean L0 degree {rec[2]:.2f}")
    index_build.remove_hnsw_gpu(base, remove_rows=[0], want_export=False)  # warm-up of the removal's kernels
    for share in (0.01, 0.10, 0.25):
        removed = np.random.default_rng(int(share * 1000)).random(items) < share
        res, t_all = timed(lambda: index_build.remove_hnsw_gpu(base, deny_bits=removed, want_export=False))
        c_count, c_rem = CALL["nann_hnsw_remove_count"], CALL["nann_hnsw_remove_device"]
        st = res["state"]
        kept_ids = ids[res["kept_rows"].cpu().numpy()]
        ex, t_ex = timed(lambda: index_build.export_hnsw_gpu(st))
        a = recall(st["item_embs"], kept_ids, ex, q, ef)
        built = index_build.build_hnsw_gpu(st["item_embs"], M, 40, seed=1236, want_state=True)["state"]
        c_build = CALL["nann_hnsw_build_device_metric"]
        b = recall(st["item_embs"], kept_ids, index_build.export_hnsw_gpu(built), q, ef)
        del built
        c = recall_filtered(old_ix, removed, q, ef)
        d = recall(st["item_embs"], kept_ids, index_build.export_hnsw_gpu(drop_only(base, removed)), q, ef)
        lines.append(f"remove {int(removed.sum())} ({share:.0%}): count {c_count:.3f} s + remove {c_rem:.3f} s = {c_count + c_rem:.3f} s "
                     f"({t_all:.3f} s with the bitmap and the gather of the rows), device export {t_ex * 1e3:.1f} ms; build of the {len(kept_ids)} "
                     f"survivors {c_build:.3f} s; rebuild / remove = {c_build / (c_count + c_rem):.1f}; stats {[int(s) for s in res['stats']]}")
        lines.append(f"    recall / valid / mean L0 degree: (a) compacted {a[0]:.4f} / {a[1]:.3f} / {a[2]:.2f}; (b) rebuilt {b[0]:.4f} / {b[1]:.3f} / "
                     f"{b[2]:.2f}; (c) old graph, filtered at F = {c[2]} {c[0]:.4f} / {c[1]:.3f} / {rec[2]:.2f}; (d) drop-only {d[0]:.4f} / {d[1]:.3f} "
                     f"/ {d[2]:.2f}")
        del res, st, ex
    text = "\n".join(lines)
    print(text, flush=True)
    if items == 1_000_000 and dim == 128:
        with open(os.path.join(ROOT, "profiles", "hnsw_remove_rate.txt"), "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
