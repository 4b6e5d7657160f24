"""Shared by test_index_update_model_cpu.py and test_index_update_gpu.py: the cases at which nann_hnsw_update_device is held to the
model of hnsw_update_model.py -- the smallest that reach each path --, their masks, refreshed tables and distance matrices.
Everything is computed once per key (hnsw_build_cases' cache) and left unchanged."""
import numpy as np

import hnsw_build_cases as HC
import hnsw_build_model as HM
import hnsw_update_model as UM

NEW_SEED = 4321  # the corpus the new embeddings come from: no row of it equals a row of the seed-1234 corpus


def _rng_mask(n):
    return np.random.default_rng(11).random(n) < 0.25


def _tiny_mask(marked):
    mask = np.zeros(64, bool)
    mask[list(marked)] = True
    return mask


# name -> (base: a key of HC.BUILDS, or "n64" of HC.TINY built through the C call; the mask; whether the marked rows get new
#          embeddings; the model counters the case must reach)
CASES = {
    "l2_random": ("l2_f16_d64_m8", lambda: HC.remove_mask("l2_random"), True, ("repaired", "copied", "batches_gt1", "reselect")),
    "l2_random_kp": ("l2_f16_d64_m8_kp", lambda: HC.remove_mask("l2_random"), True, ("select_fill", "reselect")),
    "ip_random": ("ip_f16_d64_m8", lambda: HC.remove_mask("l2_random"), True, ("repaired", "copied", "neg_dist")),
    "l2_m32_kp_cluster": ("l2_f16_d64_m32_kp", lambda: HC.remove_mask("l2_m32_kp_cluster"), True, ("repaired", "pool_over_64", "batches_of_one")),
    "bf16_d128": ("l2_bf16_d128_m8_kp", lambda: _rng_mask(600), True, ("repaired",)),
    "f16_d256": ("l2_f16_d256_m16", lambda: _rng_mask(400), True, ("select_over_gpw",)),
    "taller": ("n64", lambda: _tiny_mask([10, 3, 20, 40]), True, ("taller_than_entry",)),
    "taller_alone": ("n64", lambda: _tiny_mask([10]), True, ("taller_than_entry",)),
    "all_but_one": ("n64", lambda: ~_tiny_mask([10]), True, ("batches_of_one",)),
    "relink": ("l2_f16_d64_m8", lambda: HC.remove_mask("l2_random"), False, ("repaired",)),
}
EQUIVALENT = ("l2_random", "ip_random", "bf16_d128")  # update == remove + append under the permutation (no ties in either)


def is_tiny(name):
    return CASES[name][0] in HC.TINY


def base_case(name):
    base = CASES[name][0]
    return HC.tiny_case(base) if base in HC.TINY else HC.build_case(base)


def case(name):
    """-> dict(base: the build's case, mask, rows: the table with the marked rows refreshed, dist: its distance matrix, levels,
    want) -- and d, M, keep_pruned, metric of the base"""
    def make():
        base, mask, fresh, want = CASES[name]
        c = base_case(name)
        mask = mask()
        rows = c["rows"].copy()
        n = len(rows)
        assert len(mask) == n and 0 < mask.sum() < n
        if fresh:
            rows[mask] = HC.clustered(n, c["d"], c["dtype"], seed=NEW_SEED)[0][mask]
            assert not (rows[mask] == c["rows"][mask]).all(1).any()
            dist = HC.dist(("update", name), rows, c["metric"])
        else:
            dist = c["dist"]
        return {"base": c, "mask": mask, "rows": rows, "dist": dist, "levels": c["levels"], "want": want, "d": c["d"], "M": c["M"],
                "keep_pruned": c["keep_pruned"], "metric": c["metric"], "dtype": c["dtype"]}
    return HC._cached(("update_case", name), make)


def model_base(name):
    """the base graph by the model (the CPU tests; the GPU tests start from the device's own base)"""
    c = base_case(name)
    if is_tiny(name):
        return HC._cached(("update_tiny_base", CASES[name][0]),
                          lambda: HM.build(c["dist"], c["d"], c["levels"], c["M"], HC.EF, c["keep_pruned"], c["metric"]))
    return HC.model_build(CASES[name][0])


def model_update(name, adj0, adj_up, mask=None, wrong=None):
    u = case(name)
    return UM.update(u["dist"], u["d"], u["levels"], adj0, adj_up, u["mask"] if mask is None else mask, u["M"], HC.EF,
                     u["keep_pruned"], u["metric"], wrong=wrong)


def permutation(mask):
    """survivors in order, then the marked rows in order: perm[new id] = old id, and its inverse"""
    perm = np.concatenate([np.nonzero(~mask)[0], np.nonzero(mask)[0]])
    inv = np.empty(len(perm), np.int64)
    inv[perm] = np.arange(len(perm))
    return perm, inv


def through(a, inv):
    """an array of ids (-1: empty) through old -> new"""
    return np.where(a >= 0, inv[np.maximum(a, 0)], -1).astype(np.int32)


def permuted_arrays(res, levels, mask):
    """the update's arrays (row numbers unchanged) as remove + append numbers them -> adj0, adj_up in the new numbering"""
    perm, inv = permutation(mask)
    up_old, _ = HM.up_rows_of(levels)
    lv_new = np.asarray(levels)[perm]
    up_new, n_up = HM.up_rows_of(lv_new)
    adj0 = through(res["adj0"][perm], inv)
    adj_up = np.full((max(n_up, 1), res["adj_up"].shape[1]), -1, np.int32)
    for new, old in enumerate(perm):
        for l in range(1, int(lv_new[new])):
            adj_up[up_new[new] + l - 1] = through(res["adj_up"][up_old[old] + l - 1], inv)
    return adj0, adj_up, lv_new
