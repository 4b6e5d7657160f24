"""Shared by test_index_build_model_cpu.py and test_index_build_exact_gpu.py: the cases at which the device builder's arrays
are held to the model of hnsw_build_model.py -- the smallest shapes that reach each path --, their corpora, levels, distance
matrices and the coverage counters each case has to reach.  Everything is computed once per key and left unchanged."""
import ctypes as C

import numpy as np

import hnsw_build_model as HM
import ip_reference as R

EF = 40
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def drawn_levels(n, m, seed):
    """nann_hnsw_draw_levels: a host function of the library, it needs no device"""
    from nann_amd import _lib
    lv = np.zeros(n, np.int32)
    assert _lib.lib().nann_hnsw_draw_levels(C.c_int64(n), C.c_int32(m), C.c_uint64(seed), C.c_void_p(lv.ctypes.data), None) == 0
    return lv


def clustered(n, d, dtype="f16", spread=False, seed=1234):
    """n rows in 16 clusters: an f16 array, or bf16 bit patterns (uint16); spread: row norms vary by 16x.  -> rows, cluster ids"""
    def make():
        from nann_amd import synth
        x, assign = synth.make_corpus(n, d, n_clusters=16, noise=1.0, seed=seed)
        x = x.astype(np.float32)
        if spread:
            x = R.scaled_rows(x, 7)
        return (R.to_bf16_bits(x) if dtype == "bf16" else x.astype(np.float16)), assign
    return _cached(("clustered", n, d, dtype, spread, seed), make)


def grid(n, d=64, seed=3):
    """rows on the integer grid [-3, 3]^4 in the first 4 dims, zero elsewhere; the last third are copies of earlier rows, and the
    whole is shuffled.  Exact in f16 and f32: distances are small integers, so ties and zeros are exact."""
    def make():
        rng = np.random.default_rng(seed)
        x = np.zeros((n, d), np.float16)
        first = n - n // 3
        x[:first, :4] = rng.integers(-3, 4, (first, 4))
        x[first:] = x[rng.integers(0, first, n - first)]
        return x[rng.permutation(n)]
    return _cached(("grid", n, d, seed), make)


def line(xs, d=64):
    """rows e_i = (x_i, 0, ...): small integers, exact in f16 and f32"""
    x = np.zeros((len(xs), d), np.float16)
    x[:, 0] = xs
    return x


def dist(rows_key, rows, metric):
    """the distance matrix of a corpus as nested lists (what the model indexes), once per (corpus, metric)"""
    return _cached(("dist", rows_key, metric), lambda: HM.distance_matrix(rows, metric).tolist())


# ---- builds with drawn levels: name -> (n, d, dtype, M, keep_pruned, metric, spread, level seed, counters the case must reach)
BUILDS = {
    "l2_f16_d64_m4": (1000, 64, "f16", 4, False, "l2", False, 5, ("levels_ge3", "reselect", "batches_gt1")),
    "l2_bf16_d128_m8_kp": (600, 128, "bf16", 8, True, "l2", False, 5, ("select_over_gpw", "select_fill", "reselect")),
    "l2_f16_d256_m16": (400, 256, "f16", 16, False, "l2", False, 5, ("select_over_gpw",)),
    "l2_f16_d64_m32_kp": (600, 64, "f16", 32, True, "l2", False, 5, ("reselect_cap64", "select_fill")),
    "ip_bf16_d64_m8_spread": (600, 64, "bf16", 8, False, "ip", True, 5, ("neg_dist", "pos_dist", "reselect")),
    "ip_f16_d256_m4": (300, 256, "f16", 4, False, "ip", False, 5, ("select_over_gpw", "neg_dist", "pos_dist")),
    "tie_l2": (300, 64, "f16", 4, False, "l2", False, 5, ("ties", "zero_dist")),
    "tie_ip": (300, 64, "f16", 4, False, "ip", False, 5, ("ties", "zero_dist", "neg_dist", "pos_dist")),
    # the bases of the append and remove cases
    "l2_f16_d64_m8": (600, 64, "f16", 8, False, "l2", False, 5, ()),
    "l2_f16_d64_m8_kp": (600, 64, "f16", 8, True, "l2", False, 5, ()),
    "ip_f16_d64_m8": (600, 64, "f16", 8, False, "ip", False, 5, ()),
    "ip_f16_d64_m8_kp": (600, 64, "f16", 8, True, "ip", False, 5, ()),
}


def build_case(name):
    """-> dict(rows, d, dtype, M, keep_pruned, metric, levels, dist, seed, want)"""
    def make():
        n, d, dtype, m, kp, metric, spread, seed, want = BUILDS[name]
        if name.startswith("tie"):
            rows, key = grid(n, d), ("grid", n, d)
        else:
            rows, key = clustered(n, d, dtype, spread)[0], ("clustered", n, d, dtype, spread)
        return {"rows": rows, "d": d, "dtype": dtype, "M": m, "keep_pruned": kp, "metric": metric, "seed": seed,
                "levels": drawn_levels(n, m, seed), "dist": dist(key, rows, metric), "want": want}
    return _cached(("build_case", name), make)


def model_build(name, mutant=None):
    def make():
        c = build_case(name)
        return HM.build(c["dist"], c["d"], c["levels"], c["M"], EF, c["keep_pruned"], c["metric"], mutant)
    return _cached(("model_build", name, mutant), make)


# ---- levels of the test's choosing through the C call: name -> levels (rows: clustered f16, d 64, M 4, L2)
TINY = {
    "n1": [2],
    "n2": [1, 1],
    "n5": [1, 2, 1, 3, 1],
    "n9": [1, 1, 2, 1, 1, 1, 3, 2, 1],
    "n64": [2] * 10 + [4] + [2] * 53,   # order[0] = node 10 with 4 levels, every other node with 2
}
TINY_M = 4


def tiny_case(name):
    def make():
        levels = np.array(TINY[name], np.int32)
        rows = clustered(64, 64)[0][:len(levels)]
        return {"rows": rows, "d": 64, "dtype": "f16", "M": TINY_M, "keep_pruned": False, "metric": "l2", "levels": levels,
                "dist": dist(("clustered", 64, 64, "f16", False), clustered(64, 64)[0], "l2"), "want": ()}
    return _cached(("tiny_case", name), make)


# ---- appends with drawn levels: name -> (rows of, d, dtype, M, metric, n_old, build seed, append seed)
APPENDS = {
    "l2_d64_m8": (64, "f16", 8, "l2", 400, 5, 7),
    "ip_d128_m8": (128, "f16", 8, "ip", 400, 5, 7),
}
APPEND_N = 600


def append_case(name):
    """400 rows built, 200 appended: levels = the build's draw, then the append's"""
    def make():
        d, dtype, m, metric, n_old, seed, seed2 = APPENDS[name]
        rows = clustered(APPEND_N, d, dtype)[0]
        levels = np.concatenate([drawn_levels(n_old, m, seed), drawn_levels(APPEND_N - n_old, m, seed2)])
        return {"rows": rows, "d": d, "dtype": dtype, "M": m, "keep_pruned": False, "metric": metric, "n_old": n_old, "levels": levels,
                "seed": seed, "seed2": seed2, "dist": dist(("clustered", APPEND_N, d, dtype, False), rows, metric),
                "want": ("batches_gt1",)}
    return _cached(("append_case", name), make)


def taller_case():
    """40 nodes of at most 2 levels; then one new node with 4 levels -- more than the entry point's --, followed by ordinary
    nodes: two of 3 levels (rows on a level only the taller node has), some of 2, the rest of 1"""
    def make():
        rows = clustered(64, 64)[0]
        old = [1] * 40
        old[3] = old[17] = old[30] = 2
        new = [1, 2, 1, 4, 1, 3, 1, 1, 2, 1, 3, 1, 1, 1, 2, 1, 1, 1, 1, 1, 1, 2, 1, 1]
        return {"rows": rows, "d": 64, "dtype": "f16", "M": TINY_M, "keep_pruned": False, "metric": "l2", "n_old": 40,
                "levels": np.array(old + new, np.int32), "dist": dist(("clustered", 64, 64, "f16", False), rows, "l2"),
                "want": ("taller_than_entry",)}
    return _cached(("taller_case",), make)


def model_append(c, adj0, adj_up, mutant=None):
    return HM.append(c["dist"], c["d"], c["levels"], c["n_old"], adj0, adj_up, c["M"], EF, c["keep_pruned"], c["metric"], mutant)


# ---- removals: name -> (the build it starts from, what leaves, counters)
REMOVES = {
    "l2_random": ("l2_f16_d64_m8", "random", ("repaired", "copied")),
    "l2_random_kp": ("l2_f16_d64_m8_kp", "random", ("repaired", "copied", "select_fill")),
    "ip_random": ("ip_f16_d64_m8", "random", ("repaired", "copied")),
    "ip_random_kp": ("ip_f16_d64_m8_kp", "random", ("repaired", "copied", "select_fill")),
    "l2_m32_kp_cluster": ("l2_f16_d64_m32_kp", "cluster", ("repaired", "pool_over_64")),
}


def remove_mask(name):
    base, what, _ = REMOVES[name]
    n, d, dtype, _, _, _, spread, _, _ = BUILDS[base]
    if what == "random":
        return np.random.default_rng(11).random(n) < 0.25
    return clustered(n, d, dtype, spread)[1] == 3  # one of the corpus' 16 clusters: neighbours leave together


def model_remove(name, adj0, adj_up, mutant=None):
    c = build_case(REMOVES[name][0])
    return HM.remove(c["dist"], c["d"], c["levels"], adj0, adj_up, remove_mask(name), c["M"], c["keep_pruned"], c["metric"], mutant)


def check_arrays(levels, adj0, up_row, adj_up, m, connected=True):
    """the structural rules tests/test_index_build_gpu.py::_check_export asks of a build, asked of the three arrays, every level"""
    levels = np.asarray(levels)
    n = len(levels)
    want_up, n_up = HM.up_rows_of(levels)
    assert adj0.shape == (n, 2 * m) and adj_up.shape == (max(n_up, 1), m) and (up_row == want_up).all()
    for i in range(n):
        for l in range(int(levels[i])):
            r = adj0[i] if l == 0 else adj_up[up_row[i] + l - 1]
            used = r[r >= 0]
            assert (r[:len(used)] >= 0).all() and (r[len(used):] == -1).all(), "a row is a dense prefix"
            assert used.max(initial=0) < n and (used != i).all(), "ids in range, no self loop"
            assert len(set(used.tolist())) == len(used), "a link twice in one row"
            assert (levels[used] > l).all(), "a link to a node that is absent on this level"
    if connected and n > 1:
        assert ((adj0 >= 0).sum(1) > 0).all(), "a node without neighbours"
