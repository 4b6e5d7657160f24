"""CPU: nann_user_seq_interests as far as it can be held without a GPU -- the numpy model of the contract
(interests_model.model) against its plain Python restatement on random small users, the properties the header promises, the
symbol, the constants, the build lists, every refusal of the call (they stand in front of the first launch and so need no
device) and the header's key phrases."""
import ctypes as C
import os
import re

import numpy as np

import interests_model as IM
from nann_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARGUMENT, UNSUPPORTED = 0, 7, 102
F = np.float32


def _header():
    return open(os.path.join(ROOT, "include", "nann_hip.h")).read()


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float16)).view(np.uint16)


def _small_user(rng):
    """integer- and half-integer-valued rows drawn from a small pool (so exact duplicates and equal distances are common),
    now and then a pad row of +0 or -0 halves, now and then nothing but pad rows"""
    L, d = int(rng.integers(1, 25)), int(rng.integers(1, 10))
    pool = rng.integers(-4, 5, (int(rng.integers(1, 7)), d)).astype(np.float16) * np.float16(0.5)
    x = pool[rng.integers(0, len(pool), L)]
    if rng.random() < 0.3:
        x = x + (rng.integers(-1, 2, (L, d)) * 0.5).astype(np.float16)
    elif rng.random() < 0.5:
        x = (rng.integers(-1, 2, (L, d)) * 0.5).astype(np.float16)  # a lattice of 3^d points: equal distances everywhere
    bits = _bits(x).copy()
    pad = rng.random(L) < (1.0 if rng.random() < 0.03 else 0.15)
    bits[pad] = np.where(rng.random((int(pad.sum()), d)) < 0.5, 0x8000, 0).astype(np.uint16)
    return bits


def test_model_equals_the_restatement_on_1000_users():
    rng = np.random.default_rng(20241101)
    seen = {"seed_tie": 0, "assign_tie": 0, "few": 0, "emptied": 0, "dropped": 0, "reordered": 0, "all_pad": 0}
    for i in range(1000):
        bits = _small_user(rng)
        n_vec, n_iter = int(rng.integers(1, 7)), int(rng.integers(0, 5))
        trace = {}
        # the user stands second in a batch of two
        got = IM.model(np.stack([np.zeros_like(bits), bits]), n_vec, n_iter, trace)
        q, w, n, a = IM.restate([[np.float16(v) for v in row] for row in bits.view(np.float16)], n_vec, n_iter)
        assert int(got["n_interests"][1]) == n, i
        assert got["assign"][1].tolist() == a, i
        assert (got["q"][1].view(np.uint32) == np.array(q, F).view(np.uint32)).all(), i
        assert (got["weights"][1].view(np.uint32) == np.array(w, F).view(np.uint32)).all(), i
        assert got["n_interests"][0] == 0 and not got["q"][0].any() and (got["assign"][0] == -1).all()
        m = int((got["assign"][1] >= 0).sum())
        for key in ("seed_tie", "assign_tie", "emptied", "dropped", "reordered"):
            seen[key] += trace.get(key, 0) > 0
        seen["few"] += 0 < n < n_vec
        seen["all_pad"] += m == 0
    print(seen)
    assert all(seen[k] >= v for k, v in FLOORS.items()), seen


# About half of what the model alone counts on these 1000 users: seed_tie 537, assign_tie 153, few 281, reordered 560, all_pad
# 44.  "emptied" (a cluster without members in a Lloyd round) and "dropped" (one the final assignment leaves empty) are counted
# as well and their floor is 0: the model counts none here, nor on 570 000 further histories searched for one (integer lattices
# with heavy multiplicity in 1-2 dimensions, Gaussian rows and Gaussian clusters in 2-6).  Farthest-point seeds start every
# cluster on a row of its own, and two clusters cannot meet in one centroid: each member is strictly nearer its own centroid
# than any lower-numbered one, so the means lie strictly on their own sides.  The contract still says what happens.
FLOORS = {"seed_tie": 270, "assign_tie": 75, "few": 140, "emptied": 0, "dropped": 0, "reordered": 280, "all_pad": 22}


def _random_batch(rng, n, L, d, pad=0.2):
    x = (rng.integers(-6, 7, (n, L, d)) * 0.5).astype(np.float16)
    bits = _bits(x).copy()
    bits[rng.random((n, L)) < pad] = 0x8000
    return bits


def test_one_vector_is_the_mean_bitwise(oracle):
    rng = np.random.default_rng(5)
    for _ in range(40):
        bits = _random_batch(rng, 3, int(rng.integers(1, 20)), int(rng.integers(1, 12)))
        bits[0] = _bits(rng.standard_normal(bits[0].shape))  # and values that round
        exp = np.stack([oracle.user_seq_mean(b.view(np.float16)) for b in bits])
        for n_iter in (0, 1, 3):
            got = IM.model(bits, 1, n_iter)
            assert (got["q"][:, 0].view(np.uint32) == exp.astype(F).view(np.uint32)).all()
            live = ((bits & 0x7FFF) != 0).any(axis=2)
            assert (got["weights"][:, 0] == live.any(axis=1)).all() and (got["n_interests"] == live.any(axis=1)).all()
            assert ((got["assign"] == 0) == live).all()


def test_without_rounds_the_vectors_are_seed_rows():
    rng = np.random.default_rng(6)
    for _ in range(100):
        bits = _random_batch(rng, 1, int(rng.integers(1, 20)), int(rng.integers(1, 8)))
        n_vec = int(rng.integers(2, 7))
        got = IM.model(bits, n_vec, 0)
        rows = {tuple(r) for r in bits[0].view(np.float16).astype(F).view(np.uint32).tolist()}
        for s in range(int(got["n_interests"][0])):
            assert tuple(got["q"][0, s].view(np.uint32).tolist()) in rows


def test_weights_counts_and_padding():
    rng = np.random.default_rng(7)
    for _ in range(200):
        bits = _random_batch(rng, 2, int(rng.integers(1, 30)), int(rng.integers(1, 8)), pad=float(rng.choice([0.0, 0.3, 1.0])))
        n_vec, n_iter = int(rng.integers(1, 9)), int(rng.integers(0, 4))
        got = IM.model(bits, n_vec, n_iter)
        for u in range(2):
            n, a, w = int(got["n_interests"][u]), got["assign"][u], got["weights"][u]
            m = int((a >= 0).sum())
            assert ((a >= 0) == ((bits[u] & 0x7FFF) != 0).any(axis=1)).all()
            if m == 0:
                assert n == 0 and not w.any() and not got["q"][u].view(np.uint32).any()
                continue
            count = np.bincount(a[a >= 0], minlength=n_vec)
            assert 1 <= n <= min(n_vec, m) and (count[:n] > 0).all() and not count[n:].any()
            assert (np.diff(count[:n]) <= 0).all()                                   # descending member count
            assert (w.view(np.uint32) == (count.astype(F) / F(m)).view(np.uint32)).all()  # exactly count / m, 0 behind
            assert abs(float(w.astype(np.float64).sum()) - 1.0) <= n * 2.0 ** -24         # each share is within half an ulp
            assert (got["q"][u, n:].view(np.uint32) == got["q"][u, 0].view(np.uint32)).all()  # bit copies of slot 0


def test_a_user_does_not_depend_on_its_batch():
    rng = np.random.default_rng(8)
    bits = _random_batch(rng, 5, 12, 4)
    whole = IM.model(bits, 3, 2)
    for u in range(5):
        alone = IM.model(bits[u:u + 1], 3, 2)
        for key in whole:
            assert (whole[key][u] == alone[key][0]).all()


def test_two_tastes_by_hand():
    # rows 0, 2, 4 near (8, 0), rows 1, 3 near (-8, 0), row 5 pad: the mean lies between them, the interests on them
    x = np.array([[8, 0], [-8, 0], [8, 1], [-8, 1], [8, -1], [0, 0]], np.float16)
    got = IM.model(_bits(x)[None], 2, 2)
    assert got["n_interests"][0] == 2 and got["assign"][0].tolist() == [0, 1, 0, 1, 0, -1]
    assert got["q"][0].tolist() == [[8.0, 0.0], [-8.0, 0.5]]
    assert got["weights"][0].tolist() == [F(3) / F(5), F(2) / F(5)]
    # the same rows twice are still two tastes: the two spare slots repeat slot 0 with weight 0
    got = IM.model(_bits(np.array([[8, 0], [-8, 0], [8, 0], [0, 0], [8, 0]], np.float16))[None], 4, 2)
    assert got["n_interests"][0] == 2 and got["assign"][0].tolist() == [0, 1, 0, -1, 0]
    assert got["q"][0].tolist() == [[8.0, 0.0], [-8.0, 0.0], [8.0, 0.0], [8.0, 0.0]]
    assert got["weights"][0].tolist() == [0.75, 0.25, 0.0, 0.0]
    # the known weakness: an outlier becomes a seed, and keeps a cluster of its own
    x = np.array([[1, 0], [1, 1], [1, -1], [40, 40]], np.float16)
    got = IM.model(_bits(x)[None], 2, 3)
    assert got["assign"][0].tolist() == [0, 0, 0, 1] and got["q"][0, 1].tolist() == [40.0, 40.0]


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_exported_and_bound():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = C.CDLL(build.build())
    bound = _lib.lib()
    s = "nann_user_seq_interests"
    assert re.search(r"\bint %s\s*\(" % s, code)
    assert hasattr(lib, s) and s in _lib.SYMBOLS
    assert len(getattr(bound, s).argtypes) == 11
    assert "#define NANN_ABI_VERSION 6" in _header() and bound.nann_abi_version() == 6
    assert _header().index("int nann_user_seq_mean(") < _header().index("int nann_user_seq_interests(") < _header().index("int nann_score(")


def test_the_limits_are_the_same_everywhere():
    from nann_amd import ops
    assert re.search(r"#define NANN_INTERESTS_MAX_VEC 16\b", _header())
    assert re.search(r"#define NANN_INTERESTS_MAX_ITER 32\b", _header())
    assert _lib.INTERESTS_MAX_VEC == ops.INTERESTS_MAX_VEC == IM.MAX_VEC == 16
    assert _lib.INTERESTS_MAX_ITER == ops.INTERESTS_MAX_ITER == IM.MAX_ITER == 32
    assert "NANN_INTERESTS_MAX_VEC == 16 && NANN_INTERESTS_MAX_ITER == 32" in open(os.path.join(build.SRC_DIR, "nann_interests.h")).read()


def test_the_kernel_rides_in_the_candidate_object():
    assert "nann_interests.h" in build.DEPS
    assert len(build.UNITS) == 17
    src = open(os.path.join(build.SRC_DIR, "nann_cand_inst.hip")).read()
    assert '#include "nann_interests.h"' in src and "#define NANN_INTERESTS_IMPL" in src
    assert "-ffp-contract=off" in build.FLAGS
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = text[text.index("\n## 2. Build"):text.index("\n## 3. ")]
    assert "nann_interests.h" in section and "seventeen translation units" in section


def test_the_header_states_the_contract():
    text = _header()
    section = text[text.index("user interests: cluster a behaviour sequence"):text.index("int nann_user_seq_interests(")]
    section = " ".join(section.replace("\n *", " ").split())
    for phrase in ("The reference has no such call",
                   "Every step is a single f32 operation",
                   "no FMA contraction",
                   "a row whose d halves are all +-0 is pad",
                   "assign = -1",
                   "t = (float)x[r][k] - c[k]; acc = acc + t * t",
                   "no tree, no lanes",
                   "what nann_user_seq_mean returns for this user, bit for bit",
                   "greatest dist(r, mean), ties to the lowest r",
                   "if that greatest value is 0, seeding stops",
                   "n_seed <= min(n_vec, distinct non-pad rows)",
                   "deterministic and needs no RNG state",
                   "an outlier becomes a seed",
                   "ties to the lowest cluster number",
                   "in ascending r and one divide by (float)count",
                   "a cluster without members keeps its centroid",
                   "clusters it leaves empty are dropped",
                   "descending member count, ties to the lower cluster number",
                   "(float)count_c / (float)m",
                   "a copy of slot 0's vector with weight 0.0f",
                   "all-zero q, zero weights, n_interests = 0",
                   "with n_vec == 1, q is nann_user_seq_mean's output bit for bit for every n_iter",
                   "q holds the seed rows themselves",
                   "does not depend on its batch",
                   "NaN / inf in comm_seq are outside the contract",
                   "no host read-back",
                   "Nothing is launched and nothing is written by a refused call",
                   "then the early NANN_OK, then the null pointers",
                   "200 x 128 x 8, 50 x 256 x 16 and 600 x 16 x 4"):
        assert phrase in section, phrase
    assert "nann_user_seq_interests" in text[text.index("There is no _model form: a comm_seq is ONE user sequence"):][:400]


# ---- every refusal, without a device ---------------------------------------------------------------------------------------
def _call(L, n_users=2, seq_len=5, d=4, n_vec=3, n_iter=2, seq=1, q=1, weights=0, n_interests=0, assign=0):
    """made-up addresses: nothing is dereferenced by a refused call"""
    p = lambda v: C.c_void_p(0x10000 * v) if v else None
    return L.nann_user_seq_interests(p(seq), n_users, seq_len, d, n_vec, n_iter, p(q), p(weights), p(n_interests), p(assign), None)


def test_refusals_need_no_device():
    L = _lib.lib()
    # the sizes: BAD_ARGUMENT
    assert _call(L, n_users=-1) == BAD_ARGUMENT
    assert _call(L, seq_len=0) == BAD_ARGUMENT
    assert _call(L, seq_len=-3) == BAD_ARGUMENT
    assert _call(L, d=0) == BAD_ARGUMENT
    assert _call(L, n_vec=0) == BAD_ARGUMENT
    assert _call(L, n_iter=-1) == BAD_ARGUMENT
    assert b"bad shape" in L.nann_last_error()
    # ... ahead of their UNSUPPORTED
    assert _call(L, n_vec=17, n_iter=-1) == BAD_ARGUMENT
    assert _call(L, n_iter=33, d=0) == BAD_ARGUMENT
    assert _call(L, n_users=2 ** 31, seq_len=0) == BAD_ARGUMENT
    assert _call(L, n_vec=17) == UNSUPPORTED and b"NANN_INTERESTS_MAX_VEC" in L.nann_last_error()
    assert _call(L, n_iter=33) == UNSUPPORTED and b"NANN_INTERESTS_MAX_ITER" in L.nann_last_error()
    assert _call(L, n_users=2 ** 31) == UNSUPPORTED and b"too many users" in L.nann_last_error()
    assert _call(L, seq_len=210, d=128, n_vec=8) == UNSUPPORTED and b"LDS budget" in L.nann_last_error()
    assert _call(L, seq_len=2 ** 31 - 1, d=2 ** 31 - 1, n_vec=16) == UNSUPPORTED
    assert _call(L, seq_len=1, d=2 ** 31 - 1, n_vec=1) == UNSUPPORTED
    # ... ahead of the early NANN_OK, which stands ahead of the pointers
    assert _call(L, n_users=0, n_vec=17) == UNSUPPORTED
    assert _call(L, n_users=0, n_iter=-1) == BAD_ARGUMENT
    assert _call(L, n_users=0, seq_len=210, d=128, n_vec=8) == UNSUPPORTED
    assert _call(L, n_users=0, seq=0, q=0) == OK
    assert _call(L, n_users=0, n_vec=16, n_iter=32) == OK
    assert _call(L, n_users=0, seq_len=200, d=128, n_vec=8) == OK   # the three shapes the budget must admit
    assert _call(L, n_users=0, seq_len=50, d=256, n_vec=16) == OK
    assert _call(L, n_users=0, seq_len=600, d=16, n_vec=4) == OK
    # then the pointers
    assert _call(L, seq=0) == BAD_ARGUMENT and b"null argument" in L.nann_last_error()
    assert _call(L, q=0) == BAD_ARGUMENT
    assert _call(L, seq=0, n_vec=17) == UNSUPPORTED
