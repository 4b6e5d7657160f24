"""GPU: the coarse quantiser (nann_kmeans_assign, nann_kmeans_train; retrieval.kmeans_assign, kmeans_train,
train_partition(method="device")) against float64 numpy: argmin of |x - c|^2 and a plain Lloyd loop.  Exact where every product and
sum is exact in f32; elsewhere within the bounds DESIGN.md 4.28 derives, computed here from d and the norms."""
import numpy as np
import pytest
import torch

from gpu_util import cuda, require_gpu
from test_sq8_gpu import _index, _scorer

pytestmark = pytest.mark.gpu
U = 2.0 ** -24  # the unit roundoff of f32
DTYPES = ("f16", "bf16")
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _to(x, dtype):
    """f16 values, or bf16 bit patterns (truncated)"""
    return x.astype(np.float16) if dtype == "f16" else (x.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def _widen(b):
    return (b if b.dtype == np.float16 else (b.astype(np.uint32) << 16).view(np.float32)).astype(np.float64)


def _case(key, make):
    """(rows as the index holds them in f64, device index) of a test's rows -- made once"""
    if key not in _CACHE:
        b = make()
        _CACHE[key] = (_widen(b), _index(b))
    return _CACHE[key]


def _dist(x, c):
    """float64 |x - c|^2, [n, n_lists]"""
    return ((x[:, None, :] - c[None, :, :]) ** 2).sum(2) if x.shape[0] * c.shape[0] * x.shape[1] < 5e7 else \
        (x * x).sum(1)[:, None] - 2.0 * x @ c.T + (c * c).sum(1)[None, :]


def _assign(dix, cent, rows=None):
    from nann_amd import retrieval
    lst, dist = retrieval.kmeans_assign(dix, cuda(cent, torch.float32), rows)
    torch.cuda.synchronize()
    return lst.cpu().numpy(), dist.cpu().numpy()


def _train(dix, seeds, n_iter):
    from nann_amd import retrieval
    cent = cuda(seeds, torch.float32).contiguous()
    out = retrieval.kmeans_train(dix, cent, n_iter)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (cent,) + tuple(out)]


def _score_bound(nx, nc, d, dtype):
    """|computed (|c|^2 - 2 <x, c>) - true| <= this, [n, n_lists] from the norms: the split's truncation tau (and the
    f16 subnormal step of lo), T d + T additions inside the MFMAs at 2^-23 each, |c|^2 over d + 1 roundings, the subtraction."""
    T, tau, sub = (2, 2.0 ** -22, 2.0 ** -25) if dtype == "f16" else (3, 2.0 ** -27, 0.0)
    dot = (1.01 * T * (d + 1) * 2.0 ** -23 + tau) * nx[:, None] * nc[None, :] + sub * np.sqrt(d) * nx[:, None]
    return 2.0 * dot + 1.01 * (d + 2) * U * nc[None, :] ** 2 + 2.0 * U * nx[:, None] * nc[None, :]


def _dist_bound(nx, nc, d, dtype):
    """... and of out_dist: |x|^2 over d + 1 roundings and the last addition on top"""
    return _score_bound(nx, nc, d, dtype) + 1.01 * (d + 2) * U * nx[:, None] ** 2 + U * (nx[:, None] + nc[None, :]) ** 2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [64, 512])
@pytest.mark.parametrize("n_lists", [1, 33, 300])
def test_exact_assignment_on_integers(dtype, d, n_lists):
    """1 000 rows (not a whole number of row tiles) and centroids in [-3, 3]^d: every product, sum and split is exact in f32, so
    the lists and the distances are float64's, ties to the lower number; n_lists below one MFMA tile, just past one, several
    LDS tiles with a ragged tail.  A window that starts and ends inside a tile gives the same answers."""
    x, dix = _case(("int", d, dtype), lambda: _to(np.random.default_rng(d).integers(-3, 4, (1000, d)).astype(np.float32), dtype))
    cent = np.random.default_rng(n_lists).integers(-3, 4, (n_lists, d)).astype(np.float32)
    cent[0] = x[7]                         # rows 7 and 500 sit on centroid 0 ...
    x500 = x[500].astype(np.float32)
    if n_lists > 1:
        cent[n_lists - 1] = cent[0]        # ... and on its twin at the highest number
        cent[n_lists // 2] = x500
        cent[1] = x500                     # (a twin pair the other way round: low number written last)
    want = _dist(x, cent.astype(np.float64))
    lst, dist = _assign(dix, cent)
    assert np.array_equal(lst, want.argmin(1))
    assert np.array_equal(dist, want.min(1).astype(np.float32))
    assert lst[7] == 0 and dist[7] == 0.0
    w_lst, w_dist = _assign(dix, cent, (37, 901))
    assert np.array_equal(w_lst, lst[37:901]) and np.array_equal(w_dist, dist[37:901])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [64, 256])
def test_the_lowest_split_term_decides(dtype, d):
    """Pairs of centroids A, B that differ ONLY in the lowest split term (f16: lo, bf16: the third term), on a support of 4
    elements of their own, zero elsewhere: B = A + delta sign(A).  A row g sign(A) on that support is nearer to B by
    (8 g - 2 sum|A|) delta - 4 delta^2, although |B| > |A|.  Without the term (or with it at a wrong place in the fragment) the
    MFMA operands of A and B are the same and |c|^2 decides for A.  The centroids are k 2^-bits with 2^(bits-1) <= k: every
    product and partial sum of the dot product is a multiple of 2^-bits below 2^(24-bits), exact in f32; what is rounded is
    |c|^2 (<= 4: 8 operations) and the subtraction (|s| <= 36 < 64), for both centroids less than 2^-24 (2 * 32 + 2 * 64), which the
    margin is asserted to exceed 8 times.  The supports cover every element, so every k-step's fragment is read.  No tolerance."""
    bits, g, step = (22, 1, 512) if dtype == "f16" else (20, 6, 3)
    rng = np.random.default_rng(d)
    n_pairs = d // 4
    if dtype == "f16":  # 11 bits of hi in [0.5, 0.625), lo = 256 2^-22 (a normal f16); B: lo = 768 2^-22, still below half an ulp of hi
        k = rng.integers(1024, 1280, (n_pairs, 4)) * 2048 + 256
    else:               # 8 bits of hi in [0.5, 0.625), a mid of 8 bits whose ulp is 8 (below half an ulp of hi); B: a third term of 3 2^-20
        k = rng.integers(128, 160, (n_pairs, 4)) * 4096 + rng.integers(128, 256, (n_pairs, 4)) * 8
    sign = rng.choice([-1.0, 1.0], (n_pairs, 4))
    cent = np.zeros((2 * n_pairs, d), np.float32)
    x = np.zeros((2 * n_pairs, d), np.float32)  # rows p and n_pairs + p: the row of pair p (an index has at least as many rows as lists)
    b_at = np.arange(n_pairs) % 2  # B at the lower number of the pair, then at the higher
    for p in range(n_pairs):
        cent[2 * p + 1 - b_at[p], 4 * p:4 * p + 4] = sign[p] * k[p] * 2.0 ** -bits
        cent[2 * p + b_at[p], 4 * p:4 * p + 4] = sign[p] * (k[p] + step) * 2.0 ** -bits
        x[p, 4 * p:4 * p + 4] = g * sign[p]
        x[n_pairs + p] = x[p]
    assert np.array_equal(cent.astype(np.float64), cent) and (np.abs(x).sum(1) * (k + step).max() <= 2 ** 24).all()
    want = _dist(x.astype(np.float64), cent.astype(np.float64))
    two = np.sort(want, 1)[:, :2]
    assert np.array_equal(want.argmin(1), np.tile(2 * np.arange(n_pairs) + b_at, 2)) and (two[:, 1] - two[:, 0] > 8 * U * 192).all()
    _, dix = _case(("split", d, dtype), lambda: _to(x, dtype))
    lst, _ = _assign(dix, cent)
    assert np.array_equal(lst, want.argmin(1))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [64, 256])
def test_assignment_with_real_mantissas(dtype, d):
    """Gaussian rows, 257 centroids that are f32 means of 8 rows each (hi, lo and the third bf16 term all non-zero): the assigned
    centroid is within the derived bound of the float64 minimum, and out_dist within its bound of the float64 distance.  (A
    worst-case bound cannot see a dropped lowest term on such data except for f16 at d = 64: that is
    test_the_lowest_split_term_decides' work)"""
    x, dix = _case(("gauss", d, dtype), lambda: _to(np.random.default_rng(d + 1).standard_normal((2000, d)), dtype))
    pick = np.random.default_rng(d + 2).integers(0, 2000, (257, 8))
    cent = x.astype(np.float32)[pick].mean(1, dtype=np.float32)
    c64 = cent.astype(np.float64)
    lst, dist = _assign(dix, cent)
    want = _dist(x, c64)
    nx, nc, r = np.sqrt((x * x).sum(1)), np.sqrt((c64 * c64).sum(1)), np.arange(2000)
    e_score, e_dist = _score_bound(nx, nc, d, dtype), _dist_bound(nx, nc, d, dtype)
    excess = want[r, lst] - want.min(1)
    print("largest excess over its bound:", (excess / (e_score[r, lst] + e_score[r, want.argmin(1)])).max(),
          "largest distance error over its bound:", (np.abs(dist - want[r, lst]) / e_dist[r, lst]).max())
    assert (excess <= e_score[r, lst] + e_score[r, want.argmin(1)]).all()
    assert (np.abs(dist - want[r, lst]) <= e_dist[r, lst]).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_update_is_exact_on_integers(dtype):
    """one round on integer rows: the sums are exact in any order, so a centroid is f32(sum) / f32(count) bit for bit; list 0
    holds about 70 % of 5 000 rows (four segments), a seed far from every row keeps its bits and a count of 0"""
    rng = np.random.default_rng(5)
    pat = rng.choice([-2.0, 2.0], (6, 64))
    label = np.where(rng.random(5000) < 0.7, 0, rng.integers(1, 6, 5000))
    x, dix = _case(("update", dtype), lambda: _to(pat[label] + rng.integers(-1, 2, (5000, 64)), dtype))
    seeds = np.concatenate([pat, np.full((1, 64), 100.0)]).astype(np.float32)
    first = _dist(x, seeds.astype(np.float64)).argmin(1)
    count = np.bincount(first, minlength=7)
    assert count[0] > 3 * 1024 and count[6] == 0
    want = seeds.copy()
    for l in range(6):
        want[l] = x[first == l].sum(0).astype(np.float32) / np.float32(count[l])
    cent, lst, counts, inertia = _train(dix, seeds, 1)
    assert np.array_equal(cent.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(lst, _dist(x, want.astype(np.float64)).argmin(1))
    assert np.array_equal(counts, np.bincount(lst, minlength=7)) and counts[6] == 0
    assert inertia.shape == (2,) and inertia[0] == _dist(x, seeds.astype(np.float64)).min(1).sum()


@pytest.mark.parametrize("dtype", DTYPES)
def test_training_on_planted_clusters(dtype):
    """8 blobs 20 noise scales apart and more, seeds one row per blob, 5 rounds: the float64 Lloyd loop's margins exceed the
    assignment bound at every row and round (asserted: a condition on the inputs), so the lists are float64's; the centroids
    and the inertia are within the rounding bounds of float64's; a second call returns the same bits"""
    d, n, k, n_iter = 64, 4000, 8, 5
    rng = np.random.default_rng(9)
    centres = rng.standard_normal((k, d)) * 20.0 / np.sqrt(2.0)  # (pairwise distance ~ 20 sqrt(d): far beyond 20 noise scales)
    blob = np.arange(n) % k
    x, dix = _case(("blobs", dtype), lambda: _to(centres[blob] + rng.standard_normal((n, d)), dtype))
    assert min(np.linalg.norm(centres[i] - centres[j]) for i in range(k) for j in range(i)) >= 20.0
    seeds = x[:k].astype(np.float32)
    nx = np.sqrt((x * x).sum(1))
    c, lists, inertia64 = seeds.astype(np.float64), [], []
    for it in range(n_iter + 1):
        dist = _dist(x, c)
        two = np.sort(dist, 1)[:, :2]
        assert (two[:, 1] - two[:, 0] > 2.0 * _score_bound(nx, np.sqrt((c * c).sum(1)), d, dtype).max(1)).all()
        lists.append(dist.argmin(1))
        inertia64.append(dist.min(1).sum())
        if it < n_iter:
            c = np.stack([x[lists[-1] == l].mean(0) for l in range(k)])
    cent, lst, counts, inertia = _train(dix, seeds, n_iter)
    assert np.array_equal(lst, lists[-1]) and np.array_equal(counts, np.bincount(lst, minlength=k))
    # a mean of m rows in f32: m - 1 additions in some order and one division -> m u of the mean of |x_e| (1.01: second order)
    m = counts.max()
    e_mean = 1.01 * m * U * np.stack([np.abs(x[lst == l]).mean(0) for l in range(k)])
    assert (np.abs(cent - c) <= e_mean).all()
    # a row's distance: its own bound, and the centroid's error through 2 |x - c| |dc| + |dc|^2
    dc = np.sqrt((e_mean ** 2).sum(1)).max()
    nc = np.sqrt((c * c).sum(1))
    e_in = (_dist_bound(nx, nc, d, dtype).max(1) + 2.0 * np.sqrt(_dist(x, c).min(1)) * dc + dc * dc).sum()
    print("inertia", inertia, "float64", inertia64, "bound", e_in)
    assert inertia.shape == (n_iter + 1,) and (np.diff(inertia) <= e_in).all() and abs(inertia[-1] - inertia64[-1]) <= e_in
    again = _train(dix, seeds, n_iter)
    for a, b in zip((cent, lst, counts, inertia), again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_through_the_public_interface():
    """train_partition(method="device"): the partition's lists hold exactly the rows kmeans_assign gives each centroid, and probing
    every list returns search_all's items"""
    from nann_amd import retrieval
    x, dix = _case(("public",), lambda: _to(np.random.default_rng(3).standard_normal((3000, 64)), "f16"))
    part, cent = retrieval.train_partition(dix, 16, iters=3, seed=1, method="device")
    lst, _ = _assign(dix, cent.cpu().numpy())
    splits, rows = part.list_splits().cpu().numpy(), part.list_rows().cpu().numpy()
    assert part.n_listed_rows == 3000
    for l in range(16):
        assert np.array_equal(rows[splits[l]:splits[l + 1]], np.flatnonzero(lst == l))
    q = cuda(np.random.default_rng(4).standard_normal((20, 64)), torch.float32)
    sc = _scorer("l2", 64)
    got = retrieval.search_partitioned(dix, part, cent, sc, q, 10, n_probe=16)
    want = retrieval.search_all(dix, sc, q, 10)
    torch.cuda.synchronize()
    assert np.array_equal(got.item_ids.cpu().numpy(), want.item_ids.cpu().numpy())
