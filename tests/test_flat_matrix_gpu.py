"""-m gpu: every compiled kernel of the flat L2 / inner-product scorers against references that are not the device.

The vector scorers behind nann_score, nann_search_all*, nann_search_candidates* and nann_mmr_topk compile to the 96 kernels of
KERNELS below: the stand-alone scorer, the exhaustive scan and the candidate-list scorer, each per (lanes per row, row dtype)
under both metrics, and k_mmr per (lanes per row, row dtype, similarity).  Each is a code object of its own with its own
register allocation, so each is launched here: 12 cases (d, row dtype), each under both metrics through the four launch kinds
of LAUNCHES and the public Python calls (ops.blaze_score, retrieval.search_all, retrieval.search_candidates, retrieval.mmr).
test_flat_matrix_cpu.py holds KERNELS to the build's own list of kernels and the launches to KERNELS.

The workload and both references are flat_matrix.py's: reference A, the canonical order of DESIGN.md 2 in numpy with a correctly
rounded fma -- every device score equals it BIT FOR BIT, the edge block of signed zeros, subnormals, the largest finite f16 and
planted ties included -- and reference B, float64 with a derived bound that every device score lies within and that decides
the row sets of the queries reference A is not computed for.  The MMR outputs equal mmr_model.model bit for bit on both sides
of the boundary between its LDS path and its table path.

Measured on an MI355X: 96 kernels entered (8 per case), none disagreed with reference A in any bit; the largest
|device - float64| / bound over every score of the 12 cases is 0.218 under L2 and 0.236 under the inner product (reference A's
own figures, as the bits are equal); a case takes 0.33 - 0.87 s up to d = 256 and 1.56 - 1.63 s at d = 512, of which 0.26 - 0.82 s
and 1.50 - 1.57 s are the CPU references (cached per module) and 0.06 s the device launches and their checks (0.38 s in the
module's first case).  A case prints its own figures (pytest -s)."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import flat_matrix as W
import ip_reference as R
from gpu_util import bits, cuda, require_gpu

pytestmark = pytest.mark.gpu

LPR = {d: d // 8 for d in W.DIMS}                  # lanes per row
DT = {"f16": 0, "bf16": 1, "f32": 2}               # DT_F16, DT_BF16, DT_F32
MT = {"l2": 0, "ip": 1}                            # MT_L2, MT_IP
TQ = W.SCAN_TILE                                   # the third template argument of the scans: kScanTileQueries

# every kernel the flat scorers' dispatch can reach, template arguments in order
KERNELS = tuple(
    [("k_score_%s" % m, lpr, dt) for m in MT for lpr in LPR.values() for dt in DT.values()] +              # 12 + 12
    [("k_scan_%s" % m, lpr, dt, TQ) for m in MT for lpr in LPR.values() for dt in DT.values()] +           # 12 + 12
    [("k_cand_score_%s" % m, lpr, dt) for m in MT for lpr in LPR.values() for dt in DT.values()] +         # 12 + 12
    [("k_mmr", lpr, dt, mt) for lpr in LPR.values() for dt in DT.values() for mt in MT.values()])          # 24

# the launch kinds of one (case, metric), in the order they run (the lists compare their bits with the scan's)
LAUNCHES = ("score", "scan", "lists", "mmr")
# the untemplated kernels a launch enters besides (the scan's transpose, slab top-k and merge; the lists' plan and top-k)
SHARED = {"score": (), "scan": ("k_scan_transpose_q", "k_scan_slab_topk", "k_scan_merge"), "lists": ("k_cand_plan", "k_cand_topk"), "mmr": ()}


def claimed(d, dtype, metric, launch):
    """the KERNELS entries a launch of this case under this metric enters"""
    if launch == "score":
        return [("k_score_%s" % metric, LPR[d], DT[dtype])]
    if launch == "scan":
        return [("k_scan_%s" % metric, LPR[d], DT[dtype], TQ)]
    if launch == "lists":
        return [("k_cand_score_%s" % metric, LPR[d], DT[dtype])]
    assert launch == "mmr"
    return [("k_mmr", LPR[d], DT[dtype], MT[metric])]


_TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
_CACHE = {}
# the largest |device - float64| / bound this run has seen so far, per metric: printed at the end of every case (pytest -s)
WORST = {"l2": 0.0, "ip": 0.0}
MMR_OUTPUTS = ("n_out", "index", "pos", "item_ids", "scores", "mmr")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _ring(n, deg=8):
    """the flat calls never read the graph: every node linked to its next eight, 64 enter points"""
    nbv = ((np.arange(n, dtype=np.int64)[:, None] + 1 + np.arange(deg)) % n).astype(np.int32).reshape(-1)
    rs = np.arange(n + 1, dtype=np.int64) * deg
    return [nbv, nbv.copy()], [rs, rs.copy()], np.arange(0, n, max(n // 64, 1), dtype=np.int32)[:64]


def _indices(d, dtype):
    """-> (device index of the large table, device index of the small one)"""
    from nann_amd import retrieval
    key = (d, dtype)
    if key not in _CACHE:
        _CACHE.clear()                                                     # one case's tables at a time
        stored = W.table(d, dtype)[0]
        ids = W.item_ids()
        _CACHE[key] = tuple(retrieval.Index(stored[:n], ids[:n], *_ring(n)) for n in (W.N_BIG, W.N_SMALL))
    return _CACHE[key]


def _score(sc, q, table, idx=None):
    """nann_score of one query: over the table's rows in order, or over table[idx]"""
    from nann_amd import ops
    s = ops.blaze_score(sc, q, item_emb=table) if idx is None else ops.blaze_score(sc, q, table=table, indices=idx)
    torch.cuda.synchronize()
    return s.cpu().numpy()


def _within(got, ref, bound, metric, what):
    """every score within the derived bound of float64"""
    ratio = W.ratio_to_bound(got, ref, bound)
    WORST[metric] = max(WORST[metric], ratio)
    assert ratio <= 1.0, (what, "score against float64, ratio to the bound", ratio)


def _same_bits(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.nonzero(bits(got).reshape(-1) != bits(exp).reshape(-1))[0]
    assert not len(bad), (what, "score bits", len(bad), "first at", int(bad[0]), hex(int(bits(got).reshape(-1)[bad[0]])), hex(int(bits(exp).reshape(-1)[bad[0]])))


def _nann_score(sc, q, table, idx):
    """nann_score through the C ABI -> (status, first bad position): what ops.blaze_score raises on"""
    from nann_amd import _lib
    from nann_amd.ops import _ptr, _stream
    out = torch.zeros(len(idx), dtype=torch.float32, device="cuda")
    idx_d = cuda(idx, torch.int32)
    bad = C.c_int64(-7)
    st = _lib.lib().nann_score(sc.handle, _ptr(q), _ptr(table), C.c_int64(table.shape[0]), _ptr(idx_d), C.c_int64(len(idx)), _ptr(out),
                               C.byref(bad), _stream())
    torch.cuda.synchronize()
    return st, bad.value


def _check_score(case, metric, sc, small):
    """the stand-alone scorer on the small table: every count of score_counts gathered (with repeats; the last one past the
    grid's cap) and all but the last in order, against reference A bit for bit and reference B within its bound; a shorter
    call is the head of a longer one; two bad indices report the smaller position"""
    d, dtype = case
    table = small.item_embs
    counts = W.score_counts(d)
    idx = np.random.default_rng(d + 3).integers(0, W.N_SMALL, counts[-1]).astype(np.int32)
    idx_d = cuda(idx, torch.int32)
    ref, bound = W.ref_b(d, dtype, metric)
    a = W.ref_a_small(d, dtype, metric)
    assert len(np.unique(idx)) == W.N_SMALL                               # the largest call scores every row, the edge block included
    for b in W.SCORE_QUERIES:
        q = cuda(W.queries(d, dtype)[b])
        got = {n: _score(sc, q, table, idx_d[:n]) for n in counts}
        for n in counts:
            what = case + (metric, "score", "query", b, "gathered", n)
            _same_bits(got[n], a[b][idx[:n]], what)                       # (reference A on the distinct rows, gathered)
            _within(got[n], ref[b][idx[:n]], bound[b][idx[:n]], metric, what)
            _same_bits(got[n], got[counts[-1]][:n], what + ("a shorter call is the head of a longer one",))
        for n in counts[:-1] + (W.N_SMALL,):
            what = case + (metric, "score", "query", b, "in order", n)
            s = _score(sc, q, table[:n])
            _same_bits(s, a[b][:n], what)
            _within(s, ref[b][:n], bound[b][:n], metric, what)
    n = counts[-1]
    q = cuda(W.queries(d, dtype)[0])
    one, two = idx.copy(), idx.copy()
    one[n - 1] = W.N_SMALL
    two[n // 2], two[n - 1] = -1, W.N_SMALL
    assert _nann_score(sc, q, table, one) == (5, n - 1), case + (metric,)  # NANN_ERR_INDEX_OUT_OF_RANGE
    assert _nann_score(sc, q, table, two) == (5, n // 2), case + (metric, "the smaller bad position")


def _search_all(dix, sc, q, k):
    from nann_amd import retrieval
    r = retrieval.search_all(dix, sc, q, k)
    torch.cuda.synchronize()
    return r.index.cpu().numpy(), r.scores.cpu().numpy(), r.item_ids.cpu().numpy()


def _check_scan(case, metric, sc, big, small):
    """search_all on both tables -> [{row: score bits}] of the large table's k = 1024 lists"""
    d, dtype = case
    q = cuda(W.queries(d, dtype))
    ref, bound = W.ref_b(d, dtype, metric)
    dec = W.decided(d, dtype)
    ids = W.item_ids()
    # nann_score of every (query, row): what the scan must give bit for bit ("bit-identical across entry points")
    alone = np.stack([_score(sc, q[b], big.item_embs) for b in range(W.NQ)])
    # the small table: the full score vector, every query held to reference A
    a = W.ref_a_small(d, dtype, metric)
    res = {k: _search_all(small, sc, q, k) for k in W.K_SMALL}
    rows, got, iid = res[W.N_SMALL]
    for b in range(W.NQ):
        what = case + (metric, "scan", W.N_SMALL, "query", b)
        top = R.topk_stable(a[b], W.N_SMALL)
        assert (rows[b] == top).all(), what + ("rows in TopKV2 order", int(np.nonzero(rows[b] != top)[0][0]))
        _same_bits(got[b], a[b][top], what)
        _same_bits(got[b], alone[b][rows[b]], what + ("nann_score's bits",))
        _within(got[b], ref[b][rows[b]], bound[b][rows[b]], metric, what)
        assert (iid[b] == ids[rows[b]]).all(), what
    assert (res[1][0] == rows[:, :1]).all() and (bits(res[1][1]) == bits(got[:, :1])).all(), case + (metric, "small: k = 1 is the head")
    lo, hi = W.PAIR[metric]
    assert res[1][0][W.CHOSEN_CUT[0], 0] == lo and rows[W.CHOSEN_CUT[0], 1] == hi, case + (metric, "the tie goes to the lower row")
    # the large table: two slabs
    res = {k: _search_all(big, sc, q, k) for k in W.K_BIG}
    kmax = W.K_BIG[-1]
    rows, got, iid = res[kmax]
    abig = W.ref_a_big(d, dtype, metric)
    order = W.order_b(d, dtype, metric)
    for b in range(W.NQ):
        what = case + (metric, "scan", W.N_BIG, "query", b)
        if b in abig:
            top = R.topk_stable(abig[b], kmax)
            assert (rows[b] == top).all(), what + ("rows in TopKV2 order", int(np.nonzero(rows[b] != top)[0][0]))
            _same_bits(got[b], abig[b][top], what)
        _same_bits(got[b], alone[b][rows[b]], what + ("nann_score's bits",))
        assert (rows[b] == R.topk_stable(alone[b], kmax)).all(), what + ("TopKV2 order of nann_score's scores",)
        _within(got[b], ref[b][rows[b]], bound[b][rows[b]], metric, what)
        assert (iid[b] == ids[rows[b]]).all(), what
        for k in W.K_BIG:
            if dec[(metric, W.N_BIG, k)][b]:
                assert set(rows[b, :k].tolist()) == set(order[b, :k].tolist()), what + ("the decided row set", k)
    assert res[1][0][W.CHOSEN_CUT[0], 0] == lo and rows[W.CHOSEN_CUT[0], 1] == hi, case + (metric, "the tie goes to the lower row")
    for k in W.K_BIG[:-1]:
        assert (res[k][0] == rows[:, :k]).all() and (bits(res[k][1]) == bits(got[:, :k])).all() and (res[k][2] == iid[:, :k]).all(), \
            case + (metric, "k = %d is the head of k = %d" % (k, kmax))
    return [{int(i): s for i, s in zip(rows[b], bits(got[b]))} for b in range(W.NQ)]


def _check_lists(case, metric, sc, big, scan_bits):
    """search_candidates on the ragged lists, k = 64, against topk_stable over reference A of each list"""
    from nann_amd import retrieval
    d, dtype = case
    k = W.CAND_K
    lists, users = W.candidate_lists(d, dtype)
    exp = W.list_scores(d, dtype, metric)
    ref, bound = W.ref_b(d, dtype, metric)
    ids = W.item_ids()
    r = retrieval.search_candidates(big, sc, cuda(W.queries(d, dtype)[users]), candidates=lists, k=k)
    torch.cuda.synchronize()
    rows, got, pos, iid = r.index.cpu().numpy(), r.scores.cpu().numpy(), r.pos.cpu().numpy(), r.item_ids.cpu().numpy()
    n_out, st = r.n_out.cpu().numpy(), r.status.cpu().numpy()
    assert (st == 0).all(), (case, metric, st)
    assert (n_out == np.minimum(k, [len(li) for li in lists])).all(), (case, metric, n_out)
    common = 0
    for i, li in enumerate(lists):
        what = case + (metric, "lists", i, len(li))
        n, b = n_out[i], users[i]
        assert not rows[i, n:].any() and not bits(got[i, n:]).any() and not pos[i, n:].any() and not iid[i, n:].any(), what + ("zeros behind n_out",)
        if n == 0:
            continue
        top = R.topk_stable(exp[i], n)
        assert (pos[i, :n] == top).all(), what + ("pos",)
        assert (rows[i, :n] == li[top]).all() and (iid[i, :n] == ids[li[top]]).all(), what + ("index / item ids",)
        _same_bits(got[i, :n], exp[i][top], what)
        _within(got[i, :n], ref[b][li[top]], bound[b][li[top]], metric, what)
        both = [(int(row), s) for row, s in zip(rows[i, :n], bits(got[i, :n])) if int(row) in scan_bits[b]]
        assert all(scan_bits[b][row] == s for row, s in both), what + ("a list's score is not the scan's",)
        common += len(both)
    i, first, second = W.CAND_DUP   # the row listed twice: both positions, the lower one first, the same bits
    at = np.nonzero(rows[i, :n_out[i]] == lists[i][first])[0]
    assert len(at) == 2 and pos[i][at].tolist() == [first, second] and bits(got[i][at[0]]) == bits(got[i][at[1]]), (case, metric, at)
    assert common >= 100, (case, metric, "the identity with the scan was checked on too few pairs", common)


def _check_mmr(case, sim, big):
    """retrieval.mmr on both sides of the LDS boundary and on the list of 65 against mmr_model, every output bit for bit"""
    from nann_amd import retrieval
    from test_mmr_gpu import _boundary
    d, dtype = case
    edge = _boundary(d, dtype)
    assert edge == W.mmr_edge(d, dtype)
    room, per_row = W.MMR_LDS_BYTES - W.MMR_STATE_BYTES, W.row_bytes(d, dtype) + W.MMR_ROW_PAD
    calls = W.mmr_calls(d, dtype)
    sides = [k_in * per_row <= room for k_in, _, _, _, _ in calls]       # mmr_rows_in_lds
    assert sides == [True, False, True, True], (case, sides)
    for (k_in, rows, scores, k, lam), exp in zip(calls, W.mmr_expected(d, dtype, sim)):
        r = retrieval.mmr(big, cuda(scores), cuda(rows), retrieval.make_diversity(lam=lam, sim=sim), k)
        torch.cuda.synchronize()
        for name in MMR_OUTPUTS:
            g = getattr(r, name).cpu().numpy()
            assert g.shape == exp[name].shape and (g.view(np.uint8) == exp[name].view(np.uint8)).all(), case + (sim, "mmr", k_in, k, lam, name)


@pytest.mark.parametrize("dtype", W.DTYPES)
@pytest.mark.parametrize("d", W.DIMS)
def test_every_flat_kernel_against_the_canonical_order(d, dtype):
    from nann_amd import ops
    case = (d, dtype)
    t0 = time.perf_counter()
    n_dec = W.references(d, dtype)        # check_conditions first: on the references alone, so that a pass below means something
    t1 = time.perf_counter()
    big, small = _indices(d, dtype)
    assert big.d == small.d == d and big.n_items == W.N_BIG and small.n_items == W.N_SMALL
    entered = []
    for metric in W.METRICS:
        sc = ops.Scorer(metric, d, _TORCH_DT[dtype])
        scan_bits = None
        for launch in LAUNCHES:
            assert all(k in KERNELS for k in claimed(d, dtype, metric, launch)), (case, metric, launch)
            entered += claimed(d, dtype, metric, launch)
            if launch == "score":
                _check_score(case, metric, sc, small)
            elif launch == "scan":
                scan_bits = _check_scan(case, metric, sc, big, small)
            elif launch == "lists":
                _check_lists(case, metric, sc, big, scan_bits)
            else:
                _check_mmr(case, metric, big)
    assert len(set(entered)) == 8
    print("flat matrix d=%d %s: %d kernels entered, %d of %d cuts decided; references %.2f s, device launches and checks %.2f s; "
          "largest ratio to the float64 bound l2 %.3g, ip %.3g"
          % (d, dtype, len(set(entered)), n_dec, W.NQ * len(W.decided(d, dtype)), t1 - t0, time.perf_counter() - t1, WORST["l2"], WORST["ip"]))
