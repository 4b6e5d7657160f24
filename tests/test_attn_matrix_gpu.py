"""-m gpu: every compiled kernel of the attention + DNN scorer (nann_attn*.h) against references that are not
the device.

The scorer compiles to the 46 kernels of KERNELS below, besides the four k_search_eval<.., SC 3, ..> that
test_eval_matrix_gpu.py launches: the traversal that reads the embedding rows, per (d, row dtype) in the f32 and the split-f16
form on the 16K-slot hash set and both bitmaps; the traversal on the pre-projected table (one instance per form and plan, every
d and dtype) with the split form's resident kernel on the hash set; the stand-alone scorer and the two per-user prepare
kernels; the kernel that builds the table; the exhaustive scan and the candidate-list scorer.  Each is a code object of its
own, so each is launched here: 4 cases (d, row dtype) x the launches of LAUNCHES, every traversal asserting the plan it got and
looking up the kernel that plan names in KERNELS.  test_attn_matrix_cpu.py holds KERNELS to the build's own list of kernels.

The workload and both references are attn_matrix.py's.  No attention kernel is bit-exact with the oracle, so the expectation
is the model in float64: every score within 1e-5 max(1, |ref|) of attn_reference.np_model for the row returned with it, and on
the DECISIVE requests (attn_matrix.py: every cut of the float64 schedule wider than 3e-5) the schedule's row set and counters,
with no allowance for a diverged query.

The overflow rerun (test_an_overflowing_request_is_rerun_from_a_clean_start): on a forced hash plan a request whose set could
overflow is handed back and run again on the fallback plan's kernel with redo = 1; its answer must be, bit for bit, what the
same call forced to that plan returns (the same kernel with redo = 0).

Measured on an MI355X: the largest |device - float64| / max(1, |float64|) over every score of the four cases is 1.4e-6 in the
f32 form (8.1e-7, 8.9e-7, 1.1e-6, 1.4e-6 at (64, f16), (64, bf16), (128, f16), (128, bf16)) and 8.3e-7 in the split-f16 form;
a case takes 0.65-1.75 s, of which 0.5-1.5 s are the CPU references (cached per module) and 0.1-0.5 s the 20 launches and
their checks; the rerun test takes 1.7 s (1.55 s graph and references, 0.15 s its eight launches), with 8 reruns per launch and
the LDS bitmap as the fallback plan."""
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch

import attn_matrix as W
from attn_reference import rel_err
from gpu_util import bits, cuda, require_gpu, synth_index

pytestmark = pytest.mark.gpu

LPR = {64: 8, 128: 16}                             # lanes per row: d / 8
DT = {"f16": 0, "bf16": 1}
VIS = {"lds_bitmap": 0, "hbm_bitmap": 1, "lds_hash": 2}
# SC of k_search: kScorerAttn (f32 form, embedding rows), kScorerAttnSplit (split-f16, embedding rows), kScorerAttnXProj /
# kScorerAttnProj (f32 / split on the table), kScorerAttnRes (split on the table, keys and weights resident: the hash plan's)
SC_ROWS = {"exact": 3, "split": 4}
SC_TABLE = {"exact": 10, "split": 6}
SC_RES = 11
NT = 512                                           # kAttnNT: every attention traversal
PREPARE = {"exact": ("k_attn_prepare",), "split": ("k_attn_prepare_split",)}
SCORE = {"exact": "k_score_attn", "split": "k_score_attn_split"}
EXACT = {"exact": 1, "split": 0}                   # the bool of k_scan_attn / k_cand_score_attn
MODES = ("lds_hash", "lds_bitmap", "hbm_bitmap")

# every kernel the attention scorer's dispatch can reach, template arguments in order
KERNELS = tuple(
    [("k_search", LPR[d], dt, VIS[m], SC_ROWS[p], NT) for p in SC_ROWS for d in LPR for dt in DT.values() for m in MODES] +  # 12 + 12
    [("k_search", 16, 0, VIS[m], SC_TABLE["exact"], NT) for m in MODES] +                                                # 3
    [("k_search", 16, 0, VIS[m], SC_TABLE["split"], NT) for m in ("lds_bitmap", "hbm_bitmap")] +                         # 2
    [("k_search", 16, 0, VIS["lds_hash"], SC_RES, NT)] +
    [(SCORE[p], d, dt) for p in SCORE for d in LPR for dt in DT.values()] +                                              # 4 + 4
    [PREPARE["exact"], PREPARE["split"]] +
    [("k_attn_preproject", dt) for dt in DT.values()] +
    [("k_scan_attn", e) for e in EXACT.values()] + [("k_cand_score_attn", e) for e in EXACT.values()])

# the launches of one case: (what, precision, forced plan or None), in the order they run -- the rows first (no table yet), then
# per precision the hash plan on the table (the model's first call on a table builds it)
LAUNCHES = tuple(
    [("rows", p, m) for p in ("exact", "split") for m in MODES] + [("rows_per_request", p, "lds_hash") for p in ("exact", "split")] +
    [("table", p, m) for p in ("exact", "split") for m in MODES] +
    [(what, p, None) for what in ("scan", "lists", "score") for p in ("exact", "split")])


def claimed(d, dtype, launch):
    """the KERNELS entries a launch of this case enters; a traversal's first: the kernel its plan names"""
    what, precision, mode = launch
    if what in ("rows", "rows_per_request"):
        return [("k_search", LPR[d], DT[dtype], VIS[mode], SC_ROWS[precision], NT), PREPARE[precision]]
    if what == "table":
        resident = precision == "split" and mode == "lds_hash"
        first = ("k_search", 16, 0, VIS[mode], SC_RES if resident else SC_TABLE[precision], NT)
        return [first, PREPARE[precision]] + ([("k_attn_preproject", DT[dtype])] if mode == "lds_hash" else [])
    if what == "scan":
        return [("k_scan_attn", EXACT[precision]), PREPARE[precision]]
    if what == "lists":
        return [("k_cand_score_attn", EXACT[precision]), PREPARE[precision]]
    assert what == "score"
    return [(SCORE[precision], d, DT[dtype]), PREPARE[precision]]


_TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16}
_CACHE = {}
# the largest |device - float64| / max(1, |float64|) this run has seen so far, per form: printed at the end of every case (pytest -s)
WORST = {"exact": 0.0, "split": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


@pytest.fixture(scope="module")
def model_dirs(tmp_path_factory):
    """path of the weights directory of (d, precision), written once"""
    root = tmp_path_factory.mktemp("attn_matrix")

    def get(d, precision):
        from nann_amd import ops
        path = str(root / ("attn_%d_%s" % (d, precision)))
        if not os.path.isdir(path):
            ops.save_scorer_dir(path, "attention", W.weights(d), precision=precision)
        return path
    return get


def _device_index(d, dtype):
    """-> (device index, its row tensor)"""
    from nann_amd import retrieval
    key = (d, dtype)
    if key not in _CACHE:
        g = W.graph(d)[0]
        t = W.table(d, dtype)[0]
        rows = torch.as_tensor(t.view(np.int16)).cuda().view(torch.bfloat16) if dtype == "bf16" else torch.as_tensor(t).cuda()
        _CACHE[key] = (retrieval.Index(rows, g["item_ids"], g["nb_values"], g["nb_row_splits"], g["enter_points"]), rows)
    return _CACHE[key]


def _within(got, ref, precision, what):
    """every score within the contract of float64 -> the largest error"""
    err = rel_err(got, ref)
    worst = float(err.max()) if err.size else 0.0
    WORST[precision] = max(WORST[precision], worst)
    assert worst <= W.TOL, (what, "score against float64", worst)
    return worst


def _launch(dix, model, seq, topn, case, launch, preprojection, rerun=False):
    """one retrieval.search_model forced to the launch's plan; asserts the plan against the launch's claim and that the kernel
    it names is in KERNELS -> (the five outputs on the host, the plan)"""
    from nann_amd import retrieval
    what, precision, mode = launch
    r = retrieval.search_model(dix, model, seq, topn, options=retrieval.search_options(traversal=mode, preprojection=preprojection))
    torch.cuda.synchronize()
    on_table = what == "table"
    assert r.plan["table"] == on_table and not r.plan["phased"], (launch, r.plan)
    assert r.plan["visited_set"] == mode and r.plan["threads"] == NT, (launch, r.plan)
    if on_table:
        resident = precision == "split" and r.plan["visited_set"] == "lds_hash"
        ran = ("k_search", 16, 0, VIS[r.plan["visited_set"]], SC_RES if resident else SC_TABLE[precision], r.plan["threads"])
    else:
        ran = ("k_search", LPR[dix.d], DT[case[1]], VIS[r.plan["visited_set"]], SC_ROWS[precision], r.plan["threads"])
    assert ran == claimed(case[0], case[1], launch)[0] and ran in KERNELS, (launch, ran, r.plan)
    assert all(k in KERNELS for k in claimed(case[0], case[1], launch)), launch
    if r.plan["visited_set"] == "lds_hash" and not rerun:
        assert r.reruns() == 0, "the set overflowed: the answers would be the fallback kernel's"
    return tuple(getattr(r, f).cpu().numpy() for f in ("status", "item_ids", "scores", "index", "counters")), r


def _assert_traversal(got, g, users, topn, sched, score_of, precision, what):
    """a traversal's outputs for `users` under `topn` against their float64 schedule `sched`.  Every request: the schedule's
    status, scores descending and within 1e-5 of float64 for the row returned with each, item ids that belong to the rows,
    zeros behind the request's own k.  Every decisive request: the schedule's row set and counters -> decisive requests checked"""
    st, ids, sc, rows, ctr = got
    k = topn[5]
    n_dec = 0
    for i, b in enumerate(users):
        est, erows, ectr, margin = sched[i]
        assert st[i] == est, (what, "user", b, "status", st[i], est)
        assert not ids[i, k:].any() and not bits(sc[i, k:]).any() and not rows[i, k:].any(), (what, "user", b, "zeros behind k")
        if est:
            assert not ids[i].any() and not bits(sc[i]).any() and not rows[i].any(), (what, "user", b, "a failed request's rows")
            continue
        assert ((rows[i, :k] >= 0) & (rows[i, :k] < len(g["item_ids"]))).all(), (what, "user", b, "rows of the index")
        _within(sc[i, :k], score_of(b, rows[i, :k]), precision, what + ("user", b))
        assert (np.diff(sc[i, :k]) <= 0).all(), (what, "user", b, "scores descend")
        assert (ids[i, :k] == np.asarray(g["item_ids"])[rows[i, :k]]).all(), (what, "user", b, "item ids of the rows")
        if margin > W.MARGIN:
            n_dec += 1
            assert set(rows[i, :k].tolist()) == set(erows.tolist()) and len(set(rows[i, :k].tolist())) == k, (what, "user", b, "row set")
            assert (ctr[i] == ectr).all(), (what, "user", b, "counters", ctr[i], ectr)
    return n_dec


def _assert_case_traversal(got, case, topn, sel, precision, what, scores64=W.scores64, schedule=W.schedule64):
    """(scores64 / schedule: what the mutation checks replace)"""
    d, dtype = case
    users = np.arange(W.NQ) if sel is None else sel
    return _assert_traversal(got, W.graph(d)[0], users, topn, schedule(d, dtype, topn, sel), lambda b, r: scores64(d, dtype, b, r), precision, what)


def _ordered(scores, keys):
    """score descending (-0 = +0), ties -> the lower key"""
    s = scores + np.float32(0.0)
    return bool(((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (keys[:-1] < keys[1:]))).all())


def _assert_best_of(what, rows, sc, keys, ref_of_rows, pool, k, precision):
    """a top-k list: scores within 1e-5 of float64, ordered, and every returned row's float64 logit at least the pool's k-th best
    minus 2e-5 max(1, |kth|) (a row may enter or leave the list only on a near-tie: 1e-5 on either side)"""
    _within(sc, ref_of_rows, precision, what)
    assert _ordered(sc, keys), (what, "order")
    if len(pool) > k:
        kth = np.sort(pool)[::-1][k - 1]
        assert (ref_of_rows >= kth - 2e-5 * max(1.0, abs(kth))).all(), (what, "a row below the k-th best")


def _check_scan(case, dix, model, seq, precision):
    """search_all_model at k = 64 and k = 1024 -> {user: {row: score bits}} of the wide list"""
    from nann_amd import ops, retrieval
    d, dtype = case
    ref = W.scores64_all(d, dtype)
    res = {}
    for k in W.K_SCAN:
        r = retrieval.search_all_model(dix, model, seq, k)
        torch.cuda.synchronize()
        res[k] = (r.index.cpu().numpy(), r.scores.cpu().numpy(), r.item_ids.cpu().numpy())
        rows, sc, ids = res[k]
        assert rows.shape == (W.NQ, k)
        for b in range(W.NQ):
            assert len(set(rows[b].tolist())) == k and (ids[b] == np.asarray(W.graph(d)[0]["item_ids"])[rows[b]]).all(), (case, precision, k, b)
            _assert_best_of(case + ("scan", precision, k, b), rows[b], sc[b], rows[b], ref[b][rows[b]], ref[b], k, precision)
    (r64, s64, _), (r1k, s1k, _) = res[W.K_SCAN[0]], res[W.K_SCAN[1]]
    assert (r64 == r1k[:, :W.K_SCAN[0]]).all() and (bits(s64) == bits(s1k[:, :W.K_SCAN[0]])).all(), (case, precision, "k = 64 is the head of k = 1024")
    with pytest.raises(ops.NannError) as e:
        retrieval.search_all_model(dix, model, seq, W.K_SCAN[1] + 1)
    assert e.value.status == 102, e.value   # NANN_ERR_UNSUPPORTED: 1024 is the widest k
    return [{int(i): s for i, s in zip(r1k[b], bits(s1k[b]))} for b in range(W.NQ)]


def _check_lists(case, dix, model, seq, precision, scan_bits):
    """search_candidates_model on the ragged lists, k = 64; a list's score of a (user, row) has the scan's bits"""
    from nann_amd import retrieval
    d, dtype = case
    k = W.K_SCAN[0]
    lists = W.candidate_lists()
    ref = W.scores64_all(d, dtype)
    r = retrieval.search_candidates_model(dix, model, seq, candidates=lists, k=k)
    torch.cuda.synchronize()
    rows, sc, pos, ids = r.index.cpu().numpy(), r.scores.cpu().numpy(), r.pos.cpu().numpy(), r.item_ids.cpu().numpy()
    n_out, st = r.n_out.cpu().numpy(), r.status.cpu().numpy()
    assert (st == 0).all(), st
    assert (n_out == np.minimum(k, [len(li) for li in lists])).all(), n_out
    common = possible = 0
    for b, li in enumerate(lists):
        n = n_out[b]
        assert not rows[b, n:].any() and not bits(sc[b, n:]).any() and not pos[b, n:].any() and not ids[b, n:].any(), (case, precision, b, "zeros behind n_out")
        if n == 0:
            continue
        assert len(set(pos[b, :n].tolist())) == n and (li[pos[b, :n]] == rows[b, :n]).all(), (case, precision, b, "pos")
        assert (ids[b, :n] == np.asarray(W.graph(d)[0]["item_ids"])[rows[b, :n]]).all()
        _assert_best_of(case + ("lists", precision, b), rows[b, :n], sc[b, :n], pos[b, :n], ref[b][rows[b, :n]], ref[b][li], k, precision)
        both = [(int(i), s) for i, s in zip(rows[b, :n], bits(sc[b, :n])) if int(i) in scan_bits[b]]
        assert all(scan_bits[b][i] == s for i, s in both), (case, precision, b, "a list's score is not the scan's")
        common += len(both)
        possible += n
    ub, first, second = W.CAND_DUP   # the row listed twice: both copies or neither (or the first as the last entry), the same bits
    dup = np.nonzero(rows[ub, :n_out[ub]] == lists[ub][first])[0]
    assert len(dup) in (0, 2) or (len(dup) == 1 and dup[0] == k - 1 and pos[ub, dup[0]] == first), (ub, dup)
    if len(dup) == 2:
        assert pos[ub][dup].tolist() == [first, second] and bits(sc[ub][dup[0]]) == bits(sc[ub][dup[1]])
    assert 2 * common >= possible, (case, precision, "the identity was checked on too few pairs", common, possible)


def _nann_attn_score(sc, kt, upad, table, idx):
    """nann_attn_score through the C ABI -> (status, first bad position): what AttnScorer.score raises on"""
    from nann_amd import _lib
    from nann_amd.ops import _ptr, _stream
    out = torch.zeros(len(idx), dtype=torch.float32, device="cuda")
    idx_d = cuda(idx, torch.int32)
    bad = C.c_int64(-7)
    st = _lib.lib().nann_attn_score(sc.handle, _ptr(kt), _ptr(upad), _ptr(table), C.c_int64(table.shape[0]), _ptr(idx_d), C.c_int64(len(idx)),
                                    _ptr(out), C.byref(bad), _stream())
    torch.cuda.synchronize()
    return st, bad.value


def _check_score(case, table, precision):
    """ops.AttnScorer: one prepare for the 24 users, then per user the rows idx[:n] for every n of score_counts (the count above
    the grid's stride for the first and the last user), the header's promises about kt / upad in the exact form, and the
    report of an index out of range"""
    from nann_amd import ops
    from oracle import oracle as O
    d, dtype = case
    seqs = W.seqs()
    sc = ops.AttnScorer(d, W.SEQ_LEN, _TORCH_DT[dtype], W.weights(d), precision=precision)
    kt, upad = sc.prepare(cuda(seqs))
    torch.cuda.synchronize()
    counts = W.score_counts(precision)
    idx = np.random.default_rng(d).integers(0, W.N_ITEMS, counts[-1]).astype(np.int32)   # with repeats
    idx_d = cuda(idx, torch.int32)
    ref = W.scores64_all(d, dtype)
    L = W.SEQ_LEN
    for b in range(W.NQ):
        ns = counts if b in (0, W.NQ - 1) else counts[:-1]
        got = {n: sc.score(kt[b], upad[b], table=table, indices=idx_d[:n]).cpu().numpy() for n in ns}
        for n in ns:
            assert got[n].shape == (n,)
            _within(got[n], ref[b][idx[:n]], precision, case + ("score", precision, b, n))
            assert (bits(got[n]) == bits(got[ns[-1]][:n])).all(), (case, precision, b, n, "a shorter call is the head of a longer one")
        n = counts[4]
        pre = sc.score(kt[b], upad[b], item_emb=table[idx_d[:n].long()]).cpu().numpy()
        assert (bits(pre) == bits(got[n])).all(), (case, precision, b, "pre-gathered rows score differently from gathered ones")
    if precision == "exact":   # the header: the per-user projection bit for bit, zero padding
        kt_h, upad_h = kt.cpu().numpy(), upad.cpu().numpy()
        am = W.oracle_model(d, dtype)
        for b, u in enumerate(seqs):
            rc, kproj = O.attn_prepare(am, u.astype(np.float32))
            assert rc == 0
            assert (bits(kt_h[b][:, :L]) == bits(kproj.T)).all(), (case, b, "kt")
            assert not bits(kt_h[b][:, L:]).any() and not bits(upad_h[b][L:]).any(), (case, b, "padding")
            assert (bits(upad_h[b][:L]) == bits(u.astype(np.float32))).all(), (case, b, "upad")
    n = counts[-1]
    one, two = idx.copy(), idx.copy()
    one[n - 1] = W.N_ITEMS
    two[n // 2], two[n - 1] = -1, W.N_ITEMS
    assert _nann_attn_score(sc, kt[0], upad[0], table, one) == (5, n - 1), (case, precision)  # NANN_ERR_INDEX_OUT_OF_RANGE
    assert _nann_attn_score(sc, kt[0], upad[0], table, two) == (5, n // 2), (case, precision, "the smaller bad position")


@pytest.mark.parametrize("dtype", W.DTYPES)
@pytest.mark.parametrize("d", W.DIMS)
def test_every_attention_kernel_against_float64(model_dirs, d, dtype):
    from nann_amd import ops, retrieval
    case = (d, dtype)
    t0 = time.perf_counter()
    W.check_conditions(d, dtype)          # on the references alone: a pass below means something
    W.scores64_all(d, dtype)
    t1 = time.perf_counter()
    dix, table = _device_index(d, dtype)
    assert dix.d == d
    models = {p: ops.Model(model_dirs(d, p), d, W.SEQ_LEN, _TORCH_DT[dtype]) for p in ("exact", "split")}
    assert all(m.kind == "attention" for m in models.values())
    seq = cuda(W.seqs())
    tq = W.level_topn_rows()
    scan_bits, table_hash = {}, {}
    for launch in LAUNCHES:
        what, precision, mode = launch
        tag = case + launch
        model = models[precision]
        if what == "score":
            _check_score(case, table, precision)
        elif what == "scan":
            scan_bits[precision] = _check_scan(case, dix, model, seq, precision)
        elif what == "lists":
            _check_lists(case, dix, model, seq, precision, scan_bits[precision])
        elif what == "rows_per_request":
            got, _ = _launch(dix, model, seq, tq, case, launch, False)
            assert got[1].shape == (W.NQ, max(W.TOPN[5], W.TOPN_ODD[5]))
            n_dec = sum(_assert_case_traversal(tuple(o[sel] for o in got), case, topn, sel, precision, tag + (tuple(topn),))
                        for sel, topn in W.per_request())
            assert n_dec >= W.MIN_DECISIVE, (tag, n_dec)
        else:
            builds = ("k_attn_preproject", DT[dtype]) in claimed(d, dtype, launch)
            if builds:
                assert retrieval.table_bytes(dix, model)[1] == 0, (tag, "the table was there before its first call")
            got, _ = _launch(dix, model, seq, W.TOPN, case, launch, what == "table")
            if builds:
                assert retrieval.table_bytes(dix, model)[1] > 0, tag
            elif what == "rows":
                assert retrieval.table_bytes(dix, model)[1] == 0, (tag, "a call without preprojection built a table")
            assert _assert_case_traversal(got, case, W.TOPN, None, precision, tag) >= W.MIN_DECISIVE, tag
            if what == "table" and mode == "lds_hash":
                table_hash[precision] = got
    # the header's identity: the split scan's bits are the hash-set traversal's (the resident kernel's) for the same (user, row)
    st, _, sc, rows, _ = table_hash["split"]
    common = possible = 0
    for b in np.nonzero(st == 0)[0]:
        both = [(int(i), s) for i, s in zip(rows[b], bits(sc[b])) if int(i) in scan_bits["split"][b]]
        assert all(scan_bits["split"][b][i] == s for i, s in both), (case, b, "the traversal's score is not the scan's")
        common += len(both)
        possible += rows.shape[1]
    assert possible and 2 * common >= possible, (case, "the identity was checked on too few pairs", common, possible)
    print("attention matrix d=%d %s: references %.2f s, device launches and checks %.2f s; largest error exact %.3g, split %.3g"
          % (d, dtype, t1 - t0, time.perf_counter() - t1, WORST["exact"], WORST["split"]))


# ---- the overflow rerun -----------------------------------------------------------------------------------------------------------
RERUN_LAUNCHES = tuple((what, p, "lds_hash") for what in ("table", "rows") for p in ("split", "exact"))


def test_an_overflowing_request_is_rerun_from_a_clean_start(model_dirs):
    """Once, at (64, f16): one launch mixes (per-request level_topn) beams that outgrow the 16K-slot set with beams that fit it,
    on a forced hash plan, table / rows x split / exact.  The float64 schedule, on the CPU, says which requests overflow
    (attn_matrix.check_rerun_conditions).  Every wide request is handed back and rerun; its status, rows, item ids, score bits
    and counters are those of the same call forced to the fallback plan, where the same kernel runs it with redo = 0 -- a
    rerun that started from stale slot state or from the first launch's permutation would differ.  Every score within 1e-5 of
    float64; the narrow requests as in the matrix."""
    from nann_amd import ops
    d, dtype = W.RERUN_CASE
    t0 = time.perf_counter()
    g, _, dix = synth_index(W.RERUN_GRAPH["n"], d, W.RERUN_GRAPH["ef"], n_clusters=W.RERUN_GRAPH["n_clusters"], mode=W.RERUN_GRAPH["mode"])
    seqs, score_of, settings = W.rerun_reference(g)
    n_wide_served, kept_w, kept_n = W.check_rerun_conditions(g)
    t1 = time.perf_counter()
    tq = W.rerun_level_topn()
    wide_users = settings[0][0]
    seq = cuda(seqs)
    for launch in RERUN_LAUNCHES:
        what, precision, _ = launch
        model = ops.Model(model_dirs(d, precision), d, W.SEQ_LEN, _TORCH_DT[dtype])
        got, r = _launch(dix, model, seq, tq, (d, dtype), launch, what == "table", rerun=True)
        assert r.reruns() == len(wide_users), (launch, r.reruns(), len(wide_users))
        fallback = r.plan["fallback_visited_set"]
        assert fallback in ("lds_bitmap", "hbm_bitmap"), r.plan
        direct, _ = _launch(dix, model, seq, tq, (d, dtype), (what, precision, fallback), what == "table")
        n_dec = 0
        for users, topn, sched in settings:
            n_dec += _assert_traversal(tuple(o[users] for o in got), g, users, topn, sched, score_of, precision, launch + (topn[1],))
        for b in wide_users:
            for name, a, e in zip(("status", "item ids", "scores", "rows", "counters"), got, direct):
                same = (bits(a[b]) == bits(e[b])).all() if a.dtype == np.float32 else (a[b] == e[b]).all()
                assert same, (launch, "user", b, name, "the rerun is not the fallback plan's own answer")
        print("rerun %s %s: %d reruns, fallback %s, %d decisive requests checked" % (what, precision, len(wide_users), fallback, n_dec))
    print("overflow rerun: references %.2f s, device %.2f s; wide requests served %d, kept ids %d..%d, narrow %d..%d"
          % (t1 - t0, time.perf_counter() - t1, n_wide_served, min(kept_w), max(kept_w), min(kept_n), max(kept_n)))
