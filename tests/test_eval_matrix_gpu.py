"""-m gpu: every compiled instantiation of the evaluation traversal that the MLP matrix does not launch, against a reference
that is not the device, and the boundaries of its dispatch.

k_search_eval<LPR, DT, SC, NT, SEEN_LDS> (nann_eval.h) is compiled 46 times: for the L2 scorer once per row width (LPR 8 / 16 /
32 / 64 for d = 64 / 128 / 256 / 512), row dtype (f16, bf16, f32) and form -- SEEN_LDS 0 = `seen` in the slot's HBM, 1 = in LDS, one
window, 2 = in LDS, the id space swept in windows --, four times for the attention model (d 64 / 128, f16 / bf16) and six times
for the MLP scorer (test_mlp_matrix_gpu.py launches those).  KERNELS below: the 36 + 4.  Every launch first asks
retrieval.search_eval_plan what will run, asserts the form, the windows and the threads it expects, and looks the
instantiation up in KERNELS; test_eval_matrix_cpu.py holds KERNELS to the build's own list of kernels.

The slot form is what eval_plan picks only beyond eight windows, for a neighbour row of 65 536 entries, or under
NANN_EVAL_SEEN=hbm -- read once per process, so one fresh child process runs everything that needs it and records the plans
it was given.  The workload and every expected value are eval_matrix.py's: oracle.search_eval, compared bit for bit (status,
n_out, rows, item ids, score bits, zero tails); the attention model is held to RTOL of test_attn_shapes_gpu.py."""
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import eval_matrix as W
import traverse_matrix as T
from gpu_util import bits, cuda, require_gpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LPR = {64: 8, 128: 16, 256: 32, 512: 64}           # lanes per row: d / 8
DT = {"f16": 0, "bf16": 1, "f32": 2}
SC_L2, SC_ATTN = 0, 3                              # NANN_SCORER_L2, kScorerAttn
FORMS = (0, 1, 2)                                  # SEEN_LDS: slot, one window in LDS, windows
NT_L2, NT_ATTN = 1024, 512

# (LPR, DT, SC, NT, SEEN_LDS): every k_search_eval the dispatch of nann_eval_inst.hip, nann_eval_lds_inst.hip and
# nann_eval_win_inst.hip can reach
KERNELS = tuple([(lpr, dt, SC_L2, NT_L2, form) for form in FORMS for lpr in sorted(LPR.values()) for dt in sorted(DT.values())] +
                [(LPR[d], DT[t], SC_ATTN, NT_ATTN, 0) for d in W.ATTN_DIMS for t in W.ATTN_DTYPES])

# what launches each entry: (test, d, dtype, form)
LAUNCHES = tuple([("l2", d, t, form) for form in FORMS for d in W.DIMS for t in W.DTYPES] +
                 [("attn", d, t, 0) for d in W.ATTN_DIMS for t in W.ATTN_DTYPES])

_TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
_FIELDS = ("status", "n_out", "item_ids", "scores", "index")
_CACHE = {}


def claimed(kind, d, dtype, form):
    """the KERNELS entry a launch of this case enters"""
    return (LPR[d], DT[dtype], SC_L2, NT_L2, form) if kind == "l2" else (LPR[d], DT[dtype], SC_ATTN, NT_ATTN, 0)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


# ---- shared by the parent and the child ------------------------------------------------------------------------------------
def _rows_on_device(rows, dtype):
    return torch.as_tensor(rows.view(np.int16)).cuda().view(torch.bfloat16) if dtype == "bf16" else torch.as_tensor(rows).cuda()


def _device_index(rows, dtype, g, n=None):
    """the graph g over `rows`; n: relabelled into n rows through eval_matrix.pi, the table a zero fill and one scatter on the
    device"""
    from nann_amd import retrieval
    table = _rows_on_device(rows, dtype)
    if n is not None:
        p = W.pi(len(g["item_ids"]), n)
        g = W.relabel(g, p, n)
        small, table = table, torch.zeros((n, rows.shape[1]), dtype=table.dtype, device="cuda")
        table[torch.as_tensor(p).cuda()] = small
    return retrieval.Index(table, g["item_ids"], g["nb_values"], g["nb_row_splits"], g["enter_points"])


def _run(dix, dtype, q, cfg, form, n_windows=None, want_counters=False, use_dirty=None):
    """the plan asserted (form, windows, threads, an entry of KERNELS), then retrieval.search_eval -> its outputs on the host,
    the plan and the seconds of the launch"""
    from nann_amd import ops, retrieval
    sc = ops.Scorer("l2", dix.d, _TORCH_DT[dtype])
    plan = retrieval.search_eval_plan(dix, sc, len(q))
    assert plan["form"] == form and plan["threads"] == NT_L2, (plan, form)
    assert n_windows is None or plan["n_windows"] == n_windows, (plan, n_windows)
    assert use_dirty is None or plan["use_dirty"] == use_dirty, (plan, use_dirty)
    assert plan["slots"] == min(len(q), CUS_SLOTS[form]), plan
    assert (LPR[dix.d], DT[dtype], SC_L2, plan["threads"], plan["form"]) in KERNELS
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = retrieval.search_eval(dix, sc, cuda(q), *cfg, want_counters=want_counters)
    torch.cuda.synchronize()
    out = {f: getattr(r, f).cpu().numpy() for f in _FIELDS}
    out["seconds"] = time.perf_counter() - t0
    out["plan"] = plan
    if want_counters:
        out["counters"] = r.counters.cpu().numpy()
    return out


def _check(out, exp, what, fails=None):
    """_check of test_eval_edges_gpu.py: status, n_out, rows, item ids and score bits the oracle's, zero tails.  fails: the users
    predicted to exceed the frontier limit -- status NANN_ERR_CAPACITY, no rows"""
    st, n_out, ids, scs, idx = (out[f] for f in _FIELDS)
    assert len(st) == len(exp), what
    for b, (rc, eids, esc, eidx) in enumerate(exp):
        if fails is not None and fails[b]:
            rc = W.ERR_CAPACITY
        assert st[b] == rc, (what, b, st[b], rc)
        if rc:
            assert n_out[b] == 0 and not ids[b].any() and not bits(scs[b]).any() and not idx[b].any(), (what, b)
            continue
        n = len(eids)
        assert n_out[b] == n, (what, b, n_out[b], n)
        assert (idx[b, :n] == eidx).all(), (what, b, np.nonzero(idx[b, :n] != eidx)[0][:8])
        assert (ids[b, :n] == eids).all(), (what, b)
        assert (bits(scs[b, :n]) == bits(esc)).all(), (what, b)
        assert not ids[b, n:].any() and not bits(scs[b, n:]).any() and not idx[b, n:].any(), (what, b, "tail")


def _same_bits(a, b, what):
    for f in _FIELDS:
        x, y = (bits(a[f]), bits(b[f])) if f == "scores" else (a[f], b[f])
        assert x.shape == y.shape and (x == y).all(), (what, f)


def _identical_users_agree(out, src, what):
    """users with the same query return the same bits wherever they sit in the batch"""
    first = {}
    for b, s in enumerate(src):
        if s < 0:
            continue
        if s in first:
            a = first[s]
            assert all((out[f][a] == out[f][b]).all() for f in ("status", "n_out", "item_ids", "index")), (what, a, b)
            assert (bits(out["scores"][a]) == bits(out["scores"][b])).all(), (what, a, b)
        first.setdefault(s, b)
    assert len(first) == W.NQ and sum(s >= 0 for s in src) >= 2 * W.NQ, what


def _small(d, dtype):
    key = ("small", d, dtype)
    if key not in _CACHE:
        _CACHE[key] = _device_index(T.table(d, dtype)[0], dtype, T.graph(d)[0])
    return _CACHE[key]


def _fail_users(slots):
    """3 x slots users of the cluster case, `slots` aimed users at the front -> (queries, the predicted failures)"""
    key = ("fail_users", slots)
    if key not in _CACHE:
        q = W.cluster_users(slots, 2 * slots)
        _CACHE[key] = (q, W.predict_failures(q))
    return _CACHE[key]


# ---- the child process: everything under NANN_EVAL_SEEN=hbm -----------------------------------------------------------------
def child_main(spec_path, out_path):
    """runs every case of the pickled spec through _run with form 0 asserted, and writes outputs and plans"""
    spec = pickle.load(open(spec_path, "rb"))
    res = {}
    for name, c in spec.items():
        dix = _device_index(c["rows"], c["dtype"], c["g"], c.get("n"))
        for tag, q, cfg in c["runs"]:
            out = _run(dix, c["dtype"], q, cfg, 0, use_dirty=c.get("use_dirty"))
            assert out["plan"]["form"] == 0   # (recorded per case: the parent asserts it again on what it reads)
            res[name + "/" + tag] = out
        del dix
        torch.cuda.empty_cache()
    pickle.dump(res, open(out_path, "wb"))


_CHILD = ("import sys\nsys.path[:0] = [%r, %r]\nimport test_eval_matrix_gpu as M\nM.child_main(sys.argv[1], sys.argv[2])\n"
          % (ROOT, os.path.join(ROOT, "tests")))
CUS_SLOTS = {0: 2 * W.CUS, 1: W.CUS, 2: W.CUS}   # workgroups of a full batch per form: two per CU in the slot form
SLOTS_SLOT_FORM = CUS_SLOTS[0]


@pytest.fixture(scope="module")
def slot_form(tmp_path_factory):
    """ONE fresh process under NANN_EVAL_SEEN=hbm: the twelve slot-form instances on the small case under both settings, a batch
    of 3 x slots users, the same behind failures, and the sparse case on either side of the use_dirty threshold -> its outputs"""
    tmp = tmp_path_factory.mktemp("eval_slot")
    g64 = {k: T.graph(64)[0][k] for k in ("item_ids", "nb_values", "nb_row_splits", "enter_points")}
    spec = {}
    for d in W.DIMS:
        g = {k: T.graph(d)[0][k] for k in ("item_ids", "nb_values", "nb_row_splits", "enter_points")}
        for dtype in W.DTYPES:
            runs = [("cfg%d" % i, T.graph(d)[1], cfg) for i, cfg in enumerate(W.CFGS)]
            if (d, dtype) == (64, "f16"):
                runs.append(("reuse", W.reuse_queries(64, 3 * SLOTS_SLOT_FORM)[0], W.CFG_CHEAP))
            spec["small_%d_%s" % (d, dtype)] = {"rows": T.table(d, dtype)[0], "dtype": dtype, "g": g, "runs": runs}
    c = W.cluster_case()
    spec["cluster"] = {"rows": c["table"], "dtype": "f16", "g": c["g"], "runs": [("fail", _fail_users(SLOTS_SLOT_FORM)[0], W.CFG_FAIL)]}
    for n in (W.N_DIRTY, W.N_DIRTY + 1):
        spec["sparse_%d" % n] = {"rows": T.table(64, "f16")[0], "dtype": "f16", "g": g64, "n": n, "use_dirty": W.use_dirty(n),
                                 "runs": [("cfg0", W.queries(64, "f16"), W.CFG_SCALED)]}
    pickle.dump(spec, open(tmp / "spec.pkl", "wb"))
    env = dict(os.environ, NANN_EVAL_SEEN="hbm")
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, "-c", _CHILD, str(tmp / "spec.pkl"), str(tmp / "out.pkl")], env=env, capture_output=True,
                       text=True, timeout=300)
    print("the slot-form child: %.1f s" % (time.perf_counter() - t0))
    assert p.returncode == 0, p.stderr[-3000:]
    res = pickle.load(open(tmp / "out.pkl", "rb"))
    assert all(r["plan"]["form"] == 0 for r in res.values()) and len(res) == 12 * 2 + 1 + 1 + 2
    return res


# ---- 3. the matrix ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", W.DTYPES)
@pytest.mark.parametrize("d", W.DIMS)
def test_l2_one_window_and_slot_forms_equal_the_oracle(slot_form, d, dtype):
    """the small case through SEEN_LDS = 1 in process and SEEN_LDS = 0 in the child: both the oracle's bits, hence each
    other's; with counters the same bits, and the counters the per-op spelling's on every third user"""
    dix = _small(d, dtype)
    q = T.graph(d)[1]
    for i, cfg in enumerate(W.CFGS):
        exp = W.expected(d, dtype, cfg)
        assert all(rc == 0 for rc, _, _, _ in exp), "the oracle serves every user"
        lds = _run(dix, dtype, q, cfg, 1, n_windows=1)
        assert claimed("l2", d, dtype, 1) in KERNELS
        _check(lds, exp, (d, dtype, cfg, "lds"))
        slot = slot_form["small_%d_%s/cfg%d" % (d, dtype, i)]
        assert slot["plan"]["form"] == 0 and slot["plan"]["threads"] == NT_L2 and claimed("l2", d, dtype, 0) in KERNELS
        _check(slot, exp, (d, dtype, cfg, "slot"))
        _same_bits(slot, lds, (d, dtype, cfg, "slot form against LDS form"))
    ctr = _run(dix, dtype, q, W.CFG_DRY, 1, n_windows=1, want_counters=True)
    _same_bits(ctr, lds, (d, dtype, "with counters"))
    users = list(W.COUNTER_USERS)
    assert (ctr["counters"][users] == W.expected_counters(d, dtype, W.CFG_DRY)).all(), (d, dtype, ctr["counters"][users])


@pytest.mark.parametrize("dtype", W.DTYPES)
@pytest.mark.parametrize("d", W.DIMS)
def test_l2_window_form_equals_the_oracle(d, dtype):
    """the sparse case of 2 031 617 rows: three windows, nodes on both sides of both seams, the last window one bit wide"""
    n = W.N_SPARSE
    p = W.pi(T.N_ITEMS, n)
    t0 = time.perf_counter()
    dix = _device_index(T.table(d, dtype)[0], dtype, T.graph(d)[0], n)
    for cfg in W.CFGS:
        small = W.expected(d, dtype, cfg, aimed=True)
        assert (small[-1][3] == T.N_ITEMS - 1).any(), "the graph's last node, the third window's one row, is in an answer"
        exp = W.through(small, p)
        out = _run(dix, dtype, W.queries(d, dtype), cfg, 2, n_windows=3)
        assert claimed("l2", d, dtype, 2) in KERNELS
        _check(out, exp, (d, dtype, cfg, "windows"))
        assert {int(x) // W.WIN_ITEMS for x in out["index"][0][:out["n_out"][0]]} <= {0, 1, 2}
    rows = np.concatenate([e[3] for e in exp])
    assert len({int(x) // W.WIN_ITEMS for x in rows}) >= 2, "the answers lie in more than one window"
    print("windows d=%d %s: %.2f s" % (d, dtype, time.perf_counter() - t0))


@pytest.mark.parametrize("dtype", W.ATTN_DTYPES)
@pytest.mark.parametrize("d", W.ATTN_DIMS)
def test_attention_instances(tmp_path, d, dtype):
    """nann_search_eval_model on the small case: status and n_out the oracle's, every score of every user's valid rows within
    RTOL (test_attn_shapes_gpu.py) of the oracle's logit of that row, and a split weights directory the bits of an exact one"""
    from nann_amd import ops, retrieval
    from test_attn_shapes_gpu import RTOL, _oracle_rows, _within
    dix, seqs = _small(d, dtype), W.attn_seqs()
    exp = W.expected_attn(d, dtype)
    assert all(rc == 0 for rc, _, _, _ in exp), "the oracle serves every user"
    out = {}
    for prec in ("exact", "split"):
        ops.save_scorer_dir(str(tmp_path / prec), "attention", W.attn_weights(d), precision=prec)
        model = ops.Model(str(tmp_path / prec), d, W.ATTN_L, emb_dtype=_TORCH_DT[dtype])
        plan = retrieval.search_eval_plan(dix, model, len(seqs))
        assert plan["form"] == 0 and plan["threads"] == NT_ATTN and plan["slots"] == len(seqs), plan
        assert (LPR[d], DT[dtype], SC_ATTN, plan["threads"], plan["form"]) == claimed("attn", d, dtype, 0) in KERNELS
        r = retrieval.search_eval(dix, model, cuda(seqs), *W.ATTN_CFG)
        torch.cuda.synchronize()
        out[prec] = {f: getattr(r, f).cpu().numpy() for f in _FIELDS}
    a = out["exact"]
    assert (a["status"] == 0).all() and (a["n_out"] == [len(e[1]) for e in exp]).all(), (a["status"], a["n_out"])
    host = T.table(d, dtype)[0]
    own = _oracle_rows(W.attn_oracle_model(d, dtype), seqs, [host[a["index"][b, :a["n_out"][b]]] for b in range(len(seqs))])
    worst = max(_within(a["scores"][b, :a["n_out"][b]], own[b]) for b in range(len(seqs)))
    print("attention eval d=%d %s: rescored max err %.3g" % (d, dtype, worst))
    assert worst <= RTOL, worst
    ids = T.graph(d)[0]["item_ids"]
    for b in range(len(seqs)):
        n = a["n_out"][b]
        assert (a["item_ids"][b, :n] == ids[a["index"][b, :n]]).all() and not a["item_ids"][b, n:].any() and not bits(a["scores"][b, n:]).any()
    _same_bits(out["split"], a, (d, dtype, "split against exact"))


# ---- 4. the boundaries of the dispatch, d = 64 f16 --------------------------------------------------------------------------
def _sparse_run(n, form, n_windows, use_dirty=None, cfg=W.CFG_SCALED):
    p = W.pi(T.N_ITEMS, n)
    small = W.expected(64, "f16", cfg, aimed=True)
    assert (small[-1][3] == T.N_ITEMS - 1).any() and p[-1] == n - 1, "some user's answer holds the last node, row n - 1"
    exp = W.through(small, p)
    t0 = time.perf_counter()
    dix = _device_index(T.table(64, "f16")[0], "f16", T.graph(64)[0], n)
    out = _run(dix, "f16", W.queries(64, "f16"), cfg, form, n_windows=n_windows, use_dirty=use_dirty)
    _check(out, exp, (n, "form", form))
    print("n = %d: form %d, %d windows, use_dirty %d: launch %.2f s, test %.2f s"
          % (n, form, out["plan"]["n_windows"], out["plan"]["use_dirty"], out["seconds"], time.perf_counter() - t0))
    return out


def test_one_full_window_and_one_row_more():
    """992 owners, a window exactly full -> SEEN_LDS = 1; one row more -> two windows, the second one bit wide.  The row n - 1
    is a node that some user's answer holds."""
    assert W.windows(W.N_ONE_WINDOW) == (W.WIN_OWNERS, 1, 1) and W.windows(W.N_TWO_WINDOWS) == (W.WIN_OWNERS + 1, 2, 2)
    _sparse_run(W.N_ONE_WINDOW, 1, 1)
    _sparse_run(W.N_TWO_WINDOWS, 2, 2)


def test_eight_windows_and_one_row_more(slot_form):
    """8 126 464 rows: eight windows, the LDS form's last; one row more: the slot form in process.  The slot form keeps the
    second-level bitmap of `seen` up to W.N_DIRTY = 4 718 592 rows (eval_matrix.py derives it from eval_dirty_room()) and scans
    `seen` whole beyond: 8 126 465 is beyond, and the child runs the slot form at 4 718 592 and 4 718 593 rows."""
    assert W.use_dirty(W.N_DIRTY) == 1 and W.use_dirty(W.N_DIRTY + 1) == 0 and W.N_SLOT > W.N_DIRTY
    _sparse_run(W.N_EIGHT_WINDOWS, 2, 8)
    _sparse_run(W.N_SLOT, 0, 9, use_dirty=0)
    for n in (W.N_DIRTY, W.N_DIRTY + 1):
        out = slot_form["sparse_%d/cfg0" % n]
        assert out["plan"]["form"] == 0 and out["plan"]["use_dirty"] == W.use_dirty(n), out["plan"]
        _check(out, W.through(W.expected(64, "f16", W.CFG_SCALED, aimed=True), W.pi(T.N_ITEMS, n)), (n, "slot form in the child"))
        print("n = %d in the child: use_dirty %d, launch %.2f s" % (n, out["plan"]["use_dirty"], out["seconds"]))


@pytest.mark.parametrize("row_len,form", [(W.ROW_LEN_LDS, 1), (W.ROW_LEN_LDS + 1, 0)])
def test_a_row_of_65535_neighbours_and_one_more(row_len, form):
    """a hub whose level-0 row holds 65 535 distinct neighbours runs in the LDS form (the length fills its 16 bits), 65 536
    in the slot form; the users that walk the hub gather at least that many neighbours"""
    c = W.hub_case(row_len)
    users, on_hub, widest = W.hub_users(row_len)
    assert on_hub.sum() >= 1 and (~on_hub).sum() == 2 and widest <= W.FRONTIER_MAX
    q = T.graph(64)[1][users]
    exp = W.run_oracle(c["oix"], 64, "f16", q, W.CFG_SCALED)
    assert all(rc == 0 and (rows < T.N_ITEMS).all() for rc, _, _, rows in exp), "no filler row is kept"
    dix = _device_index(c["table"], "f16", c["g"])
    assert max(dix.max_deg) == row_len
    out = _run(dix, "f16", q, W.CFG_SCALED, form, n_windows=1, want_counters=True)
    _check(out, exp, ("hub", row_len))
    g = out["counters"][:, 1]
    assert (g[on_hub] >= row_len).all() and (g[~on_hub] < W.ROW_LEN_LDS).all(), g


@pytest.mark.parametrize("form", [1, 2])
def test_slots_taken_over_by_later_users(form):
    """3 x slots users in one batch, so that every slot serves a second and a third user behind a success (`seen` is left
    clear, not cleared): every user the oracle's, identical queries identical bits"""
    n_users = 3 * W.CUS
    q, src = W.reuse_queries(64, n_users)
    exp = W.expected_reuse(64, "f16", n_users)
    if form == 1:
        dix = _small(64, "f16")
    else:
        exp = W.through(exp, W.pi(T.N_ITEMS, W.N_SPARSE))
        dix = _device_index(T.table(64, "f16")[0], "f16", T.graph(64)[0], W.N_SPARSE)
    out = _run(dix, "f16", q, W.CFG_CHEAP, form)
    assert out["plan"]["slots"] * 3 == n_users
    _check(out, exp, ("reuse", form))
    _identical_users_agree(out, src, ("reuse", form))


def test_slot_form_slots_taken_over_by_later_users(slot_form):
    n_users = 3 * SLOTS_SLOT_FORM
    out = slot_form["small_64_f16/reuse"]
    assert out["plan"]["form"] == 0 and out["plan"]["slots"] * 3 == n_users
    _check(out, W.expected_reuse(64, "f16", n_users), ("reuse", 0))
    _identical_users_agree(out, W.reuse_queries(64, n_users)[1], ("reuse", 0))


def _check_behind_failures(out, q, fails, slots, what, p=None):
    assert fails[:slots].all() and fails.sum() >= slots and (~fails).sum() >= slots, (what, int(fails.sum()))
    exp = W.run_oracle(W.cluster_case()["oix"], 64, "f16", q, W.CFG_FAIL)
    _check(out, exp if p is None else W.through(exp, p), what, fails=fails)


def test_slots_taken_over_behind_failed_users(slot_form):
    """the cluster case: the first `slots` users of 3 x slots exceed the frontier limit (NANN_ERR_CAPACITY, predicted on the CPU
    from the per-op spelling's frontiers), so every slot's second user starts behind a failure and has to clear `seen` whole.
    The device's status is the prediction's for every user, every other user the oracle's; the LDS and the window form in process,
    the slot form in the child."""
    c = W.cluster_case()
    q, fails = _fail_users(W.CUS)
    out = _run(_device_index(c["table"], "f16", c["g"]), "f16", q, W.CFG_FAIL, 1, n_windows=1)
    assert out["plan"]["slots"] == W.CUS
    _check_behind_failures(out, q, fails, W.CUS, "behind failures, LDS form")
    n = W.N_SPARSE   # the same graph relabelled into three windows: the window form
    out = _run(_device_index(c["table"], "f16", c["g"], n), "f16", q, W.CFG_FAIL, 2, n_windows=3)
    _check_behind_failures(out, q, fails, W.CUS, "behind failures, window form", p=W.pi(len(c["table"]), n))
    q, fails = _fail_users(SLOTS_SLOT_FORM)
    slot = slot_form["cluster/fail"]
    assert slot["plan"]["form"] == 0 and slot["plan"]["slots"] == SLOTS_SLOT_FORM
    _check_behind_failures(slot, q, fails, SLOTS_SLOT_FORM, "behind failures, slot form")


def test_the_plan_query_refuses_what_the_call_refuses():
    from nann_amd import ops, retrieval
    dix = _small(64, "f16")
    with pytest.raises(ops.NannError) as e:
        retrieval.search_eval_plan(dix, ops.Scorer("ip", 64, torch.float16), 4)
    assert e.value.status == 102 and "NANN_SCORER_IP" in str(e.value)
    with pytest.raises(ops.NannError) as e2:
        retrieval.search_eval(dix, ops.Scorer("ip", 64, torch.float16), cuda(T.graph(64)[1][:4]))
    assert e2.value.status == e.value.status
