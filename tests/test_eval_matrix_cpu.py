"""CPU: what the evaluation-traversal matrix (test_eval_matrix_gpu.py) rests on, checked without a device -- its table of
kernels is the build's own list of k_search_eval instances outside the MLP scorer, with the MLP matrix's six it is every
k_search_eval compiled, its launches enter every entry, and its workload (eval_matrix.py) meets the conditions under which a
pass means something."""
import os
import re

import numpy as np
import pytest

import eval_matrix as W
import traverse_matrix as T
from test_eval_matrix_gpu import CUS_SLOTS, KERNELS, LAUNCHES, SC_ATTN, SC_L2, claimed

_NAME = re.compile(r"Function Name: \S*?\dk_search_evalILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EL[ib](\d+)EEE")
_SC_MLP = 1  # NANN_SCORER_MLP


def compiled_kernels(out_dir, units):
    """the (LPR, DT, SC, NT, SEEN_LDS) of every k_search_eval that the units' resource reports (<obj>.d/compile.log, what
    build.check_resources walks) name.  Kernel names only: no assembly is opened."""
    found = set()
    for obj, _ in units:
        log = os.path.join(out_dir, obj[:-2] + ".d", "compile.log")
        assert os.path.exists(log), "no resource report for the unit %s (%s)" % (obj, log)
        for m in _NAME.finditer(open(log, errors="replace").read()):
            found.add(tuple(int(v) for v in m.groups()))
    return found


def test_the_table_is_what_the_build_compiled():
    """a new instantiation fails here until the matrix launches it; so does an entry no dispatch can reach any more"""
    from nann_amd import build
    from test_mlp_matrix_gpu import KERNELS as MLP_KERNELS
    build.build()
    found = compiled_kernels(build.OUT_DIR, build.UNITS)
    ours = {k for k in found if k[2] != _SC_MLP}
    table = set(KERNELS)
    assert not ours - table, ("compiled, not in the matrix", sorted(ours - table))
    assert not table - ours, ("in the matrix, not compiled", sorted(table - ours))
    assert len(table) == len(KERNELS) == 40 and {k[2] for k in table} == {SC_L2, SC_ATTN}
    assert sum(k[4] == form for k in table for form in (0,)) == 12 + 4 and all(sum(k[4] == f for k in table) == 12 for f in (1, 2))
    # with the six evaluation traversals of the MLP matrix: every k_search_eval there is
    mlp = {k[1:] for k in MLP_KERNELS if k[0] == "k_search_eval"}
    assert len(mlp) == 6 and mlp == found - ours and len(found) == 46


def test_a_unit_without_a_report_is_named(tmp_path):
    from nann_amd import build
    with pytest.raises(AssertionError, match="nann_core.o"):
        compiled_kernels(str(tmp_path), build.UNITS)


def test_the_name_pattern_keeps_the_evaluation_traversal_only(tmp_path):
    d = tmp_path / "u.d"
    d.mkdir()
    (d / "compile.log").write_text(
        "remark: x:1:0: Function Name: _ZN4nann13k_search_evalILi16ELi0ELi0ELi1024ELi2EEEvNS_8EvalArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann13k_search_evalILi8ELi1ELi3ELi512ELi0EEEvNS_8EvalArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann13k_search_evalILi32ELi1ELi1ELi512ELi0EEEvNS_8EvalArgsE\n"   # the MLP scorer's
        "remark: x:1:0: Function Name: _ZN4nann8k_searchILi16ELi0ELi2ELi0ELi512EEEvNS_10SearchArgsE\n"       # the serving traversal
        "remark: x:1:0: Function Name: _ZN4nann13k_search_leanILi64ELi2ELi3ELi0ELi1024EEEvNS_10SearchArgsE\n")
    assert compiled_kernels(str(tmp_path), [("u.o", [])]) == {(16, 0, 0, 1024, 2), (8, 1, 3, 512, 0), (32, 1, 1, 512, 0)}


def test_the_launches_enter_every_kernel_of_the_table():
    entered = [claimed(*launch) for launch in LAUNCHES]
    assert len(entered) == len(set(entered)) == 40 and set(entered) == set(KERNELS)


def test_the_window_arithmetic_of_the_constants():
    """restated in numpy from bm_words (one bit per row, padded to four words) and 992 owners of 32 words a window"""
    def restated(n):
        words = int(np.ceil(np.ceil(n / 32) / 4) * 4)
        owners = int(np.ceil(words / 32))
        return owners, int(np.ceil(owners / min(owners, 992)))
    assert W.WIN_ITEMS == 992 * 32 * 32 == 1015808
    for n, owners, wins, form in ((W.N_ONE_WINDOW, 992, 1, 1), (W.N_TWO_WINDOWS, 993, 2, 2), (W.N_SPARSE, 1985, 3, 2),
                                  (W.N_EIGHT_WINDOWS, 7936, 8, 2), (W.N_SLOT, 7937, 9, 0), (W.N_DIRTY, 4608, 5, 2), (W.N_DIRTY + 1, 4609, 5, 2)):
        assert restated(n) == (owners, wins) and W.windows(n) == (owners, wins, form), n
    assert (W.N_ONE_WINDOW, W.N_TWO_WINDOWS, W.N_SPARSE, W.N_EIGHT_WINDOWS, W.N_SLOT) == (1015808, 1015809, 2031617, 8126464, 8126465)
    # the second-level bitmap: 256 + 4 bytes per owner within eval_dirty_room() = 18 688
    assert W.DIRTY_ROOM == 18688 and W.N_DIRTY == 4718592
    assert 256 + 4 * restated(W.N_DIRTY)[0] == W.DIRTY_ROOM and W.use_dirty(W.N_DIRTY) == 1 and W.use_dirty(W.N_DIRTY + 1) == 0
    assert W.use_dirty(W.N_SLOT) == 0


def test_pi_puts_nodes_in_every_window_and_on_both_sides_of_every_seam():
    for n in (W.N_ONE_WINDOW, W.N_TWO_WINDOWS, W.N_SPARSE, W.N_EIGHT_WINDOWS, W.N_SLOT, W.N_DIRTY, W.N_DIRTY + 1):
        p = W.pi(T.N_ITEMS, n)
        assert (np.diff(p) > 0).all() and p[0] >= 0 and p[-1] == n - 1
        wins = W.windows(n)[1]
        assert set((p // W.WIN_ITEMS).tolist()) == set(range(wins)), n
        for seam in range(W.WIN_ITEMS, n, W.WIN_ITEMS):
            assert seam - 1 in p and seam in p, (n, seam)
    assert {1015807, 1015808} <= set(W.pi(T.N_ITEMS, W.N_SPARSE).tolist())


@pytest.mark.parametrize("d,dtype,n", [(64, "f16", W.N_SPARSE), (64, "bf16", W.N_SPARSE), (128, "f32", W.N_SPARSE), (256, "bf16", W.N_SPARSE),
                                       (512, "f32", W.N_SPARSE), (64, "f16", W.N_ONE_WINDOW), (64, "f16", W.N_TWO_WINDOWS),
                                       (64, "f16", W.N_SLOT)])
def test_the_oracle_on_the_relabelled_graph_is_the_small_answer_through_pi(d, dtype, n):
    """guards the construction of the sparse case, not a kernel; and a pi shifted behind a seam is not the oracle's answer"""
    cfg = W.CFG_SCALED
    p, got = W.oracle_on_sparse(d, dtype, n, cfg)
    small = W.expected(d, dtype, cfg, aimed=True)
    assert len(got) == W.NQ + 1 and all(e[0] == 0 for e in got) and W.same_answers(got, W.through(small, p))
    assert (got[-1][3] == n - 1).any(), "the answer of the user aimed at it holds the last row"
    if n > W.WIN_ITEMS:
        assert not W.same_answers(got, W.through(small, p, shift_from=W.WIN_ITEMS))


@pytest.mark.parametrize("d", W.DIMS)
def test_the_oracle_serves_every_user_of_the_small_case(d):
    for dtype in W.DTYPES:
        for cfg in W.CFGS:
            exp = W.expected(d, dtype, cfg)
            assert len(exp) == W.NQ and all(rc == 0 and len(ids) == min(cfg[2], cfg[1][0]) for rc, ids, _, _ in exp), (d, dtype, cfg)
    # the second setting: k above what the start level and level 1 hold, and frontiers that run dry on both levels
    g = T.graph(d)[0]
    assert len(g["enter_points"]) < W.CFG_DRY[1][2] and int((np.diff(g["nb_row_splits"][1]) > 0).sum()) < W.CFG_DRY[1][1]
    for fr in W.walks({"g": g, "table": T.table(d, "f16")[0]}, T.graph(d)[1][:6], W.CFG_DRY, d, "f16"):
        assert any(lvl == 1 and len(ids) == 0 for lvl, ids in fr) and any(lvl == 0 and len(ids) == 0 for lvl, ids in fr)
        assert max(len(ids) for _, ids in fr) <= W.FRONTIER_MAX


@pytest.mark.parametrize("d,dtype", [(d, t) for d in W.ATTN_DIMS for t in W.ATTN_DTYPES])
def test_the_oracle_serves_every_user_under_the_attention_model(d, dtype):
    exp = W.expected_attn(d, dtype)
    assert len(exp) == W.NQ and all(rc == 0 and len(ids) == W.ATTN_CFG[2] for rc, ids, _, _ in exp)


@pytest.mark.parametrize("row_len", [W.ROW_LEN_LDS, W.ROW_LEN_LDS + 1])
def test_the_hub_is_walked_and_no_filler_is_kept(row_len):
    c = W.hub_case(row_len)
    assert int(np.diff(c["g"]["nb_row_splits"][0]).max()) == row_len
    users, on_hub, widest = W.hub_users(row_len)
    assert on_hub.sum() >= 1 and (~on_hub).sum() == 2 and widest <= W.FRONTIER_MAX
    exp = W.run_oracle(c["oix"], 64, "f16", T.graph(64)[1][users], W.CFG_SCALED)
    assert all(rc == 0 and (rows < T.N_ITEMS).all() for rc, _, _, rows in exp)
    # a filler scores far below every kept score: it cannot tie into a threshold
    q = T.graph(64)[1][users]
    filler = -((q - W.HUB_FILL) ** 2).sum(axis=1)
    assert all(filler[b] < 4 * float(exp[b][2].min()) < 0 for b in range(len(users))), (filler, [float(e[2].min()) for e in exp])


@pytest.mark.parametrize("slots", sorted(set(CUS_SLOTS.values())))
def test_the_reuse_batches_are_served_and_hold_identical_users(slots):
    q, src = W.reuse_queries(64, 3 * slots)
    exp = W.expected_reuse(64, "f16", 3 * slots)
    assert len(exp) == 3 * slots and all(rc == 0 and len(ids) == W.CFG_CHEAP[2] for rc, ids, _, _ in exp)
    assert (src >= 0).sum() >= 2 * W.NQ and set(src[src >= 0].tolist()) == set(range(W.NQ))
    assert all((q[b] == T.graph(64)[1][s]).all() for b, s in enumerate(src) if s >= 0)
    assert len({q[b].tobytes() for b in range(len(q))}) == len(q) - int((src >= 0).sum()) + W.NQ


@pytest.mark.parametrize("slots", sorted(set(CUS_SLOTS.values())))
def test_the_cluster_case_fails_and_serves_enough_users(slots):
    """at least `slots` users predicted to exceed the frontier limit -- the first `slots` of the batch among them -- and at
    least `slots` predicted to succeed; the oracle, which has no such limit, serves them all"""
    from test_eval_matrix_gpu import _fail_users
    q, fails = _fail_users(slots)
    assert len(q) == 3 * slots and fails[:slots].all() and fails.sum() >= slots and (~fails).sum() >= slots, int(fails.sum())
    c = W.cluster_case()
    assert int(np.diff(c["g"]["nb_row_splits"][0]).max()) == W.CLUSTER > W.FRONTIER_MAX
    assert (c["table"][T.N_ITEMS:] == c["table"][c["anchor"]]).all()
    assert all(rc == 0 for rc, _, _, _ in W.run_oracle(c["oix"], 64, "f16", q[::7], W.CFG_FAIL))


def test_the_plan_query_checks_its_arguments_without_a_device():
    import ctypes as C
    from nann_amd import _lib
    L, plan = _lib.lib(), _lib.EvalPlan()
    assert "nann_search_eval_plan" in _lib.SYMBOLS and C.sizeof(plan) == 24
    assert L.nann_search_eval_plan(None, None, None, 4, C.byref(plan)) == 7   # NANN_ERR_BAD_ARGUMENT
    assert "nann_search_eval_plan" in _lib.last_error()
    assert L.nann_abi_version() == 6   # a new symbol, the version unchanged
