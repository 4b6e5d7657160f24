"""CPU: what the MLP matrix (test_mlp_matrix_gpu.py) rests on, checked without a device -- its table of kernels is the
build's own list of MLP-scorer kernels, its launches enter every entry of the table, and its workload meets the conditions
under which a pass means something (mlp_matrix.check_conditions: enough requests served, enough of them decisive, the oracle
and the float64 schedule at one on those, the oracle's scores within its bound of float64)."""
import os
import re

import numpy as np
import pytest

import mlp_matrix as W
from test_mlp_matrix_gpu import KERNELS, LAUNCHES, claimed

# <name>I<template arguments>E of the kernels the MLP scorer compiles to; k_search and k_search_eval are kept by their SC
_NAME = re.compile(r"Function Name: \S*?\d(k_search_eval|k_search|k_mlp_phase_score|k_mlp_phase_certify|k_mlp_preproject|k_score_mlp2|k_score_mlp)"
                   r"I((?:L[ib]\d+E)+)E")
_MLP_SC = {"k_search": (4, (1, 2, 7, 8, 9)), "k_search_eval": (3, (1,))}  # kernel: (position of SC in its entry, the MLP's values)


def compiled_kernels(out_dir, units):
    """(kernel, template arguments ...) of every MLP-scorer kernel that the units' resource reports (<obj>.d/compile.log, what
    build.check_resources walks) name.  Kernel names only: no assembly is opened."""
    found = set()
    for obj, _ in units:
        log = os.path.join(out_dir, obj[:-2] + ".d", "compile.log")
        assert os.path.exists(log), "no resource report for the unit %s (%s)" % (obj, log)
        for m in _NAME.finditer(open(log, errors="replace").read()):
            t = (m.group(1),) + tuple(int(v) for v in re.findall(r"L[ib](\d+)E", m.group(2)))
            if m.group(1) not in _MLP_SC or t[_MLP_SC[m.group(1)][0]] in _MLP_SC[m.group(1)][1]:
                found.add(t)
    return found


def test_the_table_is_what_the_build_compiled():
    """a new instantiation fails here until the matrix launches it; so does an entry no dispatch can reach any more"""
    from nann_amd import build
    build.build()
    found = compiled_kernels(build.OUT_DIR, build.UNITS)
    table = set(KERNELS)
    assert not found - table, ("compiled, not in the matrix", sorted(found - table))
    assert not table - found, ("in the matrix, not compiled", sorted(table - found))
    # 36 traversal kernels (30 on the embedding rows, 4 with layer 2 resident, 2 stages), 5 scoring launches of the pipeline,
    # 2 table builders, 12 stand-alone scorers, 6 evaluation traversals
    assert len(table) == len(KERNELS) == 61, "an entry twice, or not the 61 kernels of the MLP scorer"


def test_the_name_pattern_keeps_the_mlp_kernels_only(tmp_path):
    d = tmp_path / "u.d"
    d.mkdir()
    (d / "compile.log").write_text(
        "remark: x:1:0: Function Name: _ZN4nann8k_searchILi16ELi0ELi1ELi1ELi512EEEvNS_10SearchArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann8k_searchILi8ELi1ELi2ELi2ELi256EEEvNS_10SearchArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann8k_searchILi16ELi0ELi3ELi9ELi1024EEEvNS_10SearchArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann8k_searchILi16ELi0ELi2ELi12ELi512EEEvNS_10SearchArgsE\n"      # the inner product
        "remark: x:1:0: Function Name: _ZN4nann8k_searchILi16ELi0ELi2ELi0ELi512EEEvNS_10SearchArgsE\n"       # L2
        "remark: x:1:0: Function Name: _ZN4nann13k_search_leanILi64ELi2ELi3ELi0ELi1024EEEvNS_10SearchArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann13k_search_evalILi16ELi0ELi0ELi1024ELb1EEEvNS_8EvalArgsE\n"  # L2's evaluation traversal
        "remark: x:1:0: Function Name: _ZN4nann13k_search_evalILi32ELi1ELi1ELi512ELb0EEEvNS_8EvalArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann17k_mlp_phase_scoreILb0ELi2EEEvNS_14PhaseScoreArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann19k_mlp_phase_certifyILi256EEEvNS_14PhaseScoreArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann16k_mlp_preprojectILi1EEEvPKvxiPKfPf\n"
        "remark: x:1:0: Function Name: _ZN4nann11k_score_mlpILi256ELi0ELb1EEEvNS_9MlpParamsEPKvxPKixPKfPfPNS_8OpResultE\n"
        "remark: x:1:0: Function Name: _ZN4nann12k_score_mlp2ILi64ELi1EEEvNS_9MlpParamsEPKvxPKixPKfPfPNS_8OpResultE\n"
        "remark: x:1:0: Function Name: _ZN4nann10k_score_l2ILi16ELi0EEEvPKvxiPKixPKfPfPNS_8OpResultE\n"
        "remark: x:1:0: Function Name: _ZN4nann9k_scan_ipILi16ELi0ELi16EEEvPKvxPKfiiPf\n")
    assert compiled_kernels(str(tmp_path), [("u.o", [])]) == {
        ("k_search", 16, 0, 1, 1, 512), ("k_search", 8, 1, 2, 2, 256), ("k_search", 16, 0, 3, 9, 1024),
        ("k_search_eval", 32, 1, 1, 512, 0), ("k_mlp_phase_score", 0, 2), ("k_mlp_phase_certify", 256), ("k_mlp_preproject", 1),
        ("k_score_mlp", 256, 0, 1), ("k_score_mlp2", 64, 1)}


def test_a_unit_without_a_report_is_named(tmp_path):
    from nann_amd import build
    with pytest.raises(AssertionError, match="nann_core.o"):
        compiled_kernels(str(tmp_path), build.UNITS)


def test_the_launches_enter_every_kernel_of_the_table():
    entered = [k for d in W.DIMS for dtype in W.DTYPES for launch in LAUNCHES for k in claimed(d, dtype, launch)]
    assert len(LAUNCHES) == 19 and set(entered) == set(KERNELS)
    # per case: the kernels of its own d and dtype once each, but the split hash-set kernel on the embedding rows and the exact
    # LDS-bitmap one twice (uniform and per-request level_topn), and the table's builder three times (one table per scorer)
    per_case = {k: entered.count(k) for k in claimed(64, "bf16", LAUNCHES[0]) + claimed(64, "bf16", LAUNCHES[2]) + [("k_mlp_preproject", 1)]}
    assert per_case == {("k_search", 8, 1, 0, 1, 512): 2, ("k_search", 8, 1, 2, 2, 256): 2, ("k_mlp_preproject", 1): 9}


def test_threads_of_the_split_hash_set_kernel():
    """the second mapping's 256 threads at d <= 128 and nowhere else: what nann_search_plan.threads has to report"""
    from test_mlp_matrix_gpu import rows_threads
    assert [rows_threads(d, "split", "lds_hash") for d in W.DIMS] == [256, 256, 512]
    assert {rows_threads(d, p, m) for d in W.DIMS for p in ("exact", "split") for m in ("lds_bitmap", "hbm_bitmap")} == {512}


@pytest.mark.parametrize("dtype", W.DTYPES)
@pytest.mark.parametrize("d", W.DIMS)
def test_the_workload_catches_something(d, dtype):
    """the conditions the matrix asserts per case, here on the CPU: a failure of the workload, not of a device"""
    W.check_conditions(d, dtype)
    # the evaluation traversal's six users are all served, with the full list
    assert all(rc == 0 and len(ids) == W.EVAL_CFG[2] for rc, ids, _, _ in W.expected_eval(d, dtype))
    # the oracle's stand-alone scores of the whole table are within its bound of float64 too
    q = W.graph(d)[1][0]
    ref = W.scores64(d, dtype, q, np.arange(W.N_ITEMS))
    err = np.abs(W.oracle_scores_all(d, dtype, q).astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
    assert err.max() <= W.ORACLE_TOL, (d, dtype, float(err.max()))


def test_the_float64_reference_tells_the_slopes_apart():
    """scores64 with alpha1 / alpha2 negated is further from the oracle than any tolerance of the matrix: the reference is not
    blind to the PReLU slopes (both signs occur)"""
    d, dtype = 128, "f16"
    w = dict(W.weights(d))
    assert (w["alpha1"] < 0).any() and (w["alpha1"] > 0).any() and (w["alpha2"] < 0).any() and (w["alpha2"] > 0).any()
    w["alpha1"], w["alpha2"] = -w["alpha1"], -w["alpha2"]
    q = W.graph(d)[1][0]
    rows = np.arange(256)
    good, bad = W.scores64(d, dtype, q, rows), W.scores64(d, dtype, q, rows, w)
    assert np.abs(good - bad).min() > 100 * W.MARGIN
