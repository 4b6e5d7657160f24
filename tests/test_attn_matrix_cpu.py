"""CPU: what the attention matrix (test_attn_matrix_gpu.py) rests on, checked without a device -- its table of kernels is the
build's own list of attention-scorer kernels, its launches enter every entry of the table, its workload meets the conditions
under which a pass means something (attn_matrix.check_conditions: enough requests served, enough of them decisive, the oracle
and the float64 schedule at one on those, the oracle's scores within its bound of float64), and its float64 reference tells
each of attn_reference.WRONG_VARIANTS apart at this gain."""
import os
import re

import numpy as np
import pytest

import attn_matrix as W
from attn_reference import WRONG_VARIANTS
from test_attn_matrix_gpu import KERNELS, LAUNCHES, RERUN_LAUNCHES, claimed

# <name>[I<template arguments>E] of the kernels the attention scorer compiles to; k_search is kept by its SC.  k_search_eval and
# k_search_lean do not match: the name must end where the template arguments (or, without any, the parameter list) begin
_NAME = re.compile(r"Function Name: \S*?\d(k_search|k_score_attn_split|k_score_attn|k_attn_prepare_split|k_attn_prepare|k_attn_preproject|"
                   r"k_scan_attn|k_cand_score_attn)(?:I((?:L[ib]\d+E)+)E|E)")
_ATTN_SC = (3, 4, 6, 10, 11)   # kScorerAttn, kScorerAttnSplit, kScorerAttnProj, kScorerAttnXProj, kScorerAttnRes: position 4 of a k_search entry


def compiled_kernels(out_dir, units):
    """(kernel, template arguments ...) of every attention-scorer kernel that the units' resource reports (<obj>.d/compile.log,
    what build.check_resources walks) name.  Kernel names only: no assembly is opened."""
    found = set()
    for obj, _ in units:
        log = os.path.join(out_dir, obj[:-2] + ".d", "compile.log")
        assert os.path.exists(log), "no resource report for the unit %s (%s)" % (obj, log)
        for m in _NAME.finditer(open(log, errors="replace").read()):
            t = (m.group(1),) + tuple(int(v) for v in re.findall(r"L[ib](\d+)E", m.group(2) or ""))
            if m.group(1) != "k_search" or t[4] in _ATTN_SC:
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
    # 30 traversal kernels (24 on the embedding rows, 5 on the table, 1 resident), 8 stand-alone scorers, 2 prepare kernels, 2 table
    # builders, 2 scans, 2 candidate-list scorers; k_search<16, 0, 2, 6, 512> (the table's split form on the hash set), reachable by
    # no call, is not compiled
    assert len(table) == len(KERNELS) == 46, "an entry twice, or not the 46 kernels of the attention scorer"
    assert ("k_search", 16, 0, 2, 6, 512) not in found


def test_the_name_pattern_keeps_the_attention_kernels_only(tmp_path):
    d = tmp_path / "u.d"
    d.mkdir()
    (d / "compile.log").write_text(
        "remark: x:1:0: Function Name: _ZN4nann8k_searchILi8ELi1ELi2ELi3ELi512EEEvNS_10SearchArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann8k_searchILi16ELi0ELi1ELi4ELi512EEEvNS_10SearchArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann8k_searchILi16ELi0ELi0ELi6ELi512EEEvNS_10SearchArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann8k_searchILi16ELi0ELi2ELi10ELi512EEEvNS_10SearchArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann8k_searchILi16ELi0ELi2ELi11ELi512EEEvNS_10SearchArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann8k_searchILi16ELi0ELi1ELi1ELi512EEEvNS_10SearchArgsE\n"       # the MLP, exact
        "remark: x:1:0: Function Name: _ZN4nann8k_searchILi8ELi1ELi2ELi2ELi256EEEvNS_10SearchArgsE\n"        # the MLP, split
        "remark: x:1:0: Function Name: _ZN4nann8k_searchILi16ELi0ELi2ELi7ELi512EEEvNS_10SearchArgsE\n"       # the MLP, layer 2 resident
        "remark: x:1:0: Function Name: _ZN4nann8k_searchILi16ELi0ELi3ELi9ELi1024EEEvNS_10SearchArgsE\n"      # the MLP's pipeline stage
        "remark: x:1:0: Function Name: _ZN4nann8k_searchILi16ELi0ELi2ELi12ELi512EEEvNS_10SearchArgsE\n"      # the inner product
        "remark: x:1:0: Function Name: _ZN4nann8k_searchILi16ELi0ELi2ELi0ELi512EEEvNS_10SearchArgsE\n"       # L2
        "remark: x:1:0: Function Name: _ZN4nann13k_search_leanILi64ELi2ELi3ELi0ELi1024EEEvNS_10SearchArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann13k_search_evalILi8ELi0ELi3ELi512ELi0EEEvNS_8EvalArgsE\n"    # the attention scorer's four
        "remark: x:1:0: Function Name: _ZN4nann13k_search_evalILi8ELi1ELi3ELi512ELi0EEEvNS_8EvalArgsE\n"    # evaluation traversals:
        "remark: x:1:0: Function Name: _ZN4nann13k_search_evalILi16ELi0ELi3ELi512ELi0EEEvNS_8EvalArgsE\n"   # test_eval_matrix_gpu.py's
        "remark: x:1:0: Function Name: _ZN4nann13k_search_evalILi16ELi1ELi3ELi512ELi0EEEvNS_8EvalArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann14k_attn_prepareENS_10AttnParamsEPKtPfS3_\n"
        "remark: x:1:0: Function Name: _ZN4nann20k_attn_prepare_splitENS_10AttnParamsEPKtPtS3_\n"
        "remark: x:1:0: Function Name: _ZN4nann12k_score_attnILi128ELi1EEEvNS_10AttnParamsEPKfS3_PKvxPKixPfPx\n"
        "remark: x:1:0: Function Name: _ZN4nann18k_score_attn_splitILi64ELi0EEEvNS_10AttnParamsEPKfS3_PKvxPKixPfPx\n"
        "remark: x:1:0: Function Name: _ZN4nann17k_attn_preprojectILi1EEEvNS_10AttnParamsEPKvxPf\n"
        "remark: x:1:0: Function Name: _ZN4nann11k_scan_attnILb1EEEvNS_10AttnParamsEPKfxS3_S3_iPf\n"
        "remark: x:1:0: Function Name: _ZN4nann17k_cand_score_attnILb0EEEvNS_10AttnParamsENS_17CandAttnScoreArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann16k_mlp_preprojectILi1EEEvPKvxiPKfPf\n"
        "remark: x:1:0: Function Name: _ZN4nann12k_score_mlp2ILi64ELi1EEEvNS_9MlpParamsEPKvxPKixPKfPfPNS_8OpResultE\n"
        "remark: x:1:0: Function Name: _ZN4nann9k_scan_ipILi16ELi0ELi16EEEvPKvxPKfiiPf\n")
    assert compiled_kernels(str(tmp_path), [("u.o", [])]) == {
        ("k_search", 8, 1, 2, 3, 512), ("k_search", 16, 0, 1, 4, 512), ("k_search", 16, 0, 0, 6, 512), ("k_search", 16, 0, 2, 10, 512),
        ("k_search", 16, 0, 2, 11, 512), ("k_attn_prepare",), ("k_attn_prepare_split",), ("k_score_attn", 128, 1),
        ("k_score_attn_split", 64, 0), ("k_attn_preproject", 1), ("k_scan_attn", 1), ("k_cand_score_attn", 0)}


def test_a_unit_without_a_report_is_named(tmp_path):
    from nann_amd import build
    with pytest.raises(AssertionError, match="nann_core.o"):
        compiled_kernels(str(tmp_path), build.UNITS)


def test_the_launches_enter_every_kernel_of_the_table():
    entered = [k for d, dtype in W.CASES for launch in LAUNCHES for k in claimed(d, dtype, launch)]
    assert len(LAUNCHES) == 20 and set(entered) == set(KERNELS)
    assert all(k in KERNELS for launch in RERUN_LAUNCHES for k in claimed(*W.RERUN_CASE, launch))
    # per case: the kernels of its own d and dtype once each, but the hash-set kernels on the embedding rows twice (uniform and
    # per-request level_topn), and the table's builder twice (one table per model)
    case = [k for launch in LAUNCHES for k in claimed(128, "bf16", launch)]
    per_case = {k: case.count(k) for k in set(case) if k[0] not in ("k_attn_prepare", "k_attn_prepare_split")}
    twice = {("k_search", 16, 1, 2, 3, 512), ("k_search", 16, 1, 2, 4, 512), ("k_attn_preproject", 1)}
    assert per_case == {k: 2 if k in twice else 1 for k in per_case} and twice <= set(per_case)
    assert case.count(("k_attn_prepare",)) == case.count(("k_attn_prepare_split",)) == 10


def test_constants_read_from_the_sources():
    """kCandAttnRows, the pass of the stand-alone scorer and the caps of its grid are the sources' own"""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nann_amd", "csrc")
    cand = open(os.path.join(src, "nann_cand.h")).read()
    assert int(re.search(r"constexpr int kCandAttnRows = (\d+);", cand).group(1)) == W.CAND_ROWS
    lengths = set(W.CAND_LENGTHS)
    assert {0, 1, W.CAND_ROWS - 1, W.CAND_ROWS, W.CAND_ROWS + 1} <= lengths and max(lengths) > 2 * W.CAND_ROWS and len(W.CAND_LENGTHS) == W.NQ
    attn = open(os.path.join(src, "nann_attn.h")).read()
    nt = int(re.search(r"constexpr int kAttnNT = (\d+);", attn).group(1))
    assert (nt // 64) * 32 == W.SCORE_PASS                     # CPP of k_score_attn / k_score_attn_split
    score = open(os.path.join(src, "nann_scorers.hip")).read()
    body = score[score.index("int nann_attn_score("):]
    m = re.search(r"const unsigned blocks = \(unsigned\)std::min<long long>\(\(n \+ 255\) / 256, (\d+)\);", body)
    assert int(m.group(1)) == W.SCORE_BLOCKS["exact"]
    m = re.search(r"launch_score_attn_split\(s->emb_dtype, std::min\(blocks, (\d+)u\)", body)
    assert int(m.group(1)) == W.SCORE_BLOCKS["split"]
    for p in ("exact", "split"):
        counts = W.score_counts(p)
        assert counts[:5] == (1, W.SCORE_PASS - 1, W.SCORE_PASS, W.SCORE_PASS + 1, 2 * W.SCORE_PASS + 1) and counts[5] > W.SCORE_BLOCKS[p] * W.SCORE_PASS


@pytest.mark.parametrize("d,dtype", W.CASES)
def test_the_workload_catches_something(d, dtype):
    """the conditions the matrix asserts per case, here on the CPU: a failure of the workload, not of a device"""
    W.check_conditions(d, dtype)
    for (served, n_dec, err) in W.measure(d, dtype):
        print("attention workload d=%d %s: served %d, decisive %d, oracle against float64 %.3g" % (d, dtype, served, n_dec, err))
    # the lists' identity with the k = 1024 scan can be checked on at least half of the pairs: decided by the float64 logits
    # (a row within 1e-5 of the 1024th may fall either way; counted out)
    ref = W.scores64_all(d, dtype)
    common = possible = 0
    for b, li in enumerate(W.candidate_lists()):
        kth = np.sort(ref[b])[::-1][W.K_SCAN[1] - 1]
        top = np.sort(ref[b][li])[::-1][:W.K_SCAN[0]]
        common += int((top > kth + 2e-5 * max(1.0, abs(kth))).sum())
        possible += len(top)
    assert 2 * common >= possible, (d, dtype, common, possible)


@pytest.mark.parametrize("variant", sorted(WRONG_VARIANTS))
@pytest.mark.parametrize("d,dtype", W.CASES)
def test_the_float64_reference_tells_the_wrong_variants_apart(d, dtype, variant):
    """each wrong variant of the model moves some logit of this workload by more than the contract: a device that computed the
    variant would fail the matrix"""
    worst = 0.0
    for b in range(W.NQ):
        good = W.scores64(d, dtype, b)
        bad = W.scores64(d, dtype, b, **WRONG_VARIANTS[variant])
        worst = max(worst, float((np.abs(good - bad) / np.maximum(1.0, np.abs(good))).max()))
    print("wrong variant %s d=%d %s: moves a logit by %.3g" % (variant, d, dtype, worst))
    assert worst > W.TOL, (variant, d, dtype, worst)
