"""CPU: what the flat scorer matrix (test_flat_matrix_gpu.py) rests on, checked without a device -- its table of kernels is the
build's own list of L2 / inner-product scoring kernels, its launches enter every entry of the table, the shapes of its workload
sit on the constants the sources hold today, its workload meets the conditions under which a pass means something
(flat_matrix.check_conditions), reference A lies within the derived bound of reference B and its L2 scores are the C oracle's
bit for bit, and reference A tells each of flat_matrix.WRONG_VARIANTS apart in every case."""
import os
import re
import time

import numpy as np
import pytest

import flat_matrix as W
from test_flat_matrix_gpu import KERNELS, LAUNCHES, SHARED, claimed

# <name>I<template arguments>E of the seven templated kernels of the flat scorers.  The name must end where the template arguments
# begin, so k_scan_mlp, k_scan_attn, k_scan_sq8, k_cand_score_mlp*, k_cand_score_attn, k_score_mlp2 and k_score_attn do not match
_NAME = re.compile(r"Function Name: \S*?\d(k_score_l2|k_score_ip|k_scan_l2|k_scan_ip|k_cand_score_l2|k_cand_score_ip|k_mmr)I((?:L[ib]\d+E)+)E")
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nann_amd", "csrc")


def compiled_kernels(out_dir, units):
    """(kernel, template arguments ...) of every flat scoring kernel that the units' resource reports (<obj>.d/compile.log, what
    build.check_resources walks) name.  Kernel names only: no assembly is opened."""
    found = set()
    for obj, _ in units:
        log = os.path.join(out_dir, obj[:-2] + ".d", "compile.log")
        assert os.path.exists(log), "no resource report for the unit %s (%s)" % (obj, log)
        for m in _NAME.finditer(open(log, errors="replace").read()):
            found.add((m.group(1),) + tuple(int(v) for v in re.findall(r"L[ib](\d+)E", m.group(2))))
    return found


def test_the_table_is_what_the_build_compiled():
    """a new instantiation fails here, by name, until the matrix launches it; so does an entry no dispatch can reach any more"""
    from nann_amd import build
    build.build()
    found = compiled_kernels(build.OUT_DIR, build.UNITS)
    table = set(KERNELS)
    assert not found - table, ("compiled, not in the matrix", sorted(found - table))
    assert not table - found, ("in the matrix, not compiled", sorted(table - found))
    # 4 lanes-per-row x 3 row dtypes: the stand-alone scorer, the scan and the candidate-list scorer under both metrics (6 x 12),
    # k_mmr under both similarities (24) -- what the dispatch code promises is what the build's reports name
    assert len(table) == len(KERNELS) == 96, "an entry twice, or not the 96 kernels of the flat scorers"


def test_the_name_pattern_keeps_the_flat_kernels_only(tmp_path):
    d = tmp_path / "u.d"
    d.mkdir()
    (d / "compile.log").write_text(
        "remark: x:1:0: Function Name: _Z10k_score_ipILi16ELi0EEvPKvxiPKixPKfPfPN4nann8OpResultE\n"
        "remark: x:1:0: Function Name: _Z10k_score_l2ILi64ELi2EEvPKvxiPKixPKfPfPN4nann8OpResultE\n"
        "remark: x:1:0: Function Name: _ZN4nann9k_scan_ipILi16ELi0ELi16EEEvPKvxPKfiiPf\n"
        "remark: x:1:0: Function Name: _ZN4nann9k_scan_l2ILi8ELi1ELi16EEEvPKvxPKfiiPf\n"
        "remark: x:1:0: Function Name: _ZN4nann15k_cand_score_ipILi32ELi2EEEvNS_13CandScoreArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann15k_cand_score_l2ILi8ELi0EEEvNS_13CandScoreArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann5k_mmrILi64ELi1ELi1EEEvNS_7MmrArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann10k_scan_mlpILb1EEEvNS_9MlpParamsEPKfxS3_iPf\n"
        "remark: x:1:0: Function Name: _ZN4nann11k_scan_attnILb1EEEvNS_10AttnParamsEPKfxS3_S3_iPf\n"
        "remark: x:1:0: Function Name: _ZN4nann10k_scan_sq8ILi16EEEvNS_11Sq8ScanArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann16k_cand_score_mlpILb0EEEvNS_9MlpParamsENS_13CandScoreArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann17k_cand_score_attnILb0EEEvNS_10AttnParamsENS_17CandAttnScoreArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann12k_score_mlp2ILi64ELi1EEEvNS_9MlpParamsEPKvxPKixPKfPfPNS_8OpResultE\n"
        "remark: x:1:0: Function Name: _ZN4nann12k_score_attnILi128ELi1EEEvNS_10AttnParamsEPKfS3_PKvxPKixPfPx\n"
        "remark: x:1:0: Function Name: _ZN4nann18k_scan_transpose_qEPKfiiiPf\n"
        "remark: x:1:0: Function Name: _ZN4nann11k_cand_topkEPKNS_9CandQueryEPKiPKfiPKxPxPfPiS9_S9_S9_\n")
    assert compiled_kernels(str(tmp_path), [("u.o", [])]) == {
        ("k_score_ip", 16, 0), ("k_score_l2", 64, 2), ("k_scan_ip", 16, 0, 16), ("k_scan_l2", 8, 1, 16), ("k_cand_score_ip", 32, 2),
        ("k_cand_score_l2", 8, 0), ("k_mmr", 64, 1, 1)}


def test_a_unit_without_a_report_is_named(tmp_path):
    from nann_amd import build
    with pytest.raises(AssertionError, match="nann_core.o"):
        compiled_kernels(str(tmp_path), build.UNITS)


def test_the_launches_enter_every_kernel_of_the_table():
    entered = [k for d, dtype in W.CASES for metric in W.METRICS for launch in LAUNCHES for k in claimed(d, dtype, metric, launch)]
    assert LAUNCHES == ("score", "scan", "lists", "mmr") and set(SHARED) == set(LAUNCHES)
    assert sorted(entered) == sorted(KERNELS), "every entry exactly once"
    shared = sorted(k for launch in LAUNCHES for k in SHARED[launch])
    assert shared == ["k_cand_plan", "k_cand_topk", "k_scan_merge", "k_scan_slab_topk", "k_scan_transpose_q"]
    assert len(W.CASES) == 12 and W.METRICS == ("l2", "ip")


def _const(text, name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def test_constants_read_from_the_sources():
    """the tile, slab and block sizes the workload's shapes sit on are the sources' own: a changed constant fails here"""
    scan = open(os.path.join(SRC, "nann_scan.h")).read()
    assert (_const(scan, "kScanSlabRows"), _const(scan, "kScanRows"), _const(scan, "kScanTileQueries")) == (W.SCAN_SLAB_ROWS, W.SCAN_ROWS, W.SCAN_TILE)
    assert W.N_BIG == W.SCAN_SLAB_ROWS + W.SCAN_ROWS + 3 and W.N_SMALL == W.SCAN_ROWS + 1 and W.NQ == W.SCAN_TILE + 1
    dev = open(os.path.join(SRC, "nann_device.h")).read()
    assert _const(dev, "kMaxK") == W.K_BIG[-1] == W.MMR_MAX and W.K_BIG == (1, 200, 1024) and W.K_SMALL == (1, W.N_SMALL)
    cand = open(os.path.join(SRC, "nann_cand.h")).read()
    c = _const(cand, "kCandRows")
    assert c == W.CAND_ROWS and W.CAND_LENGTHS == (0, 1, c - 1, c, c + 1, 2 * c + 37)
    assert len(W.CAND_SHORT) == 12 and all(3 <= n <= 9 for n in W.CAND_SHORT) and sum(W.CAND_SHORT) < c and W.CAND_K == 64
    mmr = open(os.path.join(SRC, "nann_mmr.h")).read()
    assert (_const(mmr, "kMmrLdsBytes"), _const(mmr, "kMmrStateBytes"), _const(mmr, "kMmrRowPad")) == (W.MMR_LDS_BYTES, W.MMR_STATE_BYTES, W.MMR_ROW_PAD)
    assert re.search(r"return \(long long\)k_in \* \(row_bytes \+ kMmrRowPad\) <= \(long long\)\(kMmrLdsBytes - kMmrStateBytes\);", mmr)
    score = open(os.path.join(SRC, "nann_scorers.hip")).read()
    body = score[score.index("int nann_score("):]
    assert int(re.search(r"const long long rows_per_block = (\d+) \* \(64 / lpr\);", body).group(1)) == W.SCORE_WAVES
    m = re.search(r"const unsigned blocks = \(unsigned\)std::min<long long>\(\(n \+ rows_per_block - 1\) / rows_per_block, (\d+)\);", body)
    assert int(m.group(1)) == W.SCORE_GRID
    for d in W.DIMS:
        r = W.rows_per_block(d)
        assert r == 4 * 64 // (d // 8) and W.score_counts(d) == (1, r - 1, r, r + 1, 2 * r + 1, 8192 * r + 5)
        assert W.score_counts(d)[-1] > W.SCORE_GRID * r                   # past the grid's cap: the stride loop iterates
        for dtype in W.DTYPES:
            edge = W.mmr_edge(d, dtype)
            per_row = W.row_bytes(d, dtype) + W.MMR_ROW_PAD
            assert edge * per_row <= W.MMR_LDS_BYTES - W.MMR_STATE_BYTES < (edge + 1) * per_row and W.MMR_SHORT < edge < W.MMR_MAX
            assert [c[0] for c in W.mmr_calls(d, dtype)] == [edge, edge + 1, 65, 65] and [c[3] for c in W.mmr_calls(d, dtype)] == [12, 12, 65, 65]
            assert [c[4] for c in W.mmr_calls(d, dtype)] == [0.5, 0.5, 0.5, 0.0]


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("d,dtype", W.CASES)
def test_the_edge_block_holds_what_it_says(d, dtype):
    e = W.edge_rows(d, dtype)
    q = W.queries(d, dtype)
    tiny = {"f16": 2.0 ** -14, "bf16": 2.0 ** -126, "f32": 2.0 ** -126}[dtype]
    assert (_bits(e["+0"]) == 0).all() and (_bits(e["-0"]) == 0x80000000).all()
    top_a = 2.0 ** -126 if dtype == "bf16" else 2.0 ** -14               # (an f32 table: row a holds f16-subnormal values, row b f32 subnormals)
    assert ((e["subnormal a"] != 0) & (np.abs(e["subnormal a"]) < top_a)).all()
    assert ((e["subnormal b"] != 0) & (np.abs(e["subnormal b"]) < tiny)).all()
    assert np.abs(e["big"]).max() == W.big_value(dtype) and (np.abs(e["big"]) == W.big_value(dtype)).sum() == 1
    assert np.isfinite(np.float32(W.big_value(dtype)) ** 2 * np.float32(512))
    assert (_bits(e["query 0"]) == _bits(q[0])).all()
    for name, factor in (("pair l2", 1.0), ("pair ip", 2.0)):
        assert (_bits(e[name][0]) == _bits(e[name][1])).all() and np.allclose(e[name][0], factor * q[1], rtol=2.0 ** -7)
    z = _bits(e["alternating zeros"])
    assert (z[1::2] == 0x80000000).all() and (z[2::16] == 0).all() and (e["alternating zeros"][::16] == 0.5).all()
    assert (np.abs(e["smallest normal"]) == tiny).all()
    assert (np.abs(e["mixed"][::3]) < tiny).all() and (e["mixed"][::3] != 0).all() and (np.abs(e["mixed"][1::3]) >= tiny).all()
    assert np.isfinite(W.table(d, dtype)[1]).all()
    # the row equal to its query: +0 exactly under L2, and -0 from a kernel that negated the sum
    assert _bits(W.ref_a_small(d, dtype, "l2")[0, W.ROW_Q0]) == 0
    assert _bits(W.variant_scores("l2_negated_sum", d, dtype, "l2", 0)[W.ROW_Q0]) == 0x80000000


@pytest.mark.parametrize("d,dtype", W.CASES)
def test_the_workload_catches_something(d, dtype):
    """the conditions the matrix asserts per case, here on the CPU: a failure of the workload, not of a device; reference A
    within the derived bound of float64; reference A's L2 scores the oracle's, bit for bit"""
    from oracle import oracle as O
    t0 = time.perf_counter()
    n_dec = W.references(d, dtype)
    t1 = time.perf_counter()
    worst = {}
    for metric in W.METRICS:
        ref, bound = W.ref_b(d, dtype, metric)
        worst[metric] = max([W.ratio_to_bound(W.ref_a_small(d, dtype, metric), ref[:, :W.N_SMALL], bound[:, :W.N_SMALL])] +
                            [W.ratio_to_bound(s, ref[b], bound[b]) for b, s in W.ref_a_big(d, dtype, metric).items()])
        assert worst[metric] <= 1.0, (d, dtype, metric, "reference A outside the bound of reference B", worst[metric])
        # canonical() with nothing replaced is reference A
        assert (_bits(W.canonical(metric, W.queries(d, dtype)[2], W.table(d, dtype)[1][:W.N_SMALL])) == _bits(W.ref_a_small(d, dtype, metric)[2])).all()
    stored = W.table(d, dtype)[0]
    osc = O.Scorer("l2", d, {"f16": O.EMB_F16, "bf16": O.EMB_BF16, "f32": O.EMB_F32}[dtype])
    for b in range(W.NQ):
        rc, s = O.score_rows(osc, W.queries(d, dtype)[b], stored[:W.N_SMALL])
        assert rc == 0 and (_bits(s) == _bits(W.ref_a_small(d, dtype, "l2")[b])).all(), (d, dtype, b, "l2_scores is not the oracle's L2 score")
    for b, a in W.ref_a_big(d, dtype, "l2").items():
        rc, s = O.score_rows(osc, W.queries(d, dtype)[b], stored)
        assert rc == 0 and (_bits(s) == _bits(a)).all(), (d, dtype, b, "l2_scores is not the oracle's L2 score on the large table")
    print("flat workload d=%d %s: %d of %d cuts decided; reference A against float64, ratio to the bound: l2 %.3g, ip %.3g; references %.2f s"
          % (d, dtype, n_dec, W.NQ * len(W.decided(d, dtype)), worst["l2"], worst["ip"], t1 - t0))


@pytest.mark.parametrize("variant", sorted(W.WRONG_VARIANTS))
@pytest.mark.parametrize("d,dtype", W.CASES)
def test_reference_a_tells_the_wrong_variants_apart(d, dtype, variant):
    """each wrong variant moves the bits of some score of the case: a device that computed it would fail the matrix"""
    applies = W.WRONG_VARIANTS[variant][3]
    if dtype not in applies:
        assert variant == "bf16_widened_as_f16" and dtype == "f32"       # an f32 table has no 16-bit widening to mistake
        return
    moved = 0
    for metric in W.METRICS:
        good = W.ref_a_small(d, dtype, metric)
        bad = np.stack([W.variant_scores(variant, d, dtype, metric, b) for b in (0, 1, 16)])
        n = int((_bits(bad) != _bits(good[[0, 1, 16]])).sum())
        assert n > 0 or (variant == "l2_negated_sum" and metric == "ip"), (variant, d, dtype, metric)
        moved += n
    print("wrong variant %s d=%d %s: moves the bits of %d scores" % (variant, d, dtype, moved))
    assert moved > 0
