"""CPU: what the traversal matrix (test_traverse_matrix_gpu.py) rests on, checked without a device -- its table of kernels is
the build's own list of flat-scorer traversal kernels, its launches enter every entry of the table, and its workload meets the
conditions under which a pass means something (enough requests succeed; the inner product and L2 rank differently)."""
import os
import re

import pytest

import traverse_matrix as W
from test_traverse_matrix_gpu import KERNELS, LAUNCHES, claimed

_NAME = re.compile(r"Function Name: \S*?(k_search(?:_lean)?)ILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E")
_FLAT = (0, 12)  # SC: NANN_SCORER_L2, kScorerIp


def compiled_kernels(out_dir, units):
    """the (kernel, LPR, DT, VIS, SC, NT) of every k_search / k_search_lean with a flat scorer that the units' resource reports
    (<obj>.d/compile.log, what build.check_resources walks) name.  Kernel names only: no assembly is opened."""
    found = set()
    for obj, _ in units:
        log = os.path.join(out_dir, obj[:-2] + ".d", "compile.log")
        assert os.path.exists(log), "no resource report for the unit %s (%s)" % (obj, log)
        for m in _NAME.finditer(open(log, errors="replace").read()):
            t = (m.group(1),) + tuple(int(v) for v in m.groups()[1:])
            if t[4] in _FLAT:
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
    assert len(table) == len(KERNELS) == 144, "an entry twice, or not the 96 general + 48 lean instantiations"


def test_a_unit_without_a_report_is_named(tmp_path):
    from nann_amd import build
    with pytest.raises(AssertionError, match="nann_core.o"):
        compiled_kernels(str(tmp_path), build.UNITS)


def test_the_name_pattern_keeps_the_flat_traversal_kernels_only(tmp_path):
    d = tmp_path / "u.d"
    d.mkdir()
    (d / "compile.log").write_text(
        "remark: x:1:0: Function Name: _ZN4nann8k_searchILi16ELi0ELi2ELi12ELi512EEEvNS_10SearchArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann13k_search_leanILi64ELi2ELi3ELi0ELi1024EEEvNS_10SearchArgsE\n"
        "remark: x:1:0: Function Name: _ZN4nann8k_searchILi16ELi0ELi1ELi1ELi512EEEvNS_10SearchArgsE\n"       # the MLP scorer
        "remark: x:1:0: Function Name: _ZN4nann13k_search_evalILi16ELi0ELi0ELi1024ELb1EEEvNS_8EvalArgsE\n"  # another kernel
        "remark: x:1:0: Function Name: _ZN4nann9k_scan_ipILi16ELi0ELi16EEEvPKvxPKfiiPf\n")
    assert compiled_kernels(str(tmp_path), [("u.o", [])]) == {("k_search", 16, 0, 2, 12, 512), ("k_search_lean", 64, 2, 3, 0, 1024)}


def test_the_launches_enter_every_kernel_of_the_table():
    entered = [claimed(d, dtype, scorer, mode, lean) for d in W.DIMS for dtype in W.DTYPES for scorer in W.SCORERS
               for _, mode, lean in LAUNCHES]
    assert len(LAUNCHES) == 8 and set(entered) == set(KERNELS)
    # the general hash-set kernels are entered twice (phase ticks, per-request level_topn), every other kernel once
    assert len(entered) == len(KERNELS) + 48


@pytest.mark.parametrize("d", W.DIMS)
def test_the_workload_catches_something(d):
    """the conditions the matrix asserts per case, here on the CPU: a failure of the workload, not of a device"""
    for dtype in W.DTYPES:
        for scorer in W.SCORERS:
            W.check_conditions(d, dtype, scorer)
        ip, l2 = W.expected(d, dtype, "ip"), W.expected(d, dtype, "l2")
        ok = (ip[0] == 0) & (l2[0] == 0)
        assert (ip[3][ok] != l2[3][ok]).any(axis=1).all(), ("the two scorers rank some query alike", d, dtype)
