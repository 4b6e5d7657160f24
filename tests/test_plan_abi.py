"""CPU: nann_search_plan as Python sees it (nann_amd/_lib.py SearchPlan) is the struct of include/nann_hip.h -- the same fields
in the same order and types, the same size, and the trailing `lean` field (which launch a plain L2 / inner-product call took)
at the same offset.  The C side is asked through a compiled three-line program, not re-derived from the header's text."""
import ctypes as C
import os
import re
import subprocess

from nann_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CTYPES = {"int32_t": C.c_int32, "float": C.c_float, "int64_t": C.c_int64}


def _declared_fields():
    text = open(os.path.join(ROOT, "include", "nann_hip.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} nann_search_plan;", text)
    assert m, "nann_search_plan not found in include/nann_hip.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return re.findall(r"\b(int32_t|int64_t|float)\s+([a-z_0-9]+)\s*;", body)


def test_search_plan_fields_match_the_header():
    fields = _declared_fields()
    assert [(n, _CTYPES[t]) for t, n in fields] == list(_lib.SearchPlan._fields_)
    assert fields[-1] == ("int32_t", "lean")


def test_search_plan_layout_matches_the_compiler(tmp_path):
    src = tmp_path / "plan.c"
    names = [n for _, n in _declared_fields()]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nann_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(nann_search_plan));\n' +
                   "".join('  printf(" %%zu", offsetof(nann_search_plan, %s));\n' % n for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "plan"
    subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(_lib.SearchPlan) == 36
    assert got[1:] == [getattr(_lib.SearchPlan, n).offset for n in names]
    assert _lib.SearchPlan.lean.offset == 32 and _lib.SearchPlan.lean.size == 4
