"""Every host source of nann_core.o compiles ON ITS OWN: what one of them takes from another is declared in
csrc/nann_host.h (or a header it includes), not picked up from the source that happens to stand in front of it in the unit.
nann_lean_inst.hip is left out: it is parameterised by the macros build.UNITS defines around it."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from nann_amd import build


def _hipcc():
    cc = build._hipcc()
    return cc if os.path.isabs(cc) and os.path.exists(cc) else shutil.which(cc)


@pytest.mark.skipif(_hipcc() is None, reason="no hipcc")
def test_every_host_source_of_the_core_unit_compiles_alone():
    parts = dict(build.UNITS)["nann_core.o"]
    sources = [src for src, _ in parts if src != "nann_lean_inst.hip"]
    assert "nann_hip.hip" in sources and len(sources) >= 7

    def syntax_only(src):
        cmd = [_hipcc()] + build.FLAGS + ["-I", build.SRC_DIR, "-fsyntax-only", os.path.join(build.SRC_DIR, src)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        return src, p.returncode, p.stdout

    with ThreadPoolExecutor(min(8, len(sources))) as pool:
        results = list(pool.map(syntax_only, sources))
    for src, status, log in results:
        assert status == 0, f"{src} does not compile on its own:\n{log[-4000:]}"
