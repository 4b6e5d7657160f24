#!/usr/bin/env python3
"""sha256 of the device assembly of every object of the DEFAULT build (kernels only: comment and
directive lines that can carry paths are dropped).  Used to show that an edit guarded by a
build-time knob leaves the shipped kernels byte-for-byte unchanged:
    tools/isa_fingerprint.py > before.txt; <edit>; tools/isa_fingerprint.py | diff before.txt -
--per-kernel: one hash per symbol of each object instead, its own name and the function index of its labels
(.LBB<n>_, .Lfunc_end<n>) masked, so that kernels compare across a rename or a move within the object."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nann_amd import build  # noqa: E402


def one(unit, per_kernel=False):
    obj, parts = unit
    d = tempfile.mkdtemp(prefix="isa_")
    subprocess.check_call(build.unit_command(obj, parts, d), stderr=subprocess.DEVNULL)
    hashes, sym = {}, obj
    for f in sorted(os.listdir(d)):
        if f.endswith(".s") and "amdgcn" in f:
            for line in open(os.path.join(d, f), errors="replace"):
                s = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", line.split(";")[0].rstrip())  # per-compile id
                if not s or re.match(r"\s*\.(file|ident|section|loc|amdgpu_metadata|end_amdgpu_metadata)\b", s):
                    continue
                if per_kernel:  # a symbol's lines run from its .protected / .globl / .type / label to the next symbol's
                    m = re.match(r"\s*\.(?:protected|globl|type)\s+([^\s,]+)|([A-Za-z_$][\w.$]*):", s)
                    if m:
                        sym = m.group(1) or m.group(2)
                    s = re.sub(r"(\.L(?:BB|func_end))\d+", r"\1", s.replace(sym, "<sym>"))
                hashes.setdefault(sym, hashlib.sha256()).update(s.encode() + b"\n")
    subprocess.call(["rm", "-rf", d])
    return [(obj if sym == obj else obj + " " + sym, h.hexdigest()) for sym, h in hashes.items()]


if __name__ == "__main__":
    per_kernel = "--per-kernel" in sys.argv
    with ThreadPoolExecutor(4) as ex:
        for lines in ex.map(lambda u: one(u, per_kernel), build.UNITS):
            for name, digest in lines:
                print(name, digest)
