"""Builds libnann_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC_DIR = os.path.join(HERE, "csrc")
OUT_DIR = os.path.join(HERE, "_build")
LIB = os.path.join(OUT_DIR, "libnann_hip.so")
# translation units: (object name, [(source, {macro: value} defined around its #include), ...]) -- compiled in parallel, then
# linked.  A unit of several sources is compiled through a generated wrapper (_build/<obj>.d/unit.hip) that includes them
# one after the other.  Seventeen objects:
#   nann_core.o        the host side, one unit: the core of the C ABI (nann_hip.hip), the drop-in ops (nann_ops.hip), the scorers and
#                      the model loader (nann_scorers.hip), the flat retrieval calls (nann_flat.hip), the traversal family
#                      (nann_traverse.hip), the RCCL exchange (nann_comm.hip), the HNSW builder (nann_hnsw_build.hip).  Each
#                      compiles on its own -- what they share is declared in nann_host.h --; their order here is the order
#                      of the kernels in the object's metadata and nothing else
#   nann_l2_*.o        the fused traversal under the L2 scorer, one object per row dtype (one object for all three was the
#                      longest to build)
#   nann_eval*.o       the evaluation traversal: slot form and attention model; LDS form; LDS form in windows.  These three
#                      bound a build from scratch
#   nann_mlp_d*.o      the MLP traversal per embedding dim; the resident-layer-2 kernels ride with d = 64
#   nann_attn.o, nann_attn_split.o   the attention model, f32 and split-f16 form
#   nann_scan.o        the exhaustive search, with the range and wide selections (nann_range.h, nann_wide.h) and the int8 code table, scan and
#                      certified survivor pass (nann_sq8.h, nann_sq8_inst.hip); nann_scan_attn.o its scan under the attention model
#   nann_filter.o      filtered retrieval, with the group cap (nann_groupcap.h) and the attribute predicates (nann_predicate.h)
#   nann_cand.o        the candidate-list search, with the union and the fused top-k (nann_union.h, nann_fuse.h), the MMR
#                      re-ranking (nann_mmr.h) and the user interests (nann_interests.h); nann_cand_attn.o its scorer under the
#                      attention model
# The inner-product traversal (nann_ip_inst.hip, as heavy as an L2 object per row dtype) rides in the three LIGHTEST objects,
# one dtype each -- f16 in nann_filter.o, bf16 in nann_cand_attn.o, f32 in nann_scan_attn.o -- and the lean instantiations of
# the L2 and inner-product hash-set kernels (nann_lean_inst.hip, half an L2 object each) in the six that were quickest to
# build, so that no object outlasts the evaluation objects.
def _lean(scorer, dt, name):
    return ("nann_lean_inst.hip", {"NANN_LEAN_SC": scorer, "NANN_LEAN_DT": dt, "NANN_LEAN_NAME": name})


UNITS = [("nann_core.o", [("nann_ops.hip", {}), ("nann_hip.hip", {}), ("nann_scorers.hip", {}), ("nann_flat.hip", {}), ("nann_traverse.hip", {}),
                          ("nann_comm.hip", {}), ("nann_hnsw_build.hip", {}), _lean("kScorerIp", "1", "ip_bf16")]),
         ("nann_l2_f16.o", [("nann_l2_inst.hip", {"NANN_L2_DT": "0", "NANN_L2_NAME": "f16"})]),
         ("nann_l2_bf16.o", [("nann_l2_inst.hip", {"NANN_L2_DT": "1", "NANN_L2_NAME": "bf16"})]),
         ("nann_l2_f32.o", [("nann_l2_inst.hip", {"NANN_L2_DT": "2", "NANN_L2_NAME": "f32"})]),
         ("nann_mlp_d64_res.o", [("nann_mlp_inst.hip", {"NANN_MLP_D": "64"}), ("nann_mlp_res_inst.hip", {})]),
         ("nann_mlp_d128.o", [("nann_mlp_inst.hip", {"NANN_MLP_D": "128"}), _lean("NANN_SCORER_L2", "2", "l2_f32")]),
         ("nann_mlp_d256.o", [("nann_mlp_inst.hip", {"NANN_MLP_D": "256"})]),
         ("nann_attn.o", [("nann_attn_inst.hip", {})]),
         ("nann_attn_split.o", [("nann_attn_split_inst.hip", {}), _lean("kScorerIp", "2", "ip_f32")]),
         ("nann_eval.o", [("nann_eval_inst.hip", {})]),
         ("nann_eval_lds.o", [("nann_eval_lds_inst.hip", {})]),
         ("nann_eval_win.o", [("nann_eval_win_inst.hip", {})]),
         ("nann_scan.o", [("nann_scan_inst.hip", {}), ("nann_sq8_inst.hip", {}), _lean("NANN_SCORER_L2", "1", "l2_bf16")]),
         ("nann_scan_attn.o", [("nann_scan_attn_inst.hip", {}), ("nann_ip_inst.hip", {"NANN_IP_DT": "2", "NANN_IP_NAME": "f32"})]),
         ("nann_filter.o", [("nann_filter_inst.hip", {}), ("nann_ip_inst.hip", {"NANN_IP_DT": "0", "NANN_IP_NAME": "f16"})]),
         ("nann_cand.o", [("nann_cand_inst.hip", {}), _lean("NANN_SCORER_L2", "0", "l2_f16"), _lean("kScorerIp", "0", "ip_f16")]),
         ("nann_cand_attn.o", [("nann_cand_attn_inst.hip", {}), ("nann_ip_inst.hip", {"NANN_IP_DT": "1", "NANN_IP_NAME": "bf16"})])]


def _deps():
    """Every file the library is built from: the .h and .hip of csrc/, the .h of csrc/host/, the public header."""
    here = [f for f in os.listdir(SRC_DIR) if f.endswith((".h", ".hip"))]
    host = [os.path.join("host", f) for f in os.listdir(os.path.join(SRC_DIR, "host")) if f.endswith(".h")]
    return sorted(here + host) + [os.path.join("..", "..", "include", "nann_hip.h")]


DEPS = _deps()
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-fno-fast-math", "-ffp-contract=off"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def source_hash():
    """Content hash of every source the library is built from (mtimes do not survive the copy to
    the GPU box; contents do)."""
    import hashlib
    h = hashlib.sha256()
    for d in sorted(DEPS):
        with open(os.path.join(SRC_DIR, d), "rb") as f:
            h.update(d.encode() + b"\0" + f.read())
    h.update(" ".join(FLAGS).encode())
    return h.hexdigest()


def is_stale():
    """True when there is no library or it was built from other sources (hash recorded next to it)."""
    if not os.path.exists(LIB):
        return True
    try:
        with open(LIB + ".srchash") as f:
            return f.read().strip() != source_hash()
    except OSError:
        return True


def build(force=False, verbose=False, variant=None, extra_flags=()):
    """Compile every HIP source for gfx950 into nann_amd/_build/libnann_hip.so (objects in
    parallel, then one link).  Returns the library path.  `variant`: build into
    nann_amd/_build/var_<variant>/ with `extra_flags` instead (kernel experiments; load it
    with NANN_HIP_LIB)."""
    if variant is None:
        if not force and not is_stale():
            return LIB
        # one builder at a time: the ranks of a multi-process launch that all find the library stale (a snapshot whose
        # sources are newer than its .so) must not compile into the same directory together -- the first one builds, the
        # others wait on the lock and find a fresh library
        import fcntl
        os.makedirs(OUT_DIR, exist_ok=True)
        with open(os.path.join(OUT_DIR, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            try:
                if not force and not is_stale():
                    return LIB
                return _build_into(OUT_DIR, LIB, (), verbose)
            finally:
                fcntl.flock(lock, fcntl.LOCK_UN)
    out = os.path.join(OUT_DIR, "var_" + variant)
    return _build_into(out, os.path.join(out, "libnann_hip.so"), tuple(extra_flags), verbose)


# What the compiler's resource report (-Rpass-analysis=kernel-resource-usage, a unit's compile.log) must show before an object is
# linked: (name, pattern of the mangled kernel name, most scratch bytes per lane or None, fewest waves per SIMD or None, the kernel
# in the message's words).  None of these faults changes a bit of an answer; each only costs time, without any other symptom.
RULES = [
    # The 16K-slot hash-set traversal with the L2 scorer (k_search<.., VIS=2, SC=0, 512>) only pays off with TWO workgroups per
    # CU = 4 waves per SIMD; one VGPR over 128 halves its occupancy (seen: 130 VGPRs -> 2.82 ms instead of 1.99 ms).
    ("occupancy", r"k_searchILi\d+ELi\d+ELi2ELi0ELi512E", None, 4, "the hash-set kernel"),
    # The L2 scan of the exhaustive search (k_scan_l2, nann_scan.h) stages every byte of the table it reads through registers into
    # LDS.  When hipcc leaves that staging buffer in private memory the kernel still computes the same bits, with three times the
    # memory traffic (seen: ScratchSize 144 from an indexed uint4 array held across a barrier).
    ("scan_scratch", r"k_scan_l2", 0, None, "the scan kernel"),
    # The split-f16 scan under the attention model (k_scan_attn<false>, nann_scan_attn_inst.hip) keeps 150 KB of a CU's LDS for one
    # 512-thread workgroup: two wavefronts per SIMD, which the kernel reaches only within 256 VGPRs, and it has no slack for spills
    # -- a scratch frame there goes to memory once per 32-row block, between the MFMAs.  (The f32 form, k_scan_attn<true>, is the
    # parity form and is not held to this.)
    ("scan_attn", r"k_scan_attnILb0E", 0, 2, "the split-form attention scan"),
    # The split-form scorer of the candidate-list search under the attention model (k_cand_score_attn<false>,
    # nann_cand_attn_inst.hip) has the body and the 150 KB of LDS of k_scan_attn<false> and is held to the same.
    ("cand_attn", r"k_cand_score_attnILb0E", 0, 2, "the split-form attention scorer"),
    # The inner-product twin of the hash-set kernel (k_search<.., VIS=2, SC=12 (kScorerIp), 512>, nann_ip_inst.hip): the same two
    # workgroups per CU, lost the same way.
    ("ip_occupancy", r"k_searchILi\d+ELi\d+ELi2ELi12ELi512E", None, 4, "the inner-product hash-set kernel"),
    # The lean instantiations of both (k_search_lean<.., VIS=2, SC, 512>, nann_lean_inst.hip): what a plain call launches.
    ("lean_occupancy", r"k_search_leanILi\d+ELi\d+ELi2ELi(0|12)ELi512E", None, 4, "the lean hash-set kernel"),
    # The inner-product scan (k_scan_ip, nann_scan.h) stages the table as k_scan_l2 does and is held to the same.
    ("scan_ip_scratch", r"k_scan_ip", 0, None, "the inner-product scan kernel"),
    # The int8 scan (k_scan_sq8, nann_sq8.h) keeps the B fragments of a wavefront's 32 rows, d / 8 registers, across its sweep over
    # the query tiles; spilled, every MFMA of the sweep would wait for a reload from private memory.
    ("scan_sq8_scratch", r"k_scan_sq8", 0, None, "the int8 scan kernel"),
    # The survivor pass of the certified int8 search (k_sq8_surv_count / k_sq8_surv_fill, nann_sq8.h) streams the chunk's score buffer
    # twice and holds a block's eight positions per thread in registers; a frame in private memory would add its traffic to a pass that
    # is nothing but memory traffic.
    ("sq8_surv_scratch", r"k_sq8_surv_(count|fill)", 0, None, "the survivor pass"),
    # The range form of the certified int8 search (k_sq8_range_lists / k_sq8_range_count / k_sq8_range_fill, nann_sq8.h): the
    # selection holds a block's eight scores per thread in registers, as the survivor pass does, and is held to the same.
    ("sq8_range_scratch", r"k_sq8_range_(lists|count|fill)", 0, None, "the certified range selection"),
    # The streaming kernels of the wide selection (k_wide_hist / k_wide_count / k_wide_fill, nann_wide.h) read the chunk's score buffer
    # five times between them and hold a block's eight scores per thread in registers; a frame in private memory would add its traffic
    # to passes that are nothing but memory traffic.
    ("wide_scratch", r"k_wide_(hist|count|fill)", 0, None, "the wide selection"),
]


def check_resources(log_path, rules=RULES):
    """One walk over a resource report: refuse (RuntimeError) to link a kernel that breaks one of `rules`."""
    import re
    name = None
    for line in open(log_path, errors="replace"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        scratch = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        waves = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", line)
        if not name or not (scratch or waves):
            continue
        for _, pattern, most_scratch, fewest_waves, what in rules:
            if not re.search(pattern, name):
                continue
            if scratch and most_scratch is not None and int(scratch.group(1)) > most_scratch:
                raise RuntimeError(f"{name}: {scratch.group(1)} bytes of scratch per lane, {what} must have "
                                   f"{'none' if most_scratch == 0 else 'at most %d' % most_scratch}")
            if waves and fewest_waves is not None and int(waves.group(1)) < fewest_waves:
                raise RuntimeError(f"{name}: occupancy {waves.group(1)} waves/SIMD, {what} needs {fewest_waves}")


def _rule(name):
    return [r for r in RULES if r[0] == name]


def _check_occupancy(log_path):
    check_resources(log_path, _rule("occupancy"))


def _check_scan_scratch(log_path):
    check_resources(log_path, _rule("scan_scratch"))


def _check_scan_attn(log_path):
    check_resources(log_path, _rule("scan_attn"))


def _check_cand_attn(log_path):
    check_resources(log_path, _rule("cand_attn"))


def _check_ip_occupancy(log_path):
    check_resources(log_path, _rule("ip_occupancy"))


def _check_scan_ip_scratch(log_path):
    check_resources(log_path, _rule("scan_ip_scratch"))


def _check_scan_sq8_scratch(log_path):
    check_resources(log_path, _rule("scan_sq8_scratch"))


def _check_wide_scratch(log_path):
    check_resources(log_path, _rule("wide_scratch"))


def unit_command(obj, parts, odir, extra_flags=(), save_temps=True):
    """Write the wrapper of a translation unit into `odir` and return the hipcc command that compiles it to odir/obj."""
    unit = os.path.join(odir, "unit.hip")
    with open(unit, "w") as f:
        for src, macros in parts:
            for k, v in macros.items():
                f.write("#define %s %s\n" % (k, v))
            f.write('#include "%s"\n' % os.path.join(SRC_DIR, src))
            for k in macros:
                f.write("#undef %s\n" % k)
    return [_hipcc()] + FLAGS + list(extra_flags) + ["-I", SRC_DIR] + (["--save-temps=obj"] if save_temps else []) + \
           ["-Rpass-analysis=kernel-resource-usage", "-c", unit, "-o", os.path.join(odir, obj)]


def _build_into(OUT_DIR, LIB, extra_flags, verbose, only=None):
    """only: names of the objects to recompile (kernel iteration: `python -m nann_amd.build --only nann_eval.o`); the others are
    linked as they lie -- the caller vouches that their sources did not change."""
    os.makedirs(OUT_DIR, exist_ok=True)
    procs = []
    for obj, parts in UNITS:
        if only is not None and obj not in only:
            continue
        # one directory per object: --save-temps keeps the device assembly for the audit below
        odir = os.path.join(OUT_DIR, obj[:-2] + ".d")
        os.makedirs(odir, exist_ok=True)
        cmd = unit_command(obj, parts, odir, extra_flags)
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        log = open(os.path.join(odir, "compile.log"), "w")
        procs.append((cmd, odir, subprocess.Popen(cmd, stderr=log, stdout=log)))
    for cmd, odir, p in procs:
        if p.wait() != 0:
            sys.stderr.write(open(os.path.join(odir, "compile.log")).read()[-6000:])
            raise subprocess.CalledProcessError(p.returncode, cmd)
        check_resources(os.path.join(odir, "compile.log"))
    # hipcc (ROCm 7.2) can place VGPR spill code ahead of the exec restore of a join block; the
    # lanes that were masked off then reload garbage (seen: top-k positions all -1).  Refuse
    # to ship an object with that pattern.
    from . import isa_audit
    for cmd, odir, _ in procs:
        for f in os.listdir(odir):
            if f.endswith(".s") and "amdgcn" in f:
                hits = isa_audit.flow_hits(os.path.join(odir, f))
                if hits:
                    raise RuntimeError("miscompiled spill placement in %s: %s" % (f, hits[:3]))
            if not f.endswith(".o") and f != "compile.log" and not os.environ.get("NANN_KEEP_TEMPS"):
                os.remove(os.path.join(odir, f))  # preprocessed sources, bitcode, assembly: ~15 MB per object
    link = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + \
           [os.path.join(OUT_DIR, obj[:-2] + ".d", obj) for obj, _ in UNITS] + ["-ldl"]
    if verbose:
        print(" ".join(link), file=sys.stderr)
    subprocess.check_call(link)
    with open(LIB + ".srchash", "w") as f:
        f.write(source_hash())
    return LIB


if __name__ == "__main__":
    if "--only" in sys.argv:
        names = sys.argv[sys.argv.index("--only") + 1].split(",")
        assert all(any(n == o for o, _ in UNITS) for n in names), names
        print(_build_into(OUT_DIR, LIB, (), True, only=names))
    else:
        print(build(force="--force" in sys.argv, verbose=True))
