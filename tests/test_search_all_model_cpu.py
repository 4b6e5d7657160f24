"""Exhaustive search under a model (nann_search_all_model), the parts that need no GPU: the ABI, the Python spelling, the
argument checks that run in front of any device call, and the build gate on the split-form scan kernel's resource report."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nann_search_all_model_workspace_bytes", "nann_search_all_model")


def test_header_declares_and_lib_binds_both_functions():
    from nann_amd import _lib
    L = _lib.lib()  # builds for gfx950 when the sources changed
    assert L.nann_abi_version() == 6
    header = open(os.path.join(ROOT, "include", "nann_hip.h")).read()
    for name in NAMES:
        assert name in _lib.SYMBOLS and getattr(L, name) is not None
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int
    assert len(L.nann_search_all_model.argtypes) == 12 and len(L.nann_search_all_model_workspace_bytes.argtypes) == 5
    assert "#define NANN_ABI_VERSION 6" in header
    # the contract of nann_search_all, word for word
    doc = header[header.index("exhaustive search under a model"):header.index("int nann_search_all_model_workspace_bytes")]
    for clause in ("k < 0 or n_users < 0 -> NANN_ERR_BAD_ARGUMENT", "k > n_items -> NANN_ERR_TOPK_K_GT_N, nothing launched",
                   "n_users == 0 -> NANN_OK, nothing written", "k > 1024 -> NANN_ERR_UNSUPPORTED", "256-byte aligned",
                   "NANN_ERR_CAPACITY", "does not depend on the batch", "no host read-back, re-entrant on shared handles"):
        assert clause in " ".join(doc.replace("*", " ").split()), clause


def test_library_exports_both_functions():
    from nann_amd import _lib
    _lib.lib()
    fresh = C.CDLL(_lib.lib_path())  # the cross-compiled library itself, through dlsym
    for name in NAMES:
        assert C.cast(getattr(fresh, name), C.c_void_p).value, name
    blob = open(_lib.lib_path(), "rb").read()
    assert b"k_scan_attnILb0E" in blob and b"k_scan_attnILb1E" in blob  # both device kernels are linked in


def test_null_handles_are_bad_arguments_without_a_device():
    from nann_amd import _lib
    L = _lib.lib()
    nbytes = C.c_int64(-1)
    assert L.nann_search_all_model_workspace_bytes(None, None, 4, 10, C.byref(nbytes)) == 7
    assert b"null argument" in L.nann_last_error()
    assert L.nann_search_all_model_workspace_bytes(None, None, 4, 10, None) == 7
    assert L.nann_search_all_model(None, None, None, 4, 10, None, None, None, None, 0, None, None) == 7
    assert b"nann_search_all_model" in L.nann_last_error()


HEAD = "remark: x:1:0: Function Name: _ZN4nann11k_scan_attnILb0EEEvNS_10AttnParamsEPKfxS3_S3_iPf\n"
EXACT = "remark: x:1:0: Function Name: _ZN4nann11k_scan_attnILb1EEEvNS_10AttnParamsEPKfxS3_S3_iPf\n"
OTHER = "remark: x:1:0: Function Name: _ZN4nann8k_searchILi16ELi0ELi1ELi0ELi1024EEEvNS_10SearchArgsE\n"


def _report(scratch, waves):
    return ("remark: x:1:0:     VGPRs: 197\nremark: x:1:0:     ScratchSize [bytes/lane]: %d\n"
            "remark: x:1:0:     Occupancy [waves/SIMD]: %d\n" % (scratch, waves))


def test_build_gate_on_the_split_form_scan_kernel(tmp_path):
    """The split-form k_scan_attn holds 150 KB of LDS for one workgroup per CU: it must reach 2 waves per SIMD and have no
    scratch frame (build._check_scan_attn).  A clean report passes; a scratch frame or 1 wave per SIMD is refused; the f32 form
    and other kernels are not held to it; and the report of the library that was just built passes."""
    from nann_amd import _lib, build
    good, scratch, waves, others = (tmp_path / n for n in ("good.log", "scratch.log", "waves.log", "others.log"))
    good.write_text(OTHER + _report(64, 1) + HEAD + _report(0, 2) + EXACT + _report(0, 2))
    scratch.write_text(HEAD + _report(16, 2))
    waves.write_text(OTHER + _report(0, 4) + HEAD + _report(0, 1))
    others.write_text(EXACT + _report(128, 1) + OTHER + _report(64, 1))
    build._check_scan_attn(str(good))
    build._check_scan_attn(str(others))
    with pytest.raises(RuntimeError, match="scratch"):
        build._check_scan_attn(str(scratch))
    with pytest.raises(RuntimeError, match="waves/SIMD"):
        build._check_scan_attn(str(waves))
    assert any(obj == "nann_scan_attn.o" for obj, _ in build.UNITS) and "nann_scan_attn_inst.hip" in build.DEPS
    _lib.lib()
    log = os.path.join(build.OUT_DIR, "nann_scan_attn.d", "compile.log")
    if os.path.exists(log):  # (a library named by NANN_HIP_LIB or shipped prebuilt has no report beside it)
        text = open(log).read()
        assert len(re.findall(r"Function Name: \S*k_scan_attnILb[01]E", text)) == 2
        build._check_scan_attn(log)


def test_search_all_model_is_importable_and_documented():
    from nann_amd import evaluate, retrieval
    f = retrieval.search_all_model
    assert list(inspect.signature(f).parameters) == ["index", "model", "comm_seq", "k", "options"]
    doc = " ".join(f.__doc__.split())
    for word in ("nann_search_all_model", "main.py:194-237", "attention", "TypeError", "SearchAllResult", "103", "102"):
        assert word in doc, word
    assert "search_all_model" in retrieval.__doc__
    p = inspect.signature(evaluate.test_all).parameters
    assert p["model_scan"].default is False and p["batched"].default is False
    assert inspect.signature(evaluate._search_all_or_none).parameters["model_scan"].default is False
