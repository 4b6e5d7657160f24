"""The certified MLP precision (NANN_MLP_CERTIFIED) where a CPU can check it: the enum and the new entry point in the
header and the library, the Python spelling, the weights-directory spelling, and its rejection by the attention model
(checked before anything is allocated)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARGUMENT = 7  # NANN_ERR_BAD_ARGUMENT


def test_enum_and_entry_point_in_the_header_and_the_library():
    from nann_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nann_hip.h")).read()
    assert re.search(r"NANN_MLP_CERTIFIED\s*=\s*3\b", hdr)
    assert re.search(r"int nann_search_refined\(const void\* workspace, int64_t out\[NANN_NUM_ROUNDS\], nann_stream_t stream\);", hdr)
    assert _lib.MLP_CERTIFIED == 3
    assert "nann_search_refined" in _lib.SYMBOLS
    L = _lib.lib()
    assert L.nann_abi_version() == 6
    assert hasattr(L, "nann_search_refined")
    out = (C.c_int64 * _lib.NUM_ROUNDS)()
    assert L.nann_search_refined(None, out, None) == BAD_ARGUMENT


def test_python_precision_names():
    from nann_amd import _lib, ops
    assert ops._precision_code("certified") == _lib.MLP_CERTIFIED
    assert ops._precision_code("exact") == _lib.MLP_EXACT_F32 and ops._precision_code("split") == _lib.MLP_SPLIT_F16
    with pytest.raises(ValueError, match="certified"):
        ops._precision_code("certifed")


def test_weights_directory_spelling(tmp_path):
    from nann_amd import ops, synth
    ops.save_scorer_dir(str(tmp_path), "mlp", synth.make_mlp_weights(64), precision="certified")
    assert open(tmp_path / "precision.txt").read().split() == ["certified"]
    assert open(tmp_path / "scorer.txt").read().split() == ["mlp"]
    src = open(os.path.join(ROOT, "nann_amd", "csrc", "nann_scorers.hip")).read()
    # both weights-directory forms (precision.txt, <graph>.precision) read the word
    assert src.count('prec == "certified"') == 2


def _attn_desc(precision):
    from nann_amd import _lib, synth
    w = synth.make_attn_weights(64, 64)
    keep = []

    def p(a):
        a = np.ascontiguousarray(a, np.float32)
        keep.append(a)
        return a.ctypes.data

    d = _lib.AttnDesc()
    d.d, d.seq_len, d.emb_dtype, d.precision = 64, 50, _lib.F16, precision
    for name in ("wq1", "bq1", "aq", "wq2", "bq2", "wk1", "bk1", "ak", "wk2", "bk2"):
        setattr(d, name, p(w[name]))
    for i in range(4):
        d.w[i] = p(w["w"][i])
    for i in range(3):
        d.b[i] = p(w["b"][i])
        d.bn_scale[i] = p(w["bn_scale"][i])
        d.bn_shift[i] = p(w["bn_shift"][i])
        d.alpha[i] = p(w["alpha"][i])
    return d, keep


def test_the_attention_model_rejects_the_certified_precision():
    from nann_amd import _lib
    L = _lib.lib()
    d, keep = _attn_desc(_lib.MLP_CERTIFIED)
    h = C.c_void_p()
    assert L.nann_attn_scorer_create(C.byref(d), C.byref(h)) == BAD_ARGUMENT
    assert b"certified" in L.nann_last_error()
    assert not h.value
