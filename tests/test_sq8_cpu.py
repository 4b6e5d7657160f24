"""CPU: the scalar-quantised exhaustive search as far as it can be held without a GPU -- the seven symbols, the build lists and
the scratch rule of the int8 scan, the refusals that stand in front of any device call, and the numpy model of the contract
(sq8_model) against a float64 restatement on inputs where quantisation is lossless, on zero vectors, on the largest f16, and
on a corpus with duplicated rows (the tie rule of both stages)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sq8_model as M
from nann_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nann_sq8_create", "nann_sq8_destroy", "nann_sq8_info", "nann_sq8_view", "nann_sq8_encode",
           "nann_search_all_sq8_workspace_bytes", "nann_search_all_sq8")
OK, BAD_ARGUMENT, UNSUPPORTED = 0, 7, 102
F = np.float32


def _header():
    return open(os.path.join(ROOT, "include", "nann_hip.h")).read()


# ---- the ABI and the build ------------------------------------------------------------------------------------------------
def test_the_seven_symbols_are_declared_exported_and_bound():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = C.CDLL(build.build())
    bound = _lib.lib()
    for s in SYMBOLS:
        assert re.search(r"\b(int|void) %s\s*\(" % s, code), s
        assert hasattr(lib, s), s
        assert s in _lib.SYMBOLS, s
        assert getattr(bound, s).argtypes, s
    assert re.search(r"typedef struct nann_sq8 nann_sq8;", code)
    assert bound.nann_sq8_destroy.restype is None
    assert "#define NANN_ABI_VERSION 6" in _header() and bound.nann_abi_version() == 6


def test_the_kernels_ride_in_the_scan_object():
    assert len(build.UNITS) == 17
    parts = [src for src, _ in dict(build.UNITS)["nann_scan.o"]]
    assert parts[:2] == ["nann_scan_inst.hip", "nann_sq8_inst.hip"]
    assert "nann_sq8.h" in build.DEPS and "nann_sq8_inst.hip" in build.DEPS
    src = open(os.path.join(build.SRC_DIR, "nann_sq8.h")).read()
    assert "__builtin_amdgcn_mfma_i32_32x32x32_i8" in src and "__fdiv_rn" in src
    assert "-ffp-contract=off" in build.FLAGS
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = text[text.index("\n## 2. Build"):text.index("\n## 3. ")]
    assert "nann_sq8_inst.hip" in section and "seventeen translation units" in section


REPORT = """remark: unit.hip:1:1: Function Name: _ZN4nann10k_scan_sq8ILi4ELi0EEEvPKaPKfPKixS2_S4_S6_iPf [-Rpass-analysis=kernel-resource-usage]
remark: unit.hip:1:1:     VGPRs: 60 [-Rpass-analysis=kernel-resource-usage]
remark: unit.hip:1:1:     ScratchSize [bytes/lane]: %d [-Rpass-analysis=kernel-resource-usage]
remark: unit.hip:1:1:     Occupancy [waves/SIMD]: 8 [-Rpass-analysis=kernel-resource-usage]
remark: unit.hip:1:1: Function Name: _ZN4nann15k_sq8_sort_rowsEPKiPKfiPiPxS4_Pf [-Rpass-analysis=kernel-resource-usage]
remark: unit.hip:1:1:     ScratchSize [bytes/lane]: 16 [-Rpass-analysis=kernel-resource-usage]
"""


def test_the_build_refuses_a_scan_with_a_scratch_frame(tmp_path):
    good, bad = tmp_path / "good.log", tmp_path / "bad.log"
    good.write_text(REPORT % 0)
    bad.write_text(REPORT % 64)
    build._check_scan_sq8_scratch(str(good))   # (the sort kernel's frame is no business of the rule)
    build.check_resources(str(good))
    with pytest.raises(RuntimeError, match="k_scan_sq8.*64 bytes of scratch.*int8 scan"):
        build._check_scan_sq8_scratch(str(bad))
    with pytest.raises(RuntimeError, match="k_scan_sq8"):
        build.check_resources(str(bad))        # (what the build runs over every unit's report)


# ---- the refusals in front of any device call -----------------------------------------------------------------------------
def test_refusals_without_a_device():
    L = _lib.lib()
    out = C.c_void_p(0)
    assert L.nann_sq8_create(None, None, C.byref(out)) == BAD_ARGUMENT and b"null" in L.nann_last_error()
    assert L.nann_sq8_create(None, None, None) == BAD_ARGUMENT
    L.nann_sq8_destroy(None)  # a no-op
    info = (C.c_int64 * 4)()
    assert L.nann_sq8_info(None, info) == BAD_ARGUMENT
    p = C.c_void_p(0)
    assert L.nann_sq8_view(None, C.byref(p), None, None) == BAD_ARGUMENT
    assert L.nann_sq8_encode(None, -1, 64, None, None, None, None) == BAD_ARGUMENT
    assert L.nann_sq8_encode(None, 4, 100, None, None, None, None) == UNSUPPORTED and b"64, 128, 256 or 512" in L.nann_last_error()
    assert L.nann_sq8_encode(None, 0, 64, None, None, None, None) == OK
    assert L.nann_sq8_encode(None, 4, 64, None, None, None, None) == BAD_ARGUMENT
    nb = C.c_int64(-1)
    assert L.nann_search_all_sq8_workspace_bytes(None, None, None, 4, 8, 4, C.byref(nb)) == BAD_ARGUMENT
    assert L.nann_search_all_sq8_workspace_bytes(None, None, None, 4, 8, 4, None) == BAD_ARGUMENT
    assert L.nann_search_all_sq8(None, None, None, None, 4, 8, 4, None, None, None, None, None, None, 0, None, None) == BAD_ARGUMENT
    assert nb.value == -1


# ---- the model ------------------------------------------------------------------------------------------------------------
def _lossless(rng, n, d):
    """rows with entries in {-127 .. 127} * 2^-7 and amax = 127 * 2^-7: scale = 2^-7 exactly, code = 128 x"""
    c = rng.integers(-127, 128, (n, d)).astype(np.int32)
    c[np.arange(n), rng.integers(0, d, n)] = rng.choice([-127, 127], n)
    return (c.astype(F) / F(128.0)).astype(np.float16), c


@pytest.mark.parametrize("d", [64, 128, 512])
def test_lossless_inputs_against_float64(d):
    rng = np.random.default_rng(d)
    x, cx = _lossless(rng, 300, d)
    q16, cq = _lossless(rng, 9, d)
    q = q16.astype(F)
    xe, qe = M.encode(x), M.encode(q)
    assert (xe[0] == cx).all() and (qe[0] == cq).all()
    assert (xe[1] == F(2.0 ** -7)).all() and (qe[1] == F(2.0 ** -7)).all()
    assert (xe[2] == (cx.astype(np.int64) ** 2).sum(1)).all()
    D = cq.astype(np.int64) @ cx.astype(np.int64).T
    assert (M.dots(qe[0], xe[0]) == D).all() and np.abs(D).max() < 2 ** 24
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    ip = M.approx_scores(qe, xe, "ip")
    assert (ip.astype(np.float64) == q64 @ x64.T).all()          # the approximate IP IS the exact IP: D * 2^-14
    l2 = M.approx_scores(qe, xe, "l2")
    # the approximate L2: c = 2 D 2^-14 and a + b = (nq + nx) 2^-14 are exact (nq + nx < 2^24), so s is the ONE rounding of the
    # exact -|q - x|^2 = (2 D - nq - nx) 2^-14, an integer of up to 25 bits times a power of two
    exact = -((q64[:, None, :] - x64[None, :, :]) ** 2).sum(-1)
    assert (exact == (2 * D - qe[2][:, None].astype(np.int64) - xe[2][None, :]) * 2.0 ** -14).all()
    assert (l2.view(np.uint32) == exact.astype(F).view(np.uint32)).all()
    # and the whole call returns the exact top k, in TopKV2 order, at fetch = k under the inner product
    rows, scores, f_rows, f_scores = M.search(q, x, "ip", 20, 20, M.exact_f64(q, x, "ip"))
    for b in range(len(q)):
        er, es = M.topk((q64[b] @ x64.T).astype(F), 20)
        assert (rows[b] == er).all() and (scores[b].view(np.uint32) == es.view(np.uint32)).all()
        assert (f_rows[b] == er).all() and (f_scores[b].view(np.uint32) == es.view(np.uint32)).all()


def test_zero_vectors():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((40, 64)).astype(np.float16)
    x[7] = 0
    x[8] = -0.0
    q = rng.standard_normal((3, 64)).astype(F)
    q[1] = 0
    xe, qe = M.encode(x), M.encode(q)
    for e, i in ((xe, 7), (xe, 8), (qe, 1)):
        assert (e[0][i] == 0).all() and e[1][i] == 0 and e[2][i] == 0
    assert np.isfinite(xe[1]).all() and (xe[0][[0, 1, 9]] != 0).any()
    for metric in ("ip", "l2"):
        s = M.approx_scores(qe, xe, metric)
        assert np.isfinite(s).all()
    ip, l2 = M.approx_scores(qe, xe, "ip"), M.approx_scores(qe, xe, "l2")
    assert (ip[:, 7] == 0).all() and (ip[1] == 0).all()
    a = (qe[1] * qe[1]) * qe[2].astype(F)
    b = (xe[1] * xe[1]) * xe[2].astype(F)
    assert (l2[:, 7].view(np.uint32) == (F(0) - (a + F(0))).view(np.uint32)).all()   # the zero row: -|q|^2 as quantised
    assert (l2[1].view(np.uint32) == (F(0) - (F(0) + b)).view(np.uint32)).all()        # the zero query: -|x|^2 as quantised
    assert l2[1, 7] == 0
    # the zero query ties every row under the inner product: the fetch is rows 0 .. fetch - 1
    assert M.fetch(ip, 5)[0][1].tolist() == [0, 1, 2, 3, 4]


def test_a_row_with_the_largest_f16():
    x = np.zeros((2, 64), np.float16)
    x[0, 3] = 65504.0
    x[0, 4] = -300.0
    x[0, 5] = 257.0     # 257 / (65504 / 127) = 0.498..: rounds to 0
    x[0, 6] = 258.0     # 0.5002..: rounds to 1
    x[1, :] = 1.0
    codes, scales, norms = M.encode(x)
    assert scales[0] == F(65504.0) / F(127.0) and np.isfinite(scales).all()
    assert codes[0, 3] == 127 and codes[0, 4] == -1 and codes[0, 5] == 0 and codes[0, 6] == 1
    assert norms[0] == 127 * 127 + 2 and (codes[1] == 127).all() and norms[1] == 64 * 127 * 127
    q = np.zeros((1, 64), F)
    q[0, 3] = 1.0
    qe = M.encode(q)
    s = M.approx_scores(qe, (codes, scales, norms), "ip")
    assert s[0, 0] == (qe[1][0] * scales[0]) * F(127 * 127) and abs(float(s[0, 0]) - 65504.0) < 65504.0 * 2.0 ** -20
    assert np.isfinite(M.approx_scores(qe, (codes, scales, norms), "l2")).all()


def test_the_tie_rule_of_both_stages():
    """rows duplicated three times at shuffled positions: equal approximate AND exact scores; both stages order them by row"""
    rng = np.random.default_rng(5)
    base = rng.standard_normal((50, 64)).astype(np.float16)
    x = np.tile(base, (3, 1))[rng.permutation(150)]
    q = base[[3, 11, 40]].astype(F) + F(0.01)
    for metric in ("ip", "l2"):
        xf = x.astype(F)
        exact = (lambda qi, rows: ((xf[rows] * q[qi]).sum(1) if metric == "ip" else -((xf[rows] - q[qi]) ** 2).sum(1)).astype(F))
        rows, scores, f_rows, f_scores = M.search(q, x, metric, 30, 12, exact)
        for r, s in ((f_rows, f_scores), (rows, scores)):
            for b in range(3):
                assert (np.diff(s[b]) <= 0).all()
                same = np.diff(s[b]) == 0
                assert same.sum() >= len(s[b]) // 2          # the triples are there
                assert (np.diff(r[b])[same] > 0).all()       # equal scores: ascending rows
        # the result holds rows of the fetch only, and the best of them
        for b in range(3):
            assert set(rows[b]) <= set(f_rows[b])
            er, es = M.topk(exact(b, np.sort(f_rows[b])), 12, np.sort(f_rows[b]))
            assert (rows[b] == er).all() and (scores[b].view(np.uint32) == es.view(np.uint32)).all()
    # a fetch that cuts a triple keeps its LOWER rows
    approx = M.approx_scores(M.encode(q), M.encode(x), "l2")
    top = M.fetch(approx, 2)[0]
    for b, src in enumerate((3, 11, 40)):
        twins = np.flatnonzero((x == base[src]).all(1))
        assert top[b].tolist() == twins[:2].tolist()
