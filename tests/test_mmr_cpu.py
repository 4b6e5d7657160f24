"""CPU: the MMR re-ranking and the diversified searches as far as they can be held without a GPU -- by-hand cases of the numpy
model of the contract (mmr_model), the nine symbols, the header's words, the build lists, make_diversity, and every refusal that
stands in front of the first launch and so needs no device."""
import ctypes as C
import os
import re

import numpy as np
import torch

import mmr_model as MM
from nann_amd import _lib, build, retrieval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nann_mmr_topk", "nann_search_diverse_workspace_bytes", "nann_search_diverse",
           "nann_search_model_diverse_workspace_bytes", "nann_search_model_diverse", "nann_search_all_diverse_workspace_bytes",
           "nann_search_all_diverse", "nann_search_all_model_diverse_workspace_bytes", "nann_search_all_model_diverse")
OK, BAD_ARGUMENT, UNSUPPORTED = 0, 7, 102


def _header():
    return open(os.path.join(ROOT, "include", "nann_hip.h")).read()


# ---- the model, by hand -----------------------------------------------------------------------------------------------------
def _table():
    """rows 0 and 1 identical, row 2 far from them, row 3 in between; d = 8"""
    t = np.zeros((4, 8), np.float32)
    t[0, 0] = t[1, 0] = 1.0
    t[2, 1] = 10.0
    t[3, 0] = 2.0
    return t


def test_two_identical_rows_and_a_far_one():
    t = _table()
    rows, scores = np.array([[0, 1, 2]], np.int32), np.array([[3.0, 2.5, 1.0]], np.float32)
    got = MM.model(scores, rows, None, t, 0.5, "l2", 3)
    # step 0: r = (1.5, 1.25, 0.5) -> j 0.  sim(1, 0) = -0, sim(2, 0) = -(1 + 100) = -101: v_1 = 1.25 - 0.5 * -0 = 1.25,
    # v_2 = 0.5 + 50.5 = 51 -> the far row second, the copy last at v = 1.25 - 0.5 * max(-0, -101) = 1.25
    assert got["n_out"].tolist() == [3] and got["pos"][0].tolist() == [0, 2, 1] and got["index"][0].tolist() == [0, 2, 1]
    assert got["mmr"][0].tolist() == [1.5, 51.0, 1.25] and got["scores"][0].tolist() == [3.0, 1.0, 2.5]
    # under the inner product the copy is the MOST similar row (<x0, x1> = 1, <x0, x2> = 0): v_1 = 1.25 - 0.5, v_2 = 0.5 - 0
    got = MM.model(scores, rows, None, t, 0.5, "ip", 2)
    assert got["pos"][0].tolist() == [0, 1] and got["mmr"][0].tolist() == [1.5, 0.75]
    scores[0, 1] = 1.9                                           # ... until its score no longer carries it: 0.45 < 0.5
    assert MM.model(scores, rows, None, t, 0.5, "ip", 2)["pos"][0].tolist() == [0, 2]


def test_lambda_one_is_the_ranked_prefix():
    t = _table()
    rows, scores = np.array([[2, 0, 3, 1]], np.int32), np.array([[9.0, 7.0, 7.0, -1.0]], np.float32)
    got = MM.model(scores, rows, None, t, 1.0, "l2", 3)
    assert got["pos"][0].tolist() == [0, 1, 2] and got["index"][0].tolist() == [2, 0, 3]   # the tie at 7 goes to the lower j
    assert got["mmr"][0].tolist() == [9.0, 7.0, 7.0]                                       # b = 0: v = r - 0 * p
    # an unranked list comes out in (score descending, position ascending) order
    got = MM.model(scores[:, ::-1], rows[:, ::-1], None, t, 1.0, "l2", 4)
    assert got["pos"][0].tolist() == [3, 1, 2, 0]
    # -0 and +0 tie: the lower position wins
    z = np.array([[-0.0, 0.0, -0.0]], np.float32)
    assert MM.model(z, rows[:, :3], None, t, 1.0, "l2", 3)["pos"][0].tolist() == [0, 1, 2]


def test_lambda_zero_is_the_first_valid_entry_then_the_farthest_row():
    t = _table()
    rows, scores = np.array([[7, 0, 3, 2, 1]], np.int32), np.array([[9.0, 1.0, 5.0, 2.0, 8.0]], np.float32)
    got = MM.model(scores, rows, None, t, 0.0, "l2", 4)
    # entry 0 (row 7) is out of range.  r = 0 everywhere: step 0 takes j = 1 (row 0).  Then v = -(1 * p) = the distance^2:
    # row 3 -> 1, row 2 -> 101, row 1 -> 0 (v = -(-0) = +0): j = 3; then p = max: row 3 -> max(-1, -104) = -1, row 1 -> -0
    assert got["pos"][0].tolist() == [1, 3, 2, 4] and got["mmr"][0].tolist() == [0.0, 101.0, 1.0, 0.0]
    assert got["n_out"].tolist() == [4]


def test_invalid_entries_are_dropped_and_duplicates_kept():
    t = _table()
    rows = np.array([[0, -1, 4, 2, 0, 1, 3]], np.int32)
    scores = np.array([[5.0, 9.0, 9.0, np.nan, 4.0, np.inf, -np.inf]], np.float32)
    got = MM.model(scores, rows, None, t, 1.0, "l2", 7, item_ids=np.arange(4) * 10 + 3)
    # -1 and 4: out of range; NaN, +inf, -inf: not finite.  Row 0 stands twice and is two candidates.
    assert got["n_out"].tolist() == [2] and got["pos"][0].tolist() == [0, 4, 0, 0, 0, 0, 0]
    assert got["index"][0].tolist() == [0] * 7 and got["item_ids"][0].tolist() == [3, 3, 0, 0, 0, 0, 0]
    assert not got["scores"][0, 2:].view(np.uint32).any() and not got["mmr"][0, 2:].view(np.uint32).any()
    # a denied and an excluded row; a failed query
    deny = np.array([True, False, False, False])
    ok = np.array([[1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]], np.float32)
    assert MM.model(ok, rows, None, t, 1.0, "l2", 7, deny=deny)["pos"][0, :3].tolist() == [6, 5, 3]
    assert MM.model(ok, rows, None, t, 1.0, "l2", 7, exclude=[[3, 9, -1]])["pos"][0, :4].tolist() == [5, 4, 3, 0]
    assert MM.model(ok, rows, None, t, 1.0, "l2", 7, status=[3])["n_out"].tolist() == [0]


def test_n_valid_is_clamped():
    t = _table()
    rows, scores = np.array([[0, 1, 2, 3]] * 5, np.int32), np.array([[1.0, 2.0, 3.0, 4.0]] * 5, np.float32)
    got = MM.model(scores, rows, [-3, 0, 2, 4, 9], t, 1.0, "l2", 4)
    assert got["n_out"].tolist() == [0, 0, 2, 4, 4]
    assert got["pos"][2].tolist() == [1, 0, 0, 0] and got["pos"][4].tolist() == [3, 2, 1, 0]
    # k cuts the picks short; k = 0 is nothing
    assert MM.model(scores, rows, None, t, 1.0, "l2", 2)["n_out"].tolist() == [2] * 5
    assert MM.model(scores, rows, None, t, 1.0, "l2", 0)["index"].shape == (5, 0)


def test_per_query_lambdas_are_clamped():
    assert [float(MM.clamp_lambda(x)) for x in (-1.0, np.nan, 0.0, 0.25, 1.0, 2.0, np.inf, -np.inf)] == [0, 0, 0, 0.25, 1, 1, 1, 0]
    t = _table()
    rows, scores = np.array([[0, 1, 2]] * 3, np.int32), np.array([[3.0, 2.5, 1.0]] * 3, np.float32)
    got = MM.model(scores, rows, None, t, 0.7, "l2", 3, lams=[2.0, np.nan, 0.5])
    assert got["pos"].tolist() == [[0, 1, 2], [0, 2, 1], [0, 2, 1]]


def test_the_key_is_topkv2s():
    xs = np.array([-np.inf, -3.0, -1e-30, -0.0, 0.0, 1e-30, 2.0, np.inf], np.float32)
    ks = [MM.key(x) for x in xs]
    assert ks[3] == ks[4] and ks == sorted(ks) and len(set(ks)) == 7
    assert MM.keys_of(xs).tolist() == ks
    src = open(os.path.join(build.SRC_DIR, "nann_device.h")).read()
    assert "s = s + 0.0f;" in src and "(u & 0x80000000u) ? ~u : (u | 0x80000000u)" in src


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_the_nine_symbols_are_declared_exported_and_bound():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = C.CDLL(build.build())
    for s in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % s, code), s
        assert hasattr(lib, s), s
        assert s in _lib.SYMBOLS, s
    assert "#define NANN_ABI_VERSION 6" in _header()
    assert sorted(_lib.SYMBOLS) == sorted(set(re.findall(r"\b(nann_[a-z0-9_]+)\s*\(", code)))
    assert C.sizeof(_lib.Diversity) == 24
    assert re.search(r"int32_t struct_bytes;[^}]*float lambda;[^}]*const float\* lambdas;[^}]*int32_t sim;[^}]*\} nann_diversity;", code)
    for name in ("Diversity", "make_diversity", "DiverseResult", "mmr", "search_diverse", "search_model_diverse",
                 "search_all_diverse", "search_all_model_diverse"):
        assert hasattr(retrieval, name), name


def test_the_header_states_the_contract():
    text = _header()
    assert text.index("group caps: at most m rows per group") < text.index("diversified results: MMR re-ranking")
    section = text[text.index("diversified results: MMR re-ranking"):text.index("8(f3): the evaluation graph")]
    section = " ".join(section.replace("\n *", " ").split())
    for phrase in ("The reference has no such call",
                   "j < clamp(n_valid[i], 0, k_in)",
                   "its score is finite",
                   "malformed input never faults",
                   "A row that appears twice gives two candidates",
                   "!(x >= 0) ? 0 : (x > 1 ? 1 : x)",
                   "NANN_SCORER_MLP: NANN_ERR_UNSUPPORTED",
                   "b = 1.0f - a",
                   "bit for bit what nann_score returns for that pair",
                   "f32 and uncontracted",
                   "r_j = a * s_j, computed once",
                   "p_j = (sim(j, t) > p_j) ? sim(j, t) : p_j",
                   "v_j = r_j - (b * p_j)",
                   "x + 0.0f, then the monotone u32 map",
                   "ties go to the lower j",
                   "n_out = min(k, #valid)",
                   "(score descending, position ascending) order",
                   "does not depend on the batch",
                   "not over the whole table",
                   "NO PREFIX PROPERTY",
                   "the ORIGINAL s_j",
                   "No workspace",
                   "Where several apply",
                   "None of these checks touches the device",
                   "no host read-back",
                   "A failed query gets n_out = 0",
                   "fetch > n_items -> NANN_ERR_TOPK_K_GT_N"):
        assert phrase in section, phrase


def test_the_kernel_rides_in_the_candidate_object():
    assert "nann_mmr.h" in build.DEPS
    assert len(build.UNITS) == 17
    inst = open(os.path.join(build.SRC_DIR, "nann_cand_inst.hip")).read()
    assert '#include "nann_mmr.h"' in inst and "#define NANN_MMR_IMPL" in inst
    assert any(src == "nann_cand_inst.hip" for _, parts in build.UNITS for src, _ in parts)
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "nann_mmr.h" in text[text.index("\n## 2. Build"):text.index("\n## 3. ")]
    # the kernel's header exports what decides between its two paths
    src = open(os.path.join(build.SRC_DIR, "nann_mmr.h")).read()
    for name in ("kMmrLdsBytes", "kMmrStateBytes", "kMmrRowPad"):
        assert re.search(r"constexpr int %s = \d+;" % name, src), name


# ---- every refusal that needs no device -----------------------------------------------------------------------------------
def _div(lam=0.5, lambdas=0, sim=_lib.SCORER_L2, struct_bytes=None):
    d = _lib.Diversity()
    d.struct_bytes = C.sizeof(_lib.Diversity) if struct_bytes is None else struct_bytes
    d.lam = lam
    d.lambdas = lambdas or None
    d.sim = sim
    return d


def _mmr(L, ix=0, n_queries=2, k_in=8, k=5, scores=3, rows=1, out_index=2, div="default"):
    """nann_mmr_topk with made-up addresses (and no index): nothing is dereferenced by a refused call"""
    p = lambda v: C.c_void_p(0x10000 * v) if v else None
    d = _div() if div == "default" else div
    return L.nann_mmr_topk(p(ix), p(scores), p(rows), None, n_queries, k_in, C.byref(d) if d is not None else None, k,
                           p(out_index), None, None, None, None, None, None)


def test_mmr_refusals_need_no_device():
    L = _lib.lib()
    who = b"nann_mmr_topk"
    assert _mmr(L, n_queries=-1) == BAD_ARGUMENT and who in L.nann_last_error()
    assert _mmr(L, k_in=-1, k=0) == BAD_ARGUMENT and b"negative size" in L.nann_last_error()
    assert _mmr(L, k=-1) == BAD_ARGUMENT
    assert _mmr(L, k=9) == BAD_ARGUMENT and b"k exceeds" in L.nann_last_error() and who in L.nann_last_error()
    assert _mmr(L, k_in=1025, k=5) == UNSUPPORTED and b"k_in <= 1024" in L.nann_last_error()
    assert _mmr(L, n_queries=2 ** 31) == UNSUPPORTED
    assert _mmr(L, div=None) == BAD_ARGUMENT and b"null nann_diversity" in L.nann_last_error() and who in L.nann_last_error()
    assert _mmr(L, div=_div(struct_bytes=16)) == BAD_ARGUMENT and b"struct_bytes" in L.nann_last_error()
    assert _mmr(L, div=_div(sim=_lib.SCORER_MLP)) == UNSUPPORTED and b"nann_diversity" in L.nann_last_error()
    assert _mmr(L, div=_div(sim=3)) == BAD_ARGUMENT and b"unknown sim" in L.nann_last_error()
    assert _mmr(L, div=_div(sim=-1)) == BAD_ARGUMENT
    for lam in (-0.001, 1.001, float("nan"), float("inf"), -float("inf")):
        assert _mmr(L, div=_div(lam=lam)) == BAD_ARGUMENT and b"lambda" in L.nann_last_error(), lam
    # with every struct right, the null pointers are next; the index is the last thing looked at and is null here
    assert _mmr(L, rows=0, div=_div(struct_bytes=0)) == BAD_ARGUMENT and b"null argument" in L.nann_last_error()
    assert _mmr(L, scores=0) == BAD_ARGUMENT and b"null argument" in L.nann_last_error()
    assert _mmr(L, out_index=0) == BAD_ARGUMENT
    assert _mmr(L, div=_div(lam=0.0)) == BAD_ARGUMENT and b"null argument" in L.nann_last_error() and who in L.nann_last_error()
    assert _mmr(L, div=_div(lam=1.0, sim=_lib.SCORER_IP, lambdas=5)) == BAD_ARGUMENT and b"null argument" in L.nann_last_error()
    # nothing to do: NANN_OK whatever the pointers, a made-up index among them ...
    assert _mmr(L, ix=7, n_queries=0, rows=0, out_index=0) == OK
    assert _mmr(L, ix=7, k=0, rows=0, scores=0, out_index=0) == OK
    # ... but the sizes and the diversity are looked at in front of it
    assert _mmr(L, ix=7, n_queries=0, div=None) == BAD_ARGUMENT
    assert _mmr(L, ix=7, k=0, div=_div(lam=2.0)) == BAD_ARGUMENT
    assert _mmr(L, ix=7, k=9, rows=0, div=None) == BAD_ARGUMENT and b"k exceeds" in L.nann_last_error()
    assert _mmr(L, ix=7, k_in=2000, k=5, div=None) == UNSUPPORTED
    assert _mmr(L, ix=7, k_in=2000, k=2001, div=None) == BAD_ARGUMENT   # (BAD_ARGUMENT of the sizes before their UNSUPPORTED)


def test_null_handles_of_the_search_forms_are_bad_arguments_without_a_gpu():
    L = _lib.lib()
    nb = C.c_int64(-1)
    t = (C.c_int32 * 6)(8, 16, 32, 32, 32, 50)
    d = _div()
    assert L.nann_search_diverse_workspace_bytes(None, t, 3, C.byref(nb)) == BAD_ARGUMENT
    assert L.nann_search_model_diverse_workspace_bytes(None, None, t, 3, C.byref(nb)) == BAD_ARGUMENT
    assert L.nann_search_all_diverse_workspace_bytes(None, None, 3, 10, C.byref(nb)) == BAD_ARGUMENT
    assert L.nann_search_all_model_diverse_workspace_bytes(None, None, 3, 10, C.byref(nb)) == BAD_ARGUMENT
    assert nb.value == -1
    assert L.nann_search_diverse(None, None, None, 3, t, None, None, 0, None, None, None, None, None, None, None, None, None,
                                 C.byref(d), 10, None, None, None, None) == BAD_ARGUMENT
    assert b"nann_search_diverse" in L.nann_last_error()
    assert L.nann_search_model_diverse(None, None, None, 3, t, None, None, 0, None, None, None, None, None, None, None, None,
                                       C.byref(d), 10, None, None, None, None) == BAD_ARGUMENT
    assert b"nann_search_model_diverse" in L.nann_last_error()
    assert L.nann_search_all_diverse(None, None, None, 3, 20, 10, None, None, None, None, None, None, 0, None, None, C.byref(d),
                                     None, None) == BAD_ARGUMENT
    assert b"nann_search_all_diverse" in L.nann_last_error()
    assert L.nann_search_all_model_diverse(None, None, None, 3, 20, 10, None, None, None, None, None, None, 0, None, None,
                                           C.byref(d), None, None) == BAD_ARGUMENT
    assert b"nann_search_all_model_diverse" in L.nann_last_error()


# ---- make_diversity without a GPU -------------------------------------------------------------------------------------------
def test_make_diversity_on_the_cpu():
    dv = retrieval.make_diversity()
    assert dv.lam == 0.5 and dv.lams is None and dv.sim is None and dv.n_queries is None
    dev = torch.device("cpu")
    ref, keep = retrieval._diversity_args(dv, 4, dev)
    st = keep[0]
    assert st.struct_bytes == 24 and st.lam == 0.5 and not st.lambdas and st.sim == _lib.SCORER_L2
    class _Ip:
        kind = "ip"
    assert retrieval._diversity_args(dv, 4, dev, _Ip())[1][0].sim == _lib.SCORER_IP          # sim=None follows an IP scorer
    assert retrieval._diversity_args(retrieval.make_diversity(sim="l2"), 4, dev, _Ip())[1][0].sim == _lib.SCORER_L2
    dv = retrieval.make_diversity(lam=1.0, lams=[0.0, 2.0, float("nan")], sim="ip")
    assert dv.lams.dtype == torch.float32 and dv.n_queries == 3
    ref, (st, lams) = retrieval._diversity_args(dv, 3, dev)
    assert st.sim == _lib.SCORER_IP and st.lambdas == lams.data_ptr() and st.lam == 1.0
    for bad in (dict(lam=-0.1), dict(lam=1.5), dict(lam=float("nan")), dict(sim="mlp")):
        try:
            retrieval.make_diversity(**bad)
        except AssertionError:
            continue
        raise AssertionError(bad)
    try:
        retrieval._diversity_args(dv, 4, dev)   # three lambdas, four queries
    except AssertionError:
        pass
    else:
        raise AssertionError("lams of another batch size")
