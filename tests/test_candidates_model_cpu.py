"""Candidate-list search under a model (nann_search_candidates_model), the parts that need no GPU: the ABI, the argument checks
that run in front of any device call, the block size read from one place, the chunked item ranges of the attention form as a
numpy model, and the expected-value helper of the GPU tests checked against the oracle's brute force."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from test_candidates_cpu import SPLIT_CASES, plan_model, well_formed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nann_search_candidates_model_workspace_bytes", "nann_search_candidates_model")
CHUNK = 128  # users whose keys are resident at a time (kCandAttnChunk)


def candidate_attn_topk(oracle, am, seq, embs, rows, k):
    """the expected answer of the attention form everywhere: oracle.attn_score_rows on the gathered rows, oracle.topk of
    min(k, len) -> (pos, rows, scores)"""
    rows = np.asarray(rows, np.int64)
    kk = min(k, len(rows))
    if kk == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.float32)
    rc, scores = oracle.attn_score_rows(am, np.ascontiguousarray(seq, dtype=np.float32), np.ascontiguousarray(embs[rows]))
    assert rc == 0
    rc, ov, oi = oracle.topk(scores, kk)
    assert rc == 0
    return oi, rows[oi], ov


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_library_exports_both_symbols_and_header_documents_the_model_form():
    from nann_amd import _lib
    L = _lib.lib()  # builds for gfx950 when the sources changed
    assert L.nann_abi_version() == 6
    header = open(os.path.join(ROOT, "include", "nann_hip.h")).read()
    fresh = C.CDLL(_lib.lib_path())  # the cross-compiled library itself, through dlsym
    for name in NAMES:
        assert name in _lib.SYMBOLS and getattr(L, name) is not None
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int
        assert C.cast(getattr(fresh, name), C.c_void_p).value, name
    assert len(L.nann_search_candidates_model.argtypes) == 16 and len(L.nann_search_candidates_model_workspace_bytes.argtypes) == 6
    assert "#define NANN_ABI_VERSION 6" in header
    doc = header[header.index("candidate-list search under a model"):header.index("int nann_search_candidates_model_workspace_bytes")]
    doc = " ".join(doc.replace("*", " ").split())
    for clause in ("comm_seq_f16 is f16[n_users, seq_len, E]", "word for word the contract of nann_search_candidates",
                   "bit-identical to what nann_search_all_model returns", "chunks of at most 128", "min(n_users, 128) x 80 KB",
                   "NANN_ERR_CAPACITY", "NANN_ERR_UNSUPPORTED", "256-byte grid", "does not depend on the batch",
                   "no host read-back, re-entrant on shared handles"):
        assert clause in doc, clause
    blob = open(_lib.lib_path(), "rb").read()
    assert b"k_cand_score_attnILb0E" in blob and b"k_cand_score_attnILb1E" in blob  # both device kernels are linked in


def test_null_handles_and_struct_bytes_are_bad_arguments_without_a_device():
    from nann_amd import _lib
    L = _lib.lib()
    nbytes = C.c_int64(-1)
    assert L.nann_search_candidates_model_workspace_bytes(None, None, 4, 100, 10, C.byref(nbytes)) == 7
    assert b"null argument" in L.nann_last_error() and nbytes.value == -1
    assert L.nann_search_candidates_model_workspace_bytes(None, None, 4, 100, 10, None) == 7
    cand = _lib.Candidates()
    cand.struct_bytes = C.sizeof(_lib.Candidates)
    args = (None, None, None, None, None, None, None, 0, None, None)
    assert L.nann_search_candidates_model(None, None, None, 4, 10, None, *args) == 7          # no lists
    assert b"nann_search_candidates_model" in L.nann_last_error()
    assert L.nann_search_candidates_model(None, None, None, 4, 10, C.byref(cand), *args) == 7  # no handles
    assert b"null argument" in L.nann_last_error()
    cand.struct_bytes = C.sizeof(_lib.Candidates) + 8
    assert L.nann_search_candidates_model(None, None, None, 4, 10, C.byref(cand), *args) == 7
    assert b"struct_bytes" in L.nann_last_error()


def test_block_size_is_read_from_one_place_and_the_unit_is_built():
    from nann_amd import build, retrieval
    src = open(os.path.join(ROOT, "nann_amd", "csrc", "nann_cand.h")).read()
    r = int(re.search(r"constexpr int kCandAttnRows = (\d+);", src).group(1))
    assert r == retrieval.CANDIDATE_ATTN_BLOCK_ROWS and r % 256 == 0 and r > 0
    at = src.index("constexpr int kCandAttnRows")
    assert "unmeasured" in src[at - 1000:at]  # (the comment on the constant says so)
    assert int(re.search(r"constexpr int kCandAttnChunk = (\d+);", src).group(1)) == CHUNK
    assert any(obj == "nann_cand_attn.o" for obj, _ in build.UNITS) and "nann_cand_attn_inst.hip" in build.DEPS
    # the LDS sizes are defined once, in the header both attention units include
    text = lambda rel: open(os.path.join(ROOT, "nann_amd", "csrc", rel)).read()
    for name in ("kScanAttnSplitLds", "kScanAttnExactLds"):
        assert len(re.findall(r"constexpr int %s =" % name, text("nann_scan.h"))) == 1
        assert not re.search(r"constexpr int %s =" % name, text("nann_scan_attn_inst.hip") + text("nann_cand_attn_inst.hip"))
        assert name in text("nann_scan_attn_inst.hip") and name in text("nann_cand_attn_inst.hip")


def test_build_gate_on_the_split_form_kernel(tmp_path):
    import pytest
    from nann_amd import _lib, build
    head = "remark: x:1:0: Function Name: _ZN4nann17k_cand_score_attnILb0EEEvNS_10AttnParamsENS_17CandAttnScoreArgsE\n"
    exact = "remark: x:1:0: Function Name: _ZN4nann17k_cand_score_attnILb1EEEvNS_10AttnParamsENS_17CandAttnScoreArgsE\n"
    rep = lambda scratch, waves: ("remark: x:1:0:     ScratchSize [bytes/lane]: %d\nremark: x:1:0:     Occupancy [waves/SIMD]: %d\n"
                                  % (scratch, waves))
    good, scratch, waves = (tmp_path / n for n in ("good.log", "scratch.log", "waves.log"))
    good.write_text(exact + rep(64, 1) + head + rep(0, 2))
    scratch.write_text(head + rep(16, 2))
    waves.write_text(head + rep(0, 1))
    build._check_cand_attn(str(good))
    with pytest.raises(RuntimeError, match="scratch"):
        build._check_cand_attn(str(scratch))
    with pytest.raises(RuntimeError, match="waves/SIMD"):
        build._check_cand_attn(str(waves))
    _lib.lib()
    log = os.path.join(build.OUT_DIR, "nann_cand_attn.d", "compile.log")
    if os.path.exists(log):  # (a library named by NANN_HIP_LIB or shipped prebuilt has no report beside it)
        assert len(re.findall(r"Function Name: \S*k_cand_score_attnILb[01]E", open(log).read())) == 2
        build._check_cand_attn(log)


def test_python_call_is_importable_and_documented():
    from nann_amd import retrieval
    f = retrieval.search_candidates_model
    assert list(inspect.signature(f).parameters) == ["index", "model", "comm_seq", "candidates", "candidate_item_ids", "k", "options"]
    assert inspect.signature(f).parameters["k"].default == 200
    doc = " ".join(f.__doc__.split())
    for word in ("nann_search_candidates_model", "attention", "TypeError", "CandidateResult", "103", "102", "128 users"):
        assert word in doc, word
    assert "search_candidates_model" in retrieval.__doc__ and "search_candidates_model" in retrieval.search_candidates.__doc__
    assert list(inspect.signature(retrieval.search_candidates).parameters) == ["index", "scorer", "q", "candidates", "candidate_item_ids",
                                                                                "k", "options"]


# ---- the chunked item ranges --------------------------------------------------------------------------------------------
def test_chunked_item_ranges_partition_the_items_and_stay_in_their_chunk():
    """the launches of the attention form: chunk c0 walks the items [item_off[c0], item_off[c0 + n_q)); together the ranges are
    [0, item_off[n]) without gap or overlap, every item of a chunk resolves (by the kernels' bisection over ALL users) to a user
    of that chunk -- so qi - c0 indexes the chunk's keys -- and a chunk's item count stays within the bound its grid is sized by"""
    rng = np.random.default_rng(47)
    cases = [(np.asarray(s), n) for s, n, _ in SPLIT_CASES.values()]
    for nu in (1, 2, 127, 128, 129, 130, 256, 300):
        for _ in range(3):
            n_cand = int(rng.integers(0, 50 * nu))
            s = np.sort(rng.integers(0, n_cand + 1, nu + 1))
            if rng.integers(0, 2):  # a few ill-formed users
                for at in rng.integers(0, nu + 1, 3):
                    s[at] = rng.integers(-3, n_cand + 4)
            cases.append((s, n_cand))
        cases.append((np.zeros(nu + 1, np.int64), 0))  # every list empty
    seen_cross = 0
    for r in (4, 256):
        for s, n_cand in cases:
            nu = len(s) - 1
            begin, length, status, items = plan_model(s, n_cand, r)
            nb = (length + r - 1) // r
            off = np.concatenate([[0], np.cumsum(nb)])
            assert ((status == 0) == well_formed(s, n_cand)).all()
            covered = 0
            for c0 in range(0, nu, CHUNK):
                n_q = min(CHUNK, nu - c0)
                lo, hi = int(off[c0]), int(off[c0 + n_q])
                assert lo == covered and hi >= lo
                covered = hi
                assert hi - lo <= n_cand // r + min(n_q, n_cand)
                for w in range(lo, hi):
                    qi, b, cnt = items[w]
                    assert c0 <= qi < c0 + n_q and 1 <= cnt <= r, (s, w)
                seen_cross += int(c0 > 0 and hi > lo)
            assert covered == off[nu] == len(items)
    assert seen_cross > 10  # chunks beyond the first had work


# ---- the expected-value helper of the GPU tests ---------------------------------------------------------------------------
def test_expected_value_helper_equals_brute_force_on_the_identity_list(oracle):
    """the list arange(n): positions equal rows, so attn_score_rows + topk must be oracle.brute_force exactly"""
    from nann_amd import synth
    n, d, seq_len = 500, 64, 50
    embs, assign = synth.make_corpus(n, d, n_clusters=16, noise=1.0, seed=5)
    ids = np.arange(n, dtype=np.int64) * 7 + 3
    ix = oracle.Index(embs, ids, [np.zeros(0, np.int32)] * 2, [np.zeros(n + 1, np.int64)] * 2, np.zeros(1, np.int32))
    am = oracle.AttnModel(d, 64, seq_len, oracle.EMB_F16, synth.make_attn_weights(d, 64))
    sc = oracle.Scorer("attention", d, oracle.EMB_F16, attn_model=am)
    seqs = np.ascontiguousarray(synth.make_queries(embs, assign, 3, seq_len=seq_len, seed=6)[:, :, :64])
    for u, seq in enumerate(seqs):
        for k in (1, 200, 500, 700):
            pos, rows, scores = candidate_attn_topk(oracle, am, seq, embs, np.arange(n), k)
            rc, bi, bv = oracle.brute_force(ix, sc, seq.astype(np.float32).ravel(), min(k, n))
            assert rc == 0
            assert (pos == bi).all() and (rows == bi).all(), (u, k)
            assert (scores.view(np.uint32) == bv.view(np.uint32)).all(), (u, k)
    assert len(candidate_attn_topk(oracle, am, seqs[0], embs, [], 5)[0]) == 0
