"""-m gpu: the status codes of the flat retrieval calls through the C ABI, pinned.  nann_search_all, nann_search_all_filtered,
nann_search_all_model, nann_search_all_model_filtered, nann_search_candidates, nann_search_candidates_model and the
*_workspace_bytes twin of each, under every kind of scorer or model the call takes: which status a faulty argument gets, a
substring of nann_last_error(), and WHICH fault wins where two are present -- the entry points differ in that, and callers may
rely on either.  The expected values are literals, recorded from the library before the entry points were given one shared host
path (csrc/nann_flat.hip); nothing here is computed from the code under test.  300 rows of d = 64, batch 3, k = 5, lists of 7
rows: the calls reach every branch and take milliseconds."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from gpu_util import cuda, require_gpu
from test_search_all_model_gpu import L_SEQ, _corpus, _model

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu
N, N_BIG, B, K, LIST = 300, 1100, 3, 5, 7
OK, TOPK, BAD, UNSUPPORTED, CAPACITY = 0, 4, 7, 102, 103
SENTINEL = -77
K_ROOM = N + 1  # the outputs hold the widest k a case of this file gets through a call

# entry point -> the kinds of scorer (l2, mlp) or model (l2m, mlpm, attn) it is called under
ENTRIES = {"all": ("l2", "mlp"), "all_filtered": ("l2", "mlp"), "all_model": ("l2m", "mlpm", "attn"),
           "all_model_filtered": ("l2m", "mlpm", "attn"), "candidates": ("l2", "mlp"), "candidates_model": ("l2m", "mlpm", "attn")}
EXHAUSTIVE = ("all", "all_filtered", "all_model", "all_model_filtered")
CONFIGS = [(e, kind) for e, kinds in ENTRIES.items() for kind in kinds]


def _by_family(exhaustive, candidates):
    return {(e, kind): (exhaustive if e in EXHAUSTIVE else candidates) for e, kind in CONFIGS}


def _by_kind(l2, other):
    return {(e, kind): (l2 if kind in ("l2", "l2m") else other) for e, kind in CONFIGS}


def _short_and_bad_options():
    """nann_search_all* under a model look at the workspace first; every other entry point at the options first"""
    return {(e, kind): ((CAPACITY, b"workspace smaller than") if e in ("all_model", "all_model_filtered")
                        else (BAD, b"nann_search_options: struct_bytes")) for e, kind in CONFIGS}


# case -> {(entry, kind): (status, substring of nann_last_error() or None)} of the SEARCH call
SEARCH = {
    "k = -1": _by_family((BAD, b"k >= 0"), (BAD, b"k >= 0")),
    "k = n_items + 1": _by_family((TOPK, b"at least k"), (OK, None)),
    "k = 1025 of 1100 rows": _by_family((UNSUPPORTED, b"k <= 1024"), (UNSUPPORTED, b"k <= 1024")),
    "index of d = 128": _by_family((BAD, b"disagree"), (BAD, b"disagree")),
    "workspace one byte short": _by_family((CAPACITY, b"workspace smaller than"), (CAPACITY, b"workspace smaller than")),
    "workspace offset by 8 bytes": _by_family((BAD, b"aligned"), (BAD, b"aligned")),
    "preprojection off": _by_kind((OK, None), (UNSUPPORTED, b"preprojection")),
    "options.struct_bytes = 4": _by_family((BAD, b"nann_search_options: struct_bytes"), (BAD, b"nann_search_options: struct_bytes")),
    "short workspace + bad options": _short_and_bad_options(),
    "short workspace + preprojection off": _by_family((CAPACITY, b"workspace smaller than"), (CAPACITY, b"workspace smaller than")),
    "misaligned workspace + k = n_items + 1": _by_family((TOPK, b"at least k"), (BAD, b"aligned")),
}
# the same of the *_workspace_bytes twin (the cases it has the arguments for)
BYTES = {case: SEARCH[case] for case in ("k = -1", "k = n_items + 1", "k = 1025 of 1100 rows", "index of d = 128")}


class _Setup:
    """the three indexes, the five scorers / models and one set of inputs, built once"""

    def __init__(self, tmp):
        from nann_amd import _lib, ops, retrieval, synth
        self.L = _lib.lib()
        self.dix = _corpus(N, 64)[2]
        self.dix128 = _corpus(N, 128)[2]
        self.dix_big = _corpus(N_BIG, 64)[2]
        w = synth.make_mlp_weights(64)
        ops.save_scorer_dir(str(tmp / "l2"), "l2")
        ops.save_scorer_dir(str(tmp / "mlp"), "mlp", w, precision="exact")
        self.by = {"l2": ops.Scorer("l2", 64), "mlp": ops.Scorer("mlp", 64, torch.float16, w, precision="split"),
                   "l2m": ops.Model(str(tmp / "l2"), 64, L_SEQ), "mlpm": ops.Model(str(tmp / "mlp"), 64, L_SEQ),
                   "attn": _model(tmp, 64, "split")}
        rng = np.random.default_rng(5)
        self.q = cuda(rng.standard_normal((B, 64)).astype(np.float32))
        self.seq = cuda(_corpus(N, 64)[5][:B], torch.float16)
        self.splits = cuda(np.arange(B + 1, dtype=np.int64) * LIST)
        self.rows = cuda(rng.integers(0, N, B * LIST).astype(np.int32))
        self.filter = retrieval.make_filter(self.dix, deny_rows=np.array([1, 2, 3]))
        self.off = retrieval.search_options(preprojection=False)
        self.bad_options = retrieval.search_options()
        self.bad_options.struct_bytes = 4
        self.bad_options_off = retrieval.search_options(preprojection=False)
        self.bad_options_off.struct_bytes = 4


class _Call:
    """one entry point under one scorer or model, every argument replaceable; outputs pre-filled with a sentinel"""

    def __init__(self, s, entry, kind):
        self.s, self.entry, self.kind = s, entry, kind
        self.model = entry.endswith("model") or entry.endswith("model_filtered")
        self.lists = entry.startswith("candidates")
        self.filtered = entry.endswith("filtered")
        self.fn = getattr(s.L, "nann_search_" + entry)
        self.fn_bytes = getattr(s.L, "nann_search_" + entry + "_workspace_bytes")
        st, self.nbytes = self.ws_bytes()
        assert st == OK and self.nbytes > 0 and self.nbytes % 256 == 0, (entry, kind, st, self.nbytes)
        self.ws = torch.zeros(self.nbytes + 256, dtype=torch.uint8, device="cuda")
        assert self.ws.data_ptr() % 256 == 0
        self.fill()

    def fill(self):
        shapes = {"item_ids": ((B, K_ROOM), torch.int64), "scores": ((B, K_ROOM), torch.float32), "index": ((B, K_ROOM), torch.int32),
                  "pos": ((B, K_ROOM), torch.int32), "n_out": ((B,), torch.int32), "status": ((B,), torch.int32)}
        self.out = {f: torch.full(shape, SENTINEL, dtype=dt, device="cuda") for f, (shape, dt) in shapes.items()}

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in self.out.values())

    def ws_bytes(self, **kw):
        nb = C.c_int64(-1)
        head = (kw.get("ix", self.s.dix).handle, self.s.by[self.kind].handle, kw.get("n", B))
        if self.lists:
            st = self.fn_bytes(*head, B * LIST, kw.get("k", K), C.byref(nb))
        else:
            st = self.fn_bytes(*head, kw.get("k", K), C.byref(nb))
        return st, nb.value

    def __call__(self, **kw):
        from nann_amd import _lib
        from nann_amd.ops import _ptr, _stream
        s, o = self.s, self.out
        options = kw.get("options")
        head = (kw.get("ix", s.dix).handle, s.by[self.kind].handle, _ptr(s.seq if self.model else s.q), kw.get("n", B), kw.get("k", K))
        tail = (_ptr(kw.get("ws", self.ws)), kw.get("ws_bytes", self.nbytes), C.byref(options) if options is not None else None)
        if self.lists:
            cand = _lib.Candidates()
            cand.struct_bytes = C.sizeof(_lib.Candidates)
            cand.row_splits, cand.rows, cand.n_cand = s.splits.data_ptr(), s.rows.data_ptr(), B * LIST
            st = self.fn(*head, C.byref(cand), _ptr(o["item_ids"]), _ptr(o["scores"]), _ptr(o["index"]), _ptr(o["pos"]),
                         _ptr(o["n_out"]), _ptr(o["status"]), *tail, _stream())
        elif self.filtered:
            st = self.fn(*head, _ptr(o["item_ids"]), _ptr(o["scores"]), _ptr(o["index"]), *tail, C.byref(s.filter.struct),
                         _ptr(o["n_out"]), _stream())
        else:
            st = self.fn(*head, _ptr(o["item_ids"]), _ptr(o["scores"]), _ptr(o["index"]), *tail, _stream())
        torch.cuda.synchronize()
        return st

    def arguments(self, case):
        """the keyword arguments of __call__ / ws_bytes that make `case`"""
        s = self.s
        return {"k = -1": {"k": -1}, "k = n_items + 1": {"k": N + 1}, "k = 1025 of 1100 rows": {"ix": s.dix_big, "k": 1025},
                "index of d = 128": {"ix": s.dix128}, "workspace one byte short": {"ws_bytes": self.nbytes - 1},
                "workspace offset by 8 bytes": {"ws": self.ws[8:]}, "preprojection off": {"options": s.off},
                "options.struct_bytes = 4": {"options": s.bad_options},
                "short workspace + bad options": {"ws_bytes": self.nbytes - 1, "options": s.bad_options},
                "short workspace + preprojection off": {"ws_bytes": self.nbytes - 1, "options": s.off},
                "misaligned workspace + k = n_items + 1": {"ws": self.ws[8:], "k": N + 1}}[case]


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    require_gpu()
    return _Setup(tmp_path_factory.mktemp("flat_contract"))


def _check(got, want, error, what):
    status, text = want
    print(what, "->", got, error)
    assert got == status, (what, got, error)
    if text is not None:
        assert text in error, (what, error)


@pytest.mark.parametrize("entry,kind", CONFIGS)
def test_status_codes_of_the_search_call(setup, entry, kind):
    call = _Call(setup, entry, kind)
    for case, want in SEARCH.items():
        call.fill()
        got = call(**call.arguments(case))
        _check(got, want[(entry, kind)], setup.L.nann_last_error(), (entry, kind, case))
        if got != OK:
            assert call.untouched(), (entry, kind, case)


@pytest.mark.parametrize("entry,kind", CONFIGS)
def test_status_codes_of_the_workspace_size(setup, entry, kind):
    call = _Call(setup, entry, kind)
    for case, want in BYTES.items():
        kw = {a: v for a, v in call.arguments(case).items() if a in ("ix", "k")}
        got, _ = call.ws_bytes(**kw)
        _check(got, want[(entry, kind)], setup.L.nann_last_error(), (entry, kind, case, "bytes"))
    assert call.ws_bytes(n=0) == (OK, 0) and call.ws_bytes(k=0) == (OK, 0)


@pytest.mark.parametrize("entry,kind", CONFIGS)
def test_no_op_calls_write_nothing(setup, entry, kind):
    call = _Call(setup, entry, kind)
    assert call(n=0) == OK and call(k=0) == OK and call(k=0, ws=None, ws_bytes=0) == OK and call(n=0, ws=None, ws_bytes=0) == OK
    assert call.untouched()
