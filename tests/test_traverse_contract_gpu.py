"""-m gpu: the status codes of the traversal family through the C ABI, pinned.  nann_search_opt, nann_search_model_opt,
nann_search_filtered, nann_search_model_filtered, nann_search_eval, nann_search_eval_ex, nann_search_eval_model and the
*_workspace_bytes call of each, under every kind of scorer (l2, ip, split-f16 mlp) or model (l2, mlp, ip, split-f16 attention)
the call takes: which status a faulty argument gets, the text of nann_last_error(), WHICH fault wins where two are present --
the entry points differ in that, and callers may rely on either -- and that a refused call leaves its outputs alone.  The
expected values are literals, recorded by running this file's own calls against the library of commit 23ff5b5 ("HNSW builder:
append rows to a built graph, export CSR on the device"), the last one before the family was given one shared host path
(csrc/nann_traverse.hip); nothing here is computed from the code under test.  300 rows of d = 64 on a ring graph, batch 3,
level_topn (16, 16, 16, 8, 4, 5), evaluation arguments (3, 1, 1) / (16, 8, 5) / 5: the calls reach every branch and take
milliseconds."""
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
N, N_BIG, B, F = 300, 1100, 3, 5
T = (16, 16, 16, 8, 4, F)  # (every query of every call is served: narrower beams run out of new rows on the ring)
NUM_SCORING, TOP_K, TOPK_EVAL = (3, 1, 1), (16, 8, 5), 5
OK, BAD, UNSUPPORTED, CAPACITY = 0, 7, 102, 103
SENTINEL = -77
WIDTH = 8  # columns of the outputs: the widest k or topk_eval a case of this file gets through a call, and room behind it

SCORERS, MODELS = ("l2", "ip", "mlp"), ("l2m", "mlpm", "ipm", "attn")
ENTRIES = {"opt": SCORERS, "model_opt": MODELS, "filtered": SCORERS, "model_filtered": MODELS,
           "eval": SCORERS, "eval_ex": SCORERS, "eval_model": MODELS}
CONFIGS = [(e, kind) for e, kinds in ENTRIES.items() for kind in kinds]
SYMBOL = {"opt": "nann_search_opt", "model_opt": "nann_search_model_opt", "filtered": "nann_search_filtered",
          "model_filtered": "nann_search_model_filtered", "eval": "nann_search_eval", "eval_ex": "nann_search_eval_ex",
          "eval_model": "nann_search_eval_model"}
BYTES_SYMBOL = {"opt": "nann_search_workspace_bytes", "model_opt": "nann_search_model_workspace_bytes",
                "filtered": "nann_search_filtered_workspace_bytes", "model_filtered": "nann_search_model_filtered_workspace_bytes",
                "eval": "nann_search_eval_workspace_bytes", "eval_ex": "nann_search_eval_workspace_bytes",
                "eval_model": "nann_search_eval_workspace_bytes"}

# ---- the cases: name -> keyword arguments of _Call.__call__ ---------------------------------------------------------------
_ANY = {
    "plain": {},
    "null out_item_ids": {"null_out": True},
    "n = 0": {"n": 0},
    "n = 0, workspace null and 0 bytes": {"n": 0, "ws": None, "ws_bytes": 0},
    "index of d = 128": {"ix": "dix128"},
    "index of d = 128, n = 0": {"ix": "dix128", "n": 0},
    "workspace null": {"ws": None},
    "workspace one byte short": {"short": 1},
}
_TRAVERSAL = dict(_ANY, **{
    "level_topn entry of 1025": {"t_1025": True},
    "options.struct_bytes = 4": {"options": "bad_options"},
    "short workspace + bad options": {"short": 1, "options": "bad_options"},
})
_TICKS = {"per-query level_topn + phase_ticks": {"per_query": True, "ticks": True}}
_FILTERED = {
    "k = -1": {"k": -1},
    "k = F + 1": {"k": F + 1},
    "k = F + 1, n = 0": {"k": F + 1, "n": 0},
    "filter.struct_bytes = 4": {"filter": "bad_filter"},
    "bad filter + short workspace": {"filter": "bad_filter", "short": 1},
}
_EVAL = dict(_ANY, **{
    "num_scoring[2] = 2": {"num_scoring": (3, 1, 2)},
    "top_k_per_level entry of 0": {"top_k": (16, 0, 5)},
    "top_k_per_level entry of 2049": {"top_k": (16, 2049, 5)},
    "topk_eval = 0": {"topk_eval": 0},
})
CASES = {"opt": dict(_TRAVERSAL, **_TICKS), "model_opt": _TRAVERSAL, "filtered": dict(_TRAVERSAL, **_TICKS, **_FILTERED),
         "model_filtered": dict(_TRAVERSAL, **_FILTERED), "eval": _EVAL, "eval_ex": _EVAL, "eval_model": _EVAL}
# the *_workspace_bytes calls (the cases each has the arguments for)
_BYTES_T = {"plain": {}, "null nbytes": {"null_nbytes": True}, "level_topn entry of 1025": {"t_1025": True}, "n = 0": {"n": 0}}
_BYTES_E = {"plain": {}, "null nbytes": {"null_nbytes": True}, "n = 0": {"n": 0}}
BYTES_CASES = {e: (_BYTES_E if e.startswith("eval") else _BYTES_T) for e in ENTRIES}

# ---- what commit 23ff5b5 answers: entry -> case -> kind ("*": every kind of the entry) -> (status, nann_last_error()) ------
# (the scorer form of the traversal checks its workspace against the plan it runs, not the widest: one byte short is enough
#  for it; the model forms hold the caller to the size they named)
NO_IP_SCORER = (UNSUPPORTED, "nann_search_eval: the inner-product scorer (NANN_SCORER_IP) is not supported by the evaluation traversal")
NO_IP_MODEL = (UNSUPPORTED, "nann_search_eval_model: an inner-product model (NANN_MODEL_IP) is not supported by the evaluation traversal")
EXPECTED = {"opt": {"plain": {"*": (0, None)},
         "null out_item_ids": {"*": (7, "nann_search_opt: null argument")},
         "n = 0": {"*": (0, None)},
         "n = 0, workspace null and 0 bytes": {"*": (0, None)},
         "index of d = 128": {"*": (7, "scorer and index disagree on d / dtype")},
         "index of d = 128, n = 0": {"*": (0, None)},
         "workspace null": {"*": (103, "workspace smaller than nann_search_workspace_bytes()")},
         "workspace one byte short": {"*": (0, None)},
         "level_topn entry of 1025": {"*": (102, "level_topn entries must be in [0, 1024]")},
         "options.struct_bytes = 4": {"*": (7, "nann_search_options: struct_bytes")},
         "short workspace + bad options": {"*": (7, "nann_search_options: struct_bytes")},
         "per-query level_topn + phase_ticks": {"*": (102, "nann_search_opt: phase ticks with a uniform level_topn only")}},
 "model_opt": {"plain": {"*": (0, None)},
               "null out_item_ids": {"*": (7, "nann_search_model: null argument")},
               "n = 0": {"*": (0, None)},
               "n = 0, workspace null and 0 bytes": {"*": (7, "nann_search_model: null argument")},
               "index of d = 128": {"*": (7, "model and index disagree on d / dtype")},
               "index of d = 128, n = 0": {"*": (0, None)},
               "workspace null": {"*": (7, "nann_search_model: null argument")},
               "workspace one byte short": {"*": (103, "workspace smaller than nann_search_model_workspace_bytes()")},
               "level_topn entry of 1025": {"*": (102, "level_topn entries must be in [0, 1024]")},
               "options.struct_bytes = 4": {"*": (7, "nann_search_options: struct_bytes")},
               "short workspace + bad options": {"*": (103, "workspace smaller than nann_search_model_workspace_bytes()")}},
 "filtered": {"plain": {"*": (0, None)},
              "null out_item_ids": {"*": (7, "nann_search_filtered: null argument")},
              "n = 0": {"*": (0, None)},
              "n = 0, workspace null and 0 bytes": {"*": (0, None)},
              "index of d = 128": {"*": (7, "scorer and index disagree on d / dtype")},
              "index of d = 128, n = 0": {"*": (0, None)},
              "workspace null": {"*": (103, "workspace smaller than nann_search_filtered_workspace_bytes()")},
              "workspace one byte short": {"*": (103, "workspace smaller than nann_search_filtered_workspace_bytes()")},
              "level_topn entry of 1025": {"*": (102, "level_topn entries must be in [0, 1024]")},
              "options.struct_bytes = 4": {"*": (7, "nann_search_options: struct_bytes")},
              "short workspace + bad options": {"*": (103, "workspace smaller than nann_search_filtered_workspace_bytes()")},
              "per-query level_topn + phase_ticks": {"*": (102, "nann_search_opt: phase ticks with a uniform level_topn only")},
              "k = -1": {"*": (7, "nann_search_filtered: k must lie in [0, level_topn_max[5]]")},
              "k = F + 1": {"*": (7, "nann_search_filtered: k must lie in [0, level_topn_max[5]]")},
              "k = F + 1, n = 0": {"*": (7, "nann_search_filtered: k must lie in [0, level_topn_max[5]]")},
              "filter.struct_bytes = 4": {"*": (7, "nann_filter: struct_bytes")},
              "bad filter + short workspace": {"*": (7, "nann_filter: struct_bytes")}},
 "model_filtered": {"plain": {"*": (0, None)},
                    "null out_item_ids": {"*": (7, "nann_search_model_filtered: null argument")},
                    "n = 0": {"*": (0, None)},
                    "n = 0, workspace null and 0 bytes": {"*": (7, "nann_search_model_filtered: null argument")},
                    "index of d = 128": {"*": (7, "model and index disagree on d / dtype")},
                    "index of d = 128, n = 0": {"*": (0, None)},
                    "workspace null": {"*": (7, "nann_search_model_filtered: null argument")},
                    "workspace one byte short": {"*": (103, "workspace smaller than nann_search_model_filtered_workspace_bytes()")},
                    "level_topn entry of 1025": {"*": (102, "level_topn entries must be in [0, 1024]")},
                    "options.struct_bytes = 4": {"*": (7, "nann_search_options: struct_bytes")},
                    "short workspace + bad options": {"*": (103,
                                                            "workspace smaller than nann_search_model_filtered_workspace_bytes()")},
                    "k = -1": {"*": (7, "nann_search_model_filtered: k must lie in [0, level_topn_max[5]]")},
                    "k = F + 1": {"*": (7, "nann_search_model_filtered: k must lie in [0, level_topn_max[5]]")},
                    "k = F + 1, n = 0": {"*": (7, "nann_search_model_filtered: k must lie in [0, level_topn_max[5]]")},
                    "filter.struct_bytes = 4": {"*": (7, "nann_filter: struct_bytes")},
                    "bad filter + short workspace": {"*": (7, "nann_filter: struct_bytes")}},
 "eval": {"plain": {"l2": (0, None), "ip": NO_IP_SCORER, "mlp": (0, None)},
          "null out_item_ids": {"*": (7, "nann_search_eval: null argument")},
          "n = 0": {"*": (0, None)},
          "n = 0, workspace null and 0 bytes": {"*": (0, None)},
          "index of d = 128": {"*": (7, "scorer and index disagree on d / dtype")},
          "index of d = 128, n = 0": {"*": (0, None)},
          "workspace null": {"l2": (103, "workspace smaller than nann_search_eval_workspace_bytes()"),
                             "ip": NO_IP_SCORER,
                             "mlp": (103, "workspace smaller than nann_search_eval_workspace_bytes()")},
          "workspace one byte short": {"l2": (0, None), "ip": NO_IP_SCORER, "mlp": (0, None)},
          "num_scoring[2] = 2": {"l2": (7, "num_scoring_per_level[2] must be 1 (model.py:347)"),
                                 "ip": NO_IP_SCORER,
                                 "mlp": (7, "num_scoring_per_level[2] must be 1 (model.py:347)")},
          "top_k_per_level entry of 0": {"l2": (102, "top_k_per_level entries must be in [1, 2048]"),
                                         "ip": NO_IP_SCORER,
                                         "mlp": (102, "top_k_per_level entries must be in [1, 2048]")},
          "top_k_per_level entry of 2049": {"l2": (102, "top_k_per_level entries must be in [1, 2048]"),
                                            "ip": NO_IP_SCORER,
                                            "mlp": (102, "top_k_per_level entries must be in [1, 2048]")},
          "topk_eval = 0": {"l2": (102, "topk_eval must be in [1, 2048]"),
                            "ip": NO_IP_SCORER,
                            "mlp": (102, "topk_eval must be in [1, 2048]")}},
 "eval_ex": {"plain": {"l2": (0, None), "ip": NO_IP_SCORER, "mlp": (0, None)},
             "null out_item_ids": {"*": (7, "nann_search_eval_ex: null argument")},
             "n = 0": {"*": (0, None)},
             "n = 0, workspace null and 0 bytes": {"*": (0, None)},
             "index of d = 128": {"*": (7, "scorer and index disagree on d / dtype")},
             "index of d = 128, n = 0": {"*": (0, None)},
             "workspace null": {"l2": (103, "workspace smaller than nann_search_eval_workspace_bytes()"),
                                "ip": NO_IP_SCORER,
                                "mlp": (103, "workspace smaller than nann_search_eval_workspace_bytes()")},
             "workspace one byte short": {"l2": (0, None), "ip": NO_IP_SCORER, "mlp": (0, None)},
             "num_scoring[2] = 2": {"l2": (7, "num_scoring_per_level[2] must be 1 (model.py:347)"),
                                    "ip": NO_IP_SCORER,
                                    "mlp": (7, "num_scoring_per_level[2] must be 1 (model.py:347)")},
             "top_k_per_level entry of 0": {"l2": (102, "top_k_per_level entries must be in [1, 2048]"),
                                            "ip": NO_IP_SCORER,
                                            "mlp": (102, "top_k_per_level entries must be in [1, 2048]")},
             "top_k_per_level entry of 2049": {"l2": (102, "top_k_per_level entries must be in [1, 2048]"),
                                               "ip": NO_IP_SCORER,
                                               "mlp": (102, "top_k_per_level entries must be in [1, 2048]")},
             "topk_eval = 0": {"l2": (102, "topk_eval must be in [1, 2048]"),
                               "ip": NO_IP_SCORER,
                               "mlp": (102, "topk_eval must be in [1, 2048]")}},
 "eval_model": {"plain": {"l2m": (0, None), "mlpm": (0, None), "ipm": NO_IP_MODEL, "attn": (0, None)},
                "null out_item_ids": {"*": (7, "nann_search_eval_model: null argument")},
                "n = 0": {"*": (0, None)},
                "n = 0, workspace null and 0 bytes": {"*": (7, "nann_search_eval_model: null argument")},
                "index of d = 128": {"*": (7, "model and index disagree on d / dtype")},
                "index of d = 128, n = 0": {"*": (0, None)},
                "workspace null": {"*": (7, "nann_search_eval_model: null argument")},
                "workspace one byte short": {"l2m": (103, "workspace smaller than nann_search_eval_workspace_bytes()"),
                                             "mlpm": (103, "workspace smaller than nann_search_eval_workspace_bytes()"),
                                             "ipm": NO_IP_MODEL,
                                             "attn": (103, "workspace smaller than nann_search_eval_workspace_bytes()")},
                "num_scoring[2] = 2": {"l2m": (7, "num_scoring_per_level[2] must be 1 (model.py:347)"),
                                       "mlpm": (7, "num_scoring_per_level[2] must be 1 (model.py:347)"),
                                       "ipm": NO_IP_MODEL,
                                       "attn": (7, "num_scoring_per_level[2] must be 1 (model.py:347)")},
                "top_k_per_level entry of 0": {"l2m": (102, "top_k_per_level entries must be in [1, 2048]"),
                                               "mlpm": (102, "top_k_per_level entries must be in [1, 2048]"),
                                               "ipm": NO_IP_MODEL,
                                               "attn": (102, "top_k_per_level entries must be in [1, 2048]")},
                "top_k_per_level entry of 2049": {"l2m": (102, "top_k_per_level entries must be in [1, 2048]"),
                                                  "mlpm": (102, "top_k_per_level entries must be in [1, 2048]"),
                                                  "ipm": NO_IP_MODEL,
                                                  "attn": (102, "top_k_per_level entries must be in [1, 2048]")},
                "topk_eval = 0": {"l2m": (102, "topk_eval must be in [1, 2048]"),
                                  "mlpm": (102, "topk_eval must be in [1, 2048]"),
                                  "ipm": NO_IP_MODEL,
                                  "attn": (102, "topk_eval must be in [1, 2048]")}}}
# the same of the *_workspace_bytes calls: -> (status, nann_last_error(), nbytes; -1: not written)
EXPECTED_BYTES = {"opt": {"plain": {"*": (0, None, 439040)},
         "null nbytes": {"*": (7, "nann_search_workspace_bytes: null argument", -1)},
         "level_topn entry of 1025": {"*": (102, "level_topn entries must be in [0, 1024]", -1)},
         "n = 0": {"*": (0, None, 152576)}},
 "model_opt": {"plain": {"l2m": (0, None, 440064), "mlpm": (0, None, 440064), "ipm": (0, None, 440064), "attn": (0, None, 488448)},
               "null nbytes": {"*": (7, "nann_search_model_workspace_bytes: null argument", -1)},
               "level_topn entry of 1025": {"*": (102, "level_topn entries must be in [0, 1024]", -1)},
               "n = 0": {"l2m": (0, None, 152832), "mlpm": (0, None, 152832), "ipm": (0, None, 152832), "attn": (0, None, 87296)}},
 "filtered": {"plain": {"*": (0, None, 439296)},
              "null nbytes": {"*": (7, "nann_search_workspace_bytes: null argument", -1)},
              "level_topn entry of 1025": {"*": (102, "level_topn entries must be in [0, 1024]", -1)},
              "n = 0": {"*": (0, None, 152576)}},
 "model_filtered": {"plain": {"l2m": (0, None, 440320),
                              "mlpm": (0, None, 440320),
                              "ipm": (0, None, 440320),
                              "attn": (0, None, 488704)},
                    "null nbytes": {"*": (7, "nann_search_model_workspace_bytes: null argument", -1)},
                    "level_topn entry of 1025": {"*": (102, "level_topn entries must be in [0, 1024]", -1)},
                    "n = 0": {"l2m": (0, None, 152832),
                              "mlpm": (0, None, 152832),
                              "ipm": (0, None, 152832),
                              "attn": (0, None, 87296)}},
 "eval": {"plain": {"*": (0, None, 525056)},
          "null nbytes": {"*": (7, "nann_search_eval_workspace_bytes: null argument", -1)},
          "n = 0": {"*": (0, None, 175360)}},
 "eval_ex": {"plain": {"*": (0, None, 525056)},
             "null nbytes": {"*": (7, "nann_search_eval_workspace_bytes: null argument", -1)},
             "n = 0": {"*": (0, None, 175360)}},
 "eval_model": {"plain": {"l2m": (0, None, 525824), "mlpm": (0, None, 525824), "ipm": (0, None, 525824), "attn": (0, None, 770816)},
                "null nbytes": {"*": (7, "nann_search_eval_workspace_bytes: null argument", -1)},
                "n = 0": {"*": (0, None, 175360)}}}


class _Setup:
    """the indexes, the seven scorers / models and one set of inputs, built once"""

    def __init__(self, tmp):
        from nann_amd import _lib, ops, retrieval, synth
        self.L = _lib.lib()
        self.dix = _corpus(N, 64)[2]
        self.dix128 = _corpus(N, 128)[2]
        self.dix_big = _corpus(N_BIG, 64)[2]
        w = synth.make_mlp_weights(64)
        ops.save_scorer_dir(str(tmp / "l2"), "l2")
        ops.save_scorer_dir(str(tmp / "ip"), "ip")
        ops.save_scorer_dir(str(tmp / "mlp"), "mlp", w, precision="exact")
        self.by = {"l2": ops.Scorer("l2", 64), "ip": ops.Scorer("ip", 64),
                   "mlp": ops.Scorer("mlp", 64, torch.float16, w, precision="split"),
                   "l2m": ops.Model(str(tmp / "l2"), 64, L_SEQ), "mlpm": ops.Model(str(tmp / "mlp"), 64, L_SEQ),
                   "ipm": ops.Model(str(tmp / "ip"), 64, L_SEQ), "attn": _model(tmp, 64, "split")}
        rng = np.random.default_rng(5)
        self.q = cuda(rng.standard_normal((B, 64)).astype(np.float32))
        self.seq = cuda(_corpus(N, 64)[5][:B], torch.float16)
        self.filter = retrieval.make_filter(self.dix, deny_rows=np.array([1, 2, 3]))
        self.filter_big = retrieval.make_filter(self.dix_big, deny_rows=np.array([1, 2, 3]))
        self.bad_filter = retrieval.make_filter(self.dix, deny_rows=np.array([1, 2, 3]))
        self.bad_filter.struct.struct_bytes = 4
        self.bad_options = retrieval.search_options()
        self.bad_options.struct_bytes = 4


def _i32s(v):
    return (C.c_int32 * len(v))(*[int(x) for x in v])


class _Call:
    """one entry point under one scorer or model, every argument replaceable; outputs pre-filled with a sentinel"""

    def __init__(self, s, entry, kind):
        self.s, self.entry, self.kind = s, entry, kind
        self.model = "model" in entry
        self.eval = entry.startswith("eval")
        self.filtered = entry.endswith("filtered")
        self.fn = getattr(s.L, SYMBOL[entry])
        self.fn_bytes = getattr(s.L, BYTES_SYMBOL[entry])
        st, _, self.nbytes = self.ws_bytes()
        assert st == OK and self.nbytes > 0, (entry, kind, st, self.nbytes)
        self.ws = torch.zeros(self.nbytes + 256, dtype=torch.uint8, device="cuda")
        self.fill()

    def fill(self):
        from nann_amd import _lib
        shapes = {"item_ids": ((B, WIDTH), torch.int64), "scores": ((B, WIDTH), torch.float32), "index": ((B, WIDTH), torch.int32),
                  "n_out": ((B,), torch.int32), "status": ((B,), torch.int32),
                  "counters": ((B, 3, _lib.NUM_ROUNDS), torch.int32), "ticks": ((B, _lib.NUM_PHASES), torch.int64)}
        self.out = {f: torch.full(shape, SENTINEL, dtype=dt, device="cuda") for f, (shape, dt) in shapes.items()}

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in self.out.values())

    def ws_bytes(self, ix="dix", t_1025=False, n=B, null_nbytes=False):
        """(status, nann_last_error() or None, nbytes)"""
        s = self.s
        t = (T[0], 1025) + T[2:] if t_1025 else T
        nb = C.c_int64(-1)
        ref = None if null_nbytes else C.byref(nb)
        ixh, h = getattr(s, ix).handle, s.by[self.kind].handle
        if self.eval:
            st = self.fn_bytes(ixh, h if self.model else None, C.c_int64(n), ref)
        elif self.model:
            st = self.fn_bytes(ixh, h, _i32s(t), C.c_int64(n), ref)
        else:
            st = self.fn_bytes(ixh, _i32s(t), C.c_int64(n), ref)
        return st, (s.L.nann_last_error().decode() if st != OK else None), nb.value

    def __call__(self, ix="dix", n=B, t_1025=False, ws="own", ws_bytes=None, short=0, options=None, null_out=False, per_query=False,
                 ticks=False, k=F, filter="filter", num_scoring=NUM_SCORING, top_k=TOP_K, topk_eval=TOPK_EVAL):
        """-> (status, nann_last_error() or None)"""
        from nann_amd import _lib
        from nann_amd.ops import _ptr, _stream
        s, o = self.s, self.out
        t = (T[0], 1025) + T[2:] if t_1025 else T
        tq = cuda(np.tile(np.array(t, dtype=np.int32), (B, 1))) if per_query else None  # (every query at the maxima)
        ws = self.ws if isinstance(ws, str) else ws
        ws_bytes = C.c_int64((self.nbytes if ws_bytes is None else ws_bytes) - short)
        opt = C.byref(getattr(s, options)) if options is not None else None
        ids = C.c_void_p(0) if null_out else _ptr(o["item_ids"])
        head = (getattr(s, ix).handle, s.by[self.kind].handle, _ptr(s.seq if self.model else s.q), C.c_int64(n))
        outs = (ids, _ptr(o["scores"]), _ptr(o["index"]))
        if self.eval:
            tail = (_ptr(o["counters"]),) if self.entry == "eval_ex" else ()
            st = self.fn(*head, _i32s(num_scoring), _i32s(top_k), C.c_int32(topk_eval), _ptr(ws), ws_bytes, *outs,
                         _ptr(o["n_out"]), _ptr(o["status"]), *tail, _stream())
        else:
            plan = _lib.SearchPlan()
            args = head + (_i32s(t), _ptr(tq), _ptr(ws), ws_bytes) + outs + \
                (_ptr(o["status"]), _ptr(o["counters"]))
            if not self.model:
                args += (_ptr(o["ticks"] if ticks else None),)
            args += (opt, C.byref(plan))
            if self.filtered:
                args += (C.byref(getattr(s, filter).struct), C.c_int32(k), _ptr(o["n_out"]))
            st = self.fn(*args, _stream())
        torch.cuda.synchronize()
        return st, (s.L.nann_last_error().decode() if st != OK else None)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    require_gpu()
    return _Setup(tmp_path_factory.mktemp("traverse_contract"))


def _want(table, entry, case, kind):
    by_kind = table[entry][case]
    return tuple(by_kind[kind] if kind in by_kind else by_kind["*"])


def observe(s, entry, kind):
    """what the library answers: ({case: (status, error)}, {case: (status, error, nbytes)}), every refused or no-op call
    checked to have left its outputs alone, the plain call to have served every query"""
    call = _Call(s, entry, kind)
    search, size = {}, {}
    for case, kw in CASES[entry].items():
        call.fill()
        got = call(**kw)
        print((entry, kind, case), "->", got)
        search[case] = got
        if got[0] != OK or kw.get("n") == 0:
            assert call.untouched(), (entry, kind, case)
        elif case == "plain":
            assert bool((call.out["status"] == 0).all()), (entry, kind, call.out["status"])
    for case, kw in BYTES_CASES[entry].items():
        size[case] = call.ws_bytes(**kw)
        print((entry, kind, case, "bytes"), "->", size[case])
    return search, size


@pytest.mark.parametrize("entry,kind", CONFIGS)
def test_status_codes(setup, entry, kind):
    search, size = observe(setup, entry, kind)
    for case, got in search.items():
        assert got == _want(EXPECTED, entry, case, kind), (entry, kind, case, got)
    for case, got in size.items():
        assert got == _want(EXPECTED_BYTES, entry, case, kind), (entry, kind, case, "bytes", got)


def test_a_filter_made_for_another_index_is_refused_before_the_call(setup):
    """(the C ABI cannot tell: a nann_filter carries no size -- retrieval.search / search_model hold the two together)"""
    from nann_amd import retrieval
    s = setup
    for fn, by, x in ((retrieval.search, s.by["l2"], s.q), (retrieval.search_model, s.by["l2m"], s.seq)):
        with pytest.raises(AssertionError, match="the filter was made for another index"):
            fn(s.dix, by, x, T, filter=s.filter_big)
