"""-m gpu: the status codes of the scalar-quantised search calls through the C ABI, pinned.  nann_search_all_sq8,
nann_search_all_sq8_stream, nann_search_all_sq8_exact, nann_search_all_range_sq8_exact, nann_search_all_sq8_stream_exact,
nann_search_all_range_sq8_stream_exact, the *_workspace_bytes twin of each and nann_search_all_sq8_exact_layout, under an L2 and an
inner-product scorer: which status a faulty argument gets, nann_last_error()'s text, WHICH fault wins where two are present, what a
call with nothing to do looks at, and the workspace sizes at one shape -- the six forms differ in all of these, and callers may rely
on any.  The expected values are literals, recorded from the library before the six forms were given one shared host path
(csrc/nann_flat.hip); nothing here is computed from the code under test.  300 rows of d = 64 in f16, batch 3, k = 5, fetch = 10,
cap = 16, sample_rows = 64: every faulty call is refused on the host before any launch, and the few that run take milliseconds."""
import ctypes as C

import numpy as np
import pytest
import torch

import sq8_model as M
from gpu_util import cuda, require_gpu
from test_sq8_exact_gpu import _index, _rows

pytestmark = pytest.mark.gpu
N, B, K, FETCH, CAP, SAMPLE, CAPACITY_ROWS = 300, 3, 5, 10, 16, 64, 64
OK, TOPK, BAD, UNSUPPORTED, CAPACITY = 0, 4, 7, 102, 103
SENTINEL = -77
K_ROOM = 16  # the outputs hold the widest k a case of this file gets through a call

# form -> (entry point, has bounds, is a range form, has sample_rows, cap: None, "i32" or "i64")
FORMS = {"plain": ("nann_search_all_sq8", False, False, False, None),
         "stream": ("nann_search_all_sq8_stream", False, False, True, "i32"),
         "exact": ("nann_search_all_sq8_exact", True, False, False, "i64"),
         "range": ("nann_search_all_range_sq8_exact", True, True, False, "i64"),
         "stream_exact": ("nann_search_all_sq8_stream_exact", True, False, True, "i64"),
         "range_stream": ("nann_search_all_range_sq8_stream_exact", True, True, False, "i64")}
METRICS = ("l2", "ip")
CONFIGS = [(form, metric) for form in FORMS for metric in METRICS]
# one below the least cap a form takes: k, fetch or 1
CAP_FLOOR = {"stream": K - 1, "exact": FETCH - 1, "stream_exact": FETCH - 1, "range": 0, "range_stream": 0}
TWIN_ARGUMENTS = ("ix", "t", "b", "sc", "n", "k", "fetch", "cap", "sample_rows")

# ---- the literals: {who} is the entry point's name ------------------------------------------------------------------------------
NULL = (BAD, "{who}: null argument")
OPTIONS = (BAD, "nann_search_options: struct_bytes")
K_RANGE = (BAD, "{who}: k must lie in [0, fetch]")
NO_ENTRIES = (BAD, "{who}: out_item_ids is null while capacity > 0")
F32 = (UNSUPPORTED, "{who}: 16-bit rows (f16, bf16) only")
SAMPLE_ROWS = (BAD, "{who}: sample_rows must not be negative")
EVERY_FORM = {"index of d = 128": (BAD, "scorer and index disagree on d / dtype"), "null table": NULL,
              "table of another index": (BAD, "{who}: the code table was made from another index"),
              "MLP scorer": (UNSUPPORTED, "{who}: the scorer is NANN_SCORER_L2 or NANN_SCORER_IP, not a learned scorer"),
              "null q": NULL, "options.struct_bytes = 4": OPTIONS,
              "workspace one byte short": (CAPACITY, "workspace smaller than {who}_workspace_bytes()"),
              "workspace offset by 8 bytes": (BAD, "{who}: workspace must be 256-byte aligned"), "short workspace + bad options": OPTIONS}
TOP_K = {"null out_item_ids": NULL, "null output + short workspace": NULL, "k = -1": K_RANGE, "k > fetch": K_RANGE,
         "fetch = 1025": (TOPK, "input must have at least k columns. Had 300, needed 1025"), "k > fetch + table of another index": K_RANGE}
BOUNDED = {"null bounds": NULL, "bounds of another table": (BAD, "{who}: the bounds were made from another index or code table"),
           "null bounds + null table": NULL, "null bounds + MLP scorer": NULL, "null out_certified": NULL, "null out_n_survivors": NULL,
           "cap = 2**31": (UNSUPPORTED, "{who}: cap beyond the longest list of a candidate-list search, 715827882 at this chunk")}
RANGE = {"null out_item_ids": NO_ENTRIES, "null output + short workspace": NO_ENTRIES, "cap below its floor": (BAD, "{who}: cap must be at least 1"),
         "f32 index": F32, "f32 index + null bounds": F32, "capacity = -1": (BAD, "{who}: capacity < 0"), "null out_row_splits": NULL,
         "null thresholds": NULL, "cap below its floor + capacity = -1": (BAD, "{who}: cap must be at least 1")}
CAP_K, CAP_FETCH = (BAD, "{who}: cap must be at least k"), (BAD, "{who}: cap must be at least fetch")
# form -> case -> (status, nann_last_error() or None) of the SEARCH call, the same under either metric.  The *_workspace_bytes twin
# and nann_search_all_sq8_exact_layout gave, for the cases they have the arguments of, the same with their own name for {who}
SEARCH = {"plain": {**EVERY_FORM, **TOP_K},
          "stream": {**EVERY_FORM, **TOP_K, "cap below its floor": CAP_K, "null out_n_survivors": (OK, None), "sample_rows = -1": SAMPLE_ROWS,
                     "bad cap + bad sample_rows": CAP_K, "null out_complete": NULL},
          "exact": {**EVERY_FORM, **TOP_K, **BOUNDED, "cap below its floor": CAP_FETCH},
          "range": {**EVERY_FORM, **BOUNDED, **RANGE},
          "stream_exact": {**EVERY_FORM, **TOP_K, **BOUNDED, "cap below its floor": CAP_FETCH, "sample_rows = -1": SAMPLE_ROWS,
                           "bad cap + bad sample_rows": CAP_FETCH},
          "range_stream": {**EVERY_FORM, **BOUNDED, **RANGE}}
NULL_BYTES = (BAD, "{who}_workspace_bytes: null argument")
# form -> what *_workspace_bytes gives at the shape of this file, under either metric
SIZES = {"plain": 11520, "stream": 9216, "exact": 13568, "range": 11264, "stream_exact": 10496, "range_stream": 3328}
# the eight numbers of nann_search_all_sq8_exact_layout at the shape of this file, and at k = 0, under either metric
LAYOUT_NUMBERS = [3, 16, 13056, 13312, 12544, 32, 12288, 13568]
LAYOUT_NUMBERS_K0 = [3, 16, 12544, 12800, 12032, 32, 12032, 13056]
# form -> a call with nothing to do, its outputs and workspace NULL and its options faulty
NOTHING, BAD_CAPACITY = {"n = 0": (OK, None), "k = 0": (OK, None)}, {"n = 0": (OK, None), "n = 0 + capacity = -1": (BAD, "{who}: capacity < 0")}
EMPTY = {"plain": NOTHING, "stream": NOTHING, "exact": NOTHING, "range": BAD_CAPACITY, "stream_exact": NOTHING, "range_stream": BAD_CAPACITY}


def _named(want, suffix):
    """a literal of the search call as its twin words it"""
    return (want[0], None if want[1] is None else want[1].replace("{who}", "{who}" + suffix))


class _Setup:
    """the indexes, tables, bounds and scorers and one set of inputs, built once"""

    def __init__(self):
        from nann_amd import _lib, ops, retrieval, synth
        self.L = _lib.lib()
        x = _rows(N, 64, 11)
        self.dix, self.dix_other = _index(x), _index(x)
        self.dix128 = _index(_rows(N, 128, 12))
        self.dix_f32 = _index(M.widen(x).astype(np.float32))
        self.t = retrieval.make_sq8(self.dix)
        self.b = retrieval.make_sq8_bounds(self.dix, self.t)
        self.t_other = retrieval.make_sq8(self.dix_other)          # a table of another index of the same shape
        self.t_again = retrieval.make_sq8(self.dix)                # another table of the same index,
        self.b_other = retrieval.make_sq8_bounds(self.dix, self.t_again)  # and its bounds
        self.sc = {m: ops.Scorer(m, 64, torch.float16) for m in METRICS}
        self.sc_f32 = {m: ops.Scorer(m, 64, torch.float32) for m in METRICS}
        self.mlp = ops.Scorer("mlp", 64, torch.float16, synth.make_mlp_weights(64), precision="exact")
        rng = np.random.default_rng(5)
        self.q = cuda(rng.standard_normal((B, 64)).astype(np.float32))
        self.thr = {"l2": cuda(np.full(B, -60.0, np.float32)), "ip": cuda(np.full(B, 5.0, np.float32))}
        self.bad_options = retrieval.search_options()
        self.bad_options.struct_bytes = 4


class _Call:
    """one entry point under one scorer, every argument replaceable; outputs pre-filled with a sentinel"""

    def __init__(self, s, form, metric):
        self.s, self.form, self.metric = s, form, metric
        self.who, self.bounds, self.range, self.sampled, self.cap = FORMS[form]
        self.fn = getattr(s.L, self.who)
        self.fn_bytes = getattr(s.L, self.who + "_workspace_bytes")
        st, self.nbytes = self.ws_bytes()
        assert st == OK and self.nbytes > 0 and self.nbytes % 256 == 0, (form, metric, st, self.nbytes)
        self.ws = torch.zeros(self.nbytes + 256, dtype=torch.uint8, device="cuda")
        assert self.ws.data_ptr() % 256 == 0
        self.fill()

    def fill(self):
        shapes = {"item_ids": ((B, K_ROOM), torch.int64), "scores": ((B, K_ROOM), torch.float32), "index": ((B, K_ROOM), torch.int32),
                  "fetch_index": ((B, K_ROOM), torch.int32), "fetch_scores": ((B, K_ROOM), torch.float32),
                  "complete": ((B,), torch.int32), "certified": ((B,), torch.int32), "n_survivors": ((B,), torch.int32),
                  "cut": ((B,), torch.float32), "row_splits": ((B + 1,), torch.int64)}
        if self.range:
            for f in ("item_ids", "scores", "index"):
                shapes[f] = ((CAPACITY_ROWS,), shapes[f][1])
        self.out = {f: torch.full(shape, SENTINEL, dtype=dt, device="cuda") for f, (shape, dt) in shapes.items()}

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in self.out.values())

    def _head(self, kw):
        s = self.s
        handle = lambda v: v.handle if v is not None else None  # noqa: E731
        head = [handle(kw.get("ix", s.dix)), handle(kw.get("t", s.t))]
        if self.bounds:
            head.append(handle(kw.get("b", s.b)))
        return head + [handle(kw.get("sc", s.sc[self.metric]))]

    def _shape(self, kw):
        """the arguments between n_queries and the outputs, in the order of the form"""
        if self.range:
            return [kw.get("cap", CAP)]
        shape = [kw.get("fetch", FETCH)]
        if self.sampled:
            shape.append(kw.get("sample_rows", SAMPLE))
        if self.cap:
            shape.append(kw.get("cap", CAP))
        return shape + [kw.get("k", K)]

    def ws_bytes(self, layout=False, **kw):
        fn = getattr(self.s.L, self.who + "_layout") if layout else self.fn_bytes
        nb = (C.c_int64 * 8)(*[-1] * 8)
        st = fn(*self._head(kw), kw.get("n", B), *self._shape(kw), nb)
        return st, (list(nb) if layout else nb[0])

    def __call__(self, **kw):
        from nann_amd.ops import _ptr, _stream
        s = self.s
        o = {f: (None if kw.get("null") == "all" or f in kw.get("null", ()) else t) for f, t in self.out.items()}
        options = kw.get("options")
        q = None if "q" in kw.get("null", ()) else s.q
        thr = None if "thresholds" in kw.get("null", ()) else s.thr[self.metric]
        tail = (_ptr(kw.get("ws", self.ws)), kw.get("ws_bytes", self.nbytes), C.byref(options) if options is not None else None, _stream())
        top = (_ptr(o["item_ids"]), _ptr(o["scores"]), _ptr(o["index"]))
        if self.range:
            args = [_ptr(q), kw.get("n", B), _ptr(thr), kw.get("cap", CAP), kw.get("capacity", CAPACITY_ROWS), _ptr(o["row_splits"]), *top,
                    _ptr(o["certified"]), _ptr(o["n_survivors"])]
        else:
            args = [_ptr(q), kw.get("n", B), *self._shape(kw), *top]
            if self.form == "plain":
                args += [_ptr(o["fetch_index"]), _ptr(o["fetch_scores"])]
            elif self.form == "stream":
                args += [_ptr(o["complete"]), _ptr(o["n_survivors"]), _ptr(o["cut"])]
            else:
                args += [_ptr(o["certified"]), _ptr(o["n_survivors"])]
        st = self.fn(*self._head(kw), *args, *tail)
        torch.cuda.synchronize()
        return st

    def cases(self):
        """case -> the keyword arguments of __call__ / ws_bytes that make it, for the cases this form has the arguments of"""
        s, m = self.s, self.metric
        short = {"ws_bytes": self.nbytes - 1}
        c = {"index of d = 128": {"ix": s.dix128}, "null table": {"t": None}, "table of another index": {"t": s.t_other},
             "MLP scorer": {"sc": s.mlp}, "null q": {"null": ("q",)}, "null out_item_ids": {"null": ("item_ids",)},
             "options.struct_bytes = 4": {"options": s.bad_options}, "workspace one byte short": short,
             "workspace offset by 8 bytes": {"ws": self.ws[8:]}, "short workspace + bad options": dict(short, options=s.bad_options),
             "null output + short workspace": dict(short, null=("item_ids",))}
        if not self.range:
            c.update({"k = -1": {"k": -1}, "k > fetch": {"k": FETCH + 1}, "fetch = 1025": {"fetch": 1025},
                      "k > fetch + table of another index": {"k": FETCH + 1, "t": s.t_other}})
        if self.bounds:
            c.update({"null bounds": {"b": None}, "bounds of another table": {"b": s.b_other}, "null bounds + null table": {"b": None, "t": None},
                      "null bounds + MLP scorer": {"b": None, "sc": s.mlp}, "null out_certified": {"null": ("certified",)}})
        if self.cap:
            c["cap below its floor"] = {"cap": CAP_FLOOR[self.form]}
            c["null out_n_survivors"] = {"null": ("n_survivors",)}
        if self.cap == "i64":
            c["cap = 2**31"] = {"cap": 2 ** 31}
        if self.sampled:
            c["sample_rows = -1"] = {"sample_rows": -1}
            c["bad cap + bad sample_rows"] = {"cap": CAP_FLOOR[self.form], "sample_rows": -1}
        if self.form == "stream":
            c["null out_complete"] = {"null": ("complete",)}
        if self.range:
            f32 = {"ix": s.dix_f32, "sc": s.sc_f32[m]}
            c.update({"f32 index": f32, "f32 index + null bounds": dict(f32, b=None), "capacity = -1": {"capacity": -1},
                      "null out_row_splits": {"null": ("row_splits",)}, "null thresholds": {"null": ("thresholds",)},
                      "cap below its floor + capacity = -1": {"cap": 0, "capacity": -1}})
        return c

    def twin_cases(self):
        return {case: kw for case, kw in self.cases().items() if all(a in TWIN_ARGUMENTS for a in kw)}

    def empty_cases(self):
        """calls with nothing to do, every other argument faulty: NULL outputs, NULL workspace, bad options"""
        rest = {"null": "all", "ws": None, "ws_bytes": 0, "options": self.s.bad_options}
        c = {"n = 0": dict(rest, n=0)}
        if self.range:
            c["n = 0 + capacity = -1"] = dict(rest, n=0, capacity=-1)
        else:
            c["k = 0"] = dict(rest, k=0)
        return c


def observe(status, lib, who):
    """(status, nann_last_error() with the entry point's name taken out, or None behind a call that succeeded)"""
    return (status, None if status == OK else lib.nann_last_error().decode().replace(who, "{who}"))


@pytest.fixture(scope="module")
def setup():
    require_gpu()
    return _Setup()


def _check(got, want, what):
    print(what, "->", got)
    assert got == tuple(want), (what, got, want)


@pytest.mark.parametrize("form,metric", CONFIGS)
def test_status_codes_of_the_search_call(setup, form, metric):
    call = _Call(setup, form, metric)
    cases = call.cases()
    assert sorted(cases) == sorted(SEARCH[form]), form
    for case, kw in cases.items():
        call.fill()
        got = observe(call(**kw), setup.L, call.who)
        _check(got, SEARCH[form][case], (form, metric, case))
        if got[0] != OK:
            assert call.untouched(), (form, metric, case)


@pytest.mark.parametrize("form,metric", CONFIGS)
def test_status_codes_of_the_workspace_size(setup, form, metric):
    call = _Call(setup, form, metric)
    for case, kw in call.twin_cases().items():
        want = SEARCH[form][case]
        _check(observe(call.ws_bytes(**kw)[0], setup.L, call.who), _named(want, "_workspace_bytes"), (form, metric, case, "bytes"))
        if form == "exact":
            _check(observe(call.ws_bytes(layout=True, **kw)[0], setup.L, call.who), _named(want, "_layout"), (form, metric, case, "layout"))
    assert call.ws_bytes() == (OK, SIZES[form])
    assert call.ws_bytes(n=0) == (OK, 0) and (call.range or call.ws_bytes(k=0) == (OK, 0))
    assert observe(call.fn_bytes(*call._head({}), B, *call._shape({}), None), setup.L, call.who) == NULL_BYTES
    if form == "exact":
        assert call.ws_bytes(layout=True) == (OK, LAYOUT_NUMBERS)
        assert call.ws_bytes(layout=True, k=0) == (OK, LAYOUT_NUMBERS_K0)


@pytest.mark.parametrize("form,metric", CONFIGS)
def test_calls_with_nothing_to_do(setup, form, metric):
    call = _Call(setup, form, metric)
    cases = call.empty_cases()
    assert sorted(cases) == sorted(EMPTY[form]), form
    for case, kw in cases.items():
        _check(observe(call(**kw), setup.L, call.who), EMPTY[form][case], (form, metric, case))
    assert call(n=0) == OK and (call.range or call(k=0) == OK)
    assert call.untouched()
