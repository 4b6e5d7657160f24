"""-m gpu: every compiled instantiation of the flat-scorer traversal against a reference that is not the device.

search_queries<LPR, DT, VIS, SC, NT, LEAN> (nann_search.h) is compiled once per row width (LPR 8 / 16 / 32 / 64 for d = 64 / 128 /
256 / 512), row dtype (f16, bf16, f32), plan (VIS_LDS_HASH at 512 threads, VIS_LDS_HASH32 / VIS_LDS_BITMAP / VIS_HBM_BITMAP at
1024) and scorer (L2 = 0, inner product = kScorerIp = 12), as k_search and, on the two hash-set plans, as k_search_lean as
well: KERNELS below, 96 + 48.  Each is a code object of its own with its own register allocation and spill placement, so each
is launched here: 24 cases (d, dtype, scorer) x 8 launches, every launch asserting the plan it got and looking up the
instantiation that plan names in KERNELS.  test_traverse_matrix_cpu.py holds KERNELS to the build's own list of kernels.

The workload (traverse_matrix.py) is one 4 000-row host-built graph per d with scaled rows; expected values are
oracle.search_batch (L2) and ip_reference.py_search over ip_scores (inner product), compared bit for bit: status, item ids,
score bits, rows, per-round counters."""
import numpy as np
import pytest
import torch

import traverse_matrix as W
from gpu_util import bits, cuda, require_gpu, traversal_mode

pytestmark = pytest.mark.gpu

LPR = {64: 8, 128: 16, 256: 32, 512: 64}           # lanes per row: d / 8
DT = {"f16": 0, "bf16": 1, "f32": 2}
SC = {"l2": 0, "ip": 12}                           # NANN_SCORER_L2, kScorerIp
VIS = {"lds_bitmap": 0, "hbm_bitmap": 1, "lds_hash": 2, "lds_hash32": 3}
THREADS = {"lds_hash": 512, "lds_hash32": 1024, "lds_bitmap": 1024, "hbm_bitmap": 1024}
HASH_MODES = ("lds_hash", "lds_hash32")
MODES = HASH_MODES + ("lds_bitmap", "hbm_bitmap")

# (kernel, LPR, DT, VIS, SC, NT): every instantiation the dispatch of nann_l2_inst.hip, nann_ip_inst.hip and nann_lean_inst.hip
# can reach
KERNELS = tuple(
    (kernel, lpr, dt, VIS[mode], sc, THREADS[mode])
    for kernel, modes in (("k_search", MODES), ("k_search_lean", HASH_MODES))
    for sc in sorted(SC.values()) for dt in sorted(DT.values()) for lpr in sorted(LPR.values()) for mode in modes)

# the launches of one case: (what is special about the call, mode, lean)
LAUNCHES = tuple([("plain", m, int(m in HASH_MODES)) for m in MODES] +
                 [("phase_ticks", m, 0) for m in HASH_MODES] + [("per_request", m, 0) for m in HASH_MODES])

_TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
_CACHE = {}


def claimed(d, dtype, scorer, mode, lean):
    """the KERNELS entry a launch of this case in `mode` enters"""
    return ("k_search_lean" if lean else "k_search", LPR[d], DT[dtype], VIS[mode], SC[scorer], THREADS[mode])


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _device_index(d, dtype):
    from nann_amd import retrieval
    key = (d, dtype)
    if key not in _CACHE:
        g, q = W.graph(d)
        t = W.table(d, dtype)[0]
        rows = torch.as_tensor(t.view(np.int16)).cuda().view(torch.bfloat16) if dtype == "bf16" else torch.as_tensor(t).cuda()
        _CACHE[key] = (retrieval.Index(rows, g["item_ids"], g["nb_values"], g["nb_row_splits"], g["enter_points"]), cuda(q))
    return _CACHE[key]


def _launch(dix, sc, q, topn, mode, case, lean, **kw):
    """one retrieval.search under `mode`; asserts the plan and that it names an entry of KERNELS -> the five outputs on the host"""
    from nann_amd import retrieval
    with traversal_mode(mode):
        r = retrieval.search(dix, sc, q, topn, **kw)
        torch.cuda.synchronize()
    assert r.plan["visited_set"] == mode, (mode, r.plan)
    assert r.plan["threads"] == THREADS[mode], (mode, r.plan)
    assert r.plan["lean"] == lean, (mode, kw.keys(), r.plan)
    ran = ("k_search_lean" if r.plan["lean"] else "k_search", LPR[dix.d], DT[case[1]], VIS[r.plan["visited_set"]], SC[case[2]], r.plan["threads"])
    assert ran == claimed(case[0], case[1], case[2], mode, lean) and ran in KERNELS, ran
    if mode in HASH_MODES:
        assert r.reruns() == 0, "the set overflowed: the answers would be the fallback kernel's"
    return tuple(getattr(r, f).cpu().numpy() for f in ("status", "item_ids", "scores", "index", "counters"))


def _assert_equal(got, exp, what, k=None):
    """status, ids, score bits, rows, counters of `got` against the reference's; k: the request's own k in wider rows, zeros
    behind it.  A request the reference fails: its status and zeroed rows."""
    st, ids, sc, rows, ctr = got
    est, eids, esc, erows, ectr = exp
    k = ids.shape[1] if k is None else k
    assert ids.shape[0] == len(est) and eids.shape[1] == k, what
    assert (st == est).all(), (what, "status", st, est)
    ok = est == 0
    assert (rows[ok][:, :k] == erows[ok]).all(), (what, "rows")
    assert (ids[ok][:, :k] == eids[ok]).all(), (what, "item ids")
    assert (bits(sc[ok][:, :k]) == bits(esc[ok])).all(), (what, "score bits")
    assert (ctr[ok] == ectr[ok]).all(), (what, "counters")
    assert not ids[:, k:].any() and not bits(sc[:, k:]).any() and not rows[:, k:].any(), (what, "zeros behind k")
    assert not ids[~ok].any() and not bits(sc[~ok]).any() and not rows[~ok].any(), (what, "a failed request's rows")


@pytest.mark.parametrize("scorer", W.SCORERS)
@pytest.mark.parametrize("dtype", W.DTYPES)
@pytest.mark.parametrize("d", W.DIMS)
def test_every_instantiation_equals_the_reference(d, dtype, scorer):
    from nann_amd import ops
    case = (d, dtype, scorer)
    W.check_conditions(d, dtype, scorer)          # on the reference alone: a pass below means something
    exp = W.expected(d, dtype, scorer)
    per = W.expected_per_request(d, dtype, scorer)
    dix, q = _device_index(d, dtype)
    assert dix.d == d
    sc = ops.Scorer(scorer, d, _TORCH_DT[dtype])
    tq = W.level_topn_rows()
    for what, mode, lean in LAUNCHES:
        tag = (d, dtype, scorer, what, mode)
        if what == "per_request":
            got = _launch(dix, sc, q, tq, mode, case, lean)
            assert got[1].shape == (W.NQ, max(W.TOPN[5], W.TOPN_ODD[5]))
            for sel, topn, e in per:
                _assert_equal(tuple(o[sel] for o in got), e, tag + (tuple(topn),), k=topn[5])
        else:
            got = _launch(dix, sc, q, W.TOPN, mode, case, lean, want_phase_ticks=(what == "phase_ticks"))
            _assert_equal(got, exp, tag)
