"""-m gpu: the device HNSW builder's arrays (nann_hnsw_build_device_metric, nann_hnsw_append_device_metric,
nann_hnsw_remove_device) equal the model of tests/hnsw_build_model.py ENTRY FOR ENTRY, at the smallest shapes that reach each
path (tests/hnsw_build_cases.py; tests/test_index_build_model_cpu.py shows on the CPU that each case reaches its path and that a
model wrong in one rule changes the arrays of some case).  No tolerance: no decision of these kernels depends on anything but
f32 values computed in one fixed order.  An append and a removal start the model from the DEVICE's base arrays, so a mismatch
of the base cannot cascade into them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from gpu_util import require_gpu

import hnsw_build_cases as HC
import hnsw_build_model as HM

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu

_BUILT = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _device_rows(rows):
    """an f16 array, or bf16 bit patterns -> the CUDA tensor of those bits"""
    if rows.dtype == np.uint16:
        return torch.as_tensor(np.ascontiguousarray(rows).view(np.int16)).view(torch.bfloat16).cuda()
    return torch.as_tensor(np.ascontiguousarray(rows)).cuda()


def _arrays(state, levels):
    """the three arrays of a state on the host; adj_up cut to the upper rows the levels imply (beyond them it is padding)"""
    n_up = HM.up_rows_of(levels)[1]
    return {"adj0": state["adj0"].cpu().numpy(), "up_row": state["up_row"].cpu().numpy(), "adj_up": state["adj_up"].cpu().numpy()[:n_up]}


def _with_dist(row, dist, node):
    return [(int(v), dist[node][int(v)]) for v in row if v >= 0]


def _same(what, c, levels, dev, model, old_ids=None):
    """device arrays == model arrays; on a mismatch, first the report: the earliest batch (the model's index) with a differing
    row -- the divergence lies in that batch or before it --, the node and the level, both rows with their distances to the node"""
    levels = np.asarray(levels)
    up_row, n_up = HM.up_rows_of(levels)
    want = {"adj0": model["adj0"], "up_row": model["up_row"], "adj_up": model["adj_up"][:n_up]}
    assert dev["up_row"].shape == want["up_row"].shape and (dev["up_row"] == want["up_row"]).all(), f"{what}: up_row differs from the prefix rule"
    assert dev["adj0"].shape == want["adj0"].shape and dev["adj_up"].shape == want["adj_up"].shape, f"{what}: shapes"
    owner = np.repeat(np.arange(len(levels)), levels - 1)
    differing = [(int(i), 0) for i in np.nonzero((dev["adj0"] != want["adj0"]).any(1))[0]]
    differing += [(int(owner[r]), int(r - up_row[owner[r]] + 1)) for r in np.nonzero((dev["adj_up"] != want["adj_up"]).any(1))[0]]
    if differing:
        written = lambda nl: model["touched"].get(nl, model["batch_of"][nl[0]])  # the model's last batch that wrote the row
        node, level = min(differing, key=lambda nl: (written(nl), nl[0], -nl[1]))
        ident = node if old_ids is None else int(old_ids[node])  # distances are indexed by the ids of the corpus
        row = (lambda a: a["adj0"][node] if level == 0 else a["adj_up"][up_row[node] + level - 1])
        as_old = (lambda r: r if old_ids is None else [int(old_ids[v]) if v >= 0 else -1 for v in r])
        pytest.fail(f"{what}: {len(differing)} rows differ; earliest: batch {written((node, level))} of the model's {model['n_batches']} (the last "
                    f"that wrote the row), node {node} (inserted by batch {model['batch_of'][node]}), level {level}\n"
                    f"  device (id, distance to the node): {_with_dist(as_old(row(dev)), c['dist'], ident)}\n"
                    f"  model  (id, distance to the node): {_with_dist(as_old(row(want)), c['dist'], ident)}")
    assert (dev["adj0"] == want["adj0"]).all() and (dev["adj_up"] == want["adj_up"]).all()


# ---- builds with drawn levels, through the Python builder ---------------------------------------------------------------------
def _built(name):
    """the device build of a case, once: (state, its arrays on the host)"""
    if name not in _BUILT:
        from nann_amd import index_build
        c = HC.build_case(name)
        st = index_build.build_hnsw_gpu(_device_rows(c["rows"]), c["M"], HC.EF, seed=c["seed"], keep_pruned=c["keep_pruned"],
                                        want_state=True, metric=c["metric"])["state"]
        assert (st["levels"] == c["levels"]).all()
        _BUILT[name] = (st, _arrays(st, c["levels"]))
    return _BUILT[name]


@pytest.mark.parametrize("name", list(HC.BUILDS))
def test_build_equals_the_model(name):
    c = HC.build_case(name)
    _same(f"build {name}", c, c["levels"], _built(name)[1], HC.model_build(name))


# ---- levels of the test's choosing, through the C calls -----------------------------------------------------------------------
def _build_raw(c, n):
    from nann_amd import _lib
    from nann_amd.ops import _check, _ptr, _stream, _DT
    rows = _device_rows(c["rows"][:n])
    levels = np.ascontiguousarray(c["levels"][:n], np.int32)
    m, n_up = c["M"], HM.up_rows_of(levels)[1]
    st = {"item_embs": rows, "adj0": torch.full((n, 2 * m), -7, dtype=torch.int32, device=rows.device),
          "up_row": torch.full((n,), -7, dtype=torch.int32, device=rows.device),
          "adj_up": torch.full((max(n_up, 1), m), -7, dtype=torch.int32, device=rows.device), "levels": levels, "M": m}
    torch.cuda.synchronize()
    _check(_lib.lib().nann_hnsw_build_device_metric(_ptr(rows), n, c["d"], _DT[rows.dtype], m, HC.EF, 1 if c["keep_pruned"] else 0,
                                                    _lib.SCORER_IP if c["metric"] == "ip" else _lib.SCORER_L2, C.c_void_p(levels.ctypes.data),
                                                    _ptr(st["adj0"]), _ptr(st["up_row"]), _ptr(st["adj_up"]), _stream()), "build")
    return st


def _append_raw(c, base):
    """the append of rows [n_old, n) onto grown copies of the base state's arrays, tails filled with junk"""
    from nann_amd import _lib
    from nann_amd.ops import _check, _ptr, _stream, _DT
    rows = _device_rows(c["rows"])
    levels = np.ascontiguousarray(c["levels"], np.int32)
    n, n_old, m = len(levels), c["n_old"], c["M"]
    n_up_old, n_up = HM.up_rows_of(levels[:n_old])[1], HM.up_rows_of(levels)[1]
    st = {"item_embs": rows, "adj0": torch.full((n, 2 * m), -7, dtype=torch.int32, device=rows.device),
          "up_row": torch.full((n,), -7, dtype=torch.int32, device=rows.device),
          "adj_up": torch.full((max(n_up, 1), m), -7, dtype=torch.int32, device=rows.device), "levels": levels, "M": m}
    st["adj0"][:n_old], st["up_row"][:n_old] = base["adj0"], base["up_row"]
    st["adj_up"][:n_up_old] = base["adj_up"][:n_up_old]
    torch.cuda.synchronize()
    _check(_lib.lib().nann_hnsw_append_device_metric(_ptr(rows), n_old, n - n_old, c["d"], _DT[rows.dtype], m, HC.EF,
                                                     1 if c["keep_pruned"] else 0, _lib.SCORER_IP if c["metric"] == "ip" else _lib.SCORER_L2,
                                                     C.c_void_p(levels.ctypes.data), _ptr(st["adj0"]), _ptr(st["up_row"]), _ptr(st["adj_up"]),
                                                     _stream()), "append")
    return st


@pytest.mark.parametrize("name", list(HC.TINY))
def test_tiny_graphs_equal_the_model(name):
    """n = 1, 2, 5, 9: batches of one and the quarter rule at its start; n = 64 with order[0] at 4 levels and every other node at
    2: upper rows for every node"""
    c = HC.tiny_case(name)
    n = len(c["levels"])
    dev = _arrays(_build_raw(c, n), c["levels"])
    model = HM.build(c["dist"], c["d"], c["levels"], c["M"], HC.EF, c["keep_pruned"], c["metric"])
    _same(f"tiny {name}", c, c["levels"], dev, model)
    if n == 1:
        assert (dev["adj0"] == -1).all() and (dev["adj_up"] == -1).all()


# ---- appends --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HC.APPENDS))
def test_append_equals_the_model(name):
    """200 rows onto a device-built graph of 400: batches of ceil(200 / 64) = 4"""
    from nann_amd import index_build
    c = HC.append_case(name)
    n_old = c["n_old"]
    rows = _device_rows(c["rows"])
    st0 = index_build.build_hnsw_gpu(rows[:n_old], c["M"], HC.EF, seed=c["seed"], want_state=True, metric=c["metric"])["state"]
    base = _arrays(st0, c["levels"][:n_old])
    st1 = index_build.append_hnsw_gpu(st0, rows[n_old:], seed=c["seed2"], want_export=False)["state"]
    assert (st1["levels"] == c["levels"]).all()
    model = HC.model_append(c, base["adj0"], base["adj_up"])
    assert model["counters"]["batches_gt1"] >= 10
    _same(f"append {name}", c, c["levels"], _arrays(st1, c["levels"]), model)
    # the base itself: the build of the first 400 rows
    sub = [r[:n_old] for r in c["dist"][:n_old]]
    _same(f"append {name}: its base", c, c["levels"][:n_old], base, HM.build(sub, c["d"], c["levels"][:n_old], c["M"], HC.EF, False, c["metric"]))


def test_append_of_a_node_taller_than_the_entry_point_equals_the_model():
    """one new node with more levels than the entry point, followed by ordinary nodes: the taller node goes in alone, its rows
    above the graph's top stay empty until a later node of that height links to it, and it is the entry point for the rest"""
    c = HC.taller_case()
    n_old = c["n_old"]
    st0 = _build_raw(c, n_old)
    base = _arrays(st0, c["levels"][:n_old])
    dev = _arrays(_append_raw(c, st0), c["levels"])
    model = HC.model_append(c, base["adj0"], base["adj_up"])
    assert model["counters"]["taller_than_entry"] == 1
    _same("append of a taller node", c, c["levels"], dev, model)
    tall = int(np.argmax(c["levels"]))
    top = dev["adj_up"][dev["up_row"][tall] + c["levels"][tall] - 2]
    assert (top == -1).all(), "the row above every other node's top"


# ---- removals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HC.REMOVES))
def test_remove_equals_the_model(name):
    from nann_amd import index_build
    base_name = HC.REMOVES[name][0]
    c = HC.build_case(base_name)
    st0, base = _built(base_name)
    mask = HC.remove_mask(name)
    r = index_build.remove_hnsw_gpu(st0, deny_bits=mask, want_export=False)
    model = HC.model_remove(name, base["adj0"], base["adj_up"])
    if name.endswith("cluster"):
        assert model["stats"][2] > 0, "no pool beyond 64: the case does not test what it is here for"
    assert (r["kept_rows"].cpu().numpy() == model["kept_rows"]).all() and (r["state"]["levels"] == model["levels"]).all()
    _same(f"remove {name}", c, model["levels"], _arrays(r["state"], model["levels"]), model, old_ids=model["kept_rows"])
    assert list(r["stats"]) == list(model["stats"]), (list(r["stats"]), list(model["stats"]))
