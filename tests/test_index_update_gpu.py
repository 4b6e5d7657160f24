"""-m gpu: rows of a built HNSW graph refreshed in place (nann_hnsw_update_device) and the rows a heal would mark
(nann_hnsw_orphan_bits).  The device arrays equal the model of tests/hnsw_update_model.py ENTRY FOR ENTRY at the cases of
tests/hnsw_update_cases.py (tests/test_index_update_model_cpu.py shows on the CPU that each case reaches its path); the model
starts from the DEVICE's base arrays, as the append and remove comparisons of tests/test_index_build_exact_gpu.py do, whose
helpers and device builds this file shares.  Then: the update against remove + append on the device alone; the edges; the
refusals before anything is written; serving from the result; the orphans and the heal of a removal."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_util import require_gpu

import hnsw_build_cases as HC
import hnsw_build_model as HM
import hnsw_update_cases as UC
import hnsw_update_model as UM
import test_index_build_exact_gpu as X

pytestmark = pytest.mark.gpu

_TINY = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _base(name):
    """the device build a case starts from, once: (state, its arrays on the host)"""
    if not UC.is_tiny(name):
        return X._built(UC.CASES[name][0])
    if "n64" not in _TINY:
        c = UC.base_case(name)
        st = X._build_raw(c, 64)
        st.update(ef_construction=HC.EF, keep_pruned=False, metric="l2")
        _TINY["n64"] = (st, X._arrays(st, c["levels"]))
    return _TINY["n64"]


def _bits(mask):
    n = len(mask)
    flags = np.zeros((n + 31) // 32 * 32, bool)
    flags[:n] = mask
    words = (flags.reshape(-1, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)
    return torch.as_tensor(words.view(np.int32)).cuda()


def _update_raw(u, st, rows, bits, fill=-7):
    """nann_hnsw_update_device into arrays filled with junk -> (status, the three arrays, stats)"""
    from nann_amd import _lib
    from nann_amd.ops import _ptr, _stream, _DT
    levels = np.ascontiguousarray(u["levels"], np.int32)
    n, m, n_up = len(levels), u["M"], HM.up_rows_of(levels)[1]
    out = {"adj0": torch.full((n, 2 * m), fill, dtype=torch.int32, device="cuda"), "up_row": torch.full((n,), fill, dtype=torch.int32, device="cuda"),
           "adj_up": torch.full((max(n_up, 1), m), fill, dtype=torch.int32, device="cuda")}
    stats = (C.c_int64 * 4)(-7, -7, -7, -7)
    torch.cuda.synchronize()
    rc = _lib.lib().nann_hnsw_update_device(_ptr(rows), n, u["d"], _DT[rows.dtype], m, HC.EF, 1 if u["keep_pruned"] else 0,
                                            _lib.SCORER_IP if u["metric"] == "ip" else _lib.SCORER_L2, C.c_void_p(levels.ctypes.data),
                                            _ptr(st["adj0"]), _ptr(st["up_row"]), _ptr(st["adj_up"]), _ptr(bits), _ptr(out["adj0"]),
                                            _ptr(out["up_row"]), _ptr(out["adj_up"]), stats, _stream())
    torch.cuda.synchronize()
    return rc, out, list(stats)


def _untouched(out, stats):
    return all(bool((o == -7).all()) for o in out.values()) and stats == [-7] * 4


# ---- the device equals the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(UC.CASES))
def test_update_equals_the_model(name):
    u = UC.case(name)
    st, base = _base(name)
    levels, mask = u["levels"], u["mask"]
    rows = X._device_rows(u["rows"])
    before = {k: st[k].clone() for k in ("adj0", "up_row", "adj_up")}
    rows_before = rows.clone()
    rc, out, stats = _update_raw(u, st, rows, _bits(mask))
    assert rc == 0
    for k in before:
        assert torch.equal(st[k], before[k]), f"the old {k} changed"
    assert torch.equal(rows.view(torch.int16), rows_before.view(torch.int16)), "item_embs changed"
    dev = X._arrays(out, levels)
    assert all((a != -7).all() for a in dev.values()), "an output entry was not written"
    model = UC.model_update(name, base["adj0"], base["adj_up"])
    for k in u["want"]:
        assert model["counters"][k] > 0, (name, k)
    X._same(f"update {name}", u, levels, dev, model)
    assert stats == model["stats"].tolist(), (stats, model["stats"].tolist())
    # structure: what an append, an export, a removal or the next update relies on
    HC.check_arrays(levels, dev["adj0"], dev["up_row"], dev["adj_up"] if len(dev["adj_up"]) else np.full((1, u["M"]), -1, np.int32), u["M"],
                    connected=False)
    assert ((dev["adj0"][mask] >= 0).sum(1) > 0).all(), "a re-inserted node with an empty level-0 row"
    if name.startswith("taller"):
        assert model["counters"]["taller_than_entry"] == 1
        assert (dev["adj_up"][dev["up_row"][10] + 1: dev["up_row"][10] + 3] == -1).all(), "node 10's rows on levels 2 and 3"
    if name == "all_but_one":
        assert stats[1] == 1 and model["n_batches"] == 63
    if name == "l2_m32_kp_cluster":
        assert stats[2] > 0
    if name == "relink":
        assert (dev["adj0"] != base["adj0"]).any()


# ---- the update against remove + append, on the device alone ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["l2_random", "ip_random"])
def test_update_equals_remove_then_append_on_the_device(name):
    """the refreshed rows appended at the tail of the compacted graph WITH THEIR LEVELS (append_hnsw_gpu would draw new ones, so
    the append goes through the C call, as _append_raw does): the same arrays under the permutation"""
    from nann_amd import index_build
    u = UC.case(name)
    st, _ = _base(name)
    mask, levels = u["mask"], np.asarray(u["levels"])
    marked = np.nonzero(mask)[0]
    new = X._device_rows(u["rows"])
    res = index_build.update_hnsw_gpu(st, marked, new[torch.as_tensor(marked).cuda()], want_export=False)
    assert set(res) == {"levels", "state", "stats"} and set(res["state"]) == set(st)
    assert torch.equal(res["state"]["item_embs"].view(torch.int16), new.view(torch.int16)) and res["state"]["item_embs"] is not st["item_embs"]
    assert torch.equal(st["item_embs"].view(torch.int16), X._device_rows(u["base"]["rows"]).view(torch.int16)), "the input state changed"
    perm, _ = UC.permutation(mask)
    removed = index_build.remove_hnsw_gpu(st, deny_bits=mask, want_export=False)
    assert list(removed["stats"][:3]) == list(res["stats"][:3]) and res["stats"][3] == len(marked)
    c2 = {"rows": u["rows"][perm], "levels": levels[perm], "n_old": int((~mask).sum()), "M": u["M"], "d": u["d"],
          "keep_pruned": u["keep_pruned"], "metric": u["metric"]}
    appended = X._arrays(X._append_raw(c2, removed["state"]), c2["levels"])
    adj0, adj_up, lv_new = UC.permuted_arrays(X._arrays(res["state"], levels), levels, mask)
    n_up = HM.up_rows_of(lv_new)[1]
    assert (adj0 == appended["adj0"]).all() and (adj_up[:n_up] == appended["adj_up"]).all()


# ---- edges and refusals -----------------------------------------------------------------------------------------------------------
def test_nothing_marked_gives_the_inputs_back():
    u = UC.case("l2_random")
    st, base = _base("l2_random")
    rc, out, stats = _update_raw(u, st, X._device_rows(u["rows"]), _bits(np.zeros(len(u["mask"]), bool)))
    assert rc == 0 and stats == [0, 0, 0, 0]
    dev = X._arrays(out, u["levels"])
    for k in dev:
        assert (dev[k] == base[k]).all(), k
    # bits at and beyond n in the last word are ignored (n = 600: bit 24 of word 18 is the first of them)
    dirty = _bits(np.zeros(len(u["mask"]), bool))
    dirty[-1] = -(1 << 24)
    rc, out, stats = _update_raw(u, st, X._device_rows(u["rows"]), dirty)
    assert rc == 0 and stats == [0, 0, 0, 0] and (X._arrays(out, u["levels"])["adj0"] == base["adj0"]).all()


def test_update_refuses_a_malformed_graph_before_it_writes():
    from nann_amd import _lib
    u = UC.case("l2_random")
    st, base = _base("l2_random")
    rows, bits = X._device_rows(u["rows"]), _bits(u["mask"])
    bad = dict(st, adj0=st["adj0"].clone())
    bad["adj0"][5, 0] = len(u["mask"])
    rc, out, stats = _update_raw(u, bad, rows, bits)
    assert rc == 7 and _untouched(out, stats)
    assert "outside [-1, n_old)" in _lib.last_error() and "nann_hnsw_update_device: malformed graph, node 5" in _lib.last_error()
    # every row marked: nothing stays to link to
    rc, out, stats = _update_raw(u, st, rows, _bits(np.ones(len(u["mask"]), bool)))
    assert rc == 7 and _untouched(out, stats) and "every row is marked" in _lib.last_error()
    # ... and the process goes on: the graph as it was built is accepted
    rc, out, stats = _update_raw(u, st, rows, bits)
    assert rc == 0 and stats[3] == u["mask"].sum()


def test_python_call_checks_its_rows():
    from nann_amd import index_build
    u = UC.case("l2_random")
    st, _ = _base("l2_random")
    new = X._device_rows(u["rows"])
    with pytest.raises(ValueError):
        index_build.update_hnsw_gpu(st, [3, 600], new[:2], want_export=False)
    with pytest.raises(ValueError):
        index_build.update_hnsw_gpu(st, [3, 3], new[:2], want_export=False)
    with pytest.raises(ValueError):
        index_build.update_hnsw_gpu(st, [3, 4], new[:2].float(), want_export=False)
    with pytest.raises(ValueError):
        index_build.update_hnsw_gpu(st, [3, 4], new[:3], want_export=False)
    with pytest.raises(RuntimeError):
        index_build.update_hnsw_gpu(st, np.arange(600), want_export=False)


# ---- serving from the result ------------------------------------------------------------------------------------------------------
def _first_hits(table, state, rows):
    """how many of `rows` the L2 traversal returns first for the row's own embedding, on the export of `state` over `table`.
    Beams of 16: among 600 rows in 16 clusters a step does not always find the 64 new candidates a beam of 64 asks for, and a
    top-k of fewer candidates than k fails the request, as in the reference."""
    from nann_amd import index_build, ops, retrieval
    ex = index_build.export_hnsw_gpu(state)
    n, d = table.shape
    dix = retrieval.Index(table, np.arange(n, dtype=np.int64), ex["nb_values"], ex["nb_row_splits"], ex["enter_points"])
    q = table[torch.as_tensor(rows).cuda()].float().contiguous()
    r = retrieval.search(dix, ops.Scorer("l2", d), q, [min(16, ex["enter_points"].numel()), 16, 16, 16, 16, 10])
    torch.cuda.synchronize()
    ok = r.status.cpu().numpy() == 0
    return int(((r.index.cpu().numpy()[:, 0] == rows) & ok).sum())


def test_updated_graph_serves_the_refreshed_rows():
    """the result through export_hnsw_gpu into retrieval.Index: an L2 search for each refreshed row's new embedding returns the
    row first at least as often as on the stale export over the new table.  Measured on the MI355X (l2_random, 158 rows, every
    request valid): stale graph 80, updated graph 158."""
    from nann_amd import index_build
    u = UC.case("l2_random")
    st, _ = _base("l2_random")
    marked = np.nonzero(u["mask"])[0]
    new = X._device_rows(u["rows"])
    res = index_build.update_hnsw_gpu(st, marked, new[torch.as_tensor(marked).cuda()])
    assert set(res) == {"levels", "enter_points", "nb_values", "nb_row_splits", "state", "stats"}
    stale = _first_hits(new, dict(st, item_embs=new), marked)
    updated = _first_hits(new, res["state"], marked)
    print(f"refreshed rows returned first for their own new embedding, of {len(marked)}: stale graph {stale}, updated graph {updated}")
    assert updated >= stale and updated > 0


# ---- orphans and the heal of a removal --------------------------------------------------------------------------------------------
def _orphans_raw(adj0, m):
    from nann_amd import _lib
    from nann_amd.ops import _ptr, _stream
    n = adj0.shape[0]
    words = (n + 31) // 32
    bits = torch.full((words,), -7, dtype=torch.int32, device="cuda")
    count = C.c_int64(-7)
    torch.cuda.synchronize()
    assert _lib.lib().nann_hnsw_orphan_bits(_ptr(adj0), n, m, _ptr(bits), C.byref(count), _stream()) == 0
    w = bits.cpu().numpy().view(np.uint32)
    flags = ((w[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(-1)
    assert not flags[n:].any(), "a bit at or beyond n"
    return np.nonzero(flags[:n])[0], count.value


def _removed():
    from nann_amd import index_build
    if "removed" not in _TINY:
        _TINY["removed"] = index_build.remove_hnsw_gpu(_base("l2_random")[0], deny_bits=HC.remove_mask("l2_random"), want_export=False)
    return _TINY["removed"]


@pytest.mark.parametrize("name", ["l2_f16_d64_m8", "ip_f16_d64_m8", "l2_f16_d64_m4", "removed"])
def test_orphan_bits_equal_the_numpy_set(name):
    from nann_amd import index_build
    st = _removed()["state"] if name == "removed" else X._built(name)[0]
    adj0 = st["adj0"].cpu().numpy()
    want = UM.orphans(adj0)
    got, count = _orphans_raw(st["adj0"], st["M"])
    print(f"orphans [{name}]: {len(want)} of {len(adj0)}")
    assert (got == want).all() if len(got) == len(want) else False, (got, want)
    assert count == len(want)
    rows = index_build.orphan_rows_gpu(st)
    assert rows.is_cuda and (rows.cpu().numpy() == want).all()
    if name == "removed":
        assert len(want) > 0, "a 25 % removal that leaves no orphan: the case does not test what it is here for"


def test_orphan_bits_skip_entries_outside_the_graph():
    st = X._built("l2_f16_d64_m8")[0]
    n = st["adj0"].shape[0]
    bad, clean = st["adj0"].clone(), st["adj0"].clone()
    bad[7, 0], bad[11, 1] = n + 5, -9
    clean[7, 0], clean[11, 1] = -1, -1
    got, count = _orphans_raw(bad, st["M"])
    want, count2 = _orphans_raw(clean, st["M"])
    assert (got == UM.orphans(bad.cpu().numpy())).all() and count == len(got)
    assert len(got) == len(want) and (got == want).all() and count == count2


def test_heal_of_a_removal_equals_the_model():
    """nann_hnsw_orphan_bits on the removal's output, then the update with those bits and the embeddings as they are"""
    from nann_amd import index_build
    c = HC.build_case("l2_f16_d64_m8")
    r = _removed()
    st = r["state"]
    kept = r["kept_rows"].cpu().numpy()
    rows = index_build.orphan_rows_gpu(st)
    healed = index_build.update_hnsw_gpu(st, rows, want_export=False)
    assert torch.equal(healed["state"]["item_embs"], st["item_embs"])
    levels = st["levels"]
    mask = np.zeros(len(levels), bool)
    mask[rows.cpu().numpy()] = True
    D = np.array(c["dist"], np.float32)[np.ix_(kept, kept)].tolist()
    before = X._arrays(st, levels)
    model = UM.update(D, c["d"], levels, before["adj0"], before["adj_up"], mask, c["M"], HC.EF, c["keep_pruned"], c["metric"])
    dev = X._arrays(healed["state"], levels)
    X._same("heal", dict(c, dist=D), levels, dev, model)
    assert list(healed["stats"]) == model["stats"].tolist()
    HC.check_arrays(levels, dev["adj0"], dev["up_row"], dev["adj_up"], c["M"], connected=False)
    assert ((dev["adj0"][mask] >= 0).sum(1) > 0).all(), "a listed node with an empty row"
    print(f"heal: {int(mask.sum())} orphans before, {len(UM.orphans(dev['adj0']))} after, stats {list(healed['stats'])}")
