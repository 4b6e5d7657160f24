"""-m gpu: the device paths of the shard merge and of TopKV2 beyond k = 1024 against the plain model of tests/merge_model.py,
on the cases of tests/merge_cases.py (which tests/test_merge_model_cpu.py shows to tell a wrong merge from a right one).

  k_merge_records   through nann_merge_records: `world` records packed on the host from `world` DIFFERENT shards' lists --
                    the shard of a position, the record stride, the id section's offset, the dynamic-LDS opt-in beyond
                    48 KB, k_out < k_in, one query, one shard; and through nann_sharded_topk (world == 1 and loopback
                    communicators, with and without a status), which must equal the seam over copies of its record
  k_merge_topk      every case, one of 17 408 keys (the selection re-reads its keys from memory) among them; the device,
                    the host function and the model agree
  k_topk_sort       nann_topk with k > 1024 (the whole-row sort in LDS), and the per-op evaluation schedule at
                    top_k_per_level beyond 1024, which runs on it

All of these select and carry; none computes.  Every comparison is exact: ids, and the bits of the scores."""
import ctypes as C

import numpy as np
import pytest
import torch

import merge_cases as MC
import merge_model as MM
from gpu_util import bits, cuda, queries_for, require_gpu, synth_index

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else a


def _up(a):
    return cuda(np.array(a))  # (a copy: the cases' arrays are shared and read-only)


def _same(got, exp):
    """(scores, ids) pairs, tensors or arrays: equal ids, equal score bits"""
    gs, gi, es, ei = _host(got[0]), _host(got[1]), _host(exp[0]), _host(exp[1])
    return gs.shape == es.shape and gi.shape == ei.shape and (gi == ei).all() and (bits(gs) == bits(es)).all()


# ---- nann_merge_records: distinct shards -------------------------------------------------------------------------------------------
SIDE_STREAM = {"a200:distinct", "a50:failed", "w1:special", "odd:ties", "e4097:failed", "lds_optin:failed", "q257:distinct"}


@pytest.mark.parametrize("name", MC.MERGE_CASES)
def test_merge_records_equals_the_model(name):
    from nann_amd import shard
    c = MC.merge_case(name)
    recv = _up(MC.records(name))
    if name in SIDE_STREAM:  # not the default stream
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = shard.merge_records_device(recv, c["b"], c["k_in"], c["k_out"])
        side.synchronize()
    else:
        got = shard.merge_records_device(recv, c["b"], c["k_in"], c["k_out"])
        torch.cuda.synchronize()
    assert _same(got, MC.expected(name))


def test_side_stream_sample_is_run():
    assert SIDE_STREAM <= set(MC.MERGE_CASES)


@pytest.mark.parametrize("name", ["a200:failed", "odd:distinct"])
def test_merge_records_off_the_page_grid_and_with_a_longer_stride(name):
    """recv 256-byte but not 4 KB aligned; then records that lie further apart than the padded record (record_bytes is the
    caller's stride, not a constant of the layout)"""
    from nann_amd import shard
    c = MC.merge_case(name)
    r = MC.records(name)
    world, rb = r.shape
    buf = torch.zeros(r.size + 8192, dtype=torch.uint8, device="cuda")
    off = (256 - buf.data_ptr()) % 4096
    recv = buf[off:off + r.size].view(world, rb)
    recv.copy_(torch.as_tensor(np.array(r)))
    assert recv.data_ptr() % 4096 == 256
    got = shard.merge_records_device(recv, c["b"], c["k_in"], c["k_out"])
    torch.cuda.synchronize()
    assert _same(got, MC.expected(name))
    wide = np.full((world, rb + 260), 0xa5, np.uint8)  # (a stride that is no multiple of 256 or 8 either)
    wide[:, :rb] = r
    assert _same(MM.merge_records(wide, world, c["b"], c["k_in"], c["k_out"], stride=rb + 260), MC.expected(name))
    got = shard.merge_records_device(cuda(wide), c["b"], c["k_in"], c["k_out"])
    torch.cuda.synchronize()
    assert _same(got, MC.expected(name))


# ---- nann_sharded_topk: the call the seam was cut from -------------------------------------------------------------------------------
@pytest.mark.parametrize("with_status", [True, False], ids=["status", "null_status"])
@pytest.mark.parametrize("name", [f"{s}:{c}" for s in ("w1", "w1_min", "a200", "a50", "odd", "lds_optin", "limit")
                                  for c in ("distinct", "failed")])
def test_sharded_topk_equals_the_model_and_the_seam(name, with_status):
    """world == 1 communicators and loopbacks (every slot gets this rank's record): shard 0's lists of the case through pack +
    exchange + merge, against the model over the repeated record and against nann_merge_records over copies of it"""
    from nann_amd import retrieval, shard
    c = MC.merge_case(name)
    world, b, k_in, k_out = c["world"], c["b"], c["k_in"], c["k_out"]
    sc, ids = c["scores"][:, 0], c["ids"][:, 0]
    st = None
    if with_status:
        st = np.zeros(b, np.int32) if c["status"] is None else c["status"][0]
    comm = shard.Comm(1, 0) if world == 1 else shard.Comm.loopback(world)
    ss = shard.ShardedSearch([0, 0, 0, 0, 0, k_out], world, 0, transport="rccl", comm=comm)
    local = retrieval.SearchResult(_up(ids), _up(sc), None, _up(st) if st is not None else None, None)
    mi, ms = ss.merge(local)
    torch.cuda.synchronize()
    recv = np.tile(MM.pack(sc, ids, st), (world, 1))
    exp = MM.merge_records(recv, world, b, k_in, k_out)
    if with_status and c["status"] is not None:
        assert np.isneginf(exp[0][st != 0]).all() and not exp[1][st != 0].any()  # failed here = failed on every slot
    assert _same((ms, mi), exp)
    seam = shard.merge_records_device(cuda(recv), b, k_in, k_out)
    torch.cuda.synchronize()
    assert _same(seam, (ms.cpu().numpy(), mi.cpu().numpy()))
    del ss, comm


# ---- nann_merge_topk ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.MERGE_TOPK_CASES)
def test_merge_topk_equals_the_model_and_the_host(name):
    from nann_amd import shard
    c = MC.merge_case(name)
    sc, ii = MC.merge_inputs(name)
    exp = MM.merge(sc, ii, c["k_out"])
    got = shard.merge_device(_up(sc), _up(ii), c["k_out"])
    torch.cuda.synchronize()
    assert _same(got, exp)
    hs, hi = shard.merge_host(sc, ii, c["k_out"])
    assert _same(got, (hs, hi))


# ---- nann_topk, k > 1024 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", MC.TOPK_CONTENTS)
@pytest.mark.parametrize("n,k", MC.TOPK_SHAPES)
def test_topk_beyond_1024_equals_the_model(n, k, content):
    from nann_amd import ops
    rows, vals, idx = MC.topk_case(n, k, content)
    ov, oi = ops.top_k(_up(rows), k)
    torch.cuda.synchronize()
    assert oi.dtype == torch.int32 and tuple(oi.shape) == (MC.TOPK_ROWS, k)
    assert (oi.cpu().numpy() == idx).all() and (bits(ov.cpu().numpy()) == bits(vals)).all()
    if content == "special":
        assert (bits(vals) == 0x80000000).any() and (bits(vals) == 0).any()  # a selected -0 leaves as -0, a +0 as +0


def test_topk_beyond_1024_refusals():
    from nann_amd import ops
    with pytest.raises(ops.UnimplementedError) as e:  # a row beyond what the sort holds in LDS
        ops.top_k(torch.zeros((1, 16385), device="cuda"), 1025)
    assert e.value.status == 102
    with pytest.raises(ops.InvalidArgumentError) as e:  # k == n + 1
        ops.top_k(torch.zeros((2, 1500), device="cuda"), 1501)
    assert e.value.status == 4
    torch.cuda.synchronize()


# ---- the evaluation schedule on it ----------------------------------------------------------------------------------------------------
EVAL_CFG = ((3, 1, 1), (2000, 1500, 1100), 1500)


def test_eval_schedule_beyond_1024_matches_oracle(oracle):
    """retrieval.search_eval_per_op with top_k_per_level beyond the selection kernel's 1024: its level-0 selections run on
    k_topk_sort.  Equal to the oracle's search_eval, and to the fused kernel, for every query the oracle accepts."""
    from types import SimpleNamespace
    from nann_amd import ops, retrieval
    g, oix, dix = synth_index(20000, 64, 32)
    osc, sc = oracle.Scorer("l2", 64, oracle.EMB_F16), ops.Scorer("l2", 64, torch.float16)
    qs = np.stack([oracle.user_seq_mean(s) for s in queries_for(g, 6, seed=9)])
    calls = []

    def top_k(values, k):
        calls.append((int(values.shape[-1]), int(k)))
        return ops.top_k(values, k)

    backend = SimpleNamespace(group_gather=ops.group_gather, bitmap_ref_difference=ops.bitmap_ref_difference,
                              blaze_score=ops.blaze_score, top_k=top_k, gather=ops.gather)
    fused = retrieval.search_eval(dix, sc, cuda(qs), *EVAL_CFG)
    torch.cuda.synchronize()
    n_ok = 0
    for b, q in enumerate(qs):
        rc, eids, esc, eidx = oracle.search_eval(oix, osc, q, *EVAL_CFG)
        assert int(fused.status[b]) == rc
        if rc:
            continue
        ids, s, idx = retrieval.search_eval_per_op(dix, sc, cuda(q), *EVAL_CFG, backend=backend)
        assert (idx.cpu().numpy() == eidx).all() and (ids.cpu().numpy() == eids).all()
        assert (bits(s.cpu().numpy()) == bits(esc)).all()
        n = len(eids)
        assert int(fused.n_out[b]) == n and (fused.index[b, :n].cpu().numpy() == eidx).all()
        assert (fused.item_ids[b, :n].cpu().numpy() == eids).all() and (bits(fused.scores[b, :n].cpu().numpy()) == bits(esc)).all()
        n_ok += 1
    assert n_ok >= 3
    assert any(k > 1024 for _, k in calls), calls  # the whole-row sort did run


# ---- refusals of nann_merge_records ---------------------------------------------------------------------------------------------------
def _call(recv, record_bytes, world, b, k_in, k_out, out_s, out_i):
    from nann_amd import _lib
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    return _lib.lib().nann_merge_records(p(recv), C.c_int64(record_bytes), C.c_int32(world), C.c_int64(b), C.c_int32(k_in),
                                         C.c_int32(k_out), p(out_s), p(out_i), None)


@pytest.mark.parametrize("what,status", [("null_recv", 7), ("null_out_scores", 7), ("null_out_ids", 7), ("k_out_1025", 102),
                                         ("keys_16385", 102), ("k_out_above_keys", 4), ("record_256_short", 103),
                                         ("record_4_short", 103), ("record_off_the_word_grid", 7), ("empty_batch", 0),
                                         ("k_out_0", 0)])
def test_merge_records_refusals_write_nothing(what, status):
    world, b, k_in, k_out = 8, 70, 200, 200
    rb = MM.record_bytes(b, k_in)
    assert rb % 256 == 0 and rb > b * k_in * 12
    if what == "keys_16385":
        world, k_in, rb = 5, 3277, MM.record_bytes(b, 3277)
    recv = torch.zeros(world * rb, dtype=torch.uint8, device="cuda")
    out_s = torch.full((b, 1025), -7.0, device="cuda")
    out_i = torch.full((b, 1025), -7, dtype=torch.int64, device="cuda")
    args = dict(recv=recv, record_bytes=rb, world=world, b=b, k_in=k_in, k_out=k_out, out_s=out_s, out_i=out_i)
    args.update({"null_recv": dict(recv=None), "null_out_scores": dict(out_s=None), "null_out_ids": dict(out_i=None),
                 "k_out_1025": dict(k_out=1025), "keys_16385": {}, "k_out_above_keys": dict(world=2, k_in=10, k_out=21),
                 "record_256_short": dict(record_bytes=rb - 256), "record_4_short": dict(record_bytes=b * k_in * 12),
                 "record_off_the_word_grid": dict(record_bytes=rb + 2), "empty_batch": dict(b=0), "k_out_0": dict(k_out=0)}[what])
    if what == "keys_16385":
        assert args["world"] * args["k_in"] == 16385
    assert _call(**args) == status
    torch.cuda.synchronize()
    assert (out_s == -7.0).all() and (out_i == -7).all()
