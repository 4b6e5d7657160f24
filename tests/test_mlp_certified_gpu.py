"""-m gpu: the certified MLP form (NANN_MLP_CERTIFIED, csrc/nann_mlp6.h).  An f16 filter with a rigorous error bound
scores every candidate, and only the rows whose bound interval reaches a round's k-th largest lower bound are rescored
exactly.  Every answer -- ids, scores, internal indices, per-round counters -- must be bitwise what EXACT_F32 and the
CPU oracle return, for every weight set, and the filter must actually leave rows out."""
import numpy as np
import pytest
import torch

from gpu_util import bits, cuda, queries_for, require_gpu, synth_index, traversal_mode

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


def _run(dix, sc, q, topn, options=None):
    from nann_amd import retrieval
    r = retrieval.search(dix, sc, cuda(q), topn, options=options)
    torch.cuda.synchronize()
    got = (r.status.cpu().numpy(), r.item_ids.cpu().numpy(), r.scores.cpu().numpy(), r.index.cpu().numpy(),
           r.counters.cpu().numpy())
    return got, r


def _assert_same(got, exp):
    st, ids, scores, idx, ctr = got
    est, eids, escores, eidx, ectr = exp[:5]
    assert (st == est).all(), (st, est)
    ok = est == 0
    assert (idx[ok] == eidx[ok]).all()
    assert (ids[ok] == eids[ok]).all()
    assert (bits(scores[ok]) == bits(escores[ok])).all()
    assert (ctr[ok] == ectr[ok]).all()


class _Certified:
    """what the certified call reported beside its answers (read before the exact call reuses the workspace)"""
    def __init__(self, r):
        self.plan = r.plan
        self._refined = r.refined()

    def refined(self):
        return self._refined


def _both(dix, w, d, q, topn, options=None):
    """(certified, exact) results of the same call, and the certified call's plan and refined rows"""
    from nann_amd import ops
    cert, r = _run(dix, ops.Scorer("mlp", d, torch.float16, w, precision="certified"), q, topn, options)
    rc = _Certified(r)
    exact, _ = _run(dix, ops.Scorer("mlp", d, torch.float16, w, precision="exact"), q, topn, options)
    return cert, exact, rc


def _queries(oracle, g, n, seed):
    return np.stack([oracle.user_seq_mean(s) for s in queries_for(g, n, seed=seed)])


@pytest.mark.parametrize("d", [64, 128, 256])
def test_certified_equals_oracle_and_exact(oracle, d):
    from nann_amd import synth
    g, oix, dix = synth_index(20000, d, 32)
    w = synth.make_mlp_weights(d)
    q = _queries(oracle, g, 24, seed=41)
    topn = [32] * 5 + [20]
    cert, exact, r = _both(dix, w, d, q, topn)
    assert r.plan["phased"] == 1
    exp = oracle.search_batch(oix, oracle.Scorer("mlp", d, oracle.EMB_F16, w), q, topn, n_threads=16)
    assert (exp[0] == 0).mean() > 0.5
    _assert_same(cert, exp)
    _assert_same(cert, exact)


def test_certified_with_metric_weights_and_per_query_level_topn(oracle):
    """Per-query level_topn rows (wide ones included) on metric weights, against the oracle row group by row group."""
    from nann_amd import synth
    g, oix, dix = synth_index(120000, 64, 256, n_clusters=4, mode="knn")  # (wide beams find 400 new candidates a round)
    w = synth.make_mlp_weights_metric(64, g["item_embs"][::16])
    q = _queries(oracle, g, 12, seed=43)
    variants = [[100, 200, 400, 400, 400, 200], [128] * 5 + [200], [64, 96, 48, 160, 32, 50]]
    rows = np.asarray([variants[b % 3] for b in range(len(q))], np.int32)
    cert, exact, r = _both(dix, w, 64, q, rows)
    _assert_same(cert, exact)
    osc = oracle.Scorer("mlp", 64, oracle.EMB_F16, w)
    for v, topn in enumerate(variants):
        sel = np.arange(v, len(q), 3)
        exp = oracle.search_batch(oix, osc, q[sel], topn, n_threads=16)
        assert (exp[0] == 0).mean() > 0.5
        _assert_same(tuple(a[sel][:, :topn[5]] if a.ndim == 2 else a[sel] for a in cert), exp)
    # uniform wide level_topn through the same path
    topn = [100, 200, 400, 400, 400, 200]
    cert, exact, r = _both(dix, w, 64, q[:6], topn)
    _assert_same(cert, exact)
    _assert_same(cert, oracle.search_batch(oix, osc, q[:6], topn, n_threads=16))


@pytest.mark.parametrize("batch", [1, 64, 1024])
def test_certified_batches(oracle, batch):
    """Batches of 1, 64 and 1024 (one full chunk of the pipeline): bitwise the exact form's; a sample against the oracle."""
    from nann_amd import synth
    g, oix, dix = synth_index(20000, 128, 32)
    w = synth.make_mlp_weights_metric(128, g["item_embs"][::4])
    q = _queries(oracle, g, batch, seed=45)
    topn = [32] * 5 + [20]
    cert, exact, r = _both(dix, w, 128, q, topn)
    assert r.plan["phased"] == 1
    _assert_same(cert, exact)
    sample = np.unique(np.r_[0:min(batch, 16), max(0, batch - 8):batch])
    exp = oracle.search_batch(oix, oracle.Scorer("mlp", 128, oracle.EMB_F16, w), q[sample], topn, n_threads=16)
    _assert_same(tuple(a[sample] for a in cert), exp)


def test_weights_beyond_the_split_form_range(oracle):
    """|w| > 511: the split form refuses the weights, the certified form refines what its filter cannot bound."""
    from nann_amd import ops, synth
    g, oix, dix = synth_index(20000, 64, 32)
    w = dict(synth.make_mlp_weights(64))
    w["w2"] = np.asarray(w["w2"], np.float32) * 1.0e4
    w["w3"] = np.asarray(w["w3"], np.float32) / 1.0e4
    with pytest.raises(Exception, match="511"):
        ops.Scorer("mlp", 64, torch.float16, w, precision="split")
    q = _queries(oracle, g, 16, seed=47)
    topn = [32] * 5 + [20]
    cert, exact, r = _both(dix, w, 64, q, topn)
    _assert_same(cert, exact)
    _assert_same(cert, oracle.search_batch(oix, oracle.Scorer("mlp", 64, oracle.EMB_F16, w), q, topn, n_threads=16))


def test_tie_heavy_rows_and_quantised_weights(oracle):
    """Items that share their embedding (97 distinct rows for 20k items) score exactly equal, and quantised weights
    make many more near-equal: TopKV2's position rule must pick the same entries as the exact form."""
    from nann_amd import retrieval, synth
    from oracle import oracle as O
    g, _, _ = synth_index(20000, 64, 32)
    g2 = dict(g)
    g2["item_embs"] = np.ascontiguousarray(g["item_embs"][np.arange(len(g["item_embs"])) % 97])
    oix = O.Index(g2["item_embs"], g2["item_ids"], g2["nb_values"], g2["nb_row_splits"], g2["enter_points"])
    dix = retrieval.Index.from_dict(g2)
    w = {k: np.round(np.asarray(v, np.float32) * 8.0) / 8.0 for k, v in synth.make_mlp_weights(64).items()}
    q = _queries(oracle, g, 16, seed=49)
    topn = [32] * 5 + [20]
    cert, exact, r = _both(dix, w, 64, q, topn)
    _assert_same(cert, exact)
    _assert_same(cert, oracle.search_batch(oix, oracle.Scorer("mlp", 64, oracle.EMB_F16, w), q, topn, n_threads=16))
    ok = cert[0] == 0
    assert ok.any() and any(len(np.unique(bits(s))) < len(s) for s in cert[2][ok])  # ties reached the output


def test_activations_beyond_f16_refine_every_row(oracle):
    """Hidden activations past f16's range (x 2^7) overflow the filter: every row is rescored, and the answers are
    still the exact form's."""
    from nann_amd import synth
    g, oix, dix = synth_index(20000, 64, 32)
    w = dict(synth.make_mlp_weights(64))
    w["w1"] = np.asarray(w["w1"], np.float32) * 4096.0
    w["b1"] = np.asarray(w["b1"], np.float32) * 4096.0
    q = _queries(oracle, g, 16, seed=51)
    topn = [32] * 5 + [20]
    cert, exact, r = _both(dix, w, 64, q, topn)
    assert r.plan["phased"] == 1
    _assert_same(cert, exact)
    _assert_same(cert, oracle.search_batch(oix, oracle.Scorer("mlp", 64, oracle.EMB_F16, w), q, topn, n_threads=16))
    ok = cert[0] == 0
    assert ok.all()
    assert r.refined() == cert[4][:, 2, :].astype(np.int64).sum(0).tolist()


def test_the_filter_leaves_rows_out():
    """A random 100k-item graph with metric weights: fewer rows rescored than scored, answers the exact form's."""
    from nann_amd import synth
    g, _, dix = synth_index(100000, 128, 64)
    w = synth.make_mlp_weights_metric(128, g["item_embs"][::8])
    from oracle import oracle as O
    q = np.stack([O.user_seq_mean(s) for s in queries_for(g, 256, seed=53)])
    topn = [64] * 5 + [50]
    cert, exact, r = _both(dix, w, 128, q, topn)
    assert r.plan["phased"] == 1
    _assert_same(cert, exact)
    refined = np.asarray(r.refined())
    scored = cert[4][:, 2, :].astype(np.int64).sum(0)
    print("refined / scored per round:", (refined / np.maximum(scored, 1)).round(4).tolist())
    assert refined.sum() > 0 and refined.sum() < scored.sum()
    assert (refined <= scored).all()


def test_fallback_paths_equal_exact(oracle, tmp_path):
    """Where the pipeline of phases does not run, certified runs the exact kernels: forced HBM bitmap, no
    pre-projected table, the fused form asked for (taken as phased), the model form through precision.txt, and
    the evaluation traversal."""
    from nann_amd import ops, retrieval, synth
    g, oix, dix = synth_index(20000, 64, 32)
    w = synth.make_mlp_weights(64)
    q = _queries(oracle, g, 16, seed=55)
    topn = [32] * 5 + [20]
    with traversal_mode("hbm_bitmap"):
        cert, exact, r = _both(dix, w, 64, q, topn)
    assert r.plan["phased"] == 0 and r.refined() == [0] * 5
    _assert_same(cert, exact)
    cert, exact, r = _both(dix, w, 64, q, topn, options=retrieval.search_options(preprojection=False))
    assert r.plan["table"] == 0
    _assert_same(cert, exact)
    cert, exact, r = _both(dix, w, 64, q, topn, options=retrieval.search_options(mlp_form="fused"))
    assert r.plan["phased"] == 1
    _assert_same(cert, exact)
    exp = oracle.search_batch(oix, oracle.Scorer("mlp", 64, oracle.EMB_F16, w), q, topn, n_threads=16)
    _assert_same(cert, exp)
    # the model form: a weights directory whose precision.txt says certified
    seqs = queries_for(g, 16, seed=55)
    outs = {}
    for prec in ("certified", "exact"):
        ops.save_scorer_dir(str(tmp_path / prec), "mlp", w, precision=prec)
        m = ops.Model(str(tmp_path / prec), 64, 50)
        rm = retrieval.search_model(dix, m, cuda(seqs), topn)
        torch.cuda.synchronize()
        outs[prec] = (rm.status.cpu().numpy(), rm.item_ids.cpu().numpy(), rm.scores.cpu().numpy(),
                      rm.index.cpu().numpy(), rm.counters.cpu().numpy())
    _assert_same(outs["certified"], outs["exact"])
    # the evaluation traversal
    sc_c = ops.Scorer("mlp", 64, torch.float16, w, precision="certified")
    sc_e = ops.Scorer("mlp", 64, torch.float16, w, precision="exact")
    for cfg in [((3, 1, 1), (400, 200, 100), 200), ((2, 2, 1), (60, 40, 16), 30)]:
        rc = retrieval.search_eval(dix, sc_c, cuda(q), *cfg)
        re_ = retrieval.search_eval(dix, sc_e, cuda(q), *cfg)
        torch.cuda.synchronize()
        assert (rc.status.cpu().numpy() == re_.status.cpu().numpy()).all()
        assert (rc.n_out.cpu().numpy() == re_.n_out.cpu().numpy()).all()
        assert (rc.item_ids.cpu().numpy() == re_.item_ids.cpu().numpy()).all()
        assert (rc.index.cpu().numpy() == re_.index.cpu().numpy()).all()
        assert (bits(rc.scores.cpu().numpy()) == bits(re_.scores.cpu().numpy())).all()
