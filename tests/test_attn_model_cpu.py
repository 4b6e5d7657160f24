"""CPU: the oracle's restatement of the reference's scorer model (attention over the
50 x 64 user sequence + DNN 128-64-32-1, model.py:189-233, model_util.py:70-97) against an
independent float64 numpy restatement written from the same lines (tests/attn_reference.py).  PARITY
UNPINNED: TensorFlow is not in the image, so neither has been compared with a run of the frozen graph."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from attn_reference import GAINS, LENGTHS, WRONG_VARIANTS, np_model, rel_err, rows_as, sharpen, user_seqs

N_ROWS = 300


@pytest.mark.parametrize("d,dtype", [(64, "f16"), (128, "f32"), (64, "bf16")])
def test_attn_model_matches_numpy(oracle, d, dtype):
    from nann_amd import synth
    E, L, n = 64, 50, 300
    w = synth.make_attn_weights(d, E)
    rng = np.random.default_rng(d)
    u = (rng.standard_normal((L, E)) / 8).astype(np.float16).astype(np.float32)
    u[37:] = 0.0                                                        # zero-padded tail of the history
    x = (rng.standard_normal((n, d)) / 8).astype(np.float32)
    rows, code, xf = rows_as(x, dtype, oracle)
    m = oracle.AttnModel(d, E, L, code, w)
    rc, got = oracle.attn_score_rows(m, u, rows)
    exp = np_model(w, u.astype(np.float64), xf)
    assert rc == 0
    assert np.abs(got - exp).max() <= 1e-5 * max(1.0, np.abs(exp).max()), np.abs(got - exp).max()
    assert np.std(exp) > 1e-3                                           # the logits do depend on the row
    rc, _ = oracle.attn_score_rows(m, u, rows[:0])
    assert rc == 6                                                      # empty batch (blaze_xla_predictor.cc:259-263)


def _inputs(d, L):
    """(the five users f16[5, L, 64], rows f32[300, d]), seeded by (d, L)"""
    rng = np.random.default_rng(1000 * d + L)
    return user_seqs(L, rng), (rng.standard_normal((N_ROWS, d)) / 8).astype(np.float32)


@pytest.mark.parametrize("g", GAINS)
@pytest.mark.parametrize("L", LENGTHS)
def test_oracle_matches_float64_at_every_length_and_gain(oracle, L, g):
    """The condition on the inputs of every attention test: the f32 oracle sits a factor of 10 inside the 1e-5 contract,
    |oracle - float64| <= 1e-6 max(1, |s|) for every row, at L on both sides of the 32-position tile and at both ends of
    [1, 64], with the softmax near-uniform (g = 1) and peaked (g = 16, 32), d in {64, 128}, rows f16 / bf16 / f32, the five
    users of user_seqs.  Measured: 6.9e-7 at most over all of them (g = 1: 3.7e-7, g = 16: 3.6e-7, g = 32: 6.9e-7, at L = 64); no
    combination had to be dropped.  At g = 64 the oracle reaches 1.3e-6, which is why GAINS ends at 32."""
    from nann_amd import synth
    cases = []
    for d in (64, 128):
        w = sharpen(synth.make_attn_weights(d, 64), g)
        users, x = _inputs(d, L)
        for dtype in ("f16", "bf16", "f32"):
            rows, code, xf = rows_as(x, dtype, oracle)
            m = oracle.AttnModel(d, 64, L, code, w)
            cases += [(d, dtype, b, m, w, u, rows, xf) for b, u in enumerate(users)]

    def one(case):
        d, dtype, b, m, w, u, rows, xf = case
        rc, got = oracle.attn_score_rows(m, u.astype(np.float32), rows)
        assert rc == 0
        return rel_err(got, np_model(w, u, xf)).max()

    with ThreadPoolExecutor(8) as ex:  # (the oracle is a C call: the threads run side by side)
        errs = list(ex.map(one, cases))
    print("L = %d g = %d: oracle vs float64 %.3g" % (L, g, max(errs)))
    for case, err in zip(cases, errs):
        assert err <= 1e-6, (case[:3], err)


def test_sharpened_weights_peak_the_softmax():
    """what `sharpen` is for: at g = 1 a row's largest softmax weight is 1 / L to within 2 %, at g = 32 it averages over 0.4"""
    from nann_amd import synth
    f = np.float64
    for g, lo, hi in ((1, 0.0, 1.02 / 50), (32, 0.4, 1.0)):
        w = sharpen(synth.make_attn_weights(64, 64), g)
        users, x = _inputs(64, 50)
        prelu = lambda v, a: np.maximum(0.0, v) + a * np.minimum(0.0, v)
        q = prelu(x.astype(f) @ w["wq1"].astype(f) + w["bq1"], w["aq"]) @ w["wq2"].astype(f) + w["bq2"]
        k = prelu(users[0].astype(f) @ w["wk1"].astype(f) + w["bk1"], w["ak"]) @ w["wk2"].astype(f) + w["bk2"]
        att = q @ k.T / 16.0
        p = np.exp(att - att.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        assert lo < p.max(-1).mean() <= hi, (g, p.max(-1).mean())


@pytest.mark.parametrize("L", [L for L in LENGTHS if L >= 17])
def test_wrong_models_are_told_apart_in_the_sharp_regime(L):
    """Why the sharp regime exists.  For the full-history user and 300 rows, the largest difference between the float64 model
    and a deliberately wrong one, relative to max(1, |s|):
      g = 32, L >= 17: every variant differs by at least 1e-4, 10x the 1e-5 contract the kernels are held to.  Smallest
        measured over L in {17, 31, 32, 33, 50, 63, 64} and d in {64, 128}: exp_slope=1.01 5.4e-4, swap_positions=(0, 1)
        8.5e-3, admit_pad_position 1.05e-3.
      g = 1 (the weights as synth.make_attn_weights draws them): a 1 % error in the slope of exp moves no logit by 1e-5
        (largest measured 2.5e-6) -- a test at g = 1 alone cannot see it."""
    from nann_amd import synth
    for d in (64, 128):
        w1 = synth.make_attn_weights(d, 64)
        users, x = _inputs(d, L)
        u, xf = users[0].astype(np.float64), x.astype(np.float16).astype(np.float64)
        w32 = sharpen(w1, 32)
        right = np_model(w32, u, xf)
        for name, kw in WRONG_VARIANTS.items():
            diff = rel_err(np_model(w32, u, xf, **kw), right).max()
            print("L = %d d = %d g = 32 %s: %.3g" % (L, d, name, diff))
            assert diff >= 1e-4, (d, name, diff)
        blind = rel_err(np_model(w1, u, xf, exp_slope=1.01), np_model(w1, u, xf)).max()
        print("L = %d d = %d g = 1 exp_slope: %.3g" % (L, d, blind))
        assert blind < 1e-5, (d, blind)


def test_split_form_drops_a_position_whose_key_leaves_f16():
    """What include/nann_hip.h says about the split form's range, on the restatement of its lines in attn_reference.py: a key
    component with |k| >= 511.875 converts to hi = +-inf, lo = -+inf, its position's attention logit is NaN, and the softmax
    gives that position weight 0 and renormalises the rest -- finite weights, nothing for an isfinite check to catch; the
    weights are NaN only when every live position overflows."""
    from attn_reference import KEY_LIMIT, exp_nonpos, split_key, split_softmax
    below = np.nextafter(np.float32(KEY_LIMIT), np.float32(0))
    for sign in (1.0, -1.0):
        hi, lo = split_key(np.float32([sign * below, sign * KEY_LIMIT, sign * 3000.0]))
        assert np.isfinite(hi[0]) and abs(float(hi[0])) == 65504.0 and np.isfinite(lo[0])
        assert np.isinf(hi[1:]).all() and np.isinf(lo[1:]).all() and (np.sign(hi[1:]) == sign).all() and (np.sign(lo[1:]) == -sign).all()
        q = np.float32(0.37)                                            # hi.q + lo.q, the MFMA's f32 sum of products
        with np.errstate(invalid="ignore"):
            assert np.isnan(hi[1].astype(np.float32) * q + lo[1].astype(np.float32) * q)
    rng = np.random.default_rng(5)
    L, n = 33, 200
    att = (rng.standard_normal((n, 64)) * 6).astype(np.float32)         # logits spanning ~25 per row, as at g = 32
    live = att[:, :L].astype(np.float64)
    p = np.exp(live - live.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    w = split_softmax(att, L)
    assert (w[:, L:] == 0).all() and np.abs(w[:, :L] - p).max() <= 1e-6  # the restatement is a softmax: exp_nonpos is exp
    assert np.abs(exp_nonpos(np.float32([0.0, -1.0, -30.0])) - np.exp([0.0, -1.0, -30.0])).max() <= 2e-7
    for l0 in (5, 32):                                                  # one NaN logit, in either position tile
        bad = att.copy()
        bad[:, l0] = np.nan
        w = split_softmax(bad, L)
        keep = [l for l in range(L) if l != l0]
        pk = np.exp(live[:, keep] - live[:, keep].max(-1, keepdims=True))
        pk /= pk.sum(-1, keepdims=True)
        assert np.isfinite(w).all() and (w[:, l0] == 0).all()
        assert np.abs(w[:, keep] - pk).max() <= 1e-6                    # the softmax of the sequence without that position
    bad = att.copy()
    bad[:, :L] = np.nan                                                 # every live position: sum 0, 1 / 0 = inf, 0 * inf
    assert np.isnan(split_softmax(bad, L)).all()
