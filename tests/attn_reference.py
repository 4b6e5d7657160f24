"""Test-side reference of the attention + DNN scorer (model.py:189-233, model_util.py:70-97): the float64
numpy restatement every attention test is measured against, the inputs that put its softmax to work, and deliberately
wrong variants of it.  Shared by test_attn_model_cpu.py, test_attn_kernel_model.py and test_attn_shapes_gpu.py; nothing
under nann_amd/ imports it.

Why `sharpen`: synth.make_attn_weights draws glorot scales, and with inputs of size ~1/8 the attention logits of a row span
about 0.02 -- the softmax is a mean to within 1 %.  Multiplying wq2 and wk2 by g scales the logits by g^2; at g = 32 they
span 15-21 per row and the largest weight of a row averages 0.56-0.67, so an error in the exponential, the mask or the
order of the positions shows in the logit of the model."""
import numpy as np

LENGTHS = (1, 2, 16, 17, 31, 32, 33, 50, 63, 64)   # both sides of the 32-position tile, both ends of [1, 64]
GAINS = (1, 16, 32)                                # g = 64: the f32 oracle itself leaves 1e-6 (1.3e-6), so it is left out
N_USERS = 5


def np_model(w, u, rows, exp_slope=1.0, swap_positions=None, admit_pad_position=False):
    """The model in float64: u [L, 64], rows [n, d] -> logits [n].  The three keyword arguments make it WRONG on purpose
    (tests of what the suite can tell apart, nothing else): exp_slope scales the argument of the softmax's exponential,
    swap_positions=(i, j) exchanges the softmax weights of two positions, admit_pad_position lets one position of the
    kernels' layout padding (key 0, so logit 0; sequence row 0) into the softmax."""
    f = np.float64
    u = np.asarray(u, f)
    rows = np.asarray(rows, f)
    prelu = lambda x, a: np.maximum(0.0, x) + a * np.minimum(0.0, x)   # model_util.py:9-11
    q = prelu(rows @ w["wq1"].astype(f) + w["bq1"], w["aq"])            # :81
    q_ = q @ w["wq2"].astype(f) + w["bq2"]                              # :82
    k = prelu(u @ w["wk1"].astype(f) + w["bk1"], w["ak"])               # :84
    k_ = k @ w["wk2"].astype(f) + w["bk2"]                              # :85
    att = q_ @ k_.T / np.sqrt(q_.shape[-1])                             # :90-91
    if admit_pad_position:
        att = np.concatenate([att, np.zeros((len(att), 1))], axis=1)
        u = np.concatenate([u, np.zeros((1, u.shape[1]))], axis=0)
    att = np.exp(exp_slope * (att - att.max(-1, keepdims=True)))
    p = att / att.sum(-1, keepdims=True)                                # :93
    if swap_positions is not None:
        i, j = swap_positions
        p[:, [i, j]] = p[:, [j, i]]
    a = p @ u                                                           # :95 + model.py:206
    x = np.concatenate([a, rows], axis=-1)                              # model.py:211
    for i in range(3):                                                  # :213-216
        x = prelu((x @ w["w"][i].astype(f) + w["b"][i]) * w["bn_scale"][i] + w["bn_shift"][i], w["alpha"][i])
    return x @ w["w"][3].astype(f)                                      # :218-219


WRONG_VARIANTS = {"exp_slope": dict(exp_slope=1.01), "swap_positions": dict(swap_positions=(0, 1)),
                  "admit_pad_position": dict(admit_pad_position=True)}


def sharpen(w, g):
    """a copy of the weights with wq2 and wk2 multiplied by float32(g): the attention logits scale by g^2"""
    out = {k: ([np.array(a, copy=True) for a in v] if isinstance(v, list) else np.array(v, copy=True)) for k, v in w.items()}
    out["wq2"] = (out["wq2"] * np.float32(g)).astype(np.float32)
    out["wk2"] = (out["wk2"] * np.float32(g)).astype(np.float32)
    return out


def user_seqs(L, rng):
    """f16 [5, L, 64], each user drawn as standard_normal / 8: a full history; a zero tail of max(1, L // 5) rows; one zero
    row in the middle (L >= 3); every row zero; a tail of -0.0 halves.  (The model does not mask zero rows: they are
    positions of the softmax like any other, with the key of a zero input.)"""
    u = (rng.standard_normal((N_USERS, L, 64)) / 8).astype(np.float16)
    tail = max(1, L // 5)
    u[1, L - tail:] = 0
    if L >= 3:
        u[2, L // 2] = 0
    u[3] = 0
    u[4, L - tail:] = np.float16(-0.0)
    return u


# ---- the split-f16 form's key conversion and softmax, restated line by line in f32 (nann_attn_split.h: k_attn_prepare_split,
# exp_nonpos, the softmax block; nann_attn_proj.h carries the same softmax twice).  For what the header says about a key
# beyond f16's range -- NOT a second reference of the model.
KEY_LIMIT = 511.875   # |k| x 2^7 = 65520: where a round-to-nearest conversion to f16 stops being finite


def split_key(k):
    """f32 key components -> (hi, lo) f16 planes of k x 2^7, as k_attn_prepare_split converts them"""
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.asarray(k, np.float32) * np.float32(128.0)
        hi = v.astype(np.float16)                                       # round to nearest: inf from 65520 on
        lo = (v - hi.astype(np.float32)).astype(np.float16)             # v - inf = -inf
    return hi, lo


def exp_nonpos(x):
    """exp_nonpos of nann_attn_split.h on f32 values: clamp from below, 2^(x log2 e) with the product in two floats"""
    x = np.fmax(np.asarray(x, np.float32), np.float32(-128.0))          # fmaxf: a NaN operand is skipped
    log2e, log2e_lo = np.float32(1.44269502162933349609375), np.float32(1.92596299112661746e-08)
    t = x * log2e
    exact = x.astype(np.float64) * np.float64(log2e)                    # (the product of two f32 is exact in f64)
    e = (x.astype(np.float64) * np.float64(log2e_lo) + (exact - t).astype(np.float32)).astype(np.float32)
    r = np.exp2(t.astype(np.float64)).astype(np.float32)                # v_exp_f32; 2^-184 is 0 in f32
    return (r * np.float32(0.693147182464599609375) * e + r).astype(np.float32)


def split_softmax(att, L):
    """att f32[n, 64] (scaled attention logits in the kernels' 64-position layout) -> softmax weights f32[n, 64] as the split
    kernels compute them: padding masked to -inf, row maximum by fmaxf, exp_nonpos, one f32 sum, weights = e * (1 / sum)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.where(np.arange(64) < L, np.asarray(att, np.float32), np.float32(-np.inf)).astype(np.float32)
        mx = np.fmax.reduce(a, axis=-1, initial=np.float32(-np.inf), keepdims=True)
        w = exp_nonpos(a - mx)
        inv = np.float32(1.0) / w.sum(-1, keepdims=True, dtype=np.float32)
        return (w * inv).astype(np.float32)


def rows_as(x, dtype, O):
    """f32 [n, d] -> (rows as the oracle and the device take them, the oracle's dtype code, their exact values in f64)"""
    x = np.ascontiguousarray(x, np.float32)
    if dtype == "f16":
        rows = x.astype(np.float16)
        return rows, O.EMB_F16, rows.astype(np.float64)
    if dtype == "bf16":
        rows = (x.view(np.uint32) >> 16).astype(np.uint16)              # truncation is fine for a test input
        return rows, O.EMB_BF16, (rows.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return x, O.EMB_F32, x.astype(np.float64)


def rel_err(got, exp):
    """|got - exp| / max(1, |exp|), element by element: the scale of the project's 1e-5 contract"""
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    return np.abs(got - exp) / np.maximum(1.0, np.abs(exp))
