"""-m gpu: nann_user_seq_interests on the device against the numpy model of its contract (interests_model.model), bit for bit
on q, weights, n_interests and assign.  The calls go through the C ABI with outputs pre-filled with a canary and guard bands
around them.  A user's answer does not depend on its batch, so the contents of one shape -- random, all pad, one live row,
identical rows, two values, interleaved pads, planted clusters, the ends of the f16 range -- stand side by side as the users
of ONE call."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import interests_model as IM
from gpu_util import bits, require_gpu

pytestmark = pytest.mark.gpu
GUARD = 64
CANARY = 0x5A
F = np.float32
# (n_users, seq_len, d, n_vec, n_iter): the smallest; odd everything; d no multiple of 8; the serving shape; more rows than a
# wavefront with n_vec at the limit; more rows than threads; the largest LDS (63.3 of the 64 KB, past the 48 KB opt-in)
SHAPES = [(1, 1, 1, 1, 0), (3, 5, 3, 2, 1), (2, 7, 130, 3, 2), (4, 50, 128, 4, 8), (2, 65, 8, 16, 4), (2, 600, 16, 4, 3),
          (2, 200, 128, 8, 3)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


class _Out:
    """an output of n elements inside a canary-filled buffer with GUARD elements in front and behind"""

    def __init__(self, shape, dtype):
        self.shape = shape
        self.n = int(np.prod(shape))
        host = torch.empty(self.n + 2 * GUARD, dtype=dtype)
        host.view(torch.uint8).fill_(CANARY)
        self.canary = host[0].clone()
        self.buf = host.cuda()

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

    def get(self):
        h = self.buf.cpu()
        assert (h.view(torch.uint8)[:GUARD * h.element_size()] == CANARY).all(), "guard band written"
        assert (h.view(torch.uint8)[(GUARD + self.n) * h.element_size():] == CANARY).all(), "guard band written"
        return h[GUARD:GUARD + self.n].reshape(self.shape).numpy()


def _call(seq_bits, n_vec, n_iter, want=("weights", "n_interests", "assign"), shift=False, stream=None):
    """nann_user_seq_interests -> dict like interests_model.model's; outputs not in `want` are passed as NULL.  shift: the
    sequence starts 2 bytes behind a 16-byte boundary"""
    from nann_amd import _lib
    from nann_amd.ops import _stream
    L = _lib.lib()
    n_users, seq_len, d = seq_bits.shape
    flat = np.concatenate([np.zeros(8 + int(shift), np.uint16), seq_bits.reshape(-1)]).view(np.int16)
    dev = torch.as_tensor(flat).cuda()
    src = dev.data_ptr() + 2 * (8 + int(shift))
    assert dev.data_ptr() % 16 == 0 and src % 16 == (2 if shift else 0)
    outs = {"q": _Out((n_users, n_vec, d), torch.float32)}
    if "weights" in want:
        outs["weights"] = _Out((n_users, n_vec), torch.float32)
    if "n_interests" in want:
        outs["n_interests"] = _Out((n_users,), torch.int32)
    if "assign" in want:
        outs["assign"] = _Out((n_users, seq_len), torch.int32)
    p = lambda name: outs[name].ptr() if name in outs else None
    st = L.nann_user_seq_interests(C.c_void_p(src), n_users, seq_len, d, n_vec, n_iter, p("q"), p("weights"), p("n_interests"),
                                   p("assign"), C.c_void_p(stream.cuda_stream) if stream is not None else _stream())
    assert st == 0, _lib.last_error()
    torch.cuda.synchronize()
    return {name: o.get() for name, o in outs.items()}


def _same(got, exp, what=""):
    for name, g in got.items():
        e = exp[name]
        if name in ("q", "weights"):
            g, e = bits(g), bits(e)
        assert g.shape == e.shape and (g == e).all(), (what, name, np.argwhere(g != e)[:4].tolist())


def _h(x):
    return np.ascontiguousarray(np.asarray(x, np.float16)).view(np.uint16)


def _planted(rng, seq_len, d, n_vec):
    """n_c = min(n_vec, seq_len) centres 100 apart on the first axis, integer noise of at most 1 per column: every distance
    inside a cluster is at most 4 d <= 520, every distance between two at least 98^2.  -> (bits, label of every row)"""
    n_c = min(n_vec, seq_len)
    label = rng.permutation(np.arange(seq_len) % n_c)
    x = rng.integers(-1, 2, (seq_len, d)).astype(np.float32)
    x[:, 0] += 100.0 * (label + 1)
    return _h(x), label


def _contents(rng, n_users, seq_len, d, n_vec):
    """-> (bits u16[n, seq_len, d], what each user is, {user: planted labels})"""
    users, names, planted = [], [], {}
    for i in range(n_users):
        users.append(_h(rng.integers(-4, 5, (seq_len, d)) * 0.5)); names.append("random")
        users.append(np.where(rng.random((seq_len, d)) < 0.5, 0x8000, 0).astype(np.uint16)); names.append("all pad")
        one = np.zeros((seq_len, d), np.uint16)
        one[seq_len // 2] = _h(rng.integers(1, 5, d))
        users.append(one); names.append("one live row")
        users.append(np.repeat(_h(rng.integers(-4, 5, (1, d)) * 0.5 + 8), seq_len, axis=0)); names.append("identical rows")
        two = _h(rng.integers(-4, 5, (2, d)) * 0.5 + np.array([[8.0], [-8.0]]))
        users.append(two[np.arange(seq_len) % 2]); names.append("two values")
        pads = _h(rng.integers(-4, 5, (seq_len, d)) * 0.5)
        pads[i % 2::2] = 0x8000
        users.append(pads); names.append("pads interleaved")
        b, label = _planted(rng, seq_len, d, n_vec)
        planted[len(users)] = label
        users.append(b); names.append("planted")
        ends = rng.choice(np.array([0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x7BFF, 0xFBFF, 0x3C00, 0x0000, 0x8000], np.uint16),
                          (seq_len, d))
        users.append(ends); names.append("subnormals and +-65504")
    return np.stack(users), names, planted


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_content_of_a_shape_bitwise(shape):
    n_users, seq_len, d, n_vec, n_iter = shape
    rng = np.random.default_rng(list(shape))
    seq, names, planted = _contents(rng, n_users, seq_len, d, n_vec)
    exp = IM.model(seq, n_vec, n_iter)
    got = _call(seq, n_vec, n_iter)
    for u, name in enumerate(names):
        _same({k: v[u] for k, v in got.items()}, {k: v[u] for k, v in exp.items()}, (shape, u, name))
    for u, label in planted.items():  # the planted partition, up to the order of the slots
        a = got["assign"][u]
        n_c = min(n_vec, seq_len)
        assert got["n_interests"][u] == n_c and (a >= 0).all(), (shape, u)
        assert ((a[:, None] == a[None, :]) == (label[:, None] == label[None, :])).all(), (shape, u)
        assert (np.diff(got["weights"][u, :n_c]) <= 0).all()


def _small(seed=3, n_users=3, seq_len=9, d=5):
    rng = np.random.default_rng(seed)
    seq = _h(rng.integers(-4, 5, (n_users, seq_len, d)) * 0.5)
    seq[:, 2] = 0x8000
    return seq


def test_optional_outputs_as_null_in_every_combination():
    seq = _small()
    exp = IM.model(seq, 3, 2)
    for n in range(4):
        for want in itertools.combinations(("weights", "n_interests", "assign"), n):
            got = _call(seq, 3, 2, want=want)
            assert set(got) == {"q"} | set(want)
            _same(got, exp, want)


@pytest.mark.parametrize("shape", [(4, 50, 128, 4, 8), (2, 7, 130, 3, 2)], ids=["d128", "d130"])
def test_a_base_off_the_16_byte_grid_gives_the_same_bits(shape):
    n_users, seq_len, d, n_vec, n_iter = shape
    rng = np.random.default_rng(11)
    seq, _, _ = _contents(rng, 1, seq_len, d, n_vec)
    aligned, shifted = _call(seq, n_vec, n_iter), _call(seq, n_vec, n_iter, shift=True)
    _same(shifted, aligned, "shifted")
    _same(shifted, IM.model(seq, n_vec, n_iter), "model")


def test_a_non_default_stream():
    seq = _small(seed=4)
    s = torch.cuda.Stream()
    _same(_call(seq, 4, 3, stream=s), IM.model(seq, 4, 3), "stream")


def test_a_user_alone_equals_the_user_in_a_batch_of_five():
    seq = _small(seed=5, n_users=5, seq_len=40, d=16)
    whole = _call(seq, 4, 3)
    _same(whole, IM.model(seq, 4, 3), "batch")
    for u in (0, 3):
        alone = _call(seq[u:u + 1], 4, 3)
        _same({k: v[0] for k, v in alone.items()}, {k: v[u] for k, v in whole.items()}, u)


def test_ops_wrapper_and_one_vector_is_the_mean():
    from nann_amd import ops
    seq = _small(seed=6, n_users=4, seq_len=50, d=128)
    t = torch.as_tensor(seq.view(np.int16)).view(torch.float16).cuda()
    q, w, n, a = ops.user_seq_interests(t, 4, n_iter=8, want_assign=True)
    exp = IM.model(seq, 4, 8)
    _same(dict(q=q.cpu().numpy(), weights=w.cpu().numpy(), n_interests=n.cpu().numpy(), assign=a.cpu().numpy()), exp, "ops")
    assert len(ops.user_seq_interests(t, 4)) == 3
    mean = ops.user_seq_mean(t).cpu().numpy()
    for n_iter in (0, 1, 8):
        q1, w1, n1 = ops.user_seq_interests(t, 1, n_iter=n_iter)
        assert (bits(q1.cpu().numpy()[:, 0]) == bits(mean)).all() and (w1 == 1).all() and (n1 == 1).all()
