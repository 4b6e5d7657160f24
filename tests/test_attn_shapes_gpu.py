"""-m gpu: the attention + DNN scorer at the sequence lengths and in the softmax regime no other test
reaches, through every kernel family that runs it: the stand-alone scorer in its f32 and split-f16 forms with their two
per-user prepare kernels, nann_model_forward, the fused traversal (on embedding rows, on the pre-projected table, with
everything resident in LDS), the exhaustive scan, the candidate-list scorer and the evaluation traversal.

Sequence lengths: the header promises seq_len in [1, 64]; every other attention test runs L = 50.  Here L = 64 (no layout
padding at all), 33 and 32 / 17 / 16 (one position into the second 32-position tile; a whole tile masked), 63 and 1.
Softmax regime: with synth.make_attn_weights as drawn the softmax is a mean to within 1 % and a 1 % error in exp moves no
logit by 1e-5; attn_reference.sharpen(w, 32) peaks it (test_attn_model_cpu.py measures both).

The reference everywhere is the CPU oracle (oracle_attn_score_rows), itself within 1e-6 of the float64 model on these
inputs (test_attn_model_cpu.py); the tolerance everywhere is the project's own, |got - oracle| <= 1e-5 max(1, |oracle|),
for EVERY score.  Bit-identity is asserted where include/nann_hip.h promises it.  Measured on an MI355X, the largest error
of any score of this file: split-f16 6.3e-7, f32 form 5.7e-7 (both at g = 32); split against exact 5.4e-7."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from attn_reference import rel_err, rows_as, sharpen, user_seqs
from gpu_util import bits, cuda, require_gpu, synth_index, tolerant_parity

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu
RTOL = 1e-5
N_TABLE, N_SCORE = 1000, 300
TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()


@pytest.fixture(scope="module")
def model_dirs(tmp_path_factory):
    """path of the weights directory of (d, g, precision), written once"""
    root = tmp_path_factory.mktemp("attn_shapes")

    def get(d, g, precision):
        from nann_amd import ops
        path = str(root / ("attn_%d_%d_%s" % (d, g, precision)))
        if not os.path.isdir(path):
            ops.save_scorer_dir(path, "attention", _weights(d, g), precision=precision)
        return path
    return get


# ---- shared inputs and references (computed once, never changed) -------------------------------------------------------
def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _weights(d, g):
    from nann_amd import synth
    return _cached(("w", d, g), lambda: sharpen(synth.make_attn_weights(d, 64), g))


def _users(L):
    return _cached(("users", L), lambda: user_seqs(L, np.random.default_rng(900 + L)))


def _table(d, dtype):
    """(host rows, oracle dtype code, device rows, indices i32[300] into them)"""
    def make():
        from oracle import oracle as O
        rng = np.random.default_rng(7 * d)
        host, code, _ = rows_as((rng.standard_normal((N_TABLE, d)) / 8).astype(np.float32), dtype, O)
        dev = cuda(host.view(np.int16)).view(torch.bfloat16) if dtype == "bf16" else cuda(host)
        return host, code, dev, rng.integers(0, N_TABLE, size=N_SCORE).astype(np.int32)
    return _cached(("table", d, dtype), make)


def _oracle_rows(am, seqs, rows_per_user, threads=16):
    """oracle logits, user by user: seqs f16[B, L, 64], rows_per_user: B arrays of rows -> list of f32 arrays"""
    from oracle import oracle as O

    def one(args):
        u, rows = args
        if len(rows) == 0:
            return np.zeros(0, np.float32)
        rc, s = O.attn_score_rows(am, u.astype(np.float32), rows)
        assert rc == 0
        return s
    with ThreadPoolExecutor(threads) as ex:  # (the oracle is a C call: the threads run side by side)
        return list(ex.map(one, list(zip(seqs, rows_per_user))))


def _oracle_model(d, dtype_code, g, L):
    from oracle import oracle as O
    return _cached(("am", d, dtype_code, g, L), lambda: O.AttnModel(d, 64, L, dtype_code, _weights(d, g)))


def _reference(d, dtype, g, L):
    """oracle logits f32[5, 300] of the five users on the table's indexed rows"""
    def make():
        host, code, _, idx = _table(d, dtype)
        users = _users(L)
        return np.stack(_oracle_rows(_oracle_model(d, code, g, L), users, [host[idx]] * len(users)))
    return _cached(("ref", d, dtype, g, L), make)


def _within(got, exp):
    err = rel_err(got, exp)
    return float(err.max()) if err.size else 0.0


# ---- 3a. the stand-alone scorer: nann_attn_prepare + nann_attn_score ---------------------------------------------------
LENGTHS_GPU = [1, 16, 17, 32, 33, 50, 63, 64]


def _standalone(precision, d, dtype, g, L):
    """one prepare call for the five users, then per user: 300 rows through `indices`, a 31-row and a 1-row pass, each also
    pre-gathered -> dict(kt, upad, full f32[5, 300], p31 f32[5, 31], p1 f32[5, 1], pregathered_same bool)"""
    def make():
        from nann_amd import ops
        host, code, dev, idx = _table(d, dtype)
        users = _users(L)
        sc = ops.AttnScorer(d, L, TDT[dtype], _weights(d, g), precision=precision)
        kt, upad = sc.prepare(cuda(users))
        didx = torch.as_tensor(idx).long().cuda()
        out = {"full": [], "p31": [], "p1": [], "same": True}
        for b in range(len(users)):
            for name, n in (("full", N_SCORE), ("p31", 31), ("p1", 1)):
                got = sc.score(kt[b], upad[b], table=dev, indices=idx[:n]).cpu().numpy()
                pre = sc.score(kt[b], upad[b], item_emb=dev[didx[:n]]).cpu().numpy()
                out["same"] = out["same"] and bool((bits(got) == bits(pre)).all())
                out[name].append(got)
        torch.cuda.synchronize()
        res = {k: (np.stack(v) if isinstance(v, list) else v) for k, v in out.items()}
        res["kt"], res["upad"] = kt.cpu().numpy(), upad.cpu().numpy()
        return res
    return _cached(("standalone", precision, d, dtype, g, L), make)


@pytest.mark.parametrize("L", LENGTHS_GPU)
@pytest.mark.parametrize("g", [1, 32])
@pytest.mark.parametrize("d,dtype", [(64, "f16"), (128, "bf16")])
@pytest.mark.parametrize("precision", ["exact", "split"])
def test_standalone_scorer(oracle, precision, d, dtype, g, L):
    """Five users through ONE prepare call (the user * L * 64 stride of both prepare kernels), 300 table rows through
    `indices` plus a 31-row and a 1-row pass: every logit within 1e-5 of the oracle, the pre-gathered form the same bits.
    Exact form: the header's "per-user projection bit for bit" -- kt[:, :L] is oracle_attn_prepare transposed, bitwise,
    kt[:, L:] and upad[L:] are zero, upad[:L] is the sequence.
    Measured on an MI355X, largest |got - oracle| / max(1, |oracle|) over the cases of this test: exact 3.3e-7 at g = 1 and
    5.7e-7 at g = 32; split 4.5e-7 at g = 1 and 6.3e-7 at g = 32 (the number the split form's 22-bit operands left open:
    |att| reaches ~25 there, and it stays a factor of 15 inside the contract)."""
    exp = _reference(d, dtype, g, L)
    r = _standalone(precision, d, dtype, g, L)
    errs = {n: _within(r[n], exp[:, :r[n].shape[1]]) for n in ("full", "p31", "p1")}
    print("standalone %s d=%d %s g=%d L=%d: max err %s" % (precision, d, dtype, g, L, errs))
    assert np.isfinite(r["full"]).all()
    for n, e in errs.items():
        assert e <= RTOL, (n, e)
    assert (bits(r["p31"]) == bits(r["full"][:, :31])).all() and (bits(r["p1"]) == bits(r["full"][:, :1])).all()
    assert r["same"], "pre-gathered rows score differently from gathered ones"
    if precision == "exact":
        users = _users(L)
        am = _oracle_model(d, _table(d, dtype)[1], g, L)
        for b, u in enumerate(users):
            rc, kproj = oracle.attn_prepare(am, u.astype(np.float32))
            assert rc == 0
            assert (bits(r["kt"][b][:, :L]) == bits(kproj.T)).all(), b
            assert (bits(r["kt"][b][:, L:]) == 0).all() and (bits(r["upad"][b][L:]) == 0).all(), b
            assert (bits(r["upad"][b][:L]) == bits(u.astype(np.float32))).all(), b


@pytest.mark.parametrize("L", LENGTHS_GPU)
@pytest.mark.parametrize("g", [1, 32])
@pytest.mark.parametrize("d,dtype", [(64, "f16"), (128, "bf16")])
def test_standalone_scorer_between_precisions(d, dtype, g, L):
    """the split-f16 form against the f32 form on the device, same users, same rows: within 1e-5"""
    a, b = _standalone("split", d, dtype, g, L)["full"], _standalone("exact", d, dtype, g, L)["full"]
    e = _within(a, b)
    print("split vs exact d=%d %s g=%d L=%d: %.3g" % (d, dtype, g, L, e))
    assert e <= RTOL, e


# ---- 3b. the range check on seq_len ------------------------------------------------------------------------------------
def test_seq_len_range_check(model_dirs):
    """seq_len 0, -1 and 65 -> NANN_ERR_UNSUPPORTED (102) from nann_attn_scorer_create and from nann_model_load of an
    attention directory; 64 is accepted by both"""
    from nann_amd import ops
    w, path = _weights(64, 1), model_dirs(64, 1, "split")
    for bad in (0, -1, 65):
        for precision in ("exact", "split"):
            with pytest.raises(ops.NannError) as e:
                ops.AttnScorer(64, bad, torch.float16, w, precision=precision)
            assert e.value.status == 102 and "seq_len" in str(e.value), (bad, precision)
        with pytest.raises(ops.NannError) as e:
            ops.Model(path, 64, bad)
        assert e.value.status == 102 and "seq_len" in str(e.value), bad
    assert ops.AttnScorer(64, 64, torch.float16, w, precision="split").handle.value
    assert ops.AttnScorer(64, 1, torch.float16, w, precision="exact").handle.value
    assert ops.Model(path, 64, 64).kind == "attention"


# ---- 3c. nann_model_forward: weights directory and frozen GraphDef -----------------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("L", [17, 64])
def test_model_forward_directory_and_frozen_graphdef(tmp_path, model_dirs, d, L):
    """nann_model_forward at g = 32 for the five users, the model loaded from a weights directory and from a frozen GraphDef
    written for seq_len = L: the two bit-identical, both within 1e-5 of the oracle, in both precisions"""
    from nann_amd import frozen_graph, ops
    g = 32
    host, code, dev, idx = _table(d, "f16")
    exp = _reference(d, "f16", g, L)
    users = _users(L)
    rows = dev[torch.as_tensor(idx).long().cuda()]
    pb = tmp_path / "frozen_graph.pb"
    frozen_graph.write_attention_graph(str(pb), _weights(d, g), seq_len=L)
    for prec in ("split", "exact"):
        (tmp_path / "frozen_graph.pb.precision").write_text(prec + "\n")
        m_pb, m_dir = ops.Model(str(pb), d, L), ops.Model(model_dirs(d, g, prec), d, L)
        assert m_pb.kind == "attention" and m_dir.kind == "attention"
        for b, u in enumerate(users):
            a = m_pb.forward(cuda(u)[None], rows).cpu().numpy().ravel()
            c = m_dir.forward(cuda(u)[None], rows).cpu().numpy().ravel()
            assert (bits(a) == bits(c)).all(), (prec, b)
            e = _within(a, exp[b])
            print("model_forward %s d=%d L=%d user %d: %.3g" % (prec, d, L, b, e))
            assert e <= RTOL, (prec, b, e)


# ---- 3d. the fused traversal: nann_search_model_opt --------------------------------------------------------------------
TOPN = [32] * 5 + [20]
NQ = 16


def _traversal_case(L, g):
    """(seqs f16[16, L, 64], the oracle's traversal: status, rows, scores) on synth_index(20000, 64, 32)"""
    def make():
        from nann_amd import synth
        from oracle import oracle as O
        gr, oix, _ = synth_index(20000, 64, 32)
        seqs = synth.make_queries(gr["item_embs"], gr["assign"], NQ, seq_len=L, min_len=min(7, L), seed=17 + L)
        am = _oracle_model(64, O.EMB_F16, g, L)
        osc = O.Scorer("attention", 64, O.EMB_F16, attn_model=am)
        est, _, esc, eidx, _ = O.search_batch(oix, osc, seqs.astype(np.float32).reshape(NQ, -1), TOPN, n_threads=16)
        return seqs, est, eidx, esc
    return _cached(("traversal", L, g), make)


def _rescored(am, host, seqs, idx, scores, ok):
    """the check with no exemptions: the oracle's logit of every row the device returned, for the users in `ok` ->
    the largest |device score - oracle| / max(1, |oracle|)"""
    users = list(np.nonzero(ok)[0])
    own = _oracle_rows(am, [seqs[b] for b in users], [host[idx[b]] for b in users])
    return max([_within(scores[b], o) for b, o in zip(users, own)] + [0.0])


@pytest.mark.parametrize("mode", ["auto", "lds_bitmap"])
@pytest.mark.parametrize("preprojection", [1, 0])
@pytest.mark.parametrize("precision", ["split", "exact"])
@pytest.mark.parametrize("L,g", [(64, 32), (33, 32), (1, 1), (50, 32)])
def test_fused_traversal(oracle, model_dirs, L, g, precision, preprojection, mode):
    """nann_search_model_opt with the attention model, 16 users: precision x preprojection x traversal mode reach the
    resident, the table and the row kernels of both forms.  Two checks per call: the tie-aware comparison with the
    oracle's traversal (thresholds of test_search_model_attention_split_f16: >= 80 % of the lists exact, diverged no more
    than 2 in 40, so at most 1 of 16), and, with no exemption, every score the device returned within 1e-5 of the oracle's
    logit of that row (which way a near-tie fell does not matter to it)."""
    from nann_amd import ops, retrieval
    gr, oix, dix = synth_index(20000, 64, 32)
    seqs, est, eidx, esc = _traversal_case(L, g)
    m = ops.Model(model_dirs(64, g, precision), 64, L)
    opt = retrieval.search_options(traversal=mode, preprojection=bool(preprojection))
    r = retrieval.search_model(dix, m, cuda(seqs), TOPN, options=opt)
    torch.cuda.synchronize()
    st, idx, sc = r.status.cpu().numpy(), r.index.cpu().numpy(), r.scores.cpu().numpy()
    ok = (est == 0) & (st == 0)
    kinds = [tolerant_parity(idx[b], sc[b], eidx[b], esc[b]) for b in np.nonzero(ok)[0]]
    worst = _rescored(_oracle_model(64, oracle.EMB_F16, g, L), gr["item_embs"], seqs, idx, sc, st == 0)
    print("traversal L=%d g=%d %s pp=%d %s plan=%s: status ok %d/%d, %s, rescored max err %.3g"
          % (L, g, precision, preprojection, mode, r.plan, int(ok.sum()), NQ, kinds, worst))
    # the kernel this case is meant to reach did run: the table kernels iff preprojection, the visited set that was asked
    # for, and in auto mode the 16K-slot hash set -- with split precision and the table, the plan of the resident kernel
    assert r.plan["table"] == bool(preprojection), r.plan
    assert r.plan["visited_set"] == ("lds_hash" if mode == "auto" else mode), r.plan
    assert (st == est).sum() >= NQ - 1 and ok.mean() > 0.5, (st, est)
    assert kinds.count("exact") >= 0.8 * len(kinds) and kinds.count("diverged") <= 1, kinds
    assert worst <= RTOL, worst


# ---- 3e. the exhaustive scan and the candidate lists under the model ---------------------------------------------------
K_FLAT, N_FLAT, LIST_LEN = 64, 4096, 300


def _flat_case(L, g):
    """(the five users, candidate lists i32[5, 300] with one duplicate each, oracle logits f32[5, 4096] of every row)"""
    def make():
        from oracle import oracle as O
        gr, _, _ = synth_index(N_FLAT, 64, 32)
        users = _users(L)
        rng = np.random.default_rng(31 * L + g)
        lists = np.stack([rng.choice(N_FLAT, size=LIST_LEN, replace=False) for _ in users]).astype(np.int32)
        lists[:, 200] = lists[:, 17]   # one row listed twice: scored twice, a tie that goes to the lower position
        am = _oracle_model(64, O.EMB_F16, g, L)
        chunks = np.array_split(np.arange(N_FLAT), 4)
        parts = _oracle_rows(am, [u for u in users for _ in chunks], [gr["item_embs"][c] for _ in users for c in chunks])
        full = np.concatenate(parts).reshape(len(users), N_FLAT)
        return users, lists, full
    return _cached(("flat", L, g), make)


def _descending(scores, keys):
    """score descending (-0 = +0), ties -> the lower key"""
    s = scores + np.float32(0.0)
    return all((s[i] > s[i + 1]) or (s[i] == s[i + 1] and keys[i] < keys[i + 1]) for i in range(len(s) - 1))


@pytest.mark.parametrize("precision", ["split", "exact"])
@pytest.mark.parametrize("L,g", [(64, 1), (64, 32), (33, 1), (33, 32), (1, 1)])
def test_scan_and_candidate_lists(oracle, model_dirs, L, g, precision):
    """nann_search_all_model and nann_search_candidates_model on synth_index(4096, 64, 32), the five users, k = 64, lists of
    300 rows with one duplicate.  Every returned score within 1e-5 of the oracle's logit of its row; scores descend, ties to
    the lower row (scan) or position (lists); every returned row's oracle logit is at least the oracle's k-th best minus
    2e-5 max(1, |s|) (a row may enter or leave the list only on a near-tie: 1e-5 on either side); and the header's
    bit-identities at these L: the list's score of a (user, row) is the scan's, and for split-f16 the traversal's too."""
    from nann_amd import ops, retrieval
    gr, oix, dix = synth_index(N_FLAT, 64, 32)
    users, lists, full = _flat_case(L, g)
    m = ops.Model(model_dirs(64, g, precision), 64, L)
    seq = cuda(users)
    scan = retrieval.search_all_model(dix, m, seq, K_FLAT)
    wide = retrieval.search_all_model(dix, m, seq, 1024)   # (for the bit-identity: most of a list's best 64 are in it)
    cand = retrieval.search_candidates_model(dix, m, seq, candidates=list(lists), k=K_FLAT)
    torch.cuda.synchronize()
    s_rows, s_sc = scan.index.cpu().numpy(), scan.scores.cpu().numpy()
    w_rows, w_sc = wide.index.cpu().numpy(), wide.scores.cpu().numpy()
    c_rows, c_sc, c_pos = cand.index.cpu().numpy(), cand.scores.cpu().numpy(), cand.pos.cpu().numpy()
    assert (cand.status.cpu().numpy() == 0).all() and (cand.n_out.cpu().numpy() == K_FLAT).all()
    assert (s_rows == w_rows[:, :K_FLAT]).all() and (bits(s_sc) == bits(w_sc[:, :K_FLAT])).all()
    worst, common = 0.0, 0
    for b in range(len(users)):
        assert (lists[b][c_pos[b]] == c_rows[b]).all(), b
        for what, rows, sc, keys, pool in (("scan", s_rows[b], s_sc[b], s_rows[b], full[b]),
                                           ("lists", c_rows[b], c_sc[b], c_pos[b], full[b][lists[b]])):
            own = full[b][rows]
            e = _within(sc, own)
            worst = max(worst, e)
            assert e <= RTOL, (what, b, e)
            assert _descending(sc, keys), (what, b)
            kth = np.sort(pool)[::-1][K_FLAT - 1]
            assert (own >= kth - 2e-5 * max(1.0, abs(kth))).all(), (what, b)
        dup = np.nonzero(c_rows[b] == lists[b][17])[0]   # the duplicate: both copies or neither, the same bits, 17 before 200
        assert len(dup) in (0, 2) or (len(dup) == 1 and dup[0] == K_FLAT - 1), (b, dup)
        if len(dup) == 2:
            assert c_pos[b][dup].tolist() == [17, 200] and bits(c_sc[b][dup[0]]) == bits(c_sc[b][dup[1]]), b
        in_scan = {int(i): s for i, s in zip(w_rows[b], bits(w_sc[b]))}
        both = [(int(i), s) for i, s in zip(c_rows[b], bits(c_sc[b])) if int(i) in in_scan]
        common += len(both)
        assert all(in_scan[i] == s for i, s in both), (b, [(i, hex(s), hex(in_scan[i])) for i, s in both if in_scan[i] != s][:4])
    assert common >= len(users) * K_FLAT // 2, common   # the identity was checked on rows, not on an empty set
    print("scan + lists L=%d g=%d %s: max err %.3g, %d (user, row) pairs bit-identical" % (L, g, precision, worst, common))
    if precision == "split":   # the traversal's rows as the lists: every score the same bits
        from nann_amd import synth
        near = synth.make_queries(gr["item_embs"], gr["assign"], 11, seq_len=L, min_len=min(7, L), seed=3 + L)
        seq16 = cuda(np.concatenate([users, near]))   # the five users, and 11 drawn near rows of the index
        r = retrieval.search_model(dix, m, seq16, TOPN)
        torch.cuda.synchronize()
        st, t_rows, t_sc = r.status.cpu().numpy(), r.index.cpu().numpy(), r.scores.cpu().numpy()
        print("traversal vs lists L=%d g=%d: status 0 for %d of the 5 users, %d of the 11 near rows"
              % (L, g, int((st[:5] == 0).sum()), int((st[5:] == 0).sum())))
        assert (st == 0).sum() >= 9, st   # a majority of the 16: the identity is not checked on a user or two
        again = retrieval.search_candidates_model(dix, m, seq16, candidates=[t_rows[b] if st[b] == 0 else t_rows[b][:0]
                                                                          for b in range(len(st))], k=TOPN[5])
        torch.cuda.synchronize()
        a_rows, a_sc = again.index.cpu().numpy(), again.scores.cpu().numpy()
        for b in np.nonzero(st == 0)[0]:
            got = {int(i): s for i, s in zip(a_rows[b], bits(a_sc[b]))}
            assert all(got[int(i)] == s for i, s in zip(t_rows[b], bits(t_sc[b]))), b


# ---- the split form's range: a key beyond f16 -------------------------------------------------------------------------
def test_split_form_drops_a_position_whose_key_overflows(oracle, model_dirs):
    """What include/nann_hip.h states about the split form's range, on the device.  One row of a user's sequence is scaled by
    512, so that position's projected key has components beyond 511.875 (checked on the oracle's projection, which
    k_attn_prepare_split computes bit for bit) while every other position's stay far inside.  The split form then returns
    FINITE logits: those of the model for the sequence WITHOUT that position, within 1e-5 of the oracle run on the L - 1
    remaining rows -- through the stand-alone scorer, the scan (the table kernel's softmax) and the traversal on the hash
    plan (the resident kernel's; its users are full histories drawn near rows of the index).  The position sits in the first tile for one user and in the second for another; the other
    three users' logits are the bits they always were."""
    from nann_amd import ops, retrieval, synth
    from attn_reference import KEY_LIMIT
    d, g, L, dtype = 64, 32, 33, "f16"
    host, code, dev, idx = _table(d, dtype)
    users = _users(L).copy()
    dropped = {0: 5, 2: 32}
    for b, l0 in dropped.items():
        users[b, l0] = (users[b, l0].astype(np.float32) * 512).astype(np.float16)
    am, am_short = _oracle_model(d, code, g, L), _oracle_model(d, code, g, L - 1)
    for b, l0 in dropped.items():
        rc, kproj = oracle.attn_prepare(am, users[b].astype(np.float32))
        assert rc == 0 and np.abs(kproj[l0]).max() >= 2 * KEY_LIMIT, np.abs(kproj[l0]).max()
        assert np.abs(np.delete(kproj, l0, axis=0)).max() < KEY_LIMIT / 2
    short = {b: np.delete(users[b], l0, axis=0) for b, l0 in dropped.items()}
    sc = ops.AttnScorer(d, L, TDT[dtype], _weights(d, g), precision="split")
    kt, upad = sc.prepare(cuda(users))
    got = np.stack([sc.score(kt[b], upad[b], table=dev, indices=idx).cpu().numpy() for b in range(len(users))])
    assert np.isfinite(got).all()
    for b in dropped:
        exp = _oracle_rows(am_short, [short[b]], [host[idx]])[0]
        e = _within(got[b], exp)
        print("overflowed key, stand-alone, user %d: %.3g from the model without the position" % (b, e))
        assert e <= RTOL, (b, e)
    same = [b for b in range(len(users)) if b not in dropped]
    assert (bits(got[same]) == bits(_standalone("split", d, dtype, g, L)["full"][same])).all()
    gr, _, dix = synth_index(N_FLAT, 64, 32)
    m = ops.Model(model_dirs(64, g, "split"), 64, L)
    scan = retrieval.search_all_model(dix, m, cuda(users), K_FLAT)
    torch.cuda.synchronize()
    rows, scores = scan.index.cpu().numpy(), scan.scores.cpu().numpy()
    assert np.isfinite(scores).all()
    for b in dropped:
        e = _within(scores[b], _oracle_rows(am_short, [short[b]], [gr["item_embs"][rows[b]]])[0])
        print("overflowed key, scan, user %d: %.3g from the model without the position" % (b, e))
        assert e <= RTOL, (b, e)
    # the traversal: 8 full histories drawn near rows of the index (so that the requests succeed), position 5 of each scaled
    near = synth.make_queries(gr["item_embs"], gr["assign"], 8, seq_len=L, min_len=L, seed=77)
    near[:, 5] = (near[:, 5].astype(np.float32) * 512).astype(np.float16)
    for u in near:
        rc, kproj = oracle.attn_prepare(am, u.astype(np.float32))
        assert rc == 0 and np.abs(kproj[5]).max() >= 2 * KEY_LIMIT and np.abs(np.delete(kproj, 5, axis=0)).max() < KEY_LIMIT / 2
    trav = retrieval.search_model(dix, m, cuda(near), TOPN, options=retrieval.search_options(traversal="lds_hash", preprojection=True))
    torch.cuda.synchronize()
    assert trav.plan["table"] and trav.plan["visited_set"] == "lds_hash", trav.plan   # the resident kernel's plan
    st, rows, scores = trav.status.cpu().numpy(), trav.index.cpu().numpy(), trav.scores.cpu().numpy()
    assert (st == 0).sum() >= 5, st
    assert np.isfinite(scores[st == 0]).all()
    ok = np.nonzero(st == 0)[0]
    own = _oracle_rows(am_short, [np.delete(near[b], 5, axis=0) for b in ok], [gr["item_embs"][rows[b]] for b in ok])
    e = max(_within(scores[b], o) for b, o in zip(ok, own))
    print("overflowed key, traversal, %d of 8 users: %.3g from the model without the position" % (len(ok), e))
    assert e <= RTOL, e


# ---- 3f. the evaluation traversal: nann_search_eval_model --------------------------------------------------------------
@pytest.mark.parametrize("L", [17, 64])
def test_evaluation_traversal(oracle, model_dirs, L):
    """nann_search_eval_model at g = 32: every score of every user's valid rows within 1e-5 of the oracle's logit of that
    row, and a split weights directory bit-identical to an exact one (the evaluation job runs the f32 form whatever
    precision the directory asks serving for)"""
    from nann_amd import ops, retrieval, synth
    g, cfg = 32, ((2, 1, 1), (100, 60, 30), 50)
    gr, oix, dix = synth_index(20000, 64, 32)
    seqs = synth.make_queries(gr["item_embs"], gr["assign"], 8, seq_len=L, min_len=min(7, L), seed=5 + L)
    r = retrieval.search_eval(dix, ops.Model(model_dirs(64, g, "exact"), 64, L), cuda(seqs), *cfg)
    r2 = retrieval.search_eval(dix, ops.Model(model_dirs(64, g, "split"), 64, L), cuda(seqs), *cfg)
    torch.cuda.synchronize()
    st, n_out, idx, sc = r.status.cpu().numpy(), r.n_out.cpu().numpy(), r.index.cpu().numpy(), r.scores.cpu().numpy()
    assert (st == 0).all() and (n_out > 0).all(), (st, n_out)
    am = _oracle_model(64, oracle.EMB_F16, g, L)
    own = _oracle_rows(am, seqs, [gr["item_embs"][idx[b, :n_out[b]]] for b in range(len(seqs))])
    worst = max(_within(sc[b, :n_out[b]], own[b]) for b in range(len(seqs)))
    print("eval traversal L=%d: rescored max err %.3g" % (L, worst))
    assert worst <= RTOL, worst
    assert (r2.status.cpu().numpy() == st).all() and (r2.n_out.cpu().numpy() == n_out).all()
    assert (r2.index.cpu().numpy() == idx).all() and (bits(r2.scores.cpu().numpy()) == bits(sc)).all()
