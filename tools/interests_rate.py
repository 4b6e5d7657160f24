#!/usr/bin/env python3
"""User interests (ops.user_seq_interests: a behaviour sequence clustered into interest vectors) in front of the multi-vector
search, at a size a user runs: 1M x 128 f16 under L2 on the shipped builder's graph, ef 128, top-200; 256 and 1 024 users with
histories of 50 rows drawn from 1, 2 and 4 planted clusters (synth knows every item's cluster), n_vec 4 and 8, 8 Lloyd rounds.
Reported:
  1. ms per call of  I  ops.user_seq_interests,  A  ops.user_seq_mean on the same sequences (the reduction the serving path
     runs today) and  T  the same algorithm in batched torch ops on the device (torch_interests below; not bit-exact, same steps);
  2. Q  retrieval.search_seq_multi(k = 200) and  M  retrieval.search_multi over the vectors I made: I's share of Q;
  3. recall@200 of search_seq_multi and of retrieval.search over the mean query.  Ground truth for both: the union of the
     exhaustive top-200 of the user's planted cluster centres (retrieval.search_all_multi over the centres at k = 200).  In 128
     dimensions the rows of a cluster lie in a thin shell around its centre, and WHICH 200 of a cluster's ~3 900 rows are
     nearest depends on the query point more than on the cluster, so this recall is near chance for any query made of a
     finite history; next to it therefore, per answer: "in taste", the share of returned rows that belong to one of the
     user's planted clusters, and "tastes reached", the share of the user's planted clusters with at least one returned row.
One process, every shape warmed, the calls alternating inside a round, device events around work that ends in a synchronise;
median of the rounds, min..max beside it.  The kernel's share of a call's kernel time comes from kernel times, in a run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kt -- python tools/interests_rate.py --trace
  python tools/interests_rate.py --stats DIR/.../kt_kernel_stats.csv      # appends the share to the output file
--trace runs search_seq_multi (256 users, 2 planted clusters, n_vec 4) and nothing else that launches its kernels but the
index's own probe.
usage: tools/interests_rate.py [items] [dim] [--rounds R] [--out FILE] [--trace | --stats CSV]
writes profiles/interests_rate.txt (or FILE) and prints the same."""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

USERS = (256, 1024)
N_VECS = (4, 8)
PLANTED = (1, 2, 4)
K, EF, SEQ_LEN, N_ITER, N_CLUSTERS = 200, 128, 50, 8, 256
TRACE_CALLS = 5
KERNEL = "k_user_seq_interests"
OTHER_KERNELS = ("k_search", "k_order_key", "k_order_perm", "k_union_topk")


def kernel_share(path):
    """kernel_stats.csv of the --trace run -> lines: the interests kernel's share of search_seq_multi's kernel time"""
    total = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0)
            for k in (KERNEL,) + OTHER_KERNELS:
                if k in name:
                    total[k] = total.get(k, 0.0) + ns
    assert KERNEL in total and "k_search" in total, f"{path}: no row for the interests or the traversal kernel"
    mine, rest = total[KERNEL], sum(total.get(k, 0.0) for k in OTHER_KERNELS)
    return [f"kernel times (rocprofv3 --kernel-trace --stats, {TRACE_CALLS} calls of search_seq_multi, {USERS[0]} users, 2 planted "
            f"clusters, n_vec {N_VECS[0]}, k = {K}; the traversal's total includes the index's 64-query probe):",
            f"  {KERNEL:22s} {mine / 1e6:10.3f} ms in all = {mine / TRACE_CALLS * 1e-3:.2f} us per call",
            f"  traversal and union    {rest / 1e6:10.3f} ms in all = {rest / TRACE_CALLS * 1e-3:.2f} us per call",
            f"  the interests kernel is {100 * mine / (mine + rest):.1f} % of search_seq_multi's kernel time"]


def torch_interests(torch, seq, n_vec, n_iter):
    """the contract's steps in batched torch ops: seq f16[B, L, d] -> (q [B, n_vec, d], weights [B, n_vec])"""
    x = seq.float()
    live = (x != 0).any(dim=2)                                    # [B, L]
    m = live.sum(dim=1).clamp(min=1).float()
    mean = x.sum(dim=1) / m[:, None]
    inf = torch.full((), float("inf"), device=x.device)

    def dist(c):                                                  # c [B, C, d] -> [B, L, C]
        return ((x[:, :, None, :] - c[:, None, :, :]) ** 2).sum(dim=3)

    first = torch.where(live, dist(mean[:, None])[:, :, 0], -inf).argmax(dim=1)
    cent = [torch.gather(x, 1, first[:, None, None].expand(-1, 1, x.shape[2]))[:, 0]]
    mind = torch.full(live.shape, float("inf"), device=x.device)
    for _ in range(1, n_vec):  # (a user that runs out of distinct rows repeats a seed: its cluster stays empty)
        mind = torch.minimum(mind, dist(cent[-1][:, None])[:, :, 0])
        nxt = torch.where(live, mind, -inf).argmax(dim=1)
        cent.append(torch.gather(x, 1, nxt[:, None, None].expand(-1, 1, x.shape[2]))[:, 0])
    cent = torch.stack(cent, dim=1)                               # [B, n_vec, d]

    def assign():
        one = torch.nn.functional.one_hot(dist(cent).argmin(dim=2), n_vec).float() * live[:, :, None]
        return one, one.sum(dim=1)                                # [B, L, n_vec], [B, n_vec]

    for _ in range(n_iter):
        one, count = assign()
        sums = torch.einsum("blc,bld->bcd", one, x)
        cent = torch.where(count[:, :, None] > 0, sums / count.clamp(min=1)[:, :, None], cent)
    _, count = assign()
    order = torch.sort(count, dim=1, descending=True, stable=True).indices
    q = torch.gather(cent, 1, order[:, :, None].expand(-1, -1, x.shape[2]))
    return q, torch.gather(count, 1, order) / m[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("items", nargs="?", type=int, default=1_000_000)
    ap.add_argument("dim", nargs="?", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interests_rate.txt"))
    ap.add_argument("--trace", action="store_true", help="a short run for a kernel trace")
    ap.add_argument("--stats", help="kernel_stats.csv of a --trace run: append the interests kernel's share to the output file")
    args = ap.parse_args()
    if args.stats:
        lines = kernel_share(args.stats)
        print("\n".join(lines))
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        return

    import numpy as np
    import torch
    from nann_amd import ops, retrieval, synth
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n, d = args.items, args.dim
    g = synth.make_index(n, d, ef=EF, device="cuda", n_clusters=N_CLUSTERS)
    index = retrieval.Index.from_dict(g)
    sc = ops.Scorer("l2", d, torch.float16)
    topn = [EF, EF, EF, EF, EF, K]
    centres = synth.make_centres(d, N_CLUSTERS)  # (make_index's own)
    order = np.argsort(g["assign"], kind="stable")
    starts = np.searchsorted(g["assign"][order], np.arange(N_CLUSTERS + 1))

    def users(n_users, planted, seed):
        """-> (comm_seq f16[n_users, 50, d] on the device, the planted clusters i64[n_users, planted]): a user's 50 rows are
        items of its clusters, shared evenly and shuffled"""
        rng = np.random.default_rng(seed)
        seq = np.zeros((n_users, SEQ_LEN, d), np.float16)
        cl = np.stack([rng.choice(N_CLUSTERS, planted, replace=False) for _ in range(n_users)])
        for u in range(n_users):
            of_row = rng.permutation(np.arange(SEQ_LEN) % planted)
            for j, c in enumerate(cl[u]):
                rows = np.flatnonzero(of_row == j)
                seq[u, rows] = g["item_embs"][order[rng.integers(starts[c], starts[c + 1], len(rows))]]
        return torch.as_tensor(seq).to(dev), cl

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    if args.trace:
        seq, _ = users(USERS[0], 2, seed=31)
        for _ in range(TRACE_CALLS):
            retrieval.search_seq_multi(index, sc, seq, N_VECS[0], topn, k=K, n_iter=N_ITER)
        torch.cuda.synchronize()
        print(f"trace run: {TRACE_CALLS} calls of search_seq_multi, {USERS[0]} users, n_vec {N_VECS[0]}")
        return

    lines = [f"interests_rate: {n} items x {d} f16, L2, ef {EF}, top-{K}, histories of {SEQ_LEN} rows, {N_ITER} Lloyd rounds, rounds = "
             f"{args.rounds} (median, min..max); device {torch.cuda.get_device_name(0)}"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def fmt(ms):
        return f"{statistics.median(ms) * 1e3:9.1f} us ({min(ms) * 1e3:.1f}..{max(ms) * 1e3:.1f})"

    def recall(rows, n_out, truth):
        hit = 0
        for u in range(rows.shape[0]):
            hit += len(set(rows[u, :int(n_out[u])].tolist()) & set(truth[u].tolist()))
        return hit / float(truth.size)

    assign_of_row = np.asarray(g["assign"])

    def tastes(rows, n_out, cl):
        """-> (share of returned rows in one of the user's planted clusters, share of its planted clusters with a row)"""
        inside = total = reached = 0
        for u in range(rows.shape[0]):
            got = assign_of_row[rows[u, :int(n_out[u])]]
            inside += int(np.isin(got, cl[u]).sum())
            total += len(got)
            reached += len(set(got.tolist()) & set(cl[u].tolist()))
        return inside / max(total, 1), reached / float(cl.size)

    for n_users in USERS:
        for planted in PLANTED:
            seq, cl = users(n_users, planted, seed=1000 * planted + n_users)
            truth = retrieval.search_all_multi(index, sc, torch.as_tensor(centres[cl]).to(dev), K)
            mean_q = ops.user_seq_mean(seq)
            by_mean = retrieval.search(index, sc, mean_q, topn, want_counters=False)
            torch.cuda.synchronize()
            assert bool((truth.n_out == K).all())
            truth_rows = truth.index.cpu().numpy()
            emit(f"{n_users} users, {planted} planted cluster{'s' if planted > 1 else ''} per history:")
            emit(f"  A  user_seq_mean:                          {fmt([timed(lambda: ops.user_seq_mean(seq)) for _ in range(args.rounds + 2)][2:])}")
            mean_rows = by_mean.index.cpu().numpy()
            emit(f"     recall@{K} of search over the mean query:            "
                 f"{recall(mean_rows, np.full(n_users, K), truth_rows):.4f}   in taste {tastes(mean_rows, np.full(n_users, K), cl)[0]:.4f}, "
                 f"tastes reached {tastes(mean_rows, np.full(n_users, K), cl)[1]:.4f}")
            for nv in N_VECS:
                q = ops.user_seq_interests(seq, nv, n_iter=N_ITER)[0]
                tq, tw = torch_interests(torch, seq, nv, N_ITER)
                torch.cuda.synchronize()
                pairs = [("I", lambda: ops.user_seq_interests(seq, nv, n_iter=N_ITER)),
                         ("T", lambda: torch_interests(torch, seq, nv, N_ITER)),
                         ("Q", lambda: retrieval.search_seq_multi(index, sc, seq, nv, topn, k=K, n_iter=N_ITER)),
                         ("M", lambda: retrieval.search_multi(index, sc, q, topn, k=K))]
                for _, fn in pairs:  # warm every shape
                    fn()
                torch.cuda.synchronize()
                res = {name: [] for name, _ in pairs}
                for _ in range(args.rounds):
                    for name, fn in pairs:
                        res[name].append(timed(fn))
                r, interests = retrieval.search_seq_multi(index, sc, seq, nv, topn, k=K, n_iter=N_ITER)
                torch.cuda.synchronize()
                i, t, qq, mm = (statistics.median(res[c]) for c in "ITQM")
                found = float(interests.n_interests.float().mean())
                emit(f"  n_vec {nv}: {found:.2f} interests per user on average")
                emit(f"    I  user_seq_interests:                   {fmt(res['I'])}")
                emit(f"    T  the same steps in batched torch ops:  {fmt(res['T'])}   (I = {i / t:.4f} x T's time)")
                emit(f"    Q  search_seq_multi(k = {K}):            {fmt(res['Q'])}")
                emit(f"    M  search_multi over I's vectors:        {fmt(res['M'])}   (I = {100 * i / qq:.1f} % of Q, {100 * i / mm:.1f} % of M; Q - M = {(qq - mm) * 1e3:.1f} us)")
                got_rows, got_n = r.index.cpu().numpy(), r.n_out.cpu().numpy()
                emit(f"       recall@{K} of search_seq_multi:                     "
                     f"{recall(got_rows, got_n, truth_rows):.4f}   in taste {tastes(got_rows, got_n, cl)[0]:.4f}, "
                     f"tastes reached {tastes(got_rows, got_n, cl)[1]:.4f}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
