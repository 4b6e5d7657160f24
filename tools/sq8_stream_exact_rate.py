#!/usr/bin/env python3
"""The certified sq8 searches without a score buffer (retrieval.search_all_sq8_stream_exact, search_all_range_sq8_stream_exact:
the survivor predicate in the int8 scan's epilogue) next to the calls they stand beside, in one build and one run: 1M and 4M x
128 f16 from synth, L2 and IP, batches of 64 and 1 024 queries, k = 200.
Top-k form, fetch = 200, cap = 8 192, fallback off, per (size, metric, batch):
  A   retrieval.search_all                                   ms per call
  E   retrieval.search_all_sq8_exact(cap = 8 192)            ms per call, share certified
  X   retrieval.search_all_sq8_stream_exact, default sample  ms per call, share certified, mean and max n_survivors, and whether
                                                             every certified row of the result is search_all's, bit for bit
  X4  the same at sample_rows = n_items / 4
Range form, thresholds that give about 10, 100, 1 000 and 10 000 matches per query, cap = 16 384, capacity = the total:
  R   retrieval.search_all_range(capacity = total)           ms per call
  C   retrieval.search_all_range_sq8_exact                   ms per call, share certified
  S   retrieval.search_all_range_sq8_stream_exact            ms per call, share certified, mean and max n_survivors, and whether
                                                             every certified segment is search_all_range's, bit for bit
One process, every shape warmed, the calls of a line alternating inside a round, device events around work that ends in a
synchronise; median of the rounds, min..max beside it.  Code table and bounds are made outside the timed region.
usage: tools/sq8_stream_exact_rate.py [--sizes N,N] [--dim D] [--rounds R] [--out FILE]
writes profiles/sq8_stream_exact_rate.txt (or FILE) and prints the same."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, CAP, RANGE_CAP = 200, 8192, 16384
BATCHES = (64, 1024)
MATCHES = (10, 100, 1000, 10000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,4000000")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sq8_stream_exact_rate.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from nann_amd import ops, retrieval, synth
    from sq8_stream_rate import make_index
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    d = args.dim
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def rounds(pairs):
        """the calls of a line, alternating inside a round -> {name: [ms]}"""
        res = {name: [] for name, _ in pairs}
        for _ in range(args.rounds):
            for name, fn in pairs:
                res[name].append(timed(fn))
        return res

    def fmt(ms):
        return f"{statistics.median(ms):9.3f} ms ({min(ms):.3f}..{max(ms):.3f})"

    def same_bits(a, b):
        return bool((a.view(torch.int32) == b.view(torch.int32)).all())

    emit(f"sq8_stream_exact_rate: x {d} f16, k = {K}, fetch = {K}, cap = {CAP} (range: {RANGE_CAP}), fallback off, rounds = {args.rounds} "
         f"(median, min..max); device {torch.cuda.get_device_name(0)}")
    for n in (int(s) for s in args.sizes.split(",")):
        index, embs, assign = make_index(n, d)
        sq8 = retrieval.make_sq8(index)
        bounds = retrieval.make_sq8_bounds(index, sq8)
        q_all = ops.user_seq_mean(torch.as_tensor(synth.make_queries(embs, assign, max(BATCHES), seed=99)).to(dev))
        x = torch.as_tensor(embs).to(dev).float()
        matches = tuple(m for m in MATCHES if m <= n)
        for metric in ("l2", "ip"):
            sc = ops.Scorer(metric, d, torch.float16)
            # thresholds f32[len(matches), queries]: per query the score of its m-th best row by a float32 product in torch -- near
            # the exact scorer's value, which is all 'about m matches' asks
            thr_all = torch.empty((len(matches), max(BATCHES)), dtype=torch.float32, device=dev)
            for c0 in range(0, max(BATCHES), 64):
                qc = q_all[c0:c0 + 64]
                s = qc @ x.T
                if metric == "l2":
                    s = 2 * s - (x * x).sum(1)[None, :] - (qc * qc).sum(1)[:, None]
                top = torch.topk(s, max(matches), dim=1).values
                for j, m in enumerate(matches):
                    thr_all[j, c0:c0 + 64] = top[:, m - 1]
                del s, top
            for b in BATCHES:
                q = q_all[:b]
                emit(f"{n} items, {metric}, batch {b}")
                run = {"A": lambda: retrieval.search_all(index, sc, q, K),
                       "E": lambda: retrieval.search_all_sq8_exact(index, sq8, bounds, sc, q, K, fetch=K, cap=CAP, fallback=False),
                       "X": lambda: retrieval.search_all_sq8_stream_exact(index, sq8, bounds, sc, q, K, fetch=K, cap=CAP, fallback=False),
                       "X4": lambda: retrieval.search_all_sq8_stream_exact(index, sq8, bounds, sc, q, K, fetch=K, sample_rows=n // 4,
                                                                           cap=CAP, fallback=False)}
                out = {name: fn() for name, fn in run.items()}  # (the warming calls)
                torch.cuda.synchronize()
                res = rounds(list(run.items()))
                a = statistics.median(res["A"])
                emit(f"  top-k  A  search_all:                          {fmt(res['A'])}")
                emit(f"         E  search_all_sq8_exact:                {fmt(res['E'])}   A / E = {a / statistics.median(res['E']):.2f}   "
                     f"certified {out['E'].certified.float().mean().item():.4f}")
                for name, what in (("X", "default sample"), ("X4", "sample = n / 4  ")):
                    r, t = out[name], statistics.median(res[name])
                    cert = r.certified.bool()
                    ok = bool((r.index[cert] == out["A"].index[cert]).all()) and same_bits(r.scores[cert], out["A"].scores[cert])
                    surv = r.n_survivors.cpu().numpy()
                    emit(f"         {name:2s} search_all_sq8_stream_exact, {what}: {fmt(res[name])}   A / {name} = {a / t:.2f}   E / {name} = "
                         f"{statistics.median(res['E']) / t:.2f}   certified {cert.float().mean().item():.4f}   n_survivors mean "
                         f"{surv.mean():.0f} max {surv.max()}   certified rows equal search_all's bits: {ok}")
                for j, m in enumerate(matches):
                    thr = thr_all[j, :b].contiguous()
                    ref = retrieval.search_all_range(index, sc, q, thr)
                    total = ref.total
                    run = {"R": lambda: retrieval.search_all_range(index, sc, q, thr, capacity=total),
                           "C": lambda: retrieval.search_all_range_sq8_exact(index, sq8, bounds, sc, q, thr, cap=RANGE_CAP, capacity=total,
                                                                             fallback=False),
                           "S": lambda: retrieval.search_all_range_sq8_stream_exact(index, sq8, bounds, sc, q, thr, cap=RANGE_CAP,
                                                                                    capacity=total, fallback=False)}
                    out = {name: fn() for name, fn in run.items()}  # (the warming calls)
                    torch.cuda.synchronize()
                    res = rounds(list(run.items()))
                    r_ms, c_ms, s_ms = (statistics.median(res[name]) for name in ("R", "C", "S"))
                    sr = out["S"]
                    cert = sr.certified.bool()
                    ok = True  # every certified segment against search_all_range's: the same length, rows and score bits
                    sp, rp = sr.row_splits.cpu().numpy(), ref.row_splits.cpu().numpy()
                    for i in np.flatnonzero(cert.cpu().numpy()):
                        g, e = slice(sp[i], sp[i + 1]), slice(rp[i], rp[i + 1])
                        ok = ok and sp[i + 1] - sp[i] == rp[i + 1] - rp[i] and bool((sr.index[g] == ref.index[e]).all()) and \
                            same_bits(sr.scores[g], ref.scores[e])
                    surv = sr.n_survivors.cpu().numpy()
                    emit(f"  range, about {m:5d} matches ({total / b:.1f} per query)")
                    emit(f"         R  search_all_range:                    {fmt(res['R'])}")
                    emit(f"         C  search_all_range_sq8_exact:          {fmt(res['C'])}   R / C = {r_ms / c_ms:.2f}   certified "
                         f"{out['C'].certified.float().mean().item():.4f}")
                    emit(f"         S  search_all_range_sq8_stream_exact:   {fmt(res['S'])}   R / S = {r_ms / s_ms:.2f}   C / S = {c_ms / s_ms:.2f}   "
                         f"certified {cert.float().mean().item():.4f}   n_survivors mean {surv.mean():.0f} max {surv.max()}   certified "
                         f"segments equal search_all_range's bits: {ok}")
        del index, sq8, bounds, x
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
