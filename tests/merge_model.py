"""The shard merge and TopKV2 in plain numpy: what k_merge_records, nann_merge_topk, nann_sharded_topk and nann_topk have to
return, written without the library and without the oracle.

  order    positions of a row's k best: value descending, -0 == +0, ties to the lower position.  Over the shard-major
           concatenation of a query's lists that is "ties to the lower shard, then the lower slot".
  pack     the record a rank contributes (nann_comm.hip k_pack_record): scores f32[B, k], then at byte B * k * 4 the ids
           i64[B, k], padded to 256 bytes; a query that failed on the shard (status != 0) carries (-inf, 0).
  merge_records
           the merge read straight from `world` records that lie record_bytes apart: shard s of position pos is pos // k_in,
           its scores start at s * stride, its ids at s * stride + B * k_in * 4.

Scores leave with the bits they came in with (a selected -0 stays -0).

MUTANTS are this model made wrong in one rule each; tests/test_merge_model_cpu.py shows for every one a case of
tests/merge_cases.py whose output it changes -- the evidence, obtained without a GPU, that the comparison on the device would
notice a kernel that is wrong in that way."""
import numpy as np

MUTANTS = (
    "tie_high_shard",       # equal scores: the higher shard first
    "ids_from_shard0",      # the ids of every shard are read from shard 0's record
    "id_offset_k_out",      # the id section is taken to start at B * k_out * 4
    "id_stride_unpadded",   # the id base steps by the unpadded record (the score base by the padded one)
    "stride_unpadded",      # records are taken to lie B * k_in * 12 bytes apart
    "neg_zero_below",       # -0 sorts below +0
    "failed_keeps_scores",  # a failed query's ids become 0, its scores stay
)


def record_bytes(n_queries, k):
    return (n_queries * k * 12 + 255) & ~255


def order(scores, k, k_in=None, mutant=None):
    """positions of the k best of a row (k_in: the length of one shard's list, for the mutant that needs the shard)"""
    scores = np.asarray(scores, np.float32)
    if mutant == "tie_high_shard":
        pos = np.arange(scores.size)
        shard, slot = pos // k_in, pos % k_in
        return np.lexsort((slot, -shard, -scores))[:k]
    if mutant == "neg_zero_below":
        u = scores.view(np.uint32).astype(np.int64)
        key = np.where(u >> 31, 0xffffffff - u, u + 0x80000000)  # monotone in the value, -0 one below +0
        return np.argsort(-key, kind="stable")[:k]
    return np.argsort(-scores, kind="stable")[:k]


def top_k(row, k):
    """TopKV2 of one row -> (values with their own bits, indices i32)"""
    row = np.asarray(row, np.float32)
    pos = order(row, k)
    return row[pos], pos.astype(np.int32)


def merge(scores, ids, k_out, mutant=None):
    """scores f32[B, world, k_in], ids i64[B, world, k_in] -> (scores f32[B, k_out], ids i64[B, k_out])"""
    scores = np.asarray(scores, np.float32)
    ids = np.asarray(ids, np.int64)
    b, world, k_in = scores.shape
    out_s = np.empty((b, k_out), np.float32)
    out_i = np.empty((b, k_out), np.int64)
    for q in range(b):
        row = scores[q].reshape(-1)
        pos = order(row, k_out, k_in, mutant)
        out_s[q] = row[pos]
        out_i[q] = ids[q].reshape(-1)[pos]
    return out_s, out_i


def pack(scores, ids, status, mutant=None):
    """scores f32[B, k], ids i64[B, k], status i32[B] or None -> uint8[record_bytes(B, k)]"""
    scores = np.ascontiguousarray(scores, np.float32)
    ids = np.ascontiguousarray(ids, np.int64)
    b, k = scores.shape
    s, i = scores.copy(), ids.copy()
    if status is not None:
        for q in range(b):
            if status[q] != 0:
                if mutant != "failed_keeps_scores":
                    s[q] = -np.inf
                i[q] = 0
    rec = np.zeros(record_bytes(b, k), np.uint8)
    rec[:b * k * 4] = np.frombuffer(s.tobytes(), np.uint8)
    rec[b * k * 4:b * k * 12] = np.frombuffer(i.tobytes(), np.uint8)
    return rec


def _read(buf, off, count, dtype):
    """count items of dtype at byte off of buf (zeros behind its end: a mutant may look there)"""
    n = count * np.dtype(dtype).itemsize
    raw = bytes(buf[off:off + n])
    return np.frombuffer(raw + bytes(n - len(raw)), dtype)


def gathered(recv, world, n_queries, k_in, stride=None, k_out=None, mutant=None):
    """the records as the merge sees them -> (scores f32[B, world, k_in], ids i64[B, world, k_in])"""
    buf = np.ascontiguousarray(recv, np.uint8).reshape(-1)
    b = n_queries
    padded = record_bytes(b, k_in) if stride is None else stride
    s_stride = b * k_in * 12 if mutant == "stride_unpadded" else padded
    i_stride = b * k_in * 12 if mutant in ("stride_unpadded", "id_stride_unpadded") else padded
    i_off = b * (k_out if mutant == "id_offset_k_out" else k_in) * 4
    sc, ii = [], []
    for s in range(world):
        sc.append(_read(buf, s * s_stride, b * k_in, np.float32).reshape(b, k_in))
        ii.append(_read(buf, (0 if mutant == "ids_from_shard0" else s) * i_stride + i_off, b * k_in, np.int64).reshape(b, k_in))
    return np.stack(sc, 1), np.stack(ii, 1)


def merge_records(recv, world, n_queries, k_in, k_out, stride=None, mutant=None):
    """recv: `world` records, record s at byte s * stride (default: the padded record) -> merge() of what they hold"""
    sc, ii = gathered(recv, world, n_queries, k_in, stride, k_out, mutant)
    return merge(sc, ii, k_out, mutant)


def exchange(scores, ids, status, k_out, mutant=None):
    """pack every shard's own lists, lay the records side by side, merge: scores f32[B, world, k_in], ids i64[B, world, k_in],
    status i32[world, B] or None -> (scores f32[B, k_out], ids i64[B, k_out])"""
    b, world, k_in = scores.shape
    recv = np.concatenate([pack(scores[:, s], ids[:, s], None if status is None else status[s], mutant) for s in range(world)])
    return merge_records(recv, world, b, k_in, k_out, mutant=mutant)
