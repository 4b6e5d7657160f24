"""Test-side statement of the range selection (csrc/nann_range.h), shared by test_range_cpu.py and test_range_gpu.py; nothing
under nann_amd/ imports it.

reference()  the plain answer: per query np.nonzero of the match rule, rows ascending, cut at the capacity.
model()      count -> scan -> fill as the kernels do it: blocks of BLOCK positions that begin on a 4-position boundary of the
             chunk's score buffer, a block-count prefix built in steps of SCAN_STEP blocks with a carry, row_splits carried
             from chunk to chunk, every store guarded by pos < capacity."""
import numpy as np

BLOCK = 2048      # kRangeBlockRows
SCAN_STEP = 256   # blocks per step of k_range_scan's loop
CHUNK = 128       # kScanMaxChunk: most queries of a chunk
SENTINEL = -77


def match(scores, thr):
    """s >= thr and s != -inf, IEEE: a NaN on either side matches nothing, -0 >= +0 holds"""
    with np.errstate(invalid="ignore"):
        return (scores >= np.float32(thr)) & (scores != -np.inf)


def _outputs(capacity):
    return (np.full(capacity, SENTINEL, np.int32), np.full(capacity, SENTINEL, np.float32), np.full(capacity, SENTINEL, np.int64))


def reference(scores, thr, item_ids, capacity):
    """-> (row_splits i64[B + 1], index i32[capacity], scores f32[capacity], item_ids i64[capacity]); untouched = SENTINEL"""
    b = scores.shape[0]
    rows = [np.nonzero(match(scores[i], thr[i]))[0] for i in range(b)]
    splits = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    out_index, out_scores, out_ids = _outputs(capacity)
    flat = np.concatenate(rows) if b else np.zeros(0, np.int64)
    flat_scores = np.concatenate([scores[i][rows[i]] for i in range(b)]) if b else np.zeros(0, np.float32)
    m = min(capacity, len(flat))
    out_index[:m] = flat[:m]
    out_scores[:m] = flat_scores[:m]
    out_ids[:m] = item_ids[flat[:m]]
    return splits, out_index, out_scores, out_ids


def n_blocks(n_items, block=BLOCK):
    return (n_items + 3 + block - 1) // block


def model(scores, thr, item_ids, capacity, chunk=CHUNK, block=BLOCK, scan_step=SCAN_STEP):
    """the same outputs, built the way the kernels build them"""
    b, n = scores.shape
    nb = n_blocks(n, block)
    splits = np.full(b + 1, SENTINEL, np.int64)
    out_index, out_scores, out_ids = _outputs(capacity)
    for c0 in range(0, b, chunk):
        n_q = min(chunk, b - c0)
        buf = np.ascontiguousarray(scores[c0:c0 + n_q]).reshape(-1)  # the chunk's score buffer: query i at position i * n
        # count: block j of query i covers positions [first, first + block) where first = (i * n rounded down to 4) + j * block
        hit = []
        counts = np.zeros((n_q, nb), np.int64)
        for i in range(n_q):
            begin, end = i * n, (i + 1) * n
            per = []
            for j in range(nb):
                lo = (begin & ~3) + j * block
                pos = np.arange(max(lo, begin), min(lo + block, end))
                pos = pos[match(buf[pos], thr[c0 + i])] if len(pos) else pos
                per.append(pos)
                counts[i, j] = len(pos)
            hit.append(per)
        # scan: exclusive prefix of a query's block counts, scan_step blocks at a time with the sum so far carried
        prefix = np.zeros_like(counts)
        totals = np.zeros(n_q, np.int64)
        for i in range(n_q):
            carry = 0
            for j0 in range(0, nb, scan_step):
                part = counts[i, j0:j0 + scan_step]
                inclusive = np.cumsum(part)
                prefix[i, j0:j0 + scan_step] = carry + inclusive - part
                carry += int(inclusive[-1])
            totals[i] = carry
        # splits: the first chunk writes the leading 0, a later one continues from the last split of the chunk before it
        if c0 == 0:
            splits[0] = 0
        base = splits[c0]
        for i in range(n_q):
            splits[c0 + i + 1] = base + totals[:i + 1].sum()
        # fill: every store guarded by pos < capacity
        for i in range(n_q):
            for j in range(nb):
                for rank, p in enumerate(hit[i][j]):
                    at = splits[c0 + i] + prefix[i, j] + rank
                    if at < capacity:
                        row = p - i * n
                        out_index[at], out_scores[at], out_ids[at] = row, buf[p], item_ids[row]
    return splits, out_index, out_scores, out_ids
