"""Seeded predicate sets and filters for the device tests of the attribute predicates, in the dict form predicate_model reads,
and their way onto the device through retrieval.make_attributes / make_predicates / make_filter.  Query i's conditions go by
i % 8, so that a batch of 17 or more holds every profile: nothing passes, everything passes, and the mixtures between."""
import types

import numpy as np

I32_MIN = np.iinfo(np.int32).min
N_LABELS = 20   # the labels of the rows: 0 .. 19, and a few rows at -1 and at INT32_MIN


def make(rng, n_items, n_q, tests=7):
    """tests: bit 0 labels, bit 1 values, bit 2 tags -> the predicate dict of predicate_model"""
    pred = {}
    if tests & 1:
        lab = rng.integers(0, N_LABELS, n_items).astype(np.int32)
        lab[rng.random(n_items) < 0.03] = -1
        lab[rng.random(n_items) < 0.03] = I32_MIN
        every = np.concatenate((np.arange(N_LABELS), [-1, I32_MIN])).astype(np.int32)
        lists = []
        for i in range(n_q):
            p = i % 8
            if p == 0:
                lists.append(every)                                                              # every label there is
            elif p == 1:
                lists.append(np.array([99, -7], np.int32))                                       # none of them
            elif p == 2:
                lists.append(np.zeros(0, np.int32))                                              # empty: no label test
            elif p == 3:
                lists.append(np.tile(rng.choice(N_LABELS, 10, replace=False), 60).astype(np.int32))   # 600 entries, ten distinct
            elif p == 4:
                lists.append(np.array([I32_MIN, 3, 3], np.int32))
            elif p == 5:
                lists.append(np.concatenate((np.full(300, 99), [5], np.full(140, 98), [-1])).astype(np.int32))  # hits in rounds 3 and 4
            else:
                lists.append(rng.integers(0, N_LABELS, int(rng.integers(1, 9))).astype(np.int32))
        pred["label_of_row"] = lab
        pred["label_splits"] = np.concatenate(([0], np.cumsum([len(l) for l in lists]))).astype(np.int64)
        pred["labels"] = np.concatenate(lists).astype(np.int32)
    if tests & 2:
        v = rng.standard_normal(n_items).astype(np.float32)
        v[rng.random(n_items) < 0.03] = np.nan
        lo = rng.standard_normal(n_q).astype(np.float32) - 1
        hi = lo + 2 * rng.random(n_q).astype(np.float32) + 0.5
        for i in range(n_q):
            if i % 8 == 0:
                lo[i], hi[i] = -np.inf, np.inf
            elif i % 8 == 1:
                lo[i], hi[i] = 1.0, -1.0                                                         # lo > hi
            elif i % 8 == 7:
                hi[i] = np.nan
        pred["value_of_row"], pred["value_lo"], pred["value_hi"] = v, lo, hi
    if tests & 4:
        t = rng.integers(0, 2 ** 63, n_items, dtype=np.uint64) | rng.integers(0, 2 ** 63, n_items, dtype=np.uint64)
        t[rng.random(n_items) < 0.5] |= np.uint64(1 << 63)
        one = lambda b: np.uint64(1 << int(b))
        ta, ty, tn = np.zeros(n_q, np.uint64), np.zeros(n_q, np.uint64), np.zeros(n_q, np.uint64)
        for i in range(n_q):
            p = i % 8
            if p in (0, 2):
                continue                                                                         # no tag asked for, none barred
            if p == 1:
                ta[i], tn[i] = one(5), one(5)                                                    # asked for and barred: nothing
            else:
                ta[i] = one(63) if p % 2 else one(rng.integers(0, 63))
                ty[i] = one(rng.integers(0, 64)) | one(rng.integers(0, 64)) if p >= 5 else 0
                tn[i] = one(rng.integers(0, 64)) if p != 4 else 0
        pred["tags_of_row"], pred["tags_all"], pred["tags_any"], pred["tags_none"] = t, ta, ty, tn
    return pred


def make_filter(rng, n_items, n_q, hot=None):
    """(deny bool[n_items], one exclusion list per query): rows out of range and repeats among the lists; hot[i]: rows that
    query i's list is known to hold, of which some are excluded"""
    deny = rng.random(n_items) < 0.15
    exclude = []
    for i in range(n_q):
        parts = [rng.integers(-2, n_items + 2, int(rng.integers(0, 30)))]
        if hot is not None and len(hot[i]):
            parts.append(np.asarray(hot[i])[:3])
        e = np.concatenate(parts).astype(np.int64)
        exclude.append(np.concatenate((e, e[:2])) if i % 3 == 0 else e)                          # a row listed twice
    return deny, exclude


def index_like(n_items, item_ids, device):
    import torch
    return types.SimpleNamespace(n_items=n_items, item_ids=torch.as_tensor(item_ids).to(device), device=torch.device(device))


def on_device(index, pred, n_q, filter=None):
    """-> (retrieval.Predicates, retrieval.Filter or None) on the index's device"""
    from nann_amd import retrieval
    at = retrieval.make_attributes(index, label_of_row=pred.get("label_of_row"), value_of_row=pred.get("value_of_row"),
                                   tags_of_row=pred.get("tags_of_row"))
    label_in = None
    if "label_splits" in pred:
        s = pred["label_splits"]
        label_in = [pred["labels"][s[i]:s[i + 1]] for i in range(n_q)]
    rng_ = (pred["value_lo"], pred["value_hi"]) if "value_lo" in pred else None
    p = retrieval.make_predicates(at, n_q, label_in=label_in, value_range=rng_, tags_all=pred.get("tags_all"),
                                  tags_any=pred.get("tags_any"), tags_none=pred.get("tags_none"))
    f = None
    if filter is not None:
        f = retrieval.make_filter(index, deny_rows=np.nonzero(filter[0])[0], exclude_rows=filter[1])
    return p, f
