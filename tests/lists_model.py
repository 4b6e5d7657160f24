"""The shared-list search in numpy: the partition's CSR from list_of_row, and the candidate list a query's probes stand for
(what nann_search_lists is defined by: nann_search_candidates over that list)."""
import numpy as np


def partition_csr(list_of_row, n_lists):
    """(list_splits i64[n_lists + 1], list_rows i32[n_listed]): every list in ascending row order; a negative value: in no list"""
    lor = np.asarray(list_of_row, np.int64)
    assert (lor < n_lists).all()
    rows = np.flatnonzero(lor >= 0)
    order = np.argsort(lor[rows], kind="stable")  # stable: rows stay ascending within a list
    splits = np.zeros(n_lists + 1, np.int64)
    splits[1:] = np.cumsum(np.bincount(lor[rows], minlength=n_lists))
    return splits, rows[order].astype(np.int32)


def expansion(splits, rows, probes):
    """the rows query `probes` (one row of the probes array) names: its lists in slot order, negative slots skipped; None for
    a query that names a list >= n_lists"""
    n_lists = len(splits) - 1
    if any(p >= n_lists for p in probes):
        return None
    parts = [rows[splits[p]:splits[p + 1]] for p in probes if p >= 0]
    return np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)
