"""HNSW index construction + export in the reference's on-disk layout.

Mirrors NANN_impls/nann/delivery/build_hnsw_index.py: `build_and_save_index(embeddings,
start_level, num_neighbors, output_dir)` writes `enter_points.npy`,
`neighbors_level_{l}_values.npy` (int64, -1 slots dropped) and
`neighbors_level_{l}_row_splits.npy` (int64[N+1], a row for every item, empty when the node is
absent at that level).  The graph itself comes from nann_amd/csrc/host/hnsw_build.cpp (C++,
multi-threaded) instead of Faiss, which is not available; its raw arrays have Faiss' shapes
(`levels`, `offsets`, `neighbors`, `cum_nneighbor_per_level`) so the export code below is the
reference's, vectorised.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "csrc", "host", "hnsw_build.cpp")
# every source of libnann_host.so (the HNSW builder + the CPU hooks onto the frozen-GraphDef reader and the
# pre-projected tables' cache) and what they include
_SRCS = [_SRC, os.path.join(_HERE, "csrc", "host", "nann_graphdef_c.cpp"),
         os.path.join(_HERE, "csrc", "host", "nann_projcache_c.cpp")]
_DEPS = _SRCS + [os.path.join(_HERE, "csrc", "host", "nann_graphdef.h"), os.path.join(_HERE, "csrc", "host", "nann_graphdef_text.h"),
                 os.path.join(_HERE, "csrc", "host", "nann_blaze_options.h"), os.path.join(_HERE, "csrc", "host", "nann_npy.h"), os.path.join(_HERE, "csrc", "host", "nann_projcache.h")]
_LIB_PATH = os.path.join(_HERE, "_build", "libnann_host.so")
_LIB = None


def build_host_lib(force=False, sanitize=False):
    """g++ -O3 the host-side builder into nann_amd/_build/libnann_host.so.  sanitize: the same sources under AddressSanitizer +
    UBSan into libnann_host_asan.so -- what the parser fuzzers of the CPU suite load (tests/fuzz/; the process needs
    LD_PRELOAD=libasan.so)."""
    path = _LIB_PATH.replace(".so", "_asan.so") if sanitize else _LIB_PATH
    if force or not os.path.exists(path) or max(os.path.getmtime(p) for p in _DEPS) > os.path.getmtime(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        flags = (["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
                 if sanitize else ["-O3"])
        subprocess.check_call(["g++"] + flags + ["-std=c++17", "-fPIC", "-shared", "-pthread", "-mavx2", "-mfma", "-Wno-invalid-offsetof",
                                                 "-o", path] + _SRCS)
    return path


def _lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build_host_lib())
    return _LIB


_METRICS = {"l2": 0, "ip": 2}  # nann_scorer_kind (include/nann_hip.h): the scorer the index is searched with


def _metric_kind(metric):
    if not isinstance(metric, str) or metric not in _METRICS:
        raise ValueError(f"metric must be 'l2' or 'ip', not {metric!r}")
    return _METRICS[metric]


def build_hnsw(embeddings, num_neighbors=32, ef_construction=40, seed=0, n_threads=None, metric="l2"):
    """-> dict(levels i32[N], offsets i64[N+1], neighbors i32[slots], cum_nneighbor_per_level),
    the arrays build_hnsw_index.py:36-39 reads from faiss' `index.hnsw`.  metric: "l2", or "ip" for an index that is searched
    with the inner-product scorer -- rows are linked by dist(a, b) = -<a, b> (Faiss' METRIC_INNER_PRODUCT)."""
    kind = _metric_kind(metric)
    x = np.ascontiguousarray(embeddings, dtype=np.float32)
    n, d = x.shape
    if n_threads is None:
        n_threads = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 1
    levels = np.zeros(n, np.int32)
    offsets = np.zeros(n + 1, np.int64)
    cum = np.zeros(64, np.int32)
    n_slots, max_levels = C.c_int64(0), C.c_int32(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    args = [p(x), C.c_int64(n), C.c_int32(d), C.c_int32(num_neighbors), C.c_int32(ef_construction),
            C.c_uint64(seed), C.c_int32(n_threads), C.c_int32(kind), p(levels), p(offsets)]
    rc = _lib().nann_hnsw_build_metric(*args, None, C.byref(n_slots), p(cum), C.byref(max_levels))
    if rc:
        raise ValueError(f"nann_hnsw_build: bad argument ({rc})")
    neighbors = np.empty(n_slots.value, np.int32)
    rc = _lib().nann_hnsw_build_metric(*args, p(neighbors), C.byref(n_slots), p(cum), C.byref(max_levels))
    if rc:
        raise ValueError(f"nann_hnsw_build: bad argument ({rc})")
    return {"levels": levels, "offsets": offsets, "neighbors": neighbors,
            "cum_nneighbor_per_level": cum[: max_levels.value + 1].copy()}


def export_levels(raw, start_level=2):
    """build_hnsw_index.py:41-66 on the raw arrays: enter points = nodes with
    `levels > start_level`; per level below it a CSR over ALL items."""
    levels, offsets, neighbors, cum = (raw["levels"], raw["offsets"], raw["neighbors"],
                                       raw["cum_nneighbor_per_level"])
    n = len(levels)
    enter_points = np.nonzero(levels > start_level)[0]                      # :45
    nb_values, nb_row_splits = [], []
    for level in range(start_level):                                         # :49
        width = int(cum[level + 1] - cum[level])
        present = levels > level                                             # :53 `level >= levels[idx]` -> empty
        slots = offsets[:-1, None] + int(cum[level]) + np.arange(width)[None, :]
        vals = neighbors[np.minimum(slots, len(neighbors) - 1)]
        keep = present[:, None] & (vals >= 0)                                # :59 drop -1 slots
        row_len = keep.sum(1)
        rs = np.zeros(n + 1, np.int64)
        np.cumsum(row_len, out=rs[1:])
        nb_values.append(vals[keep].astype(np.int64))                        # :66 int64 on disk
        nb_row_splits.append(rs)
    return {"enter_points": enter_points, "nb_values": nb_values, "nb_row_splits": nb_row_splits}


def build_and_save_index(embeddings, start_level, num_neighbors, output_dir, seed=0, n_threads=None, metric="l2"):
    """Same name and arguments as the reference's function (build_hnsw_index.py:33); metric as build_hnsw's."""
    raw = build_hnsw(embeddings, num_neighbors=num_neighbors, seed=seed, n_threads=n_threads, metric=metric)
    ex = export_levels(raw, start_level)
    os.makedirs(output_dir, exist_ok=True)
    np.save(os.path.join(output_dir, "enter_points.npy"), ex["enter_points"])
    for level in range(start_level):
        np.save(os.path.join(output_dir, f"neighbors_level_{level}_values.npy"), ex["nb_values"][level])
        np.save(os.path.join(output_dir, f"neighbors_level_{level}_row_splits.npy"), ex["nb_row_splits"][level])
    return raw, ex


# ---- construction on the device (csrc/nann_hnsw_build.hip) -----------------------------------------------------
def _export_torch(levels, adj0, up_row, adj_up, m, start_level):
    """build_hnsw_index.py:41-66 on the device builder's arrays, assembled with torch on the device -> numpy"""
    import torch
    n = len(levels)
    lev = torch.as_tensor(levels, device=adj0.device)
    out = {"levels": levels, "enter_points": np.nonzero(levels > start_level)[0],  # build_hnsw_index.py:45
           "nb_values": [], "nb_row_splits": []}
    for level in range(start_level):                                              # :49
        if level == 0:
            rows = adj0
        else:  # row of node i on level l >= 1: up_row[i] + l - 1 (absent: an empty row, :53)
            rows = torch.full((n, m), -1, dtype=torch.int32, device=adj0.device)
            has = lev > level
            rows[has] = adj_up[(up_row[has] + (level - 1)).long()]
        keep = rows >= 0                                                          # :59 drop the -1 slots
        rs = torch.zeros(n + 1, dtype=torch.int64, device=adj0.device)
        torch.cumsum(keep.sum(1), 0, out=rs[1:])
        out["nb_values"].append(rows[keep].to(torch.int64).cpu().numpy())         # :66 int64 on disk
        out["nb_row_splits"].append(rs.cpu().numpy())
    return out


def _device_api():
    """what every device call below starts with: torch, the library, and ops' call helpers"""
    import torch
    from . import _lib
    from .ops import _check, _ptr, _stream, _DT
    return torch, _lib.lib(), _check, _ptr, _stream, _DT


def _graph_arrays(n, n_up, m, device, fill=None):
    """new i32 tensors adj0 [n, 2m], up_row [n], adj_up [max(n_up, 1), m] on `device`: uninitialised, or full of `fill`"""
    import torch
    new = lambda *shape: (torch.empty(shape, dtype=torch.int32, device=device) if fill is None else
                          torch.full(shape, fill, dtype=torch.int32, device=device))
    return new(max(n, 1), 2 * m)[:n], new(max(n, 1))[:n], new(max(n_up, 1), m)


def _device_rows(rows, device=None):
    """rows (a tensor, or what numpy takes) -> a contiguous tensor on `device` (None: the current CUDA device)"""
    import torch
    t = rows if isinstance(rows, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(rows))
    return (t.cuda() if device is None else t.to(device=device)).contiguous()


def _state(item_embs, adj0, up_row, adj_up, levels, m, ef_construction, keep_pruned, metric):
    """the builder's own arrays on the device with what the next append, removal or export needs to know"""
    return {"item_embs": item_embs, "adj0": adj0, "up_row": up_row, "adj_up": adj_up, "levels": levels, "M": m,
            "ef_construction": int(ef_construction), "keep_pruned": bool(keep_pruned), "metric": metric}


def _result(state, start_level, want_export=True, want_state=True):
    """what the device calls return: the torch export of the arrays of `state` (or "levels" alone), and "state" itself"""
    out = (_export_torch(state["levels"], state["adj0"], state["up_row"], state["adj_up"], state["M"], start_level)
           if want_export else {"levels": state["levels"]})
    if want_state:
        out["state"] = state
    return out


def build_hnsw_gpu(item_embs, num_neighbors=32, ef_construction=40, seed=0, start_level=2, want_raw=False,
                   keep_pruned=False, want_state=False, metric="l2"):
    """HNSW(M) over the rows of `item_embs` (CUDA tensor f16 | bf16 [N, d], or a numpy f16 array) built ON THE GPU
    (nann_hnsw_build_device_metric).  Returns the export of build_hnsw_index.py:41-66 -- {"enter_points", "nb_values"
    [start_level], "nb_row_splits"[start_level], "levels"} as numpy arrays (values int64 on disk) -- assembled with
    torch on the device; with want_raw also the Faiss-shaped raw arrays of build_hnsw().  keep_pruned: the selection
    heuristic's keepPrunedConnections switch (off in Faiss, hence in the reference's graphs): rows fill up to their cap --
    the dense-graph family (mean level-0 degree ~55 of 64 instead of ~17).  want_state: also "state", the builder's own
    arrays on the device (item_embs, adj0, up_row, adj_up) with levels, M, ef_construction, keep_pruned and metric -- what
    append_hnsw_gpu() grows and export_hnsw_gpu() turns into an Index without leaving the device.  metric: "l2", or "ip" for an
    index that is searched with the inner-product scorer: rows are linked by dist(a, b) = -<a, b>.  Under "ip" the default
    heuristic leaves sparse rows (mean level-0 degree 2-3 where L2 on the same rows gives 3-4); keep_pruned fills them."""
    kind = _metric_kind(metric)
    torch, L, _check, _ptr, _stream, _DT = _device_api()
    x = _device_rows(item_embs)
    n, d = x.shape
    m = int(num_neighbors)
    levels = np.zeros(n, np.int32)
    n_up = C.c_int64(0)
    _check(L.nann_hnsw_draw_levels(C.c_int64(n), C.c_int32(m), C.c_uint64(seed), levels.ctypes.data_as(C.c_void_p),
                                   C.byref(n_up)), "hnsw levels")
    adj0, up_row, adj_up = _graph_arrays(n, n_up.value, m, x.device)
    torch.cuda.synchronize()
    _check(L.nann_hnsw_build_device_metric(_ptr(x), n, d, _DT[x.dtype], m, int(ef_construction), 1 if keep_pruned else 0, kind,
                                           levels.ctypes.data_as(C.c_void_p), _ptr(adj0), _ptr(up_row), _ptr(adj_up), _stream()),
           "hnsw build")
    out = _result(_state(x, adj0, up_row, adj_up, levels, m, ef_construction, keep_pruned, metric), start_level, want_state=want_state)
    if want_raw:
        cum = np.concatenate([[0], 2 * m + m * np.arange(int(levels.max()))]).astype(np.int32)
        offsets = np.zeros(n + 1, np.int64)
        np.cumsum(2 * m + (levels.astype(np.int64) - 1) * m, out=offsets[1:])
        nb = np.full(int(offsets[-1]), -1, np.int32)
        a0, au, ur = adj0.cpu().numpy(), adj_up.cpu().numpy(), up_row.cpu().numpy()
        nb[(offsets[:-1, None] + np.arange(2 * m)[None, :]).ravel()] = a0.ravel()
        for i in np.nonzero(levels > 1)[0]:
            for l in range(1, levels[i]):
                nb[offsets[i] + cum[l]: offsets[i] + cum[l] + m] = au[ur[i] + l - 1]
        out["raw"] = {"levels": levels, "offsets": offsets, "neighbors": nb, "cum_nneighbor_per_level": cum}
    return out


def append_hnsw_gpu(state, new_rows, seed, start_level=2, want_export=True):
    """Append `new_rows` ([n_new, d], the dtype of the state's rows) to the graph of `state` (build_hnsw_gpu(want_state=True)
    or an earlier append) ON THE GPU (nann_hnsw_append_device_metric, with the state's "metric"; a state without one is "l2").  The rows are concatenated and the three arrays grown into NEW
    tensors: the input state is left as it is, so an index still serving from it is safe (back-links rewrite old rows).  The
    new nodes' levels are drawn with `seed`.  Returns what build_hnsw_gpu(want_state=True) returns, over the grown corpus;
    want_export=False: {"levels", "state"} only, without the torch export and its copy to the host -- the live path, which goes
    on with export_hnsw_gpu(state) on the device."""
    torch, L, _check, _ptr, _stream, _DT = _device_api()
    metric = state.get("metric", "l2")
    kind = _metric_kind(metric)
    x0, m = state["item_embs"], int(state["M"])
    n_old, d = x0.shape
    new = _device_rows(new_rows, x0.device).reshape(-1, d)
    if new.dtype != x0.dtype:
        raise ValueError(f"append_hnsw_gpu: rows are {new.dtype}, the graph's are {x0.dtype}")
    n_new = new.shape[0]
    x = torch.cat([x0, new]).contiguous()
    new_levels = np.zeros(n_new, np.int32)
    if n_new:
        _check(L.nann_hnsw_draw_levels(C.c_int64(n_new), C.c_int32(m), C.c_uint64(seed), new_levels.ctypes.data_as(C.c_void_p),
                                       None), "hnsw levels")
    levels = np.ascontiguousarray(np.concatenate([np.asarray(state["levels"], np.int32), new_levels]))
    n = n_old + n_new
    n_up_old, n_up = int((levels[:n_old] - 1).sum()), int((levels.astype(np.int64) - 1).sum())
    adj0, up_row, adj_up = _graph_arrays(n, n_up, m, x.device, fill=-1)
    adj0[:n_old], up_row[:n_old], adj_up[:n_up_old] = state["adj0"], state["up_row"], state["adj_up"][:n_up_old]
    torch.cuda.synchronize()
    _check(L.nann_hnsw_append_device_metric(_ptr(x), n_old, n_new, d, _DT[x.dtype], m, int(state["ef_construction"]),
                                            1 if state["keep_pruned"] else 0, kind, levels.ctypes.data_as(C.c_void_p), _ptr(adj0),
                                            _ptr(up_row), _ptr(adj_up), _stream()), "hnsw append")
    return _result(_state(x, adj0, up_row, adj_up, levels, m, state["ef_construction"], state["keep_pruned"], metric), start_level, want_export)


def _remove_bits(n, remove_rows, deny_bits, dev):
    """the removal bitmap of remove_hnsw_gpu: i32[ceil(n / 32)] on `dev`, bit (r & 31) of word (r >> 5) = row r is removed"""
    import torch
    if (remove_rows is None) == (deny_bits is None):
        raise ValueError("remove_hnsw_gpu: give exactly one of remove_rows and deny_bits")
    words = (n + 31) // 32
    if deny_bits is not None:
        b = deny_bits if isinstance(deny_bits, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(deny_bits))
        if b.dtype != torch.bool:  # packed words, as retrieval.make_filter(...).deny_bits
            if b.dtype not in (torch.int32, torch.uint32) or b.numel() != words:
                raise ValueError(f"remove_hnsw_gpu: deny_bits is a bool mask [n] or {words} packed 32-bit words")
            return b.view(torch.int32).to(dev).contiguous()
        if b.numel() != n:
            raise ValueError(f"remove_hnsw_gpu: the mask has {b.numel()} entries, the graph {n} rows")
        flags = torch.zeros(words * 32, dtype=torch.bool, device=dev)
        flags[:n] = b.reshape(-1).to(dev)
    else:
        r = remove_rows if isinstance(remove_rows, torch.Tensor) else torch.as_tensor(np.asarray(remove_rows, dtype=np.int64))
        r = r.reshape(-1).to(device=dev, dtype=torch.int64)
        flags = torch.zeros(words * 32, dtype=torch.bool, device=dev)
        flags[r[(r >= 0) & (r < n)]] = True  # rows outside the graph remove nothing; a row named twice is removed once
    w = (flags.view(words, 32).to(torch.int64) << torch.arange(32, dtype=torch.int64, device=dev)).sum(1)
    return torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32).contiguous()


def remove_hnsw_gpu(state, remove_rows=None, deny_bits=None, start_level=2, want_export=True):
    """Remove rows from the graph of `state` (build_hnsw_gpu(want_state=True), an append or an earlier removal) ON THE GPU
    (nann_hnsw_remove_count / nann_hnsw_remove_device, with the state's "metric"; a state without one is "l2").  Exactly one of
    remove_rows (an integer array or tensor of internal rows; rows outside the graph are dropped, duplicates allowed) and
    deny_bits (a bool mask [n], or the packed words of retrieval.make_filter(...).deny_bits as they are).  The survivors are
    renumbered in order, rows that lost an entry are repaired from their removed neighbours' rows (one hop; include/nann_hip.h),
    and everything goes into NEW tensors: the input state is left as it is.  Returns what append_hnsw_gpu returns, over the
    survivors ("state" holds item_embs gathered by kept_rows), and "kept_rows" (device i32[n_keep]: the old row of every new
    row, for the caller's item_ids) and "stats" (i64[4]: rows repaired, level-0 rows that came out empty, rows whose pool
    exceeded 64, survivors).  No back-links are added, isolated nodes are counted and not healed, and the entry layer (survivors
    with levels > start_level) is the caller's to watch.  want_export=False skips the torch export, as in the append."""
    torch, L, _check, _ptr, _stream, _DT = _device_api()
    metric = state.get("metric", "l2")
    kind = _metric_kind(metric)
    x0, m = state["item_embs"], int(state["M"])
    n, d = x0.shape
    dev = x0.device
    old_levels = np.ascontiguousarray(state["levels"], dtype=np.int32)
    bits = _remove_bits(n, remove_rows, deny_bits, dev)
    kept = torch.empty(n, dtype=torch.int32, device=dev)
    new_levels = np.zeros(n, np.int32)
    n_keep, n_up = C.c_int64(0), C.c_int64(0)
    torch.cuda.synchronize()
    _check(L.nann_hnsw_remove_count(_ptr(bits), old_levels.ctypes.data_as(C.c_void_p), n, _ptr(kept),
                                    new_levels.ctypes.data_as(C.c_void_p), C.byref(n_keep), C.byref(n_up), _stream()), "hnsw remove count")
    nk = n_keep.value
    adj0, up_row, adj_up = _graph_arrays(nk, n_up.value, m, dev)
    stats = (C.c_int64 * 4)()
    _check(L.nann_hnsw_remove_device(_ptr(x0), n, d, _DT[x0.dtype], m, 1 if state["keep_pruned"] else 0, kind,
                                     old_levels.ctypes.data_as(C.c_void_p), _ptr(state["adj0"]), _ptr(state["up_row"]),
                                     _ptr(state["adj_up"]), _ptr(bits), nk, _ptr(adj0), _ptr(up_row), _ptr(adj_up), stats, _stream()),
           "hnsw remove")
    kept, levels = kept[:nk].contiguous(), np.ascontiguousarray(new_levels[:nk])
    x = x0[kept.long()].contiguous()
    out = _result(_state(x, adj0, up_row, adj_up, levels, m, state["ef_construction"], state["keep_pruned"], metric), start_level, want_export)
    out["kept_rows"] = kept
    out["stats"] = np.array(list(stats), np.int64)
    return out


def update_hnsw_gpu(state, rows, new_rows=None, start_level=2, want_export=True):
    """Refresh rows of the graph of `state` IN PLACE ON THE GPU (nann_hnsw_update_device, with the state's "metric"; a state
    without one is "l2"): every row keeps its number and its levels, so filters, candidate lists and the caller's item_ids stay
    valid.  rows: an integer array or tensor of internal rows.  new_rows ([len(rows), d], the dtype of the state's rows): their
    new embeddings, row i of new_rows for rows[i]; a row outside the graph or named twice is a ValueError, so is another dtype.
    new_rows=None relinks the rows with the embeddings as they are -- the heal of a removal: update_hnsw_gpu(state,
    orphan_rows_gpu(state)) --; rows outside the graph are then dropped and duplicates allowed, as in remove_hnsw_gpu.  The marked
    nodes are detached (rows that named them are repaired as a removal repairs them) and inserted again as an append inserts
    (include/nann_hip.h).  Everything goes into NEW tensors: the input state is left as it is, "item_embs" of the result is a new
    tensor with the rows replaced.  Returns what append_hnsw_gpu returns, and "stats" (i64[4]: rows repaired by the detach, level-0
    rows of staying nodes that came out of it empty, rows whose pool exceeded 64, rows updated).  Marking every row is refused:
    that is a build."""
    torch, L, _check, _ptr, _stream, _DT = _device_api()
    metric = state.get("metric", "l2")
    kind = _metric_kind(metric)
    x0, m = state["item_embs"], int(state["M"])
    n, d = x0.shape
    dev = x0.device
    levels = np.ascontiguousarray(state["levels"], dtype=np.int32)
    r = rows if isinstance(rows, torch.Tensor) else torch.as_tensor(np.asarray(rows, dtype=np.int64))
    r = r.reshape(-1).to(device=dev, dtype=torch.int64)
    x = x0.clone()
    if new_rows is not None:
        new = _device_rows(new_rows, dev).reshape(-1, d)
        if new.dtype != x0.dtype:
            raise ValueError(f"update_hnsw_gpu: rows are {new.dtype}, the graph's are {x0.dtype}")
        if new.shape[0] != r.numel():
            raise ValueError(f"update_hnsw_gpu: {r.numel()} rows named, {new.shape[0]} new rows given")
        if r.numel() and (int(r.min()) < 0 or int(r.max()) >= n):
            raise ValueError("update_hnsw_gpu: a row outside the graph")
        if torch.unique(r).numel() != r.numel():
            raise ValueError("update_hnsw_gpu: a row named twice")
        x[r] = new
    bits = _remove_bits(n, r, None, dev)
    n_up = int((levels.astype(np.int64) - 1).sum())
    adj0, up_row, adj_up = _graph_arrays(n, n_up, m, dev)
    if n_up == 0:
        adj_up.fill_(-1)  # no upper rows: the call does not write the placeholder row
    stats = (C.c_int64 * 4)()
    torch.cuda.synchronize()
    _check(L.nann_hnsw_update_device(_ptr(x), n, d, _DT[x.dtype], m, int(state["ef_construction"]), 1 if state["keep_pruned"] else 0,
                                     kind, levels.ctypes.data_as(C.c_void_p), _ptr(state["adj0"]), _ptr(state["up_row"]),
                                     _ptr(state["adj_up"]), _ptr(bits), _ptr(adj0), _ptr(up_row), _ptr(adj_up), stats, _stream()),
           "hnsw update")
    out = _result(_state(x, adj0, up_row, adj_up, levels, m, state["ef_construction"], state["keep_pruned"], metric), start_level, want_export)
    out["stats"] = np.array(list(stats), np.int64)
    return out


def orphan_rows_gpu(state):
    """The rows of the graph of `state` whose level-0 row is empty or that no level-0 row names (nann_hnsw_orphan_bits): a device
    tensor i64 of row numbers, ascending -- what update_hnsw_gpu(state, rows) relinks after a removal."""
    torch, L, _check, _ptr, _stream, _ = _device_api()
    adj0, m = state["adj0"], int(state["M"])
    n, dev = adj0.shape[0], adj0.device
    words = (n + 31) // 32
    bits = torch.empty(words, dtype=torch.int32, device=dev)
    count = C.c_int64(0)
    torch.cuda.synchronize()
    _check(L.nann_hnsw_orphan_bits(_ptr(adj0), n, m, _ptr(bits), C.byref(count), _stream()), "hnsw orphans")
    flags = ((bits.view(words, 1) >> torch.arange(32, dtype=torch.int32, device=dev)) & 1).reshape(-1)[:n]
    out = torch.nonzero(flags).reshape(-1)
    assert out.numel() == count.value
    return out


def export_hnsw_gpu(state, start_level=2):
    """The export of build_hnsw_index.py:41-66 ON THE DEVICE (nann_hnsw_export_count / _fill): {"enter_points" i32,
    "nb_values" [i32 l0, l1], "nb_row_splits" [i64 l0, l1]} as device tensors -- what retrieval.Index(...) takes as they are,
    so a grown graph reaches serving without a host round trip."""
    torch, L, _check, _ptr, _stream, _ = _device_api()
    adj0, up_row, adj_up, levels, m = state["adj0"], state["up_row"], state["adj_up"], state["levels"], int(state["M"])
    levels = np.ascontiguousarray(levels, dtype=np.int32)
    n, dev = len(levels), adj0.device
    rs = [torch.empty(n + 1, dtype=torch.int64, device=dev) for _ in range(2)]
    nnz, n_enter = (C.c_int64 * 2)(), C.c_int64(0)
    torch.cuda.synchronize()
    head = (_ptr(adj0), _ptr(up_row), _ptr(adj_up), levels.ctypes.data_as(C.c_void_p), n, m, int(start_level), _ptr(rs[0]), _ptr(rs[1]))
    _check(L.nann_hnsw_export_count(*head, nnz, C.byref(n_enter), _stream()), "hnsw export count")
    vals = [torch.empty(max(int(nnz[l]), 1), dtype=torch.int32, device=dev)[:int(nnz[l])] for l in range(2)]
    enter = torch.empty(max(n_enter.value, 1), dtype=torch.int32, device=dev)[:n_enter.value]
    _check(L.nann_hnsw_export_fill(*head, nnz, _ptr(vals[0]), _ptr(vals[1]), _ptr(enter), _stream()), "hnsw export fill")
    return {"enter_points": enter, "nb_values": vals, "nb_row_splits": rs}
