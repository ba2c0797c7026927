"""Lloyd aggregation on the device: drop-ins for the reference's

* ``bellman_ford(method='standard')``  -- pyamg/graph.py:129-200
* ``lloyd_cluster``                    -- pyamg/graph.py:203-286
* ``lloyd_aggregation``                -- pyamg/aggregation/aggregate.py:313-421

Same signatures, same error types, and the reference's arrays bit for bit (csrc/pamg_lloyd.hip; the per-edge and per-node rules are
csrc/pamg_lloyd.h).  ``lloyd_cluster`` keeps the whole loop resident: the graph is uploaded once and one int comes back per Lloyd
iteration.  An integer ``centers`` is drawn on the host with the reference's ``np.random.permutation(n)[:centers]``, so a seeded caller
sees the same stream; the reference's first ``bellman_ford`` call, whose results it throws away, is not repeated.

The reference's Bellman-Ford is an in-place serial loop whose ties -- with ``measure='unit'`` nearly every node is tied -- go to whoever
wrote first.  That winner has a closed form which order-free rounds compute: the distances are the unique fixed point of
``d[j] = min_i (d[i] + A_ij)``; the final ``d[j]`` is written once, by the first visit of a row i that holds its own final value over a
tight edge, and row i is first visited with it in sweep ``v(i) = s_i`` if its own writer ``p_i < i``, else ``s_i + 1``, so the stamp
``(s_j, p_j)`` is the lexicographic minimum over tight i of ``(v(i), i)``; the labels follow the predecessor chains.

The closed form needs every sum to be exact: under rounding two different ``d[i]`` can give the same ``d[i] + A_ij``, and the reference
then keeps the writer of the earlier, not yet final value.  So the device path takes **exact weights only** -- every stored weight an
integer-valued float64 in [1, 2^31] with ``n * max(weight) < 2^53``, which ``measure='unit'`` always satisfies -- on a CSR matrix with
int32 indices and unique centres.  Real-valued weights (``'abs'``, ``'inv'``, ``'min'``, ``None`` on a real matrix), explicit zeros,
float32 or complex data, CSC input and ``method='balanced'`` raise ``NotImplementedError`` before anything runs or is drawn;
``aggregation.device_setup(pyamg, lloyd=True)`` then hands the call to the reference function it patched out.  The balanced variants
and ``center_nodes`` are not here: their ties depend on cluster sizes that change during the sweep.
"""
from __future__ import annotations

from warnings import warn

import numpy as np
import scipy.sparse as sp

from . import amg_core

__all__ = ["bellman_ford", "lloyd_cluster", "lloyd_aggregation"]


def _asgraph(G):
    """pyamg.graph.asgraph"""
    if not sp.issparse(G) or G.format not in ("csc", "csr"):
        G = sp.csr_array(G)
    if G.shape[0] != G.shape[1]:
        raise ValueError("expected square matrix")
    return G


def _device_graph(G, what):
    """(indptr, indices, data) of what the device path takes; NotImplementedError for everything else"""
    if G.format != "csr":
        raise NotImplementedError(f"{what} on the device takes CSR graphs")
    if G.dtype != np.float64:
        raise NotImplementedError(f"{what} on the device is float64 only (got {G.dtype})")
    if G.indptr.dtype != np.int32 or G.indices.dtype != np.int32:
        raise NotImplementedError(f"{what} on the device takes int32 index arrays")
    w = np.ascontiguousarray(G.data)
    if w.size:
        wmin, wmax = float(w.min()), float(w.max())         # (a NaN fails the comparisons; equal weights need no third pass)
        if not (1.0 <= wmin and wmax <= 2.0 ** 31 and wmin == np.floor(wmin) and (wmin == wmax or np.array_equal(w, np.floor(w)))):
            raise NotImplementedError(f"{what} on the device takes exact weights only: integer-valued, in [1, 2^31]")
        if float(G.shape[0]) * wmax >= 2.0 ** 53:
            raise NotImplementedError(f"{what} on the device takes exact weights only: n * max(weight) < 2^53")
    return np.ascontiguousarray(G.indptr), np.ascontiguousarray(G.indices), w


def _unique(centers, what):
    if np.unique(centers).size != centers.size:
        raise NotImplementedError(f"{what} on the device takes unique centers")


def bellman_ford(G, centers, method="standard", tiebreaking=True, info=None):
    """pyamg.graph.bellman_ford(method='standard'): (distances, nearest, predecessors) of the shortest paths from the centers along the
    stored edges.  ``info``: a list that receives (distance rounds, stamp rounds)."""
    G = _asgraph(G)
    n = G.shape[0]
    if G.nnz > 0:
        if G.data.min() < 0:
            raise ValueError("Bellman-Ford is defined only for positive weights.")
    if G.dtype == complex:
        raise ValueError("Bellman-Ford is defined only for real weights.")
    if method == "balanced":
        raise NotImplementedError("bellman_ford(method='balanced') is not on the device path: its ties depend on cluster sizes that change "
                                  "during the sweep")
    if method != "standard":
        raise ValueError(f"Method {method} is not supported in Bellman-Ford")
    Gp, Gj, Gx = _device_graph(G, "bellman_ford")
    centers = np.ascontiguousarray(np.asarray(centers, dtype=np.int32))
    if centers.ndim != 1:
        raise NotImplementedError("bellman_ford on the device takes a one-dimensional list of centers")
    if centers.size and centers.min() < 0:
        raise NotImplementedError("bellman_ford on the device takes center indices from 0 (NumPy wraps negative ones in the reference)")
    if centers.size and centers.max() >= n:
        raise IndexError(f"index {centers.max()} is out of bounds for axis 0 with size {n}")    # the reference's distances[centers] = 0
    _unique(centers, "bellman_ford")
    num_clusters = len(centers)
    distances = np.full(n, np.inf, dtype=G.dtype)
    nearest = np.full(n, -1, dtype=np.int32)
    predecessors = np.full(n, -1, dtype=np.int32)
    distances[centers] = 0
    nearest[centers] = np.arange(num_clusters)
    amg_core.bellman_ford(n, Gp, Gj, Gx, centers, distances, nearest, predecessors, info=info)
    return distances, nearest, predecessors


def lloyd_cluster(G, centers, maxiter=5, info=None):
    """pyamg.graph.lloyd_cluster: (clusters, centers) after up to ``maxiter`` Lloyd iterations.  As in the reference the clusters are
    those of the last iteration's Bellman-Fords, computed before its centre update, and the centers those after it.  ``info``: a list
    that receives (Lloyd iterations, distance rounds, stamp rounds, centres moved in the last iteration)."""
    G = _asgraph(G)
    n = G.shape[0]
    if G.dtype.kind == "c":
        raise NotImplementedError("lloyd_cluster on the device is float64 only (got a complex graph)")
    if G.nnz > 0:
        if G.data.min() < 0:
            raise ValueError("Lloyd Clustering is defined only for positive weights.")
    Gp, Gj, Gx = _device_graph(G, "lloyd_cluster")          # before the draw: a refused call has not touched the random stream
    if np.isscalar(centers):
        centers = np.random.permutation(n)[:centers]
        centers = np.int32(centers)
    else:
        centers = np.asarray(centers, dtype=np.int32)
    num_clusters = len(centers)
    if num_clusters < 1:
        raise ValueError("at least one center is required")
    if centers.min() < 0:
        raise ValueError(f"invalid center index {centers.min()}")
    if centers.max() >= n:
        raise ValueError(f"invalid center index {centers.max()}")
    if centers.ndim != 1 or not centers.flags.c_contiguous:
        raise NotImplementedError("lloyd_cluster on the device takes a contiguous one-dimensional array of centers")
    _unique(centers, "lloyd_cluster")
    clusters = np.empty(n, dtype=np.int32)
    amg_core.lloyd_cluster(n, Gp, Gj, Gx, centers, maxiter, clusters, info=info)
    return clusters, centers


def lloyd_aggregation(C, ratio=0.1, measure="unit", maxiter=5, info=None):
    """pyamg.aggregation.aggregate.lloyd_aggregation: (AggOp, centers).  ``info`` as for ``lloyd_cluster``."""
    if not sp.issparse(C) or C.format not in ("csc", "csr"):
        raise TypeError("Expected csr_array or csc_array.")
    if C.shape[0] != C.shape[1]:
        raise ValueError("graph should be a square matrix.")
    if ratio <= 0 or ratio > 1:
        raise ValueError("ratio must be > 0.0 and <= 1.0")
    n = C.shape[0]
    naggs = int(min(max(ratio * n, 1), n))
    data = C.data
    if measure is None:
        data = C.data
    elif measure == "abs":
        data = np.abs(C.data)
    elif measure == "inv":
        data = 1.0 / abs(C.data)
    elif measure == "unit":
        data = np.ones_like(C.data).astype(float)
    elif measure == "min":
        data = C.data - C.data.min()
    else:
        raise ValueError(f"Unrecognized value measure={measure}")
    if C.dtype == complex:
        data = np.real(data)
    if len(data) > 0:
        if data.min() < 0:
            raise ValueError("Lloyd aggregation requires a positive measure.")
    if C.dtype.kind == "c":
        raise NotImplementedError("lloyd_aggregation on the device is float64 only (got a complex matrix)")
    G = C.__class__((data, C.indices, C.indptr), shape=C.shape)
    clusters, centers = lloyd_cluster(G, naggs, maxiter=maxiter, info=info)
    if np.any(clusters < 0):
        warn("Lloyd aggregation encountered a point that is unaggregated.")
    if clusters.min() < 0:
        warn("Lloyd clustering did not cluster every point")
    # what coo_array((ones, (row, col)), shape=(n, naggs)).tocsr() yields: one entry per aggregated row, in row order
    member = clusters >= 0
    indptr = np.concatenate(([0], np.cumsum(member))).astype(C.indices.dtype)
    indices = clusters[member].astype(C.indices.dtype, copy=False)
    AggOp = sp.csr_array((np.ones(indices.size, dtype=np.int32), indices, indptr), shape=(n, naggs))
    return AggOp, centers
