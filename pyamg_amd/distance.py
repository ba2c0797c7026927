"""The relaxation-vector and the vertex-distance strength measures on the device: drop-ins for the reference's

* ``relaxation_vectors``               -- pyamg/strength.py:860-892
* ``affinity_distance``                -- pyamg/strength.py:895-950
* ``algebraic_distance``               -- pyamg/strength.py:953-1016
* ``distance_strength_of_connection``  -- pyamg/strength.py:24-111

Same signatures and defaults, the same ``ValueError`` texts in the same order, the same implicit-conversion warning, the same return
format, and **exactly one** ``np.random.rand(n * R)`` per call, drawn on the host: a seeded caller sees the reference's stream, as with
``classical.PMIS``.  The arrays are the reference's bit for bit.

The kernels (csrc/pamg_distance.hip; the per-row and per-entry arithmetic is csrc/pamg_distance.h) keep the whole chain of
``distance_measure_common`` resident: A and the random block go up once, all R vectors are relaxed by one launch per sweep (A is read k
times, not R k times), the measure, the removal of zero distances and the relative filter are one kernel, and one array of nnz doubles
comes back on A's pattern.  What SciPy and NumPy do around them -- the conversion of a non-CSR operator, the BSR amalgamation,
``eliminate_zeros``, ``1.0 / data``, ``+ eye``, the final row scaling -- stays on the host with the same calls.

Float64 CSR operators (anything else the reference converts is converted the same way first).  What the device path does not take --
complex or non-float64 data, a matrix without canonical format, a non-square matrix, index values beyond int32, more than 32 vectors, a
``p`` other than 1, 2 or inf (a general ``pow`` is not reproducible bit for bit), more than 8 coordinates -- raises
``NotImplementedError`` before any device call and before the random draw; ``aggregation.device_setup(pyamg, distance=True)`` then
hands the call to the reference function it patched out.
"""
from __future__ import annotations

from warnings import warn

import numpy as np
import scipy.sparse as sp

from . import _capi as capi
from . import amg_core
from .classical import _i32
from .evolution import _scale_rows_by_largest_entry

__all__ = ["relaxation_vectors", "algebraic_distance", "affinity_distance", "distance_strength_of_connection"]

MAX_R = 32
MAX_DIM = 8


def _device_takes(A, what):
    """the CSR operator as the kernels want it: (indptr, indices) as int32; NotImplementedError for what the device path does not take"""
    if A.dtype != np.float64:
        raise NotImplementedError(f"{what} on the device is float64 only (got {A.dtype})")
    if A.shape[0] != A.shape[1]:
        raise NotImplementedError(f"{what} on the device takes a square operator")
    if not A.has_canonical_format:
        raise NotImplementedError(f"{what} on the device takes a matrix in canonical format")
    return _i32(A.indptr), _i32(A.indices)


def _vectors_taken(R, what):
    if R > MAX_R:
        raise NotImplementedError(f"{what} on the device takes at most {MAX_R} vectors (got {R})")


def _random_block(n, R):
    """the reference's draw (strength.py:882-883): the n x R block in column ordering, and the flat view the kernels relax in place"""
    x = np.random.rand(n * R) - 0.5
    x = np.reshape(x, (n, R), order="F")
    return x, x.T.reshape(-1)


def relaxation_vectors(A, R, k, alpha):
    """pyamg.strength.relaxation_vectors: R random vectors relaxed by k weighted-Jacobi sweeps on ``A x = 0``, all R in one launch per
    sweep.  ``A`` is a float64 CSR operator, ``R`` and ``k`` positive integers (the callers have checked them)."""
    what = "relaxation_vectors"
    if not sp.issparse(A) or A.format != "csr":
        raise NotImplementedError(f"{what} on the device takes a CSR operator")
    if not isinstance(R, (int, np.integer)) or not isinstance(k, (int, np.integer)) or R < 1 or k < 0:
        raise NotImplementedError(f"{what} on the device takes a positive number of vectors and of sweeps")
    Ap, Aj = _device_takes(A, what)
    _vectors_taken(R, what)
    n = A.shape[0]
    x, flat = _random_block(n, R)
    amg_core.relaxation_vectors(Ap, Aj, np.ascontiguousarray(A.data), flat, n, R, k, alpha)
    return x


def _distance_measure_common(A, measure, alpha, R, k, epsilon, what):
    """strength.py:1019-1072 with its func(x) one of the device measures"""
    Ap, Aj = _device_takes(A, what)
    _vectors_taken(R, what)
    n = A.shape[0]
    _, flat = _random_block(n, R)
    Dx = np.empty(A.nnz, dtype=np.float64)
    amg_core.distance_strength(capi.DISTANCE[measure], Ap, Aj, np.ascontiguousarray(A.data), flat, n, R, k, alpha, epsilon, Dx)
    # on A's pattern: the diagonal, stored zeros, zero distances and what the filter dropped are 0.0
    C = sp.csr_array((Dx, Aj.copy(), Ap.copy()), shape=A.shape)
    C.eliminate_zeros()
    C.data = 1.0 / C.data
    C = C + sp.eye_array(C.shape[0], C.shape[1], format="csr")
    return _scale_rows_by_largest_entry(C)


def _common_checks(alpha, R, k, epsilon):
    if alpha < 0:
        raise ValueError("expected alpha>0")
    if R <= 0 or not isinstance(R, int):
        raise ValueError("expected integer R>0")
    if k <= 0 or not isinstance(k, int):
        raise ValueError("expected integer k>0")
    if epsilon < 1:
        raise ValueError("expected epsilon>1.0")


def affinity_distance(A, alpha=0.5, R=5, k=20, epsilon=4.0):
    """pyamg.strength.affinity_distance: ``1 - (x_i . x_j)^2 / ((x_i . x_i) (x_j . x_j))`` over R relaxed random vectors, filtered
    relative to the smallest distance of each row"""
    if not sp.issparse(A) or A.format != "csr":
        A = sp.csr_array(A)
    _common_checks(alpha, R, k, epsilon)
    return _distance_measure_common(A, "affinity", alpha, R, k, epsilon, "affinity_distance")


def algebraic_distance(A, alpha=0.5, R=5, k=20, epsilon=2.0, p=2):
    """pyamg.strength.algebraic_distance: the p-norm (p = 1, 2 or inf on the device) of ``x_i - x_j`` over R relaxed random vectors,
    filtered relative to the smallest distance of each row"""
    if not sp.issparse(A) or A.format != "csr":
        A = sp.csr_array(A)
    _common_checks(alpha, R, k, epsilon)
    if p < 1:
        raise ValueError("expected p>1 or equal to numpy.inf")
    if p == 1:
        measure = "algebraic_p1"
    elif p == 2:
        measure = "algebraic_p2"
    elif p == np.inf:
        measure = "algebraic_pinf"
    else:
        raise NotImplementedError(f"algebraic_distance on the device takes p = 1, 2 or inf (got {p})")
    return _distance_measure_common(A, measure, alpha, R, k, epsilon, "algebraic_distance")


def distance_strength_of_connection(A, V, theta=2.0, relative_drop=True):
    """pyamg.strength.distance_strength_of_connection: ``C(i, j)`` from the distance of the vertices ``V[i]`` and ``V[j]`` on the pattern
    of A (of its blocks, for a BSR operator), filtered per row relative to the closest vertex or by the absolute distance ``theta``"""
    what = "distance_strength_of_connection"
    if sp.issparse(A) and A.format == "bsr":
        sn = int(A.shape[0] / A.blocksize[0])
        u = np.ones((A.data.shape[0],))
        A = sp.csr_array((u, A.indices, A.indptr), shape=(sn, sn))

    if not sp.issparse(A) or A.format != "csr":
        warn("Implicit conversion of A to csr", sp.SparseEfficiencyWarning)
        A = sp.csr_array(A)

    dim = V.shape[1]
    if not isinstance(V, np.ndarray) or V.ndim != 2 or V.dtype != np.float64:
        raise NotImplementedError(f"{what} on the device takes a float64 n x dim array of coordinates")
    if dim < 1 or dim > MAX_DIM:
        raise NotImplementedError(f"{what} on the device takes 1 to {MAX_DIM} coordinates (got {dim})")
    if V.shape[0] < A.shape[0]:
        raise NotImplementedError(f"{what} on the device takes coordinates for every vertex")
    Ap, Aj = _device_takes(A, what)
    n = A.shape[0]

    Cx = np.empty(A.nnz, dtype=np.float64)
    amg_core.vertex_distance(Ap, Aj, np.ascontiguousarray(V).reshape(-1), n, dim, Cx)
    C = sp.csr_array((Cx, A.indices.copy(), A.indptr.copy()), shape=A.shape)

    if relative_drop is True:
        if theta != np.inf:
            amg_core.apply_distance_filter(C.shape[0], theta, _i32(C.indptr), _i32(C.indices), C.data)
    else:
        amg_core.apply_absolute_distance_filter(C.shape[0], theta, _i32(C.indptr), _i32(C.indices), C.data)
    C.eliminate_zeros()

    C = C + sp.eye_array(C.shape[0], C.shape[1], format="csr")
    C.data = 1.0 / C.data
    return _scale_rows_by_largest_entry(C)
