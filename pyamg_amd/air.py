"""The setup of approximate ideal restriction (AIR) AMG on the device: drop-ins for the reference's

* ``one_point_interpolation``  -- pyamg/classical/interpolate.py:241-321 (amg_core air.h:46-98)
* ``local_air``                -- interpolate.py:324-426 (air.h:124-327, the least-squares solve of linalg.h:1172-1472)

Same signatures, same error types, same return formats, and the reference's arrays bit for bit (csrc/pamg_air.hip; the per-row arithmetic
is csrc/pamg_air.h).  The strength matrix of ``local_air`` comes from ``pyamg_amd.classical``, and ``R.eliminate_zeros()`` stays with SciPy
on the host, where the reference has it.

Float64 CSR operators; BSR operators have a module of their own, ``pyamg_amd.block_air`` (``device_setup(pyamg, block_air=True)``), and
are refused here.  What the device path does not take (other formats and dtypes, ``use_gmres=True``, index arrays beyond int32) raises
``NotImplementedError``; ``aggregation.device_setup(pyamg, air=True)`` then hands the call to the reference function it patched out.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from . import amg_core
from .classical import _f64, _i32, classical_strength_of_connection

__all__ = ["one_point_interpolation", "local_air"]


def _csr_f64(M, what, name):
    if not sp.issparse(M) or M.format != "csr":
        raise NotImplementedError(f"{what} on the device takes a CSR {name}")
    return _i32(M.indptr), _i32(M.indices), _f64(M, what)


def _splitting(splitting, n, what):
    s = np.asarray(splitting)
    if s.ndim != 1 or s.size != n or s.dtype.kind not in "iub":
        raise NotImplementedError(f"{what} on the device takes one integer splitting entry per row")
    return np.ascontiguousarray(s, dtype=np.int32)


def one_point_interpolation(A, C, splitting, by_val=False):
    """pyamg.classical.interpolate.one_point_interpolation: C-points by injection, every F-point from the C-neighbour with the largest
    ``|C_ij|`` (the first stored one among equals) -- with weight 1, or with ``-A_ij`` searched in A when ``by_val``.  An F-point
    without a C-neighbour gets an empty row.

    The returned index and data arrays hold exactly ``indptr[-1]`` entries; the reference's have length n with an uninitialised tail
    (and, with ``by_val=True``, uninitialised values in the C-rows, which are 1.0 here)."""
    if not sp.issparse(A):
        raise TypeError("Invalid sparse matrix type, not sparse.")
    what = "one_point_interpolation"
    if A.format != "csr":
        raise NotImplementedError(f"{what} on the device takes CSR operators")
    if A.dtype != np.float64:
        raise NotImplementedError(f"{what} on the device is float64 only (got {A.dtype})")
    n = A.shape[0]
    it = A.indptr.dtype
    Mp, Mj, Mx = _csr_f64(A if by_val else C, what, "operator" if by_val else "strength matrix")
    if Mp.size != n + 1:
        raise NotImplementedError(f"{what} on the device takes a strength matrix with the rows of A")
    split = _splitting(splitting, n, what)
    nc = np.sum(splitting)
    Pp = np.empty(n + 1, dtype=np.int32)
    Pj = np.empty(n, dtype=np.int32)
    Px = np.empty(n, dtype=np.float64)
    amg_core.one_point_interpolation(Pp, Pj, Px, Mp, Mj, Mx, split)
    nnz = int(Pp[-1])
    data = Px[:nnz].copy() if by_val else np.ones(nnz, dtype=A.dtype)
    return sp.csr_array((data, Pj[:nnz].astype(it), Pp.astype(it, copy=False)), shape=[n, nc])


def local_air(A, splitting, theta=0.1, norm="abs", degree=1, use_gmres=False, maxiter=10, precondition=True):
    """pyamg.classical.interpolate.local_air: the rows of R solve ``(R A)_ij = 0`` on their own pattern -- the strong F-neighbours of the
    C-point (and theirs with ``degree=2``), ascending, followed by the identity entry -- by the reference's Householder least squares,
    operation for operation; exact zeros are eliminated afterwards."""
    if not sp.issparse(A):
        raise TypeError("Invalid sparse matrix type, not sparse.")
    what = "local_air"
    if A.format != "csr":
        raise NotImplementedError(f"{what} on the device takes CSR operators")
    if use_gmres:
        raise NotImplementedError(f"{what}(use_gmres=True) is not on the device path")
    if A.shape[0] != A.shape[1]:
        raise NotImplementedError(f"{what} on the device takes a square operator")
    Ap, Aj, Ax = _csr_f64(A, what, "operator")
    n = A.shape[0]
    it = A.indptr.dtype
    split = _splitting(splitting, n, what)
    if not isinstance(degree, (int, np.integer)) or isinstance(degree, bool):
        raise NotImplementedError(f"{what} on the device takes an integer degree")
    C = classical_strength_of_connection(A, theta=theta, block=False, norm=norm)
    Cp, Cj, Cx = _i32(C.indptr), _i32(C.indices), np.ascontiguousarray(C.data, dtype=np.float64)
    Cpts = np.ascontiguousarray(np.where(split == 1)[0], dtype=np.int32)
    nc = Cpts.shape[0]
    Rp = np.empty(nc + 1, dtype=np.int32)
    amg_core.approx_ideal_restriction_pass1(Rp, Cp, Cj, Cpts, split, int(degree))
    nnz = int(Rp[-1])
    Rj = np.zeros(nnz, dtype=np.int32)
    Rx = np.zeros(nnz, dtype=np.float64)
    amg_core.approx_ideal_restriction_pass2(Rp, Rj, Rx, Ap, Aj, Ax, Cp, Cj, Cx, Cpts, split, int(degree), 0, int(maxiter), int(bool(precondition)))
    R = sp.csr_array((Rx, Rj.astype(it, copy=False), Rp.astype(it, copy=False)), shape=[nc, n])
    R.eliminate_zeros()
    return R
