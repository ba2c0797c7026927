"""The setup of approximate ideal restriction (AIR) AMG for BLOCK (BSR) operators on the device: drop-ins for the reference's

* ``classical_strength_of_connection(block=True)``  -- pyamg/strength.py:114-245 on BSR: every block reduced to one number by 'abs',
  'min' or 'fro' (:200-214), then the classical measure on the block pattern
* ``one_point_interpolation``                       -- pyamg/classical/interpolate.py:241-321 on BSR: the one-point rule on the block
  strength matrix, identity blocks
* ``local_air``                                     -- interpolate.py:324-426 on BSR (amg_core air.h:378-584): per C-point one dense
  system of order N * b with b right-hand sides -- one Householder QR, then ``Q^T b`` and the triangular solve per right-hand side

Same signatures, same error types, same return formats, and the reference's arrays bit for bit (csrc/pamg_air_block.hip; the per-row
arithmetic is csrc/pamg_air_block.h over csrc/pamg_air.h).  The block measure is a kernel of its own; its result goes through the
classical strength kernels of ``pyamg_amd.classical`` on the block pattern, pass 1 and the one-point rule are the scalar kernels of
``pyamg_amd.air`` on that pattern, and ``R.eliminate_zeros()`` stays with SciPy on the host, where the reference has it.

Float64 BSR operators with square blocks of 1 .. 8.  ``norm='fro'`` with blocks of 8 raises ``NotImplementedError``: NumPy sums eight
squares with eight accumulators there, and that order is not reproduced (up to 7 its order is the plain one the kernel uses).  What the
device path does not take -- CSR and other formats (they are ``pyamg_amd.air``'s and ``pyamg_amd.classical``'s), other dtypes, non-square
blocks or blocks beyond 8, ``block=False`` (the reference converts and amalgamates there), ``use_gmres=True``, index arrays beyond
int32 -- raises ``NotImplementedError``; ``aggregation.device_setup(pyamg, block_air=True)`` then hands the call to the function it
patched out: the CSR function of ``air=True`` when that keyword is on, and the reference's otherwise.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from . import amg_core
from .air import _splitting
from .classical import _i32

__all__ = ["classical_strength_of_connection", "one_point_interpolation", "local_air"]

MAX_BLOCK = 8


def _bsr_f64(A, what):
    """(blocksize, block rows, indptr, indices, values of the stored blocks as one flat array) of a float64 BSR operator"""
    if A.format != "bsr":
        raise NotImplementedError(f"{what} on the block device path takes BSR operators")
    if A.dtype != np.float64:
        raise NotImplementedError(f"{what} on the device is float64 only (got {A.dtype})")
    b = int(A.blocksize[0])
    if A.blocksize[0] != A.blocksize[1] or not 1 <= b <= MAX_BLOCK:
        raise NotImplementedError(f"{what} on the device takes square blocks of 1 .. {MAX_BLOCK} (got {tuple(A.blocksize)})")
    if A.shape[0] != A.shape[1]:
        raise NotImplementedError(f"{what} on the device takes a square operator")
    Ap, Aj = _i32(A.indptr), _i32(A.indices)
    Ax = np.ascontiguousarray(A.data[:Aj.size], dtype=np.float64).reshape(-1)
    return b, A.shape[0] // b, Ap, Aj, Ax


def classical_strength_of_connection(A, theta=0.1, block=True, norm="abs"):
    """pyamg.strength.classical_strength_of_connection on a BSR operator with ``block=True``: the classical measure of the block
    pattern with every block reduced to its largest magnitude ('abs'), its smallest entry ('min') or the sum of its squares ('fro');
    a CSR matrix of one row per block row, magnitudes scaled by each row's largest entry, without exact zeros."""
    what = "classical_strength_of_connection"
    if not sp.issparse(A):
        raise NotImplementedError(f"{what} on the block device path takes BSR operators")
    b, N, Ap, Aj, Ax = _bsr_f64(A, what)
    if theta < 0 or theta > 1:
        raise ValueError("expected theta in [0,1]")
    if not block:
        raise NotImplementedError(f"{what}(block=False) on a BSR operator is not on the device path")
    if norm not in amg_core.BLOCK_NORMS:
        raise ValueError("Invalid choice of norm.")
    if norm == "fro" and b == MAX_BLOCK:
        raise NotImplementedError(f"{what}(norm='fro') with blocks of {MAX_BLOCK} is not on the device path")
    data = np.empty(Aj.size, dtype=np.float64)
    amg_core.block_strength_measure(b, norm, Ax, data)
    index_type = A.indptr.dtype
    Sp = np.empty(N + 1, dtype=np.int32)
    Sj = np.empty(Aj.size, dtype=np.int32)
    Sx = np.empty(Aj.size, dtype=np.float64)
    fn = amg_core.classical_strength_of_connection_min if norm == "min" else amg_core.classical_strength_of_connection_abs
    fn(N, theta, Ap, Aj, data, Sp, Sj, Sx)
    nnz = int(Sp[-1])
    return sp.csr_array((Sx[:nnz].copy(), Sj[:nnz].astype(index_type), Sp.astype(index_type)), shape=(N, N))


def one_point_interpolation(A, C, splitting, by_val=False):
    """pyamg.classical.interpolate.one_point_interpolation on a BSR operator: the one-point rule on the block strength matrix C --
    C-points by injection, every F-point from the C-neighbour with the largest ``|C_ij|`` -- as a BSR matrix of identity blocks
    (``by_val`` is CSR-only in the reference and is ignored here as it is there).

    The returned index and data arrays hold exactly ``indptr[-1]`` blocks; the reference's hold n with an uninitialised tail."""
    if not sp.issparse(A):
        raise TypeError("Invalid sparse matrix type, not sparse.")
    what = "one_point_interpolation"
    b, n, _, _, _ = _bsr_f64(A, what)
    if not sp.issparse(C) or C.format != "csr" or C.shape != (n, n):
        raise NotImplementedError(f"{what} on the device takes a CSR strength matrix with one row per block row of A")
    if C.dtype != np.float64:
        raise NotImplementedError(f"{what} on the device is float64 only (got {C.dtype})")
    it = A.indptr.dtype
    Cp, Cj, Cx = _i32(C.indptr), _i32(C.indices), np.ascontiguousarray(C.data, dtype=np.float64)
    split = _splitting(splitting, n, what)
    nc = np.sum(splitting)
    Pp = np.empty(n + 1, dtype=np.int32)
    Pj = np.empty(n, dtype=np.int32)
    Px = np.empty(n, dtype=np.float64)
    amg_core.one_point_interpolation(Pp, Pj, Px, Cp, Cj, Cx, split)
    nnz = int(Pp[-1])
    data = np.array(nnz * [np.identity(b, dtype=A.dtype)], dtype=A.dtype).reshape(nnz, b, b)      # interpolate.py:317, on the host
    return sp.bsr_array((data, Pj[:nnz].astype(it), Pp.astype(it, copy=False)), blocksize=[b, b], shape=[b * n, b * nc])


def local_air(A, splitting, theta=0.1, norm="abs", degree=1, use_gmres=False, maxiter=10, precondition=True):
    """pyamg.classical.interpolate.local_air on a BSR operator: the block rows of R solve ``(R A)_ij = 0`` on their own pattern -- the
    strong F-neighbours of the C-point in the block strength matrix (and theirs with ``degree=2``), ascending, followed by the identity
    block -- by the reference's Householder QR, operation for operation; entries up to 1e-15 in magnitude are stored as zero and blocks
    of zeros are eliminated afterwards.  BSR with blocksize (b, b) and shape (nc * b, n * b)."""
    if not sp.issparse(A):
        raise TypeError("Invalid sparse matrix type, not sparse.")
    what = "local_air"
    b, n, Ap, Aj, Ax = _bsr_f64(A, what)
    if use_gmres:
        raise NotImplementedError(f"{what}(use_gmres=True) is not on the device path")
    it = A.indptr.dtype
    split = _splitting(splitting, n, what)
    if not isinstance(degree, (int, np.integer)) or isinstance(degree, bool):
        raise NotImplementedError(f"{what} on the device takes an integer degree")
    C = classical_strength_of_connection(A, theta=theta, block=True, norm=norm)
    Cp, Cj, Cx = _i32(C.indptr), _i32(C.indices), np.ascontiguousarray(C.data, dtype=np.float64)
    Cpts = np.ascontiguousarray(np.where(split == 1)[0], dtype=np.int32)
    nc = Cpts.shape[0]
    Rp = np.empty(nc + 1, dtype=np.int32)
    amg_core.approx_ideal_restriction_pass1(Rp, Cp, Cj, Cpts, split, int(degree))
    nnz = int(Rp[-1])
    Rj = np.zeros(nnz, dtype=np.int32)
    Rx = np.zeros(nnz * b * b, dtype=np.float64)
    amg_core.block_approx_ideal_restriction_pass2(Rp, Rj, Rx, Ap, Aj, Ax, Cp, Cj, Cx, Cpts, split, b, int(degree), 0, int(maxiter),
                                                  int(bool(precondition)))
    R = sp.bsr_array((Rx.reshape(nnz, b, b), Rj.astype(it, copy=False), Rp.astype(it, copy=False)), blocksize=[b, b], shape=[nc * b, A.shape[0]])
    R.eliminate_zeros()
    return R
