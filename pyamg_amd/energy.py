"""Energy-minimisation prolongation smoothing with CG and GMRES on the device: drop-ins for the reference's

* ``satisfy_constraints``             -- pyamg/aggregation/smooth.py:17-58
* ``cg_prolongation_smoothing``       -- pyamg/aggregation/smooth.py:275-442
* ``gmres_prolongation_smoothing``    -- pyamg/aggregation/smooth.py:648-872

with the reference's signatures.  The kernels are csrc/pamg_energy.hip, their arithmetic csrc/pamg_energy.h.

``satisfy_constraints`` is the reference's bit for bit, ``U @ B`` included (it runs in the order of SciPy's ``bsr_matvecs``).

``cg_prolongation_smoothing`` runs the whole Krylov loop resident: T, expanded onto the pattern, is uploaded once and downloaded once,
and per iteration one int comes back (the loop's exit).  Everything local to a block row -- the incomplete product, ``U @ B``, the
projection, the updates -- is computed in the reference's order; the two Frobenius inner products are summed by a fixed tree over the
block rows where the reference sums in SciPy's and NumPy's order, so ``newsum`` and T agree with the reference to rounding, not bit for
bit.  The row weights ``Dinv`` are formed on the host with the reference's own expressions.  What stays with the caller
(``energy_prolongation_smoother``): ``compute_BtBinv`` and ``filter_operator`` (device paths of their own: ``pyamg_amd.rootnode``),
``get_Cpt_params``, the pattern and the filters.

The loop's head is the reference's: it runs while ``i < maxiter`` and the stored size of R exceeds ``tol`` (R's all-zero blocks not
counted, as SciPy's subtraction drops them), and leaves at the first ``newsum < tol``.

``gmres_prolongation_smoothing`` is the same for non-symmetric operators: the Krylov basis ``V_0 .. V_maxiter`` lives on the pattern's
structure in HBM, the modified Gram-Schmidt coefficients ``H[j, i] = <V_j, W>`` are taken one after the other on the already updated W
through the same fixed tree, the Hessenberg column, the Givens rotations, ``g`` and ``normr`` are the reference's real-arithmetic
statements run by one lane, and one int comes back per iteration.  The triangular solve (at most ``maxiter x maxiter``) is done on
the host, ``y`` goes up, and one kernel forms ``T + sum y[j] V_j`` and resets the C-point rows -- also when no iteration ran
(``normr <= tol``).  It runs ``while i < maxiter - 1 and normr > tol`` from ``i = -1``; the breakdown branch (``H[i+1, i] == 0.0``: no
normalisation, no rotation, ``normr = 0``) is the reference's.  T and the ``normr`` history agree with the reference to rounding.

What the device path does not take raises ``NotImplementedError`` before a device call: ``weighting='block'``, non-float64 or complex
operands, inputs that are not BSR / CSR, a pattern that does not contain T's structure (or, with root nodes, the injection's), index
arrays beyond int32, blocks larger than 6 x 6 or more than 6 candidates, and for GMRES ``maxiter`` above 32 (the basis).
``aggregation.device_setup(pyamg, energy=True)`` / ``(pyamg, energy_gmres=True)`` then hands the call to the reference function it
patched out.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from . import amg_core
from .classical import _i32

__all__ = ["satisfy_constraints", "cg_prolongation_smoothing", "gmres_prolongation_smoothing"]

MAX_BLOCK = 6
MAX_NULLDIM = 6
GMRES_MAXITER = 32                                          # the basis is maxiter + 1 arrays of the pattern's size


def _bsr(M, what):
    """M as BSR (CSR: 1 x 1 blocks), float64, int32 indices; anything else is not on the device path"""
    if not sp.issparse(M) or M.format not in ("bsr", "csr"):
        raise NotImplementedError(f"{what} on the device takes BSR or CSR operands")
    if M.dtype != np.float64:
        raise NotImplementedError(f"{what} on the device is float64 only (got {M.dtype})")
    if M.format == "csr":
        M = sp.bsr_array((M.data.reshape(-1, 1, 1), M.indices, M.indptr), shape=M.shape)
    if max(M.blocksize) > MAX_BLOCK:
        raise NotImplementedError(f"{what} on the device takes blocks up to {MAX_BLOCK} x {MAX_BLOCK} (got {M.blocksize})")
    return M


def _candidates(B, what):
    B = np.asarray(B)
    if B.dtype != np.float64 or B.ndim != 2:
        raise NotImplementedError(f"{what} on the device takes a two-dimensional float64 B (got {B.dtype}, {B.ndim} dimensions)")
    if B.shape[1] > MAX_NULLDIM:
        raise NotImplementedError(f"{what} on the device takes at most {MAX_NULLDIM} candidates (got {B.shape[1]})")
    return B


def satisfy_constraints(U, B, BtBinv):
    """pyamg.aggregation.smooth.satisfy_constraints: project the components of span(B) out of every block row of U, so that
    ``U @ B = 0``.  U (bsr_array) is modified in place and returned."""
    what = "satisfy_constraints"
    if not sp.issparse(U) or U.format != "bsr":
        raise NotImplementedError(f"{what} on the device takes a bsr_array")
    if U.dtype != np.float64 or np.asarray(BtBinv).dtype != np.float64:
        raise NotImplementedError(f"{what} on the device is float64 only")
    B = _candidates(B, what)
    r, c = U.blocksize
    if max(r, c) > MAX_BLOCK:
        raise NotImplementedError(f"{what} on the device takes blocks up to {MAX_BLOCK} x {MAX_BLOCK} (got {U.blocksize})")
    if not U.data.flags.c_contiguous:
        raise NotImplementedError(f"{what} on the device takes contiguous block data")
    n = U.shape[0] // r
    amg_core.satisfy_constraints(r, c, n, B.shape[1], np.ascontiguousarray(np.ravel(B)), np.ascontiguousarray(np.ravel(BtBinv)),
                                 _i32(U.indptr), _i32(U.indices), np.ravel(U.data))
    return U


def _expand(M, pattern, keys, order, what, fn):
    """the block values of M on the pattern's structure (zero blocks where M stores nothing); M's structure must lie inside"""
    r, c = pattern.blocksize
    if M.blocksize != (r, c) or M.shape != pattern.shape:
        raise NotImplementedError(f"{fn} on the device: {what} and the pattern differ in shape or block size")
    nbc = pattern.shape[1] // c
    rows = np.repeat(np.arange(M.indptr.size - 1, dtype=np.int64), np.diff(M.indptr))
    mk = rows * nbc + M.indices
    at = np.searchsorted(keys, mk)
    if mk.size and (at.max(initial=0) >= keys.size or not np.array_equal(keys[np.minimum(at, keys.size - 1)], mk)):
        raise NotImplementedError(f"{fn} on the device: the pattern does not contain the structure of {what}")
    out = np.zeros(pattern.data.shape, dtype=np.float64)
    out[order[at]] = M.data
    return out


def _prepare(what, A, T, B, BtBinv, pattern, weighting, Cpt_params):
    """what the Krylov drop-ins share before their device call: the checks, T (and with root nodes the injection P_I) expanded onto the
    pattern, the C-point byte per row.  Returns the arguments of ``amg_core.energy_cg`` / ``energy_gmres`` up to PIx (Dinv left out: it
    is formed after this, as the reference forms it after its allocations), the pattern and T as BSR"""
    if weighting == "block":
        raise NotImplementedError(f"{what}(weighting='block') is not on the device path")
    if weighting not in ("diagonal", "local"):
        raise ValueError("weighting value is invalid")
    A_, T_, pat = _bsr(A, what), _bsr(T, what), _bsr(pattern, what)
    B = _candidates(B, what)
    BtBinv = np.asarray(BtBinv)
    if BtBinv.dtype != np.float64:
        raise NotImplementedError(f"{what} on the device is float64 only (BtBinv: {BtBinv.dtype})")
    r, c = T_.blocksize
    if A_.blocksize != (r, r) or A_.shape[0] != A_.shape[1] or A_.shape[0] != T_.shape[0]:
        raise NotImplementedError(f"{what} on the device takes a square A whose blocks match T's rows")
    n, nbc, K = T_.shape[0] // r, T_.shape[1] // c, B.shape[1]
    if B.shape[0] != T_.shape[1] or BtBinv.size != n * K * K:
        raise NotImplementedError(f"{what} on the device: B or BtBinv do not fit T")
    Ap, Aj, Sp, Sj = _i32(A_.indptr), _i32(A_.indices), _i32(pat.indptr), _i32(pat.indices)
    _i32(T_.indptr), _i32(T_.indices)
    if pat.data.size > np.iinfo(np.int32).max:
        raise NotImplementedError("index arrays beyond int32 are not supported on the device path")

    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(pat.indptr))
    keys = rows * nbc + pat.indices
    if keys.size < 2 or np.all(keys[1:] > keys[:-1]):       # sorted rows without duplicates (what the reference's caller builds): as stored
        order = np.arange(keys.size)
    else:
        order = np.argsort(keys, kind="stable")
        keys = keys[order]
        if np.any(keys[1:] == keys[:-1]):
            raise NotImplementedError(f"{what} on the device: the pattern stores a block twice")
    Tx = _expand(T_, pat, keys, order, "T", what)
    cmask = PIx = None
    if Cpt_params is not None and Cpt_params[0]:
        P_I = Cpt_params[1]["P_I"]
        I_F = Cpt_params[1]["I_F"]
        PIx = _expand(_bsr(sp.bsr_array(P_I, blocksize=(r, c)) if sp.issparse(P_I) else P_I, what), pat, keys, order, "P_I", what).ravel()
        if not sp.issparse(I_F) or I_F.dtype != np.float64:
            raise NotImplementedError(f"{what} on the device takes I_F as a float64 sparse matrix")
        dF = I_F.diagonal()
        if I_F.count_nonzero() != np.count_nonzero(dF) or np.any((dF != 0.0) & (dF != 1.0)):        # I_F must be the identity on the F rows and nothing else
            raise NotImplementedError(f"{what} on the device takes I_F as an identity with the C-point rows removed")
        cmask = np.ascontiguousarray(dF == 0.0, dtype=np.uint8)
    head = (n, nbc, r, c, K, Ap, Aj, np.ascontiguousarray(np.ravel(A_.data)), Sp, Sj, Tx.ravel(), np.ascontiguousarray(np.ravel(B)),
            np.ascontiguousarray(np.ravel(BtBinv)))
    return head, (cmask, PIx), pat, T_


def _row_weights(A, weighting):
    """Dinv with the reference's expressions (smooth.py:332-343 and :717-728, util.utils.get_diagonal)"""
    if weighting == "diagonal":
        A.sort_indices()
        D = A.diagonal()
        Dinv = np.zeros_like(D)
        mask = D != 0.0
        Dinv[mask] = 1.0 / D[mask]
    else:
        D = np.abs(A) @ np.ones((A.shape[0], 1), dtype=A.dtype)
        Dinv = np.zeros_like(D)
        Dinv[D != 0] = 1.0 / np.abs(D[D != 0])
    return np.ascontiguousarray(np.ravel(Dinv), dtype=np.float64)


def _empty_pattern(pat):
    """R.nnz == 0 (R lives on the pattern, explicit zeros included): the reference's message; the caller returns the tentative T"""
    if pat.indices.size:
        return False
    print("Error in sa_energy_min(..).  Initial R no nonzeros on a level. "
          "Returning tentative prolongator\n")
    return True


def _smooth(what, driver, cap, A, T, B, BtBinv, pattern, maxiter, tol, weighting, Cpt_params):
    """a Krylov drop-in: the preparation, ``amg_core.<driver>`` on T expanded onto the pattern, and the result on the pattern's structure"""
    head, rooted, pat, T_ = _prepare(what, A, T, B, BtBinv, pattern, weighting, Cpt_params)
    if cap is not None and int(maxiter) > cap:
        raise NotImplementedError(f"{what} on the device keeps at most {cap} + 1 basis vectors (maxiter {maxiter})")
    Dinv = _row_weights(A, weighting)
    if _empty_pattern(pat):
        return T
    getattr(amg_core, driver)(*head, Dinv, *rooted, int(maxiter), float(tol))
    Tx = head[10]                                           # smoothed in place
    return sp.bsr_array((Tx.reshape(-1, *T_.blocksize), pat.indices.copy(), pat.indptr.copy()), shape=T_.shape)


def cg_prolongation_smoothing(A, T, B, BtBinv, pattern, maxiter, tol, weighting="local", Cpt_params=None):
    """pyamg.aggregation.smooth.cg_prolongation_smoothing: smooth T with CG on ``A T = 0`` inside ``pattern``, keeping ``T @ B``.

    Returns a ``bsr_array`` with T's block size on the pattern's structure.  The reference's SciPy additions drop all-zero blocks;
    this one may hold explicit zero blocks, which the caller's ``T.eliminate_zeros()`` removes (``energy_prolongation_smoother`` calls
    it right after).  The module docstring says what is bit for bit and what agrees to rounding."""
    return _smooth("cg_prolongation_smoothing", "energy_cg", None, A, T, B, BtBinv, pattern, maxiter, tol, weighting, Cpt_params)


def gmres_prolongation_smoothing(A, T, B, BtBinv, pattern, maxiter, tol, weighting="local", Cpt_params=None):
    """pyamg.aggregation.smooth.gmres_prolongation_smoothing: smooth T with GMRES on ``A T = 0`` inside ``pattern``, keeping ``T @ B`` --
    what ``energy_prolongation_smoother`` runs for non-symmetric operators, once on A for P and once on ``A^H`` for R.

    Returns a ``bsr_array`` on the pattern's structure, explicit zero blocks possible, as ``cg_prolongation_smoothing`` does.  The Krylov
    basis costs ``maxiter + 1`` arrays of the pattern's size in HBM; more than ``GMRES_MAXITER`` iterations are not on the device path."""
    return _smooth("gmres_prolongation_smoothing", "energy_gmres", GMRES_MAXITER, A, T, B, BtBinv, pattern, maxiter, tol, weighting, Cpt_params)
