"""The setup of ``rootnode_solver`` around the energy-minimisation loop, on the device: drop-ins for the reference's

* ``compute_BtBinv``                  -- pyamg/util/utils.py:1533-1624
* ``scale_T``                         -- pyamg/util/utils.py:1275-1381
* ``filter_operator``                 -- pyamg/util/utils.py:1119-1272
* ``relaxation_as_linear_operator``   -- pyamg/relaxation/utils.py:9-82

with the reference's signatures and error behaviour.  The kernels are csrc/pamg_rootnode.hip, their arithmetic csrc/pamg_rootnode.h.

``compute_BtBinv`` sums every entry of ``B_i^H B_i`` in the reference's order (the pattern row's stored blocks in stored order, the columns
of a block ascending), so ``BtB`` is ``amg_core.calc_BtB``'s bit for bit; it stays on the device, where a lane per node transposes and
pseudo-inverts its block.  With one candidate the inverse is the reference's reciprocal rule, bit for bit; with more it is a one-sided
Jacobi SVD with ``gelss``' rank rule at ``cond = set_tol(float64)``, LAPACK's blocks to rounding.

``scale_T`` takes the case the reference's own caller builds: T sorted without duplicates, every root row holding its aggregate's block
and nothing else (so ``D = P_I.T @ T`` is block diagonal), ``P_I`` the injection with identity blocks, ``I_F`` the identity with the root
rows removed.  The products run in the order of SciPy's ``bsr_matmat``; the result has the structure SciPy's ``I_F @ T + P_I`` leaves: T's
without its all-zero blocks, the identity block in every root row.  Bit for bit for 1 x 1 blocks, to rounding through the pseudo-inverse
otherwise.

``filter_operator`` expands A onto the sorted structure of C on the host (values outside C dropped, ``0.0 + a`` inside, as the
reference's COO detour leaves them), and one kernel forms ``A @ B - Bf`` in the order of SciPy's ``bsr_matvecs`` and projects.  Given
the same ``BtBinv`` the result is the reference's bit for bit.

``relaxation_as_linear_operator`` has the caller's package set the smoother up, exactly as the reference does -- its ``Dinv``, its
``omega``, its random draws --, reads the parameters back with ``hierarchy.smoother_spec`` and ships A once; ``matvec`` and ``matmat``
relax every column from its copy with the order-exact sweeps of the resident engine: the reference's result bit for bit.  Taken:
``gauss_seidel``, ``sor``, ``jacobi``, ``block_gauss_seidel``, ``block_jacobi``.

What the device path does not take raises ``NotImplementedError`` before a device call and before anything is drawn: non-float64 or
complex data, more than 6 candidates, blocks beyond 6, index arrays beyond int32, inputs that are not BSR / CSR, structures with a
block stored twice where the reference would add them up, other relaxation methods.  ``aggregation.device_setup(pyamg, rootnode=True)``
then hands the call to the reference function it patched out.  ``get_Cpt_params``, the row filters and the CGNR variant stay in the
reference.
"""
from __future__ import annotations

import importlib

import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import LinearOperator

from . import amg_core
from .classical import _i32

__all__ = ["compute_BtBinv", "scale_T", "filter_operator", "relaxation_as_linear_operator"]

MAX_BLOCK = 6
MAX_NULLDIM = 6
RELAXATION_METHODS = ("gauss_seidel", "sor", "jacobi", "block_gauss_seidel", "block_jacobi")


def _candidates(B, what):
    if not isinstance(B, np.ndarray) or B.dtype != np.float64 or B.ndim != 2:
        raise NotImplementedError(f"{what} on the device takes a two-dimensional float64 array of candidates")
    if B.shape[1] < 1 or B.shape[1] > MAX_NULLDIM:
        raise NotImplementedError(f"{what} on the device takes 1 to {MAX_NULLDIM} candidates (got {B.shape[1]})")
    return B


def _blocks(M):
    """(rows per block, columns per block) of a CSR / BSR matrix"""
    return tuple(M.blocksize) if M.format == "bsr" else (1, 1)


def _sorted_keys(M, nbc, what, fn):
    """row * nbc + column of every stored block of M, ascending, and the permutation that sorts them; a block stored twice is refused"""
    rows = np.repeat(np.arange(M.indptr.size - 1, dtype=np.int64), np.diff(M.indptr))
    keys = rows * nbc + M.indices
    if keys.size < 2 or np.all(keys[1:] > keys[:-1]):
        return keys, None
    order = np.argsort(keys, kind="stable")
    keys = keys[order]
    if np.any(keys[1:] == keys[:-1]):
        raise NotImplementedError(f"{fn} on the device: {what} stores a block twice")
    return keys, order


def compute_BtBinv(B, C):
    """pyamg.util.utils.compute_BtBinv: ``BtBinv[i] = pinv(B_i^H B_i)`` with ``B_i`` the rows of B in the pattern of block row i of C."""
    if not sp.issparse(C) or C.format not in ("csr", "bsr"):
        raise TypeError("Expected bsr_array or csr_array for C")
    if C.shape[1] != B.shape[0]:
        raise TypeError("Expected matching dimensions such that C @ B")
    B = _candidates(B, "compute_BtBinv")
    r, c = _blocks(C)
    if c > MAX_BLOCK:
        raise NotImplementedError(f"compute_BtBinv on the device takes up to {MAX_BLOCK} columns per block (got {c})")
    K, n = B.shape[1], int(C.shape[0] / r)
    Sp, Sj = _i32(C.indptr), _i32(C.indices)
    BtBinv = np.zeros((n, K, K), dtype=np.float64)
    amg_core.compute_BtBinv(K, n, c, np.ascontiguousarray(np.ravel(B)), Sp, Sj, BtBinv.reshape(-1))
    return BtBinv


def _injection(T, P_I, I_F, bs):
    """Cnodes[a] = the block row of aggregate a's root node, read from P_I; refuses what is not an injection beside its I_F"""
    what = "scale_T"
    n, nagg = T.shape[0] // bs, T.shape[1] // bs
    if P_I.shape != T.shape or I_F.shape != (T.shape[0], T.shape[0]):
        raise NotImplementedError(f"{what} on the device: P_I or I_F do not fit T")
    eye = np.eye(bs)
    if P_I.indices.size != nagg or not np.all(P_I.data == eye) or np.any(np.diff(P_I.indptr) > 1):
        raise NotImplementedError(f"{what} on the device takes P_I as an injection: one identity block per aggregate")
    Cnodes = np.full(nagg, -1, dtype=np.int32)
    Cnodes[P_I.indices] = np.flatnonzero(np.diff(P_I.indptr))
    if np.any(Cnodes < 0):
        raise NotImplementedError(f"{what} on the device takes P_I as an injection: one identity block per aggregate")
    dF = I_F.diagonal()
    root = np.zeros(n, dtype=bool)
    root[Cnodes] = True
    if I_F.count_nonzero() != np.count_nonzero(dF) or not np.array_equal(dF, np.repeat(np.where(root, 0.0, 1.0), bs)):
        raise NotImplementedError(f"{what} on the device takes I_F as the identity with the root rows removed")
    return Cnodes


def scale_T(T, P_I, I_F):
    """pyamg.util.utils.scale_T: scale T from the right with the inverse of its root-node blocks, so that it is the identity at the
    root rows."""
    for M, name in ((T, "T"), (P_I, "P_I"), (I_F, "I_F")):
        if not sp.issparse(M) or M.format != "bsr":
            raise TypeError(f"Expected BSR matrix {name}")
        if M.blocksize[0] != M.blocksize[1]:
            raise TypeError(f"Expected BSR matrix {name} with square blocks")
    if (I_F.blocksize[0] != P_I.blocksize[0]) or (I_F.blocksize[0] != T.blocksize[0]):
        raise TypeError("Expected identical blocksize in I_F, P_I and T")
    if P_I.nnz == 0:
        return T
    bs = T.blocksize[0]
    if T.dtype != np.float64 or P_I.dtype != np.float64 or I_F.dtype != np.float64:
        raise NotImplementedError("scale_T on the device is float64 only")
    if bs > MAX_BLOCK:
        raise NotImplementedError(f"scale_T on the device takes blocks up to {MAX_BLOCK} x {MAX_BLOCK} (got {T.blocksize})")
    n, nagg = T.shape[0] // bs, T.shape[1] // bs
    Tp, Tj = _i32(T.indptr), _i32(T.indices)
    if _sorted_keys(T, nagg, "T", "scale_T")[1] is not None:
        raise NotImplementedError("scale_T on the device takes T with sorted rows")
    Cnodes = _injection(T, P_I, I_F, bs)
    if np.any(np.diff(Tp)[Cnodes] != 1) or np.any(Tj[Tp[Cnodes]] != np.arange(nagg)):
        raise NotImplementedError("scale_T on the device takes root rows that hold their aggregate's block and nothing else")
    Tx = np.array(T.data, dtype=np.float64, order="C").reshape(-1)
    amg_core.scale_T(n, nagg, bs, Tp, Tj, Tx, Cnodes)
    Tx = Tx.reshape(-1, bs, bs)
    keep = np.any(Tx.reshape(Tx.shape[0], -1) != 0.0, axis=1)          # SciPy's `+` stores no all-zero block
    indptr = np.zeros(n + 1, dtype=np.int32)
    rows = np.repeat(np.arange(n), np.diff(Tp))
    indptr[1:] = np.cumsum(np.bincount(rows[keep], minlength=n))
    return sp.bsr_array((Tx[keep], Tj[keep], indptr), shape=T.shape)


def filter_operator(A, C, B, Bf, BtBinv=None):
    """pyamg.util.utils.filter_operator: A on the matrix graph of C, changed row by row so that ``A_new @ B = Bf``."""
    if A.shape[0] != C.shape[0]:
        raise ValueError("A and C must be the same size")
    if A.shape[1] != C.shape[1]:
        raise ValueError("A and C must be the same size")
    if not sp.issparse(C) or C.format not in ("bsr", "csr") or not sp.issparse(A) or A.format != C.format:
        raise ValueError("A and C must either both be CSR or BSR")
    r, c = _blocks(C)
    if _blocks(A) != (r, c):
        raise ValueError("A and C must have same BSR blocksizes")
    if len(Bf.shape) == 1:
        Bf = Bf.reshape(-1, 1)
    if Bf.shape[0] != A.shape[0]:
        raise ValueError("A and Bf must have the same first dimension")
    if len(B.shape) == 1:
        B = B.reshape(-1, 1)
    if B.shape[0] != A.shape[1]:
        raise ValueError("A and B must have matching dimensions such that A*B is computable")
    if B.shape[1] != Bf.shape[1]:
        raise ValueError("B and Bf must have the same second dimension")
    what = "filter_operator"
    B, Bf = _candidates(B, what), _candidates(Bf, what)
    if A.dtype != np.float64 or (BtBinv is not None and np.asarray(BtBinv).dtype != np.float64):
        raise NotImplementedError(f"{what} on the device is float64 only")
    if max(r, c) > MAX_BLOCK:
        raise NotImplementedError(f"{what} on the device takes blocks up to {MAX_BLOCK} x {MAX_BLOCK} (got {(r, c)})")
    n, nbc, K = A.shape[0] // r, A.shape[1] // c, B.shape[1]
    _i32(A.indptr), _i32(A.indices)
    Sp = _i32(C.indptr)
    # the structure the reference's COO detour leaves: C's, sorted
    keys, order = _sorted_keys(C, nbc, "C", what)
    Sj = _i32(C.indices if order is None else np.asarray(C.indices)[order])
    akeys, aorder = _sorted_keys(A, nbc, "A", what)
    adata = np.asarray(A.data).reshape(akeys.size, r, c)
    if aorder is not None:
        adata = adata[aorder]
    at = np.searchsorted(keys, akeys)
    inside = np.zeros(akeys.size, dtype=bool)
    if keys.size:
        inside = keys[np.minimum(at, keys.size - 1)] == akeys
    if BtBinv is None:
        BtBinv = compute_BtBinv(B, C)
    if np.asarray(BtBinv).size != n * K * K:
        raise NotImplementedError(f"{what} on the device: BtBinv does not fit C")
    Sx = np.zeros((keys.size, r, c), dtype=np.float64)
    Sx[at[inside]] = 0.0 + adata[inside]
    amg_core.filter_constraints(r, c, n, K, np.ascontiguousarray(np.ravel(B)), np.ascontiguousarray(np.ravel(Bf)),
                                np.ascontiguousarray(np.ravel(BtBinv)), Sp, Sj, Sx.reshape(-1))
    if C.format == "bsr":
        out = sp.bsr_array((Sx, Sj, Sp.copy()), shape=A.shape)
    else:
        out = sp.csr_array((Sx.reshape(-1), Sj, Sp.copy()), shape=A.shape)
    out.eliminate_zeros()
    return out


class _DeviceRelaxation(LinearOperator):
    """the operator ``relaxation_as_linear_operator`` returns: A, b and the smoother's parameters resident for its lifetime"""

    def __init__(self, A, b, spec):
        from . import _capi as capi
        from .hierarchy import sparse_op
        from .multilevel import DeviceMatrix
        super().__init__(dtype=A.dtype, shape=A.shape)
        self._capi, self._spec = capi, spec
        self._A = DeviceMatrix(sparse_op(A))
        self._b = capi.DeviceArray.from_host(np.ascontiguousarray(b.reshape(-1)))
        self._x = capi.DeviceArray(A.shape[0], np.float64)
        self._work = capi.DeviceArray(max(A.shape[0], 1), np.float64) if spec.kind in ("jacobi", "block_jacobi") else None
        self._Dinv = capi.DeviceArray.from_host(np.ascontiguousarray(spec.Dinv, dtype=np.float64).reshape(-1)) if spec.Dinv is not None else None

    def _relax(self, x):
        if x.dtype != np.float64:
            raise TypeError("arguments A, x, and b must have the same dtype")
        s = self._spec
        self._x.upload(x)
        if s.kind in ("gauss_seidel", "sor"):
            self._A.gauss_seidel(self._x, self._b, sweep=s.sweep, omega=s.omega, iterations=s.iterations)
        elif s.kind == "jacobi":
            self._A.jacobi(self._x, self._b, self._work, s.omega, s.iterations)
        elif s.kind == "block_jacobi":
            self._A.block_jacobi(self._x, self._b, self._work, self._Dinv, s.omega, s.iterations)
        else:
            self._A.block_gauss_seidel(self._x, self._b, self._Dinv, s.sweep, s.iterations)
        self._capi.sync()
        return self._x.download()

    def _matvec(self, x):
        return self._relax(np.asarray(x)).reshape(np.shape(x))

    def _matmat(self, X):
        X = np.asarray(X)
        out = np.empty(X.shape, dtype=np.float64)
        for j in range(X.shape[1]):
            out[:, j] = self._relax(X[:, j])
        return out


def relaxation_as_linear_operator(method, A, b, pyamg=None):
    """pyamg.relaxation.utils.relaxation_as_linear_operator: the operator that applies a relaxation method for the fixed right-hand side
    b.  ``pyamg``: the reference package whose ``relaxation.smoothing`` sets the smoother up (``device_setup`` binds the caller's; default:
    the importable ``pyamg``)."""
    fn, kwargs = (method[0], method[1]) if isinstance(method, tuple) else (method, {})
    what = "relaxation_as_linear_operator"
    if fn not in RELAXATION_METHODS:
        raise NotImplementedError(f"{what}('{fn}') is not on the device path")
    if not sp.issparse(A) or A.format not in ("csr", "bsr") or A.dtype != np.float64 or A.shape[0] != A.shape[1]:
        raise NotImplementedError(f"{what} on the device takes a square float64 CSR or BSR operator")
    _i32(A.indptr), _i32(A.indices)
    r, c = _blocks(A)
    if r != c or r > MAX_BLOCK:
        raise NotImplementedError(f"{what} on the device takes square blocks up to {MAX_BLOCK} x {MAX_BLOCK}")
    if fn.startswith("block_") and (kwargs.get("Dinv") is not None or kwargs.get("blocksize") not in (None, r)):
        raise NotImplementedError(f"{what} on the device takes the block methods with the operator's own blocks")
    if np.asarray(b).size != A.shape[0]:
        raise NotImplementedError(f"{what} on the device takes one right-hand side of A's size")
    if pyamg is None:
        pyamg = importlib.import_module("pyamg")
    from .hierarchy import smoother_spec
    smoothing = importlib.import_module(f"{pyamg.__name__}.relaxation.smoothing")
    Level = importlib.import_module(f"{pyamg.__name__}.multilevel").MultilevelSolver.Level
    b = np.array(b, dtype=A.dtype)
    lvl = Level()
    lvl.A = A
    relax = getattr(smoothing, "setup_" + fn)(lvl, **kwargs)          # the reference's own Dinv, omega and random draws
    return _DeviceRelaxation(A, b, smoother_spec(relax, A))
