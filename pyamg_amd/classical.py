"""The setup of classical (Ruge-Stuben) AMG on the device: drop-ins for the reference's

* ``classical_strength_of_connection``  -- pyamg/strength.py:114-245
* ``MIS`` / ``PMIS``                    -- pyamg/classical/split.py:336-384, :155-194
* ``CLJP`` / ``CLJPc``                  -- split.py:243-333 (csrc/pamg_cljp.hip, the rules in csrc/pamg_cljp.h)
* ``vertex_coloring(method='MIS')``     -- pyamg/graph.py:84-126
* ``direct_interpolation``              -- pyamg/classical/interpolate.py:12-83
* ``classical_interpolation``           -- interpolate.py:86-171 (``modified`` True and False)

Same signatures, same error types, same return formats, and the reference's arrays bit for bit (csrc/pamg_classical.hip; the per-row
arithmetic is csrc/pamg_classical.h).  What SciPy does between the kernels -- ``eliminate_zeros``, ``C.multiply(A)`` -- stays with SciPy
on the host, exactly where the reference has it, and ``PMIS`` draws its random numbers from NumPy's global stream where the reference
draws them, so a patched setup consumes the same stream.

Float64 CSR operators.  What the device path does not take (BSR operators, other dtypes, ``norm='fro'``, a bounded ``maxiter``, a
non-symmetric graph handed to ``MIS``) raises ``NotImplementedError``; ``aggregation.device_setup(pyamg, classical=True)`` then hands
the call to the reference function it patched out (``CLJP``, ``CLJPc`` and ``vertex_coloring`` under its keyword ``cljp=True``).

``CLJP`` is not an order-dependent sweep although the reference writes it as one.  Its selection is synchronous (``Dlist`` is collected
against the unchanged splitting); its weight updates P5 and P6 only remove edges into, and decrement, undecided nodes, and once such a
node drops below 1 and turns F nothing reads its weight or its edges again, so for the nodes still undecided at the end of a pass the
removed edges and the number of decrements do not depend on the order of the C-points; ``w - count`` is exact.  The MIS colouring gives
node i the colour K exactly when no lower-index in-neighbour takes K, which rounds decide from the lowest index up.  What remains
order-dependent and is not here: the serial ``RS`` splitting, the ``JP`` / ``LDF`` colourings (one in-place sweep plus first-fit per
colour) and ``CR``.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from . import amg_core

__all__ = ["classical_strength_of_connection", "MIS", "PMIS", "CLJP", "CLJPc", "vertex_coloring", "direct_interpolation",
           "classical_interpolation"]


def _i32(a):
    a = np.asarray(a)
    if a.dtype != np.int32:
        if a.size and a.max() > np.iinfo(np.int32).max:
            raise NotImplementedError("index arrays beyond int32 are not supported on the device path")
        a = a.astype(np.int32)
    return np.ascontiguousarray(a)


def _f64(M, what):
    if M.dtype != np.float64:
        raise NotImplementedError(f"{what} on the device is float64 only (got {M.dtype})")
    return np.ascontiguousarray(M.data, dtype=np.float64)


def classical_strength_of_connection(A, theta=0.1, block=True, norm="abs"):
    """pyamg.strength.classical_strength_of_connection: the strong connections ``|a_ij| >= theta max_k |a_ik|`` (norm='abs') or
    ``-a_ij >= theta max_k -a_ik`` (norm='min') plus the diagonal, in A's stored order, as magnitudes scaled by each row's largest
    entry, without exact zeros."""
    if sp.issparse(A) and A.format == "bsr":
        if (A.blocksize[0] != A.blocksize[1]) or (A.blocksize[0] < 1):
            raise ValueError("Matrix must have square blocks")
    if theta < 0 or theta > 1:
        raise ValueError("expected theta in [0,1]")
    if not sp.issparse(A) or A.format != "csr":
        raise NotImplementedError("classical_strength_of_connection on the device takes CSR operators")
    if norm == "fro":
        raise NotImplementedError("classical_strength_of_connection(norm='fro') is not on the device path")
    if norm not in ("abs", "min"):
        raise ValueError("Unrecognized option for norm for strength.")
    Ax = _f64(A, "classical_strength_of_connection")
    index_type = A.indptr.dtype
    Ap, Aj = _i32(A.indptr), _i32(A.indices)
    N = A.shape[0]
    Sp = np.empty(N + 1, dtype=np.int32)
    Sj = np.empty(Aj.size, dtype=np.int32)
    Sx = np.empty(Aj.size, dtype=np.float64)
    fn = amg_core.classical_strength_of_connection_abs if norm == "abs" else amg_core.classical_strength_of_connection_min
    fn(N, theta, Ap, Aj, Ax, Sp, Sj, Sx)
    nnz = int(Sp[-1])
    return sp.csr_array((Sx[:nnz].copy(), Sj[:nnz].astype(index_type), Sp.astype(index_type)), shape=(N, N))


def _square_csr(S):
    """the checks of util.utils.remove_diagonal (the kernels skip the diagonal instead of removing it)"""
    if not sp.issparse(S) or S.format != "csr":
        raise TypeError("expected csr_array")
    if S.shape[0] != S.shape[1]:
        raise ValueError(f"expected square matrix, shape={S.shape}")


def MIS(G, weights, maxiter=None, rounds=None):
    """pyamg.classical.split.MIS: the maximal independent set of the graph of G (1 = in the set) the reference's sweeps arrive at --
    the greedy set in descending (weight, index) order.  ``rounds``: a list that receives the number of rounds the device ran."""
    _square_csr(G)
    if maxiter is not None:
        if maxiter < 0:
            raise ValueError("maxiter must be >= 0")
        raise NotImplementedError("MIS(maxiter=...) is not on the device path: a bounded number of in-place sweeps depends on the sweep order")
    n = G.shape[0]
    y = np.ascontiguousarray(np.ravel(np.asarray(weights)), dtype=np.float64)
    if y.size < n:
        raise ValueError("expected one weight per vertex")
    mis = np.empty(n, dtype="intc")
    mis[:] = -1
    try:
        amg_core.maximal_independent_set_parallel(n, _i32(G.indptr), _i32(G.indices), -1, 1, 0, mis, y, -1, rounds=rounds)
    except NotImplementedError as e:                         # PAMG_E_UNSUPPORTED
        raise NotImplementedError("MIS on the device takes symmetric patterns") from e
    return mis


def PMIS(S, rounds=None):
    """pyamg.classical.split.PMIS: C/F splitting (1 = coarse, 0 = fine) by the parallel modified independent set method, with the
    reference's weights: in-degree in the off-diagonal pattern of S plus ``np.random.rand(n)`` from the global stream."""
    _square_csr(S)
    n = S.shape[0]
    Sp, Sj = _i32(S.indptr), _i32(S.indices)
    rnd = np.random.rand(n)                                  # split.py:441: the reference's only draw
    splitting = np.empty(n, dtype="intc")
    amg_core.pmis_splitting(n, Sp, Sj, rnd, splitting, rounds=rounds)
    return splitting


def _pattern_only(M, what):
    """what the pattern-only kernels take: no BSR blocks, int32-sized index arrays"""
    if M.format == "bsr":
        raise NotImplementedError(f"{what} on the device takes CSR patterns, not BSR blocks")
    return _i32(M.indptr), _i32(M.indices)


def CLJP(S, color=False, info=None):
    """pyamg.classical.split.CLJP: C/F splitting (1 = coarse, 0 = fine) by the parallel CLJP method, with the reference's weights --
    ``srand(2448422)`` / ``rand()`` of the C library, or with ``color=True`` the MIS colouring of S -- plus the in-degree.  Only the
    pattern of S is read; its diagonal is skipped and no transpose is formed on the host.  ``info``: a list that receives
    (passes, colours, colouring rounds, nodes selected)."""
    if sp.issparse(S) and S.format == "bsr":
        raise NotImplementedError("CLJP on the device takes CSR patterns, not BSR blocks")
    _square_csr(S)
    n = S.shape[0]
    Sp, Sj = _pattern_only(S, "CLJP")
    splitting = np.empty(n, dtype="intc")
    amg_core.cljp_naive_splitting(n, Sp, Sj, None, None, splitting, 1 if color else 0, info=info)
    return splitting


def CLJPc(S):
    """pyamg.classical.split.CLJPc: CLJP in colour"""
    return CLJP(S, color=True)


def vertex_coloring(G, method="MIS", info=None):
    """pyamg.graph.vertex_coloring(method='MIS'): colour K goes to the greedy independent set, in index order, of the vertices without a
    colour.  Sparse input as ``asgraph`` takes it (CSR or CSC as stored, anything else through CSR).  'JP' and 'LDF' are one in-place
    sweep plus first-fit per colour, which does depend on the sweep order: NotImplementedError.  ``info``: a list that receives
    (colours, rounds)."""
    if not sp.issparse(G) or G.format not in ("csc", "csr"):
        if sp.issparse(G) and G.format == "bsr":
            raise NotImplementedError("vertex_coloring on the device takes CSR patterns, not BSR blocks")
        G = sp.csr_array(G)
    if G.shape[0] != G.shape[1]:
        raise ValueError("expected square matrix")
    if method in ("JP", "LDF"):
        raise NotImplementedError(f"vertex_coloring(method='{method}') is not on the device path: its in-place sweep depends on the sweep order")
    if method != "MIS":
        raise ValueError(f"Unknown method ({method})")
    n = G.shape[0]
    Gp, Gj = _pattern_only(G, "vertex_coloring")
    coloring = np.empty(n, dtype="intc")
    amg_core.vertex_coloring_mis(n, Gp, Gj, coloring, info=info)
    return coloring


def _pattern_with_values_of(C, A):
    """interpolate.py:63-68 / :151-157, SciPy on the host as in the reference"""
    C.eliminate_zeros()
    C.data[:] = 1.0
    return C.multiply(A)


def _interp_inputs(A, C, splitting, what):
    if A.shape[0] != A.shape[1] or C.shape != A.shape:
        raise NotImplementedError(f"{what} on the device takes a square A and a strength matrix of its shape")
    splitting = np.ascontiguousarray(splitting, dtype=np.int32)
    if splitting.ndim != 1 or splitting.size != A.shape[0]:
        raise NotImplementedError(f"{what} on the device takes one splitting entry per row")
    return (_i32(A.indptr), _i32(A.indices), _f64(A, what)), (_i32(C.indptr), _i32(C.indices), _f64(C, what)), splitting


def direct_interpolation(A, C, splitting, theta=None, norm="min"):
    """pyamg.classical.interpolate.direct_interpolation"""
    if not sp.issparse(A) or A.format != "csr":
        raise TypeError("expected csr_array for A")
    if not sp.issparse(C) or C.format != "csr":
        raise TypeError("expected csr_array for C")
    if theta is not None:
        C = classical_strength_of_connection(A, theta=theta, norm=norm)
    else:
        C = C.copy()
    C = _pattern_with_values_of(C, A)
    a, c, split = _interp_inputs(A, C, splitting, "direct_interpolation")
    n = A.shape[0]
    P_indptr = np.empty(n + 1, dtype=np.int32)
    amg_core.rs_direct_interpolation_pass1(n, c[0], c[1], split, P_indptr)
    nnz = int(P_indptr[-1])
    P_indices = np.empty(nnz, dtype=np.int32)
    P_data = np.empty(nnz, dtype=np.float64)
    amg_core.rs_direct_interpolation_pass2(n, *a, *c, split, P_indptr, P_indices, P_data)
    nc = np.sum(splitting)
    it = A.indptr.dtype
    return sp.csr_array((P_data, P_indices.astype(it, copy=False), P_indptr.astype(it, copy=False)), shape=[n, nc])


def classical_interpolation(A, C, splitting, theta=None, norm="min", modified=True):
    """pyamg.classical.interpolate.classical_interpolation: distance-1 classical interpolation, Eq. (9) of De Sterck et al. (2008)
    with ``modified=True`` and Eq. (8) otherwise"""
    if not sp.issparse(A) or A.format != "csr":
        raise TypeError("expected csr_array for A")
    if not sp.issparse(C) or C.format != "csr":
        raise TypeError("Expected csr_array SOC matrix, C.")
    nc = np.sum(splitting)
    n = A.shape[0]
    if A.dtype != np.float64:
        raise NotImplementedError(f"classical_interpolation on the device is float64 only (got {A.dtype})")
    if theta is not None:
        C = classical_strength_of_connection(A, theta=theta, norm=norm)
    else:
        C = C.copy()
    if modified:
        if C.dtype != np.float64:
            raise NotImplementedError(f"classical_interpolation on the device is float64 only (got {C.dtype})")
        split = np.ascontiguousarray(splitting, dtype=np.int32)
        if C.shape[0] != C.shape[1] or split.ndim != 1 or split.size != C.shape[0]:
            raise NotImplementedError("classical_interpolation on the device takes a square strength matrix and one splitting entry per row")
        Cx = np.ascontiguousarray(C.data)
        amg_core.remove_strong_FF_connections(C.shape[0], _i32(C.indptr), _i32(C.indices), Cx, split)
        if Cx is not C.data:
            C.data[:] = Cx
    C = _pattern_with_values_of(C, A)
    a, c, split = _interp_inputs(A, C, splitting, "classical_interpolation")
    P_indptr = np.empty(n + 1, dtype=np.int32)
    amg_core.rs_classical_interpolation_pass1(n, c[0], c[1], split, P_indptr)
    nnz = int(P_indptr[-1])
    P_indices = np.empty(nnz, dtype=np.int32)
    P_data = np.empty(nnz, dtype=np.float64)
    amg_core.rs_classical_interpolation_pass2(n, *a, *c, split, P_indptr, P_indices, P_data, modified)
    it = A.indptr.dtype
    return sp.csr_array((P_data, P_indices.astype(it, copy=False), P_indptr.astype(it, copy=False)), shape=[n, nc])
