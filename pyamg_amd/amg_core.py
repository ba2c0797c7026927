"""GPU twins of the ``pyamg.amg_core`` relaxation entry points and of SciPy's
``_sparsetools.csr_matvec`` / ``bsr_matvec`` -- same names, same positional arguments
(NumPy host buffers, in-place on ``x`` / ``Yx``), bound through ctypes to Layer 1 of the
C ABI (include/pyamg_amd.h).  This is the stub a maintainer drops in place of
``from pyamg import amg_core`` for the solve path.

Like the reference's pybind11 overload set (relaxation_bind.cpp:708-715, ``.noconvert()``)
every array must already have the right dtype: a mismatch raises ``TypeError``.
"""
from __future__ import annotations

import numpy as np

from . import _capi as capi

__all__ = ["csr_matvec", "bsr_matvec", "gauss_seidel", "sor_gauss_seidel", "bsr_gauss_seidel",
           "jacobi", "bsr_jacobi", "block_jacobi", "block_jacobi_indexed", "block_gauss_seidel", "jacobi_indexed", "gauss_seidel_indexed", "overlapping_schwarz_csr", "extract_subblocks", "gauss_seidel_ne",
           "gauss_seidel_nr", "jacobi_ne", "pinv_array", "standard_aggregation", "fit_candidates",
           "classical_strength_of_connection_abs", "classical_strength_of_connection_min", "maximal_independent_set_parallel", "pmis_splitting",
           "cljp_naive_splitting", "vertex_coloring_mis", "bellman_ford", "most_interior_nodes", "lloyd_cluster", "rs_direct_interpolation_pass1", "rs_direct_interpolation_pass2", "remove_strong_FF_connections",
           "rs_classical_interpolation_pass1", "rs_classical_interpolation_pass2",
           "one_point_interpolation", "approx_ideal_restriction_pass1", "approx_ideal_restriction_pass2",
           "block_strength_measure", "block_approx_ideal_restriction_pass2",
           "incomplete_mat_mult_csr", "evolution_strength_helper", "apply_distance_filter", "apply_absolute_distance_filter", "min_blocks",
           "evolution_strength_vector", "relaxation_vectors", "distance_measure", "distance_strength", "vertex_distance", "incomplete_mat_mult_bsr", "satisfy_constraints_helper", "satisfy_constraints", "energy_cg", "energy_gmres",
           "calc_BtB", "compute_BtBinv", "filter_constraints", "scale_T"]


def _sfx(Ax, *vals):
    dt = Ax.dtype
    if dt not in (np.float64, np.float32):
        raise TypeError("incompatible function arguments (float32/float64 only on the device path)")
    for v in vals:
        if not isinstance(v, np.ndarray) or v.dtype != dt or not v.flags.c_contiguous:
            raise TypeError("incompatible function arguments (dtype mismatch or non-contiguous array)")
    return "f64" if dt == np.float64 else "f32"


def _idx(*arrs):
    for a in arrs:
        if not isinstance(a, np.ndarray) or a.dtype != np.int32 or not a.flags.c_contiguous:
            raise TypeError("incompatible function arguments (index arrays must be contiguous int32)")


def _csr5(Ap, Aj, Ax, x, b):
    p = capi.ptr
    return (p(Ap), Ap.size, p(Aj), Aj.size, p(Ax), Ax.size, p(x), x.size, p(b), b.size)


def csr_matvec(n_row, n_col, Ap, Aj, Ax, Xx, Yx):
    """Yx += A @ Xx (scipy.sparse._sparsetools.csr_matvec)."""
    _idx(Ap, Aj)
    s = _sfx(Ax, Xx, Yx)
    capi.check(getattr(capi.lib(), f"pamg_csr_matvec_{s}")(int(n_row), int(n_col), capi.ptr(Ap), capi.ptr(Aj),
                                                          capi.ptr(Ax), capi.ptr(Xx), capi.ptr(Yx)), "csr_matvec")


def bsr_matvec(n_brow, n_bcol, R, C, Ap, Aj, Ax, Xx, Yx):
    """Yx += A @ Xx for BSR with R x C blocks (scipy.sparse._sparsetools.bsr_matvec)."""
    _idx(Ap, Aj)
    s = _sfx(Ax, Xx, Yx)
    capi.check(getattr(capi.lib(), f"pamg_bsr_matvec_{s}")(int(n_brow), int(n_bcol), int(R), int(C), capi.ptr(Ap),
                                                          capi.ptr(Aj), capi.ptr(Ax), capi.ptr(Xx), capi.ptr(Yx)),
               "bsr_matvec")


def gauss_seidel(Ap, Aj, Ax, x, b, row_start, row_stop, row_step):
    _idx(Ap, Aj)
    s = _sfx(Ax, x, b)
    capi.check(getattr(capi.lib(), f"pamg_gauss_seidel_{s}")(*_csr5(Ap, Aj, Ax, x, b), int(row_start),
                                                            int(row_stop), int(row_step)), "gauss_seidel")


def sor_gauss_seidel(Ap, Aj, Ax, x, b, row_start, row_stop, row_step, omega):
    _idx(Ap, Aj)
    s = _sfx(Ax, x, b)
    capi.check(getattr(capi.lib(), f"pamg_sor_gauss_seidel_{s}")(*_csr5(Ap, Aj, Ax, x, b), int(row_start),
                                                                int(row_stop), int(row_step), float(omega)),
               "sor_gauss_seidel")


def bsr_gauss_seidel(Ap, Aj, Ax, x, b, row_start, row_stop, row_step, blocksize):
    _idx(Ap, Aj)
    s = _sfx(Ax, x, b)
    capi.check(getattr(capi.lib(), f"pamg_bsr_gauss_seidel_{s}")(*_csr5(Ap, Aj, Ax, x, b), int(row_start),
                                                                int(row_stop), int(row_step), int(blocksize)),
               "bsr_gauss_seidel")


def jacobi(Ap, Aj, Ax, x, b, temp, row_start, row_stop, row_step, omega):
    _idx(Ap, Aj)
    s = _sfx(Ax, x, b, temp, omega)
    capi.check(getattr(capi.lib(), f"pamg_jacobi_{s}")(*_csr5(Ap, Aj, Ax, x, b), capi.ptr(temp), temp.size,
                                                      int(row_start), int(row_stop), int(row_step),
                                                      capi.ptr(omega), omega.size), "jacobi")


def gauss_seidel_ne(Ap, Aj, Ax, x, b, row_start, row_stop, row_step, Tx, omega):
    """amg_core.gauss_seidel_ne (relaxation.h:875-904)."""
    _idx(Ap, Aj)
    s = _sfx(Ax, x, b, Tx)
    capi.check(getattr(capi.lib(), f"pamg_gauss_seidel_ne_{s}")(*_csr5(Ap, Aj, Ax, x, b), int(row_start), int(row_stop),
                                                               int(row_step), capi.ptr(Tx), Tx.size, float(omega)),
               "gauss_seidel_ne")


def gauss_seidel_nr(Ap, Aj, Ax, x, z, col_start, col_stop, col_step, Tx, omega):
    """amg_core.gauss_seidel_nr (relaxation.h:939-975); Ap/Aj/Ax are the CSC arrays of A, z the residual."""
    _idx(Ap, Aj)
    s = _sfx(Ax, x, z, Tx)
    capi.check(getattr(capi.lib(), f"pamg_gauss_seidel_nr_{s}")(*_csr5(Ap, Aj, Ax, x, z), int(col_start), int(col_stop),
                                                               int(col_step), capi.ptr(Tx), Tx.size, float(omega)),
               "gauss_seidel_nr")


def jacobi_ne(Ap, Aj, Ax, x, b, Tx, temp, row_start, row_stop, row_step, omega):
    """amg_core.jacobi_ne (relaxation.h:811-840); Tx = delta, the row-scaled residual."""
    _idx(Ap, Aj)
    s = _sfx(Ax, x, b, Tx, temp, omega)
    capi.check(getattr(capi.lib(), f"pamg_jacobi_ne_{s}")(*_csr5(Ap, Aj, Ax, x, b), capi.ptr(Tx), Tx.size, capi.ptr(temp),
                                                         temp.size, int(row_start), int(row_stop), int(row_step),
                                                         capi.ptr(omega), omega.size), "jacobi_ne")


def jacobi_indexed(Ap, Aj, Ax, x, b, indices, omega):
    """amg_core.jacobi_indexed (relaxation.h:382-427)."""
    _idx(Ap, Aj)
    if indices.dtype != np.int32:
        raise TypeError("jacobi_indexed(): incompatible function arguments (indices must be int32)")
    s = _sfx(Ax, x, b, omega)
    capi.check(getattr(capi.lib(), f"pamg_jacobi_indexed_{s}")(*_csr5(Ap, Aj, Ax, x, b), capi.ptr(indices), indices.size,
                                                              capi.ptr(omega), omega.size), "jacobi_indexed")


def bsr_jacobi(Ap, Aj, Ax, x, b, temp, row_start, row_stop, row_step, blocksize, omega):
    _idx(Ap, Aj)
    s = _sfx(Ax, x, b, temp, omega)
    capi.check(getattr(capi.lib(), f"pamg_bsr_jacobi_{s}")(*_csr5(Ap, Aj, Ax, x, b), capi.ptr(temp), temp.size,
                                                          int(row_start), int(row_stop), int(row_step),
                                                          int(blocksize), capi.ptr(omega), omega.size),
               "bsr_jacobi")


def block_jacobi(Ap, Aj, Ax, x, b, Tx, temp, row_start, row_stop, row_step, omega, blocksize):
    _idx(Ap, Aj)
    s = _sfx(Ax, x, b, Tx, temp, omega)
    capi.check(getattr(capi.lib(), f"pamg_block_jacobi_{s}")(*_csr5(Ap, Aj, Ax, x, b), capi.ptr(Tx), Tx.size,
                                                            capi.ptr(temp), temp.size, int(row_start),
                                                            int(row_stop), int(row_step), capi.ptr(omega),
                                                            omega.size, int(blocksize)), "block_jacobi")


def overlapping_schwarz_csr(Ap, Aj, Ax, x, b, Tx, Tp, Sj, Sp, nsdomains, nrows, row_start, row_stop, row_step):
    """amg_core.overlapping_schwarz_csr (relaxation.h:1420-1492)."""
    _idx(Ap, Aj)
    for a, n in ((Tp, "Tp"), (Sj, "Sj"), (Sp, "Sp")):
        if a.dtype != np.int32:
            raise TypeError(f"overlapping_schwarz_csr(): incompatible function arguments ({n} must be int32)")
    s = _sfx(Ax, x, b, Tx)
    capi.check(getattr(capi.lib(), f"pamg_overlapping_schwarz_csr_{s}")(*_csr5(Ap, Aj, Ax, x, b), capi.ptr(Tx), Tx.size,
                                                                       capi.ptr(Tp), Tp.size, capi.ptr(Sj), Sj.size,
                                                                       capi.ptr(Sp), Sp.size, int(nsdomains), int(nrows),
                                                                       int(row_start), int(row_stop), int(row_step)),
               "overlapping_schwarz_csr")


def extract_subblocks(Ap, Aj, Ax, Tx, Tp, Sj, Sp, nsdomains, nrows):
    """amg_core.extract_subblocks (relaxation.h:1333-1396): Tx <- the dense diagonal block of every subdomain, at the caller's
    offsets Tp.  Subdomains of at most 64 rows."""
    _idx(Ap, Aj)
    for a, n in ((Tp, "Tp"), (Sj, "Sj"), (Sp, "Sp")):
        if a.dtype != np.int32:
            raise TypeError(f"extract_subblocks(): incompatible function arguments ({n} must be int32)")
    s = _sfx(Ax, Tx)
    p = capi.ptr
    capi.check(getattr(capi.lib(), f"pamg_extract_subblocks_{s}")(p(Ap), Ap.size, p(Aj), Aj.size, p(Ax), Ax.size, p(Tx), Tx.size,
                                                                 p(Tp), Tp.size, p(Sj), Sj.size, p(Sp), Sp.size, int(nsdomains),
                                                                 int(nrows)), "extract_subblocks")


def gauss_seidel_indexed(Ap, Aj, Ax, x, b, Id, row_start, row_stop, row_step):
    """amg_core.gauss_seidel_indexed (relaxation.h:736-790)."""
    _idx(Ap, Aj)
    if Id.dtype != np.int32:
        raise TypeError("gauss_seidel_indexed(): incompatible function arguments (Id must be int32)")
    s = _sfx(Ax, x, b)
    capi.check(getattr(capi.lib(), f"pamg_gauss_seidel_indexed_{s}")(*_csr5(Ap, Aj, Ax, x, b), capi.ptr(Id), Id.size,
                                                                    int(row_start), int(row_stop), int(row_step)),
               "gauss_seidel_indexed")


def block_jacobi_indexed(Ap, Aj, Ax, x, b, Tx, indices, omega, blocksize):
    """amg_core.block_jacobi_indexed (relaxation.h:1129-1199)."""
    _idx(Ap, Aj)
    if indices.dtype != np.int32:
        raise TypeError("block_jacobi_indexed(): incompatible function arguments (indices must be int32)")
    s = _sfx(Ax, x, b, Tx, omega)
    capi.check(getattr(capi.lib(), f"pamg_block_jacobi_indexed_{s}")(*_csr5(Ap, Aj, Ax, x, b), capi.ptr(Tx), Tx.size,
                                                                    capi.ptr(indices), indices.size, capi.ptr(omega),
                                                                    omega.size, int(blocksize)), "block_jacobi_indexed")


def block_gauss_seidel(Ap, Aj, Ax, x, b, Tx, row_start, row_stop, row_step, blocksize):
    _idx(Ap, Aj)
    s = _sfx(Ax, x, b, Tx)
    capi.check(getattr(capi.lib(), f"pamg_block_gauss_seidel_{s}")(*_csr5(Ap, Aj, Ax, x, b), capi.ptr(Tx), Tx.size,
                                                                  int(row_start), int(row_stop), int(row_step),
                                                                  int(blocksize)), "block_gauss_seidel")


def pinv_array(AA, m, n, TransA):
    """amg_core.pinv_array (linalg.h:930-1000): the (m, n, n) array AA, passed ravelled like the reference's callers do
    (util/utils.py:684), is overwritten block by block with the pseudo-inverses.  n <= 6."""
    if not isinstance(AA, np.ndarray) or AA.dtype not in (np.float64, np.float32) or not AA.flags.c_contiguous:
        raise TypeError("incompatible function arguments (contiguous float32/float64 array expected)")
    s = "f64" if AA.dtype == np.float64 else "f32"
    t = TransA if isinstance(TransA, bytes) else str(TransA).encode()
    capi.check(getattr(capi.lib(), f"pamg_pinv_array_{s}")(capi.ptr(AA), AA.size, int(m), int(n), t[:1]), "pinv_array")


def standard_aggregation(n_row, Ap, Aj, x, y):
    """amg_core.standard_aggregation (smoothed_aggregation.h:137-268): x <- aggregate of every node (-1: none), y <- root
    nodes; returns the number of aggregates, like the reference."""
    import ctypes
    _idx(Ap, Aj, x, y)
    na = ctypes.c_int(0)
    capi.check(capi.lib().pamg_standard_aggregation(int(n_row), capi.ptr(Ap), Ap.size, capi.ptr(Aj), Aj.size, capi.ptr(x), x.size,
                                                   capi.ptr(y), y.size, ctypes.byref(na)), "standard_aggregation")
    return int(na.value)


def fit_candidates(n_row, n_col, K1, K2, Ap, Ai, Ax, B, R, tol):
    """amg_core.fit_candidates (real; smoothed_aggregation.h:484-660): Ap / Ai = CSC arrays of AggOp, Ax (ravelled
    (nnz, K1, K2)) and R (ravelled (n_col, K2, K2)) are overwritten."""
    _idx(Ap, Ai)
    s = _sfx(Ax, B, R)
    capi.check(getattr(capi.lib(), f"pamg_fit_candidates_{s}")(int(n_row), int(n_col), int(K1), int(K2), capi.ptr(Ap), Ap.size,
                                                              capi.ptr(Ai), Ai.size, capi.ptr(Ax), Ax.size, capi.ptr(B), B.size,
                                                              capi.ptr(R), R.size, float(tol)), "fit_candidates")


# ------------------------------------------------------------------ classical (Ruge-Stuben) setup: csrc/pamg_classical.hip
def _f64(*arrs):
    for a in arrs:
        if not isinstance(a, np.ndarray) or a.dtype != np.float64 or not a.flags.c_contiguous:
            raise TypeError("incompatible function arguments (contiguous float64 arrays on the device path)")


def _pairs(*arrs):
    out = []
    for a in arrs:
        out += [capi.ptr(a), a.size]
    return out


def _strength(norm, n_row, theta, Ap, Aj, Ax, Sp, Sj, Sx):
    _idx(Ap, Aj, Sp, Sj)
    _f64(Ax, Sx)
    capi.check(getattr(capi.lib(), f"pamg_classical_strength_of_connection_{norm}")(int(n_row), float(theta), *_pairs(Ap, Aj, Ax, Sp, Sj, Sx)),
               f"classical_strength_of_connection_{norm}")


def classical_strength_of_connection_abs(n_row, theta, Ap, Aj, Ax, Sp, Sj, Sx):
    """amg_core.classical_strength_of_connection_abs (ruge_stuben.h:64-111) followed by strength.py:237-240: Sp / Sj / Sx receive the
    finished strength matrix -- magnitudes, rows scaled by their largest entry, zeros dropped; Sp[-1] entries of Sj / Sx are set."""
    _strength("abs", n_row, theta, Ap, Aj, Ax, Sp, Sj, Sx)


def classical_strength_of_connection_min(n_row, theta, Ap, Aj, Ax, Sp, Sj, Sx):
    """amg_core.classical_strength_of_connection_min (ruge_stuben.h:156-204), finished like the _abs form."""
    _strength("min", n_row, theta, Ap, Aj, Ax, Sp, Sj, Sx)


def maximal_independent_set_parallel(num_rows, Ap, Aj, active, C, F, x, y, max_iters=-1, rounds=None):
    """amg_core.maximal_independent_set_parallel (graph.h:140-203), max_iters = -1 only; returns the number of nodes added to the
    set.  ``rounds``: a list that receives the number of synchronous rounds."""
    import ctypes
    _idx(Ap, Aj, x)
    _f64(y)
    n_mis, nr = ctypes.c_int(0), ctypes.c_int(0)
    capi.check(capi.lib().pamg_maximal_independent_set(int(num_rows), *_pairs(Ap, Aj), int(active), int(C), int(F), *_pairs(x, y), int(max_iters),
                                                      ctypes.byref(n_mis), ctypes.byref(nr)), "maximal_independent_set_parallel")
    if rounds is not None:
        rounds.append(int(nr.value))
    return int(n_mis.value)


def pmis_splitting(n_nodes, Sp, Sj, rnd, splitting, rounds=None):
    """classical.split.PMIS after its random draw (no amg_core twin: the reference composes it in Python)."""
    import ctypes
    _idx(Sp, Sj, splitting)
    _f64(rnd)
    nr = ctypes.c_int(0)
    capi.check(capi.lib().pamg_pmis_splitting(int(n_nodes), *_pairs(Sp, Sj, rnd, splitting), ctypes.byref(nr)), "pmis_splitting")
    if rounds is not None:
        rounds.append(int(nr.value))


def cljp_naive_splitting(n, Sp, Sj, Tp, Tj, splitting, colorflag, info=None):
    """amg_core.cljp_naive_splitting (ruge_stuben.h:577-741), the reference's argument order; ``Tp`` / ``Tj`` are accepted and ignored
    (the device builds the transposed pattern itself).  ``info``: a list that receives (passes, colours, colouring rounds, nodes selected)."""
    _idx(Sp, Sj, splitting)
    out = np.zeros(4, dtype=np.int32)
    capi.check(capi.lib().pamg_cljp_splitting(int(n), *_pairs(Sp, Sj), int(colorflag), *_pairs(splitting), capi.ptr(out)), "cljp_naive_splitting")
    if info is not None:
        info.append(tuple(int(v) for v in out))


def vertex_coloring_mis(num_rows, Ap, Aj, x, info=None):
    """amg_core.vertex_coloring_mis (graph.h:218-235); returns the number of colours.  ``info``: a list that receives (colours, rounds)."""
    _idx(Ap, Aj, x)
    out = np.zeros(2, dtype=np.int32)
    capi.check(capi.lib().pamg_vertex_coloring_mis(int(num_rows), *_pairs(Ap, Aj, x), capi.ptr(out)), "vertex_coloring_mis")
    if info is not None:
        info.append(tuple(int(v) for v in out))
    return int(out[0])


def _f64(*arrs):
    for a in arrs:
        if not isinstance(a, np.ndarray) or a.dtype != np.float64 or not a.flags.c_contiguous:
            raise TypeError("incompatible function arguments (float64 only on the device path)")


def bellman_ford(num_nodes, Ap, Aj, Ax, c, d, m, p, info=None):
    """amg_core.bellman_ford (graph.h:670-697), in place on ``d``, ``m``, ``p``.  Exact weights only (csrc/pamg_lloyd.h): anything else
    raises NotImplementedError.  ``info``: a list that receives (distance rounds, stamp rounds)."""
    _idx(Ap, Aj, c, m, p)
    _f64(Ax, d)
    out = np.zeros(2, dtype=np.int32)
    capi.check(capi.lib().pamg_bellman_ford(int(num_nodes), *_pairs(Ap, Aj, Ax, c, d, m, p), capi.ptr(out)), "bellman_ford")
    if info is not None:
        info.append(tuple(int(v) for v in out))


def most_interior_nodes(num_nodes, Ap, Aj, Ax, c, d, m, p, info=None):
    """amg_core.most_interior_nodes (graph.h:842-889), in place on ``c``, ``d``, ``m``, ``p``; returns whether a centre moved.  ``info``: a
    list that receives (distance rounds, stamp rounds, centres moved)."""
    _idx(Ap, Aj, c, m, p)
    _f64(Ax, d)
    out = np.zeros(3, dtype=np.int32)
    capi.check(capi.lib().pamg_most_interior_nodes(int(num_nodes), *_pairs(Ap, Aj, Ax, c, d, m, p), capi.ptr(out)), "most_interior_nodes")
    if info is not None:
        info.append(tuple(int(v) for v in out))
    return bool(out[2])


def lloyd_cluster(num_nodes, Ap, Aj, Ax, c, maxiter, clusters, info=None):
    """the loop of pyamg.graph.lloyd_cluster (graph.py:270-284) with the graph resident, in place on ``c`` and ``clusters``.  ``info``: a
    list that receives (Lloyd iterations, distance rounds, stamp rounds, centres moved in the last iteration)."""
    _idx(Ap, Aj, c, clusters)
    _f64(Ax)
    out = np.zeros(4, dtype=np.int32)
    capi.check(capi.lib().pamg_lloyd_cluster(int(num_nodes), *_pairs(Ap, Aj, Ax, c), int(maxiter), *_pairs(clusters), capi.ptr(out)),
               "lloyd_cluster")
    if info is not None:
        info.append(tuple(int(v) for v in out))


def rs_direct_interpolation_pass1(n_nodes, Sp, Sj, splitting, Pp):
    _idx(Sp, Sj, splitting, Pp)
    capi.check(capi.lib().pamg_rs_direct_interpolation_pass1(int(n_nodes), *_pairs(Sp, Sj, splitting, Pp)), "rs_direct_interpolation_pass1")


def rs_direct_interpolation_pass2(n_nodes, Ap, Aj, Ax, Sp, Sj, Sx, splitting, Pp, Pj, Px):
    _idx(Ap, Aj, Sp, Sj, splitting, Pp, Pj)
    _f64(Ax, Sx, Px)
    capi.check(capi.lib().pamg_rs_direct_interpolation_pass2(int(n_nodes), *_pairs(Ap, Aj, Ax, Sp, Sj, Sx, splitting, Pp, Pj, Px)),
               "rs_direct_interpolation_pass2")


def remove_strong_FF_connections(n_nodes, Sp, Sj, Sx, splitting):
    _idx(Sp, Sj, splitting)
    _f64(Sx)
    capi.check(capi.lib().pamg_remove_strong_FF_connections(int(n_nodes), *_pairs(Sp, Sj, Sx, splitting)), "remove_strong_FF_connections")


def rs_classical_interpolation_pass1(n_nodes, Sp, Sj, splitting, Pp):
    _idx(Sp, Sj, splitting, Pp)
    capi.check(capi.lib().pamg_rs_classical_interpolation_pass1(int(n_nodes), *_pairs(Sp, Sj, splitting, Pp)), "rs_classical_interpolation_pass1")


def rs_classical_interpolation_pass2(n_nodes, Ap, Aj, Ax, Sp, Sj, Sx, splitting, Pp, Pj, Px, modified):
    _idx(Ap, Aj, Sp, Sj, splitting, Pp, Pj)
    _f64(Ax, Sx, Px)
    capi.check(capi.lib().pamg_rs_classical_interpolation_pass2(int(n_nodes), *_pairs(Ap, Aj, Ax, Sp, Sj, Sx, splitting, Pp, Pj, Px),
                                                               int(bool(modified))), "rs_classical_interpolation_pass2")


# ------------------------------------------------------------------ approximate ideal restriction (AIR) setup: csrc/pamg_air.hip
def one_point_interpolation(Pp, Pj, Px, Cp, Cj, Cx, splitting):
    """amg_core.one_point_interpolation (air.h:46-98).  Pp[-1] entries of Pj / Px are written; a C-row's value is 1.0 (the reference
    writes its column only)."""
    _idx(Pp, Pj, Cp, Cj, splitting)
    _f64(Px, Cx)
    capi.check(capi.lib().pamg_one_point_interpolation(*_pairs(Pp, Pj, Px, Cp, Cj, Cx, splitting)), "one_point_interpolation")


def approx_ideal_restriction_pass1(Rp, Cp, Cj, Cpts, splitting, distance=2):
    """amg_core.approx_ideal_restriction_pass1 (air.h:124-163)"""
    _idx(Rp, Cp, Cj, Cpts, splitting)
    capi.check(capi.lib().pamg_approx_ideal_restriction_pass1(*_pairs(Rp, Cp, Cj, Cpts, splitting), int(distance)), "approx_ideal_restriction_pass1")


def approx_ideal_restriction_pass2(Rp, Rj, Rx, Ap, Aj, Ax, Cp, Cj, Cx, Cpts, splitting, distance=2, use_gmres=0, maxiter=10, precondition=1):
    """amg_core.approx_ideal_restriction_pass2 (air.h:212-327) with the least-squares local solve; ``use_gmres`` raises
    NotImplementedError.  Rx need not be zeroed."""
    _idx(Rp, Rj, Ap, Aj, Cp, Cj, Cpts, splitting)
    _f64(Rx, Ax, Cx)
    capi.check(capi.lib().pamg_approx_ideal_restriction_pass2(*_pairs(Rp, Rj, Rx, Ap, Aj, Ax, Cp, Cj, Cx, Cpts, splitting), int(distance),
                                                             int(bool(use_gmres)), int(maxiter), int(bool(precondition))),
               "approx_ideal_restriction_pass2")


# ------------------------------------------------------------------ block (BSR) AIR setup: csrc/pamg_air_block.hip
BLOCK_NORMS = {"abs": 0, "min": 1, "fro": 2}


def block_strength_measure(blocksize, norm, Ax, out):
    """the block measure of classical_strength_of_connection(block=True) (strength.py:200-214; no amg_core twin: the reference composes
    it in NumPy): ``out[p]`` for the stored block ``Ax[p * blocksize**2:(p + 1) * blocksize**2]``, ``norm`` one of 'abs', 'min', 'fro',
    with magnitudes below 1e-16 as 0.0.  'fro' with blocksize 8 and blocks beyond 8 raise NotImplementedError."""
    _f64(Ax, out)
    if norm not in BLOCK_NORMS:
        raise ValueError("Invalid choice of norm.")
    capi.check(capi.lib().pamg_block_strength_measure(int(out.size), int(blocksize), BLOCK_NORMS[norm], *_pairs(Ax, out)), "block_strength_measure")


def block_approx_ideal_restriction_pass2(Rp, Rj, Rx, Ap, Aj, Ax, Cp, Cj, Cx, Cpts, splitting, blocksize, distance=2, use_gmres=0, maxiter=10,
                                         precondition=1):
    """amg_core.block_approx_ideal_restriction_pass2 (air.h:378-584): one QR of the system of order N * blocksize per C-point and
    blocksize right-hand sides; ``use_gmres`` and blocks beyond 8 raise NotImplementedError.  Rx need not be zeroed."""
    _idx(Rp, Rj, Ap, Aj, Cp, Cj, Cpts, splitting)
    _f64(Rx, Ax, Cx)
    capi.check(capi.lib().pamg_block_approx_ideal_restriction_pass2(*_pairs(Rp, Rj, Rx, Ap, Aj, Ax, Cp, Cj, Cx, Cpts, splitting), int(blocksize),
                                                                   int(distance), int(bool(use_gmres)), int(maxiter), int(bool(precondition))),
               "block_approx_ideal_restriction_pass2")


# ------------------------------------------------------------------ evolution strength of connection: csrc/pamg_evolution.hip
def incomplete_mat_mult_csr(Ap, Aj, Ax, Bp, Bj, Bx, Sp, Sj, Sx, num_rows):
    """amg_core.incomplete_mat_mult_csr (evolution_strength.h:586-712): Sx = (A @ B) on the stored pattern of S; A, S CSR, B CSC, sorted."""
    _idx(Ap, Aj, Bp, Bj, Sp, Sj)
    _f64(Ax, Bx, Sx)
    capi.check(capi.lib().pamg_incomplete_mat_mult_csr_f64(*_pairs(Ap, Aj, Ax, Bp, Bj, Bx, Sp, Sj, Sx), int(num_rows)), "incomplete_mat_mult_csr")


def evolution_strength_helper(Sx, Sp, Sj, nrows, x, y, b, BDBCols, NullDim, tol):
    """amg_core.evolution_strength_helper (evolution_strength.h:329-550), real float64, 1 <= NullDim <= 6 (beyond: NotImplementedError)."""
    _idx(Sp, Sj)
    _f64(Sx, x, y, b)
    capi.check(capi.lib().pamg_evolution_strength_helper_f64(*_pairs(Sx, Sp, Sj), int(nrows), *_pairs(x, y, b), int(BDBCols), int(NullDim), float(tol)),
               "evolution_strength_helper")


def apply_distance_filter(n_row, epsilon, Sp, Sj, Sx):
    """amg_core.apply_distance_filter (evolution_strength.h:140-172)"""
    _idx(Sp, Sj)
    _f64(Sx)
    capi.check(capi.lib().pamg_apply_distance_filter_f64(int(n_row), float(epsilon), *_pairs(Sp, Sj, Sx)), "apply_distance_filter")


def apply_absolute_distance_filter(n_row, epsilon, Sp, Sj, Sx):
    """amg_core.apply_absolute_distance_filter (evolution_strength.h:62-85)"""
    _idx(Sp, Sj)
    _f64(Sx)
    capi.check(capi.lib().pamg_apply_absolute_distance_filter_f64(int(n_row), float(epsilon), *_pairs(Sp, Sj, Sx)), "apply_absolute_distance_filter")


def min_blocks(n_blocks, blocksize, Sx, Tx):
    """amg_core.min_blocks (evolution_strength.h:220-245)"""
    _f64(Sx, Tx)
    capi.check(capi.lib().pamg_min_blocks_f64(int(n_blocks), int(blocksize), *_pairs(Sx, Tx)), "min_blocks")


def evolution_strength_vector(Sx, Sp, Sj, nrows, d, b):
    """The one-candidate shortcut of evolution_strength_of_connection (strength.py:738-779), fused: Sx holds Atilde's values and receives
    ``|1 - r|`` or 0.0 per stored entry; ``d`` is Atilde's diagonal, ``b`` the candidate with its zeros made ones."""
    _idx(Sp, Sj)
    _f64(Sx, d, b)
    capi.check(capi.lib().pamg_evolution_strength_vector_f64(*_pairs(Sx, Sp, Sj), int(nrows), *_pairs(d, b)), "evolution_strength_vector")


# ------------------------------------------------------------------ relaxation-vector and vertex-distance strength: csrc/pamg_distance.hip
def relaxation_vectors(Ap, Aj, Ax, X, n, R, k, omega):
    """relaxation_vectors (strength.py:888-889): k weighted-Jacobi sweeps with b = 0 on every column of the n x R block ``X``
    (column-major, flat: ``X[r * n + i]``), in place; one launch per sweep for all R columns.  1 <= R <= 32 (beyond: NotImplementedError)."""
    _idx(Ap, Aj)
    _f64(Ax, X)
    capi.check(capi.lib().pamg_relaxation_vectors_f64(*_pairs(Ap, Aj, Ax, X), int(n), int(R), int(k), float(omega)), "relaxation_vectors")


def distance_measure(measure, Ap, Aj, Ax, X, n, R, Dx):
    """The distance of every stored entry of A from the block ``X`` (as above), on A's pattern; ``measure`` is one of ``capi.DISTANCE``:
    strength.py:945-948 (affinity) and :1008-1014 (algebraic, p = 1, 2, inf).  The diagonal and stored zeros get 0.0."""
    _idx(Ap, Aj)
    _f64(Ax, X, Dx)
    capi.check(capi.lib().pamg_distance_measure_f64(int(measure), *_pairs(Ap, Aj, Ax, X), int(n), int(R), *_pairs(Dx)), "distance_measure")


def distance_strength(measure, Ap, Aj, Ax, X, n, R, k, omega, epsilon, Dx):
    """distance_measure_common (strength.py:1044-1060) resident: one upload of A and of the random block ``X``, k sweeps, the measure and,
    fused with it, eliminate_zeros + apply_distance_filter; ``Dx`` (on A's pattern, dropped entries 0.0) and the relaxed ``X`` come back."""
    _idx(Ap, Aj)
    _f64(Ax, X, Dx)
    capi.check(capi.lib().pamg_distance_strength_f64(int(measure), *_pairs(Ap, Aj, Ax, X), int(n), int(R), int(k), float(omega), float(epsilon),
                                                    *_pairs(Dx)), "distance_strength")


def vertex_distance(Ap, Aj, V, n, dim, Cx):
    """distance_strength_of_connection's values (strength.py:83-87): the Euclidean distance of the two vertices of every stored entry,
    never below 1e-6; ``V`` is n x dim row-major, flat, 1 <= dim <= 8 (beyond: NotImplementedError)."""
    _idx(Ap, Aj)
    _f64(V, Cx)
    capi.check(capi.lib().pamg_vertex_distance_f64(*_pairs(Ap, Aj, V), int(n), int(dim), *_pairs(Cx)), "vertex_distance")


# ------------------------------------------------------------------ energy-minimisation prolongation smoothing: csrc/pamg_energy.hip
def incomplete_mat_mult_bsr(Ap, Aj, Ax, Bp, Bj, Bx, Sp, Sj, Sx, n_brow, n_bcol, brow_A, bcol_A, bcol_B):
    """amg_core.incomplete_mat_mult_bsr (smoothed_aggregation.h:970-1042): Sx += (A @ B) on the stored blocks of S; blocks up to 6 x 6."""
    _idx(Ap, Aj, Bp, Bj, Sp, Sj)
    _f64(Ax, Bx, Sx)
    capi.check(capi.lib().pamg_incomplete_mat_mult_bsr_f64(*_pairs(Ap, Aj, Ax, Bp, Bj, Bx, Sp, Sj, Sx), int(n_brow), int(n_bcol), int(brow_A),
                                                          int(bcol_A), int(bcol_B)), "incomplete_mat_mult_bsr")


def satisfy_constraints_helper(rows_per_block, cols_per_block, num_block_rows, NullDim, x, y, z, Sp, Sj, Sx):
    """amg_core.satisfy_constraints_helper (smoothed_aggregation.h:722-771), real float64: x = conj(B) ravelled, y = U @ B ravelled,
    z = BtBinv ravelled."""
    _idx(Sp, Sj)
    _f64(x, y, z, Sx)
    capi.check(capi.lib().pamg_satisfy_constraints_helper_f64(int(rows_per_block), int(cols_per_block), int(num_block_rows), int(NullDim),
                                                             *_pairs(x, y, z, Sp, Sj, Sx)), "satisfy_constraints_helper")


def satisfy_constraints(rows_per_block, cols_per_block, num_block_rows, NullDim, B, BtBinv, Sp, Sj, Sx):
    """smooth.py's satisfy_constraints on the raw arrays: U @ B in the order of SciPy's bsr_matvecs, then the helper, as one kernel.  (The
    reference composes this in Python; it has no amg_core twin.)"""
    _idx(Sp, Sj)
    _f64(B, BtBinv, Sx)
    capi.check(capi.lib().pamg_satisfy_constraints_f64(int(rows_per_block), int(cols_per_block), int(num_block_rows), int(NullDim),
                                                      *_pairs(B, BtBinv, Sp, Sj, Sx)), "satisfy_constraints")


def _energy_driver_arguments(n_brow, r, Ap, Aj, Ax, Sp, Sj, Tx, B, BtBinv, Dinv, cmask, PIx):
    _idx(Ap, Aj, Sp, Sj)
    _f64(Ax, Tx, B, BtBinv, Dinv)
    if (cmask is None) != (PIx is None):
        raise TypeError("incompatible function arguments (cmask and PIx go together)")
    if cmask is not None:
        _f64(PIx)
        if not isinstance(cmask, np.ndarray) or cmask.dtype != np.uint8 or not cmask.flags.c_contiguous or cmask.size != n_brow * r or PIx.size != Tx.size:
            raise TypeError("incompatible function arguments (cmask: contiguous uint8 per row, PIx: like Tx)")


def energy_cg(n_brow, n_bcol, r, c, NullDim, Ap, Aj, Ax, Sp, Sj, Tx, B, BtBinv, Dinv, cmask, PIx, maxiter, tol):
    """The loop of cg_prolongation_smoothing resident on the device (pamg_energy_cg_f64): Tx, T expanded onto the pattern Sp / Sj, is
    smoothed in place; returns (iterations done, the newsum of every iteration)."""
    import ctypes
    _energy_driver_arguments(n_brow, r, Ap, Aj, Ax, Sp, Sj, Tx, B, BtBinv, Dinv, cmask, PIx)
    its, ns = ctypes.c_int(0), ctypes.c_int(0)
    sums = np.zeros(max(int(maxiter), 1))
    p = capi.ptr
    capi.check(capi.lib().pamg_energy_cg_f64(int(n_brow), int(n_bcol), int(r), int(c), int(NullDim), *_pairs(Ap, Aj, Ax, Sp, Sj, Tx, B, BtBinv, Dinv),
                                            p(cmask), p(PIx), int(maxiter), float(tol), ctypes.byref(its), p(sums), ctypes.byref(ns)), "energy_cg")
    return int(its.value), sums[:int(ns.value)].copy()


def energy_gmres(n_brow, n_bcol, r, c, NullDim, Ap, Aj, Ax, Sp, Sj, Tx, B, BtBinv, Dinv, cmask, PIx, maxiter, tol, H=None):
    """The loop of gmres_prolongation_smoothing resident on the device (pamg_energy_gmres_f64), the arguments as for ``energy_cg``: Tx is
    smoothed in place; returns (iterations done, the normr history: the initial norm first, then the one after every iteration).
    ``H``, a contiguous float64 array of (maxiter + 1)^2 values, receives the rotated Hessenberg matrix."""
    import ctypes
    _energy_driver_arguments(n_brow, r, Ap, Aj, Ax, Sp, Sj, Tx, B, BtBinv, Dinv, cmask, PIx)
    if H is not None:
        _f64(H)
        if H.size != (max(int(maxiter), 0) + 1) ** 2:
            raise TypeError("incompatible function arguments (H: (maxiter + 1)^2 values)")
    its, ns = ctypes.c_int(0), ctypes.c_int(0)
    normrs = np.zeros(max(int(maxiter), 0) + 1)
    p = capi.ptr
    capi.check(capi.lib().pamg_energy_gmres_f64(int(n_brow), int(n_bcol), int(r), int(c), int(NullDim), *_pairs(Ap, Aj, Ax, Sp, Sj, Tx, B, BtBinv, Dinv),
                                               p(cmask), p(PIx), int(maxiter), float(tol), ctypes.byref(its), p(normrs), ctypes.byref(ns), p(H)),
               "energy_gmres")
    return int(its.value), normrs[:int(ns.value)].copy()


# ------------------------------------------------------------------ the setup of rootnode_solver: csrc/pamg_rootnode.hip
def calc_BtB(NullDim, Nnodes, cols_per_block, b, BsqCols, x, Sp, Sj):
    """amg_core.calc_BtB (smoothed_aggregation.h:829-907): x <- BtB [Nnodes, NullDim, NullDim], a block column-major, from b = Bsq ravelled;
    at most 6 candidates and 6 columns per block."""
    _idx(Sp, Sj)
    _f64(b, x)
    capi.check(capi.lib().pamg_calc_BtB_f64(int(NullDim), int(Nnodes), int(cols_per_block), capi.ptr(b), b.size, int(BsqCols), *_pairs(x, Sp, Sj)),
               "calc_BtB")


def compute_BtBinv(NullDim, Nnodes, cols_per_block, B, Sp, Sj, BtBinv):
    """util.utils.compute_BtBinv on the raw arrays: BtBinv [Nnodes, NullDim, NullDim] <- pinv of every node's B_i^H B_i, BtB staying on the
    device.  (The reference composes this in Python; it has no amg_core twin.)"""
    _idx(Sp, Sj)
    _f64(B, BtBinv)
    capi.check(capi.lib().pamg_compute_BtBinv_f64(int(NullDim), int(Nnodes), int(cols_per_block), *_pairs(B, Sp, Sj, BtBinv)), "compute_BtBinv")


def filter_constraints(rows_per_block, cols_per_block, num_block_rows, NullDim, B, Bf, BtBinv, Sp, Sj, Sx):
    """The projection of util.utils.filter_operator on the raw arrays: diff = S @ B - Bf in the order of SciPy's bsr_matvecs, then
    satisfy_constraints_helper with diff, as one kernel, in place on Sx.  (No amg_core twin in the reference.)"""
    _idx(Sp, Sj)
    _f64(B, Bf, BtBinv, Sx)
    capi.check(capi.lib().pamg_filter_constraints_f64(int(rows_per_block), int(cols_per_block), int(num_block_rows), int(NullDim),
                                                     *_pairs(B, Bf, BtBinv, Sp, Sj, Sx)), "filter_constraints")


def scale_T(n_brow, n_bcol, blocksize, Tp, Tj, Tx, Cnodes):
    """util.utils.scale_T on T's arrays, in place on Tx: T pinv(P_I^T T) with the identity block in every root row; Cnodes: the block row
    of every aggregate's root node.  (No amg_core twin in the reference.)"""
    _idx(Tp, Tj, Cnodes)
    _f64(Tx)
    capi.check(capi.lib().pamg_scale_T_f64(int(n_brow), int(n_bcol), int(blocksize), *_pairs(Tp, Tj, Tx, Cnodes)), "scale_T")
