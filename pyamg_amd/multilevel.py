"""Device-resident drop-in for ``pyamg.multilevel.MultilevelSolver.solve`` /
``aspreconditioner`` (reference: pyamg/multilevel.py:355-582).

``DeviceMultilevelSolver(ml)`` wraps a hierarchy that the *reference* built on the host
(setup stays there, north star), ships every level to HBM once and runs the cycle as HIP
kernels through the C ABI (include/pyamg_amd.h, Layer 2).  Signatures, return conventions
and error behaviour follow the reference:

* ``solve(b, x0=None, tol=1e-5, maxiter=100, cycle='V', accel=None, callback=None,
  residuals=None, cycles_per_level=1, return_info=False)`` -- returns a ravelled ``(n,)``
  array even for ``(n, 1)`` input (multilevel.py:553-554), dtype = upcast of (A, b, x0)
  (:551-552), ``info`` = 0 on convergence else the iteration count (:574-582),
  ``residuals[:] = [r0, r1, ...]`` (:546-569), ``callback(x)`` after every cycle (:571-572).
* ``aspreconditioner(cycle)`` -- SciPy ``LinearOperator`` whose matvec is exactly one cycle
  from a zero initial guess (:390-396).
* ``accel=`` -- 'cg', 'gmres' / 'gmres_householder', 'fgmres', 'bicgstab', 'cr', 'steepest_descent' and
  'minimal_residual' run on the device (vectors resident, one host read-back per iteration); any other
  accelerator, and any call with ``callback=``, runs on the host exactly as in the reference (:479-535) with
  the device cycle as preconditioner ``M``.

There is no CPU fallback: unsupported configurations raise ``NotImplementedError``.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import numpy as np

from . import _capi as capi
from .hierarchy import HierarchySpec, SmootherSpec, SparseOp, extract

__all__ = ["DeviceMatrix", "DeviceMultilevelSolver", "TUNE_KEYS"]


# the tuning knobs of an operator: name -> key of pamg_matrix_tune (the PAMG_TUNE_<NAME> constants of include/pyamg_amd.h, which documents them),
# in ascending key order -- the order DeviceMatrix.tune applies them in
TUNE_KEYS = {
    "lds_entries": 0, "max_rows": 2, "flow_cap": 3, "gs_mode": 5, "gran_cap": 6, "gran_xcd": 7, "stream_flags": 8, "gs_prof": 11, "tile_G": 12, "tile_W": 13, "tile_cap": 14,
    "tile_default": 15, "tile_D": 16, "tile_Q": 17, "tile_part": 18, "idx16": 19, "gs_cap": 20, "val8": 21, "rowgather": 22, "rowpat": 23, "gs_order": 24, "lane_L": 25, "lane_G": 26,
    "lane_wide": 27, "lane_flags": 28, "line_scan": 30, "rowmask_kz": 31, "rowmask_flags": 32, "lane_merge": 33, "lanem_ahead": 34, "lanem_rpw": 35, "lds_pad": 36, "sym_fused": 37,
    "lanem_cluster": 38, "zero_plans": 39, "zero_merge": 40, "gs_correction": 41,
}


class DeviceMatrix:
    """A SparseOp resident in HBM (``pamg_matrix_t``)."""

    def __init__(self, op: SparseOp):
        lib = capi.lib()
        self.op = op
        self.dtype = np.dtype(op.dtype)
        R, Cc = op.blocksize
        h = C.c_void_p()
        capi.check(lib.pamg_matrix_create(
            C.byref(h), capi.dtype_code(op.dtype), capi.BSR if op.fmt == "bsr" else capi.CSR,
            op.shape[0] // R, op.shape[1] // Cc, R, Cc,
            capi.ptr(op.indptr), capi.ptr(op.indices), capi.ptr(op.data)), "pamg_matrix_create")
        self.handle = h
        self.shape = tuple(op.shape)

    # -- info / tuning
    def info(self) -> dict:
        a = (C.c_int64 * 8)()
        capi.check(capi.lib().pamg_matrix_info(self.handle, a), "pamg_matrix_info")
        keys = ("rows", "cols", "nnz", "row_blocks", "lds_entries", "hbm_bytes", "gs_levels_fwd", "gs_levels_bwd")
        return dict(zip(keys, [int(v) for v in a]))

    def autotune(self, allow_cap=True):
        capi.check(capi.lib().pamg_matrix_autotune(self.handle, int(bool(allow_cap))), "pamg_matrix_autotune")

    def subset_rows(self, rows) -> "DeviceMatrix":
        """row-subset copy (rows: int32 host list, kept in order) for the indexed smoothers"""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        sub = DeviceMatrix.__new__(DeviceMatrix)
        h = C.c_void_p()
        capi.check(capi.lib().pamg_matrix_subset_rows(self.handle, capi.ptr(rows), rows.size, C.byref(h)),
                   "pamg_matrix_subset_rows")
        sub.__dict__.update(self.__dict__)
        sub.handle = h
        return sub

    def kaczmarz(self, v, Dinv, omega, sweep="forward", iterations=1, b=None, xout=None, stream=None):
        """Kaczmarz-type sweeps over the rows of this operator (pamg_matrix_kaczmarz): b given ->
        gauss_seidel_ne on v = x; xout given -> gauss_seidel_nr (self = CSR of A^T, v = running residual)."""
        nr = xout is not None
        capi.check(capi.lib().pamg_matrix_kaczmarz(self.handle, int(nr), v.ptr, b.ptr if b is not None else None, Dinv.ptr,
                                                   float(omega), capi.SWEEP[sweep], int(iterations),
                                                   xout.ptr if nr else None, stream), "pamg_matrix_kaczmarz")

    def jacobi_indexed(self, x, b, omega, work, stream=None):
        """amg_core.jacobi_indexed on a row-subset operator (self): relaxes the listed rows of x from the old x"""
        capi.check(capi.lib().pamg_matrix_jacobi_indexed(self.handle, x.ptr, b.ptr, float(omega), work.ptr, stream),
                   "pamg_matrix_jacobi_indexed")

    def flow_error(self) -> bool:
        e = C.c_int(0)
        capi.check(capi.lib().pamg_matrix_flow_error(self.handle, C.byref(e)), "pamg_matrix_flow_error")
        return bool(e.value)

    def gs_profile(self, which=0):
        """time stamps of the granular sweep (tune(gs_prof=1)): int64 array [ranges, 8]"""
        import numpy as np
        n = C.c_int64(0)
        lib = capi.lib()
        capi.check(lib.pamg_matrix_gs_profile(self.handle, which, None, 0, C.byref(n)), "pamg_matrix_gs_profile")
        out = np.zeros((n.value, 8), dtype=np.int64)
        if n.value:
            capi.check(lib.pamg_matrix_gs_profile(self.handle, which, C.c_void_p(out.ctypes.data), n.value, C.byref(n)),
                       "pamg_matrix_gs_profile")
        return out

    def value_codes(self) -> int:
        """size of the value dictionary when the whole-operator kernels stream 8-bit value codes, else 0"""
        n = C.c_int(0)
        capi.check(capi.lib().pamg_matrix_value_codes(self.handle, C.byref(n)), "pamg_matrix_value_codes")
        return int(n.value)

    def row_patterns(self) -> int:
        """size of the row-pattern table when the whole-operator kernels run in the row-pattern form, else 0"""
        n = C.c_int(0)
        capi.check(capi.lib().pamg_matrix_row_patterns(self.handle, C.byref(n)), "pamg_matrix_row_patterns")
        return int(n.value)

    def row_masks(self) -> dict:
        """the row-mask form of the row patterns (constant-coefficient stencils): dict, all zero when another form runs"""
        out = (C.c_longlong * 8)()
        capi.check(capi.lib().pamg_matrix_row_masks(self.handle, out), "pamg_matrix_row_masks")
        keys = ("entries", "walked_rows", "lattice", "line", "plane", "planes_per_lane", "flags", "launch_grid")
        return dict(zip(keys, (int(v) for v in out)))

    def tile_info(self, which=0):
        """plan of the tiled sweep (schedule 0 = forward, 1 = backward): dict, all zero if none is built"""
        a = (C.c_int64 * 8)()
        capi.check(capi.lib().pamg_matrix_tile_info(self.handle, which, a), "pamg_matrix_tile_info")
        d = dict(zip(("tiles", "ring", "geom", "steps", "early_local", "early_global", "publishing_rows", "lds_bytes"), list(a)))
        geom = d.pop("geom")
        d.update(code_chunks=geom & 0xFF, lds_slots=(geom >> 8) & 0xFF, gather_depth=(geom >> 16) & 0xFF, loader_in_flight=(geom >> 24) & 0xFF)
        return d

    def lane_info(self, which=0):
        """layout of the lane-parallel fast-order sweep (schedule 0 = forward, 1 = backward): dict, all zero if none is built"""
        a = (C.c_int64 * 8)()
        capi.check(capi.lib().pamg_matrix_lane_info(self.handle, which, a), "pamg_matrix_lane_info")
        return dict(zip(("lanes_per_row", "slots_per_lane", "groups", "entry_slots", "early_entries", "launch_grid", "widest_level_groups", "bytes"), list(a)))

    def lanem_info(self, which=0):
        """plan of the MERGED lane-parallel sweep (s dependency levels eliminated into one super-level; schedule 0 = forward, 1 = backward):
        dict, all zero if the schedule runs unmerged; which = 4 / 5: the operator's zero-iterate plans Zf / Zb (tune(zero_plans=...))"""
        a = (C.c_int64 * 20)()
        gr = C.c_double(0.0)
        capi.check(capi.lib().pamg_matrix_lanem_info(self.handle, which, a, C.byref(gr)), "pamg_matrix_lanem_info")
        d = dict(zip(("super_levels", "dependency_levels", "rows", "units", "early_operands", "old_operands", "b_operands", "longest_row", "s_max",
                      "closed_by_length", "closed_by_growth", "launch_grid", "cluster_rows", "groups", "padded_slots", "unique_units",
                      "unique_early", "unique_old", "unique_b", "early_lines"), list(a)))
        d["max_growth"] = gr.value
        d["padding"] = d["padded_slots"] / max(1, d["early_operands"] + d["old_operands"] + d["b_operands"])      # padded slots per real operand
        return d

    def point_twin(self) -> int:
        """fast order of the BSR point sweep: 0 = no scalar twin (exact order / not swept yet), 1 = the twin carries the sweeps, 2 = no fast form fits"""
        st = C.c_int(0)
        capi.check(capi.lib().pamg_matrix_point_twin(self.handle, C.byref(st)), "pamg_matrix_point_twin")
        return int(st.value)

    def lanem_levels(self, which=0):
        """first row of every super-level of the merged plan: int64 array [super_levels + 1] (empty if the schedule runs unmerged)"""
        n = C.c_int64(0)
        lib = capi.lib()
        capi.check(lib.pamg_matrix_lanem_levels(self.handle, which, None, 0, C.byref(n)), "pamg_matrix_lanem_levels")
        out = np.zeros(n.value, dtype=np.int64)
        if n.value:
            capi.check(lib.pamg_matrix_lanem_levels(self.handle, which, C.c_void_p(out.ctypes.data), n.value, C.byref(n)), "pamg_matrix_lanem_levels")
        return out

    def sym_info(self):
        """the fused symmetric sweep (tune(sym_fused=...)): launches so far, the form of the last one (it keeps that name until another fused launch,
        also after a tune change that ends the form), the state of its buffers between launches"""
        a = (C.c_int64 * 9)()
        capi.check(capi.lib().pamg_matrix_sym_info(self.handle, a), "pamg_matrix_sym_info")
        d = dict(zip(("launches", "zero_launches", "form", "launch_grid", "enabled", "handoff_not_sentinel", "counters_not_zero", "zero_plan_launches", "correction_launches"), list(a)))
        d["form"] = {0: "none", 1: "merged", 2: "line", 3: "merged_one_xcd"}[d["form"]]
        return d

    def line_info(self, which=0):
        """layout of the line-scan fast-order sweep (schedule 0 = forward, 1 = backward): dict, all zero if none is built"""
        a = (C.c_int64 * 8)()
        capi.check(capi.lib().pamg_matrix_line_info(self.handle, which, a), "pamg_matrix_line_info")
        return dict(zip(("slots_per_row", "chunks", "lines", "line_levels", "early_entries", "launch_grid", "widest_level_lines", "bytes"), list(a)))

    def kz_info(self, which=0):
        """layout of the lane-parallel fast-order Kaczmarz sweep of the operator's `which`-th line schedule: dict, all zero if none is built"""
        a = (C.c_int64 * 8)()
        capi.check(capi.lib().pamg_matrix_kz_info(self.handle, which, a), "pamg_matrix_kz_info")
        return dict(zip(("lanes_per_line", "slots_per_lane", "groups", "dependency_levels", "widest_level_groups", "launch_grid", "bytes"), list(a)[:7]))

    def lane_profile(self, which=0):
        """time stamps of the lane sweep (tune(gs_prof=1)): int64 array [groups, 4]"""
        n = C.c_int64(0)
        lib = capi.lib()
        capi.check(lib.pamg_matrix_lane_profile(self.handle, which, None, 0, C.byref(n)), "pamg_matrix_lane_profile")
        out = np.zeros((n.value, 4), dtype=np.int64)
        if n.value:
            capi.check(lib.pamg_matrix_lane_profile(self.handle, which, C.c_void_p(out.ctypes.data), n.value, C.byref(n)), "pamg_matrix_lane_profile")
        return out

    def tune(self, **knobs):
        """Set tuning knobs by name (TUNE_KEYS; include/pyamg_amd.h says for each its range, its default and what it chooses).  ``None`` leaves
        a knob alone; the others are applied in ascending key order, whatever order they were written in -- the re-planning keys come first,
        gs_order before the keys that shape its layouts.
        Speed only (every setting computes the same bits) -- except gs_order: 0 = order-exact row sums (the reference's bits), 1 = fast
        order (lane-parallel row sums, same sweep order, agrees to rounding).  Refused (PAMG_E_STATE) once a solver holds the operator:
        captured graphs point into the plans these calls rebuild.  ``DeviceMultilevelSolver(level_tune=...)`` takes the same names per level."""
        unknown = [k for k in knobs if k not in TUNE_KEYS]
        if unknown:
            raise TypeError(f"tune() got an unexpected keyword argument {unknown[0]!r}")
        lib = capi.lib()
        for name, key in TUNE_KEYS.items():
            if knobs.get(name) is not None:
                capi.check(lib.pamg_matrix_tune(self.handle, key, int(knobs[name])), "pamg_matrix_tune")

    # -- kernels on DeviceArray operands
    def spmv(self, mode, x, y, b=None, c=0.0, stream=None, part=None):
        """y (op)= A x; part = 1 / 2: only the row ranges that read owned columns / the halo (after split_ranges)"""
        if part is not None:
            capi.check(capi.lib().pamg_matrix_spmv_part(self.handle, int(part), mode, x.ptr, b.ptr if b is not None else None,
                                                        float(c), y.ptr, stream), "pamg_matrix_spmv_part")
            return
        capi.check(capi.lib().pamg_matrix_spmv(self.handle, mode, x.ptr, b.ptr if b is not None else None,
                                               float(c), y.ptr, stream), "pamg_matrix_spmv")

    def split_ranges(self, n_owned_cols: int):
        """a row shard in local numbering [owned | halo]: sort the row ranges into interior (part 1) and boundary (part 2)"""
        capi.check(capi.lib().pamg_matrix_split_ranges(self.handle, int(n_owned_cols)), "pamg_matrix_split_ranges")

    def resid_sumsq(self, x, b, out, stream=None):
        capi.check(capi.lib().pamg_matrix_resid_sumsq(self.handle, x.ptr, b.ptr, out.ptr, stream),
                   "pamg_matrix_resid_sumsq")

    def jacobi(self, x, b, work, omega, iterations=1, stream=None):
        capi.check(capi.lib().pamg_matrix_jacobi(self.handle, x.ptr, b.ptr, work.ptr, float(omega),
                                                 int(iterations), stream), "pamg_matrix_jacobi")

    def gauss_seidel(self, x, b, sweep="forward", omega=1.0, iterations=1, stream=None):
        capi.check(capi.lib().pamg_matrix_gauss_seidel(self.handle, x.ptr, b.ptr, capi.SWEEP[sweep],
                                                       float(omega), int(iterations), stream),
                   "pamg_matrix_gauss_seidel")

    def gauss_seidel_correction(self, x, b, r, iterations=1, stream=None):
        """symmetric sweeps in correction form (r = b - A x, x += sweep(0, r) on the zero-iterate plans; r: scratch DeviceArray); raises where the
        operator holds no such plans"""
        capi.check(capi.lib().pamg_matrix_gauss_seidel_correction(self.handle, x.ptr, b.ptr, r.ptr, int(iterations), stream), "pamg_matrix_gauss_seidel_correction")

    def dense_tri(self, mode, block_rows=0):
        """the dense block-triangular form of the symmetric sweep from zero (pamg_matrix_dense_tri): mode 0 automatic (a solver decides per level),
        1 off, 2 on wherever it fits; block_rows 0 = default.  Refused once a solver holds the operator"""
        capi.check(capi.lib().pamg_matrix_dense_tri(self.handle, int(mode), int(block_rows)), "pamg_matrix_dense_tri")

    def dense_tri_info(self):
        """state of the dense block-triangular form: dict (built = 0 where the operator does not hold it)"""
        a = (C.c_int64 * 16)()
        gr = C.c_double(0.0)
        capi.check(capi.lib().pamg_matrix_dense_tri_info(self.handle, a, C.byref(gr)), "pamg_matrix_dense_tri_info")
        d = dict(zip(("built", "blocks", "block_rows", "bytes", "off_block_entries", "zero_launches", "correction_launches", "auto_eligible",
                      "declined_by_growth", "inverse_us", "mode", "kernel_launches", "resident_bytes"), (int(v) for v in a)))
        d["growth"] = gr.value
        return d

    def gauss_seidel_x0(self, x, b, sweep="symmetric", omega=1.0, iterations=1, x_is_zero=False, stream=None):
        capi.check(capi.lib().pamg_matrix_gauss_seidel_x0(self.handle, x.ptr, b.ptr, capi.SWEEP[sweep], float(omega), int(iterations),
                                                          int(bool(x_is_zero)), stream), "pamg_matrix_gauss_seidel_x0")

    def polynomial(self, x, b, work, coefficients, iterations=1, x_is_zero=False, stream=None):
        co = np.ascontiguousarray(coefficients, dtype=np.float64)
        capi.check(capi.lib().pamg_matrix_polynomial(self.handle, x.ptr, b.ptr, work.ptr, capi.ptr(co),
                                                     co.size, int(iterations), int(bool(x_is_zero)), stream),
                   "pamg_matrix_polynomial")

    def block_jacobi(self, x, b, work, Dinv, omega, iterations=1, stream=None):
        capi.check(capi.lib().pamg_matrix_block_jacobi(self.handle, x.ptr, b.ptr, work.ptr, Dinv.ptr,
                                                       float(omega), int(iterations), stream),
                   "pamg_matrix_block_jacobi")

    def block_gauss_seidel(self, x, b, Dinv, sweep="forward", iterations=1, stream=None):
        capi.check(capi.lib().pamg_matrix_block_gauss_seidel(self.handle, x.ptr, b.ptr, Dinv.ptr,
                                                             capi.SWEEP[sweep], int(iterations), stream),
                   "pamg_matrix_block_gauss_seidel")

    def free(self):
        if getattr(self, "handle", None):
            try:
                capi._lib.pamg_matrix_destroy(self.handle)
            except Exception:       # pragma: no cover
                pass
            self.handle = None

    def __del__(self):
        self.free()


def _set_smoother(lib, S, level, which, s: Optional[SmootherSpec], dtype, aux, fast=False, schwarz=None):
    if s is None or s.kind == "none":
        capi.check(lib.pamg_solver_set_smoother(S, level, which, 0, 0, 1.0, 0, None, 0, None, 1), "set_smoother")
        return
    if s.kind in ("gauss_seidel_ne", "gauss_seidel_nr", "jacobi_ne"):
        Dinv = np.ascontiguousarray(s.Dinv, dtype=dtype)
        At = None
        if s.At is not None:
            At = DeviceMatrix(s.At)
            aux.append(At)                      # borrowed by the solver: keep it alive
        Ar = None
        if getattr(s, "Ar", None) is not None:
            Ar = DeviceMatrix(s.Ar)
            aux.append(Ar)
        if fast:
            # order = 'fast': the Kaczmarz sweeps over these operators run lane-parallel too (csrc/pamg_kz.hip)
            for m_ in (At, Ar):
                if m_ is not None:
                    m_.tune(gs_order=1)
        capi.check(lib.pamg_solver_set_ne_smoother(S, level, which, capi.SMOOTH[s.kind], int(s.iterations), float(s.omega),
                                                   capi.SWEEP.get(s.sweep, 0), capi.ptr(Dinv), At.handle if At else None,
                                                   Ar.handle if Ar else None),
                   f"pamg_solver_set_ne_smoother({s.kind})")
        return
    if s.kind in capi.KRYLOV:
        At = None
        if s.At is not None:
            At = DeviceMatrix(s.At)
            aux.append(At)                      # borrowed by the solver: keep it alive
        capi.check(lib.pamg_solver_set_krylov_smoother(S, level, which, capi.KRYLOV[s.kind], float(s.tol), int(s.iterations),
                                                       int(s.restart), At.handle if At else None),
                   f"pamg_solver_set_krylov_smoother({s.kind})")
        return
    if s.kind in ("cf_jacobi", "fc_jacobi"):
        F = np.ascontiguousarray(s.Fpts, dtype=np.int32)
        Cp = np.ascontiguousarray(s.Cpts, dtype=np.int32)
        capi.check(lib.pamg_solver_set_cf_smoother(S, level, which, capi.SMOOTH[s.kind], int(s.iterations),
                                                   int(s.f_iterations), int(s.c_iterations), float(s.omega),
                                                   capi.ptr(F), F.size, capi.ptr(Cp), Cp.size),
                   f"pamg_solver_set_cf_smoother({s.kind})")
        return
    if s.kind == "schwarz":
        Ar = None
        if getattr(s, "Ar", None) is not None:
            Ar = DeviceMatrix(s.Ar)
            aux.append(Ar)                      # borrowed by the solver: keep it alive
        Sp, Sj = np.ascontiguousarray(s.subdomain_ptr, dtype=np.int32), np.ascontiguousarray(s.subdomain, dtype=np.int32)
        report = {"path": s.blocks_by, **(s.setup_report or {})}
        if schwarz is not None and schwarz["setup"] == "device" and s.blocks_by != "device":
            # the blocks are rebuilt on the device from the operator the sweep runs on and the smoother's subdomains
            from .relaxation import _schwarz_blocks_device
            last = schwarz.get("last")
            if last is not None and last[0] == level and np.array_equal(last[1], Sj) and np.array_equal(last[2], Sp):
                Tx, Tp, report = last[3:]       # pre- and post-smoother over the same subdomains: built once
            else:
                host_op = s.Ar if s.Ar is not None else schwarz["A_host"]
                Tx, Tp, report = _schwarz_blocks_device(host_op.to_scipy(), Sj, Sp, dA=Ar if Ar is not None else schwarz["A_dev"])
                schwarz["last"] = (level, Sj, Sp, Tx, Tp, report)
        else:
            Tp, Tx = np.ascontiguousarray(s.inv_subblock_ptr, dtype=np.int32), np.ascontiguousarray(s.inv_subblock, dtype=dtype)
        if schwarz is not None:
            schwarz["reports"].setdefault(level, {})["pre" if which == 0 else "post"] = report
        capi.check(lib.pamg_solver_set_schwarz_smoother(S, level, which, int(s.iterations), capi.SWEEP.get(s.sweep, 0),
                                                        Ar.handle if Ar else None, Sp.size - 1, capi.ptr(Sp), capi.ptr(Sj),
                                                        capi.ptr(Tp), capi.ptr(Tx)),
                   "pamg_solver_set_schwarz_smoother")
        return
    if s.kind in ("cf_block_jacobi", "fc_block_jacobi"):
        F = np.ascontiguousarray(s.Fpts, dtype=np.int32)
        Cp = np.ascontiguousarray(s.Cpts, dtype=np.int32)
        Dinv = np.ascontiguousarray(s.Dinv, dtype=dtype)
        capi.check(lib.pamg_solver_set_cf_block_smoother(S, level, which, capi.SMOOTH[s.kind], int(s.iterations),
                                                         int(s.f_iterations), int(s.c_iterations), float(s.omega),
                                                         capi.ptr(Dinv), int(s.blocksize), capi.ptr(F), F.size,
                                                         capi.ptr(Cp), Cp.size),
                   f"pamg_solver_set_cf_block_smoother({s.kind})")
        return
    coeffs = None
    ncoef = 0
    if s.kind == "polynomial":
        coeffs = np.ascontiguousarray(s.coefficients, dtype=np.float64)
        ncoef = coeffs.size
    Dinv = None
    if s.kind in ("block_jacobi", "block_gauss_seidel"):
        Dinv = np.ascontiguousarray(s.Dinv, dtype=dtype)
    capi.check(lib.pamg_solver_set_smoother(
        S, level, which, capi.SMOOTH[s.kind], int(s.iterations), float(s.omega),
        capi.SWEEP.get(s.sweep, 0), capi.ptr(coeffs), ncoef, capi.ptr(Dinv), int(s.blocksize)),
        f"pamg_solver_set_smoother({s.kind})")


# pamg_solver_dense_tail_info's reason codes (include/pyamg_amd.h)
DENSE_TAIL_REASONS = (None, "off", "no level meets the rule", "AMLI cycle", "Krylov smoother", "host coarse solver", "order-exact Gauss-Seidel",
                      "sharded cycle", "sweep time-out during tabulation", "guard above its bar", "fell back to level launches")
DENSE_TAIL_HARD_MAX_ROWS = 4096


def dense_tail_args(dense_tail):
    """``DeviceMultilevelSolver(dense_tail=...)`` -> (mode, max_rows) of ``pamg_solver_dense_tail``: None = automatic with the default limit,
    False = off, a dict with ``mode`` (0 automatic, 1 off, 2 forced; default 2: a caller who passes a dict asks for the form) and ``max_rows``
    (1 .. 4096, default 0 = the library's).  With None, the environment's PAMG_DENSE_TAIL decides where it is set: ``0`` = off, ``auto`` or
    ``force``, optionally with a row limit (``auto:2048``) -- for scans through tools that build their own solvers."""
    if dense_tail is None:
        import os
        env = os.environ.get("PAMG_DENSE_TAIL", "").strip()
        if env:
            word, _, rows = env.partition(":")
            if word not in ("0", "auto", "force") or (rows and not rows.isdigit()):
                raise ValueError("PAMG_DENSE_TAIL must be 0, auto[:rows] or force[:rows]")
            return dense_tail_args({"mode": {"0": 1, "auto": 0, "force": 2}[word], "max_rows": int(rows or 0)})
    if dense_tail is None or dense_tail is True:
        return 0, 0
    if dense_tail is False:
        return 1, 0
    if not isinstance(dense_tail, dict) or set(dense_tail) - {"mode", "max_rows"}:
        raise ValueError("dense_tail must be None, False or dict(mode=..., max_rows=...)")
    mode, rows = int(dense_tail.get("mode", 2)), int(dense_tail.get("max_rows", 0))
    if mode not in (0, 1, 2):
        raise ValueError("dense_tail: mode must be 0 (automatic), 1 (off) or 2 (forced)")
    if rows < 0 or rows > DENSE_TAIL_HARD_MAX_ROWS:
        raise ValueError(f"dense_tail: max_rows must lie in 0 .. {DENSE_TAIL_HARD_MAX_ROWS}")
    return mode, rows


class DeviceMultilevelSolver:
    """MI355X-resident multigrid solve phase for a reference-built hierarchy.

    Parameters
    ----------
    ml : pyamg.MultilevelSolver (duck-typed) or HierarchySpec
    device : int, HIP device ordinal
    graph : bool, replay cycles from a hipGraph (default) or launch eagerly
    autotune : bool, time a few LDS-window / streaming-policy candidates per large operator at
        upload (speed only, results are bit-identical; default on, PAMG_AUTOTUNE=0 disables)
    order : 'fast' (default; PAMG_GS_ORDER overrides) or 'exact' -- the row sums of the scalar Gauss-Seidel / SOR sweeps.
        Both keep the reference's sweep order over the rows (amg_core/relaxation.h:48-76).  'exact' adds every row's
        products in storage order and divides by a_ii: the reference's iterates bit for bit.  'fast' lets the lanes of
        a wave share a row (parallel partial sums, multiplication by 1/a_ii): the same iterates up to rounding -- residual
        norms agree with the reference to ~1e-15 relative per cycle (BASELINE's bar is 1e-10) -- at about half the
        latency per dependency level.  Every other kernel is bit-identical to the reference in both modes.
    schwarz_setup : 'reference' (default) or 'device' -- the inverted subdomain blocks of Schwarz smoothers.  'reference' ships the blocks the
        hierarchy holds (LAPACK gelss: the reference's own).  'device' builds them on the GPU from the operator the sweep runs on and the
        smoother's subdomains (``relaxation.schwarz_parameters(device=True)``: equal to the reference's to rounding, not bit for bit);
        ``stats()['schwarz_setup']`` says per level what was done.
    renumber : bool, number the unknowns of the large interior levels blob by blob on the DEVICE copy of the hierarchy (renumber.py;
        default OFF, PAMG_RENUMBER=1 enables -- it costs about as much host time as the upload of the level and pays back only over
        hundreds of cycles: DESIGN 3, round 6).  Speed only: rows are moved and columns renamed, row sums keep their stored order, the
        caller never sees a level >= 1 vector -- results are bit-identical.  Levels with order-dependent smoothers (Gauss-Seidel,
        Kaczmarz, Schwarz, block sweeps, Krylov) keep the reference's numbering; ``renumbered`` lists the levels that were changed.
    dense_tri : None (automatic), False (off on every level) or a dict ``{level: dict(mode=..., block_rows=...)}`` -- the dense block-triangular form
        of the symmetric Gauss-Seidel sweeps (``DeviceMatrix.dense_tri``; fast order, f64).  Automatic: mid-size coarse levels (more than 8192 rows,
        inverse triangles at most 16 x the operator's bytes) smoothed by symmetric Gauss-Seidel before and after.  Agrees with the merged form to rounding.
    dense_tail : None (automatic), False (off) or ``dict(mode=..., max_rows=...)`` -- the tail of the hierarchy as one dense operator
        (``pamg_solver_dense_tail``): every visit of the tail level t is one launch x_t = M b_t, M tabulated once per kind of cycle with the launches it
        replaces and checked against them.  Automatic: t = the first level of at most 1024 rows below a level of more than 32768 rows; mode 2 forces the
        first level within ``max_rows``.  Declined (``stats()['dense_tail']['declined']`` says why) for AMLI cycles, Krylov smoothers or a host coarse
        solver in the tail, and for ``order='exact'``.  Agrees with the launches to rounding (1e-13), not bit for bit.
    """

    def __init__(self, ml, device: Optional[int] = None, graph: bool = True, autotune: Optional[bool] = None,
                 level_tune=None, order: Optional[str] = None, strict: bool = True, renumber: Optional[bool] = None,
                 schwarz_setup: str = "reference", dense_tri=None, dense_tail=None):
        import os
        self.fallback = None
        self._dense_tail = dense_tail
        tail_mode, tail_rows = dense_tail_args(dense_tail)
        if schwarz_setup not in ("reference", "device"):
            raise ValueError("schwarz_setup must be 'reference' or 'device'")
        self.schwarz_setup, self._schwarz_reports = schwarz_setup, {}
        if not strict:
            # "unsupported smoothers / cycles / coarse solvers => transparent fallback to the wrapped ml (or an explicit
            # NotImplementedError if strict=True)".  The fallback is the CALLER's own solver object -- never the oracle, never a
            # CPU restatement of ours -- and it is announced once.
            try:
                self.__init__(ml, device=device, graph=graph, autotune=autotune, level_tune=level_tune, order=order, strict=True, renumber=renumber,
                              schwarz_setup=schwarz_setup, dense_tri=dense_tri, dense_tail=dense_tail)
                return
            except NotImplementedError as e:
                if isinstance(ml, HierarchySpec) or not hasattr(ml, "solve"):
                    raise
                import warnings
                warnings.warn(f"pyamg_amd: this hierarchy is not on the device path ({e}); strict=False hands every call to the wrapped "
                              "solver on the host", RuntimeWarning, stacklevel=2)
                self.free()
                self.fallback, self.ml, self.spec, self.handle = ml, ml, None, None
                self.renumbered, self.renumber_seconds = [], 0.0
                self.order = order or "fast"
                A0 = ml.levels[0].A
                self.dtype, self.shape = np.dtype(A0.dtype), tuple(A0.shape)
                self.A, self._mats, self._aux = [], [], []
                self.symmetric_smoothing = getattr(ml, "symmetric_smoothing", False)
                return
        if autotune is None:
            autotune = os.environ.get("PAMG_AUTOTUNE", "1") != "0"
        if order is None:
            order = os.environ.get("PAMG_GS_ORDER", "fast")
        if order not in ("fast", "exact"):
            raise ValueError("order must be 'fast' or 'exact'")
        self.order = order
        self._device, self._graph, self._autotune, self._level_tune = device, graph, autotune, level_tune
        # reading the hierarchy comes first: what is not on the device path is refused (NotImplementedError) before any device is touched
        self.ml = None if isinstance(ml, HierarchySpec) else ml
        self.spec = ml if isinstance(ml, HierarchySpec) else extract(ml, schwarz_setup)
        lib = capi.lib()
        if renumber is None:
            renumber = os.environ.get("PAMG_RENUMBER", "0") != "0"
        # the DEVICE copy of the hierarchy: self.spec (what `levels` shows) keeps the reference's numbering
        dev_spec, self.renumbered, self.renumber_seconds = self.spec, [], 0.0
        if renumber:
            import time
            from .renumber import renumber_levels
            t0 = time.perf_counter()
            dev_spec, orders = renumber_levels(self.spec)
            self.renumbered, self.renumber_seconds = sorted(orders), time.perf_counter() - t0
        if device is not None:
            capi.check(lib.pamg_set_device(int(device)), "pamg_set_device")
        self.dtype = np.dtype(self.spec.dtype)
        self.shape = tuple(self.spec.levels[0].A.shape)
        self._mats: List[DeviceMatrix] = []
        self._aux: List[DeviceMatrix] = []          # operators borrowed by smoothers (A^T forms)
        self.A: List[DeviceMatrix] = []
        h = C.c_void_p()
        capi.check(lib.pamg_solver_create(C.byref(h), capi.dtype_code(self.dtype)), "pamg_solver_create")
        self.handle = h
        nlev = len(self.spec.levels)
        # every operator of the hierarchy is shipped by its own host thread: structure checks, the diagonal scan, the
        # row-range and 16-bit column plans and the (pageable) copies of different operators overlap
        ops = []
        for i, L in enumerate(dev_spec.levels):
            ops += [L.A] + ([L.P, L.R] if i < nlev - 1 else [])

        # HIP's current device is per host thread and a new thread starts on device 0: the workers take over the device
        # of the calling thread (the one `device` selected above, or whatever the caller had selected before)
        cur = C.c_int(0)
        capi.check(lib.pamg_get_device(C.byref(cur)), "pamg_get_device")
        cur = int(cur.value)

        def ship(op):
            capi.check(lib.pamg_set_device(cur), "pamg_set_device")
            return DeviceMatrix(op)

        nthreads = int(os.environ.get("PAMG_UPLOAD_THREADS", "8"))
        if nthreads > 1 and len(ops) > 1:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=min(nthreads, len(ops))) as ex:
                shipped = list(ex.map(ship, ops))
        else:
            shipped = [ship(op) for op in ops]
        self._mats = list(shipped)
        shipped = iter(shipped)
        for i, L in enumerate(dev_spec.levels):
            A = next(shipped)
            P = next(shipped) if i < nlev - 1 else None
            R = next(shipped) if i < nlev - 1 else None
            self.A.append(A)
            if autotune:
                # speed-only choice of LDS window / streaming policy per large operator; the window of
                # an operator that carries order-exact sweeps is left alone (its level schedules and
                # the pipelined sweep kernels are sized for the default)
                gs_level = i < nlev - 1 and any(s is not None and s.kind in ("gauss_seidel", "sor", "block_gauss_seidel")
                                                for s in (L.pre, L.post))
                A.autotune(allow_cap=not gs_level)
                for m in (P, R):
                    if m is not None:
                        m.autotune(allow_cap=True)
            if order == "fast":
                A.tune(gs_order=1)
            if level_tune is not None:
                # speed-only knobs per level operator (DeviceMatrix.tune keywords), before the solver borrows it:
                # a dict for every level or a callable level index -> dict / None
                kw = level_tune(i) if callable(level_tune) else level_tune
                if kw:
                    A.tune(**kw)
            if dense_tri is False:
                A.dense_tri(1)
            elif dense_tri is not None and dense_tri.get(i):
                A.dense_tri(**dense_tri[i])
            capi.check(lib.pamg_solver_add_level(h, A.handle, P.handle if P else None, R.handle if R else None),
                       "pamg_solver_add_level")
            if i < nlev - 1:
                sw = {"setup": schwarz_setup, "A_host": L.A, "A_dev": A, "reports": self._schwarz_reports}
                _set_smoother(lib, h, i, 0, L.pre, self.dtype, self._aux, fast=order == "fast", schwarz=sw)
                _set_smoother(lib, h, i, 1, L.post, self.dtype, self._aux, fast=order == "fast", schwarz=sw)
        n_c = self.spec.levels[-1].A.shape[0]
        if self.spec.coarse_kind == "relax":
            # multilevel.py:765-782: sweeps of a relaxation method from x = 0 -- the smoother slot of the coarsest level
            _set_smoother(lib, h, nlev - 1, 0, self.spec.coarse_smoother, self.dtype, self._aux, fast=order == "fast",
                          schwarz={"setup": schwarz_setup, "A_host": dev_spec.levels[-1].A, "A_dev": self.A[-1], "reports": self._schwarz_reports})
            capi.check(lib.pamg_solver_set_coarse_relax(h), "set_coarse_relax")
        elif self.spec.coarse_kind == "host":
            # multilevel.py:752-762 (Krylov names other than 'cg' / 'gmres') and :786-788 (callables): the caller's own solver
            # object gets the coarse right-hand side on the host, inside the device cycle
            cs, A_c = self.spec.coarse_host
            dt = self.dtype

            def _coarse(_user, b_ptr, x_ptr, n):
                try:
                    bh = np.ctypeslib.as_array(C.cast(b_ptr, C.POINTER(C.c_double if dt == np.float64 else C.c_float)), shape=(int(n),))
                    xh = np.ctypeslib.as_array(C.cast(x_ptr, C.POINTER(C.c_double if dt == np.float64 else C.c_float)), shape=(int(n),))
                    xh[:] = np.ravel(cs(A_c, np.array(bh, dtype=dt))).astype(dt, copy=False)      # coarse_x[:] = coarse_solver(A, coarse_b)  (:618)
                    return 0
                except Exception:                    # noqa: BLE001 -- an exception must not unwind through the C frames
                    import traceback
                    traceback.print_exc()
                    return 1
            self._coarse_cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64)(_coarse)
            capi.check(lib.pamg_solver_set_coarse_host(h, C.cast(self._coarse_cb, C.c_void_p), None, n_c), "set_coarse_host")
        elif self.spec.coarse_kind == "zero":
            capi.check(lib.pamg_solver_set_coarse_dense(h, None, n_c), "set_coarse")
        else:
            M = np.ascontiguousarray(self.spec.coarse_op, dtype=self.dtype)     # row-major for the device gemv
            capi.check(lib.pamg_solver_set_coarse_dense(h, capi.ptr(M), n_c), "set_coarse")
        capi.check(lib.pamg_solver_set_graph(h, int(bool(graph))), "set_graph")
        capi.check(lib.pamg_solver_dense_tail(h, tail_mode, tail_rows), "pamg_solver_dense_tail")
        capi.check(lib.pamg_solver_finalize(h), "pamg_solver_finalize")
        self.symmetric_smoothing = getattr(self.ml, "symmetric_smoothing", False)
        self._xd = capi.DeviceArray(self.shape[0], self.dtype)
        self._bd = capi.DeviceArray(self.shape[0], self.dtype)

    # ------------------------------------------------------------------ reference-like API
    @property
    def levels(self):
        return self.spec.levels if self.spec is not None else self.fallback.levels

    def __repr__(self):
        if self.fallback is not None:
            return "DeviceMultilevelSolver (strict=False: not on the device path, calls go to the wrapped solver)\n" + repr(self.fallback)
        lines = ["DeviceMultilevelSolver (MI355X resident)", f"Number of Levels:     {len(self.spec.levels)}",
                 f"Coarse Solver:        {self.spec.coarse_name}", "  level   unknowns     nonzeros"]
        tot = sum(L.A.nnz for L in self.spec.levels)
        for i, L in enumerate(self.spec.levels):
            lines.append(f"{i:>6} {L.A.shape[0]:>11} {L.A.nnz:>12} [{100 * L.A.nnz / max(tot, 1):2.2f}%]")
        return "\n".join(lines) + "\n"

    def _need_device(self, what):
        # strict=False on a hierarchy that is not on the device path: solve / aspreconditioner / change_solve_matrix / levels go to the
        # wrapped solver; the device-resident entry points have no host twin to hand the call to
        if self.fallback is not None:
            raise NotImplementedError(f"DeviceMultilevelSolver.{what}: this hierarchy is not on the device path (strict=False handed it "
                                      "to the wrapped solver); only solve(), aspreconditioner(), change_solve_matrix() and levels are available")

    def stats(self) -> dict:
        self._need_device("stats")
        a = (C.c_int64 * 8)()
        capi.check(capi.lib().pamg_solver_stats(self.handle, a), "pamg_solver_stats")
        out = {"levels": int(a[0]), "gs_level_launches": int(a[1]), "hbm_bytes": int(a[2]), "graphs": int(a[3]),
               "sweep_timeouts_recovered": int(a[4])}
        t, fig = (C.c_int64 * 16)(), (C.c_double * 2)()
        capi.check(capi.lib().pamg_solver_dense_tail_info(self.handle, t, fig), "pamg_solver_dense_tail_info")
        # the tail of the hierarchy as one dense operator: operators built (one per kind of cycle run so far), why it was declined (None: it was not),
        # tail level and its rows, bytes, launches enqueued (a captured cycle counts once), tabulation time, the plan-time guard's figure
        out["dense_tail"] = {"built": int(t[0]), "declined": DENSE_TAIL_REASONS[int(t[1])], "level": int(t[2]), "rows": int(t[3]), "bytes": int(t[4]),
                             "applications": int(t[5]), "mode": int(t[6]), "max_rows": int(t[7]), "tabulation_ms": float(fig[0]), "guard": float(fig[1])}
        if self._schwarz_reports:
            # levels smoothed by Schwarz: what built the inverted blocks of the pre- / post-smoother ('reference': the blocks of the
            # hierarchy as given; 'device': pamg_schwarz_blocks, with its info -- entries, largest block, Jacobi sweeps of the slowest
            # block, blocks with a truncated singular value, subdomains handed to the host)
            out["schwarz_setup"] = {lvl: {k: dict(v) for k, v in r.items()} for lvl, r in sorted(self._schwarz_reports.items())}
        return out

    def cycle_device(self, xd, bd, cycle="V", cycles_per_level=1, stream=None):
        """One cycle on DEVICE vectors (DeviceArray) in place."""
        self._need_device("cycle_device")
        capi.check(capi.lib().pamg_solver_cycle(self.handle, xd.ptr, bd.ptr, capi.CYCLE[cycle],
                                                int(cycles_per_level), stream), "pamg_solver_cycle")

    def solve_device(self, xd, bd, tol=1e-5, maxiter=100, cycle="V", cycles_per_level=1, check_every=1,
                     stream=None):
        """accel=None branch of ``solve`` on DEVICE vectors; returns (residuals, n_iter, info)."""
        self._need_device("solve_device")
        res = np.zeros(int(maxiter) + 1, dtype=np.float64)
        nit, info = C.c_int(0), C.c_int(0)
        capi.check(capi.lib().pamg_solver_solve(self.handle, xd.ptr, bd.ptr, float(tol), int(maxiter),
                                                capi.CYCLE[cycle], int(cycles_per_level), int(check_every),
                                                capi.ptr(res), C.byref(nit), C.byref(info), stream),
                   "pamg_solver_solve")
        self._report_sweep_timeouts()
        return res[: nit.value + 1], nit.value, info.value

    def _report_sweep_timeouts(self):
        """A persistent sweep that gave up waiting (its workgroups were not all running: another process on the device, a debugger,
        a small partition) makes the engine switch to one launch per dependency level -- correct, but several times slower.  Say so,
        once per occurrence, instead of slowing down silently."""
        n = self.stats()["sweep_timeouts_recovered"]
        if n > getattr(self, "_timeouts_reported", 0):
            self._timeouts_reported = n
            import warnings
            warnings.warn("pyamg_amd: a persistent Gauss-Seidel sweep timed out waiting for its workgroups (is the GPU shared with another "
                          "process?); this solver now runs its sweeps as one launch per dependency level -- same results, several times "
                          "slower.  Recreate the solver on an idle device to get the persistent sweeps back.", RuntimeWarning, stacklevel=3)

    def load_device(self, xd, bd, stream=None):
        self._need_device("load_device")
        capi.check(capi.lib().pamg_solver_load(self.handle, xd.ptr, bd.ptr, stream), "pamg_solver_load")

    def iterate_device(self, k, cycle="V", cycles_per_level=1, want_residuals=True, stream=None):
        """Run exactly k x (cycle + convergence-check norm) on the resident state."""
        self._need_device("iterate_device")
        res = np.zeros(max(int(k), 1), dtype=np.float64) if want_residuals else None
        capi.check(capi.lib().pamg_solver_iterate(self.handle, int(k), capi.CYCLE[cycle], int(cycles_per_level),
                                                  capi.ptr(res), stream), "pamg_solver_iterate")
        self._report_sweep_timeouts()
        return res[:k] if want_residuals else None

    def store_device(self, xd, stream=None):
        self._need_device("store_device")
        capi.check(capi.lib().pamg_solver_store(self.handle, xd.ptr, stream), "pamg_solver_store")

    def stream(self):
        self._need_device("stream")
        s = C.c_void_p()
        capi.check(capi.lib().pamg_solver_stream(self.handle, C.byref(s)), "pamg_solver_stream")
        return s

    def solve(self, b, x0=None, tol=1e-5, maxiter=100, cycle="V", accel=None, callback=None,
              residuals=None, cycles_per_level=1, return_info=False):
        """Execute multigrid cycling on the GPU (reference: multilevel.py:398-582)."""
        if self.fallback is not None:
            return self.fallback.solve(b, x0=x0, tol=tol, maxiter=maxiter, cycle=cycle, accel=accel, callback=callback,
                                       residuals=residuals, cycles_per_level=cycles_per_level, return_info=return_info)
        b = np.asarray(b)
        x = np.zeros_like(b) if x0 is None else np.array(x0)       # copy (:464-467)
        cycle = str(cycle).upper()
        if cycle == "AMLI":
            A0 = getattr(self.ml.levels[0], "A", None) if self.ml is not None else None
            if A0 is not None and hasattr(A0, "symmetry") and A0.symmetry != "hermitian":
                raise ValueError("AMLI cycles require symmetry to be hermitian")       # multilevel.py:474-477
            if accel is not None and accel != "fgmres":
                raise ValueError("AMLI cycles require acceleration (accel) to be fgmres, or no acceleration")
        if cycle not in capi.CYCLE:
            raise TypeError(f"Unrecognized cycle type ({cycle})")
        n = self.shape[0]
        if b.size != n or x.size != n:
            raise ValueError("b and x0 must have as many entries as the fine-level operator has rows")

        if accel is not None:
            return self._solve_accel(b, x0, tol, maxiter, cycle, accel, callback, residuals, return_info)
        if maxiter is None or int(maxiter) < 1:
            # the reference loops `while True ... if it == maxiter` (multilevel.py:558-580): nothing but a positive
            # integer terminates it by count -- refuse instead of spinning
            raise ValueError("maxiter must be a positive integer when no accelerator is given")

        tp = np.result_type(b.dtype, x.dtype, self.dtype)          # upcast (:551-552)
        if np.dtype(tp) != self.dtype:
            raise NotImplementedError(f"solve in {tp} with a {self.dtype} hierarchy is not on the device path")
        self._bd.upload(np.ravel(b).astype(tp, copy=False))
        self._xd.upload(np.ravel(x).astype(tp, copy=False))
        if callback is None:
            res, nit, info = self.solve_device(self._xd, self._bd, tol, maxiter, cycle, cycles_per_level, 1)
            if residuals is not None:
                residuals[:] = list(res)
            out = self._xd.download()
            return (out, info) if return_info else out
        # callback(x) needs a host copy of the iterate after every cycle (:571-572)
        hist, it, info = None, 0, 0
        while True:
            res, _, info1 = self.solve_device(self._xd, self._bd, tol, 1, cycle, cycles_per_level, 1)
            if hist is None:
                hist = [res[0]]
                normb = np.linalg.norm(np.ravel(b))
                normb = 1.0 if normb == 0.0 else normb
            hist.append(res[-1])
            it += 1
            xh = self._xd.download()
            callback(xh)
            if res[-1] < tol * normb:
                info = 0
                break
            if it == maxiter:
                info = it
                break
        if residuals is not None:
            residuals[:] = hist
        return (xh, info) if return_info else xh

    def pcg_device(self, xd, bd, tol=1e-5, maxiter=100, cycle="V", cycles_per_level=1, stream=None):
        """Device-resident preconditioned CG (krylov/_cg.py, criteria 'rr') on DEVICE vectors;
        returns (residuals, n_iter, info)."""
        self._need_device("pcg_device")
        if maxiter is None:                                  # krylov/_cg.py:92-96
            maxiter = int(1.3 * self.shape[0]) + 2
        elif maxiter < 1:
            raise ValueError("Number of iterations must be positive")
        res = np.zeros(int(maxiter) + 1, dtype=np.float64)
        nit, info = C.c_int(0), C.c_int(0)
        capi.check(capi.lib().pamg_solver_pcg(self.handle, xd.ptr, bd.ptr, float(tol), int(maxiter), capi.CYCLE[cycle],
                                              int(cycles_per_level), capi.ptr(res), C.byref(nit), C.byref(info), stream),
                   "pamg_solver_pcg")
        return res[: nit.value + 1], nit.value, info.value

    def gmres_device(self, xd, bd, tol=1e-5, maxiter=None, restart=None, cycle="V", cycles_per_level=1, stream=None):
        """Device-resident GMRES, the reference's default Householder variant (krylov/_gmres_householder.py:
        left-preconditioned, residuals are preconditioned-residual norms); returns (residuals, n_iter, info)."""
        self._need_device("gmres_device")
        return self.fgmres_device(xd, bd, tol, maxiter, restart, cycle, cycles_per_level, stream, _entry="pamg_solver_gmres")

    def fgmres_device(self, xd, bd, tol=1e-5, maxiter=None, restart=None, cycle="V", cycles_per_level=1, stream=None,
                      _entry="pamg_solver_fgmres"):
        """Device-resident flexible GMRES (krylov/_fgmres.py's control flow and residual history) on
        DEVICE vectors; returns (residuals, n_iter, info)."""
        self._need_device("fgmres_device")
        n = self.shape[0]
        inner = min(int(restart), n) if restart else (min(int(maxiter), n) if maxiter else min(n, 40))
        outer = (int(maxiter) if maxiter else 1) if restart else 1
        cap = 1 + outer * (inner + 1)
        res = np.zeros(cap, dtype=np.float64)
        nres, nit, info = C.c_int(0), C.c_int(0), C.c_int(0)
        capi.check(getattr(capi.lib(), _entry)(self.handle, xd.ptr, bd.ptr, float(tol), int(maxiter or 0), int(restart or 0),
                                               capi.CYCLE[cycle], int(cycles_per_level), capi.ptr(res), cap, C.byref(nres),
                                               C.byref(nit), C.byref(info), stream), _entry)
        return res[: min(nres.value, cap)], nit.value, info.value

    def krylov_device(self, method, xd, bd, tol=1e-5, maxiter=None, cycle="V", cycles_per_level=1, stream=None):
        """Device-resident BiCGStab / CR / steepest descent / minimal residual (krylov/_bicgstab.py, _cr.py,
        _steepest_descent.py, _minimal_residual.py, criteria 'rr') on DEVICE vectors; returns (residuals, n_iter, info).
        minimal_residual reports preconditioned norms ||M r||, as the reference does."""
        self._need_device("krylov_device")
        if method not in capi.ACCEL:
            raise ValueError(f"krylov_device: unknown method {method!r} (one of {sorted(capi.ACCEL)})")
        n = self.shape[0]
        if maxiter is None:                                  # the methods' own defaults
            maxiter = {"bicgstab": n + 5, "steepest_descent": n}.get(method, int(1.3 * n) + 2)
        elif maxiter < 1:
            raise ValueError("Number of iterations must be positive")
        cap = int(maxiter) + 1
        res = np.zeros(cap, dtype=np.float64)
        nres, nit, info = C.c_int(0), C.c_int(0), C.c_int(0)
        capi.check(capi.lib().pamg_solver_krylov(self.handle, capi.ACCEL[method], xd.ptr, bd.ptr, float(tol), int(maxiter),
                                                 capi.CYCLE[cycle], int(cycles_per_level), capi.ptr(res), cap, C.byref(nres),
                                                 C.byref(nit), C.byref(info), stream), "pamg_solver_krylov")
        return res[: min(nres.value, cap)], nit.value, info.value

    # the reference's warnings on info == -1 (krylov/_cr.py:195, _minimal_residual.py:137, _steepest_descent.py:148/164/193)
    _BREAKDOWN = {"cr": "\nSingular preconditioner detected in CR, ceasing iterations\n",
                  "minimal_residual": "\nIndefinite matrix detected in minimal residual, stopping.\n"}

    def _solve_accel(self, b, x0, tol, maxiter, cycle, accel, callback, residuals, return_info):
        """multilevel.py:479-535.  Without a callback, on a fine level of more than one unknown and in the hierarchy's dtype,
        these accelerators run entirely on the device: 'cg' (``pamg_solver_pcg``), 'fgmres' (``pamg_solver_fgmres``), 'gmres' and
        'gmres_householder' (``pamg_solver_gmres``), 'bicgstab', 'cr', 'steepest_descent' and 'minimal_residual'
        (``pamg_solver_krylov``).  Everything else -- callables, ``callback=``, 'cgne' / 'cgnr' / 'gmres_mgs', SciPy's
        names -- is the host Krylov method of the reference / SciPy around the device preconditioner."""
        if accel == "cg" and not self.symmetric_smoothing and self.ml is not None:
            from warnings import warn
            warn("Incompatible non-symmetric multigrid preconditioner detected, due to presmoother/postsmoother "
                 "combination. CG requires SPD preconditioner, not just SPD matrix.")
        if accel == "cg" and callback is None and np.result_type(b.dtype, self.dtype) == self.dtype:
            x = np.zeros(self.shape[0], dtype=self.dtype) if x0 is None else np.ravel(np.array(x0)).astype(self.dtype)
            self._bd.upload(np.ravel(b).astype(self.dtype, copy=False))
            self._xd.upload(x)
            res, nit, info = self.pcg_device(self._xd, self._bd, tol, maxiter, cycle)
            if info == -1:
                from warnings import warn
                warn("\nIndefinite matrix or preconditioner detected in CG, aborting\n")
            if residuals is not None:
                residuals[:] = list(res)
            out = self._xd.download()
            return (out, info) if return_info else out
        device_ok = callback is None and self.shape[0] > 1 and np.result_type(b.dtype, self.dtype) == self.dtype
        if device_ok and isinstance(accel, str) and (accel in ("fgmres", "gmres", "gmres_householder") or accel in capi.ACCEL):
            x = np.zeros(self.shape[0], dtype=self.dtype) if x0 is None else np.ravel(np.array(x0)).astype(self.dtype)
            self._bd.upload(np.ravel(b).astype(self.dtype, copy=False))
            self._xd.upload(x)
            if accel in capi.ACCEL:
                res, nit, info = self.krylov_device(accel, self._xd, self._bd, tol, maxiter, cycle)
                if info == -1 and accel in self._BREAKDOWN:
                    from warnings import warn
                    warn(self._BREAKDOWN[accel])
                elif info == -1 and accel == "steepest_descent":
                    from warnings import warn
                    # an indefinite preconditioner stops the reference before the iteration's history entry, an indefinite matrix
                    # after the previous one; a singular preconditioner ((r, M r) == 0 exactly, also -1 through the C ABI) gets
                    # the second text
                    warn("\nIndefinite preconditioner detected in steepest descent, stopping.\n" if len(res) == nit else
                         "\nIndefinite matrix detected in steepest descent, aborting\n")
            else:
                run = self.fgmres_device if accel == "fgmres" else self.gmres_device
                res, nit, info = run(self._xd, self._bd, tol, maxiter, None, cycle)
            if residuals is not None:
                residuals[:] = list(res)
            out = self._xd.download()
            return (out, info) if return_info else out
        return self._host_krylov(b, x0, tol, maxiter, cycle, accel, callback, residuals, return_info)

    def _host_krylov(self, b, x0, tol, maxiter, cycle, accel, callback, residuals, return_info):
        """Host Krylov method around the device cycle (reference: multilevel.py:494-535).  ``accel`` is a callable or
        the name of one -- looked up in the reference package's ``krylov`` module when this solver wraps a reference
        hierarchy, else in ``scipy.sparse.linalg``.  The two families differ in how they report residuals: the
        reference's solvers take ``residuals=``/``tol=``, SciPy's take ``rtol=``/``atol=`` and only a callback."""
        import scipy.sparse.linalg as sla
        A = self.spec.levels[0].A.to_scipy()
        solver = accel if callable(accel) else self._find_krylov(accel, sla)
        M = self.aspreconditioner(cycle=cycle)
        finish = (lambda x, info: (x, info)) if return_info else (lambda x, info: x)

        def pyamg_style():
            return solver(A, b, x0=x0, tol=tol, maxiter=maxiter, M=M, callback=callback, residuals=residuals)

        def scipy_style():
            cb = callback
            if residuals is not None:
                start = np.zeros_like(b) if x0 is None else np.asarray(x0)
                residuals[:] = [np.linalg.norm(b - A @ start)]

                def cb(xk):                                  # SciPy hands over the iterate or (GMRES) a residual norm
                    residuals.append(xk if np.isscalar(xk) else np.linalg.norm(b - A @ xk))
                    if callback is not None:
                        callback(xk)
            return solver(A, b, x0=x0, maxiter=maxiter, M=M, callback=cb, rtol=tol, atol=0)

        try:
            return finish(*pyamg_style())
        except TypeError:                                    # no ``residuals=`` / ``tol=``: a SciPy-style signature
            return finish(*scipy_style())

    def _find_krylov(self, name, sla):
        pkg = None
        if self.ml is not None:
            import importlib
            try:
                pkg = importlib.import_module(type(self.ml).__module__.split(".")[0] + ".krylov")
            except Exception:       # pragma: no cover
                pkg = None
        return getattr(pkg, name) if pkg is not None and hasattr(pkg, name) else getattr(sla, name)

    def change_solve_matrix(self, A):
        """Swap the fine-level operator (reference: multilevel.py:320-337 -- the host solver
        rebuilds its level-0 smoothers) and re-ship the hierarchy: the resident copy is
        invalid once the host ``ml`` changes."""
        if self.ml is None:
            raise NotImplementedError("change_solve_matrix needs the wrapped reference solver")
        if self.fallback is not None:
            return self.fallback.change_solve_matrix(A)
        self.ml.change_solve_matrix(A)
        ml = self.ml
        device, graph, autotune, level_tune = self._device, self._graph, self._autotune, self._level_tune
        self.free()
        self.__init__(ml, device=device, graph=graph, autotune=autotune, level_tune=level_tune, order=self.order, dense_tail=self._dense_tail)

    def aspreconditioner(self, cycle="V"):
        """multilevel.py:355-396: LinearOperator applying one cycle from x = 0."""
        from scipy.sparse.linalg import LinearOperator

        def matvec(b):
            return self.solve(b, maxiter=1, cycle=cycle, tol=1e-12)

        return LinearOperator(self.shape, matvec, dtype=self.dtype)

    def free(self):
        if getattr(self, "handle", None):
            try:
                capi._lib.pamg_solver_destroy(self.handle)
            except Exception:       # pragma: no cover
                pass
            self.handle = None
        for m in getattr(self, "_mats", []) + getattr(self, "_aux", []):
            m.free()
        self._mats = []
        self._aux = []

    def __del__(self):
        self.free()
