"""GPU parity at the sizes where the planners choose the forms the benchmarks run.

The committed fixtures (40^2, 12^3, 14^2 hierarchies) only reach the single-workgroup and one-XCD forms.  Here smoothed-
aggregation hierarchies of 0.26 M - 1.23 M rows are built at test time WITHOUT the reference (tests/midsize.py) and
DeviceMultilevelSolver is compared with the oracle's restatement of the solve (oracle.OracleSolver) under the reference's
protocol (b = 0, x0 = rand; 10 cycles, 3 on the largest cases).  Bars: those of test_gpu_solver.py (f64: residual norms
1e-10 relative, iterates 1e-12; f32: 2e-4).  Every case also asserts graph replay == eager launches == a second solve
(bits), no flow error on any level, and THE FORM THAT RAN on each level: a case that passes because a planner declined
proves nothing, so it fails.

The fast order's rounding is measured against the long-double oracle (x86-64 80-bit, oracle/amg_oracle.c): the device's
error may be at most max(8 e_seq, 32 u g), e_seq the fp64 sequential sweep's own error, u = 2^-53, g the growth factor
of the merged form (1 elsewhere)."""
import numpy as np
import pytest

import midsize as M
from oracle import oracle as orc
from pyamg_amd import DeviceMultilevelSolver
from pyamg_amd import _capi as capi
from pyamg_amd.multilevel import DeviceMatrix

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
C3 = "poisson:64x96x200"            # 1.23 M rows, 200-row lines: 3 full 64-row chunks and a partial one
C4 = "poisson:72x96x128"            # nx a multiple of 64, 72 planes: not a multiple of 8 kz
L2 = "poisson:1000x1000"            # 1000-row lines
C5 = "elasticity:47"                # 101 614 block rows, BSR(3,3)
F32 = "poisson:64x64x64"
NR = "convdiff:64"


def _parity(spec, k, order="fast", level_tune=None, tag=""):
    """solve under the reference's protocol on the device (graph replay, a second replay, eager) and on the oracle; returns the solver"""
    f32 = spec.dtype == np.float32
    n = spec.levels[0].A.shape[0]
    x0 = np.random.RandomState(77).rand(n).astype(spec.dtype)
    b = np.zeros_like(x0)
    dml = DeviceMultilevelSolver(spec, graph=True, order=order, level_tune=level_tune)
    r1, r2, r3 = [], [], []
    x1 = dml.solve(b, x0=x0, tol=1e-30, maxiter=k, residuals=r1)
    x2 = dml.solve(b, x0=x0, tol=1e-30, maxiter=k, residuals=r2)
    capi.check(capi.lib().pamg_solver_set_graph(dml.handle, 0), "pamg_solver_set_graph")
    x3 = dml.solve(b, x0=x0, tol=1e-30, maxiter=k, residuals=r3)
    assert np.array_equal(x1, x2) and r1 == r2, "a second solve must give the same bits"
    assert np.array_equal(x1, x3) and r1 == r3, "graph replay and eager launches must give the same bits"
    for i, A in enumerate(dml.A):
        assert not A.flow_error(), f"flow error on level {i}"
    ro = []
    xo = orc.OracleSolver(spec).solve(b, x0=x0, tol=1e-30, maxiter=k, residuals=ro)
    r1, ro = np.array(r1), np.array(ro)
    assert r1.shape == ro.shape == (k + 1,)
    rel = float(np.max(np.abs(r1 - ro) / ro))
    dx = float(np.linalg.norm(x1 - xo) / np.linalg.norm(xo))
    bar_r, bar_x = (2e-4, 2e-4) if f32 else (1e-10, 1e-12)
    print(f"\n[midsize] {tag}: residual {rel:.2e} = {rel / bar_r:.1e} of its bar, iterate {dx:.2e} = {dx / bar_x:.1e} of its bar; "
          f"residuals {ro[0]:.3e} -> {ro[-1]:.3e}")
    assert rel <= bar_r, rel
    assert dx <= bar_x, dx
    return dml


def _assert_fine_lines(A, line_len, grid):
    nlines = int(np.prod(grid))
    for which in (0, 1):
        li = A.line_info(which)
        assert li["lines"] == nlines, (which, li)                      # one line per grid line
        assert li["chunks"] == nlines * -(-line_len // 64), (which, li)  # 64-row chunks, the last one partial
        assert li["line_levels"] == sum(grid) - len(grid) + 1, (which, li)   # lines hand off along the wavefront of the grid of lines
    assert A.lanem_info(0)["rows"] == 0 and A.tile_info(0)["tiles"] == 0


def _assert_merged(A):
    for which in (0, 1):
        mi = A.lanem_info(which)
        assert mi["rows"] == A.shape[0] and 0 < mi["super_levels"] < mi["dependency_levels"], (which, mi)


def _assert_unmerged_lanes(A):
    for which in (0, 1):
        assert A.lanem_info(which)["rows"] == 0, which
        assert A.lane_info(which)["groups"] > 0, which


# ----------------------------------------------------------------- solver-level parity
def test_c3_fast_order_line_scan_and_merged_lanes():
    spec = M.hierarchy(C3, ("gs", "symmetric"))
    dml = _parity(spec, 3, "fast", tag="C3 fast")
    _assert_fine_lines(dml.A[0], 200, (64, 96))
    _assert_merged(dml.A[1])


def test_c3_exact_order_tiles_and_forced_granular():
    spec = M.hierarchy(C3, ("gs", "symmetric"))
    dml = _parity(spec, 3, "exact", level_tune=lambda i: dict(gs_mode=2, gran_xcd=2) if i == 1 else None, tag="C3 exact")
    A0, A1 = dml.A[0], dml.A[1]
    for which in (0, 1):
        assert A0.tile_info(which)["tiles"] > 0, which                 # the tiled sweep carries the fine level
        assert A0.line_info(which)["lines"] == 0 and A0.lane_info(which)["groups"] == 0
        assert A1.tile_info(which)["tiles"] == 0 and A1.lane_info(which)["groups"] == 0 and A1.lanem_info(which)["rows"] == 0
    # the granular sweep is what level 1 runs with these settings: its profile (allocated at launch, so not inside the solver's captured
    # graphs) is filled on a copy of the operator swept eagerly, and that sweep is the oracle's bits
    op1 = spec.levels[1].A
    dA = DeviceMatrix(op1)
    dA.tune(gs_mode=2, gran_xcd=2, gs_prof=1)
    rng = np.random.RandomState(3)
    x, b = rng.rand(op1.shape[0]), rng.rand(op1.shape[0])
    dx, db = capi.DeviceArray.from_host(x), capi.DeviceArray.from_host(b)
    dA.gauss_seidel(dx, db, sweep="symmetric")
    ref = x.copy(); orc.relax_gauss_seidel(op1, ref, b, 1, "symmetric")
    assert np.array_equal(dx.download(), ref)
    prof = dA.gs_profile(0)
    assert prof.shape[0] > 0 and np.any(prof != 0), prof.shape        # the granular kernel ran and stamped its ranges
    assert dA.tile_info(0)["tiles"] == 0 and not dA.flow_error()
    dA.free()


@pytest.mark.parametrize("pre,post", [(("gs", "symmetric"), ("sor", 1.3, "forward")), (("sor", 1.3, "forward"), ("sor", 1.3, "backward"))],
                         ids=["gs_then_sor", "sor_both"])
def test_c3_sor_takes_the_unmerged_lane_layout(pre, post):
    """SOR with omega = 1.3 on CSR levels (where omega takes effect, relaxation.py:326-346): level 1 (30 entries per row, > 8 dependency
    levels) would get the merged layout, whose coefficients do not know omega.  Its schedules must be built unmerged before anything runs:
    the first solve replays a graph, and a lazy build inside that capture fails.  Parity with the oracle (which applies omega on CSR) shows
    the SOR epilogue ran on every level."""
    spec = M.hierarchy(C3, pre, post, scalar_csr=True)
    assert all(L.A.fmt == "csr" for L in spec.levels)
    A1 = spec.levels[1].A
    assert A1.nnz >= 12 * A1.shape[0]
    dml = _parity(spec, 3, "fast", tag=f"C3 SOR {pre[0]}/{post[0]} (CSR levels)")
    assert dml.A[1].info()["gs_levels_fwd"] >= 8
    _assert_unmerged_lanes(dml.A[1])


def test_c3_sor_on_bsr_levels_keeps_the_merged_layout():
    """on the BSR(1,1) levels of the reference's SA setup 'SOR' is a plain Gauss-Seidel sweep (omega ignored, relaxation.py:343-346): the
    merged layout stays"""
    spec = M.hierarchy(C3, ("gs", "symmetric"), ("sor", 1.3, "forward"))
    assert spec.levels[1].A.fmt == "bsr"
    dml = _parity(spec, 3, "fast", tag="C3 SOR on BSR(1,1) levels")
    _assert_merged(dml.A[1])


def test_c4_chebyshev_runs_the_lattice_row_masks():
    spec = M.hierarchy(C4, ("chebyshev", 3))
    dml = _parity(spec, 3, "fast", tag="C4 Chebyshev")
    rm = dml.A[0].row_masks()
    assert rm["lattice"] > 0 and rm["entries"] == 7, rm               # the fused h = c0 r store of the lattice kernel


@pytest.mark.parametrize("line_scan", [None, 2], ids=["planner", "line_scan"])
def test_long_2d_lines(line_scan):
    """1000-row lines, 1999 dependency levels.  The line scan's estimate never prefers it on a 2-D grid in natural order, so the planner
    keeps the fine level on the lane-parallel form; tune line_scan = 2 takes the line scan anyway: 1000 lines of 16 chunks (the last
    one partial)."""
    spec = M.hierarchy(L2, ("gs", "symmetric"))
    dml = _parity(spec, 3, "fast", level_tune=(lambda i: dict(line_scan=2) if i == 0 else None) if line_scan else None,
                  tag=f"2-D 1000^2 ({'line scan' if line_scan else 'planner'})")
    A0 = dml.A[0]
    assert A0.info()["gs_levels_fwd"] >= 999 and A0.info()["gs_levels_bwd"] >= 999
    if line_scan:
        _assert_fine_lines(A0, 1000, (1000,))
    else:
        _assert_unmerged_lanes(A0)
        assert A0.line_info(0)["lines"] == 0


@pytest.mark.parametrize("smoother,order", [(("block_gs", "symmetric"), "fast"), (("block_gs", "symmetric"), "exact"),
                                            (("block_jacobi",), "fast"), (("gs", "symmetric"), "fast")],
                         ids=["block_gs_fast", "block_gs_exact", "block_jacobi", "point_gs_fast"])
def test_c5_elasticity_block_forms(smoother, order):
    spec = M.hierarchy(C5, smoother)
    assert spec.levels[0].A.blocksize == (3, 3) and spec.levels[0].A.shape[0] // 3 >= 100_000
    dml = _parity(spec, 3, order, tag=f"C5 {smoother[0]} {order}")
    A0 = dml.A[0]
    if smoother[0] == "block_gs" and order == "fast":
        for which in (0, 1):
            assert A0.lane_info(which)["groups"] > 0, which            # bsr_lane
            assert A0.lane_info(which)["launch_grid"] > 8, which       # across the chip, not one XCD's handful of workgroups
    if smoother[0] == "block_gs" and order == "exact":
        assert A0.lane_info(0)["groups"] == 0
    if smoother[0] == "gs":
        assert A0.point_twin() == 1                                     # the BSR point sweep runs on its scalar twin


def test_f32_unmerged_lanes_on_level_1():
    spec = M.hierarchy(F32, ("gs", "symmetric"), dtype="float32")
    assert spec.dtype == np.float32
    dml = _parity(spec, 10, "fast", tag="f32 64^3")
    _assert_unmerged_lanes(dml.A[1])


def test_normal_equations_kaczmarz_lanes():
    spec = M.hierarchy(NR, ("gs_nr", "symmetric"))
    dml = _parity(spec, 10, "fast", tag="convection-diffusion gauss_seidel_nr")
    At0 = dml._aux[0]                                                   # the level-0 smoother's A^T (CSR of A's CSC arrays)
    assert At0.shape == spec.levels[0].A.shape
    assert At0.kz_info(0)["groups"] > 0 and At0.kz_info(1)["groups"] > 0


# ----------------------------------------------------------------- the fast order against a long-double yardstick
def _ld(op):
    from dataclasses import replace
    return replace(op, data=op.data.astype(np.longdouble))


def _err(x, ref):
    return float(np.max(np.abs(x - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("which", [(C3, 0, None), (C3, 1, None), (L2, 0, None), (L2, 0, 2)],
                         ids=["c3_level0", "c3_level1", "2d_level0", "2d_level0_line_scan"])
def test_fast_order_rounding_against_long_double(which):
    assert np.finfo(np.longdouble).nmant >= 63
    name, lvl, line_scan = which
    op = M.level_op(name, lvl, csr=True)
    opl = _ld(op)
    n = op.shape[0]
    rng = np.random.RandomState(5)
    x, b = rng.rand(n), rng.rand(n)
    sweeps = [("forward", 1.0), ("backward", 1.0), ("symmetric", 1.0), ("forward", 1.3)]
    refs, lds = [], []
    for sw, om in sweeps:
        r = x.copy(); orc.relax_gauss_seidel(op, r, b, 1, sw, om); refs.append(r)
        rl = x.astype(np.longdouble); orc.relax_gauss_seidel(opl, rl, b.astype(np.longdouble), 1, sw, om); lds.append(rl)
    dx, db = capi.DeviceArray.from_host(x), capi.DeviceArray.from_host(b)
    # exact order: the f64 oracle's bits
    dA = DeviceMatrix(op)
    for (sw, om), r in zip(sweeps, refs):
        dx.upload(x)
        dA.gauss_seidel(dx, db, sweep=sw, omega=om)
        assert np.array_equal(dx.download(), r), (sw, om)
    # resid_sumsq: the sum of squares within 64 u of the long-double one
    out = capi.DeviceArray(1, np.float64)
    dA.resid_sumsq(dx, db, out)
    xs = dx.download().astype(np.longdouble)
    yl = np.zeros(n, dtype=np.longdouble)
    orc.csr_matvec(n, opl.indptr, opl.indices, opl.data, xs, yl)
    rl = b.astype(np.longdouble) - yl
    ss = np.sum(rl * rl)
    e_ss = float(abs(out.download()[0] - ss) / ss)
    print(f"\n[midsize] resid_sumsq {name} level {lvl}: {e_ss:.2e} = {e_ss / (64 * U):.1e} of its bar")
    assert e_ss <= 64 * U, e_ss
    dA.free()
    # fast order
    dA = DeviceMatrix(op)
    dA.tune(gs_order=1, line_scan=line_scan)
    for (sw, om), r, rl in zip(sweeps, refs, lds):
        dx.upload(x)
        dA.gauss_seidel(dx, db, sweep=sw, omega=om)
        got = dx.download()
        mi = dA.lanem_info(0)
        g = mi["max_growth"] if (mi["rows"] and om == 1.0) else 1.0
        e_dev, e_seq = _err(got, rl), _err(r, rl)
        bar = max(8 * e_seq, 32 * U * g)
        form = "line" if dA.line_info(0)["lines"] else "lanem" if mi["rows"] else "lane" if dA.lane_info(0)["groups"] else "other"
        print(f"[midsize] fast {name} level {lvl} {sw} omega={om} ({form}): e_dev {e_dev:.2e}, e_seq {e_seq:.2e}, {e_dev / bar:.2f} of its bar")
        assert e_dev <= bar, (sw, om, e_dev, e_seq, g)
        assert not dA.flow_error()
    if (name == C3 and lvl == 0) or line_scan:
        assert dA.line_info(0)["lines"] > 0                            # the line scan is what was measured
    elif lvl == 1:
        assert dA.lanem_info(0)["rows"] == n                           # the merged form is what was measured
    else:
        assert dA.lane_info(0)["groups"] > 0 and dA.lanem_info(0)["rows"] == 0     # the unmerged lane form
    dA.free()


@pytest.mark.parametrize("drop", [dict(lds_entries=2048), dict(lane_merge=2)], ids=["schedules_dropped", "lane_keys"])
def test_point_twin_follows_tune_and_scaling(drop):
    """BSR(3,3) operator: a point sweep builds the scalar twin.  A tune call -- one that drops the schedules (lds_entries) or one of the
    lane keys the twin copies (lane_merge) -- then scale_values(2.0) must not leave the next point sweep on the twin's old snapshot of the
    values: it equals the oracle's sweep on 2 A"""
    op = M.level_op("elasticity:16", 0)
    assert op.blocksize == (3, 3)
    n = op.shape[0]
    rng = np.random.RandomState(9)
    x, b = rng.rand(n), rng.rand(n)
    dA = DeviceMatrix(op)
    dA.tune(gs_order=1)
    dx, db = capi.DeviceArray.from_host(x), capi.DeviceArray.from_host(b)
    dA.gauss_seidel(dx, db, sweep="forward")
    ref = x.copy(); orc.relax_gauss_seidel(op, ref, b, 1, "forward")
    assert dA.point_twin() == 1
    assert _err(dx.download(), ref) <= 1e-13
    dA.tune(**drop)
    capi.check(capi.lib().pamg_matrix_scale_values(dA.handle, 2.0), "pamg_matrix_scale_values")
    dx.upload(x)
    dA.gauss_seidel(dx, db, sweep="forward")
    from dataclasses import replace
    op2 = replace(op, data=op.data * 2.0)
    ref2 = x.copy(); orc.relax_gauss_seidel(op2, ref2, b, 1, "forward")
    assert dA.point_twin() == 1
    e = _err(dx.download(), ref2)
    assert e <= 1e-13, e
    assert not dA.flow_error()
    dA.free()
