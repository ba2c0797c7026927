"""The CLUSTER layout of the merged lane sweep (tune key lanem_cluster = 4 / 8: rows of a super-level that are consecutive in row-index order
share a wave, which loads the union of their operands once and forms the row sums from LDS) on level 1 of the mid-size hierarchies of
tests/midsize.py -- below the size at which an automatic choice would ever take it, so the key forces it.

Against the pair / row layout (lanem_cluster = 1) a sweep of each direction and the symmetric sweep agree to 1e-13 relative (another association
of the same row sums: the bar tests/test_gpu_kernels.py holds the fast order to); the fused symmetric launch equals the two directional launches
BIT FOR BIT (one device function forms the rows in both), with x known to be zero and not; graph replay == eager launches == a second solve; the
error word stays clear and the hand-off buffers are back to sentinels between launches; and the info call must say that the cluster layout RAN."""
import numpy as np
import pytest

import midsize as M
from oracle import oracle as orc
from pyamg_amd import DeviceMultilevelSolver
from pyamg_amd import _capi as capi
from pyamg_amd.multilevel import DeviceMatrix

pytestmark = pytest.mark.gpu

C3 = "poisson:64x96x200"            # level 1: 46 K rows
C6 = "poisson:64x64x64"             # level 1: 10 K rows
TOL = 1e-13


def _rel(got, ref):
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("R", [4, 8])
@pytest.mark.parametrize("name", [C3, C6])
def test_level1_sweeps_against_the_pair_layout(name, R):
    op = M.level_op(name, 1, csr=True)
    n = op.shape[0]
    rng = np.random.RandomState(5)
    x, b = rng.rand(n), rng.rand(n)
    Ac, Ac2, Ar = DeviceMatrix(op), DeviceMatrix(op), DeviceMatrix(op)
    Ac.tune(gs_order=1, lanem_cluster=R, sym_fused=1)
    Ac2.tune(gs_order=1, lanem_cluster=R, sym_fused=0)
    Ar.tune(gs_order=1, lanem_cluster=1, sym_fused=1)
    dx, db = capi.DeviceArray.from_host(x), capi.DeviceArray.from_host(b)

    def sweep(A, start, how, zero=False, its=1):
        dx.upload(start)
        if how == "symmetric":
            A.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=its, x_is_zero=zero)
        else:
            A.gauss_seidel(dx, db, sweep=how)
        return dx.download()

    for how in ("forward", "backward", "symmetric"):
        ref, got = sweep(Ar, x, how), sweep(Ac, x, how)
        e = _rel(got, ref)
        print(f"\n[lanec] {name} level 1 ({n} rows) R={R} {how}: {e:.2e} relative to the pair layout")
        assert e <= TOL, (how, e)
        assert np.array_equal(sweep(Ac2, x, how), got), f"{how}: fused != two launches"
    assert np.array_equal(sweep(Ac, x, "symmetric", its=2), sweep(Ac2, x, "symmetric", its=2)), "two iterations"
    z = np.zeros(n)
    ref0 = sweep(Ac2, z, "symmetric")
    assert np.array_equal(sweep(Ac, z, "symmetric", zero=False), ref0), "x = 0, not announced"
    assert np.array_equal(sweep(Ac, z, "symmetric", zero=True), ref0), "x = 0, announced"
    assert _rel(ref0, sweep(Ar, z, "symmetric", zero=True)) <= TOL
    for A in (Ac, Ac2):
        for which in (0, 1):
            mi = A.lanem_info(which)
            assert mi["cluster_rows"] == R and mi["rows"] == n and (n + R - 1) // R <= mi["groups"] < n, mi      # the cluster layout is what ran
            assert mi["unique_early"] < mi["early_operands"] and mi["unique_old"] < mi["old_operands"], mi       # and its rows share operands
    mi = Ac.lanem_info(0)
    per = lambda k: mi[k] / n
    print(f"[lanec] {name} R={R}: groups {mi['groups']}, operands per row {per('early_operands') + per('old_operands') + per('b_operands'):.1f}, unique early / old / b "
          f"{per('unique_early'):.1f} / {per('unique_old'):.1f} / {per('unique_b'):.1f}, early lines {per('early_lines'):.1f}, padding {mi['padding']:.2f}, grid {mi['launch_grid']}")
    assert Ar.lanem_info(0)["cluster_rows"] == 0 and Ar.lanem_info(0)["rows"] == n
    s1, s0 = Ac.sym_info(), Ac2.sym_info()
    assert s1["launches"] > 0 and s1["form"] == "merged" and s1["zero_launches"] == 1, s1
    assert s1["handoff_not_sentinel"] == 0 and s1["counters_not_zero"] == 0, s1
    assert s0["launches"] == 0, s0
    assert not Ac.flow_error() and not Ac2.flow_error() and not Ar.flow_error()      # the error word is clear
    Ac.free(); Ac2.free(); Ar.free()


@pytest.mark.parametrize("R", [4, 8])
def test_solve_graph_equals_eager_and_fused_equals_two_launches(R):
    k = 3
    spec = M.hierarchy(C6, ("gs", "symmetric"))
    n = spec.levels[0].A.shape[0]
    x0 = np.random.RandomState(77).rand(n)
    b = np.zeros_like(x0)
    outs = []
    for fused in (1, 0):
        dml = DeviceMultilevelSolver(spec, graph=True, order="fast", level_tune=dict(sym_fused=fused, lanem_cluster=R))
        r1, r2, r3 = [], [], []
        x1 = dml.solve(b, x0=x0, tol=1e-30, maxiter=k, residuals=r1)
        x2 = dml.solve(b, x0=x0, tol=1e-30, maxiter=k, residuals=r2)
        capi.check(capi.lib().pamg_solver_set_graph(dml.handle, 0), "pamg_solver_set_graph")
        x3 = dml.solve(b, x0=x0, tol=1e-30, maxiter=k, residuals=r3)
        assert np.array_equal(x1, x2) and r1 == r2, "a second solve must give the same bits"
        assert np.array_equal(x1, x3) and r1 == r3, "graph replay and eager launches must give the same bits"
        for i, A in enumerate(dml.A):
            assert not A.flow_error(), f"flow error on level {i}"
        assert dml.A[1].lanem_info(0)["cluster_rows"] == R and dml.A[1].lanem_info(1)["cluster_rows"] == R
        si = dml.A[1].sym_info()
        assert (si["launches"] > 0 and si["form"] == "merged" and si["handoff_not_sentinel"] == 0 and si["counters_not_zero"] == 0) if fused else si["launches"] == 0, si
        outs.append((x1, r1))
        dml.free()
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1], "fused != two launches"
    ro = []
    xo = orc.OracleSolver(spec).solve(b, x0=x0, tol=1e-30, maxiter=k, residuals=ro)
    r1a, ro = np.array(outs[0][1]), np.array(ro)
    rel = float(np.max(np.abs(r1a - ro) / ro))
    dx = float(np.linalg.norm(outs[0][0] - xo) / np.linalg.norm(xo))
    print(f"\n[lanec] {C6} R={R}: residual {rel:.2e}, iterate {dx:.2e} against the oracle")
    assert rel <= 1e-10, rel
    assert dx <= 1e-12, dx
