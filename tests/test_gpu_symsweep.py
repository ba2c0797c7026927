"""The fused symmetric Gauss-Seidel sweep (tune key sym_fused: forward schedule, completion barrier, backward schedule in ONE
persistent launch) against the two directional launches it replaces, on the mid-size hierarchies of tests/midsize.py.

The fused kernels walk the same two schedules with the same per-row arithmetic, so everything here is BIT FOR BIT: the iterate
and every residual norm of a solve (sym_fused 1 against 0), graph replay == eager launches == a second solve, a single sweep per
level with x known to be zero and not.  Between launches the forward hand-off buffer must be all sentinels and the counters
zero; a directional sweep on the same operator between two fused sweeps changes nothing (it has buffers of its own); no flow
error on any level; and the info call must say that the fused form RAN on the level (line form on the fine grid, merged lanes
across the chip, merged lanes inside one XCD): a case that passes because the path declined proves nothing, so it fails.
Oracle parity: the bars of test_gpu_midsize.py (f64: residual norms 1e-10 relative, iterates 1e-12)."""
import numpy as np
import pytest

import midsize as M
from oracle import oracle as orc
from pyamg_amd import DeviceMultilevelSolver
from pyamg_amd import _capi as capi
from pyamg_amd.multilevel import DeviceMatrix

pytestmark = pytest.mark.gpu

C3 = "poisson:64x96x200"            # 1.23 M rows: line form on level 0, merged lanes below (two rows per wave on level 1)
C6 = "poisson:64x64x64"             # 0.26 M rows: level 1 one row per wave
CASES = [C3, C6]


def _solve3(spec, k, fused):
    """graph replay, a second replay, eager: the three must agree in every bit; returns (solver, x, residuals)"""
    n = spec.levels[0].A.shape[0]
    x0 = np.random.RandomState(77).rand(n)
    b = np.zeros_like(x0)
    dml = DeviceMultilevelSolver(spec, graph=True, order="fast", level_tune=dict(sym_fused=fused))
    r1, r2, r3 = [], [], []
    x1 = dml.solve(b, x0=x0, tol=1e-30, maxiter=k, residuals=r1)
    x2 = dml.solve(b, x0=x0, tol=1e-30, maxiter=k, residuals=r2)
    capi.check(capi.lib().pamg_solver_set_graph(dml.handle, 0), "pamg_solver_set_graph")
    x3 = dml.solve(b, x0=x0, tol=1e-30, maxiter=k, residuals=r3)
    assert np.array_equal(x1, x2) and r1 == r2, "a second solve must give the same bits"
    assert np.array_equal(x1, x3) and r1 == r3, "graph replay and eager launches must give the same bits"
    for i, A in enumerate(dml.A):
        assert not A.flow_error(), f"flow error on level {i}"
    return dml, x1, r1, (b, x0)


def _expected_form(A):
    """what the planners built decides what must have run: lines on both schedules -> 'line', merged lanes on both -> 'merged*'"""
    if A.line_info(0)["lines"] and A.line_info(1)["lines"]:
        return "line"
    if A.lanem_info(0)["rows"] and A.lanem_info(1)["rows"]:
        return "merged"
    return "none"


@pytest.mark.parametrize("name", CASES)
def test_solve_fused_equals_two_launches(name):
    k = 3
    spec = M.hierarchy(name, ("gs", "symmetric"))
    d1, x1, r1, (b, x0) = _solve3(spec, k, 1)
    d0, x0_, r0, _ = _solve3(spec, k, 0)
    assert np.array_equal(x1, x0_), "iterate: fused != two launches"
    assert r1 == r0, (r1, r0)
    nlev = len(d1.A)
    forms = []
    for i in range(nlev - 1):
        s1, s0 = d1.A[i].sym_info(), d0.A[i].sym_info()
        want = _expected_form(d1.A[i])
        print(f"\n[symsweep] {name} level {i}: rows {d1.A[i].shape[0]}, fused {s1}, planned {want}")
        assert s0["launches"] == 0 and s0["enabled"] == 0, (i, s0)
        forms.append(s1["form"])
        if want == "none":
            continue
        assert s1["launches"] > 0 and s1["form"].startswith(want), (i, s1, want)
        assert s1["handoff_not_sentinel"] == 0, (i, s1)              # the invariant between launches
        assert s1["counters_not_zero"] == 0, (i, s1)
        if i > 0 and want == "merged":
            assert s1["zero_launches"] > 0, (i, s1)                  # the pre-smoothing below the finest level knows x = 0
    assert forms[0] == "line", forms                                 # the fine grid ran the fused line form
    assert forms[1] == "merged", forms                               # level 1 the fused merged form across the chip
    assert "merged_one_xcd" in forms, forms                          # and a small level the one-XCD ticket form
    ro = []
    xo = orc.OracleSolver(spec).solve(b, x0=x0, tol=1e-30, maxiter=k, residuals=ro)
    r1a, ro = np.array(r1), np.array(ro)
    rel = float(np.max(np.abs(r1a - ro) / ro))
    dx = float(np.linalg.norm(x1 - xo) / np.linalg.norm(xo))
    print(f"[symsweep] {name}: residual {rel:.2e}, iterate {dx:.2e} against the oracle")
    assert rel <= 1e-10, rel
    assert dx <= 1e-12, dx
    d1.free(); d0.free()


@pytest.mark.parametrize("name", CASES)
def test_each_level_fused_equals_two_launches(name):
    ops = M.operators(name)
    ran = []
    for lvl in range(len(ops) - 1):
        op = M.level_op(name, lvl, csr=True)
        n = op.shape[0]
        rng = np.random.RandomState(11 + lvl)
        x, b = rng.rand(n), rng.rand(n)
        A1, A0 = DeviceMatrix(op), DeviceMatrix(op)
        A1.tune(gs_order=1, sym_fused=1)
        A0.tune(gs_order=1, sym_fused=0)
        dx, db = capi.DeviceArray.from_host(x), capi.DeviceArray.from_host(b)

        def sweep(A, start, zero=False, its=1):
            dx.upload(start)
            A.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=its, x_is_zero=zero)
            return dx.download()

        ref = sweep(A0, x)
        got = sweep(A1, x)
        assert np.array_equal(got, ref), f"level {lvl}: fused != two launches"
        # a directional sweep on the same operator between two fused sweeps changes nothing
        dx.upload(x)
        A1.gauss_seidel(dx, db, sweep="backward")
        A1.gauss_seidel(dx, db, sweep="forward")
        assert np.array_equal(sweep(A1, x), ref), f"level {lvl}: a directional sweep in between changed the fused sweep"
        # two iterations in one call
        assert np.array_equal(sweep(A1, x, its=2), sweep(A0, x, its=2)), f"level {lvl}: two iterations"
        # x known to be zero: the same bits with and without the word, fused and not
        z = np.zeros(n)
        ref0 = sweep(A0, z)
        assert np.array_equal(sweep(A1, z, zero=False), ref0), f"level {lvl}: x = 0, not announced"
        assert np.array_equal(sweep(A1, z, zero=True), ref0), f"level {lvl}: x = 0, announced"
        assert np.array_equal(sweep(A1, z, zero=True, its=2), sweep(A0, z, its=2)), f"level {lvl}: x = 0 holds for the first iteration only"
        s1, s0 = A1.sym_info(), A0.sym_info()
        want = _expected_form(A1)
        print(f"\n[symsweep] {name} level {lvl}: rows {n}, fused {s1}, planned {want}")
        assert s0["launches"] == 0, s0
        if want != "none":
            assert s1["launches"] >= 8 and s1["form"].startswith(want), (lvl, s1, want)
            assert s1["handoff_not_sentinel"] == 0 and s1["counters_not_zero"] == 0, (lvl, s1)
            if want == "merged":
                assert s1["zero_launches"] == 2, (lvl, s1)
        ran.append(s1["form"])
        assert not A1.flow_error() and not A0.flow_error()
        A1.free(); A0.free()
    assert ran[0] == "line" and ran[1] == "merged" and "merged_one_xcd" in ran, ran
