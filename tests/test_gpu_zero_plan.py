"""Zero-iterate plans on the device (tune key 39; host logic: tests/test_zero_plan.py) on the mid-size hierarchies of tests/midsize.py.

A cycle enters every level below the finest with x = 0, so a solver builds, per such level, the merged forward plan of tril(A) and the merged
backward plan of triu(A) and runs its symmetric pre-smoothing sweep on them: the forward half also stores the numerators w = b - s, the backward
half takes w as right-hand side.  Checked here:
  * a solver with the plans: fused launch == two launches, graph replay == eager launches == a second solve, BIT FOR BIT (the two paths walk the
    same plans with the same per-row arithmetic);
  * plans on against plans off, one announced-zero sweep per coarse level on a bare operator (key 2 against key 1): <= 1e-13 relative, the
    fast order's bar per sweep; a bare operator left alone (key 0) has no plans and runs none;
  * against the oracle over 3 cycles: residual norms <= 1e-10 relative, iterate <= 1e-12 (the bars of test_gpu_midsize.py);
  * the info calls say that the plans RAN on every level >= 1 that sweeps in the merged form, the small one-XCD level included -- a case that
    passes because the path declined proves nothing, so it fails; no flow error on any level; between launches the forward hand-off buffer is all
    sentinels and the counters are zero."""
import numpy as np
import pytest

import midsize as M
from oracle import oracle as orc
from pyamg_amd import DeviceMultilevelSolver
from pyamg_amd import _capi as capi
from pyamg_amd.multilevel import DeviceMatrix

pytestmark = pytest.mark.gpu

CASES = ["poisson:64x96x200", "poisson:64x64x64"]
SWEEP_TOL = 1e-13


def _solve3(spec, k, fused, zero_plans=0):
    """graph replay, a second replay, eager: the three must agree in every bit; returns (solver, x, residuals, (b, x0))"""
    n = spec.levels[0].A.shape[0]
    x0 = np.random.RandomState(77).rand(n)
    b = np.zeros_like(x0)
    dml = DeviceMultilevelSolver(spec, graph=True, order="fast", level_tune=dict(sym_fused=fused, zero_plans=zero_plans))
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


def _merged(A):
    return bool(A.lanem_info(0)["rows"] and A.lanem_info(1)["rows"])


@pytest.mark.parametrize("name", CASES)
def test_solver_with_zero_plans(name):
    k = 3
    spec = M.hierarchy(name, ("gs", "symmetric"))
    d1, x1, r1, (b, x0) = _solve3(spec, k, 1)
    d0, x0_, r0, _ = _solve3(spec, k, 0)
    assert np.array_equal(x1, x0_), "iterate: fused != two launches"
    assert r1 == r0, (r1, r0)
    nlev = len(d1.A)
    forms, ran_on = [], []
    for i in range(nlev - 1):
        A1, A0 = d1.A[i], d0.A[i]
        s1, s0 = A1.sym_info(), A0.sym_info()
        zf, zb = A1.lanem_info(4), A1.lanem_info(5)
        print(f"\n[zero plan] {name} level {i}: rows {A1.shape[0]}, fused {s1}, two launches {s0}")
        if zf["rows"]:
            ff, fb = A1.lanem_info(0), A1.lanem_info(1)
            ops = lambda d: (d["early_operands"] + d["old_operands"] + d["b_operands"]) / max(1, d["rows"])
            uni = lambda d: (d["unique_early"] + d["unique_old"] + d["unique_b"]) / max(1, d["rows"])
            print(f"[zero plan]   Zf: s {zf['s_max']}, super-levels {zf['super_levels']}, operands per row {ops(zf):.1f}, unique {uni(zf):.1f}, groups {zf['groups']}, old {zf['old_operands']};"
                  f" Zb: s {zb['s_max']}, super-levels {zb['super_levels']}, operands per row {ops(zb):.1f}, unique {uni(zb):.1f}, groups {zb['groups']}, old {zb['old_operands']}")
            print(f"[zero plan]   full forward: s {ff['s_max']}, super-levels {ff['super_levels']}, operands per row {ops(ff):.1f}, unique {uni(ff):.1f}, groups {ff['groups']};"
                  f" backward: super-levels {fb['super_levels']}, operands per row {ops(fb):.1f}, unique {uni(fb):.1f}, groups {fb['groups']}")
            assert zf["old_operands"] == 0 and zb["old_operands"] == 0, (i, zf, zb)          # every row of these operators has its diagonal
        forms.append(s1["form"])
        if i == 0:
            assert s1["zero_plan_launches"] == 0 and s0["zero_plan_launches"] == 0 and zf["rows"] == 0, (i, s1, s0)      # the finest level: on request only
            continue
        if not _merged(A1):
            continue
        ran_on.append(i)
        assert zf["rows"] == A1.shape[0] and zb["rows"] == A1.shape[0], (i, zf, zb)
        # every announced-zero sweep on this level (counted when enqueued or captured) ran on the plans, fused or as two launches
        assert s1["zero_plan_launches"] == s1["zero_launches"] > 0, (i, s1)
        assert s0["zero_plan_launches"] == s1["zero_plan_launches"] and s0["launches"] == 0, (i, s0)
        assert s1["handoff_not_sentinel"] == 0 and s1["counters_not_zero"] == 0, (i, s1)     # the invariants between launches
    assert 1 in ran_on and len(ran_on) >= 2, ran_on
    assert forms[1] == "merged" and "merged_one_xcd" in forms, forms                        # across the chip on level 1, the ticket form on a small level
    assert any(forms[i] == "merged_one_xcd" for i in ran_on), (forms, ran_on)
    # the same hierarchy without the plans: to rounding, cycle after cycle
    dn, xn, rn, _ = _solve3(spec, k, 1, zero_plans=1)
    for i in range(nlev - 1):
        assert dn.A[i].sym_info()["zero_plan_launches"] == 0 and dn.A[i].lanem_info(4)["rows"] == 0, i
    rel_off = float(np.max(np.abs(np.array(r1) - np.array(rn)) / np.array(rn)))
    dx_off = float(np.max(np.abs(x1 - xn)) / np.max(np.abs(xn)))
    print(f"[zero plan] {name}: against the solver without plans: residual norms {rel_off:.2e}, iterate {dx_off:.2e}")
    assert rel_off <= 1e-10 and dx_off <= 1e-12, (rel_off, dx_off)
    ro = []
    xo = orc.OracleSolver(spec).solve(b, x0=x0, tol=1e-30, maxiter=k, residuals=ro)
    r1a, ro = np.array(r1), np.array(ro)
    rel = float(np.max(np.abs(r1a - ro) / ro))
    dx = float(np.linalg.norm(x1 - xo) / np.linalg.norm(xo))
    print(f"[zero plan] {name}: residual {rel:.2e}, iterate {dx:.2e} against the oracle")
    assert rel <= 1e-10, rel
    assert dx <= 1e-12, dx
    d1.free(); d0.free(); dn.free()


@pytest.mark.parametrize("name", CASES)
def test_each_coarse_level_on_against_off(name):
    ops = M.operators(name)
    ran = []
    for lvl in range(1, len(ops) - 1):
        op = M.level_op(name, lvl, csr=True)
        n = op.shape[0]
        b = np.random.RandomState(21 + lvl).rand(n)
        z = np.zeros(n)
        mats = {}
        for key, fused in ((0, 1), (1, 1), (2, 1), (2, 0)):
            A = DeviceMatrix(op)
            A.tune(gs_order=1, sym_fused=fused, zero_plans=key)
            mats[(key, fused)] = A
        dx, db = capi.DeviceArray.from_host(z), capi.DeviceArray.from_host(b)

        def sweep(A, start, zero, its=1):
            dx.upload(start)
            A.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=its, x_is_zero=zero)
            return dx.download()

        off = sweep(mats[(1, 1)], z, True)
        bare = sweep(mats[(0, 1)], z, True)
        assert np.array_equal(bare, off), f"level {lvl}: a bare operator left alone must run the general plans"
        on = sweep(mats[(2, 1)], z, True)
        on2 = sweep(mats[(2, 0)], z, True)
        merged = _merged(mats[(2, 1)])
        s_on, s_on2, s_bare, s_off = (mats[k].sym_info() for k in ((2, 1), (2, 0), (0, 1), (1, 1)))
        err = float(np.max(np.abs(on - off)) / np.max(np.abs(off)))
        print(f"\n[zero plan] {name} level {lvl}: rows {n}, merged {merged}, on against off {err:.2e}; {s_on}")
        assert s_bare["zero_plan_launches"] == 0 and s_off["zero_plan_launches"] == 0, (lvl, s_bare, s_off)
        assert mats[(0, 1)].lanem_info(4)["rows"] == 0 and mats[(1, 1)].lanem_info(4)["rows"] == 0
        assert err <= SWEEP_TOL, (lvl, err)
        assert np.array_equal(on, on2), f"level {lvl}: fused != two launches on the zero-iterate plans"
        if merged:
            assert s_on["zero_plan_launches"] == 1 and s_on2["zero_plan_launches"] == 1 and s_on2["launches"] == 0, (lvl, s_on, s_on2)
            assert s_on["handoff_not_sentinel"] == 0 and s_on["counters_not_zero"] == 0, (lvl, s_on)
            ran.append(s_on["form"])
            # the word holds for the first iteration only; without the word the general plans run
            two_on, two_off = sweep(mats[(2, 1)], z, True, its=2), sweep(mats[(1, 1)], z, True, its=2)
            e2 = float(np.max(np.abs(two_on - two_off)) / np.max(np.abs(two_off)))
            assert e2 <= 2 * SWEEP_TOL, (lvl, e2)
            assert np.array_equal(two_on, sweep(mats[(2, 0)], z, True, its=2)), f"level {lvl}: two iterations, fused != two launches"
            assert np.array_equal(sweep(mats[(2, 1)], z, False), off), f"level {lvl}: x = 0 not announced"
            x = np.random.RandomState(5).rand(n)
            assert np.array_equal(sweep(mats[(2, 1)], x, False), sweep(mats[(1, 1)], x, False)), f"level {lvl}: a sweep from x != 0"
            assert mats[(2, 1)].sym_info()["zero_plan_launches"] == 2
            # the plans are part of what the operator reports to hold
            assert mats[(2, 1)].info()["hbm_bytes"] > mats[(1, 1)].info()["hbm_bytes"], lvl
        for A in mats.values():
            assert not A.flow_error()
            A.free()
    assert "merged" in ran and "merged_one_xcd" in ran, ran
