"""The correction form of a symmetric Gauss-Seidel smoothing step (tune key 41): from x != 0 a solver's level below the finest runs r = b - A x and
then the launch announced from zero on its zero-iterate plans (tune key 39) with right-hand side r, whose backward half ADDS to x -- Gauss-Seidel is
affine, sweep(x, b) = x + sweep(0, b - A x).

The hierarchy is tests/midsize.py's convdiff:32 with scalar CSR levels (32 768 / 4 192 / 117 / 4 rows), correction forced on (key 41 = 2: the automatic
rule leaves levels this small on the general plans), in the chip-wide cluster layout (lanem_cluster = 8) and in the automatic layout (one row per wave,
the one-XCD ticket form on these levels), each as one fused launch and as two launches.  Checked:
  * fused == two launches, graph replay == eager == a second solve, BIT FOR BIT, over V, W and F cycles and a 2-iteration smoother;
  * the accumulating kernels against the plain ones on a bare operator: x + (sweep from zero on r into a scratch vector, existing instantiation), added
    on the host, is what the correction form leaves in x, bit for bit;
  * against the oracle over 3 cycles: residual norms <= 1e-10 relative, iterate <= 1e-12 (the bars of test_gpu_midsize.py / test_gpu_sweep_families.py);
  * the form RAN: correction_launches advances by the visits a mirror of the cycle recursion counts, the general plans are not launched on those
    levels, key 41 = 1 runs none and gives the bits of a solver that does not know the key; no flow error, hand-off buffers all sentinels and counters
    zero between launches;
  * defaults leave these small levels alone;
  * rows without a diagonal keep their x bit for bit and values changed in place are followed (families of tests/sweep_families.py)."""
import numpy as np
import pytest
import scipy.sparse as sp

import midsize as M
import sweep_families as F
from oracle import oracle as orc
from pyamg_amd import DeviceMultilevelSolver
from pyamg_amd import _capi as capi
from pyamg_amd.hierarchy import sparse_op
from pyamg_amd.multilevel import DeviceMatrix

pytestmark = pytest.mark.gpu

HIER = "convdiff:32"
K = 3
LAYOUTS = [8, 0]                    # lanem_cluster: 8 = the cluster layout across the chip, 0 = automatic (one row per wave, one XCD on these levels)
LAYOUT_IDS = ["cluster8", "automatic"]


def visits_of(nlev, cycle, cpl):
    """[entered with x != 0, entered from zero] per level and cycle, from the recursion of the reference's cycle (multilevel.py:584-662): below a level a V
    cycle makes one visit from zero; a W cycle two, the first from zero; an F cycle an F visit from zero and then cpl V visits that start from what it left"""
    v = [[0, 0] for _ in range(nlev - 1)]

    def go(lvl, kind, from_zero):
        v[lvl][int(from_zero)] += 1
        if lvl == nlev - 2:
            return
        if kind == "V":
            go(lvl + 1, "V", True)
        elif kind == "W":
            go(lvl + 1, "W", True)
            go(lvl + 1, "W", False)
        else:
            go(lvl + 1, "F", True)
            for _ in range(cpl):
                go(lvl + 1, "V", False)
    go(0, cycle, False)                                               # solve(x0 = rand): the finest level starts from x != 0
    return v


def corrections_per_cycle(not_zero, from_zero, its):
    """steps in correction form: every post-smoothing iteration, every pre-smoothing iteration of a visit entered with x != 0, and iterations 2.. of an
    announced-zero pre-smoothing.  its = 1: post-smoothing visits + visits entered with x != 0"""
    return from_zero * (2 * its - 1) + not_zero * 2 * its


def _tune(cluster, fused, correction):
    t = dict(sym_fused=fused)
    if cluster:
        t["lanem_cluster"] = cluster
    if correction is not None:
        t["gs_correction"] = correction
    return t


def _solve(spec, cycle, cpl, tune):
    """graph replay, a second replay, eager: bit for bit the same; returns (solver, x, residuals, (b, x0), sym_info per level before / after the eager solve)"""
    n = spec.levels[0].A.shape[0]
    x0 = np.random.RandomState(77).rand(n)
    b = np.zeros_like(x0)
    dml = DeviceMultilevelSolver(spec, graph=True, order="fast", level_tune=tune)
    r1, r2, r3 = [], [], []
    kw = dict(x0=x0, tol=1e-30, maxiter=K, cycle=cycle, cycles_per_level=cpl)
    x1 = dml.solve(b, residuals=r1, **kw)
    x2 = dml.solve(b, residuals=r2, **kw)
    capi.check(capi.lib().pamg_solver_set_graph(dml.handle, 0), "pamg_solver_set_graph")
    before = [A.sym_info() for A in dml.A]
    x3 = dml.solve(b, residuals=r3, **kw)
    after = [A.sym_info() for A in dml.A]
    assert np.array_equal(x1, x2) and r1 == r2, "a second solve must give the same bits"
    assert np.array_equal(x1, x3) and r1 == r3, "graph replay and eager launches must give the same bits"
    for i, A in enumerate(dml.A):
        assert not A.flow_error(), f"flow error on level {i}"
    return dml, x1, r1, (b, x0), before, after


@pytest.fixture(scope="module")
def oracle_solves():
    cache = {}

    def get(key, spec, cycle, cpl, b, x0):
        if (key, cycle, cpl) not in cache:
            ro = []
            xo = orc.OracleSolver(spec).solve(b, x0=x0, tol=1e-30, maxiter=K, cycle=cycle, cycles_per_level=cpl, residuals=ro)
            cache[(key, cycle, cpl)] = (xo, np.array(ro))
        return cache[(key, cycle, cpl)]
    return get


def _parity(tag, x, r, xo, ro):
    r = np.array(r)
    assert r.shape == ro.shape
    rel = float(np.max(np.abs(r - ro) / ro))
    dx = float(np.linalg.norm(x - xo) / np.linalg.norm(xo))
    print(f"[correction] {tag}: residual norms {rel:.2e}, iterate {dx:.2e} against the oracle; {ro[0]:.3e} -> {ro[-1]:.3e}")
    assert rel <= 1e-10, (tag, rel)
    assert dx <= 1e-12, (tag, dx)


def _check_counts(dml, spec, cycle, cpl, its, fused, cluster, before, after):
    nlev = len(spec.levels)
    visits = visits_of(nlev, cycle, cpl)
    for l in range(1, nlev - 1):
        A = dml.A[l]
        n = A.shape[0]
        for which in (0, 1, 4, 5):
            mi = A.lanem_info(which)
            assert mi["rows"] == n and mi["cluster_rows"] == cluster, (l, which, mi)              # merged in the layout asked for, zero-iterate plans built
        d = {key: after[l][key] - before[l][key] for key in ("launches", "zero_launches", "zero_plan_launches", "correction_launches")}
        not_zero, from_zero = visits[l]
        want = K * corrections_per_cycle(not_zero, from_zero, its)
        assert want > 0 and d["correction_launches"] == want, (cycle, cpl, its, l, fused, d, visits[l])
        # every symmetric step of the level is a sweep announced from zero on the zero-iterate plans now: the pre-smoothing of a visit from zero on b,
        # everything else on a residual
        assert d["zero_plan_launches"] == K * 2 * its * (not_zero + from_zero), (cycle, cpl, l, fused, d)
        if fused:
            assert d["launches"] - d["zero_plan_launches"] == 0 and d["zero_launches"] == d["launches"], (cycle, cpl, l, d)      # the general plans did not run
            assert after[l]["handoff_not_sentinel"] == 0 and after[l]["counters_not_zero"] == 0, (l, after[l])
            # (automatic layout: the ticket form inside one XCD on the 117-row level for certain; the 4 192-row level by the size rule of the day)
            assert after[l]["form"] in (("merged",) if cluster else ("merged_one_xcd",) if n <= 1024 else ("merged", "merged_one_xcd")), (l, after[l])
        else:
            assert after[l]["launches"] == 0, (l, after[l])
    s0 = dml.A[0].sym_info()
    assert s0["correction_launches"] == 0 and s0["zero_plan_launches"] == 0, s0                     # the finest level has no plans and is untouched


@pytest.mark.parametrize("cluster", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("cycle", ["V", "W", "F"])
def test_cycles_in_correction_form(cycle, cluster, oracle_solves):
    spec = M.hierarchy(HIER, ("gs", "symmetric"), scalar_csr=True)
    assert [lv.A.shape[0] for lv in spec.levels] == [32768, 4192, 117, 4]
    outs = {}
    for fused in (1, 0):
        dml, x, r, (b, x0), before, after = _solve(spec, cycle, 1, _tune(cluster, fused, 2))
        outs[fused] = (x, r)
        _check_counts(dml, spec, cycle, 1, 1, fused, cluster, before, after)
        dml.free()
    assert np.array_equal(outs[1][0], outs[0][0]) and outs[1][1] == outs[0][1], "fused != two launches"
    xo, ro = oracle_solves("sym", spec, cycle, 1, b, x0)
    _parity(f"{cycle}(1) cluster {cluster}", outs[1][0], outs[1][1], xo, ro)


@pytest.mark.parametrize("cluster", LAYOUTS, ids=LAYOUT_IDS)
def test_two_smoothing_iterations(cluster, oracle_solves):
    """x = 0 holds for the first pre-smoothing iteration of an announced visit only: the second one and both post-smoothing ones take the correction form"""
    spec = M.hierarchy(HIER, ("gs", "symmetric", 2), scalar_csr=True)
    assert spec.levels[1].pre.iterations == 2 and spec.levels[1].post.iterations == 2
    outs = {}
    for fused in (1, 0):
        dml, x, r, (b, x0), before, after = _solve(spec, "V", 1, _tune(cluster, fused, 2))
        outs[fused] = (x, r)
        _check_counts(dml, spec, "V", 1, 2, fused, cluster, before, after)
        dml.free()
    assert np.array_equal(outs[1][0], outs[0][0]) and outs[1][1] == outs[0][1], "fused != two launches"
    xo, ro = oracle_solves("its2", spec, "V", 1, b, x0)
    _parity(f"V(1), 2 smoothing iterations, cluster {cluster}", outs[1][0], outs[1][1], xo, ro)


@pytest.mark.parametrize("cluster", LAYOUTS, ids=LAYOUT_IDS)
def test_switched_off_and_default_leave_the_general_plans(cluster):
    """key 41 = 1: no step in correction form; key 41 left alone: none either on levels this small (4 192 and 117 rows) -- and both give the same bits,
    those of the general plans"""
    spec = M.hierarchy(HIER, ("gs", "symmetric"), scalar_csr=True)
    visits = visits_of(len(spec.levels), "W", 1)
    outs = {}
    for corr in (1, None):
        for fused in (1, 0):
            dml, x, r, _, before, after = _solve(spec, "W", 1, _tune(cluster, fused, corr))
            outs[(corr, fused)] = (x, r)
            for l in range(len(spec.levels) - 1):
                assert after[l]["correction_launches"] == 0, (corr, fused, l, after[l])
            for l in range(1, len(spec.levels) - 1):
                d = {key: after[l][key] - before[l][key] for key in ("launches", "zero_plan_launches")}
                not_zero, from_zero = visits[l]
                assert d["zero_plan_launches"] == K * from_zero, (corr, fused, l, d)                 # the announced pre-smoothing alone
                if fused:
                    assert d["launches"] - d["zero_plan_launches"] == K * (from_zero + 2 * not_zero), (corr, fused, l, d)
            dml.free()
    first = outs[(1, 1)]
    for key, (x, r) in outs.items():
        assert np.array_equal(x, first[0]) and r == first[1], (key, "off, default, fused and two launches must agree in every bit")


def _bare(op, cluster, fused):
    A = DeviceMatrix(op)
    A.tune(gs_order=1, lane_wide=1, line_scan=0, sym_fused=fused, zero_plans=2, **({"lanem_cluster": cluster} if cluster else {}))
    return A


@pytest.mark.parametrize("cluster", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("lvl", [1, 2])
def test_accumulating_kernels_against_the_plain_ones(lvl, cluster):
    """bare level operators with zero-iterate plans: the correction form on (x, b) leaves r = b - A x in the scratch vector and x + e in x, where e is the
    sweep from zero on r the EXISTING instantiation writes into a vector of its own -- added on the host, bit for bit; a bare operator's own sweeps do
    not take the form"""
    op = M.level_op(HIER, lvl, csr=True)
    n = op.shape[0]
    rng = np.random.RandomState(31 + lvl)
    x, b = rng.rand(n), rng.rand(n)
    outs = {}
    for fused in (1, 0):
        A = _bare(op, cluster, fused)
        dx, db, dr, de = (capi.DeviceArray.from_host(v) for v in (x, b, np.zeros(n), np.zeros(n)))
        dx.upload(x)
        A.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=1, x_is_zero=False)
        general = dx.download()
        assert A.sym_info()["correction_launches"] == 0 and A.sym_info()["zero_plan_launches"] == 0         # a bare operator keeps today's behaviour
        dx.upload(x)
        A.gauss_seidel_correction(dx, db, dr)
        got, r = dx.download(), dr.download()
        dx.upload(x)
        A.spmv(2, dx, de, b=db)                                                                          # PAMG_SPMV_RESID: y = b - A x
        assert np.array_equal(r, de.download()), "the scratch vector holds the residual"
        de.upload(np.zeros(n))
        A.gauss_seidel_x0(de, dr, sweep="symmetric", iterations=1, x_is_zero=True)
        e = de.download()
        si = A.sym_info()
        assert si["correction_launches"] == 1 and si["zero_plan_launches"] == 2, si
        for which in (4, 5):
            assert A.lanem_info(which)["rows"] == n and A.lanem_info(which)["cluster_rows"] == cluster, (which, A.lanem_info(which))
        if fused:
            assert si["form"] in (("merged",) if cluster else ("merged_one_xcd",) if n <= 1024 else ("merged", "merged_one_xcd")), si
            assert si["handoff_not_sentinel"] == 0 and si["counters_not_zero"] == 0, si
        else:
            assert si["launches"] == 0, si
        assert np.array_equal(got, x + e), (lvl, cluster, fused, float(np.max(np.abs(got - (x + e)))))
        err = F.rel_err(got, general)
        print(f"[correction] {HIER} level {lvl} ({n} rows) cluster {cluster} fused {fused}: correction form against the direct sweep {err:.2e}")
        assert err <= 1e-13, err                                                                          # the fast order's bar per sweep
        # a second and a third step: the buffers are back where the next launch expects them
        dx.upload(x)
        A.gauss_seidel_correction(dx, db, dr, iterations=3)
        three = dx.download()
        dx.upload(got)
        A.gauss_seidel_correction(dx, db, dr, iterations=2)
        assert np.array_equal(three, dx.download()), "1 + 2 steps != 3 steps"
        assert not A.flow_error()
        outs[fused] = (got, three)
        for v in (dx, db, dr, de):
            v.free()
        A.free()
    assert np.array_equal(outs[1][0], outs[0][0]) and np.array_equal(outs[1][1], outs[0][1]), "fused != two launches"


@pytest.mark.parametrize("cluster", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name,change", [("nodiag", None), ("nodiag", "scale_rows"), ("nonsym", "scale_values")])
def test_families_through_the_correction_form(name, change, cluster):
    """rows without a diagonal (missing, stored as 0.0, an empty row) keep their x bit for bit -- they are the only rows whose x a zero-iterate launch
    would read, and in correction form they must carry 0, not x; after the values change in place the next step in correction form is the sequential
    sweep of the CHANGED operator (the plans hold copies of the values).  Bar: the family's own against the f64 sequential reference"""
    fam = F.FAMILIES[name]
    S = fam.make("large")
    n = S.shape[0]
    rng = np.random.RandomState(9)
    x, b = rng.rand(n), rng.rand(n)
    outs = {}
    for fused in (1, 0):
        A = _bare(sparse_op(sp.csr_array(S)), cluster, fused)
        dx, db, dr = (capi.DeviceArray.from_host(v) for v in (x, b, np.zeros(n)))
        S2 = sp.csr_array(S, copy=True)
        if change is not None:
            A.gauss_seidel_correction(dx, db, dr)                                                        # the plans are built on the old values
            assert A.lanem_info(4)["rows"] == n
            if change == "scale_values":
                S2.data = S2.data * 2.0
                capi.check(capi.lib().pamg_matrix_scale_values(A.handle, 2.0), "pamg_matrix_scale_values")
            else:
                d = 0.5 + 1.5 * np.random.RandomState(8).rand(n)
                S2.data = S2.data * np.repeat(d, np.diff(S2.indptr))
                capi.check(capi.lib().pamg_matrix_scale_rows(A.handle, capi.ptr(np.ascontiguousarray(d))), "pamg_matrix_scale_rows")
        idle = F.untouched_rows(S2)
        assert name != "nodiag" or idle.size > n // 8
        got = {}
        for its in (1, 2):
            dx.upload(x)
            A.gauss_seidel_correction(dx, db, dr, iterations=its)
            got[its] = dx.download()
            ref = F.ref_sweeps(S2, x, b, "symmetric", its)
            err = F.rel_err(got[its], ref)
            print(f"[correction] {name} {change} cluster {cluster} fused {fused} iterations {its}: {err:.2e} against the sequential sweep (bar {fam.tol:.0e})")
            assert err <= fam.tol, (name, change, cluster, fused, its, err)
            assert np.array_equal(got[its][idle], x[idle]), (name, change, cluster, fused, its, "rows without a diagonal")
        for which in (4, 5):
            assert A.lanem_info(which)["rows"] == n and A.lanem_info(which)["cluster_rows"] == cluster, (which, A.lanem_info(which))
        si = A.sym_info()
        assert si["correction_launches"] == 3 + (change is not None), si
        if fused:
            assert si["handoff_not_sentinel"] == 0 and si["counters_not_zero"] == 0, si
        assert not A.flow_error()
        outs[fused] = got
        for v in (dx, db, dr):
            v.free()
        A.free()
    for its in outs[1]:
        assert np.array_equal(outs[1][its], outs[0][its]), (name, change, cluster, its, "fused != two launches")
