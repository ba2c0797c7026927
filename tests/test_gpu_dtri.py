"""The dense block-triangular form of the symmetric Gauss-Seidel sweep (pamg_matrix_dense_tri; pyamg_amd/csrc/pamg_dtri.hip) on the device.

Bare operators: levels 1 (31 868 rows) and 2 (768 rows) of tests/midsize.py's poisson:64x64x64 with the form switched on at B = 64, 256, 2048 -- many blocks,
a ragged last block (31 868 = 124 x 256 + 124 = 15 x 2048 + 1148), a single block (768 rows at B = 2048) -- from zero against the general sweep announced
from zero with the form off, in correction form from a random iterate against the general sweep from that iterate: 1e-13 relative in the max norm (the
fast order's bar per sweep); two runs bit for bit; dense_tri_info says the launches ran (a case that passes because the form stepped aside fails).
Automatic rule (operator side): a strictly dominant 125-point operator on 21^3 (9 261 rows, 105 entries per row) is eligible; the 31 868-row 30-per-row
operator is not (memory proportion), nor is anything of at most 8 192 rows.
Solver: poisson:64x64x64 with the form on levels 1 (B = 256) and 2, three V cycles: graph replay == eager == a second solve bit for bit; residual norms
<= 1e-10 relative and iterate <= 1e-12 against the oracle (the bars of test_gpu_midsize.py); no zero-iterate plans on the claimed levels; the resident
bytes grow by exactly what the form reports.  With defaults the form is built nowhere and runs nowhere on that hierarchy.
Defaults on a hierarchy whose level 1 is the 125-point operator: the automatic mode builds the form there at finalise and runs it, and nowhere else; asked for
by name on a level without a symmetric Gauss-Seidel smoother it is not built."""
import numpy as np
import pytest
import scipy.sparse as sp

import midsize as M
from oracle import oracle as orc
from pyamg_amd import DeviceMultilevelSolver
from pyamg_amd import _capi as capi
from pyamg_amd.hierarchy import sparse_op
from pyamg_amd.multilevel import DeviceMatrix

pytestmark = pytest.mark.gpu

HIER = "poisson:64x64x64"
TOL = 1e-13
K = 3


def _rel(got, ref):
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


def _vectors(n, seed):
    rng = np.random.RandomState(seed)
    return rng.rand(n), rng.rand(n)


@pytest.fixture(scope="module")
def general():
    """per level: (x0, b, the general sweep from zero on b, the general sweep from x0) with the form off -- computed once"""
    cache = {}

    def get(lvl):
        if lvl not in cache:
            op = M.level_op(HIER, lvl)
            n = op.shape[0]
            x0, b = _vectors(n, 40 + lvl)
            A = DeviceMatrix(op)
            A.tune(gs_order=1)
            A.dense_tri(1)
            dx, db = capi.DeviceArray.from_host(np.zeros(n)), capi.DeviceArray.from_host(b)
            A.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=1, x_is_zero=True)
            from_zero = dx.download()
            dx.upload(x0)
            A.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=1, x_is_zero=False)
            from_x0 = dx.download()
            assert A.dense_tri_info()["built"] == 0 and not A.flow_error()
            for v in (dx, db):
                v.free()
            A.free()
            cache[lvl] = (x0, b, from_zero, from_x0)
        return cache[lvl]
    return get


@pytest.mark.parametrize("B", [64, 256, 2048])
@pytest.mark.parametrize("lvl", [1, 2])
def test_bare_operator(general, lvl, B):
    op = M.level_op(HIER, lvl)
    n = op.shape[0]
    assert n == (31868, 768)[lvl - 1]
    x0, b, ref_zero, ref_x0 = general(lvl)
    A = DeviceMatrix(op)
    A.tune(gs_order=1)
    A.dense_tri(2, B)
    dx, db, dr = (capi.DeviceArray.from_host(v) for v in (np.zeros(n), b, np.zeros(n)))
    runs = []
    for rep in range(2):
        dx.upload(np.full(n, 7.0))                                   # announced zero: what x holds must not matter
        A.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=1, x_is_zero=True)
        zero = dx.download()
        dx.upload(x0)
        A.gauss_seidel_correction(dx, db, dr)
        corr = dx.download()
        runs.append((zero, corr))
    di = A.dense_tri_info()
    nb = -(-n // B)
    assert di["built"] == 1 and di["blocks"] == nb and di["block_rows"] == B and di["kernel_launches"] == 4 * nb - 2, di
    assert di["zero_launches"] == 2 and di["correction_launches"] == 2 and di["declined_by_growth"] == 0, di
    assert (di["off_block_entries"] == 0) == (nb == 1) and 0.0 < di["growth"] <= 1e3, di
    assert A.sym_info()["correction_launches"] == 0 and A.sym_info()["zero_plan_launches"] == 0            # the merged plans did not run
    e0, e1 = _rel(runs[0][0], ref_zero), _rel(runs[0][1], ref_x0)
    print(f"[dtri] {HIER} level {lvl} ({n} rows) B={B}: {nb} blocks, growth {di['growth']:.3f}, inverses {di['inverse_us']} us; from zero {e0:.2e}, "
          f"correction form {e1:.2e} against the general sweeps")
    assert e0 <= TOL and e1 <= TOL, (lvl, B, e0, e1)
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), "two runs must give the same bits"
    dx.upload(x0)
    A.spmv(2, dx, dr, b=db)                                           # PAMG_SPMV_RESID
    r = dr.download()
    dx.upload(x0)
    A.gauss_seidel_correction(dx, db, dr)
    assert np.array_equal(dr.download(), r), "the scratch vector holds the residual"
    A.dense_tri(1)                                                    # switched off: dropped, the general path again
    assert A.dense_tri_info()["built"] == 0
    dx.upload(np.zeros(n))
    A.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=1, x_is_zero=True)
    assert np.array_equal(dx.download(), ref_zero)
    for v in (dx, db, dr):
        v.free()
    A.free()


def stencil125(m, c=126.0):
    P = sp.diags_array([np.ones(m - abs(k)) for k in range(-2, 3)], offsets=list(range(-2, 3)), format="csr")
    A = sp.csr_array(c * sp.eye_array(m ** 3) - sp.kron(sp.kron(P, P), P))
    A.sort_indices()
    return A


def test_automatic_rule_operator_side(general):
    A21 = stencil125(21)
    n = A21.shape[0]
    assert n == 9261 and 100 < A21.nnz / n < 110                         # (5 * 21 - 6)^3 / 21^3 = 104.8 entries per row
    A = DeviceMatrix(sparse_op(A21))
    A.tune(gs_order=1)
    di = A.dense_tri_info()
    assert di["auto_eligible"] == 1 and di["built"] == 0 and di["mode"] == 0, di
    # a bare operator never takes the form by itself; switched on it runs, multi-block, on 105 entries per row
    x0, b = _vectors(n, 5)
    dx, db = capi.DeviceArray.from_host(np.zeros(n)), capi.DeviceArray.from_host(b)
    A.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=1, x_is_zero=True)
    ref = dx.download()
    assert A.dense_tri_info()["built"] == 0 and A.dense_tri_info()["zero_launches"] == 0
    A.dense_tri(2)
    A.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=1, x_is_zero=True)
    di = A.dense_tri_info()
    assert di["built"] == 1 and di["blocks"] == 5 and di["zero_launches"] == 1, di
    err = _rel(dx.download(), ref)
    print(f"[dtri] 125-point 21^3: growth {di['growth']:.3f}, {di['bytes'] / 2 / (12 * A21.nnz + 4 * (n + 1)):.1f} x the CSR bytes per direction; from zero {err:.2e}")
    assert err <= TOL
    A.tune(gs_order=0)                                                # exact order: the form no longer applies and is dropped
    assert A.dense_tri_info()["built"] == 0 and A.dense_tri_info()["auto_eligible"] == 0
    for v in (dx, db):
        v.free()
    A.free()
    for op in (M.level_op(HIER, 1), M.level_op(HIER, 2), sparse_op(stencil125(20))):       # 30 per row; 768 rows; 8 000 rows of ~104 per row
        A = DeviceMatrix(op)
        A.tune(gs_order=1)
        assert op.shape[0] in (31868, 768, 8000) and A.dense_tri_info()["auto_eligible"] == 0, op.shape
        A.free()


def _solve(spec, b, x0, **kw):
    dml = DeviceMultilevelSolver(spec, graph=True, order="fast", **kw)
    r1, r2, r3 = [], [], []
    x1 = dml.solve(b, x0=x0, tol=1e-30, maxiter=K, residuals=r1)
    x2 = dml.solve(b, x0=x0, tol=1e-30, maxiter=K, residuals=r2)
    capi.check(capi.lib().pamg_solver_set_graph(dml.handle, 0), "pamg_solver_set_graph")
    x3 = dml.solve(b, x0=x0, tol=1e-30, maxiter=K, residuals=r3)
    assert np.array_equal(x1, x2) and r1 == r2, "a second solve must give the same bits"
    assert np.array_equal(x1, x3) and r1 == r3, "graph replay and eager launches must give the same bits"
    for i, A in enumerate(dml.A):
        assert not A.flow_error(), f"flow error on level {i}"
    return dml, x1, np.array(r1)


def test_solver_levels():
    spec = M.hierarchy(HIER, ("gs", "symmetric"))
    n = spec.levels[0].A.shape[0]
    x0 = np.random.RandomState(77).rand(n)
    b = np.zeros(n)
    ro = []
    xo = orc.OracleSolver(spec).solve(b, x0=x0, tol=1e-30, maxiter=K, residuals=ro)
    ro = np.array(ro)
    off = lambda i: {"zero_plans": 1} if i in (1, 2) else None       # noqa: E731 -- both solvers without zero-iterate plans there: the bytes compare
    dml, x, r = _solve(spec, b, x0, dense_tri={1: dict(mode=2, block_rows=256), 2: dict(mode=2)}, level_tune=off)
    rel, dxr = float(np.max(np.abs(r - ro) / ro)), float(np.linalg.norm(x - xo) / np.linalg.norm(xo))
    print(f"[dtri] {HIER} solver, the form on levels 1 and 2: residual norms {rel:.2e}, iterate {dxr:.2e} against the oracle; {ro[0]:.3e} -> {ro[-1]:.3e}")
    assert rel <= 1e-10 and dxr <= 1e-12, (rel, dxr)
    infos = [A.dense_tri_info() for A in dml.A]
    bytes_on = [A.info()["hbm_bytes"] for A in dml.A]
    for l in (1, 2):
        di = infos[l]
        assert di["built"] == 1 and di["block_rows"] == (256, 2048)[l - 1], (l, di)
        # launches are counted where they are enqueued or captured: one captured V cycle (replayed by the first two solves), K eager ones; each
        # visits the level once from zero (pre-smoothing) and once in correction form (post-smoothing)
        assert di["zero_launches"] == K + 1 and di["correction_launches"] == K + 1, (l, di)
        assert dml.A[l].lanem_info(4)["rows"] == 0 and dml.A[l].lanem_info(5)["rows"] == 0, l
        assert dml.A[l].sym_info()["zero_plan_launches"] == 0 and dml.A[l].sym_info()["correction_launches"] == 0, l
    assert infos[0]["built"] == 0 and infos[0]["zero_launches"] == 0
    dml.free()
    # the form claims a level's zero-iterate plans too (nothing switched them off here)
    dz, xz, rz = _solve(spec, b, x0, dense_tri={1: dict(mode=2, block_rows=256), 2: dict(mode=2)})
    assert np.array_equal(xz, x) and np.array_equal(rz, r)
    for l in (1, 2):
        assert dz.A[l].lanem_info(4)["rows"] == 0 and dz.A[l].lanem_info(5)["rows"] == 0, l
    dz.free()
    # switched off, and with defaults: built nowhere, run nowhere, no bytes -- and the bytes of the form are exactly what it reports
    for kw in (dict(dense_tri=False, level_tune=off), dict()):
        d0, x_0, r_0 = _solve(spec, b, x0, **kw)
        for l, A in enumerate(d0.A):
            di = A.dense_tri_info()
            assert di["built"] == 0 and di["zero_launches"] == 0 and di["correction_launches"] == 0 and di["resident_bytes"] == 0 and di["bytes"] == 0, (kw, l, di)
            if "level_tune" in kw:
                assert bytes_on[l] - A.info()["hbm_bytes"] == infos[l]["resident_bytes"], (l, bytes_on[l], A.info()["hbm_bytes"], infos[l])
                assert infos[l]["resident_bytes"] >= infos[l]["bytes"]
        assert float(np.max(np.abs(r_0 - ro) / ro)) <= 1e-10
        d0.free()


def _spec_with_125_point_level():
    """a hierarchy whose level 1 is the 125-point operator on 21^3: a finest level of twice its rows above it (pairs of unknowns aggregated, P = R^T of
    ones), tests/midsize.py's coarsening below it.  The solver and the oracle run the same operators; no Galerkin relation is needed for parity"""
    from pyamg_amd.hierarchy import HierarchySpec, LevelSpec
    A1 = stencil125(21)
    n1 = A1.shape[0]
    A0 = sp.csr_array(sp.kron(A1, sp.eye_array(2)) + sp.kron(sp.eye_array(n1), sp.csr_array(np.array([[40.0, -40.0], [-40.0, 40.0]]))))
    A0.sort_indices()
    P0 = sp.csr_array(sp.kron(sp.eye_array(n1), np.ones((2, 1))))
    ops = [(A0, P0, sp.csr_array(P0.T), 1)] + list(M._sa(A1, np.ones((n1, 1)), 1))
    sm = M.gs("symmetric")
    levels = []
    for lvl, (A, P, R, bs) in enumerate(ops):
        last = P is None
        A, P, R = (None if m is None else M._csr(m) for m in (A, P, R))
        levels.append(LevelSpec(sparse_op(A), None if last else sparse_op(P), None if last else sparse_op(R), None if last else sm(A, bs, lvl), None if last else sm(A, bs, lvl)))
    coarse = np.ascontiguousarray(np.linalg.pinv(ops[-1][0].toarray().astype(np.float64)))
    return HierarchySpec(levels=levels, coarse_kind="dense", coarse_op=coarse, coarse_name="'pinv'")


def test_solver_defaults_engage_on_an_eligible_level():
    """the path the automatic mode takes at finalise: nothing is switched on by name, level 1 (9 261 rows, 105 entries per row, symmetric Gauss-Seidel before
    and after) meets the rule and runs the form; the finest level and the small ones do not; a Jacobi hierarchy with the form asked for by name builds none"""
    spec = _spec_with_125_point_level()
    sizes = [l.A.shape[0] for l in spec.levels]
    assert sizes[0] == 18522 and sizes[1] == 9261 and len(sizes) >= 3 and max(sizes[2:]) <= 8192, sizes
    n = sizes[0]
    x0 = np.random.RandomState(78).rand(n)
    b = np.random.RandomState(79).rand(n)
    ro = []
    xo = orc.OracleSolver(spec).solve(b, x0=x0, tol=1e-30, maxiter=K, residuals=ro)
    ro = np.array(ro)
    dml, x, r = _solve(spec, b, x0)
    rel, dxr = float(np.max(np.abs(r - ro) / ro)), float(np.linalg.norm(x - xo) / np.linalg.norm(xo))
    infos = [A.dense_tri_info() for A in dml.A]
    print(f"[dtri] defaults on {sizes}: built {[d['built'] for d in infos]}; residual norms {rel:.2e}, iterate {dxr:.2e} against the oracle; {ro[0]:.3e} -> {ro[-1]:.3e}")
    assert rel <= 1e-10 and dxr <= 1e-12, (rel, dxr)
    assert [d["built"] for d in infos] == [0, 1] + [0] * (len(sizes) - 2), infos
    d1 = infos[1]
    assert d1["mode"] == 0 and d1["auto_eligible"] == 1 and d1["blocks"] == 5 and d1["block_rows"] == 2048, d1
    assert d1["zero_launches"] == K + 1 and d1["correction_launches"] == K + 1, d1          # one captured cycle, K eager ones
    assert dml.A[1].lanem_info(4)["rows"] == 0 and dml.A[1].sym_info()["zero_plan_launches"] == 0
    for l in range(2, len(sizes) - 1):
        assert infos[l]["zero_launches"] == 0 and infos[l]["auto_eligible"] == 0, l                       # the small levels keep the merged plans
    dml.free()
    d0, x_off, r_off = _solve(spec, b, x0, dense_tri=False)
    assert all(A.dense_tri_info()["built"] == 0 for A in d0.A)
    assert float(np.max(np.abs(r_off - r) / r)) <= 1e-10 and float(np.max(np.abs(x_off - x)) / np.max(np.abs(x))) <= 1e-12
    d0.free()
    # asked for by name on a level without a symmetric Gauss-Seidel smoother: not built (it would never run)
    jac = M.hierarchy(HIER, ("chebyshev", 3))
    dj = DeviceMultilevelSolver(jac, graph=True, order="fast", dense_tri={1: dict(mode=2), 2: dict(mode=2)})
    for l in (1, 2):
        di = dj.A[l].dense_tri_info()
        assert di["mode"] == 2 and di["built"] == 0 and di["resident_bytes"] == 0, (l, di)
    dj.free()
