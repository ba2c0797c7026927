"""The dense block-triangular form of the symmetric Gauss-Seidel sweep (pamg_dtri.hip, pamg_matrix_dense_tri, DeviceMultilevelSolver(dense_tri=...)) on
the adversarial families of tests/dtri_families.py, at their large size, on the device.

Bare operators (DeviceMatrix, tune(gs_order=1), dense_tri(2, B)).  Every case DECLARES its outcome and the test asserts it from dense_tri_info: a case
that passes because the form stepped aside fails.
  engages: built, blocks, block_rows, 4 nb - 2 kernel launches, the zero and correction counters, no growth decline, the device's growth figure within
    1e-10 relative of NumPy's (dense inverses of the diagonal blocks; closed form for the chains), no flow error; from zero (x pre-filled with 7.0 and
    announced zero) and in correction form from a random iterate within 1e-13 relative in the max norm of the oracle's sequential sweep on long-double
    copies (the project's per-sweep bar); two runs the same bits; the scratch vector holds b - A x; after dense_tri(1) the operator's byte account is
    back where it was.  `rowscale` gives the bits and the growth of the unscaled operator.
  declines (host: diagonal or non-finite value; growth; size): nothing built, declined_by_growth as declared, both launch counters 0, and bytes and
    both sweeps those of a second upload of the same operator with dense_tri(1), bit for bit (NaN equal to NaN); the correction entry asked by name is
    refused (a bare operator has no zero-iterate plans), on an upload that has declined already and on a fresh one, and builds and counts nothing.
State changes on nonsym: another block size, scale_values / scale_rows after a first sweep (the triangles hold copies of the values), a tune key that
drops the lane layouts, tune(gs_correction=1) (the correction entry leaves the form: refused without zero-iterate plans, on the merged plans with
them; back on the form at 0 and 2), two iterations on a bare operator, three correction launches, the argument checks.

Solver: tests/midsize.py's convdiff:16 (4096 / 514 / 18 / 1 rows, non-symmetric) with the form on by name at small blocks, cycles V, W, F and F with two
cycles per level: graph replay == eager == a second solve bit for bit, residual norms <= 1e-10 relative and iterate <= 1e-12 against OracleSolver
(the bars of test_gpu_dtri.py), and the per-level counters equal to the counts of the reference's cycle recursion (`_counts`: the first visit of a level
pre-smooths from zero, every later pre-smoothing and every post-smoothing runs in correction form).  Two iterations per smoothing step, symmetric
Gauss-Seidel on one side only, level 0 by name.  A growth decline inside a solver (level 1 = chains of 7 rows) leaves the level with the zero-iterate
plans, the bits and the counters of dense_tri=False.  Together with dense_tail.  f32 and BSR hierarchies: built nowhere.

Measured on the MI355X: every engaging case is within 4.7e-16 (from zero) and 3.3e-15 (correction form) of the long-double sweep; the whole file takes
19 s, its slowest case (nonsym at 4097 rows, B = 4096: NumPy inverts the 4096-row block twice) 3.7 s.  With the parent's library the
`nonfinite_*_off_block` cases fail: one NaN or inf in an off-block entry of 3000 rows at B = 257 is accepted (built, growth 1.432) and the form leaves
1285 rows finite where the general sweep leaves 2006; build_dtri_plan now declines every non-finite stored value on the host."""
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import dtri_families as F
import midsize as M
import sweep_families as SF
from oracle import oracle as orc
from pyamg_amd import DeviceMultilevelSolver
from pyamg_amd import _capi as capi
from pyamg_amd.hierarchy import HierarchySpec, LevelSpec, load_spec, sparse_op
from pyamg_amd.multilevel import DeviceMatrix

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
LARGE = F.cases("large")
TOL = F.TOL
K = 3


def _upload(A, mode=2, B=0):
    dm = DeviceMatrix(sparse_op(sp.csr_array(A)))
    dm.tune(gs_order=1)
    dm.dense_tri(mode, B)
    return dm


def _vectors(c):
    A = c.A()
    b, x0 = F.vectors(A.shape[0])
    if c.name == "rowscale":
        b = np.ldexp(b, F.rowscale_exponents(A.shape[0]))
    return A, b, x0


def _dev(*vs):
    return [capi.DeviceArray.from_host(np.ascontiguousarray(v, dtype=np.float64)) for v in vs]


def _free(*things):
    for t in things:
        t.free()


def _from_zero(dm, dx, db, n, iterations=1):
    dx.upload(np.full(n, 7.0))                                       # announced zero: what x holds must not matter
    dm.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=iterations, x_is_zero=True)
    return dx.download()


def _yardstick(A, b, x0):
    n = A.shape[0]
    return (SF.ref_sweeps(A, np.zeros(n), b, "symmetric", dtype=np.longdouble), SF.ref_sweeps(A, x0, b, "symmetric", dtype=np.longdouble))


def _engage(c):
    """run an engaging case; returns (growth, from zero, correction form)"""
    A, b, x0 = _vectors(c)
    n, B, nb = A.shape[0], c.B, c.blocks()
    dm = _upload(A, 2, B)
    assert dm.info()["nnz"] == A.nnz, "the upload keeps every stored entry (explicit zeros, duplicates)"
    bytes0 = dm.info()["hbm_bytes"]
    dx, db, dr = _dev(np.zeros(n), b, np.zeros(n))
    runs = []
    for _ in range(2):
        zero = _from_zero(dm, dx, db, n)
        dx.upload(x0)
        dm.gauss_seidel_correction(dx, db, dr)
        runs.append((zero, dx.download()))
    di = dm.dense_tri_info()
    assert di["built"] == 1 and di["blocks"] == nb and di["block_rows"] == B and di["kernel_launches"] == 4 * nb - 2, (c.id, di)
    assert di["zero_launches"] == 2 and di["correction_launches"] == 2 and di["declined_by_growth"] == 0, (c.id, di)
    assert dm.sym_info()["correction_launches"] == 0 and dm.sym_info()["zero_plan_launches"] == 0          # the merged plans did not run
    assert not dm.flow_error()
    want = c.growth()
    assert abs(di["growth"] - want) <= 1e-10 * want and di["growth"] <= F.GROWTH_CAP, (c.id, di["growth"], want)
    if c.off_block is not None:
        assert di["off_block_entries"] == c.off_block, (c.id, di)
    assert di["bytes"] == F.tri_bytes(n, B), (c.id, di)
    assert dm.info()["hbm_bytes"] - bytes0 == di["resident_bytes"] >= di["bytes"], (c.id, di, bytes0)
    ref0, ref1 = _yardstick(A, b, x0)
    e0, e1 = SF.rel_err(runs[0][0], ref0), SF.rel_err(runs[0][1], ref1)
    print(f"[dtri families] {c.id} ({n} rows): {nb} blocks, {di['off_block_entries']} off-block entries, growth {di['growth']:.6g} (NumPy {want:.6g}); "
          f"from zero {e0:.2e}, correction form {e1:.2e} against the long-double sweep")
    assert e0 <= TOL and e1 <= TOL, (c.id, e0, e1)
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), "two runs must give the same bits"
    dx.upload(x0)
    dm.spmv(2, dx, dr, b=db)                                          # PAMG_SPMV_RESID
    r = dr.download()
    dx.upload(x0)
    dm.gauss_seidel_correction(dx, db, dr)
    assert np.array_equal(dr.download(), r), "the scratch vector holds the residual"
    dm.dense_tri(1)
    assert dm.dense_tri_info()["built"] == 0 and dm.info()["hbm_bytes"] == bytes0, (c.id, dm.info(), bytes0)
    _free(dx, db, dr, dm)
    return di["growth"], runs[0][0], runs[0][1]


@pytest.mark.parametrize("c", [c for c in LARGE if c.outcome == "engages"], ids=lambda c: c.id)
def test_bare_engages(c):
    _engage(c)


def test_rowscale_gives_the_bits_of_the_unscaled_operator():
    """2^e_i on row i of A and of b, e_i in [-200, 200]: the growth figure and every output bit, from zero and in correction form, are nonsym's"""
    c = next(c for c in LARGE if c.name == "rowscale" and c.B == 257)
    plain = next(p for p in LARGE if p.name == "nonsym[3000]" and p.B == 257)
    g1, z1, c1 = _engage(c)
    g0, z0, c0 = _engage(plain)
    assert g1 == g0 and np.array_equal(z1, z0) and np.array_equal(c1, c0)


@pytest.mark.parametrize("c", [c for c in LARGE if c.outcome != "engages"], ids=lambda c: c.id)
def test_bare_declines(c):
    A, b, x0 = _vectors(c)
    n = A.shape[0]
    dm, off = _upload(A, 2, c.B), _upload(A, 1)
    assert dm.info()["hbm_bytes"] == off.info()["hbm_bytes"]
    dx, db = _dev(np.zeros(n), b)
    got = []
    for m in (dm, off):
        zero = _from_zero(m, dx, db, n)
        dx.upload(x0)
        m.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=1, x_is_zero=False)
        got.append((zero, dx.download()))
    di = dm.dense_tri_info()
    print(f"[dtri families] {c.id} ({n} rows): {c.outcome}, growth figure {di['growth']:.6g}")
    assert di["built"] == 0 and di["blocks"] == 0 and di["resident_bytes"] == 0, (c.id, di)
    assert di["declined_by_growth"] == (1 if c.outcome == "declines_growth" else 0), (c.id, di)
    assert di["zero_launches"] == 0 and di["correction_launches"] == 0, (c.id, di)
    if c.outcome == "declines_growth":
        assert di["growth"] > F.GROWTH_CAP and abs(di["growth"] - c.growth()) <= 1e-10 * c.growth(), (c.id, di, c.growth())
    assert dm.info()["hbm_bytes"] == off.info()["hbm_bytes"], "a decline leaves the byte account alone"
    assert np.array_equal(got[0][0], got[1][0], equal_nan=True) and np.array_equal(got[0][1], got[1][1], equal_nan=True), c.id
    assert dm.sym_info() == off.sym_info()
    # the correction entry asked by name: on the declined upload (decline already taken by the sweep from zero), on a fresh one (the entry itself meets
    # the decline) and on the twin -- no form, no zero-iterate plans on a bare operator: refused, x untouched, nothing built, counted or allocated
    lib = capi.lib()
    fresh = _upload(A, 2, c.B)
    dr = _dev(np.zeros(n))[0]
    for m in (dm, fresh, off):
        before = m.info()["hbm_bytes"]
        dx.upload(x0)
        assert lib.pamg_matrix_gauss_seidel_correction(m.handle, dx.ptr, db.ptr, dr.ptr, 1, None) == capi.E_UNSUPPORTED, c.id
        assert np.array_equal(dx.download(), x0)
        dj = m.dense_tri_info()
        assert dj["built"] == 0 and dj["zero_launches"] == 0 and dj["correction_launches"] == 0 and dj["resident_bytes"] == 0, (c.id, dj)
        assert m.info()["hbm_bytes"] == before and m.sym_info()["correction_launches"] == 0, c.id
    df = fresh.dense_tri_info()
    assert df["declined_by_growth"] == di["declined_by_growth"] and (df["growth"] == di["growth"] or c.outcome != "declines_growth"), (c.id, df, di)
    _free(dx, db, dr, dm, fresh, off)


# ------------------------------------------------------------------------------------------------ state changes on nonsym
@pytest.fixture(scope="module")
def nonsym():
    A = F.nonsym_rows(3000)
    b, x0 = F.vectors(3000)
    return A, b, x0


def _both(dm, dx, db, dr, x0):
    n = x0.size
    zero = _from_zero(dm, dx, db, n)
    dx.upload(x0)
    dm.gauss_seidel_correction(dx, db, dr)
    return zero, dx.download()


def _errs(A, b, x0, zero, corr):
    ref0, ref1 = _yardstick(A, b, x0)
    return SF.rel_err(zero, ref0), SF.rel_err(corr, ref1)


def test_another_block_size_rebuilds(nonsym):
    A, b, x0 = nonsym
    n = A.shape[0]
    dm = _upload(A, 2, 65)
    bytes0 = dm.info()["hbm_bytes"]
    dx, db, dr = _dev(np.zeros(n), b, np.zeros(n))
    z65, c65 = _both(dm, dx, db, dr, x0)
    d65 = dm.dense_tri_info()
    assert d65["built"] == 1 and d65["block_rows"] == 65 and d65["blocks"] == 47 and dm.info()["hbm_bytes"] == bytes0 + d65["resident_bytes"]
    dm.dense_tri(2, 257)
    assert dm.dense_tri_info()["built"] == 0 and dm.info()["hbm_bytes"] == bytes0
    z257, c257 = _both(dm, dx, db, dr, x0)
    d257 = dm.dense_tri_info()
    assert d257["built"] == 1 and d257["block_rows"] == 257 and d257["blocks"] == 12 and d257["kernel_launches"] == 46, d257
    assert d257["bytes"] == F.tri_bytes(n, 257) != d65["bytes"] == F.tri_bytes(n, 65)
    assert dm.info()["hbm_bytes"] == bytes0 + d257["resident_bytes"], "the byte account is exact"
    assert d257["zero_launches"] == 2 and d257["correction_launches"] == 2                               # (the counters are the operator's)
    assert max(_errs(A, b, x0, z65, c65) + _errs(A, b, x0, z257, c257)) <= TOL
    _free(dx, db, dr, dm)


def test_scaled_values_rebuild_the_triangles(nonsym):
    """the triangles hold copies of the values: scale_values / scale_rows drop the form, the next sweep rebuilds it on the scaled operator"""
    A, b, x0 = nonsym
    n = A.shape[0]
    lib = capi.lib()
    dm = _upload(A, 2, 257)
    dx, db, dr = _dev(np.zeros(n), b, np.zeros(n))
    stale = _both(dm, dx, db, dr, x0)
    capi.check(lib.pamg_matrix_scale_values(dm.handle, 2.0), "scale_values")
    assert dm.dense_tri_info()["built"] == 0, "dropped"
    got = _both(dm, dx, db, dr, x0)
    A2 = SF._finish(2.0 * A)
    e = _errs(A2, b, x0, *got)
    print(f"[dtri families] nonsym after scale_values(2): from zero {e[0]:.2e}, correction form {e[1]:.2e}")
    assert dm.dense_tri_info()["built"] == 1 and max(e) <= TOL
    assert not np.array_equal(got[0], stale[0]) and SF.rel_err(got[0], stale[0]) > 0.1
    d = 0.5 + np.random.RandomState(9).rand(n)
    capi.check(lib.pamg_matrix_scale_rows(dm.handle, capi.ptr(np.ascontiguousarray(d))), "scale_rows")
    assert dm.dense_tri_info()["built"] == 0, "dropped"
    got3 = _both(dm, dx, db, dr, x0)
    A3 = SF._finish(sp.diags_array(d) @ A2)
    e = _errs(A3, b, x0, *got3)
    print(f"[dtri families] nonsym after scale_rows(d): from zero {e[0]:.2e}, correction form {e[1]:.2e}")
    assert dm.dense_tri_info()["built"] == 1 and dm.dense_tri_info()["zero_launches"] == 3 and max(e) <= TOL
    assert SF.rel_err(got3[0], got[0]) > 0.01
    # one row's scale 0: its diagonal is stored as 0.0 -- a host decline, the general sweep leaves that row alone
    d0 = np.ones(n)
    d0[1234] = 0.0
    capi.check(lib.pamg_matrix_scale_rows(dm.handle, capi.ptr(d0)), "scale_rows")
    zero = _from_zero(dm, dx, db, n)
    di = dm.dense_tri_info()
    assert di["built"] == 0 and di["declined_by_growth"] == 0 and di["zero_launches"] == 3, di
    A4 = sp.csr_array(A3, copy=True)
    A4.data[A4.indptr[1234]:A4.indptr[1235]] *= 0.0                  # (the row stays stored, in its order)
    off = _upload(A4, 1)
    assert np.array_equal(zero, _from_zero(off, dx, db, n)) and zero[1234] == 7.0
    _free(dx, db, dr, dm, off)


def test_tune_keys(nonsym):
    """a key whose effect drops the lane layouts drops the form, the next sweep rebuilds it; gs_correction = 1 keeps the correction entry off the
    form, the sweep from zero still takes it"""
    A, b, x0 = nonsym
    n = A.shape[0]
    dm = _upload(A, 2, 257)
    dx, db, dr = _dev(np.zeros(n), b, np.zeros(n))
    bytes0 = dm.info()["hbm_bytes"]
    first = _both(dm, dx, db, dr, x0)
    assert dm.info()["hbm_bytes"] == bytes0 + dm.dense_tri_info()["resident_bytes"] > bytes0
    dm.tune(lanem_cluster=4)
    assert dm.dense_tri_info()["built"] == 0 and dm.info()["hbm_bytes"] == bytes0
    again = _both(dm, dx, db, dr, x0)
    di = dm.dense_tri_info()
    assert di["built"] == 1 and di["zero_launches"] == 2 and di["correction_launches"] == 2, di
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    lib = capi.lib()
    dm.tune(gs_correction=1)
    zero = _from_zero(dm, dx, db, n)
    di = dm.dense_tri_info()
    assert di["built"] == 1 and di["zero_launches"] == 3 and di["correction_launches"] == 2, di
    assert np.array_equal(zero, first[0])
    # the correction entry, asked by name: the form no longer takes it, and without zero-iterate plans nothing else does -- refused, x untouched
    dx.upload(x0)
    assert lib.pamg_matrix_gauss_seidel_correction(dm.handle, dx.ptr, db.ptr, dr.ptr, 1, None) == capi.E_UNSUPPORTED
    assert np.array_equal(dx.download(), x0)
    di = dm.dense_tri_info()
    assert di["built"] == 1 and di["correction_launches"] == 2 and dm.sym_info()["correction_launches"] == 0, (di, dm.sym_info())
    # with zero-iterate plans allowed on a bare operator the entry runs on THEM: the merged plans' counter advances, the form's stays put
    dm.tune(zero_plans=2)
    dx.upload(x0)
    dm.gauss_seidel_correction(dx, db, dr)
    merged = dx.download()
    di = dm.dense_tri_info()
    assert di["built"] == 1 and di["zero_launches"] == 3 and di["correction_launches"] == 2, di
    assert dm.sym_info()["correction_launches"] == 1 and dm.lanem_info(4)["rows"] == n and dm.lanem_info(5)["rows"] == n, dm.sym_info()
    ref0, ref1 = _yardstick(A, b, x0)
    assert SF.rel_err(merged, ref1) <= TOL
    # the general sweep from x != 0 of a bare operator has no scratch vector: never the form
    dx.upload(x0)
    dm.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=1, x_is_zero=False)
    assert SF.rel_err(dx.download(), ref1) <= TOL and dm.dense_tri_info()["correction_launches"] == 2
    # switched back (automatic, then on): the correction entry returns to the form, with the bits it gave before
    for value, count in ((0, 3), (2, 4)):
        dm.tune(gs_correction=value)
        dx.upload(x0)
        dm.gauss_seidel_correction(dx, db, dr)
        di = dm.dense_tri_info()
        assert di["built"] == 1 and di["correction_launches"] == count and dm.sym_info()["correction_launches"] == 1, (value, di, dm.sym_info())
        assert np.array_equal(dx.download(), first[1])
    assert not dm.flow_error()
    _free(dx, db, dr, dm)


def test_iterations(nonsym):
    """two iterations from zero on a bare operator (no scratch vector): the first is a zero launch, the second the general sweep; three iterations of the
    correction entry: three correction launches"""
    A, b, x0 = nonsym
    n = A.shape[0]
    dm = _upload(A, 2, 257)
    dx, db, dr = _dev(np.zeros(n), b, np.zeros(n))
    two = _from_zero(dm, dx, db, n, iterations=2)
    di = dm.dense_tri_info()
    assert di["built"] == 1 and di["zero_launches"] == 1 and di["correction_launches"] == 0, di
    e2 = SF.rel_err(two, SF.ref_sweeps(A, np.zeros(n), b, "symmetric", iterations=2, dtype=np.longdouble))
    dx.upload(x0)
    dm.gauss_seidel_correction(dx, db, dr, iterations=3)
    di = dm.dense_tri_info()
    assert di["zero_launches"] == 1 and di["correction_launches"] == 3, di
    e3 = SF.rel_err(dx.download(), SF.ref_sweeps(A, x0, b, "symmetric", iterations=3, dtype=np.longdouble))
    print(f"[dtri families] nonsym: two iterations from zero {e2:.2e}, three in correction form {e3:.2e}")
    assert e2 <= TOL and e3 <= TOL
    assert not dm.flow_error()
    _free(dx, db, dr, dm)


def test_arguments(nonsym):
    A = nonsym[0]
    lib = capi.lib()
    dm = _upload(A, 2, 257)
    for mode, rows in ((3, 0), (-1, 0), (2, -1), (2, 8193)):
        assert lib.pamg_matrix_dense_tri(dm.handle, mode, rows) == capi.E_ARG, (mode, rows)
    assert lib.pamg_matrix_dense_tri(dm.handle, 2, 8192) == 0
    di = dm.dense_tri_info()
    assert di["mode"] == 2 and di["built"] == 0
    dm.free()
    spec = M.hierarchy("convdiff:16", ("gs", "symmetric"))
    dml = DeviceMultilevelSolver(spec, graph=True, order="fast")
    assert lib.pamg_matrix_dense_tri(dml.A[1].handle, 2, 65) == capi.E_STATE, "an operator a solver holds"
    dml.free()


# ------------------------------------------------------------------------------------------------ solver
HIER = "convdiff:16"
SYM, SYM2, CHEB = ("gs", "symmetric"), ("gs", "symmetric", 2), ("chebyshev", 3)


def _counts(smoothers, cycle, cpl):
    """(zero launches, correction launches) per level of ONE cycle from a non-zero iterate, from the recursion of the reference's cycle
    (multilevel.py:584-662).  smoothers[l] = (iterations of a symmetric Gauss-Seidel pre-smoother or 0, the same of the post-smoother); the last level
    is the coarse solve.  A visit from zero: the first iteration of the pre-smoother is a zero launch; everything else runs in correction form"""
    nlev = len(smoothers) + 1
    zero, corr = [0] * nlev, [0] * nlev

    def visit(l, kind, c, from_zero):
        pre, post = smoothers[l]
        if pre:
            zero[l] += 1 if from_zero else 0
            corr[l] += pre - (1 if from_zero else 0)
        if l < nlev - 2:
            if kind == "V":
                visit(l + 1, "V", 1, True)
            elif kind == "W":
                visit(l + 1, "W", c, True)
                visit(l + 1, "W", c, False)
            else:
                visit(l + 1, "F", c, True)
                for _ in range(c):
                    visit(l + 1, "V", 1, False)
        corr[l] += post
    visit(0, cycle, cpl, False)
    return zero, corr


def test_counts_of_the_recursion():
    sm = [(1, 1)] * 3
    assert _counts(sm, "V", 1) == ([0, 1, 1, 0], [2, 1, 1, 0])
    assert _counts(sm, "W", 1) == ([0, 1, 2, 0], [2, 3, 6, 0])
    assert _counts(sm, "F", 1) == ([0, 1, 2, 0], [2, 3, 4, 0])          # level 2: from zero under F and under V, once from x != 0
    assert _counts(sm, "F", 2) == ([0, 1, 3, 0], [2, 5, 7, 0])
    assert _counts([(2, 2)] * 3, "V", 1) == ([0, 1, 1, 0], [4, 3, 3, 0])


def _solve(spec, b, x0, cycle, cpl, **kw):
    """graph replay, a second replay, eager: the same bits; returns (solver, x, residuals, dense_tri_info per level before / after the eager solve)"""
    dml = DeviceMultilevelSolver(spec, graph=True, order="fast", **kw)
    r1, r2, r3 = [], [], []
    args = dict(x0=x0, tol=1e-30, maxiter=K, cycle=cycle, cycles_per_level=cpl)
    x1 = dml.solve(b, residuals=r1, **args)
    x2 = dml.solve(b, residuals=r2, **args)
    capi.check(capi.lib().pamg_solver_set_graph(dml.handle, 0), "pamg_solver_set_graph")
    before = [A.dense_tri_info() for A in dml.A]
    x3 = dml.solve(b, residuals=r3, **args)
    after = [A.dense_tri_info() for A in dml.A]
    assert np.array_equal(x1, x2, equal_nan=True) and np.array_equal(r1, r2, equal_nan=True), "a second solve must give the same bits"
    assert np.array_equal(x1, x3, equal_nan=True) and np.array_equal(r1, r3, equal_nan=True), "graph replay and eager launches must give the same bits"
    for i, A in enumerate(dml.A):
        assert not A.flow_error(), f"flow error on level {i}"
    return dml, x1, np.array(r1), before, after


def _solver_case(tag, pre, post, forms, cycle, cpl, correction_off=()):
    """forms: {level: block rows} switched on by name; asserts parity with the oracle and the per-level counters of K eager cycles.
    correction_off: levels tuned to gs_correction = 1 -- their sweeps from x != 0 stay off the form (and off the merged plans' correction form)"""
    spec = M.hierarchy(HIER, pre, post)
    sizes = [l.A.shape[0] for l in spec.levels]
    assert sizes == [4096, 514, 18, 1]
    n = sizes[0]
    x0, b = np.random.RandomState(77).rand(n), np.random.RandomState(78).rand(n)
    ro = []
    xo = orc.OracleSolver(spec).solve(b, x0=x0, tol=1e-30, maxiter=K, cycle=cycle, cycles_per_level=cpl, residuals=ro)
    ro = np.array(ro)
    tune = (lambda i: {"gs_correction": 1} if i in correction_off else None) if correction_off else None
    dml, x, r, before, after = _solve(spec, b, x0, cycle, cpl, dense_tri={l: dict(mode=2, block_rows=B) for l, B in forms.items()}, level_tune=tune)
    rel, dxr = float(np.max(np.abs(r - ro) / ro)), float(np.linalg.norm(x - xo) / np.linalg.norm(xo))
    its = lambda d: (d[2] if len(d) > 2 else 1) if d[0] == "gs" else 0       # noqa: E731
    zero, corr = _counts([(its(pre), its(post))] * 3, cycle, cpl)
    got = [(a["zero_launches"] - p["zero_launches"], a["correction_launches"] - p["correction_launches"]) for p, a in zip(before, after)]
    print(f"[dtri families] solver {tag} {cycle}{cpl}: residual norms {rel:.2e}, iterate {dxr:.2e} against the oracle; {ro[0]:.3e} -> {ro[-1]:.3e}; "
          f"launches of {K} eager cycles per level (zero, correction) {got}")
    assert rel <= 1e-10 and dxr <= 1e-12, (tag, cycle, rel, dxr)
    for l in range(4):
        di = after[l]
        if l in forms:
            assert di["built"] == 1 and di["block_rows"] == forms[l] and di["blocks"] == -(-sizes[l] // forms[l]) and di["declined_by_growth"] == 0, (l, di)
            assert got[l] == (K * zero[l], 0 if l in correction_off else K * corr[l]), (tag, cycle, cpl, l, got, zero, corr)
            assert dml.A[l].sym_info()["zero_plan_launches"] == 0 and dml.A[l].sym_info()["correction_launches"] == 0, l
        else:
            assert di["built"] == 0 and di["zero_launches"] == 0 and di["correction_launches"] == 0, (l, di)
    dml.free()


CYCLES = [("V", 1), ("W", 1), ("F", 1), ("F", 2)]


@pytest.mark.parametrize("cycle,cpl", CYCLES)
def test_solver_cycles(cycle, cpl):
    """levels 1 (B = 65: 7 full blocks and one of 59 rows) and 2 (B = 7: 7 + 7 + 4 rows); W and F visit them again from x != 0"""
    _solver_case("levels 1, 2", SYM, SYM, {1: 65, 2: 7}, cycle, cpl)


@pytest.mark.parametrize("cycle,cpl", [("W", 1), ("F", 2)])
@pytest.mark.parametrize("tag,pre,post,forms", [
    ("two iterations", SYM2, SYM2, {1: 65, 2: 7}),
    ("gs before, chebyshev after", SYM, CHEB, {1: 65, 2: 7}),
    ("chebyshev before, gs after", CHEB, SYM, {1: 65, 2: 7}),
    ("level 0 by name", SYM, SYM, {0: 257, 1: 65, 2: 7}),
], ids=["iterations2", "gs_cheby", "cheby_gs", "level0"])
def test_solver_smoothers(tag, pre, post, forms, cycle, cpl):
    _solver_case(tag, pre, post, forms, cycle, cpl)


def test_solver_correction_form_switched_off_on_one_level():
    """gs_correction = 1 on level 1: its first visit still pre-smooths from zero on the form, every sweep from x != 0 runs the general kernels; level 2
    keeps both entries on the form"""
    _solver_case("gs_correction = 1 on level 1", SYM, SYM, {1: 65, 2: 7}, "W", 1, correction_off=(1,))


def _spec_with_level_1(A1):
    """a hierarchy whose level 1 is A1: a finest level of twice its rows above it (pairs of unknowns aggregated, P = R^T of ones), tests/midsize.py's
    coarsening below it (the construction of test_gpu_dtri.py's 125-point hierarchy).  Solvers run the same operators; no Galerkin relation is needed"""
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


@pytest.mark.parametrize("name", ["chains7", "nonsym_chain8"])
def test_solver_growth_decline_keeps_the_zero_plans(name):
    """level 1 = chains of 7 rows (growth 1093 at B = 64), or nonsym with a chain of 8 rows laid over it: finalise skipped the level's zero-iterate
    plans for the form and must build them once the guard has declined -- the level then is the level of dense_tri=False: plans, bits, counters.
    (On the band operator neither solver holds zero-iterate plans -- measured: 0 rows in both -- so the second operator, a general sparse one, carries
    the check that they ARE built)"""
    A1 = F.chains(3000, 7) if name == "chains7" else F.nonsym_with_chain(3000, 8)
    growth = 1093.0 if name == "chains7" else F.growth_numpy(A1, 64)
    spec = _spec_with_level_1(A1)
    n = spec.levels[0].A.shape[0]
    assert n == 6000 and spec.levels[1].A.shape[0] == 3000
    x0, b = np.random.RandomState(80).rand(n), np.random.RandomState(81).rand(n)
    dec, xd, rd, _, info_d = _solve(spec, b, x0, "W", 1, dense_tri={1: dict(mode=2, block_rows=64)})
    off, xf, rf, _, info_f = _solve(spec, b, x0, "W", 1, dense_tri=False)
    d1 = info_d[1]
    assert d1["declined_by_growth"] == 1 and d1["built"] == 0 and d1["mode"] == 2 and d1["resident_bytes"] == 0, d1
    assert abs(d1["growth"] - growth) <= 1e-10 * growth, d1
    plans = [(dec.A[1].lanem_info(w), off.A[1].lanem_info(w)) for w in (4, 5)]
    print(f"[dtri families] solver, growth decline on level 1: zero-iterate plans of {[p[0]['rows'] for p in plans]} rows "
          f"(dense_tri=False: {[p[1]['rows'] for p in plans]}); sym_info {dec.A[1].sym_info()}")
    for got, want in plans:
        assert got == want and (got["rows"] > 0) == (name == "nonsym_chain8"), (got, want)
    assert np.array_equal(xd, xf, equal_nan=True) and np.array_equal(rd, rf, equal_nan=True), "the bits of dense_tri=False"
    for l, (A, Bm) in enumerate(zip(dec.A, off.A)):
        assert A.sym_info() == Bm.sym_info(), l
        assert A.info()["hbm_bytes"] == Bm.info()["hbm_bytes"], l
        assert all(info_d[l][k] == info_f[l][k] for k in ("built", "zero_launches", "correction_launches", "resident_bytes")), l
    dec.free()
    off.free()


def _cycles(dml, b, x0, cycle, k=6):
    x, out = np.array(x0), []
    for _ in range(k):
        x = dml.solve(b, x0=x, tol=1e-30, maxiter=1, cycle=cycle)
        out.append(x)
    return out


@pytest.mark.parametrize("cycle", ["V", "W"])
def test_solver_with_dense_tail(cycle):
    """the form on level 1 (514 rows, B = 65) together with a dense tail that starts there: the tail tabulates its operator with the launches it
    replaces -- the form's launches on level 1, counted at tabulation (515 from zero and 515 in correction form for the 514 columns) -- and every
    visit of level 1 in a cycle then is ONE tail launch: the form is built and held, its counters stand still while the tail's applications advance.  On against off 1e-13 per cycle over six cycles, the dense-tail bar"""
    spec = M.hierarchy(HIER, SYM)
    n = spec.levels[0].A.shape[0]
    x0, b = np.random.RandomState(82).rand(n), np.random.RandomState(83).rand(n)
    form = {1: dict(mode=2, block_rows=65)}
    on = DeviceMultilevelSolver(spec, order="fast", graph=False, dense_tri=form, dense_tail=dict(mode=2, max_rows=514))      # (eager: every application is counted)
    off = DeviceMultilevelSolver(spec, order="fast", dense_tri=form, dense_tail=False)
    first = _cycles(on, b, x0, cycle, k=1)
    st1, d1 = on.stats()["dense_tail"], on.A[1].dense_tri_info()
    xs_on = first + _cycles(on, b, first[0], cycle, k=5)
    xs_off = _cycles(off, b, x0, cycle)
    st, di = on.stats()["dense_tail"], on.A[1].dense_tri_info()
    worst = max(float(np.max(np.abs(a - c)) / np.max(np.abs(c))) for a, c in zip(xs_on, xs_off))
    print(f"[dtri families] dense tail from level {st['level']} ({st['rows']} rows) over the form, {cycle}: guard {st['guard']:.2e}, on against off {worst:.2e}; "
          f"level 1 form built {di['built']}, launches (zero, correction) {di['zero_launches'], di['correction_launches']}")
    assert (st["level"], st["rows"]) == (1, 514) and st["built"] >= 1 and st["declined"] is None, st
    assert st["guard"] <= 1e-13 and worst <= 1e-13, (st, worst)
    assert di["built"] == 1 and d1["zero_launches"] >= 1, (d1, di)                               # the tabulation ran the form
    assert (di["zero_launches"], di["correction_launches"]) == (d1["zero_launches"], d1["correction_launches"]), "cycles do not launch the form"
    per_cycle = 2 if cycle == "W" else 1
    assert st1["applications"] == per_cycle and st["applications"] == 6 * per_cycle, (st1, st)
    do = off.A[1].dense_tri_info()
    assert do["built"] == 1 and do["zero_launches"] >= 1 and off.stats()["dense_tail"]["applications"] == 0
    on.free()
    off.free()


@pytest.mark.parametrize("name", ["rs3d_gs_f32", "el2d_pointgs"])
def test_solver_f32_and_bsr_build_nothing(name):
    """asked for by name on every level of a float32 and of a BSR hierarchy: the form is f64 scalar only -- built nowhere, the bits of dense_tri=False"""
    spec, ex = load_spec(GOLD / f"hier_{name}.npz")
    nlev = len(spec.levels)
    cycle = str(ex["cycle"])
    on, x, r, _, info = _solve(spec, ex["b"], ex["x0"], cycle, 1, dense_tri={l: dict(mode=2, block_rows=65) for l in range(nlev)})
    off, xf, rf, _, _ = _solve(spec, ex["b"], ex["x0"], cycle, 1, dense_tri=False)
    for l, di in enumerate(info):
        assert di["built"] == 0 and di["zero_launches"] == 0 and di["correction_launches"] == 0 and di["resident_bytes"] == 0 and di["declined_by_growth"] == 0, (l, di)
        assert on.A[l].info()["hbm_bytes"] == off.A[l].info()["hbm_bytes"], l
    assert np.array_equal(x, xf) and np.array_equal(r, rf)
    on.free()
    off.free()
