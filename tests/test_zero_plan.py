"""Zero-iterate plans of the merged lane-parallel Gauss-Seidel sweep (CPU, no GPU; tune key 39).  A symmetric sweep that starts from x = 0 is
    forward : the merged forward plan Zf of tril(A) -- the strictly upper entries multiply zeros;
    backward: the merged backward plan Zb of triu(A) with right-hand side w = D y -- after the forward sweep b_r - sum_{j<r} a_rj y_j = a_rr y_r
              for every updated row, the numerator the forward row holds (the device stores it; here it is formed as diag(A) * y).
Both plans come from the project's own planner (pyamg_amd/csrc/pamg_lanem_plan.h) and are replayed by the existing emulators' entry points
(tests/lanec_emul.cpp: cluster layout of 4 / 8 rows; tests/lanem_emul.cpp: one row per wave and the pair layout), built into a scratch directory of
this test's own.  Checked, at depths s = 3, 8, 16 in every layout: Zf from zero followed by Zb equals the oracle's symmetric sweep from zero to
1e-13 relative (the bar of test_lanec_plan.py); OLD operands occur only where rows lack a usable diagonal; a triangular plan holds at most the
operands of the full plan; the replay runs in the adversarial wave order, so its deadlock check (a polled operand whose producer has not
published when no wave can move) is part of every case.
Operators: level 1 of the golden smoothed-aggregation hierarchies, the chains operator of test_lanem_plan.py / test_lanec_plan.py (|a_ir / a_rr| =
3: the growth bound closes super-levels early) and an SA level with every fifth diagonal removed."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle as orc
from pyamg_amd.hierarchy import load_spec

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
GOLDEN = HERE / "golden"
TOL = 1e-13
DEPTHS = (3, 8, 16)
LAYOUTS = (("cluster", 4), ("cluster", 8), ("row", 1), ("pair", 2))
WAVES = 7                                                                  # replay order: the last wave first (adversarial), 7 waves
SA_LEVEL1 = ("sa3d_gs", "sa2d_gs", "sa2d_sor", "sa2d_cheby")


@pytest.fixture(scope="module")
def emul():
    out = HERE / "build" / "zero_plan"
    out.mkdir(parents=True, exist_ok=True)
    hdrs = [ROOT / "pyamg_amd" / "csrc" / h for h in ("pamg_lanem_plan.h", "pamg_lane_plan.h", "pamg_tile_plan.h")]
    libs = {}
    for name in ("lanec_emul", "lanem_emul"):
        so, src = out / f"{name}.so", HERE / f"{name}.cpp"
        if not so.exists() or so.stat().st_mtime < max([src.stat().st_mtime] + [h.stat().st_mtime for h in hdrs]):
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
        libs[name] = ctypes.CDLL(str(so))
    libs["lanec_emul"].lanec_emul_sweep_f64.restype = ctypes.c_int
    libs["lanem_emul"].lanem_emul_sweep_f64.restype = ctypes.c_int
    return libs


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _csr(A):
    A = sp.csr_array(A)
    A.sort_indices()
    return (A, np.ascontiguousarray(A.indptr, dtype=np.int32), np.ascontiguousarray(A.indices, dtype=np.int32), np.ascontiguousarray(A.data, dtype=np.float64))


def sweep(libs, layout, A, x, b, direction, s_max, growth_cap=1e3, waves=WAVES):
    """one directional merged sweep of x over all rows through the emulator of `layout`; returns (rc, x, operand counts)"""
    A, Ap, Aj, Ax = _csr(A)
    n = A.shape[0]
    start, stop, step = (0, n, 1) if direction > 0 else (n - 1, -1, -1)
    xx = np.array(x, dtype=np.float64)
    bb = np.ascontiguousarray(b, dtype=np.float64)
    kind, arg = layout
    if kind == "cluster":
        st = np.zeros(18, dtype=np.int64)
        rc = libs["lanec_emul"].lanec_emul_sweep_f64(ctypes.c_int(n), _p(Ap), _p(Aj), _p(Ax), _p(xx), _p(bb), start, stop, step, s_max,
                                                     ctypes.c_double(growth_cap), arg, _p(st), waves, 0)
    else:
        st = np.zeros(16, dtype=np.int64)
        gs = np.zeros(2)
        rc = libs["lanem_emul"].lanem_emul_sweep_f64(ctypes.c_int(n), _p(Ap), _p(Aj), _p(Ax), _p(xx), _p(bb), start, stop, step, s_max,
                                                     ctypes.c_double(growth_cap), 512, _p(st), _p(gs), waves, 0, arg)
    return rc, xx, dict(super=int(st[0]), levels=int(st[1]), early=int(st[4]), old=int(st[5]), b=int(st[6]))


def zero_sweep(libs, layout, A, b, s_max, **kw):
    """Zf from zero, then Zb with w = diag(A) * y: (rc, x, stats of Zf, stats of Zb)"""
    A = sp.csr_array(A)
    n = A.shape[0]
    rc, y, sf = sweep(libs, layout, sp.tril(A, format="csr"), np.zeros(n), b, +1, s_max, **kw)
    if rc:
        return rc, y, sf, None
    w = A.diagonal() * y
    rc, x, sb = sweep(libs, layout, sp.triu(A, format="csr"), y, w, -1, s_max, **kw)
    return (200 + rc if rc else 0), x, sf, sb


def ref_symmetric_from_zero(A, b):
    A, Ap, Aj, Ax = _csr(A)
    n = A.shape[0]
    x = np.zeros(n)
    bb = np.ascontiguousarray(b, dtype=np.float64)
    orc.gauss_seidel(Ap, Aj, Ax, x, bb, 0, n, 1)
    orc.gauss_seidel(Ap, Aj, Ax, x, bb, n - 1, -1, -1)
    return x


def chains(n=400):
    main, off = np.full(n, 1.0), np.full(n - 1, -3.0)
    off[23::24] = 0.0                                                  # chains of 24 rows: the sweep itself stays finite (3^23)
    return sp.csr_array(sp.diags_array([off, main, 0.1 * off], offsets=[-1, 0, 1]))


def sa_level1(name):
    spec = load_spec(GOLDEN / f"hier_{name}.npz")[0]
    A = sp.csr_array(spec.levels[1].A.to_scipy()).astype(np.float64)
    assert A.shape[0] == A.shape[1]
    return A


def without_some_diagonals(A, every=5):
    A = sp.lil_array(A)
    for i in range(0, A.shape[0], every):
        A[i, i] = 0.0
    A = sp.csr_array(A)
    A.eliminate_zeros()
    return A


def _rel(got, ref):
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


def _check(libs, name, A, b, nodiag=False):
    ref = ref_symmetric_from_zero(A, b)
    n = A.shape[0]
    for layout in LAYOUTS:
        for s in DEPTHS:
            rc, x, sf, sb = zero_sweep(libs, layout, A, b, s)
            assert rc == 0, (name, layout, s, rc)
            err = _rel(x, ref)
            full = [sweep(libs, layout, A, np.zeros(n), b, d, s) for d in (+1, -1)]
            assert full[0][0] == 0 and full[1][0] == 0, (name, layout, s)
            print(f"[zero plan] {name} {layout[0]} {layout[1]} s={s}: |dx|/|x| = {err:.2e}; operands per row Zf {sum(sf[k] for k in ('early', 'old', 'b')) / n:.1f} "
                  f"Zb {sum(sb[k] for k in ('early', 'old', 'b')) / n:.1f}, full {sum(full[0][2][k] for k in ('early', 'old', 'b')) / n:.1f} / "
                  f"{sum(full[1][2][k] for k in ('early', 'old', 'b')) / n:.1f}; super-levels {sf['super']} / {sb['super']} (full {full[0][2]['super']} / {full[1][2]['super']})")
            assert err <= TOL, (name, layout, s, err)
            for z, f in ((sf, full[0][2]), (sb, full[1][2])):
                assert z["early"] + z["old"] + z["b"] <= f["early"] + f["old"] + f["b"], (name, layout, s, z, f)
                if not nodiag:
                    assert z["old"] == 0, (name, layout, s, z)


@pytest.mark.parametrize("name", SA_LEVEL1)
def test_zero_plans_on_sa_level1(emul, name):
    A = sa_level1(name)
    _check(emul, name, A, np.random.RandomState(2).rand(A.shape[0]))


def test_zero_plans_on_chains(emul):
    A = chains()
    _check(emul, "chains", A, np.random.RandomState(3).rand(A.shape[0]))


def test_zero_plans_with_rows_that_lack_a_diagonal(emul):
    """rows without a usable diagonal keep their value (zero) in both halves; they alone bring OLD operands into the triangular plans -- the same
    operator with its diagonal whole has none (checked above), and unmerged (s = 1) every entry of a triangle is polled, so none appear either"""
    base = sa_level1("sa2d_gs")
    A = without_some_diagonals(base)
    n = A.shape[0]
    b = np.random.RandomState(4).rand(n)
    _check(emul, "sa2d_gs without every fifth diagonal", A, b, nodiag=True)
    ref = ref_symmetric_from_zero(A, b)
    assert np.array_equal(ref[0::5], np.zeros(len(ref[0::5])))
    for layout in LAYOUTS:
        rc, x, sf, sb = zero_sweep(emul, layout, A, b, 8)
        assert rc == 0 and np.array_equal(x[0::5], np.zeros(len(x[0::5]))), (layout, rc)
        assert sf["old"] > 0 or sb["old"] > 0, (layout, sf, sb)       # the case exercises what it is meant to
        rc, x, sf, sb = zero_sweep(emul, layout, A, b, 1)
        assert rc == 0 and sf["old"] == 0 and sb["old"] == 0 and sf["b"] == 0 and sb["b"] == 0, (layout, rc, sf, sb)
        assert _rel(x, ref) <= TOL
