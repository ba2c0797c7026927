"""GPU parity of the device-resident BiCGStab / CR / steepest descent / minimal residual accelerators (pamg_solver_krylov):
solve(accel=...) against the reference's own histories on the committed hierarchies (tests/golden/accel_krylov.npz), bit
reproducibility (second solve, graph replay against eager launches), the device-vector entry point, and two mid-size hierarchies
against the NumPy restatements of tests/krylov_ref.py with the device cycle as preconditioner.

Bars as test_device_pcg_matches_reference_history: same list length and info, every residual within 1e-10 ||r0|| (f32: 2e-4),
the solution within 1e-9 relative (f32: 2e-4)."""
import numpy as np
import pytest

from conftest import GOLDEN
import krylov_ref
import midsize
from pyamg_amd import DeviceMultilevelSolver, _capi as capi
from pyamg_amd.hierarchy import load_spec

pytestmark = pytest.mark.gpu


def _cases():
    z = np.load(GOLDEN / "accel_krylov.npz")
    return sorted({k.rsplit(".", 1)[0] for k in z.files if k.endswith(".b") and k.count(".") == 3})


def _solve(dml, method, z, case, tag, cycle):
    res = []
    x, info = dml.solve(z[f"{case}.b"], tol=float(z[f"{case}.{tag}.tol"]), maxiter=int(z[f"{case}.{tag}.maxiter"]), cycle=cycle,
                        accel=method, residuals=res, return_info=True)
    return x, info, res


@pytest.mark.parametrize("case", _cases())
def test_device_krylov_matches_reference_history(case):
    method, name, cycle = case.split(".")
    z = np.load(GOLDEN / "accel_krylov.npz")
    spec, _ = load_spec(GOLDEN / f"hier_{name}.npz")
    f32 = spec.dtype == np.float32
    dml = DeviceMultilevelSolver(spec)
    for tag in ("a", "b"):
        x, info, res = _solve(dml, method, z, case, tag, cycle)
        ref, xr = z[f"{case}.{tag}.res"], z[f"{case}.{tag}.x"]
        assert len(res) == len(ref) and info == int(z[f"{case}.{tag}.info"]), (tag, len(res), len(ref), info)
        assert x.dtype == spec.dtype
        assert np.max(np.abs(np.array(res) - ref)) <= (2e-4 if f32 else 1e-10) * ref[0], tag
        assert np.linalg.norm(x - xr) <= (2e-4 if f32 else 1e-9) * np.linalg.norm(xr), tag
    dml.free()


@pytest.mark.parametrize("case", ["bicgstab.rs2d_nonsym_gs.V", "cr.sa3d_gs.W", "steepest_descent.sa2d_gs.V", "minimal_residual.sa3d_gs.V"])
def test_device_krylov_is_bit_reproducible(case):
    """a second solve and a solve with every cycle launched eagerly (no graph replay) return the same bits"""
    method, name, cycle = case.split(".")
    z = np.load(GOLDEN / "accel_krylov.npz")
    spec, _ = load_spec(GOLDEN / f"hier_{name}.npz")
    dml = DeviceMultilevelSolver(spec)
    x1, i1, r1 = _solve(dml, method, z, case, "b", cycle)
    x2, i2, r2 = _solve(dml, method, z, case, "b", cycle)
    capi.check(capi.lib().pamg_solver_set_graph(dml.handle, 0), "pamg_solver_set_graph")
    x3, i3, r3 = _solve(dml, method, z, case, "b", cycle)
    assert np.array_equal(x1, x2) and r1 == r2 and i1 == i2
    assert np.array_equal(x1, x3) and r1 == r3 and i1 == i3
    dml.free()


def test_krylov_device_entry_point_and_workspace():
    """krylov_device on device vectors is what solve(accel=...) computes; the work vectors are allocated once, on first use"""
    z = np.load(GOLDEN / "accel_krylov.npz")
    case = "bicgstab.sa2d_gs.V"
    spec, _ = load_spec(GOLDEN / "hier_sa2d_gs.npz")
    n = spec.levels[0].A.shape[0]
    dml = DeviceMultilevelSolver(spec)
    b = z[f"{case}.b"]
    tol, maxiter = float(z[f"{case}.b.tol"]), int(z[f"{case}.b.maxiter"])
    before = dml.stats()["hbm_bytes"]
    ress = []
    xs, infos = dml.solve(b, tol=tol, maxiter=maxiter, accel="bicgstab", residuals=ress, return_info=True)
    grown = dml.stats()["hbm_bytes"]
    assert grown >= before + 5 * n * 8
    xd, bd = capi.DeviceArray(n, np.float64), capi.DeviceArray.from_host(b)
    xd.zero()
    res, nit, info = dml.krylov_device("bicgstab", xd, bd, tol=tol, maxiter=maxiter)
    assert np.array_equal(xd.download(), xs) and list(res) == ress and info == infos and nit == len(res) - 1
    # the other methods share the first work vectors: nothing more is allocated for them
    for m in ("cr", "steepest_descent", "minimal_residual"):
        xd.zero()
        dml.krylov_device(m, xd, bd, tol=1e-6, maxiter=5)
    assert dml.stats()["hbm_bytes"] == grown
    with pytest.raises(ValueError):
        dml.krylov_device("cgne", xd, bd)
    dml.free()


def test_gmres_householder_runs_the_device_gmres():
    """'gmres_householder' is the reference's default GMRES: the same device method as accel='gmres'"""
    spec, ex = load_spec(GOLDEN / "hier_rs2d_nonsym_gs.npz")
    dml = DeviceMultilevelSolver(spec)
    r1, r2 = [], []
    x1 = dml.solve(ex["b"], tol=1e-8, maxiter=20, accel="gmres", residuals=r1)
    x2 = dml.solve(ex["b"], tol=1e-8, maxiter=20, accel="gmres_householder", residuals=r2)
    assert np.array_equal(x1, x2) and r1 == r2
    dml.free()


def test_callback_keeps_the_host_path():
    """callback= needs the iterate on the host after every iteration: the host Krylov method runs around the device cycle"""
    z = np.load(GOLDEN / "accel_krylov.npz")
    case = "bicgstab.sa3d_gs.V"
    spec, _ = load_spec(GOLDEN / "hier_sa3d_gs.npz")
    dml = DeviceMultilevelSolver(spec)
    seen, res = [], []
    x, info = dml.solve(z[f"{case}.b"], tol=float(z[f"{case}.b.tol"]), maxiter=int(z[f"{case}.b.maxiter"]), accel="bicgstab",
                        callback=lambda xk: seen.append(np.array(xk, copy=True)), residuals=res, return_info=True)
    assert len(seen) == len(res) - 1 and len(seen) >= 1
    assert all(isinstance(v, np.ndarray) and v.shape == x.shape for v in seen)
    dml.free()


@pytest.mark.parametrize("which", [("bicgstab", "convdiff:64", ("gs_nr", "symmetric"), 1e-8),
                                   ("cr", "poisson:64x96x200", ("gs", "symmetric"), 1e-6)],
                         ids=["bicgstab_convdiff64_gsnr", "cr_poisson_64x96x200"])
def test_midsize_against_restatement(which):
    method, problem, smoother, tol = which
    spec = midsize.hierarchy(problem, smoother)
    dml = DeviceMultilevelSolver(spec)
    n = spec.levels[0].A.shape[0]
    A = spec.levels[0].A.to_scipy()
    b = np.random.RandomState(11).rand(n)
    res = []
    x, info = dml.solve(b, tol=tol, maxiter=40, accel=method, residuals=res, return_info=True)
    for i, Ad in enumerate(dml.A):
        assert not Ad.flow_error(), f"flow error on level {i}"
    M = dml.aspreconditioner()
    xr, infor, rr = krylov_ref.METHODS[method](A, b, lambda v: M @ v, tol=tol, maxiter=40)
    res, rr = np.array(res), np.array(rr)
    print(f"\n[midsize krylov] {method} {problem}: {len(res) - 1} iterations, info {info}, residuals {res[0]:.3e} -> {res[-1]:.3e}")
    assert len(res) == len(rr) and info == infor
    m = min(8, len(rr))
    assert np.max(np.abs(res[:m] - rr[:m]) / rr[:m]) <= 1e-9
    assert np.max(np.abs(res - rr)) <= 1e-9 * rr[0]
    assert np.linalg.norm(x - xr) <= 1e-8 * np.linalg.norm(xr)
    dml.free()
