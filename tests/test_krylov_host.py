"""Device BiCGStab / CR / steepest descent / minimal residual, host side: the C ABI of pamg_solver_krylov and the test's own
NumPy restatements (tests/krylov_ref.py) against the reference's recorded histories (tests/golden/accel_krylov.npz, made by
tests/golden/make_golden_krylov.py) with the oracle's cycle as preconditioner.  No GPU needed."""
import ctypes
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import krylov_ref
from pyamg_amd import _capi as capi


def test_header_declares_the_krylov_entry_point():
    hdr = (ROOT / "include" / "pyamg_amd.h").read_text()
    consts = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define PAMG_ACCEL_([A-Z_]+)\s+(\d+)", hdr)}
    assert consts == capi.ACCEL
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"int pamg_solver_krylov\(([^)]*)\);", code)
    assert m, "pamg_solver_krylov is not declared"
    assert len(m.group(1).split(",")) == 14
    assert hasattr(ctypes.CDLL(str(capi.LIB_PATH)), "pamg_solver_krylov")


def _cases():
    z = np.load(GOLDEN / "accel_krylov.npz")
    return sorted({k.rsplit(".", 1)[0] for k in z.files if k.endswith(".b") and k.count(".") == 3})


def test_fixture_covers_the_issue_cases():
    cases = _cases()
    methods = {c.split(".")[0] for c in cases}
    assert methods == set(capi.ACCEL)
    assert any(c.endswith(".W") for c in cases)
    assert "bicgstab.rs3d_gs_f32.V" in cases and "bicgstab.el2d_blockgs.V" in cases
    assert (GOLDEN / "accel_krylov.npz").stat().st_size < 1 << 20


@pytest.mark.parametrize("case", _cases())
def test_restatements_reproduce_the_reference(case, load_hier):
    from oracle import oracle as orc
    method, name, cycle = case.split(".")
    spec, _ = load_hier(name)
    osol = orc.OracleSolver(spec)
    A = spec.levels[0].A.to_scipy()
    z = np.load(GOLDEN / "accel_krylov.npz")
    b = z[f"{case}.b"]

    def M(v):
        return osol.solve(v, tol=1e-12, maxiter=1, cycle=cycle)

    for tag in ("a", "b"):
        x, info, res = krylov_ref.METHODS[method](A, b, M, tol=float(z[f"{case}.{tag}.tol"]), maxiter=int(z[f"{case}.{tag}.maxiter"]))
        ref, xr = z[f"{case}.{tag}.res"], z[f"{case}.{tag}.x"]
        assert len(res) == len(ref) and info == int(z[f"{case}.{tag}.info"]), (case, tag, len(res), len(ref), info)
        assert np.max(np.abs(np.array(res) - ref) / ref) <= 1e-12, (case, tag)
        assert np.linalg.norm(x - xr) <= 1e-12 * np.linalg.norm(xr), (case, tag)
