#!/usr/bin/env python3
"""Generate tests/golden/accel_krylov.npz: the reference's own BiCGStab / CR / steepest descent / minimal residual on the
committed hierarchies, preconditioned exactly as MultilevelSolver.solve(accel=...) preconditions them.

Run in the build container (needs the reference built into oracle/_ref by oracle/build_ref.py):
    python tests/golden/make_golden_krylov.py

For each case the committed ``hier_<name>.npz`` spec is loaded and the reference's ``pyamg.krylov.<method>`` runs with
A = level 0 and M = LinearOperator(v -> OracleSolver(spec).solve(v, tol=1e-12, maxiter=1, cycle=cycle)) -- what
``ml.solve(accel=...)`` calls (multilevel.py:508-516, ``aspreconditioner`` :355-396), with the oracle's cycle in place of the
reference's.  The construction is proven first: the same harness with ``pyamg.krylov.cg`` / ``fgmres`` reproduces the committed
accel_cg.npz / accel_fgmres.npz histories (bit for bit where the oracle's cycle is bit-exact to the reference, 1e-12 relative
elsewhere).

Keys: ``<method>.<name>.<cycle>.b`` and ``.<tag>.{tol,maxiter,res,info,x}`` with tag ``a`` (stops on maxiter) and ``b``
(converges; the last two residuals are >= 1 % away from the threshold so the list length is robust to rounding).
"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

import oracle.refimport  # noqa: E402,F401
import pyamg.krylov as krylov  # noqa: E402
from scipy.sparse.linalg import LinearOperator  # noqa: E402

from oracle import oracle as orc  # noqa: E402
from pyamg_amd.hierarchy import load_spec  # noqa: E402

SEED = 20261016
CASES = ([("bicgstab", n, None) for n in ("sa2d_gs", "sa3d_gs", "el2d_blockgs", "rs2d_nonsym_gs", "bb2d_nonsym_gsnr", "air2d_fcjacobi",
                                          "rs3d_gs_f32")]
         + [("bicgstab", "sa2d_gs", "W")]
         + [("cr", n, None) for n in ("sa2d_gs", "sa3d_gs", "el2d_blockgs")] + [("cr", "sa3d_gs", "W")]
         + [("steepest_descent", n, None) for n in ("sa2d_gs", "sa3d_gs")]
         + [("minimal_residual", n, None) for n in ("sa2d_gs", "sa3d_gs", "rs2d_nonsym_gs")])
A_RUN = dict(tol=1e-30, maxiter=3)
B_TOLS = (1e-6, 1.3e-6, 7e-7, 2e-6, 5e-7, 3e-6, 1e-5, 1e-4, 1e-3, 2e-3, 3e-3, 1e-2)   # first one whose last two residuals clear the threshold by 1 %
B_MAXITER = 300


def harness(name, cycle):
    spec, ex = load_spec(HERE / f"hier_{name}.npz")
    cycle = cycle or str(ex["cycle"])
    A = spec.levels[0].A.to_scipy()
    osol = orc.OracleSolver(spec)
    M = LinearOperator(A.shape, lambda v: osol.solve(v, tol=1e-12, maxiter=1, cycle=cycle), dtype=A.dtype)
    return spec, A, M, cycle


def run(method, A, b, M, **kw):
    res = []
    x, info = getattr(krylov, method)(A, b, x0=None, M=M, residuals=res, **kw)
    return x, info, np.array(res)


def prove_construction():
    """the harness reproduces the reference's own ml.solve(accel='cg' / 'fgmres') histories"""
    for fname, method, prefix in (("accel_cg.npz", "cg", ""), ("accel_fgmres.npz", "fgmres", "")):
        z = np.load(HERE / fname)
        names = sorted({k.split(".")[0] for k in z.files})
        for name in names:
            _, A, M, cycle = harness(name, str(z[f"{name}.cycle"]))
            b = z[f"{name}.b"]
            for tag in ("a", "b"):
                x, info, res = run(method, A, b, M, tol=float(z[f"{name}.{tag}.tol"]), maxiter=int(z[f"{name}.{tag}.maxiter"]))
                ref, xr = z[f"{name}.{tag}.res"], z[f"{name}.{tag}.x"]
                assert len(res) == len(ref) and info == int(z[f"{name}.{tag}.info"]), (fname, name, tag)
                exact = np.array_equal(res, ref) and np.array_equal(x, xr)
                dr = np.max(np.abs(res - ref) / ref)
                dx = np.linalg.norm(x - xr) / np.linalg.norm(xr)
                assert exact or (dr <= 1e-12 and dx <= 1e-12), (fname, name, tag, dr, dx)
                print(f"construction {method:7s} {name:18s} {tag}: {'bit-exact' if exact else f'dr {dr:.1e} dx {dx:.1e}'}")


def main():
    prove_construction()
    out = {}
    for method, name, cyc in CASES:
        spec, A, M, cycle = harness(name, cyc)
        n = A.shape[0]
        b = np.random.RandomState(SEED + n).rand(n).astype(spec.dtype)
        key = f"{method}.{name}.{cycle}"
        out[f"{key}.b"] = b
        x, info, res = run(method, A, b, M, **A_RUN)
        assert info == A_RUN["maxiter"], (key, info)
        out.update({f"{key}.a.tol": np.array(A_RUN["tol"]), f"{key}.a.maxiter": np.array(A_RUN["maxiter"]), f"{key}.a.res": res,
                    f"{key}.a.info": np.array(info), f"{key}.a.x": x})
        if method == "minimal_residual":
            normb = np.linalg.norm(b)
            scale = np.linalg.norm(M @ b) if normb != 0.0 else 1.0
        else:
            scale = np.linalg.norm(b) or 1.0
        for tol in B_TOLS:
            x, info, res = run(method, A, b, M, tol=tol, maxiter=B_MAXITER)
            thr = tol * scale
            if info == 0 and len(res) >= 2 and all(abs(v - thr) >= 0.01 * thr for v in res[-2:]):
                break
        else:
            raise AssertionError(f"{key}: no converging tol with a 1 % margin")
        out.update({f"{key}.b.tol": np.array(tol), f"{key}.b.maxiter": np.array(B_MAXITER), f"{key}.b.res": res,
                    f"{key}.b.info": np.array(info), f"{key}.b.x": x})
        print(f"{key:40s} a: {len(out[key + '.a.res'])} residuals; b: tol {tol:g}, {len(res)} residuals, info {info}")
    np.savez_compressed(HERE / "accel_krylov.npz", **out)
    print("accel_krylov.npz written:", len(out), "arrays,", (HERE / "accel_krylov.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
