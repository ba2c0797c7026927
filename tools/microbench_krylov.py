#!/usr/bin/env python3
"""Per-iteration cost of the device BiCGStab / CR accelerators (pamg_solver_krylov) against what one iteration is made of and
against the host path they replace.  Not product code.

    python tools/microbench_krylov.py [--iters K] [--reps R]

For two SA hierarchies (tests/midsize.py: 3-D Poisson 128^3 with symmetric Gauss-Seidel, convection-diffusion 64^3 with
gauss_seidel_nr) and each method it prints, from the same run:
  * ms per iteration of krylov_device (K iterations, tol = 1e-30, one warm-up solve first);
  * ms per cycle (cycle_device) and per fine-level SpMV;
  * ms per iteration of the host path: _host_krylov with the NumPy restatement of tests/krylov_ref.py as the accelerator,
    i.e. host vectors and one PCIe round trip per preconditioner application.
BiCGStab costs 2 cycles + 2 SpMVs per iteration, CR 1 cycle + 1 SpMV: `overhead` is the rest, relative to that sum."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import krylov_ref  # noqa: E402
import midsize  # noqa: E402
from pyamg_amd import DeviceMultilevelSolver, _capi as capi  # noqa: E402

CASES = [("poisson:128x128x128", ("gs", "symmetric")), ("convdiff:64", ("gs_nr", "symmetric"))]
PER_ITER = {"bicgstab": (2, 2), "cr": (1, 1)}      # (cycles, fine-level SpMVs) per iteration


def wall(fn, reps):
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    capi.sync()
    return (time.perf_counter() - t) * 1e3 / reps


def pyamg_style(method):
    """the restatement behind the reference's keyword interface, for _host_krylov"""
    def run(A, b, x0=None, tol=1e-5, maxiter=None, M=None, callback=None, residuals=None):
        x, info, res = krylov_ref.METHODS[method](A, b, lambda v: M @ v, tol=tol, maxiter=maxiter)
        if residuals is not None:
            residuals[:] = res
        return x, info
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    K = a.iters
    for problem, smoother in CASES:
        t = time.time()
        spec = midsize.hierarchy(problem, smoother)
        dml = DeviceMultilevelSolver(spec)
        n = spec.levels[0].A.shape[0]
        print(f"{problem} {smoother[0]}: {len(spec.levels)} levels, n = {n}, setup {time.time() - t:.1f} s", flush=True)
        b = np.random.RandomState(3).rand(n)
        xd, bd, yd = capi.DeviceArray(n, np.float64), capi.DeviceArray.from_host(b), capi.DeviceArray(n, np.float64)
        ms_cycle = wall(lambda: dml.cycle_device(xd, bd), a.reps)
        ms_spmv = wall(lambda: dml.A[0].spmv(capi.SPMV_SET, bd, yd), a.reps)
        for method in ("bicgstab", "cr"):
            def device():
                xd.zero()
                res, nit, info = dml.krylov_device(method, xd, bd, tol=1e-30, maxiter=K)
                assert nit == K, (method, nit, info)
            device()
            ms_dev = wall(device, 1) / K
            t = time.perf_counter()
            dml._host_krylov(b, None, 1e-30, K, "V", pyamg_style(method), None, None, False)
            ms_host = (time.perf_counter() - t) * 1e3 / K
            nc, ns = PER_ITER[method]
            parts = nc * ms_cycle + ns * ms_spmv
            rec = {"problem": problem, "smoother": smoother[0], "n": n, "method": method, "iters": K,
                   "device_ms_per_iter": round(ms_dev, 3), "cycle_ms": round(ms_cycle, 3), "spmv_ms": round(ms_spmv, 3),
                   "cycles_plus_spmvs_ms": round(parts, 3), "overhead_pct": round(100 * (ms_dev - parts) / parts, 1),
                   "host_ms_per_iter": round(ms_host, 3), "host_over_device": round(ms_host / ms_dev, 2)}
            print(json.dumps(rec), flush=True)
        dml.free()


if __name__ == "__main__":
    main()
