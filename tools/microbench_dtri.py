#!/usr/bin/env python3
"""The dense block-triangular form of the symmetric Gauss-Seidel sweep (pamg_matrix_dense_tri) against the merged zero-iterate plans on ONE level of
the SA hierarchy of 3-D Poisson (default: level 2 of 256^3), same session, --reps repetitions of 10 interleaved applications each of
  * the present launch announced from zero (zero-iterate plans),
  * the present correction form (residual + accumulating launch),
  * the dense form at every --block-rows, from zero and in correction form
(profiles/r17_microbench_dtri_scan.json; the default block size, DTRI_BLOCK_ROWS in csrc/pamg_dtri_plan.h, is this scan's winner).
--operator FILE.npz (indptr, indices, data of a CSR operator) times that operator instead of building the hierarchy with the reference.
The timed applications follow one another on the same vectors: the kernels' work does not depend on the data.  Not product code."""
import argparse, json, sys, time
from pathlib import Path
import numpy as np
import scipy.sparse as sp
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from pyamg_amd import _capi as capi
from pyamg_amd.hierarchy import sparse_op
from pyamg_amd.multilevel import DeviceMatrix

ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, nargs="+", default=[256, 256, 256])
ap.add_argument("--level", type=int, default=2)
ap.add_argument("--operator", default=None)
ap.add_argument("--block-rows", type=int, nargs="+", default=[512, 1024, 2048, 4096])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if a.operator:
    z = np.load(a.operator)
    n = int(z["indptr"].size - 1)
    op = sparse_op(sp.csr_array((z["data"], z["indices"], z["indptr"]), shape=(n, n)))
    source = f"operator file {Path(a.operator).name}"
else:
    import oracle.refimport  # noqa: F401
    import pyamg
    from pyamg_amd.aggregation import device_setup
    from pyamg_amd.hierarchy import extract
    np.random.seed(1)
    with device_setup(pyamg):
        ml = pyamg.smoothed_aggregation_solver(pyamg.gallery.poisson(tuple(a.grid), format="csr"), max_coarse=10)
    op = extract(ml).levels[a.level].A
    source = f"level {a.level} of the SA hierarchy of Poisson {a.grid}"
n = op.shape[0]
print(f"{source}: {n} rows, {op.nnz} entries", flush=True)


def timeit(fn, reps=10):
    fn(); fn(); capi.sync()
    e0, e1 = capi.Event(), capi.Event()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_ms(e1) / reps


rs = np.random.RandomState(1)
x, b = rs.rand(n), rs.rand(n)
dx, db, dr = capi.DeviceArray.from_host(x), capi.DeviceArray.from_host(b), capi.DeviceArray.from_host(np.zeros(n))
ops, build_s = {}, {}
t0 = time.time()
M0 = DeviceMatrix(op)
M0.tune(gs_order=1, lane_wide=1, zero_plans=2)
M0.dense_tri(1)
dx.upload(np.zeros(n))
M0.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=1, x_is_zero=True)
ref_zero = dx.download()
dx.upload(x)
M0.gauss_seidel_correction(dx, db, dr)
ref_corr = dx.download()
build_s["merged"] = round(time.time() - t0, 2)
variants = {"merged_zero": lambda: M0.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=1, x_is_zero=True),
            "merged_correction": lambda: M0.gauss_seidel_correction(dx, db, dr)}
info, err = {}, {}
for B in a.block_rows:
    t0 = time.time()
    m = DeviceMatrix(op)
    m.tune(gs_order=1, lane_wide=1)
    m.dense_tri(2, B)
    dx.upload(np.zeros(n))
    m.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=1, x_is_zero=True)
    ez = float(np.max(np.abs(dx.download() - ref_zero)) / np.max(np.abs(ref_zero)))
    dx.upload(x)
    m.gauss_seidel_correction(dx, db, dr)
    ec = float(np.max(np.abs(dx.download() - ref_corr)) / np.max(np.abs(ref_corr)))
    build_s[f"dtri_{B}"] = round(time.time() - t0, 2)
    info[B], err[B], ops[B] = m.dense_tri_info(), (ez, ec), m
    assert info[B]["built"] == 1, info[B]
    variants[f"dtri_{B}_zero"] = (lambda m=m: m.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=1, x_is_zero=True))
    variants[f"dtri_{B}_correction"] = (lambda m=m: m.gauss_seidel_correction(dx, db, dr))
    print(f"B={B}: {info[B]}, rel. difference from zero {ez:.2e}, correction {ec:.2e}", flush=True)
ms = {k: [] for k in variants}
for _ in range(a.reps):                                 # interleaved: a drift of the session hits every variant alike
    for k, fn in variants.items():
        ms[k].append(round(timeit(fn), 4))
out = {"source": source, "rows": int(n), "nnz": int(op.nnz), "reps": a.reps, "applications_per_rep": 10, "launches": "eager, one stream", "ms": ms,
       "dense_tri_info": {str(B): info[B] for B in info}, "rel_diff_vs_merged_zero_and_correction": {str(B): err[B] for B in err},
       "build_and_first_sweeps_s": build_s, "timeout": bool(M0.flow_error())}
print(json.dumps(out), flush=True)
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1))
print("done")
