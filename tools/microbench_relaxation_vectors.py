#!/usr/bin/env python3
"""Device time of the relaxation of a block of R random vectors (``relaxation_vectors``, the first step of ``algebraic_distance`` and
``affinity_distance``) on the 7-point Laplacian, everything resident, copies excluded:

  multi    k launches of the multi-vector sweep of csrc/pamg_distance.hip: one record of R doubles per node, A read once per sweep
  single   R k launches of the resident single-vector Jacobi step (``pamg_matrix_jacobi_step``): what the package could do before
  tail     the fused measure-and-filter kernel (algebraic distance, p = 2) on the relaxed block

and, as wall time, what surrounds them: the creation of the resident matrix the single-vector step needs (upload and plan), and the
whole Layer-1 call ``relaxation_vectors`` on host arrays (upload, k sweeps, download).

Both relaxation variants run in one process, alternating, ``--runs`` times after one warm-up each; medians, and the spread (min, max)
of each.  Times are device events around the launches of one variant.  The shares of peak are the algorithmic bytes -- per sweep
``12 nnz + 4 (n + 1) + 16 n R``, for the tail ``12 nnz + 8 n R + 8 nnz`` -- over the time, against 8 TB/s.  Before anything is timed the
first column of the multi-vector result is compared with k single-vector steps on the same column: the bits must be the same.

    python tools/microbench_relaxation_vectors.py --n 128          # -> profiles/relaxation_vectors_n128.json  (--out DIR: somewhere else)
    python tools/microbench_relaxation_vectors.py --n 256
    python tools/microbench_relaxation_vectors.py --n 128 --reference     # one host core, the reference from oracle/_ref; no GPU needed

Not product code."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=128, help="grid points per side")
ap.add_argument("--R", type=int, default=5)
ap.add_argument("--k", type=int, default=20)
ap.add_argument("--omega", type=float, default=0.5)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--reference", action="store_true", help="time the reference's relaxation_vectors and algebraic_distance on the host instead")
ap.add_argument("--out", default=str(ROOT / "profiles"))
a = ap.parse_args()

from tools.problems import poisson_csr  # noqa: E402

PEAK = 8.0e12                                               # bytes per second
A = poisson_csr((a.n,) * 3)
n, nnz, R, k = A.shape[0], A.nnz, a.R, a.k
sweep_bytes = 12 * nnz + 4 * (n + 1) + 16 * n * R
tail_bytes = 12 * nnz + 8 * n * R + 8 * nnz
rec = {"operator": f"7-point Laplacian {a.n}^3", "rows": n, "nnz": nnz, "R": R, "k": k, "omega": a.omega, "runs": a.runs,
       "sweep_bytes": sweep_bytes, "tail_bytes": tail_bytes}

if a.reference:
    import oracle.refimport as ri
    if not ri.available():
        sys.exit("oracle/_ref is not here: nothing to measure")
    import pyamg.strength as rstr
    np.random.seed(1)
    t0 = time.perf_counter()
    rstr.relaxation_vectors(A, R, k, a.omega)
    t1 = time.perf_counter()
    np.random.seed(1)
    rstr.algebraic_distance(A, alpha=a.omega, R=R, k=k)
    t2 = time.perf_counter()
    rec.update({"reference_relaxation_vectors_s": t1 - t0, "reference_algebraic_distance_s": t2 - t1, "what": "one host core, one call each"})
    out = Path(a.out) / f"relaxation_vectors_n{a.n}_reference.json"
    out.write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))
    sys.exit(0)

from pyamg_amd import _capi as capi  # noqa: E402

if capi.device_count() < 1:
    sys.exit("no GPU here: nothing to measure")
lib = capi.lib()
DA = capi.DeviceArray

dAp, dAj, dAx = DA.from_host(A.indptr), DA.from_host(A.indices), DA.from_host(A.data)
mat = C.c_void_p()
t0 = time.perf_counter()
capi.check(lib.pamg_matrix_create(C.byref(mat), capi.F64, capi.CSR, n, n, 1, 1, capi.ptr(A.indptr), capi.ptr(A.indices), capi.ptr(A.data)), "matrix_create")
capi.sync()
rec["single_matrix_create_s"] = time.perf_counter() - t0     # what the single-vector variant needs before its first step (upload and plan)
x0 = np.random.RandomState(1).rand(n * R) - 0.5             # as records: node after node
dX0, dXa, dXb = DA.from_host(x0), DA(n * R, np.float64), DA(n * R, np.float64)
dva, dvb, db = DA(n, np.float64), DA(n, np.float64), DA(n, np.float64)
db.zero()
dDx = DA(nnz, np.float64)


def load_block():
    capi.check(lib.pamg_memcpy_d2d(dXa.ptr, dX0.ptr, n * R * 8, None), "d2d")


def multi():
    capi.check(lib.pamg_dev_relaxation_sweeps_f64(n, R, k, a.omega, dAp.ptr, dAj.ptr, dAx.ptr, dXa.ptr, dXb.ptr, None), "sweeps")


def single(columns=R):
    for _ in range(columns):
        src, dst = dva, dvb
        for _ in range(k):
            capi.check(lib.pamg_matrix_jacobi_step(mat, src.ptr, db.ptr, dst.ptr, a.omega, None), "jacobi_step")
            src, dst = dst, src


def tail():
    capi.check(lib.pamg_dev_distance_measure_f64(capi.DISTANCE["algebraic_p2"], 1, n, nnz, R, 2.0, dAp.ptr, dAj.ptr, dAx.ptr, result.ptr, dDx.ptr, None),
               "measure")


def timed(fn):
    e0, e1 = capi.Event(), capi.Event()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_ms(e1)


# the same bits: column 0 of the block against k single-vector steps on it
result = dXb if k % 2 else dXa
load_block()
multi()
capi.sync()
col0 = result.download()[0::R].copy()
dva.upload(np.ascontiguousarray(x0[0::R]))
single(columns=1)
capi.sync()
one = (dvb if k % 2 else dva).download()
rec["same_bits_column_0"] = bool(np.array_equal(col0, one))
if not rec["same_bits_column_0"]:
    rec["max_abs_difference_column_0"] = float(np.abs(col0 - one).max())

dva.upload(np.ascontiguousarray(x0[0::R]))
load_block(); timed(multi); timed(single)                   # warm-up
tm, ts = [], []
for _ in range(a.runs):                                     # (the iterate keeps relaxing: the time does not depend on the values)
    tm.append(timed(multi))
    ts.append(timed(single))
load_block(); multi(); capi.sync()
timed(tail)
tt = [timed(tail) for _ in range(a.runs)]


def stats(t, nbytes, launches):
    med = statistics.median(t)
    return {"median_ms": med, "min_ms": min(t), "max_ms": max(t), "launches": launches,
            "algorithmic_GBps": nbytes / (med * 1e-3) / 1e9, "share_of_8TBps": nbytes / (med * 1e-3) / PEAK}


# the entry point as a caller sees it: host arrays in, host arrays out (upload of A and of the block, k sweeps, download), twice
from pyamg_amd import amg_core as gcore  # noqa: E402
xh = np.ascontiguousarray(x0.reshape(n, R).T).reshape(-1)   # column after column
rec["layer1_relaxation_vectors_s"] = []
for _ in range(2):
    t0 = time.perf_counter()
    gcore.relaxation_vectors(A.indptr, A.indices, A.data, xh, n, R, k, a.omega)
    rec["layer1_relaxation_vectors_s"].append(time.perf_counter() - t0)
rec["multi"] = stats(tm, k * sweep_bytes, k)
rec["single"] = stats(ts, k * sweep_bytes, R * k)          # against the same bytes: what the task needs, not what this variant moves
rec["tail"] = stats(tt, tail_bytes, 1)
spread = max(max(tm) - min(tm), max(ts) - min(ts))
rec["single_over_multi"] = rec["single"]["median_ms"] / rec["multi"]["median_ms"]
rec["difference_ms"] = rec["single"]["median_ms"] - rec["multi"]["median_ms"]
rec["run_to_run_spread_ms"] = spread
rec["multi_faster_beyond_spread"] = bool(rec["difference_ms"] > spread)
capi.check(lib.pamg_matrix_destroy(mat), "matrix_destroy")
out = Path(a.out)
out.mkdir(parents=True, exist_ok=True)
(out / f"relaxation_vectors_n{a.n}.json").write_text(json.dumps(rec, indent=1) + "\n")
print(json.dumps(rec))
