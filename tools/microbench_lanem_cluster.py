#!/usr/bin/env python3
"""The CLUSTER layout of the merged lane sweep (tune key 38) on one level of the SA hierarchy of 3-D Poisson: fused symmetric launch and forward
sweep time by rows per wave R (1 = the pair / row layout) x merge depth s (key 33) x workgroups (key 26), with the planner's statistics of every
variant (profiles/r08_microbench_lanem_cluster_scan_level1.json).  Not product code."""
import argparse, json, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import oracle.refimport  # noqa: F401
import pyamg
from pyamg_amd import _capi as capi
from pyamg_amd.aggregation import device_setup
from pyamg_amd.hierarchy import extract
from pyamg_amd.multilevel import DeviceMatrix

ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, nargs="+", default=[256, 256, 256])
ap.add_argument("--R", type=int, nargs="+", default=[1, 4, 8])
ap.add_argument("--s", type=int, nargs="+", default=[3, 4, 5])
ap.add_argument("--grids", type=int, nargs="+", default=[0, 512, 768])
ap.add_argument("--level", type=int, default=1)
ap.add_argument("--out", default=None, help="write the record here as JSON (every variant is printed as a line in any case)")
a = ap.parse_args()
A = pyamg.gallery.poisson(tuple(a.grid), format="csr")
np.random.seed(1)
t = time.time()
with device_setup(pyamg):
    ml = pyamg.smoothed_aggregation_solver(A, max_coarse=10)
print(f"setup {time.time() - t:.1f}s", flush=True)
spec = extract(ml)
outp = Path(a.out) if a.out else None
if outp:
    outp.parent.mkdir(parents=True, exist_ok=True)


def timeit(fn, reps=10):
    fn(); fn(); capi.sync()
    e0, e1 = capi.Event(), capi.Event()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_ms(e1) / reps


op = spec.levels[a.level].A
n = op.shape[0]
rng = np.random.RandomState(1)
x0, b = rng.rand(n), rng.rand(n)
dx, db = capi.DeviceArray.from_host(x0), capi.DeviceArray.from_host(b)
out = {"rows": int(n), "nnz": int(op.nnz), "variants": []}
ref = None
for s in a.s:
    for R in a.R:
        dA = DeviceMatrix(op)
        dA.tune(gs_order=1, lane_wide=1, lane_merge=s, lanem_cluster=R, sym_fused=1)
        t0 = time.time()
        dx.upload(x0)
        dA.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=1, x_is_zero=False)
        got = dx.download()
        tb = time.time() - t0
        if ref is None:
            ref = got
        err = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
        for G in a.grids:
            dA.tune(lane_G=G)
            ms = timeit(lambda: dA.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=1, x_is_zero=False))
            msf = timeit(lambda: dA.gauss_seidel(dx, db, sweep="forward"))
            mi = dA.lanem_info(0)
            ops = mi["early_operands"] + mi["old_operands"] + mi["b_operands"]
            v = {"s": s, "R": R, "lane_G": G, "ms_symmetric_fused": round(ms, 4), "ms_forward_with_prepare": round(msf, 4), "grid": dA.sym_info()["launch_grid"],
                 "rel_diff_vs_first": err, "groups": mi["groups"], "super_levels": mi["super_levels"], "operands_per_row": round(ops / n, 2),
                 "unique_early_old_b_per_row": [round(mi[k] / n, 2) for k in ("unique_early", "unique_old", "unique_b")], "early_lines_per_row": round(mi["early_lines"] / n, 2),
                 "padding": round(mi["padding"], 3), "build_and_first_sweep_s": round(tb, 2), "timeout": bool(dA.flow_error()), "sym": dA.sym_info()["form"]}
            out["variants"].append(v)
            print(json.dumps(v), flush=True)
            if outp:
                outp.write_text(json.dumps(out, indent=1))
            if v["timeout"]:
                print("flow error: stopping", flush=True)
                sys.exit(3)
        dA.free()
print("done")
