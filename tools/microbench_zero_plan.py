#!/usr/bin/env python3
"""The zero-iterate plans (tune key 39) on one level of the SA hierarchy of 3-D Poisson: time of the fused symmetric launch announced to start from
x = 0 by merge depth of the plans (key 40) x workgroups (key 26), against the same launch on the general plans (key 39 = 1), with the planner's
statistics of every variant (profiles/r09_microbench_zero_plan_scan_level*.json).  The timed launches follow one another without x being put back
to zero: the kernels' work does not depend on the data.  Not product code."""
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
ap.add_argument("--level", type=int, nargs="+", default=[1])
ap.add_argument("--s", type=int, nargs="+", default=[4, 5, 6, 8], help="merge depths of the zero-iterate plans; the same list for every level unless --s2 is given")
ap.add_argument("--s2", type=int, nargs="+", default=None, help="merge depths for the levels after the first one of --level")
ap.add_argument("--grids", type=int, nargs="+", default=[0, 512, 768])
ap.add_argument("--grids2", type=int, nargs="+", default=[0])
ap.add_argument("--reps", type=int, default=3, help="timed repetitions of 10 launches each: the spread is reported")
ap.add_argument("--out", default=None)
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


out = {"grid": a.grid, "levels": []}
for li, level in enumerate(a.level):
    op = spec.levels[level].A
    n = op.shape[0]
    b = np.random.RandomState(1).rand(n)
    z = np.zeros(n)
    dx, db = capi.DeviceArray.from_host(z), capi.DeviceArray.from_host(b)
    rec = {"level": level, "rows": int(n), "nnz": int(op.nnz), "variants": []}
    out["levels"].append(rec)
    depths = a.s if (li == 0 or a.s2 is None) else a.s2
    grids = a.grids if li == 0 else a.grids2
    ref = None
    for s in [0] + list(depths):                       # 0: the general plans (zero-iterate plans off)
        dA = DeviceMatrix(op)
        dA.tune(gs_order=1, lane_wide=1, sym_fused=1, zero_plans=2 if s else 1, **({"zero_merge": s} if s else {}))
        t0 = time.time()
        dx.upload(z)
        dA.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=1, x_is_zero=True)
        got = dx.download()
        tb = time.time() - t0
        if ref is None:
            ref = got
        err = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
        for G in grids:
            dA.tune(lane_G=G)
            ms = [timeit(lambda: dA.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=1, x_is_zero=True)) for _ in range(a.reps)]
            sym = dA.sym_info()
            mi = [dA.lanem_info(w) for w in ((4, 5) if s else (0, 1))]
            ops = [m["early_operands"] + m["old_operands"] + m["b_operands"] for m in mi]
            v = {"zero_merge": s, "plans": "zero-iterate" if s else "general", "lane_G": G, "ms_fused_from_zero": [round(x, 4) for x in ms],
                 "grid": mi[0]["launch_grid"] if s else sym["launch_grid"], "zero_plan_launches": sym["zero_plan_launches"], "rel_diff_vs_general": err,
                 "s_max": mi[0]["s_max"], "super_levels": [m["super_levels"] for m in mi], "groups": [m["groups"] for m in mi],
                 "operands_per_row": [round(o / n, 2) for o in ops],
                 "unique_per_row": [round((m["unique_early"] + m["unique_old"] + m["unique_b"]) / n, 2) for m in mi],
                 "closed_by_length": [m["closed_by_length"] for m in mi], "longest_row": [m["longest_row"] for m in mi],
                 "hbm_bytes": dA.info()["hbm_bytes"], "build_and_first_sweep_s": round(tb, 2), "timeout": bool(dA.flow_error()), "sym": sym["form"]}
            rec["variants"].append(v)
            print(json.dumps(v), flush=True)
            if outp:
                outp.write_text(json.dumps(out, indent=1))
            if v["timeout"]:
                print("flow error: stopping", flush=True)
                sys.exit(3)
        dA.free()
print("done")
