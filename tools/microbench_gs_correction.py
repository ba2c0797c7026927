#!/usr/bin/env python3
"""The correction form of a symmetric Gauss-Seidel step from x != 0 (tune key 41) on single levels of the SA hierarchy of 3-D Poisson: the fused launch
on the general plans against residual + the accumulating launch on the zero-iterate plans (pamg_matrix_gauss_seidel_correction), same session, --reps
repetitions of 10 steps each; also the two parts alone -- the residual launch and the launch announced from zero -- so that the cost of the accumulating
instantiation over the plain one shows (profiles/r10_microbench_gs_correction_scan.json).  The automatic rule of key 41 (GS_CORRECTION_MIN_ROWS,
csrc/pamg_common.h) sits between the largest level that loses and the smallest that wins by more than the spread of the repetitions.  The timed steps
follow one another on the same x: the kernels' work does not depend on the data.  Not product code."""
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
ap.add_argument("--level", type=int, nargs="+", default=[1, 2, 3])
ap.add_argument("--reps", type=int, default=3, help="timed repetitions of 10 steps each: the spread is reported")
ap.add_argument("--fused", type=int, nargs="+", default=[1], help="tune key 37: 1 = one launch per symmetric sweep, 0 = two")
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


def spread(ms):
    return (max(ms) - min(ms)) / min(ms)


out = {"grid": a.grid, "reps": a.reps, "steps_per_rep": 10, "levels": []}
for level in a.level:
    if level >= len(spec.levels) - 1:
        continue
    op = spec.levels[level].A
    n = op.shape[0]
    rs = np.random.RandomState(1)
    x, b = rs.rand(n), rs.rand(n)
    dx, db, dr = capi.DeviceArray.from_host(x), capi.DeviceArray.from_host(b), capi.DeviceArray.from_host(np.zeros(n))
    for fused in a.fused:
        dA = DeviceMatrix(op)
        dA.tune(gs_order=1, lane_wide=1, sym_fused=fused, zero_plans=2)
        t0 = time.time()
        dx.upload(x)
        dA.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=1, x_is_zero=False)
        ref = dx.download()
        dx.upload(x)
        dA.gauss_seidel_correction(dx, db, dr)
        got = dx.download()
        tb = time.time() - t0
        err = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
        ms = {"general": [], "correction": [], "residual_alone": [], "from_zero_alone": []}
        for _ in range(a.reps):                         # interleaved: a drift of the session hits every variant alike
            ms["general"].append(timeit(lambda: dA.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=1, x_is_zero=False)))
            ms["correction"].append(timeit(lambda: dA.gauss_seidel_correction(dx, db, dr)))
            ms["residual_alone"].append(timeit(lambda: dA.spmv(2, dx, dr, b=db)))
            ms["from_zero_alone"].append(timeit(lambda: dA.gauss_seidel_x0(dx, dr, sweep="symmetric", iterations=1, x_is_zero=True)))
        sym = dA.sym_info()
        g, c = min(ms["general"]), min(ms["correction"])
        v = {"level": level, "rows": int(n), "nnz": int(op.nnz), "sym_fused": fused, "form": sym["form"],
             "ms_general": [round(v_, 4) for v_ in ms["general"]], "ms_residual_plus_accumulating_zero_launch": [round(v_, 4) for v_ in ms["correction"]],
             "ms_residual_alone": [round(v_, 4) for v_ in ms["residual_alone"]], "ms_plain_zero_launch_alone": [round(v_, 4) for v_ in ms["from_zero_alone"]],
             "gain_pct_best_of_reps": round(100 * (g - c) / g, 2), "spread_pct": {k: round(100 * spread(v_), 2) for k, v_ in ms.items()},
             "accumulating_over_plain_plus_residual_pct": round(100 * (c - min(ms["residual_alone"]) - min(ms["from_zero_alone"])) / c, 2),
             "grid_general": sym["launch_grid"], "grid_zero": dA.lanem_info(4)["launch_grid"], "correction_launches": sym["correction_launches"],
             "rel_diff_correction_vs_general": err, "build_and_first_sweeps_s": round(tb, 2), "timeout": bool(dA.flow_error())}
        out["levels"].append(v)
        print(json.dumps(v), flush=True)
        if outp:
            outp.write_text(json.dumps(out, indent=1))
        if v["timeout"]:
            print("flow error: stopping", flush=True)
            sys.exit(3)
        dA.free()
print("done")
