#!/usr/bin/env python3
"""Wall time of the AIR setup pieces of pyamg_amd.air -- one_point_interpolation and local_air (degree 1 and 2) -- uploads and downloads
included, beside the reference's functions from oracle/_ref (alternating calls, medians and ranges), and of the whole ``air_solver`` setup
with and without ``device_setup(air=True)``.

  shape 1 : the 512^2 upwind convection-diffusion operator of the benchmark's AIR workload (c7a)
  shape 2 : the 64^3 operator of the same family (diffusion added in z)

With a GPU and the reference build on one host both sides alternate in one process, the results are compared array for array and
the whole setup is timed (``same_process``).  A machine that has only one of the two measures that side and completes a record that
already holds the other (--out); the two columns then come from two hosts, no ratio is recorded, and the results are compared
through a digest of their arrays (``same_digest``).  The splitting is PMIS on the
'min' strength (theta 0.3) with a fixed seed -- the device's and the reference's are the same array, so both hosts see the same
input; local_air runs with theta 0.05.

``--hierarchy`` also builds a whole PMIS hierarchy from each side's own functions and times ``local_air`` level by level.

    python tools/microbench_air_setup.py                      # -> profiles/r13_air_setup.json  (--out DIR: somewhere else)

Not product code."""
import argparse
import hashlib
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import scipy.sparse as sp

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--setup-runs", type=int, default=3)
ap.add_argument("--grid2", type=int, nargs=2, default=[512, 512])
ap.add_argument("--grid3", type=int, nargs=3, default=[64, 64, 64])
ap.add_argument("--setup-3d", action="store_true", help="time the whole air_solver setup of shape 2 as well (minutes per run in the reference)")
ap.add_argument("--hierarchy", action="store_true", help="build a PMIS hierarchy step by step on each side and time local_air level by level")
ap.add_argument("--no-setup", action="store_true", help="leave out the whole air_solver setup")
ap.add_argument("--out", default=str(ROOT / "profiles"))
a = ap.parse_args()
OUT = Path(a.out) / "r13_air_setup.json"

from pyamg_amd import _capi as capi  # noqa: E402
import oracle.refimport as ri  # noqa: E402

have_gpu = capi.device_count() > 0
have_ref = ri.available()
if not (have_gpu or have_ref):
    sys.exit("neither a GPU nor oracle/_ref here: nothing to measure")
if have_ref:
    import pyamg
    from pyamg.classical import interpolate as ref_interp
    from pyamg.classical import split as ref_split
    from pyamg.strength import classical_strength_of_connection as ref_strength
if have_gpu:
    from pyamg_amd import air as dev
    from pyamg_amd import classical as dev_cls
    from pyamg_amd.aggregation import device_setup
    capi.lib()


def convdiff(grid, c=3.0):
    mx, my = grid[:2]
    Dx = sp.diags_array([np.ones(mx), -np.ones(mx - 1)], offsets=[0, -1], shape=(mx, mx))
    Dy = sp.diags_array([2 * np.ones(my), -np.ones(my - 1), -np.ones(my - 1)], offsets=[0, -1, 1], shape=(my, my))
    A = sp.csr_array(c * sp.kron(sp.eye_array(my), Dx) + sp.kron(Dy, sp.eye_array(mx)))
    if len(grid) == 3:
        mz = grid[2]
        Dz = sp.diags_array([2 * np.ones(mz), -np.ones(mz - 1), -np.ones(mz - 1)], offsets=[0, -1, 1], shape=(mz, mz))
        A = sp.csr_array(sp.kron(sp.eye_array(mz), A) + sp.kron(Dz, sp.eye_array(mx * my)))
    A.sort_indices()
    return sp.csr_array((A.data, A.indices.astype(np.int32), A.indptr.astype(np.int32)), shape=A.shape)


def same(x, y):
    n = int(x.indptr[-1])
    return bool(np.array_equal(x.indptr, y.indptr) and np.array_equal(x.indices[:n], y.indices[:n]) and np.array_equal(x.data[:n], y.data[:n]))


def digest(x):
    """of the arrays a result holds: what two hosts compare where they cannot compare the arrays"""
    n = int(x.indptr[-1])
    h = hashlib.sha256()
    for arr in (x.indptr.astype(np.int64), x.indices[:n].astype(np.int64), np.ascontiguousarray(x.data[:n], dtype=np.float64)):
        h.update(arr.tobytes())
    return h.hexdigest()[:16]


def stats(t):
    return {"seconds": [round(x, 5) for x in t], "median_s": round(statistics.median(t), 5), "range_s": [round(min(t), 5), round(max(t), 5)]}


def alternate(fns, runs):
    """{side: callable} -> ({side: times}, {side: last result}); one untimed call each first (library load, code objects, caches)"""
    times, last = {s: [] for s in fns}, {}
    for fn in fns.values():
        fn()
    for _ in range(runs):
        for s, fn in fns.items():
            t0 = time.perf_counter()
            last[s] = fn()
            times[s].append(time.perf_counter() - t0)
    return times, last


def hierarchy(A, side):
    """the steps of air_solver (CF='PMIS', its other defaults) one by one on one side, each level's local_air timed: where the setup
    time goes below the finest level, where the neighbourhoods grow.  Both sides build the same arrays."""
    if side == "device":
        from pyamg_amd.aggregation import galerkin_product
        strength, pmis, one_point, lair = dev_cls.classical_strength_of_connection, dev_cls.PMIS, dev.one_point_interpolation, dev.local_air
    else:
        strength, pmis, one_point, lair = ref_strength, ref_split.PMIS, ref_interp.one_point_interpolation, ref_interp.local_air
        galerkin_product = lambda R, A, P: R @ A @ P      # noqa: E731
    np.random.seed(11)
    levels, t_all = [], time.perf_counter()
    while A.shape[0] > 20 and len(levels) < 19:
        C = strength(A, theta=0.3, norm="min")
        splitting = np.asarray(pmis(C), dtype=np.int32)
        P = one_point(A, C, splitting)
        t0 = time.perf_counter()
        R = lair(A, splitting, theta=0.05, degree=2)
        dt = time.perf_counter() - t0
        N = np.diff(R.indptr) - 1
        levels.append({"rows": int(A.shape[0]), "nnz": int(A.nnz), "coarse": int(R.shape[0]), "local_air_s": round(dt, 5),
                       "stored_per_row_median": float(np.median(N)) if N.size else 0.0, "stored_per_row_max": int(N.max()) if N.size else 0,
                       "rows_beyond_64": int(np.sum(N > 64)), "sha256_16": digest(R)})
        A = sp.csr_array(galerkin_product(R, A, P))
        A = sp.csr_array((A.data, A.indices.astype(np.int32), A.indptr.astype(np.int32)), shape=A.shape)
    return {"levels": levels, "local_air_s": round(sum(lv["local_air_s"] for lv in levels), 5), "all_steps_s": round(time.perf_counter() - t_all, 5)}


res = json.loads(OUT.read_text()) if OUT.exists() else {}
res.setdefault("what", "wall seconds, uploads and downloads included; medians of alternating runs")
if not isinstance(res.get("runs"), dict):
    res["runs"] = {}
for side, ok in (("device", have_gpu), ("reference", have_ref)):
    if ok:
        res["runs"][side] = {"functions": a.runs, "setup": a.setup_runs}
res.setdefault("shapes", {})
for label, grid in (("convdiff_%dx%d" % tuple(a.grid2), tuple(a.grid2)), ("convdiff_%dx%dx%d" % tuple(a.grid3), tuple(a.grid3))):
    A = convdiff(grid)
    C = (dev_cls.classical_strength_of_connection if have_gpu else ref_strength)(A, theta=0.3, norm="min")
    np.random.seed(12)
    splitting = np.asarray((dev_cls.PMIS if have_gpu else ref_split.PMIS)(C), dtype=np.int32)
    shape = res["shapes"].setdefault(label, {})
    shape.update(rows=int(A.shape[0]), nnz=int(A.nnz), coarse=int(splitting.sum()))
    cases = {"one_point_interpolation": lambda m: m.one_point_interpolation(A, C, splitting),
             "local_air_degree1": lambda m: m.local_air(A, splitting, theta=0.05, degree=1),
             "local_air_degree2": lambda m: m.local_air(A, splitting, theta=0.05, degree=2)}
    for fname, call in cases.items():
        fns = {}
        if have_gpu:
            fns["device"] = lambda: call(dev)
        if have_ref:
            fns["reference"] = lambda: call(ref_interp)
        times, last = alternate(fns, a.runs)
        row = shape.setdefault(fname, {})
        for s, t in times.items():
            row[s] = dict(stats(t), sha256_16=digest(last[s]))
        row["same_process"] = len(fns) == 2
        if "device" in row and "reference" in row:
            row["same_digest"] = row["device"]["sha256_16"] == row["reference"]["sha256_16"]
        if len(fns) == 2:
            row["same_arrays"] = same(last["device"], last["reference"])
            row["speedup_of_medians"] = round(row["reference"]["median_s"] / row["device"]["median_s"], 2)
        else:
            row.pop("same_arrays", None)
            row.pop("speedup_of_medians", None)
        if fname.startswith("local_air"):
            N = np.diff(next(iter(last.values())).indptr) - 1    # (after eliminate_zeros: a lower bound of the neighbourhood sizes)
            row["stored_per_row"] = {"median": float(np.median(N)), "max": int(N.max())}
        print(json.dumps({label: {fname: {s: row[s]["median_s"] for s in times}}}), flush=True)
    if a.hierarchy:
        row = shape.setdefault("hierarchy_pmis", {})
        for side, ok in (("device", have_gpu), ("reference", have_ref and (len(grid) == 2 or a.setup_3d))):
            if ok:
                if side == "device":
                    hierarchy(A, side)                       # first contact
                row[side] = hierarchy(A, side)
                print(json.dumps({label: {"hierarchy_pmis": {side: {k: v for k, v in row[side].items() if k != "levels"}}}}), flush=True)
        if "device" in row and "reference" in row:
            row["same_digests"] = [lv["sha256_16"] for lv in row["device"]["levels"]] == [lv["sha256_16"] for lv in row["reference"]["levels"]]
    if not have_ref or (len(grid) == 3 and not a.setup_3d) or a.no_setup:
        continue                                             # the whole setup runs inside the reference package

    inside = {"one_point_interpolation": [], "local_air": []}    # seconds per unpatched setup inside the two functions, all levels

    def setup(patched):
        np.random.seed(11)
        if patched:
            with device_setup(pyamg, air=True):
                return pyamg.air_solver(A, max_coarse=20)
        import pyamg.classical.air as ref_air
        spent, saved = dict.fromkeys(inside, 0.0), {}
        for name in inside:
            def timed(*args, _fn=getattr(ref_air, name), _name=name, **kw):
                t0 = time.perf_counter()
                try:
                    return _fn(*args, **kw)
                finally:
                    spent[_name] += time.perf_counter() - t0
            saved[name] = getattr(ref_air, name)
            setattr(ref_air, name, timed)
        try:
            return pyamg.air_solver(A, max_coarse=20)
        finally:
            for name, fn in saved.items():
                setattr(ref_air, name, fn)
                inside[name].append(spent[name])

    fns = {"reference": lambda: setup(False)}
    if have_gpu:
        fns["device_setup_air"] = lambda: setup(True)
    times, last = alternate(fns, a.setup_runs)
    row = shape.setdefault("air_solver_setup", {})
    for s, t in times.items():
        row[s] = stats(t)
    w = last["reference"]
    row["levels"] = len(w.levels)
    if have_gpu:
        g = last["device_setup_air"]
        row["same_arrays"] = len(g.levels) == len(w.levels) and all(
            same(sp.csr_array(getattr(lg, nm)), sp.csr_array(getattr(lw, nm))) for lg, lw in zip(g.levels, w.levels) for nm in ("A", "P", "R")
            if hasattr(lw, nm))
        row["speedup_of_medians"] = round(row["reference"]["median_s"] / row["device_setup_air"]["median_s"], 2)
    # the share of the two functions in the reference's setup, all levels (the first, untimed run left out)
    for name, spent in inside.items():
        row[f"reference_seconds_inside_{name}"] = round(statistics.median(spent[1:]), 5)
        row[f"reference_share_of_{name}"] = round(statistics.median(spent[1:]) / row["reference"]["median_s"], 4)
    print(json.dumps({label: {"air_solver_setup": {s: row[s]["median_s"] for s in times}}}), flush=True)
if not (have_gpu and have_ref):
    res["note"] = ("device column: one process on an MI355X machine; reference column: one process on a machine without a GPU (the reference "
                   "build does not exist on the GPU machine). Different hosts: same_process is false, no ratio is recorded, and the whole "
                   "air_solver setup under device_setup(air=True) is not measured.")
else:
    res.pop("note", None)
OUT.parent.mkdir(exist_ok=True)
OUT.write_text(json.dumps(res, indent=1))
