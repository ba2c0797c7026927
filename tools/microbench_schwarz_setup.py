#!/usr/bin/env python3
"""Wall time of the Schwarz setup: relaxation.schwarz_parameters(device=True) -- upload of the operator and the subdomain lists, the
plan / extract / pinv kernels, download of the blocks -- against device=False (the host loops: one searchsorted per row, one LAPACK
gelss call per subdomain; the same code as before the device option existed), in one process, five alternating runs each, medians.

  shape 1 : the fine level of the c8s workload: 384^2 5-point Poisson, one subdomain per row (its pattern)
  shape 2 : level 1 of a smoothed-aggregation hierarchy of the 64^3 7-point Poisson operator built by the reference (when oracle/_ref
            travelled), one subdomain per row: about 30 entries per row

    python tools/microbench_schwarz_setup.py                      # -> profiles/r11_schwarz_setup.json  (--out DIR: somewhere else)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/prof -- python tools/microbench_schwarz_setup.py --once --out DIR
    python tools/microbench_schwarz_setup.py --out DIR --kernel-stats DIR/prof/.../*_kernel_stats.csv     # folds the kernels' share in
    python tools/microbench_schwarz_setup.py --out DIR --kernel-stats CSV --fold-only                      # the same on an existing record, no GPU

Not product code."""
import argparse
import csv
import json
import re
import statistics
import sys
import time
import warnings
from pathlib import Path

import numpy as np
import scipy.sparse as sp

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--once", action="store_true", help="one device run per shape (for a profiler around this process)")
ap.add_argument("--kernel-stats", default=None, help="kernel stats CSV of a profiled --once run")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--fine", type=int, nargs=2, default=[384, 384])
ap.add_argument("--sa", type=int, nargs=3, default=[64, 64, 64])
ap.add_argument("--level1", default=None, help="level 1 of the SA hierarchy as a scipy .npz (for a box without oracle/_ref)")
ap.add_argument("--out", default=str(ROOT / "profiles"), help="directory of r11_schwarz_setup.json (and of the --once record)")
ap.add_argument("--fold-only", action="store_true", help="add the kernel trace of --kernel-stats to the existing record, measure nothing")
a = ap.parse_args()
OUT = Path(a.out)
OUT.mkdir(exist_ok=True)


def fold_kernel_trace(res):
    """the profiled --once process ran every shape twice (first contact + the timed run): the kernels' share of the device wall time"""
    once = json.loads((OUT / "schwarz_setup_once.json").read_text())
    ks = {}
    with open(a.kernel_stats, newline="") as f:
        for r in csv.DictReader(f):
            hit = re.search(r"schwarz_\w+(<[^>]*>)?", r.get("Name") or r.get("KernelName") or "")
            if hit:
                k = ks.setdefault(hit.group(0), {"calls": 0, "total_ns": 0})
                k["calls"] += int(r.get("Calls", 0))
                k["total_ns"] += int(float(r.get("TotalDurationNs", 0)))
    kernel_s = sum(v["total_ns"] for v in ks.values()) * 1e-9
    wall = 2 * sum(s["device_s"] for s in once["shapes"].values())        # (both runs of every shape are in the trace)
    res["kernel_trace"] = {"kernels": ks, "kernel_seconds_all_runs": round(kernel_s, 5), "device_wall_seconds_all_runs_approx": round(wall, 4),
                           "kernel_share_of_wall": round(kernel_s / wall, 3) if wall else None,
                           "note": "one rocprofv3 --kernel-trace --stats run of --once; wall = 2 x the timed run of every shape (under the profiler)"}


if a.fold_only:
    res = json.loads((OUT / "r11_schwarz_setup.json").read_text())
    fold_kernel_trace(res)
    (OUT / "r11_schwarz_setup.json").write_text(json.dumps(res, indent=1))
    sys.exit(0)

from pyamg_amd import _capi as capi  # noqa: E402
from pyamg_amd import relaxation as grelax  # noqa: E402
from tools.problems import poisson_csr  # noqa: E402


def shapes():
    A = sp.csr_array(poisson_csr(tuple(a.fine))).astype(np.float64)
    A.sort_indices()
    yield "fine_%dx%d_5pt" % tuple(a.fine), A
    import oracle.refimport as ri
    if a.level1:
        A1 = sp.csr_array(sp.load_npz(a.level1)).astype(np.float64)           # the same operator, built where the reference is
        A1.sort_indices()
        yield "sa_%dx%dx%d_level1" % tuple(a.sa), A1
    elif ri.available():
        import pyamg
        np.random.seed(7)
        ml = pyamg.smoothed_aggregation_solver(pyamg.gallery.poisson(tuple(a.sa), format="csr"), max_levels=2, max_coarse=10)
        A1 = sp.csr_array(ml.levels[1].A.tocsr()).astype(np.float64)
        A1.sort_indices()
        yield "sa_%dx%dx%d_level1" % tuple(a.sa), A1


def fresh(A):
    return sp.csr_array((A.data, A.indices, A.indptr), shape=A.shape)       # no cached schwarz_parameters on it


def timed(A, device):
    B = fresh(A)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        t0 = time.perf_counter()
        out = grelax.schwarz_parameters(B, device=device)
        t = time.perf_counter() - t0
    return t, out, getattr(B, "schwarz_setup_report", None)


capi.lib()
res = {"what": "wall seconds of relaxation.schwarz_parameters, device=True (upload + kernels + download) vs device=False (host loops), "
               "medians of alternating runs in one process", "runs": a.runs, "shapes": {}}
for name, A in shapes():
    m = np.diff(A.indptr)
    row = {"rows": int(A.shape[0]), "nnz": int(A.nnz), "largest_subdomain": int(m.max()), "mean_subdomain": round(float(m.mean()), 1),
           "block_entries": int(np.sum(m.astype(np.int64) ** 2))}
    timed(A, True)                                       # first contact: library load, code objects
    if a.once:
        t, _, rep = timed(A, True)
        row.update(device_s=round(t, 4), report=rep)
    else:
        td, th = [], []
        for _ in range(a.runs):
            t, dev, rep = timed(A, True)
            td.append(t)
            t, host, _ = timed(A, False)
            th.append(t)
        d = np.abs(dev[2] - host[2])
        row.update(device_s=[round(t, 4) for t in td], host_s=[round(t, 3) for t in th], device_median_s=round(statistics.median(td), 4),
                   host_median_s=round(statistics.median(th), 3), speedup_of_medians=round(statistics.median(th) / statistics.median(td), 1),
                   ranges_s={"device": [round(min(td), 4), round(max(td), 4)], "host": [round(min(th), 3), round(max(th), 3)]},
                   report=rep, max_abs_difference_to_host_blocks=float(d.max()), max_abs_host_block_entry=float(np.abs(host[2]).max()))
    res["shapes"][name] = row
    print(json.dumps({name: row}), flush=True)

if a.once:
    (OUT / "schwarz_setup_once.json").write_text(json.dumps(res, indent=1))
    sys.exit(0)

if a.kernel_stats and Path(a.kernel_stats).exists() and (OUT / "schwarz_setup_once.json").exists():
    fold_kernel_trace(res)
(OUT / "r11_schwarz_setup.json").write_text(json.dumps(res, indent=1))
