#!/usr/bin/env python3
"""Wall time of pyamg_amd.graph.lloyd_aggregation on the strength pattern of two operators, uploads and downloads included, against the
reference's function from oracle/_ref where that is present: five alternating runs in one process, median and range, with the Lloyd
iterations and the distance and stamp rounds the device ran beside the times.

  shape 1 : 256^2 5-point Laplacian            shape 2 : 64^3 27-point operator (-1 off the diagonal, 26 on it)

The side that is missing on a machine is skipped, and a record that already holds the other side (--out) is completed.  Only when both
sides ran in one process does the record say so (``same_process``) and are the arrays compared; otherwise the two columns come from two
machines and no ratio is recorded.

    python tools/microbench_lloyd_setup.py                          # -> profiles/r20_lloyd_setup.json  (--out DIR: somewhere else)

Not product code."""
import argparse
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
ap.add_argument("--grid2", type=int, nargs=2, default=[256, 256])
ap.add_argument("--grid3", type=int, nargs=3, default=[64, 64, 64])
ap.add_argument("--seed", type=int, default=20261021)
ap.add_argument("--out", default=str(ROOT / "profiles"))
a = ap.parse_args()
OUT = Path(a.out) / "r20_lloyd_setup.json"

from pyamg_amd import _capi as capi  # noqa: E402
from tools.problems import poisson_csr  # noqa: E402
import oracle.refimport as ri  # noqa: E402

have_gpu = capi.device_count() > 0
have_ref = ri.available()
if not (have_gpu or have_ref):
    sys.exit("neither a GPU nor oracle/_ref here: nothing to measure")
if have_gpu:
    from pyamg_amd import graph as dev
    from pyamg_amd.aggregation import symmetric_strength_of_connection as dev_strength
    capi.lib()
if have_ref:
    from pyamg.aggregation.aggregate import lloyd_aggregation as ref_lloyd_aggregation
    from pyamg.strength import symmetric_strength_of_connection as ref_strength


def box27(nx, ny, nz):
    def band(n):
        return sp.diags_array([np.ones(n - 1), np.ones(n), np.ones(n - 1)], offsets=[-1, 0, 1], format="csr")
    A = sp.csr_array(-sp.kron(sp.kron(band(nx), band(ny)), band(nz), format="csr"))
    A = sp.csr_array(A + sp.diags_array(np.full(A.shape[0], 27.0)))
    A.sort_indices()
    return sp.csr_array((A.data, A.indices.astype(np.int32), A.indptr.astype(np.int32)), shape=A.shape)


res = json.loads(OUT.read_text()) if OUT.exists() else {}
res.setdefault("what", "wall seconds of lloyd_aggregation(C) (ratio 0.1, measure 'unit', maxiter 5) from one seed, C the symmetric strength "
                       "pattern (theta 0), uploads and downloads included; median and range of alternating runs; info = (Lloyd iterations, "
                       "distance rounds, stamp rounds, centres moved in the last iteration) of the device run")
res["runs"] = a.runs
res.setdefault("shapes", {})
for label, A in (("grid_%dx%d_5pt" % tuple(a.grid2), sp.csr_array(poisson_csr(tuple(a.grid2))).astype(np.float64)),
                 ("box_%dx%dx%d_27pt" % tuple(a.grid3), box27(*a.grid3))):
    A.sort_indices()
    A = sp.csr_array((A.data, A.indices.astype(np.int32), A.indptr.astype(np.int32)), shape=A.shape)
    C = sp.csr_array((dev_strength if have_gpu else ref_strength)(A, theta=0.0))
    shape = res["shapes"].setdefault(label, {})
    shape.update(rows=int(A.shape[0]), nnz=int(A.nnz), strong_entries=int(C.nnz))
    info = []
    fns = {}
    if have_gpu:
        fns["device"] = lambda S: dev.lloyd_aggregation(S, info=info)
    if have_ref:
        fns["reference"] = ref_lloyd_aggregation
    times, last = {s: [] for s in fns}, {}
    for s, fn in fns.items():
        np.random.seed(a.seed)
        fn(C)                                                 # first contact: library load, code objects, caches
    for _ in range(a.runs):
        for s, fn in fns.items():                             # alternating
            np.random.seed(a.seed)
            t0 = time.perf_counter()
            last[s] = fn(C)
            times[s].append(time.perf_counter() - t0)
    row = shape.setdefault("lloyd_aggregation", {})
    for s, t in times.items():
        row[s] = {"seconds": [round(x, 5) for x in t], "median_s": round(statistics.median(t), 5),
                  "range_s": [round(min(t), 5), round(max(t), 5)], "aggregates": int(last[s][0].shape[1])}
    if have_gpu:
        row["device"].update(zip(("lloyd_iterations", "distance_rounds", "stamp_rounds", "centres_moved_last"), info[-1]))
    row["same_process"] = len(fns) == 2
    if len(fns) == 2:
        (Ad, cd), (Ar, cr) = last["device"], last["reference"]
        row["same_arrays"] = bool(np.array_equal(Ad.indptr, Ar.indptr) and np.array_equal(Ad.indices, Ar.indices) and
                                  np.array_equal(Ad.data, Ar.data) and np.array_equal(cd, cr))
        row["reference_over_device"] = round(row["reference"]["median_s"] / row["device"]["median_s"], 2)
    else:
        row.pop("same_arrays", None)
        row.pop("reference_over_device", None)
    print(json.dumps({label: row}), flush=True)
if not (have_gpu and have_ref):
    res["note"] = ("device column: one process on an MI355X machine; reference column: one process on a machine without a GPU. Different "
                   "hosts: same_process is false and no ratio is recorded.")
else:
    res.pop("note", None)
OUT.parent.mkdir(exist_ok=True)
OUT.write_text(json.dumps(res, indent=1))
