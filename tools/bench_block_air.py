#!/usr/bin/env python3
"""Wall time of the block (BSR) AIR setup pieces of pyamg_amd.block_air -- the block strength of connection and local_air (degree 1 and
2) -- uploads and downloads included, beside the reference's functions from oracle/_ref on one core (alternating calls, medians and
ranges).

The operator is the perturbed-kron family of the tests: the upwind convection-diffusion stencil on a g x g grid with every stored entry
a_ij replaced by a dense b x b block a_ij * (I or I / 2 plus a perturbation).  The splitting is every node whose two grid coordinates are
even (the same array on every host, no random draw; F-F connections remain for degree 2); local_air runs with theta 0.05.

With a GPU and the reference build on one host both sides alternate in one process and the results are compared array for array
(``same_process``).  A machine that has only one of the two measures that side and completes a record that already holds the other
(--out); the two columns then come from two hosts, no ratio is recorded, and the results are compared through a digest of their arrays
(``same_digest``).

    python tools/bench_block_air.py --b 2 4 --grid 512        # -> profiles/block_air_setup.json  (--out DIR: somewhere else)

Not product code, and not bench.py's workload."""
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
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--b", type=int, nargs="+", default=[2, 4])
ap.add_argument("--grid", type=int, default=512)
ap.add_argument("--out", default=str(ROOT / "profiles"))
a = ap.parse_args()
OUT = Path(a.out) / "block_air_setup.json"

from pyamg_amd import _capi as capi  # noqa: E402
import oracle.refimport as ri  # noqa: E402

have_gpu = capi.device_count() > 0
have_ref = ri.available()
if not (have_gpu or have_ref):
    sys.exit("neither a GPU nor oracle/_ref here: nothing to measure")
sides = {}
if have_gpu:
    from pyamg_amd import block_air as dev
    capi.lib()
    sides["device"] = (dev.classical_strength_of_connection, dev.local_air)
if have_ref:
    from pyamg.classical import interpolate as ref_interp
    from pyamg.strength import classical_strength_of_connection as ref_strength
    sides["reference"] = (ref_strength, ref_interp.local_air)


def operator(g, b, seed=5):
    Dx = sp.diags_array([np.ones(g), -np.ones(g - 1)], offsets=[0, -1], shape=(g, g))
    Dy = sp.diags_array([2 * np.ones(g), -np.ones(g - 1), -np.ones(g - 1)], offsets=[0, -1, 1], shape=(g, g))
    A0 = sp.csr_array(3.0 * sp.kron(sp.eye_array(g), Dx) + sp.kron(Dy, sp.eye_array(g)))
    A0.sort_indices()
    rng = np.random.RandomState(seed)
    rows = np.repeat(np.arange(A0.shape[0]), np.diff(A0.indptr))
    base = np.where(rows == A0.indices, 1.0, 0.5)[:, None, None] * np.eye(b)[None]
    data = A0.data[:, None, None] * (base + rng.randint(0, 3, size=(A0.nnz, b, b)) / 32.0)
    n = A0.shape[0]
    return sp.bsr_array((data, A0.indices.astype(np.int32), A0.indptr.astype(np.int32)), blocksize=(b, b), shape=(n * b, n * b))


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
    return {"median_s": round(statistics.median(t), 5), "range_s": [round(min(t), 5), round(max(t), 5)]}


def alternate(fns, runs):
    times, last = {s: [] for s in fns}, {}
    for fn in fns.values():
        fn()                                                 # first contact: library load, code objects, caches
    for _ in range(runs):
        for s, fn in fns.items():
            t0 = time.perf_counter()
            last[s] = fn()
            times[s].append(time.perf_counter() - t0)
    return times, last


res = json.loads(OUT.read_text()) if OUT.exists() else {}
res["what"] = "wall seconds, uploads and downloads included; medians of alternating runs; the reference on one core"
res.setdefault("runs", {}).update({s: a.runs for s in sides})
res.setdefault("shapes", {})
g = a.grid
for b in a.b:
    A = operator(g, b)
    ij = np.arange(g * g)
    splitting = (((ij % g) % 2 == 0) & ((ij // g) % 2 == 0)).astype(np.int32)
    shape = res["shapes"].setdefault(f"ck_b{b}_{g}x{g}", {})
    shape.update(block_rows=g * g, blocks=int(A.indices.size), coarse=int(splitting.sum()))
    cases = {"block_strength_min": lambda s: sides[s][0](A, theta=0.3, block=True, norm="min"),
             "block_strength_fro": lambda s: sides[s][0](A, theta=0.3, block=True, norm="fro"),
             "local_air_degree1": lambda s: sides[s][1](A, splitting, theta=0.05, degree=1),
             "local_air_degree2": lambda s: sides[s][1](A, splitting, theta=0.05, degree=2)}
    for name, call in cases.items():
        times, last = alternate({s: (lambda s=s: call(s)) for s in sides}, a.runs)
        row = shape.setdefault(name, {})
        for s, t in times.items():
            row[s] = dict(stats(t), sha256_16=digest(last[s]))
        row["same_process"] = len(sides) == 2
        for k in ("same_arrays", "speedup_of_medians"):
            row.pop(k, None)
        if "device" in row and "reference" in row:
            row["same_digest"] = row["device"]["sha256_16"] == row["reference"]["sha256_16"]
        if len(sides) == 2:
            row["same_arrays"] = same(last["device"], last["reference"])
            row["speedup_of_medians"] = round(row["reference"]["median_s"] / row["device"]["median_s"], 2)
        if name.startswith("local_air"):
            N = np.diff(next(iter(last.values())).indptr) - 1    # (after eliminate_zeros: a lower bound of the neighbourhood sizes)
            row["order_n"] = {"median": float(np.median(N)) * b, "max": int(N.max()) * b}
        print(json.dumps({f"b{b}": {name: row}}), flush=True)
OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text(json.dumps(res, indent=1))
