#!/usr/bin/env python3
"""The reference's evolution_strength_of_connection and the drop-in (pyamg_amd.evolution) on the same operators, one process.

    python tools/evolution_verify.py [--problem poisson128|elasticity32|...] [--side both|reference|device] [--rho-from FILE] [--out FILE]

With both sides available (the reference built into oracle/_ref, and a device) it runs the reference, then the drop-in with the
reference's spectral radius -- pattern equality and the largest value difference --, then the drop-in with the device Arnoldi's own
spectral radius, and prints both wall times, the per-kernel times of the drop-in (the wall time of each Layer-1 call: upload, kernel,
download) and, for the reference, the wall time of its ``amg_core`` calls and of its Arnoldi inside the one call.  Where only one side
is available it records that side with digests of the result's arrays; ``--rho-from`` gives the device side the spectral radius a
reference-side record holds, so that the digests of two hosts can be compared.

Problems: ``poissonN`` -- N^3 seven-point Poisson, B=None, k=2;  ``elasticityN`` -- 3-D linear elasticity (P1 tets, tools/problems.py)
on N^3 vertices with its six rigid-body modes, BSR(3,3), k=2.
"""
import argparse
import hashlib
import json
import os
import sys
import time
import warnings
from pathlib import Path

import numpy as np
import scipy.sparse as sp

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.problems import elasticity3d, poisson_csr  # noqa: E402


def problem(name):
    if name.startswith("poisson"):
        n = int(name[len("poisson"):])
        return sp.csr_array(poisson_csr((n, n, n))), None
    if name.startswith("elasticity"):
        A, B = elasticity3d(int(name[len("elasticity"):]))
        return sp.bsr_array(A), np.ascontiguousarray(B)
    raise SystemExit(f"unknown problem {name}")


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def record(C, seconds, rho):
    C = sp.csr_array(C)
    return {"seconds": round(seconds, 4), "rho": float(rho).hex(), "shape": list(C.shape), "nnz": int(C.nnz),
            "pattern": digest(C.indptr.astype(np.int64), C.indices.astype(np.int64)), "values": digest(C.data)}


def run(fn, A, B, mod, rho=None, rho_seconds=None):
    """fn(A, B, k=2) with ``mod.approximate_spectral_radius`` fixed to ``rho`` (or recorded, its wall time appended to ``rho_seconds``);
    returns (C, seconds, rho)"""
    seen = []
    old = mod.approximate_spectral_radius

    def recorded(*a, **k):
        t0 = time.perf_counter()
        seen.append(old(*a, **k))
        if rho_seconds is not None:
            rho_seconds.append(time.perf_counter() - t0)
        return seen[-1]
    mod.approximate_spectral_radius = (lambda *a, **k: rho) if rho is not None else recorded
    try:
        np.random.seed(0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t0 = time.perf_counter()
            C = fn(A.copy(), None if B is None else B.copy(), k=2)
            dt = time.perf_counter() - t0
    finally:
        mod.approximate_spectral_radius = old
    return sp.csr_array(C), dt, (rho if rho is not None else seen[0])


def timed_kernels(gcore, names):
    """wall time of every call of ``gcore.<name>`` from now on; returns (times, originals to put back)"""
    names = [n for n in names if hasattr(gcore, n)]
    times = {n: 0.0 for n in names}
    originals = {n: getattr(gcore, n) for n in names}
    for n in names:
        def wrapped(*a, _n=n, **k):
            t0 = time.perf_counter()
            originals[_n](*a, **k)
            times[_n] += time.perf_counter() - t0
        setattr(gcore, n, wrapped)
    return times, originals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problem", action="append")
    ap.add_argument("--side", default="both", choices=["both", "reference", "device"])
    ap.add_argument("--rho-from", default=None, help="a JSON this tool wrote on the reference side: its rho per problem is given to the device side")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    problems = a.problem or ["poisson128", "elasticity32"]
    given = {}
    if a.rho_from:
        for r in json.loads(Path(a.rho_from).read_text())["results"]:
            given[r["problem"]] = float.fromhex(r["reference"]["rho"])
    ref = evo = gcore = None
    if a.side in ("both", "reference"):
        import oracle.refimport as ri
        if not ri.available():
            raise SystemExit("the reference is not built (oracle/build_ref.py)")
        import pyamg.strength as rstr
        ref = rstr.evolution_strength_of_connection
    if a.side in ("both", "device"):
        from pyamg_amd import _capi as capi
        from pyamg_amd import amg_core as gcore
        from pyamg_amd import evolution as evo
        capi.lib()                                            # a missing device is an error here, not a fall-back
    names = ["incomplete_mat_mult_csr", "evolution_strength_helper", "evolution_strength_vector", "apply_distance_filter", "min_blocks"]
    results = []
    for name in problems:
        A, B = problem(name)
        out = {"problem": name, "rows": int(A.shape[0]), "nnz": int(A.nnz), "candidates": 1 if B is None else int(B.shape[1])}
        Cr = None
        rho = given.get(name)
        if ref is not None:
            # the reference's amg_core calls and its Arnoldi, timed inside the one call (strength.py binds both names itself)
            core = type("timed_amg_core", (), {})()
            for n in dir(rstr.amg_core):
                if not n.startswith("_"):
                    setattr(core, n, getattr(rstr.amg_core, n))
            rtimes, _ = timed_kernels(core, names)
            real_core, rstr.amg_core, rho_s = rstr.amg_core, core, []
            try:
                Cr, dt, rho = run(ref, A, B, rstr, rho_seconds=rho_s)
            finally:
                rstr.amg_core = real_core
            out["reference"] = record(Cr, dt, rho)
            out["reference"]["approximate_spectral_radius"] = round(sum(rho_s), 4)
            out["reference"]["kernels"] = {k: round(v, 4) for k, v in rtimes.items() if v}
            print(f"{name}: reference {dt:.3f} s (spectral radius {sum(rho_s):.3f} s, amg_core {out['reference']['kernels']}), "
                  f"rho {float(rho)!r}, nnz {Cr.nnz}", flush=True)
        if evo is not None:
            run(evo.evolution_strength_of_connection, problem("poisson16")[0], None, evo)        # first-call costs (context, code objects)
            times, originals = timed_kernels(gcore, names)
            try:
                if rho is not None:
                    Cd, dt, _ = run(evo.evolution_strength_of_connection, A, B, evo, rho=rho)
                    out["device_same_rho"] = record(Cd, dt, rho)
                    out["device_same_rho"]["kernels"] = {k: round(v, 4) for k, v in times.items() if v}
                    print(f"{name}: drop-in with that rho {dt:.3f} s, kernels {out['device_same_rho']['kernels']}", flush=True)
                    if Cr is not None:
                        same = np.array_equal(Cd.indptr, Cr.indptr) and np.array_equal(Cd.indices, Cr.indices)
                        out["same_rho_pattern_equal"] = bool(same)
                        out["same_rho_max_abs_diff"] = float(np.abs(Cd.data - Cr.data).max()) if same else None
                        out["ratio_reference_over_device"] = round(out["reference"]["seconds"] / dt, 2)
                        print(f"{name}: pattern equal {same}, max |C - C_ref| {out['same_rho_max_abs_diff']}", flush=True)
                for k in times:
                    times[k] = 0.0
                Cd2, dt2, rho_dev = run(evo.evolution_strength_of_connection, A, B, evo)
                out["device_own_rho"] = record(Cd2, dt2, rho_dev)
                out["device_own_rho"]["kernels"] = {k: round(v, 4) for k, v in times.items() if v}
                print(f"{name}: drop-in with the device rho {dt2:.3f} s, rho {float(rho_dev)!r}", flush=True)
                if rho is not None:
                    out["rho_relative_difference"] = abs(float(rho_dev) - float(rho)) / float(rho)
                if Cr is not None:
                    same = np.array_equal(Cd2.indptr, Cr.indptr) and np.array_equal(Cd2.indices, Cr.indices)
                    out["own_rho_pattern_equal"] = bool(same)
                    out["own_rho_max_abs_diff"] = float(np.abs(Cd2.data - Cr.data).max()) if same else None
            finally:
                for k, fn in originals.items():
                    setattr(gcore, k, fn)
        results.append(out)
    doc = {"tool": "tools/evolution_verify.py", "side": a.side, "host_cpus": os.cpu_count(), "results": results}
    text = json.dumps(doc, indent=1)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
