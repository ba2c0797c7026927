#!/usr/bin/env python3
"""Wall time of ``cg_prolongation_smoothing`` (maxiter 4, weighting 'local') on the finest level of two operators, uploads and
downloads included: ``pyamg_amd.energy`` on the device, or the reference's function from oracle/_ref on one host core.

  poisson   : the 7-point Laplacian on 128^3, one candidate, root nodes (C-point rows reset)
  elasticity: 3-D linear elasticity (P1 tets, tools/problems.py) on 64^3 vertices, six rigid-body modes, (3,6) blocks

``--krylov gmres`` measures ``gmres_prolongation_smoothing`` instead (maxiter 3, as blackbox.py sets it), on

  convdiff  : first-order upwind convection-diffusion on 1024^2 (epsilon 0.01, flow at 36 degrees: not symmetric), one candidate

The arguments are built here the way ``energy_prolongation_smoother`` builds them (degree 1) -- symmetric strength (theta 0),
standard aggregation, the tentative prolongator, the pattern ``C @ T``, ``BtBinv`` -- from this package's device functions where
there is a GPU and from the reference's where there is oracle/_ref; the aggregates and T are the same arrays on either side.  A
machine that has only one of the two measures that side and completes a record that already holds the other (--out): the two
columns then come from two hosts and no ratio is recorded.  Medians of --runs calls after one warm-up call.

    python tools/microbench_energy.py [--small]              # -> profiles/r15_energy_cg.json  (--out DIR: somewhere else)
    python tools/microbench_energy.py --once poisson         # one device call and nothing else: the command to put under rocprofv3
    python tools/microbench_energy.py --krylov gmres [--small | --once convdiff]         # -> profiles/r16_energy_gmres.json

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
ap.add_argument("--small", action="store_true", help="24^3, 10^3 and 48^2: a rehearsal of the code path, not a measurement")
ap.add_argument("--krylov", choices=["cg", "gmres"], default="cg")
ap.add_argument("--once", choices=["poisson", "elasticity", "convdiff"])
ap.add_argument("--side", choices=["device", "reference"])
ap.add_argument("--out", default=str(ROOT / "profiles"))
a = ap.parse_args()
OUT = Path(a.out) / ("r15_energy_cg.json" if a.krylov == "cg" else "r16_energy_gmres.json")
MAXITER = 4 if a.krylov == "cg" else 3

from pyamg_amd import _capi as capi  # noqa: E402
import oracle.refimport as ri  # noqa: E402
from tools.problems import elasticity3d, poisson_csr  # noqa: E402

have_gpu = capi.device_count() > 0 and a.side != "reference"
have_ref = ri.available() and a.side != "device" and not a.once
if not (have_gpu or have_ref):
    sys.exit("neither a GPU nor oracle/_ref here: nothing to measure")
if have_gpu:
    capi.lib()
    from pyamg_amd import aggregation as dagg
    from pyamg_amd import energy as den
if have_ref:
    import pyamg  # noqa: F401
    import pyamg.aggregation.smooth as rsm
    from pyamg.aggregation.aggregate import standard_aggregation as ref_aggregate
    from pyamg.aggregation.tentative import fit_candidates as ref_fit
    from pyamg.strength import symmetric_strength_of_connection as ref_strength


def btbinv(B, pattern):
    """pinv(B_i^H B_i) per block row of the pattern (util.utils.compute_BtBinv), with NumPy's batched pinv"""
    r, c = pattern.blocksize
    K = B.shape[1]
    Bj = B.reshape(-1, c, K)
    BtB = np.einsum("jck,jcl->jkl", Bj, Bj).reshape(-1, K * K)
    rows = sp.csr_array((np.ones(pattern.indices.size), pattern.indices, pattern.indptr), shape=(pattern.shape[0] // r, pattern.shape[1] // c))
    return np.linalg.pinv((rows @ BtB).reshape(-1, K, K), hermitian=True)


def upwind2d(n, epsilon=0.01, degrees=36.0):
    """-epsilon Laplace(u) + w . grad(u) on n x n points, w = (cos, sin) of the flow angle, backward differences for the convection"""
    h = 1.0 / (n + 1)
    e = np.ones(n)
    lap = sp.diags_array([-e[:-1], 2 * e, -e[:-1]], offsets=[-1, 0, 1]) * (epsilon / h**2)
    back = sp.diags_array([-e[:-1], e], offsets=[-1, 0]) / h
    one = [lap + back * w for w in (np.cos(np.deg2rad(degrees)), np.sin(np.deg2rad(degrees)))]
    return sp.csr_array(sp.kron(sp.eye_array(n), one[0]) + sp.kron(one[1], sp.eye_array(n)))


def arguments(name, device):
    if name == "convdiff":
        A = upwind2d(48 if a.small else 1024)
        A = sp.bsr_array((A.data.reshape(-1, 1, 1), A.indices, A.indptr), shape=A.shape)
        B = np.ones((A.shape[0], 1))
    elif name == "poisson":
        n = 24 if a.small else 128
        A = sp.csr_array(poisson_csr((n, n, n)))
        A = sp.bsr_array((A.data.reshape(-1, 1, 1), A.indices, A.indptr), shape=A.shape)
        B = np.ones((A.shape[0], 1))
    else:
        A, B = elasticity3d(10 if a.small else 64)
        A = sp.bsr_array(A, blocksize=(3, 3))
    A.sort_indices()
    bs = A.blocksize[0]
    strength, aggregate, fit = (dagg.symmetric_strength_of_connection, dagg.standard_aggregation, dagg.fit_candidates) if device else \
                               (ref_strength, ref_aggregate, ref_fit)
    C = strength(A if bs > 1 else A.tocsr(), 0.0)
    AggOp, Cnodes = aggregate(sp.csr_array(C))
    T, Bc = fit(AggOp, B)
    T = sp.bsr_array(T, blocksize=(bs, B.shape[1]))
    T.sort_indices()
    nb, nbc = A.shape[0] // bs, T.shape[1] // B.shape[1]
    t = sp.csr_array((np.ones(T.indices.size), T.indices, T.indptr), shape=(nb, nbc))
    params = (False, {})
    if name == "poisson":                                   # root nodes: identity at the C points, in T and in the pattern
        Cnodes = np.asarray(Cnodes)
        P_I = sp.csr_array((np.ones(nbc), (Cnodes, np.arange(nbc))), shape=(nb, nbc))
        f = np.ones(nb)
        f[Cnodes] = 0.0
        I_F = sp.dia_array((f[None, :], [0]), shape=(nb, nb)).tocsr()
        I_F.eliminate_zeros()
        params = (True, {"P_I": sp.bsr_array(P_I, blocksize=(1, 1)), "I_F": sp.bsr_array(I_F, blocksize=(1, 1))})
        T = sp.bsr_array(I_F @ sp.csr_array(T) + P_I, blocksize=(1, 1))
    s = sp.csr_array((np.ones(C.indices.size), C.indices, C.indptr), shape=(nb, nb)) @ t
    if params[0]:
        s = sp.csr_array(I_F @ s + P_I)
    s.sort_indices()
    pattern = sp.bsr_array((np.ones((s.indices.size, bs, B.shape[1])), s.indices.astype(np.int32), s.indptr.astype(np.int32)), shape=T.shape)
    T.sort_indices()
    for M in (A, T):
        M.indices, M.indptr = M.indices.astype(np.int32), M.indptr.astype(np.int32)
    return (A, T, np.ascontiguousarray(Bc), btbinv(np.ascontiguousarray(Bc), pattern), pattern, MAXITER, 1e-8, "local", params)


LAYER2 = []                                                 # seconds inside amg_core.energy_cg / energy_gmres (uploads, kernels, download) per device call
ITERATIONS = []                                             # what that call returned first: the iterations done
if have_gpu:
    def _timed(driver):
        def call(*x, **k):
            t0 = time.perf_counter()
            out = driver(*x, **k)
            LAYER2.append(time.perf_counter() - t0)
            ITERATIONS.append(int(out[0]))
            return out
        return staticmethod(call)
    den.amg_core = type("Core", (), {"energy_cg": _timed(den.amg_core.energy_cg), "energy_gmres": _timed(den.amg_core.energy_gmres)})


def timed(fn, args):
    fresh = [x.copy() if hasattr(x, "copy") else x for x in args[:5]]      # (the copies are not part of the call)
    t0 = time.perf_counter()
    T = fn(*fresh, *args[5:])
    if have_gpu:
        capi.sync()
    return time.perf_counter() - t0, T


def measure(name):
    rec = {}
    smoother = f"{a.krylov}_prolongation_smoothing"
    for side, have, fn in (("device", have_gpu, getattr(den, smoother) if have_gpu else None),
                           ("reference", have_ref, getattr(rsm, smoother) if have_ref else None)):
        if not have:
            continue
        args = arguments(name, side == "device")
        A, T, pattern = args[0], args[1], args[4]
        timed(fn, args)                                      # warm-up
        times, out = [], None
        for _ in range(1 if a.once else a.runs):
            dt, out = timed(fn, args)
            times.append(dt)
        out = sp.csr_array(out)
        rec[side] = {"rows": int(A.shape[0]), "blocks": [int(v) for v in T.blocksize], "pattern_blocks": int(pattern.indices.size),
                     "T_blocks_in": int(T.indices.size), "seconds_median": statistics.median(times), "seconds_min": min(times),
                     "seconds_max": max(times), "runs": len(times), "abs_sum_T_out": float(np.abs(out.data).sum()),
                     "abs_sum_T_in": float(np.abs(T.data).sum())}
        if side == "device":
            rec[side]["seconds_in_layer2_call_median"] = statistics.median(LAYER2[-len(times):])
            rec[side]["iterations"] = ITERATIONS[-1]
        print(name, side, json.dumps(rec[side]), flush=True)
    return rec


names = [a.once] if a.once else (["poisson", "elasticity"] if a.krylov == "cg" else ["convdiff"])
result = {n: measure(n) for n in names}
if not a.once:
    OUT.parent.mkdir(parents=True, exist_ok=True)
    old = json.loads(OUT.read_text()) if OUT.exists() else {}
    for n, rec in result.items():
        old.setdefault(n, {}).update(rec)
    old["small"] = bool(a.small)
    old["same_process"] = bool(have_gpu and have_ref)
    OUT.write_text(json.dumps(old, indent=1) + "\n")
    print(OUT)
