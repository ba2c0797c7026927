#!/usr/bin/env python3
"""Wall time of the root-node setup pieces on the finest level of two operators, uploads and downloads included: ``pyamg_amd.rootnode``
on the device, or the reference's functions from oracle/_ref on one host core.

  poisson   : the 7-point Laplacian on 128^3, one candidate (no filter_operator: one candidate on 1 x 1 blocks)
  elasticity: 3-D linear elasticity (P1 tets, tools/problems.py) on 64^3 vertices, six rigid-body modes on 3 x 3 blocks

Pieces: the candidate improvement ``relaxation_as_linear_operator((gs, symmetric x 4), A, 0) @ B`` (block Gauss-Seidel on the BSR
operator), ``compute_BtBinv``, ``scale_T`` and ``filter_operator``.  The arguments are built here the way ``rootnode._extend_hierarchy``
and ``energy_prolongation_smoother`` build them (degree 1) -- symmetric strength (theta 0), standard aggregation, the tentative
prolongator of the first block-size candidates, the injection, the pattern -- from this package's device functions where there is a
GPU and from the reference's where there is oracle/_ref.  On the device side the smoother is set up by a stand-in for the caller's
package (the reference's partials, the block diagonal inverted by ``pyamg_amd.relaxation.get_block_diag``).  A machine that has only
one of the two sides measures that side and completes a record that already holds the other (--out): the two columns then come from
two hosts and no ratio is recorded.  Medians of --runs calls after one warm-up call.

    python tools/microbench_rootnode.py [--small]            # -> profiles/r22_rootnode_setup.json  (--out DIR: somewhere else)

Not product code."""
import argparse
import functools
import json
import statistics
import sys
import time
import types
from pathlib import Path

import numpy as np
import scipy.sparse as sp

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--small", action="store_true", help="24^3 and 10^3: a rehearsal of the code path, not a measurement")
ap.add_argument("--side", choices=["device", "reference"])
ap.add_argument("--out", default=str(ROOT / "profiles"))
a = ap.parse_args()
OUT = Path(a.out) / "r22_rootnode_setup.json"

from pyamg_amd import _capi as capi  # noqa: E402
import oracle.refimport as ri  # noqa: E402
from tools.problems import elasticity3d, poisson_csr  # noqa: E402

have_gpu = capi.device_count() > 0 and a.side != "reference"
have_ref = ri.available() and a.side != "device"
if not (have_gpu or have_ref):
    sys.exit("neither a GPU nor oracle/_ref here: nothing to measure")
if have_gpu:
    capi.lib()
    from pyamg_amd import aggregation as dagg
    from pyamg_amd import rootnode as drn
    from pyamg_amd.relaxation import get_block_diag
if have_ref:
    import pyamg  # noqa: F401
    import pyamg.util.utils as rut
    from pyamg.aggregation.aggregate import standard_aggregation as ref_aggregate
    from pyamg.aggregation.tentative import fit_candidates as ref_fit
    from pyamg.relaxation.utils import relaxation_as_linear_operator as ref_relax
    from pyamg.strength import symmetric_strength_of_connection as ref_strength


def standin():
    """the caller's package for the device side: the reference's smoother setup (relaxation/smoothing.py:494-499, :582-608) restated"""
    mods = {sub: types.ModuleType("standin_mb" + sub) for sub in ("", ".relaxation", ".relaxation.smoothing", ".multilevel")}
    for m in mods.values():
        sys.modules[m.__name__] = m

    def gauss_seidel(A, x, b, iterations=1, sweep="forward"):
        raise AssertionError

    def block_gauss_seidel(A, x, b, iterations=1, sweep="forward", blocksize=1, Dinv=None):
        raise AssertionError

    def setup_block_gauss_seidel(lvl, iterations=1, sweep="forward", Dinv=None, blocksize=None):
        bs = lvl.A.blocksize[0] if lvl.A.format == "bsr" else 1
        if bs == 1:
            return functools.partial(gauss_seidel, iterations=iterations, sweep=sweep)
        return functools.partial(block_gauss_seidel, iterations=iterations, Dinv=get_block_diag(lvl.A, blocksize=bs, inv_flag=True), blocksize=bs, sweep=sweep)
    mods[".relaxation.smoothing"].setup_block_gauss_seidel = setup_block_gauss_seidel
    mods[".multilevel"].MultilevelSolver = type("MultilevelSolver", (), {"Level": type("Level", (), {})})
    return mods[""]


def arguments(name, device):
    if name == "poisson":
        n = 24 if a.small else 128
        A = sp.csr_array(poisson_csr((n, n, n)))
        B = np.ones((A.shape[0], 1))
        bs = 1
    else:
        A, B = elasticity3d(10 if a.small else 64)
        A = sp.bsr_array(A, blocksize=(3, 3))
        bs = 3
    A.sort_indices()
    A.indices, A.indptr = A.indices.astype(np.int32), A.indptr.astype(np.int32)
    strength, aggregate, fit = (dagg.symmetric_strength_of_connection, dagg.standard_aggregation, dagg.fit_candidates) if device else \
                               (ref_strength, ref_aggregate, ref_fit)
    C = strength(A, 0.0)
    AggOp, Cnodes = aggregate(sp.csr_array(C))
    Cnodes = np.asarray(Cnodes)
    T, _ = fit(AggOp, np.ascontiguousarray(B[:, :bs]))
    T = sp.bsr_array(T, blocksize=(bs, bs))
    T.sort_indices()
    T.indices, T.indptr = T.indices.astype(np.int32), T.indptr.astype(np.int32)
    nb, nagg = A.shape[0] // bs, T.shape[1] // bs
    # get_Cpt_params' injection and F-point identity
    P_I = sp.bsr_array((np.tile(np.eye(bs), (nagg, 1, 1)), np.argsort(Cnodes).astype(np.int32),
                        np.concatenate(([0], np.cumsum(np.bincount(Cnodes, minlength=nb)))).astype(np.int32)), shape=T.shape)
    f = np.ones(nb)
    f[Cnodes] = 0.0
    keep = np.flatnonzero(f)
    I_F = sp.bsr_array((np.tile(np.eye(bs), (keep.size, 1, 1)), keep.astype(np.int32), np.concatenate(([0], np.cumsum(f))).astype(np.int32)),
                       shape=(A.shape[0], A.shape[0]))
    Bc = np.ascontiguousarray(P_I.T @ B)
    t = sp.csr_array((np.ones(T.indices.size), T.indices, T.indptr), shape=(nb, nagg))
    s = sp.csr_array((np.ones(C.indices.size), C.indices, C.indptr), shape=(nb, nb)) @ t
    pi = sp.csr_array((np.ones(nagg), (Cnodes, np.arange(nagg))), shape=(nb, nagg))
    s = sp.csr_array(sp.dia_array((f[None, :], [0]), shape=(nb, nb)) @ s + pi)
    s.eliminate_zeros()
    s.sort_indices()
    pattern = sp.bsr_array((np.ones((s.indices.size, bs, bs)), s.indices.astype(np.int32), s.indptr.astype(np.int32)), shape=T.shape)
    return {"A": A, "B": B, "T": T, "P_I": P_I, "I_F": I_F, "Bc": Bc, "pattern": pattern}


def median_of(fn):
    fn()                                                     # warm-up
    times = []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        out = fn()
        if have_gpu:
            capi.sync()
        times.append(time.perf_counter() - t0)
    return {"seconds_median": statistics.median(times), "seconds_min": min(times), "seconds_max": max(times), "runs": len(times)}, out


def measure(name):
    rec = {}
    for side, have in (("device", have_gpu), ("reference", have_ref)):
        if not have:
            continue
        g = arguments(name, side == "device")
        A, B, T, P_I, I_F, Bc, pattern = (g[k] for k in ("A", "B", "T", "P_I", "I_F", "Bc", "pattern"))
        method = ("block_gauss_seidel", {"sweep": "symmetric", "iterations": 4})
        b = np.zeros((A.shape[0], 1))
        if side == "device":
            pkg = standin()
            relax, binv, scale, filt = functools.partial(drn.relaxation_as_linear_operator, pyamg=pkg), drn.compute_BtBinv, drn.scale_T, drn.filter_operator
        else:
            relax, binv, scale, filt = ref_relax, rut.compute_BtBinv, rut.scale_T, rut.filter_operator
        r = {"rows": int(A.shape[0]), "block": int(T.blocksize[0]), "candidates": int(B.shape[1]), "aggregates": int(T.shape[1] // T.blocksize[0]),
             "pattern_blocks": int(pattern.indices.size)}
        r["candidate_relaxation"], Bs = median_of(lambda: relax(method, A, b) @ B)
        r["compute_BtBinv"], BtBinv = median_of(lambda: binv(Bc, pattern))
        r["scale_T"], Ts = median_of(lambda: scale(T, P_I, I_F))
        if B.shape[1] > T.blocksize[0]:
            r["filter_operator"], Tf = median_of(lambda: filt(Ts, pattern, Bc, B, BtBinv))
            r["abs_sum_filtered"] = float(np.abs(Tf.data).sum())
        r["abs_sum_relaxed"], r["abs_sum_BtBinv"], r["abs_sum_scaled"] = float(np.abs(Bs).sum()), float(np.abs(BtBinv).sum()), float(np.abs(Ts.data).sum())
        rec[side] = r
        print(name, side, json.dumps(r), flush=True)
    return rec


result = {n: measure(n) for n in ("poisson", "elasticity")}
OUT.parent.mkdir(parents=True, exist_ok=True)
old = json.loads(OUT.read_text()) if OUT.exists() else {}
for n, rec in result.items():
    old.setdefault(n, {}).update(rec)
old["small"] = bool(a.small)
old["same_process"] = bool(have_gpu and have_ref)
OUT.write_text(json.dumps(old, indent=1) + "\n")
print(OUT)
