#!/usr/bin/env python3
"""Generate tests/golden/kernels_energy_gmres.npz: inputs and the reference's own outputs for energy-minimisation prolongation smoothing
with GMRES (``gmres_prolongation_smoothing``, pyamg/aggregation/smooth.py).

Run in the build container (needs the reference built into oracle/_ref by oracle/build_ref.py):
    python tests/golden/make_golden_energy_gmres.py

Data only; every operator has at most 300 rows.  BSR matrices are ``<prefix>.data / .indices / .indptr / .shape``.

  gm.<case>.args      the case whose arrays this one takes (itself, for a captured case)
  gm.<case>.A / .T / .pattern / .B / .BtBinv / .rooted (/ .P_I / .I_F_diag)      captured cases only: the arguments of the level-0 call of
                      gmres_prolongation_smoothing inside energy_prolongation_smoother
  gm.<case>.maxiter / .tol / .weighting
  gm.<case>.T_out (dense) / .TB_out / .normr / .H / .hsub / .cond      the reference's final T, T @ B, normr before the loop and after
                      every iteration, the rotated Hessenberg matrix as the function leaves it ((maxiter + 1)^2), every sub-diagonal
                      H[i+1, i] before its rotation, and cond(H[0:k, 0:k]) for the k iterations done (0.0 for none)

      sa_cd_P, sa_cd_R  smoothed_aggregation_solver(symmetry='nonsymmetric'), upwind convection-diffusion 12 x 11 (energy_gmres_cases.upwind:
                        epsilon 0.01, flow at 36 degrees), maxiter 4, degree 1: the two calls of level 0, on A for P and on A^H for R
      rn_cd             rootnode_solver(symmetry='nonsymmetric'), the same operator on 14 x 14, maxiter 3, degree 2 (P_I, I_F): the call for P
      rn_elas           rootnode_solver, 2-D elasticity 10 x 10, BSR (2,2), three candidates, maxiter 4
      diagonal          rn_cd's arguments, weighting='diagonal'
      maxiter1          sa_cd_P's arguments, maxiter 1
      bigtol            sa_cd_P's arguments, tol the geometric mean of its normr[1] and normr[2]: exactly two iterations
      notol             rn_cd's arguments, tol above normr[0]: no iteration, T with the C-point rows reset only

Asserted here of every case and recorded (conditions: a nearly broken-down basis or an ill-conditioned H would amplify the difference
between two summation orders beyond any bar): every H[i+1, i] before its rotation is at least 0.05 of its column's 2-norm, and
cond(H[0:k, 0:k]) <= 100.
"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

import oracle.refimport  # noqa: E402,F401
import pyamg  # noqa: E402
import pyamg.aggregation.smooth as rsm  # noqa: E402
from pyamg.gallery import linear_elasticity  # noqa: E402

import energy_gmres_cases as gc  # noqa: E402

SEED = 20261019
OUT = HERE / "kernels_energy_gmres.npz"
out = {}


def run_reference(args, kw):
    """the reference's function, with its locals watched line by line: normr after every iteration (the value the loop's head sees),
    each H[i+1, i] as it stands before the rotation clears it, and H at the end"""
    code = rsm.gmres_prolongation_smoothing.__code__
    normr, hsub, last = {}, {}, {}

    def local(frame, event, arg):
        f = frame.f_locals
        if "normr" in f and "i" in f:
            i = f["i"]
            normr[i] = float(f["normr"])
            if i >= 0 and f["H"][i + 1, i] != 0.0:
                hsub[i] = float(f["H"][i + 1, i])
            last["H"] = f["H"]
        return local

    def tracer(frame, event, arg):
        return local if frame.f_code is code else None
    sys.settrace(tracer)
    try:
        T = rsm.gmres_prolongation_smoothing(*[a.copy() if hasattr(a, "copy") else a for a in args], **kw)
    finally:
        sys.settrace(None)
    its = max(normr)
    assert sorted(normr) == list(range(-1, its + 1)) and sorted(hsub) == list(range(its + 1))
    return T, np.array([normr[i] for i in range(-1, its + 1)]), last["H"].copy(), np.array([hsub[i] for i in range(its + 1)])


def capture(solver, A, B, maxiter, degree, **kw):
    """the arguments of the level-0 calls of gmres_prolongation_smoothing inside energy_prolongation_smoother"""
    seen = []
    keep = rsm.gmres_prolongation_smoothing

    def spy(A_, T, B_, BtBinv, pattern, maxiter_, tol, weighting="local", Cpt_params=None):
        seen.append(((A_.copy(), T.copy(), np.array(B_), np.array(BtBinv), pattern.copy()),
                     {"maxiter": maxiter_, "tol": tol, "weighting": weighting, "Cpt_params": Cpt_params}))
        return keep(A_, T, B_, BtBinv, pattern, maxiter_, tol, weighting, Cpt_params)
    rsm.gmres_prolongation_smoothing = spy
    try:
        np.random.seed(SEED % 2**31)
        solver(A, B=B, smooth=("energy", {"krylov": "gmres", "maxiter": maxiter, "degree": degree}), max_coarse=10, max_levels=2, **kw)
    finally:
        rsm.gmres_prolongation_smoothing = keep
    return seen


def put(name, args, kw, of=None):
    A, T, B, BtBinv, pattern = args
    p = f"gm.{name}"
    out[p + ".args"] = np.str_(of or name)
    if of is None:
        for k, M in (("A", A), ("T", T), ("pattern", pattern)):
            gc.put_bsr(out, f"{p}.{k}", M)
        out[p + ".B"], out[p + ".BtBinv"] = B, BtBinv
        rooted = bool(kw["Cpt_params"][0])
        out[p + ".rooted"] = np.bool_(rooted)
        if rooted:
            gc.put_bsr(out, p + ".P_I", kw["Cpt_params"][1]["P_I"])
            out[p + ".I_F_diag"] = kw["Cpt_params"][1]["I_F"].diagonal()
    out[p + ".maxiter"], out[p + ".tol"], out[p + ".weighting"] = np.int64(kw["maxiter"]), np.float64(kw["tol"]), np.str_(kw["weighting"])
    Tout, normr, H, hsub = run_reference(args, kw)
    k = len(normr) - 1
    # the conditions: far from a breakdown, H well conditioned
    ratios = np.array([hsub[i] / np.sqrt(np.sum(H[:i + 1, i] ** 2)) for i in range(k)])     # (a rotation keeps the column's 2-norm)
    cond = float(np.linalg.cond(H[:k, :k])) if k else 0.0
    assert np.all(ratios >= gc.SUBDIAGONAL_FLOOR) and cond <= gc.COND_CEILING, (name, ratios, cond)
    assert A.shape[0] <= 300 and k == gc.ITERATIONS[name], (name, k)
    out[p + ".T_out"], out[p + ".TB_out"], out[p + ".normr"], out[p + ".H"] = Tout.toarray(), Tout @ B, normr, H
    out[p + ".hsub"], out[p + ".cond"] = hsub, np.float64(cond)
    print(f"{name}: {A.shape[0]} rows, blocks {T.blocksize}, normr {normr}, sub-diagonal / column {ratios.round(3)}, cond {cond:.2f}")
    return normr


def whole():
    sa, rn = pyamg.smoothed_aggregation_solver, pyamg.rootnode_solver
    calls = capture(sa, gc.upwind(12, 11), None, 4, 1, symmetry="nonsymmetric")
    assert len(calls) == 2 and (calls[0][0][0] != calls[1][0][0]).nnz and (calls[0][0][0].T != calls[1][0][0]).nnz == 0        # A, then A^H
    sa_P, sa_R = calls
    first = put("sa_cd_P", *sa_P)
    put("sa_cd_R", *sa_R)
    calls = capture(rn, gc.upwind(14, 14), None, 3, 2, symmetry="nonsymmetric")
    assert len(calls) == 2 and calls[0][1]["Cpt_params"][0]
    rn_cd = calls[0]
    rn_first = put("rn_cd", *rn_cd)
    Ae, Be = linear_elasticity((10, 10), format="bsr")
    calls = capture(rn, Ae, Be, 4, 1)
    assert len(calls) == 1 and calls[0][0][1].blocksize == (2, 2) and calls[0][0][2].shape[1] == 3 and calls[0][1]["Cpt_params"][0]
    put("rn_elas", *calls[0])
    put("diagonal", rn_cd[0], dict(rn_cd[1], weighting="diagonal"), of="rn_cd")
    put("maxiter1", sa_P[0], dict(sa_P[1], maxiter=1), of="sa_cd_P")
    assert first[2] < first[1]
    put("bigtol", sa_P[0], dict(sa_P[1], tol=float(np.sqrt(first[1] * first[2]))), of="sa_cd_P")
    put("notol", rn_cd[0], dict(rn_cd[1], tol=float(2.0 * rn_first[0])), of="rn_cd")


if __name__ == "__main__":
    whole()
    out["gm.names"] = np.array(gc.GMRES)
    np.savez_compressed(OUT, **out)
    print(OUT, OUT.stat().st_size, "bytes")
