#!/usr/bin/env python3
"""Generate tests/golden/kernels_energy.npz: inputs and the reference's own outputs for energy-minimisation prolongation smoothing with
CG -- its two ``amg_core`` calls, ``satisfy_constraints``, and ``cg_prolongation_smoothing`` whole.

Run in the build container (needs the reference built into oracle/_ref by oracle/build_ref.py):
    python tests/golden/make_golden_energy.py

Data only; every operator has at most 300 rows.  BSR matrices are ``<prefix>.data / .indices / .indptr / .shape``.

  imm.<case>.A / .B / .S (the pattern, with the values that go in) / .out (the reference's Sx)      incomplete_mat_mult_bsr
      grid9x7    1 x 1 blocks: the 9 x 7 five-point Laplacian times its tentative prolongator, on the pattern of A @ T, from zero
      elas2x3    (2,2) (2,3) blocks: 2-D elasticity and the tentative prolongator of its three rigid-body modes
      elas3x6    (3,3) (3,6) blocks: 3-D elasticity (tools/problems.py, 4 x 4 x 4 vertices) and its six rigid-body modes
      unsortedB  seeded 2 x 2 blocks, every row of B in shuffled order, one column stored twice in a row of B
      crafted    seeded 2 x 2 blocks: row 1 of S empty, row 0 of S full (160 stored elements: beyond the widest group), entries of S
                 that receive no contribution, Sx non-zero on entry
  sc.<case>.U / .B / .BtBinv / .UB (U @ B, what the helper receives) / .out      satisfy_constraints
      nd1 / nd3 / nd6   the residual-like A @ T of the three operators above, one, three and six candidates
      nd_gt_cols        seeded (2,2) blocks with three candidates: NullDim larger than cols_per_block
      oneblock          nd3 with row 2 cut to one block
      zero_btbinv       nd3 with BtBinv[3] all zero
  cg.<case>.A / .T / .pattern / .B / .BtBinv / .maxiter / .tol / .weighting / .rooted (/ .P_I / .I_F_diag) -> .T_out (dense) / .TB_out /
      .newsums      the arguments of cg_prolongation_smoothing captured at its call inside energy_prolongation_smoother on level 0, the
      final T, T @ B, and the newsum of every iteration (the one that met ``newsum < tol`` included)
      sa_poisson  smoothed_aggregation_solver, Poisson 12 x 11, maxiter 4, degree 1
      sa_aniso    smoothed_aggregation_solver, rotated anisotropic diffusion 14 x 14, maxiter 4, degree 2
      sa_elas     smoothed_aggregation_solver, 2-D elasticity 10 x 10 (BSR), maxiter 1, degree 1
      rn_poisson  rootnode_solver, Poisson 12 x 11, maxiter 4, degree 2
      rn_aniso    rootnode_solver, the same diffusion operator, maxiter 1, degree 1
      rn_elas     rootnode_solver, the same elasticity operator, maxiter 4, degree 1
      bigtol      sa_poisson's arguments with tol between its second and its first newsum: the loop leaves at the first newsum < tol
      diagonal    rn_poisson's arguments with weighting='diagonal'
  e2e.A           rotated anisotropic diffusion on 20 x 15 (300 rows): the operator of the end-to-end hierarchy test
"""
import sys
from pathlib import Path

import numpy as np
import scipy.sparse as sp

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

import oracle.refimport  # noqa: E402,F401
import pyamg  # noqa: E402
import pyamg.aggregation.smooth as rsm  # noqa: E402
from pyamg import amg_core as rcore  # noqa: E402
from pyamg.aggregation.aggregate import standard_aggregation  # noqa: E402
from pyamg.aggregation.tentative import fit_candidates  # noqa: E402
from pyamg.gallery import linear_elasticity, poisson, stencil_grid  # noqa: E402
from pyamg.gallery.diffusion import diffusion_stencil_2d  # noqa: E402
from pyamg.strength import symmetric_strength_of_connection  # noqa: E402
from pyamg.util.utils import compute_BtBinv  # noqa: E402

import energy_cases as ec  # noqa: E402
from tools.problems import elasticity3d  # noqa: E402

SEED = 20261019
OUT = HERE / "kernels_energy.npz"
out = {}


def tentative(A, B):
    """the tentative prolongator of standard aggregation on A's own graph"""
    bs = A.blocksize[0] if A.format == "bsr" else 1
    C = symmetric_strength_of_connection(A.tocsr() if bs == 1 else A, 0.0)
    AggOp = standard_aggregation(C)[0]
    T, Bc = fit_candidates(AggOp, B)
    return sp.bsr_array(T, blocksize=(bs, B.shape[1])) if T.format != "bsr" else T, Bc


def pattern_of(A, T):
    bsA, bsT = A.blocksize, T.blocksize
    a = sp.csr_array((np.ones(A.indices.size), A.indices, A.indptr), shape=(A.shape[0] // bsA[0], A.shape[1] // bsA[1]))
    t = sp.csr_array((np.ones(T.indices.size), T.indices, T.indptr), shape=(T.shape[0] // bsT[0], T.shape[1] // bsT[1]))
    s = (a @ t).tocsr()
    s.sort_indices()
    return sp.bsr_array((np.zeros((s.indices.size, bsA[0], bsT[1])), s.indices.astype(np.int32), s.indptr.astype(np.int32)),
                        shape=(A.shape[0], T.shape[1]))


def i32(M):
    M.indices, M.indptr = M.indices.astype(np.int32), M.indptr.astype(np.int32)
    return M


def ref_imm(A, B, S):
    Sx = np.ravel(S.data).copy()
    r, m = A.blocksize
    c = B.blocksize[1]
    rcore.incomplete_mat_mult_bsr(A.indptr, A.indices, np.ravel(A.data), B.indptr, B.indices, np.ravel(B.data), S.indptr, S.indices, Sx,
                                  A.shape[0] // r, B.shape[1] // c, r, m, c)
    return Sx.reshape(S.data.shape)


def put_imm(name, A, B, S):
    for k, M in (("A", A), ("B", B), ("S", S)):
        ec.put_bsr(out, f"imm.{name}.{k}", M)
    out[f"imm.{name}.out"] = ref_imm(A, B, S)


def put_sc(name, U, B, BtBinv):
    ec.put_bsr(out, f"sc.{name}.U", U)
    out[f"sc.{name}.B"], out[f"sc.{name}.BtBinv"] = B.copy(), BtBinv.copy()
    out[f"sc.{name}.UB"] = U @ B
    V = U.copy()
    rsm.satisfy_constraints(V, B, BtBinv)
    out[f"sc.{name}.out"] = V.data.copy()


def random_bsr(rng, nbr, nbc, bs, density, dense_rows=(), empty_rows=()):
    M = (rng.random((nbr, nbc)) < density)
    for i in dense_rows:
        M[i] = True
    for i in empty_rows:
        M[i] = False
    s = sp.csr_array(M.astype(float))
    s.sort_indices()
    return sp.bsr_array((rng.standard_normal((s.indices.size, *bs)), s.indices.astype(np.int32), s.indptr.astype(np.int32)),
                        shape=(nbr * bs[0], nbc * bs[1]))


def operators():
    A1 = sp.bsr_array(poisson((9, 7), format="csr"), blocksize=(1, 1))
    A2, B2 = linear_elasticity((6, 6), format="bsr")
    A3, B3 = elasticity3d(4)
    A3 = sp.bsr_array(A3, blocksize=(3, 3))
    return (A1, np.ones((A1.shape[0], 1))), (sp.bsr_array(A2), B2), (A3, B3)


def kernels():
    rng = np.random.default_rng(SEED)
    ops = operators()
    for name, sc, (A, B) in zip(("grid9x7", "elas2x3", "elas3x6"), ("nd1", "nd3", "nd6"), ops):
        A.sort_indices()
        T, Bc = tentative(A, B)
        A, T = i32(A), i32(T)
        S = pattern_of(A, T)
        put_imm(name, A, T, S)
        U = S.copy()
        U.data = ref_imm(A, T, S)
        U.data += 0.01 * rng.standard_normal(U.data.shape)  # (A T B = A Bf is nearly zero inside: give the projection something to remove)
        put_sc(sc, U, Bc, compute_BtBinv(Bc, U))
        if sc == "nd3":
            V = U.copy()
            keep = np.ones(V.indices.size, dtype=bool)
            keep[V.indptr[2] + 1:V.indptr[3]] = False
            cut = np.diff(V.indptr).copy()
            cut[2] = 1
            V = sp.bsr_array((V.data[keep], V.indices[keep], np.concatenate(([0], np.cumsum(cut))).astype(np.int32)), shape=V.shape)
            put_sc("oneblock", V, Bc, compute_BtBinv(Bc, V))
            Z = compute_BtBinv(Bc, U)
            Z[3] = 0.0
            put_sc("zero_btbinv", U, Bc, Z)
    U = random_bsr(rng, 40, 30, (2, 2), 0.2)
    Bc = rng.standard_normal((60, 3))
    put_sc("nd_gt_cols", U, Bc, compute_BtBinv(Bc, U))
    # B with unsorted rows, and one row of B that stores a column twice: every match is accumulated
    A = random_bsr(rng, 50, 50, (2, 2), 0.12)
    Bm = random_bsr(rng, 50, 40, (2, 2), 0.15)
    for i in range(50):
        lo, hi = Bm.indptr[i], Bm.indptr[i + 1]
        perm = rng.permutation(hi - lo)
        Bm.indices[lo:hi], Bm.data[lo:hi] = Bm.indices[lo:hi][perm], Bm.data[lo:hi][perm]
    lo = Bm.indptr[7]
    assert Bm.indptr[8] - lo >= 2
    Bm.indices[lo + 1] = Bm.indices[lo]
    put_imm("unsortedB", A, Bm, pattern_of(A, Bm))
    A = random_bsr(rng, 60, 60, (2, 2), 0.1)
    Bm = random_bsr(rng, 60, 40, (2, 2), 0.1)
    S = random_bsr(rng, 60, 40, (2, 2), 0.3, dense_rows=(0,), empty_rows=(1,))
    put_imm("crafted", A, Bm, S)


def newsum_recorder(sums):
    scale_rows = rsm.scale_rows

    def recording(R, Dinv, *a, **k):
        Z = scale_rows(R, Dinv, *a, **k)
        sums.append((R.conjugate().multiply(Z)).sum())       # the reference's own expression, on its own operands
        return Z
    return recording


def run_reference_cg(args, kw):
    sums = []
    keep = rsm.scale_rows
    rsm.scale_rows = newsum_recorder(sums)
    try:
        T = rsm.cg_prolongation_smoothing(*[a.copy() if hasattr(a, "copy") else a for a in args], **kw)
    finally:
        rsm.scale_rows = keep
    return T, np.array(sums, dtype=np.float64)


def capture(solver, A, B, maxiter, degree):
    """the arguments of the level-0 call of cg_prolongation_smoothing inside energy_prolongation_smoother"""
    seen = []
    keep = rsm.cg_prolongation_smoothing

    def spy(A_, T, B_, BtBinv, pattern, maxiter_, tol, weighting="local", Cpt_params=None):
        if not seen:
            seen.append(((A_.copy(), T.copy(), np.array(B_), np.array(BtBinv), pattern.copy()),
                         {"maxiter": maxiter_, "tol": tol, "weighting": weighting, "Cpt_params": Cpt_params}))
        return keep(A_, T, B_, BtBinv, pattern, maxiter_, tol, weighting, Cpt_params)
    rsm.cg_prolongation_smoothing = spy
    try:
        np.random.seed(SEED % 2**31)
        solver(A, B=B, smooth=("energy", {"krylov": "cg", "maxiter": maxiter, "degree": degree}), max_coarse=10, max_levels=2)
    finally:
        rsm.cg_prolongation_smoothing = keep
    return seen[0]


def put_cg(name, args, kw):
    A, T, B, BtBinv, pattern = args
    p = f"cg.{name}"
    for k, M in (("A", A), ("T", T), ("pattern", pattern)):
        ec.put_bsr(out, f"{p}.{k}", M)
    out[p + ".B"], out[p + ".BtBinv"] = B, BtBinv
    out[p + ".maxiter"], out[p + ".tol"], out[p + ".weighting"] = np.int64(kw["maxiter"]), np.float64(kw["tol"]), np.str_(kw["weighting"])
    rooted = bool(kw["Cpt_params"][0])
    out[p + ".rooted"] = np.bool_(rooted)
    if rooted:
        ec.put_bsr(out, p + ".P_I", kw["Cpt_params"][1]["P_I"])
        out[p + ".I_F_diag"] = kw["Cpt_params"][1]["I_F"].diagonal()
    Tout, sums = run_reference_cg(args, kw)
    out[p + ".T_out"], out[p + ".TB_out"], out[p + ".newsums"] = Tout.toarray(), Tout @ B, sums
    assert A.shape[0] <= 300
    print(f"{name}: {A.shape[0]} rows, blocks {T.blocksize}, {len(sums)} newsums {sums}")
    return sums


def whole():
    Ap = poisson((12, 11), format="csr")
    An = stencil_grid(diffusion_stencil_2d(epsilon=0.001, theta=np.pi / 3, type="FE"), (14, 14), format="csr")
    Ae, Be = linear_elasticity((10, 10), format="bsr")
    sa, rn = pyamg.smoothed_aggregation_solver, pyamg.rootnode_solver
    got = {}
    for name, solver, A, B, maxiter, degree in (("sa_poisson", sa, Ap, None, 4, 1), ("sa_aniso", sa, An, None, 4, 2), ("sa_elas", sa, Ae, Be, 1, 1),
                                                ("rn_poisson", rn, Ap, None, 4, 2), ("rn_aniso", rn, An, None, 1, 1), ("rn_elas", rn, Ae, Be, 4, 1)):
        got[name] = capture(solver, A, B, maxiter, degree)
        sums = put_cg(name, *got[name])
        assert len(sums) == maxiter and bool(got[name][1]["Cpt_params"][0]) == (solver is rn)
        if name == "sa_poisson":
            first = sums
    args, kw = got["sa_poisson"]
    assert first[1] < first[0] and first[0] < args[4].nnz
    sums = put_cg("bigtol", args, dict(kw, tol=float(np.sqrt(first[0] * first[1]))))
    assert len(sums) == 2                                    # one update, then newsum < tol
    args, kw = got["rn_poisson"]
    put_cg("diagonal", args, dict(kw, weighting="diagonal"))
    E = stencil_grid(diffusion_stencil_2d(epsilon=0.01, theta=np.pi / 6, type="FE"), (20, 15), format="csr")
    E.sort_indices()
    ec.put_bsr(out, "e2e.A", sp.bsr_array(E, blocksize=(1, 1)))


if __name__ == "__main__":
    kernels()
    whole()
    out["imm.names"], out["sc.names"], out["cg.names"] = np.array(ec.IMM), np.array(ec.SC), np.array(ec.CG)
    np.savez_compressed(OUT, **out)
    print(OUT, OUT.stat().st_size, "bytes")
