#!/usr/bin/env python3
"""Generate tests/golden/kernels_rootnode.npz: inputs and the reference's own outputs for the setup of ``rootnode_solver`` around the
energy-minimisation loop -- ``calc_BtB`` / ``compute_BtBinv``, ``scale_T``, ``filter_operator`` and the candidate relaxation.

Run in the build container (needs the reference built into oracle/_ref by oracle/build_ref.py):
    python tests/golden/make_golden_rootnode.py

Data only; every operator has at most 300 rows.  Matrices are ``<prefix>.data / .indices / .indptr / .shape`` (BSR; ``.csr`` true where
the reference saw a csr_array).

  btb.<case>.B / .C (the pattern) -> .BtB (amg_core.calc_BtB's output, [n, K, K], a block column-major) / .BtBinv (compute_BtBinv)
      k1        one candidate, CSR pattern of 67 nodes (no multiple of a group count); the rows of B under node 5 are zero (inverse 0)
      k3        three candidates on (2, 2) blocks: NullDim larger than cols_per_block
      k6        six candidates on (3, 3) blocks
      crafted   three candidates, CSR pattern of 67 x 170: row 0 stores 160 blocks (beyond the widest lane group), row 1 none, row 2 is
                shuffled and stores one column twice, the rows of B under node 3 are zero (inverse 0); rows with fewer than three
                neighbours have rank-deficient blocks
      rankdef   three candidates, the third equal to the first: every block has rank two
      For K > 1 the script asserts the knife-edge condition of tests/schwarz_setup_cases.py on every block: no singular-value ratio
      within [0.2, 5] x set_tol.
  st.<case>.T / .P_I / .I_F_diag -> .out      scale_T, captured at its call inside rootnode_solver on level 0
      rn_poisson  Poisson 12 x 11;  rn_aniso  rotated anisotropic diffusion 14 x 14;  rn_elas  2-D elasticity 10 x 10 (2 x 2 blocks)
      no_coarse   rn_poisson's T with an injection that stores nothing (P_I.nnz == 0): T comes back as it is
  fo.<case>.A / .C / .B / .Bf / .BtBinv -> .out      filter_operator, captured at its call inside energy_prolongation_smoother
      rn_elas     the elasticity operator with its three rigid-body modes on 2 x 2 blocks (the only one of the three that filters)
  rx.<case>.A / .B / .method / .kwargs (JSON) -> .out      relaxation_as_linear_operator(method, A, 0) @ B
      gs_aniso        gauss_seidel, symmetric, 4 iterations, the diffusion operator, the constant
      bgs_elas        block_gauss_seidel, symmetric, 4 iterations, the elasticity operator (BSR), its three candidates
      jacobi_poisson  jacobi with withrho=False, omega 2/3, 2 iterations, the Poisson operator, two seeded candidates
  e2e.elas.A / .B   the elasticity operator and the gallery's three rigid-body modes: the end-to-end hierarchy test.  Measured by this
      script over every BtB block of every level of rootnode_solver on it: kappa_+ <= 656 (asserted: <= 1e3) with the gallery's own
      coordinates, which are therefore not rescaled; the pseudo-inverse bound 64 eps kappa_+ is then 9.4e-12, a decade under the 1e-10
      bar.
"""
import json
import sys
from pathlib import Path

import numpy as np
import scipy.sparse as sp

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

import oracle.refimport  # noqa: E402,F401
import pyamg  # noqa: E402
import pyamg.aggregation.rootnode as rrn  # noqa: E402
import pyamg.aggregation.smooth as rsm  # noqa: E402
import pyamg.util.utils as rut  # noqa: E402
from pyamg import amg_core as rcore  # noqa: E402
from pyamg.gallery import linear_elasticity, poisson, stencil_grid  # noqa: E402
from pyamg.gallery.diffusion import diffusion_stencil_2d  # noqa: E402
from pyamg.relaxation.utils import relaxation_as_linear_operator  # noqa: E402

import rootnode_cases as rc  # noqa: E402

SEED = 20261021
OUT = HERE / "kernels_rootnode.npz"
TOL = 1e6 * np.finfo(np.float64).eps
out = {}


def put(prefix, M):
    rc.put_bsr(out, prefix, sp.bsr_array(M, blocksize=(1, 1)) if M.format == "csr" else M)
    out[prefix + ".csr"] = np.bool_(M.format == "csr")
    assert M.shape[0] <= 300


def pattern(rng, n, nc, bs, density, fmt):
    M = rng.random((n, nc)) < density
    s = sp.csr_array(M.astype(float))
    s.sort_indices()
    s.indices, s.indptr = s.indices.astype(np.int32), s.indptr.astype(np.int32)
    if fmt == "csr":
        return s
    return sp.bsr_array((np.ones((s.indices.size, *bs)), s.indices, s.indptr), shape=(n * bs[0], nc * bs[1]))


def put_btb(name, B, C):
    K = B.shape[1]
    r, c = C.blocksize if C.format == "bsr" else (1, 1)
    n = C.shape[0] // r
    BtB = np.zeros(n * K * K)
    rcore.calc_BtB(K, n, c, np.ravel(rc.bsq(B)), K * (K + 1) // 2, BtB, C.indptr.astype(np.int32), C.indices.astype(np.int32))
    BtB = BtB.reshape(n, K, K)
    put(f"btb.{name}.C", C)
    out[f"btb.{name}.B"], out[f"btb.{name}.BtB"], out[f"btb.{name}.BtBinv"] = B.copy(), BtB, rut.compute_BtBinv(B, C)
    ranks = []
    for i in range(n):
        s = np.linalg.svd(BtB[i].T, compute_uv=False)
        if K > 1 and s[0] > 0:
            assert not np.any((s > 0.2 * TOL * s[0]) & (s < 5 * TOL * s[0])), (name, i, s / s[0])       # no rank decision on a knife edge
        ranks.append(int(np.sum(s > TOL * s[0])) if s[0] > 0 else 0)
    print(f"btb.{name}: {n} nodes, K = {K}, blocks of {c} columns, ranks {sorted(set(ranks))}, longest row {np.diff(C.indptr).max()}")
    return ranks


def kernels():
    rng = np.random.default_rng(SEED)
    C = pattern(rng, 67, 90, None, 0.08, "csr")
    B = rng.standard_normal((90, 1))
    B[C.indices[C.indptr[5]:C.indptr[6]]] = 0.0
    assert C.indptr[6] > C.indptr[5]
    put_btb("k1", B, C)
    assert out["btb.k1.BtBinv"][5, 0, 0] == 0.0
    put_btb("k3", rng.standard_normal((80, 3)), pattern(rng, 41, 40, (2, 2), 0.15, "bsr"))
    put_btb("k6", rng.standard_normal((90, 6)), pattern(rng, 33, 30, (3, 3), 0.3, "bsr"))
    # crafted
    C = pattern(rng, 67, 170, None, 0.04, "csr").tolil()
    C[0, :] = 0.0
    C[0, :160] = 1.0
    C[1, :] = 0.0
    C[3, :] = 0.0
    C[3, [11, 29, 47, 160]] = 1.0
    C = C.tocsr()
    C.eliminate_zeros()
    C.sort_indices()
    C.indices, C.indptr = C.indices.astype(np.int32), C.indptr.astype(np.int32)
    lo, hi = C.indptr[2], C.indptr[3]
    if hi - lo < 4:
        raise SystemExit("row 2 of the crafted pattern is too short: change the seed")
    C.indices[lo:hi] = C.indices[lo:hi][rng.permutation(hi - lo)]
    C.indices[lo + 1] = C.indices[lo]                        # one column stored twice
    B = rng.standard_normal((170, 3))
    B[[11, 29, 47, 160]] = 0.0
    ranks = put_btb("crafted", B, C)
    assert np.diff(C.indptr)[0] == 160 and np.diff(C.indptr)[1] == 0 and ranks[1] == 0 and ranks[3] == 0 and not out["btb.crafted.BtBinv"][3].any()
    assert 3 in ranks
    B = rng.standard_normal((80, 3))
    B[:, 2] = B[:, 0]
    ranks = put_btb("rankdef", B, pattern(rng, 41, 40, (2, 2), 0.3, "bsr"))
    assert max(ranks) == 2


def operators():
    Ap = poisson((12, 11), format="csr")
    An = stencil_grid(diffusion_stencil_2d(epsilon=0.001, theta=np.pi / 3, type="FE"), (14, 14), format="csr")
    Ae, Be = linear_elasticity((10, 10), format="bsr")
    return {"rn_poisson": (Ap, None), "rn_aniso": (An, None), "rn_elas": (Ae, Be)}


def spy(module, name, seen, snapshot):
    keep = getattr(module, name)

    def wrapper(*a, **k):
        args = snapshot(*a, **k)
        res = keep(*a, **k)
        seen.append((args, res))
        return res
    setattr(module, name, wrapper)
    return keep


def captured():
    for name, (A, B) in operators().items():
        scale, filt = [], []
        k1 = spy(rrn, "scale_T", scale, lambda T, P_I, I_F: (T.copy(), P_I.copy(), I_F.copy()))
        k2 = spy(rsm, "filter_operator", filt, lambda A_, C, B_, Bf, BtBinv=None: (A_.copy(), C.copy(), np.array(B_), np.array(Bf), np.array(BtBinv)))
        try:
            np.random.seed(SEED % 2**31)
            pyamg.rootnode_solver(A, B=B, smooth=("energy", {"krylov": "cg", "maxiter": 4, "degree": 1}), max_coarse=10, max_levels=2)
        finally:
            rrn.scale_T, rsm.filter_operator = k1, k2
        (T, P_I, I_F), res = scale[0]
        p = f"st.{name}"
        put(p + ".T", T), put(p + ".P_I", P_I), put(p + ".out", res)
        out[p + ".I_F_diag"] = I_F.diagonal()
        print(f"{p}: T {T.shape} blocks {T.blocksize}, {T.indices.size} -> {res.indices.size} stored blocks")
        assert bool(filt) == (name == "rn_elas")
        if filt:
            (A_, C, B_, Bf, BtBinv), res = filt[0]
            p = f"fo.{name}"
            put(p + ".A", A_), put(p + ".C", C), put(p + ".out", res)
            out[p + ".B"], out[p + ".Bf"], out[p + ".BtBinv"] = B_, Bf, BtBinv
            print(f"{p}: A {A_.shape} blocks {A_.blocksize}, {A_.indices.size} stored blocks on a pattern of {C.indices.size} -> {res.indices.size}")
        if name == "rn_poisson":
            none = sp.bsr_array((np.zeros((0, 1, 1)), np.zeros(0, dtype=np.int32), np.zeros(P_I.shape[0] + 1, dtype=np.int32)), shape=P_I.shape)
            res = rut.scale_T(T.copy(), none, I_F.copy())
            p = "st.no_coarse"
            put(p + ".T", T), put(p + ".P_I", none), put(p + ".out", res)
            out[p + ".I_F_diag"] = I_F.diagonal()


def relaxed():
    rng = np.random.default_rng(SEED + 1)
    ops = operators()
    An, (Ae, Be), Ap = ops["rn_aniso"][0], ops["rn_elas"], ops["rn_poisson"][0]
    for name, method, A, B in (("gs_aniso", ("gauss_seidel", {"sweep": "symmetric", "iterations": 4}), An, np.ones((An.shape[0], 1))),
                               ("bgs_elas", ("block_gauss_seidel", {"sweep": "symmetric", "iterations": 4}), Ae, Be),
                               ("jacobi_poisson", ("jacobi", {"withrho": False, "omega": 2.0 / 3.0, "iterations": 2}), Ap,
                                rng.standard_normal((Ap.shape[0], 2)))):
        b = np.zeros((A.shape[0], 1))
        p = f"rx.{name}"
        put(p + ".A", A)
        out[p + ".B"], out[p + ".method"], out[p + ".kwargs"] = B.copy(), np.str_(method[0]), np.str_(json.dumps(method[1]))
        out[p + ".out"] = relaxation_as_linear_operator(method, A, b) @ B
        print(f"{p}: {method}, A {A.shape} {A.format}, B {B.shape}")


def end_to_end():
    Ae, Be = operators()["rn_elas"]
    worst = {}
    for label, B in (("gallery", Be),):
        seen = []
        keep = rcore.calc_BtB

        def recording(K, n, c, b, cols, x, Sp, Sj):
            keep(K, n, c, b, cols, x, Sp, Sj)
            seen.append(x.reshape(n, K, K).copy())
        rcore.calc_BtB = recording
        try:
            np.random.seed(7)
            ml = rc.e2e_solver(pyamg, Ae.copy(), B.copy())
        finally:
            rcore.calc_BtB = keep
        k = 0.0
        for BtB in seen:
            for blk in BtB:
                s = np.linalg.svd(blk, compute_uv=False)
                keepers = s[s > TOL * s[0]]
                assert not np.any((s > 0.2 * TOL * s[0]) & (s < 5 * TOL * s[0]))
                k = max(k, s[0] / keepers[-1])
        worst[label] = k
        print(f"e2e elasticity, {label} modes: {len(ml.levels)} levels, {len(seen)} calc_BtB calls, largest kappa_+ = {k:.3g}")
    assert worst["gallery"] <= 1e3
    put("e2e.elas.A", Ae)
    out["e2e.elas.B"] = Be.copy()


if __name__ == "__main__":
    kernels()
    captured()
    relaxed()
    end_to_end()
    out["btb.names"], out["st.names"], out["fo.names"], out["rx.names"] = np.array(rc.BTB), np.array(rc.SCALE), np.array(rc.FILTER), np.array(rc.RELAX)
    np.savez_compressed(OUT, **out)
    print(OUT, OUT.stat().st_size, "bytes")
