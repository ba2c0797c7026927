#!/usr/bin/env python3
"""Generate tests/golden/kernels_classical.npz: inputs and the reference's own outputs for the setup of classical (Ruge-Stuben) AMG --
``classical_strength_of_connection``, ``MIS`` / ``PMIS``, ``direct_interpolation`` and ``classical_interpolation``.

Run in the build container (needs the reference built into oracle/_ref by oracle/build_ref.py):
    python tests/golden/make_golden_classical.py

Keys (CSR triples are ``<prefix>.indptr / .indices / .data``; ``names`` lists the cases of each family):

  str.<op>.A                      the operator; str.<op>.<norm>.<k>  the strength matrix for theta = THETAS[k]
      odd150    150 rows, filled unsorted: rows without off-diagonals, an empty row, rows without a diagonal, stored zeros on and off the
                diagonal, positive off-diagonals, all-positive rows (nothing but the diagonal is strong under 'min'), one row of 80 entries
      grid9x7   the 5-point Laplacian
  mis.<g>.G (pattern) / .weights / .mis
      grid17x13, irr200 (symmetrised), each with random weights and (``_ties``) with all-equal weights: every decision is the index
      tie-break; path300: a path with increasing weights, one decision per round -- the deepest chain
  pmis.<g>.S (pattern) / .seed / .splitting      np.random.seed(seed) right before the call
      grid17x13, irr200: non-symmetric, with nodes without any entry and nodes with nothing but a diagonal
  int.<case>.A / .C / .splitting  and the prolongators  .direct / .mod  (with .splitting) and  .unmod  (with .splitting_rs, the
      reference's RS splitting with its second pass: no inner denominator is zero); <P>.nc = P.shape[1]
      aniso11x9   anisotropic 5-point operator, PMIS splitting          box6x5x4   27-point operator, PMIS splitting
      convdiff    non-symmetric, strong POSITIVE off-diagonals ('abs' strength): direct interpolation's sum_strong_pos != 0 branch,
                  classical interpolation's sign rule
      sparseC     8 x 8 Laplacian, every third point in both directions coarse: strong F-F pairs without a common C-point, F-rows
                  without any strong C-neighbour
      level1      the level-1 operator of a reference RS hierarchy, rows unsorted as R @ A @ P leaves them
      hub         one row with 100 strong neighbours, half of them coarse (beyond the 64-lane size class)
  e2e.A / .seed / .P0 / .A1       ruge_stuben_solver(A, CF='PMIS', max_levels=3) of the 17 x 13 grid: its first prolongator and level-1
                                  operator
"""
import sys
from pathlib import Path

import numpy as np
import scipy.sparse as sp

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

import oracle.refimport  # noqa: E402,F401
import pyamg  # noqa: E402
from pyamg.classical import interpolate as ri  # noqa: E402
from pyamg.classical import split as rs  # noqa: E402
from pyamg.gallery import poisson, stencil_grid  # noqa: E402
from pyamg.strength import classical_strength_of_connection as ref_strength  # noqa: E402

SEED = 20261018
THETAS = (0.0, 0.25, 1.0)
OUT = HERE / "kernels_classical.npz"


def put(out, prefix, M, data=True):
    out[prefix + ".indptr"] = np.asarray(M.indptr, dtype=np.int32)
    out[prefix + ".indices"] = np.asarray(M.indices, dtype=np.int32)
    if data:
        out[prefix + ".data"] = np.asarray(M.data, dtype=np.float64)


def raw_csr(rows, n):
    """rows: list of (cols, vals) in the order they are to be stored"""
    indptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int32)
    indices = np.concatenate([np.asarray(c, dtype=np.int32) for c, _ in rows])
    data = np.concatenate([np.asarray(v, dtype=np.float64) for _, v in rows])
    return sp.csr_array((data, indices, indptr), shape=(n, n))


def odd150():
    rng = np.random.RandomState(SEED)
    n, rows = 150, []
    for i in range(n):
        k = 80 if i == 30 else rng.randint(2, 9)
        cols = rng.choice(np.delete(np.arange(n), i), size=k, replace=False)
        vals = -rng.rand(k) - 0.05
        if i % 7 == 3:
            vals[rng.rand(k) < 0.4] *= -1.0                 # positive off-diagonals
        if 20 <= i < 25:
            vals = np.abs(vals)                             # all-positive rows
        if i % 11 == 5:
            vals[0] = 0.0                                   # a stored zero
        diag = [np.abs(vals).sum() + rng.rand()]
        if i % 13 == 6:
            diag = [0.0]                                    # a stored zero on the diagonal
        if i < 5:
            cols, vals = cols[:0], vals[:0]                 # no off-diagonals
        if 10 <= i < 15:
            diag = []                                       # no diagonal
        c, v = np.concatenate([cols, [i] * len(diag)]), np.concatenate([vals, diag])
        if i == 7:
            c, v = c[:0], v[:0]                             # an empty row
        perm = rng.permutation(len(c))
        rows.append((c[perm], v[perm]))
    A = raw_csr(rows, n)
    assert not A.has_canonical_format and np.diff(A.indptr).max() > 64
    return A


def irr200():
    """a non-symmetric strength-like matrix: nodes 0-4 without any entry (and in nobody's row), nodes 5-9 with a diagonal only"""
    rng = np.random.RandomState(SEED + 1)
    n, rows = 200, []
    for i in range(n):
        if i < 5:
            rows.append(([], []))
        elif i < 10:
            rows.append(([i], [1.0]))
        else:
            cols = rng.choice(np.arange(10, n), size=rng.randint(1, 7), replace=False)
            cols = np.unique(np.concatenate([cols[cols != i], [i] if i % 3 else []])).astype(np.int32)
            perm = rng.permutation(len(cols))
            rows.append((cols[perm], rng.rand(len(cols)) + 0.1))
    return raw_csr(rows, n)


def sym_pattern(S):
    S = sp.csr_array(S)
    G = sp.csr_array((np.ones(S.nnz), S.indices, S.indptr), shape=S.shape)
    G = sp.csr_array(G + G.T)
    G.data[:] = 1.0
    return G


def interp_case(out, name, A, C, splitting):
    A, C = sp.csr_array(A), sp.csr_array(C)
    splitting = np.asarray(splitting, dtype=np.int32)
    put(out, f"int.{name}.A", A); put(out, f"int.{name}.C", C)
    out[f"int.{name}.splitting"] = splitting
    todo = [("direct", lambda s: ri.direct_interpolation(A, C, s), splitting),
            ("mod", lambda s: ri.classical_interpolation(A, C, s, modified=True), splitting)]
    split_rs = np.asarray(rs.RS(C, second_pass=True), dtype=np.int32)
    out[f"int.{name}.splitting_rs"] = split_rs
    todo.append(("unmod", lambda s: ri.classical_interpolation(A, C, s, modified=False), split_rs))
    kinds = []
    for kind, fn, s in todo:
        P = sp.csr_array(fn(s.copy()))
        if kind == "unmod" and not np.all(np.isfinite(P.data)):
            continue                                        # (only where the issue's case list asks for it is it required below)
        assert np.all(np.isfinite(P.data)), (name, kind)
        put(out, f"int.{name}.{kind}", P)
        out[f"int.{name}.{kind}.nc"] = np.int64(P.shape[1])
        kinds.append(kind)
    out[f"int.{name}.kinds"] = np.array(kinds)
    return kinds


def main():
    out = {}
    # ---------------------------------------------------------------- strength
    ops = {"odd150": odd150(), "grid9x7": sp.csr_array(poisson((9, 7), format="csr"))}
    for name, A in ops.items():
        put(out, f"str.{name}.A", A)
        for norm in ("abs", "min"):
            for k, theta in enumerate(THETAS):
                put(out, f"str.{name}.{norm}.{k}", ref_strength(A.copy(), theta=theta, norm=norm))
    out["str.names"] = np.array(sorted(ops))
    out["str.thetas"] = np.array(THETAS)
    # ---------------------------------------------------------------- MIS / PMIS
    rng = np.random.RandomState(SEED + 2)
    Sg = ref_strength(sp.csr_array(poisson((17, 13), format="csr")), theta=0.25)
    Si = irr200()
    path = sp.csr_array(sp.diags_array([np.ones(299), np.ones(299)], offsets=[-1, 1], format="csr"))
    graphs = {"grid17x13": sym_pattern(Sg), "irr200": sym_pattern(Si)}
    mis_cases = {}
    for g, G in graphs.items():
        mis_cases[g] = (G, rng.rand(G.shape[0]) + rng.randint(0, 3, G.shape[0]))
        mis_cases[g + "_ties"] = (G, np.ones(G.shape[0]))
    mis_cases["path300"] = (path, np.arange(300, dtype=np.float64))
    for name, (G, w) in mis_cases.items():
        put(out, f"mis.{name}.G", G, data=False)
        out[f"mis.{name}.weights"] = np.asarray(w, dtype=np.float64)
        out[f"mis.{name}.mis"] = np.asarray(rs.MIS(G.copy(), w.copy()), dtype=np.int32)
    out["mis.names"] = np.array(sorted(mis_cases))
    for k, (name, S) in enumerate((("grid17x13", Sg), ("irr200", Si))):
        put(out, f"pmis.{name}.S", S, data=False)
        out[f"pmis.{name}.seed"] = np.int64(SEED + 10 + k)
        np.random.seed(SEED + 10 + k)
        out[f"pmis.{name}.splitting"] = np.asarray(rs.PMIS(sp.csr_array(S).copy()), dtype=np.int32)
    out["pmis.names"] = np.array(["grid17x13", "irr200"])
    assert out["pmis.irr200.splitting"][:10].sum() == 0      # _set_dirichlet
    # ---------------------------------------------------------------- interpolation
    names = []

    def pmis(C, k):
        np.random.seed(SEED + 20 + k)
        return rs.PMIS(sp.csr_array(C).copy())

    A = sp.csr_array(stencil_grid(np.array([[0.0, -1.0, 0.0], [-0.05, 2.1, -0.05], [0.0, -1.0, 0.0]]), (11, 9), format="csr"))
    C = ref_strength(A, theta=0.25)
    interp_case(out, "aniso11x9", A, C, pmis(C, 0)); names.append("aniso11x9")
    st = -np.ones((3, 3, 3)); st[1, 1, 1] = 26.0
    A = sp.csr_array(stencil_grid(st, (6, 5, 4), format="csr"))
    C = ref_strength(A, theta=0.25)
    interp_case(out, "box6x5x4", A, C, pmis(C, 1)); names.append("box6x5x4")
    A = sp.csr_array(stencil_grid(np.array([[0.0, -1.0, 0.0], [-3.0, 4.5, 1.0], [0.0, -1.0, 0.0]]), (9, 8), format="csr"))
    C = ref_strength(A, theta=0.25, norm="abs")
    interp_case(out, "convdiff", A, C, pmis(C, 2)); names.append("convdiff")
    assert (C.multiply(A)).data.max() > 0 and A.data[A.data > 0].size > A.shape[0]
    A = sp.csr_array(poisson((8, 8), format="csr"))
    C = ref_strength(A, theta=0.25)
    ii, jj = np.divmod(np.arange(64), 8)
    k = interp_case(out, "sparseC", A, C, ((ii % 3 == 0) & (jj % 3 == 0)).astype(np.int32)); names.append("sparseC")
    assert "unmod" in k                                      # the modified=False case of the issue: RS second-pass splitting
    np.random.seed(SEED + 30)
    ml = pyamg.ruge_stuben_solver(sp.csr_array(poisson((20, 20), format="csr")), max_levels=3, max_coarse=5)
    A1 = sp.csr_array(ml.levels[1].A)
    assert not A1.has_sorted_indices and np.any(np.concatenate([np.diff(A1.indices[a:b]) < 0 for a, b in zip(A1.indptr[:-1], A1.indptr[1:])]))
    C = ref_strength(A1, theta=0.25)
    interp_case(out, "level1", A1, C, pmis(C, 3)); names.append("level1")
    n = 131
    rows, cols = [], []
    for j in range(1, 101):
        rows += [0, j]; cols += [j, 0]
    for j in range(1, n - 1):
        rows += [j, j + 1]; cols += [j + 1, j]
    G = sp.coo_array((-np.ones(len(rows)), (rows, cols)), shape=(n, n)).tocsr()
    A = sp.csr_array(G + sp.diags_array(-G.sum(axis=1) + 0.5))
    A = sp.csr_array((A.data, A.indices.astype(np.int32), A.indptr.astype(np.int32)), shape=A.shape)
    C = ref_strength(A, theta=0.25)
    splitting = (np.arange(n) % 2 == 1).astype(np.int32)
    interp_case(out, "hub", A, C, splitting); names.append("hub")
    assert C.indptr[1] - C.indptr[0] >= 100
    out["int.names"] = np.array(names)
    # ---------------------------------------------------------------- end to end
    A = sp.csr_array(poisson((17, 13), format="csr"))
    np.random.seed(SEED + 40)
    ml = pyamg.ruge_stuben_solver(A, CF="PMIS", max_levels=3, max_coarse=5)
    assert len(ml.levels) == 3
    put(out, "e2e.A", A)
    out["e2e.seed"] = np.int64(SEED + 40)
    put(out, "e2e.P0", sp.csr_array(ml.levels[0].P)); out["e2e.P0.nc"] = np.int64(ml.levels[0].P.shape[1])
    put(out, "e2e.A1", sp.csr_array(ml.levels[1].A))
    np.savez_compressed(OUT, **out)
    size = OUT.stat().st_size
    assert size < (1 << 20), size
    print(f"{OUT.name}: {len(out)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
