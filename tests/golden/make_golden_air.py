#!/usr/bin/env python3
"""Generate tests/golden/kernels_air.npz: inputs and the reference's own outputs for the setup of approximate ideal restriction (AIR) AMG
-- ``one_point_interpolation`` and ``local_air``.

Run in the build container (needs the reference built into oracle/_ref by oracle/build_ref.py):
    python tests/golden/make_golden_air.py

Keys (CSR triples are ``<prefix>.indptr / .indices / .data``):

  air.ops / air.<op>.A            the operators; air.names lists the cases, each with
  air.<case>.op / .splitting / .theta / .norm / .degree
  air.<case>.Rp                   the row pointer of approx_ideal_restriction_pass1
  air.<case>.Rraw                 R as approx_ideal_restriction_pass2 leaves it (the identity entry last in every row, solution entries
                                  that are exactly 0.0 still stored); air.<case>.R: what local_air returns (after eliminate_zeros)
      line5            poisson((5,)), splitting [1,0,1,0,1]: the docstring example of local_air
      convdiff13x11.*  the benchmark's upwind convection-diffusion stencil (non-symmetric), RS splitting with second pass; degree 1 and 2,
                       (theta, norm) = (0.05, 'abs') and (0.3, 'min')
      box6x5x4         27-point operator, PMIS splitting, degree 2: the wide lane groups (box6x5x4.d1: degree 1, the 9-16 class)
      hub.d1 / .d2     one C-point with 100 strong F-neighbours (non-symmetric values): beyond the 64-lane cap
      level1           the level-1 operator of a reference air_solver hierarchy, rows unsorted as R @ A @ P leaves them
      singular         rank-deficient local systems: an F-point with a stored zero diagonal and no entry inside the neighbourhood (its
                       column of the local system is all zero), two F-points with equal rows (the second column becomes negligible only
                       after the first reflection), a stored explicit zero a_cj; a C-point without any strong F-neighbour
  onept.names / onept.<case>.A / .C / .splitting / .nc  and  .P0 (by_val=False) / .P1 (by_val=True), cut to indptr[-1] entries.  The
      reference leaves the VALUES of the C-rows of P1 unwritten (np.empty); the fixture holds 1.0 there, the value of an injection
      line5     the docstring example          convdiff   the 13 x 11 operator with its reference strength matrix (diagonal kept)
      mixed48   unsorted rows, ties in |C| (the first stored entry wins), F-rows without any C-neighbour, positive and negative entries
  e2e.A / e2e.<cf>.sizes / .seed  air_solver(A, max_coarse=20) of the 17 x 13 convection-diffusion grid, cf = 'rs' (the default) and 'pmis'
  e2e.<cf>.A<l> (l = 0, 1, 2), .P<l>, .R<l> (l = 0, 1)
"""
import sys
from pathlib import Path

import numpy as np
import scipy.sparse as sp

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

import oracle.refimport  # noqa: E402,F401
import pyamg  # noqa: E402
from pyamg import amg_core as ref_core  # noqa: E402
from pyamg.classical import interpolate as ri  # noqa: E402
from pyamg.classical import split as rs  # noqa: E402
from pyamg.gallery import poisson, stencil_grid  # noqa: E402
from pyamg.strength import classical_strength_of_connection as ref_strength  # noqa: E402

SEED = 20261118
OUT = HERE / "kernels_air.npz"


def put(out, prefix, M):
    M = sp.csr_array(M)
    out[prefix + ".indptr"] = np.asarray(M.indptr, dtype=np.int32)
    out[prefix + ".indices"] = np.asarray(M.indices, dtype=np.int32)
    out[prefix + ".data"] = np.asarray(M.data, dtype=np.float64)


def raw_csr(rows, n):
    """rows: list of (cols, vals) in the order they are to be stored"""
    indptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int32)
    indices = np.concatenate([np.asarray(c, dtype=np.int32) for c, _ in rows])
    data = np.concatenate([np.asarray(v, dtype=np.float64) for _, v in rows])
    return sp.csr_array((data, indices, indptr), shape=(n, n))


def convdiff(mx, my, c=3.0):
    """the upwind convection-diffusion operator of the benchmark's AIR workload"""
    Dx = sp.diags_array([np.ones(mx), -np.ones(mx - 1)], offsets=[0, -1], shape=(mx, mx))
    Dy = sp.diags_array([2 * np.ones(my), -np.ones(my - 1), -np.ones(my - 1)], offsets=[0, -1, 1], shape=(my, my))
    A = sp.csr_array(c * sp.kron(sp.eye_array(my), Dx) + sp.kron(Dy, sp.eye_array(mx)))
    A.sort_indices()
    return sp.csr_array((A.data, A.indices.astype(np.int32), A.indptr.astype(np.int32)), shape=A.shape)


def unsorted(A):
    return any(np.any(np.diff(A.indices[a:b]) < 0) for a, b in zip(A.indptr[:-1], A.indptr[1:]))


def air_case(out, sizes, name, op, A, splitting, theta, norm, degree):
    """the steps of interpolate.py:324-426 one by one, so that R is seen before eliminate_zeros; returns the raw R"""
    A = sp.csr_array(A)
    splitting = np.asarray(splitting, dtype=np.int32)
    assert A.shape[0] <= 300 and A.indptr.dtype == np.int32
    C = ref_strength(A=A, theta=theta, block=False, norm=norm)
    Cpts = np.array(np.where(splitting == 1)[0], dtype=A.indptr.dtype)
    nc = Cpts.shape[0]
    Rp = np.empty(nc + 1, dtype=A.indptr.dtype)
    ref_core.approx_ideal_restriction_pass1(Rp, C.indptr, C.indices, Cpts, splitting, degree)
    nnz = Rp[-1]
    Rj = np.zeros(nnz, dtype=A.indptr.dtype)
    Rx = np.zeros(nnz, dtype=A.dtype)
    ref_core.approx_ideal_restriction_pass2(Rp, Rj, Rx, A.indptr, A.indices, A.data, C.indptr, C.indices, C.data, Cpts, splitting, degree, False,
                                            10, True)
    raw = sp.csr_array((Rx.copy(), Rj.copy(), Rp.copy()), shape=[nc, A.shape[0]])
    R = sp.csr_array(ri.local_air(A.copy(), splitting.copy(), theta=theta, norm=norm, degree=degree))
    fin = raw.copy()
    fin.eliminate_zeros()
    assert np.array_equal(fin.indptr, R.indptr) and np.array_equal(fin.indices, R.indices) and np.array_equal(fin.data, R.data)
    assert np.all(np.isfinite(raw.data)), name
    for r in range(nc):                                     # ascending and unique, the identity entry last
        row = Rj[Rp[r]:Rp[r + 1]]
        assert row[-1] == Cpts[r] and Rx[Rp[r + 1] - 1] == 1.0 and np.all(np.diff(row[:-1]) > 0)
    out[f"air.{name}.op"] = np.array(op)
    out[f"air.{name}.splitting"] = splitting
    out[f"air.{name}.theta"] = np.float64(theta)
    out[f"air.{name}.norm"] = np.array(norm)
    out[f"air.{name}.degree"] = np.int64(degree)
    out[f"air.{name}.Rp"] = np.asarray(Rp, dtype=np.int32)
    put(out, f"air.{name}.Rraw", raw)
    put(out, f"air.{name}.R", R)
    sizes[name] = np.diff(Rp) - 1
    return raw


def householder_norms(M):
    """normx of every step of the reference's QR (linalg.h:1197-1260) on the column-major system M, in plain NumPy"""
    M = M.copy()
    n = M.shape[0]
    norms = []
    for j in range(n):
        normx = np.sqrt(np.sum(M[j:, j] ** 2))
        norms.append(normx)
        if normx < 1e-12:
            continue
        normx *= -1.0 if M[j, j] >= 0 else 1.0
        scale = M[j, j] - normx
        tau = -scale / normx
        v = M[j:, j] / scale
        v[0] = 1.0
        M[j:, j:] -= tau * np.outer(v, v @ M[j:, j:])
    return np.array(norms)


def singular():
    rows = [([0, 2, 3, 4, 6], [4.0, -1.0, -1.0, -1.0, 0.0]),          # C; a stored explicit zero a_06
            ([1], [1.0]),                                              # C without any strong F-neighbour
            ([0, 2, 3, 6], [-1.0, 3.0, -1.0, -1.0]),                   # F
            ([2, 3, 6, 7], [3.0, -1.0, -1.0, -1.0]),                   # F with the row of node 2 inside the neighbourhood
            ([4, 0, 1], [0.0, -1.0, -1.0]),                            # F: stored zero diagonal, nothing inside the neighbourhood
            ([5, 7], [2.0, -1.0]),                                     # F, not strongly connected to node 0
            ([6, 2, 0], [2.0, -1.0, -0.5]),                            # F at distance 2
            ([7, 5, 3], [3.0, -1.0, -1.0])]                            # C
    return raw_csr(rows, 8), np.array([1, 1, 0, 0, 0, 0, 0, 1], dtype=np.int32)


def onept_case(out, name, A, C, splitting):
    A, C = sp.csr_array(A), sp.csr_array(C)
    splitting = np.asarray(splitting, dtype=np.int32)
    n = A.shape[0]
    put(out, f"onept.{name}.A", A); put(out, f"onept.{name}.C", C)
    out[f"onept.{name}.splitting"] = splitting
    out[f"onept.{name}.nc"] = np.int64(splitting.sum())
    res = {}
    for by_val in (False, True):
        P = sp.csr_array(ri.one_point_interpolation(A.copy(), C.copy(), splitting.copy(), by_val=by_val))
        assert P.shape == (n, splitting.sum())
        M = A if by_val else C
        # the amg_core routine on a value array that starts as ones: it leaves the C-rows' values alone (air.h:70-73)
        Pp, Pj, Px = np.empty(n + 1, dtype=np.int32), np.empty(n, dtype=np.int32), np.ones(n)
        ref_core.one_point_interpolation(Pp, Pj, Px, M.indptr, M.indices, M.data, splitting)
        nnz = Pp[-1]
        frow = np.repeat(splitting == 0, np.diff(Pp))
        assert np.array_equal(Pp, P.indptr) and np.array_equal(Pj[:nnz], P.indices[:nnz])
        data = Px[:nnz].copy() if by_val else np.ones(nnz)
        assert np.array_equal(data[frow], P.data[:nnz][frow]) and np.all(data[~frow] == 1.0)
        if not by_val:
            assert np.array_equal(data, P.data[:nnz])
        key = f"onept.{name}.P{int(by_val)}"
        out[key + ".indptr"], out[key + ".indices"], out[key + ".data"] = Pp.copy(), Pj[:nnz].copy(), data
        res[by_val] = (Pp.copy(), Pj[:nnz].copy(), data)
    return res


def mixed48():
    rng = np.random.RandomState(SEED + 5)
    n = 48
    splitting = (rng.rand(n) < 0.4).astype(np.int32)
    splitting[:4] = [0, 0, 1, 1]
    cpts, fpts = np.where(splitting == 1)[0], np.where(splitting == 0)[0]
    rowsA, rowsC = [], []
    for i in range(n):
        k = rng.randint(2, 7)
        cols = rng.choice(np.delete(np.arange(n), i), size=k, replace=False)
        if i in (0, 10, 20) or (splitting[i] == 0 and i % 9 == 4):
            cols = rng.choice(fpts[fpts != i], size=3, replace=False)        # an F-row (0, ...) without any C-neighbour
        elif i % 3 == 1:
            cols = np.concatenate([rng.choice(cpts[cpts != i], size=3, replace=False), rng.choice(fpts[fpts != i], size=2, replace=False)])
        vals = rng.choice([-1.0, 1.0], size=len(cols)) * (rng.rand(len(cols)) + 0.1)
        if i % 3 == 1:
            vals = np.sign(vals) * 0.5                                       # ties in |.|, of both signs
        cols, vals = np.concatenate([cols, [i]]), np.concatenate([vals, [3.0]])   # the diagonal is kept
        perm = rng.permutation(len(cols))
        rowsA.append((cols[perm], vals[perm]))
        perm = rng.permutation(len(cols))                                    # C: the same pattern in another order, other values
        cv = np.abs(vals[perm]) * rng.choice([-1.0, 1.0], size=len(cols))
        if i % 3 == 1:
            cv = np.sign(cv) * 0.25
        rowsC.append((cols[perm], cv))
    return raw_csr(rowsA, n), raw_csr(rowsC, n), splitting


def main():
    out, sizes = {}, {}
    ops = {}
    # ---------------------------------------------------------------- local_air
    ops["line5"] = sp.csr_array(poisson((5,), format="csr"))
    raw = air_case(out, sizes, "line5", "line5", ops["line5"], [1, 0, 1, 0, 1], 0.1, "abs", 1)
    fin = sp.csr_array((out["air.line5.R.data"], out["air.line5.R.indices"], out["air.line5.R.indptr"]), shape=(3, 5))
    assert np.array_equal(fin.toarray(), [[1, 0.5, 0, 0, 0], [0, 0.5, 1, 0.5, 0], [0, 0, 0, 0.5, 1]])       # interpolate.py:371-374
    ops["convdiff13x11"] = A = convdiff(13, 11)
    assert (A - A.T).nnz > 0
    split_cd = np.asarray(rs.RS(ref_strength(A, theta=0.3, norm="min"), second_pass=True), dtype=np.int32)
    for degree in (1, 2):
        for k, (theta, norm) in enumerate(((0.05, "abs"), (0.3, "min"))):
            air_case(out, sizes, f"convdiff13x11.d{degree}.t{k}", "convdiff13x11", A, split_cd, theta, norm, degree)
    st = -np.ones((3, 3, 3)); st[1, 1, 1] = 26.0
    ops["box6x5x4"] = A = sp.csr_array(stencil_grid(st, (6, 5, 4), format="csr"))
    np.random.seed(SEED + 1)
    split_box = np.asarray(rs.PMIS(ref_strength(A, theta=0.25)), dtype=np.int32)
    air_case(out, sizes, "box6x5x4", "box6x5x4", A, split_box, 0.25, "abs", 2)
    air_case(out, sizes, "box6x5x4.d1", "box6x5x4", A, split_box, 0.25, "abs", 1)        # (the 9-16 class)
    assert np.all(sizes["box6x5x4"] > sizes["box6x5x4.d1"])                  # distance 2 adds F-F neighbours
    # hub: node 0 (C) with the F-neighbours 1..100, a chain behind them, non-symmetric values
    rng = np.random.RandomState(SEED + 2)
    n = 131
    r_, c_ = [], []
    for j in range(1, 101):
        r_ += [0, j]; c_ += [j, 0]
    for j in range(1, n - 1):
        r_ += [j, j + 1]; c_ += [j + 1, j]
    G = sp.coo_array((-(0.5 + rng.rand(len(r_))), (r_, c_)), shape=(n, n)).tocsr()
    A = sp.csr_array(G + sp.diags_array(-G.sum(axis=1) + 0.5))
    ops["hub"] = A = sp.csr_array((A.data, A.indices.astype(np.int32), A.indptr.astype(np.int32)), shape=A.shape)
    split_hub = np.zeros(n, dtype=np.int32)
    split_hub[0] = 1
    split_hub[103::2] = 1
    for degree in (1, 2):
        air_case(out, sizes, f"hub.d{degree}", "hub", A, split_hub, 0.0, "abs", degree)
    assert sizes["hub.d1"][0] == 100 and sizes["hub.d2"][0] == 101           # the chain behind the hub's neighbours
    # level1: the level-1 operator of a reference AIR hierarchy
    np.random.seed(SEED + 3)
    ml = pyamg.air_solver(convdiff(24, 20), max_levels=3, max_coarse=5)
    A1 = sp.csr_array(ml.levels[1].A)
    ops["level1"] = A1 = sp.csr_array((A1.data, A1.indices.astype(np.int32), A1.indptr.astype(np.int32)), shape=A1.shape)
    assert unsorted(A1) and A1.shape[0] <= 300
    split_l1 = np.asarray(rs.RS(ref_strength(A1, theta=0.3, norm="min"), second_pass=True), dtype=np.int32)
    air_case(out, sizes, "level1", "level1", A1, split_l1, 0.05, "abs", 2)
    air_case({}, sizes, "level1.d1", "level1", A1, split_l1, 0.05, "abs", 1)
    assert np.any(sizes["level1"] > sizes.pop("level1.d1"))
    # singular
    ops["singular"], split_s = singular()
    raw = air_case(out, sizes, "singular", "singular", ops["singular"], split_s, 0.0, "abs", 2)
    A = ops["singular"]
    Nf = raw.indices[raw.indptr[0]:raw.indptr[1] - 1]
    assert list(Nf) == [2, 3, 4, 6] and list(sizes["singular"]) == [4, 0, 4]
    Ad = A.toarray()
    M = Ad[np.ix_(Nf, Nf)].T
    norms = householder_norms(M)
    col0 = np.linalg.norm(M, axis=0)
    assert col0[2] == 0.0 and norms[2] == 0.0                                # an all-zero column: skipped
    assert col0[1] >= 1.0 and norms[1] < 1e-12                               # negligible only after the first reflection: skipped
    assert norms[0] > 1.0 and norms[3] > 1e-3
    assert A.data[A.indptr[0]:A.indptr[1]][list(A.indices[A.indptr[0]:A.indptr[1]]).index(6)] == 0.0      # the stored a_06
    x = raw.data[raw.indptr[0]:raw.indptr[1] - 1]
    assert np.sum(x == 0.0) >= 2 and x[0] != 0.0                             # the zero-pivot rule
    assert out["air.singular.R.indptr"][1] == raw.indptr[1] - np.sum(x == 0.0)       # ... and eliminate_zeros removes them
    # the size classes of the lane groups, over all cases
    allN = np.concatenate(list(sizes.values()))
    for lo, hi in ((0, 0), (1, 1), (2, 8), (9, 16), (17, 32), (33, 64), (65, 10 ** 6)):
        assert np.any((allN >= lo) & (allN <= hi)), (lo, hi)
    boxN = sizes["box6x5x4"]
    assert np.any(boxN > 16) and np.any(boxN > 32)
    out["air.names"] = np.array(sorted(sizes))
    out["air.ops"] = np.array(sorted(ops))
    for name, A in ops.items():
        put(out, f"air.{name}.A", A)
    # ---------------------------------------------------------------- one_point_interpolation
    names = []
    A = sp.csr_array(poisson((5,), format="csr"))
    res = onept_case(out, "line5", A, A, [1, 0, 1, 0, 1]); names.append("line5")
    Pp, Pj, Px = res[False]
    assert np.array_equal(sp.csr_array((Px, Pj, Pp), shape=(5, 3)).toarray(), [[1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 1, 0], [0, 0, 1]])  # :275-279
    A = ops["convdiff13x11"]
    C = ref_strength(A, theta=0.3, norm="min")
    assert np.all(C.diagonal() != 0)                                          # C keeps its diagonal
    onept_case(out, "convdiff", A, C, split_cd); names.append("convdiff")
    A, C, s = mixed48()
    res = onept_case(out, "mixed48", A, C, s); names.append("mixed48")
    assert unsorted(A) and unsorted(C)
    for by_val, M in ((False, C), (True, A)):
        Pp, Pj, Px = res[by_val]
        empty = (np.diff(Pp) == 0)
        assert np.all(s[empty] == 0) and empty.sum() >= 3 and empty[0]        # F-rows without a C-neighbour
        ties = 0
        for i in np.where((s == 0) & ~empty)[0]:
            cols, vals = M.indices[M.indptr[i]:M.indptr[i + 1]], M.data[M.indptr[i]:M.indptr[i + 1]]
            isC = s[cols] == 1
            best = np.abs(vals[isC]).max()
            ties += np.sum(np.abs(vals[isC]) == best) > 1
        assert ties >= 3
        if by_val:
            fvals = Px[np.repeat(s == 0, np.diff(Pp))]
            assert np.any(fvals > 0) and np.any(fvals < 0)                    # -val of negative and positive entries
    out["onept.names"] = np.array(names)
    # ---------------------------------------------------------------- end to end
    A = convdiff(17, 13)
    put(out, "e2e.A", A)
    for cf, CF in (("rs", None), ("pmis", "PMIS")):
        seed = SEED + 40
        np.random.seed(seed)
        ml = pyamg.air_solver(A.copy(), max_coarse=20) if CF is None else pyamg.air_solver(A.copy(), CF=CF, max_coarse=20)
        assert len(ml.levels) >= 3, (cf, len(ml.levels))
        out[f"e2e.{cf}.seed"] = np.int64(seed)
        out[f"e2e.{cf}.sizes"] = np.array([lv.A.shape[0] for lv in ml.levels], dtype=np.int64)
        for lvl in range(3):
            put(out, f"e2e.{cf}.A{lvl}", ml.levels[lvl].A)
        for lvl in range(2):
            put(out, f"e2e.{cf}.P{lvl}", ml.levels[lvl].P)
            put(out, f"e2e.{cf}.R{lvl}", ml.levels[lvl].R)
            out[f"e2e.{cf}.P{lvl}.shape"] = np.array(ml.levels[lvl].P.shape, dtype=np.int64)
    np.savez_compressed(OUT, **out)
    size = OUT.stat().st_size
    assert size < (1 << 19), size
    print(f"{OUT.name}: {len(out)} arrays, {size} bytes")
    print({k: (int(v.min()), int(v.max())) for k, v in sizes.items()})


if __name__ == "__main__":
    main()
