#!/usr/bin/env python3
"""Generate tests/golden/kernels_distance.npz: inputs and the reference's own outputs for the relaxation-vector strength measures
(``algebraic_distance``, ``affinity_distance``) and for ``distance_strength_of_connection``.

Run in the build container (needs the reference built into oracle/_ref by oracle/build_ref.py):
    python tests/golden/make_golden_distance.py

Data only, at most 512 KiB.  Keys (CSR triples are ``<prefix>.indptr / .indices / .data``):

  op.<name>                          the operators of distance_cases.OPERATORS, each with at most 300 rows
      poisson12x11   the five-point Laplacian
      aniso10x9      rotated anisotropic diffusion (epsilon = 0.001, theta = pi / 3), nine-point
      rand97         seeded, non-symmetric: row lengths 0 to 12, an empty row, a row without a stored diagonal
      arrow130       a dense first row and a dense first column: a row longer than two waves
      zeros7x5       the five-point Laplacian with stored zeros: off the diagonal, and on it (a row that keeps its values)
  case.<i>.x0 / .x / .d / .kept / .C (+ .C.index_dtype)     for distance_cases.CASES[i] = (operator, measure, R, k, epsilon, alpha):
      the drawn block ``np.random.rand(n * R) - 0.5`` after ``np.random.seed(case.seeds[i])`` (flat, column after column), the block after
      relaxation (the same layout), the per-entry distances on A's pattern with 0.0 on the diagonal and on stored zeros, the positions
      in A's pattern that apply_distance_filter and eliminate_zeros keep, and the final strength matrix
  vd.<case>.A (CSR, or .A.bsr_data / .indices / .indptr) / .V / .Cx / .C     distance_strength_of_connection for distance_cases.VERTEX;
      .Cx are the distances as the filter receives them (absent for theta = inf, where the reference calls none)
      grid2d*      poisson12x11 with its grid coordinates
      line1d_abs   rand97 with one seeded coordinate
      cloud3d*     aniso10x9 with seeded 3-D coordinates, two neighbouring vertices coincident (the 1e-6 clamp)
      elas_bsr     2-D linear elasticity on a 6 x 6 grid, BSR with 2 x 2 blocks: the supernode pattern
  err.names / .types / .msgs           what the reference raises for distance_cases.BAD, in their order
  warn.dense                           the category and text of the warning for a dense operator
"""
import sys
import warnings
from pathlib import Path

import numpy as np
import scipy.sparse as sp

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

import oracle.refimport  # noqa: E402,F401
import pyamg  # noqa: E402,F401
import pyamg.strength as rstr  # noqa: E402
from pyamg import amg_core as rcore  # noqa: E402
from pyamg.gallery import linear_elasticity, poisson, stencil_grid  # noqa: E402
from pyamg.gallery.diffusion import diffusion_stencil_2d  # noqa: E402

import distance_cases as dc  # noqa: E402

SEED = 20261020
OUT = HERE / "kernels_distance.npz"
LIMIT = 512 * 1024


def put(out, prefix, M, dtype_too=False):
    out[prefix + ".indptr"] = np.asarray(M.indptr, dtype=np.int32)
    out[prefix + ".indices"] = np.asarray(M.indices, dtype=np.int32)
    out[prefix + ".data"] = np.asarray(M.data, dtype=np.float64)
    if dtype_too:
        out[prefix + ".index_dtype"] = np.array(M.indptr.dtype.name)


def operators():
    ops = {}
    ops["poisson12x11"] = sp.csr_array(poisson((12, 11), format="csr"))
    sten = diffusion_stencil_2d(epsilon=0.001, theta=np.pi / 3, type="FD")
    ops["aniso10x9"] = sp.csr_array(stencil_grid(sten, (10, 9), format="csr"))
    rng = np.random.RandomState(SEED)
    n = 97
    rows, cols = [], []
    lengths = rng.randint(1, 13, n)
    lengths[50] = 0                                          # an empty row
    for i, m in enumerate(lengths):
        pool = np.delete(np.arange(n), i)
        c = list(rng.choice(pool, size=max(m - 1, 0), replace=False))
        if m and i != 31:                                    # row 31 has no stored diagonal
            c.append(i)
        rows += [i] * len(c); cols += sorted(c)
    vals = rng.randn(len(rows))
    vals[np.asarray(rows) == np.asarray(cols)] = 3.0 + rng.rand(int(np.sum(np.asarray(rows) == np.asarray(cols))))
    A = sp.coo_array((vals, (rows, cols)), shape=(n, n)).tocsr()
    A.sort_indices()
    assert np.diff(A.indptr)[50] == 0 and A.diagonal()[31] == 0 and abs(A - A.T).max() > 0.1
    ops["rand97"] = A
    n = 130
    rows = [0] * n + list(range(1, n)) + list(range(1, n))
    cols = list(range(n)) + [0] * (n - 1) + list(range(1, n))
    vals = -(rng.rand(len(rows)) + 0.1)
    vals[np.asarray(rows) == np.asarray(cols)] = 4.0 + rng.rand(n)
    A = sp.coo_array((vals, (rows, cols)), shape=(n, n)).tocsr()
    A.sort_indices()
    assert A.indptr[1] > 128
    ops["arrow130"] = A
    A = sp.csr_array(poisson((7, 5), format="csr"))
    for r in (2, 9, 20):                                     # stored zeros off the diagonal ...
        assert A.indices[A.indptr[r]] != r
        A.data[A.indptr[r]] = 0.0
    i = 17
    A.data[A.indptr[i] + int(np.flatnonzero(A.indices[A.indptr[i]:A.indptr[i + 1]] == i)[0])] = 0.0      # ... and a stored zero diagonal
    assert A.nnz == sp.csr_array(poisson((7, 5), format="csr")).nnz and (A.data == 0).sum() >= 3 and A.diagonal()[17] == 0.0
    ops["zeros7x5"] = A
    for name, A in ops.items():
        A = ops[name] = sp.csr_array((A.data, A.indices.astype(np.int32), A.indptr.astype(np.int32)), shape=A.shape)     # as the fixture stores them
        assert A.shape[0] <= 300 and A.has_canonical_format and A.dtype == np.float64, name
    assert list(ops) == dc.OPERATORS
    return ops


def check_coverage():
    for m in dc.MEASURES:
        mine = [c for c in dc.CASES if c[1] == m]
        assert {c[0] for c in mine} == set(dc.OPERATORS), m
        assert {c[2] for c in mine} == {1, 5, 7, 8, 9, 17, 32}, m
        assert {c[3] for c in mine} == {1, 2, 20}, m
        assert {c[4] for c in mine} == {1.0, 2.0, 4.0}, m
        assert {c[5] for c in mine} == {0.0, 0.5, 0.7}, m
    for o in dc.OPERATORS:
        mine = [c for c in dc.CASES if c[0] == o]
        assert {c[3] for c in mine} == {1, 2, 20}, o
        assert {c[4] for c in mine} == {1.0, 2.0, 4.0}, o
        assert {c[5] for c in mine} == {0.0, 0.5, 0.7}, o


class Recorder:
    """wraps one amg_core function of the reference's strength module: the arguments as they go in, and as they come out"""

    def __init__(self, name):
        self.name, self.calls = name, []
        self.fn = getattr(rcore, name)

    def __call__(self, *a):
        before = [np.array(x, copy=True) if isinstance(x, np.ndarray) else x for x in a]
        self.fn(*a)
        self.calls.append((before, [np.array(x, copy=True) if isinstance(x, np.ndarray) else x for x in a]))


class patched:
    """the reference's strength module with recording amg_core filters and, where asked for, a distance_measure_common that records the
    relaxed block and the distances its function returns"""

    def __init__(self, filters, seen=None):
        self.filters, self.seen = filters, seen

    def __enter__(self):
        self.old_core, self.old_common = rstr.amg_core, rstr.distance_measure_common
        ns = type("core", (), {})()
        for n in dir(rcore):
            if not n.startswith("_"):
                setattr(ns, n, getattr(rcore, n))
        for n, r in self.filters.items():
            setattr(ns, n, r)
        rstr.amg_core = ns
        if self.seen is not None:
            def common(A, func, alpha, R, k, epsilon):
                def recording(x):
                    d = func(x)
                    self.seen["x"], self.seen["d"] = x.copy(order="F"), np.array(d, copy=True)
                    return d
                return self.old_common(A, recording, alpha, R, k, epsilon)
            rstr.distance_measure_common = common
        return self

    def __exit__(self, *exc):
        rstr.amg_core, rstr.distance_measure_common = self.old_core, self.old_common


def positions(A):
    """(row, column) -> position in A's stored pattern"""
    P = sp.csr_array((np.arange(1, A.nnz + 1, dtype=np.float64), A.indices, A.indptr), shape=A.shape)
    return P


def do_cases(out, ops):
    seeds = []
    counts = {"zero_distance": 0, "dropped": 0, "carried": 0}
    for i, (op, measure, R, k, eps, alpha) in enumerate(dc.CASES):
        A = ops[op]
        n = A.shape[0]
        seed = SEED + 100 + i
        seeds.append(seed)
        np.random.seed(seed)
        x0 = np.random.rand(n * R) - 0.5
        rec, seen = Recorder("apply_distance_filter"), {}
        Ain = A.copy()
        np.random.seed(seed)
        with patched({"apply_distance_filter": rec}, seen):
            if measure == "affinity":
                C = rstr.affinity_distance(Ain, alpha=alpha, R=R, k=k, epsilon=eps)
            else:
                C = rstr.algebraic_distance(Ain, alpha=alpha, R=R, k=k, epsilon=eps, p=dc.P_OF[measure])
        assert np.array_equal(Ain.data, A.data) and len(rec.calls) == 1
        after = np.random.get_state()
        np.random.seed(seed)
        np.random.rand(n * R)
        assert np.array_equal(after[1], np.random.get_state()[1]) and after[2] == np.random.get_state()[2]
        x = seen["x"]                                        # n x R
        p = f"case.{i}"
        out[p + ".x0"] = x0
        out[p + ".x"] = np.ascontiguousarray(x.T).reshape(-1)
        # the distances on A's pattern: A.nonzero() keeps the stored order and drops stored zeros
        stored = A.data != 0
        rows = np.repeat(np.arange(n), np.diff(A.indptr))
        assert seen["d"].shape == (int(stored.sum()),)
        d = np.zeros(A.nnz)
        d[stored] = seen["d"]
        d[rows == A.indices] = 0.0
        out[p + ".d"] = d
        (_, _, sp_, sj, _), (_, _, _, _, sx_out) = rec.calls[0]
        F = sp.csr_array((sx_out, sj, sp_), shape=A.shape)
        F.eliminate_zeros()
        P = positions(A)
        frows = np.repeat(np.arange(n), np.diff(F.indptr))
        kept = np.asarray(P[frows, F.indices]).ravel().astype(np.int64) - 1 if F.nnz else np.zeros(0, dtype=np.int64)
        assert np.all(kept >= 0) and np.array_equal(d[kept], F.data) and np.all(np.diff(kept) > 0)
        out[p + ".kept"] = kept
        C = sp.csr_array(C)
        put(out, p + ".C", C, dtype_too=True)
        off = (rows != A.indices) & stored
        counts["zero_distance"] += int((d[off] == 0).sum())
        counts["dropped"] += int(off.sum() - (d[off] == 0).sum() - kept.size)
        carried = np.flatnonzero(A.diagonal() == 0)
        if carried.size:
            assert np.array_equal(x[carried], np.reshape(x0, (n, R), order="F")[carried])       # those rows keep their values
            counts["carried"] += carried.size
        print(dc.IDS[i], "nnz", A.nnz, "kept", kept.size, "C.nnz", C.nnz)
    print(counts)
    assert counts["zero_distance"] > 0 and counts["dropped"] > 0 and counts["carried"] > 0
    out["case.seeds"] = np.array(seeds, dtype=np.int64)


def vertex_cases(ops):
    rng = np.random.RandomState(SEED + 7)
    cases = {}
    ii, jj = np.divmod(np.arange(132), 11)
    grid = np.ascontiguousarray(np.stack([jj * 1.0, ii * 1.5], axis=1))
    cases["grid2d"] = (ops["poisson12x11"], grid)
    cases["grid2d_abs"] = (ops["poisson12x11"], grid)
    cases["line1d_abs"] = (ops["rand97"], rng.rand(97, 1))
    cloud = rng.rand(90, 3)
    cloud[41] = cloud[40]                                    # two neighbouring vertices coincide
    for name in ("cloud3d", "cloud3d_inf", "cloud3d_abs"):
        cases[name] = (ops["aniso10x9"], cloud)
    Ae, _ = linear_elasticity((6, 6), format="bsr")
    Ae = sp.bsr_array(Ae)
    assert Ae.blocksize == (2, 2)
    cases["elas_bsr"] = (Ae, rng.rand(36, 2))
    return cases


def do_vertex(out, ops):
    cases = vertex_cases(ops)
    clamped = 0
    for name, theta, relative in dc.VERTEX:
        A, V = cases[name]
        p = f"vd.{name}"
        if A.format == "bsr":
            out[p + ".A.bsr_data"], out[p + ".A.indices"], out[p + ".A.indptr"] = A.data.copy(), A.indices.astype(np.int32), A.indptr.astype(np.int32)
        else:
            put(out, p + ".A", A)
        out[p + ".V"] = V.copy()
        recs = {n: Recorder(n) for n in ("apply_distance_filter", "apply_absolute_distance_filter")}
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            with patched(recs):
                C = sp.csr_array(rstr.distance_strength_of_connection(A.copy(), V.copy(), theta=theta, relative_drop=relative))
        calls = recs["apply_distance_filter"].calls + recs["apply_absolute_distance_filter"].calls
        assert len(calls) == (0 if theta == np.inf else 1)
        assert len(recs["apply_distance_filter"].calls) == (1 if relative and theta != np.inf else 0)
        if calls:
            out[p + ".Cx"] = calls[0][0][4]
            clamped += int((calls[0][0][4] == 1e-6).sum())
        put(out, p + ".C", C, dtype_too=True)
        print(p, "dim", V.shape[1], "C.nnz", C.nnz)
    assert clamped > 90                                      # the diagonals, and the coincident pair


def do_errors(out):
    types, msgs = [], []
    for name, fn, kw in dc.BAD:
        try:
            getattr(rstr, fn)(dc._small(), **kw)
            raise AssertionError(f"the reference accepts {name}")
        except AssertionError:
            raise
        except Exception as e:      # noqa: BLE001
            types.append(type(e).__name__); msgs.append(str(e))
    out["err.names"] = np.array([n for n, _, _ in dc.BAD])
    out["err.types"], out["err.msgs"] = np.array(types), np.array(msgs)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        rstr.distance_strength_of_connection(dc._small().toarray(), np.arange(6.0).reshape(6, 1))
    assert len(w) == 1
    out["warn.dense"] = np.array([w[0].category.__name__, str(w[0].message)])


def main():
    check_coverage()
    out = {}
    ops = operators()
    for name, A in ops.items():
        put(out, f"op.{name}", A)
    do_cases(out, ops)
    do_vertex(out, ops)
    do_errors(out)
    np.savez_compressed(OUT, **out)
    size = OUT.stat().st_size
    assert size <= LIMIT, size
    print(f"{OUT.name}: {len(out)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
