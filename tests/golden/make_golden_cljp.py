#!/usr/bin/env python3
"""Generate tests/golden/kernels_cljp.npz: patterns and the reference's own outputs for the CLJP / CLJP-c coarse-grid selection and the
MIS vertex colouring.

Run in the build container (needs the reference built into oracle/_ref by oracle/build_ref.py):
    python tests/golden/make_golden_cljp.py

Keys (patterns are ``<prefix>.indptr / .indices``; ``cljp.names`` lists the patterns, ``col.names`` those with a colouring):

  cljp.<g>.S (pattern) / .cljp / .cljpc      the reference's CLJP(S) and CLJPc(S)
      grid17x13    strength pattern of the 5-point Laplacian, with its diagonal
      box6x5x4     strength pattern of the 27-point operator
      irr200       non-symmetric, unsorted, nodes without any entry and nodes with nothing but a diagonal
      irr200_sym   its symmetrised pattern
      hub          one row of 100 off-diagonals whose node stands in 50 other rows: beyond the 64-lane size class
      path300      a path stored in index order: the deepest colouring chain
      n1           a single node
      nonsym_ties  a small non-symmetric pattern on which CLJP-c's colour weights tie between adjacent nodes, so that two adjacent nodes
                   are selected in one pass (asserted below from the reference's colouring)
  col.<g>.coloring                           vertex_coloring(G, 'MIS') for the symmetric patterns and for irr200
  rand.head                                  the first 16 values of rand() after srand(2448422) from this machine's C library
  e2e.A, e2e.<CF>.P0 / .A1                   ruge_stuben_solver(A, CF=<CF>, max_levels=3) of the 17 x 13 grid for CF = CLJP, CLJPc: the
                                             first prolongator and the level-1 operator
"""
import ctypes
import ctypes.util
import sys
from pathlib import Path

import numpy as np
import scipy.sparse as sp

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE))

import oracle.refimport  # noqa: E402,F401
import pyamg  # noqa: E402
from pyamg import amg_core as ref_core  # noqa: E402
from pyamg.classical import split as rs  # noqa: E402
from pyamg.gallery import poisson, stencil_grid  # noqa: E402
from pyamg.graph import vertex_coloring as ref_coloring  # noqa: E402
from pyamg.strength import classical_strength_of_connection as ref_strength  # noqa: E402
from make_golden_classical import irr200, put, raw_csr, sym_pattern  # noqa: E402

SEED = 20261020
OUT = HERE / "kernels_cljp.npz"
LIMIT = (HERE / "kernels_classical.npz").stat().st_size


def hub():
    n, rows = 131, []
    for i in range(n):
        cols = list(range(1, 101)) if i == 0 else [c for c in (i - 1, i + 1) if 1 <= c < n]
        if 1 <= i <= 50:
            cols.append(0)
        rows.append((cols, np.ones(len(cols))))
    S = raw_csr(rows, n)
    assert S.indptr[1] == 100 and np.sum(S.indices == 0) == 50
    return S


def first_pass_ties(S):
    """CLJP-c's first pass, from the reference's colouring of S: True when two adjacent nodes are selected together"""
    n = S.shape[0]
    S = sp.csr_array(rs.remove_diagonal(S))
    coloring = np.empty(n, dtype="intc")
    ref_core.vertex_coloring_mis(n, S.indptr, S.indices, coloring)
    w = coloring / float(coloring.max() + 1)
    for j in S.indices:
        w[j] += 1.0
    G = sp.coo_array(S + S.T)
    beaten = np.zeros(n, dtype=bool)
    beaten[G.row[w[G.col] > w[G.row]]] = True
    return bool(np.any(~beaten[G.row] & ~beaten[G.col]))


def nonsym_ties():
    rng = np.random.RandomState(SEED)
    for _ in range(2000):
        n = 12
        rows = []
        for i in range(n):
            cols = rng.choice(np.delete(np.arange(n), i), size=rng.randint(0, 4), replace=False)
            rows.append((cols, np.ones(len(cols))))
        S = raw_csr(rows, n)
        if abs(S - S.T).nnz and first_pass_ties(S):
            return S
    raise AssertionError("no tie pattern found")


def main():
    out = {}
    Sg = ref_strength(sp.csr_array(poisson((17, 13), format="csr")), theta=0.25)
    st = -np.ones((3, 3, 3)); st[1, 1, 1] = 26.0
    Sb = ref_strength(sp.csr_array(stencil_grid(st, (6, 5, 4), format="csr")), theta=0.25)
    Si = irr200()
    path = sp.csr_array(sp.diags_array([np.ones(299), np.ones(299)], offsets=[-1, 1], format="csr"))
    cases = {"grid17x13": Sg, "box6x5x4": Sb, "irr200": Si, "irr200_sym": sym_pattern(Si), "hub": hub(), "path300": path,
             "n1": sp.csr_array(np.array([[1.0]])), "nonsym_ties": nonsym_ties()}
    assert Sg.diagonal().all() and not Si.has_sorted_indices and abs(Si - Si.T).nnz
    assert first_pass_ties(cases["nonsym_ties"])
    for name, S in cases.items():
        S = sp.csr_array(S)
        put(out, f"cljp.{name}.S", S, data=False)
        out[f"cljp.{name}.cljp"] = np.asarray(rs.CLJP(S.copy()), dtype=np.int32)
        out[f"cljp.{name}.cljpc"] = np.asarray(rs.CLJPc(S.copy()), dtype=np.int32)
    out["cljp.names"] = np.array(list(cases))
    coloured = [g for g, S in cases.items() if not abs(sp.csr_array(S) - sp.csr_array(S).T).nnz] + ["irr200"]
    assert {"grid17x13", "box6x5x4", "irr200_sym", "path300", "n1"} <= set(coloured)
    for name in coloured:
        out[f"col.{name}.coloring"] = np.asarray(ref_coloring(sp.csr_array(cases[name]).copy(), "MIS"), dtype=np.int32)
    out["col.names"] = np.array(coloured)
    libc = ctypes.CDLL(ctypes.util.find_library("c"))
    libc.srand(2448422)
    out["rand.head"] = np.array([libc.rand() for _ in range(16)], dtype=np.int64)
    # ---------------------------------------------------------------- end to end
    A = sp.csr_array(poisson((17, 13), format="csr"))
    put(out, "e2e.A", A)
    for CF in ("CLJP", "CLJPc"):
        ml = pyamg.ruge_stuben_solver(A.copy(), CF=CF, max_levels=3)
        assert len(ml.levels) == 3
        put(out, f"e2e.{CF}.P0", sp.csr_array(ml.levels[0].P)); out[f"e2e.{CF}.P0.nc"] = np.int64(ml.levels[0].P.shape[1])
        put(out, f"e2e.{CF}.A1", sp.csr_array(ml.levels[1].A))
    np.savez_compressed(OUT, **out)
    size = OUT.stat().st_size
    assert size <= LIMIT, (size, LIMIT)
    print(f"{OUT.name}: {len(out)} arrays, {size} bytes (limit {LIMIT})")


if __name__ == "__main__":
    main()
