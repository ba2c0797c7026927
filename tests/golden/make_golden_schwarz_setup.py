#!/usr/bin/env python3
"""Generate tests/golden/kernels_schwarz_setup.npz: inputs and the reference's own outputs for the setup of overlapping Schwarz
-- ``amg_core.extract_subblocks`` (the dense diagonal block of every subdomain) and ``relaxation.schwarz_parameters`` (the blocks
inverted by LAPACK's gelss with the reference's rank tolerance).

Run in the build container (needs the reference built into oracle/_ref by oracle/build_ref.py):
    python tests/golden/make_golden_schwarz_setup.py

Cases (keys ``<case>.{indptr,indices,data,sub,sptr,tptr,blocks}`` and, where the blocks are inverted, ``.inv`` / ``.iptr``):

  chain_<dtype>    1-D Neumann Laplacian chains of length 1, 2, 8, 9, 16, 17, 32, 33, 64 (every edge of the device's size classes) as
                   the disconnected components of one matrix, one subdomain per component: every block singular, rank m - 1, the
                   length-1 block is [0].  The smallest kept singular value of the longest chain is 5 x above the float32 rank
                   threshold (10^6 x above the float64 one), the dropped one is at rounding level.
  chainp_<dtype>   the same chains + 0.1 I (nonsingular)
  dup              a small nonsymmetric operator whose rows were filled unsorted, then sorted, with rows that store one column twice
                   (extraction only: the first stored entry is the one the reference copies)
  part             subdomains that are not row patterns: every third row's pattern united with its neighbour's, on a nonsymmetric
                   operator with a 5-point pattern (the [lowest, highest] range of every subdomain contains columns that are not members)
"""
import sys
from pathlib import Path

import numpy as np
import scipy.sparse as sp

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

import oracle.refimport  # noqa: E402,F401
import pyamg  # noqa: E402
from pyamg import amg_core  # noqa: E402
from pyamg.relaxation import relaxation as rr  # noqa: E402

SEED = 20261018
CHAINS = (1, 2, 8, 9, 16, 17, 32, 33, 64)


def chain_matrix(shift, dtype):
    Ap, Aj, Ax, Sp, Sj = [0], [], [], [0], []
    n = 0
    for L in CHAINS:
        for i in range(L):
            deg = (i > 0) + (i + 1 < L)
            if i > 0:
                Aj.append(n + i - 1); Ax.append(-1.0)
            Aj.append(n + i); Ax.append(deg + shift)                 # (an explicit zero on the length-1 chain)
            if i + 1 < L:
                Aj.append(n + i + 1); Ax.append(-1.0)
            Ap.append(len(Aj))
            Sj.append(n + i)
        n += L
        Sp.append(len(Sj))
    A = sp.csr_array((np.array(Ax, dtype=dtype), np.array(Aj, dtype=np.int32), np.array(Ap, dtype=np.int32)), shape=(n, n))
    return A, np.array(Sj, dtype=np.int32), np.array(Sp, dtype=np.int32)


def duplicate_matrix(rng):
    n = 14
    Ap, Aj, Ax = [0], [], []
    for i in range(n):
        cols = list(rng.choice(n, size=rng.randint(2, 6), replace=False))
        if i not in cols:
            cols.append(i)
        if i % 3 == 0:                                   # one column stored twice (a second copy of a random member)
            cols.append(cols[rng.randint(len(cols))])
        if i == 6:
            cols += [i, i]                               # and the diagonal three times
        vals = rng.rand(len(cols)) + 0.5
        order = np.argsort(np.array(cols), kind="stable")              # filled unsorted, then sorted: duplicates keep their stored order
        Aj += list(np.array(cols)[order]); Ax += list(vals[order])
        Ap.append(len(Aj))
    A = sp.csr_array((np.array(Ax), np.array(Aj, dtype=np.int32), np.array(Ap, dtype=np.int32)), shape=(n, n))
    Sp, Sj = [0], []
    for i in range(n):
        Sj += list(np.unique(A.indices[A.indptr[i]:A.indptr[i + 1]]))
        Sp.append(len(Sj))
    return A, np.array(Sj, dtype=np.int32), np.array(Sp, dtype=np.int32)


def partial_matrix(rng):
    P = sp.csr_array(pyamg.gallery.poisson((11, 9), format="csr"))
    P.sort_indices()
    A = sp.csr_array((P.data + 0.3 * rng.rand(P.nnz), P.indices.astype(np.int32), P.indptr.astype(np.int32)), shape=P.shape)
    n = A.shape[0]
    Sp, Sj = [0], []
    for r in range(0, n - 1, 3):
        a = A.indices[A.indptr[r]:A.indptr[r + 1]]
        b = A.indices[A.indptr[r + 1]:A.indptr[r + 2]]
        Sj += list(np.union1d(a, b))
        Sp.append(len(Sj))
    return A, np.array(Sj, dtype=np.int32), np.array(Sp, dtype=np.int32)


def record(out, key, A, sub, sptr, invert):
    m = np.diff(sptr).astype(np.int64)
    tptr = np.zeros(len(sptr), dtype=np.int32)
    tptr[1:] = np.cumsum(m * m)
    blocks = np.full(int(tptr[-1]), np.nan, dtype=A.dtype)              # (the reference clears it)
    amg_core.extract_subblocks(A.indptr, A.indices, A.data, blocks, tptr, sub, sptr, len(sptr) - 1, A.shape[0])
    out[f"{key}.indptr"], out[f"{key}.indices"], out[f"{key}.data"] = A.indptr, A.indices, A.data
    out[f"{key}.sub"], out[f"{key}.sptr"], out[f"{key}.tptr"], out[f"{key}.blocks"] = sub, sptr, tptr, blocks
    if invert:
        B = sp.csr_array((A.data.copy(), A.indices.copy(), A.indptr.copy()), shape=A.shape)
        s2, p2, inv, iptr = rr.schwarz_parameters(B, subdomain=sub.copy(), subdomain_ptr=sptr.copy())
        assert np.array_equal(s2, sub) and np.array_equal(p2, sptr) and np.array_equal(iptr, tptr)
        out[f"{key}.inv"], out[f"{key}.iptr"] = inv, iptr


def main():
    rng = np.random.RandomState(SEED)
    out = {}
    for dt in (np.float64, np.float32):
        for tag, shift in (("chain", 0.0), ("chainp", 0.1)):
            A, sub, sptr = chain_matrix(shift, dt)
            record(out, f"{tag}_{np.dtype(dt).name}", A, sub, sptr, True)
    # the rank decision of the singular chains is not on a knife edge
    for dt, tol in ((np.float64, 1e6 * np.finfo(np.float64).eps), (np.float32, 1e3 * np.finfo(np.float32).eps)):
        k = f"chain_{np.dtype(dt).name}"
        for d, L in enumerate(CHAINS):
            B = out[f"{k}.blocks"][out[f"{k}.tptr"][d]:out[f"{k}.tptr"][d + 1]].reshape(L, L).astype(np.float64)
            s = np.linalg.svd(B, compute_uv=False)
            if L > 1:
                assert s[-2] >= 5 * tol * s[0] and s[-1] <= 1e-3 * tol * s[0], (k, L, s[-2:] / s[0], tol)
    A, sub, sptr = duplicate_matrix(rng)
    record(out, "dup", A, sub, sptr, False)
    A, sub, sptr = partial_matrix(rng)
    record(out, "part", A, sub, sptr, True)
    np.savez_compressed(HERE / "kernels_schwarz_setup.npz", **out)
    size = (HERE / "kernels_schwarz_setup.npz").stat().st_size
    print("kernels_schwarz_setup.npz written:", len(out), "arrays,", size, "bytes")


if __name__ == "__main__":
    main()
