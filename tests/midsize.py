"""Mid-size smoothed-aggregation hierarchies for the solver parity tests, built WITHOUT the reference and without the
product's own setup path: the project's test problems (tools/problems.py), the pinned oracle's aggregation and
tentative-prolongator kernels (oracle.standard_aggregation / fit_candidates) and plain SciPy / NumPy.  The checker
shares no code with what it checks (no pyamg, no oracle.refimport, no pyamg_amd.aggregation).

Construction per level: strength = the symmetric filter with theta = 0 (every stored off-diagonal block couples),
standard aggregation, T from fit_candidates (B = ones for scalar problems, the rigid-body modes for elasticity),
P = (I - omega D^-1 A) T with omega = 4 / (3 rho), rho from a fixed number of seeded power iterations, R = P^T,
A_c = R A P by SciPy; the coarsest operator (<= max_coarse unknowns) is solved by a dense pinv.

Host setup at these sizes takes seconds: hierarchies are cached per process (functools.lru_cache).
"""
from __future__ import annotations

import functools
import numpy as np
import scipy.sparse as sp

from oracle import oracle as orc
from pyamg_amd.hierarchy import HierarchySpec, LevelSpec, SmootherSpec, _normal_equation_spec, sparse_op

MAX_COARSE = 10
POWER_ITERS = 15


def _power_rho(M, its=POWER_ITERS, seed=0):
    """spectral-radius estimate of M (a linear operator with @) from seeded power iterations"""
    v = np.random.RandomState(seed).rand(M.shape[0])
    rho = 0.0
    for _ in range(its):
        w = M @ v
        nw = np.linalg.norm(w)
        if nw == 0.0:
            return 1.0
        rho = nw / np.linalg.norm(v)
        v = w / nw
    return rho


def _block_diag(A, bs):
    """(n_brow, bs, bs) diagonal blocks of A (CSR or BSR)"""
    Ab = sp.bsr_array(A, blocksize=(bs, bs)) if bs > 1 else sp.bsr_array(A.tocsr(), blocksize=(1, 1))
    Ab.sort_indices()
    nb = Ab.shape[0] // bs
    D = np.zeros((nb, bs, bs), dtype=A.dtype)
    for i in range(nb):
        for p in range(Ab.indptr[i], Ab.indptr[i + 1]):
            if Ab.indices[p] == i:
                D[i] = Ab.data[p]
    return D


def _strength(A, bs):
    """symmetric filter, theta = 0: the pattern of the off-diagonal blocks (block norms are never compared)"""
    if bs > 1:
        Ab = sp.bsr_array(A, blocksize=(bs, bs))
        S = sp.csr_array((np.ones(Ab.indices.size), Ab.indices, Ab.indptr), shape=(Ab.shape[0] // bs,) * 2)
    else:
        S = sp.csr_array(A, copy=True)
        S.data = np.ones_like(S.data)
    S = sp.csr_array(S + S.T)
    S.setdiag(0)
    S.eliminate_zeros()
    S.sort_indices()
    return S


def _level(A, B, bs):
    """one SA coarsening step: (P, R, A_c, B_c) or None when it would not coarsen"""
    S = _strength(A, bs)
    agg, _, n_agg = orc.standard_aggregation(S.indptr.astype(np.int32), S.indices.astype(np.int32))
    nf = S.shape[0]
    if n_agg < 1 or n_agg >= nf:
        return None
    keep = np.flatnonzero(agg >= 0)
    AggOp = sp.csr_array((np.ones(keep.size), (keep, agg[keep])), shape=(nf, n_agg)).tocsc()
    AggOp.sort_indices()
    K2 = B.shape[1]
    Ap, Ai = AggOp.indptr.astype(np.int32), AggOp.indices.astype(np.int32)       # int32 already: the oracle's pointers stay valid
    Qx, Rc = orc.fit_candidates(n_agg, bs, K2, Ap, Ai, np.ascontiguousarray(B, dtype=np.float64), 1e-10)
    Tt = sp.bsr_array((np.ascontiguousarray(Qx.swapaxes(1, 2)), Ai, Ap), shape=(n_agg * K2, nf * bs))
    T = sp.csr_array(Tt.T)
    Ac = sp.csr_array(A)
    dinv = 1.0 / Ac.diagonal()
    DA = sp.csr_array(sp.diags_array(dinv) @ Ac)
    omega = 4.0 / (3.0 * _power_rho(DA))
    P = sp.csr_array(T - omega * (DA @ T))
    P.sort_indices()
    R = sp.csr_array(P.T)
    R.sort_indices()
    Acoarse = sp.csr_array(R @ Ac @ P)
    Acoarse.sort_indices()
    return P, R, Acoarse, Rc.reshape(n_agg * K2, K2)


def _bsr(M, r, c):
    out = sp.bsr_array(M, blocksize=(r, c))
    out.sort_indices()
    return out


def _sa(A, B, bs):
    """[(A, P, R, blocksize)...] of scipy operators, level 0 first; the last entry has P = R = None"""
    out = []
    while A.shape[0] > MAX_COARSE:
        step = _level(A, B, bs)
        if step is None:
            break
        P, R, Ac, B = step
        K2 = B.shape[1]
        out.append((A, _bsr(P, bs, K2), _bsr(R, K2, bs), bs))
        A, bs = _bsr(Ac, K2, K2), K2
    out.append((A, None, None, bs))
    return out


def _cast(M, dtype):
    return None if M is None else M.astype(dtype)


@functools.lru_cache(maxsize=None)
def operators(name, dtype="float64"):
    """the operators of a named problem's hierarchy: tuple of (A, P, R, blocksize) scipy matrices (cached per process)"""
    from tools.problems import elasticity3d, poisson_csr
    kind, *arg = name.split(":")
    if kind == "poisson":
        grid = tuple(int(v) for v in arg[0].split("x"))
        A = poisson_csr(grid)
        levels = _sa(A, np.ones((A.shape[0], 1)), 1)
    elif kind == "elasticity":
        Ab, Bm = elasticity3d(int(arg[0]))
        Ab = _bsr(Ab, 3, 3)
        levels = _sa(Ab, np.ascontiguousarray(Bm, dtype=np.float64), 3)
    elif kind == "convdiff":
        A = convection_diffusion(int(arg[0]))
        levels = _sa(A, np.ones((A.shape[0], 1)), 1)
    else:
        raise ValueError(name)
    dt = np.dtype(dtype)
    return tuple((_cast(A, dt), _cast(P, dt), _cast(R, dt), bs) for A, P, R, bs in levels)


def convection_diffusion(n, velocity=(1.0, 0.5, 0.25), peclet=20.0):
    """3-D -Laplace(u) + w . grad(u), first-order upwind differences on an n^3 grid (lexicographic, last axis fastest): a
    non-symmetric M-matrix with sorted rows"""
    e = np.ones(n)
    I = sp.eye_array(n, format="csr")
    L = sp.diags_array([-e[:-1], 2 * e, -e[:-1]], offsets=[-1, 0, 1], format="csr")
    U = sp.diags_array([-e[:-1], e], offsets=[-1, 0], format="csr") * (peclet / n)      # upwind for a positive velocity

    def kron3(a, b, c):
        return sp.kron(sp.kron(a, b), c)
    A = sum(kron3(*[L if k == d else I for k in range(3)]) + velocity[d] * kron3(*[U if k == d else I for k in range(3)]) for d in range(3))
    A = sp.csr_array(A)
    A.sum_duplicates()
    A.sort_indices()
    A.indptr, A.indices = A.indptr.astype(np.int32), A.indices.astype(np.int32)
    return A


def chebyshev_coefficients(A, degree=3):
    """the helper's own Chebyshev polynomial p (highest power first, the reference's Horner order): 1 - x p(x) vanishes at the
    roots of the degree + 1 Chebyshev polynomial shifted to [rho / 30, 1.1 rho] (parity does not depend on the values)"""
    rho = 1.1 * _power_rho(sp.csr_array(A))
    a, b = rho / 30.0, rho
    k = degree + 1
    roots = (a + b) / 2 + (b - a) / 2 * np.cos(np.pi * (np.arange(k) + 0.5) / k)
    q = np.poly1d([1.0])
    for r in roots:
        q = q * np.poly1d([-1.0 / r, 1.0])                 # prod (1 - x / r)
    p = (np.poly1d([1.0]) - q).coeffs[:-1]              # (1 - q(x)) / x: q(0) = 1, drop the constant, divide by x
    return np.ascontiguousarray(p, dtype=np.float64)


# ----------------------------------------------------------------- smoother specs, filled directly
def gs(sweep="symmetric", iterations=1):
    return lambda A, bs, lvl: SmootherSpec("gauss_seidel", int(iterations), 1.0, sweep, name="gauss_seidel")


def sor(omega=1.3, sweep="forward"):
    return lambda A, bs, lvl: SmootherSpec("sor", 1, float(omega), sweep, name="sor")


def chebyshev(degree=3):
    return lambda A, bs, lvl: SmootherSpec("polynomial", 1, coefficients=chebyshev_coefficients(A, degree), name="chebyshev")


def _dinv(A, bs):
    D = np.ascontiguousarray(_block_diag(A, bs), dtype=np.float64)
    orc.pinv_array(D, D.shape[0], bs, "T")
    return np.ascontiguousarray(D, dtype=A.dtype)


def block_gs(sweep="symmetric"):
    return lambda A, bs, lvl: SmootherSpec("block_gauss_seidel", 1, 1.0, sweep, Dinv=_dinv(A, bs), blocksize=bs, name="block_gauss_seidel")


def block_jacobi(omega=0.6):
    return lambda A, bs, lvl: SmootherSpec("block_jacobi", 1, float(omega), Dinv=_dinv(A, bs), blocksize=bs, name="block_jacobi")


def gs_nr(sweep="symmetric"):
    return lambda A, bs, lvl: _normal_equation_spec("gauss_seidel_nr", A, 1, sweep, 1.0)


@functools.lru_cache(maxsize=None)
def hierarchy(name, pre, post=None, dtype="float64", scalar_csr=False):
    """HierarchySpec of problem `name` with smoothers `pre` / `post` (names of the factories above, with arguments as a tuple:
    ("sor", 1.3, "forward")); post = None: the same as pre.  The coarse levels of a scalar problem are BSR(1,1) as the reference's SA
    setup makes them (its relaxation then ignores SOR's omega); scalar_csr = True ships them as CSR, where omega takes effect."""
    def make(desc):
        return globals()[desc[0]](*desc[1:])
    pre_f, post_f = make(pre), make(post if post is not None else pre)
    ops = operators(name, dtype)
    levels = []
    for lvl, (A, P, R, bs) in enumerate(ops):
        last = P is None
        if scalar_csr and bs == 1:
            A, P, R = (None if M is None else _csr(M) for M in (A, P, R))
        levels.append(LevelSpec(sparse_op(A), None if last else sparse_op(P), None if last else sparse_op(R),
                                None if last else pre_f(A, bs, lvl), None if last else post_f(A, bs, lvl)))
    Ac = ops[-1][0]
    coarse = np.ascontiguousarray(np.linalg.pinv(Ac.toarray().astype(np.float64)), dtype=np.dtype(dtype))
    return HierarchySpec(levels=levels, coarse_kind="dense", coarse_op=coarse, coarse_name="'pinv'")


def _csr(M):
    out = sp.csr_array(M)
    out.sort_indices()
    return out


def level_op(name, lvl, dtype="float64", csr=False):
    """the SparseOp of one level's operator (csr: its scalar CSR form)"""
    A = operators(name, dtype)[lvl][0]
    return sparse_op(_csr(A) if csr else A)
