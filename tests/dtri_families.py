"""Named operator families for the DENSE BLOCK-TRIANGULAR form of the symmetric Gauss-Seidel sweep (pyamg_amd/csrc/pamg_dtri_plan.h, pamg_dtri.hip,
pamg_matrix_dense_tri): the shapes on which kernels that consume a sound plan can still go wrong.  A helper module like tests/sweep_families.py and
tests/schwarz_families.py, shared by tests/test_dtri_families_plan.py (CPU replay through tests/dtri_emul.cpp, small size) and
tests/test_gpu_dtri_families.py (the device, large size: at most ~3000 rows unless a case says otherwise).

Every case is deterministic (seeded) and DECLARES its outcome; both test files assert it -- a case that passes because the form stepped aside is a
failure:
    engages          the form is built, with `blocks` blocks, and its growth figure is `growth()`
    declines_host    build_dtri_plan refuses (`status`: DTRI_E_DIAGONAL or DTRI_E_NONFINITE)
    declines_growth  the guard's figure is above DTRI_GROWTH_CAP = 1e3
    declines_size    more than 65535 blocks, or triangles above 2 GB (build_dtri_part's rule: the device only -- the plan header has none, the CPU
                     test checks the arithmetic of the rule instead)

The growth figure max_i sum_j |W_ij| |a_jj| over W = tril(A_kk)^-1 and triu(A_kk)^-1 of every diagonal block comes from NumPy's dense inverses
(`growth_numpy`), or from a closed form where there is one (chains: (3^L - 1) / 2 for a chain of L rows inside one block; a diagonal block: 1).

What the kernels partition by, and so where the block sizes sit: the dense phase owns slot q by thread q mod 256 (a pair of rows spills into a second
pass for m > ~509), one wave's 64 slots end at m ~ 125, the inverse kernel's second column workgroup starts at m = 257, the sparse phase puts 16 rows
and the growth kernel 4 rows into a workgroup.

The yardstick is tests/sweep_families.py's: ref_sweeps(..., dtype=np.longdouble), the oracle's sequential sweep on long-double copies, and rel_err.
The yardstick, the replay and the device take the arrays AS STORED: the upload (pamg_matrix_create) keeps explicit zeros, unsorted rows and
duplicate entries as they are (pamg_matrix_create copies the three arrays).  The device test asserts the stored-entry count, which shows that zeros
and duplicates are kept; the order inside a row is not readable through the binding and is not asserted."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

import sweep_families as SF

OK, E_SHAPE, E_DIAGONAL, E_GROWTH, E_NONFINITE = 0, 1, 2, 3, 4          # pamg_dtri_plan.h
GROWTH_CAP = 1e3
MAX_BLOCKS = 65535                                                     # build_dtri_part: blocks are a grid dimension
MAX_BYTES = 2 ** 31                                                    # DTRI_MAX_BYTES: both directions together
TOL = 1e-13                                                            # the project's per-sweep bar
NONSYM_B = (2, 3, 15, 16, 17, 63, 64, 65, 125, 129, 255, 256, 257, 509, 513, 1000, 2048)
OTHER_B = (65, 257, 2048)


def tri_slots(m):
    """slots of a packed triangle of m rows: row i holds i + 1 values in an even number of slots (dtri_tri_slots)"""
    return sum((i + 2) & ~1 for i in range(m))


def tri_bytes(n, B):
    """bytes of the inverse triangles of BOTH directions at block size B"""
    full, rest = divmod(n, B)
    return 2 * 8 * (full * tri_slots(B) + tri_slots(rest))


@dataclass(frozen=True)
class Case:
    name: str
    make: object                                   # make() -> scipy CSR, arrays as stored
    B: int
    outcome: str = "engages"
    status: int = OK                               # what the CPU replay reports (declines_size: OK -- the rule is the device's)
    exact_growth: float | None = None              # closed form, where there is one
    growth_of: object = None                       # operator whose NumPy figure is this case's (rowscale: the unscaled one)
    off_block: int | None = None                   # declared number of off-block entries, where the family is about them
    note: str = ""

    @property
    def id(self):
        return f"{self.name}-B{self.B}"

    def A(self):
        return _made(self.make)

    def blocks(self):
        return -(-self.A().shape[0] // self.B)

    def growth(self):
        if self.exact_growth is not None:
            return self.exact_growth
        return growth_numpy(_made(self.growth_of or self.make), self.B)


@functools.lru_cache(maxsize=None)
def _made(make):
    return make()


def growth_numpy(A, B):
    """max_i sum_j |W_ij| |a_jj| over the dense inverses of the lower and the upper triangle of every diagonal block"""
    A = sp.csr_array(A)
    n = A.shape[0]
    d = np.abs(A.diagonal())
    g = 0.0
    for lo in range(0, n, B):
        hi = min(lo + B, n)
        K = A[lo:hi, lo:hi].toarray()                                  # (duplicate entries add up: halves stored twice are exact)
        for T in (np.tril(K), np.triu(K)):
            g = max(g, float(np.max(np.abs(np.linalg.inv(T)) @ d[lo:hi])))
    return g


class _Make:
    """a hashable, named constructor call: equal calls share one cached operator"""
    def __init__(self, fn, *args):
        self.fn, self.args = fn, args

    def __call__(self):
        return self.fn(*self.args)

    def __hash__(self):
        return hash((self.fn, self.args))

    def __eq__(self, other):
        return isinstance(other, _Make) and (self.fn, self.args) == (other.fn, other.args)


# ----------------------------------------------------------------- operators
def nonsym_rows(n):
    """sweep_families.nonsym at n rows (n = 3000: the same operator)"""
    S, r = SF._pattern(n, 18, 101)
    return SF._dominant(S, r)


def _matrix_block(B, r):
    """one dominant block of B rows whose LAST row and LAST column hold exactly one off-diagonal entry each: (B-1, B-2) and (B-2, B-1)"""
    if B == 1:
        return np.array([[1.0 + r.rand()]])
    m = B - 1
    K = np.where(r.rand(m, m) < min(1.0, 6.0 / max(m, 1)), -(0.05 + 0.95 * r.rand(m, m)), 0.0)
    out = np.zeros((B, B))
    out[:m, :m] = K
    out[B - 1, B - 2], out[B - 2, B - 1] = -(0.05 + 0.95 * r.rand()), -(0.05 + 0.95 * r.rand())
    np.fill_diagonal(out, 0.0)
    np.fill_diagonal(out, np.abs(out).sum(axis=1) + 0.5 + r.rand(B))
    return out


def block_aligned(B, k, shifted):
    """block-diagonal, k blocks of exactly B rows: 0 off-block entries at block size B and nb = k.  shifted: the same operator moved down and right
    by one row behind a 1 x 1 block and cut to k B rows -- every matrix block then straddles a boundary of the partition through its last row and
    column, which hold one entry each: every block of the partition keeps exactly one entry in each slice (none before the first / after the last)"""
    r = np.random.RandomState(120 + B)
    blocks = [sp.csr_array(_matrix_block(B, r)) for _ in range(k)]
    M = sp.block_diag(blocks, format="csr")
    if shifted:
        n = k * B
        M = sp.csr_array(sp.block_diag([sp.csr_array(np.array([[1.5]])), M], format="csr"))[:n, :n]
    return SF._finish(M)


def arrow(n):
    """every 97th row stores an entry in every third column of the whole operator, all other rows 2 - 4 entries: slice rows of hundreds of entries sit
    beside empty ones in the same 16-row workgroup of the sparse phase.  Strictly diagonally dominant"""
    r = np.random.RandomState(131)
    rows, cols, vals = [], [], []
    for i in range(n):
        if i % 97 == 0:
            js = np.arange(i % 3, n, 3)
            js = js[js != i]
            v = -(0.05 + 0.95 * r.rand(js.size)) / js.size
        else:
            js = r.choice(np.setdiff1d(np.arange(max(0, i - 40), min(n, i + 41)), [i]), size=r.randint(2, 5), replace=False)
            v = -(0.05 + 0.95 * r.rand(js.size))
        rows += [i] * js.size
        cols += list(js)
        vals += list(v)
    S = sp.csr_array((vals, (rows, cols)), shape=(n, n))
    return SF._dominant(S, r)


def stored(n):
    """what a CSR operator may legally store: every 5th off-diagonal entry is an explicit 0.0 (in-block and off-block alike), every 3rd row has its
    columns in REVERSED order, and in every 7th row the first off-diagonal entry is stored twice as two halves (0.5 v is exact).  Nothing is sorted,
    summed or eliminated afterwards"""
    A = nonsym_rows(n)
    Ap, Aj, Ax = A.indptr, A.indices, A.data.copy()
    offd = np.flatnonzero(Aj != np.repeat(np.arange(n), np.diff(Ap)))
    Ax[offd[::5]] = 0.0
    ptr, idx, val = [0], [], []
    for i in range(n):
        js, vs = list(Aj[Ap[i]:Ap[i + 1]]), list(Ax[Ap[i]:Ap[i + 1]])
        if i % 7 == 0:
            p = next((q for q, j in enumerate(js) if j != i and vs[q] != 0.0), None)
            if p is not None:
                vs[p] *= 0.5
                js.insert(p + 1, js[p])
                vs.insert(p + 1, vs[p])
        if i % 3 == 0:
            js, vs = js[::-1], vs[::-1]
        idx += js
        val += vs
        ptr.append(len(idx))
    out = sp.csr_array((np.array(val), np.array(idx, dtype=np.int32), np.array(ptr, dtype=np.int32)), shape=(n, n))
    assert out.nnz == A.nnz + sum(1 for i in range(0, n, 7)) and not out.has_canonical_format
    assert np.count_nonzero(out.data == 0.0) == offd[::5].size
    return out


ROWSCALE_SEED = 141


def rowscale_exponents(n):
    return np.random.RandomState(ROWSCALE_SEED).randint(-200, 201, size=n)


def rowscale(n):
    """nonsym with row i multiplied by 2^e_i, e_i in [-200, 200] (the right-hand side's row too: `rowscale_exponents`).  Every product of the sweep is
    scaled by a power of two and scaled back by the diagonal: the growth figure and every output bit are those of the unscaled operator"""
    A = nonsym_rows(n)
    return SF._finish(sp.diags_array(np.ldexp(1.0, rowscale_exponents(n))) @ A)


def chains(n, L):
    """a_ii = 1, sub-diagonal -3 cut every L rows, super-diagonal -0.3 (not cut: the operator stays connected and its sweeps n levels deep): NOT
    diagonally dominant.  A chain of c rows inside one block gives the forward triangle the growth (3^c - 1) / 2; the backward triangle's stays below
    1 / 0.7"""
    main, off = np.full(n, 1.0), np.full(n - 1, -3.0)
    off[L - 1::L] = 0.0
    A = sp.csr_array(sp.diags_array([off, main, np.full(n - 1, -0.3)], offsets=[-1, 0, 1]))
    A.eliminate_zeros()
    return SF._finish(A)


def nonsym_with_chain(n, L=8):
    """nonsym with a chain laid over rows 8 .. 8 + L - 1: a_{i,i-1} = -3 a_ii there.  A general sparse operator (merged lane plans, zero-iterate plans)
    whose first block's forward inverse grows like 3^L: a growth decline on an operator that is not a band"""
    A = sp.lil_array(nonsym_rows(n))
    for i in range(9, 8 + L):
        A[i, i - 1] = -3.0 * A[i, i]
    return SF._finish(sp.csr_array(A))


def chain_growth(L, B):
    """closed form for chains(n, L) at block size B, n large: the longest piece of a chain that lies inside one block"""
    c = min(L, B)
    return (3.0 ** c - 1.0) / 2.0


RANDOM_CHAIN_SEED = 5
RANDOM_CHAINS = ((2.0, 2.4, 8), (1.7, 2.0, 10), (1.5, 1.75, 12))


def random_chains(n, which, seed=RANDOM_CHAIN_SEED):
    """chains with random ratios: sub-diagonal -ratio, ratio uniform in [lo, hi], cut every L rows; the guard's figure sits a little under its cap"""
    lo, hi, L = RANDOM_CHAINS[which]
    r = np.random.RandomState(1000 * seed + which)
    off = -(lo + (hi - lo) * r.rand(n - 1))
    off[L - 1::L] = 0.0
    A = sp.csr_array(sp.diags_array([off, np.full(n, 1.0), np.full(n - 1, -0.3)], offsets=[-1, 0, 1]))
    A.eliminate_zeros()
    return SF._finish(A)


def tridiag_rows(n):
    r = np.random.RandomState(109)
    return SF._finish(sp.diags_array([-(0.1 + 0.4 * r.rand(n - 1)), 1.0 + r.rand(n), -(0.1 + 0.4 * r.rand(n - 1))], offsets=[-1, 0, 1]))


BAD_DIAG = ("missing", "zero", "twice", "inf", "nan")


def bad_diag(n, kind):
    """nonsym with the diagonal of row n // 2 + 3 missing, stored as 0.0, stored twice (two halves), inf or NaN"""
    A = nonsym_rows(n)
    i = n // 2 + 3
    Ap, Aj, Ax = A.indptr.copy(), A.indices.copy(), A.data.copy()
    p = Ap[i] + int(np.flatnonzero(Aj[Ap[i]:Ap[i + 1]] == i)[0])
    if kind == "missing":
        Aj, Ax = np.delete(Aj, p), np.delete(Ax, p)
        Ap[i + 1:] -= 1
    elif kind == "twice":
        Ax[p] *= 0.5
        Aj, Ax = np.insert(Aj, p, i), np.insert(Ax, p, Ax[p])
        Ap[i + 1:] += 1
    else:
        Ax[p] = {"zero": 0.0, "inf": np.inf, "nan": np.nan}[kind]
    return sp.csr_array((Ax, Aj.astype(np.int32), Ap.astype(np.int32)), shape=A.shape)


NONFINITE = (("nan", "in_block"), ("inf", "in_block"), ("nan", "off_block"), ("inf", "off_block"))


def nonfinite_offdiag(size, B, value, where):
    """lower_only with one off-diagonal entry of a row in the middle block set to NaN or inf: the first stored entry of that row inside its diagonal
    block, or the first outside it.  (On a one-sided operator the sequential sweep keeps the value to the rows that depend on the poisoned one; on
    nonsym it reaches every row by either path and nothing could be told apart)"""
    A = sp.csr_array(SF.lower_only(size), copy=True)
    n = A.shape[0]
    k = (n // B) // 2
    lo, hi = k * B, min((k + 1) * B, n)
    for i in range(lo, hi):
        js = A.indices[A.indptr[i]:A.indptr[i + 1]]
        inside = (js >= lo) & (js < hi) & (js != i)
        pick = np.flatnonzero(inside if where == "in_block" else ~inside & (js != i))
        if pick.size:
            A.data[A.indptr[i] + pick[0]] = np.nan if value == "nan" else np.inf
            return A
    raise AssertionError("no such entry")


# ----------------------------------------------------------------- the cases
def _nonsym_sizes(B, n_full):
    """rows at which nonsym runs at block size B: the full size, k B + 1 (a ragged block of ONE row) and k B - 1"""
    k = 1 if B > 1500 else max(2, 600 // B)
    return (n_full, k * B + 1, k * B - 1)


@functools.lru_cache(maxsize=None)
def cases(size):
    """every case of `size` ("small": the CPU replay; "large": the device)"""
    big = size == "large"
    out = []

    def add(name, fn, *args, B, **kw):
        out.append(Case(name, _Make(fn, *args), B, **kw))

    # -- operator content
    nfull = 3000 if big else 300
    for B in (NONSYM_B if big else (2, 3, 16, 17, 63, 64, 65, 125, 129)):
        for n in _nonsym_sizes(B, nfull) if big else (nfull, 2 * B + 1, 2 * B - 1):
            add(f"nonsym[{n}]", nonsym_rows, n, B=B)
    if big:
        add("nonsym[4097]", nonsym_rows, 4097, B=4096, note="one full block and a block of one row; nine passes of the dense loop")
    Bs = OTHER_B if big else (16, 65)
    for B in Bs:
        add("mixed_sign", SF.mixed_sign, size, B=B)
        add("tridiag", SF.tridiag, size, B=B)
        add("convdiff_l1", SF.convdiff_l1, size, B=B)
        add("lower_only", SF.lower_only, size, B=B, note="Uo is empty and every backward triangle is diagonal")
        add("upper_only", SF.upper_only, size, B=B, note="Lo is empty and every forward triangle is diagonal")
        add("diag_only", SF.diag_only, size, B=B, exact_growth=1.0, off_block=0, note="nb > 1 with no off-block entry")
        k = max(2, (2000 if big else 200) // B)
        add("block_aligned", block_aligned, B, k, False, B=B, off_block=0, note="nb > 1 with no off-block entry")
        add("block_aligned_shifted", block_aligned, B, k, True, B=B, off_block=2 * (k - 1), note="exactly one entry in each slice of every block")
        add("arrow", arrow, 3000 if big else 400, B=B)
        add("stored", stored, nfull, B=B, note="explicit zeros, reversed rows, halves stored twice: kept as stored by the upload")
        add("rowscale", rowscale, nfull, B=B, growth_of=_Make(nonsym_rows, nfull), note="bits and growth of nonsym")
        for w in range(len(RANDOM_CHAINS)):
            add(f"random_chains{w}", random_chains, 2880 if big else 960, w, B=B)
    for n in (1, 2, 3, 5, 9, 63, 65, 300):
        for B in ((65,) if n < 300 or not big else OTHER_B) if big else (4, 65):
            add(f"dense_rows[{n}]", SF.tiny, n, B=B, note="every in-block entry stored; at B < n every slice row is full")
    add("dense_rows[9]", SF.tiny, 9, B=1, note="B = 1: every triangle is 1 / a_ii")
    # -- the growth edge
    nch = 3000 if big else 420
    for B in Bs + (96,):
        add("chains6", chains, nch, 6, B=B, exact_growth=chain_growth(6, B))
    add("chains7", chains, nch, 7, B=4, exact_growth=chain_growth(7, 4), note="the guard depends on the block size: growth 40 at B = 4")
    for B in (64, 100):
        add("chains7", chains, nch, 7, B=B, outcome="declines_growth", status=E_GROWTH, exact_growth=chain_growth(7, B))
    for w in range(len(RANDOM_CHAINS)):
        add(f"random_chains{w}", random_chains, 2880 if big else 960, w, B=96)
    add("nonsym_chain8", nonsym_with_chain, nfull, 8, B=64, outcome="declines_growth", status=E_GROWTH, note="a growth decline off the band")
    # -- host declines
    Bd = 257 if big else 64
    for kind in BAD_DIAG:
        add(f"bad_diag_{kind}", bad_diag, nfull, kind, B=Bd, outcome="declines_host", status=E_DIAGONAL)
    for value, where in NONFINITE:
        add(f"nonfinite_{value}_{where}", nonfinite_offdiag, size, Bd, value, where, B=Bd, outcome="declines_host", status=E_NONFINITE)
    # -- size
    add("tridiag[600]", tridiag_rows, 600, B=1, exact_growth=1.0, note="600 blocks: 2398 launches")
    if big:
        add("too_many_blocks", tridiag_rows, 65536, B=1, outcome="declines_size", note="65536 blocks: one past the grid dimension")
        add("too_many_bytes", tridiag_rows, 32768, B=8192, outcome="declines_size", note="2 148 007 936 bytes of triangles against the 2^31 cap")
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return tuple(out)


def select(size, outcome=None):
    return [c for c in cases(size) if outcome is None or c.outcome == outcome]


def vectors(n, seed=7):
    """(b, x0) of a case"""
    rng = np.random.RandomState(seed)
    return rng.rand(n), rng.rand(n)
