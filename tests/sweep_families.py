"""Named operator families for the merged lane-parallel Gauss-Seidel sweeps (cluster layout, fused symmetric launch, zero-iterate plans): the shapes
on which a kernel that consumes a sound plan can still go wrong.  A helper module like tests/midsize.py, shared by tests/test_sweep_families_plan.py
(CPU replay of the planner, small size) and tests/test_gpu_sweep_families.py (the device, large size: a few thousand rows, plans build in
milliseconds).  Every family is deterministic (seeded) and DECLARES the form it must take on the device; the tests assert that form, from the
planner's statistics on the CPU and from lanem_info / lane_info / sym_info on the device -- a case that passes because the path under test stepped
aside is a failure.

What decides the form (pyamg_amd/csrc/pamg_lane.hip: lanem_smax, build_lanem_part, lanem_to_device, build_zero_plan):
  * a schedule of fewer than 8 dependency levels is never merged (MIN_LEVELS): a diagonal operator has ONE level and n < 8 rows cannot have 8 --
    these are not declines of the planner, there is nothing to merge.  (Levels count connections through an entry in either direction: a triangle
    swept against its entries is as deep as swept along them -- every operand old -- and IS merged; its other triangle is the diagonal alone, so it
    has no zero-iterate plans);
  * the device tries the merged form only on a schedule the UNMERGED lane form can hold too (lane_eligible: one layout per schedule, an SOR sweep of
    the same operator needs the unmerged one) -- at most LANE_ENTRIES = 256 off-diagonal entries in every stored row.  `lane_edge` sits on that
    edge (rows of 254 .. 256 entries, whose merged rows then grow to the planner's 512); `long_fits` and `long_declines` are beyond it and run the
    order-exact sweep on the device in every layout;
  * a merged row of more than 512 operands (LANEM_KMAX * 64; 256 in the pair layout, 32 lanes per row) closes its super-level early, and a STORED
    row of more makes build_lanem_plan decline: `long_declines` in every layout, `long_fits` (rows of 500 .. 512 operands) in the pair layout only
    -- what the CPU replay of the planner sees;
  * a plan that merges nothing (super-levels > 0.9 dependency levels) is not kept: `wide` in the pair layout, where two of its rows merged pass
    256 operands;
  * the zero-iterate plans exist where BOTH directions of the general sweep are merged and tril(A) / triu(A) pass the same rules.
`Form` holds the declaration for the LARGE size, the one the device runs: forward / backward merged or not, zero plans present or not, and the
layouts in which the planner declines (those hold for the small size too: they follow from the longest row) or gains nothing."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp

from oracle import oracle as orc
from pyamg_amd.hierarchy import sparse_op

MIN_LEVELS = 8                      # lanem_smax / build_zero_plan: fewer dependency levels are never merged
LANE_ENTRIES = 256                  # LANE_KMAX * 64: off-diagonal entries of the longest row the unmerged lane form holds (lane_eligible)
ROW_OPERANDS = 512                  # LANEM_KMAX * 64: the longest row a wave holds (cluster layout, one row per wave)
PAIR_OPERANDS = 256                 # two rows per wave: 32 lanes x LANEM_KMAX
TINY = (2, 3, 5, 9, 63, 65)
U = 2.0 ** -53


@dataclass(frozen=True)
class Form:
    """what must run: `fwd` / `bwd` -- the general sweep of that direction takes the merged form; `zero` -- the operator holds zero-iterate plans;
    `declines` -- the layouts ("row", "pair", "cluster") in which build_lanem_plan must decline (fwd / bwd / zero then hold for the others);
    `gains_nothing` -- the layouts in which the plan is built but merges (next to) nothing, so the device does not keep it;
    `lane_fits` -- no stored row has more than LANE_ENTRIES off-diagonal entries (otherwise the device runs no lane form at all, merged or not)"""
    fwd: bool = True
    bwd: bool = True
    zero: bool = True
    declines: tuple = ()
    gains_nothing: tuple = ()
    lane_fits: bool = True


@dataclass(frozen=True)
class Family:
    name: str
    make: object                                  # make(size) -> scipy CSR, size in ("small", "large")
    form: Form = field(default_factory=Form)
    tol: float = 1e-13                            # against the sequential sweep, relative (chains: growth <= 1e3 costs three digits)
    note: str = ""


def _finish(A):
    A = sp.csr_array(A)
    A.sort_indices()
    A.indptr, A.indices = A.indptr.astype(np.int32), A.indices.astype(np.int32)
    return A


def _pattern(n, per_row, seed):
    """random structurally non-symmetric off-diagonal pattern, about per_row entries in every row, values in -(0, 1]"""
    r = np.random.RandomState(seed)
    S = sp.random(n, n, density=min(1.0, per_row / n), random_state=r, format="csr")
    S.data = -(0.05 + 0.95 * S.data)
    S.setdiag(0)
    S.eliminate_zeros()
    return sp.csr_array(S), r


def _dominant(S, r):
    """S + D with a_ii = sum |a_ij| + 0.5 + rand: strictly diagonally dominant"""
    d = np.asarray(abs(S).sum(axis=1)).ravel() + 0.5 + r.rand(S.shape[0])
    return _finish(S + sp.diags_array(d))


def nonsym(size):
    n = 300 if size == "small" else 3000
    S, r = _pattern(n, 18, 101)
    return _dominant(S, r)


def mixed_sign(size):
    """nonsym with random column signs (the diagonal's too): products and sums of both signs, cancellation in the row sums"""
    A = nonsym(size)
    sg = np.where(np.random.RandomState(102).rand(A.shape[0]) < 0.5, -1.0, 1.0)
    return _finish(A @ sp.diags_array(sg))


def lower_only(size):
    return _finish(sp.tril(nonsym(size), format="csr"))


def upper_only(size):
    return _finish(sp.triu(nonsym(size), format="csr"))


def diag_only(size):
    n = 200 if size == "small" else 2000
    return _finish(sp.diags_array(1.0 + np.random.RandomState(103).rand(n)))


def nodiag_rows(n):
    """(missing, explicit zero, empty): every 7th diagonal is not stored, every 11th of the others is stored as 0.0, one row holds nothing"""
    empty = n // 2 + 1
    missing = [i for i in range(0, n, 7)]
    zero = [i for i in range(4, n, 11) if i % 7 and i != empty]
    assert empty % 7 and empty not in zero
    return missing, zero, empty


def nodiag(size):
    n = 280 if size == "small" else 2500
    r = np.random.RandomState(104)
    S = sp.random(n, n, density=16.0 / n, random_state=r, format="csr")
    S = sp.csr_array(-abs(S + S.T))
    S.setdiag(0)
    S.eliminate_zeros()
    A = sp.coo_array(_dominant(S, r))
    missing, zero, empty = nodiag_rows(n)
    row, col, val = A.row.copy(), A.col.copy(), A.data.copy()
    isd = row == col
    val[isd & np.isin(row, zero)] = 0.0                                   # stored, explicit 0.0
    keep = ~(isd & np.isin(row, missing)) & (row != empty)
    out = sp.csr_array((val[keep], (row[keep], col[keep])), shape=(n, n))  # (no eliminate_zeros: the explicit zeros stay stored)
    out = _finish(out)
    assert out.indptr[empty] == out.indptr[empty + 1] and out.nnz == int(keep.sum())
    return out


def untouched_rows(A):
    """rows a Gauss-Seidel sweep leaves alone: no stored diagonal, or a diagonal of 0.0 (amg_core's gauss_seidel updates a row only where diag != 0)"""
    return np.flatnonzero(~(sp.csr_array(A).diagonal() != 0.0))


def _with_long_rows(n, lengths, seed):
    """a sparse dominant operator (about 12 entries per row) in which row i_k holds lengths[k] off-diagonal entries and column i_k as many; the
    long rows sit far apart"""
    S, r = _pattern(n, 12, seed)
    S = sp.lil_array(S)
    long_rows = [(2 * k + 1) * n // (2 * len(lengths)) for k in range(len(lengths))]
    for i, L in zip(long_rows, lengths):
        cols = r.choice(np.setdiff1d(np.arange(n), long_rows), size=L, replace=False)
        S.rows[i], S.data[i] = [], []
        for j in np.sort(cols):
            S[i, j] = -(0.05 + 0.95 * r.rand()) / L * 12.0
            S[j, i] = -(0.05 + 0.95 * r.rand())                           # and the column: row i is an operand of as many rows
    A = _dominant(sp.csr_array(S), r)
    got = np.sort(np.diff(A.indptr))[::-1][:len(lengths)] - 1
    assert sorted(got) == sorted(lengths), (got, lengths)
    return A


def lane_edge(size):
    """rows of 254, 255 and 256 off-diagonal entries: the last is the longest the device takes into a lane form; merged with the rows they depend on
    they reach the planner's 512 operands, so super-levels close by length around them"""
    return _with_long_rows(500 if size == "small" else 3000, (254, 255, 256), 111)


def long_fits(size):
    """rows of 500, 511 and 512 operands: the last is the longest a wave holds (512 slots); their columns are as long"""
    return _with_long_rows(700 if size == "small" else 3000, (500, 511, 512), 105)


def long_declines(size):
    """one row of 513 operands, one past the planner's edge (in the large size also one of 257, one past the device's, and one of 700):
    build_lanem_plan declines, the device runs the order-exact sweep"""
    return _with_long_rows(900 if size == "small" else 3000, (513,) if size == "small" else (257, 513, 700), 106)


def mixed_lengths(size):
    """rows of 1 entry (the diagonal) and of about 100 entries alternating in row-index order: a cluster packs unequal rows into one wave"""
    n = 400 if size == "small" else 2000
    S, r = _pattern(n, 100, 107)
    S = sp.lil_array(S)
    for i in range(0, n, 2):
        S.rows[i], S.data[i] = [], []
    return _dominant(sp.csr_array(S), r)


def wide(size):
    """about 150 entries per row: every row spans three 64-slot units before anything is merged"""
    n = 400 if size == "small" else 2000
    S, r = _pattern(n, 150, 108)
    return _dominant(S, r)


def tridiag(size):
    n = 300 if size == "small" else 2000
    r = np.random.RandomState(109)
    return _finish(sp.diags_array([-(0.1 + 0.4 * r.rand(n - 1)), 1.0 + r.rand(n), -(0.1 + 0.4 * r.rand(n - 1))], offsets=[-1, 0, 1]))


def tiny(n):
    """dense, dominant, non-symmetric values: row i depends on every row before it (n dependency levels in both directions)"""
    r = np.random.RandomState(110 + n)
    D = -(0.1 + r.rand(n, n))
    np.fill_diagonal(D, 0.0)
    np.fill_diagonal(D, np.abs(D).sum(axis=1) + 0.5 + r.rand(n))
    return _finish(sp.csr_array(D))


def tiny_form(n):
    """n rows have at most n dependency levels: below MIN_LEVELS nothing is merged and no zero-iterate plan exists"""
    ok = n >= MIN_LEVELS
    return Form(fwd=ok, bwd=ok, zero=ok)


def chains(size):
    """NOT diagonally dominant: |a_ir / a_rr| = 3 along independent chains of 24 rows (the operator of test_lanem_plan.py / test_gpu_kernels.py)"""
    n = 400 if size == "small" else 3000
    main, off = np.full(n, 1.0), np.full(n - 1, -3.0)
    off[23::24] = 0.0
    return _finish(sp.diags_array([off, main, 0.1 * off], offsets=[-1, 0, 1]))


CONVDIFF = {"small": "convdiff:16", "large": "convdiff:32"}


@functools.lru_cache(maxsize=None)
def convdiff_l1(size):
    """level 1 of the smoothed-aggregation hierarchy of the upwind convection-diffusion problem (tests/midsize.py): non-symmetric values on a
    symmetric SA pattern, about 40 entries per row"""
    import midsize as M
    return _finish(sp.csr_array(M.operators(CONVDIFF[size])[1][0]).astype(np.float64))


ONE_WAY = "one sweep reads only new values, the other only old ones; the other triangle is the diagonal alone (one level): no zero-iterate plans"
FAMILIES = {f.name: f for f in (
    Family("nonsym", nonsym),
    Family("mixed_sign", mixed_sign),
    Family("lower_only", lower_only, Form(zero=False), note=ONE_WAY),
    Family("upper_only", upper_only, Form(zero=False), note=ONE_WAY),
    Family("diag_only", diag_only, Form(fwd=False, bwd=False, zero=False), note="one dependency level in both directions: nothing to merge"),
    Family("nodiag", nodiag),
    Family("lane_edge", lane_edge, note="254 .. 256 entries: the longest rows the device merges"),
    Family("long_fits", long_fits, Form(declines=("pair",), lane_fits=False),
           note="500 .. 512 operands: the planner fits them into a wave's 512 slots (not into the pair layout's 256); the device is past its 256-entry edge"),
    Family("long_declines", long_declines, Form(fwd=False, bwd=False, zero=False, declines=("row", "pair", "cluster"), lane_fits=False),
           note="a row above 512 operands"),
    Family("mixed_lengths", mixed_lengths),
    Family("wide", wide, Form(gains_nothing=("pair",)), note="two merged rows pass the pair layout's 256 operands: every super-level closes at one level"),
    Family("tridiag", tridiag),
    Family("chains", chains, tol=1e-10),
    Family("convdiff_l1", convdiff_l1),
)}


def layout_of(cluster, rpw):
    return "cluster" if cluster >= 4 else "pair" if rpw == 2 else "row"


def expected(form, cluster, rpw):
    """(fwd merged, bwd merged, zero plans) the device must report for `form` in the layout of (lanem_cluster, lanem_rpw)"""
    if not form.lane_fits or layout_of(cluster, rpw) in form.declines + form.gains_nothing:
        return False, False, False
    return form.fwd, form.bwd, form.zero


# ----------------------------------------------------------------- the yardstick
def _arrays(A):
    A = sp.csr_array(A)
    return (np.ascontiguousarray(A.indptr, dtype=np.int32), np.ascontiguousarray(A.indices, dtype=np.int32), np.ascontiguousarray(A.data))


def ld_op(A):
    """SparseOp of A with np.longdouble values (what _ld of tests/test_gpu_midsize.py makes of an operator)"""
    from dataclasses import replace
    op = sparse_op(sp.csr_array(A))
    return replace(op, data=op.data.astype(np.longdouble))


def ref_sweeps(A, x, b, how, iterations=1, dtype=np.float64):
    """the oracle's sequential sweep (amg_core::gauss_seidel restated in oracle/amg_oracle.c) on copies of A, x, b in `dtype` -- np.float64: what the
    device's exact order gives bit for bit; np.longdouble (x86-64: 64-bit mantissa): the yardstick"""
    Ap, Aj, Ax = _arrays(A)
    Ax = np.ascontiguousarray(Ax, dtype=dtype)
    xx, bb = np.array(x, dtype=dtype), np.ascontiguousarray(b, dtype=dtype)
    n = xx.size
    for _ in range(iterations):
        if how in ("forward", "symmetric"):
            orc.gauss_seidel(Ap, Aj, Ax, xx, bb, 0, n, 1)
        if how in ("backward", "symmetric"):
            orc.gauss_seidel(Ap, Aj, Ax, xx, bb, n - 1, -1, -1)
    return xx


def plain_sweep(A, x, b, how, iterations=1):
    """the same sweep as a plain Python loop in np.longdouble: pins the yardstick itself (tiny operators only)"""
    Ap, Aj, Ax = _arrays(A)
    Ax, x, b = Ax.astype(np.longdouble), np.array(x, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    n = x.size
    orders = {"forward": [range(n)], "backward": [range(n - 1, -1, -1)], "symmetric": [range(n), range(n - 1, -1, -1)]}[how]
    for _ in range(iterations):
        for rows in orders:
            for i in rows:
                s, d = np.longdouble(0), np.longdouble(0)
                for p in range(Ap[i], Ap[i + 1]):
                    if Aj[p] == i:
                        d = Ax[p]
                    else:
                        s = s + Ax[p] * x[Aj[p]]
                if d != 0:
                    x[i] = (b[i] - s) / d
    return x


def rel_err(got, ref):
    ref = np.asarray(ref)
    return float(np.max(np.abs(np.asarray(got, dtype=ref.dtype) - ref)) / np.max(np.abs(ref)))


def dependency_levels(A, direction):
    """number of dependency levels of the sweep of `direction` over all rows, as the planner counts them (sweep_levels, pamg_tile_plan.h): a row runs
    after every connected row visited before it and before every connected row visited after it -- connected through a stored entry in EITHER
    direction, so the rows of a triangle swept against its entries still form a deep schedule (every operand old) while a diagonal has one level"""
    Ap, Aj, _ = _arrays(A)
    n = len(Ap) - 1
    lvl, pend = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for i in (range(n) if direction > 0 else range(n - 1, -1, -1)):
        js = Aj[Ap[i]:Ap[i + 1]]
        before = js[js < i] if direction > 0 else js[js > i]
        after = js[js > i] if direction > 0 else js[js < i]
        lvl[i] = max(pend[i], 1 + lvl[before].max() if before.size else 0)
        if after.size:
            pend[after] = np.maximum(pend[after], lvl[i] + 1)
    return int(lvl.max()) + 1 if n else 0


# ----------------------------------------------------------------- solver level (device)
def solve_three_ways(spec, k, cycle, cpl, tune):
    """graph replay, a second replay, eager (bit for bit the same); returns (solver, x, residuals, sym_info per level before and after the eager solve)"""
    from pyamg_amd import DeviceMultilevelSolver
    from pyamg_amd import _capi as capi
    n = spec.levels[0].A.shape[0]
    x0 = np.random.RandomState(77).rand(n)
    b = np.zeros_like(x0)
    dml = DeviceMultilevelSolver(spec, graph=True, order="fast", level_tune=tune)
    r1, r2, r3 = [], [], []
    kw = dict(x0=x0, tol=1e-30, maxiter=k, cycle=cycle, cycles_per_level=cpl)
    x1 = dml.solve(b, residuals=r1, **kw)
    x2 = dml.solve(b, residuals=r2, **kw)
    capi.check(capi.lib().pamg_solver_set_graph(dml.handle, 0), "pamg_solver_set_graph")
    before = [A.sym_info() for A in dml.A]
    x3 = dml.solve(b, residuals=r3, **kw)
    after = [A.sym_info() for A in dml.A]
    assert np.array_equal(x1, x2) and r1 == r2, "a second solve must give the same bits"
    assert np.array_equal(x1, x3) and r1 == r3, "graph replay and eager launches must give the same bits"
    for i, A in enumerate(dml.A):
        assert not A.flow_error(), f"flow error on level {i}"
    return dml, x1, r1, (b, x0), before, after


def parity(tag, x, r, xo, ro):
    r = np.array(r)
    assert r.shape == ro.shape
    rel = float(np.max(np.abs(r - ro) / ro))
    dx = float(np.linalg.norm(x - xo) / np.linalg.norm(xo))
    print(f"[families] solver {tag}: residual norms {rel:.2e}, iterate {dx:.2e} against the oracle; {ro[0]:.3e} -> {ro[-1]:.3e}")
    assert rel <= 1e-10, (tag, rel)
    assert dx <= 1e-12, (tag, dx)
