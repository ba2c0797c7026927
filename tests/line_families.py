"""Named operator families for the LINE-SCAN fast-order Gauss-Seidel / SOR sweep (pyamg_amd/csrc/pamg_line.hip, planned by pamg_line_plan.h): the
banded shapes on which a kernel that consumes a sound plan can still go wrong.  A helper module like tests/sweep_families.py (whose yardstick it
reuses), shared by tests/test_line_families_plan.py (CPU replay of the planner through tests/line_emul.cpp) and tests/test_gpu_line_families.py
(the device).  Every family is deterministic (seeded), has between 4 096 and about 5 000 rows -- line_eligible needs 4 096, nothing here needs
more -- and DECLARES the form it must take: per sweep direction the planner's statistics (entry slots per row K, chunks, lines, levels of the
line graph), whether the symmetric sweep runs as ONE launch, and whether the device takes the form at all.  The tests assert that form, from the
replay's statistics on the CPU and from line_info / sym_info on the device -- a case that passes because the path under test stepped aside is
a failure.

What decides the form (pamg_line_plan.h: build_line_plan; pamg_line.hip: line_eligible, line_sym_launch; pamg_matrix.hip: sym_form_of):
  * the visit order is cut into chunks of at most 64 consecutive rows; a row starts a new chunk when it is not coupled to the row visited just
    before it (a new LINE starts there too) or when one of its other early operands lies inside its own chunk (the line goes on: `periodic2d`);
  * K = the most entries a row has besides its diagonal and the FIRST entry of its in-line predecessor; more than LINE_KMAX = 8 and the planner
    declines (`slot_overflow`, `row_too_long` -- the latter is not even asked: a stored row of more than LINE_KMAX + 2 entries);
  * fewer than 4 096 rows are not asked either (`below_threshold`);
  * the fused symmetric launch takes structurally symmetric patterns whose two directions have the same K; the others run two launches
    (`k8`, `nonsym_pattern`, `many_preds`: snapshots of the old values; `k_differs`: K 7 forward, 8 backward).
`growth_factor` is the amplification a 64-lane scan of the recurrence x_t = B_t + A_t x_{t-1} can see, computed from the operator alone."""
from __future__ import annotations

import ctypes
import functools
import subprocess
from dataclasses import dataclass
from pathlib import Path

import numpy as np
import scipy.sparse as sp

from oracle import oracle as orc
from sweep_families import U, _arrays, _finish, plain_sweep, ref_sweeps, rel_err, untouched_rows      # noqa: F401  (the shared yardstick)

U32 = 2.0 ** -24
LINE_KMAX = 8
MIN_ROWS = 4096                     # line_eligible
MAX_ROW_ENTRIES = LINE_KMAX + 2     # line_eligible: the longest stored row


@dataclass(frozen=True)
class Dir:
    """the planner's statistics of one sweep direction"""
    K: int
    chunks: int
    lines: int
    levels: int


@dataclass(frozen=True)
class Form:
    """what must run.  fwd / bwd: the plan of that direction, None where build_line_plan declines; `device`: line_eligible holds (enough rows, no
    stored row too long) -- otherwise the device never asks the planner and line_info reports 0 lines; `fused`: the symmetric sweep is one launch
    of gs_line_sym_kernel (sym_fused = 1, f64); `sym_pattern`: the pattern is structurally symmetric (otherwise the sweeps read old operands from
    a snapshot: replayed with snapshot = 1)"""
    fwd: Dir | None
    bwd: Dir | None
    fused: bool = True
    sym_pattern: bool = True
    device: bool = True

    def on_device(self, which):
        d = (self.fwd, self.bwd)[which]
        return d if self.device else None


@dataclass(frozen=True)
class Family:
    name: str
    make: object                      # make() -> scipy CSR (cached)
    form: Form
    note: str = ""


# ----------------------------------------------------------------- construction
def _stencil(shape, offsets, seed, periodic_fast=False, upwind=1.7):
    """COO triplets (no diagonal) of a stencil on a grid in lexicographic order, last axis fastest: values -(0.1 .. 1.0), seeded, times `upwind` on
    the "minus" neighbours (column < row): non-symmetric VALUES on a symmetric pattern where the offsets come in pairs"""
    shape = tuple(shape)
    idx = np.arange(int(np.prod(shape))).reshape(shape)
    coords = np.indices(shape)
    rows, cols = [], []
    for off in offsets:
        c = [coords[d] + off[d] for d in range(len(shape))]
        if periodic_fast:
            c[-1] = c[-1] % shape[-1]
        ok = np.all([(c[d] >= 0) & (c[d] < shape[d]) for d in range(len(shape))], axis=0)
        rows.append(idx[ok])
        cols.append(np.ravel_multi_index([cd[ok] for cd in c], shape))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = -(0.1 + 0.9 * np.random.RandomState(seed).rand(rows.size))
    vals[cols < rows] *= upwind
    return rows, cols, vals


def _dominant(n, rows, cols, vals, seed):
    """triplets with the diagonal a_ii = sum |a_ij| + 0.5 + rand appended: strictly diagonally dominant"""
    d = np.bincount(rows, weights=np.abs(vals), minlength=n) + 0.5 + np.random.RandomState(seed + 1000).rand(n)
    i = np.arange(n)
    return np.concatenate([rows, i]), np.concatenate([cols, i]), np.concatenate([vals, d])


def _csr(n, rows, cols, vals):
    """CSR from triplets; explicit zeros stay stored (no eliminate_zeros)"""
    A = _finish(sp.csr_array((vals, (rows, cols)), shape=(n, n)))
    assert A.nnz == rows.size, "duplicate entries"
    return A


def _drop(trip, mask):
    return tuple(a[~mask] for a in trip)


AXIS = {3: ((0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0)), 2: ((0, -1), (0, 1), (-1, 0), (1, 0))}
NINE = tuple((dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))


def var3d_shape(nx):
    return (6, -(-MIN_ROWS // (6 * nx)), nx)


def _var3d_triplets(shape, seed=201):
    n = int(np.prod(shape))
    return n, _dominant(n, *_stencil(shape, AXIS[3], seed), seed)


def var3d(shape):
    """7-point stencil, random coefficients, upwind factor on the minus neighbours, strictly dominant"""
    n, trip = _var3d_triplets(shape)
    return _csr(n, *trip)


def periodic2d():
    """5-point on 70 x 64, periodic along the fast axis: the last row of a grid line has an early operand (the line's first row) inside its own
    chunk, so each line is a 63-row chunk plus a coupled 1-row chunk that polls what its own wave published"""
    shape = (70, 64)
    n = shape[0] * shape[1]
    return _csr(n, *_dominant(n, *_stencil(shape, AXIS[2], 202, periodic_fast=True), 202))


def growth(n=4800, run=24):
    """tridiagonal, a_{t,t-1} = -1.5, a_tt = 1, a_{t,t+1} = -0.15, the coupling cut (both entries, not stored) every `run` rows.  NOT dominant:
    the prefix products of a forward line reach 1.5^(run - 1) ~ 1.1e4, those of a backward line stay below 1"""
    i = np.arange(1, n)
    i = i[i % run != 0]
    rows = np.concatenate([i, i - 1, np.arange(n)])
    cols = np.concatenate([i - 1, i, np.arange(n)])
    vals = np.concatenate([np.full(i.size, -1.5), np.full(i.size, -0.15), np.ones(n)])
    return _csr(n, rows, cols, vals)


def k8():
    """9-point on 70 x 64 plus one entry at (+2, 0): 10 entries per row, 8 of them besides the diagonal and the in-line predecessor (LINE_KMAX),
    a structurally non-symmetric pattern (snapshot path)"""
    shape = (70, 64)
    n = shape[0] * shape[1]
    return _csr(n, *_dominant(n, *_stencil(shape, NINE + ((2, 0),), 203), 203))


K_DIFFERS_ROW = 35 * 64 + 20
K_DIFFERS_FAR = tuple(K_DIFFERS_ROW + d for d in (-1280, -640, 640, 1280, 1920))


def k_differs():
    """5-point on 70 x 64, symmetric pattern; row r gets 5 symmetric far entries and loses its coupling to r + 1 (both entries): forward r is
    coupled to r - 1 and has 7 other entries, backward it starts a line and has 8"""
    shape = (70, 64)
    n = shape[0] * shape[1]
    rows, cols, vals = _stencil(shape, AXIS[2], 204)
    r = K_DIFFERS_ROW
    cut = ((rows == r) & (cols == r + 1)) | ((rows == r + 1) & (cols == r))
    assert cut.sum() == 2
    rows, cols, vals = _drop((rows, cols, vals), cut)
    far = np.array(K_DIFFERS_FAR)
    rows = np.concatenate([rows, np.full(5, r), far])
    cols = np.concatenate([cols, far, np.full(5, r)])
    vals = np.concatenate([vals, -(0.2 + 0.1 * np.arange(10))])
    return _csr(n, *_dominant(n, rows, cols, vals, 204))


def nonsym_pattern():
    """var3d_65 with the +nx entry removed from every third row"""
    shape = var3d_shape(65)
    n, (rows, cols, vals) = _var3d_triplets(shape)
    gone = (cols == rows + shape[2]) & (rows % 3 == 0)
    assert gone.sum() > n // 4
    return _csr(n, *_drop((rows, cols, vals), gone))


def holes_rows(n):
    """(cut, missing, zero, empty): rows whose coupling to the row before them is removed (both entries), rows whose diagonal is not stored, rows
    whose diagonal is stored as 0.0, the row that holds nothing"""
    cut = np.arange(97, n, 97)
    missing = np.arange(105, n, 211)
    zero = np.arange(150, n, 301)
    empty = n // 2 + 1
    assert not set(missing) & set(zero) and empty not in set(missing) | set(zero) | set(cut) | set(cut - 1)
    return cut, missing, zero, empty


def holes(shape=None, with_empty=True):
    """var3d_65 with: the coupling t <-> t - 1 removed every 97th row, the diagonal not stored every 211th row, a diagonal stored as 0.0 every
    301st row (the explicit zero stays stored), one completely empty row -- which other rows still read: the pattern is not symmetric, the
    sweeps read old operands from a snapshot and the symmetric sweep is two launches.  with_empty = False (`holes_sym`): that row keeps its
    entries and only loses its coupling to the row before it (both entries), so the pattern stays symmetric, the fused launch takes it, and
    its 111 lines do not divide the 4 290 rows: the wipe partition of the fused kernel has a remainder"""
    shape = shape or var3d_shape(65)
    n, (rows, cols, vals) = _var3d_triplets(shape)
    cut, missing, zero, empty = holes_rows(n)
    isd = rows == cols
    vals = vals.copy()
    vals[isd & np.isin(rows, zero)] = 0.0
    gone = (np.isin(rows, cut) & (cols == rows - 1)) | (np.isin(cols, cut) & (rows == cols - 1)) | (isd & np.isin(rows, missing))
    if with_empty:
        gone |= rows == empty
    else:
        gone |= ((rows == empty) & (cols == empty - 1)) | ((rows == empty - 1) & (cols == empty))
    A = _csr(n, *_drop((rows, cols, vals), gone))
    assert (A.indptr[empty] == A.indptr[empty + 1]) == with_empty
    assert np.array_equal(untouched_rows(A), np.sort(np.concatenate([missing, zero, [empty] if with_empty else []])))
    assert (A.data == 0.0).sum() == zero.size, "the explicit zeros must stay stored"
    return A


MANY_RUNS, MANY_RUN_ROWS, MANY_LINE = 40, 32, 3072
MANY_LATE_RUN = MANY_RUNS - 1       # the run that waits for run 0


def many_preds():
    """40 short coupled runs of 32 rows (tridiagonal), then ONE tridiagonal line of 3 072 rows whose row t also reads one row of short run
    (t mod 40) -- a one-directional entry, so every row stays at <= 4 entries.  Forward the line waits for 40 other lines, more than the
    planner's NPRED = 12: the `many` branch.  The first row of the LAST run reads a row of run 0, so that run sits on level 1 and the line, which
    meets it as its 40th predecessor, on level 2: a planner that looked at the first 12 predecessors only would put the line on level 1"""
    head = MANY_RUNS * MANY_RUN_ROWS
    n = head + MANY_LINE
    i = np.arange(1, n)
    i = i[(i % MANY_RUN_ROWS != 0) | (i > head)]              # coupled to the row before: inside a run, inside the line (the line starts at `head`)
    t = np.arange(MANY_LINE)
    extra = (t % MANY_RUNS) * MANY_RUN_ROWS + (t // MANY_RUNS) % MANY_RUN_ROWS
    rows = np.concatenate([i, i - 1, head + t, [MANY_LATE_RUN * MANY_RUN_ROWS]])
    cols = np.concatenate([i - 1, i, extra, [5]])
    r = np.random.RandomState(206)
    vals = -(0.1 + 0.9 * r.rand(rows.size))
    vals[cols < rows] *= 1.7
    return _csr(n, *_dominant(n, rows, cols, vals, 206))


def many_preds_line_predecessors(A):
    """from the pattern: (the number of distinct short runs the long line reads, the position of the run that waits for run 0 among them in
    the order the line meets them, counted from 1)"""
    A = sp.csr_array(A)
    head = MANY_RUNS * MANY_RUN_ROWS
    cols = A.indices[A.indptr[head]:]
    runs = cols[cols < head] // MANY_RUN_ROWS
    _, first = np.unique(runs, return_index=True)
    order = list(runs[np.sort(first)])
    late = A.indices[A.indptr[MANY_LATE_RUN * MANY_RUN_ROWS]:A.indptr[MANY_LATE_RUN * MANY_RUN_ROWS + 1]]
    assert np.any(late < MANY_RUN_ROWS), "the late run must read run 0"
    return len(order), order.index(MANY_LATE_RUN) + 1


SLOT_OVERFLOW_ROWS = tuple(64 * y + x for y, x in ((10, 5), (18, 40), (27, 58), (33, 12), (41, 30), (47, 7), (52, 50), (55, 21), (60, 33), (64, 44)))


def slot_overflow():
    """k8 where ten rows have an in-line neighbour replaced by a far entry at (+3, 0): five lose (0, -1), the forward predecessor, five lose
    (0, +1), the backward one -- 9 entries besides the diagonal with no predecessor to take one: more than LINE_KMAX in each direction"""
    shape = (70, 64)
    n = shape[0] * shape[1]
    rows, cols, vals = _stencil(shape, NINE + ((2, 0),), 203)
    cols = cols.copy()
    for k, r in enumerate(SLOT_OVERFLOW_ROWS):
        hit = (rows == r) & (cols == (r - 1 if k % 2 == 0 else r + 1))
        assert hit.sum() == 1
        cols[hit] = r + 3 * 64
    return _csr(n, *_dominant(n, rows, cols, vals, 203))


def row_too_long():
    """9-point plus (+-2, 0): 11 entries per row, one more than line_eligible takes"""
    shape = (70, 64)
    n = shape[0] * shape[1]
    return _csr(n, *_dominant(n, *_stencil(shape, NINE + ((2, 0), (-2, 0)), 207), 207))


def five_point(shape):
    n = shape[0] * shape[1]
    return _csr(n, *_dominant(n, *_stencil(shape, AXIS[2], 208), 208))


def _var3d_form(nx):
    nz, ny, _ = var3d_shape(nx)
    d = Dir(K=5, chunks=nz * ny * -(-nx // 64), lines=nz * ny, levels=nz + ny - 1)
    return Form(d, d)


_K8 = Dir(K=8, chunks=70, lines=70, levels=70)
_H = Dir(K=5, chunks=132, lines=111, levels=16)
FAMILIES = {f.name: f for f in (
    Family("var3d_63", lambda: var3d(var3d_shape(63)), _var3d_form(63), "a line is one chunk of 63 rows: lane 63 idles in every chunk"),
    Family("var3d_64", lambda: var3d(var3d_shape(64)), _var3d_form(64), "a line is exactly one full chunk"),
    Family("var3d_65", lambda: var3d(var3d_shape(65)), _var3d_form(65), "a full chunk, then a chunk of ONE row that takes the carry"),
    Family("var3d_129", lambda: var3d(var3d_shape(129)), _var3d_form(129), "two full chunks and a one-row chunk: the carry crosses twice"),
    Family("periodic2d", periodic2d, Form(Dir(4, 140, 70, 70), Dir(4, 140, 70, 70)), "63-row chunk + coupled 1-row chunk polling its own wave's value"),
    Family("growth", growth, Form(Dir(1, 200, 200, 1), Dir(1, 200, 200, 1)), "not dominant: prefix products up to 1.5^23 forward"),
    Family("k8", k8, Form(_K8, _K8, fused=False, sym_pattern=False), "K = LINE_KMAX slot sets, snapshot path"),
    Family("k_differs", k_differs, Form(Dir(7, 71, 71, 70), Dir(8, 71, 71, 70), fused=False), "K forward != K backward: the fused launch steps aside"),
    Family("nonsym_pattern", nonsym_pattern, Form(_var3d_form(65).fwd, _var3d_form(65).bwd, fused=False, sym_pattern=False), "snapshot path at K = 5"),
    Family("holes", holes, Form(_H, _H, fused=False, sym_pattern=False), "cut couplings, rows without a usable diagonal, an empty row that others read"),
    Family("holes_sym", lambda: holes(with_empty=False), Form(_H, _H), "a cut in place of the empty row: a symmetric pattern, the fused launch, lines that do not divide the rows"),
    Family("many_preds", many_preds, Form(Dir(2, 88, 41, 3), Dir(2, 88, 41, 1), fused=False, sym_pattern=False), "a line with 40 predecessor lines, the deepest met last"),
    Family("slot_overflow", slot_overflow, Form(None, None, fused=False, sym_pattern=False), "9 other entries in a row: the planner declines"),
    Family("row_too_long", row_too_long, Form(None, None, fused=False, device=False), "11 entries per row: line_eligible is false"),
    Family("below_threshold", lambda: five_point((63, 65)), Form(Dir(3, 126, 63, 63), Dir(3, 126, 63, 63), fused=False, device=False), "4 095 rows: not asked"),
    Family("at_threshold", lambda: five_point((64, 64)), Form(Dir(3, 64, 64, 64), Dir(3, 64, 64, 64)), "4 096 rows: the smallest operator that is"),
)}
WIPE_REMAINDER = ("holes_sym",)        # fused families whose lines do not divide the rows: the fused kernel's wipe partition n = wq lines + wr has wr != 0
SMALL = {                              # about 300 rows: where a plain Python loop in long double pins the yardstick
    "var3d_65": lambda: var3d((2, 2, 65)),
    "growth": lambda: growth(312, 24),
    "holes": lambda: holes((2, 2, 65)),
}


@functools.lru_cache(maxsize=None)
def operator(name):
    return FAMILIES[name].make()


# ----------------------------------------------------------------- the CPU replay (tests/line_emul.cpp)
def build_emul(out):
    """tests/line_emul.cpp built into directory `out` on the project's planner (rebuilt when the source or pamg_line_plan.h is newer); the loaded library"""
    here = Path(__file__).resolve().parent
    out.mkdir(parents=True, exist_ok=True)
    so, src, hdr = out / "line_emul.so", here / "line_emul.cpp", here.parent / "pyamg_amd" / "csrc" / "pamg_line_plan.h"
    if not so.exists() or so.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.line_emul_sweep_f64.restype = ctypes.c_int
    return lib


def run_emul(lib, A, x, b, start, stop, step, sor=0, omega=1.0, snapshot=0, waves=7):
    """(rc, x, statistics [K, chunks, lines, levels, early, old, widest level, -]) of one replayed sweep"""
    A = sp.csr_array(A)
    Ap = np.ascontiguousarray(A.indptr, dtype=np.int32)
    Aj = np.ascontiguousarray(A.indices, dtype=np.int32)
    Ax = np.ascontiguousarray(A.data, dtype=np.float64)
    xx = np.array(x, dtype=np.float64)
    stats = np.zeros(8, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.line_emul_sweep_f64(ctypes.c_int(A.shape[0]), p(Ap), p(Aj), p(Ax), p(xx), p(np.ascontiguousarray(b, dtype=np.float64)),
                                 start, stop, step, sor, ctypes.c_double(omega), snapshot, waves, p(stats))
    return rc, xx, stats


# ----------------------------------------------------------------- the yardstick
def growth_factor(A, step, omega=1.0):
    """the largest product of |omega a_{t,prev} / a_tt| over at most 63 consecutive coupled rows in sweep order (step = +1: prev = t - 1; -1:
    prev = t + 1), never less than 1: the amplification a 64-lane scan of the recurrence can see.  From the operator alone (duplicate entries
    summed; a row without a usable diagonal is not updated and ends a run)"""
    A = sp.csr_array(A)
    n = A.shape[0]
    d = A.diagonal()
    off = np.zeros(n)
    if step > 0:
        off[1:] = A.diagonal(-1)                                  # a_{t,t-1}
    else:
        off[:-1] = A.diagonal(1)                                  # a_{t,t+1}
        off, d = off[::-1], d[::-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(d != 0.0, np.abs(omega * off / d), 0.0)
    best, cur = max(1.0, float(f.max(initial=0.0))), f.copy()
    for k in range(1, 63):                                        # cur[i] = f[i] ... f[i + k]
        if cur.size <= 1:
            break
        cur = cur[:-1] * f[k:]
        best = max(best, float(cur.max()))
    return best


def ref_sor(A, x, b, how, omega, dtype=np.float64):
    """the oracle's sequential SOR sweep (amg_core::sor_gauss_seidel restated in oracle/amg_oracle.c) on copies in `dtype`"""
    Ap, Aj, Ax = _arrays(A)
    Ax = np.ascontiguousarray(Ax, dtype=dtype)
    xx, bb = np.array(x, dtype=dtype), np.ascontiguousarray(b, dtype=dtype)
    n = xx.size
    if how == "forward":
        orc.sor_gauss_seidel(Ap, Aj, Ax, xx, bb, 0, n, 1, omega)
    else:
        orc.sor_gauss_seidel(Ap, Aj, Ax, xx, bb, n - 1, -1, -1, omega)
    return xx


def plain_sor(A, x, b, how, omega):
    """the same SOR sweep as a plain Python loop in np.longdouble (tiny operators only)"""
    Ap, Aj, Ax = _arrays(A)
    L = np.longdouble
    Ax, x, b, omega = Ax.astype(L), np.array(x, dtype=L), np.asarray(b, dtype=L), L(omega)
    n = x.size
    for i in (range(n) if how == "forward" else range(n - 1, -1, -1)):
        s, d = L(0), L(0)
        for p in range(Ap[i], Ap[i + 1]):
            if Aj[p] == i:
                d = Ax[p]
            else:
                s = s + Ax[p] * x[Aj[p]]
        if d != 0:
            x[i] = omega * ((b[i] - s) / d) + (1 - omega) * x[i]
    return x


def bar(e_seq, g, u=U):
    """e_dev <= max(8 e_seq, 32 u g): e_seq the sequential sweep's own error in the working precision against long double, g = growth_factor"""
    return max(8.0 * e_seq, 32.0 * u * g)
