"""Named subdomain families for the persistent overlapping-Schwarz sweep (pyamg_amd/csrc/pamg_schwarz.hip: schwarz_versioned_kernel and its per-level
twin schwarz_level_kernel; plan in pamg_schwarz_plan.h).  A helper module like tests/block_kz_families.py, shared by
tests/test_schwarz_families_plan.py (CPU replay of the plan, "small") and tests/test_gpu_schwarz_families.py (the device, "large").  Every family is
deterministic (seeded); make(size) returns (A, Sp, Sj, Tp, Tx) and the family DECLARES what must run (Form): the persistent versioned form, the
per-level launches because the planner declines (with its code) or because the schedule has one level, or a handle that is refused at create -- a
case that passes because the path under test stepped aside is a failure, except where stepping aside is the declaration.

Tx holds the inverses of A[S, S] (numpy, f64; pseudo-inverses for blocks of at most 256 rows, which covers the singular ones: a row listed twice,
a row without a diagonal entry), rounded to multiples of 2^-24; the operators are strictly diagonally dominant wherever a diagonal entry is
stored, so a few sweeps stay finite (every expected result is asserted finite, so that equal bits never means equal NaNs).  The device and the oracle get the same arrays, so how good the inverses are does not enter: the claim under test is bit identity with the
sequential sweep of amg_core::overlapping_schwarz_csr (relaxation.h:1420-1492)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

from oracle import oracle as orc

SW_PRE, SW_LANES, SW_MAX, SW_CH = 8, 64, 2048, 8          # pamg_schwarz.hip: block row in registers / one lane per row / LDS limit / reads in flight
MAX_UPDATES = 255                                        # pamg_schwarz_plan.h: one byte per version code


@dataclass(frozen=True)
class Form:
    """runs: "versioned" (every sweep has at least two levels and runs as ONE persistent launch under mode 0), "declined" (the planner declines
    with `declined`: per-level launches under both modes), "one_level" (a schedule of one dependency level goes to the level kernel by design),
    "rejected" (pamg_schwarz_create returns PAMG_E_UNSUPPORTED), "nothing" (no subdomain: nothing to sweep).
    largest: rows of the largest subdomain; updates: the most updates a row gets in a full sweep (small, large)"""
    runs: str
    largest: int
    updates: tuple
    declined: int = 0


@dataclass(frozen=True)
class Family:
    name: str
    make: object                                  # make(size) -> (A, Sp, Sj, Tp, Tx)
    form: Form
    sweeps: object = None                         # sweeps(nsub) -> [(name, (start, stop, step))]; None: default_sweeps
    strided: Form = None                          # the form of the strided sweep where it differs (it visits a third of the subdomains)
    f32: bool = False                             # run in float32 on the device too
    note: str = ""


def default_sweeps(nsub):
    """forward, backward and a stride of 3 from subdomain 2 (the reference loops `d != row_stop`: the stride hits it)"""
    return [("forward", (0, nsub, 1)), ("backward", (nsub - 1, -1, -1)), ("strided", (2, 2 + 3 * ((nsub - 3) // 3), 3))]


def sweeps_of(fam, nsub):
    return fam.sweeps(nsub) if fam.sweeps else default_sweeps(nsub)


def form_of(fam, sweep):
    return fam.strided if (sweep == "strided" and fam.strided is not None) else fam.form


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


# ================================================================= operators and blocks
def dominant(P, seed, zero_frac=0.0, nodiag=()):
    """CSR operator on the pattern of P plus the diagonal (minus the diagonal entries of the rows `nodiag`): off-diagonal values of random sign,
    magnitude in [0.1, 1], a fraction `zero_frac` of them STORED zeros; diagonal = 1 + the row's absolute off-diagonal sum"""
    n = P.shape[0]
    r = np.random.RandomState(seed)
    P = sp.coo_array(P)
    keep = P.row != P.col
    rows, cols = P.row[keep], P.col[keep]
    dr = np.setdiff1d(np.arange(n), np.asarray(nodiag, dtype=np.int64))
    pat = sp.csr_array((np.ones(rows.size + dr.size), (np.concatenate([rows, dr]), np.concatenate([cols, dr]))), shape=(n, n))
    pat.sum_duplicates()
    pat.sort_indices()
    rr = np.repeat(np.arange(n), np.diff(pat.indptr))
    off = rr != pat.indices
    data = (0.1 + 0.9 * r.rand(pat.nnz)) * np.where(r.rand(pat.nnz) < 0.5, -1.0, 1.0)
    data[off & (r.rand(pat.nnz) < zero_frac)] = 0.0
    rowsum = np.bincount(rr[off], weights=np.abs(data[off]), minlength=n)
    data[~off] = 1.0 + rowsum[rr[~off]]
    A = sp.csr_matrix((data, pat.indices.astype(np.int32), pat.indptr.astype(np.int32)), shape=(n, n))
    assert A.has_sorted_indices or not A.sort_indices()
    return A


def banded(n, offsets, extra=0.0, seed=0):
    P = sp.diags_array([np.ones(n - abs(o)) for o in offsets], offsets=list(offsets), shape=(n, n), format="csr")
    if extra > 0:
        P = P + sp.random(n, n, density=extra, random_state=np.random.RandomState(seed), format="csr")
    return sp.csr_array(P)


def blocks(A, Sp, Sj):
    """Tp, Tx: the inverse of A[S, S] for every subdomain, row-major (pinv up to 256 rows, inv beyond)"""
    Ad = A.toarray()
    Sp, Sj = np.asarray(Sp), np.asarray(Sj)
    Tp = np.zeros(len(Sp), dtype=np.int64)
    Tp[1:] = np.cumsum(np.diff(Sp).astype(np.int64) ** 2)
    assert Tp[-1] < 2 ** 31
    Tx = np.zeros(int(Tp[-1]))
    for d in range(len(Sp) - 1):
        rows = Sj[Sp[d]:Sp[d + 1]]
        if rows.size:
            blk = Ad[np.ix_(rows, rows)]
            Tx[Tp[d]:Tp[d + 1]] = (np.linalg.pinv(blk) if rows.size <= 256 else np.linalg.inv(blk)).ravel()
    assert np.isfinite(Tx).all()
    # multiples of 2^-24: the last bits of a LAPACK result may differ from machine to machine, these do not (the committed expectations of
    # tests/golden/kernels_schwarz_families.npz were computed from them elsewhere); still the inverse to seven digits
    return i32(Tp), np.round(Tx * 2.0 ** 24) / 2.0 ** 24


def pack(A, subs):
    Sp = np.zeros(len(subs) + 1, dtype=np.int64)
    Sp[1:] = np.cumsum([len(s) for s in subs])
    Sj = np.concatenate([np.asarray(s, dtype=np.int64) for s in subs]) if len(subs) and Sp[-1] else np.zeros(0, dtype=np.int64)
    Sp, Sj = i32(Sp), i32(Sj)
    Tp, Tx = blocks(A, Sp, Sj)
    return A, Sp, Sj, Tp, Tx


def window_subs(r, n, sizes, spread=2.0, lo=0, hi=None):
    """one subdomain per entry of `sizes`: that many distinct rows (sorted) out of a window of about spread x size rows at a random place"""
    hi = n if hi is None else hi
    subs = []
    for s in sizes:
        w = min(hi - lo, max(int(spread * s) + 4, s))
        c = lo + r.randint(0, hi - lo - w + 1)
        subs.append(np.sort(r.choice(np.arange(c, c + w), size=s, replace=False)))
    return subs


# ================================================================= the families
EDGE_SIZES = (0, 1, 2, 7, 8, 9, 63, 64, 65, 66, 127, 128, 129)


def size_edges(size):
    """every size at which schwarz_versioned_kernel changes path, several times over, in a shuffled order on overlapping windows"""
    n, rounds = (1500, 2) if size == "small" else (3000, 5)
    r = np.random.RandomState(401)
    A = dominant(banded(n, (-2, -1, 0, 1, 3), extra=0.2 / n, seed=402), 403)           # (a few far entries: most windows stay independent)
    sizes = np.concatenate([r.permutation(EDGE_SIZES) for _ in range(rounds)])
    return pack(A, window_subs(r, n, sizes))


def all_big(size):
    """65 .. 200 rows per subdomain out of windows that slide by 40 rows: every subdomain overlaps the one before it"""
    nsub = 24 if size == "small" else 60
    r = np.random.RandomState(411)
    n = 40 * nsub + 260
    A = dominant(banded(n, (-3, -1, 0, 1, 2), extra=0.001, seed=412), 413)
    sizes = r.randint(65, 201, size=nsub)
    sizes[[1, nsub // 2]] = (65, 200)
    subs = [np.sort(r.choice(np.arange(40 * d, 40 * d + 260), size=s, replace=False)) for d, s in enumerate(sizes)]
    return pack(A, subs)


def one_2048(size):
    """a chain {i, i + 1} over the first rows, ONE subdomain of 2048 of the 2400 rows, a chain over the last rows"""
    n, L = 2400, (20 if size == "small" else 80)
    r = np.random.RandomState(421)
    A = dominant(banded(n, (-3, -2, -1, 0, 1, 2, 3)), 422)
    big = np.sort(r.choice(n, size=SW_MAX, replace=False))
    subs = [[i, i + 1] for i in range(L)] + [big] + [[i, i + 1] for i in range(n - L - 1, n - 1)]
    return pack(A, subs)


def too_big(size):
    n = 2100
    r = np.random.RandomState(431)
    A = dominant(banded(n, (-1, 0, 1)), 432)
    return pack(A, [np.sort(r.choice(n, size=SW_MAX + 1, replace=False))])


ROW_LENGTHS = (1, 8, 9, 16, 17, 64, 257)


def long_rows_nodiag(n):
    return np.arange(4, n, 11)


def long_rows(size):
    """rows of 1, 8, 9, 16, 17, 64 and 257 stored entries (the chunks of SW_CH = 8 reads: full, one over, many), 15 % of the off-diagonal entries
    stored zeros, every 11th row without a diagonal entry"""
    n, nsub = (400, 150) if size == "small" else (1500, 600)
    r = np.random.RandomState(441)
    nodiag = set(long_rows_nodiag(n).tolist())
    lens = np.asarray(ROW_LENGTHS)[r.randint(0, 6, size=n)]
    lens[r.choice(n, size=n // 50, replace=False)] = 257
    lens[:7] = ROW_LENGTHS                                                           # every length at least once, with and without a diagonal
    rows, cols = [], []
    for i in range(n):
        k = int(lens[i]) - (0 if i in nodiag else 1)
        js = r.choice(np.setdiff1d(np.arange(n), [i]), size=k, replace=False)
        rows += [i] * k
        cols += js.tolist()
    P = sp.csr_array((np.ones(len(rows)), (rows, cols)), shape=(n, n))
    A = dominant(P, 442, zero_frac=0.15, nodiag=sorted(nodiag))
    assert np.array_equal(np.diff(A.indptr), lens) and (A.data == 0).sum() > n and not np.any(A.diagonal()[long_rows_nodiag(n)])
    subs = [r.choice(n, size=r.randint(1, 13), replace=False) for _ in range(nsub)]
    return pack(A, subs)


def nonsym_unused(n):
    """rows that are in no subdomain of nonsym_pattern"""
    return np.arange(5, n, 17)


def nonsym_pattern(size):
    """a strictly lower triangular band plus a sparse random part; subdomains of 1 .. 12 distinct rows out of the first half or all rows (as
    test_irregular_subdomains_and_nonsymmetric_pattern draws them), never one of nonsym_unused"""
    n, nsub = (400, 300) if size == "small" else (3000, 2000)
    r = np.random.RandomState(451)
    A = dominant(banded(n, (-7, -2, -1, 0), extra=2.0 / n, seed=452), 453)
    assert (A != A.T).nnz > A.nnz // 2
    pool = np.setdiff1d(np.arange(n), nonsym_unused(n))
    subs = []
    for _ in range(nsub):
        k = r.randint(1, 13)
        subs.append(r.choice(pool[:pool.size // 2] if r.rand() < 0.5 else pool, size=k, replace=False))
    return pack(A, subs)


HUB = 17


def _hub(count):
    def make(size):
        """`count` subdomains hold row HUB (anywhere in their list) next to 1 .. 3 other rows; 40 more subdomains do not hold it"""
        n = 600
        r = np.random.RandomState(460 + count)
        A = dominant(banded(n, (-1, 0, 1), extra=0.004, seed=461), 462)
        others = np.setdiff1d(np.arange(n), [HUB])
        subs = []
        for d in range(count + 40):
            s = r.choice(others, size=r.randint(1, 4), replace=False).tolist()
            if d % (count + 40) not in _hub_free(count):
                s.insert(r.randint(0, len(s) + 1), HUB)
            subs.append(s)
        assert sum(HUB in s for s in subs) == count
        return pack(A, subs)
    return make


def _hub_free(count):
    """the 40 positions of the list whose subdomains do not hold the hub"""
    return set(np.random.RandomState(470).choice(count + 40, size=40, replace=False).tolist())


def chain(size):
    """subdomains {i, i + 1} on a band of half-width 3: every subdomain waits for the one before it, also at a stride of 3"""
    n = 200 if size == "small" else 1500
    A = dominant(banded(n, (-3, -2, -1, 0, 1, 2, 3)), 481)
    return pack(A, [[i, i + 1] for i in range(n - 1)])


def one_level(size):
    """a block-diagonal operator (blocks of 1 .. 9 rows), one subdomain per block"""
    nblk = 60 if size == "small" else 600
    r = np.random.RandomState(491)
    bs = r.randint(1, 10, size=nblk)
    P = sp.block_diag([np.ones((b, b)) for b in bs], format="csr")
    A = dominant(P, 492)
    off = np.concatenate([[0], np.cumsum(bs)])
    return pack(A, [np.arange(off[k], off[k + 1]) for k in range(nblk)])


DUP_AT = (5, 47, 101, 140)                       # all = 2 mod 3: the strided sweep visits them too


def dup_row(size):
    """subdomains of 2 .. 10 rows; four of them list a row twice: apart (5), twice in a row (47), in a subdomain of 70 rows (101), and a row three
    times (140)"""
    n, nsub = (300, 150) if size == "small" else (900, 300)
    r = np.random.RandomState(501)
    A = dominant(banded(n, (-2, -1, 0, 1, 4), extra=0.003, seed=502), 503)
    subs = [s.tolist() for s in window_subs(r, n, r.randint(2, 11, size=nsub), spread=3.0)]
    s = subs[DUP_AT[0]]
    subs[DUP_AT[0]] = s + [s[0]]                                                      # first and last
    s = subs[DUP_AT[1]]
    subs[DUP_AT[1]] = s[:1] + s[:1] + s[1:]                                           # twice in a row
    s = window_subs(r, n, [69], spread=1.5)[0].tolist()
    subs[DUP_AT[2]] = s[:40] + [s[3]] + s[40:]                                        # lanes loop over the rows
    s = subs[DUP_AT[3]]
    subs[DUP_AT[3]] = [s[1]] + s + [s[1]]                                             # three times
    assert len(subs[DUP_AT[2]]) == 70
    return pack(A, subs)


def unsorted_members(size):
    """subdomain lists in descending (even) and in shuffled (odd) order, one of 100 rows among them"""
    n, nsub = (300, 80) if size == "small" else (1500, 400)
    r = np.random.RandomState(511)
    A = dominant(banded(n, (-2, -1, 0, 1, 3), extra=0.002, seed=512), 513)
    sizes = r.randint(2, 41, size=nsub)
    sizes[7] = 100
    subs = window_subs(r, n, sizes)
    subs = [s[::-1].copy() if d % 2 == 0 else r.permutation(s) for d, s in enumerate(subs)]
    assert any(np.any(np.diff(s) > 0) and np.any(np.diff(s) < 0) for s in subs)
    return pack(A, subs)


def _tiny(n):
    def make(size):
        A = dominant(sp.csr_array(np.ones((n, n))), 520 + n)
        return pack(A, [np.random.RandomState(521 + n).permutation(n)])
    return make


def tiny_nosub(size):
    return pack(dominant(sp.csr_array(np.ones((4, 4))), 529), [])


REGROW_SMALL = 60


def regrow(size):
    """the first 60 subdomains hold 2 rows, the others 12 .. 20: a strided sweep over the others needs more slots than the sweeps over the first 60"""
    n, nsub = 1200, 300
    r = np.random.RandomState(531)
    A = dominant(banded(n, (-2, -1, 0, 1, 2)), 532)
    subs = window_subs(r, n, [2] * REGROW_SMALL, lo=0, hi=60) + window_subs(r, n, r.randint(12, 21, size=nsub - REGROW_SMALL), lo=40, hi=n)
    return pack(A, subs)


def regrow_sweeps(nsub):
    a = REGROW_SMALL
    fwd = ("forward_small", (0, a, 1))
    return [fwd, ("backward_small", (a - 1, -1, -1)), ("strided", (a, a + 2 * ((nsub - a) // 2), 2)), ("forward_again", fwd[1])]


def tiny_sweeps(nsub):
    return [("forward", (0, 1, 1)), ("backward", (0, -1, -1))]


def nosub_sweeps(nsub):
    return [("forward", (0, 0, 1))]


def hub_sweeps(nsub):
    return default_sweeps(nsub)


V = "versioned"
FAMILIES = {f.name: f for f in (
    Family("size_edges", size_edges, Form(V, 129, (5, 5)), f32=True, note="0 .. 129 rows: registers / L1 / one lane per row / the lane loop"),
    Family("all_big", all_big, Form(V, 200, (7, 7)), note="only the lane loop, a schedule of 20 levels and more"),
    Family("one_2048", one_2048, Form(V, SW_MAX, (3, 3)), note="the largest subdomain the handle accepts"),
    Family("too_big", too_big, Form("rejected", SW_MAX + 1, (1, 1)), sweeps=tiny_sweeps),
    Family("long_rows", long_rows, Form(V, 12, (9, 10)), f32=True, note="the chunk edges of the read loop, stored zeros, rows without a diagonal"),
    Family("nonsym_pattern", nonsym_pattern, Form(V, 12, (18, 17)), f32=True, note="write-after-read edges that are no read-after-write edges"),
    Family("hub_255", _hub(255), Form(V, 4, (255, 255)), note="the last count a version byte holds"),
    Family("hub_256", _hub(256), Form("declined", 4, (256, 256), declined=1), strided=Form(V, 4, (256, 256)),
           note="one more: the planner declines; a stride of 3 visits a third of them and is versioned again"),
    Family("chain", chain, Form(V, 2, (2, 2)), note="as many levels as subdomains, every level of width 1"),
    Family("one_level", one_level, Form("one_level", 9, (1, 1))),
    Family("dup_row", dup_row, Form("declined", 70, (10, 7), declined=3), note="a row listed twice takes both increments, in list order"),
    Family("unsorted_members", unsorted_members, Form(V, 100, (16, 15))),
    *(Family(f"tiny_{n}", _tiny(n), Form("one_level", n, (1, 1)), sweeps=tiny_sweeps) for n in (1, 2, 3, 5)),
    Family("tiny_nosub", tiny_nosub, Form("nothing", 0, (0, 0)), sweeps=nosub_sweeps),
    Family("regrow", regrow, Form(V, 20, (10, 10)), sweeps=regrow_sweeps, note="a third schedule evicts the second and needs a larger hand-off buffer"),
)}


# ================================================================= the yardstick and what a family is
def reference(A, Sp, Sj, Tp, Tx, x, b, sweep, times=1, dtype=np.float64):
    """the oracle's sequential sweep (amg_core::overlapping_schwarz_csr restated in oracle/amg_oracle.c), `times` in a row, in `dtype`"""
    xx = np.array(x, dtype=dtype)
    Ax, bb, TT = np.ascontiguousarray(A.data, dtype=dtype), np.ascontiguousarray(b, dtype=dtype), np.ascontiguousarray(Tx, dtype=dtype)
    for _ in range(times):
        orc.overlapping_schwarz_csr(i32(A.indptr), i32(A.indices), Ax, xx, bb, TT, i32(Tp), i32(Sj), i32(Sp), *sweep)
    assert np.isfinite(xx).all()
    return xx


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(u), b.view(u))


def start_vectors(n):
    r = np.random.RandomState(7)
    return r.rand(n) - 0.3, r.rand(n) - 0.5


def without_empty(Sp):
    """the subdomain offsets without the subdomains of no rows (Sj stays): the reference's SETUP cannot invert a block of no rows (its gelss call
    fails), so relaxation.schwarz, which builds the blocks itself, gets the other subdomains"""
    Sp = np.asarray(Sp)
    return i32(np.concatenate([Sp[:1], Sp[1:][np.diff(Sp) > 0]]))


def largest(Sp):
    return int(np.diff(Sp).max()) if len(Sp) > 1 else 0


def most_updates(n, Sj):
    return int(np.bincount(Sj, minlength=n).max()) if len(Sj) else 0


def visited_rows(Sp, Sj, sweep):
    ds = range(*sweep)
    return np.unique(np.concatenate([Sj[Sp[d]:Sp[d + 1]] for d in ds])) if len(ds) else np.zeros(0, dtype=np.int32)


def has_duplicate(Sp, Sj, sweep):
    return any(np.unique(Sj[Sp[d]:Sp[d + 1]]).size != Sp[d + 1] - Sp[d] for d in range(*sweep))


def levels_of(A, Sp, Sj, sweep):
    """schwarz_levels in plain Python: the dependency level of every visited subdomain, in sweep order"""
    n = A.shape[0]
    lastW, lastR = np.full(n, -1), np.full(n, -1)
    out = []
    for d in range(*sweep):
        rows = Sj[Sp[d]:Sp[d + 1]]
        cols = np.concatenate([A.indices[A.indptr[i]:A.indptr[i + 1]] for i in rows]) if rows.size else np.zeros(0, dtype=np.int64)
        L = max([0] + (np.maximum(lastW[rows], lastR[rows]) + 1).tolist() + (lastW[cols] + 1).tolist())
        out.append(int(L))
        lastW[rows] = np.maximum(lastW[rows], L)
        lastR[cols] = np.maximum(lastR[cols], L)
    return out
