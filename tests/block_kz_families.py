"""Named operator families for the two other persistent fast-order sweeps: the lane-parallel BLOCK Gauss-Seidel sweep (pyamg_amd/csrc/pamg_blane.hip,
plan in pamg_blane_plan.h) and the lane-parallel KACZMARZ sweeps (pamg_kz.hip, plan in pamg_kz_plan.h).  A helper module like tests/sweep_families.py,
shared by tests/test_block_kz_families_plan.py (CPU replay of the planners, small size) and tests/test_gpu_block_kz_families.py (the device, large
size).  Every family is deterministic (seeded) and DECLARES the form it must take: lanes per row / line and slots per lane, or "the planner declines /
there is nothing to hand over" -- a case that passes because the path under test stepped aside is a failure.

What decides the form:
  * Kaczmarz (build_kz_lane_plan): lane_geometry of the LONGEST LINE -- 4 lanes x up to 4 slots for lines of at most 16 entries, then 8 x 3 .. 4
    (17 .. 32), 16 x 3 .. 4 (.. 64), 32 x 3 .. 4 (.. 128), 64 x 3 .. 4 (.. 256); a line of 257 entries, or one that holds an index twice, makes the
    planner decline and the order-exact kernels keep the sweep (`groups == 0`, the oracle's bits).  Lines are the ROWS of the operator handed in: A
    for gauss_seidel_ne, A^T for gauss_seidel_nr; a family is that operator, both kinds see the same lines.
  * block Gauss-Seidel (build_blane_plan, build_blane_part): as many lanes per block row as the longest row has off-diagonal blocks, a power of two,
    at least max(8, lane_L), at most 64; one block per lane, two where the longest row has 65 .. 128; a row of 129 makes the planner decline; a
    schedule of ONE dependency level (block-diagonal operator) has nothing to hand over (blane_eligible) -- both: `groups == 0`, the oracle's bits.
The long-double yardsticks are here too: the oracle's own loops (orc.block_gauss_seidel, orc.gauss_seidel_ne, orc.gauss_seidel_nr) on np.longdouble
copies, each pinned once against a plain Python long-double loop (plain_*)."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp

from oracle import oracle as orc
from pyamg_amd.hierarchy import _normal_equation_spec

U = 2.0 ** -53
L_ = np.longdouble
KZ_TINY = (1, 2, 3, 5, 9, 63, 65)
B_TINY = (2, 3, 5, 9)
SWEEPS = ("forward", "backward", "symmetric")
KINDS = (("gauss_seidel_ne", 0.9), ("gauss_seidel_nr", 1.1))


@dataclass(frozen=True)
class Form:
    """what must run.  `lanes`, `slots`: lanes per block row / line and blocks / entries per lane (block families: at lane_L = 0, i.e. want_L = 8);
    `longest`: entries of the longest line resp. off-diagonal blocks of the longest block row (the geometry under a forced lane_L follows from it:
    block_geometry); `declines`: the planner declines or the schedule has one level -- groups == 0 and the oracle's bits, replay return code 2
    (`one_level`: the planner itself would accept, the device never asks it)"""
    lanes: int = 0
    slots: int = 0
    longest: int = 0
    declines: bool = False
    one_level: bool = False


@dataclass(frozen=True)
class Family:
    name: str
    make: object                                  # Kaczmarz: make(size) -> CSR whose rows are the lines; block: make(size, bs) -> BSR
    form: Form = field(default_factory=Form)
    tol: float = 1e-13                            # against the f64 sequential sweep, relative
    other_bs: int = 0                             # block families: the block size run next to 3
    device: bool = True                           # False: CPU tests only
    note: str = ""


def kz_geometry(longest):
    """lane_geometry (pamg_lane_plan.h) of a longest line: (lanes, slots), (0, 0) where the plan declines"""
    for lanes in (4, 8, 16, 32, 64):
        k = max(1, -(-longest // lanes))
        if k <= 4:
            return lanes, k
    return 0, 0


def block_geometry(form, lane_L=0):
    """(lanes per block row, blocks per lane) of build_blane_plan for want_L = max(8, lane_L)"""
    lanes = 4
    while lanes < 64 and (lanes < form.longest or lanes < max(8, lane_L)):
        lanes *= 2
    return lanes, max(1, -(-form.longest // lanes))


# ================================================================= Kaczmarz families
def _csr(indptr, indices, data, shape):
    A = sp.csr_array((np.asarray(data, dtype=np.float64), np.asarray(indices, dtype=np.int32), np.asarray(indptr, dtype=np.int32)), shape=shape)
    return A


def _lines(nrows, ncols, lens, seed, allowed=None, forced=None):
    """CSR of nrows lines over ncols indices: line i holds lens[i] distinct indices drawn from `allowed` (default: all), sorted, among them
    forced[i] (a list) where given; values of random sign, magnitude in [0.1, 1]"""
    r = np.random.RandomState(seed)
    allowed = np.arange(ncols) if allowed is None else np.asarray(allowed)
    indptr, indices = [0], []
    for i in range(nrows):
        must = np.asarray(forced[i], dtype=np.int64) if forced is not None and forced[i] is not None else np.zeros(0, dtype=np.int64)
        pool = np.setdiff1d(allowed, must) if must.size else allowed
        free = r.choice(pool, size=int(lens[i]) - must.size, replace=False) if lens[i] > must.size else np.zeros(0, dtype=np.int64)
        js = np.sort(np.concatenate([must, free]))
        assert js.size == lens[i] and np.unique(js).size == js.size
        indices.extend(js.tolist())
        indptr.append(len(indices))
    vals = (0.1 + 0.9 * r.rand(len(indices))) * np.where(r.rand(len(indices)) < 0.5, -1.0, 1.0)
    return _csr(indptr, indices, vals, (nrows, ncols))


def kz_nonsym(size):
    n = 300 if size == "small" else 3000
    return _lines(n, n, np.full(n, 12), 201)


def kz_rect_wide(size):
    m, n = (60, 400) if size == "small" else (300, 2000)
    return _lines(m, n, np.full(m, 12), 202)


def kz_rect_tall(size):
    m, n = (400, 60) if size == "small" else (2000, 300)
    return _lines(m, n, np.full(m, 12), 203)


def kz_arrow(size):
    """every line holds index 0 and five others: as many dependency levels as lines, index 0 rewritten by every line"""
    n = 200 if size == "small" else 3000
    return _lines(n, n, np.full(n, 6), 204, allowed=np.arange(1, n), forced=[[0]] * n)


def kz_chain(size):
    """bidiagonal: line i holds the indices i and i + 1 (n + 1 indices): levels = lines, two entries per line"""
    n = 200 if size == "small" else 2000
    r = np.random.RandomState(205)
    idx = np.stack([np.arange(n), np.arange(n) + 1], axis=1).ravel()
    return _csr(np.arange(0, 2 * n + 1, 2), idx, 0.3 + r.rand(2 * n), (n, n + 1))


def kz_unused(ncols):
    """indices that occur in no line of kz_empty"""
    return np.arange(3, ncols, 10)


def kz_empty(size):
    """every 9th line stores nothing; the indices 3, 13, 23, ... occur in no line"""
    n = 270 if size == "small" else 2700
    lens = np.full(n, 12)
    lens[::9] = 0
    A = _lines(n, n, lens, 206, allowed=np.setdiff1d(np.arange(n), kz_unused(n)))
    assert np.all(np.diff(A.indptr)[::9] == 0) and not np.isin(A.indices, kz_unused(n)).any()
    return A


def kz_zero_line(nrows):
    return nrows // 2 + 1


def kz_zero_entries(size):
    """a fifth of the stored entries are explicit zeros; one line is all zeros (its inverse squared norm is 0 by the product's rule)"""
    n = 300 if size == "small" else 3000
    A = _lines(n, n, np.full(n, 12), 207)
    r = np.random.RandomState(208)
    A.data[r.rand(A.nnz) < 0.2] = 0.0
    z = kz_zero_line(n)
    A.data[A.indptr[z]:A.indptr[z + 1]] = 0.0
    assert A.nnz == 12 * n
    return A


def _kz_len(longest):
    def make(size):
        """three lines of exactly `longest` entries (the first, the middle and the last but one line), the others 3 .. 6: most slots are padding"""
        n = 300 if size == "small" else 2000
        r = np.random.RandomState(210 + longest)
        lens = r.randint(3, 7, size=n)
        lens[[0, n // 2, n - 2]] = longest
        A = _lines(n, n, lens, 211 + longest)
        got = np.diff(A.indptr)
        assert got.max() == longest and int((got == longest).sum()) == 3 and np.sort(got)[-4] <= 6, (longest, np.sort(got)[-5:])
        return A
    return make


def kz_cancel(size):
    """columns scaled by random signs, magnitudes within 1 % of each other, six even and six odd indices per line: with kz_cancel_v every dot
    product loses two digits to cancellation"""
    n = 300 if size == "small" else 3000
    r = np.random.RandomState(220)
    even, odd = np.arange(0, n, 2), np.arange(1, n, 2)
    indptr, indices = [0], []
    for _ in range(n):
        indices.extend(np.sort(np.concatenate([r.choice(even, 6, replace=False), r.choice(odd, 6, replace=False)])).tolist())
        indptr.append(len(indices))
    indices = np.asarray(indices)
    return _csr(indptr, indices, (1.0 + 0.01 * r.rand(indices.size)) * kz_cancel_signs(n)[indices], (n, n))


def kz_cancel_signs(n):
    return np.where(np.random.RandomState(221).rand(n) < 0.5, -1.0, 1.0)


def kz_cancel_v(n):
    """the vector the sweeps of kz_cancel start from: sign of the column times +1 / -1 on even / odd indices, within 0.1 %"""
    return kz_cancel_signs(n) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * (1.0 + 1e-3 * np.random.RandomState(222).rand(n))


def _kz_tiny(n):
    def make(size):
        r = np.random.RandomState(230 + n)
        return sp.csr_array(_csr(np.arange(0, n * n + 1, n), np.tile(np.arange(n), n), 2.0 * r.rand(n * n) - 1.0, (n, n)))
    return make


def kz_duplicate_line(nrows):
    return nrows // 3


def kz_duplicate(size):
    """kz_nonsym in which one line stores an index twice (adjacent, the arrays stay sorted): the slot protocol has one reader / writer per line
    and index, the plan declines"""
    A = kz_nonsym(size)
    i = kz_duplicate_line(A.shape[0])
    A.indices[A.indptr[i] + 1] = A.indices[A.indptr[i]]
    return A


def kz_start(fam, ncols):
    """the vector v a sweep of the family starts from (x for gauss_seidel_ne, the running residual for gauss_seidel_nr)"""
    if fam.name == "kz_cancel":
        return kz_cancel_v(ncols)
    return np.random.RandomState(7).rand(ncols) - 0.3


def _kzf(longest, **kw):
    lanes, slots = kz_geometry(longest)
    return Form(lanes=lanes, slots=slots, longest=longest, declines=lanes == 0, **kw)


KZ_FAMILIES = {f.name: f for f in (
    Family("kz_nonsym", kz_nonsym, _kzf(12)),
    Family("kz_rect_wide", kz_rect_wide, _kzf(12), note="v, b, Dinv and xout have different lengths"),
    Family("kz_rect_tall", kz_rect_tall, _kzf(12)),
    Family("kz_arrow", kz_arrow, _kzf(6), note="levels = lines; the version of index 0 runs up to the number of lines"),
    Family("kz_chain", kz_chain, _kzf(2), note="levels = lines; 15 dummy lines and a real one per group"),
    Family("kz_empty", kz_empty, _kzf(12)),
    Family("kz_zero_entries", kz_zero_entries, _kzf(12)),
    *(Family(f"kz_len_{k}", _kz_len(k), _kzf(k)) for k in (16, 17, 64, 65, 255, 256)),
    Family("kz_len_257", _kz_len(257), _kzf(257), note="one over the limit: the plan declines"),
    Family("kz_cancel", kz_cancel, _kzf(12)),
    *(Family(f"kz_tiny_{n}", _kz_tiny(n), _kzf(n)) for n in KZ_TINY),
    Family("kz_duplicate", kz_duplicate, Form(longest=12, declines=True), note="a line holds an index twice: the plan declines"),
)}
assert [KZ_FAMILIES[f"kz_len_{k}"].form.lanes for k in (16, 17, 64, 65, 255, 256)] == [4, 8, 16, 32, 64, 64]
assert [KZ_FAMILIES[f"kz_len_{k}"].form.slots for k in (16, 17, 64, 65, 255, 256)] == [4, 3, 4, 3, 4, 4] and KZ_FAMILIES["kz_len_257"].form.declines


def kz_spec(kind, Lop, omega):
    """(A, spec) of the product's _normal_equation_spec such that the LINES are the rows of Lop: A = Lop for gauss_seidel_ne, A = Lop^T for
    gauss_seidel_nr (spec.At is then Lop again).  Dinv comes from the product: empty and all-zero lines get 0"""
    A = sp.csr_array(Lop) if kind == "gauss_seidel_ne" else sp.csc_array((Lop.data, Lop.indices, Lop.indptr), shape=Lop.shape[::-1])
    return A, _normal_equation_spec(kind, A, 1, "forward", omega)


# ================================================================= block families
OFF = 0.15


def _bsr(P, bs, seed, diag_scale=None):
    """BSR operator on the block pattern P (CSR, sorted; diagonal entries of P = stored diagonal blocks): off-diagonal blocks uniform in +-0.15,
    diagonal blocks +-0.15 plus c_i I with c_i = 0.15 bs (blocks in the row) + 1, which makes the block row dominant"""
    P = sp.csr_array(P)
    P.sort_indices()
    nb = P.shape[0]
    r = np.random.RandomState(seed)
    dat = (2.0 * r.rand(P.nnz, bs, bs) - 1.0) * OFF
    rows = np.repeat(np.arange(nb), np.diff(P.indptr))
    dm = rows == P.indices
    c = OFF * bs * np.diff(P.indptr)[rows[dm]] + 1.0
    dat[dm] += c[:, None, None] * np.eye(bs)
    return sp.bsr_array((dat, P.indices.astype(np.int32), P.indptr.astype(np.int32)), shape=(bs * nb, bs * nb), blocksize=(bs, bs))


def _pattern(nb, per_row, seed, symmetric=False):
    """random block pattern with the diagonal, about per_row off-diagonal blocks per row"""
    r = np.random.RandomState(seed)
    S = sp.random(nb, nb, density=min(1.0, per_row / nb / (2 if symmetric else 1)), random_state=r, format="csr")
    S = sp.csr_array(S + S.T) if symmetric else sp.csr_array(S)
    S = sp.csr_array(((S + sp.eye_array(nb)) != 0).astype(np.float64))
    S.sort_indices()
    return S


def block_dinv(A):
    """inverses of the stored diagonal blocks (f64 LAPACK), zero where a block row stores none -- what the sweeps are handed"""
    bs = A.blocksize[0]
    nb = A.shape[0] // bs
    Dinv = np.zeros((nb, bs, bs))
    rows = np.repeat(np.arange(nb), np.diff(A.indptr))
    dm = rows == A.indices
    Dinv[rows[dm]] = np.linalg.inv(A.data[dm])
    return np.ascontiguousarray(Dinv)


def pattern_symmetric(A):
    P = sp.csr_array((np.ones(A.indices.size), A.indices, A.indptr), shape=(A.indptr.size - 1,) * 2)
    return (P != P.T).nnz == 0


def longest_row(A):
    """off-diagonal blocks of the longest block row"""
    rows = np.repeat(np.arange(A.indptr.size - 1), np.diff(A.indptr))
    return int(np.bincount(rows[rows != A.indices], minlength=1).max()) if A.indices.size else 0


def _sized(small, large):
    return lambda size: small if size == "small" else large


def _trim(P, longest):
    """drop off-diagonal entries beyond `longest` per row (keeps the diagonal)"""
    P = sp.lil_array(P)
    for i in range(P.shape[0]):
        off = [j for j in P.rows[i] if j != i]
        for j in off[longest:]:
            P[i, j] = 0
    P = sp.csr_array(P)
    P.eliminate_zeros()
    return P


def b_nonsym(size, bs):
    return _bsr(_trim(_pattern(_sized(200, 1500)(size), 6, 301), 12), bs, 302)


def b_lower(size, bs):
    return _bsr(sp.tril(_trim(_pattern(_sized(200, 1500)(size), 12, 303, symmetric=True), 16), format="csr"), bs, 304)


def b_upper(size, bs):
    return _bsr(sp.triu(_trim(_pattern(_sized(200, 1500)(size), 12, 303, symmetric=True), 16), format="csr"), bs, 305)


def b_blockdiag(size, bs):
    return _bsr(sp.eye_array(_sized(100, 1000)(size), format="csr"), bs, 306)


def b_missing(nb):
    return np.arange(0, nb, 7)


def b_nodiag(size, bs):
    """symmetric pattern in which every 7th block row stores no diagonal block (its Dinv is zero: the sweep sets the row to zero)"""
    nb = _sized(210, 1400)(size)
    P = sp.lil_array(_trim(_pattern(nb, 6, 307, symmetric=True), 16))
    for i in b_missing(nb):
        P[i, i] = 0
    P = sp.csr_array(P)
    P.eliminate_zeros()
    P = sp.csr_array(P.multiply(P.T) + sp.diags_array(P.diagonal()))               # trimming may have left one-sided entries: keep the mutual ones
    P.eliminate_zeros()
    return _bsr(P, bs, 308)


def b_lonely(nb):
    return np.arange(2, nb, 5)


def b_lonely_rows(size, bs):
    """every 5th block row stores only its diagonal block (all its slots are padding); the other rows still read it"""
    nb = _sized(200, 1500)(size)
    P = sp.lil_array(_trim(_pattern(nb, 6, 309, symmetric=True), 16))
    for i in b_lonely(nb):
        P.rows[i], P.data[i] = [i], [1.0]
    return _bsr(sp.csr_array(P), bs, 310)


def b_chain(size, bs):
    nb = _sized(200, 1500)(size)
    return _bsr(sp.csr_array(sp.diags_array([np.ones(nb - 1), np.ones(nb)], offsets=[-1, 0])), bs, 311)


def _b_len(longest):
    def make(size, bs):
        """three block rows of exactly `longest` off-diagonal blocks (and as many in their columns), the others four (offsets 1 and 7) plus at most
        three from those columns; symmetric pattern"""
        nb = _sized(300, 1000)(size)
        r = np.random.RandomState(320 + longest)
        P = sp.lil_array(sp.diags_array([np.ones(nb - 7), np.ones(nb - 1), np.ones(nb), np.ones(nb - 1), np.ones(nb - 7)], offsets=[-7, -1, 0, 1, 7]))
        long_rows = [nb // 6, nb // 2, nb - nb // 6]
        for i in long_rows:
            have = [j for j in P.rows[i] if j != i]
            pool = np.setdiff1d(np.arange(nb), np.concatenate([long_rows, have, [k for lr in long_rows for k in range(lr - 8, lr + 9)]]))
            for j in r.choice(pool, size=longest - len(have), replace=False):
                P[i, j] = 1.0
                P[j, i] = 1.0
        A = _bsr(sp.csr_array(P), bs, 321 + longest)
        rows = np.repeat(np.arange(nb), np.diff(A.indptr))
        got = np.bincount(rows[rows != A.indices], minlength=nb)
        assert got.max() == longest and (int((got == longest).sum()) == 3 or longest < 8) and np.sort(got)[-4] <= 7, (longest, np.sort(got)[-5:])
        return A
    return make


def b_arrow(size, bs):
    """a full first block row and column on a tridiagonal pattern: the first row is longer than two blocks per lane"""
    nb = _sized(200, 1500)(size)
    P = sp.lil_array(sp.diags_array([np.ones(nb - 1), np.ones(nb), np.ones(nb - 1)], offsets=[-1, 0, 1]))
    P[0, :] = 1.0
    P[:, 0] = 1.0
    return _bsr(sp.csr_array(P), bs, 330)


def b_cancel(size, bs):
    """b_nonsym with every block column (the diagonal blocks too) scaled by a random sign"""
    A = b_nonsym(size, bs)
    sg = np.where(np.random.RandomState(331).rand(A.shape[0] // bs) < 0.5, -1.0, 1.0)
    return sp.bsr_array((A.data * sg[A.indices][:, None, None], A.indices, A.indptr), shape=A.shape, blocksize=A.blocksize)


def b_stiff_rows(nb):
    return np.arange(4, nb, 10)


def b_stiff(size, bs):
    """every 10th diagonal block is Q diag(c .. 1e-6 c) Q^T (condition number 1e6, its inverse is large); the blocks of those COLUMNS are scaled by
    1e-6, so the large components come back into the other rows at the size of everything else and nothing grows from level to level"""
    nb = _sized(200, 1500)(size)
    A = _bsr(_trim(_pattern(nb, 6, 332, symmetric=True), 16), bs, 333)
    r = np.random.RandomState(334)
    rows = np.repeat(np.arange(nb), np.diff(A.indptr))
    stiff = b_stiff_rows(nb)
    dat = A.data.copy()
    for p in np.flatnonzero(np.isin(A.indices, stiff)):
        if rows[p] == A.indices[p]:
            Q, _ = np.linalg.qr(r.randn(bs, bs))
            dat[p] = (Q * (2.0 * np.logspace(0, -6, bs))) @ Q.T
        else:
            dat[p] *= 1e-6
    return sp.bsr_array((dat, A.indices, A.indptr), shape=A.shape, blocksize=A.blocksize)


def b_zero_blocks(size, bs):
    """b_nonsym in which a quarter of the stored off-diagonal blocks are all zero"""
    A = b_nonsym(size, bs)
    rows = np.repeat(np.arange(A.shape[0] // bs), np.diff(A.indptr))
    z = (np.random.RandomState(335).rand(A.indices.size) < 0.25) & (rows != A.indices)
    dat = A.data.copy()
    dat[z] = 0.0
    return sp.bsr_array((dat, A.indices, A.indptr), shape=A.shape, blocksize=A.blocksize)


def _b_tiny(nb):
    def make(size, bs):
        return _bsr(sp.csr_array(np.ones((nb, nb))), bs, 340 + nb)
    return make


def _bf(longest, **kw):
    f = Form(longest=longest, **kw)
    lanes, slots = block_geometry(f)
    return Form(lanes=lanes, slots=slots, longest=longest, declines=kw.get("declines", False) or slots > 2, one_level=kw.get("one_level", False))


B_FAMILIES = {f.name: f for f in (
    Family("b_nonsym", b_nonsym, _bf(12), other_bs=2, note="old values come from the snapshot"),
    Family("b_lower", b_lower, _bf(16), other_bs=4, note="forward: every operand early; backward: every operand old"),
    Family("b_upper", b_upper, _bf(16), other_bs=6),
    Family("b_blockdiag", b_blockdiag, _bf(0, declines=True, one_level=True), other_bs=2, note="one dependency level: nothing to hand over"),
    Family("b_nodiag", b_nodiag, _bf(16), other_bs=4),
    Family("b_lonely_rows", b_lonely_rows, _bf(16), other_bs=6),
    Family("b_chain", b_chain, _bf(1), other_bs=2, note="levels = block rows; 7 padding lanes and 7 dummy rows per group"),
    *(Family(f"b_len_{k}", _b_len(k), _bf(k), other_bs=o) for k, o in ((8, 4), (9, 6), (16, 2), (17, 4), (32, 6), (33, 2), (64, 4), (65, 6), (128, 2))),
    Family("b_len_129", _b_len(129), _bf(129), other_bs=4, note="longer than two blocks per lane: the plan declines"),
    Family("b_arrow", b_arrow, Form(declines=True), other_bs=6, note="a full first block row and column: the plan declines"),
    Family("b_cancel", b_cancel, _bf(12), other_bs=2),
    # measured on the CPU: the largest |f64 replay - f64 oracle| / max |oracle| over 1, 7 and 500 waves, both modes, every width, forward and
    # backward, bs 3 and 4 (small size; tests/test_block_kz_families_plan.py prints it) is 1.0e-16 -- times 8 that is 8.1e-16, BELOW the default
    # bar: the large inverse scales the iterate and its error alike, and the errors are taken relative to max |ref|.  The family needs no looser
    # bar and keeps the default (variants whose large components feed back with a gain of 10 per hop measure 6.6e-16)
    Family("b_stiff", b_stiff, _bf(16), other_bs=4, tol=1e-13),
    Family("b_zero_blocks", b_zero_blocks, _bf(12), other_bs=6),
    *(Family(f"b_tiny_{n}", _b_tiny(n), _bf(n - 1), other_bs=o) for n, o in zip(B_TINY, (2, 4, 6, 2))),
)}
assert [B_FAMILIES[f"b_len_{k}"].form.lanes for k in (8, 9, 16, 17, 32, 33, 64, 65, 128)] == [8, 16, 16, 32, 32, 64, 64, 64, 64]
assert [B_FAMILIES[f"b_len_{k}"].form.slots for k in (64, 65, 128)] == [1, 2, 2] and B_FAMILIES["b_len_129"].form.declines


def block_sizes(fam):
    return (3, fam.other_bs)


assert {s for f in B_FAMILIES.values() for s in block_sizes(f)} == {2, 3, 4, 6}


# ================================================================= the yardsticks
def _dirs(how, m, iterations):
    return {"forward": [(0, m, 1)], "backward": [(m - 1, -1, -1)], "symmetric": [(0, m, 1), (m - 1, -1, -1)]}[how] * iterations


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def ref_block(A, Dinv, x, b, how, iterations=1, dtype=np.float64):
    """the oracle's sequential block sweep (amg_core::block_gauss_seidel restated in oracle/amg_oracle.c) on copies in `dtype` -- np.float64: what the
    device's exact order gives bit for bit; np.longdouble (x86-64: 64-bit mantissa): the yardstick"""
    bs = A.blocksize[0]
    nb = A.shape[0] // bs
    Ap, Aj = _i32(A.indptr), _i32(A.indices)
    Ax = np.ascontiguousarray(A.data.ravel(), dtype=dtype)
    Di = np.ascontiguousarray(np.asarray(Dinv).ravel(), dtype=dtype)
    xx, bb = np.array(x, dtype=dtype), np.ascontiguousarray(b, dtype=dtype)
    for d in _dirs(how, nb, iterations):
        orc.block_gauss_seidel(Ap, Aj, Ax, xx, bb, Di, *d, bs)
    return xx


def ref_kz(kind, Lop, v, b, Dinv, omega, xout, how, iterations=1, dtype=np.float64):
    """the oracle's loops over the lines (rows) of Lop in `dtype`: gauss_seidel_ne -> (v,), gauss_seidel_nr -> (xout, v)"""
    Lp, Lj = _i32(Lop.indptr), _i32(Lop.indices)
    Lx = np.ascontiguousarray(Lop.data, dtype=dtype)
    vv, Di = np.array(v, dtype=dtype), np.ascontiguousarray(Dinv, dtype=dtype)
    m = Lop.shape[0]
    if kind == "gauss_seidel_ne":
        bb = np.ascontiguousarray(b, dtype=dtype)
        for d in _dirs(how, m, iterations):
            orc.gauss_seidel_ne(Lp, Lj, Lx, vv, bb, *d, Di, omega)
        return (vv,)
    xx = np.array(xout, dtype=dtype)
    for d in _dirs(how, m, iterations):
        orc.gauss_seidel_nr(Lp, Lj, Lx, xx, vv, *d, Di, omega)
    return (xx, vv)


def plain_block(A, Dinv, x, b, how, iterations=1):
    """block_gauss_seidel as a plain Python loop in np.longdouble: pins the yardstick itself (tiny operators only)"""
    bs = A.blocksize[0]
    nb = A.shape[0] // bs
    Ax, Di = A.data.astype(L_), np.asarray(Dinv).reshape(nb, bs, bs).astype(L_)
    x, b = np.array(x, dtype=L_), np.asarray(b, dtype=L_)
    for (r0, r1, rs) in _dirs(how, nb, iterations):
        for i in range(r0, r1, rs):
            acc = [L_(0)] * bs
            for p in range(A.indptr[i], A.indptr[i + 1]):
                j = A.indices[p]
                if j == i:
                    continue
                for r in range(bs):
                    t = L_(0)
                    for c in range(bs):
                        t = t + Ax[p, r, c] * x[j * bs + c]
                    acc[r] = acc[r] + t
            rhs = [b[i * bs + r] - acc[r] for r in range(bs)]
            for r in range(bs):
                t = L_(0)
                for c in range(bs):
                    t = t + Di[i, r, c] * rhs[c]
                x[i * bs + r] = t
    return x


def plain_kz(kind, Lop, v, b, Dinv, omega, xout, how, iterations=1):
    """gauss_seidel_ne / gauss_seidel_nr as plain Python loops in np.longdouble (tiny operators only)"""
    Lp, Lj, Lx = Lop.indptr, Lop.indices, Lop.data.astype(L_)
    v, Di, om = np.array(v, dtype=L_), np.asarray(Dinv, dtype=L_), L_(omega)
    ne = kind == "gauss_seidel_ne"
    b = np.asarray(b, dtype=L_) if ne else None
    x = None if ne else np.array(xout, dtype=L_)
    for (r0, r1, rs) in _dirs(how, Lop.shape[0], iterations):
        for i in range(r0, r1, rs):
            d = L_(0)
            for p in range(Lp[i], Lp[i + 1]):
                d = d + Lx[p] * v[Lj[p]]
            if ne:
                d = (b[i] - d) * Di[i] * om
                for p in range(Lp[i], Lp[i + 1]):
                    v[Lj[p]] = v[Lj[p]] + Lx[p] * d
            else:
                d = d * (Di[i] * om)
                x[i] = x[i] + d
                for p in range(Lp[i], Lp[i + 1]):
                    v[Lj[p]] = v[Lj[p]] - d * Lx[p]
    return (v,) if ne else (x, v)


def rel_err(got, ref):
    ref = np.asarray(ref)
    return float(np.max(np.abs(np.asarray(got, dtype=ref.dtype) - ref)) / np.max(np.abs(ref))) if ref.size and np.max(np.abs(ref)) > 0 else 0.0


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def bar(e_seq):
    """the project's yardstick against the long-double sweep (tests/test_gpu_midsize.py, tests/test_gpu_sweep_families.py) with growth factor 1:
    nothing is merged in these sweeps"""
    return max(8.0 * e_seq, 32.0 * U)
