"""Adversarial families for the smoothed-aggregation setup kernels -- standard_aggregation, fit_candidates and
symmetric_strength_of_connection -- with plain-Python restatements of the reference and the checks the CPU test
(test_sa_setup_families_host.py) and the GPU test (test_gpu_sa_setup_families.py) share.

Everything is NumPy / SciPy and seeded; nothing is read from the reference at test time.  The reference's own outputs are
the committed tests/golden/kernels_sa_setup_families.npz (written by tests/golden/make_golden_sa_setup_families.py; outputs
only -- the inputs are regenerated here from the seeds).  Every comparison is ``np.array_equal``: there is no tolerance.

Restatements (written from the reference's text, not from the kernels):
  serial_aggregation   the three passes of amg_core.standard_aggregation (smoothed_aggregation.h:137-268)
  token_rounds         the device protocol as the comment in csrc/pamg_aggregate.hip states it: sorted member lists, pend
                       counters, work lists, one turn per vertex per round, then passes 2 and 3 from the marks
  strength_restated    smoothed_aggregation.h:56-110, strength.py:349-352 and scale_rows_by_largest_entry in Python floats
  tentative_from_lists the oracle's blocks (CSC list order) put into AggOp's row order (tentative.fit_candidates)
"""
import bisect
import hashlib
import itertools
import sys
import zlib
from functools import lru_cache
from pathlib import Path

import numpy as np
import scipy.sparse as sp

GOLDEN = Path(__file__).resolve().parent / "golden" / "kernels_sa_setup_families.npz"
SEED = 20261021
SORT_MAX = 4096          # csrc/pamg_aggregate.hip: a longer row / a larger aggregate is refused (one-lane insertion sorts)


class Refused(Exception):
    """the token protocol does not apply: pattern not symmetric, duplicate entries, or pass 3 would open an aggregate"""


def _rng(name):
    return np.random.default_rng(SEED + zlib.crc32(name.encode()))


@lru_cache(maxsize=1)
def data():
    with np.load(GOLDEN) as z:
        d = {k: z[k] for k in z.files}
    for v in d.values():
        v.setflags(write=False)                              # shared among the tests: nobody changes it
    return d


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(np.ravel(got != want))[:10]
        raise AssertionError((what, "first differing positions", bad.tolist(), np.ravel(got)[bad].tolist(), np.ravel(want)[bad].tolist()))


# =============================================================================================== graphs for aggregation
def _graph(n, ei, ej, diag=None):
    """(Ap, Aj) int32: the symmetric pattern of the undirected edges, rows ascending, no duplicates; diagonal entries on
    the rows where ``diag`` is set"""
    ei, ej = np.asarray(ei, dtype=np.int64), np.asarray(ej, dtype=np.int64)
    keep = ei != ej
    ei, ej = ei[keep], ej[keep]
    r, c = np.concatenate([ei, ej]), np.concatenate([ej, ei])
    if diag is not None:
        d = np.flatnonzero(diag)
        r, c = np.concatenate([r, d]), np.concatenate([c, d])
    key = np.unique(r * n + c)
    r, c = key // n, key % n
    Ap = np.zeros(n + 1, dtype=np.int64)
    Ap[1:] = np.cumsum(np.bincount(r, minlength=n))
    return Ap.astype(np.int32), c.astype(np.int32)


def shuffled(Ap, Aj, name):
    """the same rows, each row's entries in a seeded random order (pass 2 depends on the stored order)"""
    rows = np.repeat(np.arange(Ap.size - 1), np.diff(Ap))
    order = np.lexsort((_rng(name + "/shuffle").random(Aj.size), rows))
    return Ap.copy(), Aj[order]


def _stencil_edges(shape, full):
    idx = np.arange(int(np.prod(shape))).reshape(shape)
    ei, ej = [], []
    for off in itertools.product((-1, 0, 1), repeat=len(shape)):
        if off <= (0,) * len(shape) or (not full and sum(abs(o) for o in off) != 1):
            continue
        a = tuple(slice(max(0, -o), s - max(0, o)) for o, s in zip(off, shape))
        b = tuple(slice(max(0, o), s - max(0, -o)) for o, s in zip(off, shape))
        ei.append(idx[a].ravel())
        ej.append(idx[b].ravel())
    return np.concatenate(ei), np.concatenate(ej)


def _star(n, hub, diag_hub=False):
    leaves = np.delete(np.arange(n), hub)
    d = np.zeros(n, dtype=bool)
    d[hub] = diag_hub
    return _graph(n, np.full(n - 1, hub), leaves, d)


def _pairs(n, drop_every=0):
    k = np.arange(n // 2)
    if drop_every:
        k = k[k % drop_every != drop_every - 1]
    return _graph(n, 2 * k, 2 * k + 1)


def _rand_iso():
    n, rng = 5000, _rng("rand_iso")
    live = np.flatnonzero(rng.random(n) >= 0.25)
    m = 2 * live.size                                        # mean degree 4 among the live nodes, about 3 over all
    return _graph(n, live[rng.integers(0, live.size, m)], live[rng.integers(0, live.size, m)], rng.random(n) < 0.5)


def _cliques_iso():
    n, rng = 40 * 16 + 60, _rng("cliques_iso")
    iso = np.sort(rng.choice(n, 60, replace=False))
    members = np.setdiff1d(np.arange(n), iso).reshape(40, 16)
    a, b = np.triu_indices(16, 1)
    diag = np.zeros(n, dtype=bool)
    diag[iso[::2]] = True                                    # diagonal-only rows and empty rows in turn
    return _graph(n, members[:, a].ravel(), members[:, b].ravel(), diag)


def _build(name):
    rng = _rng(name)
    if name in ("path", "path_diag", "path_perm"):
        n = 3000
        ei, ej = np.arange(n - 1), np.arange(1, n)
        if name == "path_perm":
            p = rng.permutation(n)
            return _graph(n, p[ei], p[ej], rng.random(n) < 0.5)
        return _graph(n, ei, ej, np.ones(n, dtype=bool) if name == "path_diag" else None)
    if name == "comb":
        h = 1500
        return _graph(2 * h, np.r_[np.arange(h - 1), np.arange(h)], np.r_[np.arange(1, h), h + np.arange(h)])
    if name == "star_first":
        return _star(2048, 0)
    if name == "star_last":
        return _star(2048, 2047)
    if name == "star_desc":
        Ap, Aj = _star(1025, 0)
        Aj = Aj.copy()
        Aj[Ap[0]:Ap[1]] = Aj[Ap[0]:Ap[1]][::-1]             # the hub's row descending: worst case of the row sort
        return Ap, Aj
    if name == "clique64":
        a, b = np.triu_indices(64, 1)
        return _graph(64, a, b)
    if name == "cliques_iso":
        return _cliques_iso()
    if name == "bipartite":
        a, b = np.meshgrid(np.arange(32), 32 + np.arange(32))
        return _graph(64, a.ravel(), b.ravel())
    if name == "grid5":
        return _graph(45 * 45, *_stencil_edges((45, 45), False))
    if name == "grid9_diag":
        return _graph(45 * 45, *_stencil_edges((45, 45), True), np.ones(45 * 45, dtype=bool))
    if name == "box27":
        return _graph(13 ** 3, *_stencil_edges((13, 13, 13), True), np.ones(13 ** 3, dtype=bool))
    if name.startswith("pairs_") and name != "pairs_iso":
        return _pairs(int(name[6:]))
    if name == "pairs_iso":
        return _pairs(6145, drop_every=7)
    if name == "rand_iso":
        return _rand_iso()
    if name == "empty":
        return np.zeros(51, dtype=np.int32), np.zeros(0, dtype=np.int32)
    if name == "diag_only":
        return np.arange(51, dtype=np.int32), np.arange(50, dtype=np.int32)
    if name == "one":
        return np.zeros(2, dtype=np.int32), np.zeros(0, dtype=np.int32)
    if name == "one_diag":
        return np.array([0, 1], dtype=np.int32), np.zeros(1, dtype=np.int32)
    if name == "hub_at_bound":                               # the hub's row: its diagonal and SORT_MAX - 1 leaves, ascending
        return _star(SORT_MAX, 0, diag_hub=True)
    if name == "hub_over_bound":
        return _star(SORT_MAX + 1, 0, diag_hub=True)
    raise KeyError(name)


BASE = ["path", "path_diag", "path_perm", "comb", "star_first", "star_last", "star_desc", "clique64", "cliques_iso", "bipartite",
        "grid5", "grid9_diag", "box27", "pairs_2048", "pairs_2049", "pairs_4096", "pairs_4097", "pairs_6145", "pairs_iso",
        "rand_iso", "empty", "diag_only", "one", "one_diag"]
FAMILIES = BASE + [b + "_shuf" for b in BASE] + ["rand_iso_i64"]
HUBS = ["hub_at_bound", "hub_over_bound"]                    # the guard's cases: in the fixture, on the GPU in tests of their own
REFUSALS = ["rand_iso_nonsym", "rand_iso_cycle", "rand_iso_dup_off", "rand_iso_dup_diag"]
N_ROUNDS = ["path", "path_diag", "star_first", "star_last", "star_desc", "clique64"]      # one vertex per round


def _refusal(name):
    Ap, Aj = graph("rand_iso")
    Ap, Aj = Ap.astype(np.int64), Aj.copy()
    rows = np.repeat(np.arange(Ap.size - 1), np.diff(Ap))
    rng = _rng(name)

    def insert(row, col):
        nonlocal Ap, Aj
        Aj = np.insert(Aj, Ap[row + 1], col)
        Ap[row + 1:] += 1

    if name == "rand_iso_nonsym":                            # one reverse edge removed
        p = int(rng.choice(np.flatnonzero(Aj != rows)))
        Aj = np.delete(Aj, p)
        Ap[rows[p] + 1:] -= 1
    elif name == "rand_iso_cycle":                           # a directed 3-cycle among three nodes without any entry
        a, b, c = (int(v) for v in np.flatnonzero(np.diff(Ap) == 0)[[3, 40, 90]])
        insert(a, b), insert(b, c), insert(c, a)
    elif name == "rand_iso_dup_off":                         # one off-diagonal entry stored twice
        p = int(rng.choice(np.flatnonzero(Aj != rows)))
        insert(int(rows[p]), int(Aj[p]))
    elif name == "rand_iso_dup_diag":                        # one diagonal entry stored twice, on a row with neighbours
        p = int(rng.choice(np.flatnonzero((Aj == rows) & (np.diff(Ap)[rows] > 2))))
        insert(int(rows[p]), int(rows[p]))
    else:
        raise KeyError(name)
    return Ap.astype(np.int32), Aj.astype(np.int32)


@lru_cache(maxsize=None)
def graph(name):
    """(Ap, Aj) of a family, read-only"""
    if name in REFUSALS:
        Ap, Aj = _refusal(name)
    elif name.endswith("_i64"):
        Ap, Aj = (a.astype(np.int64) for a in graph(name[:-4]))
    elif name.endswith("_shuf"):
        Ap, Aj = shuffled(*graph(name[:-5]), name)
    else:
        Ap, Aj = _build(name)
    Ap.setflags(write=False)
    Aj.setflags(write=False)
    return Ap, Aj


def graph_csr(name):
    Ap, Aj = graph(name)
    n = Ap.size - 1
    return sp.csr_array((np.ones(Aj.size), Aj.copy(), Ap.copy()), shape=(n, n))


# =============================================================================================== restatements: aggregation
def serial_aggregation(Ap, Aj):
    """(x, y, count, opened_in_pass3): amg_core.standard_aggregation, smoothed_aggregation.h:137-268, as it stands"""
    Ap, Aj = np.asarray(Ap).tolist(), np.asarray(Aj).tolist()
    n = len(Ap) - 1
    x, y = [0] * n, [0] * max(n, 1)
    nxt = 1
    for i in range(n):                                       # pass 1
        if x[i]:
            continue
        has_agg = has_nb = False
        for jj in range(Ap[i], Ap[i + 1]):
            j = Aj[jj]
            if i != j:
                has_nb = True
                if x[j]:
                    has_agg = True
                    break
        if not has_nb:
            x[i] = -n
        elif not has_agg:
            x[i] = nxt
            y[nxt - 1] = i
            for jj in range(Ap[i], Ap[i + 1]):
                x[Aj[jj]] = nxt
            nxt += 1
    for i in range(n):                                       # pass 2
        if x[i]:
            continue
        for jj in range(Ap[i], Ap[i + 1]):
            xj = x[Aj[jj]]
            if xj > 0:
                x[i] = -xj
                break
    nxt -= 1
    opened = 0
    for i in range(n):                                       # pass 3
        xi = x[i]
        if xi != 0:
            x[i] = xi - 1 if xi > 0 else (-1 if xi == -n else -xi - 1)
            continue
        x[i] = nxt
        y[nxt] = i
        for jj in range(Ap[i], Ap[i + 1]):
            if x[Aj[jj]] == 0:
                x[Aj[jj]] = nxt
        nxt += 1
        opened += 1
    return np.array(x, dtype=np.int32), np.array(y[:nxt], dtype=np.int32), nxt, opened


def token_rounds(Ap, Aj, order="reverse"):
    """(x, y, count, rounds): the traversal csrc/pamg_aggregate.hip describes.  Every vertex v owns the sorted member list
    {v} + row(v) and passes a token down it; a vertex takes its turn once it holds the token of every list it is a member
    of.  The vertices that became ready in one round take their turns in the next; within a round the work list is walked
    in reverse (order='reverse') or in a seeded random order (order=<int seed>).  Raises Refused where the kernels return
    PAMG_E_UNSUPPORTED."""
    Ap, Aj = np.asarray(Ap).tolist(), np.asarray(Aj).tolist()
    n = len(Ap) - 1
    ISO = None
    rows = [Aj[Ap[i]:Ap[i + 1]] for i in range(n)]
    L, mark = [], [0] * n
    for v in range(n):
        others = [j for j in rows[v] if j != v]
        if len(set(others)) != len(others) or len(rows[v]) - len(others) > 1:
            raise Refused("duplicate entries")
        L.append(sorted(set(others) | {v}))
        if len(L[v]) == 1:
            mark[v] = ISO                                    # isolated: marked at once, takes no part
    live = [v for v in range(n) if len(L[v]) > 1]
    pend = [0] * n
    for i in live:
        for v in L[i]:
            k = bisect.bisect_left(L[v], i)                  # i's place in v's list
            if k >= len(L[v]) or L[v][k] != i:
                raise Refused("pattern not symmetric")
            pend[i] += k > 0                                 # the smallest member holds the list's token from the start
    cnt = [0] * n
    work = [i for i in live if pend[i] == 0]
    rng = None if order == "reverse" else np.random.default_rng(order)
    rounds = done = 0
    while work:
        rounds += 1
        nxt = []
        for i in (reversed(work) if rng is None else [work[k] for k in rng.permutation(len(work))]):
            if mark[i] == 0 and all(mark[j] == 0 for j in rows[i]):
                mark[i] = i + 1                              # a root: marks itself and its neighbours
                for j in rows[i]:
                    mark[j] = i + 1
            for v in L[i]:
                cnt[v] += 1                                  # members of v's list that have had their turn
                if cnt[v] < len(L[v]):
                    t = L[v][cnt[v]]
                    pend[t] -= 1
                    if pend[t] == 0:
                        nxt.append(t)
        done += len(work)
        work = nxt
    if done != len(live):
        raise AssertionError(("the traversal stalled", done, len(live)))
    for i in range(n):                                       # pass 2: first neighbour (stored order) that pass 1 aggregated
        if mark[i] == 0:
            for j in rows[i]:
                if mark[j] is not ISO and mark[j] > 0:
                    mark[i] = -mark[j]
                    break
    roots = [i for i in range(n) if mark[i] == i + 1]
    rid = {r: k for k, r in enumerate(roots)}
    x = []
    for i in range(n):
        m = mark[i]
        if m is ISO:
            x.append(-1)
        elif m == 0:
            raise Refused("the reference's third pass would open an aggregate")
        else:
            x.append(rid[abs(m) - 1])
    return np.array(x, dtype=np.int32), np.array(roots, dtype=np.int32), len(roots), rounds


def aggop_from(x, count, index_type=np.int32):
    """aggregate.py:76-96 from amg_core's x: (indptr, indices, data, shape) of AggOp"""
    x = np.asarray(x)
    if count == 0:
        return np.zeros(x.size + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), (x.size, 1)
    Tj = x.astype(index_type)
    if Tj.min() == -1:                                       # some nodes not aggregated: through SciPy's coo -> csr, as there
        mask = Tj != -1
        row, col = np.arange(x.size, dtype=index_type)[mask], Tj[mask]
        M = sp.coo_array((np.ones(len(col), dtype=np.int32), (row, col)), shape=(x.size, count)).tocsr()
        return M.indptr, M.indices, M.data, (x.size, count)
    return np.arange(x.size + 1, dtype=index_type), Tj, np.ones(x.size, dtype=np.int32), (x.size, count)


def check_aggregation(fn, name, fixture=True):
    """fn(Ap, Aj) -> (x, y, count) against the serial restatement and, where recorded, the reference's arrays"""
    Ap, Aj = graph(name)
    keep = (Ap.copy(), Aj.copy())
    x, y, count = fn(Ap, Aj)
    sx, sy, scount, opened = serial_aggregation(Ap, Aj)
    assert opened == 0, (name, "the third pass opened aggregates", opened)
    assert count == scount, (name, count, scount)
    same(x, sx, (name, "x"))
    same(np.asarray(y)[:count], sy, (name, "y"))
    if fixture:
        same(x, data()[f"agg.{name}.x"], (name, "x / fixture"))
        same(np.asarray(y)[:count], data()[f"agg.{name}.y"], (name, "y / fixture"))
    assert np.array_equal(keep[0], Ap) and np.array_equal(keep[1], Aj)
    return x, y, count


def digest(a):
    """SHA-256 of an array's bytes (C order) as uint8[32]: how the fixture holds AggOp's arrays, which repeat x and y"""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def check_aggop(AggOp, Cpts, name):
    """aggregate.standard_aggregation's (AggOp, Cpts) against the reference's: shape, and per array dtype, size and digest.
    The arrays themselves follow from the recorded x, y (aggop_from), which names the first difference if there is one."""
    d = data()
    k = d["names.agg"].tolist().index(name)
    x, y = d[f"agg.{name}.x"], d[f"agg.{name}.y"]
    assert AggOp.format == "csr" and AggOp.shape == tuple(d["aggop.shapes"][k]), (name, AggOp.shape)
    want = aggop_from(x, y.size, np.dtype(str(d["aggop.dtypes"][k][3])))
    for slot, (got, what) in enumerate(((AggOp.indptr, "AggOp.indptr"), (AggOp.indices, "AggOp.indices"), (AggOp.data, "AggOp.data"),
                                        (Cpts, "Cpts"))):
        assert str(got.dtype) == str(d["aggop.dtypes"][k][slot]) and got.size == d["aggop.sizes"][k][slot], (name, what, got.dtype, got.size)
        if not np.array_equal(digest(got), d["aggop.sha256"][k][slot]):
            same(got, want[slot] if slot < 3 else y.astype(got.dtype), (name, what))
            raise AssertionError((name, what, "differs from the recorded digest"))
    assert AggOp.dtype == np.int32 and np.array_equal(np.diff(AggOp.indptr), (x >= 0).astype(np.int32)), name     # empty rows: unaggregated


# =============================================================================================== aggregations and candidates for fit_candidates
AGGS = ["rand_iso", "pairs_2049", "path_perm", "star_first", "grid9_diag", "empty_cols", "all_unaggregated"]
KS64 = [(1, 1), (1, 3), (2, 3), (3, 6), (6, 6)]
KS32 = [(1, 1), (1, 2), (3, 6)]
BFAMS = ["normal", "rigid", "repeat", "zero", "tiny", "mixed"]


@lru_cache(maxsize=None)
def aggop(name):
    """the AggOp (csr_array, int32) of an aggregation, read-only"""
    if name == "empty_cols":                                 # 9 aggregates, three without a node (one of them the last column)
        x = np.array([0, 0, 3, -1, 1, 1, 1, 3, 4, 4, -1, 6, 0, 4, 7, 7, 4, 4, 7, 1, 7, -1, 3, 4], dtype=np.int32)
        parts = aggop_from(x, 9)
    elif name == "all_unaggregated":
        parts = aggop_from(np.full(50, -1, dtype=np.int32), 0)
    elif name in HUBS:                                       # one aggregate of SORT_MAX / SORT_MAX + 1 nodes
        parts = aggop_from(np.zeros(graph(name)[0].size - 1, dtype=np.int32), 1)
    else:
        x, _, count, _ = serial_aggregation(*graph(name))
        parts = aggop_from(x, count)
    M = sp.csr_array(parts[:3][::-1], shape=parts[3])
    for a in (M.indptr, M.indices, M.data):
        a.setflags(write=False)
    return M


def fit_cases(agg):
    """every (K1, K2, dtype, B family, tol, layout) run on an aggregation"""
    out = []
    for dt, ks in (("f64", KS64), ("f32", KS32)):
        for K1, K2 in ks:
            for fam in BFAMS:
                if fam == "mixed" and dt == "f32":
                    continue
                out.append((K1, K2, dt, fam, 1e-10, "C"))
            out += [(K1, K2, dt, "normal", 0.0, "C"), (K1, K2, dt, "normal", 1.0, "C")]
    out += [(2, 3, "f64", "normal", 1e-10, "F"), (2, 3, "f64", "normal", 1e-10, "strided")]
    return out


def case_id(case):
    K1, K2, dt, fam, tol, layout = case
    return f"{K1}x{K2}.{dt}.{fam}.tol{tol:g}" + ("" if layout == "C" else "." + layout)


def candidates(agg, case):
    """B (n * K1, K2) of a case; layout 'F' is Fortran-ordered, 'strided' a slice of a wider array -- the same values"""
    K1, K2, dt, fam, tol, layout = case
    n = aggop(agg).shape[0]
    rng = _rng(f"B/{agg}/{K1}x{K2}.{dt}.{fam}")               # (tol and layout share the values of their family)
    dtype = np.float64 if dt == "f64" else np.float32
    B = rng.standard_normal((n * K1, K2))
    if fam == "rigid":                                       # ones and node coordinates: dependent on aggregates of one or two nodes
        node = np.repeat(np.arange(n), K1)
        B[:, 0] = 1.0
        if K2 > 1:
            B[:, 1] = (node % 45) / 45.0
        if K2 > 2:
            B[:, 2] = (node // 45) / 45.0
    elif fam == "repeat":
        B[:, K2 - 1 if K2 < 3 else 2] = B[:, 0]
    elif fam == "zero":
        B[:, K2 // 2] = 0.0
    elif fam == "tiny":                                      # its squares underflow to zero: the reference zeroes a non-zero column
        B[:, K2 // 2] *= 1e-170 if dt == "f64" else 1e-30
    elif fam == "mixed":
        B *= np.array([1e150, 1.0, 1e-150])[np.arange(K2) % 3]
    B = B.astype(dtype)
    if layout == "F":
        B = np.asfortranarray(B)
    elif layout == "strided":
        wide = np.zeros((n * K1, 2 * K2 + 1), dtype=dtype)
        wide[:, 1::2] = B
        B = wide[:, 1::2]
    B.setflags(write=False)
    return B


def fit_ratios(AggOp, B, K1):
    """per aggregate and column the norms before and after the modified Gram-Schmidt step (tol = 1e-10 rule), all
    aggregates at once in B's dtype: (before, after, zeroed), each (n_coarse, K2).  Magnitudes only -- the sums are not in the
    reference's order."""
    n, nc = AggOp.shape
    K2 = B.shape[1]
    node = np.repeat(np.arange(n), K1)
    has = np.diff(AggOp.indptr)[node] > 0
    rows = np.flatnonzero(has)
    a = AggOp.indices[AggOp.indptr[node[rows]]]
    W = np.array(B[rows], dtype=B.dtype)
    tol = B.dtype.type(1e-10)
    before, after = np.zeros((nc, K2), dtype=B.dtype), np.zeros((nc, K2), dtype=B.dtype)
    zeroed = np.zeros((nc, K2), dtype=bool)

    def agg_sum(v):
        return np.bincount(a, weights=v.astype(np.float64), minlength=nc).astype(B.dtype) if v.size else np.zeros(nc, dtype=B.dtype)
    for j in range(K2):
        before[:, j] = np.sqrt(agg_sum(W[:, j] * W[:, j]))
        for i in range(j):
            W[:, j] -= agg_sum(W[:, i] * W[:, j])[a] * W[:, i]
        after[:, j] = np.sqrt(agg_sum(W[:, j] * W[:, j]))
        keep = after[:, j] > tol * before[:, j]
        zeroed[:, j] = ~keep
        with np.errstate(divide="ignore", invalid="ignore"):
            W[:, j] *= np.where(keep, 1.0 / after[:, j], 0.0).astype(B.dtype)[a]
    return before, after, zeroed


def tentative_from_lists(oracle_Ax, csc, Tp):
    """the oracle's blocks, in the order of the CSC lists, put where AggOp's row order has them: a node's only entry is Tp[node]"""
    Ax = np.asarray(oracle_Ax)
    out = np.empty_like(Ax)
    out[np.asarray(Tp)[csc.indices]] = Ax
    return out


def oracle_fit(orc, agg, case):
    """(Q.data in AggOp's row order, R (n_coarse * K2, K2), Ax in list order) from the oracle"""
    K1, K2, _, _, tol, _ = case
    T = aggop(agg)
    csc = T.tocsc()
    Ax, R = orc.fit_candidates(T.shape[1], K1, K2, csc.indptr, csc.indices, candidates(agg, case), tol)
    return tentative_from_lists(Ax, csc, T.indptr), R.reshape(-1, K2), Ax


def recorded_fit(agg, case):
    """(Q.data, R) of the reference for a recorded case (stored as one array: Q.data then R), None for the others"""
    K1, K2 = case[:2]
    blob = data().get(f"fit.{agg}.{case_id(case)}")
    if blob is None:
        return None
    T = aggop(agg)
    return blob[:T.nnz * K1 * K2].reshape(T.nnz, K1, K2), blob[T.nnz * K1 * K2:].reshape(T.shape[1] * K2, K2)


def check_fit(fit_fn, core_fit_fn, agg, case, orc):
    """fit_fn(AggOp, B, tol) -> (Q, R) as tentative.fit_candidates; core_fit_fn the amg_core signature on the CSC lists (or
    None); against the oracle and, where recorded, the reference's arrays"""
    K1, K2, dt, fam, tol, layout = case
    T, B = aggop(agg), candidates(agg, case)
    want_Q, want_R, want_Ax = oracle_fit(orc, agg, case)
    what = (agg, case_id(case))
    Q, R = fit_fn(T, B, tol)
    assert Q.format == "bsr" and tuple(Q.blocksize) == (K1, K2) and Q.shape == (K1 * T.shape[0], K2 * T.shape[1]), what
    same(Q.indptr, T.indptr, what + ("Q.indptr",))
    same(Q.indices, T.indices, what + ("Q.indices",))
    same(Q.data, want_Q, what + ("Q.data",))
    same(R, want_R, what + ("R",))
    rec = recorded_fit(agg, case)
    if rec is not None:
        same(Q.data, rec[0], what + ("Q.data / fixture",))
        same(R, rec[1], what + ("R / fixture",))
    if core_fit_fn is not None:
        csc = T.tocsc()
        Ax = np.full(T.nnz * K1 * K2, -7, dtype=B.dtype)
        Rr = np.full(T.shape[1] * K2 * K2, -7, dtype=B.dtype)
        core_fit_fn(T.shape[0], T.shape[1], K1, K2, csc.indptr.astype(np.int32), csc.indices.astype(np.int32), Ax,
                    np.ravel(np.ascontiguousarray(B)).copy(), Rr, tol)
        same(Ax, np.ravel(want_Ax), what + ("amg_core Ax",))
        same(Rr, np.ravel(want_R), what + ("amg_core R",))


# =============================================================================================== operators for strength
THETAS = [0, 0.25, 0.5, 1.0, 4.0]
OPERATORS = ["poisson2d_eq", "aniso", "rand_signed", "zero_diag", "no_diag", "dup_diag", "dup_off", "empty_rows", "zero_rows",
             "subnormal_row", "scales", "one"]


def _csr(n, r, c, v, name=None):
    """rows in the given entry order (stable by row), shuffled within rows when ``name`` is given; int32 indices"""
    r, c, v = np.asarray(r), np.asarray(c), np.asarray(v, dtype=np.float64)
    order = np.lexsort((_rng(name + "/order").random(r.size), r)) if name else np.argsort(r, kind="stable")
    Ap = np.zeros(n + 1, dtype=np.int32)
    Ap[1:] = np.cumsum(np.bincount(r, minlength=n))
    return sp.csr_array((v[order], c[order].astype(np.int32), Ap), shape=(n, n))


def _stencil_operator(shape, centre, weights):
    """weights: per axis the off-diagonal value"""
    n = int(np.prod(shape))
    idx = np.arange(n).reshape(shape)
    r, c, v = [np.arange(n)], [np.arange(n)], [np.full(n, centre)]
    for ax, w in enumerate(weights):
        a, b = np.moveaxis(idx, ax, 0)[:-1].ravel(), np.moveaxis(idx, ax, 0)[1:].ravel()
        r += [a, b]
        c += [b, a]
        v += [np.full(a.size, w)] * 2
    M = sp.coo_array((np.concatenate(v), (np.concatenate(r), np.concatenate(c))), shape=(n, n)).tocsr()
    M.sort_indices()
    return sp.csr_array((M.data, M.indices.astype(np.int32), M.indptr.astype(np.int32)), shape=(n, n))


def _rand_entries(n):
    """(r, c, v) of a symmetric pattern (mean degree 4) with unsymmetric normal values and a signed stored diagonal"""
    rng = _rng(f"rand_signed/{n}")
    Ap, Aj = _graph(n, rng.integers(0, n, 2 * n), rng.integers(0, n, 2 * n), np.ones(n, dtype=bool))
    r = np.repeat(np.arange(n), np.diff(Ap))
    return r, Aj.astype(np.int64), rng.standard_normal(Aj.size)


@lru_cache(maxsize=None)
def operator(name):
    rng = _rng("op/" + name)
    if name == "poisson2d_eq":                               # theta = 0.25: a^2 = 1 = theta^2 * 4 * 4 exactly -- the '>='
        return _stencil_operator((23, 19), 4.0, (-1.0, -1.0))
    if name == "aniso":
        return _stencil_operator((20, 17), 2.002, (-1.0, -0.001))
    if name == "one":
        return sp.csr_array((np.array([2.0]), np.array([0], dtype=np.int32), np.array([0, 1], dtype=np.int32)), shape=(1, 1))
    n = 260 if name == "rand_signed" else 90                 # (random values do not compress: the variants stay small)
    r, c, v = _rand_entries(n)
    d = r == c
    if name == "rand_signed":
        pass
    elif name == "zero_diag":
        v = np.where(d, 0.0, v)
    elif name == "no_diag":                                  # the entry is missing on every third row
        keep = ~(d & (r % 3 == 0))
        r, c, v = r[keep], c[keep], v[keep]
    elif name == "dup_diag":                                 # two stored diagonal entries per row, every fourth pair cancels to 0
        second = np.where(np.arange(n) % 4 == 0, -v[d], rng.standard_normal(n))
        r, c, v = np.r_[r, np.arange(n)], np.r_[c, np.arange(n)], np.r_[v, second]
    elif name == "dup_off":
        p = rng.choice(np.flatnonzero(~d), 50, replace=False)
        r, c, v = np.r_[r, r[p]], np.r_[c, c[p]], np.r_[v, rng.standard_normal(50)]
    elif name == "empty_rows":
        keep = r % 5 != 2
        r, c, v = r[keep], c[keep], v[keep]
    elif name == "zero_rows":                                # stored zeros only
        v = np.where(r % 5 == 2, 0.0, v)
    elif name == "subnormal_row":                            # largest entry of the row 1e-310: the scaling starts from DBL_MIN
        big = np.zeros(n)
        np.maximum.at(big, r, np.abs(v))
        v = np.where(r % 6 == 1, v / big[r] * 1e-310, v)
    elif name == "scales":                                   # D A D with D = 1e75, 1, 1e-75: entries 1e+-150
        s = np.array([1e75, 1.0, 1e-75])[rng.integers(0, 3, n)]
        v = v * s[r] * s[c]
    else:
        raise KeyError(name)
    return _csr(n, r, c, v, name)


def strength_restated(A, theta):
    """(Sp, Sj, Sx): smoothed_aggregation.h:56-110, then magnitudes and every row times 1.0 / (its largest entry, found from
    DBL_MIN upwards) -- strength.py:349-352, scale_rows_by_largest_entry; Python floats in exactly this order"""
    Ap, Aj, Ax = A.indptr.tolist(), A.indices.tolist(), A.data.tolist()
    n = A.shape[0]
    theta = float(theta)
    diags = []
    for i in range(n):
        d = 0.0
        for jj in range(Ap[i], Ap[i + 1]):
            if Aj[jj] == i:
                d += Ax[jj]
        diags.append(abs(d))
    Sp, Sj, Sx = [0], [], []
    for i in range(n):
        eps = theta * theta * diags[i]
        for jj in range(Ap[i], Ap[i + 1]):
            j, a = Aj[jj], Ax[jj]
            if j == i or a * a >= eps * diags[j]:
                Sj.append(j)
                Sx.append(abs(a))
        Sp.append(len(Sj))
    for i in range(n):
        mx = sys.float_info.min
        for q in range(Sp[i], Sp[i + 1]):
            mx = max(mx, Sx[q])
        s = 1.0 / mx
        for q in range(Sp[i], Sp[i + 1]):
            Sx[q] = Sx[q] * s
    return np.array(Sp, dtype=A.indptr.dtype), np.array(Sj, dtype=A.indices.dtype), np.array(Sx, dtype=np.float64)


def recorded_strength(name, theta):
    """(indptr, indices, data) of the reference: per operator the row pointers of all THETAS are one 2-D array, indices and
    data the concatenation in THETAS' order"""
    d, k = data(), THETAS.index(theta)
    ptr = d[f"soc.{name}.indptr"]
    lo = int(ptr[:k, -1].sum())
    hi = lo + int(ptr[k, -1])
    return ptr[k], d[f"soc.{name}.indices"][lo:hi], d[f"soc.{name}.data"][lo:hi]


def check_strength(fn, name, theta, fixture=True):
    """fn(A, theta) -> csr_array against the restatement and, where recorded, the reference's arrays"""
    A = operator(name)
    keep = (A.indptr.copy(), A.indices.copy(), A.data.copy())
    S = fn(sp.csr_array((A.data.copy(), A.indices.copy(), A.indptr.copy()), shape=A.shape), theta)
    Sp, Sj, Sx = strength_restated(A, theta)
    what = (name, theta)
    assert S.format == "csr" and S.shape == A.shape, what
    same(S.indptr, Sp, what + ("indptr",))
    same(S.indices, Sj, what + ("indices",))
    same(S.data, Sx, what + ("data",))
    if fixture:
        rp, rj, rx = recorded_strength(name, theta)
        same(S.indptr, rp, what + ("indptr / fixture",))
        same(S.indices, rj, what + ("indices / fixture",))
        same(S.data, rx, what + ("data / fixture",))
    assert all(np.array_equal(a, b) for a, b in zip(keep, (A.indptr, A.indices, A.data))), what
    return S


# =============================================================================================== the recorded subset of fit cases
def recorded_fit_cases():
    """[(aggregation, case)]: every aggregation once and every (K1, K2, dtype, B family, tol) once.  The large aggregations
    take one small case each (random blocks do not compress); everything else runs on 'empty_cols'."""
    big = {"rand_iso": (1, 1, "f32", "normal", 1e-10, "C"), "pairs_2049": (1, 1, "f32", "tiny", 1e-10, "C"),
           "path_perm": (1, 1, "f32", "rigid", 1e-10, "C"), "star_first": (1, 1, "f64", "rigid", 1e-10, "C"),
           "grid9_diag": (1, 2, "f32", "rigid", 1e-10, "C"), "all_unaggregated": (1, 3, "f64", "normal", 1e-10, "C"),
           "hub_at_bound": (1, 1, "f32", "zero", 1e-10, "C")}
    taken = set(big.values())
    out = list(big.items())
    out += [("empty_cols", c) for c in fit_cases("empty_cols") if c not in taken and c[5] == "C"]
    return out
