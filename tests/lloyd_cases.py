"""The committed cases of Bellman-Ford, most_interior_nodes, lloyd_cluster and lloyd_aggregation (tests/golden/kernels_lloyd.npz, written by
tests/golden/make_golden_lloyd.py from the reference) and the checks the host replay and the device share: every comparison is
``np.array_equal`` -- there is no tolerance."""
import warnings
from functools import lru_cache
from pathlib import Path

import numpy as np
import scipy.sparse as sp

GOLDEN = Path(__file__).resolve().parent / "golden" / "kernels_lloyd.npz"
NAMES = ["grid17x13", "grid40x33", "box6x5x4", "irr200", "hub", "path300", "n1", "one_cluster"]


@lru_cache(maxsize=1)
def data():
    with np.load(GOLDEN) as z:
        d = {k: z[k] for k in z.files}
    for v in d.values():
        v.setflags(write=False)                              # shared among the tests: nobody changes it
    return d


def csr(prefix, shape=None):
    d = data()
    indptr = d[prefix + ".indptr"]
    n = indptr.size - 1
    return sp.csr_array((d[prefix + ".data"].copy(), d[prefix + ".indices"].copy(), indptr.copy()), shape=shape or (n, n))


def graph(name):
    return csr(f"ll.{name}.G")


def centers(name):
    return data()[f"ll.{name}.centers"].copy()


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (what, np.flatnonzero(got != want)[:10])


def rounds_ok(n, dist_rounds, stamp_rounds, calls):
    """per Bellman-Ford at least one round of each kind (the one that finds nothing to change) and at most n"""
    assert calls <= dist_rounds <= calls * n and calls <= stamp_rounds <= calls * n, (n, dist_rounds, stamp_rounds, calls)


def check_bellman_ford(gr, name):
    """the reference's (distances, nearest, predecessors); returns (distance rounds, stamp rounds)"""
    d = data()
    G, c = graph(name), centers(name)
    keep = (G.indptr.copy(), G.indices.copy(), G.data.copy(), c.copy())
    info = []
    dist, near, pred = gr.bellman_ford(G, c, info=info)
    for got, k in ((dist, "d"), (near, "m"), (pred, "p")):
        same(got, d[f"ll.{name}.bf.{k}"], (name, "bf", k))
    assert all(np.array_equal(a, b) for a, b in zip(keep, (G.indptr, G.indices, G.data, c)))      # the inputs are not touched
    assert np.array_equal(gr.bellman_ford(G, list(c), method="standard")[2], pred)
    rounds_ok(G.shape[0], *info[0], 1)
    return info[0]


def check_most_interior_nodes(core, name):
    """one amg_core.most_interior_nodes after the fixture's Bellman-Ford; returns (distance rounds, stamp rounds, centres moved)"""
    d = data()
    G, c = graph(name), centers(name)
    n = G.shape[0]
    dist = np.full(n, -7.0)                                  # overwritten: the reference fills it first
    m, p = d[f"ll.{name}.bf.m"].copy(), d[f"ll.{name}.bf.p"].copy()
    info = []
    changed = core.most_interior_nodes(n, G.indptr, G.indices, G.data, c, dist, m, p, info=info)
    for got, k in ((dist, "d"), (m, "m"), (p, "p"), (c, "c")):
        same(got, d[f"ll.{name}.mi.{k}"], (name, "mi", k))
    assert changed is bool(d[f"ll.{name}.mi.changed"])
    assert (info[0][2] > 0) == changed and info[0][2] == int(np.sum(c != centers(name)))
    rounds_ok(n, info[0][0], info[0][1], 1)
    return info[0]


def check_lloyd_cluster(gr, name, maxiter):
    """the reference's (clusters, centers); returns (Lloyd iterations, distance rounds, stamp rounds, centres moved last)"""
    d = data()
    G, c = graph(name), centers(name)
    info = []
    clusters, cent = gr.lloyd_cluster(G, c, maxiter=maxiter, info=info)
    same(clusters, d[f"ll.{name}.lc{maxiter}.clusters"], (name, "lc", maxiter, "clusters"))
    same(cent, d[f"ll.{name}.lc{maxiter}.centers"], (name, "lc", maxiter, "centers"))
    assert cent is c                                         # an int32 array of centres is updated in place, as in the reference
    its, dr, sr, moved = info[0]
    assert 1 <= its <= maxiter and (its == maxiter or moved == 0)
    rounds_ok(G.shape[0], dr, sr, 2 * its)
    return info[0]


def check_lloyd_aggregation(gr, name):
    """the reference's AggOp arrays and centres from the same seed, and the random stream where the reference leaves it"""
    d = data()
    G = graph(name)
    measure = str(d[f"ll.{name}.agg.measure"])
    state = np.random.get_state()
    try:
        np.random.seed(int(d[f"ll.{name}.agg.seed"]))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            AggOp, cent = gr.lloyd_aggregation(G, ratio=float(d[f"ll.{name}.agg.ratio"]), measure=None if measure == "none" else measure)
        follow = np.random.rand()
    finally:
        np.random.set_state(state)
    assert sp.issparse(AggOp) and AggOp.format == "csr" and AggOp.shape == (G.shape[0], int(d[f"ll.{name}.agg.naggs"]))
    for k in ("indptr", "indices", "data"):
        same(getattr(AggOp, k), d[f"ll.{name}.agg.{k}"], (name, "agg", k))
    same(cent, d[f"ll.{name}.agg.centers"], (name, "agg", "centers"))
    assert follow == float(d[f"ll.{name}.agg.next"])


def check_first_level(gr, strength, fit_candidates, product):
    """symmetric strength -> lloyd_aggregation -> fit_candidates -> Galerkin product of the 17 x 13 operator, as
    smoothed_aggregation_solver(aggregate='lloyd', smooth=None, improve_candidates=None) composes them"""
    d = data()
    A = csr("e2e.A")
    state = np.random.get_state()
    try:
        np.random.seed(int(d["e2e.seed"]))
        C = strength(A, theta=0.0)
        AggOp, _ = gr.lloyd_aggregation(C)
    finally:
        np.random.set_state(state)
    assert AggOp.shape == (A.shape[0], int(d["e2e.AggOp.naggs"]))
    for k in ("indptr", "indices", "data"):
        same(getattr(AggOp, k), d[f"e2e.AggOp.{k}"], ("e2e.AggOp", k))
    T, _ = fit_candidates(AggOp, np.ones((A.shape[0], 1)))
    T = sp.csr_array(T)
    for k in ("indptr", "indices", "data"):
        same(getattr(T, k), d[f"e2e.T.{k}"], ("e2e.T", k))
    A1 = sp.csr_array(product(sp.csr_array(T.T), A, T))
    for k in ("indptr", "indices", "data"):
        same(getattr(A1, k), d[f"e2e.A1.{k}"], ("e2e.A1", k))
