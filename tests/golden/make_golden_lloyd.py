#!/usr/bin/env python3
"""Generate tests/golden/kernels_lloyd.npz: graphs and the reference's own outputs for Bellman-Ford, most_interior_nodes, lloyd_cluster
and lloyd_aggregation.

Run in the build container (needs the reference built into oracle/_ref by oracle/build_ref.py):
    python tests/golden/make_golden_lloyd.py

Before anything is written, the closed form of csrc/pamg_lloyd.h (distances, stamps, labels, centre rule) is replayed in NumPy and
asserted equal to the reference's in-place serial loops on RANDOM_CASES random exact-weight graphs.

Keys (graphs are ``<prefix>.indptr / .indices / .data``; ``ll.names`` lists them):

  ll.<g>.G, ll.<g>.centers                   the graph and the start centres
  ll.<g>.bf.d / .m / .p                      pyamg.graph.bellman_ford(G, centers)
  ll.<g>.mi.d / .m / .p / .c / .changed      one amg_core.most_interior_nodes after it
  ll.<g>.lc<k>.clusters / .centers           pyamg.graph.lloyd_cluster(G, centers, maxiter=k), k = 1, 5
  ll.<g>.agg.indptr / .indices / .data / .centers / .naggs, .agg.seed / .ratio / .measure / .next
                                             lloyd_aggregation(G, ratio, measure) after np.random.seed(seed), and the next
                                             np.random.rand() after the call
      grid17x13    5-point lattice, unit weights: ties everywhere
      grid40x33    1320 nodes, 132 centres: more than one workgroup
      box6x5x4     27-point lattice
      irr200       non-symmetric, unsorted rows, integer weights 1..3: empty rows, diagonal-only rows, unreached nodes
      hub          one row of 100 entries
      path300      a path stored in index order, single centre at node 299: the serial loop needs about 300 sweeps
      n1           a single node
      one_cluster  a cluster without any boundary: all boundary distances inf, the centre stays
  absorb.G, absorb.centers, absorb.ref.d / .m / .p, absorb.closed.p
                                             weights 1e-20 and 1.0: a sum absorbs a weight, and the closed form names another
                                             predecessor than the reference (asserted) -- the case the device path must refuse
  e2e.A, e2e.seed, e2e.AggOp, e2e.T, e2e.A1  one level of smoothed_aggregation_solver(A, aggregate='lloyd', smooth=None,
                                             improve_candidates=None) on the 17 x 13 operator: symmetric strength ->
                                             lloyd_aggregation -> fit_candidates -> T^T A T
"""
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
from pyamg import graph as ref_graph  # noqa: E402
from pyamg.aggregation.aggregate import lloyd_aggregation as ref_lloyd_aggregation  # noqa: E402
from pyamg.aggregation.tentative import fit_candidates as ref_fit_candidates  # noqa: E402
from pyamg.gallery import poisson, stencil_grid  # noqa: E402
from pyamg.strength import symmetric_strength_of_connection as ref_strength  # noqa: E402
from make_golden_classical import irr200, put, raw_csr  # noqa: E402
from make_golden_cljp import hub  # noqa: E402

SEED = 20261021
OUT = HERE / "kernels_lloyd.npz"
LIMIT = (HERE / "kernels_classical.npz").stat().st_size
RANDOM_CASES = 240
NO_STAMP, SOURCE_STAMP, LOW = np.uint64(2 ** 64 - 1), np.uint64(0xFFFFFFFF), np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ the closed form in NumPy
def closed_bellman_ford(G, d, m, p):
    """rules 1 to 3 of csrc/pamg_lloyd.h, synchronous rounds; in place on d, m, p"""
    n = G.shape[0]
    rows = np.repeat(np.arange(n), np.diff(G.indptr)).astype(np.int64)
    cols, w = G.indices.astype(np.int64), G.data
    while True:                                             # 1. distances
        new = d.copy()
        np.minimum.at(new, cols, d[rows] + w)
        if np.array_equal(new, d):
            break
        d[:] = new
    key = np.where(d == 0, SOURCE_STAMP, NO_STAMP).astype(np.uint64)
    tight = np.isfinite(d[rows]) & (d[cols] != 0) & (d[rows] + w == d[cols])
    while True:                                             # 2. stamps
        ki = key[rows]
        ok = tight & (ki != NO_STAMP)
        sweep = (ki >> np.uint64(32)).astype(np.int64)
        writer = (ki & LOW).astype(np.int64)
        writer[writer == 0xFFFFFFFF] = -1
        visit = np.where(writer < rows, sweep, sweep + 1)
        cand = (visit.astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)
        new = key.copy()
        np.minimum.at(new, cols[ok], cand[ok])
        if np.array_equal(new, key):
            break
        key = new
    written = (key != NO_STAMP) & (key != SOURCE_STAMP)
    q = np.where(written, (key & LOW).astype(np.int64), np.arange(n))
    while not np.array_equal(q[q], q):                      # 3. labels
        q = q[q]
    p[written] = (key & LOW).astype(np.int64)[written]
    m[written] = m[q[written]]


def closed_most_interior_nodes(G, c, d, m, p):
    """rule 4; in place; returns whether a centre moved"""
    n = G.shape[0]
    rows = np.repeat(np.arange(n), np.diff(G.indptr))
    d[:] = np.inf
    d[rows[m[rows] != m[G.indices]]] = 0
    closed_bellman_ford(G, d, m, p)
    changed = False
    for a in range(len(c)):
        members = np.flatnonzero(m == a)
        if members.size and d[c[a]] < d[members].max():
            c[a] = members[d[members] == d[members].max()].min()
            changed = True
    return changed


def start(n, centers):
    d = np.full(n, np.inf)
    m = np.full(n, -1, dtype=np.int32)
    p = np.full(n, -1, dtype=np.int32)
    d[centers] = 0
    m[centers] = np.arange(len(centers))
    return d, m, p


def closed_lloyd_cluster(G, centers, maxiter):
    c = np.array(centers, dtype=np.int32)
    n = G.shape[0]
    d, m, p = start(n, c)
    changed, it = True, 0
    while changed and it < maxiter:
        d, m, p = start(n, c)
        closed_bellman_ford(G, d, m, p)
        changed = closed_most_interior_nodes(G, c, d, m, p)
        it += 1
    return m, c


def ref_bf(G, d, m, p, c):
    ref_core.bellman_ford(G.shape[0], G.indptr, G.indices, G.data, c, d, m, p)


def ref_mi(G, c, d, m, p):
    return bool(ref_core.most_interior_nodes(G.shape[0], G.indptr, G.indices, G.data, c, d, m, p))


def random_graph(rng, k):
    """exact weights: lattices, permuted lattices, non-symmetric random graphs with weights 1..3"""
    kind = k % 4
    if kind in (0, 1):
        shape = (int(rng.randint(2, 9)), int(rng.randint(2, 9)))
        G = sp.csr_array(poisson(shape, format="csr"))
        G.data[:] = 1.0
        if kind == 1:
            perm = rng.permutation(G.shape[0])
            G = sp.csr_array(sp.csr_array(G[perm][:, perm]))
            G.sort_indices()
        if k % 8 >= 4:
            G.data[:] = rng.randint(1, 4, size=G.nnz).astype(float)
        return G
    n = int(rng.randint(1, 41))
    rows = []
    for i in range(n):
        cols = rng.choice(n, size=min(n, int(rng.randint(0, 5))), replace=False)
        rows.append((cols, rng.randint(1, 4, size=len(cols)).astype(float) if kind == 2 else np.ones(len(cols))))
    return raw_csr(rows, n)


def same(a, b, what):
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), what


def check_closed_form():
    rng = np.random.RandomState(SEED)
    for k in range(RANDOM_CASES):
        G = random_graph(rng, k)
        G = sp.csr_array((G.data.astype(np.float64), G.indices.astype(np.int32), G.indptr.astype(np.int32)), shape=G.shape)
        n = G.shape[0]
        nc = int(rng.randint(1, max(2, n // 3 + 1)))
        c = rng.permutation(n)[:nc].astype(np.int32)
        # bellman_ford from the centres, and from a multi-source start with arbitrary labels, -1 included
        for arbitrary in (False, True):
            d, m, p = start(n, c)
            if arbitrary:
                m = rng.randint(-1, 4, size=n).astype(np.int32)
                p = rng.randint(-1, n, size=n).astype(np.int32)
            want = (d.copy(), m.copy(), p.copy())
            ref_bf(G, *want, c)
            closed_bellman_ford(G, d, m, p)
            same((d, m, p), want, ("bellman_ford", k, arbitrary))
        m_in, p_in = np.clip(m, -1, nc - 1).astype(np.int32), p.copy()     # any labels below the number of clusters, any predecessors
        want, cw = (np.empty(n), m_in.copy(), p_in.copy()), c.copy()
        got, cc = (np.empty(n), m_in.copy(), p_in.copy()), c.copy()
        ch_w = ref_mi(G, cw, *want)
        ch_c = closed_most_interior_nodes(G, cc, *got)
        same(got + (cc, [ch_c]), want + (cw, [ch_w]), ("most_interior_nodes", k))
        for maxiter in (1, 5):
            cw = c.copy()
            want = ref_graph.lloyd_cluster(G, cw, maxiter=maxiter)
            same(closed_lloyd_cluster(G, c, maxiter), want, ("lloyd_cluster", k, maxiter))
    return RANDOM_CASES


def absorb():
    """1e-20 is absorbed by 1.0.  Sweep 0: rows 0, 1, 2 give node 3 the distance 3e-20; row 3 writes d[5] = 1.0 (p = 3); row 4 is tight
    to 5 as well but not strictly better; row 6 lowers d[3] to 2e-20.  Node 3's FINAL value arrives after row 3 was visited, so the closed
    form has row 3 offer in sweep 1 and names row 4 (sweep 0) as the predecessor of 5; the reference keeps 3."""
    e = 1e-20
    rows = [([1, 4, 6], [e, e, e]), ([2], [e]), ([3], [e]), ([5], [1.0]), ([5], [1.0]), ([], []), ([3], [e])]
    return raw_csr(rows, 7)


def unit(G):
    G = sp.csr_array(G)
    return sp.csr_array((np.ones(G.nnz), G.indices.astype(np.int32), G.indptr.astype(np.int32)), shape=G.shape)


def record(out, name, G, centers, ratio, measure):
    G = sp.csr_array((G.data.astype(np.float64), G.indices.astype(np.int32), G.indptr.astype(np.int32)), shape=G.shape)
    n = G.shape[0]
    c = np.asarray(centers, dtype=np.int32)
    assert np.unique(c).size == c.size
    put(out, f"ll.{name}.G", G)
    out[f"ll.{name}.centers"] = c.copy()
    d, m, p = ref_graph.bellman_ford(G, c.copy())
    out[f"ll.{name}.bf.d"], out[f"ll.{name}.bf.m"], out[f"ll.{name}.bf.p"] = d.copy(), m.copy(), p.copy()
    cd, cm, cp = start(n, c)
    closed_bellman_ford(G, cd, cm, cp)
    same((cd, cm, cp), (d, m, p), name)
    cc = c.copy()
    changed = ref_mi(G, cc, d, m, p)
    for k, v in (("d", d), ("m", m), ("p", p), ("c", cc), ("changed", np.int32(changed))):
        out[f"ll.{name}.mi.{k}"] = np.array(v)
    for k in (1, 5):
        clusters, cent = ref_graph.lloyd_cluster(G, c.copy(), maxiter=k)
        same(closed_lloyd_cluster(G, c, k), (clusters, cent), (name, k))
        out[f"ll.{name}.lc{k}.clusters"], out[f"ll.{name}.lc{k}.centers"] = clusters.copy(), cent.copy()
    seed = SEED + len(name)
    np.random.seed(seed)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        AggOp, cent = ref_lloyd_aggregation(G, ratio=ratio, measure=measure)
    out[f"ll.{name}.agg.next"] = np.float64(np.random.rand())
    assert AggOp.format == "csr" and AggOp.data.dtype == np.int32 and AggOp.indices.dtype == np.int32
    for k in ("indptr", "indices", "data"):
        out[f"ll.{name}.agg.{k}"] = getattr(AggOp, k).copy()
    out[f"ll.{name}.agg.centers"], out[f"ll.{name}.agg.naggs"] = np.asarray(cent).copy(), np.int64(AggOp.shape[1])
    out[f"ll.{name}.agg.seed"], out[f"ll.{name}.agg.ratio"] = np.int64(seed), np.float64(ratio)
    out[f"ll.{name}.agg.measure"] = np.array("none" if measure is None else measure)


def main():
    ncases = check_closed_form()
    print(f"closed form == reference on {ncases} random exact-weight graphs")
    assert ncases >= 200
    rng = np.random.RandomState(SEED + 1)
    out = {}
    st = -np.ones((3, 3, 3)); st[1, 1, 1] = 26.0
    Gi = irr200()
    Gi = sp.csr_array((rng.randint(1, 4, size=Gi.nnz).astype(float), Gi.indices, Gi.indptr), shape=Gi.shape)
    assert not Gi.has_sorted_indices and abs(Gi - Gi.T).nnz
    path = sp.csr_array(sp.diags_array([np.ones(299), np.ones(299)], offsets=[-1, 1], format="csr"))
    assert path.has_sorted_indices
    cases = {
        "grid17x13": (unit(poisson((17, 13), format="csr")), rng.permutation(221)[:22], 0.1, "unit"),
        "grid40x33": (unit(poisson((40, 33), format="csr")), rng.permutation(1320)[:132], 0.1, "unit"),
        "box6x5x4": (unit(stencil_grid(st, (6, 5, 4), format="csr")), rng.permutation(120)[:9], 0.08, "unit"),
        "irr200": (Gi, np.concatenate([[7], 10 + rng.permutation(190)[:14]]), 0.1, None),
        "hub": (unit(hub()), np.array([0, 120]), 0.05, "unit"),
        "path300": (path, np.array([299]), 0.02, "unit"),
        "n1": (sp.csr_array(np.array([[1.0]])), np.array([0]), 0.1, "unit"),
        "one_cluster": (unit(poisson((5, 4), format="csr")), np.array([7]), 0.01, "unit"),
    }
    for name, (G, c, ratio, measure) in cases.items():
        record(out, name, G, c, ratio, measure)
    out["ll.names"] = np.array(list(cases))
    assert np.sum(out["ll.irr200.bf.m"] == -1) >= 5 and np.isinf(out["ll.irr200.bf.d"]).sum() >= 5      # unreached nodes keep inf / -1 / -1
    assert np.all(np.isinf(out["ll.one_cluster.mi.d"])) and out["ll.one_cluster.mi.changed"] == 0 and out["ll.one_cluster.mi.c"][0] == 7
    assert out["ll.hub.G.indptr"][1] == 100
    # ---------------------------------------------------------------- the case the device path refuses
    Ga = absorb()
    ca = np.array([0], dtype=np.int32)
    put(out, "absorb.G", Ga)
    out["absorb.centers"] = ca
    d, m, p = ref_graph.bellman_ford(Ga, ca.copy())
    cd, cm, cp = start(7, ca)
    closed_bellman_ford(Ga, cd, cm, cp)
    assert np.array_equal(cd, d) and p[5] == 3 and cp[5] == 4, (p, cp)       # same distances, another predecessor
    out["absorb.ref.d"], out["absorb.ref.m"], out["absorb.ref.p"], out["absorb.closed.p"] = d, m, p, cp
    # ---------------------------------------------------------------- end to end
    A = sp.csr_array(poisson((17, 13), format="csr"))
    put(out, "e2e.A", A)
    seed = SEED + 2
    np.random.seed(seed)
    C = ref_strength(A, theta=0.0)
    AggOp, _ = ref_lloyd_aggregation(C)
    T, _ = ref_fit_candidates(AggOp, np.ones((A.shape[0], 1)))
    T = sp.csr_array(T)
    A1 = sp.csr_array(sp.csr_array(T.T) @ A @ T)
    np.random.seed(seed)
    ml = pyamg.smoothed_aggregation_solver(A.copy(), aggregate="lloyd", smooth=None, improve_candidates=None, max_levels=2, keep=True)
    assert np.array_equal(sp.csr_array(ml.levels[0].AggOp).toarray(), AggOp.toarray())
    assert np.allclose(sp.csr_array(ml.levels[1].A).toarray(), A1.toarray(), rtol=1e-13, atol=0)      # (the solver multiplies BSR operands)
    out["e2e.seed"] = np.int64(seed)
    put(out, "e2e.AggOp", AggOp, data=False); out["e2e.AggOp.data"] = AggOp.data.copy(); out["e2e.AggOp.naggs"] = np.int64(AggOp.shape[1])
    put(out, "e2e.T", T)
    put(out, "e2e.A1", A1)
    np.savez_compressed(OUT, **out)
    size = OUT.stat().st_size
    assert size <= LIMIT, (size, LIMIT)
    print(f"{OUT.name}: {len(out)} arrays, {size} bytes (limit {LIMIT})")


if __name__ == "__main__":
    main()
