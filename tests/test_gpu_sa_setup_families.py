"""GPU parity of the smoothed-aggregation setup kernels on the adversarial families of tests/sa_setup_families.py:
standard_aggregation (csrc/pamg_aggregate.hip, host-array and resident entry), fit_candidates / fit_tentative, and
symmetric_strength_of_connection (csrc/pamg_setup.hip) against the plain-Python restatements, the oracle and the reference's
recorded outputs (tests/golden/kernels_sa_setup_families.npz).  Every comparison is ``np.array_equal``: the project claims
these arrays bit for bit.

The guard of the one-lane insertion sorts (a row / an aggregate of more than SORT_MAX = 4096 entries is refused) is tested on
both sides of the bound; the over-bound inputs are never sorted.

Not exercised: graphs above 6145 nodes, hence the 4096-workgroup cap of agg_grid (more than 1 048 576 nodes)."""
import sys
import time
import types

import numpy as np
import pytest
import scipy.sparse as sp

import sa_setup_families as fam
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


def _core_aggregation(Ap, Aj):
    """pyamg_amd.amg_core.standard_aggregation on host arrays; x, y pre-filled so an unwritten slot shows"""
    from pyamg_amd import amg_core as gcore
    n = Ap.size - 1
    x, y = np.full(n, -7, dtype=np.int32), np.full(n, -7, dtype=np.int32)
    count = gcore.standard_aggregation(n, np.ascontiguousarray(Ap, dtype=np.int32), np.ascontiguousarray(Aj, dtype=np.int32), x, y)
    assert np.all(y[count:] == -7) and not np.any(x == -7) and not np.any(y[:count] == -7)
    return x, y, count


def _csr(name):
    """the family as a csr_array that really holds the family's index type"""
    Ap, Aj = fam.graph(name)
    C = sp.csr_array((np.ones(Aj.size), Aj.astype(np.int32), Ap.astype(np.int32)), shape=(Ap.size - 1,) * 2)
    if Ap.dtype != np.int32:
        C.indptr, C.indices = Ap.copy(), Aj.copy()
    assert C.indptr.dtype == Ap.dtype and C.indices.dtype == Aj.dtype
    return C


# --------------------------------------------------------------------------------------------- aggregation
@pytest.mark.parametrize("name", fam.FAMILIES)
def test_aggregation_on_host_arrays(name):
    from pyamg_amd import amg_core as gcore
    if name.endswith("_i64"):                                # the amg_core signature takes int32 arrays only, like the reference's
        Ap, Aj = fam.graph(name)
        with pytest.raises(TypeError):
            gcore.standard_aggregation(Ap.size - 1, Ap, Aj, np.zeros(Ap.size - 1, dtype=np.int32), np.zeros(Ap.size - 1, dtype=np.int32))
    fam.check_aggregation(_core_aggregation, name)


@pytest.mark.parametrize("name", fam.FAMILIES)
def test_aggregation_returns_the_references_aggop(name):
    from pyamg_amd.aggregation import standard_aggregation
    C = _csr(name)
    AggOp, Cpts = standard_aggregation(C)
    fam.check_aggop(AggOp, Cpts, name)
    n, count = C.shape[0], fam.data()[f"agg.{name}.y"].size
    assert AggOp.shape == ((n, count) if count else (n, 1))


def test_aggregation_twice_gives_identical_arrays():
    """the atomics only decide the order of the work lists"""
    a, b = _core_aggregation(*fam.graph("rand_iso")), _core_aggregation(*fam.graph("rand_iso"))
    assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", fam.REFUSALS)
def test_aggregation_refuses_and_recovers(name):
    from pyamg_amd import amg_core as gcore
    from pyamg_amd.aggregation import standard_aggregation
    Ap, Aj = fam.graph(name)
    n = Ap.size - 1
    with pytest.raises(NotImplementedError):
        standard_aggregation(sp.csr_array((np.ones(Aj.size), Aj.copy(), Ap.copy()), shape=(n, n)))
    with pytest.raises(NotImplementedError):
        gcore.standard_aggregation(n, Ap.copy(), Aj.copy(), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32))
    fam.check_aggregation(_core_aggregation, "rand_iso_shuf")       # a good family right after: its usual result


def test_aggregation_argument_errors():
    from pyamg_amd.aggregation import standard_aggregation
    with pytest.raises(ValueError):
        standard_aggregation(sp.csr_array((3, 4)))
    with pytest.raises(TypeError):
        standard_aggregation(_csr("clique64").tocsc())
    fam.check_aggregation(_core_aggregation, "clique64")


# --------------------------------------------------------------------------------------------- strength
@pytest.mark.parametrize("name", fam.OPERATORS)
def test_strength(name):
    from pyamg_amd.aggregation import symmetric_strength_of_connection
    for theta in fam.THETAS:
        fam.check_strength(symmetric_strength_of_connection, name, theta)


# --------------------------------------------------------------------------------------------- tentative prolongator
@pytest.mark.parametrize("K1,K2,dt", [k + ("f64",) for k in fam.KS64] + [k + ("f32",) for k in fam.KS32])
@pytest.mark.parametrize("agg", fam.AGGS)
def test_fit_candidates(agg, K1, K2, dt):
    """every B family, tol and layout of one (K1, K2, dtype): aggregation.fit_candidates (pamg_fit_tentative) and
    amg_core.fit_candidates (pamg_fit_candidates) against the oracle and, where recorded, the reference"""
    from pyamg_amd import amg_core as gcore
    from pyamg_amd.aggregation import fit_candidates
    cases = [c for c in fam.fit_cases(agg) if c[:3] == (K1, K2, dt)]
    assert len(cases) >= 7
    for case in cases:
        fam.check_fit(lambda T, B, tol: fit_candidates(T, B, tol=tol), gcore.fit_candidates, agg, case, orc)


def test_every_aggregation_is_recorded_once():
    for agg in fam.AGGS:
        assert any(fam.recorded_fit(agg, case) is not None for case in fam.fit_cases(agg)), agg


# --------------------------------------------------------------------------------------------- the chain, host arrays and resident
CHAIN = [("grid9_diag", 0.1), ("rand_signed", 0), ("aniso", 0.25)]           # (centre 8, neighbours -1: theta = 0.125 is the edge)


def _chain_operator(name):
    if name != "grid9_diag":
        return fam.operator(name)
    Ap, Aj = fam.graph(name)
    rows = np.repeat(np.arange(Ap.size - 1), np.diff(Ap))
    return sp.csr_array((np.where(Aj == rows, 8.0, -1.0), Aj.copy(), Ap.copy()), shape=(Ap.size - 1,) * 2)


def _standin(monkeypatch):
    """a package with the two modules device_setup patches these names in; its own functions must never run"""
    def reference_fn(*a, **k):
        raise AssertionError("the reference function was called")
    mods = {}
    for name in ("standin_sa", "standin_sa.strength", "standin_sa.aggregation", "standin_sa.aggregation.aggregation"):
        m = types.ModuleType(name)
        mods[name] = m
        monkeypatch.setitem(sys.modules, name, m)
        if "." in name:
            setattr(mods[name.rsplit(".", 1)[0]], name.rsplit(".", 1)[1], m)
    for fn in ("symmetric_strength_of_connection", "standard_aggregation", "fit_candidates"):
        setattr(mods["standin_sa.aggregation.aggregation"], fn, reference_fn)
    mods["standin_sa.strength"].symmetric_strength_of_connection = reference_fn
    return mods["standin_sa"], mods["standin_sa.aggregation.aggregation"]


@pytest.mark.parametrize("name,theta", CHAIN)
def test_chain_on_host_arrays_and_resident(name, theta, monkeypatch):
    """strength -> aggregation -> fit_candidates(AggOp, ones) equals the chain of restatements and oracle, array for array;
    inside device_setup(aggregation=True) the strength matrix stays resident for the aggregation and gives the same"""
    from pyamg_amd import aggregation as agg
    A = _chain_operator(name)
    Sp, Sj, Sx = fam.strength_restated(A, theta)
    x, y, count, opened = fam.serial_aggregation(Sp, Sj)
    assert opened == 0 and count > 1
    indptr, indices, vals, shape = fam.aggop_from(x, count)
    T = sp.csr_array((vals, indices, indptr), shape=shape)
    csc = T.tocsc()
    Ax, R = orc.fit_candidates(count, 1, 1, csc.indptr, csc.indices, np.ones((A.shape[0], 1)), 1e-10)
    want_Q = fam.tentative_from_lists(Ax, csc, T.indptr)

    def check(S, AggOp, Cpts, Q, Rc, how):
        for got, want, what in ((S.indptr, Sp, "S.indptr"), (S.indices, Sj, "S.indices"), (S.data, Sx, "S.data"), (AggOp.indptr, indptr, "AggOp.indptr"),
                                (AggOp.indices, indices, "AggOp.indices"), (AggOp.data, vals, "AggOp.data"), (Cpts, y, "Cpts"),
                                (Q.indptr, indptr, "Q.indptr"), (Q.indices, indices, "Q.indices"), (Q.data, want_Q, "Q.data"),
                                (Rc, R.reshape(-1, 1), "R")):
            fam.same(got, want, (name, how, what))
        assert AggOp.shape == shape
    S = agg.symmetric_strength_of_connection(A.copy(), theta)
    assert not agg._RESIDENT                                 # no hand-off outside device_setup
    AggOp, Cpts = agg.standard_aggregation(S)
    Q, Rc = agg.fit_candidates(AggOp, np.ones((A.shape[0], 1)))
    check(S, AggOp, Cpts, Q, Rc, "host arrays")
    pkg, mod = _standin(monkeypatch)
    with agg.device_setup(pkg, aggregation=True, products=False):
        S = mod.symmetric_strength_of_connection(A.copy(), theta)
        assert len(agg._RESIDENT) == 1                       # the device copy waits for the aggregation
        AggOp, Cpts = mod.standard_aggregation(S)
        assert not agg._RESIDENT                             # ... and is released by it
        Q, Rc = mod.fit_candidates(AggOp, np.ones((A.shape[0], 1)))
        check(S, AggOp, Cpts, Q, Rc, "resident")
        mod.symmetric_strength_of_connection(A.copy(), theta)
        assert len(agg._RESIDENT) == 1
    assert not agg._RESIDENT                                 # nothing is left behind


# --------------------------------------------------------------------------------------------- the guard of the one-lane sorts
def test_guard_at_the_bound_is_exact(capsys):
    """a row of exactly SORT_MAX stored entries and an aggregate of exactly SORT_MAX nodes: accepted, and exact"""
    from pyamg_amd import amg_core as gcore
    from pyamg_amd.aggregation import fit_candidates, standard_aggregation
    t0 = time.perf_counter()
    fam.check_aggregation(_core_aggregation, "hub_at_bound")
    t1 = time.perf_counter()
    AggOp, Cpts = standard_aggregation(_csr("hub_at_bound"))
    t2 = time.perf_counter()
    fam.check_aggop(AggOp, Cpts, "hub_at_bound")
    assert np.array_equal(AggOp.indices, fam.aggop("hub_at_bound").indices) and AggOp.shape == (fam.SORT_MAX, 1)
    times = []
    for case in ((1, 1, "f32", "zero", 1e-10, "C"), (1, 1, "f64", "normal", 1e-10, "C"), (2, 3, "f64", "normal", 1e-10, "C"),
                 (3, 6, "f32", "normal", 1e-10, "C")):
        t3 = time.perf_counter()
        fam.check_fit(lambda T, B, tol: fit_candidates(T, B, tol=tol), gcore.fit_candidates, "hub_at_bound", case, orc)
        times.append(time.perf_counter() - t3)
    with capsys.disabled():
        print(f"\n[guard at the bound] aggregation of a {fam.SORT_MAX}-entry row: amg_core {t1 - t0:.3f} s, aggregation {t2 - t1:.3f} s; "
              f"fit of a {fam.SORT_MAX}-node aggregate (with the oracle's run): " + ", ".join(f"{t:.3f}" for t in times) + " s")


def test_guard_over_the_bound_refuses_before_any_sort(monkeypatch):
    from pyamg_amd import _capi as capi
    from pyamg_amd import aggregation as agg
    from pyamg_amd import amg_core as gcore
    Ap, Aj = fam.graph("hub_over_bound")
    n = Ap.size - 1
    fam.check_aggregation(_core_aggregation, "clique64")     # (the library is loaded and warm: the times below are the calls')
    x, y = np.full(n, -7, dtype=np.int32), np.full(n, -7, dtype=np.int32)
    t0 = time.perf_counter()
    with pytest.raises(NotImplementedError):
        gcore.standard_aggregation(n, Ap.copy(), Aj.copy(), x, y)
    t1 = time.perf_counter()
    assert np.all(x == -7) and np.all(y == -7) and t1 - t0 < 0.5
    with pytest.raises(NotImplementedError):
        agg.standard_aggregation(_csr("hub_over_bound"))
    # the resident entry finds the longest row on the device
    A = sp.csr_array((np.where(Aj == np.repeat(np.arange(n), np.diff(Ap)), 2.0, -1.0), Aj.copy(), Ap.copy()), shape=(n, n))
    pkg, mod = _standin(monkeypatch)
    with agg.device_setup(pkg, aggregation=True, products=False):
        S = mod.symmetric_strength_of_connection(A, 0)
        assert len(agg._RESIDENT) == 1
        t0 = time.perf_counter()
        with pytest.raises(NotImplementedError):
            agg.standard_aggregation(S)
        assert time.perf_counter() - t0 < 0.5
    assert not agg._RESIDENT
    # an aggregate of SORT_MAX + 1 nodes: refused by pamg_fit_tentative, outputs untouched
    T = fam.aggop("hub_over_bound")
    B = np.ones((n, 1))
    with pytest.raises(NotImplementedError):
        agg.fit_candidates(T, B)
    for fn, dtype in ((capi.lib().pamg_fit_tentative_f64, np.float64), (capi.lib().pamg_fit_tentative_f32, np.float32)):
        Qx, R, Bt = np.full(T.nnz, -7, dtype=dtype), np.full(1, -7, dtype=dtype), B.astype(dtype)
        t0 = time.perf_counter()
        with pytest.raises(NotImplementedError):
            capi.check(fn(n, 1, 1, 1, capi.ptr(T.indptr), capi.ptr(T.indices), capi.ptr(Bt), capi.ptr(Qx), capi.ptr(R), 1e-10), "fit")
        assert np.all(Qx == -7) and np.all(R == -7) and time.perf_counter() - t0 < 0.5
    fam.check_aggregation(_core_aggregation, "star_desc")    # and the device goes on as usual
