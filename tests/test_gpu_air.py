"""The approximate ideal restriction (AIR) setup on the device (pamg_air.hip) against the reference's arrays in the committed fixture
(tests/golden/kernels_air.npz): one-point interpolation and local_air -- np.array_equal on indptr, indices and data, no tolerance
(tests/air_cases.py) -- then a three-level hierarchy built from this package's functions alone, and ``air_solver`` under
``device_setup(air=True)`` against the unpatched reference.  Every operator has at most 300 rows."""
import numpy as np
import pytest
import scipy.sparse as sp

import air_cases as ac
from pyamg_amd import _capi as capi
from pyamg_amd import air
from pyamg_amd import amg_core as gcore
from pyamg_amd import classical as cls
from pyamg_amd.aggregation import device_setup, galerkin_product

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ac.AIR)
def test_local_air_is_the_references(case):
    ac.check_local_air(air, case)


@pytest.mark.parametrize("case", ac.AIR)
def test_row_pointer_and_the_rows_before_eliminate_zeros_are_the_references(case):
    ac.raw_passes(gcore, cls, case)


@pytest.mark.parametrize("case,by_val", ac.ONEPT)
def test_one_point_interpolation_is_the_references(case, by_val):
    ac.check_one_point(air, case, by_val)


def test_pass2_refuses_a_shifted_row_pointer_and_writes_nothing():
    d = ac.data()
    for case, shift in (("convdiff13x11.d2.t0", (3, 1)), ("box6x5x4", (2, -1)), ("hub.d1", (1, 1))):
        A, splitting, theta, norm, degree = ac.air_inputs(case)
        C = cls.classical_strength_of_connection(A, theta=theta, block=False, norm=norm)
        Cpts = np.ascontiguousarray(np.where(splitting == 1)[0], dtype=np.int32)
        Rp = d[f"air.{case}.Rp"].copy()
        Rp[shift[0]] += shift[1]
        Rj, Rx = np.full(int(Rp[-1]) + 2, -5, dtype=np.int32), np.full(int(Rp[-1]) + 2, -5.0)
        with pytest.raises(capi.PamgError) as e:
            gcore.approx_ideal_restriction_pass2(Rp, Rj, Rx, A.indptr, A.indices, A.data, C.indptr, C.indices, C.data, Cpts, splitting, degree)
        assert e.value.status == capi.E_ARG and np.all(Rj == -5) and np.all(Rx == -5.0)


def test_what_the_device_path_does_not_take_says_so():
    A, splitting, theta, norm, degree = ac.air_inputs("line5")
    with pytest.raises(NotImplementedError):
        air.local_air(A, splitting, use_gmres=True)
    with pytest.raises(NotImplementedError):
        air.local_air(sp.bsr_array(A.toarray()[:4, :4], blocksize=(2, 2)), splitting[:4])
    with pytest.raises(NotImplementedError):
        air.local_air(A.astype(np.float32), splitting)
    with pytest.raises(NotImplementedError):
        air.one_point_interpolation(A.astype(np.float32), A, splitting)
    C = cls.classical_strength_of_connection(A, theta=theta, block=False, norm=norm)
    Cpts = np.ascontiguousarray(np.where(splitting == 1)[0], dtype=np.int32)
    Rp = ac.data()["air.line5.Rp"].copy()
    Rj, Rx = np.full(int(Rp[-1]), -5, dtype=np.int32), np.full(int(Rp[-1]), -5.0)
    with pytest.raises(NotImplementedError):                 # PAMG_E_UNSUPPORTED from Layer 1
        gcore.approx_ideal_restriction_pass2(Rp, Rj, Rx, A.indptr, A.indices, A.data, C.indptr, C.indices, C.data, Cpts, splitting, degree, 1)
    assert np.all(Rj == -5) and np.all(Rx == -5.0)


def test_three_level_hierarchy_without_the_reference():
    """device strength -> PMIS -> one_point_interpolation -> local_air -> galerkin_product, with air_solver's default parameters"""
    d = ac.data()
    A = ac.csr("e2e.A")
    np.random.seed(int(d["e2e.pmis.seed"]))
    levels = []
    for _ in range(2):
        C = cls.classical_strength_of_connection(A, theta=0.3, norm="min")
        splitting = cls.PMIS(C)
        P = air.one_point_interpolation(A, C, splitting)
        R = air.local_air(A, splitting, theta=0.05, degree=2)
        levels.append((A, P, R))
        A = galerkin_product(R, A, P)
    levels.append((A,))
    ac.check_hierarchy("pmis", levels)


def _levels_equal(got, want):
    assert len(got.levels) == len(want.levels) >= 3
    for lg, lw in zip(got.levels, want.levels):
        for name in ("A", "P", "R"):
            if hasattr(lw, name):
                g, w = sp.csr_array(getattr(lg, name)), sp.csr_array(getattr(lw, name))
                assert g.shape == w.shape and np.array_equal(g.indptr, w.indptr) and np.array_equal(g.indices, w.indices)
                assert np.array_equal(g.data, w.data)


@pytest.mark.parametrize("cf", ac.E2E)
def test_air_solver_under_device_setup_reproduces_the_reference(cf):
    import oracle.refimport as ri
    if not ri.available():
        pytest.skip("oracle/_ref not present")
    import pyamg
    from pyamg_amd.multilevel import DeviceMultilevelSolver
    A = ac.csr("e2e.A")
    kw = {} if cf == "rs" else {"CF": "PMIS"}
    seed = int(ac.data()[f"e2e.{cf}.seed"])
    np.random.seed(seed)
    want = pyamg.air_solver(A.copy(), max_coarse=20, **kw)
    follow = np.random.rand()
    np.random.seed(seed)
    with device_setup(pyamg, air=True):
        got = pyamg.air_solver(A.copy(), max_coarse=20, **kw)
    assert np.random.rand() == follow                        # the patched run consumed the same random draws
    _levels_equal(got, want)
    ac.check_hierarchy(cf, [(lv.A, lv.P, lv.R) for lv in got.levels[:2]] + [(got.levels[2].A,)])
    # the solve phase on either hierarchy: the same residual history
    rng = np.random.RandomState(7)
    b, x0 = rng.rand(A.shape[0]), rng.rand(A.shape[0])
    hist = []
    for ml in (got, want):
        res = []
        DeviceMultilevelSolver(ml).solve(b, x0=x0, tol=1e-30, maxiter=5, residuals=res)
        hist.append(np.array(res))
    assert hist[0].size == 6 and np.array_equal(hist[0], hist[1]) and hist[0][-1] < hist[0][0]
