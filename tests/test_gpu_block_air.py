"""The block (BSR) AIR setup on the device (pamg_air_block.hip) against the reference's arrays in the committed fixture
(tests/golden/kernels_block_air.npz): the block measure and block strength, block pass 2 before eliminate_zeros, local_air and the
one-point interpolation -- np.array_equal on indptr, indices and data, no tolerance (tests/block_air_cases.py) -- then a three-level
hierarchy built from this package's functions alone, and ``air_solver`` on a BSR operator under
``device_setup(air=True, classical=True, block_air=True)`` against the unpatched reference.  Every operator has at most 300 block rows."""
import numpy as np
import pytest
import scipy.sparse as sp

import block_air_cases as bc
from pyamg_amd import _capi as capi
from pyamg_amd import amg_core as gcore
from pyamg_amd import block_air
from pyamg_amd import classical as cls
from pyamg_amd.aggregation import device_setup, galerkin_product

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", sorted(bc.STRENGTH))
def test_block_measure_and_strength_are_the_references(case):
    bc.check_measure(gcore, case)
    bc.check_strength(block_air, case)


@pytest.mark.parametrize("case", sorted(bc.AIR))
def test_rows_before_eliminate_zeros_are_the_references(case):
    bc.raw_pass2(gcore, block_air, case)


@pytest.mark.parametrize("case", sorted(bc.AIR))
def test_local_air_is_the_references(case):
    bc.check_local_air(block_air, case)


@pytest.mark.parametrize("case", sorted(bc.ONEPT))
def test_one_point_interpolation_is_the_references(case):
    bc.check_one_point(block_air, case)


def test_pass2_refuses_a_shifted_row_pointer_and_writes_nothing():
    for case, shift in (("ck2.d2", (3, 1)), ("hub8x8.d1", (1, -1)), ("hub5x13.d1", (1, 1))):
        with pytest.raises(capi.PamgError) as e:
            bc.raw_pass2(gcore, block_air, case, shift=shift)          # (raw_pass2 checks that the buffers are untouched)
        assert e.value.status == capi.E_ARG


def test_use_gmres_is_refused_and_writes_nothing():
    with pytest.raises(NotImplementedError):                           # PAMG_E_UNSUPPORTED from Layer 1
        bc.raw_pass2(gcore, block_air, "ck3u.d2", use_gmres=1)
    A, splitting = bc.operator("ck2")
    with pytest.raises(NotImplementedError):
        block_air.local_air(A, splitting, use_gmres=True)


def test_what_the_device_path_does_not_take_says_so():
    A, splitting = bc.operator("ck2")
    C = bc.strength_of("ck2.min.t1")
    A9 = sp.bsr_array(np.kron(np.eye(2), np.ones((9, 9))), blocksize=(9, 9))
    Arect = sp.bsr_array(np.kron(np.eye(4), np.ones((2, 2))), blocksize=(2, 1))
    A8, _ = bc.operator("ck8")
    for call in (lambda: block_air.local_air(A.astype(np.float32), splitting),
                 lambda: block_air.one_point_interpolation(A.astype(np.float32), C, splitting),
                 lambda: block_air.classical_strength_of_connection(A.astype(np.float32)),
                 lambda: block_air.local_air(A9, np.array([1, 0], dtype=np.int32)),
                 lambda: block_air.classical_strength_of_connection(A9),
                 lambda: block_air.local_air(Arect, np.array([1, 0, 1, 0], dtype=np.int32)),
                 lambda: block_air.classical_strength_of_connection(Arect),
                 lambda: block_air.classical_strength_of_connection(A, block=False),
                 lambda: block_air.classical_strength_of_connection(A8, norm="fro"),
                 lambda: block_air.local_air(A.tocsr(), np.zeros(A.shape[0], dtype=np.int32))):
        with pytest.raises(NotImplementedError):
            call()
    Ax, out = np.ascontiguousarray(A8.data).reshape(-1), np.full(A8.indices.size, -5.0)
    with pytest.raises(NotImplementedError):                           # PAMG_E_UNSUPPORTED from Layer 1
        gcore.block_strength_measure(8, "fro", Ax, out)
    assert np.all(out == -5.0)


def test_three_level_hierarchy_without_the_reference():
    """block strength -> PMIS -> one_point_interpolation -> local_air -> galerkin_product, with air_solver's default parameters"""
    A = bc.bsr("e2e.A0", 2)
    np.random.seed(int(bc.data()["e2e.seed"][0]))
    levels = []
    for _ in range(2):
        C = block_air.classical_strength_of_connection(A, theta=0.3, norm="min")
        splitting = cls.PMIS(C)
        P = block_air.one_point_interpolation(A, C, splitting)
        R = block_air.local_air(A, splitting, theta=0.05, degree=2)
        levels.append((A, P, R))
        A = galerkin_product(R, A, P)
    levels.append((A,))
    bc.check_hierarchy(levels)


def _levels_equal(got, want):
    assert len(got.levels) == len(want.levels) >= 3
    for lg, lw in zip(got.levels, want.levels):
        for name in ("A", "P", "R"):
            if hasattr(lw, name):
                g, w = getattr(lg, name), getattr(lw, name)
                nnz = int(w.indptr[-1])                      # (the reference's P carries an uninitialised tail beyond indptr[-1])
                assert g.format == w.format and g.shape == w.shape and np.array_equal(g.indptr, w.indptr)
                assert np.array_equal(g.indices[:nnz], w.indices[:nnz]) and np.array_equal(g.data[:nnz], w.data[:nnz])
                if w.format == "bsr":
                    assert tuple(g.blocksize) == tuple(w.blocksize)


def test_air_solver_under_device_setup_reproduces_the_reference():
    import oracle.refimport as ri
    if not ri.available():
        pytest.skip("oracle/_ref not present")
    import pyamg
    A = bc.bsr("e2e.A0", 2)
    seed = int(bc.data()["e2e.seed"][0])
    np.random.seed(seed)
    want = pyamg.air_solver(A.copy(), CF="PMIS", max_coarse=10)
    follow = np.random.rand()
    calls = []
    real = block_air.local_air

    def counted(*a, **k):
        R = real(*a, **k)
        calls.append(R.format)
        return R
    block_air.local_air = counted
    try:
        np.random.seed(seed)
        with device_setup(pyamg, air=True, classical=True, block_air=True):
            got = pyamg.air_solver(A.copy(), CF="PMIS", max_coarse=10)
    finally:
        block_air.local_air = real
    assert np.random.rand() == follow                        # the patched run consumed the same random draws
    assert calls == ["bsr"] * (len(want.levels) - 1)         # the block path ran at every level, not the fall-through
    _levels_equal(got, want)
    bc.check_hierarchy([(lv.A, lv.P, lv.R) for lv in got.levels[:2]] + [(got.levels[2].A,)])
    # a CSR operator under the same keywords falls through the block functions to the CSR device path: the reference's hierarchy still
    Ac = sp.csr_array(A)
    Ac = sp.csr_array((Ac.data, Ac.indices.astype(np.int32), Ac.indptr.astype(np.int32)), shape=Ac.shape)
    np.random.seed(seed)
    want = pyamg.air_solver(Ac.copy(), CF="PMIS", max_coarse=10)
    np.random.seed(seed)
    with device_setup(pyamg, air=True, classical=True, block_air=True):
        got = pyamg.air_solver(Ac.copy(), CF="PMIS", max_coarse=10)
    assert all(lv.A.format == "csr" for lv in got.levels)
    _levels_equal(got, want)
