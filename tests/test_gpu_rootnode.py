"""The root-node setup pieces of pyamg_amd.rootnode on the device, on the cases of tests/golden/kernels_rootnode.npz: what the host
replay (test_rootnode_host.py) is held to -- equality with the fixture where the summation order is the reference's, the 64 eps kappa_+
bound through the pseudo-inverse --, and the device's arrays equal to the replay's bit for bit (the reduction order is fixed, so that is
a condition, not a measurement).  Then the candidate relaxation against the fixture, and rootnode_solver end to end under
device_setup(rootnode=True, energy=True, evolution=True) against the reference where it is built beside the GPU."""
import functools
import sys
import types
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import rootnode_cases as rc
from pyamg_amd import amg_core as gcore
from pyamg_amd import rootnode as rn
from pyamg_amd.aggregation import device_setup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def replay():
    """every kernel case from the host replay, computed once: name -> arrays"""
    core = rc.EmulCore(rc.build_emul())
    out = {}
    keep = rn.amg_core
    rn.amg_core = core
    try:
        for name in rc.BTB:
            B, C, _, _ = rc.btb_inputs(name)
            out["btb." + name] = rn.compute_BtBinv(B, C)
        for name in rc.SCALE:
            T, P_I, I_F, _ = rc.scale_inputs(name)
            out["st." + name] = rn.scale_T(T, P_I, I_F)
        for name in rc.FILTER:
            A, C, B, Bf, BtBinv, _ = rc.filter_inputs(name)
            out["fo." + name] = rn.filter_operator(A, C, B, Bf, BtBinv)
    finally:
        rn.amg_core = keep
    return out


@pytest.mark.parametrize("name", rc.BTB)
def test_calc_BtB_is_the_references(name):
    got, want = rc.run_calc_BtB(gcore, name)
    assert np.array_equal(got, want)


def test_calc_BtB_through_the_pybind_face():
    from pyamg_amd import _build
    if not _build.pybind_path().exists():
        pytest.skip("pybind11 module not built")
    from pyamg_amd import _amg_core_pybind as pb
    got, want = rc.run_calc_BtB(pb, "k6")
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", rc.BTB)
def test_compute_BtBinv_is_the_replays_bit_for_bit_and_the_references_within_the_bound(replay, name):
    B, C, _, _ = rc.btb_inputs(name)
    got = rn.compute_BtBinv(B, C)
    assert np.array_equal(got, replay["btb." + name])
    rc.inverse_check(name, got)


@pytest.mark.parametrize("name", rc.SCALE)
def test_scale_T_is_the_replays_bit_for_bit_and_the_references_within_the_bound(replay, name):
    T, P_I, I_F, _ = rc.scale_inputs(name)
    got = rn.scale_T(T, P_I, I_F)
    if name == "no_coarse":
        assert got is T
    else:
        assert rc.same_matrix(got, replay["st." + name])
    rc.scale_check(name, got)


@pytest.mark.parametrize("name", rc.FILTER)
def test_filter_operator_is_the_references(replay, name):
    A, C, B, Bf, BtBinv, want = rc.filter_inputs(name)
    got = rn.filter_operator(A, C, B, Bf, BtBinv)
    assert rc.same_matrix(got, want) and rc.same_matrix(got, replay["fo." + name])


# ------------------------------------------------------------------------------------------------ candidate relaxation
@pytest.fixture()
def standin(monkeypatch):
    """a package with the reference's smoother setup for the three fixture methods (relaxation/smoothing.py:494-508, :582-608): partials of
    functions with the reference's names, the block diagonal inverted by pyamg_amd's get_block_diag (the reference's SVD bit for bit), so
    that the cases run where the reference is not built"""
    from pyamg_amd.relaxation import get_block_diag
    mods = {}
    for sub in ("", ".relaxation", ".relaxation.smoothing", ".multilevel"):
        m = types.ModuleType("standin_rx" + sub)
        mods[sub] = m
        monkeypatch.setitem(sys.modules, m.__name__, m)

    def gauss_seidel(A, x, b, iterations=1, sweep="forward"):
        raise AssertionError("the host smoother was called")

    def jacobi(A, x, b, iterations=1, omega=1.0):
        raise AssertionError("the host smoother was called")

    def block_gauss_seidel(A, x, b, iterations=1, sweep="forward", blocksize=1, Dinv=None):
        raise AssertionError("the host smoother was called")

    def setup_gauss_seidel(lvl, iterations=1, sweep="forward"):
        return functools.partial(gauss_seidel, iterations=iterations, sweep=sweep)

    def setup_jacobi(lvl, iterations=1, omega=1.0, withrho=True):
        assert not withrho
        return functools.partial(jacobi, iterations=iterations, omega=omega)

    def setup_block_gauss_seidel(lvl, iterations=1, sweep="forward", Dinv=None, blocksize=None):
        bs = lvl.A.blocksize[0]
        return functools.partial(block_gauss_seidel, iterations=iterations, Dinv=get_block_diag(lvl.A, blocksize=bs, inv_flag=True), blocksize=bs,
                                 sweep=sweep)
    S = mods[".relaxation.smoothing"]
    S.setup_gauss_seidel, S.setup_jacobi, S.setup_block_gauss_seidel = setup_gauss_seidel, setup_jacobi, setup_block_gauss_seidel
    mods[".multilevel"].MultilevelSolver = type("MultilevelSolver", (), {"Level": type("Level", (), {})})
    return mods[""]


@pytest.mark.parametrize("name", rc.RELAX)
def test_candidate_relaxation_is_the_references(standin, name):
    method, A, B, want = rc.relax_inputs(name)
    op = rn.relaxation_as_linear_operator(method, A, np.zeros((A.shape[0], 1)), pyamg=standin)
    assert op.shape == A.shape and op.dtype == np.float64
    got = op @ B
    assert got.shape == want.shape and np.array_equal(got, want)
    col = op @ B[:, 0]                                       # matvec: one column, flat and as a column
    assert col.shape == (A.shape[0],) and np.array_equal(col, want[:, 0])
    assert np.array_equal(op.matvec(B[:, :1]), want[:, :1])
    assert np.array_equal(op @ B, want)                      # the operator keeps A and relaxes from a copy every time


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("name", ["diffusion", "elasticity"])
def test_rootnode_solver_under_device_setup_reproduces_the_reference(name):
    import oracle.refimport as ri
    if not ri.available():
        pytest.skip("oracle/_ref not present")
    import pyamg
    from pyamg_amd.multilevel import DeviceMultilevelSolver
    A, B = rc.e2e_operators()[name]
    seen = []
    keep = {fn: getattr(rn, fn) for fn in ("compute_BtBinv", "scale_T", "filter_operator", "relaxation_as_linear_operator")}

    def counted(fn):
        def wrapper(*a, **k):
            out = keep[fn](*a, **k)
            seen.append(fn)                                  # (after the call: a refusal does not count)
            return out
        return wrapper
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        np.random.seed(7)
        want = rc.e2e_solver(pyamg, A.copy(), None if B is None else B.copy())
        follow = np.random.rand()
        np.random.seed(7)
        try:
            for fn in keep:
                setattr(rn, fn, counted(fn))
            with device_setup(pyamg, rootnode=True, energy=True, evolution=True):
                got = rc.e2e_solver(pyamg, A.copy(), None if B is None else B.copy())
        finally:
            for fn, f in keep.items():
                setattr(rn, fn, f)
    assert np.random.rand() == follow                        # the patched run consumed the same random draws
    levels = len(want.levels)
    assert [lv.A.shape for lv in got.levels] == [lv.A.shape for lv in want.levels] and levels >= 2
    assert seen.count("compute_BtBinv") >= levels - 1 and seen.count("scale_T") == levels - 1 and seen.count("relaxation_as_linear_operator") >= 1
    assert ("filter_operator" in seen) == (name == "elasticity")
    for lg, lw in zip(got.levels[:-1], want.levels[:-1]):
        Pg, Pw = lg.P.toarray(), lw.P.toarray()
        err = np.abs(Pg - Pw).max() / np.abs(Pw).max()
        print(f"[rootnode] {name}: level {lg.A.shape}, |P - P_ref| / max|P_ref| = {err:.2e}")
        assert err <= rc.BAR
    rng = np.random.RandomState(7)
    b, x0 = rng.rand(A.shape[0]), rng.rand(A.shape[0])
    hist = []
    for ml in (got, want):
        res = []
        DeviceMultilevelSolver(ml).solve(b, x0=x0, tol=1e-30, maxiter=5, residuals=res)
        hist.append(np.array(res))
    print(f"[rootnode] {name}: residual histories differ by {np.max(np.abs(hist[0] - hist[1]) / hist[1]):.2e} of themselves")
    assert hist[0].size == 6 and np.max(np.abs(hist[0] - hist[1]) / hist[1]) <= rc.BAR and hist[0][-1] < hist[0][0]
