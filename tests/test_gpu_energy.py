"""Energy-minimisation prolongation smoothing with CG on the device (pamg_energy.hip) against the committed fixture
(tests/golden/kernels_energy.npz, the reference's own arrays): the two amg_core calls and satisfy_constraints with np.array_equal, no
tolerance; the resident CG driver bit for bit against the host replay of the same header (the reduction tree is fixed, so this is a
condition, not a measurement) and against the reference at the fp64 parity bar; and a rootnode hierarchy end to end under
``device_setup(energy=True, evolution=True)``.  Every operator has at most 300 rows."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import energy_cases as ec
from pyamg_amd import amg_core as gcore
from pyamg_amd import energy as en
from pyamg_amd.aggregation import device_setup

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ec.IMM)
def test_incomplete_product_is_the_references(name):
    got, want = ec.run_imm(gcore, name)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", ec.SC)
def test_constraints_helper_is_the_references(name):
    got, want = ec.run_helper(gcore, name)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", ec.SC)
def test_satisfy_constraints_is_the_references(name):
    got, want = ec.run_satisfy(en, name)
    assert np.array_equal(got, want)


@pytest.fixture(scope="module")
def replay():
    """T and the newsums of every driver case from the host replay, computed once"""
    from test_energy_host import EmulCore, build_emul
    core = EmulCore(build_emul())
    out = {}
    keep = en.amg_core
    en.amg_core = core
    try:
        for name in ec.CG:
            T = ec.run_cg(en, name)
            out[name] = (T.data.copy(), core.last)
    finally:
        en.amg_core = keep
    return out


@pytest.fixture()
def spy(monkeypatch):
    """the device call of the driver, with what it returned kept"""
    seen = []
    device = gcore.energy_cg

    def energy_cg(*a, **k):
        seen.append(device(*a, **k))
        return seen[-1]
    monkeypatch.setattr(en, "amg_core", type("Core", (), {"energy_cg": staticmethod(energy_cg)}))
    return seen


@pytest.mark.parametrize("name", ec.CG)
def test_driver_is_the_replays_bit_for_bit_and_the_references_at_the_bar(replay, spy, name):
    got = ec.run_cg(en, name)
    its, sums = spy[-1]
    dT, dTB, dS = ec.cg_differences(name, got, sums)
    Tx, (its_replay, sums_replay) = replay[name]
    assert its == its_replay and np.array_equal(sums, sums_replay) and np.array_equal(got.data, Tx)
    assert dS <= ec.BAR and dT <= ec.BAR and dTB <= ec.BAR
    ec.c_rows_are_injected(name, got)


def test_rootnode_hierarchy_under_device_setup_reproduces_the_reference():
    import oracle.refimport as ri
    if not ri.available():
        pytest.skip("oracle/_ref not present")
    import pyamg
    from pyamg_amd.multilevel import DeviceMultilevelSolver
    from test_energy_host import e2e_solver
    A = sp.csr_array(ec.bsr("e2e.A"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        np.random.seed(7)
        want = e2e_solver(pyamg, A.copy())
        follow = np.random.rand()
        np.random.seed(7)
        with device_setup(pyamg, energy=True, evolution=True):
            got = e2e_solver(pyamg, A.copy())
    assert np.random.rand() == follow                        # the patched run consumed the same random draws
    assert [lv.A.shape for lv in got.levels] == [lv.A.shape for lv in want.levels] and len(want.levels) >= 3
    for lg, lw in zip(got.levels[:-1], want.levels[:-1]):
        Pg, Pw = lg.P.toarray(), lw.P.toarray()
        assert np.abs(Pg - Pw).max() / np.abs(Pw).max() <= ec.BAR
    rng = np.random.RandomState(7)
    b, x0 = rng.rand(A.shape[0]), rng.rand(A.shape[0])
    hist = []
    for ml in (got, want):
        res = []
        DeviceMultilevelSolver(ml).solve(b, x0=x0, tol=1e-30, maxiter=5, residuals=res)
        hist.append(np.array(res))
    assert hist[0].size == 6 and np.max(np.abs(hist[0] - hist[1]) / hist[1]) <= ec.BAR and hist[0][-1] < hist[0][0]
