"""Energy-minimisation prolongation smoothing with GMRES on the device (pamg_energy_gmres_f64) against the committed fixture
(tests/golden/kernels_energy_gmres.npz, the reference's own arrays): T and the normr history bit for bit against the host replay of the
same header (the reduction tree is fixed, so this is a condition, not a measurement) and against the reference at the fp64 parity bar;
and a non-symmetric smoothed-aggregation hierarchy end to end under ``device_setup(energy_gmres=True)``.  Every operator has at most
300 rows."""
import warnings

import numpy as np
import pytest

import energy_gmres_cases as gc
from pyamg_amd import amg_core as gcore
from pyamg_amd import energy as en
from pyamg_amd.aggregation import device_setup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def replay():
    """T, the normr history and H of every case from the host replay, computed once"""
    from test_energy_gmres_host import EmulCore, build_emul
    core = EmulCore(build_emul())
    out = {}
    keep = en.amg_core
    en.amg_core = core
    try:
        for name in gc.GMRES:
            T = gc.run(en, name)
            out[name] = (T.data.copy(), core.last, core.H.copy())
    finally:
        en.amg_core = keep
    return out


@pytest.fixture()
def spy(monkeypatch):
    """the device call of the driver, with what it returned and its H kept"""
    seen = []
    device = gcore.energy_gmres

    def energy_gmres(*a):
        H = np.zeros((a[16] + 1) ** 2)
        its, normrs = device(*a, H=H)
        seen.append((its, normrs, H.reshape(a[16] + 1, a[16] + 1)))
        return its, normrs
    monkeypatch.setattr(en, "amg_core", type("Core", (), {"energy_gmres": staticmethod(energy_gmres)}))
    return seen


@pytest.mark.parametrize("name", gc.GMRES)
def test_driver_is_the_replays_bit_for_bit_and_the_references_at_the_bar(replay, spy, name):
    got = gc.run(en, name)
    its, normrs, H = spy[-1]
    dT, dTB, dN = gc.differences(name, got, normrs)
    Tx, (its_replay, normrs_replay), H_replay = replay[name]
    assert its == its_replay == gc.ITERATIONS[name]
    assert np.array_equal(normrs, normrs_replay) and np.array_equal(got.data, Tx) and np.array_equal(H, H_replay)
    assert dN <= gc.BAR and dT <= gc.BAR and dTB <= gc.BAR
    kw = gc.inputs(name)[5]
    rooted = kw["Cpt_params"][0]
    assert gc.c_rows_are_injected(name, got) == (np.count_nonzero(kw["Cpt_params"][1]["I_F"].diagonal() == 0) if rooted else 0)


def test_the_pybind_face_returns_what_the_ctypes_face_returns():
    from pyamg_amd import _build
    if not _build.pybind_path().exists():
        pytest.skip("pybind11 module not built")
    from pyamg_amd import _amg_core_pybind as pcore
    A, T, B, BtBinv, pattern, kw = gc.inputs("rn_elas")
    out = []
    for core in (gcore, pcore):
        seen = []

        def energy_gmres(*a, _core=core):
            seen.append(_core.energy_gmres(*a))
            return seen[-1]
        keep = en.amg_core
        en.amg_core = type("Core", (), {"energy_gmres": staticmethod(energy_gmres)})
        try:
            got = gc.run(en, "rn_elas")
        finally:
            en.amg_core = keep
        out.append((got.data.copy(), seen[-1]))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1][0] == out[1][1][0] and np.array_equal(out[0][1][1], out[1][1][1])


def test_nonsymmetric_hierarchy_under_device_setup_reproduces_the_reference():
    import oracle.refimport as ri
    if not ri.available():
        pytest.skip("oracle/_ref not present")
    import pyamg
    from pyamg_amd.multilevel import DeviceMultilevelSolver
    A = gc.e2e_operator()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        np.random.seed(7)
        want = gc.e2e_solver(pyamg, A.copy())
        follow = np.random.rand()
        np.random.seed(7)
        with device_setup(pyamg, energy_gmres=True):
            got = gc.e2e_solver(pyamg, A.copy())
    assert np.random.rand() == follow                        # the patched run consumed the same random draws
    gc.hierarchies_agree(got, want)
    # BASELINE.md's parity protocol: b = 0 and a random x0, so that r = -A x has no cancellation and a residual history can be held
    # cycle by cycle relative to itself (with a random b the floor of that ratio, eps |A| |x| / |r_k|, rises as the cycles converge)
    b, x0 = np.zeros(A.shape[0]), np.random.RandomState(7).rand(A.shape[0])
    hist = []
    for ml in (got, want):
        res = []
        DeviceMultilevelSolver(ml).solve(b, x0=x0, tol=1e-30, maxiter=5, residuals=res)
        hist.append(np.array(res))
    worst = np.max(np.abs(hist[0] - hist[1]) / hist[1])
    print(f"[energy gmres] five V-cycles: {hist[0][0]:.3e} -> {hist[0][-1]:.3e}, against the reference hierarchy {worst:.2e}")
    assert hist[0].size == 6 and worst <= gc.BAR and np.all(np.diff(hist[0]) < 0)
