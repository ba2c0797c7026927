"""The evolution strength of connection on the device (pamg_evolution.hip) against the reference's arrays in the committed fixture
(tests/golden/kernels_evolution.npz): every amg_core call of it and the whole function with the recorded spectral radius --
np.array_equal on indptr, indices and data, no tolerance (tests/evolution_cases.py) --, the refusals of Layer 1, the whole function with
the device Arnoldi's own spectral radius inside the band the generator certified, and two hierarchies under
``device_setup(evolution=True)`` against the unpatched reference.  Every operator has at most 300 rows."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import evolution_cases as ec
from pyamg_amd import _capi as capi
from pyamg_amd import amg_core as gcore
from pyamg_amd import evolution as evo
from pyamg_amd.aggregation import device_setup

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ec.IMM)
def test_incomplete_product_is_the_references(name):
    ec.check_imm(gcore, name)


@pytest.mark.parametrize("case,proj", ec.HELPER)
def test_helper_is_the_references(case, proj):
    ec.check_helper(gcore, case, proj)


@pytest.mark.parametrize("kind,k", ec.FILTER)
def test_distance_filters_are_the_references(kind, k):
    ec.check_filter(gcore, kind, k)


@pytest.mark.parametrize("bs", ec.MIN_BLOCKS)
def test_min_blocks_is_the_references(bs):
    ec.check_min_blocks(gcore, bs)


@pytest.mark.parametrize("name", ec.WHOLE)
def test_whole_function_with_the_recorded_rho_is_the_references(monkeypatch, name):
    d = ec.data()
    if f"whole.{name}.rho" in d:
        rho = d[f"whole.{name}.rho"][()]
        monkeypatch.setattr(evo, "approximate_spectral_radius", lambda *a, **k: rho)
    ec.check_whole(evo, name)


def test_layer_one_refuses_a_bad_row_pointer_and_writes_nothing():
    S = ec.csr("hlp.nd2.l2.S")
    d, p = ec.data(), "hlp.nd2.l2"
    n = S.shape[0]
    for bad in ("start", "falling", "short"):
        Sp = S.indptr.copy()
        if bad == "start":
            Sp[0] = 1
        elif bad == "falling":
            Sp[5] = Sp[4] - 1
        else:
            Sp[-1] += 3                                      # more entries than Sj / Sx hold
        x = S.data.copy()
        for call in (lambda: gcore.evolution_strength_helper(x, Sp, S.indices, n, d[p + ".x"].copy(), d[p + ".y"].copy(), d[p + ".b"].copy(), 3, 2, 1e-10),
                     lambda: gcore.apply_distance_filter(n, 2.0, Sp, S.indices, x),
                     lambda: gcore.apply_absolute_distance_filter(n, 2.0, Sp, S.indices, x),
                     lambda: gcore.evolution_strength_vector(x, Sp, S.indices, n, np.ones(n), np.ones(n)),
                     lambda: gcore.incomplete_mat_mult_csr(S.indptr, S.indices, S.data, S.indptr, S.indices, S.data, Sp, S.indices, x, n)):
            with pytest.raises(capi.PamgError) as e:
                call()
            assert e.value.status == capi.E_ARG and np.array_equal(x, S.data)


def test_seven_candidates_are_not_on_the_device_path():
    S = ec.csr("hlp.nd2.l2.S")
    n = S.shape[0]
    x = S.data.copy()
    with pytest.raises(NotImplementedError):                 # PAMG_E_UNSUPPORTED from Layer 1
        gcore.evolution_strength_helper(x, S.indptr, S.indices, n, np.ones(n * 7), np.ones(n * 7), np.ones(n * 28), 28, 7, 1e-10)
    assert np.array_equal(x, S.data)
    with pytest.raises(NotImplementedError):
        evo.evolution_strength_of_connection(ec.csr("whole.poisson12x11.A"), np.ones((132, 7)))


def test_the_generator_certified_enough_cases_for_the_device_rho():
    assert len(ec.certified()) >= 4 and set(ec.certified()) <= set(ec.WHOLE)


@pytest.mark.parametrize("name", ec.certified())
def test_whole_function_with_the_device_rho_stays_inside_the_references_own_band(monkeypatch, name):
    """the device Arnoldi's rho lies within d of the recorded one; the pattern is the reference's; the values differ from the reference's
    by no more than the reference's own result moves between rho (1 - d) and rho (1 + d)"""
    d, p = ec.data(), f"whole.{name}"
    seen = []
    device_rho = evo.approximate_spectral_radius

    def recording(*a, **k):
        seen.append(device_rho(*a, **k))
        return seen[-1]
    monkeypatch.setattr(evo, "approximate_spectral_radius", recording)
    np.random.seed(int(d["whole.seed"]))
    _, _, C = ec.run_whole(evo, name)
    rho_ref, band = float(d[p + ".rho"]), float(d["whole.d"])
    rel = abs(float(seen[0]) - rho_ref) / rho_ref
    ref = d[p + ".C.data"]
    bound = max(np.abs(d[p + ".plus"] - ref).max(), np.abs(d[p + ".minus"] - ref).max())
    same_pattern = np.array_equal(C.indptr, d[p + ".C.indptr"]) and np.array_equal(C.indices, d[p + ".C.indices"])
    err = np.abs(C.data - ref).max() if same_pattern else np.inf
    print(f"{name}: rho device {float(seen[0])!r} reference {rho_ref!r} relative difference {rel:.3e} (band {band:.1e}); "
          f"max |C - C_ref| {err:.3e}, the reference's own movement in the band {bound:.3e}")
    assert len(seen) == 1 and rel <= band
    assert same_pattern
    assert err <= bound


def _levels_equal(got, want):
    assert len(got.levels) == len(want.levels) >= 2
    for lg, lw in zip(got.levels, want.levels):
        for name in ("A", "P", "R"):
            if hasattr(lw, name):
                g, w = sp.csr_array(getattr(lg, name)), sp.csr_array(getattr(lw, name))
                assert g.shape == w.shape and np.array_equal(g.indptr, w.indptr) and np.array_equal(g.indices, w.indices)
                assert np.array_equal(g.data, w.data)


@pytest.mark.parametrize("solver", ["smoothed_aggregation", "rootnode"])
def test_solvers_under_device_setup_reproduce_the_reference(monkeypatch, solver):
    """the reference's own spectral radius on both sides -- in the strength measure, and in the other by-name imports device_setup routes
    to the device Arnoldi (the prolongation smoother's omega / rho): the device's value differs in the last digits, and the comparison
    is array for array"""
    import importlib
    import oracle.refimport as ri
    if not ri.available():
        pytest.skip("oracle/_ref not present")
    import pyamg
    from pyamg.util.linalg import approximate_spectral_radius as ref_rho
    monkeypatch.setattr(evo, "approximate_spectral_radius", ref_rho)
    monkeypatch.setattr(pyamg.strength, "approximate_spectral_radius", ref_rho)
    strength = ("evolution", {"k": 2, "epsilon": 3.0})
    if solver == "smoothed_aggregation":
        A = ec.csr("whole.aniso_k2.A")
        run = lambda: pyamg.smoothed_aggregation_solver(A.copy(), strength=strength, max_coarse=10)      # noqa: E731
    else:
        A, B, _ = ec.whole_inputs("elas_bsr")
        run = lambda: pyamg.rootnode_solver(A.copy(), B=B.copy(), strength=strength, max_coarse=10)      # noqa: E731
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        np.random.seed(7)
        want = run()
        np.random.seed(7)
        with device_setup(pyamg, prolongation=False, products=False, evolution=True):
            for mod in ("aggregation.smooth", "relaxation.smoothing", "util.linalg"):      # (device_setup restores them on exit)
                setattr(importlib.import_module(f"pyamg.{mod}"), "approximate_spectral_radius", ref_rho)
            calls = []
            inner = gcore.apply_distance_filter
            monkeypatch.setattr(gcore, "apply_distance_filter", lambda *a: (calls.append(1), inner(*a))[1])
            got = run()
    assert calls                                             # the device path ran, not the fall-back
    _levels_equal(got, want)
