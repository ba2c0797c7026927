"""Host checks of energy-minimisation prolongation smoothing with GMRES (CPU, no GPU): tests/energy_gmres_emul.cpp replays
pamg_energy_gmres_f64 through the per-lane phases and the Krylov-side step functions of pyamg_amd/csrc/pamg_energy.h and is driven
THROUGH the Python surface (pyamg_amd.energy with its device call replaced by the replay).  The driver is held against the reference's
recorded T, T @ B and normr history at the project's fp64 parity bar, 1e-10 (energy_cases.BAR); then the surface: NotImplementedError
for what the device path does not take, device_setup(energy_gmres=True), the C ABI's refusals, a non-symmetric hierarchy end to end."""
import ctypes
import subprocess
import sys
import types
import warnings
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from pyamg_amd import energy as en
import energy_gmres_cases as gc

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent


class EmulCore:
    """``amg_core.energy_gmres`` on the host replay; gw = 0: the device's group width"""

    def __init__(self, lib, gw=0):
        self.lib, self.gw = lib, gw
        self.calls, self.last, self.H = [], None, None

    @staticmethod
    def p(a):
        if a is None:
            return ctypes.c_void_p(0)
        assert isinstance(a, np.ndarray) and a.flags.c_contiguous and a.dtype in (np.int32, np.float64, np.uint8)
        return a.ctypes.data_as(ctypes.c_void_p)

    def energy_gmres(self, n, nbc, r, c, K, Ap, Aj, Ax, Sp, Sj, Tx, B, BtBinv, Dinv, cmask, PIx, maxiter, tol, H=None):
        self.calls.append("energy_gmres")
        assert Tx.size == Sp[-1] * r * c and Dinv.size == n * r and B.size == nbc * c * K and (cmask is None) == (PIx is None)
        its, ns = ctypes.c_int(0), ctypes.c_int(0)
        normrs = np.zeros(maxiter + 1)
        self.H = np.zeros((maxiter + 1, maxiter + 1))
        rc = self.lib.ege_gmres(self.gw, int(n), int(nbc), int(r), int(c), int(K), *(self.p(a) for a in (Ap, Aj, Ax, Sp, Sj, Tx, B, BtBinv, Dinv, cmask, PIx)),
                                int(maxiter), ctypes.c_double(tol), ctypes.byref(its), self.p(normrs), ctypes.byref(ns), self.p(self.H))
        if rc == 2:
            raise NotImplementedError("replay: not supported on the device path")        # what _capi.check makes of PAMG_E_UNSUPPORTED
        assert rc == 0
        self.last = (int(its.value), normrs[:ns.value].copy())
        return self.last


NAMES = ["incomplete_mat_mult_bsr", "satisfy_constraints_helper", "satisfy_constraints", "energy_cg", "energy_gmres"]


def build_emul():
    out = HERE / "build"
    out.mkdir(exist_ok=True)
    so = out / "energy_gmres_emul.so"
    src = HERE / "energy_gmres_emul.cpp"
    hdr = ROOT / "pyamg_amd" / "csrc" / "pamg_energy.h"
    if not so.exists() or so.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.ege_gmres.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def emul_lib():
    return build_emul()


@pytest.fixture()
def emul(emul_lib, monkeypatch):
    core = EmulCore(emul_lib)
    monkeypatch.setattr(en, "amg_core", core)
    return core


# ------------------------------------------------------------------------------------------------ the replay against the fixture
def test_the_fixture_holds_the_cases_the_tests_name():
    d = gc.data()
    assert [str(s) for s in d["gm.names"]] == gc.GMRES
    for k in d:
        if k.endswith(".shape"):
            assert d[k][0] <= 300                            # every operator has at most 300 rows
    assert gc.GOLDEN.stat().st_size <= (HERE / "golden" / "kernels_energy.npz").stat().st_size
    kws = {n: gc.inputs(n)[5] for n in gc.GMRES}
    assert [kws[n]["maxiter"] for n in gc.GMRES] == [4, 4, 3, 4, 3, 1, 4, 3]
    assert [n for n in gc.GMRES if kws[n]["Cpt_params"][0]] == ["rn_cd", "rn_elas", "diagonal", "notol"]
    assert {n for n in gc.GMRES if kws[n]["weighting"] != "local"} == {"diagonal"}
    for n in gc.GMRES:
        normr, H, hsub, k = d[f"gm.{n}.normr"], d[f"gm.{n}.H"], d[f"gm.{n}.hsub"], gc.ITERATIONS[n]
        assert len(normr) == k + 1 == len(hsub) + 1 and H.shape == (kws[n]["maxiter"] + 1,) * 2
        # the conditions the generator asserted: far from a breakdown, a well-conditioned H
        assert all(hsub[i] >= gc.SUBDIAGONAL_FLOOR * np.sqrt(np.sum(H[:i + 1, i] ** 2)) for i in range(k))
        assert d[f"gm.{n}.cond"] <= gc.COND_CEILING and (k == 0 or np.linalg.cond(H[:k, :k]) <= gc.COND_CEILING)
    A, AR = gc.inputs("sa_cd_P")[0], gc.inputs("sa_cd_R")[0]
    assert (A != A.T).nnz and (A.T != AR).nnz == 0           # not symmetric; the second call is on A^H
    A, T, B = gc.inputs("rn_elas")[:3]
    assert A.blocksize == (2, 2) and T.blocksize == (2, 2) and B.shape[1] == 3
    n1, n2 = d["gm.sa_cd_P.normr"][1:3]
    assert n2 < kws["bigtol"]["tol"] < n1 and kws["notol"]["tol"] > d["gm.rn_cd.normr"][0]


@pytest.mark.parametrize("name", gc.GMRES)
def test_driver_agrees_with_the_reference_at_the_parity_bar(emul, name):
    """measured on the replay over the fixture: |dT| / max|T| <= 3.4e-15, |d(T B)| / max|T| <= 3.4e-16, |dnormr| / normr[0] <= 2.3e-16 --
    four orders of magnitude and more below the bar"""
    A, T, B, BtBinv, pattern, kw = gc.inputs(name)
    got = gc.run(en, name)
    its, normrs = emul.last
    dT, dTB, dN = gc.differences(name, got, normrs)
    assert dN <= gc.BAR and dT <= gc.BAR and dTB <= gc.BAR
    assert got.format == "bsr" and got.blocksize == T.blocksize and np.array_equal(got.indices, pattern.indices)
    assert its == gc.ITERATIONS[name] == len(normrs) - 1
    rooted = kw["Cpt_params"][0]
    assert gc.c_rows_are_injected(name, got) == (np.count_nonzero(kw["Cpt_params"][1]["I_F"].diagonal() == 0) if rooted else 0)
    assert emul.calls == ["energy_gmres"]
    Hw = gc.data()[f"gm.{name}.H"]                           # the rotated Hessenberg matrix, entry for entry
    assert np.abs(emul.H - Hw).max() <= gc.BAR * max(np.abs(Hw).max(), 1.0)


@pytest.mark.parametrize("gw", [1, 8, 16, 32, 64])
def test_the_group_width_does_not_move_a_bit(emul, gw):
    for name in ("rn_elas", "sa_cd_R", "diagonal"):
        emul.gw = 0
        one = gc.run(en, name)
        normr0 = emul.last[1]
        emul.gw = gw
        got = gc.run(en, name)
        assert np.array_equal(got.data, one.data) and np.array_equal(emul.last[1], normr0)          # the tree is fixed


def test_pattern_rows_in_any_stored_order(emul):
    """a pattern whose rows are not sorted: T is expanded onto it block by block and comes back on it; the row partials then run in
    another order, so the result agrees at the bar, not bit for bit"""
    A, T, B, BtBinv, pattern, kw = gc.inputs("rn_elas")
    rng = np.random.default_rng(3)
    for i in range(pattern.indptr.size - 1):
        lo, hi = pattern.indptr[i], pattern.indptr[i + 1]
        pattern.indices[lo:hi] = pattern.indices[lo:hi][rng.permutation(hi - lo)]
    pattern.has_sorted_indices = False
    got = en.gmres_prolongation_smoothing(A, T, B, BtBinv, pattern, kw["maxiter"], kw["tol"], kw["weighting"], kw["Cpt_params"])
    assert np.array_equal(got.indices, pattern.indices)
    assert max(gc.differences("rn_elas", got, emul.last[1])) <= gc.BAR and gc.c_rows_are_injected("rn_elas", got) > 0


def test_no_iteration_leaves_t_alone_on_f_rows(emul):
    A, T, B, BtBinv, pattern, kw = gc.inputs("notol")
    got = gc.run(en, "notol")
    assert emul.last[0] == 0 and len(emul.last[1]) == 1
    F = np.flatnonzero(kw["Cpt_params"][1]["I_F"].diagonal() == 1.0)
    assert 0 < F.size < A.shape[0] and np.array_equal(got.toarray()[F], T.toarray()[F])
    assert gc.c_rows_are_injected("notol", got) == A.shape[0] - F.size
    # without root nodes and without an iteration T comes back as it went in
    A, T, B, BtBinv, pattern, kw = gc.inputs("sa_cd_P")
    got = en.gmres_prolongation_smoothing(A, T, B, BtBinv, pattern, 4, 1e3)
    assert emul.last[0] == 0 and np.array_equal(got.toarray(), T.toarray())
    got = en.gmres_prolongation_smoothing(A, T, B, BtBinv, pattern, 0, 1e-8)
    assert emul.last[0] == 0 and np.array_equal(got.toarray(), T.toarray())


def test_empty_residual_returns_the_tentative_prolongator(emul, capsys):
    A, T, B, BtBinv, pattern, kw = gc.inputs("sa_cd_P")
    empty = sp.bsr_array(pattern.shape, blocksize=pattern.blocksize, dtype=np.float64)
    T0 = sp.bsr_array(T.shape, blocksize=T.blocksize, dtype=np.float64)
    assert en.gmres_prolongation_smoothing(A, T0, B, BtBinv, empty, 4, 1e-8) is T0
    assert "Initial R no nonzeros on a level" in capsys.readouterr().out and emul.calls == []


# ------------------------------------------------------------------------------------------------ the Python surface
def _boom(*a, **k):
    raise AssertionError("a device call was made")


@pytest.fixture()
def nodevice(monkeypatch):
    monkeypatch.setattr(en, "amg_core", types.SimpleNamespace(**{n: _boom for n in NAMES}))


def test_what_the_device_path_does_not_take_says_so_before_a_device_call(nodevice):
    A, T, B, BtBinv, pattern, kw = gc.inputs("rn_elas")
    gm = en.gmres_prolongation_smoothing
    big = pattern.copy()
    big.indices = big.indices.astype(np.int64)
    big.indices[-1] = 2**31 + 5
    small = sp.bsr_array((pattern.data[1:], pattern.indices[1:], np.maximum(pattern.indptr - 1, 0)), shape=pattern.shape)
    A7 = sp.bsr_array(sp.eye_array(14, format="csr"), blocksize=(7, 7))
    T7 = sp.bsr_array(np.ones((14, 7)), blocksize=(7, 7))
    not_identity = kw["Cpt_params"][1]["I_F"].copy()
    not_identity.data[0] *= 2.0
    for call in (lambda: gm(A, T, B, BtBinv, pattern, 4, 1e-8, "block", kw["Cpt_params"]),
                 lambda: gm(A, T, B, BtBinv, pattern, 33, 1e-8, "local", kw["Cpt_params"]),
                 lambda: gm(A.astype(np.float32), T, B, BtBinv, pattern, 4, 1e-8),
                 lambda: gm(A.astype(np.complex128), T, B, BtBinv, pattern, 4, 1e-8),
                 lambda: gm(A, T.astype(np.complex128), B, BtBinv, pattern, 4, 1e-8),
                 lambda: gm(A, T, B.astype(np.float32), BtBinv, pattern, 4, 1e-8),
                 lambda: gm(A, T, B, BtBinv.astype(np.complex128), pattern, 4, 1e-8),
                 lambda: gm(A.tocoo(), T, B, BtBinv, pattern, 4, 1e-8),
                 lambda: gm(A, T.toarray(), B, BtBinv, pattern, 4, 1e-8),
                 lambda: gm(A, T, B, BtBinv, pattern.tocsc(), 4, 1e-8),
                 lambda: gm(A, T, B, BtBinv, small, 4, 1e-8),                       # the pattern lost a block of T
                 lambda: gm(A, T, B, BtBinv, big, 4, 1e-8),
                 lambda: gm(A, T, B, BtBinv, pattern, 4, 1e-8, "local", (True, {"P_I": kw["Cpt_params"][1]["P_I"], "I_F": not_identity})),
                 lambda: gm(A7, T7, np.ones((7, 1)), np.ones((2, 1, 1)), T7, 4, 1e-8),
                 lambda: gm(A, T, np.ones((B.shape[0], 7)), np.ones((A.shape[0] // 2, 7, 7)), pattern, 4, 1e-8)):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(ValueError, match="weighting value is invalid"):
        gm(A, T, B, BtBinv, pattern, 4, 1e-8, "nonsense")


def test_more_than_32_iterations_are_refused_by_the_kernel_entry_too(emul):
    A, T, B, BtBinv, pattern, kw = gc.inputs("sa_cd_P")
    n = A.shape[0]
    with pytest.raises(NotImplementedError):
        emul.energy_gmres(n, T.shape[1], 1, 1, 1, A.indptr, A.indices, A.data.ravel(), pattern.indptr, pattern.indices, np.zeros(pattern.indices.size),
                          B.ravel(), BtBinv.ravel(), np.ones(n), None, None, 33, 1e-8)


CG_TARGETS = ["cg_prolongation_smoothing", "satisfy_constraints"]
GMRES_TARGETS = ["gmres_prolongation_smoothing", "satisfy_constraints"]


def test_device_setup_patches_and_restores_exactly_its_names(monkeypatch):
    import inspect
    from pyamg_amd import aggregation as agg
    assert inspect.signature(agg.device_setup).parameters["energy_gmres"].default is False
    mods = {}
    for name in ("standin_gm", "standin_gm.aggregation", "standin_gm.aggregation.smooth", "standin_gm.aggregation.aggregation"):
        m = types.ModuleType(name)
        mods[name] = m
        monkeypatch.setitem(sys.modules, name, m)
        if "." in name:
            setattr(mods[name.rsplit(".", 1)[0]], name.rsplit(".", 1)[1], m)
    smooth = mods["standin_gm.aggregation.smooth"]
    originals = {}
    for fn in ["cg_prolongation_smoothing", "gmres_prolongation_smoothing", "satisfy_constraints", "cgnr_prolongation_smoothing",
               "energy_prolongation_smoother"]:
        def reference_fn(*a, _tag=fn, **k):
            return ("reference", _tag)
        reference_fn.__name__ = fn
        setattr(smooth, fn, reference_fn)
        originals[fn] = reference_fn
    pkg = mods["standin_gm"]
    before = {name: dict(vars(m)) for name, m in mods.items()}

    def untouched():
        return all(dict(vars(m)) == before[name] for name, m in mods.items())
    for kw in ({}, {"energy_gmres": False}, {"energy": False, "energy_gmres": False}):
        with agg.device_setup(pkg, products=False, **kw):
            assert untouched()                               # off by default: <pkg>.aggregation.smooth is left alone

    def device_fn(*a, **k):
        if a and a[0] == "refuse":
            raise NotImplementedError
        return ("device",)
    for fn in set(CG_TARGETS + GMRES_TARGETS):
        monkeypatch.setattr(en, fn, device_fn)
    for kw, targets in (({"energy_gmres": True}, GMRES_TARGETS), ({"energy": True}, CG_TARGETS),
                        ({"energy": True, "energy_gmres": True}, sorted(set(CG_TARGETS + GMRES_TARGETS)))):
        with agg.device_setup(pkg, products=False, **kw):
            changed = [(name, k) for name, m in mods.items() for k, v in vars(m).items() if before[name].get(k) is not v]
            assert sorted(changed) == sorted(("standin_gm.aggregation.smooth", fn) for fn in targets)
            for fn in targets:
                patched = getattr(smooth, fn)
                assert patched is not originals[fn] and patched.__name__ == fn
                assert patched("x") == ("device",)
                assert patched("refuse") == ("reference", fn)    # not on the device path: the function that was patched out
        assert untouched()
    with pytest.raises(RuntimeError):
        with agg.device_setup(pkg, products=False, energy_gmres=True):
            raise RuntimeError("inside")
    assert untouched()


def test_device_setup_without_the_energy_keywords_does_not_import_the_module():
    code = ("import sys, types\n"
            "pkg = types.ModuleType('standin_gm2')\n"
            "sys.modules['standin_gm2'] = pkg\n"
            "from pyamg_amd import aggregation as agg\n"
            "with agg.device_setup(pkg, products=False): pass\n"
            "with agg.device_setup(pkg, products=False, energy=False, energy_gmres=False): pass\n"
            "assert 'pyamg_amd.energy' not in sys.modules\n"
            "with agg.device_setup(pkg, products=False, energy_gmres=True): pass\n"
            "assert 'pyamg_amd.energy' in sys.modules\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(ROOT))
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


def test_nonsymmetric_hierarchy_under_device_setup_with_the_replay(emul):
    """the end-to-end case of test_gpu_energy_gmres.py with the replay in place of the device and the reference's own spectral radius and
    tentative prolongator on both sides: the same level sizes, every P and R within the bar, the same random draws consumed"""
    import oracle.refimport as ri
    if not ri.available():
        pytest.skip("oracle/_ref not present")
    import importlib
    import pyamg
    from pyamg_amd.aggregation import device_setup
    host_only = [(importlib.import_module(f"pyamg.{m}"), n) for m, n in (("aggregation.aggregation", "fit_candidates"),
                 ("aggregation.smooth", "approximate_spectral_radius"), ("relaxation.smoothing", "approximate_spectral_radius"),
                 ("relaxation.chebyshev", "approximate_spectral_radius"), ("util.linalg", "approximate_spectral_radius"),
                 ("aggregation.aggregation", "symmetric_strength_of_connection"), ("strength", "symmetric_strength_of_connection"))]
    host_only = [(m, n, getattr(m, n)) for m, n in host_only if hasattr(m, n)]
    A = gc.e2e_operator()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        np.random.seed(7)
        want = gc.e2e_solver(pyamg, A.copy())
        after_want = np.random.rand()
        np.random.seed(7)
        with device_setup(pyamg, prolongation=False, products=False, energy_gmres=True):
            for m, n, fn in host_only:
                setattr(m, n, fn)
            got = gc.e2e_solver(pyamg, A.copy())
        after_got = np.random.rand()
    assert after_got == after_want                           # the same random draws were consumed
    assert emul.calls.count("energy_gmres") == 2 * (len(want.levels) - 1) and A.shape == (300, 300)          # P and R on every level
    gc.hierarchies_agree(got, want)


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_c_abi_refuses_bad_arguments_before_anything_is_written():
    from pyamg_amd import _capi as capi
    lib = capi.load()
    p = capi.ptr
    A, T, B, BtBinv, pattern, kw = gc.inputs("rn_elas")
    r, c = T.blocksize
    n, nbc, K = A.shape[0] // r, T.shape[1] // c, B.shape[1]
    Ap, Aj, Ax, Sp, Sj = A.indptr, A.indices, np.ravel(A.data), pattern.indptr, pattern.indices
    Tx = np.zeros(Sj.size * r * c)
    Bf, Zf, Dinv = np.ravel(B), np.ravel(BtBinv), np.ones(n * r)
    its, ns, normrs, H = ctypes.c_int(0), ctypes.c_int(0), np.zeros(5), np.zeros(25)
    far = Sj.copy(); far[3] = nbc
    bad_start = Sp.copy(); bad_start[0] = 1

    def gm(n_=n, r_=r, K_=K, Sp_=Sp, Sj_=Sj, Tx_size=Tx.size, B_=Bf, cmask=None, PI=None, maxiter=4, normrs_=normrs, Dinv_size=Dinv.size):
        return lib.pamg_energy_gmres_f64(n_, nbc, r_, c, K_, p(Ap), Ap.size, p(Aj), Aj.size, p(Ax), Ax.size, p(Sp_), Sp_.size, p(Sj_), Sj_.size, p(Tx),
                                         Tx_size, p(B_), Bf.size, p(Zf), Zf.size, p(Dinv), Dinv_size, p(cmask), p(PI), maxiter, 1e-8, ctypes.byref(its),
                                         p(normrs_), ctypes.byref(ns), p(H))
    assert gm(n_=-1) == capi.E_ARG and gm(Sj_=far) == capi.E_ARG and gm(Sp_=bad_start) == capi.E_ARG and gm(Tx_size=Tx.size - 1) == capi.E_ARG
    assert gm(B_=None) == capi.E_ARG and gm(maxiter=-1) == capi.E_ARG and gm(r_=0) == capi.E_ARG and gm(normrs_=None) == capi.E_ARG
    assert gm(Dinv_size=Dinv.size - 1) == capi.E_ARG
    assert gm(cmask=np.zeros(n * r, dtype=np.uint8)) == capi.E_ARG                      # a mask without the injection
    assert gm(K_=7) == capi.E_UNSUPPORTED and gm(r_=7) == capi.E_UNSUPPORTED and gm(maxiter=33) == capi.E_UNSUPPORTED
    assert not Tx.any() and not normrs.any() and not H.any() and its.value == 0 and ns.value == 0          # nothing was written


def test_standalone_program_under_the_sanitizers(tmp_path):
    """the replay as a program of its own (its main), built with -fsanitize=address,undefined: nothing sanitized is loaded into Python"""
    exe = tmp_path / "ege"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-DEGE_MAIN", str(HERE / "energy_gmres_emul.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr.lower() + r.stdout.lower() and "cannot find" in r.stderr.lower():
        pytest.skip("no sanitizer runtime for g++ here")
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
