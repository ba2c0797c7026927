"""Host checks of the evolution strength of connection (CPU, no GPU): tests/evolution_emul.cpp replays pamg_evolution.hip through the
per-row arithmetic of pyamg_amd/csrc/pamg_evolution.h -- lanes, groups and workgroups as loops -- and is held against every committed
fixture with np.array_equal, the whole-function cases THROUGH the Python surface (pyamg_amd.evolution with its device calls replaced by
the replay and its spectral radius by the recorded one), so the host steps between the kernels are checked with it.  Then the surface
itself: argument checks, error types and their order, NotImplementedError for what the device path does not take, the side effects on
the caller's objects, device_setup(evolution=True), and the C ABI's refusals."""
import builtins
import ctypes
import subprocess
import sys
import types
import warnings
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from pyamg_amd import evolution as evo
import evolution_cases as ec

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent


class EmulCore:
    """the pass-throughs of pyamg_amd.amg_core that pyamg_amd.evolution calls, on the host replay"""

    def __init__(self, lib):
        self.lib = lib
        self.calls = []

    @staticmethod
    def p(a):
        assert isinstance(a, np.ndarray) and a.flags.c_contiguous and a.dtype in (np.int32, np.float64)
        return a.ctypes.data_as(ctypes.c_void_p)

    def incomplete_mat_mult_csr(self, Ap, Aj, Ax, Bp, Bj, Bx, Sp, Sj, Sx, n):
        self.calls.append("incomplete_mat_mult_csr")
        assert Ap.size == Bp.size == Sp.size == n + 1 and Sx.size >= Sp[-1]
        self.lib.eve_imm(int(n), *(self.p(a) for a in (Ap, Aj, Ax, Bp, Bj, Bx, Sp, Sj, Sx)))

    def evolution_strength_helper(self, Sx, Sp, Sj, nrows, x, y, b, BDBCols, NullDim, tol):
        self.calls.append("evolution_strength_helper")
        assert x.size == y.size == nrows * NullDim and b.size == nrows * BDBCols and BDBCols == NullDim * (NullDim + 1) // 2
        rc = self.lib.eve_helper(self.p(Sx), self.p(Sp), self.p(Sj), int(nrows), self.p(x), self.p(y), self.p(b), int(NullDim), ctypes.c_double(tol))
        if rc == 2:
            raise NotImplementedError("replay: not supported on the device path")        # what _capi.check makes of PAMG_E_UNSUPPORTED
        assert rc == 0

    def _filter(self, relative, n, epsilon, Sp, Sj, Sx):
        self.lib.eve_distance(relative, int(n), ctypes.c_double(epsilon), self.p(Sp), self.p(Sj), self.p(Sx))

    def apply_distance_filter(self, *a):
        self.calls.append("apply_distance_filter")
        self._filter(1, *a)

    def apply_absolute_distance_filter(self, *a):
        self.calls.append("apply_absolute_distance_filter")
        self._filter(0, *a)

    def min_blocks(self, n_blocks, blocksize, Sx, Tx):
        self.calls.append("min_blocks")
        assert Sx.size == n_blocks * blocksize and Tx.size == n_blocks
        self.lib.eve_min_blocks(int(n_blocks), int(blocksize), self.p(Sx), self.p(Tx))

    def evolution_strength_vector(self, Sx, Sp, Sj, nrows, d, b):
        self.calls.append("evolution_strength_vector")
        assert d.size == b.size == nrows
        self.lib.eve_vector(self.p(Sx), self.p(Sp), self.p(Sj), int(nrows), self.p(d), self.p(b))


NAMES = [n for n in dir(EmulCore) if not n.startswith("_") and n not in ("p", "lib", "calls")]


@pytest.fixture(scope="module")
def emul_lib():
    out = HERE / "build"
    out.mkdir(exist_ok=True)
    so = out / "evolution_emul.so"
    src = HERE / "evolution_emul.cpp"
    hdrs = [ROOT / "pyamg_amd" / "csrc" / h for h in ("pamg_evolution.h", "pamg_jacobi_svd.h")]
    if not so.exists() or so.stat().st_mtime < max(f.stat().st_mtime for f in [src, *hdrs]):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.eve_helper.restype = ctypes.c_int
    return lib


@pytest.fixture()
def emul(emul_lib, monkeypatch):
    core = EmulCore(emul_lib)
    monkeypatch.setattr(evo, "amg_core", core)
    return core


def fixed_rho(monkeypatch, name):
    d = ec.data()
    if f"whole.{name}.rho" not in d:                         # the reference raised before it asked for one
        monkeypatch.setattr(evo, "approximate_spectral_radius", _boom)
        return
    rho = d[f"whole.{name}.rho"][()]                         # np.float64, the type the reference's Arnoldi returns
    monkeypatch.setattr(evo, "approximate_spectral_radius", lambda *a, **k: rho)


# ------------------------------------------------------------------------------------------------ the replay against the fixtures
def test_the_fixture_holds_the_cases_the_tests_name():
    d = ec.data()
    assert [str(s) for s in d["imm.names"]] == ec.IMM and [str(s) for s in d["whole.names"]] == ec.WHOLE
    assert sorted({c for c, _ in ec.HELPER}) == sorted(str(s) for s in d["hlp.names"])
    assert [str(s) for s in d["err.names"]] == [n for n, _ in ec.BAD]
    assert len(d["whole.certified"]) >= 4
    for k in d:
        if k.endswith(".indptr"):
            assert d[k].size - 1 <= 300                      # every operator has at most 300 rows


@pytest.mark.parametrize("name", ec.IMM)
def test_incomplete_product_is_the_references(emul, name):
    Sx = ec.check_imm(emul, name)
    if name == "rand97":
        assert (Sx == 0.0).sum() >= 5
    if name == "arrow130":
        S = ec.csr("imm.arrow130.S")
        assert S.indptr[1] > 128                             # the row of S beyond two waves: the group loops


@pytest.mark.parametrize("case,proj", ec.HELPER)
def test_helper_is_the_references(emul, case, proj):
    S, out = ec.check_helper(emul, case, proj)
    nd = int(ec.data()[f"hlp.{case}.{proj}.NullDim"])
    lengths = np.diff(S.indptr)
    if case == "craft":
        assert (lengths <= nd).sum() >= 4 and np.any(out == 1e-4) and np.any(out == 0.0)
    if case == "nd6":
        assert nd == 6 and (lengths > nd).sum() > 100 and (lengths <= nd).sum() > 0


@pytest.mark.parametrize("kind,k", ec.FILTER)
def test_distance_filters_are_the_references(emul, kind, k):
    ec.check_filter(emul, kind, k)


def test_distance_filter_minimum_ignores_nan_like_std_min(emul):
    Sp, Sj = np.array([0, 4], dtype=np.int32), np.array([0, 1, 2, 3], dtype=np.int32)
    x = np.array([5.0, np.nan, 2.0, 1.0])                   # min over the off-diagonals is 1.0: the NaN never replaces the running value
    emul.apply_distance_filter(1, 1.5, Sp, Sj, x)
    assert x[0] == 1.0 and np.isnan(x[1]) and x[2] == 0.0 and x[3] == 1.0
    x = np.array([5.0, np.nan])                             # only a NaN beside the diagonal: the minimum stays DBL_MAX, nothing is dropped
    emul.apply_distance_filter(1, 1.5, np.array([0, 2], dtype=np.int32), Sj[:2].copy(), x)
    assert x[0] == 1.0 and np.isnan(x[1])


@pytest.mark.parametrize("bs", ec.MIN_BLOCKS)
def test_min_blocks_is_the_references(emul, bs):
    ec.check_min_blocks(emul, bs)


@pytest.mark.parametrize("name", ec.WHOLE)
def test_whole_function_with_the_recorded_rho_is_the_references(emul, monkeypatch, name):
    fixed_rho(monkeypatch, name)
    ec.check_whole(evo, name)
    d = ec.data()
    if f"whole.{name}.exc" in d:
        return
    _, B, kw = ec.whole_inputs(name)
    want = {"evolution_strength_vector" if B is None or B.shape[1] == 1 else "evolution_strength_helper"}
    if kw["k"] >= 2:
        want.add("incomplete_mat_mult_csr")
    if kw["epsilon"] != np.inf:
        want.add("apply_distance_filter")
    if name.startswith("elas_bsr"):
        want.add("min_blocks")
    assert set(emul.calls) == want                           # the kernels take over wherever the reference calls amg_core


def test_side_effects_on_the_callers_operator_and_candidate(emul, monkeypatch):
    fixed_rho(monkeypatch, "bzeros")
    A, B, kw = ec.whole_inputs("bzeros")
    A2 = sp.csr_array(A.copy())
    A2.data[3] = 0.0                                         # an explicit zero in the caller's operator: gone afterwards, in place
    zeros = np.flatnonzero(B[:, 0] == 0)
    assert zeros.size > 5
    C = evo.evolution_strength_of_connection(A2, B, **kw)
    assert A2.nnz == A.nnz - 1 and A2.has_sorted_indices     # eliminate_zeros() in place
    assert np.all(B[zeros, 0] == 1.0)                        # the zeros of the caller's B are ones now, through the ravel view
    assert C.shape == A.shape


# ------------------------------------------------------------------------------------------------ the Python surface
def _boom(*a, **k):
    raise AssertionError("a device call was made")


@pytest.fixture()
def nodevice(monkeypatch):
    monkeypatch.setattr(evo, "amg_core", types.SimpleNamespace(**{n: _boom for n in NAMES}))
    monkeypatch.setattr(evo, "approximate_spectral_radius", _boom)


def test_argument_checks_raise_the_references_errors_in_its_order(nodevice):
    d = ec.data()
    for (name, make), tname, msg in zip(ec.BAD, d["err.types"], d["err.msgs"]):
        A, B, kw = make()
        with pytest.raises(getattr(builtins, str(tname))) as info:
            evo.evolution_strength_of_connection(A, B, **kw)
        assert type(info.value).__name__ == str(tname) and str(info.value) == str(msg), name


def test_reference_raises_the_same_today():
    import oracle.refimport as ri
    if not ri.available():
        pytest.skip("oracle/_ref not present")
    from pyamg.strength import evolution_strength_of_connection as ref
    d = ec.data()
    for (name, make), tname, msg in zip(ec.BAD, d["err.types"], d["err.msgs"]):
        A, B, kw = make()
        with pytest.raises(getattr(builtins, str(tname))) as info:
            ref(A, B, **kw)
        assert str(info.value) == str(msg), name


def test_what_the_device_path_does_not_take_says_so_before_anything_is_touched(nodevice):
    A = ec.csr("whole.poisson12x11.A")
    n = A.shape[0]
    unsorted = sp.csr_array((A.data[::-1].copy(), A.indices[::-1].copy(), A.indptr.copy()), shape=A.shape)
    unsorted.has_canonical_format = False
    for call in (lambda: evo.evolution_strength_of_connection(A.astype(np.complex128)),
                 lambda: evo.evolution_strength_of_connection(A.astype(np.float32)),
                 lambda: evo.evolution_strength_of_connection(A, np.ones((n, 7))),
                 lambda: evo.evolution_strength_of_connection(A, np.ones((n, 2), dtype=np.float32)),
                 lambda: evo.evolution_strength_of_connection(A, np.ones((n, 2), dtype=np.complex128)),
                 lambda: evo.evolution_strength_of_connection(sp.bsr_array(np.ones((6, 6)), blocksize=(2, 3))),
                 lambda: evo.evolution_strength_of_connection(unsorted)):
        with pytest.raises(NotImplementedError):
            call()
    B = np.zeros((n, 1), dtype=np.float32)
    with pytest.raises(NotImplementedError):
        evo.evolution_strength_of_connection(A, B)
    assert not B.any()                                       # the candidate was not touched


def test_seven_candidates_are_refused_by_the_kernel_entry_too(emul):
    S = ec.csr("hlp.nd2.l2.S")
    n = S.shape[0]
    x = S.data.copy()
    with pytest.raises(NotImplementedError):
        emul.evolution_strength_helper(x, S.indptr, S.indices, n, np.ones(n * 7), np.ones(n * 7), np.ones(n * 28), 28, 7, 1e-10)
    assert np.array_equal(x, S.data)


TARGETS = [("strength", "evolution_strength_of_connection"), ("aggregation.aggregation", "evolution_strength_of_connection"),
           ("aggregation.rootnode", "evolution_strength_of_connection"), ("aggregation.adaptive", "evolution_strength_of_connection"),
           ("classical.classical", "evolution_strength_of_connection"), ("classical.air", "evolution_strength_of_connection")]


def _standin(monkeypatch):
    mods = {}
    for name in ("standin_evo", "standin_evo.strength", "standin_evo.aggregation", "standin_evo.aggregation.aggregation",
                 "standin_evo.aggregation.rootnode", "standin_evo.aggregation.adaptive", "standin_evo.classical",
                 "standin_evo.classical.classical", "standin_evo.classical.air"):
        m = types.ModuleType(name)
        mods[name] = m
        monkeypatch.setitem(sys.modules, name, m)
        if "." in name:
            setattr(mods[name.rsplit(".", 1)[0]], name.rsplit(".", 1)[1], m)
    originals = {}
    for mod, fn in TARGETS:
        def reference_fn(*a, _tag=(mod, fn), **k):
            return ("reference",) + _tag
        reference_fn.__name__ = fn
        setattr(mods["standin_evo." + mod], fn, reference_fn)
        originals[(mod, fn)] = reference_fn
    return mods, originals


def test_device_setup_patches_and_restores_exactly_the_six_attributes(monkeypatch):
    import inspect
    from pyamg_amd import aggregation as agg
    assert inspect.signature(agg.device_setup).parameters["evolution"].default is False
    mods, originals = _standin(monkeypatch)
    pkg = mods["standin_evo"]
    get = lambda mod, fn: getattr(mods["standin_evo." + mod], fn)      # noqa: E731
    before = {name: dict(vars(m)) for name, m in mods.items()}
    with agg.device_setup(pkg, products=False):
        assert all(get(*t) is originals[t] for t in TARGETS)         # off by default: nothing is patched
    with agg.device_setup(pkg, products=False, evolution=False):
        assert all(get(*t) is originals[t] for t in TARGETS)

    def device_fn(*a, **k):
        if a and a[0] == "refuse":
            raise NotImplementedError
        return ("device",)
    monkeypatch.setattr(evo, "evolution_strength_of_connection", device_fn)
    with agg.device_setup(pkg, products=False, evolution=True):
        changed = [(name, k) for name, m in mods.items() for k, v in vars(m).items() if before[name].get(k) is not v]
        assert sorted(changed) == sorted(("standin_evo." + mod, fn) for mod, fn in TARGETS)
        for t in TARGETS:
            patched = get(*t)
            assert patched is not originals[t] and patched.__name__ == t[1]
            assert patched("x") == ("device",)
            assert patched("refuse") == ("reference",) + t                 # not on the device path: the function that was patched out
    assert all(get(*t) is originals[t] for t in TARGETS)
    assert all(dict(vars(m)) == before[name] for name, m in mods.items())
    with pytest.raises(RuntimeError):
        with agg.device_setup(pkg, products=False, evolution=True):
            raise RuntimeError("inside")
    assert all(get(*t) is originals[t] for t in TARGETS)


def test_device_setup_without_evolution_imports_nothing_new(tmp_path):
    """in a fresh interpreter, with a stand-in package whose submodules can all be imported: device_setup(evolution=False) imports what the
    default call imports and nothing else -- nothing under <pkg>.classical, neither rootnode nor adaptive, not pyamg_amd.evolution;
    evolution=True then imports exactly the modules it patches"""
    pkg = tmp_path / "standin_evo2"
    for sub in ("", "aggregation", "classical", "relaxation", "util"):
        (pkg / sub).mkdir(parents=True, exist_ok=True)
        (pkg / sub / "__init__.py").write_text("")
    body = "def evolution_strength_of_connection(*a, **k):\n    return 'reference'\n"
    for mod in ("strength", "aggregation/aggregation", "aggregation/rootnode", "aggregation/adaptive", "aggregation/smooth",
                "classical/classical", "classical/air", "classical/interpolate", "classical/split", "relaxation/smoothing",
                "relaxation/chebyshev", "relaxation/relaxation", "util/linalg"):
        (pkg / (mod + ".py")).write_text(body)
    code = ("import sys\n"
            f"sys.path.insert(0, {str(tmp_path)!r})\n"
            "import standin_evo2 as pkg\n"
            "from pyamg_amd import aggregation as agg\n"
            "with agg.device_setup(pkg, products=False): pass\n"
            "seen = set(sys.modules)\n"
            "assert 'standin_evo2.aggregation.aggregation' in seen and 'standin_evo2.strength' in seen      # the stand-in is importable\n"
            "with agg.device_setup(pkg, products=False, evolution=False): pass\n"
            "assert set(sys.modules) == seen, sorted(set(sys.modules) - seen)\n"
            "assert not [m for m in sys.modules if m.startswith('standin_evo2.classical')]\n"
            "assert 'standin_evo2.aggregation.rootnode' not in sys.modules and 'standin_evo2.aggregation.adaptive' not in sys.modules\n"
            "assert 'pyamg_amd.evolution' not in sys.modules\n"
            "with agg.device_setup(pkg, products=False, evolution=True):\n"
            "    import standin_evo2.classical.air as air\n"
            "    assert air.evolution_strength_of_connection.__name__ == 'evolution_strength_of_connection'\n"
            "new = set(sys.modules) - seen\n"
            "want = {'standin_evo2.aggregation.rootnode', 'standin_evo2.aggregation.adaptive', 'standin_evo2.classical',\n"
            "        'standin_evo2.classical.classical', 'standin_evo2.classical.air', 'pyamg_amd.evolution'}\n"
            "assert new == want, sorted(new ^ want)\n"
            "assert air.evolution_strength_of_connection() == 'reference'          # restored\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(ROOT))
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


def test_block_flag_on_a_bsr_operator_is_left_to_the_reference(nodevice):
    """the drop-in refuses before anything is touched (evolution_cases.check_whole); the patched entry then gives the reference's own
    answer -- today the exception the fixture recorded"""
    import oracle.refimport as ri
    ec.check_whole(evo, "elas_bsr_block")
    if not ri.available():
        pytest.skip("oracle/_ref not present")
    from pyamg.strength import evolution_strength_of_connection as ref
    from pyamg_amd.aggregation import _device_or_reference
    A, B, kw = ec.whole_inputs("elas_bsr_block")
    with pytest.raises(getattr(builtins, str(ec.data()["whole.elas_bsr_block.exc"]))):
        _device_or_reference(evo.evolution_strength_of_connection, ref)(A, B, **kw)


def test_solvers_under_device_setup_with_the_replay_reproduce_the_reference(emul, monkeypatch):
    """the patch targets in the real reference package: with the device calls on the host replay and the reference's own spectral radius
    on both sides, smoothed_aggregation_solver and rootnode_solver with evolution strength give the unpatched hierarchies array for array"""
    import oracle.refimport as ri
    if not ri.available():
        pytest.skip("oracle/_ref not present")
    import pyamg
    from pyamg.util.linalg import approximate_spectral_radius as ref_rho
    from pyamg_amd.aggregation import device_setup
    import importlib
    monkeypatch.setattr(evo, "approximate_spectral_radius", ref_rho)
    # what device_setup always routes to the device and this test has no device for: put back inside the block (it restores on exit)
    host_only = [(importlib.import_module(f"pyamg.{m}"), n) for m, n in (("aggregation.aggregation", "fit_candidates"),
                 ("aggregation.smooth", "approximate_spectral_radius"), ("relaxation.smoothing", "approximate_spectral_radius"),
                 ("relaxation.chebyshev", "approximate_spectral_radius"), ("util.linalg", "approximate_spectral_radius"))]
    host_only = [(m, n, getattr(m, n)) for m, n in host_only if hasattr(m, n)]
    An = ec.csr("whole.aniso_k2.A")
    Ae, Be, _ = ec.whole_inputs("elas_bsr")
    runs = [lambda: pyamg.smoothed_aggregation_solver(An.copy(), strength=("evolution", {"k": 2, "epsilon": 3.0}), max_coarse=10),
            lambda: pyamg.rootnode_solver(Ae.copy(), B=Be.copy(), strength=("evolution", {"k": 2, "epsilon": 3.0}), max_coarse=10)]
    for run in runs:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            np.random.seed(7)
            want = run()
            emul.calls.clear()
            np.random.seed(7)
            with device_setup(pyamg, prolongation=False, products=False, evolution=True):
                for m, n, fn in host_only:
                    setattr(m, n, fn)
                got = run()
            assert all(getattr(m, n) is fn for m, n, fn in host_only)
        assert len(got.levels) == len(want.levels) >= 2 and "apply_distance_filter" in emul.calls
        for lg, lw in zip(got.levels, want.levels):
            for name in ("A", "P", "R"):
                if hasattr(lw, name):
                    g, w = sp.csr_array(getattr(lg, name)), sp.csr_array(getattr(lw, name))
                    assert g.shape == w.shape and np.array_equal(g.indptr, w.indptr) and np.array_equal(g.indices, w.indices)
                    assert np.array_equal(g.data, w.data)


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_c_abi_refuses_bad_arguments_before_anything_is_written():
    from pyamg_amd import _capi as capi
    lib = capi.load()
    p = capi.ptr
    S = ec.csr("flt.S")
    n, Sp, Sj = S.shape[0], S.indptr, S.indices
    x = S.data.copy()
    keep = x.copy()
    bad_start = Sp.copy(); bad_start[0] = 1
    falling = Sp.copy(); falling[3] = falling[2] - 1
    for fn in (lib.pamg_apply_distance_filter_f64, lib.pamg_apply_absolute_distance_filter_f64):
        assert fn(n, 2.0, None, n + 1, p(Sj), Sj.size, p(x), x.size) == capi.E_ARG
        assert fn(n, 2.0, p(Sp), n + 1, None, Sj.size, p(x), x.size) == capi.E_ARG
        assert fn(n, 2.0, p(Sp), n + 1, p(Sj), Sj.size, None, x.size) == capi.E_ARG
        assert fn(-1, 2.0, p(Sp), n + 1, p(Sj), Sj.size, p(x), x.size) == capi.E_ARG
        assert fn(n, 2.0, p(Sp), n, p(Sj), Sj.size, p(x), x.size) == capi.E_ARG                  # a pointer one entry short
        assert fn(n, 2.0, p(bad_start), n + 1, p(Sj), Sj.size, p(x), x.size) == capi.E_ARG       # Sp[0] != 0
        assert fn(n, 2.0, p(falling), n + 1, p(Sj), Sj.size, p(x), x.size) == capi.E_ARG
        assert fn(n, 2.0, p(Sp), n + 1, p(Sj), Sj.size - 1, p(x), x.size) == capi.E_ARG          # fewer than Sp[n] indices
        assert fn(n, 2.0, p(Sp), n + 1, p(Sj), Sj.size, p(x), x.size - 1) == capi.E_ARG
        assert fn(n, 2.0, p(Sp), n + 1, p(Sj), -1, p(x), x.size) == capi.E_ARG
    nn = 12
    ones, cols = np.ones(nn * 28), np.ones(nn * 3)
    H = lib.pamg_evolution_strength_helper_f64
    assert H(p(x), x.size, p(Sp), n + 1, p(Sj), Sj.size, n, p(cols), cols.size, p(cols), cols.size, p(ones), ones.size, 28, 7, 1e-10) == capi.E_UNSUPPORTED
    assert H(p(x), x.size, p(Sp), n + 1, p(Sj), Sj.size, n, p(cols), cols.size, p(cols), cols.size, p(ones), ones.size, 3, 0, 1e-10) == capi.E_ARG
    assert H(p(x), x.size, p(Sp), n + 1, p(Sj), Sj.size, n, p(cols), cols.size, p(cols), cols.size, p(ones), ones.size, 2, 2, 1e-10) == capi.E_ARG   # BDBCols
    assert H(p(x), x.size, p(Sp), n + 1, p(Sj), Sj.size, n, p(cols), n * 2 - 1, p(cols), cols.size, p(ones), ones.size, 3, 2, 1e-10) == capi.E_ARG
    assert H(p(x), x.size, p(Sp), n + 1, p(Sj), Sj.size, n, None, cols.size, p(cols), cols.size, p(ones), ones.size, 3, 2, 1e-10) == capi.E_ARG
    assert H(p(x), x.size, p(bad_start), n + 1, p(Sj), Sj.size, n, p(cols), cols.size, p(cols), cols.size, p(ones), ones.size, 3, 2, 1e-10) == capi.E_ARG
    far = Sj.copy(); far[5] = n                                                                  # a column outside the matrix
    assert H(p(x), x.size, p(Sp), n + 1, p(far), Sj.size, n, p(cols), cols.size, p(cols), cols.size, p(ones), ones.size, 3, 2, 1e-10) == capi.E_ARG
    V = lib.pamg_evolution_strength_vector_f64
    d = np.ones(n)
    assert V(p(x), x.size, p(Sp), n + 1, p(Sj), Sj.size, n, p(d), n - 1, p(d), n) == capi.E_ARG
    assert V(p(x), x.size, p(Sp), n + 1, p(Sj), Sj.size, n, p(d), n, None, n) == capi.E_ARG
    assert V(p(x), x.size, p(bad_start), n + 1, p(Sj), Sj.size, n, p(d), n, p(d), n) == capi.E_ARG
    M = lib.pamg_incomplete_mat_mult_csr_f64
    args = lambda sp_=Sp, sj=Sj, sx=x, rows=n: (p(Sp), n + 1, p(Sj), Sj.size, p(keep), keep.size, p(Sp), n + 1, p(Sj), Sj.size, p(keep), keep.size,   # noqa: E731
                                                 p(sp_), n + 1, p(sj), sj.size, None if sx is None else p(sx), x.size, rows)
    assert M(*args(sp_=bad_start)) == capi.E_ARG
    assert M(*args(sj=far)) == capi.E_ARG
    assert M(*args(sx=None)) == capi.E_ARG
    assert M(*args(rows=-1)) == capi.E_ARG
    T = np.full(4, 7.0)
    B = lib.pamg_min_blocks_f64
    assert B(4, 4, p(x), 15, p(T), 4) == capi.E_ARG
    assert B(4, 4, p(x), 16, p(T), 3) == capi.E_ARG
    assert B(-1, 4, p(x), 16, p(T), 4) == capi.E_ARG
    assert B(4, 4, None, 16, p(T), 4) == capi.E_ARG
    assert np.array_equal(x, keep) and np.all(T == 7.0)      # nothing was written


def test_standalone_program_under_the_sanitizers(tmp_path):
    """the replay as a program of its own (its main), built with -fsanitize=address,undefined: nothing sanitized is loaded into Python"""
    exe = tmp_path / "eve"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-DEVE_MAIN", str(HERE / "evolution_emul.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr.lower() + r.stdout.lower() and "cannot find" in r.stderr.lower():
        pytest.skip("no sanitizer runtime for g++ here")
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
