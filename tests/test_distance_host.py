"""Host checks of the relaxation-vector and vertex-distance strength measures (CPU, no GPU): tests/distance_emul.cpp replays
pamg_distance.hip through the arithmetic of pyamg_amd/csrc/pamg_distance.h -- lanes, groups and workgroups as loops, the block of vectors
interleaved as on the device -- and is held against every committed fixture with np.array_equal, stage by stage and as whole functions
THROUGH the Python surface (pyamg_amd.distance with its device calls replaced by the replay), so the host steps around the kernels are
checked with it.  Then the surface itself: the refusals, error parity with the reference, the random numbers a call consumes,
device_setup(distance=True), two hierarchies against the unpatched reference, and the C ABI's refusals."""
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

from pyamg_amd import distance as dist
import distance_cases as dc

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent


class EmulCore:
    """the pass-throughs of pyamg_amd.amg_core that pyamg_amd.distance calls, on the host replay"""

    def __init__(self, lib, filters):
        self.lib, self.filters = lib, filters
        self.calls = []

    @staticmethod
    def p(a):
        assert isinstance(a, np.ndarray) and a.flags.c_contiguous and a.dtype in (np.int32, np.float64)
        return a.ctypes.data_as(ctypes.c_void_p)

    @staticmethod
    def done(rc):
        if rc == 2:
            raise NotImplementedError("replay: not supported on the device path")        # what _capi.check makes of PAMG_E_UNSUPPORTED
        assert rc == 0

    def relaxation_vectors(self, Ap, Aj, Ax, X, n, R, k, omega):
        self.calls.append("relaxation_vectors")
        assert Ap.size == n + 1 and (R > 32 or X.size == n * R)
        self.done(self.lib.dse_relaxation_vectors(self.p(Ap), self.p(Aj), self.p(Ax), self.p(X), int(n), int(R), int(k), ctypes.c_double(omega)))

    def distance_measure(self, measure, Ap, Aj, Ax, X, n, R, Dx):
        self.calls.append("distance_measure")
        assert Ap.size == n + 1 and X.size == n * R and Dx.size == Ap[-1]
        self.done(self.lib.dse_distance_measure(int(measure), self.p(Ap), self.p(Aj), self.p(Ax), self.p(X), int(n), int(R), self.p(Dx)))

    def distance_strength(self, measure, Ap, Aj, Ax, X, n, R, k, omega, epsilon, Dx):
        self.calls.append("distance_strength")
        assert Ap.size == n + 1 and X.size == n * R and Dx.size == Ap[-1]
        self.done(self.lib.dse_distance_strength(int(measure), self.p(Ap), self.p(Aj), self.p(Ax), self.p(X), int(n), int(R), int(k),
                                                 ctypes.c_double(omega), ctypes.c_double(epsilon), self.p(Dx)))

    def vertex_distance(self, Ap, Aj, V, n, dim, Cx):
        self.calls.append("vertex_distance")
        assert Ap.size == n + 1 and V.size >= n * dim and Cx.size == Ap[-1]
        self.done(self.lib.dse_vertex_distance(self.p(Ap), self.p(Aj), self.p(V), int(n), int(dim), self.p(Cx)))

    def apply_distance_filter(self, n, epsilon, Sp, Sj, Sx):
        self.calls.append("apply_distance_filter")
        self.filters.eve_distance(1, int(n), ctypes.c_double(epsilon), self.p(Sp), self.p(Sj), self.p(Sx))

    def apply_absolute_distance_filter(self, n, epsilon, Sp, Sj, Sx):
        self.calls.append("apply_absolute_distance_filter")
        self.filters.eve_distance(0, int(n), ctypes.c_double(epsilon), self.p(Sp), self.p(Sj), self.p(Sx))


NAMES = ["relaxation_vectors", "distance_measure", "distance_strength", "vertex_distance", "apply_distance_filter", "apply_absolute_distance_filter"]


def _compile(name, headers):
    out = HERE / "build"
    out.mkdir(exist_ok=True)
    so, src = out / f"{name}.so", HERE / f"{name}.cpp"
    hdrs = [ROOT / "pyamg_amd" / "csrc" / h for h in headers]
    if not so.exists() or so.stat().st_mtime < max(f.stat().st_mtime for f in [src, *hdrs]):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    return ctypes.CDLL(str(so))


@pytest.fixture(scope="module")
def emul_libs():
    lib = _compile("distance_emul", ["pamg_distance.h"])
    for fn in (lib.dse_relaxation_vectors, lib.dse_distance_measure, lib.dse_distance_strength, lib.dse_vertex_distance):
        fn.restype = ctypes.c_int
    # the two filters are on the device already (pamg_evolution.hip): their replay is the evolution measure's
    return lib, _compile("evolution_emul", ["pamg_evolution.h", "pamg_jacobi_svd.h"])


@pytest.fixture()
def emul(emul_libs, monkeypatch):
    core = EmulCore(*emul_libs)
    monkeypatch.setattr(dist, "amg_core", core)
    return core


# ------------------------------------------------------------------------------------------------ the replay against the fixtures
def test_the_fixture_holds_the_cases_the_tests_name():
    d = dc.data()
    assert dc.GOLDEN.stat().st_size <= 512 * 1024
    assert len(d["case.seeds"]) == len(dc.CASES) and [str(s) for s in d["err.names"]] == [n for n, _, _ in dc.BAD]
    for k in d:
        assert d[k].dtype.kind in "iufU", k                  # data only
        if k.endswith(".indptr"):
            assert d[k].size - 1 <= 300                      # every operator has at most 300 rows
    for m in dc.MEASURES:
        mine = [c for c in dc.CASES if c[1] == m]
        assert {c[0] for c in mine} == set(dc.OPERATORS) and {c[2] for c in mine} == {1, 5, 7, 8, 9, 17, 32}
        assert {c[3] for c in mine} == {1, 2, 20} and {c[4] for c in mine} == {1.0, 2.0, 4.0} and {c[5] for c in mine} == {0.0, 0.5, 0.7}
    A = dc.operator("arrow130")
    assert A.indptr[1] > 128                                 # a row beyond two waves
    A = dc.operator("rand97")
    assert np.any(np.diff(A.indptr) == 0) and np.any((A.diagonal() == 0) & (np.diff(A.indptr) > 0)) and abs(A - A.T).max() > 0
    A = dc.operator("zeros7x5")
    assert (A.data == 0).sum() >= 4 and np.any(A.diagonal() == 0)


@pytest.mark.parametrize("i", range(len(dc.CASES)), ids=dc.IDS)
def test_relaxation_of_the_block_is_the_references(emul, i):
    A, X = dc.check_relaxation(emul, i)
    op, _, R, _, _, alpha = dc.CASES[i]
    carried = np.flatnonzero(A.diagonal() == 0)
    if carried.size and alpha:
        x0 = dc.data()[f"case.{i}.x0"].reshape(R, -1)
        assert np.array_equal(X.reshape(R, -1)[:, carried], x0[:, carried])      # no diagonal, a zero diagonal, an empty row: carried over
        assert not np.array_equal(X, dc.data()[f"case.{i}.x0"])


@pytest.mark.parametrize("i", range(len(dc.CASES)), ids=dc.IDS)
def test_measure_is_the_references(emul, i):
    A, Dx = dc.check_measure(emul, i)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    assert np.all(Dx[rows == A.indices] == 0.0) and np.all(Dx[A.data == 0.0] == 0.0)


@pytest.mark.parametrize("i", range(len(dc.CASES)), ids=dc.IDS)
def test_resident_chain_is_the_references(emul, i):
    dc.check_chain(emul, i)


@pytest.mark.parametrize("i", range(len(dc.CASES)), ids=dc.IDS)
def test_whole_function_is_the_references(emul, i):
    dc.check_whole(dist, i)
    assert emul.calls == ["distance_strength"]               # one resident call, and not by way of a fall-back


@pytest.mark.parametrize("i", [0, 12, 17])
def test_relaxation_vectors_function_is_the_references(emul, i):
    op, _, R, k, _, alpha = dc.CASES[i]
    A = dc.operator(op)
    np.random.seed(dc.seed_of(i))
    x = dist.relaxation_vectors(A, R, k, alpha)
    assert x.shape == (A.shape[0], R) and x.flags.f_contiguous and emul.calls == ["relaxation_vectors"]
    assert np.array_equal(x.T.reshape(-1), dc.data()[f"case.{i}.x"])


def test_tail_minimum_ignores_nan_and_zero_like_the_reference(emul):
    """an affinity of 0 / 0 is a NaN: it never replaces the running minimum and is never dropped; a zero distance takes no part"""
    import pyamg_amd._capi as capi
    Ap, Aj = np.array([0, 4, 5, 6, 7], dtype=np.int32), np.array([0, 1, 2, 3, 1, 2, 3], dtype=np.int32)
    Ax = np.ones(7)
    X = np.array([1.0, 0.0, 1.0, -1.0, 2.0, 0.0, 2.0, 3.0])            # R = 2, column-major: the records (1, 2), (0, 0), (1, 2), (-1, 3)
    Dx = np.full(7, -1.0)
    emul.distance_strength(capi.DISTANCE["affinity"], Ap, Aj, Ax, X, 4, 2, 0, 0.5, 2.0, Dx)
    d03 = 1.0 - (5.0 * 5.0) / (5.0 * 10.0)
    assert Dx[0] == 0.0 and np.isnan(Dx[1]) and Dx[2] == 0.0 and Dx[3] == d03 and np.all(Dx[4:] == 0.0)
    emul.distance_strength(capi.DISTANCE["affinity"], Ap, Aj, Ax, X, 4, 2, 0, 0.5, 1.0, Dx)
    assert np.isnan(Dx[1]) and Dx[3] == 0.0                  # epsilon = 1: the minimum itself is at the threshold


@pytest.mark.parametrize("name,theta,relative", dc.VERTEX)
def test_vertex_distances_are_the_references(emul, name, theta, relative):
    Cx = dc.check_vertex_entries(emul, name)
    if name.startswith("cloud3d") and Cx is not None:
        assert (Cx == 1e-6).sum() >= 92                      # the diagonals and the coincident pair: the clamp
    emul.calls.clear()
    dc.check_vertex_whole(dist, name, theta, relative)
    want = ["vertex_distance"] + ([] if theta == np.inf else ["apply_distance_filter" if relative else "apply_absolute_distance_filter"])
    assert emul.calls == want


def test_dense_operator_warns_like_the_reference(emul):
    cat, msg = (str(s) for s in dc.data()["warn.dense"])
    with pytest.warns(getattr(sp, cat)) as w:
        C = dist.distance_strength_of_connection(dc._small().toarray(), np.arange(6.0).reshape(6, 1))
    assert [str(x.message) for x in w if x.category is getattr(sp, cat)] == [msg] and C.format == "csr" and emul.calls[0] == "vertex_distance"
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # algebraic_distance converts without a word
        np.random.seed(3)
        C = dist.algebraic_distance(dc._small().toarray(), R=2, k=1)
    assert C.format == "csr"


# ------------------------------------------------------------------------------------------------ the Python surface
def _boom(*a, **k):
    raise AssertionError("a device call was made")


@pytest.fixture()
def nodevice(monkeypatch):
    monkeypatch.setattr(dist, "amg_core", types.SimpleNamespace(**{n: _boom for n in NAMES}))
    monkeypatch.setattr(np.random, "rand", _boom)            # nor is a random number drawn


def test_argument_checks_raise_the_references_errors_in_its_order(nodevice):
    d = dc.data()
    for (name, fn, kw), tname, msg in zip(dc.BAD, d["err.types"], d["err.msgs"]):
        with pytest.raises(getattr(builtins, str(tname))) as info:
            getattr(dist, fn)(dc._small(), **kw)
        assert type(info.value).__name__ == str(tname) and str(info.value) == str(msg), name


def test_reference_raises_the_same_today():
    import oracle.refimport as ri
    if not ri.available():
        pytest.skip("oracle/_ref not present")
    import pyamg.strength as rstr
    d = dc.data()
    for (name, fn, kw), tname, msg in zip(dc.BAD, d["err.types"], d["err.msgs"]):
        with pytest.raises(getattr(builtins, str(tname))) as info:
            getattr(rstr, fn)(dc._small(), **kw)
        assert str(info.value) == str(msg), name


def test_what_the_device_path_does_not_take_says_so_before_anything_is_touched(nodevice):
    A = dc.operator("poisson12x11")
    n = A.shape[0]
    V = np.random.RandomState(0).rand(n, 2)
    unsorted = sp.csr_array((A.data[::-1].copy(), A.indices[::-1].copy(), A.indptr.copy()), shape=A.shape)
    unsorted.has_canonical_format = False
    wide = sp.csr_array(A[:, :100])
    for bad in (A.astype(np.complex128), A.astype(np.float32), unsorted, wide):
        for call in (lambda: dist.algebraic_distance(bad), lambda: dist.affinity_distance(bad),
                     lambda: dist.distance_strength_of_connection(bad, V), lambda: dist.relaxation_vectors(bad, 5, 2, 0.5)):
            with pytest.raises(NotImplementedError):
                call()
    for call in (lambda: dist.algebraic_distance(A, R=33), lambda: dist.affinity_distance(A, R=33), lambda: dist.relaxation_vectors(A, 33, 2, 0.5),
                 lambda: dist.algebraic_distance(A, p=3), lambda: dist.algebraic_distance(A, p=1.5),
                 lambda: dist.distance_strength_of_connection(A, np.ones((n, 9))),
                 lambda: dist.distance_strength_of_connection(A, np.ones((n, 2), dtype=np.float32)),
                 lambda: dist.distance_strength_of_connection(A, np.ones((n, 2), dtype=np.complex128))):
        with pytest.raises(NotImplementedError):
            call()


def test_thirty_three_vectors_are_refused_by_the_kernel_entry_too(emul):
    A = dc.operator("zeros7x5")
    X = np.ones(35 * 33)
    with pytest.raises(NotImplementedError):
        emul.relaxation_vectors(A.indptr, A.indices, A.data, X, 35, 33, 1, 0.5)
    assert np.all(X == 1.0)


FUNCTIONS = ("algebraic_distance", "affinity_distance", "distance_strength_of_connection")
MODULES = ("strength", "aggregation.aggregation", "aggregation.rootnode", "classical.classical", "classical.air")
TARGETS = [(mod, fn) for mod in MODULES for fn in FUNCTIONS]


def _standin(monkeypatch):
    mods = {}
    for name in ("standin_dst", "standin_dst.strength", "standin_dst.aggregation", "standin_dst.aggregation.aggregation",
                 "standin_dst.aggregation.rootnode", "standin_dst.aggregation.adaptive", "standin_dst.classical",
                 "standin_dst.classical.classical", "standin_dst.classical.air"):
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
        setattr(mods["standin_dst." + mod], fn, reference_fn)
        originals[(mod, fn)] = reference_fn
    return mods, originals


def test_device_setup_patches_and_restores_exactly_the_fifteen_attributes(monkeypatch):
    import inspect
    from pyamg_amd import aggregation as agg
    assert inspect.signature(agg.device_setup).parameters["distance"].default is False
    assert len(TARGETS) == 15
    mods, originals = _standin(monkeypatch)
    pkg = mods["standin_dst"]
    get = lambda mod, fn: getattr(mods["standin_dst." + mod], fn)      # noqa: E731
    before = {name: dict(vars(m)) for name, m in mods.items()}
    with agg.device_setup(pkg, products=False):
        assert all(get(*t) is originals[t] for t in TARGETS)         # off by default: nothing is patched
    with agg.device_setup(pkg, products=False, distance=False):
        assert all(get(*t) is originals[t] for t in TARGETS)

    for fn in FUNCTIONS:
        def device_fn(*a, _fn=fn, **k):
            if a and a[0] == "refuse":
                raise NotImplementedError
            return ("device", _fn)
        device_fn.__name__ = fn
        monkeypatch.setattr(dist, fn, device_fn)
    with agg.device_setup(pkg, products=False, distance=True):
        changed = [(name, k) for name, m in mods.items() for k, v in vars(m).items() if before[name].get(k) is not v]
        assert sorted(changed) == sorted(("standin_dst." + mod, fn) for mod, fn in TARGETS)
        for t in TARGETS:
            patched = get(*t)
            assert patched is not originals[t] and patched.__name__ == t[1]
            assert patched("x") == ("device", t[1])
            assert patched("refuse") == ("reference",) + t                 # not on the device path: the function that was patched out
    assert all(get(*t) is originals[t] for t in TARGETS)
    assert all(dict(vars(m)) == before[name] for name, m in mods.items())
    with pytest.raises(RuntimeError):
        with agg.device_setup(pkg, products=False, distance=True):
            raise RuntimeError("inside")
    assert all(get(*t) is originals[t] for t in TARGETS)


def test_device_setup_without_distance_imports_nothing_new(tmp_path):
    """in a fresh interpreter, with a stand-in package whose submodules can all be imported: device_setup(distance=False) imports what the
    default call imports and nothing else -- nothing under <pkg>.classical, not rootnode, not pyamg_amd.distance; distance=True then
    imports exactly the modules it patches (and pyamg_amd.evolution, whose row scaling pyamg_amd.distance reuses)"""
    pkg = tmp_path / "standin_dst2"
    for sub in ("", "aggregation", "classical", "relaxation", "util"):
        (pkg / sub).mkdir(parents=True, exist_ok=True)
        (pkg / sub / "__init__.py").write_text("")
    body = "".join(f"def {fn}(*a, **k):\n    return 'reference'\n" for fn in FUNCTIONS)
    for mod in ("strength", "aggregation/aggregation", "aggregation/rootnode", "aggregation/adaptive", "aggregation/smooth",
                "classical/classical", "classical/air", "classical/interpolate", "classical/split", "relaxation/smoothing",
                "relaxation/chebyshev", "relaxation/relaxation", "util/linalg"):
        (pkg / (mod + ".py")).write_text(body)
    code = ("import sys\n"
            f"sys.path.insert(0, {str(tmp_path)!r})\n"
            "import standin_dst2 as pkg\n"
            "from pyamg_amd import aggregation as agg\n"
            "with agg.device_setup(pkg, products=False): pass\n"
            "seen = set(sys.modules)\n"
            "assert 'standin_dst2.aggregation.aggregation' in seen and 'standin_dst2.strength' in seen      # the stand-in is importable\n"
            "with agg.device_setup(pkg, products=False, distance=False): pass\n"
            "assert set(sys.modules) == seen, sorted(set(sys.modules) - seen)\n"
            "assert not [m for m in sys.modules if m.startswith('standin_dst2.classical')]\n"
            "assert 'standin_dst2.aggregation.rootnode' not in sys.modules and 'pyamg_amd.distance' not in sys.modules\n"
            "with agg.device_setup(pkg, products=False, distance=True):\n"
            "    import standin_dst2.classical.air as air\n"
            "    assert air.affinity_distance.__name__ == 'affinity_distance' and air.affinity_distance is not None\n"
            "new = set(sys.modules) - seen\n"
            "want = {'standin_dst2.aggregation.rootnode', 'standin_dst2.classical', 'standin_dst2.classical.classical',\n"
            "        'standin_dst2.classical.air', 'pyamg_amd.distance', 'pyamg_amd.evolution'}\n"
            "assert new == want, sorted(new ^ want)\n"
            "assert air.affinity_distance() == 'reference'          # restored\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(ROOT))
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


def _levels_equal(got, want):
    assert len(got.levels) == len(want.levels) >= 2
    for lg, lw in zip(got.levels, want.levels):
        for name in ("A", "P", "R", "C"):
            if hasattr(lw, name):
                g, w = sp.csr_array(getattr(lg, name)), sp.csr_array(getattr(lw, name))
                assert g.shape == w.shape and np.array_equal(g.indptr, w.indptr) and np.array_equal(g.indices, w.indices)
                assert np.array_equal(g.data, w.data)


def test_solvers_under_device_setup_with_the_replay_reproduce_the_reference(emul):
    """the patch targets in the real reference package: with the device calls on the host replay, a two-level smoothed_aggregation_solver
    with algebraic-distance strength and a two-level ruge_stuben_solver with affinity strength give the unpatched hierarchies array for array
    on the same seed.  (Two levels: SciPy's Galerkin product leaves the coarse operator without canonical format, which the device path
    hands back to the reference.)"""
    import oracle.refimport as ri
    if not ri.available():
        pytest.skip("oracle/_ref not present")
    import importlib
    import pyamg
    from pyamg_amd.aggregation import device_setup
    # what device_setup always routes to the device and this test has no device for: put back inside the block (it restores on exit)
    host_only = [(importlib.import_module(f"pyamg.{m}"), n) for m, n in (("aggregation.aggregation", "fit_candidates"),
                 ("aggregation.smooth", "approximate_spectral_radius"), ("relaxation.smoothing", "approximate_spectral_radius"),
                 ("relaxation.chebyshev", "approximate_spectral_radius"), ("util.linalg", "approximate_spectral_radius"))]
    host_only = [(m, n, getattr(m, n)) for m, n in host_only if hasattr(m, n)]
    A = dc.operator("aniso10x9")
    runs = [lambda: pyamg.smoothed_aggregation_solver(A.copy(), strength="algebraic_distance", max_levels=2, max_coarse=5),
            lambda: pyamg.ruge_stuben_solver(A.copy(), strength=("affinity", {"R": 8, "k": 3, "epsilon": 3.0}), max_levels=2, max_coarse=5,
                                             keep=True)]
    for run in runs:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            np.random.seed(11)
            want = run()
            after_want = np.random.get_state()[1].copy()
            emul.calls.clear()
            np.random.seed(11)
            with device_setup(pyamg, prolongation=False, products=False, distance=True):
                for m, n, fn in host_only:
                    setattr(m, n, fn)
                got = run()
            assert np.array_equal(np.random.get_state()[1], after_want)
            assert all(getattr(m, n) is fn for m, n, fn in host_only)
        assert emul.calls and set(emul.calls) == {"distance_strength"}      # the device path ran at every level, not the fall-back
        assert len(emul.calls) == len(want.levels) - 1
        _levels_equal(got, want)


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_c_abi_refuses_bad_arguments_before_anything_is_written():
    from pyamg_amd import _capi as capi
    lib = capi.load()
    p = capi.ptr
    A = dc.operator("zeros7x5")
    n, Ap, Aj, Ax = A.shape[0], A.indptr, A.indices, A.data
    R = 5
    X = np.full(n * R, 0.25)
    Dx = np.full(A.nnz, 7.0)
    bad_start = Ap.copy(); bad_start[0] = 1
    falling = Ap.copy(); falling[3] = falling[2] - 1
    far = Aj.copy(); far[5] = n
    RV, DM, DS, VD = lib.pamg_relaxation_vectors_f64, lib.pamg_distance_measure_f64, lib.pamg_distance_strength_f64, lib.pamg_vertex_distance_f64
    rv = lambda ap=Ap, aps=n + 1, aj=Aj, ajs=Aj.size, ax=Ax, axs=Ax.size, x=X, xs=X.size, rows=n, r=R, k=2: \
        RV(p(ap), aps, p(aj), ajs, None if ax is None else p(ax), axs, None if x is None else p(x), xs, rows, r, k, 0.5)      # noqa: E731
    ds = lambda m=1, ap=Ap, aj=Aj, xs=X.size, r=R, k=2, dx=Dx, dxs=Dx.size: \
        DS(m, p(ap), n + 1, p(aj), Aj.size, p(Ax), Ax.size, p(X), xs, n, r, k, 0.5, 2.0, None if dx is None else p(dx), dxs)      # noqa: E731
    dm = lambda m=1, ap=Ap, aj=Aj, xs=X.size, r=R, dx=Dx, dxs=Dx.size: \
        DM(m, p(ap), n + 1, p(aj), Aj.size, p(Ax), Ax.size, p(X), xs, n, r, None if dx is None else p(dx), dxs)      # noqa: E731
    for st in (rv(ap=bad_start), rv(ap=falling), rv(aps=n), rv(aj=far), rv(ajs=Aj.size - 1), rv(axs=Ax.size - 1), rv(ax=None), rv(x=None),
               rv(xs=n * R - 1), rv(rows=-1), rv(r=0), rv(k=-1),
               ds(ap=bad_start), ds(ap=falling), ds(aj=far), ds(xs=n * R - 1), ds(r=0), ds(k=-1), ds(m=4), ds(m=-1), ds(dx=None), ds(dxs=Dx.size - 1),
               dm(ap=bad_start), dm(aj=far), dm(xs=n * R - 1), dm(r=0), dm(m=7), dm(dx=None), dm(dxs=Dx.size - 1)):
        assert st == capi.E_ARG
    big = np.full(n * 33, 0.25)
    assert RV(p(Ap), n + 1, p(Aj), Aj.size, p(Ax), Ax.size, p(big), big.size, n, 33, 2, 0.5) == capi.E_UNSUPPORTED
    assert DS(1, p(Ap), n + 1, p(Aj), Aj.size, p(Ax), Ax.size, p(big), big.size, n, 33, 2, 0.5, 2.0, p(Dx), Dx.size) == capi.E_UNSUPPORTED
    assert DM(1, p(Ap), n + 1, p(Aj), Aj.size, p(Ax), Ax.size, p(big), big.size, n, 33, p(Dx), Dx.size) == capi.E_UNSUPPORTED
    V = np.full(n * 9, 0.5)
    vd = lambda ap=Ap, aj=Aj, v=V, vs=V.size, dim=2, cx=Dx, cxs=Dx.size: \
        VD(p(ap), n + 1, p(aj), Aj.size, None if v is None else p(v), vs, n, dim, None if cx is None else p(cx), cxs)      # noqa: E731
    for st in (vd(ap=bad_start), vd(ap=falling), vd(aj=far), vd(v=None), vd(vs=2 * n - 1), vd(dim=0), vd(cx=None), vd(cxs=Dx.size - 1)):
        assert st == capi.E_ARG
    assert vd(dim=9) == capi.E_UNSUPPORTED
    assert np.all(X == 0.25) and np.all(Dx == 7.0) and np.all(big == 0.25)      # nothing was written


def test_standalone_program_under_the_sanitizers(tmp_path):
    """the replay as a program of its own (its main), built with -fsanitize=address,undefined: nothing sanitized is loaded into Python"""
    exe = tmp_path / "dse"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-DDSE_MAIN", str(HERE / "distance_emul.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr.lower() + r.stdout.lower() and "cannot find" in r.stderr.lower():
        pytest.skip("no sanitizer runtime for g++ here")
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
