"""Host checks of the CLJP / CLJP-c coarse-grid selection and the MIS vertex colouring (CPU, no GPU): tests/cljp_emul.cpp replays
pamg_cljp.hip through the rules of pyamg_amd/csrc/pamg_cljp.h -- lanes, groups, rounds and passes as loops -- and is held against every
committed fixture with np.array_equal, THROUGH the Python surface (pyamg_amd.classical with its device calls replaced by the replay).  Then
the surface itself: argument checks and error types, NotImplementedError for what the device path does not take, and
device_setup(cljp=True)."""
import ctypes
import subprocess
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from pyamg_amd import classical as cls
import cljp_cases as jc
from test_classical_host import EmulCore as ClassicalCore

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent


class EmulCore:
    """the pass-throughs of pyamg_amd.amg_core that CLJP, CLJPc and vertex_coloring call, on the host replay; everything else from
    ``base`` (the replay of the classical setup)"""

    def __init__(self, lib, base=None):
        self.lib = lib
        self.base = base
        self.last = np.zeros(13, dtype=np.int32)             # what cje_cljp tells beyond the device's info[4]

    def __getattr__(self, name):
        if self.base is None:
            raise AttributeError(name)
        return getattr(self.base, name)

    @staticmethod
    def p(a):
        assert a.flags.c_contiguous and a.dtype == np.int32
        return a.ctypes.data_as(ctypes.c_void_p)

    def cljp_naive_splitting(self, n, Sp, Sj, Tp, Tj, splitting, colorflag, info=None):
        assert Tp is None and Tj is None                     # no host transpose
        assert self.lib.cje_cljp(int(n), self.p(Sp), self.p(Sj), int(colorflag), self.p(splitting), self.p(self.last)) == 0
        if info is not None:
            info.append(tuple(int(v) for v in self.last[:4]))

    def vertex_coloring_mis(self, n, Ap, Aj, x, info=None):
        out = np.zeros(3, dtype=np.int32)
        assert self.lib.cje_vertex_coloring_mis(int(n), self.p(Ap), self.p(Aj), self.p(x), self.p(out)) == 0
        self.last[4] = out[2]
        if info is not None:
            info.append((int(out[0]), int(out[1])))
        return int(out[0])


def _replay(stem, header):
    out = HERE / "build"
    out.mkdir(exist_ok=True)
    so = out / f"{stem}.so"
    src = HERE / f"{stem}.cpp"
    hdr = ROOT / "pyamg_amd" / "csrc" / header
    if not so.exists() or so.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    return ctypes.CDLL(str(so))


@pytest.fixture(scope="module")
def emul_lib():
    return _replay("cljp_emul", "pamg_cljp.h")


@pytest.fixture(scope="module")
def classical_lib():
    """the replay of the classical setup (strength, MIS, interpolation), for the tests that build a whole level"""
    return _replay("classical_emul", "pamg_classical.h")


@pytest.fixture()
def emul(emul_lib, monkeypatch):
    core = EmulCore(emul_lib)
    monkeypatch.setattr(cls, "amg_core", core)
    return core


# ------------------------------------------------------------------------------------------------ the replay against the fixtures
def test_this_c_library_draws_the_references_random_numbers(emul_lib):
    """CLJP's weights are srand(2448422) / rand() of the C library, as in the reference: a C library with another generator cannot
    reproduce the fixture's CLJP splittings, and this is the test that says so first"""
    got = np.zeros(16, dtype=np.int32)
    emul_lib.cje_rand_head(16, got.ctypes.data_as(ctypes.c_void_p))
    assert np.array_equal(got.astype(np.int64), jc.data()["rand.head"]), "this machine's rand() is not the generator the fixture was drawn from"


def test_the_fixture_holds_the_cases_it_was_asked_for():
    assert set(jc.names("cljp")) == {"grid17x13", "box6x5x4", "irr200", "irr200_sym", "hub", "path300", "n1", "nonsym_ties"}
    assert set(jc.names("col")) >= {"grid17x13", "box6x5x4", "irr200_sym", "path300", "n1", "irr200"}
    S = jc.pattern("grid17x13")
    assert S.shape == (221, 221) and S.diagonal().all()
    S = jc.pattern("irr200")
    rows = np.repeat(np.arange(200), np.diff(S.indptr))
    assert abs(S - S.T).nnz and not S.has_sorted_indices and np.all(np.diff(S.indptr)[:5] == 0) and np.all(S.indices[rows < 10] == rows[rows < 10])
    assert not abs(jc.pattern("irr200_sym") - jc.pattern("irr200_sym").T).nnz
    S = jc.pattern("hub")
    assert S.indptr[1] - S.indptr[0] == 100 and np.sum(S.indices[S.indptr[1]:] == 0) == 50
    S = jc.pattern("path300")
    assert S.shape == (300, 300) and S.has_sorted_indices and S.nnz == 598
    assert jc.pattern("n1").shape == (1, 1) and abs(jc.pattern("nonsym_ties") - jc.pattern("nonsym_ties").T).nnz
    for g in jc.names("cljp"):
        for k in ("cljp", "cljpc"):
            s = jc.data()[f"cljp.{g}.{k}"]
            assert set(np.unique(s)) <= {0, 1} and s.sum() >= 1
    assert jc.GOLDEN.stat().st_size <= (jc.GOLDEN.parent / "kernels_classical.npz").stat().st_size


@pytest.mark.parametrize("name,color", jc.SPLITTINGS)
def test_cljp_is_the_references(emul, name, color):
    passes, colours, rounds, selected = jc.check_cljp(cls, name, color)
    n = jc.pattern(name).shape[0]
    assert emul.last[4] <= n                                 # rounds of the deepest colour
    if name == "hub":
        assert emul.last[12] == 1 and emul.last[5] >= 1      # the row beyond the 64-lane class staged selected entries and looped
        assert emul.last[8] > 0 and emul.last[7] > 0         # 8-lane groups; P6 removed edges
    if name == "box6x5x4":
        assert emul.last[9] > 0 and emul.last[10] > 0 and emul.last[7] > 0      # 16- and 32-lane groups
    if name == "nonsym_ties" and color:
        assert emul.last[6] >= 1                             # equal colour weights: two adjacent nodes selected in one pass
    if name == "path300" and color:
        assert (colours, rounds, emul.last[4]) == (2, 301, 300)              # one decision per round along the chain, then every odd node at once
    if name == "n1":
        assert (passes, selected) == (1, 1)


def test_cljp_repeats_and_reseeds_the_c_library_as_the_reference_does(emul, emul_lib):
    libc = ctypes.CDLL(None)
    first = cls.CLJP(jc.pattern("irr200"))
    follow = libc.rand()
    assert np.array_equal(first, cls.CLJP(jc.pattern("irr200")))
    assert follow == libc.rand()                             # the stream was reseeded and advanced by n, both times
    libc.srand(2448422)
    for _ in range(200):
        libc.rand()
    assert follow == libc.rand()


@pytest.mark.parametrize("name", jc.names("col"))
def test_vertex_coloring_is_the_references(emul, name):
    colours, rounds = jc.check_coloring(cls, name)
    assert emul.last[4] <= jc.pattern(name).shape[0]
    if name == "path300":
        assert (colours, rounds) == (2, 301)


def test_vertex_coloring_takes_what_asgraph_takes(emul):
    G = jc.pattern("irr200")
    want = jc.data()["col.irr200.coloring"]
    assert np.array_equal(cls.vertex_coloring(G.tocoo()), want)
    assert np.array_equal(cls.vertex_coloring(G.toarray()), want)
    assert np.array_equal(cls.vertex_coloring(G.astype(np.float32)), want)       # only the pattern is read
    Gt = sp.csr_array(G.T)
    assert np.array_equal(cls.vertex_coloring(Gt.tocsc()), want)                 # CSC arrays are used as stored, as in the reference
    G64 = sp.csr_array((G.data, G.indices.astype(np.int64), G.indptr.astype(np.int64)), shape=G.shape)
    assert np.array_equal(cls.vertex_coloring(G64), want)
    assert np.array_equal(cls.CLJP(G64, color=True), jc.data()["cljp.irr200.cljpc"])
    assert cls.vertex_coloring(sp.csr_array((0, 0))).shape == (0,) and cls.CLJP(sp.csr_array((0, 0))).shape == (0,)


@pytest.mark.parametrize("CF", ["CLJP", "CLJPc"])
def test_first_level_of_the_hierarchy_from_this_modules_functions(emul_lib, classical_lib, monkeypatch, CF):
    monkeypatch.setattr(cls, "amg_core", EmulCore(emul_lib, ClassicalCore(classical_lib)))
    jc.check_first_level(cls, CF, lambda R, A, P: R @ A @ P)


# ------------------------------------------------------------------------------------------------ the Python surface
def _boom(*a, **k):
    raise AssertionError("a device call was made")


@pytest.fixture()
def nodevice(monkeypatch):
    monkeypatch.setattr(cls, "amg_core", types.SimpleNamespace(cljp_naive_splitting=_boom, vertex_coloring_mis=_boom))


def test_argument_checks_raise_the_references_error_types(nodevice):
    A = sp.csr_array(sp.eye_array(4, format="csr") * 2.0)
    for fn in (cls.CLJP, cls.CLJPc):
        with pytest.raises(TypeError, match="expected csr_array"):
            fn(A.tocsc())
        with pytest.raises(TypeError, match="expected csr_array"):
            fn(A.toarray())
        with pytest.raises(ValueError, match="square"):
            fn(sp.csr_array(np.ones((2, 3))))
    with pytest.raises(ValueError, match="square"):
        cls.vertex_coloring(sp.csr_array(np.ones((2, 3))))
    with pytest.raises(ValueError, match="Unknown method"):
        cls.vertex_coloring(A, "greedy")


def test_reference_raises_the_same_types():
    import oracle.refimport as ri
    if not ri.available():
        pytest.skip("oracle/_ref not present")
    from pyamg.classical import split
    from pyamg.graph import vertex_coloring as ref
    A = sp.csr_array(sp.eye_array(4, format="csr") * 2.0)
    for call, exc in ((lambda: split.CLJP(A.tocsc()), TypeError), (lambda: split.CLJPc(A.toarray()), TypeError),
                      (lambda: split.CLJP(sp.csr_array(np.ones((2, 3)))), ValueError), (lambda: split.CLJPc(sp.csr_array(np.ones((2, 3)))), ValueError),
                      (lambda: ref(sp.csr_array(np.ones((2, 3)))), ValueError), (lambda: ref(A, "greedy"), ValueError)):
        with pytest.raises(exc):
            call()


def test_what_the_device_path_does_not_take_says_so(nodevice):
    A = sp.csr_array(sp.eye_array(4, format="csr") * 2.0)
    big = sp.csr_array((np.ones(1), np.array([2 ** 31], dtype=np.int64), np.array([0, 1, 1], dtype=np.int64)), shape=(2, 2 ** 31 + 1))
    for call in (lambda: cls.vertex_coloring(A, "JP"), lambda: cls.vertex_coloring(A, "LDF"), lambda: cls.vertex_coloring(A.tobsr(blocksize=(2, 2))),
                 lambda: cls.CLJP(A.tobsr(blocksize=(2, 2))), lambda: cls.CLJPc(A.tobsr(blocksize=(2, 2))),
                 lambda: cls._pattern_only(big, "CLJP")):
        with pytest.raises(NotImplementedError):
            call()


CLJP_TARGETS = [("classical.split", "CLJP"), ("classical.split", "CLJPc"), ("classical.split", "vertex_coloring"), ("graph", "vertex_coloring")]
AIR_TARGETS = [("classical.air", "CLJP"), ("classical.air", "CLJPc")]
OTHERS = [("classical.split", "PMIS"), ("classical.split", "MIS"), ("classical.split", "PMISc"), ("classical.split", "RS"), ("classical.air", "PMIS"),
          ("classical.air", "RS"), ("graph", "maximal_independent_set"), ("classical.classical", "classical_interpolation")]


def _standin(monkeypatch):
    mods = {}
    for name in ("standin_cljp", "standin_cljp.graph", "standin_cljp.strength", "standin_cljp.classical", "standin_cljp.classical.classical",
                 "standin_cljp.classical.interpolate", "standin_cljp.classical.split", "standin_cljp.classical.air"):
        m = types.ModuleType(name)
        mods[name] = m
        monkeypatch.setitem(sys.modules, name, m)
        if "." in name:
            setattr(mods[name.rsplit(".", 1)[0]], name.rsplit(".", 1)[1], m)
    originals = {}
    for mod, fn in CLJP_TARGETS + AIR_TARGETS + OTHERS:
        def reference_fn(*a, _tag=(mod, fn), **k):
            return ("reference",) + _tag
        reference_fn.__name__ = fn
        setattr(mods["standin_cljp." + mod], fn, reference_fn)
        originals[(mod, fn)] = reference_fn
    return mods, originals


def test_device_setup_patches_and_restores_exactly_the_cljp_targets(monkeypatch):
    import inspect
    from pyamg_amd import aggregation as agg
    assert inspect.signature(agg.device_setup).parameters["cljp"].default is False
    mods, originals = _standin(monkeypatch)
    pkg = mods["standin_cljp"]
    get = lambda mod, fn: getattr(mods["standin_cljp." + mod], fn)      # noqa: E731
    untouched = lambda ts: all(get(*t) is originals[t] for t in ts)     # noqa: E731
    everything = CLJP_TARGETS + AIR_TARGETS + OTHERS
    for fn in ("CLJP", "CLJPc", "vertex_coloring", "PMIS", "MIS", "classical_interpolation"):
        def device_fn(*a, _fn=fn, **k):
            if a and a[0] == "refuse":
                raise NotImplementedError
            return ("device", _fn)
        monkeypatch.setattr(cls, fn, device_fn)
    with agg.device_setup(pkg, products=False):
        assert untouched(everything)                         # off by default
    with agg.device_setup(pkg, products=False, cljp=False, air=False):
        assert untouched(everything)
    with agg.device_setup(pkg, products=False, classical=True):
        assert untouched(CLJP_TARGETS + AIR_TARGETS)         # classical=True alone patches what it patched before
        assert get("classical.split", "PMIS")("x") == ("device", "PMIS") and get("classical.split", "MIS")("x") == ("device", "MIS")
        assert untouched([t for t in OTHERS if t[1] in ("PMISc", "RS", "maximal_independent_set") or t[0] == "classical.air"])
    with agg.device_setup(pkg, products=False, air=True):
        assert untouched(CLJP_TARGETS + AIR_TARGETS)         # air=True alone does not reach CLJP
    with agg.device_setup(pkg, products=False, cljp=True):
        for t in CLJP_TARGETS:
            patched = get(*t)
            assert patched is not originals[t] and patched.__name__ == t[1]
            assert patched("x") == ("device", t[1])
            assert patched("refuse") == ("reference",) + t   # not on the device path: the function that was patched out
        assert untouched(AIR_TARGETS + OTHERS)               # exactly its targets
    assert untouched(everything)
    with agg.device_setup(pkg, products=False, cljp=True, air=True):
        for t in CLJP_TARGETS + AIR_TARGETS:
            assert get(*t)("x") == ("device", t[1]) and get(*t)("refuse") == ("reference",) + t
        assert get("classical.air", "PMIS")("x") == ("device", "PMIS") and untouched([("classical.split", "PMIS"), ("classical.split", "RS")])
    assert untouched(everything)
    with pytest.raises(RuntimeError):
        with agg.device_setup(pkg, products=False, cljp=True):
            raise RuntimeError("inside")
    assert untouched(everything)


def test_cljp_false_imports_nothing_on_its_account(monkeypatch):
    import importlib
    from pyamg_amd import aggregation as agg
    pkg = types.ModuleType("standin_bare")
    monkeypatch.setitem(sys.modules, "standin_bare", pkg)
    asked, real = [], importlib.import_module

    def recording(name, *a, **k):
        asked.append(name)
        return real(name, *a, **k)
    monkeypatch.setattr(importlib, "import_module", recording)
    with agg.device_setup(pkg, products=False):
        pass
    assert asked and not any(".classical" in k or k.endswith(".graph") for k in asked)
    del asked[:]
    with agg.device_setup(pkg, products=False, cljp=True):
        pass
    assert sorted(k for k in asked if ".classical" in k or k.endswith(".graph")) == ["standin_bare.classical.split"] * 3 + ["standin_bare.graph"]


@pytest.mark.parametrize("CF", ["CLJP", "CLJPc"])
def test_ruge_stuben_solver_under_device_setup_with_the_replay_reproduces_the_reference(emul_lib, classical_lib, monkeypatch, CF):
    """the patch targets in the real reference package: with the device calls on the host replay (and SciPy's own sparse products),
    ruge_stuben_solver(CF='CLJP' / 'CLJPc') under device_setup(classical=True, cljp=True) gives the unpatched hierarchy, array for array"""
    import oracle.refimport as ri
    if not ri.available():
        pytest.skip("oracle/_ref not present")
    import pyamg
    from pyamg_amd.aggregation import device_setup
    core = EmulCore(emul_lib, ClassicalCore(classical_lib))
    monkeypatch.setattr(cls, "amg_core", core)
    A = jc.csr("e2e.A")
    want = pyamg.ruge_stuben_solver(A.copy(), CF=CF)
    calls = []

    def counted(*a, _fn=core.cljp_naive_splitting, **k):
        calls.append(a[6])
        return _fn(*a, **k)
    core.cljp_naive_splitting = counted
    with device_setup(pyamg, products=False, classical=True, cljp=True):
        got = pyamg.ruge_stuben_solver(A.copy(), CF=CF)
        if CF == "CLJPc":
            S = jc.pattern("irr200_sym")
            np.random.seed(7)
            a = pyamg.classical.split.PMISc(S, method="MIS")                     # its colouring and its MIS on the replay
    nl = len(want.levels)
    assert len(got.levels) == nl >= 3 and calls == [int(CF == "CLJPc")] * (nl - 1)
    jc.same_csr(sp.csr_array(got.levels[0].P), f"e2e.{CF}.P0")
    jc.same_csr(sp.csr_array(got.levels[1].A), f"e2e.{CF}.A1")
    for lg, lw in zip(got.levels, want.levels):
        for name in ("A", "P", "R"):
            if hasattr(lw, name):
                g, w = sp.csr_array(getattr(lg, name)), sp.csr_array(getattr(lw, name))
                assert g.shape == w.shape and np.array_equal(g.indptr, w.indptr) and np.array_equal(g.indices, w.indices)
                assert np.array_equal(g.data, w.data)
    if CF == "CLJPc":
        np.random.seed(7)
        assert np.array_equal(a, pyamg.classical.split.PMISc(S, method="MIS"))


def test_standalone_program_under_the_sanitizers(tmp_path):
    """the replay as a program of its own (its main), built with -fsanitize=address,undefined: nothing sanitized is loaded into Python"""
    exe = tmp_path / "cje"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-DCJE_MAIN", str(HERE / "cljp_emul.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr.lower() + r.stdout.lower() and "cannot find" in r.stderr.lower():
        pytest.skip("no sanitizer runtime for g++ here")
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
