"""Host checks of the classical (Ruge-Stuben) setup (CPU, no GPU): tests/classical_emul.cpp replays pamg_classical.hip through the per-row
arithmetic of pyamg_amd/csrc/pamg_classical.h -- lanes, groups and MIS rounds as loops -- and is held against every committed fixture
with np.array_equal, THROUGH the Python surface (pyamg_amd.classical with its device calls replaced by the replay), so the host steps
between the kernels (eliminate_zeros, C.multiply(A), the random draw) are checked with it.  Then the surface itself: argument checks and
error types, NotImplementedError for what the device path does not take, device_setup(classical=True)."""
import ctypes
import subprocess
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from pyamg_amd import classical as cls
import classical_cases as cc

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent


class EmulCore:
    """the pass-throughs of pyamg_amd.amg_core that pyamg_amd.classical calls, on the host replay"""

    def __init__(self, lib):
        self.lib = lib
        self.classes = np.zeros(5, dtype=np.int32)

    @staticmethod
    def p(a):
        assert a.flags.c_contiguous and a.dtype in (np.int32, np.float64)
        return a.ctypes.data_as(ctypes.c_void_p)

    def _strength(self, mn, n, theta, Ap, Aj, Ax, Sp, Sj, Sx):
        self.lib.cle_strength(mn, int(n), ctypes.c_double(theta), self.p(Ap), self.p(Aj), self.p(Ax), self.p(Sp), self.p(Sj), self.p(Sx))

    def classical_strength_of_connection_abs(self, *a):
        self._strength(0, *a)

    def classical_strength_of_connection_min(self, *a):
        self._strength(1, *a)

    def maximal_independent_set_parallel(self, n, Ap, Aj, active, C, F, x, y, max_iters=-1, rounds=None):
        assert max_iters == -1
        nr = ctypes.c_int(0)
        rc = self.lib.cle_mis(int(n), self.p(Ap), self.p(Aj), active, C, F, self.p(x), self.p(y), ctypes.byref(nr))
        if rc == 2:
            raise NotImplementedError("replay: not supported on the device path")        # what _capi.check makes of PAMG_E_UNSUPPORTED
        assert rc == 0
        if rounds is not None:
            rounds.append(nr.value)

    def pmis_splitting(self, n, Sp, Sj, rnd, splitting, rounds=None):
        nr = ctypes.c_int(0)
        assert self.lib.cle_pmis(int(n), self.p(Sp), self.p(Sj), self.p(rnd), self.p(splitting), ctypes.byref(nr)) == 0
        if rounds is not None:
            rounds.append(nr.value)

    def rs_direct_interpolation_pass1(self, n, Sp, Sj, splitting, Pp):
        self.lib.cle_interp_pass1(int(n), self.p(Sp), self.p(Sj), self.p(splitting), self.p(Pp))

    rs_classical_interpolation_pass1 = rs_direct_interpolation_pass1

    def rs_direct_interpolation_pass2(self, n, Ap, Aj, Ax, Sp, Sj, Sx, splitting, Pp, Pj, Px):
        self.lib.cle_direct_pass2(int(n), *(self.p(a) for a in (Ap, Aj, Ax, Sp, Sj, Sx, splitting, Pp, Pj, Px)))

    def remove_strong_FF_connections(self, n, Sp, Sj, Sx, splitting):
        self.lib.cle_remove_ff(int(n), self.p(Sp), self.p(Sj), self.p(Sx), self.p(splitting))

    def rs_classical_interpolation_pass2(self, n, Ap, Aj, Ax, Sp, Sj, Sx, splitting, Pp, Pj, Px, modified):
        self.lib.cle_classical_pass2(int(n), *(self.p(a) for a in (Ap, Aj, Ax, Sp, Sj, Sx, splitting, Pp, Pj, Px)), int(bool(modified)),
                                     self.p(self.classes))


@pytest.fixture(scope="module")
def emul_lib():
    out = HERE / "build"
    out.mkdir(exist_ok=True)
    so = out / "classical_emul.so"
    src = HERE / "classical_emul.cpp"
    hdr = ROOT / "pyamg_amd" / "csrc" / "pamg_classical.h"
    if not so.exists() or so.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    return ctypes.CDLL(str(so))


@pytest.fixture()
def emul(emul_lib, monkeypatch):
    core = EmulCore(emul_lib)
    monkeypatch.setattr(cls, "amg_core", core)
    return core


# ------------------------------------------------------------------------------------------------ the replay against the fixtures
@pytest.mark.parametrize("op,norm,k", cc.STRENGTH)
def test_strength_is_the_references(emul, op, norm, k):
    cc.check_strength(cls, op, norm, k)


def test_strength_cases_reach_their_paths():
    A = cc.csr("str.odd150.A")
    offd = np.array([np.sum(A.indices[a:b] != i) for i, (a, b) in enumerate(zip(A.indptr[:-1], A.indptr[1:]))])
    hasd = np.array([np.any(A.indices[a:b] == i) for i, (a, b) in enumerate(zip(A.indptr[:-1], A.indptr[1:]))])
    assert A.shape[0] == 150 and A.shape[0] % 64 and offd.max() > 64 and (offd == 0).sum() >= 5 and (~hasd).sum() >= 5
    assert (A.data == 0).sum() >= 5 and (A.data[A.indices != np.repeat(np.arange(150), np.diff(A.indptr))] > 0).sum() > 20
    assert not A.has_sorted_indices
    assert cc.csr("str.odd150.min.1").nnz < cc.csr("str.odd150.abs.1").nnz < A.nnz       # zeros dropped, the norms differ


@pytest.mark.parametrize("name", cc.names("mis"))
def test_mis_is_the_references(emul, name):
    rounds = cc.check_mis(cls, name)
    if name == "path300":
        assert rounds == 300                                 # one decision per round, and never more than n rounds


@pytest.mark.parametrize("name", cc.names("pmis"))
def test_pmis_is_the_references_on_the_same_random_stream(emul, name):
    s = cc.check_pmis(cls, name)
    assert np.array_equal(s, cc.check_pmis(cls, name))
    if name == "irr200":
        assert not s[:10].any()                              # no neighbour in S union S^T: fine


@pytest.mark.parametrize("case,kind", cc.INTERP)
def test_interpolation_is_the_references(emul, case, kind):
    cc.check_interp(cls, case, kind)
    if (case, kind) == ("hub", "mod"):
        assert emul.classes[4] == 1 and emul.classes[0] > 0  # the row beyond the 64-lane class
    if (case, kind) == ("box6x5x4", "mod"):
        assert emul.classes[1] > 0 and emul.classes[2] > 0   # 16- and 32-lane groups


def test_interpolation_cases_reach_their_paths(emul):
    d = cc.data()
    assert {(c, k) for c, k in cc.INTERP} >= {(c, k) for c in cc.names("int") for k in ("direct", "mod")} | {("sparseC", "unmod")}
    # convdiff: strong positive couplings to C-points -> direct interpolation's beta branch
    A, C, s = cc.csr("int.convdiff.A"), cc.csr("int.convdiff.C"), d["int.convdiff.splitting"]
    CA = C.multiply(A).tocoo()
    assert np.any((CA.data > 0) & (s[CA.col] == 1) & (s[CA.row] == 0) & (CA.row != CA.col))
    # sparseC: remove_strong_FF_connections zeroes entries, and some F-rows have no strong C-neighbour
    C, s = cc.csr("int.sparseC.C"), d["int.sparseC.splitting"].copy()
    x = C.data.copy()
    emul.remove_strong_FF_connections(64, C.indptr, C.indices, x, s)
    assert 0 < (x == 0).sum() < x.size
    P = cc.csr("int.sparseC.mod", shape=(64, int(d["int.sparseC.mod.nc"])))
    assert np.any((np.diff(P.indptr) == 0) & (s == 0))
    # level1: unsorted rows
    A1 = cc.csr("int.level1.A")
    assert any(np.any(np.diff(A1.indices[a:b]) < 0) for a, b in zip(A1.indptr[:-1], A1.indptr[1:]))
    for c, k in cc.INTERP:
        assert np.all(np.isfinite(d[f"int.{c}.{k}.data"]))


def test_first_level_of_the_hierarchy_from_this_modules_functions(emul):
    """strength -> PMIS -> classical interpolation of the 17 x 13 grid on the seed of the fixture: the reference's first prolongator"""
    d = cc.data()
    A = cc.csr("e2e.A")
    np.random.seed(int(d["e2e.seed"]))
    C = cls.classical_strength_of_connection(A, theta=0.25)
    splitting = cls.PMIS(C)
    P = cls.classical_interpolation(A, C, splitting)
    cc.same_csr(P, "e2e.P0")
    assert P.shape[1] == int(d["e2e.P0.nc"])


# ------------------------------------------------------------------------------------------------ the Python surface
def _boom(*a, **k):
    raise AssertionError("a device call was made")


@pytest.fixture()
def nodevice(monkeypatch):
    core = types.SimpleNamespace(**{n: _boom for n in dir(EmulCore) if not n.startswith("_") and n != "p"})
    monkeypatch.setattr(cls, "amg_core", core)


def test_argument_checks_raise_the_references_error_types(nodevice):
    A = sp.csr_array(sp.eye_array(4, format="csr") * 2.0)
    s = np.array([1, 0, 1, 0], dtype=np.int32)
    for theta in (-0.1, 1.5):
        with pytest.raises(ValueError, match="theta"):
            cls.classical_strength_of_connection(A, theta=theta)
    with pytest.raises(ValueError, match="norm"):
        cls.classical_strength_of_connection(A, norm="max")
    B = sp.bsr_array(np.ones((4, 6)), blocksize=(2, 3))
    with pytest.raises(ValueError, match="square blocks"):
        cls.classical_strength_of_connection(B)
    for fn in (cls.MIS, cls.PMIS):
        args = (np.ones(4),) if fn is cls.MIS else ()
        with pytest.raises(TypeError, match="expected csr_array"):
            fn(A.tocsc(), *args)
        with pytest.raises(ValueError, match="square"):
            fn(sp.csr_array(np.ones((2, 3))), *args)
    with pytest.raises(ValueError, match="maxiter"):
        cls.MIS(A, np.ones(4), maxiter=-1)
    with pytest.raises(TypeError, match="for A"):
        cls.direct_interpolation(A.tocsc(), A, s)
    with pytest.raises(TypeError, match="for C"):
        cls.direct_interpolation(A, A.tocsc(), s)
    with pytest.raises(TypeError, match="for A"):
        cls.classical_interpolation(A.toarray(), A, s)
    with pytest.raises(TypeError, match="SOC matrix"):
        cls.classical_interpolation(A, A.tobsr(), s)


def test_reference_raises_the_same_types():
    import oracle.refimport as ri
    if not ri.available():
        pytest.skip("oracle/_ref not present")
    from pyamg.classical import interpolate, split
    from pyamg.strength import classical_strength_of_connection as ref
    A = sp.csr_array(sp.eye_array(4, format="csr") * 2.0)
    s = np.array([1, 0, 1, 0], dtype=np.int32)
    for call, exc in ((lambda: ref(A, theta=1.5), ValueError), (lambda: ref(A, norm="max"), ValueError),
                      (lambda: split.MIS(A.tocsc(), np.ones(4)), TypeError), (lambda: split.PMIS(sp.csr_array(np.ones((2, 3)))), ValueError),
                      (lambda: split.MIS(A, np.ones(4), maxiter=-1), ValueError),
                      (lambda: interpolate.direct_interpolation(A, A.tocsc(), s), TypeError),
                      (lambda: interpolate.classical_interpolation(A, A.tobsr(), s), TypeError)):
        with pytest.raises(exc):
            call()


def test_what_the_device_path_does_not_take_says_so(nodevice):
    A = sp.csr_array(sp.eye_array(4, format="csr") * 2.0)
    s = np.array([1, 0, 1, 0], dtype=np.int32)
    for call in (lambda: cls.classical_strength_of_connection(A.tobsr(blocksize=(2, 2))),
                 lambda: cls.classical_strength_of_connection(A.astype(np.float32)),
                 lambda: cls.classical_strength_of_connection(A.astype(np.complex128)),
                 lambda: cls.classical_strength_of_connection(A, norm="fro"),
                 lambda: cls.classical_strength_of_connection(A.toarray()),
                 lambda: cls.MIS(A, np.ones(4), maxiter=3),
                 lambda: cls.direct_interpolation(A.astype(np.float32), A, s),
                 lambda: cls.classical_interpolation(A.astype(np.float32), A, s),
                 lambda: cls.classical_interpolation(A, A.astype(np.float32), s)):
        with pytest.raises(NotImplementedError):
            call()


def test_a_non_symmetric_graph_is_refused_by_mis(emul):
    G = sp.csr_array(np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]]))
    with pytest.raises(NotImplementedError, match="symmetric"):
        cls.MIS(G, np.ones(3))


TARGETS = [("strength", "classical_strength_of_connection"), ("classical.classical", "classical_strength_of_connection"),
           ("classical.interpolate", "classical_strength_of_connection"), ("classical.classical", "direct_interpolation"),
           ("classical.interpolate", "direct_interpolation"), ("classical.classical", "classical_interpolation"),
           ("classical.interpolate", "classical_interpolation"), ("classical.split", "PMIS"), ("classical.split", "MIS")]


def _standin(monkeypatch):
    mods = {}
    for name in ("standin_rs", "standin_rs.strength", "standin_rs.classical", "standin_rs.classical.classical",
                 "standin_rs.classical.interpolate", "standin_rs.classical.split"):
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
        setattr(mods["standin_rs." + mod], fn, reference_fn)
        originals[(mod, fn)] = reference_fn
    return mods, originals


def test_device_setup_patches_and_restores_every_classical_target(monkeypatch):
    import inspect
    from pyamg_amd import aggregation as agg
    assert inspect.signature(agg.device_setup).parameters["classical"].default is False
    mods, originals = _standin(monkeypatch)
    pkg = mods["standin_rs"]
    get = lambda mod, fn: getattr(mods["standin_rs." + mod], fn)      # noqa: E731
    with agg.device_setup(pkg, products=False):
        assert all(get(*t) is originals[t] for t in TARGETS)         # off by default: nothing is patched
    with agg.device_setup(pkg, products=False, classical=False):
        assert all(get(*t) is originals[t] for t in TARGETS)
    for fn in ("classical_strength_of_connection", "direct_interpolation", "classical_interpolation", "PMIS", "MIS"):
        def device_fn(*a, _fn=fn, **k):
            if k.get("refuse") or (a and a[0] == "refuse"):
                raise NotImplementedError
            return ("device", _fn)
        monkeypatch.setattr(cls, fn, device_fn)
    with agg.device_setup(pkg, products=False, classical=True):
        for t in TARGETS:
            patched = get(*t)
            assert patched is not originals[t] and patched.__name__ == t[1]
            assert patched("x") == ("device", t[1])
            assert patched("refuse") == ("reference",) + t                 # not on the device path: the function that was patched out
    assert all(get(*t) is originals[t] for t in TARGETS)
    with pytest.raises(RuntimeError):
        with agg.device_setup(pkg, products=False, classical=True):
            raise RuntimeError("inside")
    assert all(get(*t) is originals[t] for t in TARGETS)


def test_ruge_stuben_solver_under_device_setup_with_the_replay_reproduces_the_reference(emul):
    """the patch targets in the real reference package: with the device calls on the host replay (and SciPy's own sparse products),
    ruge_stuben_solver(CF='PMIS') under device_setup(classical=True) gives the unpatched hierarchy, array for array, on the same seed"""
    import oracle.refimport as ri
    if not ri.available():
        pytest.skip("oracle/_ref not present")
    import pyamg
    from pyamg_amd.aggregation import device_setup
    A = cc.csr("e2e.A")
    seed = int(cc.data()["e2e.seed"])
    np.random.seed(seed)
    want = pyamg.ruge_stuben_solver(A.copy(), CF="PMIS")
    calls = []
    for name in ("classical_strength_of_connection_abs", "pmis_splitting", "remove_strong_FF_connections", "rs_classical_interpolation_pass2"):
        def counted(*a, _fn=getattr(emul, name), _name=name, **k):
            calls.append(_name)
            return _fn(*a, **k)
        setattr(emul, name, counted)
    np.random.seed(seed)
    with device_setup(pyamg, products=False, classical=True):
        got = pyamg.ruge_stuben_solver(A.copy(), CF="PMIS")
    nl = len(want.levels)
    assert len(got.levels) == nl >= 3 and all(calls.count(c) == nl - 1 for c in set(calls)) and len(set(calls)) == 4
    cc.same_csr(sp.csr_array(got.levels[0].P), "e2e.P0")
    cc.same_csr(sp.csr_array(got.levels[1].A), "e2e.A1")
    for lg, lw in zip(got.levels, want.levels):
        for name in ("A", "P", "R"):
            if hasattr(lw, name):
                g, w = sp.csr_array(getattr(lg, name)), sp.csr_array(getattr(lw, name))
                assert g.shape == w.shape and np.array_equal(g.indptr, w.indptr) and np.array_equal(g.indices, w.indices)
                assert np.array_equal(g.data, w.data)


def test_standalone_program_under_the_sanitizers(tmp_path):
    """the replay as a program of its own (its main), built with -fsanitize=address,undefined: nothing sanitized is loaded into Python"""
    exe = tmp_path / "cle"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-DCLE_MAIN", str(HERE / "classical_emul.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr.lower() + r.stdout.lower() and "cannot find" in r.stderr.lower():
        pytest.skip("no sanitizer runtime for g++ here")
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
