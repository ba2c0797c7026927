"""Host checks of the approximate ideal restriction (AIR) setup (CPU, no GPU): tests/air_emul.cpp replays pamg_air.hip through the per-row
arithmetic of pyamg_amd/csrc/pamg_air.h -- lanes and lane groups as loops -- and is held against every committed fixture with
np.array_equal, THROUGH the Python surface (pyamg_amd.air with its device calls replaced by the replay; the strength matrix from the
replay of the classical setup), so the host steps between the kernels (eliminate_zeros, the C-point list) are checked with it.  Then the
size-class boundaries against a single-lane run of the same header, and the surface itself: NotImplementedError for what the device path
does not take, device_setup(air=True)."""
import ctypes
import subprocess
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from pyamg_amd import air
from pyamg_amd import classical as cls
import air_cases as ac
from test_classical_host import EmulCore as ClassicalEmulCore
from test_classical_host import emul_lib as classical_emul_lib  # noqa: F401  (a fixture)

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
E_ARG_REPLAY = -1


class EmulCore:
    """the pass-throughs of pyamg_amd.amg_core that pyamg_amd.air calls, on the host replay"""

    def __init__(self, lib):
        self.lib = lib
        self.classes = np.zeros(5, dtype=np.int32)
        self.one_lane = 0

    @staticmethod
    def p(a):
        assert a.flags.c_contiguous and a.dtype in (np.int32, np.float64)
        return a.ctypes.data_as(ctypes.c_void_p)

    def one_point_interpolation(self, Pp, Pj, Px, Cp, Cj, Cx, splitting):
        self.lib.ale_one_point(Pp.size - 1, self.p(Cp), self.p(Cj), self.p(Cx), self.p(splitting), self.p(Pp), self.p(Pj), self.p(Px))

    def approx_ideal_restriction_pass1(self, Rp, Cp, Cj, Cpts, splitting, distance=2):
        self.lib.ale_pass1(Cp.size - 1, Cpts.size, self.p(Cp), self.p(Cj), self.p(Cpts), self.p(splitting), int(distance), self.p(Rp))

    def approx_ideal_restriction_pass2(self, Rp, Rj, Rx, Ap, Aj, Ax, Cp, Cj, Cx, Cpts, splitting, distance=2, use_gmres=0, maxiter=10, precondition=1):
        if use_gmres:
            raise NotImplementedError("replay: not supported on the device path")          # what _capi.check makes of PAMG_E_UNSUPPORTED
        rc = self.lib.ale_pass2(Ap.size - 1, Cpts.size, self.p(Rp), self.p(Rj), self.p(Rx), self.p(Ap), self.p(Aj), self.p(Ax), self.p(Cp), self.p(Cj),
                                self.p(Cpts), self.p(splitting), int(distance), self.one_lane, self.p(self.classes))
        if rc == E_ARG_REPLAY:
            raise ValueError("replay: Rp does not agree with the neighbourhood sizes")
        assert rc == 0


@pytest.fixture(scope="module")
def emul_lib():
    out = HERE / "build"
    out.mkdir(exist_ok=True)
    so = out / "air_emul.so"
    src = HERE / "air_emul.cpp"
    hdr = ROOT / "pyamg_amd" / "csrc" / "pamg_air.h"
    if not so.exists() or so.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    return ctypes.CDLL(str(so))


@pytest.fixture()
def emul(emul_lib, classical_emul_lib, monkeypatch):  # noqa: F811
    core = EmulCore(emul_lib)
    monkeypatch.setattr(air, "amg_core", core)
    monkeypatch.setattr(cls, "amg_core", ClassicalEmulCore(classical_emul_lib))
    return core


# ------------------------------------------------------------------------------------------------ the replay against the fixtures
@pytest.mark.parametrize("case", ac.AIR)
def test_local_air_is_the_references(emul, case):
    ac.check_local_air(air, case)
    if case.startswith("hub"):
        assert emul.classes[4] == 1 and emul.classes[0] > 0  # the row beyond the 64-lane class
    if case == "box6x5x4":
        assert emul.classes[2] > 0 and emul.classes[3] > 0 and emul.classes[4] > 0
    if case == "box6x5x4.d1":
        assert emul.classes[1] > 0


@pytest.mark.parametrize("case", ac.AIR)
def test_row_pointer_and_the_rows_before_eliminate_zeros_are_the_references(emul, case):
    Rp, Rj, Rx = ac.raw_passes(emul, cls, case)
    if case == "singular":
        x = Rx[Rp[0]:Rp[1] - 1]
        assert np.sum(x == 0.0) == 2 and list(Rj[Rp[0]:Rp[1]]) == [2, 3, 4, 6, 0] and Rp[2] - Rp[1] == 1       # N = 0: the identity only


def test_pass2_refuses_a_row_pointer_that_is_not_pass1s(emul):
    with pytest.raises(ValueError, match="Rp"):
        ac.raw_passes(emul, cls, "convdiff13x11.d2.t0", shift=(3, 1))


@pytest.mark.parametrize("case,by_val", ac.ONEPT)
def test_one_point_interpolation_is_the_references(emul, case, by_val):
    P = ac.check_one_point(air, case, by_val)
    if not by_val:
        assert np.all(P.data == 1.0)


def test_fixture_reaches_its_paths():
    d = ac.data()
    N = {c: np.diff(d[f"air.{c}.Rp"]) - 1 for c in ac.AIR}
    allN = np.concatenate(list(N.values()))
    for lo, hi in ((0, 0), (1, 1), (2, 8), (9, 16), (17, 32), (33, 64), (65, 10 ** 6)):
        assert np.any((allN >= lo) & (allN <= hi)), (lo, hi)
    assert N["hub.d1"].max() == 100 and N["hub.d2"].max() == 101
    A1 = ac.csr("air.level1.A")
    assert any(np.any(np.diff(A1.indices[a:b]) < 0) for a, b in zip(A1.indptr[:-1], A1.indptr[1:]))          # unsorted rows
    A = ac.csr("air.convdiff13x11.A")
    assert (A - A.T).nnz > 0
    assert d["air.singular.Rraw.data"].size > d["air.singular.R.data"].size                                  # eliminate_zeros removed entries
    assert all(d[f"air.{c}.A.indptr"].size - 1 <= 300 for c in map(str, d["air.ops"]))
    assert {c for c, _ in ac.ONEPT} >= {"line5", "convdiff", "mixed48"}
    P = d["onept.mixed48.P0.indptr"]
    assert np.sum(np.diff(P) == 0) >= 3


# ------------------------------------------------------------------------------------------------ the size-class boundaries
@pytest.mark.parametrize("keep", [7, 8, 9, 16, 17, 32, 33, 64, 65])
def test_lane_groups_equal_one_lane_on_both_sides_of_every_boundary(emul, keep):
    """the hub with its C-point's neighbourhood cut to `keep` F-points: the lane group of that width (or the host path at 65) against a
    straight single-lane run of the same header"""
    A, splitting, theta, norm, _ = ac.air_inputs("hub.d1")
    A = A.tolil()
    for j in range(keep + 1, 101):
        A[0, j] = 0.0
    A = sp.csr_array(A.tocsr())
    A.eliminate_zeros()
    A = sp.csr_array((A.data, A.indices.astype(np.int32), A.indptr.astype(np.int32)), shape=A.shape)
    got = air.local_air(A, splitting, theta=theta, norm=norm, degree=1)
    classes = emul.classes.copy()
    assert got.indptr[1] == keep + 1
    want_class = 0 if keep <= 8 else 1 if keep <= 16 else 2 if keep <= 32 else 3 if keep <= 64 else 4
    assert classes[want_class] >= 1 and (want_class == 0 or classes[want_class] == 1)
    emul.one_lane = 1
    want = air.local_air(A, splitting, theta=theta, norm=norm, degree=1)
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices) and np.array_equal(got.data, want.data)
    assert np.all(np.isfinite(got.data))


# ------------------------------------------------------------------------------------------------ the Python surface
def _boom(*a, **k):
    raise AssertionError("a device call was made")


@pytest.fixture()
def nodevice(monkeypatch):
    core = types.SimpleNamespace(**{n: _boom for n in dir(EmulCore) if not n.startswith("_") and n != "p"})
    monkeypatch.setattr(air, "amg_core", core)
    monkeypatch.setattr(cls, "amg_core", types.SimpleNamespace(classical_strength_of_connection_abs=_boom, classical_strength_of_connection_min=_boom))


def test_what_the_device_path_does_not_take_says_so(nodevice):
    A = sp.csr_array(sp.eye_array(4, format="csr") * 2.0)
    s = np.array([1, 0, 1, 0], dtype=np.int32)
    A64 = A.copy()
    A64.indptr = np.array([0, 1, 2, 3, 2 ** 31 + 5], dtype=np.int64)    # (set behind SciPy's checks: an index beyond int32)
    for call in (lambda: air.local_air(A, s, use_gmres=True),
                 lambda: air.local_air(A.tobsr(blocksize=(2, 2)), s),
                 lambda: air.local_air(A.astype(np.float32), s),
                 lambda: air.local_air(A.tocsc(), s),
                 lambda: air.local_air(A64, s),
                 lambda: air.one_point_interpolation(A.tobsr(blocksize=(2, 2)), A, s),
                 lambda: air.one_point_interpolation(A.astype(np.float32), A, s),
                 lambda: air.one_point_interpolation(A, A.astype(np.float32), s),
                 lambda: air.one_point_interpolation(A, A, s.astype(np.float64)),
                 lambda: air.one_point_interpolation(A64, A64, s)):
        with pytest.raises(NotImplementedError):
            call()
    for call in (lambda: air.local_air(A.toarray(), s), lambda: air.one_point_interpolation(A.toarray(), A, s)):
        with pytest.raises(TypeError, match="not sparse"):
            call()


TARGETS = [("classical.air", "one_point_interpolation"), ("classical.interpolate", "one_point_interpolation"), ("classical.air", "local_air"),
           ("classical.interpolate", "local_air"), ("classical.air", "classical_strength_of_connection"), ("classical.air", "PMIS")]
# what classical=True patches, and air=True must leave alone
OTHERS = [("strength", "classical_strength_of_connection"), ("classical.interpolate", "classical_strength_of_connection"), ("classical.split", "PMIS"),
          ("classical.air", "RS")]


def _standin(monkeypatch):
    mods = {}
    for name in ("standin_air", "standin_air.strength", "standin_air.classical", "standin_air.classical.air", "standin_air.classical.interpolate",
                 "standin_air.classical.split"):
        m = types.ModuleType(name)
        mods[name] = m
        monkeypatch.setitem(sys.modules, name, m)
        if "." in name:
            setattr(mods[name.rsplit(".", 1)[0]], name.rsplit(".", 1)[1], m)
    originals = {}
    for mod, fn in TARGETS + OTHERS:
        def reference_fn(*a, _tag=(mod, fn), **k):
            return ("reference",) + _tag
        reference_fn.__name__ = fn
        setattr(mods["standin_air." + mod], fn, reference_fn)
        originals[(mod, fn)] = reference_fn
    return mods, originals


def test_device_setup_patches_and_restores_every_air_target(monkeypatch):
    import inspect
    from pyamg_amd import aggregation as agg
    assert inspect.signature(agg.device_setup).parameters["air"].default is False
    mods, originals = _standin(monkeypatch)
    pkg = mods["standin_air"]
    get = lambda mod, fn: getattr(mods["standin_air." + mod], fn)      # noqa: E731
    everything = TARGETS + OTHERS
    with agg.device_setup(pkg, products=False):
        assert all(get(*t) is originals[t] for t in everything)      # off by default: nothing is patched
    with agg.device_setup(pkg, products=False, air=False):
        assert all(get(*t) is originals[t] for t in everything)
    with agg.device_setup(pkg, products=False, classical=True):
        assert all(get(*t) is originals[t] for t in TARGETS)         # classical=True patches what it patched before, nothing of .classical.air
        assert get("classical.split", "PMIS") is not originals[("classical.split", "PMIS")]
    for mod_, fn in ((air, "one_point_interpolation"), (air, "local_air"), (cls, "classical_strength_of_connection"), (cls, "PMIS")):
        def device_fn(*a, _fn=fn, **k):
            if k.get("refuse") or (a and a[0] == "refuse"):
                raise NotImplementedError
            return ("device", _fn)
        monkeypatch.setattr(mod_, fn, device_fn)
    with agg.device_setup(pkg, products=False, air=True):
        for t in TARGETS:
            patched = get(*t)
            assert patched is not originals[t] and patched.__name__ == t[1]
            assert patched("x") == ("device", t[1])
            assert patched("refuse") == ("reference",) + t                 # not on the device path: the function that was patched out
        assert all(get(*t) is originals[t] for t in OTHERS)                # the RS splitting and the classical targets stay
    assert all(get(*t) is originals[t] for t in everything)
    with pytest.raises(RuntimeError):
        with agg.device_setup(pkg, products=False, air=True):
            raise RuntimeError("inside")
    assert all(get(*t) is originals[t] for t in everything)


def test_air_solver_under_device_setup_with_the_replay_reproduces_the_reference(emul):
    """the patch targets in the real reference package: with the device calls on the host replay (and SciPy's own sparse products),
    air_solver under device_setup(air=True) gives the unpatched hierarchy, array for array, on the same seed -- and the fixture's"""
    import oracle.refimport as ri
    if not ri.available():
        pytest.skip("oracle/_ref not present")
    import pyamg
    from pyamg_amd.aggregation import device_setup
    A = ac.csr("e2e.A")
    for cf in ac.E2E:
        kw = {} if cf == "rs" else {"CF": "PMIS"}
        seed = int(ac.data()[f"e2e.{cf}.seed"])
        np.random.seed(seed)
        want = pyamg.air_solver(A.copy(), max_coarse=20, **kw)
        follow_want = np.random.rand()
        np.random.seed(seed)
        with device_setup(pyamg, products=False, air=True):
            got = pyamg.air_solver(A.copy(), max_coarse=20, **kw)
        assert np.random.rand() == follow_want                 # the same random draws were consumed
        assert len(got.levels) == len(want.levels) >= 3
        for lg, lw in zip(got.levels, want.levels):
            for name in ("A", "P", "R"):
                if hasattr(lw, name):
                    g, w = sp.csr_array(getattr(lg, name)), sp.csr_array(getattr(lw, name))
                    assert g.shape == w.shape and np.array_equal(g.indptr, w.indptr) and np.array_equal(g.indices, w.indices)
                    assert np.array_equal(g.data, w.data)
        ac.check_hierarchy(cf, [(lv.A, lv.P, lv.R) for lv in got.levels[:2]] + [(got.levels[2].A,)])


def test_standalone_program_under_the_sanitizers(tmp_path):
    """the replay as a program of its own (its main), built with -fsanitize=address,undefined: nothing sanitized is loaded into Python"""
    exe = tmp_path / "ale"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-DALE_MAIN", str(HERE / "air_emul.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr.lower() + r.stdout.lower() and "cannot find" in r.stderr.lower():
        pytest.skip("no sanitizer runtime for g++ here")
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
