"""Host checks of the block (BSR) AIR setup (CPU, no GPU): tests/block_air_emul.cpp replays pamg_air_block.hip through the per-row
arithmetic of pyamg_amd/csrc/pamg_air_block.h -- lanes and lane groups as loops -- and is held against every committed fixture with
np.array_equal, THROUGH the Python surface (pyamg_amd.block_air with its device calls replaced by the replays: the block measure and
block pass 2 from this replay, pass 1 and the one-point rule from the replay of the scalar AIR setup, the strength kernels from the replay
of the classical setup).  Every lane-group width is held against a single-lane run of the same header.  Then what the fixture covers, the
C ABI of the two new symbols without a device, and device_setup(block_air=True) alone and together with air=True."""
import ctypes
import inspect
import re
import subprocess
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from pyamg_amd import block_air
import block_air_cases as bc
from test_air_host import EmulCore as AirEmulCore
from test_air_host import emul_lib as air_emul_lib  # noqa: F401  (a fixture)
from test_classical_host import EmulCore as ClassicalEmulCore
from test_classical_host import emul_lib as classical_emul_lib  # noqa: F401  (a fixture)

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
NORMS = {"abs": 0, "min": 1, "fro": 2}


class EmulCore:
    """the pass-throughs of pyamg_amd.amg_core that pyamg_amd.block_air calls, on the host replays"""
    BLOCK_NORMS = NORMS

    def __init__(self, lib, air_core, classical_core):
        self.lib = lib
        self.classes = np.zeros(6, dtype=np.int32)           # C-rows per size class of n = N * b, and the largest n
        self.one_lane = 0
        self.one_point_interpolation = air_core.one_point_interpolation
        self.approx_ideal_restriction_pass1 = air_core.approx_ideal_restriction_pass1
        self.classical_strength_of_connection_abs = classical_core.classical_strength_of_connection_abs
        self.classical_strength_of_connection_min = classical_core.classical_strength_of_connection_min

    @staticmethod
    def p(a):
        assert a.flags.c_contiguous and a.dtype in (np.int32, np.float64)
        return a.ctypes.data_as(ctypes.c_void_p)

    def block_strength_measure(self, blocksize, norm, Ax, out):
        assert Ax.size == out.size * blocksize * blocksize
        rc = self.lib.bae_measure(out.size, int(blocksize), NORMS[norm], self.p(Ax), self.p(out))
        if rc == -2:
            raise NotImplementedError("replay: not supported on the device path")
        assert rc == 0

    def block_approx_ideal_restriction_pass2(self, Rp, Rj, Rx, Ap, Aj, Ax, Cp, Cj, Cx, Cpts, splitting, blocksize, distance=2, use_gmres=0, maxiter=10,
                                             precondition=1):
        if use_gmres:
            raise NotImplementedError("replay: not supported on the device path")          # what _capi.check makes of PAMG_E_UNSUPPORTED
        assert Rx.size >= int(Rp[-1]) * blocksize * blocksize and Ax.size == Aj.size * blocksize * blocksize
        rc = self.lib.bae_pass2(Ap.size - 1, Cpts.size, self.p(Rp), self.p(Rj), self.p(Rx), self.p(Ap), self.p(Aj), self.p(Ax), self.p(Cp), self.p(Cj),
                                self.p(Cpts), self.p(splitting), int(blocksize), int(distance), self.one_lane, self.p(self.classes))
        if rc == -1:
            raise ValueError("replay: Rp does not agree with the neighbourhood sizes")
        assert rc == 0


@pytest.fixture(scope="module")
def emul_lib():
    out = HERE / "build"
    out.mkdir(exist_ok=True)
    so = out / "block_air_emul.so"
    src = HERE / "block_air_emul.cpp"
    hdrs = [ROOT / "pyamg_amd" / "csrc" / h for h in ("pamg_air_block.h", "pamg_air.h")]
    if not so.exists() or so.stat().st_mtime < max(f.stat().st_mtime for f in [src] + hdrs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    return ctypes.CDLL(str(so))


@pytest.fixture()
def emul(emul_lib, air_emul_lib, classical_emul_lib, monkeypatch):  # noqa: F811
    core = EmulCore(emul_lib, AirEmulCore(air_emul_lib), ClassicalEmulCore(classical_emul_lib))
    monkeypatch.setattr(block_air, "amg_core", core)
    return core


def size_class(n):
    return 0 if n <= 8 else 1 if n <= 16 else 2 if n <= 32 else 3 if n <= 64 else 4


# ------------------------------------------------------------------------------------------------ the replay against the fixtures
@pytest.mark.parametrize("case", sorted(bc.STRENGTH))
def test_block_measure_and_strength_are_the_references(emul, case):
    bc.check_measure(emul, case)
    bc.check_strength(block_air, case)


@pytest.mark.parametrize("case", sorted(bc.AIR))
def test_local_air_is_the_references_at_every_width_and_by_one_lane(emul, case):
    R = bc.check_local_air(block_air, case)
    classes = emul.classes.copy()
    d = bc.data()
    b = bc.OPS[bc.AIR[case][0]]
    N = np.diff(d[f"blk.{case}.Rraw.indptr"]) - 1
    want = np.bincount([4 if k > 64 else size_class(k * b) for k in N if k > 0], minlength=5)
    assert np.array_equal(classes[:5], want) and classes[5] == N.max() * b          # every row went to the width of its n = N * b
    emul.one_lane = 1
    S = bc.check_local_air(block_air, case)
    assert np.array_equal(R.indptr, S.indptr) and np.array_equal(R.indices, S.indices) and np.array_equal(R.data, S.data)


@pytest.mark.parametrize("case", sorted(bc.AIR))
def test_rows_before_eliminate_zeros_are_the_references(emul, case):
    bc.raw_pass2(emul, block_air, case)


def test_pass2_refuses_a_row_pointer_that_is_not_pass1s(emul):
    with pytest.raises(ValueError, match="Rp"):
        bc.raw_pass2(emul, block_air, "ck2.d2", shift=(3, 1))
    with pytest.raises(NotImplementedError):
        bc.raw_pass2(emul, block_air, "ck2.d2", use_gmres=1)


@pytest.mark.parametrize("case", sorted(bc.ONEPT))
def test_one_point_interpolation_is_the_references(emul, case):
    bc.check_one_point(block_air, case)


def test_fro_with_blocks_of_eight_is_refused(emul):
    A, _ = bc.operator("ck8")
    with pytest.raises(NotImplementedError):
        block_air.classical_strength_of_connection(A, theta=0.1, norm="fro")
    with pytest.raises(NotImplementedError):
        emul.block_strength_measure(8, "fro", np.ascontiguousarray(A.data).reshape(-1), np.empty(A.indices.size))


# ------------------------------------------------------------------------------------------------ what the fixture covers
def test_fixture_covers_what_it_is_meant_to():
    d = bc.data()
    assert all(np.all(np.isfinite(v)) for v in d.values())
    assert {bc.OPS[v[0]] for v in bc.AIR.values()} >= {1, 2, 3, 4, 5, 8}
    assert all(d[f"blk.{op}.A.indptr"].size - 1 <= 300 for op in bc.OPS)
    orders, rhs_absent, sys_absent = [], {1: 0, 2: 0}, 0
    for case, (op, norm, theta, degree) in bc.AIR.items():
        b = bc.OPS[op]
        A, splitting = bc.operator(op)
        Rp, Rj = d[f"blk.{case}.Rraw.indptr"], d[f"blk.{case}.Rraw.indices"]
        Cpts = np.where(splitting == 1)[0]
        stored = [set(A.indices[A.indptr[i]:A.indptr[i + 1]]) for i in range(A.indptr.size - 1)]
        for r in range(Cpts.size):
            Nf = Rj[Rp[r]:Rp[r + 1] - 1]
            orders.append(Nf.size * b)
            rhs_absent[degree] += sum(j not in stored[Cpts[r]] for j in Nf)
            sys_absent += sum(i not in stored[j] for j in Nf for i in Nf)
    orders = np.array(orders)
    for lo, hi in ((0, 0), (1, 8), (9, 16), (17, 32), (33, 64), (65, 10 ** 6)):
        assert np.any((orders >= lo) & (orders <= hi)), (lo, hi)
    assert set(orders) >= {8, 9, 16, 17, 64, 65}                                     # both sides of every lane-group boundary
    assert {v[3] for v in bc.AIR.values()} == {1, 2}
    assert rhs_absent[2] > 0 and sys_absent > 0                                      # absent right-hand-side blocks (degree 2), absent blocks of the system
    assert np.max(np.diff(d["blk.hub1x70.d1.Rraw.indptr"])) - 1 == 70               # a neighbourhood above the 64-column staging cap
    Au, _ = bc.operator("ck3u")
    assert any(np.any(np.diff(Au.indices[a:b]) < 0) for a, b in zip(Au.indptr[:-1], Au.indptr[1:])) and "ck3u.d2" in bc.AIR
    keep = d["blk.diag3.d1.R.keep"].astype(bool)
    blocks = d["blk.diag3.d1.Rraw.data"].reshape(-1, 3, 3)
    assert np.sum(~keep) >= 1 and np.any(np.any(blocks[keep] == 0.0, axis=(1, 2)))  # a whole block removed; zeros inside kept blocks
    combos = {(v[1], v[2]) for v in bc.STRENGTH.values()}
    assert combos >= {(norm, theta) for norm in ("abs", "min", "fro") for theta in (0.0, 0.1, 1.0)}
    tiny = 0
    for case, (op, norm, theta) in bc.STRENGTH.items():
        A, _ = bc.operator(op)
        m = d[f"str.{case}.measure"]
        tiny += int(np.sum((m == 0.0) & np.any(A.data != 0.0, axis=(1, 2))))
    assert tiny >= 3                                                                 # a block whose measure falls under 1e-16, for every norm
    assert bc.GOLDEN.stat().st_size <= (bc.GOLDEN.parent / "kernels_air.npz").stat().st_size
    assert list(d["e2e.sizes"][:3]) == [d[f"e2e.A{lvl}.indptr"].size * 2 - 2 for lvl in range(3)]


# ------------------------------------------------------------------------------------------------ the Python surface
def _boom(*a, **k):
    raise AssertionError("a device call was made")


@pytest.fixture()
def nodevice(monkeypatch):
    names = ("one_point_interpolation", "approx_ideal_restriction_pass1", "classical_strength_of_connection_abs", "classical_strength_of_connection_min",
             "block_strength_measure", "block_approx_ideal_restriction_pass2")
    monkeypatch.setattr(block_air, "amg_core", types.SimpleNamespace(BLOCK_NORMS=NORMS, **{n: _boom for n in names}))


def test_what_the_device_path_does_not_take_says_so(nodevice):
    A = sp.bsr_array(np.kron(np.eye(4) * 2.0 - np.eye(4, k=1), np.array([[2.0, 1.0], [0.5, 3.0]])), blocksize=(2, 2))
    C = sp.csr_array(np.eye(4))
    s = np.array([1, 0, 1, 0], dtype=np.int32)
    A9 = sp.bsr_array(np.kron(np.eye(2), np.ones((9, 9))), blocksize=(9, 9))
    Arect = sp.bsr_array(np.kron(np.eye(4), np.ones((2, 2))), blocksize=(2, 1))
    A64 = A.copy()
    A64.indptr = np.array([0, 2, 4, 6, 2 ** 31 + 5], dtype=np.int64)         # (set behind SciPy's checks: an index beyond int32)
    for call in (lambda: block_air.local_air(A, s, use_gmres=True),
                 lambda: block_air.local_air(A.tocsr(), s),
                 lambda: block_air.local_air(A.astype(np.float32), s),
                 lambda: block_air.local_air(A9, s[:2]),
                 lambda: block_air.local_air(Arect, s),
                 lambda: block_air.local_air(A64, s),
                 lambda: block_air.local_air(A, s.astype(np.float64)),
                 lambda: block_air.one_point_interpolation(A.tocsr(), C, s),
                 lambda: block_air.one_point_interpolation(A.astype(np.float32), C, s),
                 lambda: block_air.one_point_interpolation(A, C.astype(np.float32), s),
                 lambda: block_air.one_point_interpolation(A, C.tobsr(), s),
                 lambda: block_air.one_point_interpolation(A9, C, s),
                 lambda: block_air.classical_strength_of_connection(A, block=False),
                 lambda: block_air.classical_strength_of_connection(A.tocsr()),
                 lambda: block_air.classical_strength_of_connection(A.toarray()),
                 lambda: block_air.classical_strength_of_connection(A.astype(np.float32)),
                 lambda: block_air.classical_strength_of_connection(A9),
                 lambda: block_air.classical_strength_of_connection(Arect)):
        with pytest.raises(NotImplementedError):
            call()
    for call in (lambda: block_air.local_air(A.toarray(), s), lambda: block_air.one_point_interpolation(A.toarray(), C, s)):
        with pytest.raises(TypeError, match="not sparse"):
            call()
    with pytest.raises(ValueError, match="theta"):
        block_air.classical_strength_of_connection(A, theta=1.5)
    with pytest.raises(ValueError, match="norm"):
        block_air.classical_strength_of_connection(A, norm="max")


def test_signatures_are_the_references():
    ref = {"classical_strength_of_connection": ["A", "theta", "block", "norm"], "one_point_interpolation": ["A", "C", "splitting", "by_val"],
           "local_air": ["A", "splitting", "theta", "norm", "degree", "use_gmres", "maxiter", "precondition"]}
    for name, params in ref.items():
        assert list(inspect.signature(getattr(block_air, name)).parameters) == params
    assert inspect.signature(block_air.classical_strength_of_connection).parameters["block"].default is True
    from pyamg_amd import amg_core
    assert list(inspect.signature(amg_core.block_approx_ideal_restriction_pass2).parameters) == \
        ["Rp", "Rj", "Rx", "Ap", "Aj", "Ax", "Cp", "Cj", "Cx", "Cpts", "splitting", "blocksize", "distance", "use_gmres", "maxiter", "precondition"]
    assert {"block_strength_measure", "block_approx_ideal_restriction_pass2"} <= set(amg_core.__all__)
    from pyamg_amd import air
    assert "block_air" in air.__doc__                        # the scalar module points to the block path


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_c_abi_declares_exports_and_refuses_before_anything_is_written():
    from pyamg_amd import _capi as capi
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pyamg_amd.h").read_text(), flags=re.S)
    for name, nargs in (("pamg_block_strength_measure", 7), ("pamg_block_approx_ideal_restriction_pass2", 27)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == nargs, name
    m = re.search(r"pamg_block_approx_ideal_restriction_pass2\s*\(([^)]*)\)", hdr)
    assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")][-5:] == ["blocksize", "distance", "use_gmres", "maxiter", "precondition"]
    lib = capi.load()
    p = capi.ptr
    M, P2 = lib.pamg_block_strength_measure, lib.pamg_block_approx_ideal_restriction_pass2
    assert len(M.argtypes) == 7 and len(P2.argtypes) == 27
    Ax, out = np.full(4 * 81, 0.5), np.full(4, -5.0)
    assert M(4, 2, 3, p(Ax), Ax.size, p(out), 4) == capi.E_ARG                       # no such norm
    assert M(4, 0, 0, p(Ax), Ax.size, p(out), 4) == capi.E_ARG
    assert M(4, 2, 0, p(Ax), 15, p(out), 4) == capi.E_ARG                            # too few values
    assert M(4, 2, 0, p(Ax), Ax.size, p(out), 3) == capi.E_ARG
    assert M(-1, 2, 0, p(Ax), Ax.size, p(out), 4) == capi.E_ARG
    assert M(4, 9, 0, p(Ax), Ax.size, p(out), 4) == capi.E_UNSUPPORTED
    assert M(4, 8, 2, p(Ax), Ax.size, p(out), 4) == capi.E_UNSUPPORTED               # 'fro' with blocks of 8
    assert M(0, 2, 0, None, 0, None, 0) == capi.OK
    assert np.all(out == -5.0)
    A, splitting = bc.operator("hub2x4")
    b = 2
    Apt, Aj, Axx = A.indptr, A.indices, np.ascontiguousarray(A.data).reshape(-1)
    Cpts = np.ascontiguousarray(np.where(splitting == 1)[0], dtype=np.int32)
    Rp = bc.data()["blk.hub2x4.d1.Rraw.indptr"].copy()
    Rj, Rx = np.full(int(Rp[-1]), -5, dtype=np.int32), np.full(int(Rp[-1]) * b * b, -5.0)
    Cx = np.ones(Aj.size)

    def p2(rp=Rp, rps=Rp.size, rxs=Rx.size, ap=Apt, aj=Aj, axs=Axx.size, cpts=Cpts, sps=splitting.size, bs=b, gm=0):
        return P2(p(rp), rps, p(Rj), Rj.size, p(Rx), rxs, p(ap), Apt.size, p(aj), Aj.size, p(Axx), axs, p(Apt), Apt.size, p(Aj), Aj.size, p(Cx), Cx.size,
                  p(cpts), cpts.size, p(splitting), sps, bs, 1, gm, 10, 1)
    bad_start = Apt.copy(); bad_start[0] = 1
    far = Aj.copy(); far[2] = Apt.size - 1
    not0 = Rp.copy(); not0[0] = 1
    outside = Cpts.copy(); outside[-1] = Apt.size - 1
    for st in (p2(ap=bad_start), p2(aj=far), p2(axs=Axx.size - 1), p2(rp=not0), p2(rps=Rp.size - 1), p2(rxs=Rx.size - 1), p2(cpts=outside),
               p2(sps=splitting.size - 1), p2(bs=0)):
        assert st == capi.E_ARG
    assert p2(gm=1) == capi.E_UNSUPPORTED and p2(bs=9) == capi.E_UNSUPPORTED
    assert np.all(Rj == -5) and np.all(Rx == -5.0)                                   # nothing was written


# ------------------------------------------------------------------------------------------------ device_setup(block_air=True)
BLOCK_TARGETS = [("classical.air", "classical_strength_of_connection"), ("classical.air", "one_point_interpolation"),
                 ("classical.interpolate", "one_point_interpolation"), ("classical.air", "local_air"), ("classical.interpolate", "local_air")]
AIR_ONLY = [("classical.air", "PMIS")]
# what classical=True patches, and neither air=True nor block_air=True may touch
OTHERS = [("strength", "classical_strength_of_connection"), ("classical.interpolate", "classical_strength_of_connection"), ("classical.split", "PMIS"),
          ("classical.air", "RS")]


def _standin(monkeypatch):
    mods = {}
    for name in ("standin_blk", "standin_blk.strength", "standin_blk.classical", "standin_blk.classical.air", "standin_blk.classical.interpolate",
                 "standin_blk.classical.split"):
        m = types.ModuleType(name)
        mods[name] = m
        monkeypatch.setitem(sys.modules, name, m)
        if "." in name:
            setattr(mods[name.rsplit(".", 1)[0]], name.rsplit(".", 1)[1], m)
    originals = {}
    for mod, fn in BLOCK_TARGETS + AIR_ONLY + OTHERS:
        def reference_fn(*a, _tag=(mod, fn), **k):
            return ("reference",) + _tag
        reference_fn.__name__ = fn
        setattr(mods["standin_blk." + mod], fn, reference_fn)
        originals[(mod, fn)] = reference_fn
    return mods, originals


def test_device_setup_patches_in_order_and_restores_every_target(monkeypatch):
    from pyamg_amd import aggregation as agg
    from pyamg_amd import air, classical as cls
    assert inspect.signature(agg.device_setup).parameters["block_air"].default is False
    mods, originals = _standin(monkeypatch)
    pkg = mods["standin_blk"]
    get = lambda mod, fn: getattr(mods["standin_blk." + mod], fn)      # noqa: E731
    everything = BLOCK_TARGETS + AIR_ONLY + OTHERS
    untouched = lambda ts: all(get(*t) is originals[t] for t in ts)    # noqa: E731
    with agg.device_setup(pkg, products=False):
        assert untouched(everything)                                   # off by default: nothing is patched
    with agg.device_setup(pkg, products=False, block_air=False, classical=True):
        assert untouched(BLOCK_TARGETS + AIR_ONLY)

    def device_fn(layer, name):
        def fn(*a, **k):
            what = a[0] if a else None
            if what == "refuse" or (layer == "block" and what == "csr"):
                raise NotImplementedError
            return (layer, name)
        return fn
    for mod_, layer, names in ((block_air, "block", ("classical_strength_of_connection", "one_point_interpolation", "local_air")),
                               (air, "csr", ("one_point_interpolation", "local_air")), (cls, "csr", ("classical_strength_of_connection", "PMIS"))):
        for name in names:
            monkeypatch.setattr(mod_, name, device_fn(layer, name))
    # alone: the block function, then the reference
    with agg.device_setup(pkg, products=False, block_air=True):
        for t in BLOCK_TARGETS:
            patched = get(*t)
            assert patched is not originals[t] and patched.__name__ == t[1]
            assert patched("bsr") == ("block", t[1])
            assert patched("csr") == ("reference",) + t and patched("refuse") == ("reference",) + t
        assert untouched(AIR_ONLY + OTHERS)
    assert untouched(everything)
    # with air=True: the block function, then the CSR function, then the reference
    with agg.device_setup(pkg, products=False, air=True, block_air=True):
        for t in BLOCK_TARGETS:
            patched = get(*t)
            assert patched("bsr") == ("block", t[1]) and patched("csr") == ("csr", t[1]) and patched("refuse") == ("reference",) + t
        assert get(*AIR_ONLY[0])("x") == ("csr", "PMIS")
        assert untouched(OTHERS)
    assert untouched(everything)                                       # undone in reverse order: every name is the identical object again
    with agg.device_setup(pkg, products=False, air=True, classical=True, block_air=True, cljp=True):
        assert not any(get(*t) is originals[t] for t in BLOCK_TARGETS + AIR_ONLY + OTHERS[:3])
    assert untouched(everything)
    with pytest.raises(RuntimeError):
        with agg.device_setup(pkg, products=False, air=True, block_air=True):
            raise RuntimeError("inside")
    assert untouched(everything)


def _same_levels(got, want):
    assert len(got.levels) == len(want.levels) >= 3
    for lg, lw in zip(got.levels, want.levels):
        for name in ("A", "P", "R"):
            if hasattr(lw, name):
                g, w = getattr(lg, name), getattr(lw, name)
                nnz = int(w.indptr[-1])                      # (the reference's block P carries an uninitialised tail beyond indptr[-1])
                assert g.format == w.format and g.shape == w.shape and (w.format != "bsr" or tuple(g.blocksize) == tuple(w.blocksize))
                assert np.array_equal(g.indptr, w.indptr) and np.array_equal(g.indices[:nnz], w.indices[:nnz])
                assert np.array_equal(g.data[:nnz], w.data[:nnz])


@pytest.mark.parametrize("keywords", [{"block_air": True}, {"air": True, "classical": True, "block_air": True}], ids=["alone", "with_air_and_classical"])
def test_air_solver_under_device_setup_with_the_replay_reproduces_the_reference(emul, air_emul_lib, classical_emul_lib, monkeypatch, keywords):  # noqa: F811
    """the patch targets in the real reference package: with the device calls on the host replays (and SciPy's own sparse products),
    air_solver on a BSR operator under device_setup(block_air=True), alone and with air=True and classical=True, gives the unpatched
    hierarchy, array for array, on the same seed -- and the fixture's; a CSR operator falls through the block functions and still gives
    the reference's hierarchy"""
    import oracle.refimport as ri
    if not ri.available():
        pytest.skip("oracle/_ref not present")
    import pyamg
    from pyamg_amd import air, classical as cls
    from pyamg_amd.aggregation import device_setup
    monkeypatch.setattr(air, "amg_core", AirEmulCore(air_emul_lib))
    monkeypatch.setattr(cls, "amg_core", ClassicalEmulCore(classical_emul_lib))
    A = bc.bsr("e2e.A0", 2)
    seed = int(bc.data()["e2e.seed"][0])
    np.random.seed(seed)
    want = pyamg.air_solver(A.copy(), CF="PMIS", max_coarse=10)
    follow_want = np.random.rand()
    calls = []
    for name in ("block_strength_measure", "block_approx_ideal_restriction_pass2"):
        def counted(*a, _fn=getattr(emul, name), _name=name, **k):
            calls.append(_name)
            return _fn(*a, **k)
        setattr(emul, name, counted)
    np.random.seed(seed)
    with device_setup(pyamg, products=False, **keywords):
        got = pyamg.air_solver(A.copy(), CF="PMIS", max_coarse=10)
    assert np.random.rand() == follow_want                 # the same random draws were consumed
    assert calls.count("block_approx_ideal_restriction_pass2") == len(want.levels) - 1        # the block path ran at every level, not the fall-back
    _same_levels(got, want)
    assert all(lv.A.format == "bsr" for lv in got.levels)
    bc.check_hierarchy([(lv.A, lv.P, lv.R) for lv in got.levels[:2]] + [(got.levels[2].A,)])
    Ac = sp.csr_array(A)
    Ac = sp.csr_array((Ac.data, Ac.indices.astype(np.int32), Ac.indptr.astype(np.int32)), shape=Ac.shape)
    del calls[:]
    np.random.seed(seed)
    want = pyamg.air_solver(Ac.copy(), CF="PMIS", max_coarse=10)
    np.random.seed(seed)
    with device_setup(pyamg, products=False, **keywords):
        got = pyamg.air_solver(Ac.copy(), CF="PMIS", max_coarse=10)
    assert not calls and all(lv.A.format == "csr" for lv in got.levels)
    _same_levels(got, want)


def test_standalone_program_under_the_sanitizers(tmp_path):
    """the replay as a program of its own (its main), built with -fsanitize=address,undefined: nothing sanitized is loaded into Python"""
    exe = tmp_path / "bae"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-DBAE_MAIN", str(HERE / "block_air_emul.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr.lower() + r.stdout.lower() and "cannot find" in r.stderr.lower():
        pytest.skip("no sanitizer runtime for g++ here")
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
