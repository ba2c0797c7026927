"""Host checks of energy-minimisation prolongation smoothing with CG (CPU, no GPU): tests/energy_emul.cpp replays pamg_energy.hip
through the per-lane phases of pyamg_amd/csrc/pamg_energy.h -- lanes as loops, a phase for every lane before the next -- and is driven
THROUGH the Python surface (pyamg_amd.energy with its device calls replaced by the replay).  The two kernel-level pieces and
satisfy_constraints are held against every fixture with np.array_equal; the driver against the reference's recorded newsum and T at
the project's fp64 parity bar, 1e-10 (energy_cases.BAR).  Then the surface: NotImplementedError for what the device path does not
take, device_setup(energy=True), the C ABI's refusals."""
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
import energy_cases as ec

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent


class EmulCore:
    """the pass-throughs of pyamg_amd.amg_core that pyamg_amd.energy calls, on the host replay; gw = 0: the device's group width"""

    def __init__(self, lib, gw=0):
        self.lib, self.gw = lib, gw
        self.calls, self.last = [], None

    @staticmethod
    def p(a):
        if a is None:
            return ctypes.c_void_p(0)
        assert isinstance(a, np.ndarray) and a.flags.c_contiguous and a.dtype in (np.int32, np.float64, np.uint8)
        return a.ctypes.data_as(ctypes.c_void_p)

    @staticmethod
    def done(rc):
        if rc == 2:
            raise NotImplementedError("replay: not supported on the device path")        # what _capi.check makes of PAMG_E_UNSUPPORTED
        assert rc == 0

    def incomplete_mat_mult_bsr(self, Ap, Aj, Ax, Bp, Bj, Bx, Sp, Sj, Sx, n_brow, n_bcol, brow_A, bcol_A, bcol_B, gw=None):
        self.calls.append("incomplete_mat_mult_bsr")
        assert Ap.size == Sp.size == n_brow + 1 and Sx.size == Sp[-1] * brow_A * bcol_B and (Sj.size == 0 or Sj.max() < n_bcol)
        self.done(self.lib.ene_imm(self.gw if gw is None else gw, *(self.p(a) for a in (Ap, Aj, Ax, Bp, Bj, Bx, Sp, Sj, Sx)), int(n_brow),
                                   int(brow_A), int(bcol_A), int(bcol_B)))

    def satisfy_constraints_helper(self, r, c, n, K, x, y, z, Sp, Sj, Sx, gw=None):
        self.calls.append("satisfy_constraints_helper")
        assert y.size == n * r * K and z.size == n * K * K and Sx.size == Sp[-1] * r * c
        self.done(self.lib.ene_constraints(self.gw if gw is None else gw, int(r), int(c), int(n), int(K), self.p(x), self.p(y), self.p(z), self.p(Sp),
                                           self.p(Sj), self.p(Sx)))

    def satisfy_constraints(self, r, c, n, K, B, BtBinv, Sp, Sj, Sx):
        self.calls.append("satisfy_constraints")
        assert BtBinv.size == n * K * K and Sx.size == Sp[-1] * r * c
        self.done(self.lib.ene_constraints(self.gw, int(r), int(c), int(n), int(K), self.p(B), None, self.p(BtBinv), self.p(Sp), self.p(Sj), self.p(Sx)))

    def energy_cg(self, n, nbc, r, c, K, Ap, Aj, Ax, Sp, Sj, Tx, B, BtBinv, Dinv, cmask, PIx, maxiter, tol):
        self.calls.append("energy_cg")
        assert Tx.size == Sp[-1] * r * c and Dinv.size == n * r and B.size == nbc * c * K and (cmask is None) == (PIx is None)
        its, ns = ctypes.c_int(0), ctypes.c_int(0)
        sums = np.zeros(max(maxiter, 1))
        self.done(self.lib.ene_cg(self.gw, int(n), int(nbc), int(r), int(c), int(K), *(self.p(a) for a in (Ap, Aj, Ax, Sp, Sj, Tx, B, BtBinv, Dinv, cmask, PIx)),
                                  int(maxiter), ctypes.c_double(tol), ctypes.byref(its), self.p(sums), ctypes.byref(ns)))
        self.last = (int(its.value), sums[:ns.value].copy())
        return self.last


NAMES = ["incomplete_mat_mult_bsr", "satisfy_constraints_helper", "satisfy_constraints", "energy_cg"]


def build_emul():
    out = HERE / "build"
    out.mkdir(exist_ok=True)
    so = out / "energy_emul.so"
    src = HERE / "energy_emul.cpp"
    hdr = ROOT / "pyamg_amd" / "csrc" / "pamg_energy.h"
    if not so.exists() or so.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    for f in (lib.ene_imm, lib.ene_constraints, lib.ene_cg):
        f.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def emul_lib():
    return build_emul()


@pytest.fixture()
def emul(emul_lib, monkeypatch):
    core = EmulCore(emul_lib)
    monkeypatch.setattr(en, "amg_core", core)
    return core


# ------------------------------------------------------------------------------------------------ the replay against the fixtures
def test_the_fixture_holds_the_cases_the_tests_name():
    d = ec.data()
    assert [str(s) for s in d["imm.names"]] == ec.IMM and [str(s) for s in d["sc.names"]] == ec.SC and [str(s) for s in d["cg.names"]] == ec.CG
    for k in d:
        if k.endswith(".shape"):
            assert d[k][0] <= 300                            # every operator has at most 300 rows
    A, B, S, out = ec.imm_inputs("crafted")
    lengths = np.diff(S.indptr) * 4
    assert lengths[1] == 0 and lengths[0] > 64 and S.data.all()                         # an empty row, a row beyond the widest group, Sx set on entry
    untouched = np.all(out.reshape(S.data.shape) == S.data, axis=(1, 2))
    assert untouched.sum() >= 5                              # stored blocks without a contribution: back as they went in
    A, B, S, out = ec.imm_inputs("unsortedB")
    assert any(np.any(np.diff(B.indices[B.indptr[i]:B.indptr[i + 1]]) < 0) for i in range(B.indptr.size - 1))
    assert [ec.sc_inputs(n)[1].shape[1] for n in ("nd1", "nd3", "nd6")] == [1, 3, 6]
    U, Bc, Z, _, _ = ec.sc_inputs("nd_gt_cols")
    assert Bc.shape[1] > U.blocksize[1]
    assert np.diff(ec.sc_inputs("oneblock")[0].indptr)[2] == 1 and not ec.sc_inputs("zero_btbinv")[2][3].any()
    kws = {n: ec.cg_inputs(n)[5] for n in ec.CG}
    assert {kw["maxiter"] for kw in kws.values()} == {1, 4} and kws["diagonal"]["weighting"] == "diagonal"
    assert [n for n in ec.CG if kws[n]["Cpt_params"][0]] == ["rn_poisson", "rn_aniso", "rn_elas", "diagonal"]
    assert len(d["cg.bigtol.newsums"]) == 2 < kws["bigtol"]["maxiter"] and d["cg.bigtol.newsums"][1] < kws["bigtol"]["tol"]


@pytest.mark.parametrize("name", ec.IMM)
def test_incomplete_product_is_the_references(emul, name):
    got, want = ec.run_imm(emul, name)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", ec.SC)
def test_constraints_helper_is_the_references(emul, name):
    got, want = ec.run_helper(emul, name)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", ec.SC)
def test_satisfy_constraints_is_the_references(emul, name):
    got, want = ec.run_satisfy(en, name)
    assert np.array_equal(got, want) and emul.calls == ["satisfy_constraints"]


@pytest.mark.parametrize("gw", [8, 16, 32, 64])
def test_lane_group_boundaries_against_a_single_lane(emul, gw):
    for name in ec.IMM:
        one, _ = ec.run_imm(emul, name, gw=1)
        assert np.array_equal(ec.run_imm(emul, name, gw=gw)[0], one)
    for name in ec.SC:
        one, _ = ec.run_helper(emul, name, gw=1)
        assert np.array_equal(ec.run_helper(emul, name, gw=gw)[0], one)
    for name in ("sa_elas", "rn_elas", "rn_poisson"):
        emul.gw = 1
        one = ec.run_cg(en, name)
        sums1 = emul.last[1]
        emul.gw = gw
        got = ec.run_cg(en, name)
        assert np.array_equal(got.data, one.data) and np.array_equal(emul.last[1], sums1)          # the tree is fixed: not a bit moves


@pytest.mark.parametrize("name", ec.CG)
def test_driver_agrees_with_the_reference_at_the_parity_bar(emul, name):
    """measured on the replay over the fixtures: |dT| / max|T| <= 8.5e-16, |d(T B)| / max|T| <= 3.8e-15, |dnewsum| / newsum <= 8.2e-16 --
    four orders of magnitude and more below the bar"""
    A, T, B, BtBinv, pattern, kw = ec.cg_inputs(name)
    got = ec.run_cg(en, name)
    its, sums = emul.last
    dT, dTB, dS = ec.cg_differences(name, got, sums)
    assert dS <= ec.BAR and dT <= ec.BAR and dTB <= ec.BAR
    assert got.format == "bsr" and got.blocksize == T.blocksize and np.array_equal(got.indices, pattern.indices)
    assert its == (1 if name == "bigtol" else kw["maxiter"])
    assert ec.c_rows_are_injected(name, got) == (0 if not kw["Cpt_params"][0] else np.count_nonzero(kw["Cpt_params"][1]["I_F"].diagonal() == 0))
    assert emul.calls == ["energy_cg"]


def test_pattern_rows_in_any_stored_order(emul):
    """a pattern whose rows are not sorted: T is expanded onto it block by block and comes back on it; the row partials then run in
    another order, so the result agrees at the bar, not bit for bit"""
    A, T, B, BtBinv, pattern, kw = ec.cg_inputs("rn_elas")
    rng = np.random.default_rng(3)
    for i in range(pattern.indptr.size - 1):
        lo, hi = pattern.indptr[i], pattern.indptr[i + 1]
        pattern.indices[lo:hi] = pattern.indices[lo:hi][rng.permutation(hi - lo)]
    pattern.has_sorted_indices = False
    got = en.cg_prolongation_smoothing(A, T, B, BtBinv, pattern, kw["maxiter"], kw["tol"], kw["weighting"], kw["Cpt_params"])
    assert np.array_equal(got.indices, pattern.indices)
    dT, dTB, dS = ec.cg_differences("rn_elas", got, emul.last[1])
    assert max(dT, dTB, dS) <= ec.BAR and ec.c_rows_are_injected("rn_elas", got) > 0


def test_explicit_zero_blocks_leave_with_eliminate_zeros(emul):
    d = ec.data()
    got = ec.run_cg(en, "rn_poisson")
    got.eliminate_zeros()
    want = sp.csr_array(d["cg.rn_poisson.T_out"])
    want.eliminate_zeros()
    g = sp.csr_array(got)
    g.sort_indices()
    assert np.array_equal(g.indptr, want.indptr) and np.array_equal(g.indices, want.indices)


def test_empty_residual_returns_the_tentative_prolongator(emul, capsys):
    A, T, B, BtBinv, pattern, kw = ec.cg_inputs("sa_poisson")
    empty = sp.bsr_array(pattern.shape, blocksize=pattern.blocksize, dtype=np.float64)
    T0 = sp.bsr_array(T.shape, blocksize=T.blocksize, dtype=np.float64)
    assert en.cg_prolongation_smoothing(A, T0, B, BtBinv, empty, 4, 1e-8) is T0
    assert "Initial R no nonzeros on a level" in capsys.readouterr().out and emul.calls == []


# ------------------------------------------------------------------------------------------------ the Python surface
def _boom(*a, **k):
    raise AssertionError("a device call was made")


@pytest.fixture()
def nodevice(monkeypatch):
    monkeypatch.setattr(en, "amg_core", types.SimpleNamespace(**{n: _boom for n in NAMES}))


def test_what_the_device_path_does_not_take_says_so_before_a_device_call(nodevice):
    A, T, B, BtBinv, pattern, kw = ec.cg_inputs("rn_elas")
    cg = en.cg_prolongation_smoothing
    big = pattern.copy()
    big.indices = big.indices.astype(np.int64)
    big.indices[-1] = 2**31 + 5
    small = sp.bsr_array((pattern.data[1:], pattern.indices[1:], np.maximum(pattern.indptr - 1, 0)), shape=pattern.shape)
    A7 = sp.bsr_array(sp.eye_array(14, format="csr"), blocksize=(7, 7))
    T7 = sp.bsr_array(np.ones((14, 7)), blocksize=(7, 7))
    for call in (lambda: cg(A, T, B, BtBinv, pattern, 4, 1e-8, "block", kw["Cpt_params"]),
                 lambda: cg(A.astype(np.float32), T, B, BtBinv, pattern, 4, 1e-8),
                 lambda: cg(A.astype(np.complex128), T, B, BtBinv, pattern, 4, 1e-8),
                 lambda: cg(A, T.astype(np.complex128), B, BtBinv, pattern, 4, 1e-8),
                 lambda: cg(A, T, B.astype(np.float32), BtBinv, pattern, 4, 1e-8),
                 lambda: cg(A, T, B, BtBinv.astype(np.complex128), pattern, 4, 1e-8),
                 lambda: cg(A.tocoo(), T, B, BtBinv, pattern, 4, 1e-8),
                 lambda: cg(A, T.toarray(), B, BtBinv, pattern, 4, 1e-8),
                 lambda: cg(A, T, B, BtBinv, pattern.tocsc(), 4, 1e-8),
                 lambda: cg(A, T, B, BtBinv, small, 4, 1e-8),                       # the pattern lost a block of T
                 lambda: cg(A, T, B, BtBinv, big, 4, 1e-8),
                 lambda: cg(A7, T7, np.ones((7, 1)), np.ones((2, 1, 1)), T7, 4, 1e-8),
                 lambda: cg(A, T, np.ones((B.shape[0], 7)), np.ones((A.shape[0] // 2, 7, 7)), pattern, 4, 1e-8)):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(ValueError, match="weighting value is invalid"):
        cg(A, T, B, BtBinv, pattern, 4, 1e-8, "nonsense")
    U = ec.sc_inputs("nd3")[0]
    for call in (lambda: en.satisfy_constraints(U.astype(np.complex128), B, BtBinv),
                 lambda: en.satisfy_constraints(U.tocsr(), B, BtBinv),
                 lambda: en.satisfy_constraints(U, np.ones((U.shape[1], 7)), BtBinv),
                 lambda: en.satisfy_constraints(T7, np.ones((7, 1)), np.ones((2, 1, 1)))):
        with pytest.raises(NotImplementedError):
            call()


def test_shapes_above_the_cap_are_refused_by_the_kernel_entries_too(emul):
    n = 4
    Sp, Sj = np.arange(n + 1, dtype=np.int32), np.zeros(n, dtype=np.int32)
    x = np.ones(n * 7 * 7)
    with pytest.raises(NotImplementedError):
        emul.incomplete_mat_mult_bsr(Sp, np.arange(n, dtype=np.int32), x.copy(), Sp, Sj, x.copy(), Sp, Sj, x, n, 1, 7, 7, 7)
    with pytest.raises(NotImplementedError):
        emul.satisfy_constraints_helper(2, 2, n, 7, np.ones(2 * 7), np.ones(n * 2 * 7), np.ones(n * 49), Sp, Sj, np.ones(n * 4))


TARGETS = ["cg_prolongation_smoothing", "satisfy_constraints"]


def test_device_setup_patches_and_restores_exactly_the_two_names(monkeypatch):
    import inspect
    from pyamg_amd import aggregation as agg
    assert inspect.signature(agg.device_setup).parameters["energy"].default is False
    mods = {}
    for name in ("standin_en", "standin_en.aggregation", "standin_en.aggregation.smooth", "standin_en.aggregation.aggregation"):
        m = types.ModuleType(name)
        mods[name] = m
        monkeypatch.setitem(sys.modules, name, m)
        if "." in name:
            setattr(mods[name.rsplit(".", 1)[0]], name.rsplit(".", 1)[1], m)
    smooth = mods["standin_en.aggregation.smooth"]
    originals = {}
    for fn in TARGETS + ["cgnr_prolongation_smoothing", "gmres_prolongation_smoothing", "energy_prolongation_smoother"]:
        def reference_fn(*a, _tag=fn, **k):
            return ("reference", _tag)
        reference_fn.__name__ = fn
        setattr(smooth, fn, reference_fn)
        originals[fn] = reference_fn
    pkg = mods["standin_en"]
    before = {name: dict(vars(m)) for name, m in mods.items()}
    for kw in ({}, {"energy": False}):
        with agg.device_setup(pkg, products=False, **kw):
            assert all(dict(vars(m)) == before[name] for name, m in mods.items())        # off by default: <pkg>.aggregation.smooth is left alone

    def device_fn(*a, **k):
        if a and a[0] == "refuse":
            raise NotImplementedError
        return ("device",)
    for fn in TARGETS:
        monkeypatch.setattr(en, fn, device_fn)
    with agg.device_setup(pkg, products=False, energy=True):
        changed = [(name, k) for name, m in mods.items() for k, v in vars(m).items() if before[name].get(k) is not v]
        assert sorted(changed) == sorted(("standin_en.aggregation.smooth", fn) for fn in TARGETS)
        for fn in TARGETS:
            patched = getattr(smooth, fn)
            assert patched is not originals[fn] and patched.__name__ == fn
            assert patched("x") == ("device",)
            assert patched("refuse") == ("reference", fn)    # not on the device path: the function that was patched out
    assert all(dict(vars(m)) == before[name] for name, m in mods.items())
    with pytest.raises(RuntimeError):
        with agg.device_setup(pkg, products=False, energy=True):
            raise RuntimeError("inside")
    assert all(dict(vars(m)) == before[name] for name, m in mods.items())


def test_device_setup_without_energy_does_not_import_the_module():
    code = ("import sys, types\n"
            "pkg = types.ModuleType('standin_en2')\n"
            "sys.modules['standin_en2'] = pkg\n"
            "from pyamg_amd import aggregation as agg\n"
            "with agg.device_setup(pkg, products=False): pass\n"
            "with agg.device_setup(pkg, products=False, energy=False): pass\n"
            "assert 'pyamg_amd.energy' not in sys.modules\n"
            "with agg.device_setup(pkg, products=False, energy=True): pass\n"
            "assert 'pyamg_amd.energy' in sys.modules\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(ROOT))
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


def e2e_solver(pyamg, A):
    return pyamg.rootnode_solver(A, strength="evolution", smooth=("energy", {"krylov": "cg", "maxiter": 4}), max_coarse=20)


def test_rootnode_hierarchy_under_device_setup_with_the_replay(emul, monkeypatch):
    """the end-to-end case of test_gpu_energy.py, with the replay in place of the device and the reference's own spectral radius,
    strength and tentative prolongator on both sides: the same level sizes (the aggregation is not on a tie), each P within the bar"""
    import oracle.refimport as ri
    if not ri.available():
        pytest.skip("oracle/_ref not present")
    import importlib
    import pyamg
    from pyamg_amd.aggregation import device_setup
    host_only = [(importlib.import_module(f"pyamg.{m}"), n) for m, n in (("aggregation.aggregation", "fit_candidates"),
                 ("aggregation.smooth", "approximate_spectral_radius"), ("relaxation.smoothing", "approximate_spectral_radius"),
                 ("relaxation.chebyshev", "approximate_spectral_radius"), ("util.linalg", "approximate_spectral_radius"))]
    host_only = [(m, n, getattr(m, n)) for m, n in host_only if hasattr(m, n)]
    A = sp.csr_array(ec.bsr("e2e.A"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        np.random.seed(7)
        want = e2e_solver(pyamg, A.copy())
        after_want = np.random.rand()
        np.random.seed(7)
        with device_setup(pyamg, prolongation=False, products=False, energy=True):
            for m, n, fn in host_only:
                setattr(m, n, fn)
            got = e2e_solver(pyamg, A.copy())
        after_got = np.random.rand()
    assert after_got == after_want                           # the same random draws were consumed
    assert "energy_cg" in emul.calls
    assert [lv.A.shape for lv in got.levels] == [lv.A.shape for lv in want.levels] and len(want.levels) >= 3
    for lg, lw in zip(got.levels[:-1], want.levels[:-1]):
        Pg, Pw = lg.P.toarray(), lw.P.toarray()
        assert np.abs(Pg - Pw).max() / np.abs(Pw).max() <= ec.BAR


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_c_abi_refuses_bad_arguments_before_anything_is_written():
    from pyamg_amd import _capi as capi
    lib = capi.load()
    p = capi.ptr
    A, T, B, BtBinv, pattern, kw = ec.cg_inputs("sa_elas")
    r, c = T.blocksize
    n, nbc, K = A.shape[0] // r, T.shape[1] // c, B.shape[1]
    Ap, Aj, Ax, Sp, Sj = A.indptr, A.indices, np.ravel(A.data), pattern.indptr, pattern.indices
    Tx = np.zeros(Sj.size * r * c)
    Bf, Zf, Dinv = np.ravel(B), np.ravel(BtBinv), np.ones(n * r)
    its, ns, sums = ctypes.c_int(0), ctypes.c_int(0), np.zeros(4)
    far = Sj.copy(); far[3] = nbc
    bad_start = Sp.copy(); bad_start[0] = 1

    def cg(n_=n, r_=r, K_=K, Sp_=Sp, Sj_=Sj, Tx_size=Tx.size, B_=Bf, cmask=None, PI=None, maxiter=4):
        return lib.pamg_energy_cg_f64(n_, nbc, r_, c, K_, p(Ap), Ap.size, p(Aj), Aj.size, p(Ax), Ax.size, p(Sp_), Sp_.size, p(Sj_), Sj_.size, p(Tx), Tx_size,
                                      p(B_), Bf.size, p(Zf), Zf.size, p(Dinv), Dinv.size, p(cmask), p(PI), maxiter, 1e-8, ctypes.byref(its), p(sums),
                                      ctypes.byref(ns))
    assert cg(n_=-1) == capi.E_ARG and cg(Sj_=far) == capi.E_ARG and cg(Sp_=bad_start) == capi.E_ARG and cg(Tx_size=Tx.size - 1) == capi.E_ARG
    assert cg(B_=None) == capi.E_ARG and cg(maxiter=-1) == capi.E_ARG and cg(r_=0) == capi.E_ARG
    assert cg(cmask=np.zeros(n * r, dtype=np.uint8)) == capi.E_ARG                      # a mask without the injection
    assert cg(K_=7) == capi.E_UNSUPPORTED and cg(r_=7) == capi.E_UNSUPPORTED
    Sx = np.full(Sj.size * r * c, 3.0)
    M = lib.pamg_incomplete_mat_mult_bsr_f64

    def imm(Sj_=Sj, Sx_size=Sx.size, rows=n, bs=r):
        return M(p(Ap), Ap.size, p(Aj), Aj.size, p(Ax), Ax.size, p(Sp), Sp.size, p(Sj), Sj.size, p(Tx), Tx.size, p(Sp), Sp.size, p(Sj_), Sj_.size,
                 p(Sx), Sx_size, rows, nbc, bs, r, c)
    assert imm(Sj_=far) == capi.E_ARG and imm(Sx_size=Sx.size - 1) == capi.E_ARG and imm(rows=-1) == capi.E_ARG and imm(bs=7) == capi.E_UNSUPPORTED
    H, S = lib.pamg_satisfy_constraints_helper_f64, lib.pamg_satisfy_constraints_f64
    UB = np.ones(n * r * K)
    assert H(r, c, n, K, p(Bf), Bf.size, p(UB), UB.size - 1, p(Zf), Zf.size, p(Sp), Sp.size, p(Sj), Sj.size, p(Sx), Sx.size) == capi.E_ARG
    assert H(r, c, n, K, p(Bf), Bf.size, p(UB), UB.size, p(Zf), Zf.size, p(Sp), Sp.size, p(far), Sj.size, p(Sx), Sx.size) == capi.E_ARG
    assert H(r, c, n, 7, p(Bf), Bf.size, p(UB), UB.size, p(Zf), Zf.size, p(Sp), Sp.size, p(Sj), Sj.size, p(Sx), Sx.size) == capi.E_UNSUPPORTED
    assert S(r, c, n, K, p(Bf), Bf.size, p(Zf), Zf.size - 1, p(Sp), Sp.size, p(Sj), Sj.size, p(Sx), Sx.size) == capi.E_ARG
    assert S(r, c, n, K, None, Bf.size, p(Zf), Zf.size, p(Sp), Sp.size, p(Sj), Sj.size, p(Sx), Sx.size) == capi.E_ARG
    assert np.all(Sx == 3.0) and not Tx.any() and not sums.any()                        # nothing was written


def test_standalone_program_under_the_sanitizers(tmp_path):
    """the replay as a program of its own (its main), built with -fsanitize=address,undefined: nothing sanitized is loaded into Python"""
    exe = tmp_path / "ene"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-DENE_MAIN", str(HERE / "energy_emul.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr.lower() + r.stdout.lower() and "cannot find" in r.stderr.lower():
        pytest.skip("no sanitizer runtime for g++ here")
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
