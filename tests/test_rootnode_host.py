"""The root-node setup pieces of pyamg_amd.rootnode without a GPU: tests/rootnode_emul.cpp compiles csrc/pamg_rootnode.h with the host
compiler and replays every kernel case of tests/golden/kernels_rootnode.npz.  calc_BtB, the one-candidate inverse, the 1 x 1 scale_T and
filter_operator (given the fixture's BtBinv) are held against the fixture with np.array_equal; the inverses of larger blocks with the
Schwarz setup's comparison (equal ranks, |X - X_ref|_F <= 64 eps kappa_+ |X_ref|_F).  Then the surface: the reference's errors,
NotImplementedError for what the device path does not take, device_setup(rootnode=True), the C ABI's refusals."""
import ctypes
import subprocess
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import rootnode_cases as rc
from pyamg_amd import rootnode as rn

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent


@pytest.fixture(scope="module")
def emul_lib():
    return rc.build_emul()


@pytest.fixture()
def emul(emul_lib, monkeypatch):
    core = rc.EmulCore(emul_lib)
    monkeypatch.setattr(rn, "amg_core", core)
    return core


# ------------------------------------------------------------------------------------------------ the replay against the fixture
def test_the_fixture_holds_the_cases_the_tests_name():
    d = rc.data()
    for key, names in (("btb.names", rc.BTB), ("st.names", rc.SCALE), ("fo.names", rc.FILTER), ("rx.names", rc.RELAX)):
        assert [str(s) for s in d[key]] == names
    for k in d:
        if k.endswith(".shape"):
            assert d[k][0] <= 300                            # every operator has at most 300 rows
    B, C, BtB, inv = rc.btb_inputs("crafted")
    rows = np.diff(C.indptr)
    assert rows[0] == 160 and rows[1] == 0 and C.shape[0] == 67 and B.shape[1] > 1
    assert np.unique(C.indices[C.indptr[2]:C.indptr[3]]).size == rows[2] - 1 and np.any(np.diff(C.indices[C.indptr[2]:C.indptr[3]]) < 0)
    assert not BtB[3].any() and not inv[3].any() and not inv[1].any()
    B, C, _, inv = rc.btb_inputs("k1")
    assert inv[5, 0, 0] == 0.0 and C.shape[0] == 67
    B, C, _, _ = rc.btb_inputs("k3")
    assert B.shape[1] > C.blocksize[1]
    B, _, _, _ = rc.btb_inputs("rankdef")
    assert np.array_equal(B[:, 2], B[:, 0])
    assert rc.scale_inputs("no_coarse")[1].nnz == 0


@pytest.mark.parametrize("name", rc.BTB)
def test_calc_BtB_replay_equals_the_reference(emul, name):
    got, want = rc.run_calc_BtB(emul, name)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", rc.BTB)
def test_compute_BtBinv_replay(emul, name):
    """the blocks before the inversion equal the reference's calc_BtB bit for bit although the products are formed from B; the inverse
    equals the reference's for one candidate and agrees within 64 eps kappa_+ otherwise, with equal ranks"""
    B, C, BtB, want = rc.btb_inputs(name)
    got = rn.compute_BtBinv(B, C)
    assert emul.calls == ["compute_BtBinv"] and got.shape == want.shape and got.dtype == np.float64
    K = B.shape[1]
    r, c = C.blocksize if C.format == "bsr" else (1, 1)
    before, again = np.zeros(want.size), np.zeros(want.size)
    emul.compute_BtBinv(K, want.shape[0], c, np.ravel(B), C.indptr.astype(np.int32), C.indices.astype(np.int32), again, BtB=before)
    assert np.array_equal(before.reshape(BtB.shape), BtB) and np.array_equal(again.reshape(got.shape), got)
    rc.inverse_check(name, got)


@pytest.mark.parametrize("name", rc.SCALE)
def test_scale_T_replay(emul, name):
    T, P_I, I_F, want = rc.scale_inputs(name)
    keep = T.copy()
    got = rn.scale_T(T, P_I, I_F)
    if name == "no_coarse":
        assert got is T and emul.calls == []                 # the reference's early exit
    else:
        assert emul.calls == ["scale_T"]
        roots = np.flatnonzero(np.diff(P_I.indptr))
        bs = T.blocksize[0]
        assert all(np.array_equal(got.data[got.indptr[r]], np.eye(bs)) and got.indptr[r + 1] - got.indptr[r] == 1 for r in roots)
    assert rc.same_matrix(T, keep)                           # the argument is left alone, as by the reference
    rc.scale_check(name, got)


def test_scale_T_drops_the_blocks_scipy_would_not_store(emul):
    T, P_I, I_F, _ = rc.scale_inputs("rn_elas")
    frow = int(np.flatnonzero(np.diff(P_I.indptr) == 0)[0])
    T.data[T.indptr[frow]] = 0.0
    got = rn.scale_T(T, P_I, I_F)
    assert got.indptr[frow + 1] == got.indptr[frow] and got.indices.size == T.indices.size - 1


@pytest.mark.parametrize("name", rc.FILTER)
def test_filter_operator_replay_equals_the_reference(emul, name):
    A, C, B, Bf, BtBinv, want = rc.filter_inputs(name)
    got = rn.filter_operator(A, C, B, Bf, BtBinv)
    assert emul.calls == ["filter_constraints"]
    assert rc.same_matrix(got, want)
    assert np.abs(got @ B - Bf).max() <= 1e-12 * max(1.0, np.abs(Bf).max())
    emul.calls.clear()
    again = rn.filter_operator(A, C, B, Bf)                  # BtBinv computed on the way
    assert emul.calls == ["compute_BtBinv", "filter_constraints"]
    assert np.abs(again.toarray() - want.toarray()).max() <= rc.BAR * np.abs(want.toarray()).max()


def test_filter_operator_takes_csr_and_a_shuffled_pattern(emul):
    """1 x 1 blocks stored as CSR, C's rows in shuffled order, A with entries outside C: the result has C's sorted structure"""
    rng = np.random.default_rng(5)
    C = sp.csr_array((rng.random((30, 12)) < 0.4).astype(float))
    A = sp.csr_array((rng.random((30, 12)) < 0.4) * rng.standard_normal((30, 12)))
    C.sort_indices(), A.sort_indices()
    B, Bf = rng.standard_normal((12, 2)), rng.standard_normal((30, 2))
    BtBinv = np.zeros((30, 2, 2))
    for i in range(30):
        Bi = B[C.indices[C.indptr[i]:C.indptr[i + 1]]]
        BtBinv[i] = np.linalg.pinv(Bi.T @ Bi)
    want = rn.filter_operator(A, C, B, Bf, BtBinv)
    Cs = C.copy()
    for i in range(30):
        lo, hi = Cs.indptr[i], Cs.indptr[i + 1]
        Cs.indices[lo:hi] = Cs.indices[lo:hi][rng.permutation(hi - lo)]
    got = rn.filter_operator(A, Cs, B, Bf, BtBinv)
    assert got.format == "csr" and rc.same_matrix(got, want)
    inside = C.toarray() != 0
    assert not np.any(got.toarray()[~inside])
    full = np.flatnonzero(np.diff(C.indptr) >= 2)            # two candidates need two neighbours to be met exactly
    assert np.abs((got @ B - Bf)[full]).max() <= 1e-10


# ------------------------------------------------------------------------------------------------ the surface
def _boom(*a, **k):
    raise AssertionError("a device call was made")


@pytest.fixture()
def nodevice(monkeypatch):
    monkeypatch.setattr(rn, "amg_core", types.SimpleNamespace(**{n: _boom for n in rc.NAMES}))


def test_the_reference_s_errors(nodevice):
    B, C, _, _ = rc.btb_inputs("k3")
    with pytest.raises(TypeError, match="Expected bsr_array or csr_array for C"):
        rn.compute_BtBinv(B, C.tocsc())
    with pytest.raises(TypeError, match="Expected matching dimensions"):
        rn.compute_BtBinv(B[:-1], C)
    T, P_I, I_F, _ = rc.scale_inputs("rn_elas")
    with pytest.raises(TypeError, match="Expected BSR matrix T"):
        rn.scale_T(T.tocsr(), P_I, I_F)
    with pytest.raises(TypeError, match="Expected BSR matrix P_I"):
        rn.scale_T(T, P_I.tocsr(), I_F)
    with pytest.raises(TypeError, match="square blocks"):
        rn.scale_T(sp.bsr_array(T.tocsr(), blocksize=(2, 1)), P_I, I_F)
    with pytest.raises(TypeError, match="identical blocksize"):
        rn.scale_T(T, P_I, sp.bsr_array(I_F.tocsr(), blocksize=(1, 1)))
    A, C, B, Bf, BtBinv, _ = rc.filter_inputs("rn_elas")
    with pytest.raises(ValueError, match="same size"):
        rn.filter_operator(sp.bsr_array(A.tocsr()[:-2], blocksize=(2, 2)), C, B, Bf, BtBinv)
    with pytest.raises(ValueError, match="both be CSR or BSR"):
        rn.filter_operator(A.tocsr(), C, B, Bf, BtBinv)
    with pytest.raises(ValueError, match="same BSR blocksizes"):
        rn.filter_operator(sp.bsr_array(A.tocsr(), blocksize=(1, 1)), C, B, Bf, BtBinv)
    with pytest.raises(ValueError, match="same first dimension"):
        rn.filter_operator(A, C, B, Bf[:-1], BtBinv)
    with pytest.raises(ValueError, match="same second"):
        rn.filter_operator(A, C, B, Bf[:, :2], BtBinv)


def test_what_the_device_path_does_not_take_says_so_before_a_device_call(nodevice):
    B, C, _, _ = rc.btb_inputs("k3")
    big = C.copy()
    big.indices = big.indices.astype(np.int64)
    big.indices[-1] = 2**31 + 5
    C7 = sp.bsr_array(np.ones((14, 14)), blocksize=(7, 7))
    T, P_I, I_F, _ = rc.scale_inputs("rn_elas")
    shuffled = sp.bsr_array((np.ones((2, 2, 2)), np.array([1, 0], dtype=np.int32), np.array([0, 2] + [2] * (T.shape[0] // 2 - 1), dtype=np.int32)), shape=T.shape)
    notinj = P_I.copy()
    notinj.data = notinj.data * 2.0
    A, Cp, Bc, Bf, BtBinv, _ = rc.filter_inputs("rn_elas")
    dup = Cp.copy()
    dup.indices = dup.indices.copy()
    lo = dup.indptr[int(np.flatnonzero(np.diff(dup.indptr) >= 2)[0])]
    dup.indices[lo + 1] = dup.indices[lo]
    for call in (lambda: rn.compute_BtBinv(B.astype(np.float32), C),
                 lambda: rn.compute_BtBinv(B.astype(np.complex128), C),
                 lambda: rn.compute_BtBinv(np.ones((C.shape[1], 7)), C),
                 lambda: rn.compute_BtBinv(np.ones((14, 2)), C7),
                 lambda: rn.compute_BtBinv(B, big),
                 lambda: rn.scale_T(T.astype(np.float32), P_I, I_F),
                 lambda: rn.scale_T(T.astype(np.complex128), P_I, I_F),
                 lambda: rn.scale_T(shuffled, P_I, I_F),
                 lambda: rn.scale_T(T, notinj, I_F),
                 lambda: rn.scale_T(T, P_I, sp.bsr_array(sp.eye_array(T.shape[0], format="csr"), blocksize=(2, 2))),
                 lambda: rn.scale_T(C7, C7, C7),
                 lambda: rn.filter_operator(A.astype(np.float32), Cp, Bc, Bf, BtBinv),
                 lambda: rn.filter_operator(A, Cp, Bc.astype(np.complex128), Bf.astype(np.complex128), BtBinv),
                 lambda: rn.filter_operator(A, dup, Bc, Bf, BtBinv),
                 lambda: rn.filter_operator(A, Cp, np.ones((Bc.shape[0], 7)), np.ones((Bf.shape[0], 7)), None)):
        with pytest.raises(NotImplementedError):
            call()


def test_relaxation_refuses_before_the_smoother_is_set_up():
    """what is not taken is refused before the caller's package sets the smoother up, so nothing was drawn when the reference takes over"""
    boom = types.ModuleType("standin_rx_boom")                # importing <boom>.relaxation.smoothing would fail loudly
    A = sp.csr_array(sp.eye_array(6, format="csr"))
    b = np.zeros((6, 1))
    state = np.random.get_state()[1].copy()
    for call in (lambda: rn.relaxation_as_linear_operator("schwarz", A, b, pyamg=boom),
                 lambda: rn.relaxation_as_linear_operator(("gauss_seidel_ne", {}), A, b, pyamg=boom),
                 lambda: rn.relaxation_as_linear_operator("richardson", A, b, pyamg=boom),
                 lambda: rn.relaxation_as_linear_operator("gauss_seidel", A.astype(np.float32), b, pyamg=boom),
                 lambda: rn.relaxation_as_linear_operator("gauss_seidel", A.astype(np.complex128), b, pyamg=boom),
                 lambda: rn.relaxation_as_linear_operator("gauss_seidel", A.tocsc(), b, pyamg=boom),
                 lambda: rn.relaxation_as_linear_operator("jacobi", sp.bsr_array(np.eye(14), blocksize=(7, 7)), np.zeros(14), pyamg=boom),
                 lambda: rn.relaxation_as_linear_operator(("block_jacobi", {"blocksize": 2}), A, b, pyamg=boom),
                 lambda: rn.relaxation_as_linear_operator(("block_gauss_seidel", {"Dinv": np.ones((6, 1, 1))}), A, b, pyamg=boom)):
        with pytest.raises(NotImplementedError):
            call()
    assert np.array_equal(np.random.get_state()[1], state)


def test_relaxation_reads_the_reference_s_own_parameters_back(monkeypatch):
    """with the reference as the caller's package: the smoother it set up arrives at the device operator as kind, sweep, iterations,
    omega and its own block-diagonal inverse, never recomputed"""
    import oracle.refimport as ri
    if not ri.available():
        pytest.skip("oracle/_ref not present")
    import pyamg
    from pyamg.util.utils import get_block_diag
    seen = []
    monkeypatch.setattr(rn, "_DeviceRelaxation", lambda A, b, spec: seen.append((A, b, spec)) or "op")
    want = {"gs_aniso": ("gauss_seidel", "symmetric", 4, 1.0), "bgs_elas": ("block_gauss_seidel", "symmetric", 4, 1.0),
            "jacobi_poisson": ("jacobi", "forward", 2, 2.0 / 3.0)}
    for name in rc.RELAX:
        method, A, B, _ = rc.relax_inputs(name)
        assert rn.relaxation_as_linear_operator(method, A, np.zeros((A.shape[0], 1)), pyamg=pyamg) == "op"
        A_, b, spec = seen[-1]
        assert A_ is A and b.shape == (A.shape[0], 1) and b.dtype == np.float64
        assert (spec.kind, spec.sweep, spec.iterations, spec.omega) == want[name]
        if name == "bgs_elas":
            assert spec.blocksize == 2 and np.array_equal(spec.Dinv, get_block_diag(A, blocksize=2, inv_flag=True))
        else:
            assert spec.Dinv is None
    A = rc.relax_inputs("gs_aniso")[1]
    rn.relaxation_as_linear_operator(("block_gauss_seidel", {"sweep": "symmetric", "iterations": 4}), A, np.zeros(A.shape[0]), pyamg=pyamg)
    assert seen[-1][2].kind == "gauss_seidel" and seen[-1][2].iterations == 4      # 1 x 1 blocks: the reference substitutes the point method


def test_shapes_above_the_cap_are_refused_by_the_kernel_entries_too(emul):
    n = 4
    Sp, Sj = np.arange(n + 1, dtype=np.int32), np.zeros(n, dtype=np.int32)
    with pytest.raises(NotImplementedError):
        emul.calc_BtB(7, n, 1, np.ones(28), 28, np.zeros(n * 49), Sp, Sj)
    with pytest.raises(NotImplementedError):
        emul.compute_BtBinv(2, n, 7, np.ones(14), Sp, Sj, np.zeros(n * 4))
    with pytest.raises(NotImplementedError):
        emul.scale_T(n, 1, 7, Sp, Sj, np.ones(n * 49), np.zeros(1, dtype=np.int32))
    with pytest.raises(NotImplementedError):                 # a root row that holds a second block
        emul.scale_T(2, 2, 1, np.array([0, 2, 3], dtype=np.int32), np.array([0, 1, 1], dtype=np.int32), np.ones(3), np.array([0, 1], dtype=np.int32))


# what rootnode=True binds: (module, name) -> through _device_or_reference (True) or directly (False)
TABLE = {("aggregation.smooth", "compute_BtBinv"): True, ("util.utils", "compute_BtBinv"): True, ("aggregation.smooth", "filter_operator"): True,
         ("aggregation.rootnode", "scale_T"): True, ("aggregation.rootnode", "relaxation_as_linear_operator"): True,
         ("aggregation.aggregation", "relaxation_as_linear_operator"): True, ("aggregation.rootnode", "fit_candidates"): True,
         ("aggregation.rootnode", "symmetric_strength_of_connection"): False}
WITH_AGGREGATION = {("aggregation.rootnode", "standard_aggregation"): True}
BYSTANDERS = [("util.utils", "scale_T"), ("util.utils", "filter_operator"), ("util.utils", "get_Cpt_params"), ("aggregation.smooth", "get_Cpt_params"),
              ("aggregation.rootnode", "get_Cpt_params"), ("aggregation.smooth", "cgnr_prolongation_smoothing"), ("util.utils", "truncate_rows"),
              ("util.utils", "filter_matrix_rows"), ("util.utils", "filter_matrix_columns"), ("aggregation.rootnode", "energy_prolongation_smoother"),
              ("relaxation.utils", "relaxation_as_linear_operator")]


def _standin(monkeypatch, root):
    mods = {}
    for sub in ("", ".aggregation", ".aggregation.smooth", ".aggregation.aggregation", ".aggregation.rootnode", ".util", ".util.utils", ".relaxation",
                ".relaxation.utils"):
        name = root + sub
        m = types.ModuleType(name)
        mods[name] = m
        monkeypatch.setitem(sys.modules, name, m)
        if sub:
            setattr(mods[name.rsplit(".", 1)[0]], name.rsplit(".", 1)[1], m)
    originals = {}
    for mod, fn in list(TABLE) + list(WITH_AGGREGATION) + BYSTANDERS:
        def reference_fn(*a, _tag=(mod, fn), **k):
            return ("reference",) + _tag
        reference_fn.__name__ = fn
        setattr(mods[f"{root}.{mod}"], fn, reference_fn)
        originals[(mod, fn)] = reference_fn
    return mods, originals


def test_device_setup_patches_and_restores_exactly_the_table(monkeypatch):
    import inspect
    from pyamg_amd import aggregation as agg
    assert inspect.signature(agg.device_setup).parameters["rootnode"].default is False
    root = "standin_rn"
    mods, originals = _standin(monkeypatch, root)
    pkg = mods[root]
    before = {name: dict(vars(m)) for name, m in mods.items()}

    def changed():
        return sorted((name[len(root) + 1:], k) for name, m in mods.items() for k, v in vars(m).items() if before[name].get(k) is not v)
    for kw in ({}, {"rootnode": False}, {"rootnode": False, "aggregation": True, "energy": True}):
        with agg.device_setup(pkg, products=False, **kw):
            assert changed() == []                           # rootnode=False binds nothing new: none of these names is patched by another keyword

    def device_fn(*a, **k):
        if a and a[0] == "refuse":
            raise NotImplementedError
        return ("device",)
    for fn in ("compute_BtBinv", "filter_operator", "scale_T", "relaxation_as_linear_operator"):
        monkeypatch.setattr(rn, fn, device_fn)
    for fn in ("fit_candidates", "standard_aggregation"):
        monkeypatch.setattr(agg, fn, device_fn)
    for kw, table in (({}, TABLE), ({"aggregation": True}, {**TABLE, **WITH_AGGREGATION})):
        with agg.device_setup(pkg, products=False, rootnode=True, **kw):
            assert changed() == sorted(table)
            for (mod, fn), wrapped in table.items():
                patched = getattr(mods[f"{root}.{mod}"], fn)
                if not wrapped:
                    assert patched is getattr(agg, fn)
                    continue
                assert patched is not originals[(mod, fn)] and patched.__name__ == fn
                assert patched("x") == ("device",)
                assert patched("refuse") == ("reference", mod, fn)      # not on the device path: the function that was patched out
        assert changed() == []
    with pytest.raises(RuntimeError):
        with agg.device_setup(pkg, products=False, rootnode=True):
            raise RuntimeError("inside")
    assert changed() == []


def test_the_patched_relaxation_is_bound_to_the_caller_s_package(monkeypatch):
    from pyamg_amd import aggregation as agg
    mods, _ = _standin(monkeypatch, "standin_rn3")
    seen = []
    monkeypatch.setattr(rn, "relaxation_as_linear_operator", lambda method, A, b, pyamg=None: seen.append(pyamg) or "op")
    with agg.device_setup(mods["standin_rn3"], products=False, rootnode=True):
        assert mods["standin_rn3.aggregation.rootnode"].relaxation_as_linear_operator("gauss_seidel", None, None) == "op"
    assert seen == [mods["standin_rn3"]]


def test_device_setup_without_rootnode_does_not_import_the_module():
    code = ("import sys, types\n"
            "pkg = types.ModuleType('standin_rn2')\n"
            "sys.modules['standin_rn2'] = pkg\n"
            "from pyamg_amd import aggregation as agg\n"
            "with agg.device_setup(pkg, products=False): pass\n"
            "with agg.device_setup(pkg, products=False, rootnode=False, energy=True): pass\n"
            "assert 'pyamg_amd.rootnode' not in sys.modules\n"
            "with agg.device_setup(pkg, products=False, rootnode=True): pass\n"
            "assert 'pyamg_amd.rootnode' in sys.modules\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(ROOT))
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


@pytest.mark.parametrize("name", ["diffusion", "elasticity"])
def test_rootnode_hierarchy_under_device_setup_with_the_replay(emul, monkeypatch, name):
    """the end-to-end cases of test_gpu_rootnode.py with the replay in place of the device for compute_BtBinv, scale_T and
    filter_operator; the candidate relaxation (the resident engine's sweeps, no replay) and everything else that needs a device is
    handed back to the reference: the same random draws, the same level sizes, each P within the bar"""
    import oracle.refimport as ri
    if not ri.available():
        pytest.skip("oracle/_ref not present")
    import importlib
    import warnings
    import pyamg
    from pyamg_amd.aggregation import device_setup

    def refuse(*a, **k):
        raise NotImplementedError
    monkeypatch.setattr(rn, "relaxation_as_linear_operator", refuse)
    host_only = [(importlib.import_module(f"pyamg.{m}"), n) for m, n in (("aggregation.aggregation", "fit_candidates"),
                 ("aggregation.rootnode", "fit_candidates"), ("aggregation.rootnode", "symmetric_strength_of_connection"),
                 ("aggregation.aggregation", "symmetric_strength_of_connection"), ("strength", "symmetric_strength_of_connection"),
                 ("aggregation.smooth", "approximate_spectral_radius"), ("relaxation.smoothing", "approximate_spectral_radius"),
                 ("relaxation.chebyshev", "approximate_spectral_radius"), ("util.linalg", "approximate_spectral_radius"))]
    host_only = [(m, n, getattr(m, n)) for m, n in host_only if hasattr(m, n)]
    A, B = rc.e2e_operators()[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        np.random.seed(7)
        want = rc.e2e_solver(pyamg, A.copy(), None if B is None else B.copy())
        after_want = np.random.rand()
        np.random.seed(7)
        with device_setup(pyamg, prolongation=False, products=False, rootnode=True):
            for m, n, fn in host_only:
                setattr(m, n, fn)
            got = rc.e2e_solver(pyamg, A.copy(), None if B is None else B.copy())
        after_got = np.random.rand()
    assert after_got == after_want                           # the same random draws were consumed
    levels = len(want.levels)
    assert emul.calls.count("scale_T") == levels - 1 and emul.calls.count("compute_BtBinv") >= levels - 1
    assert ("filter_constraints" in emul.calls) == (name == "elasticity")
    assert [lv.A.shape for lv in got.levels] == [lv.A.shape for lv in want.levels] and levels >= 2
    for lg, lw in zip(got.levels[:-1], want.levels[:-1]):
        Pg, Pw = lg.P.toarray(), lw.P.toarray()
        err = np.abs(Pg - Pw).max() / np.abs(Pw).max()
        print(f"[rootnode] {name} (replay): level {lg.A.shape}, |P - P_ref| / max|P_ref| = {err:.2e}")
        assert err <= rc.BAR


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_c_abi_refuses_bad_arguments_before_anything_is_written():
    from pyamg_amd import _capi as capi
    lib = capi.load()
    p = capi.ptr
    B, C, _, _ = rc.btb_inputs("k3")
    K, c = B.shape[1], C.blocksize[1]
    n, cols = C.shape[0] // C.blocksize[0], K * (K + 1) // 2
    Sp, Sj = C.indptr.astype(np.int32), C.indices.astype(np.int32)
    bq, Bf = np.ravel(rc.bsq(B)), np.ravel(B)
    x = np.full(n * K * K, 3.0)
    far = Sj.copy(); far[2] = C.shape[1] // c
    bad_start = Sp.copy(); bad_start[0] = 1

    def btb(K_=K, n_=n, c_=c, b=bq, cols_=cols, x_size=x.size, Sp_=Sp, Sj_=Sj):
        return lib.pamg_calc_BtB_f64(K_, n_, c_, p(b), bq.size, cols_, p(x), x_size, p(Sp_), Sp_.size, p(Sj_), Sj_.size)
    assert btb(n_=-1) == capi.E_ARG and btb(Sj_=far) == capi.E_ARG and btb(Sp_=bad_start) == capi.E_ARG and btb(x_size=x.size - 1) == capi.E_ARG
    assert btb(b=None) == capi.E_ARG and btb(cols_=cols + 1) == capi.E_ARG and btb(K_=0) == capi.E_ARG and btb(c_=0) == capi.E_ARG
    assert btb(K_=7, cols_=28) == capi.E_UNSUPPORTED and btb(c_=7) == capi.E_UNSUPPORTED

    def inv(K_=K, n_=n, c_=c, B_=Bf, out_size=x.size, Sj_=Sj):
        return lib.pamg_compute_BtBinv_f64(K_, n_, c_, p(B_), ctypes.c_int64(Bf.size), p(Sp), Sp.size, p(Sj_), Sj_.size, p(x), ctypes.c_int64(out_size))
    assert inv(n_=-1) == capi.E_ARG and inv(Sj_=far) == capi.E_ARG and inv(out_size=x.size - 1) == capi.E_ARG and inv(B_=None) == capi.E_ARG
    assert inv(c_=7) == capi.E_UNSUPPORTED
    T, P_I, I_F, _ = rc.scale_inputs("rn_elas")
    nb, nagg = T.shape[0] // 2, T.shape[1] // 2
    Tx = np.ravel(T.data).copy()
    keep = Tx.copy()
    Cn = np.zeros(nagg, dtype=np.int32)
    Cn[P_I.indices] = np.flatnonzero(np.diff(P_I.indptr))
    twice = Cn.copy(); twice[1] = twice[0]
    assert np.all(np.diff(T.indptr) == 1)
    away = Cn.copy(); away[0] = int(np.flatnonzero((T.indices != 0) & (np.diff(P_I.indptr) == 0))[0])      # a row of another aggregate

    def scale(n_=nb, bs=2, Tx_size=Tx.size, Cn_=Cn, Cn_size=nagg):
        return lib.pamg_scale_T_f64(n_, nagg, bs, p(T.indptr), T.indptr.size, p(T.indices), T.indices.size, p(Tx), ctypes.c_int64(Tx_size), p(Cn_), Cn_size)
    assert scale(n_=-1) == capi.E_ARG and scale(Tx_size=Tx.size - 1) == capi.E_ARG and scale(Cn_=twice) == capi.E_ARG and scale(Cn_size=nagg - 1) == capi.E_ARG
    assert scale(bs=7) == capi.E_UNSUPPORTED and scale(Cn_=away) == capi.E_UNSUPPORTED     # a root row that does not hold its aggregate's block
    A, Cp, Bc, Bff, BtBinv, _ = rc.filter_inputs("rn_elas")
    Sx = np.full(Cp.indices.size * 4, 3.0)
    b1, b2, z = np.ravel(Bc), np.ravel(Bff), np.ravel(BtBinv)

    def filt(r=2, K_=3, Bf_size=b2.size, z_size=z.size, Sx_size=Sx.size):
        return lib.pamg_filter_constraints_f64(r, 2, A.shape[0] // 2, K_, p(b1), b1.size, p(b2), Bf_size, p(z), z_size, p(Cp.indptr), Cp.indptr.size,
                                               p(Cp.indices), Cp.indices.size, p(Sx), Sx_size)
    assert filt(Bf_size=b2.size - 1) == capi.E_ARG and filt(z_size=z.size - 1) == capi.E_ARG and filt(Sx_size=Sx.size - 1) == capi.E_ARG and filt(r=0) == capi.E_ARG
    assert filt(K_=7) == capi.E_UNSUPPORTED and filt(r=7) == capi.E_UNSUPPORTED
    assert np.all(x == 3.0) and np.all(Sx == 3.0) and np.array_equal(Tx, keep)          # nothing was written
