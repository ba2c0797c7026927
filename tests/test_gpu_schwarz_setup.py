"""The Schwarz setup on the device (pamg_schwarz_setup.hip) against the reference's blocks in the committed fixtures: extraction bit for
bit through Layer 1 and Layer 2, pseudo-inverses within |X - X_ref|_F <= 64 eps kappa_+(B) |X_ref|_F with the reference's rank
(tests/schwarz_setup_cases.py), the existing sweep fed with device-built blocks, DeviceMultilevelSolver(schwarz_setup='device'), and
the cap of 64 rows.  Every operator is fixture-sized (at most 400 rows)."""
import ctypes as C
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import schwarz_setup_cases as sc
from pyamg_amd import DeviceMultilevelSolver
from pyamg_amd import _capi as capi
from pyamg_amd import relaxation as grelax
from pyamg_amd.hierarchy import sparse_op
from pyamg_amd.multilevel import DeviceMatrix

pytestmark = pytest.mark.gpu


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


@pytest.mark.parametrize("name", sc.ALL)
def test_extraction_bit_for_bit_layer1_and_layer2(name):
    import pyamg_amd.amg_core as gcore
    c = sc.cases()[name]
    A = c.A
    Ap, Aj, Ax = i32(A.indptr), i32(A.indices), np.ascontiguousarray(A.data)
    # Layer 1: amg_core's argument order, the caller's Tp; Tx is cleared up to Tp[nsub]
    Tx = np.full(c.tptr[-1], 3.0, dtype=c.dtype)
    gcore.extract_subblocks(Ap, Aj, Ax, Tx, c.tptr, c.sub, c.sptr, c.sptr.size - 1, A.shape[0])
    assert np.array_equal(Tx, c.blocks)
    from pyamg_amd import _amg_core_pybind as pb                   # the pybind11 face of the same entry point
    Tx = np.full(c.tptr[-1], 3.0, dtype=c.dtype)
    pb.extract_subblocks(Ap, Aj, Ax, Tx, c.tptr, c.sub, c.sptr, c.sptr.size - 1, A.shape[0])
    assert np.array_equal(Tx, c.blocks)
    # Layer 2 on device arrays, invert = 0
    dA = DeviceMatrix(sparse_op(A))
    dSp, dSj = capi.DeviceArray.from_host(c.sptr), capi.DeviceArray.from_host(c.sub)
    dTp, dTx = capi.DeviceArray(c.sptr.size, np.int32), capi.DeviceArray.from_host(np.full(int(c.tptr[-1]) + 5, 3.0, dtype=c.dtype))
    info = (C.c_int64 * 4)()
    capi.check(capi.lib().pamg_dev_schwarz_blocks(capi.dtype_code(c.dtype), dA.handle, c.sptr.size - 1, dSp.ptr, dSj.ptr, dTp.ptr, dTx.ptr,
                                                  int(c.tptr[-1]) + 5, 0.0, 0, None, info), "pamg_dev_schwarz_blocks")
    got = dTx.download()
    assert np.array_equal(dTp.download(), c.tptr)
    assert np.array_equal(got[:c.tptr[-1]], c.blocks) and np.all(got[c.tptr[-1]:] == 3.0)
    assert list(info) == [c.tptr[-1], np.diff(c.sptr).max(), 0, 0]
    for d in (dSp, dSj, dTp, dTx):
        d.free()
    dA.free()


@pytest.mark.parametrize("name", sc.KERNEL_OPS + sc.SETUP_INVERTED)
def test_schwarz_parameters_on_the_device_within_the_bound(name):
    c = sc.cases()[name]
    A = c.A.copy()
    sub, sptr, inv, iptr = grelax.schwarz_parameters(A, c.sub.copy(), c.sptr.copy(), device=True)
    assert np.array_equal(sub, c.sub) and np.array_equal(sptr, c.sptr)
    assert iptr.dtype == A.indices.dtype and np.array_equal(iptr, c.tptr)
    assert inv.dtype == c.dtype and inv.shape == c.inv.shape
    worst, truncated = sc.compare_blocks(c, inv)
    rep = A.schwarz_setup_report
    print(f"{name}: err / (eps kappa+) = {worst:.2f}, report {rep}")
    assert worst <= sc.BOUND, (name, worst)
    assert rep["path"] == "device" and rep["on_host"] == 0
    assert rep["largest"] == np.diff(c.sptr).max() and rep["entries"] == c.tptr[-1]
    assert rep["truncated"] == truncated == (len(sc.CHAINS) if name.startswith("chain_") else 0)
    assert 0 <= rep["sweeps"] <= 60
    assert grelax.schwarz_parameters(A, c.sub, c.sptr, device=True)[2] is inv           # cached like the host result


@pytest.mark.parametrize("name", ["irr_float64", "irr_float32", "pois_float64", "pois_float32"])
def test_sweeps_with_device_built_blocks_match_the_golden_iterates(name):
    """the bit-exact device sweep fed with device-built blocks: relative 2-norm of the difference to the reference's iterates
    <= 64 eps(dtype)"""
    import pyamg_amd.amg_core as gcore
    z = np.load(sc.GOLDEN / "kernels_schwarz.npz")
    c = sc.cases()[name]
    x, b = z[f"{name}.x"], z[f"{name}.b"]
    bound = 64 * float(np.finfo(c.dtype).eps)
    worst = 0.0
    M = c.A.copy()
    for sweep in ("forward", "backward", "symmetric"):
        y = x.copy()
        grelax.schwarz(M, y, b, iterations=2, sweep=sweep, device=True)
        want = z[f"{name}.{sweep}"]
        worst = max(worst, float(np.linalg.norm(y.astype(np.float64) - want) / np.linalg.norm(want)))
    assert M.schwarz_setup_report["path"] == "device"
    sub, sptr, inv, iptr = M.schwarz_parameters
    y = x.copy()
    n = M.shape[0]
    gcore.overlapping_schwarz_csr(i32(M.indptr), i32(M.indices), M.data, y, b, inv, i32(iptr), i32(sub), i32(sptr), len(sptr) - 1, n, 3, n - 1, 2)
    want = z[f"{name}.strided"]
    worst = max(worst, float(np.linalg.norm(y.astype(np.float64) - want) / np.linalg.norm(want)))
    print(f"{name}: worst iterate difference {worst / float(np.finfo(c.dtype).eps):.2f} eps")
    assert worst <= bound, (name, worst / float(np.finfo(c.dtype).eps))


@pytest.mark.parametrize("hier", ["sa2d_schwarz", "sa2d_sbschwarz"])
@pytest.mark.parametrize("graph", [True, False])
def test_solver_with_device_built_blocks_matches_the_reference_record(load_hier, hier, graph):
    spec, ex = load_hier(hier)
    k, cycle = int(ex["k"]), str(ex["cycle"])
    dml = DeviceMultilevelSolver(spec, graph=graph, schwarz_setup="device")
    resz = []
    xz = dml.solve(np.zeros_like(ex["x0z"]), x0=ex["x0z"], tol=1e-30, maxiter=k, cycle=cycle, residuals=resz)
    resz = np.array(resz)
    assert resz.shape == ex["resz"].shape
    assert np.max(np.abs(resz - ex["resz"]) / ex["resz"]) <= 1e-10
    res = []
    x, info = dml.solve(ex["b"], x0=ex["x0"], tol=1e-30, maxiter=k, cycle=cycle, residuals=res, return_info=True)
    res = np.array(res)
    assert info == k and len(res) == k + 1
    assert np.max(np.abs(res - ex["res"])) <= 1e-10 * ex["res"][0]
    assert np.linalg.norm(x - ex["x"]) <= 1e-12 * np.linalg.norm(ex["x"])
    assert np.linalg.norm(xz - ex["xz"]) <= 1e-12 * max(np.linalg.norm(ex["xz"]), 1e-300) + 1e-300
    st = dml.stats()["schwarz_setup"]
    assert sorted(st) == [0, 1]
    for lvl in (0, 1):
        for which in ("pre", "post"):
            r = st[lvl][which]
            assert r["path"] == "device" and r["on_host"] == 0 and r["largest"] <= 64 and r["truncated"] == 0 and r["sweeps"] >= 1
    # schwarz_setup='reference' is the solver as it was: the same bits as one built without the argument
    ref, old = DeviceMultilevelSolver(spec, graph=graph, schwarz_setup="reference"), DeviceMultilevelSolver(spec, graph=graph)
    r1, r2 = [], []
    x1 = ref.solve(ex["b"], x0=ex["x0"], tol=1e-30, maxiter=k, cycle=cycle, residuals=r1)
    x2 = old.solve(ex["b"], x0=ex["x0"], tol=1e-30, maxiter=k, cycle=cycle, residuals=r2)
    assert np.array_equal(x1, x2) and np.array_equal(r1, r2)
    assert all(r["path"] == "reference" for lv in ref.stats()["schwarz_setup"].values() for r in lv.values())
    with pytest.raises(ValueError):
        DeviceMultilevelSolver(spec, schwarz_setup="gpu")
    for s in (dml, ref, old):
        s.free()


def test_a_subdomain_of_65_rows_is_refused_and_the_wrapper_hands_it_to_the_host():
    rng = np.random.RandomState(4)
    n = 90
    A = sp.csr_array(sp.random(n, n, density=0.2, random_state=rng, format="csr") + 8.0 * sp.eye_array(n))
    A.sort_indices()
    lists = [np.arange(65), np.arange(70, 76), np.array([3, 80, 81])]
    sptr = i32(np.concatenate([[0], np.cumsum([len(x) for x in lists])]))
    sub = i32(np.concatenate(lists))
    total = int(np.sum(np.diff(sptr).astype(np.int64) ** 2))
    dA = DeviceMatrix(sparse_op(A))
    dSp, dSj = capi.DeviceArray.from_host(sptr), capi.DeviceArray.from_host(sub)
    dTp, dTx = capi.DeviceArray.from_host(np.full(sptr.size, -7, dtype=np.int32)), capi.DeviceArray.from_host(np.full(total, 3.0))
    info = (C.c_int64 * 4)()
    st = capi.lib().pamg_dev_schwarz_blocks(capi.F64, dA.handle, sptr.size - 1, dSp.ptr, dSj.ptr, dTp.ptr, dTx.ptr, total, 1e-10, 1, None, info)
    assert st == capi.E_UNSUPPORTED and info[1] == 65 and info[0] == total
    assert np.all(dTx.download() == 3.0) and np.all(dTp.download() == -7)
    for d in (dSp, dSj, dTp, dTx):
        d.free()
    dA.free()
    want = grelax.schwarz_parameters(A.copy(), sub, sptr)
    B = A.copy()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = grelax.schwarz_parameters(B, sub, sptr, device=True)
    assert len(w) == 1 and "1 of 3 subdomains" in str(w[0].message)
    assert np.array_equal(got[3], want[3]) and got[2].dtype == want[2].dtype
    a = int(want[3][1])
    assert np.array_equal(got[2][:a], want[2][:a])                              # the host part is exact
    assert np.allclose(got[2][a:], want[2][a:], rtol=1e-12, atol=1e-14)         # (well-conditioned blocks: the device part to rounding)
    assert B.schwarz_setup_report["on_host"] == 1 and B.schwarz_setup_report["largest"] == 65
