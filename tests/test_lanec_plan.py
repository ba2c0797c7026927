"""Host logic of the CLUSTER layout of the merged lane-parallel Gauss-Seidel sweep (CPU, no GPU): pyamg_amd/csrc/pamg_lanem_plan.h packs up to
4 / 8 rows of a super-level, consecutive in row-index order, into one wave's group -- the union of their operands once, row-tagged slots that index
it -- and tests/lanec_emul.cpp replays the plan the way c_group (pamg_lane.hip) consumes it.  The replay asserts what the device relies on (every
visited row in exactly one group, slot indices below the group's unique count, a lane serves one row, polled operands from EARLIER super-levels and
smaller group numbers: no deadlock for any number of waves visited in the adversarial order, gates are ancestors); the iterate after a forward, a
backward and a fused symmetric sweep must agree with the oracle's sequential sweep (amg_core::gauss_seidel, relaxation.h:48-76) to 1e-13 relative,
the bar tests/test_gpu_kernels.py holds the fast order to; with x = 0 the variant that skips the OLD operands must give the general one's bits.
Operators: level 1 of the smoothed-aggregation hierarchies under tests/golden, and the chains operator of test_lanem_plan.py whose ratio
|a_ir / a_rr| is 3 (not diagonally dominant: the growth bound closes super-levels early)."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle as orc
from pyamg_amd.hierarchy import load_spec

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
GOLDEN = HERE / "golden"
TOL = 1e-13
NAMES = ("super", "levels", "rows", "slot_units", "early", "old", "b", "direct", "max_len", "closed_len", "closed_growth", "groups", "unique_units",
         "unique_early", "unique_old", "unique_b", "early_lines", "padded_slots")
SA_LEVEL1 = ("sa3d_gs", "sa2d_gs", "sa2d_sor", "sa2d_cheby")


@pytest.fixture(scope="module")
def emul():
    out = HERE / "build"
    out.mkdir(exist_ok=True)
    so = out / "lanec_emul.so"
    src = HERE / "lanec_emul.cpp"
    hdrs = [ROOT / "pyamg_amd" / "csrc" / h for h in ("pamg_lanem_plan.h", "pamg_lane_plan.h", "pamg_tile_plan.h")]
    if not so.exists() or so.stat().st_mtime < max([src.stat().st_mtime] + [h.stat().st_mtime for h in hdrs]):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.lanec_emul_sweep_f64.restype = ctypes.c_int
    lib.lanec_emul_sym_f64.restype = ctypes.c_int
    return lib


def _csr(A):
    A = sp.csr_array(A)
    A.sort_indices()
    return (A, np.ascontiguousarray(A.indptr, dtype=np.int32), np.ascontiguousarray(A.indices, dtype=np.int32), np.ascontiguousarray(A.data, dtype=np.float64))


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run_sweep(lib, A, x, b, start, stop, step, s_max, cluster, growth_cap=1e3, waves=0, xz=0):
    A, Ap, Aj, Ax = _csr(A)
    xx = np.array(x, dtype=np.float64)
    bb = np.ascontiguousarray(b, dtype=np.float64)
    stats = np.zeros(18, dtype=np.int64)
    rc = lib.lanec_emul_sweep_f64(ctypes.c_int(A.shape[0]), _p(Ap), _p(Aj), _p(Ax), _p(xx), _p(bb), start, stop, step, s_max, ctypes.c_double(growth_cap),
                                  cluster, _p(stats), waves, xz)
    return rc, xx, dict(zip(NAMES, (int(v) for v in stats)))


def run_sym(lib, A, x, b, s_max, cluster, growth_cap=1e3, waves=0, xz=0):
    A, Ap, Aj, Ax = _csr(A)
    xx = np.array(x, dtype=np.float64)
    bb = np.ascontiguousarray(b, dtype=np.float64)
    stats = np.zeros(36, dtype=np.int64)
    rc = lib.lanec_emul_sym_f64(ctypes.c_int(A.shape[0]), _p(Ap), _p(Aj), _p(Ax), _p(xx), _p(bb), s_max, ctypes.c_double(growth_cap), cluster, _p(stats), waves, xz)
    return rc, xx, dict(zip(NAMES, (int(v) for v in stats[:18])))


def ref_sweep(A, x, b, start, stop, step):
    A, Ap, Aj, Ax = _csr(A)
    xx = np.array(x, dtype=np.float64)
    orc.gauss_seidel(Ap, Aj, Ax, xx, np.ascontiguousarray(b, dtype=np.float64), start, stop, step)
    return xx


def chains(n=400):
    main, off = np.full(n, 1.0), np.full(n - 1, -3.0)
    off[23::24] = 0.0                                                  # chains of 24 rows: the sweep itself stays finite (3^23)
    return sp.csr_array(sp.diags_array([off, main, 0.1 * off], offsets=[-1, 0, 1]))


def operators():
    ops = {}
    for name in SA_LEVEL1:
        spec = load_spec(GOLDEN / f"hier_{name}.npz")[0]
        A = sp.csr_array(spec.levels[1].A.to_scipy()).astype(np.float64)
        assert A.shape[0] == A.shape[1]
        ops[name] = A
    return ops


def _close(got, ref, tol=TOL):
    return np.max(np.abs(got - ref)) <= tol * np.max(np.abs(ref))


def test_cluster_sweeps_agree_with_the_sequential_sweep(emul):
    rng = np.random.RandomState(0)
    for name, A in operators().items():
        n = A.shape[0]
        x, b = rng.rand(n), rng.rand(n)
        fwd, bwd = ref_sweep(A, x, b, 0, n, 1), ref_sweep(A, x, b, n - 1, -1, -1)
        sym = ref_sweep(A, fwd, b, n - 1, -1, -1)
        for R in (4, 8):
            for s in (1, 3, 5):
                for waves in (0, 7, 64):
                    rc, got, st = run_sweep(emul, A, x, b, 0, n, 1, s, R, waves=waves)
                    assert rc == 0, (name, R, s, waves, rc)
                    assert _close(got, fwd), (name, R, s, waves, "forward")
                    rc, got, stb = run_sweep(emul, A, x, b, n - 1, -1, -1, s, R, waves=waves)
                    assert rc == 0, (name, R, s, waves, rc)
                    assert _close(got, bwd), (name, R, s, waves, "backward")
                    rc, got, _ = run_sym(emul, A, x, b, s, R, waves=waves)
                    assert rc == 0, (name, R, s, waves, rc)
                    assert _close(got, sym), (name, R, s, waves, "symmetric")
                ops_ = st["early"] + st["old"] + st["b"]
                assert st["rows"] == n and st["groups"] >= (n + R - 1) // R and st["groups"] <= n
                assert st["unique_early"] <= st["early"] and st["unique_old"] <= st["old"] and st["unique_b"] <= st["b"]
                assert st["early_lines"] <= st["unique_early"]
                assert st["padded_slots"] == 64 * st["slot_units"] >= ops_
                print(f"[lanec] {name} R={R} s={s}: {n} rows in {st['groups']} groups, operands per row {ops_ / n:.1f}, unique {(st['unique_early'] + st['unique_old'] + st['unique_b']) / n:.1f}"
                      f" (early {st['unique_early'] / n:.1f} in {st['early_lines'] / n:.1f} lines), padding {st['padded_slots'] / max(1, ops_):.2f}")
                if s == 1:
                    assert st["super"] == st["levels"] and st["b"] == 0 and ops_ == st["direct"]


def test_a_row_slice_and_a_partial_sweep(emul):
    rng = np.random.RandomState(4)
    A = operators()["sa3d_gs"]
    n = A.shape[0]
    x, b = rng.rand(n), rng.rand(n)
    for (start, stop, step) in ((5, n - 7, 1), (n - 3, 2, -1)):
        ref = ref_sweep(A, x, b, start, stop, step)
        for R in (4, 8):
            rc, got, st = run_sweep(emul, A, x, b, start, stop, step, 3, R, waves=16)
            assert rc == 0 and st["rows"] == len(range(start, stop, step)), (R, rc, st)
            assert _close(got, ref)
            untouched = np.setdiff1d(np.arange(n), np.arange(start, stop, step))
            assert np.array_equal(got[untouched], x[untouched])


def test_x_known_to_be_zero_gives_the_same_bits(emul):
    rng = np.random.RandomState(1)
    for name, A in operators().items():
        n = A.shape[0]
        z, b = np.zeros(n), rng.rand(n)
        for R in (4, 8):
            rc0, g0, _ = run_sweep(emul, A, z, b, 0, n, 1, 3, R, waves=9, xz=0)
            rc1, g1, _ = run_sweep(emul, A, z, b, 0, n, 1, 3, R, waves=9, xz=1)
            assert rc0 == 0 and rc1 == 0
            assert np.array_equal(g0, g1), (name, R)
            rc0, s0, _ = run_sym(emul, A, z, b, 3, R, waves=9, xz=0)
            rc1, s1, _ = run_sym(emul, A, z, b, 3, R, waves=9, xz=1)
            assert rc0 == 0 and rc1 == 0
            assert np.array_equal(s0, s1), (name, R)


def test_chains_with_a_ratio_above_one(emul):
    """|a_ir / a_rr| = 3 along chains of 24 rows: the growth bound closes super-levels early and what is kept reproduces the sequential sweep
    (three digits are lost to growth <= 1e3, the bar of test_lanem_plan.py; with the cap at 1 nothing is merged and the 1e-13 bar holds)"""
    rng = np.random.RandomState(1)
    A = chains()
    n = A.shape[0]
    x, b = rng.rand(n), rng.rand(n)
    fwd = ref_sweep(A, x, b, 0, n, 1)
    sym = ref_sweep(A, fwd, b, n - 1, -1, -1)
    for R in (4, 8):
        rc, got, st = run_sweep(emul, A, x, b, 0, n, 1, 8, R, growth_cap=1e3, waves=5)
        assert rc == 0 and st["closed_growth"] > 0 and st["super"] > (st["levels"] + 7) // 8, (rc, st)
        assert _close(got, fwd, 1e-10)
        rc, got, _ = run_sym(emul, A, x, b, 8, R, growth_cap=1e3, waves=5)
        assert rc == 0 and _close(got, sym, 1e-10)
        rc, got, st1 = run_sweep(emul, A, x, b, 0, n, 1, 8, R, growth_cap=1.0, waves=5)
        assert rc == 0 and st1["super"] == st1["levels"] and st1["b"] == 0
        assert _close(got, fwd)
        rc, got, _ = run_sym(emul, A, x, b, 8, R, growth_cap=1.0, waves=5)
        assert rc == 0 and _close(got, sym)


def test_rows_without_a_diagonal_stay_untouched(emul):
    rng = np.random.RandomState(3)
    A = sp.lil_array(operators()["sa2d_gs"])
    n = A.shape[0]
    for i in range(0, n, 5):
        A[i, i] = 0.0
    A = sp.csr_array(A)
    x, b = rng.rand(n), rng.rand(n)
    for R in (4, 8):
        for (start, stop, step) in ((0, n, 1), (n - 1, -1, -1)):
            ref = ref_sweep(A, x, b, start, stop, step)
            rc, got, _ = run_sweep(emul, A, x, b, start, stop, step, 3, R, waves=16)
            assert rc == 0 and _close(got, ref), (R, rc)
            assert np.array_equal(got[0::5], x[0::5])
        rc, got, _ = run_sym(emul, A, x, b, 3, R, waves=16)
        assert rc == 0 and _close(got, ref_sweep(A, ref_sweep(A, x, b, 0, n, 1), b, n - 1, -1, -1))

