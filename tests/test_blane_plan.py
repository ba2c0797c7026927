"""Host logic of the lane-parallel FAST-ORDER block Gauss-Seidel sweep (CPU, no GPU): the layout built by pyamg_amd/csrc/pamg_blane_plan.h is
replayed by tests/blane_emul.cpp the way bsr_lane_kernel consumes it (K blocks per lane, their gemv with x_j, XOR butterfly per component over
the lanes of a block row, one row of Dinv per lane, component-wise sentinel hand-off) with the waves visited in the adversarial order, and must
agree with the oracle's amg_core::block_gauss_seidel (relaxation.h:1242-1298) to rounding: 1e-13 relative per sweep."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle as orc

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
TOL = 1e-13


@pytest.fixture(scope="module")
def emul():
    out = HERE / "build"
    out.mkdir(exist_ok=True)
    so = out / "blane_emul.so"
    src = HERE / "blane_emul.cpp"
    hdrs = [ROOT / "pyamg_amd" / "csrc" / h for h in ("pamg_blane_plan.h", "pamg_lane_plan.h", "pamg_tile_plan.h")]
    if not so.exists() or so.stat().st_mtime < max([src.stat().st_mtime] + [h.stat().st_mtime for h in hdrs]):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.blane_emul_sweep_f64.restype = ctypes.c_int
    return lib


def block_operator(nb, bs, per_row, seed, band=25):
    rng = np.random.default_rng(seed)
    i = np.repeat(np.arange(nb), per_row // 2)
    j = np.clip(i + rng.integers(-band, band + 1, size=i.size), 0, nb - 1)
    S = sp.coo_array((np.ones(i.size), (i, j)), shape=(nb, nb)).tocsr()
    S = ((S + S.T + sp.eye_array(nb)) != 0).astype(float).tocsr()
    S.sort_indices()
    data = rng.standard_normal((S.nnz, bs, bs)) * 0.2
    A = sp.bsr_array((data, S.indices.astype(np.int32), S.indptr.astype(np.int32)), shape=(nb * bs, nb * bs))
    # strongly dominant diagonal blocks; their inverses
    rows = np.repeat(np.arange(nb), np.diff(S.indptr))
    dmask = rows == S.indices
    A.data[dmask] += np.eye(bs) * (per_row + 4.0)
    Dinv = np.linalg.inv(A.data[dmask])
    return A, np.ascontiguousarray(Dinv)


def run(lib, A, Dinv, x, b, start, stop, step, waves, snapshot=0, want_L=8, mode=0):
    """want_L = 8: what build_blane_part hands the planner at lane_L = 0; mode 0: the static form"""
    bs = A.blocksize[0]
    nb = A.shape[0] // bs
    xx = np.array(x, dtype=np.float64)
    stats = np.zeros(8, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    bAp, bAj = np.ascontiguousarray(A.indptr, dtype=np.int32), np.ascontiguousarray(A.indices, dtype=np.int32)
    bAx = np.ascontiguousarray(A.data, dtype=np.float64)
    rc = lib.blane_emul_sweep_f64(nb, bs, p(bAp), p(bAj), p(bAx), p(np.ascontiguousarray(Dinv, dtype=np.float64)), p(xx),
                                  p(np.ascontiguousarray(b, dtype=np.float64)), start, stop, step, waves, snapshot, want_L, mode, p(stats))
    return rc, xx, stats


def ref(A, Dinv, x, b, start, stop, step):
    bs = A.blocksize[0]
    xx = np.array(x, dtype=np.float64)
    orc.block_gauss_seidel(np.ascontiguousarray(A.indptr, dtype=np.int32), np.ascontiguousarray(A.indices, dtype=np.int32),
                           np.ascontiguousarray(A.data.ravel(), dtype=np.float64), xx, np.ascontiguousarray(b, dtype=np.float64),
                           np.ascontiguousarray(Dinv.ravel(), dtype=np.float64), start, stop, step, bs)
    return xx


def close(a, b):
    return np.max(np.abs(a - b)) <= TOL * max(1.0, np.max(np.abs(b)))


@pytest.mark.parametrize("waves", [1, 7, 500])
@pytest.mark.parametrize("bs,per_row", [(2, 10), (3, 42), (4, 20), (6, 40), (3, 90)])
def test_block_sweeps_agree_with_the_sequential_loop(emul, bs, per_row, waves):
    A, Dinv = block_operator(700, bs, per_row, bs * 100 + per_row)
    nb = A.shape[0] // bs
    rng = np.random.default_rng(4)
    x, b = rng.random(A.shape[0]), rng.random(A.shape[0])
    for rng_ in ((0, nb, 1), (nb - 1, -1, -1), (10, nb - 10, 1)):
        rc, got, st = run(emul, A, Dinv, x, b, *rng_, waves)
        assert rc == 0, (rng_, rc)
        assert st[0] * st[1] >= min(per_row, 2 * 64) * 0 + 1
        assert close(got, ref(A, Dinv, x, b, *rng_))


def test_nonsymmetric_block_pattern_with_snapshot_and_rows_too_long(emul):
    A, Dinv = block_operator(300, 3, 12, 9)
    # drop some off-diagonal blocks on one side: a structurally non-symmetric block pattern
    keep = np.ones(A.indices.size, dtype=bool)
    rows = np.repeat(np.arange(300), np.diff(A.indptr))
    keep[(A.indices > rows) & (rows % 3 == 0)] = False
    ip = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=300))]).astype(np.int32)
    B = sp.bsr_array((A.data[keep], A.indices[keep], ip), shape=A.shape)
    rng = np.random.default_rng(5)
    x, b = rng.random(900), rng.random(900)
    for rng_ in ((0, 300, 1), (299, -1, -1)):
        rc, got, _ = run(emul, B, Dinv, x, b, *rng_, 5, snapshot=1)
        assert rc == 0 and close(got, ref(B, Dinv, x, b, *rng_))
    D, Di = block_operator(200, 2, 320, 1, band=199)          # > 128 blocks per block row: declined
    rc, *_ = run(emul, D, Di, np.zeros(400), np.ones(400), 0, 200, 1, 1)
    assert rc == 2
