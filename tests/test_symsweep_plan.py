"""Host logic of the FUSED SYMMETRIC merged sweep (CPU, no GPU): tests/symsweep_emul.cpp replays the order in which gs_lanem_sym_kernel
(pyamg_amd/csrc/pamg_lane.hip) consumes the forward and the backward plan of pamg_lanem_plan.h in one launch -- phase 1, the completion barrier
that counts finished groups, phase 2 -- for the static and the ticket assignment of groups to waves, the waves visited in the adversarial order.

What the replay asserts (its return code names the check): (a) it terminates, and no phase-2 group starts before the barrier has opened;
(b) the wipe partition covers every entry of the buffer a phase wipes exactly once per phase, so the backward buffer -- filled with values
that would pass for published ones -- is all sentinels when the barrier opens and the forward buffer of the NEXT launch is all sentinels at the
end (launches are replayed back to back on the same buffers, the parity flipping in between); (c) no phase-1 read of x and no phase-2 read of
the vector that carries the forward sweep's values (the forward hand-off buffer) can follow a write to the same vector inside its phase: the
phase neither publishes in nor wipes the vector it reads old operands from.  The result of every launch must be the BITS of the two directional
sweeps replayed one after the other, and the oracle's symmetric sweep to rounding (1e-13 relative, the bar of tests/test_lanem_plan.py per
sweep)."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle as orc
from tools.problems import poisson_csr

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
TOL = 1e-13


@pytest.fixture(scope="module")
def emul():
    out = HERE / "build"
    out.mkdir(exist_ok=True)
    so = out / "symsweep_emul.so"
    src = HERE / "symsweep_emul.cpp"
    hdrs = [ROOT / "pyamg_amd" / "csrc" / h for h in ("pamg_lanem_plan.h", "pamg_lane_plan.h", "pamg_tile_plan.h")]
    if not so.exists() or so.stat().st_mtime < max([src.stat().st_mtime] + [h.stat().st_mtime for h in hdrs]):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.symsweep_emul_f64.restype = ctypes.c_int
    return lib


def run(lib, A, x, b, s_max, rpw, waves, ticket, xzero=0, launches=2):
    A = sp.csr_array(A)
    Ap = np.ascontiguousarray(A.indptr, dtype=np.int32)
    Aj = np.ascontiguousarray(A.indices, dtype=np.int32)
    Ax = np.ascontiguousarray(A.data, dtype=np.float64)
    xx = np.array(x, dtype=np.float64)
    x2 = np.zeros_like(xx)
    stats = np.zeros(8, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.symsweep_emul_f64(ctypes.c_int(A.shape[0]), p(Ap), p(Aj), p(Ax), p(xx), p(x2), p(np.ascontiguousarray(b, dtype=np.float64)),
                               s_max, rpw, waves, ticket, xzero, launches, p(stats))
    names = ("groups_fwd", "groups_bwd", "rounds", "wiped_b", "wiped_f", "old_read_1", "old_read_2", "waves")
    return rc, xx, x2, dict(zip(names, (int(v) for v in stats)))


def sa_like(n=1500, density=0.01, seed=5):
    rng = np.random.RandomState(seed)
    S = sp.random(n, n, density=density, random_state=rng, format="csr")
    S = sp.csr_array(-abs(S + S.T))
    S.setdiag(0)
    S.eliminate_zeros()
    d = np.asarray(abs(S).sum(axis=1)).ravel() + 0.5 + rng.rand(n)
    A = sp.csr_array(S + sp.diags_array(d))
    A.sort_indices()
    return A


def nodiag_case():
    """rows without a usable diagonal keep their value: their old value must travel through the forward hand-off buffer"""
    A = sp.lil_array(sa_like(600, 0.02, 9))
    for i in (0, 17, 311, 599):
        A[i, i] = 0.0
    A = sp.csr_array(A)
    A.sort_indices()
    return A


def ref_symmetric(A, x, b):
    A = sp.csr_array(A)
    xx = np.array(x, dtype=np.float64)
    n = A.shape[0]
    Ap, Aj, Ax = (np.ascontiguousarray(A.indptr, dtype=np.int32), np.ascontiguousarray(A.indices, dtype=np.int32),
                  np.ascontiguousarray(A.data, dtype=np.float64))
    orc.gauss_seidel(Ap, Aj, Ax, xx, b, 0, n, 1)
    orc.gauss_seidel(Ap, Aj, Ax, xx, b, n - 1, -1, -1)
    return xx


CASES = {"sa_like": sa_like, "poisson3d": lambda: poisson_csr((11, 9, 10)), "nodiag": nodiag_case}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("ticket", [0, 1], ids=["static", "tickets"])
@pytest.mark.parametrize("rpw,s_max", [(1, 8), (2, 3), (1, 2)])
def test_fused_replay(emul, case, ticket, rpw, s_max):
    A = CASES[case]()
    n = A.shape[0]
    rng = np.random.RandomState(3)
    x, b = rng.rand(n), rng.rand(n)
    ref = ref_symmetric(A, ref_symmetric(A, x, b), b)                # two launches
    for waves in (4, 12, 64, 4096):                                  # one workgroup ... more waves than groups
        rc, got, two, st = run(emul, A, x, b, s_max, rpw, waves, ticket)
        assert rc == 0, (case, waves, rc)
        assert np.array_equal(got, two), (case, waves, "fused replay != the two directional replays")
        err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
        assert err <= 4 * TOL, (case, waves, err)                    # four sweeps
        assert st["groups_fwd"] > 0 and st["groups_bwd"] > 0 and st["wiped_b"] == n and st["wiped_f"] == n, st
        assert st["old_read_2"] > 0, st


@pytest.mark.parametrize("ticket", [0, 1], ids=["static", "tickets"])
def test_x_known_to_be_zero_skips_the_old_operands_of_phase_one(emul, ticket):
    A = sa_like()
    n = A.shape[0]
    b = np.random.RandomState(4).rand(n)
    z = np.zeros(n)
    rc0, got0, two0, st0 = run(emul, A, z, b, 8, 1, 64, ticket, xzero=0, launches=1)
    rc1, got1, two1, st1 = run(emul, A, z, b, 8, 1, 64, ticket, xzero=1, launches=1)
    assert rc0 == 0 and rc1 == 0, (rc0, rc1)
    assert np.array_equal(got0, two0) and np.array_equal(got1, got0)  # the same bits
    assert st0["old_read_1"] > 0 and st1["old_read_1"] == 0, (st0, st1)   # and no old operand is fetched in phase 1
    assert st1["old_read_2"] == st0["old_read_2"] > 0
