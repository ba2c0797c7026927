"""The committed cases of the approximate ideal restriction (AIR) setup (tests/golden/kernels_air.npz, written by
tests/golden/make_golden_air.py from the reference) and the checks the host replay and the device share: every comparison is
``np.array_equal`` on indptr, indices and data -- there is no tolerance."""
from functools import lru_cache
from pathlib import Path

import numpy as np
import scipy.sparse as sp

GOLDEN = Path(__file__).resolve().parent / "golden" / "kernels_air.npz"


@lru_cache(maxsize=1)
def data():
    with np.load(GOLDEN) as z:
        d = {k: z[k] for k in z.files}
    for v in d.values():
        v.setflags(write=False)                              # shared among the tests: nobody changes it
    return d


def csr(prefix, shape=None):
    d = data()
    indptr, indices, x = d[prefix + ".indptr"].copy(), d[prefix + ".indices"].copy(), d[prefix + ".data"].copy()
    n = indptr.size - 1
    return sp.csr_array((x, indices, indptr), shape=shape or (n, n))


def same_arrays(indptr, indices, values, prefix):
    d = data()
    assert np.array_equal(indptr, d[prefix + ".indptr"]), prefix
    assert np.array_equal(indices, d[prefix + ".indices"]), prefix
    assert values.dtype == np.float64 and np.array_equal(values, d[prefix + ".data"]), prefix


def same_csr(M, prefix):
    assert sp.issparse(M) and M.format == "csr"
    same_arrays(M.indptr, M.indices, M.data, prefix)


AIR = [str(s) for s in data()["air.names"]]
ONEPT = [(str(s), by_val) for s in data()["onept.names"] for by_val in (False, True)]
E2E = ("rs", "pmis")


def air_inputs(case):
    d = data()
    A = csr(f"air.{str(d[f'air.{case}.op'])}.A")
    return A, d[f"air.{case}.splitting"].copy(), float(d[f"air.{case}.theta"]), str(d[f"air.{case}.norm"]), int(d[f"air.{case}.degree"])


def unchanged(before, *now):
    for a, b in zip(before, now):
        assert np.array_equal(a, b)


def check_local_air(air, case):
    """local_air through the Python surface: the reference's R after eliminate_zeros"""
    A, splitting, theta, norm, degree = air_inputs(case)
    keep = (A.indptr.copy(), A.indices.copy(), A.data.copy(), splitting.copy())
    R = air.local_air(A, splitting, theta=theta, norm=norm, degree=degree)
    same_csr(R, f"air.{case}.R")
    assert R.shape == (int(splitting.sum()), A.shape[0]) and R.indptr.dtype == A.indptr.dtype
    unchanged(keep, A.indptr, A.indices, A.data, splitting)
    return R


def raw_passes(core, cls, case, shift=None):
    """pass 1 and pass 2 through the amg_core layer: the reference's row pointer, and R BEFORE eliminate_zeros (the identity entry last in
    every row, the solution entries that are exactly 0.0 stored).  shift: an (index, amount) applied to Rp before pass 2"""
    d = data()
    A, splitting, theta, norm, degree = air_inputs(case)
    C = cls.classical_strength_of_connection(A, theta=theta, block=False, norm=norm)
    Cpts = np.ascontiguousarray(np.where(splitting == 1)[0], dtype=np.int32)
    Rp = np.full(Cpts.size + 1, -5, dtype=np.int32)
    core.approx_ideal_restriction_pass1(Rp, C.indptr, C.indices, Cpts, splitting, degree)
    assert np.array_equal(Rp, d[f"air.{case}.Rp"])
    Rj = np.full(int(Rp[-1]), -3, dtype=np.int32)
    Rx = np.full(int(Rp[-1]), np.nan)                        # (the entry point zeroes what the reference wants zeroed)
    if shift is not None:
        Rp = Rp.copy()
        Rp[shift[0]] += shift[1]
    core.approx_ideal_restriction_pass2(Rp, Rj, Rx, A.indptr, A.indices, A.data, C.indptr, C.indices, C.data, Cpts, splitting, degree, 0, 10, 1)
    same_arrays(Rp, Rj, Rx, f"air.{case}.Rraw")
    return Rp, Rj, Rx


def check_one_point(air, case, by_val):
    d = data()
    A, C = csr(f"onept.{case}.A"), csr(f"onept.{case}.C")
    splitting = d[f"onept.{case}.splitting"].copy()
    keep = (A.indptr.copy(), A.indices.copy(), A.data.copy(), C.indptr.copy(), C.indices.copy(), C.data.copy(), splitting.copy())
    P = air.one_point_interpolation(A, C, splitting, by_val=by_val)
    assert sp.issparse(P) and P.format == "csr" and P.shape == (A.shape[0], int(d[f"onept.{case}.nc"])) and P.indptr.dtype == A.indptr.dtype
    nnz = int(P.indptr[-1])
    assert P.indices.size == nnz and P.data.size == nnz      # exactly indptr[-1] entries
    same_arrays(P.indptr, P.indices[:nnz], P.data[:nnz], f"onept.{case}.P{int(by_val)}")
    unchanged(keep, A.indptr, A.indices, A.data, C.indptr, C.indices, C.data, splitting)
    return P


def check_hierarchy(cf, levels):
    """levels: [(A, P, R), (A, P, R), (A,)] as CSR, against the reference's air_solver hierarchy"""
    for lvl, ops in enumerate(levels):
        for name, M in zip("APR", ops):
            same_csr(sp.csr_array(M), f"e2e.{cf}.{name}{lvl}")
            assert M.shape == csr(f"e2e.{cf}.{name}{lvl}", shape=M.shape).shape
    d = data()
    assert [ops[0].shape[0] for ops in levels] == list(d[f"e2e.{cf}.sizes"][:len(levels)])
