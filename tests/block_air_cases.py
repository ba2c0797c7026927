"""The committed cases of the block (BSR) AIR setup (tests/golden/kernels_block_air.npz, written by tests/golden/make_golden_block_air.py
from the reference) and the checks the host replay and the device share: every comparison is ``np.array_equal`` on indptr, indices and
data -- there is no tolerance."""
from functools import lru_cache
from pathlib import Path

import numpy as np
import scipy.sparse as sp

GOLDEN = Path(__file__).resolve().parent / "golden" / "kernels_block_air.npz"


@lru_cache(maxsize=1)
def _file():
    with np.load(GOLDEN) as z:
        f = {k: z[k] for k in z.files}
    pools = (f["f64"], f["i32"])
    d = {}
    for key, (pool, off, size) in zip(map(str, f["keys"]), f["index"]):
        d[key] = pools[pool][off:off + size]
        d[key].setflags(write=False)                         # shared among the tests: nobody changes it
    tables = {name: [tuple(map(str, row)) for row in f[name]] for name in ("ops", "strength", "air", "onept")}
    return d, tables


def data():
    return _file()[0]


OPS = {name: int(b) for name, b in _file()[1]["ops"]}                                           # operator -> block size
STRENGTH = {c: (op, norm, float(theta)) for c, op, norm, theta in _file()[1]["strength"]}       # case -> (operator, norm, theta)
AIR = {c: (op, norm, float(theta), int(degree)) for c, op, norm, theta, degree in _file()[1]["air"]}
ONEPT = dict(_file()[1]["onept"])                                                               # case -> strength case


def bsr(prefix, b, shape=None):
    d = data()
    indptr, indices = d[prefix + ".indptr"].copy(), d[prefix + ".indices"].copy()
    x = d[prefix + ".data"].copy().reshape(-1, b, b)
    n = indptr.size - 1
    return sp.bsr_array((x, indices, indptr), blocksize=(b, b), shape=shape or (n * b, n * b))


def operator(op):
    return bsr(f"blk.{op}.A", OPS[op]), data()[f"blk.{op}.splitting"].copy()


def same_arrays(indptr, indices, values, prefix):
    d = data()
    assert np.array_equal(indptr, d[prefix + ".indptr"]), prefix
    assert np.array_equal(indices, d[prefix + ".indices"]), prefix
    values = np.asarray(values)
    assert values.dtype == np.float64 and np.array_equal(values.reshape(-1), d[prefix + ".data"]), prefix


def same_bsr(M, prefix, b):
    assert sp.issparse(M) and M.format == "bsr" and tuple(M.blocksize) == (b, b)
    nnz = int(M.indptr[-1])
    same_arrays(M.indptr, M.indices[:nnz], M.data[:nnz], prefix)


def unchanged(before, *now):
    for a, b in zip(before, now):
        assert np.array_equal(a, b)


def _snapshot(*Ms):
    out = []
    for M in Ms:
        out += [M.copy()] if isinstance(M, np.ndarray) else [M.indptr.copy(), M.indices.copy(), M.data.copy()]
    return out


def _now(*Ms):
    out = []
    for M in Ms:
        out += [M] if isinstance(M, np.ndarray) else [M.indptr, M.indices, M.data]
    return out


def check_measure(core, case):
    """the block measure through the amg_core layer"""
    op, norm, _ = STRENGTH[case]
    A, _ = operator(op)
    Ax = np.ascontiguousarray(A.data).reshape(-1)
    out = np.full(A.indices.size, np.nan)
    core.block_strength_measure(OPS[op], norm, Ax, out)
    want = data()[f"str.{case}.measure"]
    assert np.array_equal(out, want) and np.array_equal(np.signbit(out), np.signbit(want)), case


def check_strength(mod, case):
    op, norm, theta = STRENGTH[case]
    A, _ = operator(op)
    keep = _snapshot(A)
    S = mod.classical_strength_of_connection(A, theta=theta, block=True, norm=norm)
    n = A.shape[0] // OPS[op]
    assert sp.issparse(S) and S.format == "csr" and S.shape == (n, n) and S.indptr.dtype == A.indptr.dtype
    same_arrays(S.indptr, S.indices, S.data, f"str.{case}.S")
    unchanged(keep, *_now(A))
    return S


def strength_of(case):
    """the reference's strength matrix of a strength case"""
    d = data()
    p = f"str.{case}.S"
    n = d[p + ".indptr"].size - 1
    return sp.csr_array((d[p + ".data"].copy(), d[p + ".indices"].copy(), d[p + ".indptr"].copy()), shape=(n, n))


def kept(case):
    """what local_air returns, from R before eliminate_zeros and the fixture's mask: (indptr, indices, data as blocks)"""
    d = data()
    op = AIR[case][0]
    b = OPS[op]
    Rp, Rj, Rx = d[f"blk.{case}.Rraw.indptr"], d[f"blk.{case}.Rraw.indices"], d[f"blk.{case}.Rraw.data"].reshape(-1, b, b)
    keep = d[f"blk.{case}.R.keep"].astype(bool)
    rowof = np.repeat(np.arange(Rp.size - 1), np.diff(Rp))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rowof[keep], minlength=Rp.size - 1))])
    return indptr, Rj[keep], Rx[keep]


def check_local_air(mod, case):
    """local_air through the Python surface: the reference's R after eliminate_zeros"""
    op, norm, theta, degree = AIR[case]
    b = OPS[op]
    A, splitting = operator(op)
    keep = _snapshot(A, splitting)
    R = mod.local_air(A, splitting, theta=theta, norm=norm, degree=degree)
    assert sp.issparse(R) and R.format == "bsr" and tuple(R.blocksize) == (b, b)
    assert R.shape == (int(splitting.sum()) * b, A.shape[0]) and R.indptr.dtype == A.indptr.dtype
    indptr, indices, blocks = kept(case)
    nnz = int(R.indptr[-1])
    assert np.array_equal(R.indptr, indptr) and np.array_equal(R.indices[:nnz], indices), case
    assert R.data.dtype == np.float64 and np.array_equal(R.data[:nnz], blocks), case
    unchanged(keep, *_now(A, splitting))
    return R


def raw_pass2(core, mod, case, shift=None, use_gmres=0):
    """pass 1 and block pass 2 through the amg_core layer on the block strength matrix of ``mod``: the reference's row pointer, and R BEFORE
    eliminate_zeros (the identity block last in every row).  shift: an (index, amount) applied to Rp before pass 2"""
    d = data()
    op, norm, theta, degree = AIR[case]
    b = OPS[op]
    A, splitting = operator(op)
    C = mod.classical_strength_of_connection(A, theta=theta, block=True, norm=norm)
    Cpts = np.ascontiguousarray(np.where(splitting == 1)[0], dtype=np.int32)
    Rp = np.full(Cpts.size + 1, -5, dtype=np.int32)
    core.approx_ideal_restriction_pass1(Rp, C.indptr, C.indices, Cpts, splitting, degree)
    assert np.array_equal(Rp, d[f"blk.{case}.Rraw.indptr"])
    Rj = np.full(int(Rp[-1]), -3, dtype=np.int32)
    Rx = np.full(int(Rp[-1]) * b * b, np.nan)                # (the entry point zeroes what the reference wants zeroed)
    if shift is not None:
        Rp = Rp.copy()
        Rp[shift[0]] += shift[1]
    Ax = np.ascontiguousarray(A.data).reshape(-1)
    try:
        core.block_approx_ideal_restriction_pass2(Rp, Rj, Rx, A.indptr, A.indices, Ax, C.indptr, C.indices, C.data, Cpts, splitting, b, degree, use_gmres,
                                                  10, 1)
    except Exception:
        assert np.all(Rj == -3) and np.all(np.isnan(Rx))     # a refusal writes nothing
        raise
    same_arrays(Rp, Rj, Rx, f"blk.{case}.Rraw")
    assert not np.any(np.signbit(Rx[Rx == 0.0]))             # the clipped entries are +0.0
    for r in range(Cpts.size):
        assert Rj[Rp[r + 1] - 1] == Cpts[r] and np.array_equal(Rx.reshape(-1, b, b)[Rp[r + 1] - 1], np.eye(b))
    return Rp, Rj, Rx


def check_one_point(mod, case):
    d = data()
    strcase = ONEPT[case]
    op = STRENGTH[strcase][0]
    b = OPS[op]
    A, splitting = operator(op)
    C = strength_of(strcase)
    keep = _snapshot(A, C, splitting)
    P = mod.one_point_interpolation(A, C, splitting)
    n = A.shape[0] // b
    assert sp.issparse(P) and P.format == "bsr" and tuple(P.blocksize) == (b, b) and P.shape == (n * b, int(splitting.sum()) * b)
    assert P.indptr.dtype == A.indptr.dtype
    nnz = int(P.indptr[-1])
    assert P.indices.size == nnz and P.data.shape == (nnz, b, b)         # exactly indptr[-1] blocks
    assert np.array_equal(P.indptr, d[f"onept.{case}.P.indptr"]) and np.array_equal(P.indices, d[f"onept.{case}.P.indices"])
    assert np.array_equal(P.data, np.broadcast_to(np.eye(b), (nnz, b, b)))
    unchanged(keep, *_now(A, C, splitting))
    return P


def check_hierarchy(levels):
    """levels: [(A, P, R), (A, P, R), (A,)] as BSR with blocks of 2, against the reference's air_solver hierarchy"""
    d = data()
    for lvl, ops in enumerate(levels):
        same_bsr(ops[0], f"e2e.A{lvl}", 2)
        if len(ops) > 1:
            P, R = ops[1], ops[2]
            nnz = int(P.indptr[-1])
            assert P.format == "bsr" and tuple(P.blocksize) == (2, 2)
            assert np.array_equal(P.indptr, d[f"e2e.P{lvl}.indptr"]) and np.array_equal(P.indices[:nnz], d[f"e2e.P{lvl}.indices"])
            assert np.array_equal(P.data[:nnz], np.broadcast_to(np.eye(2), (nnz, 2, 2)))
            same_bsr(R, f"e2e.R{lvl}", 2)
    assert [ops[0].shape[0] for ops in levels] == list(d["e2e.sizes"][:len(levels)])
