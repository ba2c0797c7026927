"""The dense block-triangular form of the symmetric Gauss-Seidel sweep from zero (CPU, no GPU): pyamg_amd/csrc/pamg_dtri_plan.h replayed by the
stand-alone program tests/dtri_emul.cpp -- block partition, off-block slices, reference block inverses, growth guard, the phases in launch order --
against the oracle's symmetric sweep
    from zero                      x = S b,
    from a random iterate          x + S (b - A x)   (the correction form: the residual is formed here, the program accumulates).
Bar: 1e-13 relative in the max norm (the fast order's per-sweep bar; the form differs from plain substitution by rounding only: 2.5e-15 measured).
Cases: 2-D Poisson 40^2 = 1600 rows with B = 64 (25 full blocks), B = 100 (16 full blocks) and B = 96 (16 blocks and a ragged one of 64 rows);
n < B (one block, empty slices); B = 1 (no inverse beyond 1 / a_ii: every value equals plain substitution with that reciprocal, bit for bit); an upwind
convection-diffusion operator (non-symmetric: Wb is not Wf^T); the chains operator (|a_ir / a_rr| = 3 along chains of 24 rows: the growth of an inverse
block is ~3^23, the planner declines and says so); a zero and a missing diagonal entry (declines).
The same program is built once more with -fsanitize=address,undefined and run on a case of every kind."""
import subprocess
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle as orc

import midsize

HERE = Path(__file__).resolve().parent
TOL = 1e-13
OK, E_SHAPE, E_DIAGONAL, E_GROWTH = 0, 1, 2, 3


def _build(out, flags):
    src, hdr = HERE / "dtri_emul.cpp", HERE.parent / "pyamg_amd" / "csrc" / "pamg_dtri_plan.h"
    if not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", *flags, str(src), "-o", str(out)], check=True)
    return out


@pytest.fixture(scope="module")
def emul():
    d = HERE / "build" / "dtri"
    d.mkdir(parents=True, exist_ok=True)
    return _build(d / "dtri_emul", [])


@pytest.fixture(scope="module")
def emul_san():
    d = HERE / "build" / "dtri"
    d.mkdir(parents=True, exist_ok=True)
    return _build(d / "dtri_emul_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def _csr(A):
    A = sp.csr_array(A)
    A.sort_indices()
    return A, np.ascontiguousarray(A.indptr, dtype=np.int32), np.ascontiguousarray(A.indices, dtype=np.int32), np.ascontiguousarray(A.data, dtype=np.float64)


def run(prog, tmp, A, B, b, x=None):
    """(status, blocks, off-block entries, slots, growth, x) of one replay: x = S b, or x + S b where an iterate is given"""
    A, Ap, Aj, Ax = _csr(A)
    n = A.shape[0]
    case, res = tmp / "case.bin", tmp / "result.bin"
    with open(case, "wb") as f:
        np.array([n, Ax.size, B, 0 if x is None else 1], dtype=np.int32).tofile(f)
        for a in (Ap, Aj, Ax, np.ascontiguousarray(b, dtype=np.float64), np.zeros(n) if x is None else np.ascontiguousarray(x, dtype=np.float64)):
            a.tofile(f)
    subprocess.run([str(prog), str(case), str(res)], check=True)
    raw = res.read_bytes()
    status, blocks = np.frombuffer(raw, dtype=np.int32, count=2)
    off, slots = np.frombuffer(raw, dtype=np.int64, count=2, offset=8)
    growth = float(np.frombuffer(raw, dtype=np.float64, count=1, offset=24)[0])
    return int(status), int(blocks), int(off), int(slots), growth, np.frombuffer(raw, dtype=np.float64, count=n, offset=32).copy()


def ref_symmetric(A, b, x0=None):
    A, Ap, Aj, Ax = _csr(A)
    n = A.shape[0]
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
    bb = np.ascontiguousarray(b, dtype=np.float64)
    orc.gauss_seidel(Ap, Aj, Ax, x, bb, 0, n, 1)
    orc.gauss_seidel(Ap, Aj, Ax, x, bb, n - 1, -1, -1)
    return x


def _rel(got, ref):
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


def poisson2d(m=40):
    T = sp.diags_array([-np.ones(m - 1), 2 * np.ones(m), -np.ones(m - 1)], offsets=[-1, 0, 1])
    I = sp.eye_array(m)
    return sp.csr_array(sp.kron(I, T) + sp.kron(T, I))


def chains(n=400):
    main, off = np.full(n, 1.0), np.full(n - 1, -3.0)
    off[23::24] = 0.0
    return sp.csr_array(sp.diags_array([off, main, 0.1 * off], offsets=[-1, 0, 1]))


def _check(prog, tmp, name, A, B, blocks):
    A = sp.csr_array(A)
    n = A.shape[0]
    rng = np.random.RandomState(7)
    b, x0 = rng.rand(n), rng.rand(n)
    st, nb, off, slots, growth, x = run(prog, tmp, A, B, b)
    assert (st, nb) == (OK, blocks), (name, B, st, nb)
    err0 = _rel(x, ref_symmetric(A, b))
    st, _, _, _, _, x1 = run(prog, tmp, A, B, b - A @ x0, x0)
    assert st == OK
    err1 = _rel(x1, ref_symmetric(A, b, x0))
    print(f"[dtri] {name} B={B}: {nb} blocks, {off} off-block entries of {A.nnz - n}, growth {growth:.3f}; |dx|/|x| from zero {err0:.2e}, from an iterate {err1:.2e}")
    assert err0 <= TOL and err1 <= TOL, (name, B, err0, err1)
    assert growth <= 1e3
    return off, slots, x


@pytest.mark.parametrize("B,blocks", [(64, 25), (100, 16), (96, 17)])
def test_poisson_blocks(emul, tmp_path, B, blocks):
    A = poisson2d()
    off, slots, _ = _check(emul, tmp_path, "poisson 40^2", A, B, blocks)
    assert 0 < off < A.nnz - A.shape[0]
    sizes = [min(B, 1600 - k * B) for k in range(blocks)]
    assert slots == sum(sum((i + 2) & ~1 for i in range(m)) for m in sizes)        # rows of i + 1 values in an even number of slots


def test_one_block(emul, tmp_path):
    A = poisson2d()
    off, slots, _ = _check(emul, tmp_path, "poisson 40^2", A, 2048, 1)
    assert off == 0


def test_block_of_one_row_is_plain_substitution(emul, tmp_path):
    A = poisson2d(12)
    n = A.shape[0]
    off, _, x = _check(emul, tmp_path, "poisson 12^2", A, 1, n)
    assert off == A.nnz - n
    A, Ap, Aj, Ax = _csr(A)
    b = np.random.RandomState(7).rand(n)                                # the right-hand side _check used
    d = A.diagonal()
    y, z = np.zeros(n), np.zeros(n)
    for i in range(n):
        s = 0.0
        for p in range(Ap[i], Ap[i + 1]):
            if Aj[p] < i:
                s += Ax[p] * y[Aj[p]]
        y[i] = (1.0 / d[i]) * (b[i] - s)
    for i in range(n - 1, -1, -1):
        s = 0.0
        for p in range(Ap[i], Ap[i + 1]):
            if Aj[p] > i:
                s += Ax[p] * z[Aj[p]]
        z[i] = (1.0 / d[i]) * (d[i] * y[i] - s)
    assert np.array_equal(x, z)


def test_nonsymmetric_upwind(emul, tmp_path):
    A = midsize.convection_diffusion(10)
    assert abs(A - A.T).max() > 0.1
    _check(emul, tmp_path, "upwind convection-diffusion 10^3", A, 64, 16)
    _check(emul, tmp_path, "upwind convection-diffusion 10^3", A, 300, 4)


def test_growth_declines(emul, tmp_path):
    A = chains()
    n = A.shape[0]
    b = np.random.RandomState(3).rand(n)
    st, nb, _, _, growth, x = run(emul, tmp_path, A, 64, b)
    print(f"[dtri] chains B=64: status {st}, growth {growth:.3e}")
    assert st == E_GROWTH and growth > 1e3 and np.array_equal(x, np.zeros(n))
    st, _, _, _, growth, x = run(emul, tmp_path, A, 1, b)               # blocks of one row: nothing grows, the form is plain substitution
    assert st == OK and growth == 1.0 and _rel(x, ref_symmetric(A, b)) <= TOL


def test_bad_diagonal_declines(emul, tmp_path):
    base = poisson2d(12)
    n = base.shape[0]
    b = np.ones(n)
    A = sp.lil_array(base)
    A[5, 5] = 0.0
    stored = sp.csr_array(A)                                            # lil keeps no explicit zero: the entry is missing
    assert stored.nnz == base.nnz - 1
    assert run(emul, tmp_path, stored, 16, b)[0] == E_DIAGONAL
    A = sp.csr_array(base, copy=True)
    A.data[A.indptr[5]:A.indptr[6]][A.indices[A.indptr[5]:A.indptr[6]] == 5] = 0.0       # an explicit zero
    assert A.nnz == base.nnz and A.diagonal()[5] == 0.0
    assert run(emul, tmp_path, A, 16, b)[0] == E_DIAGONAL
    A.data[A.indptr[5]:A.indptr[6]][A.indices[A.indptr[5]:A.indptr[6]] == 5] = np.inf
    assert run(emul, tmp_path, A, 16, b)[0] == E_DIAGONAL


def test_under_sanitizers(emul_san, tmp_path):
    """the same program with the address and undefined-behaviour sanitizers: a case of every kind (run() raises where the program does not exit clean)"""
    A = poisson2d()
    for B, blocks in ((64, 25), (96, 17), (2048, 1), (1, 1600)):
        _check(emul_san, tmp_path, "poisson 40^2 (sanitizers)", A, B, blocks)
    _check(emul_san, tmp_path, "upwind (sanitizers)", midsize.convection_diffusion(6), 50, 5)
    assert run(emul_san, tmp_path, chains(), 64, np.ones(400))[0] == E_GROWTH
    bad = sp.csr_array(poisson2d(12), copy=True)
    bad.data[0] = 0.0
    assert run(emul_san, tmp_path, bad, 16, np.ones(144))[0] == E_DIAGONAL
