"""CPU: the mid-size hierarchy builder (tests/midsize.py) the GPU parity file relies on -- Galerkin operators, R = P^T, the
smoother specs the oracle applies, a converging solve -- checked at small sizes, and that it stays independent of what it checks."""
import numpy as np
import pytest
import scipy.sparse as sp

import midsize as M
from oracle import oracle as orc


@pytest.mark.parametrize("name,bs", [("poisson:12x10x9", 1), ("elasticity:7", 3), ("convdiff:10", 1)])
def test_operators_are_galerkin_products(name, bs):
    ops = M.operators(name)
    assert len(ops) >= 2 and ops[0][3] == bs and ops[-1][1] is None
    assert ops[-1][0].shape[0] <= M.MAX_COARSE or len(ops) > 2
    for (A, P, R, _), (Ac, *_rest) in zip(ops[:-1], ops[1:]):
        assert abs(sp.csr_array(R) - sp.csr_array(P).T).max() == 0.0
        ref = sp.csr_array(R) @ sp.csr_array(A) @ sp.csr_array(P)
        assert abs(sp.csr_array(Ac) - ref).max() <= 1e-12 * abs(ref).max()
        assert Ac.shape[0] < A.shape[0]


@pytest.mark.parametrize("name,pre,post,dtype", [
    ("poisson:12x10x9", ("gs", "symmetric"), None, "float64"),
    ("poisson:12x10x9", ("gs", "symmetric"), ("sor", 1.3, "forward"), "float64"),
    ("poisson:16x16x8", ("chebyshev", 3), None, "float64"),
    ("elasticity:7", ("block_gs", "symmetric"), None, "float64"),
    ("elasticity:7", ("block_jacobi",), None, "float64"),
    ("convdiff:10", ("gs_nr", "symmetric"), None, "float64"),
    ("poisson:12x10x9", ("gs", "symmetric"), None, "float32"),
])
def test_hierarchies_converge_on_the_oracle(name, pre, post, dtype):
    spec = M.hierarchy(name, pre, post, dtype=dtype)
    assert spec.dtype == np.dtype(dtype)
    assert M.hierarchy(name, pre, post, dtype=dtype) is spec                    # cached per process
    n = spec.levels[0].A.shape[0]
    x0 = np.random.RandomState(1).rand(n).astype(dtype)
    res = []
    orc.OracleSolver(spec).solve(np.zeros_like(x0), x0=x0, tol=1e-30, maxiter=6, residuals=res)
    assert res[-1] < 0.2 * res[0], res


def test_chebyshev_coefficients_damp_the_spectrum():
    A = M.operators("poisson:16x16x8")[0][0]
    c = M.chebyshev_coefficients(A, 3)
    assert c.size == 4
    lam = np.linalg.eigvalsh(A.toarray())
    damp = np.abs(1 - lam * np.polyval(c, lam))
    assert damp.max() < 1.0


def test_builder_shares_no_code_with_the_checked_setup():
    import ast
    mods = set()
    for node in ast.walk(ast.parse(open(M.__file__).read())):
        if isinstance(node, ast.Import):
            mods.update(a.name for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            mods.add(node.module)
            mods.update(f"{node.module}.{a.name}" for a in node.names)
    for m in mods:
        assert m != "pyamg" and not m.startswith("pyamg.") and "refimport" not in m and m != "pyamg_amd.aggregation", m
