"""The committed cases of the relaxation-vector and vertex-distance strength measures (tests/golden/kernels_distance.npz, written by
tests/golden/make_golden_distance.py from the reference) and the checks the host replay and the device share: every comparison is
``np.array_equal`` on indptr, indices and data -- there is no tolerance."""
import warnings
from functools import lru_cache
from pathlib import Path

import numpy as np
import scipy.sparse as sp

GOLDEN = Path(__file__).resolve().parent / "golden" / "kernels_distance.npz"

OPERATORS = ["poisson12x11", "aniso10x9", "rand97", "arrow130", "zeros7x5"]
MEASURES = ["algebraic_p1", "algebraic_p2", "algebraic_pinf", "affinity"]
P_OF = {"algebraic_p1": 1, "algebraic_p2": 2, "algebraic_pinf": np.inf}

# (operator, measure, R, k, epsilon, alpha).  Every operator meets every measure; every R in {1, 5, 7, 8, 9, 17, 32} (both sides of the
# change of summation order, a remainder after the groups of eight, the cap) meets every measure; k in {1, 2, 20} (odd and even buffer
# parity), epsilon in {1, 2, 4} and alpha in {0, 0.5, 0.7} meet every measure and every operator.  The large blocks sit on the small
# operators: the random block does not compress.
CASES = [("poisson12x11", "algebraic_p2", 5, 20, 2.0, 0.5),             # the defaults of algebraic_distance
         ("poisson12x11", "affinity", 5, 20, 4.0, 0.5),                 # the defaults of affinity_distance
         ("poisson12x11", "algebraic_p1", 7, 2, 1.0, 0.7),
         ("poisson12x11", "algebraic_pinf", 8, 1, 2.0, 0.0),
         ("aniso10x9", "algebraic_p2", 9, 2, 4.0, 0.7),
         ("aniso10x9", "affinity", 8, 1, 2.0, 0.0),
         ("aniso10x9", "algebraic_p1", 5, 20, 1.0, 0.5),
         ("aniso10x9", "algebraic_pinf", 1, 2, 4.0, 0.7),
         ("rand97", "algebraic_p2", 5, 1, 1.0, 0.0),
         ("rand97", "affinity", 9, 2, 1.0, 0.7),
         ("rand97", "algebraic_p1", 8, 20, 4.0, 0.5),
         ("rand97", "algebraic_pinf", 7, 2, 2.0, 0.5),
         ("arrow130", "algebraic_p2", 8, 1, 2.0, 0.5),
         ("arrow130", "affinity", 5, 2, 4.0, 0.5),
         ("arrow130", "algebraic_p1", 1, 20, 2.0, 0.7),
         ("arrow130", "algebraic_pinf", 5, 1, 1.0, 0.0),
         ("zeros7x5", "algebraic_p2", 32, 1, 2.0, 0.5),
         ("zeros7x5", "affinity", 32, 2, 4.0, 0.7),
         ("zeros7x5", "algebraic_p1", 32, 20, 2.0, 0.0),
         ("zeros7x5", "algebraic_pinf", 32, 2, 4.0, 0.5),
         ("zeros7x5", "algebraic_p2", 17, 2, 4.0, 0.0),
         ("zeros7x5", "affinity", 17, 1, 2.0, 0.5),
         ("zeros7x5", "algebraic_p1", 17, 1, 4.0, 0.5),
         ("zeros7x5", "algebraic_pinf", 17, 20, 1.0, 0.7),
         ("zeros7x5", "algebraic_p2", 7, 20, 1.0, 0.7),
         ("zeros7x5", "algebraic_p2", 1, 2, 2.0, 0.5),
         ("zeros7x5", "affinity", 7, 20, 2.0, 0.5),
         ("zeros7x5", "affinity", 1, 1, 4.0, 0.5),                      # one vector: every affinity is 0 or a rounding error away from it
         ("zeros7x5", "algebraic_p1", 9, 2, 2.0, 0.5),
         ("zeros7x5", "algebraic_pinf", 9, 1, 2.0, 0.5)]
IDS = [f"{o}-{m}-R{R}-k{k}-e{e:g}-a{a:g}" for o, m, R, k, e, a in CASES]

# distance_strength_of_connection: (case, theta, relative_drop)
VERTEX = [("grid2d", 2.0, True), ("grid2d_abs", 1.5, False), ("line1d_abs", 0.3, False), ("cloud3d", 2.0, True), ("cloud3d_inf", np.inf, True),
          ("cloud3d_abs", 0.4, False), ("elas_bsr", 2.0, True)]


def _small():
    return sp.csr_array(sp.diags_array([-np.ones(5), 2.0 * np.ones(6), -np.ones(5)], offsets=[-1, 0, 1], format="csr"))


# bad arguments, in the order of the reference's checks: (name, function, keywords); an entry that is wrong twice names the check that
# must fire first
BAD = [("alpha_negative", "algebraic_distance", {"alpha": -0.1}),
       ("R_zero", "algebraic_distance", {"R": 0}),
       ("R_float", "algebraic_distance", {"R": 5.0}),
       ("k_zero", "algebraic_distance", {"k": 0}),
       ("k_float", "algebraic_distance", {"k": 2.0}),
       ("epsilon_below_one", "algebraic_distance", {"epsilon": 0.5}),
       ("p_below_one", "algebraic_distance", {"p": 0.5}),
       ("alpha_before_R", "algebraic_distance", {"alpha": -1.0, "R": 0}),
       ("R_before_k", "algebraic_distance", {"R": -1, "k": 0}),
       ("k_before_epsilon", "algebraic_distance", {"k": 0, "epsilon": 0.0}),
       ("epsilon_before_p", "algebraic_distance", {"epsilon": 0.5, "p": 0.0}),
       ("aff_alpha_negative", "affinity_distance", {"alpha": -0.1}),
       ("aff_R_zero", "affinity_distance", {"R": 0}),
       ("aff_R_float", "affinity_distance", {"R": 3.0}),
       ("aff_k_zero", "affinity_distance", {"k": 0}),
       ("aff_epsilon_below_one", "affinity_distance", {"epsilon": 0.99}),
       ("aff_R_before_epsilon", "affinity_distance", {"R": 0, "epsilon": 0.0})]


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


def same_csr(M, prefix):
    d = data()
    assert sp.issparse(M) and M.format == "csr"
    assert np.array_equal(M.indptr, d[prefix + ".indptr"]), prefix
    assert np.array_equal(M.indices, d[prefix + ".indices"]), prefix
    assert M.data.dtype == np.float64 and np.array_equal(M.data, d[prefix + ".data"]), prefix
    assert M.indptr.dtype.name == str(d[prefix + ".index_dtype"]) and M.indices.dtype == M.indptr.dtype, prefix


def operator(name):
    return csr(f"op.{name}")


def seed_of(i):
    return int(data()["case.seeds"][i])


def check_relaxation(core, i):
    """stage 1: the recorded random block through k sweeps"""
    d = data()
    op, _, R, k, _, alpha = CASES[i]
    A = operator(op)
    n = A.shape[0]
    X = d[f"case.{i}.x0"].copy()
    assert X.shape == (n * R,)
    core.relaxation_vectors(A.indptr, A.indices, A.data, X, n, R, k, alpha)
    assert np.array_equal(X, d[f"case.{i}.x"])
    return A, X


def check_measure(core, i):
    """stage 2: the recorded relaxed block through the measure, on A's pattern"""
    import pyamg_amd._capi as capi
    d = data()
    op, measure, R, _, _, _ = CASES[i]
    A = operator(op)
    Dx = np.full(A.nnz, np.nan)
    core.distance_measure(capi.DISTANCE[measure], A.indptr, A.indices, A.data, d[f"case.{i}.x"].copy(), A.shape[0], R, Dx)
    assert np.array_equal(Dx, d[f"case.{i}.d"])
    return A, Dx


def check_chain(core, i):
    """the resident chain: what it leaves on A's pattern, with the zeros eliminated, is the pattern and the distances of the reference's
    filtered matrix (1 / the off-diagonal data of the final C before its scaling is not recorded; the pattern and X are)"""
    import pyamg_amd._capi as capi
    d = data()
    op, measure, R, k, eps, alpha = CASES[i]
    A = operator(op)
    n = A.shape[0]
    X = d[f"case.{i}.x0"].copy()
    Dx = np.full(A.nnz, np.nan)
    core.distance_strength(capi.DISTANCE[measure], A.indptr, A.indices, A.data, X, n, R, k, alpha, eps, Dx)
    assert np.array_equal(X, d[f"case.{i}.x"])
    kept = Dx != 0.0
    assert np.array_equal(Dx[kept], d[f"case.{i}.d"][kept])              # the filter changes no value it keeps
    assert np.array_equal(np.flatnonzero(kept), d[f"case.{i}.kept"])     # and keeps what apply_distance_filter kept in the reference
    return Dx


def run_whole(mod, i):
    op, measure, R, k, eps, alpha = CASES[i]
    A = operator(op)
    np.random.seed(seed_of(i))
    if measure == "affinity":
        return A, mod.affinity_distance(A, alpha=alpha, R=R, k=k, epsilon=eps)
    return A, mod.algebraic_distance(A, alpha=alpha, R=R, k=k, epsilon=eps, p=P_OF[measure])


def check_whole(mod, i):
    """the whole function through the Python surface on the recorded seed: the reference's matrix, its stream of random numbers, and the
    caller's operator untouched"""
    op, _, R, _, _, _ = CASES[i]
    before = operator(op)
    A, C = run_whole(mod, i)
    same_csr(C, f"case.{i}.C")
    state = np.random.get_state()
    np.random.seed(seed_of(i))
    np.random.rand(A.shape[0] * R)
    want = np.random.get_state()
    assert state[0] == want[0] and np.array_equal(state[1], want[1]) and state[2:] == want[2:]      # exactly n * R numbers were drawn
    assert np.array_equal(A.indptr, before.indptr) and np.array_equal(A.indices, before.indices) and np.array_equal(A.data, before.data)
    return C


def vertex_inputs(name):
    d, p = data(), f"vd.{name}"
    if p + ".A.bsr_data" in d:
        bd = d[p + ".A.bsr_data"].copy()
        nb = d[p + ".A.indptr"].size - 1
        A = sp.bsr_array((bd, d[p + ".A.indices"].copy(), d[p + ".A.indptr"].copy()), shape=(nb * bd.shape[1], nb * bd.shape[2]))
    else:
        A = csr(p + ".A")
    return A, d[p + ".V"].copy()


def check_vertex_entries(core, name):
    d, p = data(), f"vd.{name}"
    if p + ".Cx" not in d:                                   # theta = inf: the reference calls no filter, so nothing was recorded
        return None
    A, V = vertex_inputs(name)
    Ap, Aj = A.indptr, A.indices
    n = Ap.size - 1
    Cx = np.full(Aj.size, np.nan)
    core.vertex_distance(Ap, Aj, V.reshape(-1), n, V.shape[1], Cx)
    assert np.array_equal(Cx, d[p + ".Cx"])
    return Cx


def check_vertex_whole(mod, name, theta, relative_drop):
    A, V = vertex_inputs(name)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # a CSR or BSR operator: no conversion, no warning
        C = mod.distance_strength_of_connection(A, V, theta=theta, relative_drop=relative_drop)
    same_csr(C, f"vd.{name}.C")
    return C
