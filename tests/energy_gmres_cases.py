"""The cases of tests/golden/kernels_energy_gmres.npz (written by tests/golden/make_golden_energy_gmres.py on the reference) and the
checks that the host replay (test_energy_gmres_host.py) and the device (test_gpu_energy_gmres.py) share.  The bar is energy_cases.BAR."""
from pathlib import Path

import numpy as np
import scipy.sparse as sp

from energy_cases import BAR, put_bsr  # noqa: F401

GOLDEN = Path(__file__).resolve().parent / "golden" / "kernels_energy_gmres.npz"

GMRES = ["sa_cd_P", "sa_cd_R", "rn_cd", "rn_elas", "diagonal", "maxiter1", "bigtol", "notol"]
ITERATIONS = {"sa_cd_P": 4, "sa_cd_R": 4, "rn_cd": 3, "rn_elas": 4, "diagonal": 3, "maxiter1": 1, "bigtol": 2, "notol": 0}
SUBDIAGONAL_FLOOR, COND_CEILING = 0.05, 100.0               # the conditions the generator asserts of every case

_data = None


def data():
    global _data
    if _data is None:
        with np.load(GOLDEN, allow_pickle=False) as z:
            _data = {k: z[k] for k in z.files}
    return _data


def bsr(prefix):
    d = data()
    n, nc = (int(v) for v in d[prefix + ".shape"])
    return sp.bsr_array((d[prefix + ".data"].copy(), d[prefix + ".indices"].copy(), d[prefix + ".indptr"].copy()), shape=(n, nc))


def upwind(nx, ny, epsilon=0.01, degrees=36.0):
    """-epsilon Laplace(u) + w . grad(u) on an nx x ny grid (x fastest), w = (cos, sin) of the flow angle, first-order upwind
    differences for the convection (both components of w are positive: backward differences), Dirichlet boundaries: not symmetric"""
    wx, wy = np.cos(np.deg2rad(degrees)), np.sin(np.deg2rad(degrees))

    def one(m, w):
        h = 1.0 / (m + 1)
        e = np.ones(m)
        lap = sp.diags_array([-e[:-1], 2 * e, -e[:-1]], offsets=[-1, 0, 1]) * (epsilon / h**2)
        return lap + sp.diags_array([-e[:-1], e], offsets=[-1, 0]) * (w / h)
    A = sp.csr_array(sp.kron(sp.eye_array(ny), one(nx, wx)) + sp.kron(one(ny, wy), sp.eye_array(nx)))
    A.sort_indices()
    return sp.csr_array((A.data, A.indices.astype(np.int32), A.indptr.astype(np.int32)), shape=A.shape)


def inputs(name):
    """the arguments of gmres_prolongation_smoothing of a case: (A, T, B, BtBinv, pattern, kw); a case that varies another's keeps
    only what it changes (``.args``: the case whose arrays it takes)"""
    d = data()
    p = f"gm.{name}"
    q = f"gm.{str(d[p + '.args'])}"
    A, T, pattern = bsr(q + ".A"), bsr(q + ".T"), bsr(q + ".pattern")
    params = (False, {})
    if bool(d[q + ".rooted"]):
        bs = T.blocksize[0]
        I_F = sp.bsr_array(sp.diags_array(d[q + ".I_F_diag"], format="csr"), blocksize=(bs, bs))
        I_F.eliminate_zeros()
        params = (True, {"P_I": bsr(q + ".P_I"), "I_F": I_F})
    kw = {"maxiter": int(d[p + ".maxiter"]), "tol": float(d[p + ".tol"]), "weighting": str(d[p + ".weighting"]), "Cpt_params": params}
    return A, T, d[q + ".B"].copy(), d[q + ".BtBinv"].copy(), pattern, kw


def run(en, name):
    A, T, B, BtBinv, pattern, kw = inputs(name)
    return en.gmres_prolongation_smoothing(A, T, B, BtBinv, pattern, kw["maxiter"], kw["tol"], kw["weighting"], kw["Cpt_params"])


def differences(name, got, normrs, show=print):
    """the figures the driver tests assert on, printed first: T and T @ B relative to max |T|, every normr relative to normr[0]"""
    d = data()
    p = f"gm.{name}"
    want, wn, B = d[p + ".T_out"], d[p + ".normr"], inputs(name)[2]
    G = got.toarray()
    assert G.shape == want.shape and len(normrs) == len(wn), (name, len(normrs), len(wn))
    scale = np.abs(want).max()
    dT = np.abs(G - want).max() / scale
    dTB = np.abs(G @ B - d[p + ".TB_out"]).max() / scale
    dN = float(np.max(np.abs(np.asarray(normrs) - wn)) / wn[0])
    show(f"[energy gmres] {name}: iterations {len(wn) - 1}, |dT|/max|T| = {dT:.2e}, |d(TB)|/max|T| = {dTB:.2e}, |dnormr|/normr[0] = {dN:.2e}")
    return dT, dTB, dN


def c_rows_are_injected(name, got):
    """the number of C-point rows, each equal to the injection's"""
    d = data()
    q = f"gm.{str(d[f'gm.{name}.args'])}"
    if not bool(d[q + ".rooted"]):
        return 0
    rows = np.flatnonzero(d[q + ".I_F_diag"] == 0.0)
    assert np.array_equal(got.toarray()[rows], bsr(q + ".P_I").toarray()[rows])
    return rows.size


# ------------------------------------------------------------------------------------------------ the end-to-end hierarchy
def e2e_operator():
    return upwind(20, 15)


def e2e_solver(pyamg, A):
    return pyamg.smoothed_aggregation_solver(A, symmetry="nonsymmetric", smooth=("energy", {"krylov": "gmres", "maxiter": 3}), max_coarse=20)


def hierarchies_agree(got, want):
    assert [lv.A.shape for lv in got.levels] == [lv.A.shape for lv in want.levels] and len(want.levels) >= 2
    worst = 0.0
    for lg, lw in zip(got.levels[:-1], want.levels[:-1]):
        for Mg, Mw in ((lg.P, lw.P), (lg.R, lw.R)):
            Mg, Mw = Mg.toarray(), Mw.toarray()
            worst = max(worst, np.abs(Mg - Mw).max() / np.abs(Mw).max())
    print(f"[energy gmres] hierarchy: {len(want.levels)} levels, P and R within {worst:.2e}")
    assert worst <= BAR
