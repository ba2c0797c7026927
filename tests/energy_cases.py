"""The cases of tests/golden/kernels_energy.npz (written by tests/golden/make_golden_energy.py on the reference) and the checks that the
host replay (test_energy_host.py) and the device (test_gpu_energy.py) share."""
from pathlib import Path

import numpy as np
import scipy.sparse as sp

GOLDEN = Path(__file__).resolve().parent / "golden" / "kernels_energy.npz"

IMM = ["grid9x7", "elas2x3", "elas3x6", "unsortedB", "crafted"]
SC = ["nd1", "nd3", "nd6", "nd_gt_cols", "oneblock", "zero_btbinv"]
CG = ["sa_poisson", "sa_aniso", "sa_elas", "rn_poisson", "rn_aniso", "rn_elas", "bigtol", "diagonal"]
BAR = 1e-10                                                 # the project's fp64 parity bar

_data = None


def data():
    global _data
    if _data is None:
        with np.load(GOLDEN, allow_pickle=False) as z:
            _data = {k: z[k] for k in z.files}
    return _data


def bsr(prefix):
    d = data()
    x = d[prefix + ".data"]
    n, nc = (int(v) for v in d[prefix + ".shape"])
    return sp.bsr_array((x.copy(), d[prefix + ".indices"].copy(), d[prefix + ".indptr"].copy()), shape=(n, nc))


def put_bsr(out, prefix, M):
    M = sp.bsr_array(M) if M.format != "bsr" else M
    out[prefix + ".data"] = np.ascontiguousarray(M.data, dtype=np.float64)
    out[prefix + ".indices"] = M.indices.astype(np.int32)
    out[prefix + ".indptr"] = M.indptr.astype(np.int32)
    out[prefix + ".shape"] = np.array(M.shape, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ the two kernel-level pieces
def imm_inputs(name):
    A, B, S = bsr(f"imm.{name}.A"), bsr(f"imm.{name}.B"), bsr(f"imm.{name}.S")
    return A, B, S, data()[f"imm.{name}.out"]


def run_imm(core, name, **kw):
    A, B, S, want = imm_inputs(name)
    Sx = np.ravel(S.data).copy()
    r, m = A.blocksize
    c = B.blocksize[1]
    core.incomplete_mat_mult_bsr(A.indptr, A.indices, np.ravel(A.data), B.indptr, B.indices, np.ravel(B.data), S.indptr, S.indices, Sx,
                                 A.shape[0] // r, B.shape[1] // c, r, m, c, **kw)
    return Sx, np.ravel(want)


def sc_inputs(name):
    d = data()
    return bsr(f"sc.{name}.U"), d[f"sc.{name}.B"].copy(), d[f"sc.{name}.BtBinv"].copy(), d[f"sc.{name}.UB"].copy(), d[f"sc.{name}.out"]


def run_helper(core, name, **kw):
    U, B, BtBinv, UB, want = sc_inputs(name)
    r, c = U.blocksize
    Sx = np.ravel(U.data).copy()
    core.satisfy_constraints_helper(r, c, U.shape[0] // r, B.shape[1], np.conjugate(np.ravel(B)), np.ravel(UB), np.ravel(BtBinv), U.indptr,
                                    U.indices, Sx, **kw)
    return Sx, np.ravel(want)


def run_satisfy(en, name):
    U, B, BtBinv, _, want = sc_inputs(name)
    back = en.satisfy_constraints(U, B, BtBinv)
    assert back is U                                         # in place, and returned
    return np.ravel(U.data), np.ravel(want)


# ------------------------------------------------------------------------------------------------ the whole smoother
def cg_inputs(name):
    d = data()
    p = f"cg.{name}"
    A, T, pattern = bsr(p + ".A"), bsr(p + ".T"), bsr(p + ".pattern")
    rooted = bool(d[p + ".rooted"])
    params = (False, {})
    if rooted:
        P_I = bsr(p + ".P_I")
        bs = T.blocksize[0]
        I_F = sp.bsr_array(sp.diags_array(d[p + ".I_F_diag"], format="csr"), blocksize=(bs, bs))
        I_F.eliminate_zeros()
        params = (True, {"P_I": P_I, "I_F": I_F})
    kw = {"maxiter": int(d[p + ".maxiter"]), "tol": float(d[p + ".tol"]), "weighting": str(d[p + ".weighting"]), "Cpt_params": params}
    return A, T, d[p + ".B"].copy(), d[p + ".BtBinv"].copy(), pattern, kw


def run_cg(en, name):
    A, T, B, BtBinv, pattern, kw = cg_inputs(name)
    return en.cg_prolongation_smoothing(A, T, B, BtBinv, pattern, kw["maxiter"], kw["tol"], kw["weighting"], kw["Cpt_params"])


def cg_differences(name, got, sums, show=print):
    """the figures the driver tests assert on, printed first: newsum relative to itself, T and T @ B relative to max |T|"""
    d = data()
    p = f"cg.{name}"
    want, wsums, B = d[p + ".T_out"], d[p + ".newsums"], d[p + ".B"]
    G = got.toarray()
    assert G.shape == want.shape and len(sums) == len(wsums), (name, len(sums), len(wsums))
    scale = np.abs(want).max()
    dT = np.abs(G - want).max() / scale
    dTB = np.abs(G @ B - d[p + ".TB_out"]).max() / scale
    dS = max((abs(g - w) / abs(w) for g, w in zip(sums, wsums)), default=0.0)
    show(f"[energy] {name}: iterations {len(wsums)}, |dT|/max|T| = {dT:.2e}, |d(TB)|/max|T| = {dTB:.2e}, |dnewsum|/newsum = {dS:.2e}")
    return dT, dTB, dS


def c_rows_are_injected(name, got):
    d = data()
    p = f"cg.{name}"
    if not bool(d[p + ".rooted"]):
        return 0
    rows = np.flatnonzero(d[p + ".I_F_diag"] == 0.0)
    assert np.array_equal(got.toarray()[rows], bsr(p + ".P_I").toarray()[rows])
    return rows.size
