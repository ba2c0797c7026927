"""The cases of tests/golden/kernels_rootnode.npz (written by tests/golden/make_golden_rootnode.py on the reference), the host replay of
csrc/pamg_rootnode.hip (tests/rootnode_emul.cpp) behind amg_core's names, and the checks that the host tests (test_rootnode_host.py)
and the device tests (test_gpu_rootnode.py) share."""
import ctypes
import json
import subprocess
from pathlib import Path

import numpy as np
import scipy.sparse as sp

import schwarz_setup_cases as ssc
from energy_cases import put_bsr  # noqa: F401  (the generator stores matrices the same way)

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
GOLDEN = HERE / "golden" / "kernels_rootnode.npz"

BTB = ["k1", "k3", "k6", "crafted", "rankdef"]
SCALE = ["rn_poisson", "rn_aniso", "rn_elas", "no_coarse"]
FILTER = ["rn_elas"]
RELAX = ["gs_aniso", "bgs_elas", "jacobi_poisson"]
BAR = 1e-10                                                 # the project's fp64 parity bar
BOUND = ssc.BOUND                                           # |X - X_ref|_F <= BOUND eps kappa_+ |X_ref|_F

_data = None


def data():
    global _data
    if _data is None:
        with np.load(GOLDEN, allow_pickle=False) as z:
            _data = {k: z[k] for k in z.files}
    return _data


def mat(prefix):
    """a stored matrix: BSR, or CSR where the generator stored one (<prefix>.csr)"""
    d = data()
    n, nc = (int(v) for v in d[prefix + ".shape"])
    M = sp.bsr_array((d[prefix + ".data"].copy(), d[prefix + ".indices"].copy(), d[prefix + ".indptr"].copy()), shape=(n, nc))
    if prefix + ".csr" in d and bool(d[prefix + ".csr"]):
        M = sp.csr_array((M.data.reshape(-1), M.indices, M.indptr), shape=(n, nc))
    return M


def same_matrix(got, want):
    """the structure and the values, array for array"""
    return got.format == want.format and got.shape == want.shape and np.array_equal(got.indptr, want.indptr) and \
        np.array_equal(got.indices, want.indices) and np.array_equal(got.data, want.data)


# ------------------------------------------------------------------------------------------------ the replay behind amg_core's names
class EmulCore:
    """what pyamg_amd.rootnode calls of pyamg_amd.amg_core, on the host replay"""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    @staticmethod
    def p(a):
        if a is None:
            return ctypes.c_void_p(0)
        assert isinstance(a, np.ndarray) and a.flags.c_contiguous and a.dtype in (np.int32, np.float64)
        return a.ctypes.data_as(ctypes.c_void_p)

    @staticmethod
    def done(rc):
        if rc == -2:
            raise NotImplementedError("replay: not supported on the device path")        # what _capi.check makes of PAMG_E_UNSUPPORTED
        assert rc == 0, rc

    def calc_BtB(self, K, n, cpb, b, BsqCols, x, Sp, Sj):
        self.calls.append("calc_BtB")
        assert x.size == n * K * K and Sp.size == n + 1
        self.done(self.lib.rn_calc_BtB(int(K), int(n), int(cpb), self.p(b), b.size, int(BsqCols), self.p(x), self.p(Sp), self.p(Sj)))

    def compute_BtBinv(self, K, n, cpb, B, Sp, Sj, BtBinv, BtB=None):
        self.calls.append("compute_BtBinv")
        assert BtBinv.size == n * K * K and Sp.size == n + 1
        self.done(self.lib.rn_compute_BtBinv(int(K), int(n), int(cpb), self.p(B), ctypes.c_int64(B.size), self.p(Sp), self.p(Sj), self.p(BtB), self.p(BtBinv)))

    def filter_constraints(self, r, c, n, K, B, Bf, BtBinv, Sp, Sj, Sx):
        self.calls.append("filter_constraints")
        assert Bf.size == n * r * K and BtBinv.size == n * K * K and Sx.size == Sp[-1] * r * c
        self.done(self.lib.rn_filter_constraints(int(r), int(c), int(n), int(K), self.p(B), B.size, self.p(Bf), self.p(BtBinv), self.p(Sp), self.p(Sj),
                                                 self.p(Sx)))

    def scale_T(self, n, nbc, bs, Tp, Tj, Tx, Cnodes):
        self.calls.append("scale_T")
        assert Tx.size == Tp[-1] * bs * bs and Cnodes.size == nbc
        self.done(self.lib.rn_scale_T(int(n), int(nbc), int(bs), self.p(Tp), self.p(Tj), self.p(Tx), self.p(Cnodes)))


NAMES = ["calc_BtB", "compute_BtBinv", "filter_constraints", "scale_T"]


def build_emul():
    out = HERE / "build"
    out.mkdir(exist_ok=True)
    so, src = out / "rootnode_emul.so", HERE / "rootnode_emul.cpp"
    deps = [src] + [ROOT / "pyamg_amd" / "csrc" / h for h in ("pamg_rootnode.h", "pamg_energy.h", "pamg_jacobi_svd.h")]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    for f in (lib.rn_calc_BtB, lib.rn_compute_BtBinv, lib.rn_filter_constraints, lib.rn_scale_T):
        f.restype = ctypes.c_int
    return lib


# ------------------------------------------------------------------------------------------------ calc_BtB / compute_BtBinv
def btb_inputs(name):
    d = data()
    p = f"btb.{name}"
    return d[p + ".B"].copy(), mat(p + ".C"), d[p + ".BtB"], d[p + ".BtBinv"]


def bsq(B):
    """Bsq as compute_BtBinv forms it (utils.py:1603-1610)"""
    K = B.shape[1]
    cols = [np.conjugate(B[:, i]) * B[:, j] for i in range(K) for j in range(i, K)]
    return np.ascontiguousarray(np.stack(cols, axis=1))


def run_calc_BtB(core, name):
    B, C, want, _ = btb_inputs(name)
    K = B.shape[1]
    r, c = C.blocksize if C.format == "bsr" else (1, 1)
    n = C.shape[0] // r
    x = np.zeros(n * K * K)
    core.calc_BtB(K, n, c, np.ravel(bsq(B)), K * (K + 1) // 2, x, C.indptr.astype(np.int32), C.indices.astype(np.int32))
    return x.reshape(n, K, K), want


class _Blocks:
    """the BtB blocks of a case in the shape schwarz_setup_cases.compare_blocks reads: n blocks of K x K one after another"""

    def __init__(self, name, BtB, inv):
        n, K = BtB.shape[0], BtB.shape[1]
        self.name, self.dtype = name, np.dtype(np.float64)
        self.sptr = np.arange(n + 1, dtype=np.int32) * K
        self.tptr = np.arange(n + 1, dtype=np.int32) * K * K
        self.blocks = np.ascontiguousarray(BtB.transpose(0, 2, 1)).reshape(-1)          # the deep transpose: what pinv_array inverts
        self.inv = np.ascontiguousarray(inv).reshape(-1)


def inverse_check(name, got, show=print):
    """the inverse of a case against the reference's: array_equal for one candidate, the Schwarz setup's comparison otherwise (equal
    ranks, no decision on a knife edge, |X - X_ref|_F <= BOUND eps kappa_+ |X_ref|_F); returns the worst ratio to eps kappa_+ |X_ref|"""
    _, _, BtB, want = btb_inputs(name)
    assert got.shape == want.shape
    if want.shape[1] == 1:
        assert np.array_equal(got, want), name
        return 0.0
    worst, truncated = ssc.compare_blocks(_Blocks(name, BtB, want), np.ascontiguousarray(got).reshape(-1))
    show(f"[rootnode] BtBinv {name}: worst |X - X_ref| / (eps kappa_+ |X_ref|) = {worst:.2f} (bound {BOUND}), {truncated} truncated blocks")
    assert worst <= BOUND, (name, worst)
    return worst


# ------------------------------------------------------------------------------------------------ scale_T / filter_operator
def rooted(prefix, bs):
    d = data()
    I_F = sp.bsr_array(sp.diags_array(d[prefix + ".I_F_diag"], format="csr"), blocksize=(bs, bs))
    I_F.eliminate_zeros()
    return mat(prefix + ".P_I"), I_F


def scale_inputs(name):
    p = f"st.{name}"
    T = mat(p + ".T")
    P_I, I_F = rooted(p, T.blocksize[0])
    return T, P_I, I_F, mat(p + ".out")


def scale_check(name, got, show=print):
    """the structure is SciPy's; 1 x 1 blocks equal the reference's; larger ones agree through the pseudo-inverse.  A stored block is
    T_p X with X = pinv(D_a): both sides round the same product of bs terms (bs eps |T_p| |X|) and differ in X by at most
    BOUND eps kappa_+(D_a) |X| (the inverse's bound), so |got - want|_F <= (BOUND kappa_+ + 2 bs) eps |T_p|_F |X|_F.  Returns the worst
    ratio to that bound."""
    T, P_I, I_F, want = scale_inputs(name)
    assert got.format == "bsr" and got.shape == want.shape and got.blocksize == want.blocksize
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    if T.blocksize[0] == 1 or name == "no_coarse":
        assert np.array_equal(got.data, want.data), name
        return 0.0
    bs = T.blocksize[0]
    roots = np.flatnonzero(np.diff(P_I.indptr))
    nagg = T.shape[1] // bs
    kappa, xnorm = np.ones(nagg), np.ones(nagg)
    eps = np.finfo(np.float64).eps
    for r, a in zip(roots, P_I.indices[P_I.indptr[roots]]):
        D = T.data[T.indptr[r]]
        s = np.linalg.svd(D, compute_uv=False)
        assert s[-1] > 5 * 1e6 * eps * s[0]                 # the root blocks of the fixture have full rank, far from the rank rule's edge
        kappa[a], xnorm[a] = s[0] / s[-1], np.linalg.norm(np.linalg.inv(D))
    assert np.array_equal(T.indptr, want.indptr) and np.array_equal(T.indices, want.indices)       # (no block of these cases came out zero)
    worst = 0.0
    for p, a in enumerate(want.indices):
        bound = (BOUND * kappa[a] + 2 * bs) * eps * np.linalg.norm(T.data[p]) * xnorm[a]
        worst = max(worst, np.linalg.norm(got.data[p] - want.data[p]) / bound)
    show(f"[rootnode] scale_T {name}: worst |got - want|_F / ((BOUND kappa_+ + 2 bs) eps |T_p| |X|) = {worst:.3f}")
    assert worst <= 1.0, (name, worst)
    return worst


def filter_inputs(name):
    d = data()
    p = f"fo.{name}"
    return mat(p + ".A"), mat(p + ".C"), d[p + ".B"].copy(), d[p + ".Bf"].copy(), d[p + ".BtBinv"].copy(), mat(p + ".out")


# ------------------------------------------------------------------------------------------------ candidate relaxation
def relax_inputs(name):
    d = data()
    p = f"rx.{name}"
    return (str(d[p + ".method"]), json.loads(str(d[p + ".kwargs"]))), mat(p + ".A"), d[p + ".B"].copy(), d[p + ".out"]


def e2e_operators():
    """name -> (A, B): the 300-row diffusion operator of kernels_energy.npz (one candidate) and the 10 x 10 elasticity operator"""
    import energy_cases as ec
    A = sp.csr_array(ec.bsr("e2e.A"))
    return {"diffusion": (A, None), "elasticity": (mat("e2e.elas.A"), data()["e2e.elas.B"].copy())}


def e2e_solver(pyamg, A, B):
    return pyamg.rootnode_solver(A, B=B, strength="evolution", smooth=("energy", {"krylov": "cg", "maxiter": 4}), max_coarse=20)
