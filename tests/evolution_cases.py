"""The committed cases of the evolution strength of connection (tests/golden/kernels_evolution.npz, written by
tests/golden/make_golden_evolution.py from the reference) and the checks the host replay and the device share: every comparison is
``np.array_equal`` on indptr, indices and data -- there is no tolerance."""
import warnings
from functools import lru_cache
from pathlib import Path

import numpy as np
import scipy.sparse as sp

GOLDEN = Path(__file__).resolve().parent / "golden" / "kernels_evolution.npz"

IMM = ["grid9x7", "rand97", "arrow130"]
HELPER = [(c, p) for c in ("nd2", "nd3", "nd6", "craft") for p in ("l2", "D_A")]
FILTER = [(kind, k) for kind in ("rel", "abs") for k in (0, 1)]
MIN_BLOCKS = [2, 3]
WHOLE = ["poisson12x11", "aniso_k1", "aniso_k2", "aniso_k3", "aniso_k4", "aniso_inf", "aniso_nosym", "advection", "bzeros", "elas_bsr",
         "elas_bsr_block"]


def _small():
    return sp.csr_array(sp.diags_array([-np.ones(5), 2.0 * np.ones(6), -np.ones(5)], offsets=[-1, 0, 1], format="csr"))


# bad inputs, in the order of the reference's checks: each is (A, B, keywords); a later entry that is wrong twice names the check that
# must fire first
BAD = [("epsilon_below_one", lambda: (_small(), None, {"epsilon": 0.5})),
       ("zero_steps", lambda: (_small(), None, {"k": 0})),
       ("projection", lambda: (_small(), None, {"proj_type": "l1"})),
       ("csc_operator", lambda: (_small().tocsc(), None, {})),
       ("dense_operator", lambda: (_small().toarray(), None, {})),
       ("epsilon_before_steps", lambda: (_small(), None, {"epsilon": 0.5, "k": 0})),
       ("steps_before_projection", lambda: (_small(), None, {"k": -1, "proj_type": "l1"})),
       ("projection_before_format", lambda: (_small().tocsc(), None, {"proj_type": "l1"})),
       ("epsilon_before_format", lambda: (_small().toarray(), None, {"epsilon": 0.0}))]


@lru_cache(maxsize=1)
def data():
    with np.load(GOLDEN) as z:
        d = {k: z[k] for k in z.files}
    for v in d.values():
        v.setflags(write=False)                              # shared among the tests: nobody changes it
    return d


def csr(prefix, shape=None, fmt="csr"):
    d = data()
    indptr, indices, x = d[prefix + ".indptr"].copy(), d[prefix + ".indices"].copy(), d[prefix + ".data"].copy()
    n = indptr.size - 1
    return (sp.csr_array if fmt == "csr" else sp.csc_array)((x, indices, indptr), shape=shape or (n, n))


def same_csr(M, prefix):
    d = data()
    assert sp.issparse(M) and M.format == "csr"
    assert np.array_equal(M.indptr, d[prefix + ".indptr"]), prefix
    assert np.array_equal(M.indices, d[prefix + ".indices"]), prefix
    assert M.data.dtype == np.float64 and np.array_equal(M.data, d[prefix + ".data"]), prefix


def check_imm(core, name):
    A, B, S = csr(f"imm.{name}.A"), csr(f"imm.{name}.B", fmt="csc"), csr(f"imm.{name}.S")
    Sx = np.full(S.nnz, np.nan)
    core.incomplete_mat_mult_csr(A.indptr, A.indices, A.data, B.indptr, B.indices, B.data, S.indptr, S.indices, Sx, A.shape[0])
    assert np.array_equal(Sx, S.data)
    assert not np.any(np.signbit(Sx[S.data == 0.0]))         # an entry without a common index is +0.0
    return Sx


def check_helper(core, case, proj):
    d, p = data(), f"hlp.{case}.{proj}"
    S = csr(p + ".S")
    Sx = S.data.copy()
    nd = int(d[p + ".NullDim"])
    core.evolution_strength_helper(Sx, S.indptr, S.indices, S.shape[0], d[p + ".x"].copy(), d[p + ".y"].copy(), d[p + ".b"].copy(),
                                   nd * (nd + 1) // 2, nd, float(d[p + ".tol"]))
    assert np.array_equal(Sx, d[p + ".out"])
    return S, Sx


def check_filter(core, kind, k):
    d = data()
    S = csr("flt.S")
    x = S.data.copy()
    fn = core.apply_distance_filter if kind == "rel" else core.apply_absolute_distance_filter
    fn(S.shape[0], float(d["flt.eps"][k]), S.indptr, S.indices, x)
    assert np.array_equal(x, d[f"flt.{kind}.{k}"])


def check_min_blocks(core, bs):
    d = data()
    blocks = d[f"mb.{bs}.in"].copy()
    T = np.zeros(blocks.shape[0])
    core.min_blocks(blocks.shape[0], bs * bs, np.ravel(blocks), T)
    assert np.array_equal(T, d[f"mb.{bs}.out"])


def whole_inputs(name):
    d, p = data(), f"whole.{name}"
    if p + ".A.bsr_data" in d:
        bd = d[p + ".A.bsr_data"].copy()
        nb = d[p + ".A.indptr"].size - 1
        A = sp.bsr_array((bd, d[p + ".A.indices"].copy(), d[p + ".A.indptr"].copy()), shape=(nb * bd.shape[1], nb * bd.shape[2]))
    else:
        A = csr(p + ".A")
    B = d[p + ".B"].copy() if p + ".B" in d else None
    e, k, proj, bf, sym = d[p + ".kw"]
    kw = {"epsilon": float(e), "k": int(k), "proj_type": ("l2", "D_A")[int(proj)], "block_flag": bool(bf), "symmetrize_measure": bool(sym)}
    return A, B, kw


def run_whole(evo, name, A=None, B=None):
    A0, B0, kw = whole_inputs(name)
    A, B = (A0, B0) if A is None else (A, B)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # k = 3: the reference's own warning about time steps
        return A, B, evo.evolution_strength_of_connection(A, B, **kw)


REFUSED = ["elas_bsr_block"]         # the reference raises inside (the fixture records what); the drop-in leaves the call to it


def check_whole(evo, name):
    """with the module's approximate_spectral_radius already replaced by the recorded rho"""
    import pytest
    d, p = data(), f"whole.{name}"
    if name in REFUSED:
        assert p + ".exc" in d
        A, B, _ = whole_inputs(name)
        keep = (A.data.copy(), B.copy())
        with pytest.raises(NotImplementedError):
            run_whole(evo, name, A, B)
        assert np.array_equal(A.data, keep[0]) and np.array_equal(B, keep[1])      # refused before anything is touched
        return None
    if p + ".exc" in d:
        import builtins
        with pytest.raises(getattr(builtins, str(d[p + ".exc"]))):
            run_whole(evo, name)
        return None
    A, B, C = run_whole(evo, name)
    same_csr(C, p + ".C")
    assert C.indptr.dtype.name == str(d[p + ".C.index_dtype"]) and C.indices.dtype == C.indptr.dtype
    if p + ".A_after.data" in d:
        same_csr(A, p + ".A_after")                          # eliminate_zeros and sort_indices on the caller's operator
    if B is not None:
        assert np.array_equal(B, d[p + ".B_after"])          # one candidate: its zeros are ones now
    return C


def certified():
    """the whole-function cases whose pattern the generator found unchanged at rho (1 - d), rho and rho (1 + d)"""
    return [str(s) for s in data()["whole.certified"]]
