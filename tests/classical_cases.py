"""The committed cases of the classical (Ruge-Stuben) setup (tests/golden/kernels_classical.npz, written by
tests/golden/make_golden_classical.py from the reference) and the checks the host replay and the device share: every comparison is
``np.array_equal`` on indptr, indices, data and the splittings -- there is no tolerance."""
from functools import lru_cache
from pathlib import Path

import numpy as np
import scipy.sparse as sp

GOLDEN = Path(__file__).resolve().parent / "golden" / "kernels_classical.npz"


@lru_cache(maxsize=1)
def data():
    with np.load(GOLDEN) as z:
        d = {k: z[k] for k in z.files}
    for v in d.values():
        v.setflags(write=False)                              # shared among the tests: nobody changes it
    return d


def names(family):
    return [str(s) for s in data()[family + ".names"]]


def csr(prefix, shape=None, values=True):
    d = data()
    indptr, indices = d[prefix + ".indptr"].copy(), d[prefix + ".indices"].copy()
    x = d[prefix + ".data"].copy() if values else np.ones(indices.size)
    n = indptr.size - 1
    return sp.csr_array((x, indices, indptr), shape=shape or (n, n))


def same_csr(M, prefix, values=True):
    d = data()
    assert sp.issparse(M) and M.format == "csr"
    assert np.array_equal(M.indptr, d[prefix + ".indptr"]), prefix
    assert np.array_equal(M.indices, d[prefix + ".indices"]), prefix
    if values:
        assert M.data.dtype == np.float64 and np.array_equal(M.data, d[prefix + ".data"]), prefix


STRENGTH = [(op, norm, k) for op in ("grid9x7", "odd150") for norm in ("abs", "min") for k in range(3)]
# every prolongator the fixture holds: 'direct' and 'mod' for every case, 'unmod' where the reference's result is finite
INTERP = [(c, str(kind)) for c in names("int") for kind in data()[f"int.{c}.kinds"]]


def check_strength(cls, op, norm, k):
    A = csr(f"str.{op}.A")
    keep = (A.indptr.copy(), A.indices.copy(), A.data.copy())
    S = cls.classical_strength_of_connection(A, theta=float(data()["str.thetas"][k]), norm=norm)
    same_csr(S, f"str.{op}.{norm}.{k}")
    assert S.shape == A.shape
    for a, b in zip(keep, (A.indptr, A.indices, A.data)):
        assert np.array_equal(a, b)                          # the operator is not touched


def check_mis(cls, name):
    d = data()
    G = csr(f"mis.{name}.G", values=False)
    rounds = []
    mis = cls.MIS(G, d[f"mis.{name}.weights"].copy(), rounds=rounds)
    assert mis.dtype == np.intc and np.array_equal(mis, d[f"mis.{name}.mis"])
    assert len(rounds) == 1 and 1 <= rounds[0] <= G.shape[0]
    return rounds[0]


def check_pmis(cls, name):
    d = data()
    S = csr(f"pmis.{name}.S", values=False)
    np.random.seed(int(d[f"pmis.{name}.seed"]))
    rounds = []
    splitting = cls.PMIS(S, rounds=rounds)
    follow = np.random.rand()
    assert splitting.dtype == np.intc and np.array_equal(splitting, d[f"pmis.{name}.splitting"])
    np.random.seed(int(d[f"pmis.{name}.seed"]))
    np.random.rand(S.shape[0])
    assert follow == np.random.rand()                        # exactly the reference's draw was consumed
    assert 1 <= rounds[0] <= S.shape[0]
    return splitting


def check_interp(cls, case, kind):
    d = data()
    A, C = csr(f"int.{case}.A"), csr(f"int.{case}.C")
    splitting = d[f"int.{case}.splitting_rs" if kind == "unmod" else f"int.{case}.splitting"].copy()
    if kind == "direct":
        P = cls.direct_interpolation(A, C, splitting)
    else:
        P = cls.classical_interpolation(A, C, splitting, modified=(kind == "mod"))
    same_csr(P, f"int.{case}.{kind}")
    assert P.shape == (A.shape[0], int(d[f"int.{case}.{kind}.nc"]))
    same_csr(C, f"int.{case}.C")                             # the caller's strength matrix is copied, not changed
