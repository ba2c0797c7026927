"""The committed cases of the CLJP / CLJP-c coarse-grid selection and of the MIS vertex colouring (tests/golden/kernels_cljp.npz, written
by tests/golden/make_golden_cljp.py from the reference) and the checks the host replay and the device share: every comparison is
``np.array_equal`` -- there is no tolerance."""
from functools import lru_cache
from pathlib import Path

import numpy as np
import scipy.sparse as sp

GOLDEN = Path(__file__).resolve().parent / "golden" / "kernels_cljp.npz"


@lru_cache(maxsize=1)
def data():
    with np.load(GOLDEN) as z:
        d = {k: z[k] for k in z.files}
    for v in d.values():
        v.setflags(write=False)                              # shared among the tests: nobody changes it
    return d


def names(family):
    return [str(s) for s in data()[family + ".names"]]


def pattern(name):
    d = data()
    indptr, indices = d[f"cljp.{name}.S.indptr"].copy(), d[f"cljp.{name}.S.indices"].copy()
    n = indptr.size - 1
    return sp.csr_array((np.ones(indices.size), indices, indptr), shape=(n, n))


def csr(prefix, shape=None):
    d = data()
    indptr = d[prefix + ".indptr"]
    n = indptr.size - 1
    return sp.csr_array((d[prefix + ".data"].copy(), d[prefix + ".indices"].copy(), indptr.copy()), shape=shape or (n, n))


def same_csr(M, prefix):
    d = data()
    assert sp.issparse(M) and M.format == "csr"
    assert np.array_equal(M.indptr, d[prefix + ".indptr"]), prefix
    assert np.array_equal(M.indices, d[prefix + ".indices"]), prefix
    assert M.data.dtype == np.float64 and np.array_equal(M.data, d[prefix + ".data"]), prefix


SPLITTINGS = [(g, color) for g in names("cljp") for color in (False, True)]


def check_cljp(cls, name, color):
    """the reference's splitting; returns (passes, colours, colouring rounds, nodes selected)"""
    d = data()
    S = pattern(name)
    keep = (S.indptr.copy(), S.indices.copy())
    n = S.shape[0]
    info = []
    splitting = cls.CLJP(S, color=True, info=info) if color else cls.CLJP(S, info=info)
    want = d[f"cljp.{name}.cljpc" if color else f"cljp.{name}.cljp"]
    assert splitting.dtype == np.intc and splitting.shape == (n,)
    assert np.array_equal(splitting, want), (name, color, np.flatnonzero(splitting != want)[:10])
    if color:
        assert np.array_equal(cls.CLJPc(S), want)
    assert np.array_equal(keep[0], S.indptr) and np.array_equal(keep[1], S.indices)       # the pattern is not touched
    assert len(info) == 1 and len(info[0]) == 4
    passes, colours, rounds, selected = info[0]
    assert 1 <= passes <= n                                  # at least the heaviest undecided node is selected per pass
    assert selected == int(want.sum())
    if color:
        assert 1 <= colours <= n and colours <= rounds <= n * colours   # at least the lowest undecided node is decided per round
    else:
        assert colours == 0 and rounds == 0
    return info[0]


def check_coloring(cls, name):
    """the reference's colouring; returns (colours, rounds)"""
    d = data()
    G = pattern(name)
    n = G.shape[0]
    info = []
    coloring = cls.vertex_coloring(G, "MIS", info=info)
    want = d[f"col.{name}.coloring"]
    assert coloring.dtype == np.intc and np.array_equal(coloring, want), name
    assert np.array_equal(cls.vertex_coloring(G), want)      # 'MIS' is the default
    colours, rounds = info[0]
    assert colours == int(want.max()) + 1 and colours <= rounds <= n * colours
    return info[0]


def check_first_level(cls, CF, product):
    """strength -> CLJP / CLJP-c -> classical interpolation -> Galerkin product of the 17 x 13 grid, as ruge_stuben_solver composes them:
    the reference's first prolongator and level-1 operator.  ``product(R, A, P)``: the triple product"""
    d = data()
    A = csr("e2e.A")
    C = cls.classical_strength_of_connection(A, theta=0.25)
    splitting = cls.CLJP(C) if CF == "CLJP" else cls.CLJPc(C)
    P = cls.classical_interpolation(A, C, splitting)
    same_csr(P, f"e2e.{CF}.P0")
    assert P.shape == (A.shape[0], int(d[f"e2e.{CF}.P0.nc"]))
    same_csr(sp.csr_array(product(sp.csr_array(P.T), A, P)), f"e2e.{CF}.A1")
