"""The CLJP / CLJP-c coarse-grid selection and the MIS vertex colouring on the device (pamg_cljp.hip) against the reference's arrays in the
committed fixture (tests/golden/kernels_cljp.npz): np.array_equal on every splitting, colouring and end-to-end prolongator, no tolerance
(tests/cljp_cases.py).  No reference package is needed here.  The largest pattern has 300 rows."""
import numpy as np
import pytest

import cljp_cases as jc
from pyamg_amd import _capi as capi
from pyamg_amd import amg_core as gcore
from pyamg_amd import classical as cls
from pyamg_amd.aggregation import galerkin_product

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,color", jc.SPLITTINGS)
def test_cljp_is_the_references(name, color):
    passes, colours, rounds, selected = jc.check_cljp(cls, name, color)
    if name == "path300" and color:
        assert (colours, rounds) == (2, 301)                 # one decision per round along the chain, then every odd node at once
    if name == "n1":
        assert (passes, selected) == (1, 1)


def test_cljp_repeats():
    S = jc.pattern("irr200")                                 # the transposed rows come out of atomics in any order: no decision depends on it
    first = [cls.CLJP(S), cls.CLJPc(S)]
    for _ in range(3):
        assert np.array_equal(cls.CLJP(S), first[0]) and np.array_equal(cls.CLJPc(S), first[1])


@pytest.mark.parametrize("name", jc.names("col"))
def test_vertex_coloring_is_the_references(name):
    colours, rounds = jc.check_coloring(cls, name)
    if name == "path300":
        assert (colours, rounds) == (2, 301)


@pytest.mark.parametrize("CF", ["CLJP", "CLJPc"])
def test_first_level_of_the_hierarchy_without_the_reference(CF):
    jc.check_first_level(cls, CF, galerkin_product)


def test_the_two_entries_reject_bad_sizes():
    S = jc.pattern("grid17x13")
    n = S.shape[0]
    Sp, Sj = S.indptr.astype(np.int32), S.indices.astype(np.int32)
    lib, p = capi.lib(), capi.ptr
    out, info = np.full(n, -5, dtype=np.int32), np.zeros(4, dtype=np.int32)
    bad_col = Sj.copy(); bad_col[3] = n
    bad_ptr = Sp.copy(); bad_ptr[2] = bad_ptr[1] - 1
    for args in ((n, p(Sp), n, p(Sj), Sj.size), (n, p(Sp), Sp.size, p(Sj), Sj.size - 1), (n, p(bad_ptr), Sp.size, p(Sj), Sj.size),
                 (n, p(Sp), Sp.size, p(bad_col), Sj.size), (-1, p(Sp), Sp.size, p(Sj), Sj.size), (n, None, Sp.size, p(Sj), Sj.size)):
        assert lib.pamg_cljp_splitting(*args, 0, p(out), n, p(info)) == capi.E_ARG
        assert lib.pamg_cljp_splitting(*args, 1, p(out), n, p(info)) == capi.E_ARG
        assert lib.pamg_vertex_coloring_mis(*args, p(out), n, p(info)) == capi.E_ARG
    assert lib.pamg_cljp_splitting(n, p(Sp), Sp.size, p(Sj), Sj.size, 0, p(out), n - 1, p(info)) == capi.E_ARG
    assert lib.pamg_cljp_splitting(n, p(Sp), Sp.size, p(Sj), Sj.size, 0, None, n, p(info)) == capi.E_ARG
    assert lib.pamg_vertex_coloring_mis(n, p(Sp), Sp.size, p(Sj), Sj.size, p(out), n - 1, p(info)) == capi.E_ARG
    assert lib.pamg_vertex_coloring_mis(n, p(Sp), Sp.size, p(Sj), Sj.size, None, n, p(info)) == capi.E_ARG
    assert np.all(out == -5)                                 # nothing was written
    with pytest.raises(capi.PamgError) as e:
        gcore.cljp_naive_splitting(n, Sp, Sj[:-1].copy(), None, None, out, 0)
    assert e.value.status == capi.E_ARG
    with pytest.raises(TypeError):
        gcore.vertex_coloring_mis(n, Sp.astype(np.int64), Sj, out)
    # n = 0 returns at once, and a null info is allowed
    zero = np.zeros(1, dtype=np.int32)
    assert lib.pamg_cljp_splitting(0, p(zero), 1, None, 0, 1, None, 0, None) == capi.OK
    assert lib.pamg_vertex_coloring_mis(0, p(zero), 1, None, 0, None, 0, None) == capi.OK
    assert lib.pamg_cljp_splitting(n, p(Sp), Sp.size, p(Sj), Sj.size, 0, p(out), n, None) == capi.OK
    assert np.array_equal(out, jc.data()["cljp.grid17x13.cljp"])
