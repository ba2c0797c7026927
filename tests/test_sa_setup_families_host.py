"""CPU side of the SA setup families (tests/sa_setup_families.py): the serial restatement of amg_core.standard_aggregation, the
replay of the device's token protocol, the oracle and the reference's recorded outputs
(tests/golden/kernels_sa_setup_families.npz) agree on every family, array for array; the strength restatement equals the
reference on every (operator, theta); the oracle's fit_candidates equals the reference on the recorded cases, and no
expectation of a tol = 1e-10 case hangs on a comparison at the threshold.  Needs no GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

import sa_setup_families as fam
from oracle import oracle as orc


# --------------------------------------------------------------------------------------------- aggregation
@pytest.mark.parametrize("name", fam.FAMILIES + fam.HUBS)
def test_serial_restatement_oracle_and_reference_agree(name):
    def oracle_fn(Ap, Aj):
        return orc.standard_aggregation(Ap, Aj)
    x, y, count = fam.check_aggregation(oracle_fn, name)     # oracle == restatement == fixture; the third pass opens nothing
    Ap, Aj = fam.graph(name)
    index_type = np.int64 if name.endswith("_i64") else np.int32
    indptr, indices, vals, shape = fam.aggop_from(x, count, index_type)
    fam.check_aggop(sp.csr_array((vals, indices, indptr), shape=shape), y.astype(index_type), name)
    if count == 0:                                           # aggregate.py:76-79: the (n, 1) matrix without an entry
        assert shape == (Ap.size - 1, 1) and indices.size == 0


@pytest.mark.parametrize("name", fam.FAMILIES + fam.HUBS)
def test_token_protocol_replay_is_the_serial_traversal(name):
    Ap, Aj = fam.graph(name)
    sx, sy, scount, _ = fam.serial_aggregation(Ap, Aj)
    n = Ap.size - 1
    live = int(np.sum([len(set(Aj[Ap[i]:Ap[i + 1]].tolist()) - {i}) > 0 for i in range(n)]))
    rounds = set()
    for order in ("reverse", 7):                             # the order inside a round does not matter
        x, y, count, r = fam.token_rounds(Ap, Aj, order)
        assert count == scount, (name, order)
        fam.same(x, sx, (name, order, "x"))
        fam.same(y, sy, (name, order, "y"))
        rounds.add(r)
    assert len(rounds) == 1
    r = rounds.pop()
    assert r <= live, (name, r, live)
    base = name[:-5] if name.endswith("_shuf") else name
    if base in fam.N_ROUNDS or base in fam.HUBS:
        assert r == n, (name, r)
    if base.startswith("pairs_"):
        assert r == 2, (name, r)


@pytest.mark.parametrize("name", fam.REFUSALS)
def test_replay_refuses_what_the_device_refuses(name):
    Ap, Aj = fam.graph(name)
    with pytest.raises(fam.Refused):
        fam.token_rounds(Ap, Aj)
    x, y, count, opened = fam.serial_aggregation(Ap, Aj)     # the reference itself returns something there: recorded
    ox, oy, ocount = orc.standard_aggregation(Ap, Aj)
    d = fam.data()
    for got_x, got_y in ((x, y), (ox, oy)):
        fam.same(got_x, d[f"refuse.{name}.x"], (name, "x"))
        fam.same(got_y, d[f"refuse.{name}.y"], (name, "y"))
    assert opened == int(d[f"refuse.{name}.opened"]) and count == ocount


# --------------------------------------------------------------------------------------------- strength
@pytest.mark.parametrize("name", fam.OPERATORS)
def test_strength_restatement_is_the_reference(name):
    A = fam.operator(name)
    for theta in fam.THETAS:
        Sp, Sj, Sx = fam.strength_restated(A, theta)
        rp, rj, rx = fam.recorded_strength(name, theta)
        fam.same(Sp, rp, (name, theta, "indptr"))
        fam.same(Sj, rj, (name, theta, "indices"))
        fam.same(Sx, rx, (name, theta, "data"))


def test_strength_operators_hold_their_edges():
    """the inputs carry what their names say (a family that lost its edge would test nothing)"""
    P = fam.operator("poisson2d_eq")
    off = P.indices != np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))
    assert np.all(P.data[off] ** 2 == 0.25 ** 2 * 4.0 * 4.0)                          # equality in a^2 >= theta^2 |a_ii| |a_jj|
    keep = np.diff(fam.recorded_strength("poisson2d_eq", 0.25)[0])
    assert np.array_equal(keep, np.diff(P.indptr))                                    # ... and '>=' keeps them all
    assert np.array_equal(np.diff(fam.recorded_strength("poisson2d_eq", 0.5)[0]), np.ones(P.shape[0], dtype=np.int32))

    def diag_count(M):
        return np.bincount(np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))[M.indices == np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))],
                           minlength=M.shape[0])
    assert np.all(diag_count(fam.operator("dup_diag")) == 2) and np.any(fam.operator("dup_diag").diagonal() == 0.0)
    assert np.any(diag_count(fam.operator("no_diag")) == 0) and np.all(fam.operator("zero_diag").diagonal() == 0.0)
    D = fam.operator("dup_off")
    assert D.nnz > sp.csr_array(D.todense()).nnz
    assert np.any(np.diff(fam.operator("empty_rows").indptr) == 0)
    Z = fam.operator("zero_rows")
    assert any(Z.indptr[i + 1] > Z.indptr[i] and not Z.data[Z.indptr[i]:Z.indptr[i + 1]].any() for i in range(Z.shape[0]))
    S = fam.operator("subnormal_row")
    big = np.array([np.abs(S.data[S.indptr[i]:S.indptr[i + 1]]).max(initial=0.0) for i in range(S.shape[0])])
    assert np.any((big > 0) & (big < 2.3e-308)) and not S.has_sorted_indices
    assert np.abs(fam.operator("scales").data).max() > 1e140 and np.abs(fam.operator("scales").data[fam.operator("scales").data != 0]).min() < 1e-140


# --------------------------------------------------------------------------------------------- tentative prolongator
def test_oracle_fit_candidates_is_the_reference_on_the_recorded_cases():
    recorded = fam.recorded_fit_cases()
    assert {a for a, _ in recorded} >= set(fam.AGGS) | {"hub_at_bound"}                 # every aggregation once
    assert {c[:5] for _, c in recorded} == {c[:5] for c in fam.fit_cases("empty_cols")}  # every (K1, K2, dtype, B family, tol) once
    for agg, case in recorded:
        Q, R, _ = fam.oracle_fit(orc, agg, case)
        want_Q, want_R = fam.recorded_fit(agg, case)
        fam.same(Q, want_Q, (agg, fam.case_id(case), "Q.data"))
        fam.same(R, want_R, (agg, fam.case_id(case), "R"))


@pytest.mark.parametrize("agg", fam.AGGS + fam.HUBS)
def test_no_fit_expectation_hangs_on_the_threshold(agg):
    """tol = 1e-10: every column's norm after / before the projections is below 1e-13 or above 1e-6 (a column that is zero
    before counts as zeroed); on 'normal' candidates exactly the columns beyond an aggregate's row count are zeroed.

    float64: the band holds for every column of every case.  float32: it holds for every column whose fate the data decide.
    A column that is EXACTLY dependent on the earlier ones (the repeated column, the columns beyond an aggregate's row count)
    leaves rounding noise of order eps32 * |column| behind -- measured here between 1e-10 and 1e-6 of the column, on both
    sides of tol -- and no seed changes that: float32 with the default tol keeps or zeroes such a column by its last bits.
    These columns are told apart by the same projections in float64 (ratio below 1e-13 there) and left out of the band; what
    the device must give for them is the oracle's bit-exact replay, which the parity tests ask for."""
    T = fam.aggop(agg)
    sizes = np.bincount(T.indices, minlength=T.shape[1])

    def ratios(B):
        before, after, zeroed = fam.fit_ratios(T, B, K1)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(before > 0, after / before, 0.0), zeroed
    for case in fam.fit_cases(agg):
        K1, K2, dt, bfam, tol, layout = case
        if tol != 1e-10 or (agg in fam.HUBS and (K1, K2) != (1, 1)):
            continue
        B = np.ascontiguousarray(fam.candidates(agg, case))
        ratio, zeroed = ratios(B)
        noise = np.zeros_like(zeroed) if dt == "f64" else ratios(B.astype(np.float64))[0] < 1e-13
        assert np.all((ratio < 1e-13) | (ratio > 1e-6) | noise), (agg, fam.case_id(case), ratio[(ratio >= 1e-13) & (ratio <= 1e-6) & ~noise][:5])
        assert np.array_equal(zeroed | noise, (ratio < 1e-13) | noise)
        _, R, _ = fam.oracle_fit(orc, agg, case)
        Rdiag = R.reshape(T.shape[1], K2, K2)[:, np.arange(K2), np.arange(K2)]
        assert np.array_equal((Rdiag == 0) | noise, zeroed | noise), (agg, fam.case_id(case))      # the oracle zeroed exactly these columns
        if bfam == "normal" and dt == "f64":
            assert int(zeroed.sum()) == int(np.maximum(0, K2 - sizes * K1).sum()), (agg, fam.case_id(case))


def test_candidate_families_hold_their_edges():
    tiny = fam.candidates("empty_cols", (2, 3, "f64", "tiny", 1e-10, "C"))
    assert np.all(tiny[:, 1] != 0) and np.all(tiny[:, 1] * tiny[:, 1] == 0)           # a non-zero column whose squares underflow
    tiny32 = fam.candidates("empty_cols", (1, 2, "f32", "tiny", 1e-10, "C"))
    assert tiny32.dtype == np.float32 and np.all(tiny32[:, 1] != 0) and np.all(tiny32[:, 1] * tiny32[:, 1] == 0)
    F = fam.candidates("empty_cols", (2, 3, "f64", "normal", 1e-10, "F"))
    S = fam.candidates("empty_cols", (2, 3, "f64", "normal", 1e-10, "strided"))
    C = fam.candidates("empty_cols", (2, 3, "f64", "normal", 1e-10, "C"))
    assert F.flags.f_contiguous and not F.flags.c_contiguous and not S.flags.c_contiguous and not S.flags.f_contiguous
    assert np.array_equal(F, C) and np.array_equal(S, C)
    T = fam.aggop("empty_cols")
    assert np.array_equal(np.flatnonzero(np.bincount(T.indices, minlength=T.shape[1]) == 0), [2, 5, 8]) and np.any(np.diff(T.indptr) == 0)
    assert fam.aggop("all_unaggregated").shape == (50, 1) and fam.aggop("all_unaggregated").nnz == 0
    assert np.bincount(fam.aggop("hub_at_bound").indices).max() == fam.SORT_MAX
    assert np.bincount(fam.aggop("hub_over_bound").indices).max() == fam.SORT_MAX + 1
    assert np.diff(fam.graph("hub_at_bound")[0]).max() == fam.SORT_MAX and np.diff(fam.graph("hub_over_bound")[0]).max() == fam.SORT_MAX + 1
    # with tol = 1.0 every column is zeroed, the first by equality (norm > 1.0 * norm is false)
    Q, R, _ = fam.oracle_fit(orc, "empty_cols", (2, 3, "f64", "normal", 1.0, "C"))
    assert not Q.any() and not R.any()


# --------------------------------------------------------------------------------------------- the oracle's wrappers
def test_oracle_wrappers_take_int64_and_strided_index_arrays():
    """the wrappers hold the converted index arrays for the duration of the C call (they used to pass the address of a
    temporary that was already freed): int64 and non-contiguous index arrays give what contiguous int32 ones give"""
    Ap, Aj = fam.graph("rand_iso")
    want = orc.standard_aggregation(Ap, Aj)

    def strided(a):
        wide = np.zeros(2 * a.size, dtype=a.dtype)
        wide[::2] = a
        return wide[::2]
    for conv in (lambda a: a.astype(np.int64), strided, lambda a: strided(a.astype(np.int64))):
        got = orc.standard_aggregation(conv(Ap), conv(Aj))
        assert got[2] == want[2]
        fam.same(got[0], want[0], "x")
        fam.same(got[1], want[1], "y")
    T = fam.aggop("rand_iso")
    csc = T.tocsc()
    B = fam.candidates("rand_iso", (2, 3, "f64", "normal", 1e-10, "C"))
    want_Ax, want_R = orc.fit_candidates(T.shape[1], 2, 3, csc.indptr.astype(np.int32), csc.indices.astype(np.int32), B, 1e-10)
    for conv in (lambda a: a.astype(np.int64), strided, lambda a: strided(a.astype(np.int64))):
        Ax, R = orc.fit_candidates(T.shape[1], 2, 3, conv(csc.indptr), conv(csc.indices), B, 1e-10)
        fam.same(Ax, want_Ax, "Ax")
        fam.same(R, want_R, "R")


# --------------------------------------------------------------------------------------------- the fixture itself
def test_the_fixture_holds_what_it_was_asked_for():
    d = fam.data()
    assert d["names.agg"].tolist() == fam.FAMILIES + fam.HUBS
    assert d["names.soc"].tolist() == [f"{o}.{t:g}" for o in fam.OPERATORS for t in fam.THETAS]
    assert d["names.fit"].tolist() == [f"{a}.{fam.case_id(c)}" for a, c in fam.recorded_fit_cases()]
    n_fam = len(fam.FAMILIES + fam.HUBS)
    assert d["aggop.sha256"].shape == (n_fam, 4, 32) and d["aggop.dtypes"].shape == (n_fam, 4) and d["aggop.shapes"].shape == (n_fam, 2)
    for k, name in enumerate(fam.FAMILIES + fam.HUBS):
        x, y = d[f"agg.{name}.x"], d[f"agg.{name}.y"]
        assert x.dtype == y.dtype == np.int32 and x.size == fam.graph(name)[0].size - 1, name
        index = "int64" if name.endswith("_i64") else "int32"                  # the index type follows the input's
        assert d["aggop.dtypes"][k].tolist() == [index, index, "int32", index], name
    for name in fam.REFUSALS:
        assert d[f"refuse.{name}.x"].size == 5000
    for name in fam.OPERATORS:
        assert d[f"soc.{name}.indptr"].shape == (len(fam.THETAS), fam.operator(name).shape[0] + 1) and d[f"soc.{name}.data"].dtype == np.float64
        assert d[f"soc.{name}.indices"].size == d[f"soc.{name}.data"].size == int(d[f"soc.{name}.indptr"][:, -1].sum())
    for agg, case in fam.recorded_fit_cases():
        assert d[f"fit.{agg}.{fam.case_id(case)}"].dtype == (np.float64 if case[2] == "f64" else np.float32)
    assert not any(np.issubdtype(v.dtype, np.floating) and not np.isfinite(v).all() for v in d.values())      # no NaN, no overflow
    assert fam.GOLDEN.stat().st_size <= (fam.GOLDEN.parent / "kernels_energy.npz").stat().st_size


def test_live_reference_equals_the_fixture():
    import oracle.refimport as ri
    if not ri.available():
        pytest.skip("oracle/_ref not present on this box")
    from pyamg import amg_core as ref_core
    from pyamg.aggregation.aggregate import standard_aggregation as ref_aggregation
    from pyamg.aggregation.tentative import fit_candidates as ref_fit
    from pyamg.strength import symmetric_strength_of_connection as ref_strength
    d = fam.data()
    for name in fam.FAMILIES + fam.HUBS:
        Ap, Aj = (a.astype(np.int32) for a in fam.graph(name))              # (the reference's binding takes int32 only)
        n = Ap.size - 1
        x, y = np.full(n, -7, dtype=np.int32), np.full(max(n, 1), -7, dtype=np.int32)
        cnt = ref_core.standard_aggregation(n, Ap, Aj, x, y)
        fam.same(x, d[f"agg.{name}.x"], (name, "x"))
        fam.same(y[:cnt], d[f"agg.{name}.y"], (name, "y"))
        AggOp, Cpts = ref_aggregation(sp.csr_array((np.ones(Aj.size), Aj, Ap), shape=(n, n)))
        fam.check_aggop(AggOp, Cpts, name[:-4] if name.endswith("_i64") else name)       # (int32 arrays: the int32 twin's record)
    for name in fam.OPERATORS:
        for theta in fam.THETAS:
            fam.check_strength(ref_strength, name, theta)
    for agg, case in fam.recorded_fit_cases():
        T = fam.aggop(agg)
        Q, R = ref_fit(sp.csr_array((T.data.copy(), T.indices.copy(), T.indptr.copy()), shape=T.shape), np.array(fam.candidates(agg, case)), tol=case[4])
        want_Q, want_R = fam.recorded_fit(agg, case)
        fam.same(Q.data, want_Q, (agg, fam.case_id(case), "Q.data"))
        fam.same(R, want_R, (agg, fam.case_id(case), "R"))
