"""The operator families of tests/line_families.py through the CPU replay of the line-scan fast-order sweep (CPU, no GPU): tests/line_emul.cpp,
built by line_families.build_emul on the project's own planner (pyamg_amd/csrc/pamg_line_plan.h).  The replay consumes the layout
the way gs_line_kernel does and scans in the association of its DPP steps.

Per family: forward and backward, Gauss-Seidel and SOR(1.4), 1 / 7 / 64 waves visited last wave first (the replay's deadlock check is part of the
case), snapshot = 1 for the structurally non-symmetric patterns (for the symmetric ones the replay also asserts that old operands are still old):
  * the return code and the statistics K / chunks / lines / levels equal the family's DECLARED form (rc 2 where the planner declines) -- what
    tests/test_gpu_line_families.py then asserts of the device from line_info;
  * the result is within e <= max(8 e_seq, 32 u g) of the oracle's sequential sweep in long double: e_seq the f64 sequential sweep's own error,
    g = growth_factor(A, direction, omega), from the operator;
  * rows without a usable diagonal, the empty row included, keep their bits.
On 300-row instances of three families the yardstick itself is pinned by a plain Python loop (test_the_yardstick_is_the_plain_loop)."""
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import line_families as F
from line_families import run_emul

HERE = Path(__file__).resolve().parent
L = np.longdouble
NAMES = list(F.FAMILIES)
WAVES = (1, 7, 64)
BOUNDS = {"forward": lambda n: (0, n, 1), "backward": lambda n: (n - 1, -1, -1)}


@pytest.fixture(scope="module")
def emul():
    return F.build_emul(HERE / "build")


def _vectors(n, seed):
    rng = np.random.RandomState(seed)
    return rng.rand(n), rng.rand(n)


def _pattern_symmetric(A):
    P = sp.csr_array((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)
    return (P - P.T).count_nonzero() == 0


@pytest.mark.parametrize("name", NAMES)
def test_declarations_follow_from_the_operator(name):
    """the parts of a declaration that are facts about the operator: size, longest row, pattern symmetry, and what they decide on the device"""
    fam, A = F.FAMILIES[name], F.operator(name)
    n, longest = A.shape[0], int(np.diff(A.indptr).max())
    assert n <= 5000 and (n >= F.MIN_ROWS or name == "below_threshold"), n
    assert longest <= F.MAX_ROW_ENTRIES or name == "row_too_long", longest
    assert fam.form.device == (n >= F.MIN_ROWS and longest <= F.MAX_ROW_ENTRIES)
    assert fam.form.sym_pattern == _pattern_symmetric(A)
    lines = fam.form.device and fam.form.fwd is not None and fam.form.bwd is not None
    assert fam.form.fused == (lines and fam.form.sym_pattern and fam.form.fwd.K == fam.form.bwd.K)      # line_sym_launch's conditions
    assert np.all(np.isfinite(A.data)) and A.has_sorted_indices
    if name in F.WIPE_REMAINDER:
        assert fam.form.fused
        for d in (fam.form.fwd, fam.form.bwd):                                       # the fused kernel's wipe partition: n = wq lines + wr, wr != 0
            assert n % d.lines != 0, (name, n, d.lines)
    if name == "many_preds":
        preds, late = F.many_preds_line_predecessors(A)
        assert preds > 12 and late > 12                                              # the planner's NPRED: the `many` branch, and the run on level 1 is past it
    if name == "growth":
        assert F.growth_factor(A, 1) == pytest.approx(1.5 ** 23) and F.growth_factor(A, -1) == 1.0
        assert F.growth_factor(A, 1, 1.4) == pytest.approx(2.1 ** 23)
    else:
        assert F.growth_factor(A, 1) == 1.0 and F.growth_factor(A, -1) == 1.0           # strictly dominant: |a_prev / a_tt| < 1


def test_growth_factor_windows():
    """at most 63 consecutive factors, runs end at a row that is not coupled or has no usable diagonal, duplicates are summed"""
    n = 200
    A = sp.lil_array((n, n))
    A.setdiag(1.0)
    A.setdiag(-2.0, -1)
    A = sp.csr_array(A.tocsr())
    assert F.growth_factor(A, 1) == 2.0 ** 63 and F.growth_factor(A, -1) == 1.0 and F.growth_factor(A, 1, 0.5) == 1.0
    B = sp.lil_array(A)
    B[100, 100] = 0.0                                             # row 100 is not updated: it ends a run
    B[30, 29] = 0.0
    B[60, 59] = 0.0                                               # rows 30 and 60 are not coupled: runs of 29 (1 .. 29), 29 (31 .. 59), 39 (61 .. 99), 99 factors
    B = sp.csr_array(B.tocsr())
    assert F.growth_factor(B, 1) == 2.0 ** 63                     # rows 101 .. 199: capped at 63 factors
    assert F.growth_factor(B[:100, :100], 1) == 2.0 ** 39
    assert F.growth_factor(B[:60, :60], 1) == 2.0 ** 29
    assert F.growth_factor(sp.csr_array(A.T), -1) == 2.0 ** 63    # the transpose, swept backward


def test_the_yardstick_is_the_plain_loop():
    """oracle.gauss_seidel / sor_gauss_seidel on long-double copies against ten lines of Python: same products, same order -- the same bits"""
    assert np.finfo(L).nmant >= 63
    for name, make in F.SMALL.items():
        A = make()
        n = A.shape[0]
        assert 250 <= n <= 320, n
        x, b = _vectors(n, 3)
        for how in ("forward", "backward", "symmetric"):
            for its in (1, 2):
                ref = F.ref_sweeps(A, x, b, how, its, dtype=L)
                assert ref.dtype == L and np.array_equal(ref, F.plain_sweep(A, x, b, how, its)), (name, how, its)
                assert 0.0 < F.rel_err(F.ref_sweeps(A, x, b, how, its), ref) <= 64 * F.U * F.growth_factor(A, 1), (name, how, its)
        for how in ("forward", "backward"):
            for omega in (1.4, 0.6):
                ref = F.ref_sor(A, x, b, how, omega, dtype=L)
                assert ref.dtype == L and np.array_equal(ref, F.plain_sor(A, x, b, how, omega)), (name, how, omega)


@pytest.mark.parametrize("name", NAMES)
def test_family_replays_to_its_declared_form(emul, name):
    fam, A = F.FAMILIES[name], F.operator(name)
    n = A.shape[0]
    x, b = _vectors(n, 7)
    idle = F.untouched_rows(A)
    worst = 0.0
    for which, how in enumerate(("forward", "backward")):
        want = (fam.form.fwd, fam.form.bwd)[which]
        step = 1 if how == "forward" else -1
        for sor, omega in ((0, 1.0), (1, 1.4)):
            if want is not None:
                r64 = F.ref_sor(A, x, b, how, omega) if sor else F.ref_sweeps(A, x, b, how)
                rl = F.ref_sor(A, x, b, how, omega, dtype=L) if sor else F.ref_sweeps(A, x, b, how, dtype=L)
                bar = F.bar(F.rel_err(r64, rl), F.growth_factor(A, step, omega))
            for waves in WAVES:
                rc, got, st = run_emul(emul, A, x, b, *BOUNDS[how](n), sor=sor, omega=omega, snapshot=0 if fam.form.sym_pattern else 1, waves=waves)
                if want is None:
                    assert rc == 2, (name, how, rc)
                    continue
                assert rc == 0, (name, how, sor, waves, rc)
                assert F.Dir(*(int(v) for v in st[:4])) == want, (name, how, st[:7])
                e = F.rel_err(got, rl)
                worst = max(worst, e / bar)
                assert e <= bar, (name, how, sor, waves, e, bar)
                assert np.array_equal(got[idle], x[idle]), (name, how, sor, waves, "rows without a diagonal")
    print(f"[line families] {name:16s} n={n:5d} replay: fwd {fam.form.fwd} bwd {fam.form.bwd}: e / bar {worst:.3f}")


@pytest.mark.parametrize("name", ["var3d_65", "periodic2d", "holes", "growth"])
def test_the_number_of_waves_does_not_change_the_bits(emul, name):
    """the order of additions belongs to the layout, not to which wave walks a line (what the device tests assert across lane_G)"""
    A = F.operator(name)
    n = A.shape[0]
    x, b = _vectors(n, 9)
    for how in ("forward", "backward"):
        outs = [run_emul(emul, A, x, b, *BOUNDS[how](n), waves=w) for w in WAVES]
        assert all(rc == 0 for rc, _, _ in outs)
        assert all(np.array_equal(outs[0][1], o[1]) for o in outs[1:]), (name, how)
