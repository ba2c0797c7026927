"""The operator families of tests/sweep_families.py through the CPU replays of the merged lane-parallel Gauss-Seidel sweep (CPU, no GPU):
tests/lanec_emul.cpp (cluster layout, 4 / 8 rows per wave, one directional sweep and the fused symmetric sweep) and tests/lanem_emul.cpp (one row per
wave and the pair layout), built into a scratch directory of this test's own, on the project's own planner (pyamg_amd/csrc/pamg_lanem_plan.h).

Yardstick: the oracle's sequential sweep on np.longdouble copies (64-bit mantissa); on the tiny operators and the one with rows that lack a diagonal
it is itself checked against a plain Python loop (test_the_yardstick_is_the_plain_loop).  Bar: 1e-13 relative (chains, whose growth factors reach the
cap of 1e3: 1e-10, and 1e-13 with the cap at 1).

Per family, in every layout (cluster 4 / 8, row, pair), at depths 1 / 3 / 8 / 16, replayed in plan order (waves = 0) and by 7 waves visited last wave
first (the replay's deadlock check is then part of the case): forward, backward, symmetric (cluster: the fused replay; row / pair: the two
directional replays) and Zf on tril(A) from zero followed by Zb on triu(A).  Also: the return code is 0 except where the family DECLARES that the
planner declines (rc 2: a stored row above 512 operands, or above 256 in the pair layout); rows without a usable diagonal, the empty row included, keep
their input bit for bit; x = 0 announced gives the bits of x = 0 not announced (cluster replay: the row / pair replay has no such switch); and the form the device must take (sweep_families.Form), which
tests/test_gpu_sweep_families.py asserts from the info calls, follows from the planner's own statistics (test_declared_forms_follow_the_size_rules)."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import sweep_families as F
from test_lanec_plan import run_sweep, run_sym
from test_zero_plan import sweep as lane_sweep, zero_sweep

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
LAYOUTS = (("cluster", 4), ("cluster", 8), ("row", 1), ("pair", 2))
DEPTHS = (1, 3, 8, 16)
WAVES = (0, 7)
NAMES = sorted(F.FAMILIES)
NO_SIZE_RULES = F.Form()                  # the replay has no size rules: every tiny operator has a plan (the rules: test_declared_forms_...)


@pytest.fixture(scope="module")
def emul():
    out = HERE / "build" / "sweep_families"
    out.mkdir(parents=True, exist_ok=True)
    hdrs = [ROOT / "pyamg_amd" / "csrc" / h for h in ("pamg_lanem_plan.h", "pamg_lane_plan.h", "pamg_tile_plan.h")]
    libs = {}
    for name in ("lanec_emul", "lanem_emul"):
        so, src = out / f"{name}.so", HERE / f"{name}.cpp"
        if not so.exists() or so.stat().st_mtime < max([src.stat().st_mtime] + [h.stat().st_mtime for h in hdrs]):
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
        libs[name] = ctypes.CDLL(str(so))
    libs["lanec_emul"].lanec_emul_sweep_f64.restype = ctypes.c_int
    libs["lanec_emul"].lanec_emul_sym_f64.restype = ctypes.c_int
    libs["lanem_emul"].lanem_emul_sweep_f64.restype = ctypes.c_int
    return libs


def directional(libs, layout, A, x, b, direction, s, cap=1e3, waves=0, xz=0):
    """(rc, x, {super, levels}) of one directional sweep in `layout`"""
    n = A.shape[0]
    if layout[0] == "cluster":
        bounds = (0, n, 1) if direction > 0 else (n - 1, -1, -1)
        rc, got, st = run_sweep(libs["lanec_emul"], A, x, b, *bounds, s, layout[1], growth_cap=cap, waves=waves, xz=xz)
        return rc, got, st
    assert not xz
    return lane_sweep(libs, layout, A, x, b, direction, s, growth_cap=cap, waves=waves)


def symmetric(libs, layout, A, x, b, s, cap=1e3, waves=0, xz=0):
    if layout[0] == "cluster":
        rc, got, _ = run_sym(libs["lanec_emul"], A, x, b, s, layout[1], growth_cap=cap, waves=waves, xz=xz)
        return (2 if rc in (2, 102) else rc), got
    rc, y, _ = directional(libs, layout, A, x, b, +1, s, cap, waves)
    if rc:
        return rc, y
    rc, got, _ = directional(libs, layout, A, y, b, -1, s, cap, waves)
    return rc, got


def _vectors(A, seed):
    rng = np.random.RandomState(seed)
    n = A.shape[0]
    return rng.rand(n), rng.rand(n)


def _check_family(libs, name, A, form, tol, depths=DEPTHS, layouts=LAYOUTS, caps=(1e3,)):
    n = A.shape[0]
    x, b = _vectors(A, 7)
    z = np.zeros(n)
    L = np.longdouble
    refs = {how: F.ref_sweeps(A, x, b, how, dtype=L) for how in ("forward", "backward", "symmetric")}
    ref0 = F.ref_sweeps(A, z, b, "symmetric", dtype=L)
    idle = F.untouched_rows(A)
    worst = 0.0
    for cap in caps:
        bar = tol if cap > 1.0 else 1e-13
        for layout in layouts:
            declines = layout[0] in form.declines
            for s in depths:
                for waves in WAVES:
                    tag = (name, layout, s, waves, cap)
                    for how, d in (("forward", +1), ("backward", -1)):
                        rc, got, _ = directional(libs, layout, A, x, b, d, s, cap, waves)
                        assert rc == (2 if declines else 0), (tag, how, rc)
                        if declines:
                            continue
                        e = F.rel_err(got, refs[how])
                        worst = max(worst, e)
                        assert e <= bar, (tag, how, e)
                        assert np.array_equal(got[idle], x[idle]), (tag, how, "rows without a diagonal")
                    rc, got = symmetric(libs, layout, A, x, b, s, cap, waves)
                    assert rc == (2 if declines else 0), (tag, "symmetric", rc)
                    if not declines:
                        e = F.rel_err(got, refs["symmetric"])
                        worst = max(worst, e)
                        assert e <= bar, (tag, "symmetric", e)
                        assert np.array_equal(got[idle], x[idle]), (tag, "symmetric", "rows without a diagonal")
                        # from x = 0: announced (the OLD operands are not read) == not announced, in every bit
                        if layout[0] == "cluster":                      # (the row / pair replay has no such switch)
                            r0, g0 = symmetric(libs, layout, A, z, b, s, cap, waves, xz=0)
                            r1, g1 = symmetric(libs, layout, A, z, b, s, cap, waves, xz=1)
                            assert r0 == 0 and r1 == 0 and np.array_equal(g0, g1), (tag, "x = 0 announced")
                            assert F.rel_err(g0, ref0) <= bar, (tag, "from zero")
                            r0, f0, _ = directional(libs, layout, A, z, b, +1, s, cap, waves, xz=0)
                            r1, f1, _ = directional(libs, layout, A, z, b, +1, s, cap, waves, xz=1)
                            assert r0 == 0 and r1 == 0 and np.array_equal(f0, f1), (tag, "x = 0 announced, forward")
                    # Zf on tril(A) from zero, then Zb on triu(A) with w = diag(A) y.  The triangles of a row above the edge may fit where the row does
                    # not: the device never gets there (its zero-iterate plans follow the general ones), the plans are sound all the same
                    rc, got, sf, sb = zero_sweep(libs, layout, A, b, s, growth_cap=cap, waves=waves)
                    tri = max(int(np.diff(sp.tril(A, format="csr").indptr).max()), int(np.diff(sp.triu(A, format="csr").indptr).max())) - 1
                    fits = tri <= (F.PAIR_OPERANDS if layout[0] == "pair" else F.ROW_OPERANDS)
                    assert (rc == 0) == fits and rc in (0, 2, 202), (tag, "zero plans", rc, tri)
                    if rc == 0:
                        e = F.rel_err(got, ref0)
                        worst = max(worst, e)
                        assert e <= bar, (tag, "zero plans", e)
                        assert np.array_equal(got[idle], z[idle]), (tag, "zero plans", "rows without a diagonal are exactly 0.0")
    print(f"[families] {name}: {n} rows, {A.nnz} entries, {len(idle)} rows without a diagonal; worst error {worst:.2e} ({worst / tol:.2f} of {tol:g})")


@pytest.mark.parametrize("name", [n for n in NAMES if n != "chains"])
def test_family_against_the_long_double_sweep(emul, name):
    fam = F.FAMILIES[name]
    _check_family(emul, name, fam.make("small"), fam.form, fam.tol)


def test_chains_keep_their_bars(emul):
    """growth cap 1e3: 1e-10 (three digits to growth); cap 1: nothing is merged along the chains and the 1e-13 bar holds"""
    fam = F.FAMILIES["chains"]
    _check_family(emul, "chains", fam.make("small"), fam.form, fam.tol, caps=(1e3, 1.0))
    A = fam.make("small")
    x, b = _vectors(A, 7)
    for layout in LAYOUTS:
        rc, _, st = directional(emul, layout, A, x, b, +1, 8, 1e3)
        assert rc == 0 and st["super"] > (st["levels"] + 7) // 8, (layout, st)          # 3^7 > 1e3: the growth bound closed super-levels early
        rc, _, st = directional(emul, layout, A, x, b, +1, 8, 1.0)
        assert rc == 0 and st["super"] == st["levels"], (layout, st)


@pytest.mark.parametrize("n", F.TINY)
def test_tiny(emul, n):
    _check_family(emul, f"tiny {n}", F.tiny(n), NO_SIZE_RULES, 1e-13)


def test_the_yardstick_is_the_plain_loop():
    """oracle.gauss_seidel on long-double copies against ten lines of Python: same products, same order -- the same bits"""
    assert np.finfo(np.longdouble).nmant >= 63
    cases = [(f"tiny {n}", F.tiny(n)) for n in F.TINY] + [("nodiag", F.nodiag("small")), ("lower_only", F.lower_only("small"))]
    for name, A in cases:
        x, b = _vectors(A, 3)
        for how in ("forward", "backward", "symmetric"):
            for its in (1, 2):
                ref = F.ref_sweeps(A, x, b, how, its, dtype=np.longdouble)
                assert ref.dtype == np.longdouble
                assert np.array_equal(ref, F.plain_sweep(A, x, b, how, its)), (name, how, its)
                e64 = F.rel_err(F.ref_sweeps(A, x, b, how, its), ref)
                assert 0.0 < e64 <= 64 * F.U or A.nnz == A.shape[0], (name, how, its, e64)    # the f64 sweep rounds, by a few units


def _planned(libs, layout, A, direction, s, levels):
    """what the device keeps of the plan of one direction: merged (True) or not, by the rules of lanem_smax / lanem_to_device"""
    x, b = _vectors(A, 1)
    rc, _, st = directional(libs, layout, A, x, b, direction, s)
    if rc:
        assert rc == 2, rc
        return False
    assert st["levels"] == levels, (st, levels)
    return levels >= F.MIN_LEVELS and st["super"] * 10 <= st["levels"] * 9


def _assert_form(libs, name, A, form):
    """general plans at the depths lane_merge selects in tests/test_gpu_sweep_families.py, the triangles' at those of zero_merge (0 = automatic: 16);
    the cluster layouts merge what the row layout merges (the packing comes afterwards), so one of them stands for both"""
    assert form.lane_fits == (int(np.diff(A.indptr).max()) - 1 <= F.LANE_ENTRIES), (name, int(np.diff(A.indptr).max()))
    if not form.lane_fits:
        form = F.Form(fwd=form.fwd, bwd=form.bwd, zero=form.zero, declines=form.declines, gains_nothing=form.gains_nothing)   # the planner's own view
    tri = (sp.tril(A, format="csr"), sp.triu(A, format="csr"))
    lv = [F.dependency_levels(M, d) for M, d in ((A, +1), (A, -1), (tri[0], +1), (tri[1], -1))]
    for layout in LAYOUTS[1:]:
        want = F.expected(form, layout[1] if layout[0] == "cluster" else 1, 2 if layout[0] == "pair" else 1)
        general = [(_planned(libs, layout, A, +1, s, lv[0]), _planned(libs, layout, A, -1, s, lv[1])) for s in (2, 4, 8)]
        assert all(g == want[:2] for g in general), (name, layout, general, want)
        zero = [all(want[:2]) and _planned(libs, layout, tri[0], +1, s, lv[2]) and _planned(libs, layout, tri[1], -1, s, lv[3]) for s in (2, 16)]
        assert all(z == want[2] for z in zero), (name, layout, zero, want)


def test_declared_forms_follow_the_size_rules(emul):
    """the declaration the device test asserts is what the planner's statistics and the size rules give for the operators the device runs: a family
    that would stop exercising its path (too few dependency levels, a merge that gains nothing, a row past the edge) fails here, without a GPU"""
    for name, fam in F.FAMILIES.items():
        _assert_form(emul, name, fam.make("large"), fam.form)
    for n in F.TINY:
        _assert_form(emul, f"tiny {n}", F.tiny(n), F.tiny_form(n))
    assert [F.tiny_form(n).fwd for n in F.TINY] == [False, False, False, True, True, True]
    declining = [name for name, fam in F.FAMILIES.items() if set(fam.form.declines) == {"row", "pair", "cluster"}]
    assert declining == ["long_declines"], declining                                     # exactly one family declines in every layout
