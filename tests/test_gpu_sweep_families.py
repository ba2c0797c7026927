"""The merged lane-parallel Gauss-Seidel sweeps -- cluster layout (tune key 38), fused symmetric launch (key 37), zero-iterate plans (keys 39 / 40) --
on the adversarial operator families of tests/sweep_families.py.  tests/test_sweep_families_plan.py shows on the CPU that the PLANS are sound on
these shapes; here the DEVICE CODE that consumes them is held to the same answers: c_group's segmented scan over rows of unequal length and groups
with fewer than R rows, rows without a diagonal inside a cluster, rows that span several 64-slot units, the stored numerators of rows that are not
updated, phase 2 of the fused kernel reading old operands from the hand-off buffer on a non-symmetric pattern, the decline and fall-back paths,
plans after the operator's values change in place, and W / F cycles that enter a coarse level a second time with x != 0.

Bare operators, per family and configuration (CONFIGS: a covering list of the keys, each run with sym_fused 1 and 0): forward, backward and
symmetric sweeps, 1 and 2 iterations, from a random x, from zero announced and from zero not announced.
  * against the oracle's sequential sweep in long double: e_dev <= max(8 e_seq, 32 u g), e_seq the f64 oracle's own error, u = 2^-53, g the
    largest growth factor of the plans that RAN (the zero-iterate plans' where they did) -- the yardstick of tests/test_gpu_midsize.py;
  * against the f64 oracle: 1e-13 relative (chains: 1e-10);
  * fused == two launches and a second run == the first, bit for bit, two iterations announced from zero included;
  * rows without a usable diagonal and the empty row keep their bits (from zero: exactly 0.0);
  * the DECLARED form ran (sweep_families.Form): rows / cluster_rows of lanem_info, the form sym_info names, and zero_plan_launches advanced by
    exactly the number of sweeps announced to start from zero -- a case that passes because the path stepped aside fails;
  * flow_error() is clear, the hand-off buffer is all sentinels and the counters are zero between launches.
Every case prints `[families] <family> <configuration> <form> e_dev / bar` (run with -s for the table).

Solver level: the convection-diffusion hierarchy of tests/midsize.py (CSR levels), order "fast", V / W / F cycles with cycles_per_level 1 / 2,
lanem_cluster 8 and automatic: oracle parity (residual norms 1e-10 relative, iterate 1e-12: the bars of tests/test_gpu_midsize.py), graph replay ==
eager == a second solve and sym_fused 1 == 0 bit for bit, and per level >= 1 the zero-iterate plans ran for exactly the visits a Python mirror of
the recursion counts as announced from zero, the general plans for the others."""
import numpy as np
import pytest
import scipy.sparse as sp

import midsize as M
import sweep_families as F
from sweep_families import parity as _parity, solve_three_ways as _solve
from oracle import oracle as orc
from pyamg_amd import DeviceMultilevelSolver
from pyamg_amd import _capi as capi
from pyamg_amd.hierarchy import sparse_op
from pyamg_amd.multilevel import DeviceMatrix

pytestmark = pytest.mark.gpu

U = F.U
L = np.longdouble
# lanem_cluster 1 / 4 / 8; lanem_rpw 1 / 2 where cluster = 1; zero_plans 1 / 2; lane_merge 2 / 4 / 8; zero_merge 0 / 2 / 16; gran_xcd 0 / 1 / 2 (the
# cluster layout has the static form only: gran_xcd = 1 must not move it); lane_G 0 (automatic), 1 and 3 (waves that wait); lane_flags 0 / 1
CONFIGS = (
    dict(lanem_cluster=8, lanem_rpw=0, lane_merge=4, zero_plans=2, zero_merge=0, gran_xcd=0, lane_G=0, lane_flags=1),
    dict(lanem_cluster=4, lanem_rpw=0, lane_merge=2, zero_plans=2, zero_merge=2, gran_xcd=2, lane_G=3, lane_flags=0),
    dict(lanem_cluster=8, lanem_rpw=0, lane_merge=8, zero_plans=1, zero_merge=0, gran_xcd=2, lane_G=1, lane_flags=0),
    dict(lanem_cluster=4, lanem_rpw=0, lane_merge=4, zero_plans=2, zero_merge=16, gran_xcd=1, lane_G=0, lane_flags=1),
    dict(lanem_cluster=1, lanem_rpw=1, lane_merge=8, zero_plans=2, zero_merge=16, gran_xcd=1, lane_G=1, lane_flags=1),
    dict(lanem_cluster=1, lanem_rpw=1, lane_merge=2, zero_plans=1, zero_merge=0, gran_xcd=0, lane_G=0, lane_flags=0),
    dict(lanem_cluster=1, lanem_rpw=2, lane_merge=4, zero_plans=2, zero_merge=0, gran_xcd=2, lane_G=3, lane_flags=0),
    dict(lanem_cluster=1, lanem_rpw=2, lane_merge=2, zero_plans=2, zero_merge=2, gran_xcd=1, lane_G=0, lane_flags=1),
)
SWEEPS = ("forward", "backward", "symmetric")


def _tag(cfg):
    return (f"c{cfg['lanem_cluster']} rpw{cfg['lanem_rpw']} s{cfg['lane_merge']} zp{cfg['zero_plans']} zs{cfg['zero_merge']} xcd{cfg['gran_xcd']} "
            f"G{cfg['lane_G']} fl{cfg['lane_flags']}")


class Bench:
    """one operator on the device with its vectors; sweep() runs and downloads"""

    def __init__(self, A, cfg, fused, b):
        self.S = sp.csr_array(A)
        self.n = self.S.shape[0]
        self.A = DeviceMatrix(sparse_op(self.S))
        self.A.tune(gs_order=1, lane_wide=1, line_scan=0, sym_fused=fused, **cfg)
        self.dx, self.db = capi.DeviceArray.from_host(np.zeros(self.n)), capi.DeviceArray.from_host(b)

    def sweep(self, start, how, its=1, zero=False):
        self.dx.upload(start)
        if how == "symmetric":
            self.A.gauss_seidel_x0(self.dx, self.db, sweep="symmetric", iterations=its, x_is_zero=zero)
        else:
            self.A.gauss_seidel(self.dx, self.db, sweep=how, iterations=its)
        return self.dx.download()

    def free(self):
        self.A.free(); self.dx.free(); self.db.free()


def _growth(A, whiches):
    g = 1.0
    for w in whiches:
        mi = A.lanem_info(w)
        if mi["rows"]:
            g = max(g, mi["max_growth"])
    return g


def _references(S, x, b):
    """{(how, iterations, from zero): (f64 oracle, long double, e_seq)}"""
    out = {}
    z = np.zeros(S.shape[0])
    for how in SWEEPS:
        for its in (1, 2):
            for zero in (False, True):
                if zero and how != "symmetric":
                    continue
                x0 = z if zero else x
                r64, rl = F.ref_sweeps(S, x0, b, how, its), F.ref_sweeps(S, x0, b, how, its, dtype=L)
                out[(how, its, zero)] = (r64, rl, F.rel_err(r64, rl))
    return out


def _assert_form(name, B, cfg, fused, form, zero_calls):
    """the declared form is what the info calls report; returns its name for the table"""
    A, n = B.A, B.n
    cluster, rpw = cfg["lanem_cluster"], cfg["lanem_rpw"]
    fwd, bwd, zero = F.expected(form, cluster, rpw)
    zero = zero and cfg["zero_plans"] == 2
    got = []
    for which, want in ((0, fwd), (1, bwd)):
        mi = A.lanem_info(which)
        assert mi["rows"] == (n if want else 0), (name, cfg, which, mi)
        if want:
            assert mi["cluster_rows"] == (cluster if cluster >= 4 else 0), (name, cfg, which, mi)
            assert mi["s_max"] == cfg["lane_merge"] and 0 < mi["super_levels"] <= 0.9 * mi["dependency_levels"], (name, cfg, which, mi)
            per_group = cluster if cluster >= 4 else 2 if rpw == 2 else 1          # rows a wave's work item holds at most
            assert (n + per_group - 1) // per_group <= mi["groups"] <= n, (name, cfg, which, mi)
            got.append("cluster%d" % cluster if cluster >= 4 else "pair" if rpw == 2 else "row")
        else:
            got.append("lane" if A.lane_info(which)["groups"] else "other")
    si = A.sym_info()
    both = fwd and bwd
    for which in (4, 5):
        zi = A.lanem_info(which)
        assert zi["rows"] == (n if zero else 0), (name, cfg, which, zi)
        if zero:
            assert zi["cluster_rows"] == (cluster if cluster >= 4 else 0) and zi["s_max"] == (cfg["zero_merge"] or 16), (name, cfg, which, zi)
    assert si["zero_plan_launches"] == (zero_calls if zero else 0), (name, cfg, fused, si, zero_calls)
    if fused and both:
        one_xcd = cluster == 1 and cfg["gran_xcd"] in (0, 1)           # (every family is small enough for the one-XCD rule at gran_xcd = 0)
        assert si["launches"] > 0 and si["form"] == ("merged_one_xcd" if one_xcd else "merged"), (name, cfg, si)
        assert si["zero_launches"] == zero_calls, (name, cfg, si)
        assert si["handoff_not_sentinel"] == 0 and si["counters_not_zero"] == 0, (name, cfg, si)
    else:
        assert si["launches"] == 0, (name, cfg, fused, si)
    assert not A.flow_error(), (name, cfg, fused)
    return f"fwd {got[0]} bwd {got[1]} sym {'fused ' + si['form'] if fused and both else 'two launches'} zero plans {'yes' if zero else 'no'}"


def _run_family(name, S, form, tol, configs=CONFIGS):
    assert np.finfo(L).nmant >= 63
    n = S.shape[0]
    rng = np.random.RandomState(5)
    x, b = rng.rand(n), rng.rand(n)
    z = np.zeros(n)
    refs = _references(S, x, b)
    idle = F.untouched_rows(S)
    for cfg in configs:
        fwd, bwd, zero = F.expected(form, cfg["lanem_cluster"], cfg["lanem_rpw"])
        zero = zero and cfg["zero_plans"] == 2
        outs = {}
        for fused in (1, 0):
            B = Bench(S, cfg, fused, b)
            got = {}
            zero_calls = 0
            for (how, its, from_zero) in refs:
                got[(how, its, from_zero)] = B.sweep(z if from_zero else x, how, its, zero=from_zero)
                zero_calls += from_zero
            not_announced = B.sweep(z, "symmetric", 1, zero=False)
            again = {k: B.sweep(z if k[2] else x, k[0], k[1], zero=k[2]) for k in (("symmetric", 1, False), ("symmetric", 2, True), ("forward", 1, False))}
            zero_calls += 1
            form_name = _assert_form(name, B, cfg, fused, form, zero_calls)
            worst = 0.0
            for key, g in got.items():
                how, its, from_zero = key
                r64, rl, e_seq = refs[key]
                ran = {"forward": (0,), "backward": (1,), "symmetric": (0, 1)}[how]
                if from_zero and zero:                                 # the first iteration ran Zf / Zb, a second one the general plans
                    ran = (4, 5) if its == 1 else (0, 1, 4, 5)
                growth = _growth(B.A, ran)
                bar = max(8 * e_seq, 32 * U * growth)
                e_dev, e64 = F.rel_err(g, rl), F.rel_err(g, r64)
                worst = max(worst, e_dev / bar)
                assert e_dev <= bar, (name, cfg, fused, key, e_dev, e_seq, growth)
                assert e64 <= tol, (name, cfg, fused, key, e64)
                assert np.array_equal(g[idle], (z if from_zero else x)[idle]), (name, cfg, fused, key, "rows without a diagonal")
            e0 = F.rel_err(not_announced, refs[("symmetric", 1, True)][1])
            assert e0 <= max(8 * refs[("symmetric", 1, True)][2], 32 * U * _growth(B.A, (0, 1))), (name, cfg, fused, "x = 0 not announced", e0)
            assert F.rel_err(not_announced, refs[("symmetric", 1, True)][0]) <= tol, (name, cfg, fused, "x = 0 not announced, f64 oracle")
            assert np.array_equal(not_announced[idle], z[idle]), (name, cfg, fused, "x = 0 not announced: rows without a diagonal are exactly 0.0")
            for k, g in again.items():
                assert np.array_equal(g, got[k]), (name, cfg, fused, k, "a second run gives other bits")
            got["not announced"] = not_announced
            outs[fused] = got
            if fused:
                print(f"[families] {name:14s} n={n:5d} {_tag(cfg):44s} {form_name}: e_dev / bar {worst:.3f}")
            B.free()
        for k in outs[1]:
            assert np.array_equal(outs[1][k], outs[0][k]), (name, cfg, k, "fused != two launches")


@pytest.mark.parametrize("name", sorted(F.FAMILIES))
def test_family_on_the_device(name):
    fam = F.FAMILIES[name]
    _run_family(name, fam.make("large"), fam.form, fam.tol)


@pytest.mark.parametrize("n", F.TINY)
def test_tiny_on_the_device(n):
    """n = 2, 3, 5: fewer than 8 dependency levels, nothing is merged (and no zero-iterate plans); n = 9, 63, 65: merged, one row per level, every
    cluster group holds a single row -- 63 and 65 sit on either side of a wave's 64 lanes"""
    _run_family(f"tiny {n}", F.tiny(n), F.tiny_form(n), 1e-13)


def _scaled(S, alpha=None, d=None):
    S = sp.csr_array(S, copy=True)
    S.data = S.data * alpha if alpha is not None else S.data * np.repeat(d, np.diff(S.indptr))
    return S


@pytest.mark.parametrize("how", ["scale_values", "scale_rows"])
@pytest.mark.parametrize("name", ["nonsym", "nodiag", "mixed_lengths", "lane_edge", "convdiff_l1", "chains"])
def test_plans_follow_values_changed_in_place(name, how):
    """zero_plans = 2, cluster 8: after pamg_matrix_scale_values(2.0) / pamg_matrix_scale_rows(d) the next symmetric sweep announced from zero is the
    reference's on the scaled operator (the plans hold copies of the values: stale ones would give the old operator's sweep), and the zero-iterate
    plans are there again"""
    fam = F.FAMILIES[name]
    S = fam.make("large")
    n = S.shape[0]
    cfg = CONFIGS[0]
    rng = np.random.RandomState(6)
    x, b = rng.rand(n), rng.rand(n)
    z = np.zeros(n)
    for fused in (1, 0):
        B = Bench(S, cfg, fused, b)
        first = B.sweep(z, "symmetric", 1, zero=True)
        assert F.rel_err(first, F.ref_sweeps(S, z, b, "symmetric")) <= fam.tol
        assert B.A.lanem_info(4)["rows"] == n and B.A.sym_info()["zero_plan_launches"] == 1
        if how == "scale_values":
            S2 = _scaled(S, alpha=2.0)
            capi.check(capi.lib().pamg_matrix_scale_values(B.A.handle, 2.0), "pamg_matrix_scale_values")
        else:
            d = 0.5 + 1.5 * np.random.RandomState(8).rand(n)
            S2 = _scaled(S, d=d)
            capi.check(capi.lib().pamg_matrix_scale_rows(B.A.handle, capi.ptr(np.ascontiguousarray(d))), "pamg_matrix_scale_rows")
        for start, zero in ((z, True), (x, False)):
            got = B.sweep(start, "symmetric", 1, zero=zero)
            r64, rl = F.ref_sweeps(S2, start, b, "symmetric"), F.ref_sweeps(S2, start, b, "symmetric", dtype=L)
            e_seq = F.rel_err(r64, rl)
            growth = _growth(B.A, (0, 1, 4, 5) if zero else (0, 1))
            e_dev = F.rel_err(got, rl)
            print(f"[families] {name:14s} after {how} fused={fused} zero={zero}: e_dev / bar {e_dev / max(8 * e_seq, 32 * U * growth):.3f}")
            assert e_dev <= max(8 * e_seq, 32 * U * growth), (name, how, fused, zero, e_dev, e_seq, growth)
            assert F.rel_err(got, r64) <= fam.tol, (name, how, fused, zero)
            assert np.array_equal(got[F.untouched_rows(S2)], start[F.untouched_rows(S2)])
        assert B.A.lanem_info(4)["rows"] == n and B.A.lanem_info(5)["rows"] == n, (name, how, fused)
        assert B.A.lanem_info(0)["cluster_rows"] == 8 and B.A.sym_info()["zero_plan_launches"] == 2, (name, how, fused, B.A.sym_info())
        assert not B.A.flow_error()
        B.free()


def test_a_tune_change_switches_the_form_between_sweeps():
    """lane_edge (rows of 254 .. 256 entries: the full plan fits) on ONE operator: cluster 8 -> the pair layout -> unmerged on request (the lane form
    of the same schedule) -> one row per wave -> cluster 4 -> unmerged again.  Every sweep is right whatever ran before it, the info calls follow
    the form, and the zero-iterate plans come and go with the merged form"""
    fam = F.FAMILIES["lane_edge"]
    S = fam.make("large")
    n = S.shape[0]
    rng = np.random.RandomState(12)
    x, b = rng.rand(n), rng.rand(n)
    z = np.zeros(n)
    B = Bench(S, CONFIGS[0], 1, b)
    ref = {(how, zero): F.ref_sweeps(S, z if zero else x, b, how, dtype=L) for how in SWEEPS for zero in (False, True)}
    e64 = {k: F.rel_err(F.ref_sweeps(S, z if k[1] else x, b, k[0]), v) for k, v in ref.items()}
    steps = (("cluster 8", dict(lanem_cluster=8), 8, True), ("pair", dict(lanem_cluster=1, lanem_rpw=2), 0, True),
             ("unmerged on request", dict(lane_merge=1), 0, False), ("row", dict(lane_merge=4, lanem_rpw=1), 0, True),
             ("cluster 4", dict(lanem_cluster=4), 4, True), ("unmerged again", dict(lane_merge=1), 0, False))
    zpl = 0
    for label, kw, cluster, merged in steps:
        B.A.tune(**kw)
        B.A.tune(zero_plans=2)                                         # (an operator whose plans did not fit is not asked again until told so)
        for how in SWEEPS:
            for zero in ((False, True) if how == "symmetric" else (False,)):
                got = B.sweep(z if zero else x, how, 1, zero=zero)
                growth = _growth(B.A, (0, 1, 4, 5))
                e = F.rel_err(got, ref[(how, zero)])
                assert e <= max(8 * e64[(how, zero)], 32 * U * growth), (label, how, zero, e)
        zpl += merged
        for which in (0, 1, 4, 5):
            mi = B.A.lanem_info(which)
            assert mi["rows"] == (n if merged else 0) and mi["cluster_rows"] == (cluster if merged else 0), (label, which, mi)
            if not merged and which < 2:
                assert B.A.lane_info(which)["groups"] > 0, (label, which)      # the unmerged lane sweep is what ran instead
        si = B.A.sym_info()
        print(f"[families] lane_edge      tune -> {label}: merged {merged}, {si}")
        assert si["zero_plan_launches"] == zpl, (label, si)
        assert si["handoff_not_sentinel"] == 0 and si["counters_not_zero"] == 0 and not B.A.flow_error(), (label, si)
    B.free()


# ----------------------------------------------------------------- solver level
HIER = "convdiff:32"                # 32 768 / 4 192 / 117 / 4 rows: W and F cycles enter levels 1 and 2 a second time with x != 0


def mirror(nlev, cycle, cpl):
    """visits of every smoothed level in ONE cycle, split by whether the level is entered with x = 0 announced: the recursion of
    the reference's recursive cycle (what cycle_rec of pamg_solver.hip and OracleSolver.cycle restate) -- V: one coarse visit from zero; W: two, the first from zero; F: an F visit from zero, then cpl V visits"""
    counts = [[0, 0] for _ in range(nlev - 1)]

    def rec(lvl, kind, c, zero):
        counts[lvl][1 if zero else 0] += 1
        if lvl == nlev - 2:
            return
        if kind == "V":
            rec(lvl + 1, "V", 1, True)
        elif kind == "W":
            rec(lvl + 1, "W", c, True)
            rec(lvl + 1, "W", c, False)
        else:
            rec(lvl + 1, "F", c, True)
            for _ in range(c):
                rec(lvl + 1, "V", 1, False)
    rec(0, cycle, cpl, False)                                          # solve(x0 = rand): the finest level is not entered from zero
    return counts


@pytest.fixture(scope="module")
def oracle_solves():
    cache = {}

    def get(spec_key, spec, k, cycle, cpl, b, x0):
        key = (spec_key, k, cycle, cpl)
        if key not in cache:
            ro = []
            xo = orc.OracleSolver(spec).solve(b, x0=x0, tol=1e-30, maxiter=k, cycle=cycle, cycles_per_level=cpl, residuals=ro)
            cache[key] = (xo, np.array(ro))
        return cache[key]
    return get


@pytest.mark.parametrize("cluster", [8, 0], ids=["cluster8", "automatic"])
@pytest.mark.parametrize("cycle,cpl", [("V", 1), ("W", 1), ("F", 1), ("V", 2), ("W", 2), ("F", 2)])
def test_cycles_enter_coarse_levels_from_zero_and_not(cycle, cpl, cluster, oracle_solves):
    k = 3
    spec = M.hierarchy(HIER, ("gs", "symmetric"), scalar_csr=True)
    assert all(lv.A.fmt == "csr" for lv in spec.levels)
    nlev = len(spec.levels)
    assert nlev == 4
    visits = mirror(nlev, cycle, cpl)
    if cycle != "V":
        assert all(visits[l][0] > 0 and visits[l][1] > 0 for l in (1, 2)), visits       # coarse levels are entered from zero AND with x != 0
    outs = {}
    for fused in (1, 0):
        tune = dict(sym_fused=fused, lanem_cluster=cluster) if cluster else dict(sym_fused=fused)
        dml, x, r, (b, x0), before, after = _solve(spec, k, cycle, cpl, tune)
        outs[fused] = (x, r)
        for l in range(1, nlev - 1):
            A = dml.A[l]
            n = A.shape[0]
            for which in (0, 1, 4, 5):
                mi = A.lanem_info(which)
                assert mi["rows"] == n and mi["cluster_rows"] == cluster, (l, which, mi)      # merged, in the layout asked for, zero-iterate plans built
            d = {key: after[l][key] - before[l][key] for key in ("launches", "zero_launches", "zero_plan_launches")}
            not_zero, from_zero = visits[l]
            # every announced-zero visit pre-smooths on the zero-iterate plans; its post-smoothing and both sweeps of the other visits run the general plans
            assert d["zero_plan_launches"] == k * from_zero, (cycle, cpl, l, fused, d, visits[l])
            if fused:
                assert d["zero_launches"] == k * from_zero == d["zero_plan_launches"], (cycle, cpl, l, d, visits[l])
                assert d["launches"] == k * 2 * (from_zero + not_zero), (cycle, cpl, l, d, visits[l])
                assert d["launches"] - d["zero_plan_launches"] == k * (from_zero + 2 * not_zero) > 0, (cycle, cpl, l, d)
                assert after[l]["handoff_not_sentinel"] == 0 and after[l]["counters_not_zero"] == 0, (l, after[l])
            else:
                assert after[l]["launches"] == 0, (l, after[l])
            if fused and cluster:
                print(f"[families] solver {cycle}({cpl}) level {l}: {n} rows, visits from zero / not {from_zero} / {not_zero} per cycle, {after[l]}")
        assert dml.A[0].sym_info()["zero_plan_launches"] == 0 and dml.A[0].lanem_info(4)["rows"] == 0       # the finest level: on request only
        dml.free()
    assert np.array_equal(outs[1][0], outs[0][0]) and outs[1][1] == outs[0][1], "fused != two launches"
    xo, ro = oracle_solves("sym", spec, k, cycle, cpl, b, x0)
    _parity(f"{cycle}({cpl}) cluster {cluster}", outs[1][0], outs[1][1], xo, ro)


def test_directional_smoothers_run_no_zero_plans(oracle_solves):
    """pre = forward, post = backward Gauss-Seidel: nothing sweeps symmetrically, so no zero-iterate plan is built or launched"""
    k = 3
    spec = M.hierarchy(HIER, ("gs", "forward"), ("gs", "backward"), scalar_csr=True)
    for cluster in (8, 0):
        dml, x, r, (b, x0), _, after = _solve(spec, k, "W", 1, dict(lanem_cluster=cluster) if cluster else None)
        for l in range(1, len(spec.levels) - 1):
            A = dml.A[l]
            assert A.lanem_info(0)["rows"] == A.shape[0] and A.lanem_info(1)["rows"] == A.shape[0], l
            assert A.lanem_info(0)["cluster_rows"] == cluster, l
            assert A.lanem_info(4)["rows"] == 0 and A.lanem_info(5)["rows"] == 0, l
            assert after[l]["zero_plan_launches"] == 0 and after[l]["launches"] == 0, (l, after[l])
        dml.free()
        xo, ro = oracle_solves("dir", spec, k, "W", 1, b, x0)
        _parity(f"W(1) forward / backward, cluster {cluster}", x, r, xo, ro)


@pytest.mark.parametrize("cycle", ["V", "F"])
def test_two_smoothing_iterations(cycle, oracle_solves):
    """the smoother runs 2 iterations: x = 0 holds for the first one only -- one zero-iterate launch per announced visit, three general ones"""
    k = 3
    spec = M.hierarchy(HIER, ("gs", "symmetric", 2), scalar_csr=True)
    assert spec.levels[1].pre.iterations == 2 and spec.levels[1].post.iterations == 2
    visits = mirror(len(spec.levels), cycle, 1)
    outs = {}
    for fused in (1, 0):
        dml, x, r, (b, x0), before, after = _solve(spec, k, cycle, 1, dict(sym_fused=fused, lanem_cluster=8))
        outs[fused] = (x, r)
        for l in range(1, len(spec.levels) - 1):
            d = {key: after[l][key] - before[l][key] for key in ("launches", "zero_launches", "zero_plan_launches")}
            not_zero, from_zero = visits[l]
            assert d["zero_plan_launches"] == k * from_zero, (l, fused, d, visits[l])
            if fused:
                assert d["launches"] == k * 4 * (from_zero + not_zero) and d["zero_launches"] == k * from_zero, (l, d, visits[l])
        dml.free()
    assert np.array_equal(outs[1][0], outs[0][0]) and outs[1][1] == outs[0][1], "fused != two launches"
    xo, ro = oracle_solves("its2", spec, k, cycle, 1, b, x0)
    _parity(f"{cycle}(1), 2 smoothing iterations", outs[1][0], outs[1][1], xo, ro)
