"""The LINE-SCAN fast-order Gauss-Seidel / SOR sweep (pyamg_amd/csrc/pamg_line.hip) on the adversarial banded families of tests/line_families.py.
tests/test_line_families_plan.py shows on the CPU that the PLANS are sound on these shapes; here the DEVICE CODE that consumes them is held to the
same answers: the carry between the chunks of a line (lines of 63 / 64 / 65 / 129 rows), lanes >= cnt of a short last chunk, recurrence coefficients
that differ from row to row and between the two directions, the snapshot path of structurally non-symmetric patterns, rows without a usable
diagonal inside a chunk, K = 8 slot sets and K forward != K backward, a one-row chunk that polls what its own wave published, the gate path,
few workgroups (waves that wait), the wipe partition of the fused kernel where the lines do not divide the rows (`holes_sym`: 4 290 rows, 111
lines; the hand-off buffers must be all sentinels after every launch and the second iteration polls what the first one wiped), and the float32
instantiation.

Bare operators through DeviceMatrix, tune(gs_order=1, line_scan=2, sym_fused=f, lane_G=G, lane_flags=fl) over CONFIGS, each with sym_fused 1 and 0.
Per family and configuration: forward, backward and symmetric sweeps, 1 and 2 iterations, from a random x; symmetric from zero announced and not
announced; SOR forward and backward with omega 1.4 and 0.6.
  * against the oracle's sequential sweep in long double: e_dev <= max(8 e_seq, 32 u g), e_seq the f64 (f32) oracle's own error, g =
    line_families.growth_factor, from the operator;
  * against the f64 oracle: 1e-13 relative (`growth`: 1e-13 g);
  * bit for bit: fused == two launches, a second run of EVERY sweep == the first, every (lane_G, lane_flags) == the first configuration (the order of additions
    belongs to the layout, not to which wave walks a line), the layout filled on the host == the one filled on the device;
  * rows without a usable diagonal and the empty row keep their bits (from zero: exactly 0.0);
  * the DECLARED form ran: lines / chunks / slots per row / levels of line_info, the form sym_info names and its launch count, the hand-off
    buffers all sentinels and the counters zero between launches; for the families that decline, no lines and the lane form that ran instead
    -- a case that passes because the path stepped aside fails;
  * flow_error() is clear.
Every case prints `[line families] <family> <configuration> <form> e_dev / bar` (run with -s for the table).  Measured on an MI355X, worst
e_dev / bar per family (the same in every configuration, as the bits are): var3d_63 0.108, var3d_64 0.123, var3d_65 0.134 (f32 0.105),
var3d_129 0.110, periodic2d 0.118 (f32 0.119), growth 0.143, k8 0.134 (f32 0.137), k_differs 0.115, nonsym_pattern 0.114, holes 0.104 (f32 0.106),
holes_sym 0.101 (f32 0.106), many_preds 0.093, at_threshold 0.110; on the lane form that takes over: slot_overflow 0.110, row_too_long 0.111,
below_threshold 0.100."""
import functools

import numpy as np
import pytest

import line_families as F
from oracle import oracle as orc
from pyamg_amd import _capi as capi
from pyamg_amd.hierarchy import sparse_op
from pyamg_amd.multilevel import DeviceMatrix

pytestmark = pytest.mark.gpu

L = np.longdouble
CONFIGS = ((0, 1), (1, 0), (3, 9), (0, 8))                 # (lane_G, lane_flags): automatic / one workgroup / three and both gates / the line gate alone
LINE_WPB = 4                                               # waves (lines in flight) per workgroup
# (sweep, iterations, start, omega); start: "x" random, "zero" x = 0 not announced, "announced" x = 0 through gauss_seidel_x0(x_is_zero=True)
RUNS = tuple(("forward", i, "x", 1.0) for i in (1, 2)) + tuple(("backward", i, "x", 1.0) for i in (1, 2)) + tuple(("symmetric", i, "x", 1.0) for i in (1, 2)) + (
    ("symmetric", 1, "announced", 1.0), ("symmetric", 1, "zero", 1.0),
    ("forward", 1, "x", 1.4), ("backward", 1, "x", 1.4), ("forward", 1, "x", 0.6), ("backward", 1, "x", 0.6))
RUNS32 = tuple(r for r in RUNS if r[1] == 1 and r[2] == "x")


def _tag(cfg, fused):
    return f"G{cfg[0]} fl{cfg[1]} fused{fused}"


class Bench:
    """one operator on the device with its vectors; run() sweeps and downloads, counting the symmetric iterations"""

    def __init__(self, S, cfg, fused, b, line_scan=2):
        self.n = S.shape[0]
        self.dt = S.dtype
        self.A = DeviceMatrix(sparse_op(S))
        self.A.tune(gs_order=1, line_scan=line_scan, sym_fused=fused, lane_G=cfg[0], lane_flags=cfg[1])
        self.dx, self.db = capi.DeviceArray.from_host(np.zeros(self.n, dtype=self.dt)), capi.DeviceArray.from_host(np.asarray(b, dtype=self.dt))
        self.sym_iterations = 0

    def run(self, key, x):
        how, its, start, omega = key
        self.dx.upload(x if start == "x" else np.zeros(self.n, dtype=self.dt))
        if how == "symmetric":
            self.A.gauss_seidel_x0(self.dx, self.db, sweep="symmetric", iterations=its, x_is_zero=start == "announced")
            self.sym_iterations += its
        else:
            self.A.gauss_seidel(self.dx, self.db, sweep=how, omega=omega, iterations=its)
        return self.dx.download()

    def free(self):
        self.A.free(); self.dx.free(); self.db.free()


def _vectors(n, dtype=np.float64):
    rng = np.random.RandomState(5)
    return rng.rand(n).astype(dtype), rng.rand(n).astype(dtype)


def _ref(S, key, x, b, dtype):
    how, its, start, omega = key
    x0 = x if start == "x" else np.zeros_like(x)
    if omega != 1.0:
        return F.ref_sor(S, x0, b, how, omega, dtype=dtype)
    return F.ref_sweeps(S, x0, b, how, its, dtype=dtype)


def _growth(S, key):
    how, _, _, omega = key
    return max(F.growth_factor(S, step, omega) for step in {"forward": (1,), "backward": (-1,), "symmetric": (1, -1)}[how])


@functools.lru_cache(maxsize=None)
def _references(name, dtype="float64", runs=RUNS):
    """(S, x, b, {run: (oracle in the working precision, long double, e_seq, growth)}) -- computed once per family, read-only"""
    dt = np.dtype(dtype)
    S = F.operator(name).astype(dt)
    x, b = _vectors(S.shape[0], dt)
    refs = {}
    for key in runs:
        rw, rl = _ref(S, key, x, b, dt), _ref(S, key, x, b, L)
        rw.flags.writeable = rl.flags.writeable = False
        refs[key] = (rw, rl, F.rel_err(rw, rl), _growth(S, key))
    return S, x, b, refs


def _assert_form(name, B, form, cfg, fused):
    """the declared form is what the info calls report; returns its name for the table"""
    A, n = B.A, B.n
    got = []
    for which in (0, 1):
        li, want = A.line_info(which), form.on_device(which)
        if want is not None:
            assert (li["slots_per_row"], li["chunks"], li["lines"], li["line_levels"]) == (want.K, want.chunks, want.lines, want.levels), (name, cfg, which, li)
            if cfg[0] > 0:                                             # the workgroups asked for: waves that wait for their lines' turn
                assert li["launch_grid"] == min(cfg[0], -(-want.lines // LINE_WPB)), (name, cfg, which, li)
            got.append(f"line K{want.K}")
        else:
            assert li["lines"] == 0 and li["chunks"] == 0, (name, cfg, which, li)
            ran = "lanem" if A.lanem_info(which)["rows"] == n else "lane" if A.lane_info(which)["groups"] > 0 else None
            assert ran, (name, cfg, which, "neither the line form nor a lane form holds this schedule")
            got.append(ran)
    si = A.sym_info()
    lines = form.on_device(0) is not None and form.on_device(1) is not None
    if lines and form.fused and fused and B.dt == np.float64:
        assert si["form"] == "line" and si["launches"] == B.sym_iterations, (name, cfg, si, B.sym_iterations)
        assert si["handoff_not_sentinel"] == 0 and si["counters_not_zero"] == 0, (name, cfg, si)
        if cfg[0] > 0:
            assert si["launch_grid"] == min(cfg[0], -(-max(form.fwd.lines, form.bwd.lines) // LINE_WPB)), (name, cfg, si)
        sym = "fused line"
    elif lines:
        assert si["launches"] == 0, (name, cfg, fused, si)
        sym = "two launches"
    else:
        assert si["form"] != "line", (name, cfg, fused, si)
        sym = "no lines"
    assert not A.flow_error(), (name, cfg, fused)
    return f"fwd {got[0]} bwd {got[1]} sym {sym}"


def _check_results(name, tag, S, x, refs, got, u, tol64):
    """every run against the long-double sweep (the bar) and the oracle in the working precision; returns the worst e_dev / bar"""
    idle = F.untouched_rows(S)
    worst = 0.0
    for key, g in got.items():
        rw, rl, e_seq, growth = refs[key]
        bar = F.bar(e_seq, growth, u)
        e_dev = F.rel_err(g, rl)
        worst = max(worst, e_dev / bar)
        assert e_dev <= bar, (name, tag, key, e_dev, e_seq, growth)
        if tol64 is not None:
            assert F.rel_err(g, rw) <= tol64 * (growth if name == "growth" else 1.0), (name, tag, key, F.rel_err(g, rw))
        start = x if key[2] == "x" else np.zeros_like(x)
        assert np.array_equal(g[idle], start[idle]), (name, tag, key, "rows without a usable diagonal must keep their bits")
    return worst


def _run_config(name, S, x, b, cfg, fused, runs=RUNS):
    """every run, then every run a second time in reverse order (each then follows another sweep than the first time)"""
    B = Bench(S, cfg, fused, b)
    got = {key: B.run(key, x) for key in runs}
    for key in reversed(runs):
        assert np.array_equal(B.run(key, x), got[key]), (name, cfg, fused, key, "a second run gives other bits")
    return B, got


@pytest.mark.parametrize("name", list(F.FAMILIES))
def test_family_on_the_device(name):
    assert np.finfo(L).nmant >= 63
    fam = F.FAMILIES[name]
    S, x, b, refs = _references(name)
    first = None
    for cfg in CONFIGS:
        outs = {}
        for fused in (1, 0):
            B, got = _run_config(name, S, x, b, cfg, fused)
            form_name = _assert_form(name, B, fam.form, cfg, fused)
            worst = _check_results(name, _tag(cfg, fused), S, x, refs, got, F.U, 1e-13)
            print(f"[line families] {name:16s} n={B.n:5d} {_tag(cfg, fused):16s} {form_name}: e_dev / bar {worst:.3f}")
            B.free()
            outs[fused] = got
        for key in outs[1]:
            assert np.array_equal(outs[1][key], outs[0][key]), (name, cfg, key, "fused != two launches")
        if first is None:
            first = outs[1]
        for key in first:
            assert np.array_equal(outs[1][key], first[key]), (name, cfg, key, "the bits depend on lane_G / lane_flags")


@pytest.mark.parametrize("name", ["holes", "holes_sym", "k8", "periodic2d", "growth"])
def test_layout_filled_on_the_host_gives_the_same_bits(name, monkeypatch):
    """PAMG_LINE_HOST_FILL=1: the planner's own fill pass (what the CPU suite replays) uploaded, against line_fill_kernel's"""
    fam = F.FAMILIES[name]
    S, x, b, _ = _references(name)
    res = {}
    for host in ("1", "0"):
        monkeypatch.setenv("PAMG_LINE_HOST_FILL", host)
        B, got = _run_config(name, S, x, b, CONFIGS[0], 1)
        _assert_form(name, B, fam.form, CONFIGS[0], 1)
        res[host] = (got, [{k: v for k, v in B.A.line_info(w).items() if k != "bytes"} for w in (0, 1)])
        B.free()
    assert res["1"][1] == res["0"][1], (name, res["1"][1], res["0"][1])
    for key in res["0"][0]:
        assert np.array_equal(res["1"][0][key], res["0"][0][key]), (name, key, "host fill != device fill")


@pytest.mark.parametrize("name", ["var3d_65", "periodic2d", "holes", "holes_sym", "k8"])
def test_float32_against_the_reference(name):
    """the float32 instantiation against the long-double sweep of the float32 operator: the same bar with u = 2^-24 and e_seq from the f32 oracle.
    The fused kernel is f64 only: the symmetric sweep is two launches whatever sym_fused says"""
    fam = F.FAMILIES[name]
    S, x, b, refs = _references(name, "float32", RUNS32)
    assert S.dtype == np.float32 and x.dtype == np.float32
    first = None
    for cfg in (CONFIGS[0], CONFIGS[2], CONFIGS[1]):
        B, got = _run_config(name, S, x, b, cfg, 1, RUNS32)
        assert all(g.dtype == np.float32 for g in got.values())
        form_name = _assert_form(name, B, fam.form, cfg, 1)
        assert B.A.sym_info()["launches"] == 0 and B.A.line_info(0)["lines"] == fam.form.fwd.lines, (name, cfg)
        worst = _check_results(name, _tag(cfg, 1) + " f32", S, x, refs, got, F.U32, None)
        print(f"[line families] {name:16s} n={B.n:5d} {_tag(cfg, 1):16s} f32 {form_name}: e_dev / bar {worst:.3f}")
        B.free()
        if first is None:
            first = got
        for key in first:
            assert np.array_equal(got[key], first[key]), (name, cfg, key, "the bits depend on lane_G / lane_flags")


def test_a_tune_change_switches_the_form_between_sweeps():
    """var3d_65 on ONE operator: line_scan 2 -> 0 -> 2 with lane_G / lane_flags changed in between.  Every sweep is right whatever ran before it,
    line_info follows the form, and the hand-off buffers of the fused launch are all sentinels between launches"""
    name = "var3d_65"
    fam = F.FAMILIES[name]
    S, x, b, refs = _references(name)
    runs = (("forward", 1, "x", 1.0), ("backward", 1, "x", 1.0), ("symmetric", 1, "x", 1.0), ("symmetric", 2, "x", 1.0), ("symmetric", 1, "announced", 1.0),
            ("forward", 1, "x", 1.4))
    B = Bench(S, CONFIGS[0], 1, b)
    steps = (("lines", dict(), True), ("lines, three workgroups", dict(lane_G=3), True), ("off", dict(line_scan=0), False),
             ("off, one workgroup", dict(lane_G=1), False), ("lines again, one workgroup", dict(line_scan=2), True),
             ("lines, automatic, gate", dict(lane_G=0, lane_flags=8), True))
    lines_bits = None
    for label, kw, lines in steps:
        B.A.tune(**kw)
        before = B.A.sym_info()["launches"]
        B.sym_iterations = 0
        got = {key: B.run(key, x) for key in runs}
        worst = _check_results(name, label, S, x, refs, got, F.U, 1e-13)
        si = B.A.sym_info()
        for which in (0, 1):
            li, want = B.A.line_info(which), fam.form.on_device(which)
            if lines:
                assert (li["slots_per_row"], li["chunks"], li["lines"]) == (want.K, want.chunks, want.lines), (label, which, li)
            else:
                assert li["lines"] == 0, (label, which, li)
                assert B.A.lanem_info(which)["rows"] == B.n or B.A.lane_info(which)["groups"] > 0, (label, which)      # a lane form ran instead
        if lines:
            assert si["form"] == "line" and si["launches"] - before == B.sym_iterations == 4, (label, si, before)
            if lines_bits is None:
                lines_bits = got
            for key in got:
                assert np.array_equal(got[key], lines_bits[key]), (label, key, "the line form's bits changed across tune changes")
        assert si["handoff_not_sentinel"] == 0 and si["counters_not_zero"] == 0 and not B.A.flow_error(), (label, si)
        print(f"[line families] {name:16s} tune -> {label}: lines {lines}, e_dev / bar {worst:.3f}, {si}")
    B.free()


# ----------------------------------------------------------------- solver level
HIER = "convdiff:32"                # 32 768 rows on level 0: upwind differences, non-symmetric values on a symmetric 7-point pattern


@pytest.mark.parametrize("cycle", ["V", "W"])
def test_solver_with_the_line_form_on_level_0(cycle):
    """level_tune line_scan = 2 on level 0 of the convection-diffusion hierarchy of tests/midsize.py: graph replay == eager == a second solve and
    sym_fused 1 == 0 bit for bit, oracle parity at the bars of tests/test_gpu_midsize.py (residual norms 1e-10, iterate 1e-12)"""
    import midsize as M
    from sweep_families import parity as _parity, solve_three_ways as _solve
    k = 3
    spec = M.hierarchy(HIER, ("gs", "symmetric"), scalar_csr=True)
    outs = {}
    for fused in (1, 0):
        dml, x, r, (b, x0), before, after = _solve(spec, k, cycle, 1, lambda i, f=fused: dict(line_scan=2, sym_fused=f) if i == 0 else dict(sym_fused=f))
        A0 = dml.A[0]
        n = A0.shape[0]
        for which in (0, 1):
            li = A0.line_info(which)
            assert li["lines"] == 32 * 32 and li["chunks"] == 32 * 32 and li["slots_per_row"] == 5, (which, li)
        si = after[0]
        if fused:
            assert si["form"] == "line" and si["launches"] - before[0]["launches"] == 2 * k, (si, before[0])      # pre- and post-smoothing of every cycle
            assert si["handoff_not_sentinel"] == 0 and si["counters_not_zero"] == 0, si
        else:
            assert si["launches"] == 0, si
        print(f"[line families] solver {cycle} fused={fused}: level 0 {n} rows, {A0.line_info(0)}, {si}")
        outs[fused] = (x, r)
        dml.free()
    assert np.array_equal(outs[1][0], outs[0][0]) and outs[1][1] == outs[0][1], "fused != two launches"
    ro = []
    xo = orc.OracleSolver(spec).solve(b, x0=x0, tol=1e-30, maxiter=k, cycle=cycle, cycles_per_level=1, residuals=ro)
    _parity(f"{cycle}(1) line form on level 0", outs[1][0], outs[1][1], xo, np.array(ro))
