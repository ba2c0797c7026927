"""The adversarial families of tests/block_kz_families.py through the CPU replays of the two planners (no GPU): tests/blane_emul.cpp consumes the
plan of pamg_blane_plan.h the way bsr_lane_kernel does (static and one-XCD ticket order, every lane width the device can be asked for), tests/kz_emul.cpp
the plan of pamg_kz_plan.h the way kz_lane_kernel does.  Small size of every family; 1, 7 and 500 waves; forward and backward.  Asserted:
  * the return code is the declared one (0, or 2 where the planner declines) and the geometry is the declared one;
  * the yardstick of the device tests: e_replay <= max(8 e_seq, 32 u) against the oracle's loop in long double, and the family's `tol` against the
    oracle's f64 loop (relative to max |ref|);
  * rows and indices the sweep does not touch keep their bits;
  * the same bits for every number of waves and both modes: the replay fixes the order of the additions, the visiting order must not move them.
The long-double yardsticks themselves are pinned once against plain Python loops."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

import block_kz_families as F

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
WAVES = (1, 7, 500)
DIRS = ("forward", "backward")


def _load(name, headers):
    out = HERE / "build"
    out.mkdir(exist_ok=True)
    so, src = out / f"{name}.so", HERE / f"{name}.cpp"
    hdrs = [ROOT / "pyamg_amd" / "csrc" / h for h in headers]
    if not so.exists() or so.stat().st_mtime < max([src.stat().st_mtime] + [h.stat().st_mtime for h in hdrs]):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    return ctypes.CDLL(str(so))


@pytest.fixture(scope="module")
def blane():
    lib = _load("blane_emul", ("pamg_blane_plan.h", "pamg_lane_plan.h", "pamg_tile_plan.h"))
    lib.blane_emul_sweep_f64.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def kz():
    lib = _load("kz_emul", ("pamg_kz_plan.h", "pamg_lane_plan.h"))
    lib.kz_emul_sweep_f64.restype = ctypes.c_int
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _range(how, m):
    return (0, m, 1) if how == "forward" else (m - 1, -1, -1)


def run_block(lib, A, Dinv, x, b, how, waves, want_L, mode):
    bs = A.blocksize[0]
    nb = A.shape[0] // bs
    xx, stats = np.array(x, dtype=np.float64), np.zeros(8, dtype=np.int64)
    bAp, bAj = np.ascontiguousarray(A.indptr, dtype=np.int32), np.ascontiguousarray(A.indices, dtype=np.int32)
    bAx, Di, bb = np.ascontiguousarray(A.data, dtype=np.float64), np.ascontiguousarray(Dinv, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    rc = lib.blane_emul_sweep_f64(nb, bs, _p(bAp), _p(bAj), _p(bAx), _p(Di), _p(xx), _p(bb), *_range(how, nb), waves,
                                  0 if F.pattern_symmetric(A) else 1, want_L, mode, _p(stats))
    return rc, xx, stats


def run_kz(lib, Lop, v, b, Dinv, omega, nr, xout, how, waves):
    Lp, Lj = np.ascontiguousarray(Lop.indptr, dtype=np.int32), np.ascontiguousarray(Lop.indices, dtype=np.int32)
    Lx = np.ascontiguousarray(Lop.data, dtype=np.float64)
    vv, xx, stats = np.array(v, dtype=np.float64), np.array(xout, dtype=np.float64), np.zeros(8, dtype=np.int64)
    rc = lib.kz_emul_sweep_f64(Lop.shape[0], Lop.shape[1], _p(Lp), _p(Lj), _p(Lx), _p(vv), _p(np.ascontiguousarray(b, dtype=np.float64)),
                               _p(np.ascontiguousarray(Dinv, dtype=np.float64)), ctypes.c_double(omega), nr, _p(xx), *_range(how, Lop.shape[0]), waves, _p(stats))
    return rc, vv, xx, stats


# ----------------------------------------------------------------- the yardsticks themselves
def test_the_long_double_references_are_the_plain_loops():
    assert np.finfo(F.L_).nmant >= 63
    rng = np.random.RandomState(3)
    A = F.B_FAMILIES["b_tiny_5"].make("small", 3)
    Dinv = F.block_dinv(A)
    x, b = rng.rand(A.shape[0]), rng.rand(A.shape[0])
    for how in F.SWEEPS:
        got, want = F.ref_block(A, Dinv, x, b, how, 2, dtype=F.L_), F.plain_block(A, Dinv, x, b, how, 2)
        assert got.dtype == F.L_ and np.array_equal(got, want), how
        assert F.rel_err(F.ref_block(A, Dinv, x, b, how, 2), want) < 64 * F.U
    Lop = F.kz_rect_wide("small")[:20, :]
    Lop = Lop[:, :40].tocsr()
    Lop.sort_indices()
    for kind, omega in F.KINDS:
        _, spec = F.kz_spec(kind, Lop, omega)
        v, b, xo = rng.rand(Lop.shape[1]), rng.rand(Lop.shape[0]), rng.rand(Lop.shape[0])
        for how in F.SWEEPS:
            got = F.ref_kz(kind, Lop, v, b, spec.Dinv, omega, xo, how, 2, dtype=F.L_)
            want = F.plain_kz(kind, Lop, v, b, spec.Dinv, omega, xo, how, 2)
            assert all(g.dtype == F.L_ and np.array_equal(g, w) for g, w in zip(got, want)), (kind, how)


def test_the_nr_spec_hands_the_family_over_as_its_lines():
    """gauss_seidel_nr on A = Lop^T: spec.At is Lop itself, shape included (rectangular operators)"""
    for name in ("kz_rect_wide", "kz_rect_tall", "kz_chain", "kz_nonsym"):
        Lop = F.KZ_FAMILIES[name].make("small")
        A, spec = F.kz_spec("gauss_seidel_nr", Lop, 1.1)
        assert A.shape == Lop.shape[::-1] and tuple(spec.At.shape) == Lop.shape, (name, spec.At.shape)
        assert np.array_equal(spec.At.indptr, Lop.indptr) and np.array_equal(spec.At.indices, Lop.indices) and np.array_equal(spec.At.data, Lop.data)
        assert spec.Dinv.shape == (Lop.shape[0],)


# ----------------------------------------------------------------- Kaczmarz
@pytest.mark.parametrize("name", list(F.KZ_FAMILIES))
def test_kaczmarz_family_replay(kz, name):
    fam = F.KZ_FAMILIES[name]
    Lop = fam.make("small")
    m, n = Lop.shape
    assert int(np.diff(Lop.indptr).max()) == fam.form.longest, (name, np.diff(Lop.indptr).max())
    rng = np.random.RandomState(11)
    v, b, xo = F.kz_start(fam, n), rng.rand(m) - 0.5, rng.rand(m) - 0.5
    worst, padding = 0.0, 0.0
    for kind, omega in F.KINDS:
        nr = int(kind == "gauss_seidel_nr")
        _, spec = F.kz_spec(kind, Lop, omega)
        Dinv = spec.Dinv
        for how in DIRS:
            r64 = F.ref_kz(kind, Lop, v, b, Dinv, omega, xo, how)
            rl = F.ref_kz(kind, Lop, v, b, Dinv, omega, xo, how, dtype=F.L_)
            first = None
            for waves in WAVES:
                rc, vv, xx, st = run_kz(kz, Lop, v, b, Dinv, omega, nr, xo, how, waves)
                if fam.form.declines:
                    assert rc == 2, (name, kind, how, waves, rc)
                    continue
                assert rc == 0, (name, kind, how, waves, rc)
                assert (st[0], st[1]) == (fam.form.lanes, fam.form.slots), (name, st)
                assert st[3] - st[7] == Lop.nnz, (name, st)                                  # every stored entry has a slot, the rest is padding
                padding = st[7] / st[3]
                got = (xx, vv) if nr else (vv,)
                for g_, r64_, rl_ in zip(got, r64, rl):
                    e_seq, e_dev, d64 = F.rel_err(r64_, rl_), F.rel_err(g_, rl_), F.rel_err(g_, r64_)
                    worst = max(worst, e_dev / F.bar(e_seq))
                    assert e_dev <= F.bar(e_seq), (name, kind, how, waves, e_dev, e_seq)
                    assert d64 <= fam.tol, (name, kind, how, waves, d64)
                if first is None:
                    first = got
                assert all(F.same_bits(a_, b_) for a_, b_ in zip(first, got)), (name, kind, how, waves)
                if name == "kz_empty":
                    assert F.same_bits(vv[F.kz_unused(n)], v[F.kz_unused(n)])
                    if nr:
                        assert F.same_bits(xx[::9], xo[::9])
                if name == "kz_zero_entries" and nr:
                    assert F.same_bits(xx[F.kz_zero_line(m)], xo[F.kz_zero_line(m)])
    print(f"[block_kz plan] {name}: lanes {fam.form.lanes} slots {fam.form.slots} declines {fam.form.declines}; padding {padding:.0%} of the slots; "
          f"worst e_replay / bar = {worst:.3f}")


# ----------------------------------------------------------------- block Gauss-Seidel
@pytest.mark.parametrize("name", list(F.B_FAMILIES))
def test_block_family_replay(blane, name):
    fam = F.B_FAMILIES[name]
    worst, worst64 = 0.0, 0.0
    for bs in F.block_sizes(fam):
        A = fam.make("small", bs)
        nb = A.shape[0] // bs
        longest = F.longest_row(A)
        if not fam.form.declines:
            assert F.block_geometry(F.Form(longest=longest)) == (fam.form.lanes, fam.form.slots), (name, bs, longest)
        Dinv = F.block_dinv(A)
        rng = np.random.RandomState(12)
        x, b = rng.rand(nb * bs) - 0.3, rng.rand(nb * bs) - 0.5
        for how in DIRS:
            r64, rl = F.ref_block(A, Dinv, x, b, how), F.ref_block(A, Dinv, x, b, how, dtype=F.L_)
            e_seq = F.rel_err(r64, rl)
            for want_L in (8, 16, 32, 64):
                if want_L > 8 and want_L < fam.form.lanes:
                    continue                                                              # the same plan as with the family's own width
                first = None
                for mode in (0, 1):
                    for waves in WAVES:
                        rc, got, st = run_block(blane, A, Dinv, x, b, how, waves, want_L, mode)
                        if fam.form.declines and not fam.form.one_level:
                            assert rc == 2, (name, bs, how, want_L, mode, waves, rc)
                            continue
                        assert rc == 0, (name, bs, how, want_L, mode, waves, rc)
                        assert (st[0], st[1]) == F.block_geometry(F.Form(longest=longest), want_L), (name, bs, want_L, st)
                        if fam.form.one_level:
                            assert st[6] == 1 and F.same_bits(got, r64), (name, bs, st)     # one level: the device never asks the planner; no sum to reorder
                        e_dev, d64 = F.rel_err(got, rl), F.rel_err(got, r64)
                        worst, worst64 = max(worst, e_dev / F.bar(e_seq)), max(worst64, d64)
                        assert e_dev <= F.bar(e_seq), (name, bs, how, want_L, mode, waves, e_dev, e_seq)
                        assert d64 <= fam.tol, (name, bs, how, want_L, mode, waves, d64)
                        if first is None:
                            first = got
                        assert F.same_bits(first, got), (name, bs, how, want_L, mode, waves)
                        if name == "b_nodiag":
                            idle = (F.b_missing(nb)[:, None] * bs + np.arange(bs)).ravel()
                            assert F.same_bits(got[idle], r64[idle])
    print(f"[block_kz plan] {name}: lanes {fam.form.lanes} slots {fam.form.slots} declines {fam.form.declines}; worst e_replay / bar = {worst:.3f}, "
          f"worst |replay - f64 oracle| = {worst64:.3e}")
