"""The lane-parallel fast-order BLOCK Gauss-Seidel sweep (csrc/pamg_blane.hip) and the lane-parallel fast-order KACZMARZ sweeps (csrc/pamg_kz.hip)
on the adversarial operator families of tests/block_kz_families.py.  tests/test_block_kz_families_plan.py shows on the CPU that the PLANS are sound
on these shapes; here the DEVICE CODE that consumes them is held to the same answers: rectangular operators (slots sized by the columns, the
schedule by the rows), schedules as deep as they are long, groups of one real row and dummies, empty lines and indices no line touches, block rows
that are all padding, one-sided block patterns, the row lengths at which the lane geometry switches and at which the planners decline, operators
smaller than a wave, and waves that all wait on one another (lane_G = 1, 3).

Per family: forward, backward and symmetric sweeps, 1 and 2 iterations, under every configuration of CONFIGS_BLOCK resp. CONFIGS_KZ.
  * exact order (gs_order = 0): the f64 oracle's bits;
  * fast order against the oracle's loop in long double: e_dev <= max(8 e_seq, 32 u), e_seq the f64 oracle's own error, u = 2^-53, errors relative
    to max |ref| -- the yardstick of tests/test_gpu_midsize.py and tests/test_gpu_sweep_families.py with growth factor 1 (nothing is merged);
  * fast order against the f64 oracle: the family's `tol` (1e-13);
  * the DECLARED form ran (block_kz_families.Form): lanes per row / line and slots per lane from lane_info / kz_info, groups == 0 where the planner
    declines or the schedule has one level (the result is then the oracle's, bit for bit), launch_grid where lane_G forces it;
  * flow_error() is clear after every launch; a second run gives the same bits; so does every configuration -- they change the scheduling, not the
    order of the additions.  The one exception: lane_L sets the width of the butterfly over a block row (and which blocks share a lane), that IS
    the order of the additions, so block results are compared among the configurations that ran with the same lanes per row;
  * rows and indices the sweep does not touch keep their bits (kz_empty, kz_zero_entries, b_nodiag as the oracle leaves them).
Every case prints `[block_kz] <family> <configuration> e_dev / bar` (run with -s for the table)."""
import numpy as np
import pytest
import scipy.sparse as sp

import block_kz_families as F
from pyamg_amd import _capi as capi
from pyamg_amd.hierarchy import sparse_op
from pyamg_amd.multilevel import DeviceMatrix

pytestmark = pytest.mark.gpu

WPB = 4                                         # waves per workgroup of both sweeps (BLK / 64)
CASES = [(how, its) for how in F.SWEEPS for its in (1, 2)]
# lane_L 0 / 8 / 16 / 32 / 64 (a minimum: a family whose rows need more lanes keeps its own width); gran_xcd 0 (automatic) / 1 (one-XCD ticket
# form) / 2 (static form); lane_G 0 (automatic) / 1 / 3 (waves that wait on each other); lane_flags 0 / 1 (the gate)
CONFIGS_BLOCK = (
    dict(lane_L=0, gran_xcd=0, lane_G=0, lane_flags=1),
    dict(lane_L=8, gran_xcd=2, lane_G=3, lane_flags=0),
    dict(lane_L=16, gran_xcd=1, lane_G=1, lane_flags=1),
    dict(lane_L=32, gran_xcd=2, lane_G=1, lane_flags=1),
    dict(lane_L=64, gran_xcd=1, lane_G=3, lane_flags=0),
    dict(lane_L=0, gran_xcd=2, lane_G=0, lane_flags=0),
)
CONFIGS_KZ = (dict(lane_G=0), dict(lane_G=1), dict(lane_G=3))


def _tag(cfg):
    return " ".join(f"{k.replace('lane_', '').replace('gran_', '')}{v}" for k, v in cfg.items())


# ----------------------------------------------------------------- block Gauss-Seidel
def _block_form(name, fam, dM, cfg, longest, how):
    for which in {"forward": (0,), "backward": (1,), "symmetric": (0, 1)}[how]:
        info = dM.lane_info(which)
        if fam.form.declines:
            assert info["groups"] == 0, (name, cfg, which, info)
            continue
        lanes, slots = F.block_geometry(F.Form(longest=longest), cfg["lane_L"])
        assert info["groups"] > 0 and (info["lanes_per_row"], info["slots_per_lane"]) == (lanes, slots), (name, cfg, which, info)
        if cfg["lane_G"] > 0 and cfg["gran_xcd"] in (1, 2):
            want = min(cfg["lane_G"], -(-info["groups"] // WPB))                  # static form: that many workgroups
            if cfg["gran_xcd"] == 1:
                want *= 8                                                         # one-XCD form: as many for each of the 8 XCDs, one XCD stays
            assert info["launch_grid"] == want, (name, cfg, which, info)


@pytest.mark.parametrize("name", list(F.B_FAMILIES))
def test_block_family(name):
    assert np.finfo(F.L_).nmant >= 63
    fam = F.B_FAMILIES[name]
    worst = 0.0
    for bs in F.block_sizes(fam):
        A = fam.make("large", bs)
        nb = A.shape[0] // bs
        assert nb <= 1500
        longest = F.longest_row(A)
        if not fam.form.declines:
            assert F.block_geometry(F.Form(longest=longest)) == (fam.form.lanes, fam.form.slots), (name, bs, longest)
        Dinv = F.block_dinv(A)
        rng = np.random.RandomState(12)
        x, b = rng.rand(nb * bs) - 0.3, rng.rand(nb * bs) - 0.5
        refs = {}
        for how, its in CASES:
            r64, rl = F.ref_block(A, Dinv, x, b, how, its), F.ref_block(A, Dinv, x, b, how, its, dtype=F.L_)
            refs[(how, its)] = (r64, rl, F.rel_err(r64, rl))
        dM = DeviceMatrix(sparse_op(A))
        db, dD, dx = capi.DeviceArray.from_host(b), capi.DeviceArray.from_host(Dinv.reshape(-1)), capi.DeviceArray.from_host(x)

        def sweep(how, its):
            dx.upload(x)
            dM.block_gauss_seidel(dx, db, dD, sweep=how, iterations=its)
            got = dx.download()
            assert not dM.flow_error(), (name, bs, how, its)
            return got

        dM.tune(gs_order=0)
        for (how, its), (r64, _, _) in refs.items():
            assert F.same_bits(sweep(how, its), r64), (name, bs, how, its, "exact order")
        by_width = {}
        for cfg in CONFIGS_BLOCK:
            dM.tune(gs_order=1, **cfg)
            cfg_worst = 0.0
            for (how, its), (r64, rl, e_seq) in refs.items():
                got = sweep(how, its)
                assert F.same_bits(got, sweep(how, its)), (name, bs, cfg, how, its, "a second run")
                _block_form(name, fam, dM, cfg, longest, how)
                e_dev, d64 = F.rel_err(got, rl), F.rel_err(got, r64)
                cfg_worst = max(cfg_worst, e_dev / F.bar(e_seq))
                print(f"[block_kz] {name} bs{bs} {_tag(cfg)} {how} x{its}: e_dev {e_dev:.2e} e_seq {e_seq:.2e} e_dev / bar {e_dev / F.bar(e_seq):.3f} |dev - f64| {d64:.2e}")
                assert e_dev <= F.bar(e_seq), (name, bs, cfg, how, its, e_dev, e_seq)
                assert d64 <= fam.tol, (name, bs, cfg, how, its, d64)
                if fam.form.declines:
                    assert F.same_bits(got, r64), (name, bs, cfg, how, its, "the exact kernels keep the sweep")
                width = dM.lane_info(1 if how == "backward" else 0)["lanes_per_row"]
                first = by_width.setdefault((width, how, its), got)
                assert F.same_bits(first, got), (name, bs, cfg, how, its, "another configuration of the same width")
                if name == "b_nodiag":
                    idle = (F.b_missing(nb)[:, None] * bs + np.arange(bs)).ravel()
                    assert F.same_bits(got[idle], r64[idle]), (name, bs, cfg, how, its)
            worst = max(worst, cfg_worst)
        dM.free(); db.free(); dD.free(); dx.free()
    print(f"[block_kz] {name}: largest e_dev / bar = {worst:.3f}")


# ----------------------------------------------------------------- Kaczmarz
@pytest.mark.parametrize("name", [n for n, f in F.KZ_FAMILIES.items() if f.device])
def test_kaczmarz_family(name):
    assert np.finfo(F.L_).nmant >= 63
    fam = F.KZ_FAMILIES[name]
    Lop = fam.make("large")
    m, n = Lop.shape
    assert m <= 3000 and int(np.diff(Lop.indptr).max()) == fam.form.longest
    rng = np.random.RandomState(11)
    v0, b, xo = F.kz_start(fam, n), rng.rand(m) - 0.5, rng.rand(m) - 0.5
    worst = 0.0
    for kind, omega in F.KINDS:
        nr = kind == "gauss_seidel_nr"
        _, spec = F.kz_spec(kind, Lop, omega)
        op = spec.At if nr else sparse_op(sp.csr_array(Lop))
        # the operator as the device gets it: the family's lines, duplicates included
        assert tuple(op.shape) == (m, n) and np.array_equal(op.indptr, Lop.indptr) and np.array_equal(op.indices, Lop.indices) and np.array_equal(op.data, Lop.data)
        refs = {}
        for how, its in CASES:
            r64 = F.ref_kz(kind, Lop, v0, b, spec.Dinv, omega, xo, how, its)
            rl = F.ref_kz(kind, Lop, v0, b, spec.Dinv, omega, xo, how, its, dtype=F.L_)
            refs[(how, its)] = (r64, rl)
        dL = DeviceMatrix(op)
        dD, db = capi.DeviceArray.from_host(spec.Dinv), capi.DeviceArray.from_host(b)
        dv, dxo = capi.DeviceArray.from_host(v0), capi.DeviceArray.from_host(xo)

        def sweep(how, its):
            dv.upload(v0)
            if nr:
                dxo.upload(xo)
                dL.kaczmarz(dv, dD, omega, how, its, xout=dxo)
                got = (dxo.download(), dv.download())                              # x and the running residual
            else:
                dL.kaczmarz(dv, dD, omega, how, its, b=db)
                got = (dv.download(),)
            assert not dL.flow_error(), (name, kind, how, its)
            return got

        dL.tune(gs_order=0)
        for (how, its), (r64, _) in refs.items():
            assert all(F.same_bits(g_, r_) for g_, r_ in zip(sweep(how, its), r64)), (name, kind, how, its, "exact order")
        first = {}
        for cfg in CONFIGS_KZ:
            dL.tune(gs_order=1, **cfg)
            for (how, its), (r64, rl) in refs.items():
                got = sweep(how, its)
                assert all(F.same_bits(a_, b_) for a_, b_ in zip(got, sweep(how, its))), (name, kind, cfg, how, its, "a second run")
                for which in {"forward": (0,), "backward": (1,), "symmetric": (0, 1)}[how]:
                    info = dL.kz_info(which)
                    if fam.form.declines:
                        assert info["groups"] == 0, (name, kind, cfg, which, info)
                        continue
                    assert info["groups"] > 0 and (info["lanes_per_line"], info["slots_per_lane"]) == (fam.form.lanes, fam.form.slots), (name, kind, cfg, info)
                    if cfg["lane_G"] > 0:
                        assert info["launch_grid"] == min(cfg["lane_G"], -(-info["groups"] // WPB)), (name, kind, cfg, which, info)
                for what, g_, r64_, rl_ in zip(("x", "r") if nr else ("x",), got, r64, rl):
                    e_seq, e_dev, d64 = F.rel_err(r64_, rl_), F.rel_err(g_, rl_), F.rel_err(g_, r64_)
                    worst = max(worst, e_dev / F.bar(e_seq))
                    print(f"[block_kz] {name} {kind[-2:]} {_tag(cfg)} {how} x{its} {what}: e_dev {e_dev:.2e} e_seq {e_seq:.2e} e_dev / bar {e_dev / F.bar(e_seq):.3f} |dev - f64| {d64:.2e}")
                    assert e_dev <= F.bar(e_seq), (name, kind, cfg, how, its, what, e_dev, e_seq)
                    assert d64 <= fam.tol, (name, kind, cfg, how, its, what, d64)
                    if fam.form.declines:
                        assert F.same_bits(g_, r64_), (name, kind, cfg, how, its, what, "the exact kernels keep the sweep")
                ref0 = first.setdefault((how, its), got)
                assert all(F.same_bits(a_, b_) for a_, b_ in zip(ref0, got)), (name, kind, cfg, how, its, "another configuration")
                v_out = got[-1]
                if name == "kz_empty":
                    assert F.same_bits(v_out[F.kz_unused(n)], v0[F.kz_unused(n)]), (name, kind, cfg, how, its)
                    if nr:
                        assert F.same_bits(got[0][::9], xo[::9]), (name, kind, cfg, how, its)
                if name == "kz_zero_entries" and nr:
                    assert F.same_bits(got[0][F.kz_zero_line(m)], xo[F.kz_zero_line(m)]), (name, kind, cfg, how, its)
        dL.free(); dD.free(); db.free(); dv.free(); dxo.free()
    print(f"[block_kz] {name}: largest e_dev / bar = {worst:.3f}")
