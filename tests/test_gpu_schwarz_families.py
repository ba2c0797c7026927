"""The persistent overlapping-Schwarz sweep (csrc/pamg_schwarz.hip: schwarz_versioned_kernel) and its per-level twin (schwarz_level_kernel) on the
subdomain families of tests/schwarz_families.py.  tests/test_schwarz_families_plan.py shows on the CPU that the PLAN is sound on these shapes; here
the DEVICE CODE that consumes it is held to the oracle's sequential sweep (amg_core::overlapping_schwarz_csr, relaxation.h:1420-1492), bit for bit
(np.array_equal on the bit patterns: no tolerance enters): subdomains of 0 .. 129 and of exactly 2048 rows (block row in registers / in L1, one
lane per row / lanes that loop over the rows), rows of 1 .. 257 stored entries with stored zeros and without a diagonal entry, one-sided patterns,
a row updated 255 and 256 times, schedules as deep as they are long and of one level, members in any order, a row listed twice in a subdomain,
and a third schedule that evicts the second and needs a larger hand-off buffer.

Per family (f64; f32 too where the family says so), on one handle: every sweep of the family (forward, backward, strided) twice in a row on the
same device x, under mode 0, mode 1 and mode 0 again -- the three results equal each other and the oracle's; the error word is clear after every
launch; rows in no visited subdomain keep the bits of x0; and the DECLARED form ran (pamg_schwarz_schedule_info): one persistent launch under mode
0 for a versioned family, per-level launches with the declared reason where the planner declines, per-level launches for a schedule of one level,
PAMG_E_UNSUPPORTED at create for a subdomain of 2049 rows.  Then the same families through Layer 1 (amg_core.overlapping_schwarz_csr; the forward
sweeps also against the reference's own amg_core, tests/golden/kernels_schwarz_families.npz), size_edges through relaxation.schwarz against the
reference's relaxation.schwarz, and Layer 1 after a forced time-out of the persistent sweep.
Every case prints `[schwarz] <family> <sweep> <mode> levels / widest / slots` (run with -s for the table)."""
import ctypes as C
import functools

import numpy as np
import pytest

import schwarz_families as F
from conftest import GOLDEN, ROOT
from pyamg_amd import _capi as capi
from pyamg_amd.hierarchy import sparse_op
from pyamg_amd.multilevel import DeviceMatrix

pytestmark = pytest.mark.gpu

CASES = [(name, dt) for name, fam in F.FAMILIES.items() for dt in (("f64", "f32") if fam.f32 else ("f64",))]
DTYPES = {"f64": np.float64, "f32": np.float32}


@functools.lru_cache(maxsize=None)
def large(name):
    A, Sp, Sj, Tp, Tx = F.FAMILIES[name].make("large")
    n = A.shape[0]
    assert n <= 4000 and len(Sp) - 1 <= 2500
    form = F.FAMILIES[name].form
    assert F.largest(Sp) == form.largest and F.most_updates(n, Sj) == form.updates[1], (name, F.largest(Sp), F.most_updates(n, Sj))
    return A, Sp, Sj, Tp, Tx


@functools.lru_cache(maxsize=None)
def wanted(name, dt, sweep, times):
    """the oracle's sequential sweep, computed once per case and shared (read-only)"""
    A, Sp, Sj, Tp, Tx = large(name)
    x0, b = F.start_vectors(A.shape[0])
    w = F.reference(A, Sp, Sj, Tp, Tx, x0, b, dict(F.sweeps_of(F.FAMILIES[name], len(Sp) - 1))[sweep], times=times, dtype=DTYPES[dt])
    w.setflags(write=False)
    return w


def schedule_info(lib, h):
    info = (C.c_int64 * 8)()
    capi.check(lib.pamg_schwarz_schedule_info(h, -1, info), "pamg_schwarz_schedule_info")
    return dict(zip(("versioned", "declined", "levels", "widest", "slots", "reads", "grid", "ran"), (int(v) for v in info)))


@pytest.mark.parametrize("name,dt", CASES)
def test_family_on_the_device(name, dt):
    fam, dtype = F.FAMILIES[name], DTYPES[dt]
    A, Sp, Sj, Tp, Tx = large(name)
    n, nsub = A.shape[0], len(Sp) - 1
    lib = capi.lib()
    Ad = A.astype(dtype)
    TT = np.ascontiguousarray(Tx, dtype=dtype)
    x0, b = (v.astype(dtype) for v in F.start_vectors(n))
    dA = DeviceMatrix(sparse_op(Ad))
    h = C.c_void_p()
    st = lib.pamg_schwarz_create(C.byref(h), dA.handle, nsub, capi.ptr(Sp), capi.ptr(Sj), capi.ptr(Tp), capi.ptr(TT))
    if fam.form.runs == "rejected":
        assert st == capi.E_UNSUPPORTED and not h.value, (name, st)                      # nothing is swept
        dA.free()
        return
    capi.check(st, "pamg_schwarz_create")
    hinfo = (C.c_int64 * 4)()
    capi.check(lib.pamg_schwarz_info(h, hinfo), "pamg_schwarz_info")
    assert (hinfo[0], hinfo[1]) == (nsub, fam.form.largest)
    if name == "size_edges":
        sizes, lv = np.diff(Sp), np.array(F.levels_of(A, Sp, Sj, (0, nsub, 1)))
        assert any((sizes[lv == L] <= F.SW_PRE).any() and (sizes[lv == L] > F.SW_LANES).any() for L in set(lv.tolist()))
    bd, xd = capi.DeviceArray.from_host(b), capi.DeviceArray.from_host(x0)
    got, slots, levels = {}, {}, {}
    for mode in (0, 1, 0):                                                                 # (the third pass: a second run gives the same bits)
        capi.check(lib.pamg_schwarz_set_mode(h, mode), "pamg_schwarz_set_mode")
        for sweep, (r0, r1, rs) in F.sweeps_of(fam, nsub):
            form = F.form_of(fam, sweep)
            xd.upload(x0)
            for _ in range(2):                                                             # two sweeps in a row on the same device x
                capi.check(lib.pamg_schwarz_sweep(h, xd.ptr, bd.ptr, r0, r1, rs, None), "pamg_schwarz_sweep")
                err = C.c_int(-1)
                capi.check(lib.pamg_schwarz_error(h, C.byref(err)), "pamg_schwarz_error")
                assert err.value == 0, (name, dt, sweep, mode)
            x = xd.download()
            want = wanted(name, dt, sweep, 2)
            assert F.same_bits(x, want), (name, dt, sweep, mode, int((x != want).sum()), np.flatnonzero(x != want)[:8])
            assert F.same_bits(x, got.setdefault(sweep, x)), (name, dt, sweep, mode, "another mode / a second run")
            idle = np.setdiff1d(np.arange(n), F.visited_rows(Sp, Sj, (r0, r1, rs)))
            assert F.same_bits(x[idle], x0[idle]), (name, dt, sweep, mode)
            if form.runs == "nothing":
                assert lib.pamg_schwarz_schedule_info(h, -1, (C.c_int64 * 8)()) == capi.E_STATE
                continue
            info = schedule_info(lib, h)
            levels[sweep] = info["levels"]
            visited = range(r0, r1, rs)
            print(f"[schwarz] {name} {dt} {sweep} mode {mode}: levels {info['levels']} / widest {info['widest']} / slots {info['slots']}"
                  f" (grid {info['grid']}, ran {('-', 'persistent', 'per level')[info['ran']]})")
            if form.runs == "versioned":
                E = sum(int(Sp[d + 1] - Sp[d]) for d in visited)
                R = sum(int(A.indptr[i + 1] - A.indptr[i]) for d in visited for i in Sj[Sp[d]:Sp[d + 1]])
                assert (info["versioned"], info["declined"], info["slots"], info["reads"]) == (1, 0, E, R) and info["levels"] >= 2, (name, sweep, info)
                assert info["ran"] == (1 if mode == 0 else 2), (name, sweep, mode, info)
                if mode == 0:
                    assert 1 <= info["grid"] <= len(visited), (name, sweep, info)
                slots[sweep] = info["slots"]
            elif form.runs == "declined":
                assert (info["versioned"], info["declined"], info["slots"], info["ran"]) == (0, form.declined, 0, 2), (name, sweep, mode, info)
            else:
                assert form.runs == "one_level" and info["levels"] == 1 and info["ran"] == 2, (name, sweep, mode, info)
    if name == "all_big":
        assert min(levels["forward"], levels["backward"]) >= 20, levels
    if name == "chain":
        assert levels["forward"] == nsub and levels["strided"] == len(range(*dict(F.sweeps_of(fam, nsub))["strided"])), levels
    if name == "regrow":
        assert slots["strided"] > max(slots["forward_small"], slots["backward_small"])
    capi.check(lib.pamg_schwarz_destroy(h), "pamg_schwarz_destroy")
    dA.free(); bd.free(); xd.free()


@pytest.mark.parametrize("name,dt", CASES)
def test_family_through_layer_1(name, dt):
    """amg_core.overlapping_schwarz_csr: one sweep per call, against the oracle; the forward f64 sweeps also against the reference's own amg_core"""
    import pyamg_amd.amg_core as gcore
    fam, dtype = F.FAMILIES[name], DTYPES[dt]
    A, Sp, Sj, Tp, Tx = large(name)
    n, nsub = A.shape[0], len(Sp) - 1
    Ap, Aj, Ax = F.i32(A.indptr), F.i32(A.indices), np.ascontiguousarray(A.data, dtype=dtype)
    TT = np.ascontiguousarray(Tx, dtype=dtype)
    x0, b = (v.astype(dtype) for v in F.start_vectors(n))
    z = np.load(GOLDEN / "kernels_schwarz_families.npz")
    for sweep, (r0, r1, rs) in F.sweeps_of(fam, nsub):
        y = x0.copy()
        if fam.form.runs == "rejected":
            with pytest.raises(NotImplementedError):
                gcore.overlapping_schwarz_csr(Ap, Aj, Ax, y, b, TT, Tp, Sj, Sp, nsub, n, r0, r1, rs)
            assert F.same_bits(y, x0)
            continue
        gcore.overlapping_schwarz_csr(Ap, Aj, Ax, y, b, TT, Tp, Sj, Sp, nsub, n, r0, r1, rs)
        assert F.same_bits(y, wanted(name, dt, sweep, 1)), (name, dt, sweep)
        if dt == "f64" and sweep == "forward":
            assert F.same_bits(y, z[f"{name}.forward"]), (name, "the reference's amg_core")


def test_size_edges_through_relaxation_schwarz():
    """relaxation.schwarz builds the inverted blocks itself (LAPACK's gelss, like the reference) and sweeps forward and backward, twice"""
    import scipy.sparse as sp
    from pyamg_amd import relaxation as grelax
    A, Sp, Sj, _, _ = large("size_edges")
    x0, b = F.start_vectors(A.shape[0])
    y = x0.copy()
    grelax.schwarz(sp.csr_array(A.copy()), y, b, iterations=2, subdomain=Sj.copy(), subdomain_ptr=F.without_empty(Sp), sweep="symmetric")
    want = np.load(GOLDEN / "kernels_schwarz_families.npz")["size_edges.symmetric2"]
    assert np.isfinite(want).all() and F.same_bits(y, want), int((y != want).sum())


def test_layer_1_repeats_a_timed_out_sweep_as_level_launches():
    """a persistent sweep that gives up waiting (forced through the PAMG_FORCE_TIMEOUT test hook: the first check reports a time-out, nothing is
    made to wait) leaves unfilled slots in x: overlapping_schwarz_csr repeats the sweep as one launch per level from the caller's x and returns the
    oracle's bits; the next call runs persistent again.  In a fresh process: the hook is read once"""
    import os
    import subprocess
    import sys
    code = (
        "import sys, ctypes as C, numpy as np\n"
        f"sys.path[:0] = [{str(ROOT)!r}, {str(ROOT / 'tests')!r}]\n"
        "import schwarz_families as F\n"
        "import pyamg_amd.amg_core as gcore\n"
        "from pyamg_amd import _capi as capi\n"
        "A, Sp, Sj, Tp, Tx = F.FAMILIES['size_edges'].make('large')\n"
        "n, nsub = A.shape[0], len(Sp) - 1\n"
        "x0, b = F.start_vectors(n)\n"
        "want = F.reference(A, Sp, Sj, Tp, Tx, x0, b, (0, nsub, 1))\n"
        "count = C.c_int64(-1)\n"
        "for reruns in (1, 1):\n"
        "    y = x0.copy()\n"
        "    gcore.overlapping_schwarz_csr(F.i32(A.indptr), F.i32(A.indices), A.data, y, b, Tx, Tp, Sj, Sp, nsub, n, 0, nsub, 1)\n"
        "    assert F.same_bits(y, want), int((y != want).sum())\n"
        "    capi.check(capi.lib().pamg_l1_schwarz_reruns(C.byref(count)), 'pamg_l1_schwarz_reruns')\n"
        "    assert count.value == reruns, count.value\n"
        "print('rerun ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, PAMG_FORCE_TIMEOUT="1"))
    assert r.returncode == 0 and "rerun ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
