"""The BITS of the cluster layout's sweeps (c_group, pyamg_amd/csrc/pamg_lane.hip) are pinned: a change of how the kernel moves values between
lanes -- the row sums' segmented scan runs in registers (seg_scan_incl, pamg_wave.h) -- must not change a single bit of any sweep.

Operators: the families of tests/sweep_families.py that take the cluster layout in both directions and hold zero-iterate plans (2 000 .. 4 192
rows).  Settings: lanem_cluster 4 and 8 x lane_merge 3 .. 6; per setting one forward sweep, one backward sweep and the fused symmetric sweep from
a random iterate (the general plans), the symmetric sweep announced from zero (the zero-iterate form) and one step in correction form; the last
three also as two directional launches (sym_fused = 0), which must give the fused launch's bits -- so all six cluster kernels run.

Two pins:
  * tests/lanec_emul.cpp replays the general plans with c_group's association (products in slot order, then the loop
    s[i] += s[i - d] for d = 1 .. 32 inside a row's lanes): the device's forward, backward and fused symmetric sweeps EQUAL that replay bit for bit.
    This held on the build before the scan moved into registers (every case below), so it is asserted.  The replay is compiled into tests/build
    as tests/test_lanec_plan.py does; without a host compiler that part is skipped.
  * the replay has no zero-iterate and no correction form, so tests/golden/lanec_bits.json holds a digest (SHA-256 of the float64 bytes, first 16
    hex digits) of every output, recorded from the build before the change -- the project's own results.  All five forms are compared with it.
The declared form must have run (lanem_info: cluster_rows, rows, s_max of plans 0, 1, 4, 5; correction_launches), the error word stays clear."""
import ctypes
import hashlib
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import sweep_families as F
from pyamg_amd import _capi as capi
from pyamg_amd.hierarchy import sparse_op
from pyamg_amd.multilevel import DeviceMatrix

pytestmark = pytest.mark.gpu

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
FIXTURE = HERE / "golden" / "lanec_bits.json"
FAMILIES = ("nonsym", "mixed_sign", "nodiag", "lane_edge", "mixed_lengths", "wide", "tridiag", "chains", "convdiff_l1")
CLUSTERS = (4, 8)
MERGES = (3, 4, 5, 6)
GENERAL = ("forward", "backward", "symmetric")
FORMS = GENERAL + ("zero", "correction")


def digest(v):
    return hashlib.sha256(np.ascontiguousarray(v, dtype=np.float64).tobytes()).hexdigest()[:16]


def case_key(name, cluster, merge, form):
    return f"{name}/c{cluster}/s{merge}/{form}"


def build_emul():
    """tests/build/lanec_emul.so (the recipe of tests/test_lanec_plan.py), or None without a host compiler"""
    if not shutil.which("g++"):
        return None
    out = HERE / "build"
    out.mkdir(exist_ok=True)
    so, src = out / "lanec_emul.so", HERE / "lanec_emul.cpp"
    hdrs = [ROOT / "pyamg_amd" / "csrc" / h for h in ("pamg_lanem_plan.h", "pamg_lane_plan.h", "pamg_tile_plan.h")]
    if not so.exists() or so.stat().st_mtime < max([src.stat().st_mtime] + [h.stat().st_mtime for h in hdrs]):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.lanec_emul_sweep_f64.restype = ctypes.c_int
    lib.lanec_emul_sym_f64.restype = ctypes.c_int
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def replay(lib, S, x, b, form, merge, cluster):
    """the general plans' sweep `form` of x by tests/lanec_emul.cpp (waves = 0: groups in order)"""
    n = S.shape[0]
    Ap, Aj, Ax = (np.ascontiguousarray(S.indptr, dtype=np.int32), np.ascontiguousarray(S.indices, dtype=np.int32), np.ascontiguousarray(S.data, dtype=np.float64))
    xx, bb = np.array(x, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    stats = np.zeros(36, dtype=np.int64)
    if form == "symmetric":
        rc = lib.lanec_emul_sym_f64(ctypes.c_int(n), _p(Ap), _p(Aj), _p(Ax), _p(xx), _p(bb), merge, ctypes.c_double(1e3), cluster, _p(stats), 0, 0)
    else:
        start, stop, step = (0, n, 1) if form == "forward" else (n - 1, -1, -1)
        rc = lib.lanec_emul_sweep_f64(ctypes.c_int(n), _p(Ap), _p(Aj), _p(Ax), _p(xx), _p(bb), start, stop, step, merge, ctypes.c_double(1e3), cluster,
                                      _p(stats), 0, 0)
    assert rc == 0, (form, merge, cluster, rc)
    return xx


def vectors(S):
    rng = np.random.RandomState(5)
    n = S.shape[0]
    return rng.rand(n), rng.rand(n)


def device_sweeps(S, cluster, merge, x, b):
    """{form: iterate} of the fused launches; the two-launch twins of the symmetric forms must carry the same bits"""
    n = S.shape[0]
    A = DeviceMatrix(sparse_op(sp.csr_array(S)))
    A.tune(gs_order=1, lane_wide=1, line_scan=0, sym_fused=1, zero_plans=2, lanem_cluster=cluster, lanem_rpw=0, lane_merge=merge)
    dx, db, dr = (capi.DeviceArray.from_host(v) for v in (x, b, np.zeros(n)))
    z = np.zeros(n)
    out = {}

    def run(form):
        dx.upload(z if form == "zero" else x)
        if form in ("forward", "backward"):
            A.gauss_seidel(dx, db, sweep=form)
        elif form == "correction":
            A.gauss_seidel_correction(dx, db, dr)
        else:
            A.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=1, x_is_zero=form == "zero")
        return dx.download()

    for form in FORMS:
        out[form] = run(form)
    si = A.sym_info()
    assert si["launches"] > 0 and si["form"] == "merged" and si["correction_launches"] == 1 and si["zero_plan_launches"] == 2, (cluster, merge, si)
    assert si["handoff_not_sentinel"] == 0 and si["counters_not_zero"] == 0, si
    A.tune(sym_fused=0)
    for form in ("symmetric", "zero", "correction"):
        assert np.array_equal(run(form), out[form]), (cluster, merge, form, "two launches != the fused launch")
    assert A.sym_info()["correction_launches"] == 2 and A.sym_info()["zero_plan_launches"] == 4, A.sym_info()
    for which in (0, 1, 4, 5):
        mi = A.lanem_info(which)
        assert mi["rows"] == n and mi["cluster_rows"] == cluster, (cluster, merge, which, mi)          # the cluster layout is what ran
        assert which >= 4 or mi["s_max"] == merge, (cluster, merge, which, mi)
    assert not A.flow_error()
    for v in (dx, db, dr):
        v.free()
    A.free()
    return out


def collect(name, emul):
    """{case key: (digest, equals the replay | None)} of one family"""
    fam = F.FAMILIES[name]
    assert F.expected(fam.form, 8, 0) == (True, True, True), name
    S = fam.make("large")
    x, b = vectors(S)
    res = {}
    for cluster in CLUSTERS:
        for merge in MERGES:
            out = device_sweeps(S, cluster, merge, x, b)
            for form in FORMS:
                same = None
                if emul is not None and form in GENERAL:
                    same = bool(np.array_equal(out[form], replay(emul, S, x, b, form, merge, cluster)))
                res[case_key(name, cluster, merge, form)] = (digest(out[form]), same)
    return res


@pytest.fixture(scope="module")
def emul():
    return build_emul()


@pytest.fixture(scope="module")
def recorded():
    return json.loads(FIXTURE.read_text())["cases"]


@pytest.mark.parametrize("name", FAMILIES)
def test_sweeps_keep_their_bits(name, emul, recorded):
    res = collect(name, emul)
    assert len(res) == len(CLUSTERS) * len(MERGES) * len(FORMS)
    moved = [k for k, (d, _) in res.items() if recorded[k] != d]
    off_replay = [k for k, (_, same) in res.items() if same is False]
    print(f"\n[lanec bits] {name}: {len(res)} outputs, {len(moved)} differ from the recorded bits, "
          f"{'no host compiler: replay not run' if emul is None else str(len(off_replay)) + ' differ from the replay of tests/lanec_emul.cpp'}")
    assert not off_replay, off_replay
    assert not moved, moved


def test_the_fixture_holds_these_cases_and_no_others(recorded):
    want = {case_key(n, c, s, f) for n in FAMILIES for c in CLUSTERS for s in MERGES for f in FORMS}
    assert set(recorded) == want
    assert all(len(d) == 16 and int(d, 16) >= 0 for d in recorded.values())

