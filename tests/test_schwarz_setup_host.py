"""Host checks of the Schwarz setup (CPU, no GPU): tests/schwarz_setup_emul.cpp replays pamg_schwarz_setup.hip through the per-lane
arithmetic of pyamg_amd/csrc/pamg_dense_pinv.h -- the lanes of a group and the groups of a wave as loops -- and is held against the
reference's blocks in the committed fixtures; the Python surface (schwarz_parameters(device=...), the split at 64 rows,
device_setup(schwarz=True)) is checked with the device call mocked.

Measured with this replay (err = |X - X_ref|_F / (eps kappa_+ |X_ref|_F), bound 64): worst 9.5 on the committed operators
(irr_float64), 10.3 on the chains (chain_float32); at most 12 Jacobi sweeps.  The device gives the same figures."""
import ctypes
import subprocess
import sys
import types
import warnings
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from pyamg_amd import relaxation as rx
import schwarz_setup_cases as sc

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent


@pytest.fixture(scope="module")
def emul():
    out = HERE / "build"
    out.mkdir(exist_ok=True)
    so = out / "schwarz_setup_emul.so"
    src = HERE / "schwarz_setup_emul.cpp"
    hdr = ROOT / "pyamg_amd" / "csrc" / "pamg_dense_pinv.h"
    if not so.exists() or so.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    return ctypes.CDLL(str(so))


def run(lib, A, sub, sptr, invert, sweep_cap=None, capacity=None):
    dt = np.dtype(A.dtype)
    fn = lib.sse_blocks_f64 if dt == np.float64 else lib.sse_blocks_f32
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)      # noqa: E731
    Ap, Aj, Ax, Sp, Sj = i32(A.indptr), i32(A.indices), np.ascontiguousarray(A.data), i32(sptr), i32(sub)
    m = np.diff(Sp).astype(np.int64)
    total = int(np.sum(m * m)) if capacity is None else capacity
    Tp, Tx = np.full(Sp.size, -7, dtype=np.int32), np.full(max(total, 1), 7.0, dtype=dt)
    info, rank = np.zeros(4, dtype=np.int64), np.full(max(Sp.size - 1, 1), -1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    rc = fn(A.shape[0], p(Ap), p(Aj), p(Ax), Sp.size - 1, p(Sp), p(Sj), p(Tp), p(Tx), ctypes.c_longlong(total),
            ctypes.c_double(rx._rank_tol(dt)), int(invert), int(lib.sse_sweep_cap() if sweep_cap is None else sweep_cap), p(info), p(rank))
    return rc, Tp, Tx[:total] if capacity is None else Tx, info, rank


@pytest.mark.parametrize("name", sc.ALL)
def test_extraction_is_the_references_bit_for_bit(emul, name):
    c = sc.cases()[name]
    rc, Tp, Tx, info, _ = run(emul, c.A, c.sub, c.sptr, invert=0)
    assert rc == 0
    assert np.array_equal(Tp, c.tptr) and Tp.dtype == np.int32
    assert Tx.dtype == c.blocks.dtype and np.array_equal(Tx, c.blocks)
    assert info[0] == c.tptr[-1] and info[1] == np.diff(c.sptr).max()


def test_duplicate_columns_take_the_first_stored_entry(emul):
    c = sc.cases()["dup"]
    A = c.A
    dup_rows = [i for i in range(A.shape[0]) if np.any(np.diff(A.indices[A.indptr[i]:A.indptr[i + 1]]) == 0)]
    assert len(dup_rows) >= 3
    _, _, Tx, _, _ = run(emul, A, c.sub, c.sptr, invert=0)
    for i in dup_rows:                                   # subdomain i is the pattern of row i: its row of the block that belongs to row i
        cols, vals = A.indices[A.indptr[i]:A.indptr[i + 1]], A.data[A.indptr[i]:A.indptr[i + 1]]
        S = c.sub[c.sptr[i]:c.sptr[i + 1]]
        m, r = S.size, int(np.searchsorted(S, i))
        row = Tx[c.tptr[i]:c.tptr[i + 1]].reshape(m, m)[r]
        first = np.array([vals[np.flatnonzero(cols == col)[0]] for col in S])
        last = np.array([vals[np.flatnonzero(cols == col)[-1]] for col in S])
        assert np.array_equal(row, first) and not np.array_equal(first, last)


@pytest.mark.parametrize("name", sc.INVERTED)
def test_pseudo_inverses_within_the_bound_and_of_the_references_rank(emul, name):
    c = sc.cases()[name]
    rc, Tp, Tx, info, rank = run(emul, c.A, c.sub, c.sptr, invert=1)
    assert rc == 0 and np.array_equal(Tp, c.tptr)
    worst, truncated = sc.compare_blocks(c, Tx)
    print(f"{name}: err / (eps kappa+) = {worst:.2f}, sweeps {info[2]}, truncated {info[3]}")
    assert worst <= sc.BOUND, (name, worst)
    assert info[3] == truncated and 0 <= info[2] <= emul.sse_sweep_cap()
    if name.startswith("chain_"):
        assert truncated == len(sc.CHAINS) and np.array_equal(rank[:len(sc.CHAINS)], np.array(sc.CHAINS) - 1)
        assert not Tx[:1].any()                                 # the length-1 chain: [0] -> [0]
    if name.startswith("chainp_"):
        assert truncated == 0 and np.array_equal(rank[:len(sc.CHAINS)], np.array(sc.CHAINS))


def test_all_zero_blocks_give_zero_blocks(emul):
    A = sp.csr_array((np.zeros(9), np.tile(np.arange(3, dtype=np.int32), 3), np.array([0, 3, 6, 9], dtype=np.int32)), shape=(3, 3))
    rc, _, Tx, info, rank = run(emul, A, np.arange(3), np.array([0, 3]), invert=1)
    assert rc == 0 and not Tx.any() and rank[0] == 0 and info[3] == 1


def test_a_block_that_has_not_converged_is_reported(emul):
    c = sc.cases()["pois_big"]
    rc, _, _, info, _ = run(emul, c.A, c.sub, c.sptr, invert=1, sweep_cap=1)
    assert rc == 3 and info[2] == 1


def test_a_subdomain_above_the_cap_is_refused_before_any_work(emul):
    n = 70
    A = sp.csr_array(sp.eye_array(n, format="csr") * 2.0)
    sub, sptr = np.arange(65, dtype=np.int32), np.array([0, 65], dtype=np.int32)
    assert emul.sse_max_m() == 64 == rx.DEVICE_BLOCK_CAP
    rc, Tp, Tx, info, _ = run(emul, A, sub, sptr, invert=1, capacity=65 * 65)
    assert rc == 2 and np.all(Tx == 7.0) and np.all(Tp == -7) and info[1] == 65
    rc, _, Tx, _, _ = run(emul, A, sub[:64], np.array([0, 64], dtype=np.int32), invert=1)
    assert rc == 0 and np.allclose(Tx.reshape(64, 64), 0.5 * np.eye(64), rtol=0, atol=1e-15)


def test_standalone_program_under_the_sanitizers(tmp_path):
    """the replay as a program of its own (its main), built with -fsanitize=address,undefined: nothing sanitized is loaded into Python"""
    exe = tmp_path / "sse"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-DSSE_MAIN", str(HERE / "schwarz_setup_emul.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr.lower() + r.stdout.lower() and "cannot find" in r.stderr.lower():
        pytest.skip("no sanitizer runtime for g++ here")
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])


# ------------------------------------------------------------------------------------------------------------ the Python surface
def _todays_schwarz_parameters(A):
    """schwarz_parameters as it stood before the device option: one searchsorted per row, one gelss call per subdomain"""
    import scipy.linalg as la
    subdomain, subdomain_ptr = A.indices.copy(), A.indptr.copy()
    inv, ptr = rx._subdomain_blocks(A, subdomain, subdomain_ptr)
    single = np.dtype(A.dtype).char.lower() == "f"
    rank_tol = (1e3 * np.finfo(np.single).eps) if single else (1e6 * np.finfo(np.double).eps)
    gelss, = la.get_lapack_funcs(["gelss"], (np.ones((1,), dtype=A.dtype),))
    for d, m in enumerate(np.diff(subdomain_ptr)):
        blk = inv[ptr[d]:ptr[d + 1]]
        blk[:] = np.ravel(gelss(blk.reshape(m, m), np.eye(m, m, dtype=A.dtype), cond=rank_tol, overwrite_a=True, overwrite_b=True)[1])
    return subdomain, subdomain_ptr, inv, ptr


@pytest.mark.parametrize("name", ["pois_float64", "pois_float32"])
def test_device_false_is_todays_schwarz_parameters(name):
    import inspect
    assert inspect.signature(rx.schwarz_parameters).parameters["device"].default is False
    assert inspect.signature(rx.schwarz).parameters["device"].default is False
    c = sc.cases()[name]
    A = c.A.copy()
    got = rx.schwarz_parameters(A)
    want = _todays_schwarz_parameters(c.A.copy())
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert np.array_equal(got[2], c.inv)                                   # and the reference's, bit for bit
    assert rx.schwarz_parameters(A) is got and A.schwarz_parameters is got and not hasattr(A, "schwarz_setup_report")
    assert rx.schwarz_parameters(A, device=True) is got                   # the cache rule comes first, as before


class _NoDevice:
    def __init__(self, op):
        self.handle = None

    def free(self):
        pass


def _split_problem():
    """a block-diagonal operator: blocks of 70, 3, 64, 5, 66 rows, one subdomain per block plus one of two rows"""
    rng = np.random.RandomState(3)
    sizes = (70, 3, 64, 5, 66)
    A = sp.block_diag([rng.rand(k, k) + k * np.eye(k) for k in sizes], format="csr")
    A = sp.csr_array(A); A.sort_indices()
    off = np.concatenate([[0], np.cumsum(sizes)])
    lists = [np.arange(off[i], off[i + 1]) for i in range(len(sizes))] + [np.array([1, 71])]
    sptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    return A, np.concatenate(lists).astype(np.int32), sptr


def test_subdomains_above_64_rows_stay_on_the_host_with_one_warning(monkeypatch):
    A, sub, sptr = _split_problem()
    want = rx.schwarz_parameters(A.copy(), sub, sptr)
    seen = {}

    def fake_device_blocks(dA, dtype, subdomain, subdomain_ptr, invert=True):
        seen["sizes"] = np.diff(subdomain_ptr).tolist()
        seen["sub"] = np.array(subdomain)
        Tx, Tp = rx._subdomain_blocks(A, np.asarray(subdomain), np.asarray(subdomain_ptr))
        rx._invert_blocks_host(dtype, Tx, Tp, subdomain_ptr)
        return Tx, Tp.astype(np.int32), [int(Tp[-1]), int(max(seen["sizes"])), 5, 0]

    monkeypatch.setattr(rx, "_device_blocks", fake_device_blocks)
    monkeypatch.setattr(rx, "DeviceMatrix", _NoDevice)
    B = A.copy()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = rx.schwarz_parameters(B, sub, sptr, device=True)
    assert len(w) == 1 and "2 of 6 subdomains" in str(w[0].message) and issubclass(w[0].category, RuntimeWarning)
    assert seen["sizes"] == [3, 64, 5, 2] and np.array_equal(seen["sub"][-2:], [1, 71])
    for g, x in zip(got, want):
        assert g.dtype == x.dtype and np.array_equal(g, x)                 # the host part is exact, the mocked part is the same host code
    assert B.schwarz_setup_report["on_host"] == 2 and B.schwarz_setup_report["largest"] == 70 and B.schwarz_setup_report["path"] == "device"
    # nothing above the cap: no warning
    C = A.copy()
    keep = np.array([1, 2, 3, 5])
    s2, p2 = rx._take_subdomains(sub, sptr, keep)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        rx.schwarz_parameters(C, s2.astype(np.int32), p2.astype(np.int32), device=True)
    assert not w and C.schwarz_setup_report["on_host"] == 0


def test_device_true_refuses_unsorted_rows_and_complex_operators(monkeypatch):
    monkeypatch.setattr(rx, "DeviceMatrix", _NoDevice)
    A = sp.csr_array((np.array([1.0, 2.0, 3.0]), np.array([1, 0, 1], dtype=np.int32), np.array([0, 2, 3], dtype=np.int32)), shape=(2, 2))
    with pytest.raises(ValueError):
        rx.schwarz_parameters(A, device=True)
    Z = sp.csr_array(np.eye(2, dtype=np.complex128))
    with pytest.raises(NotImplementedError):
        rx.schwarz_parameters(Z, device=True)


def test_device_setup_patches_and_restores_schwarz_parameters(monkeypatch):
    from pyamg_amd import aggregation as agg
    calls = []

    def reference_fn(A, subdomain=None, subdomain_ptr=None, inv_subblock=None, inv_subblock_ptr=None):
        calls.append("reference")
        return "reference"

    pkg, rel, relrel = types.ModuleType("standin_amg"), types.ModuleType("standin_amg.relaxation"), types.ModuleType("standin_amg.relaxation.relaxation")
    relrel.schwarz_parameters = reference_fn
    pkg.relaxation, rel.relaxation = rel, relrel
    for m in (pkg, rel, relrel):
        monkeypatch.setitem(sys.modules, m.__name__, m)

    def device_fn(A, subdomain=None, subdomain_ptr=None, inv_subblock=None, inv_subblock_ptr=None, device=False):
        calls.append(("device", device))
        return "device"

    monkeypatch.setattr(rx, "schwarz_parameters", device_fn)
    with agg.device_setup(pkg, products=False):
        assert relrel.schwarz_parameters is reference_fn               # off by default
    with agg.device_setup(pkg, products=False, schwarz=True):
        patched = relrel.schwarz_parameters
        assert patched is not reference_fn and patched.__name__ == "schwarz_parameters"
        A = sp.csr_array(sp.eye_array(3, format="csr"))
        assert patched(A) == "device"
        assert patched(A.astype(np.complex128)) == "reference"         # not on the device path: the function that was patched out
        assert patched(A.tocsc()) == "reference"
    assert relrel.schwarz_parameters is reference_fn
    assert calls == [("device", True), "reference", "reference"]
    with pytest.raises(RuntimeError):
        with agg.device_setup(pkg, products=False, schwarz=True):
            raise RuntimeError("inside")
    assert relrel.schwarz_parameters is reference_fn
