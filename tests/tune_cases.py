"""What tests/golden/make_golden_tune.py records and tests/test_gpu_tune.py replays: the answers and the effects of pamg_matrix_tune.

Every tune call here goes through the C ABI BY NUMBER, so the same code runs on a library from before the keys had names and on one
after.  Three recordings (the fixture's arrays are named after them):

  accept_*   a 64-row 1-D Poisson operator (f64, CSR), fresh per key: every key of KEYS with every value of VALUES -> the return code
             and pamg_matrix_info[4] (the LDS window: shows how key 0 stores its value) after the call
  refuse_*   the same operator held by a one-level solver: every key of KEYS with the first value accept_* took (0 where it took none)
             -> the return code
  effect_*   per scene of SCENES an operator with its schedules, lane / merged / line / tile parts, zero-iterate plans and point twin
             built by one symmetric sweep and one symmetric sweep announced from x = 0; then, on a fresh such operator per action, one
             key set to the value it already has -> the observables (observe()) before and after the call.  Bytes are part of them.
"""
import ctypes as C

import numpy as np
import scipy.sparse as sp

from pyamg_amd import _capi as capi
from pyamg_amd.hierarchy import sparse_op
from pyamg_amd.multilevel import DeviceMatrix

KEYS = list(range(46)) + [1000]
# every small value, every power of two up to 2^17, and both sides of every bound the keys have
VALUES = sorted(set(range(-2, 71)) | {1 << k for k in range(18)}
                | {255, 256, 257, 400, 401, 1020, 1021, 2048, 2049, 8192, 8193, 12288, 12289, 98304, 98305})

# the live keys and the value each has on a fresh operator (include/pyamg_amd.h; key 0 is read from pamg_matrix_info[4] instead:
# an operator that streams value codes raises it at creation)
DEFAULTS = {0: None, 2: 1024, 3: 32, 5: 0, 6: 0, 7: 0, 8: 0, 11: 0, 12: 0, 13: 0, 14: 0, 15: 0, 16: 0, 17: -1, 18: 1, 19: 1, 20: 0, 21: 1,
            22: 1, 23: 1, 24: 0, 25: 0, 26: 0, 27: 0, 28: 1, 30: 1, 31: 8, 32: 3, 33: 0, 34: 40, 35: 0, 36: 0, 37: 1, 38: 0, 39: 0, 40: 0, 41: 0}
# the fields the scalar twin of a block operator takes over, each with a legal value that is not its default
INHERITED = {7: 2, 25: 8, 26: 2, 27: 1, 28: 0, 30: 0, 33: 4, 34: 20, 35: 2, 38: 4}


def poisson1d(n=64):
    return sp.diags_array([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], offsets=[-1, 0, 1], format="csr")


def poisson2d(n=16):
    T, I = poisson1d(n), sp.eye_array(n, format="csr")
    return (sp.kron(T, I) + sp.kron(I, T)).tocsr()


def poisson3d(n=16):
    """4096 rows: the smallest schedule the line scan takes"""
    T, I = poisson1d(n), sp.eye_array(n, format="csr")
    return (sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T)).tocsr()


def block_operator(nb=64):
    """2 x 2 blocks, nb block rows, block tridiagonal, symmetric positive definite"""
    return sp.bsr_array(sp.kron(poisson1d(nb), np.array([[2.0, -0.5], [-0.5, 2.0]])).tocsr(), blocksize=(2, 2))


# scene -> (operator, the keys set before the sweeps).  All in fast order with zero-iterate plans asked for, except `tiled`: the exact
# order's tiled sweep, the only form that builds tile parts.  `merged` asks for the merged lane form by name (five entries per row are
# below the automatic choice's bar), which is also what the zero-iterate plans need; `line` asks for the line scan wherever it applies, on a 16^3 lattice.
SCENES = {
    "lanes": (poisson2d, {24: 1, 39: 2}),
    "merged": (poisson2d, {24: 1, 33: 4, 39: 2}),
    "line": (poisson3d, {24: 1, 30: 2}),
    "twin": (block_operator, {24: 1, 39: 2}),
    "tiled": (poisson2d, {5: 5}),
}


def tune(A, key, value):
    return int(capi.lib().pamg_matrix_tune(A.handle, int(key), int(value)))


def window(A):
    return A.info()["lds_entries"]


def observe(A):
    """int64 [132]: pamg_matrix_info[5..7], lane_info(0, 1), lanem_info(0, 1, 4, 5), line_info(0, 1), tile_info(0, 1), the point twin's state"""
    lib, h, out = capi.lib(), A.handle, []
    a = (C.c_int64 * 8)()
    capi.check(lib.pamg_matrix_info(h, a), "pamg_matrix_info")
    out += list(a)[5:8]
    for which in (0, 1):
        capi.check(lib.pamg_matrix_lane_info(h, which, a), "pamg_matrix_lane_info")
        out += list(a)
    m = (C.c_int64 * 20)()
    for which in (0, 1, 4, 5):
        capi.check(lib.pamg_matrix_lanem_info(h, which, m, None), "pamg_matrix_lanem_info")
        out += list(m)
    for fn in ("pamg_matrix_line_info", "pamg_matrix_tile_info"):
        for which in (0, 1):
            capi.check(getattr(lib, fn)(h, which, a), fn)
            out += list(a)
    st = C.c_int(0)
    capi.check(lib.pamg_matrix_point_twin(h, C.byref(st)), "pamg_matrix_point_twin")
    out.append(st.value)
    return np.array(out, dtype=np.int64)


def accept():
    """(codes [keys, values], windows [keys, values])"""
    op = sparse_op(poisson1d())
    rc = np.zeros((len(KEYS), len(VALUES)), dtype=np.int32)
    win = np.zeros_like(rc)
    for i, key in enumerate(KEYS):
        A = DeviceMatrix(op)
        for j, v in enumerate(VALUES):
            rc[i, j], win[i, j] = tune(A, key, v), window(A)
        A.free()
    return rc, win


def refuse(accept_rc):
    """(values [keys], codes [keys]) on an operator that a solver holds"""
    lib = capi.lib()
    A = DeviceMatrix(sparse_op(poisson1d()))
    S = C.c_void_p()
    capi.check(lib.pamg_solver_create(C.byref(S), capi.F64), "pamg_solver_create")
    capi.check(lib.pamg_solver_add_level(S, A.handle, None, None), "pamg_solver_add_level")
    vals = np.array([next((v for v, r in zip(VALUES, row) if r == capi.OK), 0) for row in accept_rc], dtype=np.int32)
    rc = np.array([tune(A, key, v) for key, v in zip(KEYS, vals)], dtype=np.int32)
    capi.check(lib.pamg_solver_destroy(S), "pamg_solver_destroy")
    A.free()
    return vals, rc


def swept(op, setup):
    """the operator after `setup`, one symmetric sweep and one symmetric sweep announced from x = 0; and the iterate"""
    A = DeviceMatrix(op)
    for key, v in setup.items():
        assert tune(A, key, v) == capi.OK, (key, v)
    n = op.shape[0]
    x, b = capi.DeviceArray.from_host(np.linspace(0.0, 1.0, n)), capi.DeviceArray.from_host(np.cos(np.arange(n, dtype=np.float64)))
    A.gauss_seidel(x, b, sweep="symmetric")
    x.upload(np.zeros(n))
    A.gauss_seidel_x0(x, b, sweep="symmetric", x_is_zero=True)
    assert not A.flow_error()
    return A, x.download()


def actions(setup):
    """every live key with the value it has after `setup`, then key 39 = 1 (the one value of a key whose effect differs)"""
    return [(key, setup.get(key, v)) for key, v in DEFAULTS.items()] + [(39, 1)]


def effect(scene):
    """(actions [n, 2], codes [n], before [n, 132], after [n, 132])"""
    make, setup = SCENES[scene]
    op = sparse_op(make())
    acts, rc, before, after = [], [], [], []
    for key, v in actions(setup):
        A, _ = swept(op, setup)
        if v is None:
            v = window(A)
        before.append(observe(A))
        rc.append(tune(A, key, v))
        after.append(observe(A))
        acts.append((key, v))
        A.free()
    return np.array(acts, dtype=np.int32), np.array(rc, dtype=np.int32), np.array(before), np.array(after)
