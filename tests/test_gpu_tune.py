"""pamg_matrix_tune against its record from commit 8f4a1d7, the last one whose tune call was a switch over key numbers
(tests/golden/tune_table.npz, written there by tests/golden/make_golden_tune.py; the recording is tests/tune_cases.py, which sets every key BY
NUMBER through the C ABI):
  * what every key in 0..45 and key 1000 answers to 96 values on a free operator, and how key 0 stores its value;
  * what they answer on an operator that a solver holds;
  * what setting each live key drops from an operator that holds schedules, lane / merged / line / tile parts, zero-iterate plans and a
    point twin: every observable of the info calls before and after, the operator's bytes exactly;
and the point twin of a block operator, rebuilt after one of the keys it inherits changed, sweeps to the bits of a fresh operator that had
the setting from the start, and to the bits of the flattened rows as a scalar operator with that setting."""
import numpy as np
import pytest

import tune_cases as tc
from conftest import GOLDEN
from pyamg_amd import _capi as capi
from pyamg_amd.hierarchy import sparse_op
from pyamg_amd.multilevel import TUNE_KEYS, DeviceMatrix

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN / "tune_table.npz")
    assert z["keys"].tolist() == tc.KEYS and z["values"].tolist() == tc.VALUES
    return z


def test_every_key_accepts_and_stores_what_it_did(golden):
    rc, win = tc.accept()
    live = [k for k, row in zip(tc.KEYS, rc) if (row == capi.OK).any()]
    assert live == sorted(TUNE_KEYS.values()) == sorted(tc.DEFAULTS)
    bad = [(tc.KEYS[i], tc.VALUES[j], int(rc[i, j]), int(golden["accept.rc"][i, j])) for i, j in zip(*np.nonzero(rc != golden["accept.rc"]))]
    assert not bad, f"(key, value, return code, recorded): {bad[:20]}"
    bad = [(tc.KEYS[i], tc.VALUES[j], int(win[i, j]), int(golden["accept.window"][i, j])) for i, j in zip(*np.nonzero(win != golden["accept.window"]))]
    assert not bad, f"(key, value, LDS window, recorded): {bad[:20]}"


def test_a_held_operator_refuses_what_it_did(golden):
    vals, rc = tc.refuse(golden["accept.rc"])
    assert np.array_equal(vals, golden["refuse.values"])
    assert rc.tolist() == golden["refuse.rc"].tolist(), dict(zip(tc.KEYS, zip(rc.tolist(), golden["refuse.rc"].tolist())))
    assert rc[tc.KEYS.index(45)] == rc[tc.KEYS.index(1000)] == capi.E_STATE        # an unknown key on a held operator: the state is checked first


@pytest.mark.parametrize("scene", list(tc.SCENES))
def test_every_key_drops_what_it_did(golden, scene):
    acts, rc, before, after = tc.effect(scene)
    assert np.array_equal(acts, golden[f"effect.{scene}.actions"])
    assert np.array_equal(rc, golden[f"effect.{scene}.rc"]), (rc, golden[f"effect.{scene}.rc"])
    for what, got in (("before", before), ("after", after)):
        want = golden[f"effect.{scene}.{what}"]
        bad = [(tuple(acts[i]), j, int(got[i, j]), int(want[i, j])) for i, j in zip(*np.nonzero(got != want))]
        assert not bad, f"{scene}, {what} the call ((key, value), observable, value, recorded): {bad[:20]}"


@pytest.mark.parametrize("key", sorted(tc.INHERITED))
def test_the_rebuilt_twin_inherits_the_key(key):
    """operator 1 builds its twin with the defaults, then has the key set: the twin goes, and the next sweep builds it with the new value;
    operator 2 has the value before its first sweep.  Both go through the same copy of the fields, so the witness that the value ARRIVED is
    operator 3: the flattened rows as a scalar CSR operator with the key set on it directly -- what the twin is meant to be.  The keys of
    the merged form (34, 35, 38) are set on operators that ask for it.
    What the bits can tell (measured with a library whose twin inherited nothing: the cases of keys 25, 33, 34, 35 and 38 failed, the last
    three because the twin then lacked key 33 as well): lanes per row, merge depth and cluster layout change the association of the row
    sums.  Keys 7, 26, 27, 28, 30 -- and 34, 35 on their own -- choose grids, gates and schedulers: every value gives the same bits on this
    operator, so their cases show that the rebuilt twin sweeps right, not that the value reached it."""
    value = tc.INHERITED[key]
    blocks = tc.block_operator()
    op = sparse_op(blocks)
    setup = {24: 1, 33: 4} if key in (34, 35, 38) else {24: 1}
    n = op.shape[0]
    x0, b = np.linspace(0.0, 1.0, n), np.cos(np.arange(n, dtype=np.float64))
    dx, db = capi.DeviceArray.from_host(x0), capi.DeviceArray.from_host(b)

    def sweep(A):
        dx.upload(x0)
        for direction in ("forward", "backward"):          # what the point sweep of a block operator runs on its twin
            A.gauss_seidel(dx, db, sweep=direction)
        assert not A.flow_error()
        return dx.download()

    def operator(o, first):
        A = DeviceMatrix(o)
        for k, v in {**setup, **first}.items():
            assert tc.tune(A, k, v) == capi.OK, (k, v)
        return A

    A1, A2, A3 = operator(op, {}), operator(op, {key: value}), operator(sparse_op(blocks.tocsr()), {key: value})
    x_default = sweep(A1)
    assert A1.point_twin() == 1
    assert tc.tune(A1, key, value) == capi.OK
    assert A1.point_twin() == 0                      # dropped: it held the old value
    x1, x2, x3 = sweep(A1), sweep(A2), sweep(A3)
    assert A1.point_twin() == 1 and A2.point_twin() == 1
    assert A1.info()["hbm_bytes"] == A2.info()["hbm_bytes"], "the rebuilt twin is not the twin of a fresh operator"
    print(f"\n[tune] key {key} = {value}: the setting changes the bits of this sweep: {not np.array_equal(x3, x_default)}")
    assert np.array_equal(x1, x2), f"key {key} = {value}: rebuilt against fresh, max difference {np.max(np.abs(x1 - x2)):.3e}"
    assert np.array_equal(x2, x3), f"key {key} = {value}: twin against the scalar operator, max difference {np.max(np.abs(x2 - x3)):.3e}"
    for A in (A1, A2, A3):
        A.free()
