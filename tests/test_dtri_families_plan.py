"""The dense block-triangular form of the symmetric Gauss-Seidel sweep on the adversarial families of tests/dtri_families.py (CPU, no GPU): every
case at the small size through the stand-alone replay tests/dtri_emul.cpp of pyamg_amd/csrc/pamg_dtri_plan.h, arrays as stored (nothing sorted or
summed on the way).

Every case declares its outcome and the test asserts it: status, block count, growth figure (1e-10 relative against NumPy's dense inverses of the
diagonal blocks; exact for the chains, whose inverses hold powers of three), off-block entries where the family is about them.  Engaging cases are
compared, from zero and in correction form (the residual is formed here, the program accumulates), with the oracle's sequential sweep on long-double
copies: 1e-13 relative in the max norm, the project's per-sweep bar (measured: 6e-16 at the most).  `rowscale` gives the bits and the growth of the
unscaled operator.  A declining case leaves x as it was.

The two size declines (more than 65535 blocks, triangles above 2 GB) are rules of build_dtri_part on the device, not of the plan header: here the
arithmetic of the rule is checked against the header's layout, and the engaging twin (600 rows at B = 1) is replayed.

Found by `nonfinite_*_off_block` with the parent's header: a NaN or inf stored in ONE off-block entry (row 128 of 300, B = 64) was accepted (status 0,
growth 1.532) and the form left 128 rows finite where the sequential sweep leaves 179 -- a dense triangle multiplies its stored zeros by the value
(on the shifted block-diagonal operator of 192 rows: 0 against 180).  build_dtri_plan now declines every non-finite stored value (DTRI_E_NONFINITE); in-block ones were growth declines before.

One case of every outcome runs once more under the program's -fsanitize=address,undefined build."""
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import dtri_families as F
import sweep_families as SF
from test_dtri_plan import emul, emul_san  # noqa: F401 -- the replay program's two builds (fixtures)

SMALL = F.cases("small")


def run(prog, tmp, A, B, b, x=None):
    """(status, blocks, off-block entries, slots, growth, x) of one replay on the arrays as stored: x = S b, or x + S b where an iterate is given"""
    A = sp.csr_array(A)
    n = A.shape[0]
    Ap, Aj, Ax = (np.ascontiguousarray(A.indptr, dtype=np.int32), np.ascontiguousarray(A.indices, dtype=np.int32),
                  np.ascontiguousarray(A.data, dtype=np.float64))
    case, res = tmp / "case.bin", tmp / "result.bin"
    with open(case, "wb") as f:
        np.array([n, Ax.size, B, 0 if x is None else 1], dtype=np.int32).tofile(f)
        for a in (Ap, Aj, Ax, np.ascontiguousarray(b, dtype=np.float64), np.zeros(n) if x is None else np.ascontiguousarray(x, dtype=np.float64)):
            a.tofile(f)
    subprocess.run([str(prog), str(case), str(res)], check=True)
    raw = res.read_bytes()
    status, blocks = np.frombuffer(raw, dtype=np.int32, count=2)
    off, slots = np.frombuffer(raw, dtype=np.int64, count=2, offset=8)
    growth = float(np.frombuffer(raw, dtype=np.float64, count=1, offset=24)[0])
    return int(status), int(blocks), int(off), int(slots), growth, np.frombuffer(raw, dtype=np.float64, count=n, offset=32).copy()


def _vectors(c):
    A = c.A()
    b, x0 = F.vectors(A.shape[0])
    if c.name == "rowscale":
        b = np.ldexp(b, F.rowscale_exponents(A.shape[0]))
    return A, b, x0


def check_engages(prog, tmp, c):
    A, b, x0 = _vectors(c)
    n = A.shape[0]
    st, nb, off, slots, growth, x = run(prog, tmp, A, c.B, b)
    assert (st, nb) == (F.OK, c.blocks()), (c.id, st, nb)
    want = c.growth()
    if c.name.startswith("chains"):
        assert growth == want, (c.id, growth, want)
    else:
        assert abs(growth - want) <= 1e-10 * want, (c.id, growth, want)
    assert growth <= F.GROWTH_CAP
    if c.off_block is not None:
        assert off == c.off_block, (c.id, off)
    sizes = [min(c.B, n - k * c.B) for k in range(nb)]
    assert slots == sum(F.tri_slots(m) for m in sizes)
    err0 = SF.rel_err(x, SF.ref_sweeps(A, np.zeros(n), b, "symmetric", dtype=np.longdouble))
    st1, _, _, _, _, x1 = run(prog, tmp, A, c.B, b - A @ x0, x0)
    assert st1 == F.OK
    err1 = SF.rel_err(x1, SF.ref_sweeps(A, x0, b, "symmetric", dtype=np.longdouble))
    print(f"[dtri families] {c.id} ({n} rows): {nb} blocks, {off} off-block entries, growth {growth:.6g} (NumPy {want:.6g}); "
          f"from zero {err0:.2e}, correction form {err1:.2e} against the long-double sweep")
    assert err0 <= F.TOL and err1 <= F.TOL, (c.id, err0, err1)
    return growth, x, x1


def check_declines(prog, tmp, c):
    A, b, x0 = _vectors(c)
    n = A.shape[0]
    st, nb, _, _, growth, x = run(prog, tmp, A, c.B, b)
    assert st == c.status, (c.id, st)
    assert np.array_equal(x, np.zeros(n)), "a decline leaves x alone"
    st, _, _, _, _, x1 = run(prog, tmp, A, c.B, b, x0)
    assert st == c.status and np.array_equal(x1, x0)
    if c.outcome == "declines_growth":
        assert growth > F.GROWTH_CAP and (c.exact_growth is None or growth == c.exact_growth), (c.id, growth)
    print(f"[dtri families] {c.id} ({n} rows): declines with status {st}, growth {growth:.6g}")


@pytest.mark.parametrize("c", [c for c in SMALL if c.outcome == "engages"], ids=lambda c: c.id)
def test_engages(emul, tmp_path, c):
    check_engages(emul, tmp_path, c)


@pytest.mark.parametrize("c", [c for c in SMALL if c.outcome != "engages"], ids=lambda c: c.id)
def test_declines(emul, tmp_path, c):
    check_declines(emul, tmp_path, c)


def test_every_outcome_is_covered():
    assert {c.outcome for c in SMALL} == {"engages", "declines_host", "declines_growth"}
    assert {c.outcome for c in F.cases("large")} == {"engages", "declines_host", "declines_growth", "declines_size"}
    assert {c.status for c in SMALL if c.outcome == "declines_host"} == {F.E_DIAGONAL, F.E_NONFINITE}


@pytest.mark.parametrize("B", [16, 65])
def test_rowscale_gives_the_bits_of_the_unscaled_operator(emul, tmp_path, B):
    """2^e_i on row i of A and of b: every product is scaled by a power of two and scaled back by the diagonal"""
    c = next(c for c in SMALL if c.name == "rowscale" and c.B == B)
    g1, x, x1 = check_engages(emul, tmp_path, c)
    A0 = F.nonsym_rows(c.A().shape[0])
    b, x0 = F.vectors(A0.shape[0])
    _, _, _, _, g0, y = run(emul, tmp_path, A0, B, b)
    _, _, _, _, _, y1 = run(emul, tmp_path, A0, B, b - A0 @ x0, x0)
    assert g1 == g0 and np.array_equal(x, y) and np.array_equal(x1, y1)


@pytest.mark.parametrize("value", ["nan", "inf"])
def test_one_non_finite_off_block_value_is_not_spread(emul, tmp_path, value):
    """why the planner declines: the sequential sweep keeps such a value to the rows that depend on it; dense triangles would not"""
    c = next(c for c in SMALL if c.name == f"nonfinite_{value}_off_block")
    A, b, _ = _vectors(c)
    with np.errstate(all="ignore"):
        seq = SF.ref_sweeps(A, np.zeros(A.shape[0]), b, "symmetric")
    finite = int(np.isfinite(seq).sum())
    print(f"[dtri families] {c.id}: the sequential sweep leaves {finite} of {A.shape[0]} rows finite")
    assert finite == 179                                              # (the parent's header: accepted, 128 rows finite)
    assert run(emul, tmp_path, A, c.B, b)[0] == F.E_NONFINITE


def test_block_aligned_slices():
    """the declaration of the family itself: aligned -- no off-block entry; shifted -- one Lo entry in every block but the first, one Uo entry in every
    block but the last"""
    for c in SMALL:
        if not c.name.startswith("block_aligned"):
            continue
        A, B, nb = sp.coo_array(c.A()), c.B, c.blocks()
        kb = A.row // B
        lo, up = np.bincount(kb[A.col < kb * B], minlength=nb), np.bincount(kb[A.col >= (kb + 1) * B], minlength=nb)
        want = [0] * nb if c.name == "block_aligned" else [0] + [1] * (nb - 1)
        assert list(lo) == want and list(up) == want[::-1], (c.id, lo, up)


def test_size_rules():
    """the device's two size declines against the header's layout: 65536 blocks are one too many; four blocks of 8192 rows take 2 148 007 936 bytes
    in both directions, above the 2^31 cap, while eight blocks of 4096 rows fit"""
    big = {c.name: c for c in F.cases("large") if c.outcome == "declines_size"}
    assert set(big) == {"too_many_blocks", "too_many_bytes"}
    assert -(-65536 // big["too_many_blocks"].B) == F.MAX_BLOCKS + 1 and F.tri_bytes(65536, 1) <= F.MAX_BYTES
    assert F.tri_bytes(32768, big["too_many_bytes"].B) == 2148007936 > F.MAX_BYTES
    assert F.tri_bytes(32768, 4096) <= F.MAX_BYTES and -(-32768 // 8192) <= F.MAX_BLOCKS
    assert F.tri_slots(8192) == 2 * 4096 * 4097


def test_under_sanitizers(emul_san, tmp_path):
    """one case of every outcome under the address and undefined-behaviour sanitizers (run() raises where the program does not exit clean); the size
    declines are the device's: their engaging twin of 600 one-row blocks stands in"""
    by_id = {c.id: c for c in SMALL}
    for cid in ("nonsym[33]-B16", "nonsym[31]-B16", "stored-B65", "rowscale-B16", "dense_rows[300]-B65", "dense_rows[9]-B1", "arrow-B16",
                "block_aligned_shifted-B16", "lower_only-B65", "chains7-B4", "tridiag[600]-B1"):
        check_engages(emul_san, tmp_path, by_id[cid])
    for cid in ("chains7-B64", "bad_diag_missing-B64", "bad_diag_twice-B64", "bad_diag_nan-B64", "nonfinite_nan_in_block-B64",
                "nonfinite_inf_off_block-B64"):
        check_declines(emul_san, tmp_path, by_id[cid])
