"""The plan of the persistent Schwarz sweep (pyamg_amd/csrc/pamg_schwarz_plan.h) on the subdomain families of tests/schwarz_families.py (CPU, no GPU):
every family at its small size goes through the replay tests/schwarz_emul.cpp -- which consumes the version table the way schwarz_versioned_kernel
does and asserts what the device relies on (no deadlock for any number of waves, single assignment, consecutive versions) -- with 1, 3, 64 and
100000 waves, forward, backward and strided, and must take its DECLARED form: return code 0 and the bits of the oracle's sequential sweep
(amg_core::overlapping_schwarz_csr, relaxation.h:1420-1492), or return code 2 with the declared reason.  What a declined schedule computes is the
level kernel's business: tests/test_gpu_schwarz_families.py.  The families' own claims (sizes, update counts, depth, shared levels) are checked
here too, so that the device test sweeps what the table in the module says it sweeps."""
import numpy as np
import pytest

import schwarz_families as F
from test_schwarz_plan import emul, run  # noqa: F401  (the fixture that builds the replay)

WAVES = (1, 3, 64, 100000)


@pytest.mark.parametrize("name", list(F.FAMILIES))
def test_family_plan(emul, name):  # noqa: F811
    fam = F.FAMILIES[name]
    A, Sp, Sj, Tp, Tx = fam.make("small")
    n, nsub = A.shape[0], len(Sp) - 1
    assert F.largest(Sp) == fam.form.largest and F.most_updates(n, Sj) == fam.form.updates[0], (name, F.largest(Sp), F.most_updates(n, Sj))
    x, b = F.start_vectors(n)
    stats = {}
    for sweep, (r0, r1, rs) in F.sweeps_of(fam, nsub):
        form = F.form_of(fam, sweep)
        assert len(range(r0, r1, rs)) == 0 or range(r0, r1, rs)[-1] + rs == r1              # the stride hits row_stop
        want = F.reference(A, Sp, Sj, Tp, Tx, x, b, (r0, r1, rs)) if form.runs != "declined" else None
        for waves in WAVES:
            rc, got, st = run(emul, A, Sp, Sj, Tp, Tx, x, b, r0, r1, rs, waves)
            stats[sweep] = st
            if form.runs == "declined":
                assert rc == 2 and st["declined"] == form.declined, (name, sweep, waves, rc, st)
                continue
            assert rc == 0 and st["declined"] == 0, (name, sweep, waves, rc, st)
            assert np.array_equal(got, want), (name, sweep, waves)
            assert st["visited"] == len(range(r0, r1, rs))
            if form.runs == "versioned":
                assert st["levels"] >= 2, (name, sweep, st)
            elif form.runs in ("one_level", "rejected"):
                assert st["levels"] == 1, (name, sweep, st)
            else:
                assert st["visited"] == 0 and np.array_equal(got, x)
        idle = np.setdiff1d(np.arange(n), F.visited_rows(Sp, Sj, (r0, r1, rs)))
        if want is not None:
            assert np.array_equal(want[idle], x[idle])
        print(f"[schwarz plan] {name} {sweep}: levels {st['levels']} / widest {st['widest']} / slots {st['slots']}")
    # what the families claim about themselves
    fwd = (0, nsub, 1)
    if name == "size_edges":
        sizes, lv = np.diff(Sp), np.array(F.levels_of(A, Sp, Sj, fwd))
        assert set(F.EDGE_SIZES) <= set(sizes.tolist())
        assert any((sizes[lv == L] <= F.SW_PRE).any() and (sizes[lv == L] > F.SW_LANES).any() for L in set(lv.tolist()))   # small and large share levels
    if name == "all_big":
        assert np.diff(Sp).min() == 65 and all(s["levels"] >= 20 for k, s in stats.items() if k != "strided"), stats
    if name == "chain":
        assert all(s["levels"] == s["visited"] and s["widest"] == 1 for s in stats.values()), stats
    if name == "regrow":
        assert stats["strided"]["slots"] > max(stats["forward_small"]["slots"], stats["backward_small"]["slots"])
    if name == "nonsym_pattern":
        assert np.setdiff1d(F.nonsym_unused(n), Sj).size == F.nonsym_unused(n).size > 0
    if name == "long_rows":
        assert set(F.ROW_LENGTHS) == set(np.diff(A.indptr).tolist())
    if name == "dup_row":
        assert all(F.has_duplicate(Sp, Sj, s) for _, s in F.sweeps_of(fam, nsub))
    if name.startswith("hub"):
        assert int(np.bincount(Sj).argmax()) == F.HUB
