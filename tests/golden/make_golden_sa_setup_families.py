#!/usr/bin/env python3
"""Generate tests/golden/kernels_sa_setup_families.npz: what the reference returns on the families of
tests/sa_setup_families.py.  Outputs only -- the inputs are regenerated from the seeds there.

Run in the build container (needs the reference built into oracle/_ref by oracle/build_ref.py):
    python tests/golden/make_golden_sa_setup_families.py

Keys:
  agg.<family>.x / .y                          amg_core.standard_aggregation (y cut to the count)
  aggop.shapes / .dtypes / .sizes / .sha256    aggregate.standard_aggregation, one row per family of names.agg: AggOp's shape, and for
                                               (AggOp.indptr, AggOp.indices, AggOp.data, Cpts) dtype, size and SHA-256 of the bytes.
                                               These arrays repeat x and y (asserted here: they are aggregate.py:76-96 applied to
                                               them), and in full they alone would be as large as the whole file may be
  refuse.<graph>.x / .y / .opened              amg_core.standard_aggregation on the four graphs the device refuses; opened = the
                                               aggregates its third pass opened (by the restatement)
  fit.<aggregation>.<case>                     tentative.fit_candidates on sa_setup_families.recorded_fit_cases(): Q.data then R, ravelled
  soc.<operator>.indptr / .indices / .data     strength.symmetric_strength_of_connection for every theta of THETAS: the row pointers
                                               stacked, indices and data concatenated in that order
  names.agg / names.fit / names.soc            what is recorded

The reference must refuse nothing the families hold (asserted: every call returns).  One exception is its binding, not its
algorithm: amg_core takes int32 index arrays only and raises TypeError on int64 ones.  The int64 family is therefore run on
the int32 copies of its arrays (x, y, and AggOp checked as for every family), and what is recorded for it is aggregate.py:64-96
with index_type = int64 applied to that x, y (sa_setup_families.aggop_from: the same SciPy calls).
"""
import sys
from pathlib import Path

import numpy as np
import scipy.sparse as sp

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

import oracle.refimport  # noqa: E402,F401
from pyamg import amg_core as ref_core  # noqa: E402
from pyamg.aggregation.aggregate import standard_aggregation as ref_aggregation  # noqa: E402
from pyamg.aggregation.tentative import fit_candidates as ref_fit  # noqa: E402
from pyamg.strength import symmetric_strength_of_connection as ref_strength  # noqa: E402
import sa_setup_families as fam  # noqa: E402

OUT = HERE / "kernels_sa_setup_families.npz"
LIMIT = (HERE / "kernels_energy.npz").stat().st_size


def core_aggregation(Ap, Aj):
    n = Ap.size - 1
    x, y = np.full(n, -7, dtype=np.int32), np.full(max(n, 1), -7, dtype=np.int32)
    cnt = ref_core.standard_aggregation(n, Ap.astype(np.int32), Aj.astype(np.int32), x, y)
    return x, y[:cnt], cnt


def main():
    out = {}
    shapes, dtypes, sizes, digests = [], [], [], []
    for name in fam.FAMILIES + fam.HUBS:
        Ap, Aj = fam.graph(name)
        n = Ap.size - 1
        x, y, cnt = core_aggregation(Ap, Aj)
        sx, sy, scnt, opened = fam.serial_aggregation(Ap, Aj)
        assert cnt == scnt and opened == 0 and np.array_equal(x, sx) and np.array_equal(y, sy), name
        out[f"agg.{name}.x"], out[f"agg.{name}.y"] = x, y
        C = sp.csr_array((np.ones(Aj.size), Aj.astype(np.int32), Ap.astype(np.int32)), shape=(n, n))
        AggOp, Cpts = ref_aggregation(C)
        assert AggOp.format == "csr"
        arrays = (AggOp.indptr, AggOp.indices, AggOp.data, Cpts)
        want = fam.aggop_from(x, cnt, np.int32)              # AggOp repeats x and y: what is kept is dtype, size and digest
        assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(arrays[:3], want[:3])) and AggOp.shape == want[3], name
        assert np.array_equal(Cpts, y) and Cpts.dtype == np.int32
        if Ap.dtype == np.int64:                             # aggregate.py:64-96 with index_type = int64, on the x, y just checked
            arrays = fam.aggop_from(x, cnt, np.int64)[:3] + (y.astype(np.int64),)
        shapes.append(AggOp.shape)
        dtypes.append([str(a.dtype) for a in arrays])
        sizes.append([a.size for a in arrays])
        digests.append([fam.digest(a) for a in arrays])
    out["aggop.shapes"], out["aggop.dtypes"], out["aggop.sizes"] = np.array(shapes, dtype=np.int64), np.array(dtypes), np.array(sizes, dtype=np.int64)
    out["aggop.sha256"] = np.array(digests, dtype=np.uint8)
    for name in fam.REFUSALS:
        Ap, Aj = fam.graph(name)
        x, y, cnt = core_aggregation(Ap, Aj)
        sx, sy, scnt, opened = fam.serial_aggregation(Ap, Aj)
        assert cnt == scnt and np.array_equal(x, sx) and np.array_equal(y, sy), name
        out[f"refuse.{name}.x"], out[f"refuse.{name}.y"], out[f"refuse.{name}.opened"] = x, y, np.array(opened)
    fit_names = []
    for agg, case in fam.recorded_fit_cases():
        T = fam.aggop(agg)
        AggOp = sp.csr_array((T.data.copy(), T.indices.copy(), T.indptr.copy()), shape=T.shape)
        Q, R = ref_fit(AggOp, np.array(fam.candidates(agg, case)), tol=case[4])
        assert Q.format == "bsr" and np.array_equal(Q.indptr, T.indptr) and np.array_equal(Q.indices, T.indices), (agg, case)
        assert np.isfinite(Q.data).all() and np.isfinite(R).all(), (agg, case)
        assert Q.data.dtype == R.dtype == fam.candidates(agg, case).dtype
        out[f"fit.{agg}.{fam.case_id(case)}"] = np.concatenate([np.ravel(Q.data), np.ravel(R)])
        fit_names.append(f"{agg}.{fam.case_id(case)}")
    soc_names = []
    for name in fam.OPERATORS:
        A = fam.operator(name)
        got = [ref_strength(sp.csr_array((A.data.copy(), A.indices.copy(), A.indptr.copy()), shape=A.shape), theta) for theta in fam.THETAS]
        assert all(np.isfinite(S.data).all() and S.indptr.dtype == S.indices.dtype == np.int32 for S in got), name
        out[f"soc.{name}.indptr"] = np.stack([S.indptr for S in got])
        out[f"soc.{name}.indices"] = np.concatenate([S.indices for S in got])
        out[f"soc.{name}.data"] = np.concatenate([S.data for S in got])
        soc_names += [f"{name}.{theta:g}" for theta in fam.THETAS]
    out["names.agg"] = np.array(fam.FAMILIES + fam.HUBS)
    out["names.fit"] = np.array(fit_names)
    out["names.soc"] = np.array(soc_names)
    np.savez_compressed(OUT, **out)
    size = OUT.stat().st_size
    print(f"{OUT.name} written: {len(out)} arrays, {size} bytes (limit {LIMIT})")
    assert size <= LIMIT, (size, LIMIT)


if __name__ == "__main__":
    main()
