#!/usr/bin/env python3
"""Generate tests/golden/kernels_schwarz_families.npz: the reference's own results on the subdomain families of tests/schwarz_families.py (large
size, float64).  Only results are stored; the inputs are the families themselves (seeded; their inverted blocks are rounded to multiples of 2^-24,
so they do not depend on the machine's LAPACK).

Run in the build container (needs the reference built into oracle/_ref by oracle/build_ref.py):
    python tests/golden/make_golden_schwarz_families.py

Keys:
  <family>.forward        x after one forward sweep of the reference's amg_core.overlapping_schwarz_csr from schwarz_families.start_vectors
                          (every family but too_big, which the device path refuses)
  size_edges.symmetric2   x after the reference's relaxation.schwarz(A, x, b, iterations=2, subdomain=, subdomain_ptr=, sweep="symmetric"),
                          which inverts the blocks itself (the subdomains of no rows left out: schwarz_families.without_empty)
"""
import sys
from pathlib import Path

import numpy as np
import scipy.sparse as sp

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent.parent), str(HERE.parent)]

import oracle.refimport  # noqa: E402,F401
from pyamg import amg_core  # noqa: E402
from pyamg.relaxation import relaxation as rr  # noqa: E402

import schwarz_families as F  # noqa: E402


def main():
    out = {}
    for name, fam in F.FAMILIES.items():
        if fam.form.runs == "rejected":
            continue
        A, Sp, Sj, Tp, Tx = fam.make("large")
        n, nsub = A.shape[0], len(Sp) - 1
        x, b = F.start_vectors(n)
        amg_core.overlapping_schwarz_csr(A.indptr, A.indices, A.data, x, b, Tx, Tp, Sj, Sp, nsub, n, 0, nsub, 1)
        assert np.isfinite(x).all(), name
        assert F.same_bits(x, F.reference(A, Sp, Sj, Tp, Tx, F.start_vectors(n)[0], b, (0, nsub, 1))), name       # the oracle restates it
        out[f"{name}.forward"] = x
    A, Sp, Sj, _, _ = F.FAMILIES["size_edges"].make("large")
    x, b = F.start_vectors(A.shape[0])
    rr.schwarz(sp.csr_array(A.copy()), x, b, iterations=2, subdomain=Sj.copy(), subdomain_ptr=F.without_empty(Sp), sweep="symmetric")
    assert np.isfinite(x).all()
    out["size_edges.symmetric2"] = x
    np.savez_compressed(HERE / "kernels_schwarz_families.npz", **out)
    size = (HERE / "kernels_schwarz_families.npz").stat().st_size
    print("kernels_schwarz_families.npz written:", len(out), "arrays,", size, "bytes")


if __name__ == "__main__":
    main()
