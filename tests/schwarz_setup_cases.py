"""Cases and yardsticks shared by the host and the GPU tests of the Schwarz setup (test_schwarz_setup_host.py, test_gpu_schwarz_setup.py):
operators, subdomains and the reference's blocks from the committed fixtures, and the per-block comparison against them."""
from pathlib import Path

import numpy as np
import scipy.sparse as sp

from pyamg_amd.relaxation import _rank_tol, _subdomain_blocks

GOLDEN = Path(__file__).resolve().parent / "golden"
KERNEL_OPS = ("irr_float64", "irr_float32", "pois_float64", "pois_float32", "pois_big")
SETUP_INVERTED = ("chain_float64", "chain_float32", "chainp_float64", "chainp_float32", "part")
CHAINS = (1, 2, 8, 9, 16, 17, 32, 33, 64)
BOUND = 64.0          # |X - X_ref|_F <= BOUND * eps(dtype) * kappa_+(B) * |X_ref|_F


class Case:
    def __init__(self, name, A, sub, sptr, blocks, inv):
        self.name, self.A, self.sub, self.sptr, self.inv = name, A, np.ascontiguousarray(sub, dtype=np.int32), np.ascontiguousarray(sptr, dtype=np.int32), inv
        m = np.diff(self.sptr).astype(np.int64)
        self.tptr = np.zeros(self.sptr.size, dtype=np.int32)
        self.tptr[1:] = np.cumsum(m * m)
        # the blocks before inversion: the reference's own where the fixture recorded them; the older fixtures hold operators without
        # duplicate entries, where the host restatement of extract_subblocks is the reference's result
        self.blocks = blocks if blocks is not None else _subdomain_blocks(A, self.sub, self.sptr)[0]

    @property
    def dtype(self):
        return np.dtype(self.A.dtype)


_cache = {}


def _csr(z, k):
    ip, ix, dx = z[f"{k}.indptr"], z[f"{k}.indices"], z[f"{k}.data"]
    return sp.csr_array((dx, ix, ip), shape=(len(ip) - 1, len(ip) - 1))


def cases():
    """name -> Case, built once"""
    if _cache:
        return _cache
    z = np.load(GOLDEN / "kernels_schwarz.npz")
    for k in KERNEL_OPS:
        _cache[k] = Case(k, _csr(z, k), z[f"{k}.sub"], z[f"{k}.sptr"], None, z[f"{k}.inv"])
    z = np.load(GOLDEN / "kernels_schwarz_setup.npz")
    for k in SETUP_INVERTED + ("dup",):
        c = Case(k, _csr(z, k), z[f"{k}.sub"], z[f"{k}.sptr"], z[f"{k}.blocks"], z[f"{k}.inv"] if f"{k}.inv" in z.files else None)
        assert np.array_equal(c.tptr, z[f"{k}.tptr"])
        _cache[k] = c
    from pyamg_amd.hierarchy import load_spec
    for h in ("sa2d_schwarz", "sa2d_sbschwarz"):
        spec, _ = load_spec(GOLDEN / f"hier_{h}.npz")
        for i, L in enumerate(spec.levels[:-1]):
            s = L.pre
            if s is None or s.kind != "schwarz":
                continue
            A = (s.Ar if s.Ar is not None else L.A).to_scipy()
            _cache[f"{h}.L{i}"] = Case(f"{h}.L{i}", A, s.subdomain, s.subdomain_ptr, None, s.inv_subblock)
    return _cache


ALL = KERNEL_OPS + SETUP_INVERTED + ("dup", "sa2d_schwarz.L0", "sa2d_schwarz.L1", "sa2d_sbschwarz.L0", "sa2d_sbschwarz.L1")
INVERTED = tuple(n for n in ALL if n != "dup")


def rank_of_pinv(X, smax_B):
    """rank of a computed pseudo-inverse: its singular values are 1 / sigma_j >= 1 / sigma_max(B) for the kept j and rounding noise
    (eps |X|) for the dropped ones"""
    if X.size == 0 or smax_B == 0:
        return 0
    s = np.linalg.svd(X.astype(np.float64), compute_uv=False)
    return int(np.sum(s > 0.5 / smax_B))


def compare_blocks(case, Tx):
    """every block of Tx against the reference's: (worst err / (eps kappa_+ |X_ref|), blocks with a truncated singular value); asserts
    that the ranks agree.  kappa_+ = largest / smallest kept singular value of the block, numpy.linalg.svd in float64."""
    eps, tol = float(np.finfo(case.dtype).eps), _rank_tol(case.dtype)
    worst, truncated = 0.0, 0
    for d, m in enumerate(np.diff(case.sptr)):
        a, b = case.tptr[d], case.tptr[d + 1]
        B = case.blocks[a:b].reshape(m, m).astype(np.float64)
        X, Xr = Tx[a:b].reshape(m, m).astype(np.float64), case.inv[a:b].reshape(m, m).astype(np.float64)
        s = np.linalg.svd(B, compute_uv=False) if m else np.zeros(0)
        keep = s > tol * (s[0] if m else 0.0)
        rank = int(keep.sum())
        # the reference's decision must not be on a knife edge, or "the same rank" is not a property of the algorithm
        assert m == 0 or s[0] == 0 or not np.any((s > 0.2 * tol * s[0]) & (s < 5 * tol * s[0])), (case.name, d, s / s[0], tol)
        truncated += rank < m
        smax = s[0] if m else 0.0
        assert rank_of_pinv(Xr, smax) == rank and rank_of_pinv(X, smax) == rank, (case.name, d, m, rank, rank_of_pinv(X, smax), rank_of_pinv(Xr, smax))
        if rank == 0:
            assert not X.any(), (case.name, d)
            continue
        kappa = s[0] / s[keep][-1]
        err = np.linalg.norm(X - Xr) / (eps * kappa * np.linalg.norm(Xr))
        worst = max(worst, err)
    return worst, truncated
