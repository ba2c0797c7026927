#!/usr/bin/env python3
"""Fused symmetric Gauss-Seidel sweeps on level 1 of the 256^3 SA hierarchy, nothing else: the command to run under rocprofv3 --pmc (kernel trace
only) with a tune dict as JSON, e.g. '{"lanem_cluster": 1}' (profiles/r08_pmc_lanem_cluster_level1.json); "x_zero": 1 in the dict announces x = 0 to every
sweep, as a cycle's pre-smoothing does (with "zero_plans": 2 the launches run the zero-iterate plans: profiles/r09_pmc_zero_plan_level1.json).  Not product code."""
import sys, json
from pathlib import Path
import numpy as np
import scipy.sparse as sp
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: F401
from pyamg_amd import _capi as capi
from pyamg_amd.hierarchy import sparse_op
from pyamg_amd.multilevel import DeviceMatrix

tune = json.loads(sys.argv[1]) if len(sys.argv) > 1 else {}
x_zero = bool(tune.pop("x_zero", 0))
cache = Path("/tmp/pamg_level1_256.npz")
if not cache.exists():
    import oracle.refimport  # noqa
    import pyamg
    from pyamg_amd import aggregation
    A = pyamg.gallery.poisson((256, 256, 256), format="csr")
    np.random.seed(1)
    with aggregation.device_setup(pyamg):
        ml = pyamg.smoothed_aggregation_solver(A, max_coarse=10, max_levels=3)
    M = ml.levels[1].A.tocsr()
    np.savez(cache, data=M.data, indices=M.indices, indptr=M.indptr)
    if tune.get("cache_only"):
        sys.exit(0)
z = np.load(cache)
A = sp.csr_array((z["data"], z["indices"], z["indptr"]))
n = A.shape[0]
dA = DeviceMatrix(sparse_op(A))
dA.tune(gs_order=1, **tune)
rng = np.random.RandomState(1)
dx, db = capi.DeviceArray.from_host(rng.rand(n)), capi.DeviceArray.from_host(rng.rand(n))
for _ in range(6):
    dA.gauss_seidel_x0(dx, db, sweep="symmetric", iterations=1, x_is_zero=x_zero)
capi.sync()
print("level 1", n, A.nnz, dA.lanem_info(4 if dA.sym_info()["zero_plan_launches"] else 0), dA.sym_info(), flush=True)
dA.free()
