#!/usr/bin/env python3
"""Generate tests/golden/kernels_block_air.npz: inputs and the reference's own outputs for the BLOCK (BSR) setup of approximate ideal
restriction AMG -- ``classical_strength_of_connection(block=True)``, ``one_point_interpolation`` and ``local_air`` on BSR operators.

Run in the build container (needs the reference built into oracle/_ref by oracle/build_ref.py):
    python tests/golden/make_golden_block_air.py

The file holds a few hundred small arrays; stored one by one, the zip bookkeeping would outweigh them, so they are packed: ``f64`` and
``i32`` are two pools, ``keys`` names the arrays and ``index`` holds (pool, offset, length) of each; the tables are string arrays of
their own.  tests/block_air_cases.py unpacks them.  Keys (BSR triples are ``<prefix>.indptr / .indices / .data`` with the blocks
flattened, CSR triples the same):

  ops (table: name, block size) / blk.<op>.A / blk.<op>.splitting   the operators (at most 300 block rows)
      ck<b>       kron-like: the upwind convection-diffusion stencil of the benchmark's AIR workload on a small grid, every stored entry
                  a_ij replaced by the dense block a_ij * (I or I / 2 plus a perturbation), b = 1, 2, 3, 4, 5, 8
      ck3u        ck3 with the blocks of every row stored in a shuffled order (unsorted block rows)
      ck3t        ck3 with one off-diagonal block scaled to entries of 1e-17: its measure falls under 1e-16 for every norm
      hub<b>x<N>  node 0 (C) with the F-neighbours 1 .. N chained to each other, an isolated C-point (an empty neighbourhood: its row is
                  the identity block only) and a C-point behind the last F-point: the orders n = N * b on both sides of every lane-group
                  boundary -- 8, 9, 16, 17, 32, 33, 64 and 65 (host) -- and a neighbourhood of 70 block columns (above the staging cap)
      diag3       diagonal blocks (the b scalar problems decouple: solution entries are exactly zero or negligible INSIDE kept blocks) and
                  an F-point with a stored zero diagonal block and nothing inside the neighbourhood (its solution block is zero as a whole
                  and eliminate_zeros removes it)
  strength (table: case, operator, norm, theta)   block strength: str.<case>.measure (one value per stored block, after the 1e-16 rule) and
                  the finished strength matrix str.<case>.S; norms 'abs', 'min', 'fro' with theta 0, 0.1 and 1
  air (table: case, operator, norm, theta, degree)   local_air with the operator's splitting:
      blk.<case>.Rraw      R as block_approx_ideal_restriction_pass2 leaves it (indptr = the row pointer of pass 1; the identity block last
                           in every row, solution blocks that are zero still stored)
      blk.<case>.R.keep    what local_air returns are the blocks of Rraw with keep == 1, in place (asserted here against the reference)
  onept (table: case, strength case)   one_point_interpolation(A, C = the strength matrix of that strength case) with the operator's
                  splitting: onept.<case>.P.indptr / .indices cut to indptr[-1] entries; the data are identity blocks
  e2e.A0 / .seed / .sizes   air_solver(A, CF='PMIS', max_coarse=10) of ck2 on a larger grid: e2e.A<l> (l = 0, 1, 2), e2e.R<l> (l = 0, 1) as BSR,
                  e2e.P<l>.indptr / .indices
"""
import sys
from pathlib import Path

import numpy as np
import scipy.sparse as sp

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

import oracle.refimport  # noqa: E402,F401
import pyamg  # noqa: E402
from pyamg import amg_core as ref_core  # noqa: E402
from pyamg.classical import interpolate as ri  # noqa: E402
from pyamg.classical import split as rs  # noqa: E402
from pyamg.strength import classical_strength_of_connection as ref_strength  # noqa: E402

SEED = 20270203
OUT = HERE / "kernels_block_air.npz"
LIMIT = (HERE / "kernels_air.npz").stat().st_size


def put_bsr(out, prefix, M):
    out[prefix + ".indptr"] = np.asarray(M.indptr, dtype=np.int32)
    out[prefix + ".indices"] = np.asarray(M.indices, dtype=np.int32)[:M.indptr[-1]]
    out[prefix + ".data"] = np.asarray(M.data, dtype=np.float64)[:M.indptr[-1]].reshape(-1)


def put_csr(out, prefix, M):
    M = sp.csr_array(M)
    out[prefix + ".indptr"] = np.asarray(M.indptr, dtype=np.int32)
    out[prefix + ".indices"] = np.asarray(M.indices, dtype=np.int32)
    out[prefix + ".data"] = np.asarray(M.data, dtype=np.float64)


def convdiff(mx, my, c=3.0):
    """the scalar upwind convection-diffusion operator (non-symmetric)"""
    Dx = sp.diags_array([np.ones(mx), -np.ones(mx - 1)], offsets=[0, -1], shape=(mx, mx))
    Dy = sp.diags_array([2 * np.ones(my), -np.ones(my - 1), -np.ones(my - 1)], offsets=[0, -1, 1], shape=(my, my))
    A = sp.csr_array(c * sp.kron(sp.eye_array(my), Dx) + sp.kron(Dy, sp.eye_array(mx)))
    A.sort_indices()
    return A


def block_of(rng, a, b, diagonal, only_diagonal=False):
    """a * (I or I / 2 plus a perturbation in multiples of 1/32): few mantissa bits, so the operators compress"""
    pert = rng.randint(0, 3, size=(b, b)) / 32.0
    if only_diagonal:
        pert = np.diag(np.diag(pert))
    return a * (np.eye(b) * (1.0 if diagonal else 0.5) + pert)


def blocked(A0, b, seed, only_diagonal=False):
    """every stored a_ij of the scalar CSR pattern A0 as a dense b x b block"""
    rng = np.random.RandomState(seed)
    A0 = sp.csr_array(A0)
    rows = np.repeat(np.arange(A0.shape[0]), np.diff(A0.indptr))
    data = np.array([block_of(rng, a, b, i == j, only_diagonal) for i, j, a in zip(rows, A0.indices, A0.data)]).reshape(-1, b, b)
    n = A0.shape[0]
    return sp.bsr_array((data, A0.indices.astype(np.int32), A0.indptr.astype(np.int32)), blocksize=(b, b), shape=(n * b, n * b))


def shuffled_rows(A, seed):
    rng = np.random.RandomState(seed)
    indices, data = A.indices.copy(), A.data.copy()
    for i in range(A.indptr.size - 1):
        lo, hi = A.indptr[i], A.indptr[i + 1]
        perm = lo + rng.permutation(hi - lo)
        indices[lo:hi], data[lo:hi] = A.indices[perm], A.data[perm]
    return sp.bsr_array((data, indices, A.indptr.copy()), blocksize=A.blocksize, shape=A.shape)


def unsorted(A):
    return any(np.any(np.diff(A.indices[a:b]) < 0) for a, b in zip(A.indptr[:-1], A.indptr[1:]))


def hub_pattern(N):
    """scalar pattern and splitting: 0 = the hub (C), 1 .. N its F-neighbours in a chain, N + 1 an isolated C-point, N + 2 a C-point
    behind the last F-point"""
    n = N + 3
    r_, c_, v_ = [], [], []

    def link(i, j, v):
        r_.append(i); c_.append(j); v_.append(v)
    for j in range(1, N + 1):
        link(0, j, -1.0 - (j % 4) / 4.0); link(j, 0, -1.0 - (j % 3) / 2.0)
        if j < N:
            link(j, j + 1, -0.5 - (j % 2) / 4.0); link(j + 1, j, -0.75)
    link(N, N + 2, -1.0); link(N + 2, N, -1.5)
    for i in range(n):
        link(i, i, 6.0 + (i % 3))
    A0 = sp.csr_array(sp.coo_array((v_, (r_, c_)), shape=(n, n)))
    A0.sort_indices()
    splitting = np.zeros(n, dtype=np.int32)
    splitting[[0, N + 1, N + 2]] = 1
    return A0, splitting


def diag3():
    """b = 3, diagonal blocks; node 3 is an F-point with a stored zero diagonal block and no block inside the neighbourhood of node 0"""
    rng = np.random.RandomState(SEED + 7)
    b = 3
    pat = [[(0, 6.0), (1, -1.0), (2, -2.0), (3, -1.5)],                      # C
           [(1, 5.0), (0, -1.0), (2, -1.0)],                                  # F
           [(2, 7.0), (1, -2.0), (0, -1.0), (5, -1.0)],                       # F
           [(3, 0.0), (0, -1.0), (4, -1.0)],                                  # F: zero diagonal block, C-neighbours only
           [(4, 5.0), (5, -1.0)],                                             # C
           [(5, 6.0), (4, -2.0), (2, -1.0)]]                                  # F
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in pat])]).astype(np.int32)
    indices = np.array([c for r in pat for c, _ in r], dtype=np.int32)
    data = np.array([block_of(rng, a, b, i == c, only_diagonal=True) for i, r in enumerate(pat) for c, a in r])
    A = sp.bsr_array((data, indices, indptr), blocksize=(b, b), shape=(6 * b, 6 * b))
    return A, np.array([1, 0, 0, 0, 1, 0], dtype=np.int32)


def air_case(out, stats, name, op, A, splitting, theta, norm, degree):
    """the steps of interpolate.py:324-426 one by one, so that R is seen before eliminate_zeros"""
    b = A.blocksize[0]
    n = A.shape[0] // b
    splitting = np.asarray(splitting, dtype=np.int32)
    assert n <= 300 and A.indptr.dtype == np.int32 and A.blocksize[0] == A.blocksize[1]
    C = ref_strength(A=A, theta=theta, block=True, norm=norm)
    Cpts = np.array(np.where(splitting == 1)[0], dtype=A.indptr.dtype)
    nc = Cpts.shape[0]
    Rp = np.empty(nc + 1, dtype=A.indptr.dtype)
    ref_core.approx_ideal_restriction_pass1(Rp, C.indptr, C.indices, Cpts, splitting, degree)
    nnz = Rp[-1]
    Rj = np.zeros(nnz, dtype=A.indptr.dtype)
    Rx = np.zeros(nnz * b * b, dtype=A.dtype)
    ref_core.block_approx_ideal_restriction_pass2(Rp, Rj, Rx, A.indptr, A.indices, A.data.ravel(), C.indptr, C.indices, C.data, Cpts, splitting, b,
                                                  degree, False, 10, True)
    assert np.all(np.isfinite(Rx)), name
    R = ri.local_air(A.copy(), splitting.copy(), theta=theta, norm=norm, degree=degree)
    assert R.format == "bsr" and tuple(R.blocksize) == (b, b) and R.shape == (nc * b, n * b)
    blocks = Rx.reshape(nnz, b, b)
    keep = np.any(blocks != 0.0, axis=(1, 2))
    rowof = np.repeat(np.arange(nc), np.diff(Rp))
    assert np.array_equal(R.indptr, np.concatenate([[0], np.cumsum(np.bincount(rowof[keep], minlength=nc))]))
    nk = R.indptr[-1]
    assert np.array_equal(R.indices[:nk], Rj[keep]) and np.array_equal(R.data[:nk], blocks[keep])
    Aabsent = np.zeros((n, n), dtype=bool)                   # the stored block pattern of A
    for i in range(n):
        Aabsent[i, A.indices[A.indptr[i]:A.indptr[i + 1]]] = True
    Aabsent = ~Aabsent
    st = stats.setdefault(name, {"n": [], "rhs_absent": 0, "sys_absent": 0, "zero_inside": 0})
    for r in range(nc):                                      # ascending and unique, the identity block last
        row = Rj[Rp[r]:Rp[r + 1]]
        assert row[-1] == Cpts[r] and np.array_equal(blocks[Rp[r + 1] - 1], np.eye(b)) and np.all(np.diff(row[:-1]) > 0)
        Nf = row[:-1]
        st["n"].append(len(Nf) * b)
        st["rhs_absent"] += int(np.sum(Aabsent[Cpts[r], Nf]))
        st["sys_absent"] += int(np.sum(Aabsent[np.ix_(Nf, Nf)]))
    st["zero_inside"] += int(np.sum(np.any(blocks[keep] == 0.0, axis=(1, 2))))
    st["removed"] = int(nnz - nk)
    st["b"] = b
    st["row"] = (name, op, norm, repr(float(theta)), str(int(degree)))
    out[f"blk.{name}.Rraw.indptr"] = np.asarray(Rp, dtype=np.int32)
    out[f"blk.{name}.Rraw.indices"] = np.asarray(Rj, dtype=np.int32)
    out[f"blk.{name}.Rraw.data"] = Rx.copy()
    out[f"blk.{name}.R.keep"] = keep


def plain_fro(blocks):
    """down the rows of every column first, then across the columns, left to right"""
    res = np.zeros(blocks.shape[0])
    b = blocks.shape[1]
    for c in range(b):
        s = np.zeros(blocks.shape[0])
        for r in range(b):
            s = s + blocks[:, r, c] * blocks[:, r, c]
        res = res + s
    return res


def strength_case(out, name, op, A, theta, norm):
    b = A.blocksize[0]
    S = ref_strength(A=A.copy(), theta=theta, block=True, norm=norm)
    if norm == "abs":
        m = np.max(np.max(np.abs(A.data), axis=1), axis=1)
    elif norm == "min":
        m = np.min(np.min(A.data, axis=1), axis=1)
    else:
        m = np.conjugate(A.data) * A.data
        m = np.sum(np.sum(m, axis=1), axis=1)
        assert b >= 8 or np.array_equal(m, plain_fro(A.data)), name              # NumPy's order is the plain one up to b = 7
    m = m.copy()
    m[np.abs(m) < 1e-16] = 0.0
    assert np.all(np.isfinite(m)) and np.all(np.isfinite(S.data))
    out[f"str.{name}.measure"] = m
    put_csr(out, f"str.{name}.S", S)
    return m, S


def main():
    out, stats, ops = {}, {}, {}
    # ---------------------------------------------------------------- operators
    grids = {1: (9, 7), 2: (9, 7), 3: (6, 5), 4: (6, 5), 5: (5, 4), 8: (4, 3)}
    for b, (mx, my) in grids.items():
        ops[f"ck{b}"] = blocked(convdiff(mx, my), b, SEED + b)
    ops["ck3u"] = shuffled_rows(ops["ck3"], SEED + 30)
    assert unsorted(ops["ck3u"]) and not unsorted(ops["ck3"])
    T = ops["ck3"].copy()
    p = T.indptr[7] + int(np.where(T.indices[T.indptr[7]:T.indptr[8]] != 7)[0][0])     # an off-diagonal block of block row 7
    T.data[p] = -1e-17 * (1.0 + np.arange(9).reshape(3, 3))
    ops["ck3t"] = T
    hubs = [(8, 1), (8, 2), (8, 8), (4, 8), (2, 32), (3, 3), (3, 11), (5, 13), (1, 16), (1, 17), (1, 70), (2, 4)]
    split_hub = {}
    for b, N in hubs:
        A0, split_hub[(b, N)] = hub_pattern(N)
        ops[f"hub{b}x{N}"] = blocked(A0, b, SEED + 100 * b + N)
    ops["diag3"], split_diag = diag3()
    # ---------------------------------------------------------------- block strength
    str_table = []
    tiny = 0
    for op in ("ck3t", "ck5"):
        for norm in ("abs", "min", "fro"):
            for k, theta in enumerate((0.0, 0.1, 1.0)):
                name = f"{op}.{norm}.t{k}"
                m, S = strength_case(out, name, op, ops[op], theta, norm)
                str_table.append((name, op, norm, repr(theta)))
                if op == "ck3t":
                    assert m[p] == 0.0 and np.any(ops[op].data[p] != 0.0)        # the measure under 1e-16
                    tiny += 1
    assert tiny == 9
    for op, norm in (("ck1", "fro"), ("ck2", "abs"), ("ck2", "min"), ("ck2", "fro"), ("ck4", "fro"), ("ck8", "abs"), ("ck8", "min"), ("ck3u", "min"),
                     ("diag3", "abs")):
        name = f"{op}.{norm}.t1"
        strength_case(out, name, op, ops[op], 0.1, norm)
        str_table.append((name, op, norm, repr(0.1)))
    # ---------------------------------------------------------------- local_air
    splits = {}
    for op in ("ck1", "ck2", "ck3", "ck4", "ck5", "ck8"):
        splits[op] = np.asarray(rs.RS(ref_strength(ops[op], theta=0.3, norm="min"), second_pass=True), dtype=np.int32)
    splits["ck3u"] = splits["ck3t"] = splits["ck3"]
    for op, degree, theta, norm in (("ck1", 2, 0.05, "abs"), ("ck2", 1, 0.05, "abs"), ("ck2", 2, 0.3, "min"), ("ck3u", 2, 0.05, "fro"),
                                    ("ck3t", 1, 0.1, "abs"), ("ck4", 1, 0.1, "fro"), ("ck5", 2, 0.05, "abs"), ("ck8", 1, 0.05, "min")):
        air_case(out, stats, f"{op}.d{degree}", op, ops[op], splits[op], theta, norm, degree)
    for b, N in hubs:
        op = f"hub{b}x{N}"
        air_case(out, stats, f"{op}.d1", op, ops[op], split_hub[(b, N)], 0.0, "abs", 1)
    air_case(out, stats, "hub3x3.d2", "hub3x3", ops["hub3x3"], split_hub[(3, 3)], 0.0, "abs", 2)
    air_case(out, stats, "diag3.d1", "diag3", ops["diag3"], split_diag, 0.0, "abs", 1)
    splits.update({f"hub{b}x{N}": v for (b, N), v in split_hub.items()})
    splits["diag3"] = split_diag
    # what the cases cover
    allb = {st["b"] for st in stats.values()}
    assert allb >= {1, 2, 3, 4, 5, 8}, allb
    alln = np.concatenate([st["n"] for st in stats.values()])
    for lo, hi in ((0, 0), (1, 8), (9, 16), (17, 32), (33, 64), (65, 10 ** 6)):
        assert np.any((alln >= lo) & (alln <= hi)), (lo, hi)
    for edge in (8, 9, 16, 17, 32, 33, 64, 65):
        assert edge in alln, edge
    assert stats["hub1x70.d1"]["n"][0] == 70                                   # a neighbourhood above the staging cap of 64 block columns
    d1 = [k for k in stats if k.endswith(".d1")]
    d2 = [k for k in stats if k.endswith(".d2")]
    assert d1 and d2 and any(stats[k]["rhs_absent"] > 0 for k in d2) and any(stats[k]["sys_absent"] > 0 for k in stats)
    assert unsorted(ops["ck3u"]) and "ck3u.d2" in stats
    assert stats["diag3.d1"]["zero_inside"] > 0 and stats["diag3.d1"]["removed"] >= 1
    del ops["ck3"]                                           # (ck3u and ck3t are its cases)
    for name, A in ops.items():
        put_bsr(out, f"blk.{name}.A", A)
        out[f"blk.{name}.splitting"] = splits[name]
    # ---------------------------------------------------------------- one_point_interpolation
    onept_table = []
    for case, strcase, splitting in (("ck2", "ck2.min.t1", splits["ck2"]), ("ck3u", "ck3u.min.t1", splits["ck3u"]), ("ck8", "ck8.abs.t1", splits["ck8"]),
                                     ("diag3", "diag3.abs.t1", split_diag)):
        op = dict((r[0], r[1]) for r in str_table)[strcase]
        assert np.array_equal(splitting, splits[op])
        A = ops[op]
        b = A.blocksize[0]
        C = sp.csr_array((out[f"str.{strcase}.S.data"], out[f"str.{strcase}.S.indices"], out[f"str.{strcase}.S.indptr"]),
                         shape=(A.shape[0] // b,) * 2)
        P = ri.one_point_interpolation(A.copy(), C.copy(), splitting.copy())
        nnz = P.indptr[-1]
        assert P.format == "bsr" and tuple(P.blocksize) == (b, b) and P.shape == (A.shape[0], b * splitting.sum())
        assert np.array_equal(P.data[:nnz], np.array(nnz * [np.identity(b)]))
        out[f"onept.{case}.P.indptr"] = np.asarray(P.indptr, dtype=np.int32)
        out[f"onept.{case}.P.indices"] = np.asarray(P.indices[:nnz], dtype=np.int32)
        onept_table.append((case, strcase))
    # ---------------------------------------------------------------- end to end
    A = blocked(convdiff(10, 8), 2, SEED + 50)
    seed = SEED + 51
    np.random.seed(seed)
    ml = pyamg.air_solver(A.copy(), CF="PMIS", max_coarse=10)
    assert len(ml.levels) >= 3 and all(lv.A.format == "bsr" and tuple(lv.A.blocksize) == (2, 2) for lv in ml.levels)
    out["e2e.seed"] = np.int64(seed)
    out["e2e.sizes"] = np.array([lv.A.shape[0] for lv in ml.levels], dtype=np.int64)
    for lvl in range(3):
        assert np.all(np.isfinite(ml.levels[lvl].A.data))
        put_bsr(out, f"e2e.A{lvl}", ml.levels[lvl].A)
    for lvl in range(2):
        P, R = ml.levels[lvl].P, ml.levels[lvl].R
        nnz = P.indptr[-1]
        assert P.format == "bsr" and R.format == "bsr" and np.array_equal(P.data[:nnz], np.array(nnz * [np.identity(2)]))
        out[f"e2e.P{lvl}.indptr"] = np.asarray(P.indptr, dtype=np.int32)
        out[f"e2e.P{lvl}.indices"] = np.asarray(P.indices[:nnz], dtype=np.int32)
        put_bsr(out, f"e2e.R{lvl}", R)
    rng = np.random.RandomState(3)
    res = []
    ml.solve(rng.rand(A.shape[0]), x0=rng.rand(A.shape[0]), tol=1e-10, maxiter=40, residuals=res)
    assert res[-1] < 1e-8 * res[0], res                                           # the hierarchy converges
    # pack: two pools and an index instead of one zip member per array
    keys = sorted(out)
    pools, index = {0: [], 1: []}, []
    fill = [0, 0]
    for k in keys:
        a = np.asarray(out[k])
        pool = 0 if a.dtype == np.float64 else 1
        assert pool == 0 or a.dtype.kind in "iub", (k, a.dtype)
        a = np.atleast_1d(a).astype(np.float64 if pool == 0 else np.int32).reshape(-1)
        index.append((pool, fill[pool], a.size))
        pools[pool].append(a)
        fill[pool] += a.size
    np.savez_compressed(OUT, f64=np.concatenate(pools[0]), i32=np.concatenate(pools[1]), keys=np.array(keys), index=np.array(index, dtype=np.int64),
                        ops=np.array([(name, str(A.blocksize[0])) for name, A in sorted(ops.items())]),
                        strength=np.array(str_table), air=np.array([stats[k]["row"] for k in sorted(stats)]), onept=np.array(onept_table))
    size = OUT.stat().st_size
    assert size <= LIMIT, (size, LIMIT)
    print(f"{OUT.name}: {len(out)} arrays, {size} bytes (limit {LIMIT}); levels {list(out['e2e.sizes'])}, {len(res) - 1} cycles")
    print({k: (min(v["n"]), max(v["n"]), v["removed"]) for k, v in stats.items()})


if __name__ == "__main__":
    main()
