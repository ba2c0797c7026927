#!/usr/bin/env python3
"""Generate tests/golden/kernels_evolution.npz: inputs and the reference's own outputs for the evolution strength of connection -- every
``amg_core`` call of it, and the whole function with the ``rho`` the reference computed.

Run in the build container (needs the reference built into oracle/_ref by oracle/build_ref.py):
    python tests/golden/make_golden_evolution.py

Data only.  Keys (CSR / CSC triples are ``<prefix>.indptr / .indices / .data``; ``<family>.names`` lists the cases of a family):

  imm.<case>.A (CSR) / .B (CSC) / .S (the pattern, with the reference's product as data)
      grid9x7    a five-point Atilde, the pattern of A as S
      rand97     seeded, non-symmetric: row lengths 0 to 40, an empty row, an empty column, entries of S outside the pattern of A @ B
      arrow130   a dense first row and a dense first column: a row of S longer than two waves, a column of B as long as the matrix
  hlp.<case>.<proj>.S (Atilde as the helper receives it) / .x / .y / .b / .NullDim / .tol / .out      proj in l2, D_A
      nd2        10 x 9 anisotropic diffusion, candidates [1, x]
      nd3        2-D linear elasticity on a 6 x 6 grid (BSR) with its three rigid-body modes
      nd6        3-D linear elasticity (P1 tets, tools/problems.py) on 4 x 4 x 4 vertices, one face clamped (144 rows), with its six rigid-body modes
      craft      7 x 5 five-point operator, candidates [1, x, y] edited: corner rows of length 3 (the all-strong shortcut), all candidates
                 zero at one node (a singular LHS in its row, zhat exactly 0 in its neighbours' rows: weak by ratio), one candidate equal
                 to z on one row's neighbourhood (near-perfect: 1e-4)
  flt.S / flt.eps / flt.rel.<k> / flt.abs.<k>      apply_distance_filter / apply_absolute_distance_filter for eps[k] in (2.0, 4.0): a row
      with only its diagonal, a row without a stored diagonal, entries exactly at the thresholds (powers of two), an empty row
  mb.<bs>.in / .out                                min_blocks for 2 x 2 and 3 x 3 blocks: zeros inside a block, a block of negative
      values, an all-zero block
  whole.<case>.A (CSR, or .A.bsr_data / .indices / .indptr) / .B (absent: B=None) / .B_after / .kw (epsilon, k, proj, block_flag,
      symmetrize) / .rho / .C / .A_after, or .exc (the type name) where the reference raises; .plus / .minus: the result at
      rho (1 + d) and rho (1 - d); whole.certified: the cases whose pattern is the same at all three values; whole.d;
      whole.seed: np.random.seed(seed) right before each call (the Arnoldi's starting vector)
  err.names / err.types / err.msgs                 what the reference raises for the bad inputs of evolution_cases.BAD, in their order

d = 1e-8: the band of the device-rho test.  (If the device Arnoldi's rho ever falls outside it, widen d here to ten times the observed
relative difference and regenerate; the test is not loosened.)
"""
import sys
import warnings
from pathlib import Path

import numpy as np
import scipy.sparse as sp

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

import oracle.refimport  # noqa: E402,F401
import pyamg  # noqa: E402,F401
import pyamg.strength as rstr  # noqa: E402
from pyamg import amg_core as rcore  # noqa: E402
from pyamg.gallery import linear_elasticity, poisson, stencil_grid  # noqa: E402
from pyamg.gallery.diffusion import diffusion_stencil_2d  # noqa: E402

import evolution_cases as ec  # noqa: E402
from tools.problems import elasticity3d  # noqa: E402

SEED = 20261019
D_BAND = 1e-8
OUT = HERE / "kernels_evolution.npz"
ref = rstr.evolution_strength_of_connection


def put(out, prefix, M, data=True):
    out[prefix + ".indptr"] = np.asarray(M.indptr, dtype=np.int32)
    out[prefix + ".indices"] = np.asarray(M.indices, dtype=np.int32)
    if data:
        out[prefix + ".data"] = np.asarray(M.data, dtype=np.float64)


class Recorder:
    """wraps one amg_core function of the reference's strength module: the arguments as they go in, and as they come out"""

    def __init__(self, name):
        self.name, self.calls = name, []
        self.fn = getattr(rcore, name)

    def __call__(self, *a):
        before = [np.array(x, copy=True) if isinstance(x, np.ndarray) else x for x in a]
        self.fn(*a)
        self.calls.append((before, [np.array(x, copy=True) if isinstance(x, np.ndarray) else x for x in a]))


class patched:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old_core = rstr.amg_core
        self.old_rho = rstr.approximate_spectral_radius
        ns = type("core", (), {})()
        for n in dir(rcore):
            if not n.startswith("_"):
                setattr(ns, n, getattr(rcore, n))
        for n, r in self.kw.get("record", {}).items():
            setattr(ns, n, r)
        rstr.amg_core = ns
        if "rho" in self.kw:
            rstr.approximate_spectral_radius = lambda *a, **k: self.kw["rho"]
        elif "rho_out" in self.kw:
            def rho_(*a, **k):
                r = self.old_rho(*a, **k)
                self.kw["rho_out"].append(r)
                return r
            rstr.approximate_spectral_radius = rho_
        return self

    def __exit__(self, *exc):
        rstr.amg_core = self.old_core
        rstr.approximate_spectral_radius = self.old_rho


def quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


# ------------------------------------------------------------------------------------------------ incomplete_mat_mult_csr
def imm_cases():
    cases = {}
    A = sp.csr_array(poisson((9, 7), format="csr"))
    Dinv = 1.0 / A.diagonal()
    At = sp.csr_array(sp.eye_array(63, format="csr") - 0.55 * sp.csr_array(sp.diags_array(Dinv) @ A)).T.tocsr()
    At.sort_indices()
    S = A.copy(); S.sort_indices()
    cases["grid9x7"] = (At, At.tocsc(), S)
    rng = np.random.RandomState(SEED)
    n = 97

    def rand_rows(lengths, skip_col=None):
        rows, cols = [], []
        for i, m in enumerate(lengths):
            pool = np.arange(n) if skip_col is None else np.delete(np.arange(n), skip_col)
            c = np.sort(rng.choice(pool, size=m, replace=False))
            rows += [i] * m; cols += list(c)
        M = sp.coo_array((rng.randn(len(rows)), (rows, cols)), shape=(n, n)).tocsr()
        M.sort_indices()
        return M
    la = rng.randint(1, 41, n); la[:41] = np.arange(41); la[50] = 0
    A = rand_rows(la)
    B = rand_rows(rng.randint(1, 9, n), skip_col=None).T.tocsc()       # CSC whose column lengths are the drawn ones
    Bc = sp.csc_array(B); keep = np.ones(n, bool); keep[11] = False
    Bc = sp.csc_array(Bc @ sp.diags_array(keep.astype(float))); Bc.eliminate_zeros(); Bc.sort_indices()
    ls = rng.randint(1, 41, n); ls[:41] = np.arange(41)[::-1]; ls[7] = 0
    S = rand_rows(ls)
    assert np.diff(A.indptr).min() == 0 and np.diff(A.indptr).max() == 40 and np.diff(Bc.indptr)[11] == 0 and np.diff(S.indptr)[7] == 0
    cases["rand97"] = (A, Bc, S)
    n = 130
    rows = [0] * n + list(range(1, n)) + list(range(1, n))
    cols = list(range(n)) + [0] * (n - 1) + list(range(1, n))
    A = sp.coo_array((rng.rand(len(rows)) + 0.1, (rows, cols)), shape=(n, n)).tocsr(); A.sort_indices()
    cases["arrow130"] = (A, A.tocsc(), A.copy())
    return cases


def do_imm(out):
    for name, (A, B, S) in imm_cases().items():
        A, B, S = sp.csr_array(A), sp.csc_array(B), sp.csr_array(S)
        B.sort_indices()
        n = A.shape[0]
        assert n <= 300 and A.has_sorted_indices and B.has_sorted_indices and S.has_sorted_indices
        Sx = np.full(S.nnz, -7.0)
        i32 = lambda a: np.asarray(a, dtype=np.int32)      # noqa: E731
        rcore.incomplete_mat_mult_csr(i32(A.indptr), i32(A.indices), A.data, i32(B.indptr), i32(B.indices), B.data, i32(S.indptr), i32(S.indices), Sx, n)
        put(out, f"imm.{name}.A", A); put(out, f"imm.{name}.B", B)
        out[f"imm.{name}.S.indptr"], out[f"imm.{name}.S.indices"], out[f"imm.{name}.S.data"] = i32(S.indptr), i32(S.indices), Sx
        if name == "rand97":
            full = sp.csr_array(sp.csr_array((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape) @
                                sp.csr_array(sp.csc_array((np.ones(B.nnz), B.indices, B.indptr), shape=B.shape)))
            r = np.repeat(np.arange(n), np.diff(S.indptr))
            inside = np.asarray(full[r, S.indices]).ravel() != 0
            assert (~inside).sum() >= 5 and np.all(Sx[~inside] == 0.0) and not np.any(np.signbit(Sx[~inside]))
        if name == "arrow130":
            assert S.indptr[1] - S.indptr[0] > 128 and B.indptr[1] - B.indptr[0] == n
    out["imm.names"] = np.array(["grid9x7", "rand97", "arrow130"])


# ------------------------------------------------------------------------------------------------ evolution_strength_helper
def helper_inputs():
    sten = diffusion_stencil_2d(epsilon=0.01, theta=0.0, type="FD")
    A2 = sp.csr_array(stencil_grid(sten, (10, 9), format="csr"))
    x = (np.arange(90) % 9).astype(float)
    B2 = np.ascontiguousarray(np.stack([np.ones(90), x], axis=1))
    A3, B3 = linear_elasticity((6, 6), format="bsr")
    A6, B6 = elasticity3d(4)                                 # (the reference ships no 3-D mesher: the P1 tet assembly of tools/problems.py)
    assert B3.shape[1] == 3 and B6.shape[1] == 6 and A6.shape[0] <= 300
    Ac = sp.csr_array(poisson((7, 5), format="csr"))
    ii, jj = np.divmod(np.arange(35), 5)
    Bc = np.ascontiguousarray(np.stack([np.ones(35), 1.0 + jj, 1.0 + ii], axis=1))
    return {"nd2": (A2, B2), "nd3": (sp.bsr_array(A3), np.ascontiguousarray(B3)), "nd6": (sp.bsr_array(A6), np.ascontiguousarray(B6)),
            "craft": (Ac, Bc)}


def classify(S_in, x, y, b, NullDim, tol, out_data):
    """counts of (shortcut rows, singular rows, weak by ratio, weak by angle, near-perfect) by a NumPy re-derivation with pinv"""
    n = S_in.shape[0]
    B = x.reshape(n, NullDim); DB = y.reshape(NullDim, n)
    K1 = NullDim + 1
    short = sing = ratio_c = angle_c = perfect = 0
    for i in range(n):
        a, e = S_in.indptr[i], S_in.indptr[i + 1]
        if e - a <= NullDim:
            short += 1
            assert np.all(out_data[a:e] == 1.0)
            continue
        cols, z = S_in.indices[a:e], S_in.data[a:e]
        M = np.zeros((K1, K1))
        M[:NullDim, :NullDim] = 2.0 * (DB[:, cols] @ B[cols])
        M[NullDim, :NullDim] = B[i]; M[:NullDim, NullDim] = DB[:, i]
        if np.linalg.matrix_rank(M) < K1:
            sing += 1
        rhs = np.concatenate([2.0 * (DB[:, cols] @ z), [z[cols == i][0] if np.any(cols == i) else 1.0]])
        sol = np.linalg.pinv(M) @ rhs
        zh = B[cols] @ sol[:NullDim]
        zh[np.abs(zh) < tol * np.abs(zh).max()] = 0.0
        for t in range(e - a):
            if cols[t] == i:
                continue
            r = zh[t] / z[t]
            o = out_data[a + t]
            if r * r <= 1e-8 and o == 0.0:
                ratio_c += 1
            elif zh[t] * z[t] < 0 and o == 0.0:
                angle_c += 1
            elif o == 1e-4:
                perfect += 1
    return short, sing, ratio_c, angle_c, perfect


def do_helper(out):
    totals = np.zeros(5, dtype=int)
    for name, (A, B) in helper_inputs().items():
        for proj in ("l2", "D_A"):
            if name == "craft":
                # S does not depend on B: a first pass records it, then the candidates are edited against it
                rec = Recorder("evolution_strength_helper")
                np.random.seed(SEED)
                with patched(record={"evolution_strength_helper": rec}):
                    quiet(ref, A.copy(), B.copy(), proj_type=proj)
                (sx, sp_, sj, n, *_), _ = rec.calls[0]
                S0 = sp.csr_array((sx, sj, sp_), shape=(n, n))
                B = B.copy()
                B[17, :] = 0.0                               # all candidates vanish at node 17 (interior)
                i0 = 27                                      # an interior row away from node 17
                a, e = S0.indptr[i0], S0.indptr[i0 + 1]
                assert 17 not in S0.indices[a:e] and e - a == 5
                B[S0.indices[a:e], 1] = S0.data[a:e]         # candidate 1 equals z on the neighbourhood of row 27
            rec = Recorder("evolution_strength_helper")
            np.random.seed(SEED)
            with patched(record={"evolution_strength_helper": rec}):
                quiet(ref, A.copy(), B.copy(), proj_type=proj)
            assert len(rec.calls) == 1
            (sx, sp_, sj, n, x, y, b, cols, nd, tol), (sx_out, *_) = rec.calls[0]
            assert n <= 300 and nd == B.shape[1]
            S_in = sp.csr_array((sx, sj, sp_), shape=(n, n))
            p = f"hlp.{name}.{proj}"
            put(out, p + ".S", S_in)
            out[p + ".x"], out[p + ".y"], out[p + ".b"] = x, y, b
            out[p + ".NullDim"], out[p + ".tol"], out[p + ".out"] = np.int64(nd), np.float64(tol), sx_out
            c = classify(S_in, x, y, b, int(nd), float(tol), sx_out)
            print(p, "rows", n, "short/singular/ratio/angle/perfect", c)
            totals += np.array(c)
            if name == "nd6":
                assert c[0] < n                              # rows longer than six entries: the 7 x 7 solve runs
            if name == "craft":
                assert c[0] >= 4 and c[1] >= 1 and c[2] >= 1 and c[4] >= 1, c
    assert np.all(totals > 0), totals
    out["hlp.names"] = np.array(["nd2", "nd3", "nd6", "craft"])


# ------------------------------------------------------------------------------------------------ filters and min_blocks
def do_filters(out):
    rng = np.random.RandomState(SEED + 1)
    rows = [([0], [0.3]),                                                   # only its diagonal
            ([0, 2, 3, 5], [0.5, 1.0, 2.0, 0.75]),                          # no stored diagonal; 1.0 = 2 * 0.5 and 2.0 = 4 * 0.5 exactly
            ([0, 1, 2, 4, 6], [0.25, 3.0, 9.0, 0.5, 1.0]),                  # diagonal stored; 0.5 = 2 * 0.25, 1.0 = 4 * 0.25
            ([1, 3, 5, 7], [2.0, 7.0, 4.0, 1.5]),                           # the absolute thresholds 2.0 and 4.0 exactly
            ([], [])]                                                       # an empty row
    n = 12
    for i in range(5, n):
        c = np.sort(rng.choice(n, size=rng.randint(2, 7), replace=False))
        rows.append((list(c), list(rng.rand(len(c)) * 4 + 0.1)))
    indptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int32)
    indices = np.concatenate([np.asarray(c, dtype=np.int32) for c, _ in rows])
    data = np.concatenate([np.asarray(v, dtype=np.float64) for _, v in rows])
    out["flt.S.indptr"], out["flt.S.indices"], out["flt.S.data"] = indptr, indices, data
    eps = np.array([2.0, 4.0])
    out["flt.eps"] = eps
    for k, e in enumerate(eps):
        for kind, fn in (("rel", rcore.apply_distance_filter), ("abs", rcore.apply_absolute_distance_filter)):
            x = data.copy()
            fn(n, float(e), indptr, indices, x)
            out[f"flt.{kind}.{k}"] = x
    assert out["flt.rel.0"][2] == 0.0 and out["flt.rel.0"][4] == 0.75 and out["flt.rel.1"][3] == 0.0 and out["flt.rel.1"][2] == 1.0
    assert out["flt.rel.0"][0] == 1.0 and out["flt.abs.0"][10] == 0.0 and out["flt.abs.1"][12] == 0.0 and out["flt.abs.0"][13] == 1.5


def do_min_blocks(out):
    rng = np.random.RandomState(SEED + 2)
    for bs in (2, 3):
        blocks = rng.rand(9, bs * bs) + 0.5
        blocks[1, ::2] = 0.0                                 # zeros inside a block
        blocks[2] = -blocks[2]                               # a block of negative values
        blocks[3] = 0.0                                      # an all-zero block
        blocks[4, 0] = -0.0
        T = np.zeros(9)
        rcore.min_blocks(9, bs * bs, np.ravel(blocks), T)
        assert T[3] == np.finfo(float).max and T[2] < 0 and T[1] > 0
        out[f"mb.{bs}.in"], out[f"mb.{bs}.out"] = blocks, T
    out["mb.sizes"] = np.array([2, 3])


# ------------------------------------------------------------------------------------------------ the whole function
def whole_cases():
    cases = {}
    cases["poisson12x11"] = (sp.csr_array(poisson((12, 11), format="csr")), None, {})
    sten = diffusion_stencil_2d(epsilon=0.001, theta=np.pi / 3, type="FD")
    An = sp.csr_array(stencil_grid(sten, (13, 11), format="csr"))
    for k in (1, 2, 3, 4):
        cases[f"aniso_k{k}"] = (An, None, {"k": k})
    cases["aniso_inf"] = (An, None, {"epsilon": np.inf})
    cases["aniso_nosym"] = (An, None, {"symmetrize_measure": False})
    adv = sp.csr_array(stencil_grid(np.array([[0.0, -0.1, 0.0], [-2.1, 4.3, -0.1], [0.0, -2.0, 0.0]]), (15, 10), format="csr"))
    assert abs(adv - adv.T).max() > 1 and adv.shape[0] == 150
    cases["advection"] = (adv, None, {})
    Bz = np.ones((90, 1)); Bz[::7, 0] = 0.0; Bz[1::5, 0] = 2.0
    cases["bzeros"] = (sp.csr_array(poisson((10, 9), format="csr")), Bz, {})
    Ae, Be = linear_elasticity((6, 6), format="bsr")
    cases["elas_bsr"] = (sp.bsr_array(Ae), np.ascontiguousarray(Be), {"block_flag": False})
    cases["elas_bsr_block"] = (sp.bsr_array(Ae), np.ascontiguousarray(Be), {"block_flag": True})
    return cases


def do_whole(out):
    names, certified = [], []
    for name, (A, B, kw) in whole_cases().items():
        assert A.shape[0] <= 300
        p = f"whole.{name}"
        if A.format == "bsr":
            out[p + ".A.bsr_data"], out[p + ".A.indices"], out[p + ".A.indptr"] = A.data.copy(), A.indices.astype(np.int32), A.indptr.astype(np.int32)
        else:
            put(out, p + ".A", A)
        if B is not None:
            out[p + ".B"] = B.copy()
        full = {"epsilon": 4.0, "k": 2, "proj_type": "l2", "block_flag": False, "symmetrize_measure": True}
        full.update(kw)
        out[p + ".kw"] = np.array([full["epsilon"], full["k"], {"l2": 0, "D_A": 1}[full["proj_type"]], full["block_flag"], full["symmetrize_measure"]],
                                  dtype=np.float64)
        names.append(name)
        rho_out = []
        np.random.seed(SEED + 3)
        Ain, Bin = A.copy(), (None if B is None else B.copy())
        try:
            with patched(rho_out=rho_out):
                C = quiet(ref, Ain, Bin, **kw)
        except Exception as e:      # noqa: BLE001
            out[p + ".exc"] = np.array(type(e).__name__)
            if rho_out:
                out[p + ".rho"] = np.float64(rho_out[0])
            print(p, "raises", type(e).__name__, e)
            continue
        rho = rho_out[0]
        out[p + ".rho"] = np.float64(rho)
        C = sp.csr_array(C)
        put(out, p + ".C", C)
        out[p + ".C.index_dtype"] = np.array(C.indptr.dtype.name)
        if Ain.format == "csr":
            put(out, p + ".A_after", Ain)
        if Bin is not None:
            out[p + ".B_after"] = Bin
        # the same rho again must reproduce the result (nothing else is random)
        with patched(rho=rho):
            C2 = sp.csr_array(quiet(ref, A.copy(), None if B is None else B.copy(), **kw))
        assert np.array_equal(C2.indptr, C.indptr) and np.array_equal(C2.indices, C.indices) and np.array_equal(C2.data, C.data)
        side = {}
        for tag, r in (("plus", rho * (1.0 + D_BAND)), ("minus", rho * (1.0 - D_BAND))):
            with patched(rho=type(rho)(r)):
                side[tag] = sp.csr_array(quiet(ref, A.copy(), None if B is None else B.copy(), **kw))
        if all(np.array_equal(s.indptr, C.indptr) and np.array_equal(s.indices, C.indices) for s in side.values()):
            certified.append(name)
            for tag, s in side.items():
                out[p + f".{tag}"] = np.asarray(s.data, dtype=np.float64)
        print(p, "rho", repr(rho), "nnz", C.nnz, "certified" if name in certified else "pattern moves with rho")
    assert len(certified) >= 4, certified
    out["whole.seed"] = np.int64(SEED + 3)
    out["whole.names"], out["whole.certified"], out["whole.d"] = np.array(names), np.array(certified), np.float64(D_BAND)


def do_errors(out):
    types, msgs = [], []
    for name, make in ec.BAD:
        A, B, kw = make()
        try:
            quiet(ref, A, B, **kw)
            raise AssertionError(f"the reference accepts {name}")
        except AssertionError:
            raise
        except Exception as e:      # noqa: BLE001
            types.append(type(e).__name__); msgs.append(str(e))
    out["err.names"] = np.array([n for n, _ in ec.BAD])
    out["err.types"], out["err.msgs"] = np.array(types), np.array(msgs)


def main():
    out = {}
    do_imm(out)
    do_helper(out)
    do_filters(out)
    do_min_blocks(out)
    do_whole(out)
    do_errors(out)
    np.savez_compressed(OUT, **out)
    size = OUT.stat().st_size
    assert size < (1 << 20), size
    print(f"{OUT.name}: {len(out)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
