"""The register-only segmented inclusive scan of the cluster layout (seg_scan_incl, pyamg_amd/csrc/pamg_wave.h) on its own, through
pamg_segscan_probe: one wave per 64 (key, value) pairs, equal keys on consecutive lanes = one segment.

The yardstick is a numpy replay of the loop the scan restates,

    for d in 1, 2, 4, 8, 16, 32:   t[lane] = s[lane] + (s[lane - d] if lane - d >= seglo[lane] else 0.0)

numpy's float64 additions are IEEE additions, so the comparison is BIT FOR BIT on the uint64 views: the same additions in the same association,
only the way a lane obtains lane - d's value differs on the device.  A NaN that enters one addition alone keeps its payload on both sides (the
sentinel of the hand-off buffers travels this way), so NaNs are compared by their bits too.  Two results are left open by IEEE 754 and are held
to "is a NaN" only: the sum of TWO NaNs (which payload survives is the implementation's choice) and the NaN an addition makes of +inf and -inf
(its sign is the implementation's choice: x86 gives the negative one), and whatever such a NaN is added to afterwards.  The replay tracks these
lanes; every other lane is exact.

Segment layouts: one segment of 64 lanes; 64 segments of one lane; a single boundary at each of the lanes 1, 15, 16, 17, 31, 32, 33, 47, 48, 49,
63; up to eight segments of seeded random lengths followed by unused tail lanes with a key of their own, keys as c_group forms them (row tag
<< 9, 0x2000 = unused); a few hundred seeded random layouts (boundary densities from sparse to dense, keys that only differ from their
neighbour's).  Values: standard normal; magnitudes spread over 1e+-150; +0 and -0; +-inf among normals; the sentinel NaN among normals; all of
these mixed.  About 2 600 waves in one launch."""
import numpy as np
import pytest

from pyamg_amd import _capi as capi

pytestmark = pytest.mark.gpu

SENTINEL = np.uint64(0x7FF8DEADBEEF5A5A)
BOUNDARIES = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63)
ROWSHIFT, UNUSED = 9, 0x2000
LANES = np.arange(64)
VALUES = ("normal", "magnitudes", "zeros", "inf", "sentinel", "mixed")


def layouts():
    """(names, keys): keys is (n, 64) uint32"""
    names, keys = ["one segment"], [np.zeros(64, dtype=np.uint32)]
    names.append("64 segments"); keys.append((LANES % 8).astype(np.uint32) << ROWSHIFT)
    for b in BOUNDARIES:
        names.append(f"boundary at {b}"); keys.append((LANES >= b).astype(np.uint32) << ROWSHIFT)
    rng = np.random.RandomState(2100)
    for i in range(60):                                                    # c_group's groups: rows 0 .. nr-1 on consecutive lanes, then unused lanes
        nr = 1 + rng.randint(8)
        used = rng.randint(nr, 65)
        cuts = np.sort(rng.choice(np.arange(1, used), size=nr - 1, replace=False)) if nr > 1 else np.zeros(0, dtype=int)
        tag = np.searchsorted(cuts, LANES, side="right").astype(np.uint32)
        k = tag << ROWSHIFT
        k[used:] = UNUSED | (7 << ROWSHIFT) if i % 2 else UNUSED           # (a tail key that repeats the last row's tag bits or not)
        names.append(f"group {i}: {nr} rows on {used} lanes"); keys.append(k.astype(np.uint32))
    for i in range(360):
        heads = rng.rand(64) < (0.02, 0.1, 0.3, 0.6)[i % 4]
        seg = np.cumsum(heads)
        if i % 3 == 0:
            k = seg % 2                                                    # two keys in turn
        elif i % 3 == 1:
            k = (rng.randint(0, 1 << 30, size=65)[seg] << 1) | (seg % 2)   # random keys (the low bit keeps neighbours apart)
        else:
            k = seg
        names.append(f"random {i}"); keys.append(k.astype(np.uint32))
    return names, np.array(keys, dtype=np.uint32)


def values(kind, n, rng):
    v = rng.standard_normal((n, 64))
    if kind == "magnitudes":
        v = v * 10.0 ** rng.uniform(-150, 150, size=(n, 64))
    elif kind == "zeros":
        v = np.where(rng.rand(n, 64) < 0.5, 0.0, -0.0)
        v[::3] = np.where(rng.rand(*v[::3].shape) < 0.2, rng.standard_normal(v[::3].shape), v[::3])
    elif kind in ("inf", "sentinel", "mixed"):
        r = rng.rand(n, 64)
        dens = np.array((0.01, 0.05, 0.3))[np.arange(n) % 3][:, None]
        if kind in ("inf", "mixed"):
            v = np.where(r < dens, np.where(rng.rand(n, 64) < 0.5, np.inf, -np.inf), v)
        if kind in ("sentinel", "mixed"):
            vb = v.view(np.uint64).copy()
            vb[(r > 1.0 - dens)] = SENTINEL
            v = vb.view(np.float64)
        if kind == "mixed":
            v = np.where(rng.rand(n, 64) < 0.1, np.where(rng.rand(n, 64) < 0.5, 0.0, -0.0), v)
            v = np.where(rng.rand(n, 64) < 0.1, v * 1e150, v)
    return np.ascontiguousarray(v, dtype=np.float64)


def replay(keys, vals):
    """(sums, open): the loop above on every row of (n, 64) arrays; open = lanes whose bits IEEE 754 leaves to the implementation"""
    n = keys.shape[0]
    heads = np.ones((n, 64), dtype=bool)
    heads[:, 1:] = keys[:, 1:] != keys[:, :-1]
    seglo = np.maximum.accumulate(np.where(heads, LANES[None, :], 0), axis=1)
    s, opn = vals.copy(), np.zeros((n, 64), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in (1, 2, 4, 8, 16, 32):
            take = (LANES[None, :] - d) >= seglo
            o, oo = np.zeros_like(s), np.zeros_like(opn)
            o[:, d:], oo[:, d:] = s[:, :-d], opn[:, :-d]
            o, oo = np.where(take, o, 0.0), take & oo
            t = s + o
            made = np.isnan(t) & ~np.isnan(s) & ~np.isnan(o)               # +inf + -inf
            both = np.isnan(s) & np.isnan(o)
            opn = made | both | ((opn | oo) & np.isnan(t))
            s = t
    return s, opn


@pytest.fixture(scope="module")
def scanned():
    names, keys = layouts()
    n = keys.shape[0]
    rng = np.random.RandomState(2101)
    vals = {k: values(k, n, rng) for k in VALUES}
    allk, allv = np.concatenate([keys] * len(VALUES)), np.concatenate([vals[k] for k in VALUES])
    got = capi.segscan_probe(allk, allv)
    assert got.shape == allv.shape
    return names, keys, vals, {k: got[i * n:(i + 1) * n] for i, k in enumerate(VALUES)}


@pytest.mark.parametrize("kind", VALUES)
def test_scan_is_the_loop_bit_for_bit(scanned, kind):
    names, keys, vals, got = scanned
    ref, opn = replay(keys, vals[kind])
    g = got[kind]
    gb, rb = g.view(np.uint64), ref.view(np.uint64)
    bad = (gb != rb) & ~opn
    nan_bad = opn & ~np.isnan(g)
    print(f"\n[segscan] {kind}: {keys.shape[0]} waves, {int(opn.sum())} lanes held to 'is a NaN' only, {int(np.isnan(ref).sum())} NaN lanes, "
          f"{int(np.isinf(ref).sum())} infinite, {int(bad.sum())} differ, {int(nan_bad.sum())} not a NaN where one is due")
    if bad.any():
        w, l = np.argwhere(bad)[0]
        raise AssertionError(f"{kind}: layout '{names[w]}' lane {l}: device {gb[w, l]:#018x} replay {rb[w, l]:#018x}; {int(bad.sum())} lanes differ in "
                             f"{len(set(np.argwhere(bad)[:, 0]))} waves")
    assert not nan_bad.any(), (kind, names[np.argwhere(nan_bad)[0][0]])
    if kind in ("normal", "magnitudes", "zeros"):
        assert not opn.any() and not np.isnan(ref).any()
    if kind in ("sentinel", "mixed"):
        assert int(((rb == SENTINEL) & ~opn).sum()) > 1000                 # the sentinel's payload does travel through single-NaN additions


def test_layouts_cover_what_the_docstring_names():
    names, keys = layouts()
    heads = np.ones(keys.shape, dtype=bool)
    heads[:, 1:] = keys[:, 1:] != keys[:, :-1]
    nseg = heads.sum(axis=1)
    assert nseg[0] == 1 and nseg[1] == 64
    for i, b in enumerate(BOUNDARIES):
        assert np.flatnonzero(heads[2 + i]).tolist() == [0, b]
    assert 2000 <= keys.shape[0] * len(VALUES) <= 5000
    assert nseg.max() == 64 and (nseg[2 + len(BOUNDARIES):] > 8).any()


def test_probe_rejects_bad_arguments():
    assert capi.lib().pamg_segscan_probe(0, None, None, None) == capi.E_ARG
    with pytest.raises(ValueError):
        capi.segscan_probe(np.zeros((2, 32), dtype=np.uint32), np.zeros((2, 32)))
