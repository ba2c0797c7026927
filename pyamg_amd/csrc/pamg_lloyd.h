// pamg_lloyd.h -- the per-node and per-edge rules of Bellman-Ford, most_interior_nodes and the Lloyd clustering loop, shared by the
// kernels of pamg_lloyd.hip and the host replay tests/lloyd_emul.cpp (the lanes of a launch and the rounds as loops), as pamg_cljp.h is
// shared by the CLJP selection.
//
//   relaxes         one edge of amg_core::bellman_ford (graph.h:670-697): d[j] = min(d[j], fl(d[i] + A_ij))
//   tight, visit_sweep, stamp_of
//                   who wrote the final d[j] FIRST in the reference's in-place serial loop
//   is_boundary_edge, centre_moves
//                   amg_core::most_interior_nodes (graph.h:842-889)
//   row_of_entry    the row of a stored entry
//   check_weights, check_centres, check_start, check_labels
//                   what the device path takes (below), host only
//
// The reference is an in-place serial loop: sweeps 0, 1, 2, ... over the rows i = 0 .. n-1, each row over its entries (i -> j) in stored
// order, `if (d[i] + A_ij < d[j]) { d[j] = d[i] + A_ij; m[j] = m[i]; p[j] = i; }`, until a sweep changes nothing.  It looks
// order-dependent, and with unit weights almost every node is tied; but its result has a closed form that order-free rounds compute.
//
//   1. Distances.  With non-negative weights the fixed point of d[j] = min_i fl(d[i] + A_ij), d = 0 at the sources, is unique, and every
//      schedule of relaxations reaches it.  Non-negative doubles and +inf order like their bit patterns, so the minimum is a 64-bit
//      unsigned atomic min.
//   2. Stamps.  The strict `<` means that the final d[j] is written once, by the first visit of a row i that holds ITS final value over an
//      edge with d[i] + A_ij == d[j] (a tight edge; d[i] finite, j not a source).  Give j the stamp (s_j, p_j): written in sweep s_j by row
//      p_j; a source has (0, -1).  Row i holds its final value from its stamp on, so it is first visited with it in sweep
//      v(i) = s_i if p_i < i (row i comes after row p_i in the same sweep), else s_i + 1.  The loop is still running then: j is not final
//      yet, so that visit changes d[j].  Hence stamp(j) = the lexicographic minimum over tight i of (v(i), i), and p[j] = that i.  v is
//      monotone in the stamp and the tight edges form a DAG (d grows along them), so this too is a min-fixed-point with one solution that
//      every schedule reaches from "no stamp" -- an atomic min on the packed key (v << 32 | i).
//   3. Labels.  Once d[i] is final, m[i] is final (m is written only together with d), so m[j] = m[p[j]] down the predecessor chains,
//      which end at a source.  Sources and unreached nodes keep the m and p they came with.
//
// THE LIMIT.  Step 2 needs: a row i that holds a value that is not yet final cannot write j's final value.  With exact sums that holds --
// a larger d[i] gives a larger d[i] + A_ij.  Under rounding it fails: two different d[i] can round to the same d[i] + A_ij (1e-20 absorbed
// by 1.0; path sums taken in different orders on an anisotropic grid), the reference then keeps the predecessor of the EARLIER, non-final
// write, and the closed form names another.  So the device path takes exact weights only: every stored weight an integer-valued double in
// [1, 2^31] and n * max(weight) < 2^53, which makes every path sum an exactly represented integer.  Unit weights -- lloyd_aggregation's
// default measure -- always qualify.  Everything else is PAMG_E_UNSUPPORTED (NotImplementedError in Python) before anything runs.  A
// weight of at least 1 also makes "d == 0" the same as "is a source", which tight() and the stamps rely on.
//
// Rows need not be sorted and may hold a column twice (both entries give the same candidate); self loops are never tight.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#if defined(__HIPCC__)
#define PAMG_LLOYD_HD __host__ __device__ __forceinline__
#else
#define PAMG_LLOYD_HD inline
#endif

namespace pamg {
namespace lloyd {

typedef unsigned long long stamp_t;
constexpr stamp_t NO_STAMP = ~0ull;                         // not reached (yet)
constexpr stamp_t SOURCE_STAMP = 0xFFFFFFFFull;             // (s, p) = (0, -1)
constexpr int NO_NODE = 0x7FFFFFFF;
constexpr int OK = 0, BAD_ARG = -1, UNSUPPORTED = -2;       // PAMG_OK, PAMG_E_ARG, PAMG_E_UNSUPPORTED

PAMG_LLOYD_HD stamp_t bits_of(double d) { stamp_t b; memcpy(&b, &d, sizeof b); return b; }
PAMG_LLOYD_HD double dist_of(stamp_t b) { double d; memcpy(&d, &b, sizeof d); return d; }
PAMG_LLOYD_HD double infinity() { return dist_of(0x7FF0000000000000ull); }

// 1. the edge (i -> j) of weight w lowers d[j] to *cand
PAMG_LLOYD_HD bool relaxes(double di, double w, double dj, double *cand)
{
    *cand = di + w;
    return *cand < dj;
}

// 2. the edge (i -> j) can have written the final d[j]
PAMG_LLOYD_HD bool tight(double di, double w, double dj) { return di < infinity() && dj != 0.0 && di + w == dj; }

PAMG_LLOYD_HD unsigned sweep_of(stamp_t stamp) { return (unsigned)(stamp >> 32); }
PAMG_LLOYD_HD int writer_of(stamp_t stamp) { return (int)(unsigned)(stamp & 0xFFFFFFFFull); }

// the sweep in which row i is first visited with its final value
PAMG_LLOYD_HD unsigned visit_sweep(stamp_t stamp_i, int i) { return writer_of(stamp_i) < i ? sweep_of(stamp_i) : sweep_of(stamp_i) + 1u; }

// what row i, stamped, offers the heads of its tight edges
PAMG_LLOYD_HD stamp_t stamp_of(stamp_t stamp_i, int i) { return ((stamp_t)visit_sweep(stamp_i, i) << 32) | (stamp_t)(unsigned)i; }

// reached through an edge: the nodes whose m and p the loop wrote
PAMG_LLOYD_HD bool was_written(stamp_t stamp) { return stamp != NO_STAMP && stamp != SOURCE_STAMP; }

// most_interior_nodes: row i holds an entry of another cluster (the labels compared as they are, -1 included)
PAMG_LLOYD_HD bool is_boundary_edge(int mi, int mj) { return mi != mj; }

// most_interior_nodes: the ascending scan `if (d[c[a]] < d[i]) c[a] = i` over the nodes of cluster a ends at the first node that attains
// the cluster's maximum, unless the centre's own distance is not below it
PAMG_LLOYD_HD bool centre_moves(double d_centre, double d_max, int first) { return first != NO_NODE && d_centre < d_max; }

// ------------------------------------------------------------------------------------------------ host only: what the device path takes
inline bool exact_weight(double w) { return w >= 1.0 && w <= 2147483648.0 && (double)(long long)w == w; }    // (a NaN fails the comparisons)

// the stored weights of an n-node graph (the pattern was checked before).  Equal weights -- the unit measure -- need one test
inline int check_weights(int n, long long nnz, const double *Ax)
{
    if (nnz == 0) return OK;
    double wmin = Ax[0], wmax = Ax[0];
    bool nan = false;
    for (long long e = 0; e < nnz; ++e) {
        wmin = Ax[e] < wmin ? Ax[e] : wmin;
        wmax = Ax[e] > wmax ? Ax[e] : wmax;
        nan |= Ax[e] != Ax[e];
    }
    if (nan || !exact_weight(wmin) || !exact_weight(wmax)) return UNSUPPORTED;
    if (wmin != wmax)
        for (long long e = 0; e < nnz; ++e) if (!exact_weight(Ax[e])) return UNSUPPORTED;
    return (double)n * wmax < 9007199254740992.0 ? OK : UNSUPPORTED;
}

// centres in range (BAD_ARG) and unique (UNSUPPORTED)
inline int check_centres(int n, const int *c, int nc)
{
    if (nc < 0 || (nc && !c)) return BAD_ARG;
    for (int a = 0; a < nc; ++a) if (c[a] < 0 || c[a] >= n) return BAD_ARG;
    std::vector<char> seen((size_t)n, 0);
    for (int a = 0; a < nc; ++a) {
        if (seen[(size_t)c[a]]) return UNSUPPORTED;
        seen[(size_t)c[a]] = 1;
    }
    return OK;
}

// bellman_ford's start: 0 at the sources, +inf elsewhere
inline int check_start(int n, const double *d)
{
    for (int i = 0; i < n; ++i)                             // (-0.0 does not order like its bits)
        if (!((d[i] == 0.0 && !std::signbit(d[i])) || d[i] == std::numeric_limits<double>::infinity())) return UNSUPPORTED;
    return OK;
}

// most_interior_nodes: labels -1 .. nc-1
inline int check_labels(int n, const int *m, int nc)
{
    for (int i = 0; i < n; ++i) if (m[i] < -1 || m[i] >= nc) return BAD_ARG;
    return OK;
}

// The kernels run over edges, so a row of any length costs what its entries cost: the row of entry e is the last i with Ap[i] <= e
// (the empty rows before it share that start and are passed over)
PAMG_LLOYD_HD int row_of_entry(int n, const int *Ap, long long e)
{
    int lo = 0, hi = n;                                     // Ap[lo] <= e < Ap[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (Ap[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace lloyd
}  // namespace pamg
