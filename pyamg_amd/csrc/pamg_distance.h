// pamg_distance.h -- the per-row / per-entry arithmetic of the relaxation-vector strength measures (algebraic distance, affinity) and of
// the vertex-distance measure, shared by the kernels of pamg_distance.hip and the host replay tests/distance_emul.cpp (lanes and groups
// as loops), as pamg_evolution.h is shared by the evolution measure.
//
//   relax_value        one (row, column) pair of one weighted-Jacobi sweep with b = 0 (relaxation.h:310-346) on a block of R vectors kept
//                      as one record of R doubles per node: the off-diagonal sum in stored order, the LAST stored diagonal, and the
//                      value carried over where the row has no non-zero diagonal
//   np_sum             NumPy's sum along a contiguous row of R <= 32 elements: left to right below eight elements, eight accumulators
//                      over whole groups of eight, their pairwise combination, then the remainder left to right
//   measure_entry      the distance of one stored entry from the records of its two nodes (strength.py:945-948, :1008-1014), each
//                      rounding where NumPy's elementwise steps put it
//   row_min / tail     the reference's eliminate_zeros + apply_distance_filter (strength.py:1050-1060) on the pattern of A: zeros take
//                      no part in the minimum; std::min semantics (a NaN never replaces the running value)
//   vertex_entry       one stored entry of distance_strength_of_connection (strength.py:83-87)
//
// Every sum runs in the reference's order, so with -ffp-contract=off the results are the reference's bit for bit.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PAMG_DST_HD __host__ __device__ inline
#else
#define PAMG_DST_HD inline
#endif

namespace pamg {
namespace dst {

constexpr int MAX_R = 32;                                   // random vectors per block
constexpr int MAX_DIM = 8;                                  // coordinates per vertex
constexpr double DMAX = 1.7976931348623157e308;             // numeric_limits<double>::max()
// the measures (PAMG_DISTANCE_* of include/pyamg_amd.h)
constexpr int ALGEBRAIC_P1 = 0, ALGEBRAIC_P2 = 1, ALGEBRAIC_PINF = 2, AFFINITY = 3;

// std::min: the running value a is replaced only when the comparison holds, so a NaN operand never replaces it
PAMG_DST_HD double dmin(double a, double b) { return b < a ? b : a; }

// Column r of row i after one sweep; old is the interleaved block [n * R] before it
PAMG_DST_HD double relax_value(int i, int r, int R, const int *Ap, const int *Aj, const double *Ax, const double *old, double omega)
{
    double rsum = 0.0, diag = 0.0;
    const int r1 = Ap[i + 1];
    int p = Ap[i];
    // four stored entries at a time: their twelve loads are in flight together, and they are added in stored order all the same (the
    // record of the diagonal's own node is loaded and not used)
    for (; p + 4 <= r1; p += 4) {
        const int j0 = Aj[p], j1 = Aj[p + 1], j2 = Aj[p + 2], j3 = Aj[p + 3];
        const double a0 = Ax[p], a1 = Ax[p + 1], a2 = Ax[p + 2], a3 = Ax[p + 3];
        const double v0 = old[(int64_t)j0 * R + r], v1 = old[(int64_t)j1 * R + r], v2 = old[(int64_t)j2 * R + r], v3 = old[(int64_t)j3 * R + r];
        if (j0 == i) diag = a0; else rsum += a0 * v0;
        if (j1 == i) diag = a1; else rsum += a1 * v1;
        if (j2 == i) diag = a2; else rsum += a2 * v2;
        if (j3 == i) diag = a3; else rsum += a3 * v3;
    }
    for (; p < r1; ++p) {
        const int j = Aj[p];
        if (j == i) diag = Ax[p];
        else rsum += Ax[p] * old[(int64_t)j * R + r];
    }
    const double xi = old[(int64_t)i * R + r];
    if (diag != 0.0) return (1.0 - omega) * xi + omega * ((0.0 - rsum) / diag);
    return xi;
}

template <typename F>
PAMG_DST_HD double np_sum(int R, F f)
{
    if (R < 8) {
        double s = f(0);
        for (int r = 1; r < R; ++r) s += f(r);
        return s;
    }
    double a0 = f(0), a1 = f(1), a2 = f(2), a3 = f(3), a4 = f(4), a5 = f(5), a6 = f(6), a7 = f(7);
    int i = 8;
    for (; i + 8 <= R; i += 8) {
        a0 += f(i); a1 += f(i + 1); a2 += f(i + 2); a3 += f(i + 3);
        a4 += f(i + 4); a5 += f(i + 5); a6 += f(i + 6); a7 += f(i + 7);
    }
    double s = ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7));
    for (; i < R; ++i) s += f(i);
    return s;
}

// np.max along the row: a NaN propagates
PAMG_DST_HD double np_max_absdiff(int R, const double *xi, const double *xj)
{
    double m = std::fabs(xi[0] - xj[0]);
    for (int r = 1; r < R; ++r) {
        const double t = std::fabs(xi[r] - xj[r]);
        if (!(m != m) && (t > m || t != t)) m = t;
    }
    return m;
}

// The distance of the stored entry (i, j) with value a: 0.0 on the diagonal and for a stored zero (A.nonzero() drops those)
PAMG_DST_HD double measure_entry(int measure, int R, int i, int j, double a, const double *X)
{
    if (j == i || a == 0.0) return 0.0;
    const double *xi = X + (int64_t)i * R, *xj = X + (int64_t)j * R;
    switch (measure) {
    case ALGEBRAIC_P1:
        return np_sum(R, [&](int r) { return std::fabs(xi[r] - xj[r]); }) / (double)R;
    case ALGEBRAIC_P2:
        return std::sqrt(np_sum(R, [&](int r) { const double t = std::fabs(xi[r] - xj[r]); return t * t; }) / (double)R);
    case ALGEBRAIC_PINF:
        return np_max_absdiff(R, xi, xj);
    default: {
        const double ij = np_sum(R, [&](int r) { return xi[r] * xj[r]; });
        const double ii = np_sum(R, [&](int r) { return xi[r] * xi[r]; });
        const double jj = np_sum(R, [&](int r) { return xj[r] * xj[r]; });
        return 1.0 - (ij * ij) / (ii * jj);
    }
    }
}

// what one lane contributes to the minimum of its row: the entries p, p + stride, ... that are non-zero and off the diagonal
PAMG_DST_HD double row_min(int i, int p0, int r1, int stride, const int *Aj, const double *Dx)
{
    double mn = DMAX;
    for (int p = p0; p < r1; p += stride) {
        const double v = Dx[p];
        if (Aj[p] != i && v != 0.0) mn = dmin(mn, v);
    }
    return mn;
}

// apply_distance_filter on what eliminate_zeros left: an entry at or above the threshold becomes 0.0 (a zero stays a zero)
PAMG_DST_HD double tail(double v, double threshold) { return v >= threshold ? 0.0 : v; }

// V row-major [n * dim]: sqrt(((dx dx) + dy dy) + ...), coordinate after coordinate, never below 1e-6
PAMG_DST_HD double vertex_entry(int i, int j, int dim, const double *V)
{
    const double *vi = V + (int64_t)i * dim, *vj = V + (int64_t)j * dim;
    const double d0 = vi[0] - vj[0];
    double c = d0 * d0;
    for (int d = 1; d < dim; ++d) {
        const double dd = vi[d] - vj[d];
        c += dd * dd;
    }
    c = std::sqrt(c);
    return c < 1e-6 ? 1e-6 : c;
}

}  // namespace dst
}  // namespace pamg
